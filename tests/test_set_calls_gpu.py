"""Every refusal of the eight calls on a caller TGSW set (include/ieache.h sections 3f to 3j: cmux, lut_tree, lut_scatter,
lut_write, tlwe_rotate, lut_read, lut_add; section 3l: lut_write_coef), in both forms, through the C ABI as it stands: the code,
the message, which rule wins when two are broken, and that a refused call writes nothing.  The data-carrying cases stay with
each call's own file; this one is about refusals only, on the smallest shapes that reach every rule: a set of 2 samples, 3
items, depth 2, 2 steps, one table (or memory) of 4 rows, a window of width 1 at unit 1 under a projection key at (T, B)."""
import ctypes as C

import numpy as np
import pytest

import cmux_reference as CR
import pack_reference as PR

pytestmark = pytest.mark.gpu

N = 1024
ROW = 2 * N
N_SET, COUNT, DEPTH, STEPS = 2, 3, 2, 2
EINVAL = -22
T, B = 2, 2  # the projection key's decomposition, as tests/test_project_gpu.py's bit-exact cases take it

# Per call: the C arguments after (ctx, set) in order -- "@name" a pointer argument, anything else a scalar -- and per pointer
# argument (kind, rows or indices at the scalars above, optional, exclusive bound of an index, may be exactly the output).
CALLS = {
    "cmux": (["count", "@sel_of", "@d1", "@d0", "@out"],
             {"sel_of": ("idx", 3, True, N_SET, False), "d1": ("rows", 3, False, None, False), "d0": ("rows", 3, True, None, False),
              "out": ("rows", 3, False, None, False)}),
    "lut_tree": (["count", "depth", "@sel_of", "@tables", "n_tables", "@table_of", "@out"],
                 {"sel_of": ("idx", 6, True, N_SET, False), "tables": ("rows", 4, False, None, False), "table_of": ("idx", 3, True, 1, False),
                  "out": ("rows", 3, False, None, False)}),
    "lut_scatter": (["count", "depth", "@sel_of", "@values", "@mem", "@out"],
                    {"sel_of": ("idx", 6, True, N_SET, False), "values": ("rows", 3, False, None, False), "mem": ("rows", 12, True, None, True),
                     "out": ("rows", 12, False, None, False)}),
    "lut_write": (["count", "depth", "@sel_of", "@new", "@mem", "@out"],
                  {"sel_of": ("idx", 6, True, N_SET, False), "new": ("rows", 3, False, None, False), "mem": ("rows", 12, False, None, True),
                   "out": ("rows", 12, False, None, False)}),
    "tlwe_rotate": (["count", "steps", "@sel_of", "@amount_of", "@in", "@out"],
                    {"sel_of": ("idx", 6, True, N_SET, False), "amount_of": ("idx", 2, True, 2 * N, False), "in": ("rows", 3, False, None, True),
                     "out": ("rows", 3, False, None, False)}),
    "lut_read": (["count", "depth", "steps", "@sel_of", "@amount_of", "@tables", "n_tables", "@table_of", "coef", "flags", "@out"],
                 {"sel_of": ("idx", 12, True, N_SET, False), "amount_of": ("idx", 2, True, 2 * N, False), "tables": ("rows", 4, False, None, False),
                  "table_of": ("idx", 3, True, 1, False), "out": ("lwe", 3, False, None, False)}),
    "lut_add": (["count", "depth", "steps", "@sel_of", "@amount_of", "@values", "@mems", "n_mems", "@mem_of", "@out"],
                {"sel_of": ("idx", 12, True, N_SET, False), "amount_of": ("idx", 2, True, 2 * N, False), "values": ("rows", 3, False, None, False),
                 "mems": ("rows", 4, True, None, True), "mem_of": ("idx", 3, True, 1, False), "out": ("rows", 4, False, None, False)}),
    # new, mem and out may be null in a call without items only: with the 3 items of this file they are required
    "lut_write_coef": (["count", "depth", "steps", "width", "unit", "@sel_of", "@new", "@mem", "@out"],
                       {"sel_of": ("idx", 12, True, N_SET, False), "new": ("rows", 3, False, None, False), "mem": ("rows", 12, False, None, True),
                        "out": ("rows", 12, False, None, False)}),
}
SCALARS = {"count": COUNT, "depth": DEPTH, "steps": STEPS, "n_tables": 1, "n_mems": 1, "coef": 0, "flags": 0, "width": 1, "unit": 1}
# (scalar, bad value, fragment of the message), in the order the rules are tested: depth, steps, the count of tables, the flags;
# the window's: width, unit against width, unit x 2^steps against N (257 x 2^2 = 1028)
RULES = [("depth", -1, "depth must lie in 0 .. 12"), ("depth", 13, "depth must lie in 0 .. 12"), ("steps", -1, "steps must lie in 0 .. 64"),
         ("steps", 65, "steps must lie in 0 .. 64"), ("n_tables", 0, "n_tables must be at least 1"), ("n_mems", 0, "n_mems must be at least 1"),
         ("flags", 2, "unknown flag"), ("width", 0, "width must be at least 1"), ("unit", 0, "unit must be at least width"),
         ("unit", 257, "unit x 2^steps must not exceed N")]
NO_KEY = "lut_write_coef: no projection key set"
_key = []


def projection_key():
    """made once per module and left unchanged: full-range words, as the bit-exact cases of tests/test_project_gpu.py take them"""
    if not _key:
        _key.append(PR.full_range(np.random.default_rng(9901), (N, T, 2, N)))
    return _key[0]


class Walk:
    """One call in one form on fixed buffers: run(**changes) makes the C call with scalars or pointers replaced."""

    def __init__(self, ia, ctx, tgsw, name, device, host, arena, lwe_words):
        self.L, self.ctx, self.tgsw, self.name, self.device = ia.lib(), ctx, tgsw, name, device
        self.order, self.args = CALLS[name]
        self.fn = getattr(self.L, "ieache_" + name + ("_device" if device else ""))
        self.host = host            # name -> numpy array (the inputs' words; out prefilled with -1)
        self.arena = arena          # device form: (tensor, name -> offset in words)
        self.lwe_words = lwe_words  # words of a row of lut_read's output in this form
        self.calls = 0

    def words(self, name):
        kind, units = self.args[name][:2]
        return units * (ROW if kind == "rows" else self.lwe_words if kind == "lwe" else 1)

    def ptr(self, name):
        """the argument as this form takes it"""
        if self.device:
            return self.arena[0].data_ptr() + 4 * self.arena[1][name]
        return self.host[name].ctypes.data_as(C.POINTER(C.c_int32))

    def run(self, ctx="own", tgsw="own", **changes):
        argv = []
        for a in self.order:
            if a.startswith("@"):
                v = changes[a[1:]] if a[1:] in changes else self.ptr(a[1:])
                argv.append(C.c_void_p(v) if self.device and v is not None else v)
            else:
                argv.append(changes.get(a, SCALARS[a]))
        self.calls += 1
        rc = self.fn(self.ctx.h if ctx == "own" else ctx, self.tgsw.h if tgsw == "own" else tgsw, *argv, None)
        return rc, self.L.ieache_last_error().decode()

    def out_words(self):
        if self.device:
            o = self.arena[1]["out"]
            return self.arena[0][o:o + self.words("out")].cpu().numpy()
        return self.host["out"].reshape(-1)

    def refused(self, fragment, **changes):
        rc, msg = self.run(**changes)
        assert rc == EINVAL and fragment in msg, (self.name, self.device, changes.keys(), rc, msg, fragment)
        assert (self.out_words() == -1).all(), (self.name, self.device, changes.keys(), "a refused call wrote")

    def accepted(self, **changes):
        rc, msg = self.run(**changes)
        assert rc == 0, (self.name, self.device, changes.keys(), rc, msg)


def host_buffers(name, rng, lwe_words):
    bufs = {}
    for arg, (kind, units, _, bound, _) in CALLS[name][1].items():
        if arg == "out":
            bufs[arg] = np.full(units * (lwe_words if kind == "lwe" else ROW), -1, dtype=np.int32)
        elif kind == "idx":
            bufs[arg] = rng.integers(0, bound, size=units).astype(np.int32)
        else:
            bufs[arg] = CR.full_range(rng, (units, 2, N))
    return bufs


def scalar_rules(name):
    return [r for r in RULES if r[0] in CALLS[name][0]]


def walk_common(w, other_set):
    """what both forms refuse the same way, in the order of the C ABI: context and set, null required argument, scalars"""
    name, args = w.name, w.args
    required = [a for a, spec in args.items() if not spec[2]]
    w.refused("null argument", ctx=None)
    w.refused("null argument", tgsw=None)
    for a in required:
        w.refused("null argument", **{a: None})
    w.refused("another context", tgsw=other_set.h)
    w.refused("another context", tgsw=other_set.h, **{required[0]: None})  # the set is judged before the arguments
    rules = scalar_rules(name)
    for scalar, bad, fragment in rules:
        w.refused(name + ": " + fragment, **{scalar: bad})
        w.refused("null argument", **{scalar: bad, required[0]: None})  # a null argument wins over the scalars
        w.refused("another context", tgsw=other_set.h, **{scalar: bad})
    # two scalar rules at once: the earlier one wins
    for i, (s1, bad1, fragment1) in enumerate(rules):
        for s2, bad2, _ in rules[i + 1:]:
            if s2 != s1:
                w.refused(name + ": " + fragment1, **{s1: bad1, s2: bad2})
    # every optional argument may be null
    for a, spec in args.items():
        if spec[2]:
            w.accepted(**{a: None})
            reset_out(w)


def reset_out(w):
    if w.device:
        o = w.arena[1]["out"]
        w.arena[0][o:o + w.words("out")] = -1
    else:
        w.host["out"][:] = -1


def walk_host(w):
    """the first bad entry of each index array, in argument order; lut_read's coef after them; the scalars before them"""
    name = w.name
    index_args = [a[1:] for a in w.order if a.startswith("@") and w.args[a[1:]][0] == "idx"]
    bad_arrays = {}
    for a in index_args:
        bound = w.args[a][3]
        for bad in (bound, -1):
            arr = w.host[a].copy()
            at = len(arr) - 1  # the entries before it are good: it is the first bad one
            arr[at] = bad
            w.refused("%s: %s[%d] = %d is outside [0, %d)" % (name, a, at, bad, bound), **{a: arr.ctypes.data_as(C.POINTER(C.c_int32))})
        two = w.host[a].copy()
        two[0], two[-1] = -1, bound
        w.refused("%s: %s[0] = -1" % (name, a), **{a: two.ctypes.data_as(C.POINTER(C.c_int32))})
        bad_arrays[a] = two
    ptrs = {a: arr.ctypes.data_as(C.POINTER(C.c_int32)) for a, arr in bad_arrays.items()}
    for i, a in enumerate(index_args):  # several arrays bad at once: the first in argument order is named
        w.refused("%s: %s[0] = -1" % (name, a), **{b: ptrs[b] for b in index_args[i:]})
    for scalar, bad, fragment in scalar_rules(name):  # the scalars are judged before the indices
        w.refused(name + ": " + fragment, **dict({scalar: bad}, **ptrs))
    if name == "lut_read":
        for bad in (N, -1):
            w.refused("lut_read: coef[0] = %d is outside [0, %d)" % (bad, N), coef=bad)
        w.refused("lut_read: %s[0] = -1" % index_args[-1], coef=N, **{index_args[-1]: ptrs[index_args[-1]]})  # coef comes last
        w.accepted(coef=N - 1)
        reset_out(w)


def walk_device(w, host):
    """a host pointer for each argument in turn; the output laid over each input in turn; the exact alias that is accepted"""
    name, args = w.name, w.args
    pointer_args = [a[1:] for a in w.order if a.startswith("@")]
    for a in pointer_args:
        w.refused("d_%s is not a device pointer" % a, **{a: host[a].ctypes.data})
    # two host pointers at once: the first in argument order is named -- but lut_add checks what an empty call touches first
    first = "out" if name == "lut_add" else pointer_args[0]
    w.refused("d_%s is not a device pointer" % first, **{pointer_args[0]: host[pointer_args[0]].ctypes.data, "out": host["out"].ctypes.data})
    for scalar, bad, fragment in scalar_rules(name):  # the scalars are judged before the pointers
        w.refused(name + ": " + fragment, **{scalar: bad, "out": host["out"].ctypes.data})
    base = w.arena[0].data_ptr()
    for a in pointer_args[:-1]:
        at = base + 4 * w.arena[1][a]
        alias = args[a][4]
        # the arena's tail holds the largest output behind every input, so even this pointer names the arena's own words only
        w.refused("overlaps", out=at + 4 if alias else at)
        if alias:
            w.refused("overlaps", out=at + 4 * ROW)  # a row further: still no exact alias
            assert "only d_out == d_%s" % a in w.run(out=at + 4)[1]
    check_inputs(w, host)
    for a in pointer_args[:-1]:
        if args[a][4]:
            # the accepted alias runs, and gives the words of the call with an output of its own
            w.accepted()
            want = w.out_words().copy()
            w.accepted(out=base + 4 * w.arena[1][a])
            o = w.arena[1][a]
            assert np.array_equal(w.arena[0][o:o + w.words("out")].cpu().numpy(), want), (name, "in place")
            w.arena[0][o:o + w.words(a)] = to_device(host[a].reshape(-1))
            reset_out(w)


def walk_empty_lut_add(w, host):
    """lut_add without items still copies or zero-fills its memories: d_values may be null, the scalars, d_mems and d_out are judged"""
    w.accepted(count=0, values=None)
    assert np.array_equal(w.out_words(), host["mems"].reshape(-1)), ("lut_add", w.device, "an empty call copies the memories")
    w.accepted(count=0, values=None, mems=None, sel_of=None, mem_of=None)
    assert (w.out_words() == 0).all(), ("lut_add", w.device, "an empty call with no memories gives zeros")
    reset_out(w)
    w.refused("null argument", count=0, out=None)
    w.refused("lut_add: n_mems must be at least 1", count=0, values=None, n_mems=0)
    if w.device:
        w.refused("d_out is not a device pointer", count=0, out=host["out"].ctypes.data)
        w.refused("d_mems is not a device pointer", count=0, mems=host["mems"].ctypes.data)
        w.refused("d_mems is not a device pointer", count=0, mems=host["mems"].ctypes.data, out=host["out"].ctypes.data)  # argument order
        w.refused("only d_out == d_mems", count=0, out=w.arena[0].data_ptr() + 4 * w.arena[1]["mems"] + 4)
        check_inputs(w, host)


def walk_no_key(w, other_set, host):
    """lut_write_coef on a context without a projection key: refused after the context, the set and the null arguments, before the
    scalars, the indices and the pointers"""
    w.refused(NO_KEY)
    w.refused("null argument", new=None)
    w.refused("another context", tgsw=other_set.h)
    for scalar, bad, _ in scalar_rules(w.name):
        w.refused(NO_KEY, **{scalar: bad})
    if w.device:
        w.refused(NO_KEY, out=host["out"].ctypes.data)
        check_inputs(w, host)
    else:
        bad = host["sel_of"].copy()
        bad[0] = -1
        w.refused(NO_KEY, sel_of=bad.ctypes.data_as(C.POINTER(C.c_int32)))


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_inputs(w, host):
    for a in w.args:
        if a != "out":
            o = w.arena[1][a]
            assert np.array_equal(w.arena[0][o:o + w.words(a)].cpu().numpy(), host[a].reshape(-1)), (w.name, a, "a refused call wrote")


def test_every_refusal_of_every_call_in_both_forms(ia, gpu_ctx):
    import torch
    kb, ctx = gpu_ctx(4, N)
    p = kb.p
    rng = np.random.default_rng(9900)
    S = CR.full_range(rng, (N_SET, 2 * p.l, 2, N))
    lwe_host, lwe_dev = p.n + 1, ia.lib().ieache_lwe_stride(ctx.h)
    other = ia.Context.from_arrays(p, kb.bk, kb.ksk)
    ctx.set_projection_key(projection_key(), t=T, basebit=B)
    try:
        with ctx.tgsw_prepare(S) as own_set, other.tgsw_prepare(S) as other_set:
            host = {name: host_buffers(name, rng, lwe_host) for name in CALLS}
            walks = [Walk(ia, ctx, own_set, name, False, host[name], None, lwe_host) for name in CALLS]
            for w in walks:  # the first accepted host call of each kind: what it stages stays
                w.accepted()
                assert not (w.out_words() == -1).all()
                reset_out(w)
            warm = ctx.get_option("staging_allocations")
            for w in walks:
                walk_common(w, other_set)
                walk_host(w)
                if w.name == "lut_add":
                    walk_empty_lut_add(w, host["lut_add"])
            for name in CALLS:
                # one arena per call: every argument at an offset of its own, and behind them room for the largest output, so
                # that an output pointer laid over any input stays inside the arena
                dev_host = dict(host[name], out=np.full(CALLS[name][1]["out"][1] * (lwe_dev if name == "lut_read" else ROW), -1, dtype=np.int32))
                offsets, end = {}, 0
                for a, arr in dev_host.items():
                    offsets[a] = end
                    end += (arr.size + 63) & ~63
                arena = torch.full((end + 13 * ROW,), -1, dtype=torch.int32, device="cuda")
                for a, arr in dev_host.items():
                    arena[offsets[a]:offsets[a] + arr.size] = to_device(arr.reshape(-1))
                torch.cuda.synchronize()
                w = Walk(ia, ctx, own_set, name, True, dev_host, (arena, offsets), lwe_dev)
                w.accepted()
                assert not (w.out_words() == -1).all()
                reset_out(w)
                walk_common(w, other_set)
                walk_device(w, dev_host)
                check_inputs(w, dev_host)
                if name == "lut_add":
                    walk_empty_lut_add(w, dev_host)
                walks.append(w)
            for w in walks[:len(CALLS)]:
                w.accepted()
            assert ctx.get_option("staging_allocations") == warm
            # the write of a window in both forms once the key is gone; the seven others do not ask for it
            ctx.set_projection_key(None)
            for w in walks:
                reset_out(w)
                if w.name == "lut_write_coef":
                    walk_no_key(w, other_set, w.host)
                else:
                    w.accepted()
            print("set calls: %d C calls walked" % sum(w.calls for w in walks))
    finally:
        ctx.set_projection_key(None)
        other.close()
