"""Random programs of levelled calls that share one context's scratch: generator, reference interpreter, device interpreter and a
plain integer model.  Test support only (numpy and ieache_amd.tools; torch inside run_context alone).

A program is a list of steps over a STATE, a dictionary of named int32 arrays:

    mem, tab   [72][2][N]    the encrypted memory and a second table set: a call of (count, depth) takes the first rows as
                             [count][2^depth][2][N], a lookup as [2][2^depth][2][N], an automaton as finals [2][states][2][N]
    tlwe       [24][2][N]    the pool of TLWE rows, two halves: a call reads one half and writes the other (or, in place, its own)
    lwe        [96][n+1]     the pool of LWE rows under the gate key, two halves
    ext        [24][N+1]     extracted rows under the ring key (tlwe_extract writes them, keyswitch reads them), two halves
    sel, tof, mof, coef, amt selector indices into the TGSW set, table / final indices (0, 1), memory indices (0 .. 2),
                             coefficient indices, rotation amounts
    tgsw       [5][2l][2][N] the TGSW samples;  pk, pj  the packing key [n][8][2][N] and the projection key [N][8][2][N]

A step is  {"op": "option", "name", "value"}  or  {"op": "call" | "gate", "kind", "count", scalars ..., "args": {argument:
(entry, first row, rows) or None}, "out": (entry, first row, rows)}: it names the state entries it reads and the one it writes,
so later steps read what earlier ones wrote.  run_reference chains the tools.*_reference functions over such a list (gate steps
go through a callable of the caller's: the CPU oracle, or the gate call issued up front); run_context runs the device forms on
ONE guarded buffer and checks after every step that nothing but the rows the step names as its output changed (the padding
words of rows it wrote may have become zero: a key switch writes its rows whole, "the padding as zero", include/ieache.h); Model walks the
same steps on plain integers with plumbing of its own.

Shapes: N = 1024 with a key of n = 4; item counts 1, 3, 4, 5, 9 around the four rows of a CMux workgroup; depth 0 .. 3, steps
0 .. 3, width 1 .. 5, unit 2^steps <= N, pack with m <= 5, automata of at most 4 states and 5 letters.

corpus(): six programs -- ("mixed", 0), ("mixed", 1), ("memory", 2), ("way_back", 3), ("shrink", 4), ("grow", 5).  A mixed program
holds every call kind once, in an order the seed draws, each call behind an option change (after a gate step on fewer rows) or
behind a gate step on more rows, the two forms swapped between the two seeds; "memory" opens with the coef_idx layout
(lut_write_coef on 9, word_read on 3, lut_write_coef on 4); "way_back" walks an Euler circuit over the five kinds that fill the
lane's extracted rows, so each follows each; "shrink" runs its largest calls first and "grow" last.  That takes 16 to 44
steps a program instead of 12: the corpus conditions of tests/test_levelled_programs_cpu.py cannot hold in fewer.

run_reference per corpus program on one CPU core, full-range words, gate steps through the CPU oracle (seconds, programs in
corpus() order; the slowest is under 1 s, so no step was cut for time):

    l3_Bg7      0.68  0.49  0.44  0.28  0.53  0.30
    l2_Bg10     0.32  0.27  0.34  0.24  0.34  0.20
    l6_Bg5_rt   0.56  0.53  0.80  0.40  0.96  0.50
"""
import contextlib

import numpy as np

N, KEY_N, N_SEL = 1024, 4, 5
MEM_ROWS, TLWE_HALF, LWE_HALF, EXT_HALF = 72, 12, 48, 12
GUARD, GUARD_WORDS = 0x5A5A5A5A, 64
COUNTS = (1, 3, 4, 5, 9)
GATE_NAND = 3
# (key's gadget, set's gadget or None for the key's): the two fixed builds and the run-time build
SETS = [({}, None), ({"l": 2, "Bgbit": 10}, None), ({}, (6, 5))]
IDS = ["l3_Bg7", "l2_Bg10", "l6_Bg5_rt"]
FAMILIES = ("mixed", "memory", "way_back", "shrink", "grow")
KINDS = ("cmux", "lut_tree", "lut_scatter", "lut_write", "tlwe_rotate", "lut_read", "lut_add", "automaton_run", "tlwe_extract", "pack",
         "tlwe_project", "lut_write_coef", "unpack", "word_read", "keyswitch")
GATE_KINDS = ("gates", "mux")
UPDATES = ("lut_write", "lut_add", "lut_write_coef", "lut_scatter")  # the memory-updating calls: d_out == d_mem is accepted
EXT_FILLERS = ("gates", "mux", "lut_read", "unpack", "word_read")     # the steps that may fill lane 0's extracted rows
KS_CALLS = ("lut_read", "unpack", "word_read", "keyswitch")           # ... and the calls "force_generic" is switched around
FAMILY_KINDS = {"memory": ("lut_write", "lut_add", "lut_write_coef", "lut_scatter", "lut_tree", "lut_read", "word_read"),
                "way_back": ("lut_read", "unpack", "word_read", "keyswitch", "tlwe_extract", "pack", "tlwe_project")}
OPTION_VALUES = {"chunk": (1, 3, 7, 200, 65536), "cmux_piece_rows": (1, 2, 5, 8192), "ks_mfma_min": (1, 64, 1 << 40), "pack_piece_rows": (1, 4096),
                 "automaton_steps_per_launch": (0, 1, 3), "cmux_gadget_runtime": (0, 1)}
# most memory-updating steps of one program: the noise budget of the meaning test (about 10 worst-case writes
# at (3, 7)); tests/test_levelled_programs_cpu.py measures what this cap leaves
MAX_UPDATES = 6

_made = {}


def once(key, make):
    if key not in _made:
        _made[key] = make()
    return _made[key]


def full_range(rng, *shape):
    return rng.integers(-(1 << 31), 1 << 31, size=shape, dtype=np.int64).astype(np.int32)


def set_params(p, gadget):
    """the parameters the set's samples and every reference take: the key's, or with the set's own gadget"""
    from ieache_amd import tools
    return p if gadget is None else tools.with_gadget(p, *gadget)


# ---------------------------------------------------------------- generator
def corpus():
    return [(0, "mixed"), (1, "mixed"), (2, "memory"), (3, "way_back"), (4, "shrink"), (5, "grow")]


def largest_program():
    """the program whose calls grow every buffer furthest: the warm-up pass of the order tests"""
    return (4, "shrink")


def _other(name):
    return "tab" if name == "mem" else "mem"


def _draw_call(rng, kind, count, big=None, inplace=None):
    """One call step of `kind` on `count` items: scalars and operands drawn by rng.  big: True / False forces the largest / the
    smallest shape (shrink, grow); inplace: forces the form of a memory-updating call."""
    def pick(values):
        return int(values[-1] if big else values[0]) if big is not None else int(rng.choice(values))
    c = int(count)
    s = {"op": "call", "kind": kind, "count": c}
    depth, steps = pick((0, 1, 2, 3)), pick((0, 1, 2, 3))
    src = int(rng.integers(0, 2))
    M = ("mem", "tab")[int(rng.integers(0, 2))]
    explicit = bool(rng.integers(0, 4))  # selectors given three times in four, implied otherwise

    def sel(words):
        return ("sel", 0, c * words) if explicit and words else None

    def opt(entry, rows):
        return (entry, 0, rows) if rng.integers(0, 2) else None
    tl = lambda half, rows: ("tlwe", half * TLWE_HALF, rows)
    lw = lambda half, rows: ("lwe", half * LWE_HALF, rows)
    ex = lambda half, rows: ("ext", half * EXT_HALF, rows)
    if kind in UPDATES:
        s["inplace"] = bool(rng.random() < 0.75) if inplace is None else bool(inplace)
    if kind == "cmux":
        s["args"] = {"sel": sel(1), "d1": tl(src, c), "d0": opt("tab", c)}
        s["out"] = tl(1 - src, c)
    elif kind == "lut_tree":
        s.update(depth=depth)
        s["args"] = {"sel": sel(depth), "tables": (M, 0, 2 << depth), "tof": opt("tof", c)}
        s["out"] = tl(1 - src, c)
    elif kind == "lut_scatter":
        s.update(depth=depth)
        s["args"] = {"sel": sel(depth), "values": tl(src, c), "mem": (M, 0, c << depth)}  # always with a memory
        s["out"] = (M if s["inplace"] else _other(M), 0, c << depth)
    elif kind == "lut_write":
        s.update(depth=depth)
        s["args"] = {"sel": sel(depth), "new": tl(src, c), "mem": (M, 0, c << depth)}
        s["out"] = (M if s["inplace"] else _other(M), 0, c << depth)
    elif kind == "tlwe_rotate":
        s.update(steps=steps)
        s["args"] = {"sel": sel(steps), "amt": opt("amt", steps) if steps else None, "rows": tl(src, c)}
        s["out"] = tl(src if rng.integers(0, 2) else 1 - src, c)  # d_out == d_in rotates in place
    elif kind == "lut_read":
        s.update(depth=depth, steps=steps, coef=int(rng.choice((0, 1, 513, N - 1))))
        s["args"] = {"sel": sel(depth + steps), "amt": opt("amt", steps) if steps else None, "tables": (M, 0, 2 << depth), "tof": opt("tof", c)}
        s["out"] = lw(1 - src, c)
    elif kind == "lut_add":
        n_mems = pick((1, 3))
        s.update(depth=depth, steps=steps, n_mems=n_mems)
        s["args"] = {"sel": sel(depth + steps), "amt": opt("amt", steps) if steps else None, "values": tl(src, c), "mems": (M, 0, n_mems << depth),
                     "mof": ("mof", 0, c) if n_mems == 3 else None}
        s["out"] = (M if s["inplace"] else _other(M), 0, n_mems << depth)
    elif kind == "automaton_run":
        states, letters = pick((1, 2, 3, 4)), pick((0, 1, 2, 3, 5))
        n_out = int(rng.integers(1, min(states, TLWE_HALF // c) + 1))
        s.update(states=states, letters=letters, n_out=n_out,
                 next0=rng.integers(0, states, size=(letters, states)).astype(np.int32).tolist(),
                 next1=rng.integers(0, states, size=(letters, states)).astype(np.int32).tolist())
        s["args"] = {"sel": sel(letters), "finals": (M, 0, 2 * states), "fof": opt("tof", c)}
        s["out"] = tl(1 - src, c * n_out)
    elif kind == "tlwe_extract":
        s["args"] = {"rows": tl(src, c), "coef": opt("coef", c)}
        s["out"] = ex(int(rng.integers(0, 2)), c)
    elif kind == "pack":
        m = pick((1, 2, 3, 5))
        s.update(m=m, spread=int(rng.choice((1, 3, 200))), shift=int(rng.choice((0, 5, N, 2 * N - 1))))
        s["args"] = {"rows": lw(src, c * m)}
        s["out"] = tl(int(rng.integers(0, 2)), c)
    elif kind == "tlwe_project":
        width = pick((1, 2, 3, 5))
        s.update(width=width, first=int(rng.choice((0, 7, N - width))), dest=int(rng.choice((0, 3, N - 1, 2 * N - 1))))
        s["args"] = {"rows": tl(src, c)}
        s["out"] = tl(1 - src, c)
    elif kind == "lut_write_coef":
        width = pick((1, 2, 3, 5))
        s.update(depth=depth, steps=steps, width=width, unit=int(rng.choice((width, 8, N >> steps))))
        s["args"] = {"sel": sel(depth + steps), "new": tl(src, c), "mem": (M, 0, c << depth)}
        s["out"] = (M if s["inplace"] else _other(M), 0, c << depth)
    elif kind == "unpack":
        width = pick((1, 2, 3, 5))
        spread = int(rng.choice((1, 3, 200)))
        s.update(width=width, spread=spread, first=int(rng.choice((0, 7, N - 1 - (width - 1) * spread))))
        s["args"] = {"rows": tl(src, c)}
        s["out"] = lw(int(rng.integers(0, 2)), c * width)
    elif kind == "word_read":
        width = pick((1, 2, 3, 5))
        s.update(depth=depth, steps=steps, width=width, unit=int(rng.choice((width, 8, N >> steps))))
        s["args"] = {"sel": sel(depth + steps), "tables": (M, 0, 2 << depth), "tof": opt("tof", c)}
        s["out"] = lw(int(rng.integers(0, 2)), c * width)
    elif kind == "keyswitch":
        s["args"] = {"rows": ex(int(rng.integers(0, 2)), c)}
        s["out"] = lw(int(rng.integers(0, 2)), c)
    elif kind in GATE_KINDS:
        s["op"] = "gate"
        names = ("a", "b", "c")[:3 if kind == "mux" else 2]
        s["args"] = {name: ("lwe", src * LWE_HALF + i * c, c) for i, name in enumerate(names)}
        s["out"] = lw(1 - src, c)
    else:
        raise ValueError(kind)
    return s


ALL_OPTIONS = [(name, v) for name in sorted(OPTION_VALUES) for v in OPTION_VALUES[name]]


def _draw_option(rng, walk):
    """the next option change of a program: a walk through every (option, value) of the table from where the seed starts it"""
    name, value = ALL_OPTIONS[walk[0] % len(ALL_OPTIONS)]
    walk[0] += 1
    return {"op": "option", "name": name, "value": int(value)}


def _smaller(rng, c):
    return int(rng.choice([v for v in COUNTS if v < c])) if c > COUNTS[0] else None


def _larger(rng, c):
    return int(rng.choice([v for v in COUNTS if v > c])) if c < COUNTS[-1] else None


def _behind_option(rng, kind, steps, walk, **kw):
    """gate step on fewer rows, option change, the call: the call stands directly after an option change and after a smaller call"""
    c = int(rng.choice(COUNTS[1:]))
    steps.append(_draw_call(rng, GATE_KINDS[int(rng.integers(0, 2))], _smaller(rng, c)))
    steps.append(_draw_option(rng, walk))
    if kind in KS_CALLS and rng.integers(0, 2):
        steps += [{"op": "option", "name": "force_generic", "value": 1}, _draw_call(rng, kind, c, **kw), {"op": "option", "name": "force_generic", "value": 0}]
    else:
        steps.append(_draw_call(rng, kind, c, **kw))


def _behind_gate(rng, kind, steps, walk, **kw):
    """gate step on more rows, the call: the call stands directly after a gate step and after a larger call"""
    c = int(rng.choice(COUNTS[:-1]))
    steps += [_draw_call(rng, GATE_KINDS[int(rng.integers(0, 2))], _larger(rng, c)), _draw_call(rng, kind, c, **kw)]


def _euler_circuit(rng, nodes):
    """a closed walk over every ordered pair of different nodes once (Hierholzer on the complete digraph), edges in drawn order"""
    out = {a: [b for b in nodes if b != a] for a in nodes}
    for a in nodes:
        rng.shuffle(out[a])
    stack, walk = [nodes[int(rng.integers(0, len(nodes)))]], []
    while stack:
        if out[stack[-1]]:
            stack.append(out[stack[-1]].pop())
        else:
            walk.append(stack.pop())
    return walk[::-1]


def program(seed, family):
    """The steps of one program: the same seed and family give the same list."""
    rng = np.random.default_rng([15000, FAMILIES.index(family), int(seed)])
    steps = []
    walk = [8 * int(seed) - int(seed) // 2]  # seeds 0, 1, 2 start at 0, 8, 15 of the 17: together they set every value
    if family == "mixed":
        order = [int(k) for k in rng.permutation(len(KINDS))]
        for k in order:
            form = (k + int(seed)) % 2
            (_behind_option if form == 0 else _behind_gate)(rng, KINDS[k], steps, walk, inplace=(form == 0))
    elif family == "memory":
        # the coef_idx layout: toward | back | own[9], then toward | back alone, then own[4] again
        for kind, c in (("lut_write_coef", 9), ("word_read", 3), ("lut_write_coef", 4)):
            steps.append(_draw_call(rng, kind, c))
        for _ in range(7):
            steps.append(_draw_option(rng, walk))
            steps.append(_draw_call(rng, FAMILY_KINDS[family][int(rng.integers(0, len(FAMILY_KINDS[family])))], int(rng.choice(COUNTS))))
    elif family == "way_back":
        others = [k for k in FAMILY_KINDS[family] if k not in EXT_FILLERS]
        for kind in _euler_circuit(rng, list(EXT_FILLERS)):
            pick = int(rng.integers(0, 4))
            if pick == 0:
                steps.append(_draw_option(rng, walk))
            elif pick == 1:
                steps.append(_draw_call(rng, others[int(rng.integers(0, len(others)))], int(rng.choice(COUNTS))))
            steps.append(_draw_call(rng, kind, int(rng.choice(COUNTS))))
    else:
        kinds = [KINDS[int(k)] for k in rng.permutation(len(KINDS))[:8]]
        sized = [(k, 9, True) for k in kinds[:4]] + [(k, int(rng.choice((1, 3))), False) for k in kinds[4:]]
        for kind, c, big in (sized if family == "shrink" else sized[::-1]):
            if rng.integers(0, 3) == 0:
                steps.append(_draw_option(rng, walk))
            if rng.integers(0, 3) == 0:
                steps.append(_draw_call(rng, GATE_KINDS[int(rng.integers(0, 2))], c))
            steps.append(_draw_call(rng, kind, c, big=big))
    # the noise budget: no more than MAX_UPDATES memory-updating steps -- later ones become lookups of the same shape
    seen = 0
    for i, s in enumerate(steps):
        if s.get("kind") in UPDATES:
            seen += 1
            if seen > MAX_UPDATES:
                steps[i] = _draw_call(rng, "lut_tree", s["count"])
    return steps


def strip_options(steps):
    return [s for s in steps if s["op"] != "option"]


# ---------------------------------------------------------------- state
def keys_full_range(n):
    """packing key [n][8][2][N] and projection key [N][8][2][N] of full-range words, made once"""
    return once(("keys", n), lambda: (full_range(np.random.default_rng(15001), n, 8, 2, N), full_range(np.random.default_rng(15002), N, 8, 2, N)))


def initial_state(p, seed=0):
    """full-range words everywhere: the word-for-word tests need no encryption.  p: the set's parameters (set_params)."""
    rng = np.random.default_rng([15003, p.l, p.Bgbit, int(seed)])
    pk, pj = keys_full_range(p.n)
    return {"mem": full_range(rng, MEM_ROWS, 2, N), "tab": full_range(rng, MEM_ROWS, 2, N), "tlwe": full_range(rng, 2 * TLWE_HALF, 2, N),
            "lwe": full_range(rng, 2 * LWE_HALF, p.n + 1), "ext": full_range(rng, 2 * EXT_HALF, N + 1),
            "sel": rng.integers(0, N_SEL, size=64).astype(np.int32), "tof": rng.integers(0, 2, size=16).astype(np.int32),
            "mof": rng.integers(0, 3, size=16).astype(np.int32), "coef": rng.integers(0, N, size=16).astype(np.int32),
            "amt": rng.integers(0, 2 * N, size=8).astype(np.int32), "tgsw": full_range(rng, N_SEL, 2 * p.l, 2, N), "pk": pk, "pj": pj}


def _fetch(st, ref):
    return None if ref is None else st[ref[0]][ref[1]:ref[1] + ref[2]]


# ---------------------------------------------------------------- reference interpreter
def _reference_call(s, A, env):
    """the tools.*_reference of one call step on its operands A (numpy arrays or None) -> the rows it writes"""
    from ieache_amd import tools
    p, S, ksk, c, k = env["p"], env["state"]["tgsw"], env["ksk"], s["count"], s["kind"]
    d, t = s.get("depth", 0), s.get("steps", 0)
    if k == "cmux":
        return tools.cmux_reference(p, S, A["d1"], A["d0"], sel_of=A["sel"])
    if k == "lut_tree":
        return tools.lut_tree_reference(p, S, A["tables"], d, sel_of=A["sel"], table_of=A["tof"], count=c)
    if k == "lut_scatter":
        return tools.lut_scatter_reference(p, S, A["values"], d, sel_of=A["sel"], mem=A["mem"], count=c)
    if k == "lut_write":
        return tools.lut_write_reference(p, S, A["mem"], d, A["new"], sel_of=A["sel"])
    if k == "tlwe_rotate":
        return tools.tlwe_rotate_reference(p, S, A["rows"], t, sel_of=A["sel"], amounts=A["amt"])
    if k == "lut_read":
        return tools.lut_read_reference(p, S, A["tables"], d, t, sel_of=A["sel"], amounts=A["amt"], table_of=A["tof"], coef=s["coef"], ksk=ksk, count=c)
    if k == "lut_add":
        return tools.lut_add_reference(p, S, A["values"], d, t, sel_of=A["sel"], amounts=A["amt"], mems=A["mems"], mem_of=A["mof"])
    if k == "automaton_run":
        return tools.automaton_reference(p, S, _tables(s, 0), _tables(s, 1), A["finals"], n_out=s["n_out"], sel_of=A["sel"], final_of=A["fof"], count=c)
    if k == "tlwe_extract":
        return tools.tlwe_extract_reference(p, A["rows"], coef_of=A["coef"])
    if k == "pack":
        return tools.pack_reference(p, env["state"]["pk"], A["rows"], m=s["m"], spread=s["spread"], shift=s["shift"])
    if k == "tlwe_project":
        return tools.tlwe_project_reference(p, env["state"]["pj"], A["rows"], s["first"], s["width"], s["dest"])
    if k == "lut_write_coef":
        return tools.lut_write_coef_reference(p, S, env["state"]["pj"], A["mem"], d, t, A["new"], width=s["width"], unit=s["unit"], sel_of=A["sel"])
    if k == "unpack":
        return tools.unpack_reference(p, A["rows"], s["first"], s["width"], s["spread"], ksk=ksk)
    if k == "word_read":
        return tools.word_read_reference(p, S, A["tables"], d, t, width=s["width"], unit=s["unit"], sel_of=A["sel"], table_of=A["tof"], ksk=ksk, count=c)
    if k == "keyswitch":
        return env["keyswitch"](A["rows"])
    raise ValueError(k)


def _tables(s, letter):
    return np.asarray(s["next%d" % letter], dtype=np.int32).reshape(s["letters"], s["states"])


def run_reference(steps, state, p, ksk, gate, keyswitch):
    """Chains the references over `steps` from `state` (left unchanged).  p: the set's parameters; ksk: the key-switch key;
    gate(kind, a, b, c) -> rows: what a gate step gives ("gates" is NAND; c None); keyswitch(u) -> rows: the key switch of
    extracted rows (tools has no reference of it alone: the oracle's, or numpy's).
    -> (writes, final): writes[i] the array step i wrote (None for an option change) -- the state after step i is `state` with
    writes[0 .. i] laid over their "out" rows -- and the final state."""
    st = {k: v.copy() if k not in ("pk", "pj") else v for k, v in state.items()}
    env = {"p": p, "ksk": ksk, "state": st, "keyswitch": keyswitch}
    writes = []
    for s in steps:
        if s["op"] == "option":
            writes.append(None)
            continue
        A = {name: _fetch(st, ref) for name, ref in s["args"].items()}
        if s["op"] == "gate":
            out = gate(s["kind"], A["a"], A["b"], A.get("c"))
        else:
            out = _reference_call(s, A, env)
        entry, first, rows = s["out"]
        out = np.ascontiguousarray(out, dtype=np.int32).reshape((rows,) + st[entry].shape[1:])
        st[entry][first:first + rows] = out
        writes.append(out)
    return writes, st


# ---------------------------------------------------------------- options
class _Options:
    def __init__(self, ctx):
        self.ctx, self.found = ctx, {}

    def set(self, name, value):
        if name not in self.found:
            self.found[name] = self.ctx.get_option(name)
        self.ctx.set_option(name, value)


@contextlib.contextmanager
def options(ctx, pk=None, pj=None):
    """The context with the packing and projection keys of a program set; on the way out, whatever happened, every option set
    through the yielded object's set() is back at the value found and both keys are dropped."""
    o = _Options(ctx)
    try:
        if pk is not None:
            ctx.set_packing_key(pk)
        if pj is not None:
            ctx.set_projection_key(pj)
        yield o
    finally:
        for name, value in o.found.items():
            ctx.set_option(name, value)
        ctx.set_packing_key(None)
        ctx.set_projection_key(None)


# ---------------------------------------------------------------- device interpreter
class DeviceState:
    """The state in ONE int32 tensor on the card: every entry with GUARD_WORDS guard words (0x5A5A5A5A) in front of and behind it,
    LWE rows at the context's padded stride and extracted rows at its extract stride, the padding words guard words too.  A copy
    on the card (`shadow`) is what the tensor must still equal after a step outside the rows the step wrote."""

    def __init__(self, state, ctx):
        import torch
        self.torch = torch
        self.row_words, self.data_words, self.offset, self.rows = {}, {}, {}, {}
        at = GUARD_WORDS
        for name, a in state.items():
            if name in ("pk", "pj"):
                continue
            data = int(np.prod(a.shape[1:], dtype=np.int64))
            stride = ctx.lwe_stride if name == "lwe" else ctx.extract_stride if name == "ext" else data
            self.row_words[name], self.data_words[name], self.offset[name], self.rows[name] = stride, data, at, a.shape[0]
            at += (a.shape[0] * stride + GUARD_WORDS + 63) // 64 * 64
        host = np.full(at, GUARD, dtype=np.uint32).view(np.int32)
        for name in self.offset:
            self._host_view(host, name)[:, :self.data_words[name]] = state[name].reshape(self.rows[name], -1)
        self.shapes = {name: state[name].shape for name in self.offset}
        self.buf = torch.from_numpy(host).cuda()
        self.shadow = self.buf.clone()
        torch.cuda.synchronize()

    def _host_view(self, host, name):
        o, r, w = self.offset[name], self.rows[name], self.row_words[name]
        return host[o:o + r * w].reshape(r, w)

    def ptr(self, ref):
        if ref is None:
            return None
        name, first, _rows = ref
        return self.buf.data_ptr() + 4 * (self.offset[name] + first * self.row_words[name])

    def span(self, ref):
        name, first, rows = ref
        o = self.offset[name] + first * self.row_words[name]
        return o, o + rows * self.row_words[name]

    def read(self, ref):
        """the data words of rows `ref` as a host array shaped as the state's"""
        name, first, rows = ref
        lo, hi = self.span(ref)
        a = self.buf[lo:hi].view(rows, self.row_words[name])[:, :self.data_words[name]].cpu().numpy()
        return np.ascontiguousarray(a).reshape((rows,) + self.shapes[name][1:])

    def where(self, word):
        for name, o in self.offset.items():
            if o - GUARD_WORDS <= word < o:
                return "the guard in front of %s" % name
            if o <= word < o + self.rows[name] * self.row_words[name]:
                row, col = divmod(word - o, self.row_words[name])
                return "%s row %d word %d%s" % (name, row, col, " (padding)" if col >= self.data_words[name] else "")
        return "a guard word at %d" % word

    def check_step(self, out_ref, what):
        """Nothing changed but data words of the rows `out_ref`: every entry the step only read, every other entry, every guard
        and every padding word is as it was.  Then the shadow takes the step's rows."""
        torch = self.torch
        lo, hi = self.span(out_ref)
        name = out_ref[0]
        diff = self.buf != self.shadow
        outside = diff.clone()
        outside[lo:hi] = False
        if self.row_words[name] != self.data_words[name]:
            # the padding of the rows a call writes: as it was, or zero -- a key switch writes its rows whole, "the padding as zero"
            # (include/ieache.h); any other value there is a stray write like one anywhere else
            pad = self.buf[lo:hi].view(-1, self.row_words[name])[:, self.data_words[name]:]
            outside[lo:hi].view(-1, self.row_words[name])[:, self.data_words[name]:] = diff[lo:hi].view(-1, self.row_words[name])[:, self.data_words[name]:] & (pad != 0)
        if bool(outside.any().item()):
            bad = torch.nonzero(outside).flatten()
            raise AssertionError("%s changed %d words it does not own, the first at %s, the last at %s"
                                 % (what, bad.numel(), self.where(int(bad[0])), self.where(int(bad[-1]))))
        self.shadow[lo:hi] = self.buf[lo:hi]

    def download(self):
        host = self.buf.cpu().numpy()
        return {name: np.ascontiguousarray(self._host_view(host, name)[:, :self.data_words[name]]).reshape(self.shapes[name]) for name in self.offset}


def _device_call(s, P, ctx, tg):
    """the device form of one call step on its operands' addresses P"""
    c, k, d, t = s["count"], s["kind"], s.get("depth", 0), s.get("steps", 0)
    if k == "cmux":
        ctx.cmux_device(tg, c, P["sel"], P["d1"], P["d0"], P["out"])
    elif k == "lut_tree":
        ctx.lut_tree_device(tg, c, d, P["sel"], P["tables"], 2, P["tof"], P["out"])
    elif k == "lut_scatter":
        ctx.lut_scatter_device(tg, c, d, P["sel"], P["values"], P["mem"], P["out"])
    elif k == "lut_write":
        ctx.lut_write_device(tg, c, d, P["sel"], P["new"], P["mem"], P["out"])
    elif k == "tlwe_rotate":
        ctx.tlwe_rotate_device(tg, c, t, P["sel"], P["amt"], P["rows"], P["out"])
    elif k == "lut_read":
        ctx.lut_read_device(tg, c, d, t, P["sel"], P["amt"], P["tables"], 2, P["tof"], P["out"], coef=s["coef"])
    elif k == "lut_add":
        ctx.lut_add_device(tg, c, d, t, P["sel"], P["amt"], P["values"], P["mems"], s["n_mems"], P["mof"], P["out"])
    elif k == "automaton_run":
        with ctx.automaton(_tables(s, 0), _tables(s, 1), s["n_out"]) as au:
            ctx.automaton_run_device(tg, au, c, P["sel"], P["finals"], 2, P["fof"], P["out"])
    elif k == "tlwe_extract":
        ctx.tlwe_extract_device(c, P["rows"], P["coef"], P["out"])
    elif k == "pack":
        ctx.pack_device(c, s["m"], s["spread"], s["shift"], P["rows"], P["out"])
    elif k == "tlwe_project":
        ctx.tlwe_project_device(c, s["first"], s["width"], s["dest"], P["rows"], P["out"])
    elif k == "lut_write_coef":
        ctx.lut_write_coef_device(tg, c, d, t, s["width"], s["unit"], P["sel"], P["new"], P["mem"], P["out"])
    elif k == "unpack":
        ctx.unpack_device(c, s["first"], s["width"], s["spread"], P["rows"], P["out"])
    elif k == "word_read":
        ctx.word_read_device(tg, c, d, t, s["width"], s["unit"], P["sel"], P["tables"], 2, P["tof"], P["out"])
    elif k == "keyswitch":
        ctx.keyswitch_device(c, P["rows"], P["out"])
    elif k == "gates":
        ctx.gates_device(GATE_NAND, c, P["a"], P["b"], P["out"])
    elif k == "mux":
        ctx.mux_device(c, P["a"], P["b"], P["c"], P["out"])
    else:
        raise ValueError(k)


def describe(i, s):
    if s["op"] == "option":
        return "step %d (option %s = %d)" % (i, s["name"], s["value"])
    scalars = ", ".join("%s=%s" % (k, s[k]) for k in ("count", "depth", "steps", "width", "unit", "inplace") if k in s)
    return "step %d (%s: %s -> %s)" % (i, s["kind"], scalars, (s["out"],))


def run_context(steps, state, ctx, gadget=None, writes=None, log=None):
    """The device forms over `steps` from `state` on `ctx`, the state on the card throughout (DeviceState).  After every step:
    nothing but the step's own output rows changed (guards, padding, entries only read), and with `writes` (run_reference's)
    those rows equal the reference's word for word; a failure names the step.  log: a callable that takes each step's
    description before the step runs.  Options go through options(): back as found afterwards, the keys dropped.  -> the final state on the host."""
    import torch
    with options(ctx, state["pk"], state["pj"]) as opts:
        dev = DeviceState(state, ctx)
        tgsw = ("tgsw", 0, N_SEL)
        tg = ctx.tgsw_prepare_device(dev.ptr(tgsw), N_SEL) if gadget is None else ctx.tgsw_prepare_device(dev.ptr(tgsw), N_SEL, *gadget)
        try:
            for i, s in enumerate(steps):
                what = describe(i, s)
                if log is not None:
                    log(what)
                if s["op"] == "option":
                    opts.set(s["name"], s["value"])
                    continue
                P = {name: dev.ptr(ref) for name, ref in s["args"].items()}
                P["out"] = dev.ptr(s["out"])
                torch.cuda.synchronize()  # the checks of the step before run on torch's stream, the call on the context's
                _device_call(s, P, ctx, tg)
                torch.cuda.synchronize()
                dev.check_step(s["out"], what)
                if writes is not None:
                    got = dev.read(s["out"])
                    if not np.array_equal(got, writes[i]):
                        rows = np.nonzero((got != writes[i]).reshape(got.shape[0], -1).any(axis=1))[0]
                        raise AssertionError("%s differs from the reference in rows %s of %d" % (what, rows[:8].tolist(), got.shape[0]))
            return dev.download()
        finally:
            tg.close()


# ---------------------------------------------------------------- the plain integer model
MASK = (1 << 32) - 1
EIGHTH = 1 << 29


def _xpow(poly, a):
    """X^a poly in Z_{2^32}[X]/(X^N + 1), a taken mod 2N"""
    a %= 2 * N
    r = a % N
    out = np.roll(poly, r)
    out[:r] = -out[:r]
    return (-out if a >= N else out) & MASK


class Model:
    """The steps on plain integers: per TLWE row its message polynomial [N], per LWE or extracted row its message, mod 2^32; the
    selector bits in the clear.  It reads the steps' operand references itself and shares nothing with the interpreters above
    but the step list, so a wrong buffer handed to both the reference and the card still disagrees with it."""

    def __init__(self, plain, bits, state):
        self.m = {k: np.array(v, dtype=np.int64) & MASK for k, v in plain.items()}  # mem, tab, tlwe [rows][N]; lwe, ext [rows]
        self.bits = [int(b) for b in bits]
        self.idx = {k: np.asarray(state[k]).astype(np.int64) for k in ("sel", "tof", "mof", "coef", "amt")}
        self.adopted = self.gate_rows = 0

    def get(self, ref):
        if ref is None:
            return None
        return (self.idx if ref[0] in self.idx else self.m)[ref[0]][ref[1]:ref[1] + ref[2]]

    def letters(self, s, i, words):
        """the clear bits of item i's `words` selectors: given, or implied (i words + k) mod n"""
        sel = self.get(s["args"].get("sel"))
        return [self.bits[int(sel[i * words + k]) if sel is not None else (i * words + k) % N_SEL] for k in range(words)]

    @staticmethod
    def number(bits):
        return sum(b << k for k, b in enumerate(bits))

    def turned(self, s, poly, bits, default):
        amt = self.get(s["args"].get("amt"))
        for t, b in enumerate(bits):
            if b:
                poly = _xpow(poly, int(amt[t]) if amt is not None else default(t))
        return poly

    def step(self, s, decoded=None):
        """applies a call or gate step; decoded: the reference's rows of a gate step, decoded to the grid -- taken where the gate's
        argument sits on a decision boundary (phase 0 or 1/2), where either bit is right"""
        g, k, c = lambda name: self.get(s["args"].get(name)), s["kind"], s["count"]
        d, t = s.get("depth", 0), s.get("steps", 0)
        if k == "cmux":
            d1, d0 = g("d1"), g("d0")
            out = np.stack([d1[i] if self.letters(s, i, 1)[0] else (d0[i] if d0 is not None else np.zeros(N, dtype=np.int64)) for i in range(c)])
        elif k == "lut_tree":
            tables, tof = g("tables").reshape(2, 1 << d, N), g("tof")
            out = np.stack([tables[int(tof[i]) if tof is not None else 0][self.number(self.letters(s, i, d))] for i in range(c)])
        elif k in ("lut_scatter", "lut_write"):
            out = g("mem").reshape(c, 1 << d, N).copy()
            for i in range(c):
                at = self.number(self.letters(s, i, d))
                out[i, at] = (out[i, at] + g("values")[i]) & MASK if k == "lut_scatter" else g("new")[i]
        elif k == "tlwe_rotate":
            out = np.stack([self.turned(s, g("rows")[i], self.letters(s, i, t), lambda q: 2 * N - (1 << q)) for i in range(c)])
        elif k == "lut_read":
            tables, tof = g("tables").reshape(2, 1 << d, N), g("tof")
            out = []
            for i in range(c):
                bits = self.letters(s, i, d + t)
                row = tables[int(tof[i]) if tof is not None else 0][self.number(bits[t:])]
                out.append(self.turned(s, row, bits[:t], lambda q: 2 * N - (1 << q))[s["coef"]])
            out = np.array(out)
        elif k == "lut_add":
            out, mof = g("mems").reshape(s["n_mems"], 1 << d, N).copy(), g("mof")
            for i in range(c):
                bits = self.letters(s, i, d + t)
                m = int(mof[i]) if mof is not None else 0
                out[m, self.number(bits[t:])] = (out[m, self.number(bits[t:])] + self.turned(s, g("values")[i], bits[:t], lambda q: 1 << q)) & MASK
        elif k == "automaton_run":
            finals, fof = g("finals").reshape(2, s["states"], N), g("fof")
            out = []
            for i in range(c):
                word = self.letters(s, i, s["letters"])
                for q in range(s["n_out"]):
                    for at, b in enumerate(word):
                        q = s["next1" if b else "next0"][at][q]
                    out.append(finals[int(fof[i]) if fof is not None else 0][q])
            out = np.stack(out)
        elif k == "tlwe_extract":
            coef = g("coef")
            out = np.array([g("rows")[i][int(coef[i]) if coef is not None else 0] for i in range(c)])
        elif k == "pack":
            out = np.zeros((c, N), dtype=np.int64)
            for grp in range(c):
                for r in range(s["m"]):
                    for q in range(s["spread"]):
                        x = (r * s["spread"] + q + s["shift"]) % (2 * N)
                        out[grp, x % N] += (-1 if x >= N else 1) * int(g("rows")[grp * s["m"] + r])
            out &= MASK
        elif k == "tlwe_project":
            out = np.zeros((c, N), dtype=np.int64)
            for i in range(c):
                for q in range(s["width"]):
                    x = (s["dest"] + q) % (2 * N)
                    out[i, x % N] = (-1 if x >= N else 1) * int(g("rows")[i][s["first"] + q])
            out &= MASK
        elif k == "lut_write_coef":
            out = g("mem").reshape(c, 1 << d, N).copy()
            for i in range(c):
                bits = self.letters(s, i, d + t)
                hi, a = self.number(bits[t:]), self.number(bits[:t]) * s["unit"]
                window = np.zeros(N, dtype=np.int64)
                window[:s["width"]] = _xpow(out[i, hi], 2 * N - a)[:s["width"]]
                out[i, hi] = (out[i, hi] + _xpow((g("new")[i] - window) & MASK, a)) & MASK
        elif k == "unpack":
            out = np.array([g("rows")[i][s["first"] + q * s["spread"]] for i in range(c) for q in range(s["width"])])
        elif k == "word_read":
            tables, tof = g("tables").reshape(2, 1 << d, N), g("tof")
            out = []
            for i in range(c):
                bits = self.letters(s, i, d + t)
                row = _xpow(tables[int(tof[i]) if tof is not None else 0][self.number(bits[t:])], 2 * N - self.number(bits[:t]) * s["unit"])
                out += [row[q] for q in range(s["width"])]
            out = np.array(out)
        elif k == "keyswitch":
            out = g("rows").copy()
        elif k in GATE_KINDS:
            a, b = g("a"), g("b")
            if k == "gates":  # bootsNAND: the sign of 1/8 - a - b, as +-1/8
                args = [(EIGHTH - a - b) & MASK]
                out = np.where(args[0] < (1 << 31), EIGHTH, -EIGHTH) & MASK
            else:  # bootsMUX: the signs of -1/8 + a + b and of -1/8 - a + c as +-1/8 each, summed, plus 1/8
                args = [(-EIGHTH + a + b) & MASK, (-EIGHTH - a + g("c")) & MASK]
                out = (np.where(args[0] < (1 << 31), EIGHTH, -EIGHTH) + np.where(args[1] < (1 << 31), EIGHTH, -EIGHTH) + EIGHTH) & MASK
            edge = np.zeros(c, dtype=bool)
            for arg in args:
                edge |= (arg % (1 << 31)) == 0
            self.gate_rows += c
            self.adopted += int(edge.sum())
            if edge.any():
                out = np.where(edge, np.asarray(decoded, dtype=np.int64) & MASK, out)
        else:
            raise ValueError(k)
        entry, first, rows = s["out"]
        self.m[entry][first:first + rows] = (np.asarray(out, dtype=np.int64) & MASK).reshape((rows,) + self.m[entry].shape[1:])


def torus_error(phase, want):
    """distance on the torus of int32 phases from the model's words, as a fraction of the torus"""
    diff = (np.asarray(phase).astype(np.int64) - np.asarray(want).astype(np.int64)) & MASK
    return np.minimum(diff, (1 << 32) - diff) / float(1 << 32)


def lwe_phase(key, rows):
    """b - a . s mod 2^32 of rows [..][len(key) + 1] under a binary key"""
    rows = np.asarray(rows, dtype=np.int32)
    n = len(key)
    return ((rows[..., n].astype(np.int64) - rows[..., :n].astype(np.int64) @ np.asarray(key, dtype=np.int64)) & MASK)


def encrypted_state(kb, gadget, seed):
    """The state with real encryptions under kb's keys (messages on the grid of eighths; LWE rows gate bits at +-1/8; selector
    bits 0 1 1 0 1), real packing and projection keys, and the Model of it -> (state, model)."""
    from ieache_amd import tools
    p, pg = kb.p, set_params(kb.p, gadget)
    rng = np.random.default_rng([15004, pg.l, pg.Bgbit, int(seed)])
    st = initial_state(pg, seed)
    plain = {}
    for name, rows in (("mem", MEM_ROWS), ("tab", MEM_ROWS), ("tlwe", 2 * TLWE_HALF)):
        plain[name] = rng.integers(0, 8, size=(rows, N)) << 29
        st[name] = tools.tlwe_encrypt(p, kb.tlwe_key, (plain[name] & MASK).astype(np.uint32).view(np.int32), int(rng.integers(1, 1 << 30)))
    bits = rng.integers(0, 2, size=2 * LWE_HALF).astype(np.uint8)
    st["lwe"] = tools.encrypt_bits(p, kb.lwe_key, bits, int(rng.integers(1, 1 << 30)))
    plain["lwe"] = np.where(bits == 1, EIGHTH, -EIGHTH)
    coefs = rng.integers(0, N, size=2 * EXT_HALF).astype(np.int32)
    st["ext"] = tools.tlwe_extract_reference(p, st["tlwe"][:2 * EXT_HALF], coef_of=coefs)
    plain["ext"] = plain["tlwe"][np.arange(2 * EXT_HALF), coefs]
    sel_bits = [0, 1, 1, 0, 1]
    st["tgsw"] = tools.tgsw_encrypt(pg, kb.tlwe_key, sel_bits, int(rng.integers(1, 1 << 30)))
    st["pk"], st["pj"] = once(("real keys", p.l, p.Bgbit), lambda: (tools.packing_keygen(p, kb.lwe_key, kb.tlwe_key, seed=15005),
                                                                     tools.projection_keygen(p, kb.tlwe_key, seed=15006)))
    return st, Model(plain, sel_bits, st)


def decoded_error(kb, entry, rows, want):
    """largest torus distance of the decrypted rows of `entry` from the model's words `want`"""
    from ieache_amd import tools
    if entry in ("mem", "tab", "tlwe"):
        phase = tools.tlwe_phase(kb.p, kb.tlwe_key, rows)
    elif entry == "lwe":
        phase = lwe_phase(kb.lwe_key, rows)
    else:
        phase = lwe_phase(kb.tlwe_key[:N], rows)
    err = torus_error(phase.reshape(np.shape(want)), want)
    return float(err.max()) if err.size else 0.0


def to_grid(kb, rows):
    """LWE rows under the gate key decoded to the nearest eighth, as words"""
    return ((lwe_phase(kb.lwe_key, rows) + (1 << 28)) >> 29 << 29) & MASK
