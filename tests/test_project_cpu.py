"""The TLWE projection and the replace write of a window (include/ieache.h section 3l) without a GPU: the C references
(ieache_tlwe_project_reference, ieache_lut_write_coef_reference) against the numpy restatement (project_reference.py) word for
word, the projection key against packing_keygen on the n := N set, every refusal, the plan (csrc/project_plan.h) under
AddressSanitizer + UBSan, and both calls by meaning at N = 1024.

The 2^-8 the by-meaning tests assert is the project's own decoding condition for the levelled memory (tests/test_lut_add_cpu.py
derives it: messages are multiples of 1/64, so a phase within 1/128 of its message rounds to it, and 2^-8 leaves half of that
to whatever reads the memory afterwards).  The inputs are ones the reference keeps within it; each test prints the largest
error it sees."""
import os
import subprocess

import numpy as np
import pytest

import cmux_reference as CR
import pack_reference as PR
import project_reference as JR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECOMPOSITIONS = [(8, 2), (2, 2), (4, 4)]


def torus_distance(a, b):
    d = (np.asarray(a, dtype=np.int64) - np.asarray(b, dtype=np.int64)) & 0xFFFFFFFF
    return np.minimum(d, (1 << 32) - d).astype(np.float64) / 2.0 ** 32


def windows(N):
    """(first, width, dest): widths 1, 3 and N, the window at both ends of the sample, dest at the negacyclic wrap"""
    out = []
    for width in (1, 3, N):
        for first in sorted({0, min(5, N - width), N - width}):
            for dest in (0, 7, N - 1, 2 * N - 1):
                out.append((first, width, dest))
    return out


@pytest.mark.parametrize("t,b", DECOMPOSITIONS)
@pytest.mark.parametrize("N", [16, 64])
def test_projection_reference_is_the_definition_on_toy_rings(ia, N, t, b):
    from ieache_amd import tools
    p = ia.default_params().copy(n=5, N=N)
    rng = np.random.default_rng(11000 + N + 10 * t + b)
    pk = PR.full_range(rng, (N, t, 2, N))
    samples = CR.full_range(rng, (3, 2, N))
    for first, width, dest in windows(N):
        got = tools.tlwe_project_reference(p, pk, samples, first, width, dest, t=t, basebit=b)
        assert got.shape == (3, 2, N) and np.array_equal(got, JR.project(pk, samples, first, width, dest, t, b)), (first, width, dest)
    # the definition spelled out once: extraction by the C reference, then the C packing reference on n := N
    u = np.stack([tools.tlwe_extract_reference(p, samples, np.full(3, 2 + q, dtype=np.int32)) for q in range(3)], axis=1)
    assert np.array_equal(u, JR.window_rows(samples, 2, 3))
    assert np.array_equal(tools.tlwe_project_reference(p, pk, samples, 2, 3, 9, t=t, basebit=b),
                          tools.pack_reference(tools.projection_params(p), pk, u, m=3, spread=1, shift=9, t=t, basebit=b))
    assert tools.tlwe_project_reference(p, pk, samples[:0], 0, 1, 0, t=t, basebit=b).shape == (0, 2, N)


def test_projection_reference_at_1024(ia):
    """N = 1024 at (2, 2), the crafted keys whose words carry through every byte limb included; the windows that cross the wrap."""
    from ieache_amd import tools
    N, t, b = 1024, 2, 2
    p = ia.default_params()
    rng = np.random.default_rng(11100)
    samples = CR.full_range(rng, (2, 2, N))
    keys = dict(PR.crafted_keys(N, t, N), random=PR.full_range(rng, (N, t, 2, N)))
    for name in ("random", "varied", "constant_7fffff80"):
        for first, width, dest in ((0, 1, 0), (5, 3, 2 * N - 1), (N - 32, 32, N - 1)):
            got = tools.tlwe_project_reference(p, keys[name], samples, first, width, dest, t=t, basebit=b)
            assert np.array_equal(got, JR.project(keys[name], samples, first, width, dest, t, b, fast=True)), (name, first, width, dest)


def write_case(rng, p, n_set, count, depth, t):
    S = CR.full_range(rng, (n_set, 2 * p.l, 2, p.N))
    return S, PR.full_range(rng, (p.N, t, 2, p.N)), CR.full_range(rng, (count, 1 << depth, 2, p.N)), CR.full_range(rng, (count, 2, p.N))


@pytest.mark.parametrize("N", [16, 64])
def test_write_reference_is_the_composition_on_toy_rings(ia, N):
    """depth 0, 1, 2 x steps 0, 2 x (width, unit) (1, 1), (3, 4) x counts 1, 3; selectors implied and explicit."""
    from ieache_amd import tools
    p = ia.default_params().copy(n=5, N=N)
    t, b = 2, 2
    rng = np.random.default_rng(11200 + N)
    at = 0
    for depth in (0, 1, 2):
        for steps in (0, 2):
            for width, unit in ((1, 1), (3, 4)):
                for count in (1, 3):
                    S, pk, mem, new = write_case(rng, p, 5, count, depth, t)
                    sel = rng.integers(0, 5, size=(count, max(depth + steps, 1))).astype(np.int32) if at % 2 else None
                    at += 1
                    got = tools.lut_write_coef_reference(p, S, pk, mem, depth, steps, new, width=width, unit=unit, sel_of=sel, t=t, basebit=b)
                    want = JR.lut_write_coef(S, pk, mem, depth, steps, new, width, unit, p.l, p.Bgbit, sel_of=sel, t=t, basebit=b)
                    assert got.shape == mem.shape and np.array_equal(got, want), (depth, steps, width, unit, count)
    # depth = steps = 0: mem + new - project(mem); unit defaults to width
    S, pk, mem, new = write_case(rng, p, 2, 2, 0, t)
    flat = tools.lut_write_coef_reference(p, S, pk, mem, 0, 0, new, width=4, t=t, basebit=b)
    old = tools.tlwe_project_reference(p, pk, mem[:, 0], 0, 4, 0, t=t, basebit=b)
    assert np.array_equal(flat[:, 0], PR._wrap32(mem[:, 0].astype(np.int64) + new - old))


def test_write_reference_at_1024(ia):
    from ieache_amd import tools
    p = ia.default_params()
    t, b = 2, 2
    rng = np.random.default_rng(11300)
    S, pk, mem, new = write_case(rng, p, 3, 2, 1, t)
    sel = np.array([[2, 0, 1], [1, 1, 0]], dtype=np.int32)
    got = tools.lut_write_coef_reference(p, S, pk, mem, 1, 2, new, width=3, unit=4, sel_of=sel, t=t, basebit=b)
    assert np.array_equal(got, JR.lut_write_coef(S, pk, mem, 1, 2, new, 3, 4, p.l, p.Bgbit, sel_of=sel, t=t, basebit=b, fast=True))


def test_projection_keygen_is_packing_keygen_on_the_ring_key(ia):
    from ieache_amd import tools
    for n, N, t, b in ((5, 16, 8, 2), (7, 64, 5, 3)):
        p = ia.default_params().copy(n=n, N=N)
        k = tools.keygen_raw(p, (4, 5), with_cloud=False)
        pk = tools.projection_keygen(p, k["tlwe_key"], t=t, basebit=b, seed=17)
        q = p.copy(n=N)
        assert pk.shape == (N, t, 2, N) and np.array_equal(pk, tools.packing_keygen(q, k["tlwe_key"], k["tlwe_key"], t=t, basebit=b, seed=17))
        assert not np.array_equal(pk, tools.projection_keygen(p, k["tlwe_key"], t=t, basebit=b, seed=18))
        # row (i, j) encrypts s_i 2^(32 - (j+1) b) on coefficient 0 under the ring key
        phase = tools.tlwe_phase(p, k["tlwe_key"], pk.reshape(-1, 2, N))
        want = np.zeros_like(phase)
        idx = np.arange(N * t)
        want[:, 0] = (k["tlwe_key"][idx // t].astype(np.int64) << (32 - (idx % t + 1) * b)).astype(np.uint32).view(np.int32)
        assert torus_distance(phase, want).max() < 8 * p.tlwe_alpha_min


def refused(ia, match, f, *a, **kw):
    with pytest.raises(ia.IeacheError, match=match) as e:
        f(*a, **kw)
    assert e.value.code == -22


def test_refusals(ia):
    """Each bound at its last accepted and its first refused value, for both references."""
    from ieache_amd import tools
    p = ia.default_params().copy(n=5, N=16)
    rng = np.random.default_rng(11400)
    S, pk, mem, new = write_case(rng, p, 3, 1, 1, 8)
    proj = lambda first, width, dest, **kw: tools.tlwe_project_reference(p, pk, new, first, width, dest, **kw)
    assert proj(15, 1, 31).shape == (1, 2, 16) and proj(0, 16, 0).shape == (1, 2, 16)
    refused(ia, "first must", proj, -1, 1, 0)
    refused(ia, "first must", proj, 16, 1, 0)
    refused(ia, "width must", proj, 0, 0, 0)
    refused(ia, "exceed N", proj, 15, 2, 0)
    refused(ia, "exceed N", proj, 0, 17, 0)
    refused(ia, "dest must", proj, 0, 1, 32)
    refused(ia, "dest must", proj, 0, 1, -1)
    refused(ia, "below 32", proj, 0, 1, 0, t=16, basebit=2)
    refused(ia, "pk_basebit", proj, 0, 1, 0, t=4, basebit=5)
    refused(ia, "pk_t", proj, 0, 1, 0, t=0, basebit=2)
    refused(ia, "unsupported", tools.tlwe_project_reference, p.copy(N=8), pk, np.zeros((1, 2, 8), dtype=np.int32), 0, 1, 0)
    refused(ia, "below 32", tools.projection_keygen, p, np.zeros(16, dtype=np.int32), t=16, basebit=2)
    wr = lambda depth, steps, width, unit, key=pk, sel=None, **kw: tools.lut_write_coef_reference(
        p, S, key, mem[:, :1 << max(depth, 0)] if depth <= 1 else np.zeros((1, 1 << depth, 2, 16), dtype=np.int32), depth, steps, new, width=width,
        unit=unit, sel_of=sel, **kw)
    assert wr(1, 2, 4, 4).shape == (1, 2, 2, 16) and wr(0, 4, 1, 1).shape == (1, 1, 2, 16) and wr(0, 0, 16, 16).shape == (1, 1, 2, 16)
    refused(ia, "unit must be at least width", wr, 1, 0, 4, 3)
    refused(ia, "must not exceed N", wr, 1, 3, 4, 4)
    refused(ia, "must not exceed N", wr, 0, 5, 1, 1)
    refused(ia, "must not exceed N", wr, 0, 0, 17, 17)
    refused(ia, "width must", wr, 1, 0, 0, 1)
    refused(ia, "depth must", wr, -1, 0, 1, 1)
    refused(ia, "depth must", wr, 13, 0, 1, 1)
    refused(ia, "steps must", wr, 0, -1, 1, 1)
    refused(ia, "steps must", wr, 0, 65, 1, 1)
    refused(ia, "no projection key", wr, 1, 0, 1, 1, key=None)
    refused(ia, "below 32", wr, 1, 0, 1, 1, t=16, basebit=2)
    refused(ia, r"sel_of\[1\] = 3", wr, 1, 1, 1, 1, sel=np.array([[0, 3]], dtype=np.int32))
    refused(ia, r"sel_of\[0\] = -1", wr, 1, 1, 1, 1, sel=np.array([[-1, 0]], dtype=np.int32))


def test_project_plan_under_asan_ubsan(tmp_path):
    """tests/native/project_plan_test.cpp: a stand-alone program over csrc/project_plan.h."""
    exe = tmp_path / "project_plan_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "native", "project_plan_test.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "PROJECT_PLAN_OK" in r.stdout, r.stdout[-4000:]


_keys = {}


def reference_keys(ia):
    """N = 1024: the ring key of seed (1, 2, 3) -- the GPU suite's contexts have the same -- and the projection key (8, 2) at
    the default noise 2^-25, made once"""
    from ieache_amd import tools
    if not _keys:
        p = ia.default_params()
        k = tools.keygen_raw(p, (1, 2, 3), with_cloud=False)
        _keys["k"] = (p, k["tlwe_key"], tools.projection_keygen(p, k["tlwe_key"], seed=71))
    return _keys["k"]


def test_projection_by_meaning(ia):
    """A client-encrypted sample of multiples of 1/64 projected onto windows of width 1 and 8: the window's phases within 2^-8 of
    the source's, every other coefficient within 2^-8 of zero.  t b = 16."""
    from ieache_amd import tools
    p, tlwe_key, pk = reference_keys(ia)
    N = p.N
    assert 8 * 2 >= 16 and p.tlwe_alpha_min == 2.0 ** -25
    msg = (np.random.default_rng(11500).integers(-32, 32, size=(1, N)) << 26).astype(np.int32)
    src = tools.tlwe_encrypt(p, tlwe_key, msg, 72)
    for first, width, dest in ((5, 1, 3), (5, 8, 3), (N - 8, 8, 2 * N - 4)):
        out = tools.tlwe_project_reference(p, pk, src, first, width, dest)
        phase = tools.tlwe_phase(p, tlwe_key, out)[0]
        want = np.zeros(N, dtype=np.int64)
        for q in range(width):
            x = (dest + q) % (2 * N)
            want[x % N] = -int(msg[0, first + q]) if x >= N else int(msg[0, first + q])
        err = torus_distance(phase, PR._wrap32(want))
        inside = np.zeros(N, dtype=bool)
        inside[[(dest + q) % N for q in range(width)]] = True
        print("projection (%d, %d, %d): largest phase error %.3e on the window, %.3e elsewhere (bound 2^-8 = %.3e)"
              % (first, width, dest, err[inside].max(), err[~inside].max(), 2.0 ** -8))
        assert err.max() < 2.0 ** -8


WRITES = dict(depth=2, steps=3, width=8, unit=8, addrs=[(2, 5), (0, 7), (2, 5)])
_scenario = {}


def three_writes(p, tlwe_key, pk):
    """The scenario, made once and left unchanged: a 4-slot memory of client-encrypted multiples of 1/64, three successive writes
    of client-encrypted 8-coefficient words at encrypted (slot, word) addresses -- the third at the address of the first -- with
    the address bits of all three as ONE set of TGSW samples, selectors laid out [steps low bits][depth high bits].
    -> dict(depth, steps, width, unit, samples, sel_of [3][5], new [3][2][N], mem0 [1][4][2][N], mems: the CPU reference's memory
    after each write, want: the plaintext memory after each write)"""
    from ieache_amd import tools
    key = np.asarray(tlwe_key).tobytes()
    if key not in _scenario:
        depth, steps, width, unit, addrs = (WRITES[k] for k in ("depth", "steps", "width", "unit", "addrs"))
        N, bits = p.N, depth + steps
        rng = np.random.default_rng(11600)
        plain = rng.integers(-32, 32, size=(1 << depth, N)) << 26
        mem0 = tools.tlwe_encrypt(p, tlwe_key, plain.astype(np.int32), 81)[None]
        words = rng.integers(-32, 32, size=(len(addrs), width)) << 26
        msgs = np.zeros((len(addrs), N), dtype=np.int64)
        msgs[:, :width] = words
        new = tools.tlwe_encrypt(p, tlwe_key, msgs.astype(np.int32), 82)
        flat = [slot << steps | word for slot, word in addrs]
        samples = tools.tgsw_encrypt(p, tlwe_key, [(a >> s) & 1 for a in flat for s in range(bits)], 83)
        sel_of = np.arange(len(addrs) * bits, dtype=np.int32).reshape(len(addrs), bits)
        mems, want, mem = [], [], mem0
        for i, (slot, word) in enumerate(addrs):
            mem = tools.lut_write_coef_reference(p, samples, pk, mem, depth, steps, new[i], width=width, unit=unit, sel_of=sel_of[i:i + 1])
            plain = plain.copy()
            plain[slot, word * unit:word * unit + width] = words[i]
            mems.append(mem)
            want.append(PR._wrap32(plain))
        _scenario[key] = dict(depth=depth, steps=steps, width=width, unit=unit, samples=samples, sel_of=sel_of, new=new, mem0=mem0, mems=mems,
                              want=want, words=words)
    return _scenario[key]


def test_three_writes_by_meaning(ia):
    """After each of the three writes every written word is within 2^-8 of `new` and every other coefficient of every slot within
    2^-8 of what it held; the word written twice holds the third word."""
    from ieache_amd import tools
    p, tlwe_key, pk = reference_keys(ia)
    assert (p.N, p.l, p.Bgbit) == (1024, 3, 7)
    sc = three_writes(p, tlwe_key, pk)
    for i, (mem, want) in enumerate(zip(sc["mems"], sc["want"])):
        assert mem.shape == (1, 4, 2, p.N)
        err = torus_distance(tools.tlwe_phase(p, tlwe_key, mem[0]), want)
        slot, word = WRITES["addrs"][i]
        written = err[slot, word * 8:word * 8 + 8].max()
        print("write %d at slot %d word %d: largest phase error %.3e on the written word, %.3e over the memory (bound 2^-8 = %.3e)"
              % (i, slot, word, written, err.max(), 2.0 ** -8))
        assert err.shape == (4, p.N) and err.max() < 2.0 ** -8
    last = tools.tlwe_phase(p, tlwe_key, sc["mems"][-1][0]).astype(np.int64)
    assert np.array_equal(((last + (1 << 25)) >> 26) & 63, (sc["want"][-1].astype(np.int64) >> 26) & 63)
    assert np.array_equal((sc["want"][-1][2, 40:48].astype(np.int64) >> 26) & 63, (sc["words"][2] >> 26) & 63)
