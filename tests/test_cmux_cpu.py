"""The external product, the CMux, the CMux tree and the extraction of a coefficient without a GPU: the C references
(ieache_cmux_reference, ieache_lut_tree_reference, ieache_tlwe_extract_reference) against the numpy restatement of include/ieache.h
section 3f (cmux_reference.py) word for word, pinned to the untouched oracle's blind-rotation step, at the digit extremes, by
meaning at the product parameters, every refusal that needs no device, and the plan of a call (csrc/cmux_plan.h) under
AddressSanitizer + UBSan.

That ieache_keygen_raw's output is what it was before tgsw_encrypt shared its row routine is held by the golden tests
(test_golden_cpu.py compares key material generated now with stored words); nothing here repeats it."""
import os
import subprocess

import numpy as np
import pytest

import cmux_reference as CR
import tlwe_reference as TR
from np_tfhe import _mul_by_xai, _wrap32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# toy rings over several (l, Bgbit) of the lattice, the two device sets among them, l x Bgbit = 32 and the largest Bgbit of N = 16
TOY_SETS = [(16, 3, 7), (16, 2, 10), (16, 1, 27), (16, 2, 16), (16, 32, 1), (64, 3, 7), (64, 2, 10), (64, 4, 8), (64, 6, 5), (64, 1, 16)]


def params(ia, N, l, Bgbit, n=4):
    return ia.default_params().copy(n=n, N=N, l=l, Bgbit=Bgbit)


@pytest.mark.parametrize("N,l,Bgbit", TOY_SETS)
def test_reference_is_the_definition_word_for_word_on_toy_rings(ia, N, l, Bgbit):
    """Full-range random words for samples and rows; d0 given and None; sel_of None, explicit, all the last sample."""
    from ieache_amd import tools
    p = params(ia, N, l, Bgbit)
    rng = np.random.default_rng(9000 + N + 100 * l + Bgbit)
    n, count = 3, 7
    C = CR.full_range(rng, (n, 2 * l, 2, N))
    d1, d0 = CR.full_range(rng, (count, 2, N)), CR.full_range(rng, (count, 2, N))
    assert np.array_equal(tools.cmux_reference(p, C, d1, d0), CR.cmux_rows(C, d1, d0, l, Bgbit))
    assert np.array_equal(tools.cmux_reference(p, C, d1), CR.cmux_rows(C, d1, None, l, Bgbit))
    for sel in (rng.permutation(count) % n, np.full(count, n - 1)):
        assert np.array_equal(tools.cmux_reference(p, C, d1, d0, sel_of=sel), CR.cmux_rows(C, d1, d0, l, Bgbit, sel_of=sel))
    assert tools.cmux_reference(p, C, d1[:0], d0[:0]).shape == (0, 2, N)


def test_reference_is_the_definition_at_n1024(ia):
    """A handful of rows on the ring the kernels cover, both of their (l, Bgbit)."""
    from ieache_amd import tools
    for l, Bgbit in ((3, 7), (2, 10)):
        p = params(ia, 1024, l, Bgbit)
        rng = np.random.default_rng(9100 + l)
        C = CR.full_range(rng, (2, 2 * l, 2, 1024))
        d1, d0 = CR.full_range(rng, (3, 2, 1024)), CR.full_range(rng, (3, 2, 1024))
        sel = np.array([1, 0, 1])
        assert np.array_equal(tools.cmux_reference(p, C, d1, d0, sel_of=sel), CR.cmux_rows(C, d1, d0, l, Bgbit, sel_of=sel))
        assert np.array_equal(tools.cmux_reference(p, C, d1[:1]), CR.cmux_rows(C, d1[:1], None, l, Bgbit))


@pytest.mark.parametrize("n,N,kw", [(5, 64, {}), (3, 1024, {}), (3, 1024, {"l": 2, "Bgbit": 10}), (4, 32, {"l": 4, "Bgbit": 8})])
def test_pinned_to_the_oracles_blind_rotation_step(ia, make_keys, n, N, kw):
    """With C = bk[i], d0 = acc and d1 = X^a acc the CMux IS the untouched oracle's blind_rotate_step(acc, i, a), word for word."""
    from ieache_amd import tools
    kb = make_keys(n, N, **kw)
    rng = np.random.default_rng(9200 + n + N)
    acc = CR.full_range(rng, (2, N))
    for i in (0, n - 1):
        for a in (1, N - 1, N, 2 * N - 1):
            d1 = np.stack([_mul_by_xai(acc[c], a) for c in range(2)])
            want = kb.ck.blind_rotate_step(acc, i, a)
            assert np.array_equal(tools.cmux_reference(kb.p, kb.bk, d1[None], acc[None], sel_of=[i])[0], want), (i, a)
            assert np.array_equal(CR.cmux(kb.bk[i], d1, acc, kb.p.l, kb.p.Bgbit), want), (i, a)


def extreme_rows(N, l, Bgbit):
    """d1 (with d0 = 0) whose every digit is -2^(Bgbit-1) (the word -offset) and 2^(Bgbit-1) - 1, and the sample words they meet"""
    lo, hi = CR.all_digits_word(l, Bgbit, -(1 << (Bgbit - 1))), CR.all_digits_word(l, Bgbit, (1 << (Bgbit - 1)) - 1)
    assert lo == np.array([-CR.offset(l, Bgbit)], dtype=np.int64).astype(np.uint32).view(np.int32)[0]
    assert (CR.digits(np.array([lo]), l, Bgbit) == -(1 << (Bgbit - 1))).all() and (CR.digits(np.array([hi]), l, Bgbit) == (1 << (Bgbit - 1)) - 1).all()
    d1 = np.stack([np.full((2, N), lo, dtype=np.int32), np.full((2, N), hi, dtype=np.int32)])
    samples = np.stack([np.full((2 * l, 2, N), -(1 << 31), dtype=np.int32), np.full((2 * l, 2, N), (1 << 31) - 1, dtype=np.int32)])
    return d1, samples


@pytest.mark.parametrize("N,l,Bgbit", [(16, 3, 7), (64, 2, 10), (16, 1, 27), (1024, 3, 7), (1024, 2, 10)])
def test_digit_extremes(ia, N, l, Bgbit):
    """Every digit at its most negative / most positive against samples of -2^31 / 2^31 - 1 throughout: the largest sums the
    product can meet, with d0 = None and with a full-range d0 (d1 = d0 + the extreme word)."""
    from ieache_amd import tools
    p = params(ia, N, l, Bgbit)
    d1, samples = extreme_rows(N, l, Bgbit)
    d0 = CR.full_range(np.random.default_rng(9300), (1, 2, N))
    for s in range(2):
        sel = np.full(2, s)
        assert np.array_equal(tools.cmux_reference(p, samples, d1, sel_of=sel), CR.cmux_rows(samples, d1, None, l, Bgbit, sel_of=sel))
        shifted = _wrap32(d1.astype(np.int64) + d0)
        d0s = np.repeat(d0, 2, axis=0)
        assert np.array_equal(tools.cmux_reference(p, samples, shifted, d0s, sel_of=sel), CR.cmux_rows(samples, shifted, d0s, l, Bgbit, sel_of=sel))


def torus_distance(a, b):
    d = (np.asarray(a, dtype=np.int64) - np.asarray(b, dtype=np.int64)) & 0xFFFFFFFF
    return np.minimum(d, (1 << 32) - d).astype(np.float64) / 2.0 ** 32


# one CMux at N = 1024, l = 3, Bgbit = 7, alpha = 2^-25 adds key noise of sigma = 8.6e-5 per coefficient and, for
# mu = 1, the truncation ramp of at most 1.2e-4: 2^-10 = 9.8e-4 is the ramp plus 10 sigma
CMUX_BOUND = 2.0 ** -10


@pytest.fixture(scope="module")
def product_keys(ia):
    from ieache_amd import tools
    p = ia.default_params()
    return p, tools.keygen_raw(p, (1, 2, 3), with_cloud=False)


def test_meaning_at_the_product_parameters(ia, product_keys):
    """tgsw_encrypt of 0 and of 1 select d0's and d1's message: the phase of the CMux is the chosen polynomial within the bound
    of DESIGN.md section 7, and the external product alone (d0 None) is mu x d1's message."""
    from ieache_amd import tools
    p, k = product_keys
    rng = np.random.default_rng(9400)
    C = tools.tgsw_encrypt(p, k["tlwe_key"], [0, 1], 71)
    assert C.shape == (2, 6, 2, 1024) and C.dtype == np.int32
    m = (rng.integers(0, 8, size=(2, 1024)) << 29).astype(np.uint32).view(np.int32)  # multiples of 1/8
    d = tools.tlwe_encrypt(p, k["tlwe_key"], m, 72)
    out = tools.cmux_reference(p, C, np.stack([d[1], d[1]]), np.stack([d[0], d[0]]))
    ph = tools.tlwe_phase(p, k["tlwe_key"], out)
    err = [torus_distance(ph[0], m[0]).max(), torus_distance(ph[1], m[1]).max()]
    print("cmux at the product parameters: largest phase error %.3e (mu = 0), %.3e (mu = 1); bound %.3e" % (err[0], err[1], CMUX_BOUND))
    assert max(err) < CMUX_BOUND and min(err) > 0
    ext = tools.tlwe_phase(p, k["tlwe_key"], tools.cmux_reference(p, C, np.stack([d[1], d[1]])))
    assert torus_distance(ext[0], 0).max() < CMUX_BOUND and torus_distance(ext[1], m[1]).max() < CMUX_BOUND
    # the samples are what key generation makes for BK_i: phases of the rows are mu 2^(32 - (q+1) Bgbit) on coefficient 0 of the
    # block's polynomial -- rows of block B show it in their phase directly
    rows = tools.tlwe_phase(p, k["tlwe_key"], C[1, 3:])
    want = np.zeros((3, 1024), dtype=np.int64)
    want[:, 0] = [1 << (32 - (q + 1) * 7) for q in range(3)]
    assert torus_distance(rows, want).max() < 8 * p.tlwe_alpha_min
    # reproducible under a seed, different under another, fresh without one; a larger alpha shows
    small = params(ia, 16, 3, 7)
    ks = tools.keygen_raw(small, (4, 5), with_cloud=False)
    a = tools.tgsw_encrypt(small, ks["tlwe_key"], [1, 0, 5], 9)
    assert a.shape == (3, 6, 2, 16) and np.array_equal(a, tools.tgsw_encrypt(small, ks["tlwe_key"], [1, 0, 5], 9))
    assert not np.array_equal(a, tools.tgsw_encrypt(small, ks["tlwe_key"], [1, 0, 5], 10))
    assert not np.array_equal(tools.tgsw_encrypt(small, ks["tlwe_key"], [1], 0), tools.tgsw_encrypt(small, ks["tlwe_key"], [1], 0))
    wide = tools.tlwe_phase(small, ks["tlwe_key"], tools.tgsw_encrypt(small, ks["tlwe_key"], [0], 9, alpha=2.0 ** -10)[0])
    assert 2.0 ** -14 < torus_distance(wide, 0).max() < 8 * 2.0 ** -10


def test_tree_depth_3_every_index(ia):
    """N = 64: the C reference is the numpy tree word for word on random words, and with real selectors every one of the 8
    indices picks its row; depth 0 is a copy."""
    from ieache_amd import tools
    p = params(ia, 64, 3, 7)
    k = tools.keygen_raw(p, (6, 7), with_cloud=False)
    rng = np.random.default_rng(9500)
    C = CR.full_range(rng, (4, 6, 2, 64))
    T = CR.full_range(rng, (2, 8, 2, 64))
    sel, tof = np.array([[0, 1, 2], [3, 3, 1]]), np.array([1, 0])
    assert np.array_equal(tools.lut_tree_reference(p, C, T, 3, sel_of=sel, table_of=tof), CR.lut_tree(C, T, 3, 3, 7, sel_of=sel, table_of=tof, count=2))
    assert np.array_equal(tools.lut_tree_reference(p, C, T, 3, count=2), CR.lut_tree(C, T, 3, 3, 7, count=2))
    # selectors 0 and 1 at a small noise; tables of multiples of 1/8
    bits = tools.tgsw_encrypt(p, k["tlwe_key"], [0, 1], 73, alpha=2.0 ** -30)
    m = (rng.integers(0, 8, size=(8, 64)) << 29).astype(np.uint32).view(np.int32)
    table = tools.tlwe_encrypt(p, k["tlwe_key"], m, 74, alpha=2.0 ** -30)
    for index in range(8):
        sel = [[(index >> b) & 1 for b in range(3)]]
        out = tools.lut_tree_reference(p, bits, table, 3, sel_of=sel)
        assert out.shape == (1, 2, 64)
        assert torus_distance(tools.tlwe_phase(p, k["tlwe_key"], out)[0], m[index]).max() < 2.0 ** -8, index
    # depth 0: row 0 of the item's table
    T0 = CR.full_range(rng, (3, 1, 2, 64))
    assert np.array_equal(tools.lut_tree_reference(p, C, T0, 0, table_of=[2, 0, 1, 2]), T0[[2, 0, 1, 2], 0])
    assert np.array_equal(tools.lut_tree_reference(p, C, T0, 0), T0[:1, 0])


@pytest.mark.parametrize("N", [16, 1024])
def test_tlwe_extract_reference(ia, N):
    from ieache_amd import tools
    p = params(ia, N, 3, 7)
    acc = CR.full_range(np.random.default_rng(9600 + N), (3, 2, N))
    js = [0, 1, N - 1]
    got = tools.tlwe_extract_reference(p, acc, coef_of=js)
    for r, j in enumerate(js):
        assert np.array_equal(got[r], TR.extract_coefficient(acc[r], j)), j
    assert np.array_equal(tools.tlwe_extract_reference(p, acc), TR.extract_coefficient(acc, 0))
    assert np.array_equal(tools.trivial_tlwe(acc[:, 1]), TR.with_zero_mask(acc[:, 1]))
    assert tools.trivial_tlwe(acc[0, 1]).shape == (1, 2, N)


def refused(ia, match, f, *a, **kw):
    with pytest.raises(ia.IeacheError, match=match) as e:
        f(*a, **kw)
    assert e.value.code == -22


def test_refusals_without_a_device(ia):
    from ieache_amd import tools
    p = params(ia, 16, 3, 7)
    C = np.zeros((2, 6, 2, 16), dtype=np.int32)
    d = np.zeros((3, 2, 16), dtype=np.int32)
    T = np.zeros((2, 4, 2, 16), dtype=np.int32)
    assert tools.cmux_reference(p, C, d, sel_of=[0, 1, 1]).shape == (3, 2, 16)
    refused(ia, r"sel_of\[1\] = 2", tools.cmux_reference, p, C, d, sel_of=[0, 2, 1])
    refused(ia, r"sel_of\[2\] = -1", tools.cmux_reference, p, C, d, sel_of=[0, 1, -1])
    refused(ia, "unsupported", tools.cmux_reference, p.copy(N=8), C, d)
    refused(ia, "unsupported", tools.tgsw_encrypt, p.copy(l=5), np.zeros(16, dtype=np.int32), [1], 3)
    assert tools.lut_tree_reference(p, C, T, 2, sel_of=[[1, 0]], table_of=[1]).shape == (1, 2, 16)
    refused(ia, r"sel_of\[1\] = 2", tools.lut_tree_reference, p, C, T, 2, sel_of=[[1, 2]])
    refused(ia, r"table_of\[0\] = 2", tools.lut_tree_reference, p, C, T, 2, table_of=[2])
    refused(ia, r"table_of\[0\] = -1", tools.lut_tree_reference, p, C, T, 2, table_of=[-1])
    refused(ia, "depth", tools.lut_tree_reference, p, C, T, -1)
    # what the numpy wrappers cannot express: depth 13 (refused before the absent table is read), no table, no sample
    import ctypes as C_
    from ieache_amd.evaluator import _i32, check
    L, pc, out = ia.lib(), C_.byref(p), np.zeros((1, 2, 16), dtype=np.int32)
    refused(ia, "depth", lambda: check(L.ieache_lut_tree_reference(pc, _i32(C), 2, 1, 13, None, _i32(T), 1, None, _i32(out))))
    refused(ia, "n_tables", lambda: check(L.ieache_lut_tree_reference(pc, _i32(C), 2, 1, 2, None, _i32(T), 0, None, _i32(out))))
    refused(ia, "no samples", lambda: check(L.ieache_cmux_reference(pc, _i32(C), 0, 1, None, _i32(d), None, _i32(out))))
    refused(ia, r"coef_of\[0\] = 16", tools.tlwe_extract_reference, p, d, coef_of=[16, 0, 0])
    refused(ia, r"coef_of\[1\] = -1", tools.tlwe_extract_reference, p, d, coef_of=[0, -1, 0])
    assert ia.LUT_TREE_MAX_DEPTH == 12


def test_cmux_plan_under_asan_ubsan(tmp_path):
    """tests/native/cmux_plan_test.cpp: a stand-alone program over csrc/cmux_plan.h -- pieces cover all items once, whole items,
    the cap is respected, a single item larger than the cap still runs."""
    exe = tmp_path / "cmux_plan_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "native", "cmux_plan_test.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "CMUX_PLAN_OK" in r.stdout, r.stdout[-4000:]


def test_reference_under_asan_ubsan(tmp_path):
    """tgsw_encrypt_sample, cmux_reference, lut_tree_reference and tlwe_extract_reference of csrc/tfhe_host.cpp in a stand-alone
    program: exact-size buffers, l x Bgbit = 32, the largest Bgbit, Bgbit = 1, a tree against flat calls chained by hand."""
    csrc = os.path.join(ROOT, "ie-ache_amd", "csrc")
    exe = tmp_path / "cmux_reference_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I", csrc, os.path.join(ROOT, "tests", "native", "cmux_reference_test.cpp"),
                           os.path.join(csrc, "tfhe_host.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "CMUX_REFERENCE_OK" in r.stdout, r.stdout[-4000:]
