"""The packing key switch without a GPU: the C++ reference (ieache_pack_reference) against the numpy restatement of the definition
(pack_reference.py) word for word, key generation, decoding at the reference's parameters, every refusal, and the plan of a
call (csrc/pack_plan.h) under AddressSanitizer + UBSan.

That ieache_keygen_raw's output is what it was before the packing key existed is held by the golden tests (test_golden_cpu.py
compares key material generated now with stored words); nothing here repeats it."""
import os
import subprocess

import numpy as np
import pytest

import pack_reference as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = [(5, 16), (37, 64), (130, 1024)]
DECOMPOSITIONS = [(8, 2), (4, 4), (5, 3), (16, 1), (31, 1)]
MS = [1, 2, 33]
GROUPS = [1, 3]


def shifts(N):
    return [0, 1, N - 1, N, N + 1, 2 * N - 1]


def placements(N):
    """every (m, spread, shift, groups) of the lists above that the ring admits (m <= N)"""
    return [(m, w, s, g) for m in MS if m <= N for w in sorted({1, N // m}) for s in shifts(N) for g in GROUPS]


def check_key(tools, p, pk, rows, t, b, cases, product):
    """the C++ reference on every case against numpy; the product is computed once and the inner sums once per (m, spread)"""
    R = product(pk, rows, t, b)
    sums = {}
    for m, w, s, g in cases:
        if (m, w) not in sums:
            sums[m, w] = PR.spread_sums(R[:max(GROUPS) * m], w)
        S = sums[m, w]
        got = tools.pack_reference(p, pk, rows[:g * m], m=m, spread=w, shift=s, t=t, basebit=b)
        assert got.shape == (g, 2, p.N)
        assert np.array_equal(got, PR.place(S, g, m, w, s)), (p.n, p.N, t, b, m, w, s, g)


KEYS = ["random", "varied"] + ["constant_%08x" % (int(w) & 0xFFFFFFFF) for w in PR.CARRY_WORDS]


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("t,b", DECOMPOSITIONS)
@pytest.mark.parametrize("n,N", SETS)
def test_reference_is_the_definition_word_for_word(ia, n, N, t, b, key):
    """A random full-range key, the row-by-row varied limb-carry key and each of the seven constant limb-carry keys, every one
    over the whole lattice of placements at every set and decomposition."""
    from ieache_amd import tools
    p = ia.default_params().copy(n=n, N=N)
    rng = np.random.default_rng(7000 + 100 * n + 10 * t + b)
    rows = PR.crafted_rows(rng, max(m for m in MS if m <= N) * max(GROUPS), n, t, b)
    pk = PR.full_range(rng, (n, t, 2, N)) if key == "random" else PR.crafted_keys(n, t, N)[key]
    check_key(tools, p, pk, rows, t, b, placements(N), PR.product if N <= 64 else PR.product_fast)


def test_helper_fast_product_is_the_int64_product():
    """A test of the test helper, not of the feature (it passes without it): pack_reference.product_fast, the two exact float64
    products the larger shapes are checked with, against the int64 matrix product it stands in for."""
    rng = np.random.default_rng(7001)
    for n, N, t, b in [(130, 64, 7, 4), (37, 1024, 31, 1)]:
        rows = PR.crafted_rows(rng, 5, n, t, b)
        for pk in [PR.full_range(rng, (n, t, 2, N))] + list(PR.crafted_keys(n, t, N).values()):
            assert np.array_equal(PR.product_fast(pk, rows, t, b), PR.product(pk, rows, t, b))
    # the whole definition by the literal triple sum, once
    pk, rows = PR.full_range(rng, (5, 8, 2, 16)), PR.full_range(rng, (6, 6))
    want = np.zeros((2, 2, 16), dtype=np.int64)
    R = PR.product(pk, rows, 8, 2)
    for g in range(2):
        for p_ in range(3):
            for q in range(4):
                for c in range(2):
                    want[g, c] += PR._mul_by_xai(R[3 * g + p_, c], (p_ * 4 + q + 30) % 32)
    assert np.array_equal(PR.pack(pk, rows, 3, spread=4, shift=30), PR._wrap32(want))


@pytest.fixture(scope="module")
def reference_keys(ia):
    """n = 630, N = 1024: both secret keys and the packing key (8, 2) at the default noise, made once"""
    from ieache_amd import tools
    p = ia.default_params()
    k = tools.keygen_raw(p, (1, 2, 3), with_cloud=False)
    return p, k, tools.packing_keygen(p, k["lwe_key"], k["tlwe_key"], seed=41)


def torus(x):
    return np.asarray(x, dtype=np.int32).astype(np.float64) / 2.0 ** 32


def torus_distance(a, b):
    d = (np.asarray(a, dtype=np.int64) - np.asarray(b, dtype=np.int64)) & 0xFFFFFFFF
    return np.minimum(d, (1 << 32) - d).astype(np.float64) / 2.0 ** 32


def test_packing_keygen(ia, reference_keys):
    from ieache_amd import tools
    p, k, pk = reference_keys
    assert pk.shape == (630, 8, 2, 1024) and pk.dtype == np.int32
    alpha = p.tlwe_alpha_min
    # every 9th row (all j, both key bits): phase = s_i 2^(32 - (j+1) b) at coefficient 0, 0 elsewhere, within 8 alpha
    idx = np.arange(0, 630 * 8, 9)
    phase = tools.tlwe_phase(p, k["tlwe_key"], pk.reshape(-1, 2, 1024)[idx])
    want = np.zeros_like(phase)
    want[:, 0] = (k["lwe_key"][idx // 8].astype(np.int64) << (32 - (idx % 8 + 1) * 2)).astype(np.uint32).view(np.int32)
    assert set(k["lwe_key"][idx // 8].tolist()) == {0, 1}
    assert torus_distance(phase, want).max() < 8 * alpha
    assert torus_distance(phase, want).max() > 0          # it is an encryption
    # reproducible under a seed, different under another, fresh without one
    small = ia.default_params().copy(n=5, N=16)
    ks = tools.keygen_raw(small, (4, 5), with_cloud=False)
    a = tools.packing_keygen(small, ks["lwe_key"], ks["tlwe_key"], t=5, basebit=3, seed=9)
    assert a.shape == (5, 5, 2, 16) and np.array_equal(a, tools.packing_keygen(small, ks["lwe_key"], ks["tlwe_key"], t=5, basebit=3, seed=9))
    assert not np.array_equal(a, tools.packing_keygen(small, ks["lwe_key"], ks["tlwe_key"], t=5, basebit=3, seed=10))
    assert not np.array_equal(tools.packing_keygen(small, ks["lwe_key"], ks["tlwe_key"]), tools.packing_keygen(small, ks["lwe_key"], ks["tlwe_key"]))
    # alpha: a larger one shows
    wide = tools.packing_keygen(small, ks["lwe_key"], ks["tlwe_key"], t=5, basebit=3, alpha=2.0 ** -10, seed=9)
    ph = tools.tlwe_phase(small, ks["tlwe_key"], wide.reshape(-1, 2, 16))
    assert 2.0 ** -14 < torus_distance(ph[:, 1:], 0).max() < 8 * 2.0 ** -10


def test_bits_pack_and_decode_at_the_reference_parameters(ia, reference_keys):
    """32 encrypted bits at spread 1: +-1/8 on coefficients 0 .. 31 and nothing elsewhere, both within 1/16."""
    from ieache_amd import tools
    p, k, pk = reference_keys
    bits = np.random.default_rng(7002).integers(0, 2, size=32).astype(np.uint8)
    bits[:2] = [0, 1]
    out = tools.pack_reference(p, pk, tools.encrypt_bits(p, k["lwe_key"], bits, 43))
    assert out.shape == (1, 2, 1024)
    phase = torus(tools.tlwe_phase(p, k["tlwe_key"], out)[0])
    err = np.abs(phase[:32] - np.where(bits == 1, 0.125, -0.125))
    print("pack 32 bits: largest phase error %.3e on the bits, %.3e elsewhere" % (err.max(), np.abs(phase[32:]).max()))
    assert err.max() < 1 / 16 and np.abs(phase[32:]).max() < 1 / 16


def test_table_layout_is_lut_test_poly(ia, reference_keys):
    """Four encrypted entries at lut_pack_layout: the phase is lut_test_poly(f) at every coefficient within 1/16."""
    from ieache_amd import tools
    p, k, pk = reference_keys
    assert tools.lut_pack_layout(p, 4) == (256, 2048 - 128) and tools.lut_pack_layout(p, 512) == (2, 2047)
    with pytest.raises(ValueError):
        tools.lut_pack_layout(p, 3)
    for f_bits in ([1, 0, 0, 1], [0, 1, 1, 1]):
        f = np.where(np.array(f_bits) == 1, 1 << 29, -(1 << 29)).astype(np.int32)
        spread, shift = tools.lut_pack_layout(p, 4)
        out = tools.pack_reference(p, pk, tools.encrypt_bits(p, k["lwe_key"], np.array(f_bits, dtype=np.uint8), 44), spread=spread, shift=shift)
        err = torus_distance(tools.tlwe_phase(p, k["tlwe_key"], out)[0], tools.lut_test_poly(p, f))
        print("table layout, 4 entries: largest phase error %.3e" % err.max())
        assert err.max() < 1 / 16


def refused(ia, match, f, *a, **kw):
    with pytest.raises(ia.IeacheError, match=match) as e:
        f(*a, **kw)
    assert e.value.code == -22


def test_refusals_and_accepted_sets(ia):
    """Each bound at its last accepted and its first refused value, for key generation and for the reference."""
    from ieache_amd import tools
    p = ia.default_params().copy(n=5, N=16)
    k = tools.keygen_raw(p, (4, 5), with_cloud=False)
    gen = lambda t, b, pp=p: tools.packing_keygen(pp, k["lwe_key"], k["tlwe_key"], t=t, basebit=b, seed=3)
    for t, b in [(31, 1), (15, 2), (10, 3), (7, 4), (1, 1), (1, 4)]:
        assert gen(t, b).shape == (5, t, 2, 16)
    refused(ia, "below 32", gen, 32, 1)
    refused(ia, "below 32", gen, 16, 2)
    refused(ia, "below 32", gen, 11, 3)
    refused(ia, "below 32", gen, 8, 4)
    refused(ia, "pk_basebit", gen, 4, 5)
    refused(ia, "pk_basebit", gen, 4, 0)
    refused(ia, "pk_t", gen, 0, 2)
    refused(ia, "unsupported", gen, 8, 2, p.copy(N=8))
    # n t (2^b - 1) 128 < 2^31: at t = 7, b = 4 the last n is 159 783 (only the check runs: the refusal comes before any work)
    big = p.copy(n=159784)
    with pytest.raises(ia.IeacheError, match="2\\^31") as e:
        tools.pack_reference(big, np.zeros(1, dtype=np.int32), np.zeros((1, 159785), dtype=np.int32), m=1, t=7, basebit=4)
    assert e.value.code == -22
    pk, rows = gen(8, 2), np.zeros((16, 6), dtype=np.int32)
    ref = lambda m, spread, shift, r=rows: tools.pack_reference(p, pk, r[:max(m, 0)], m=m, spread=spread, shift=shift)
    assert ref(16, 1, 0).shape == (1, 2, 16) and ref(1, 16, 31).shape == (1, 2, 16) and ref(2, 8, 0).shape == (1, 2, 16)
    refused(ia, "m must", ref, 0, 1, 0)
    refused(ia, "spread must", ref, 1, 0, 0)
    refused(ia, "exceed N", ref, 2, 9, 0)
    refused(ia, "exceed N", ref, 1, 17, 0)
    refused(ia, "shift", ref, 1, 1, 32)
    refused(ia, "shift", ref, 1, 1, -1)
    assert tools.pack_reference(p, pk, rows[:0], m=4).shape == (0, 2, 16)   # no groups: nothing to do
    refused(ia, "below 32", tools.pack_reference, p, pk, rows[:1], m=1, t=16, basebit=2)


def test_pack_plan_under_asan_ubsan(tmp_path):
    """tests/native/pack_plan_test.cpp: a stand-alone program over csrc/pack_plan.h."""
    exe = tmp_path / "pack_plan_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "native", "pack_plan_test.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "PACK_PLAN_OK" in r.stdout, r.stdout[-4000:]


def test_reference_under_asan_ubsan(tmp_path):
    """packing_keygen and pack_reference of csrc/tfhe_host.cpp in a stand-alone program: every bound of the rotate-and-sum
    (shift 0, N - 1, N, 2N - 1; m spread = N) on the smallest ring and at N = 1024."""
    csrc = os.path.join(ROOT, "ie-ache_amd", "csrc")
    exe = tmp_path / "pack_reference_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I", csrc, os.path.join(ROOT, "tests", "native", "pack_reference_test.cpp"),
                           os.path.join(csrc, "tfhe_host.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "PACK_REFERENCE_OK" in r.stdout, r.stdout[-4000:]
