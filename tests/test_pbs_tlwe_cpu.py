"""Blind rotation on a caller's TLWE accumulator, whole-accumulator output and the public key switch: the parts that need no
GPU.  The exported symbols and the argument checks of the host entry points; the two TLWE host tools (round trip within the
noise, the sign convention tied to the bootstrapping key's rows, a stand-alone program under AddressSanitizer + UBSan); the
reference the GPU tests compare against (tlwe_reference.py: the oracle's stages composed) pinned to a numpy restatement that
shares no code with the oracle; and the noise paragraph of DESIGN.md section 7 on private tables."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import lut_reference as LR
import tlwe_reference as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22


def i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def full_range(rng, shape):
    return rng.integers(-(1 << 31), 1 << 31, size=shape, dtype=np.int64).astype(np.int32)


def test_the_symbols_are_exported_and_the_flags_are_checked_before_the_context(ia):
    L = ia.lib()
    for name in ("ieache_keyswitch", "ieache_keyswitch_device", "ieache_tlwe_encrypt", "ieache_tlwe_phase"):
        assert hasattr(L, name), name
    assert ia.PBS_TLWE_POLYS == 4 and ia.PBS_ACCUMULATOR == 8 and ia.PBS_NO_KEYSWITCH == 1
    for f in (ia.Context.keyswitch, ia.Context.keyswitch_device, ia.tools.tlwe_encrypt, ia.tools.tlwe_phase):
        assert callable(f)
    n, N = 10, 16
    x, out = np.zeros((3, n + 1), np.int32), np.zeros((3 * 2, 2 * N), np.int32)
    tv, fa, bias = np.zeros((2, 2, N), np.int32), np.zeros((2, N), np.int32), np.zeros(2, np.int32)

    def pbs(flags, n_polys=2, table=tv, poly_of=None):
        of = None if poly_of is None else i32p(np.asarray(poly_of, dtype=np.int32))
        return L.ieache_pbs(None, 3, i32p(x), None if table is None else i32p(table), n_polys, of, i32p(out), flags, None)

    def multi(flags):
        return L.ieache_pbs_multi(None, 3, i32p(x), i32p(tv), 2, None, i32p(fa), 2, i32p(bias), i32p(out), flags, None)

    def message():
        return L.ieache_last_error().decode()

    # the value 2 names no flag, alone or beside the new bits, on both entries
    for flags in (2, 2 | 4, 2 | 8, 2 | 4 | 8 | 1, 16, 32):
        assert pbs(flags) == EINVAL and "unknown flag" in message(), flags
        assert L.ieache_pbs_device(None, 3, None, None, 1, None, None, flags, None) == EINVAL and "unknown flag" in message(), flags
    for flags in (2, 2 | 4, 16):
        assert multi(flags) == EINVAL and "unknown flag" in message(), flags
        assert L.ieache_pbs_multi_device(None, 3, None, None, 1, None, None, 1, None, None, flags, None) == EINVAL and "unknown flag" in message()
    # whole accumulators are an output of ieache_pbs only
    for flags in (8, 8 | 4, 8 | 1):
        assert multi(flags) == EINVAL and "IEACHE_PBS_ACCUMULATOR" in message(), flags
        assert L.ieache_pbs_multi_device(None, 3, None, None, 1, None, None, 1, None, None, flags, None) == EINVAL
        assert "IEACHE_PBS_ACCUMULATOR" in message()
    # the new bits themselves pass the flag check: argument errors come next, and well-formed arguments reach the missing context
    for flags in (4, 8, 4 | 8, 1 | 4, 1 | 4 | 8):
        assert pbs(flags, n_polys=0) == EINVAL and "n_polys must be at least 1" in message(), flags
        assert pbs(flags, table=None) == EINVAL and "null test polynomial table" in message(), flags
        assert pbs(flags, poly_of=[0, 2, 1]) == EINVAL and "poly_of[1] = 2 is outside [0, n_polys)" in message(), flags
        assert pbs(flags, poly_of=[0, 1, 1]) == EINVAL and message() == "null argument", flags
    for flags in (4, 1 | 4):
        assert multi(flags) == EINVAL and message() == "null argument", flags
    # the key switch: nothing but its pointers to judge
    u, ks = np.zeros((3, N + 1), np.int32), np.zeros((3, n + 1), np.int32)
    assert L.ieache_keyswitch(None, 3, i32p(u), i32p(ks), None) == EINVAL and message() == "null argument"
    assert L.ieache_keyswitch_device(None, 3, None, None, None) == EINVAL and message() == "null argument"
    # the tools
    p = ia.default_params().copy(N=N)
    key = np.zeros(N, np.int32)
    assert L.ieache_tlwe_encrypt(None, i32p(key), i32p(fa), 2, 0.0, 1, i32p(tv)) == EINVAL
    assert L.ieache_tlwe_encrypt(C.byref(p), None, i32p(fa), 2, 0.0, 1, i32p(tv)) == EINVAL
    assert L.ieache_tlwe_encrypt(C.byref(p), i32p(key), None, 2, 0.0, 1, i32p(tv)) == EINVAL
    assert L.ieache_tlwe_phase(C.byref(p), i32p(key), None, 2, i32p(fa)) == EINVAL and message() == "null argument"
    assert L.ieache_tlwe_encrypt(C.byref(p), i32p(key), None, 0, 0.0, 1, None) == 0  # count == 0: a no-op
    assert L.ieache_tlwe_phase(C.byref(p), i32p(key), None, 0, None) == 0


@pytest.mark.parametrize("N", [16, 64, 1024])
def test_tlwe_encrypt_then_phase_round_trips_within_the_noise(ia, N):
    from ieache_amd import tools
    p = ia.default_params().copy(N=N)
    rng = np.random.default_rng(900 + N)
    key = rng.integers(0, 2, size=N).astype(np.int32)
    polys = full_range(rng, (3, N))
    polys[0, :4] = [-(1 << 31), (1 << 31) - 1, 0, -1]
    alpha = 2.0 ** -25
    assert p.tlwe_alpha_min == alpha
    for a in (None, alpha):  # the default is the parameter set's
        c = tools.tlwe_encrypt(p, key, polys, 5, alpha=a)
        assert c.shape == (3, 2, N) and c.dtype == np.int32 and c[:, 0].any()
        ph = tools.tlwe_phase(p, key, c)
        assert np.array_equal(ph, TR.np_tlwe_phase(key, c))  # the exact phase, by numpy's convolution
        err = LR._wrap32(ph.astype(np.int64) - polys.astype(np.int64)).astype(np.float64) / 2.0 ** 32
        assert np.abs(err).max() < 6 * alpha and err.std() > alpha / 3
    assert np.array_equal(tools.tlwe_encrypt(p, key, polys, 5), tools.tlwe_encrypt(p, key, polys, 5))  # a seed reproduces
    assert not np.array_equal(tools.tlwe_encrypt(p, key, polys, 5), tools.tlwe_encrypt(p, key, polys, 6))
    assert not np.array_equal(tools.tlwe_encrypt(p, key, polys, 0), tools.tlwe_encrypt(p, key, polys, 0))  # 0: kernel entropy
    # alpha = 1e-30: every draw is far below half a torus step of 2^-33 and rounds to 0, so the round trip is exact
    # (alpha <= 0 would mean the default)
    c = tools.tlwe_encrypt(p, key, polys, 7, alpha=1e-30)
    assert np.array_equal(tools.tlwe_phase(p, key, c), polys)
    # one polynomial, one sample; nothing
    assert np.array_equal(tools.tlwe_phase(p, key, tools.tlwe_encrypt(p, key, polys[1], 7, alpha=1e-30)), polys[1:2])
    assert tools.tlwe_encrypt(p, key, polys[:0], 7).shape == (0, 2, N) and tools.tlwe_phase(p, key, c[:0]).shape == (0, N)


@pytest.mark.parametrize("n,N", [(10, 16), (10, 64)])
def test_a_bootstrapping_key_row_has_the_phase_the_tool_expects(ia, make_keys, n, N):
    """Ties the tool's sign convention (phase B - A s) to the key's: rows bloc * l + q of BK_i are encryptions of 0 plus
    s_i 2^(32 - (q+1) Bgbit) on the constant coefficient of polynomial `bloc` -- on B that is the phase itself, on A it enters
    the phase as -h s.  The external product of the oracle is only right under this convention."""
    from ieache_amd import tools
    kb = make_keys(n, N)
    p = kb.p
    ph = tools.tlwe_phase(p, kb.tlwe_key, kb.bk.reshape(-1, 2, N)).reshape(n, 2, p.l, N).astype(np.int64)
    bound = 6 * p.tlwe_alpha_min * 2.0 ** 32
    for i in range(n):
        for q in range(p.l):
            h = int(kb.lwe_key[i]) << (32 - (q + 1) * p.Bgbit)
            on_b = np.zeros(N, dtype=np.int64)
            on_b[0] = h
            on_a = -h * kb.tlwe_key[:N].astype(np.int64)
            for bloc, msg in ((0, on_a), (1, on_b)):
                err = LR._wrap32(ph[i, bloc, q] - msg).astype(np.int64)
                assert np.abs(err).max() < bound, (i, bloc, q)
    assert kb.lwe_key.any() and not kb.lwe_key.all()  # both key bits were seen


@pytest.mark.parametrize("n,N", [(10, 16), (10, 64)])
def test_the_composed_oracle_is_a_numpy_restatement_word_for_word(make_keys, n, N):
    kb = make_keys(n, N)
    p = kb.p
    K = types.SimpleNamespace(n=p.n, N=p.N, l=p.l, Bgbit=p.Bgbit, ks_t=p.ks_t, ks_basebit=p.ks_basebit, bk=kb.bk, ksk=kb.ksk)
    rng = np.random.default_rng(910 + N)
    x, samples = full_range(rng, (5, n + 1)), full_range(rng, (5, 2, N))
    samples[0, :, :4] = [-(1 << 31), (1 << 31) - 1, 0, -1]
    rows = TR.tlwe_reference_rows(kb.ck, x, samples, np.arange(5))
    for i in range(5):
        for what in (TR.ACC, TR.EXTRACTED, TR.KEYSWITCHED):
            want = TR.np_tlwe_pbs(K, x[i], samples[i], what)
            assert np.array_equal(TR.tlwe_reference(kb.ck, x[i], samples[i], what), want), (i, what)
            assert np.array_equal(rows[what][i], want), (i, what)
    # coefficient 0 of the accumulator, extracted in numpy, is the oracle's extracted sample
    assert np.array_equal(TR.extract_coefficient(rows[TR.ACC]), rows[TR.EXTRACTED])
    # ... and the tool reads such accumulators as the restatement's phase does
    from ieache_amd import tools
    assert np.array_equal(tools.tlwe_phase(p, kb.tlwe_key, rows[TR.ACC]), TR.np_tlwe_phase(kb.tlwe_key, rows[TR.ACC]))
    # with A = 0 both are the plain-table reference
    for i in range(2):
        z = TR.with_zero_mask(samples[i, 1])
        assert np.array_equal(TR.tlwe_reference(kb.ck, x[i], z), LR.pbs_reference(kb.ck, x[i], samples[i, 1]))
        assert np.array_equal(TR.np_tlwe_pbs(K, x[i], z, TR.EXTRACTED), LR.np_pbs(K, x[i], samples[i, 1], keyswitch=False))


def test_noise_of_a_private_table(ia):
    """an encrypted table adds its own encryption variance once -- a monomial rotation permutes and negates
    coefficients, it does not amplify -- so V_out = V + sigma_tv^2 with sigma_tv = tlwe_alpha_min = 2^-25: 9e-16 against
    V = 1.05e-5, and the margins of the lookup-table budget stand to the digits they are quoted with."""
    from test_golden_cpu import predicted_gate_output_noise
    p = ia.default_params()
    V, offset_sd = predicted_gate_output_noise(p)
    var_tv = p.tlwe_alpha_min ** 2
    assert p.tlwe_alpha_min == 2.0 ** -25 and abs(var_tv - 8.9e-16) < 0.1e-16 and abs(V - 1.05e-5) < 0.03e-5
    assert var_tv / V < 1e-9
    # sigma_tv is what the tool puts on a table: 8 192 coefficients, whose sample variance is within 8 % (5 of its standard
    # deviations, sqrt(2 / 8192) = 1.6 %; the 2^-32 grid adds 1/12 of a step squared, 5e-6 of it) of tlwe_alpha_min squared
    from ieache_amd import tools
    rng = np.random.default_rng(930)
    key, polys = rng.integers(0, 2, size=p.N).astype(np.int32), full_range(rng, (8, p.N))
    err = LR._wrap32(tools.tlwe_phase(p, key, tools.tlwe_encrypt(p, key, polys, 931)).astype(np.int64) - polys.astype(np.int64))
    assert abs((err.astype(np.float64) / 2.0 ** 32).var() / var_tv - 1) < 0.08
    rounding = (1 + p.n / 2) / 12.0 / (2.0 * p.N) ** 2

    def margin(entries, k, extra):
        return (1.0 / (4 * entries) - k * 4 * offset_sd) / np.sqrt(k * (V + extra) + rounding)

    for entries, k, quoted in ((4, 1, 14.1), (4, 2, 10.1), (8, 1, 6.4)):
        plain, private = margin(entries, k, 0.0), margin(entries, k, var_tv)
        assert abs(plain - quoted) < 0.3 and 0 <= plain - private < 1e-6, (entries, k)


def test_the_tools_under_sanitizers(tmp_path):
    """tests/native/tlwe_tools_test.cpp with csrc/tfhe_host.cpp, AddressSanitizer + UBSan: count = 0, N = 16 and N = 1024."""
    exe = tmp_path / "tlwe_tools_test"
    csrc = os.path.join(ROOT, "ie-ache_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", csrc, os.path.join(ROOT, "tests", "native", "tlwe_tools_test.cpp"),
                           os.path.join(csrc, "tfhe_host.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "TLWE_TOOLS_OK" in r.stdout, r.stdout[-4000:]
