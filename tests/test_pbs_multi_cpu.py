"""Multi-output programmable bootstrap, the parts that need no GPU: the table -> factor rule through the ABI, the identity behind
it ((1 + X + ... + X^(N-1)) (1 - X) = 2), the reference the GPU tests compare against (multi_reference.py) pinned to the
single-output reference and to the oracle's accumulator, the extraction rule k_mv_extract implements restated in numpy, the
argument checks of the host entry point, and the noise budget of DESIGN.md section 7."""
import ctypes as C

import numpy as np
import pytest

import lut_reference as LR
import multi_reference as MR
from np_tfhe import _negacyclic, _wrap32

EINVAL = -22
SCHOOLBOOK = MR.O.POLYMUL_SCHOOLBOOK


def i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def random_rows(rng, count, n):
    return rng.integers(-(1 << 31), 1 << 31, size=(count, n + 1), dtype=np.int64).astype(np.int32)


@pytest.mark.parametrize("N", [16, 64, 1024])
def test_lut_factor_poly_is_v_times_one_minus_x(ia, O, N):
    from ieache_amd import tools
    p = ia.default_params().copy(N=N)
    rng = np.random.default_rng(900 + N)
    entries = 1
    while 2 * entries <= N:
        w = rng.integers(-9, 10, size=entries).astype(np.int32)
        P = tools.lut_factor_poly(p, w)
        v = LR.lut_poly(N, w)
        assert np.array_equal(v, tools.lut_test_poly(p, w))
        assert P.dtype == np.int32 and np.array_equal(P, MR.factor_poly(N, w)), entries
        one_minus_x = np.zeros(N, dtype=np.int32)
        one_minus_x[0], one_minus_x[1] = 1, -1
        assert np.array_equal(P, O.negacyclic_mul(one_minus_x, v, mode=SCHOOLBOOK))
        assert np.count_nonzero(P) <= entries + 1
        # rotating the CONSTANT polynomial c and multiplying by P is a rotation from 2c v, word for word
        for c in (1 << 29, 0x12345678, -(1 << 31)):
            const = np.full(N, c, dtype=np.int32)
            assert np.array_equal(O.negacyclic_mul(P, const, mode=SCHOOLBOOK), _wrap32(2 * c * v.astype(np.int64))), (entries, c)
        entries *= 2
    # full-range entries wrap like everything else
    w = np.array([-(1 << 31), (1 << 31) - 1], dtype=np.int32)
    assert np.array_equal(tools.lut_factor_poly(p, w), MR.factor_poly(N, w))
    for entries in (3, 5, N // 2 + 1, N):
        with pytest.raises(ia.IeacheError, match="must divide N") as e:
            tools.lut_factor_poly(p, np.zeros(entries, dtype=np.int32))
        assert e.value.code == EINVAL
    w, P = np.zeros(1, np.int32), np.zeros(N, np.int32)
    for entries in (0, -1):
        assert ia.lib().ieache_lut_factor_poly(C.byref(p), entries, i32p(w), i32p(P)) == EINVAL
    assert ia.lib().ieache_lut_factor_poly(C.byref(p), 1, None, i32p(P)) == EINVAL


def test_factor_norms_of_binary_tables():
    """|P|^2 = sum of squared jumps between neighbouring entries plus (w[0] + w[last])^2 at the negacyclic wrap."""
    N = 1024
    assert [MR.norm2(MR.factor_poly(N, w)) for w in ([0, 1, 1, 1], [0, 0, 1, 1], [0, 0, 0, 1], [0, 1, 0, 1])] == [2, 2, 2, 4]
    assert [MR.norm2(MR.factor_poly(N, w)) for w in ([0, 1], [1, 0], [1, 1])] == [2, 2, 4]
    assert max(MR.norm2(MR.factor_poly(N, [(m >> i) & 1 for i in range(4)])) for m in range(16)) == 6
    assert MR.norm2(MR.monomial(N, 0)) == 1


@pytest.mark.parametrize("N", [16, 64])
def test_schoolbook_products_agree_with_numpy_for_small_factors(O, N):
    rng = np.random.default_rng(910 + N)
    for _ in range(4):
        P = rng.integers(-128, 128, size=N).astype(np.int32)
        big = rng.integers(-(1 << 31), 1 << 31, size=N, dtype=np.int64).astype(np.int32)
        assert np.array_equal(O.negacyclic_mul(P, big, mode=SCHOOLBOOK), _negacyclic(P.astype(np.int64), big))
    # ... and with Python integers for full-range ones, where int64 would overflow
    P = rng.integers(-(1 << 31), 1 << 31, size=N, dtype=np.int64).astype(np.int32)
    P[:2] = [-(1 << 31), (1 << 31) - 1]
    big = rng.integers(-(1 << 31), 1 << 31, size=N, dtype=np.int64).astype(np.int32)
    want = [0] * N
    for i in range(N):
        for j in range(N):
            s = int(P[i]) * int(big[j])
            want[(i + j) % N] += s if i + j < N else -s
    assert np.array_equal(O.negacyclic_mul(P, big, mode=SCHOOLBOOK), _wrap32(np.array([w & 0xFFFFFFFF for w in want], dtype=np.int64)))


def kernel_rule(acc, P, bias=0):
    """k_mv_extract's rule in numpy: over the nonzero coefficients (j_k, c_k) of P, u[j] = -sum_k c_k Aext[N - j - j_k] and
    u[N] = sum_k c_k Bext[-j_k] + bias, with Xext[i] = X[i mod N], negated where i mod 2N >= N."""
    N = acc.shape[1]
    A, B = (a.astype(np.int64) for a in acc)
    u = np.zeros(N + 1, dtype=np.int64)
    j = np.arange(N)
    b = 0
    for jk in np.flatnonzero(P):
        c = int(P[jk])
        s = (N - j - jk) % (2 * N)
        u[:N] -= c * np.where(s >= N, -A[s % N], A[s % N])
        s = (-jk) % (2 * N)
        b += c * (-int(B[s % N]) if s >= N else int(B[s % N]))
    u[N] = (b + bias) & 0xFFFFFFFF
    return _wrap32(u & 0xFFFFFFFF)


@pytest.mark.parametrize("n,N", [(10, 16), (5, 64), (3, 1024)])
def test_reference_special_cases_and_the_kernels_rule(make_keys, n, N):
    kb = make_keys(n, N)
    ck = kb.ck
    rng = np.random.default_rng(920 + N)
    x = random_rows(rng, 2, n)
    v = rng.integers(-(1 << 31), 1 << 31, size=N, dtype=np.int64).astype(np.int32)
    dense = rng.integers(-(1 << 31), 1 << 31, size=N, dtype=np.int64).astype(np.int32)
    dense[:2] = [-(1 << 31), (1 << 31) - 1]
    for r in x:
        acc = MR.accumulator(ck, r, v)
        # P = 1 is the single-output bootstrap
        for ks in (True, False):
            assert np.array_equal(MR.multi_reference(ck, r, v, MR.monomial(N, 0), keyswitch=ks)[0], LR.pbs_reference(ck, r, v, keyswitch=ks))
        # P = X^(-j) extracts coefficient j of the accumulator
        for j in (1, 5, N // 2, N - 1):
            u = MR.multi_reference(ck, r, v, MR.monomial(N, -j), keyswitch=False)[0]
            assert u[N] == acc[1][j] and u[0] == acc[0][j]
            assert np.array_equal(u, ck.sample_extract(np.stack([LR._mul_by_xai(a, 2 * N - j) for a in acc])))
        # the all-zero factor leaves (0, bias)
        u = MR.multi_reference(ck, r, v, np.zeros(N, np.int32), bias=[-(1 << 31)], keyswitch=False)[0]
        assert not u[:N].any() and u[N] == -(1 << 31)
        # the extraction rule of the device kernel, factor by factor
        factors = np.stack([MR.monomial(N, 0), MR.monomial(N, 1), MR.monomial(N, N // 2), MR.monomial(N, -1), dense,
                            MR.factor_poly(N, [0, 1, 0, 1]), np.zeros(N, np.int32)])
        bias = rng.integers(-(1 << 31), 1 << 31, size=len(factors), dtype=np.int64).astype(np.int32)
        want = MR.multi_from_accumulator(ck, acc, factors, bias, keyswitch=False)
        for t, P in enumerate(factors):
            assert np.array_equal(kernel_rule(acc, P, int(bias[t])), want[t]), t
    u, ks = MR.multi_reference_rows(ck, x, v[None], factors, bias=bias)
    assert u.shape == (2, len(factors), N + 1) and ks.shape == (2, len(factors), n + 1)
    assert np.array_equal(u[1], want) and np.array_equal(ks[1, 4], ck.keyswitch(want[4]))


def test_host_entry_refuses_bad_arguments_and_the_symbols_are_exported(ia):
    L = ia.lib()
    for name in ("ieache_pbs_multi", "ieache_pbs_multi_device", "ieache_lut_factor_poly"):
        assert hasattr(L, name), name
    assert ia.PBS_MULTI_MAX_FACTORS == 64
    assert callable(ia.Context.pbs_multi) and callable(ia.Context.pbs_multi_device) and callable(ia.tools.lut_factor_poly)
    n, N = 10, 16
    x, out = np.zeros((3, n + 1), np.int32), np.zeros((3 * 65, n + 1), np.int32)
    tv, fa, bias = np.zeros((2, N), np.int32), np.zeros((65, N), np.int32), np.zeros(65, np.int32)

    def call(n_polys=2, table=tv, poly_of=None, factors=fa, n_factors=2, flags=0):
        of = None if poly_of is None else i32p(np.asarray(poly_of, dtype=np.int32))
        return L.ieache_pbs_multi(None, 3, i32p(x), None if table is None else i32p(table), n_polys, of,
                                  None if factors is None else i32p(factors), n_factors, i32p(bias), i32p(out), flags, None)

    for kw, message in ((dict(n_polys=0), "n_polys must be at least 1"),
                        (dict(table=None), "null test polynomial table"),
                        (dict(n_factors=0), "n_factors must be 1 .. 64"),
                        (dict(n_factors=65), "n_factors must be 1 .. 64"),
                        (dict(n_factors=-1), "n_factors must be 1 .. 64"),
                        (dict(factors=None), "null factor table"),
                        (dict(poly_of=[0, 2, 1]), "poly_of[1] = 2 is outside [0, n_polys)"),
                        (dict(flags=2), "unknown flag")):
        assert call(**kw) == EINVAL and message in L.ieache_last_error().decode(), kw
    # well-formed arguments get as far as the missing context
    assert call(poly_of=[0, 1, 1], n_factors=64) == EINVAL and L.ieache_last_error().decode() == "null argument"
    assert L.ieache_pbs_multi_device(None, 3, None, None, 1, None, None, 0, None, None, 0, None) == EINVAL
    assert "null test polynomial table" in L.ieache_last_error().decode()


def test_noise_budget_of_multi_output_tables(ia):
    """DESIGN.md section 7.  An output of the multi-output bootstrap carries V_out = |P|^2 (V - V_ks) + V_ks: the rotation's share
    of a bootstrap's output variance V times the factor's squared norm, the key switch's share V_ks once.  The margin of a
    consumer with `entries` slots whose input is k such outputs added up is section 7's formula with V_out for V:
    (1/(4 entries) - k 4 offset_sd) / sqrt(k V_out + rounding).  The tables of the GPU test give gate bits at +-1/8, i.e. a
    two-slot consumer (a message sits 1/8 from the nearest boundary)."""
    from test_golden_cpu import predicted_gate_output_noise
    p = ia.default_params()
    V, offset_sd = predicted_gate_output_noise(p)
    ks = MR.keyswitch_variance(p)
    assert abs(ks - 4.29e-6) < 0.02e-6 and 0 < ks < V
    assert MR.output_variance(p, V, 1) == pytest.approx(V)
    m41 = MR.margin(p, V, offset_sd, 4, 1, 1)  # section 7's four-entry table fed by one plain bootstrap output
    assert abs(m41 - 14.1) < 0.3
    # ordering: a larger norm, more summands or more slots each leave less margin
    for entries in (2, 4):
        for k in (1, 2):
            ms = [MR.margin(p, V, offset_sd, entries, k, n2) for n2 in (1, 2, 4, 6)]
            assert all(a > b for a, b in zip(ms, ms[1:])), (entries, k, ms)
    assert MR.margin(p, V, offset_sd, 2, 2, 2) < MR.margin(p, V, offset_sd, 2, 1, 2)
    # the thermometer ([0,1,1,1], [0,0,1,1], [0,0,0,1]: |P|^2 = 2) and parity ([0,1,0,1]: 4) tables of the GPU test, whose
    # outputs are gate bits: at least the margin section 7 accepts for a four-entry table
    N = p.N
    for w in ([0, 1, 1, 1], [0, 0, 1, 1], [0, 0, 0, 1], [0, 1, 0, 1]):
        n2 = MR.norm2(MR.factor_poly(N, w))
        assert MR.margin(p, V, offset_sd, 2, 1, n2) >= m41 >= 12, w
    figures = {(e, k, n2): MR.margin(p, V, offset_sd, e, k, n2) for e in (2, 4) for k in (1, 2) for n2 in (1, 2, 4, 6)}
    print("\n".join("entries %d, k %d, |P|^2 %d: margin %.1f" % (key + (m,)) for key, m in sorted(figures.items())))
    # the figures DESIGN.md section 7 quotes
    assert abs(figures[(2, 1, 2)] - 25.0) < 0.3 and abs(figures[(2, 1, 4)] - 20.1) < 0.3 and abs(figures[(2, 1, 6)] - 17.3) < 0.3
    assert abs(figures[(2, 2, 2)] - 18.3) < 0.3 and abs(figures[(2, 2, 4)] - 14.3) < 0.3 and abs(figures[(2, 2, 6)] - 12.2) < 0.3
    assert figures[(4, 1, 2)] < m41 and abs(figures[(4, 1, 2)] - 12.0) < 0.3 and abs(figures[(4, 1, 4)] - 9.7) < 0.3
