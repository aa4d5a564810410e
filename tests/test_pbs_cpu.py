"""Programmable bootstrap, the parts that need no GPU: the reference the GPU tests compare against (lut_reference.py) pinned to
the oracle's own bootstrap and to an independent numpy restatement, the table -> test polynomial rule, the argument checks of
the host entry point, and the noise budget of lookup tables at the reference's parameters."""
import ctypes as C
import types

import numpy as np
import pytest

import lut_reference as LR

MU = 1 << 29
EINVAL = -22


def i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def random_rows(rng, count, n):
    return rng.integers(-(1 << 31), 1 << 31, size=(count, n + 1), dtype=np.int64).astype(np.int32)


@pytest.mark.parametrize("n,N,rows", [(10, 16, 6), (10, 64, 4), (630, 1024, 1)])
def test_the_reference_with_the_constant_polynomial_is_the_oracles_bootstrap(make_keys, n, N, rows):
    """Pins the composition itself: with v = (mu, ..., mu) it is orc_bootstrap and orc_bootstrap_woks word for word."""
    kb = make_keys(n, N)
    x = random_rows(np.random.default_rng(700 + N), rows, n)
    v = np.full(N, MU, dtype=np.int32)
    for r in x:
        assert np.array_equal(LR.pbs_reference(kb.ck, r, v), kb.ck.bootstrap(r))
        assert np.array_equal(LR.pbs_reference(kb.ck, r, v, keyswitch=False), kb.ck.bootstrap_woks(r))
    assert np.array_equal(LR.pbs_reference_rows(kb.ck, x, v[None]), np.stack([kb.ck.bootstrap(r) for r in x]))


@pytest.mark.parametrize("n,N", [(10, 16), (5, 64)])
def test_a_numpy_restatement_agrees_with_the_reference_on_random_polynomials(make_keys, n, N):
    kb = make_keys(n, N)
    p = kb.p
    K = types.SimpleNamespace(n=p.n, N=p.N, l=p.l, Bgbit=p.Bgbit, ks_t=p.ks_t, ks_basebit=p.ks_basebit, bk=kb.bk, ksk=kb.ksk)
    rng = np.random.default_rng(710 + N)
    x = random_rows(rng, 4, n)
    polys = rng.integers(-(1 << 31), 1 << 31, size=(4, N), dtype=np.int64).astype(np.int32)
    polys[0, :4] = [-(1 << 31), (1 << 31) - 1, 0, -1]
    for r, v in zip(x, polys):
        assert np.array_equal(LR.np_pbs(K, r, v, keyswitch=False), LR.pbs_reference(kb.ck, r, v, keyswitch=False))
        assert np.array_equal(LR.np_pbs(K, r, v), LR.pbs_reference(kb.ck, r, v))
    # and the restatement with the constant polynomial is np_tfhe's own bootstrap
    import np_tfhe
    assert np.array_equal(LR.np_pbs(K, x[0], np.full(N, MU, dtype=np.int32)), np_tfhe.np_bootstrap(K, x[0]))


def test_rows_with_a_zero_mask_return_the_rotated_polynomial(make_keys):
    """Every bara_i = 0: no CMux step runs and the extracted b term is coefficient 0 of X^(2N-barb) * v, i.e. v[barb] for
    barb < N and -v[barb - N] otherwise -- the convention of include/ieache.h read off the reference."""
    kb = make_keys(10, 16)
    N = 16
    v = np.arange(1, N + 1, dtype=np.int32)
    for barb in (0, 1, N - 1, N, N + 1, 2 * N - 1):
        x = np.zeros(11, dtype=np.int32)
        x[10] = LR._wrap32(barb << (32 - 5))  # 2N = 32 steps
        u = LR.pbs_reference(kb.ck, x, v, keyswitch=False)
        assert u[N] == (v[barb] if barb < N else -v[barb - N]) and not u[:N].any(), barb


@pytest.mark.parametrize("N", [16, 1024])
def test_lut_test_poly_is_the_headers_rule(ia, N):
    from ieache_amd import tools
    p = ia.default_params().copy(N=N)
    rng = np.random.default_rng(720 + N)
    for entries in (1, 2, 4, 8, N // 2):
        f = rng.integers(-(1 << 31), 1 << 31, size=entries, dtype=np.int64).astype(np.int32)
        f[0] = -(1 << 31) if entries == 2 else f[0]  # -f[0] wraps
        v = tools.lut_test_poly(p, f)
        assert v.dtype == np.int32 and np.array_equal(v, LR.lut_poly(N, f)), entries
        h = N // (2 * entries)
        # every slot is centred on its message, and the polynomial ends in -f[0]
        for m in range(entries):
            centre = m * N // entries
            lo, hi = max(centre - h, 0), centre + h
            assert (v[lo:hi] == f[m]).all()
        assert (v[N - h:] == LR._wrap32(-np.int64(f[0]))).all()
    for entries in (3, 5, N // 2 + 1, N):
        with pytest.raises(ia.IeacheError, match="must divide N") as e:
            tools.lut_test_poly(p, np.zeros(entries, dtype=np.int32))
        assert e.value.code == EINVAL
    f, v = np.zeros(1, np.int32), np.zeros(N, np.int32)
    for entries in (0, -1):
        assert ia.lib().ieache_lut_test_poly(C.byref(p), entries, i32p(f), i32p(v)) == EINVAL


def test_host_entry_refuses_bad_tables_and_the_symbols_are_exported(ia):
    L = ia.lib()
    for name in ("ieache_pbs", "ieache_pbs_device", "ieache_extract_stride", "ieache_lut_test_poly"):
        assert hasattr(L, name), name
    assert ia.PBS_NO_KEYSWITCH == 1
    assert callable(ia.Context.pbs) and callable(ia.Context.pbs_device) and callable(ia.tools.lut_test_poly)
    assert L.ieache_extract_stride(None) == EINVAL
    n, N = 10, 16
    x, out = np.zeros((3, n + 1), np.int32), np.zeros((3, n + 1), np.int32)
    tv = np.zeros((2, N), np.int32)

    def call(n_polys, table, poly_of, flags=0):
        of = None if poly_of is None else i32p(np.asarray(poly_of, dtype=np.int32))
        return L.ieache_pbs(None, 3, i32p(x), None if table is None else i32p(table), n_polys, of, i32p(out), flags, None)

    for args, message in (((0, tv, None), "n_polys must be at least 1"),
                          ((2, None, None), "null test polynomial table"),
                          ((2, tv, [0, 2, 1]), "poly_of[1] = 2 is outside [0, n_polys)"),
                          ((2, tv, [0, 1, -1]), "poly_of[2] = -1 is outside [0, n_polys)"),
                          ((2, tv, None, 2), "unknown flag")):
        assert call(*args) == EINVAL and message in L.ieache_last_error().decode(), args[:1] + args[2:]
    # a well-formed table gets as far as the missing context
    assert call(2, tv, [0, 1, 1]) == EINVAL and L.ieache_last_error().decode() == "null argument"
    assert L.ieache_pbs_device(None, 3, None, None, 0, None, None, 0, None) == EINVAL
    assert "n_polys must be at least 1" in L.ieache_last_error().decode()


def test_noise_budget_of_lookup_tables(ia):
    """DESIGN.md section 7.  A p-entry table has slots of width 1/(2p): a message sits 1/(4p) from the nearest slot boundary.
    The input of a table is k outputs of earlier bootstraps added up (k = 1: one table's output fed to the next), each with
    variance V and the per-key offset delta shared by all of them (taken at 4 of its standard deviations, against the
    slot), plus the rounding of the n + 1 coefficients to 2N steps.  margin = (1/(4p) - k delta) / sqrt(k V + rounding)."""
    from test_golden_cpu import predicted_gate_output_noise
    p = ia.default_params()
    V, offset_sd = predicted_gate_output_noise(p)
    rounding = (1 + p.n / 2) / 12.0 / (2.0 * p.N) ** 2
    assert abs(V - 1.05e-5) < 0.03e-5 and abs(offset_sd - 1.2e-3) < 0.05e-3 and abs(rounding - 6.3e-6) < 0.1e-6

    def margin(entries, k):
        return (1.0 / (4 * entries) - k * 4 * offset_sd) / np.sqrt(k * V + rounding)

    m41, m42, m81 = margin(4, 1), margin(4, 2), margin(8, 1)
    assert abs(m41 - 14.1) < 0.3 and abs(m42 - 10.1) < 0.3 and abs(m81 - 6.4) < 0.3
    assert m41 >= 12 and m42 >= 9
    assert m81 < 8  # eight entries at libtfhe's gate parameters: not recommended; four is the ceiling
    assert m41 < 15  # ... and even four stays below what the gates keep
