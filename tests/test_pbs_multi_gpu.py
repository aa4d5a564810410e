"""The multi-output programmable bootstrap on the GPU, word for word against the untouched CPU oracle composed in
multi_reference.py (modswitch -> acc = (0, X^(2N-barb) v) -> blind_rotate -> schoolbook product with each factor ->
sample_extract -> + bias -> keyswitch).  Bit-exact cases take uniformly random rows -- no encryption is needed for that -- at
n = 37 (the 64-lane kernels accept n = 7 .. 129) and on toy rings, so that the oracle stays affordable; the table test runs at
the reference's parameters."""
import numpy as np
import pytest

import lut_reference as LR
import multi_reference as MR

pytestmark = pytest.mark.gpu

N = 1024
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def random_rows(rng, count, n):
    return rng.integers(INT32_MIN, 1 << 31, size=(count, n + 1), dtype=np.int64).astype(np.int32)


def random_polys(rng, count, ring):
    v = rng.integers(INT32_MIN, 1 << 31, size=(count, ring), dtype=np.int64).astype(np.int32)
    v[0, :4] = [INT32_MIN, INT32_MAX, 0, -1]
    return v


def factor_set(rng, ring):
    """1; X; X^(N/2); -X^(N-1) = X^(-1); dense full-range with INT32_MIN and INT32_MAX; a sparse table factor; all zero."""
    dense = rng.integers(INT32_MIN, 1 << 31, size=ring, dtype=np.int64).astype(np.int32)
    dense[[3, ring - 1]] = [INT32_MIN, INT32_MAX]
    return np.stack([MR.monomial(ring, 0), MR.monomial(ring, 1), MR.monomial(ring, ring // 2), MR.monomial(ring, -1), dense,
                     MR.factor_poly(ring, [0, 1, 0, 1]), np.zeros(ring, dtype=np.int32)])


ONE, X1, XHALF, XINV, DENSE, SPARSE, ZERO = range(7)
BIAS = np.array([0x20000000, INT32_MIN, -0x20000000, 1, INT32_MAX, -1, 0x12345678], dtype=np.int64).astype(np.int32)


def without_bias(ck, u):
    """(extracted, key-switched) reference rows of the same call with bias NULL."""
    u0 = u.copy()
    u0[..., -1] = LR._wrap32(u[..., -1].astype(np.int64) - BIAS[None, :].astype(np.int64))
    return u0, np.stack([[ck.keyswitch(r) for r in item] for item in u0])


_case = {}


def case37(kb):
    """64 random rows at n = 37, two full-range test polynomials with a mixed index array, the seven factors with a non-zero
    bias each, and the oracle's outputs [64][7][...] with and without the bias: computed once."""
    if not _case:
        rng = np.random.default_rng(901)
        x, polys = random_rows(rng, 64, 37), random_polys(rng, 2, N)
        of = rng.integers(0, 2, size=64).astype(np.int32)
        of[:2] = [1, 0]
        factors = factor_set(rng, N)
        u, ks = MR.multi_reference_rows(kb.ck, x, polys, factors, of, BIAS)
        u0, ks0 = without_bias(kb.ck, u[:40])
        _case.update(x=x, polys=polys, of=of, factors=factors, u=u, ks=ks, u0=u0, ks0=ks0)
    return _case


@pytest.mark.parametrize("count", [1, 3, 5, 40])
@pytest.mark.parametrize("pick", [[ONE], [DENSE, ZERO], [ONE, X1, XHALF, XINV, SPARSE]], ids=["1", "2", "5"])
def test_w64_kernels_word_for_word(ia, gpu_ctx, count, pick):
    kb, ctx = gpu_ctx(37, N)
    c = case37(kb)
    assert "generic" not in ctx.kernel_variant
    x, of, fa = c["x"][:count], c["of"][:count], c["factors"][pick]
    for bias, u, ks in ((BIAS[pick], c["u"], c["ks"]), (None, c["u0"], c["ks0"])):
        st = ia.Stats()
        out = ctx.pbs_multi(x, c["polys"], fa, of, bias, stats=st)
        assert out.shape == (count, len(pick), 38) and np.array_equal(out, ks[:count][:, pick])
        assert st.bootstraps == count and st.levels == 1 and st.keyswitch_launches >= 1
        st = ia.Stats()
        out = ctx.pbs_multi(x, c["polys"], fa, of, bias, keyswitch=False, stats=st)
        assert out.shape == (count, len(pick), N + 1) and np.array_equal(out, u[:count][:, pick])
        assert st.bootstraps == count and st.keyswitch_launches == 0 and st.blind_rotate_launches >= 1
    if ONE in pick:  # the factor 1 without bias is the single-output bootstrap of the same rows, bit for bit
        t = pick.index(ONE)
        assert np.array_equal(ctx.pbs_multi(x, c["polys"], fa, of)[:, t], ctx.pbs(x, c["polys"], of))
        assert np.array_equal(ctx.pbs_multi(x, c["polys"], fa, of, keyswitch=False)[:, t], ctx.pbs(x, c["polys"], of, keyswitch=False))
    if ZERO in pick:  # the all-zero factor: (0, bias) before the key switch
        t = pick.index(ZERO)
        out = ctx.pbs_multi(x, c["polys"], fa, of, BIAS[pick], keyswitch=False)[:, t]
        assert not out[:, :N].any() and (out[:, N] == BIAS[ZERO]).all()


def test_the_whole_factor_set_in_one_call(ia, gpu_ctx):
    kb, ctx = gpu_ctx(37, N)
    c = case37(kb)
    st = ia.Stats()
    assert np.array_equal(ctx.pbs_multi(c["x"][:40], c["polys"], c["factors"], c["of"][:40], BIAS, stats=st), c["ks"][:40])
    assert st.bootstraps == 40
    assert np.array_equal(ctx.pbs_multi(c["x"][:40], c["polys"], c["factors"], c["of"][:40], BIAS, keyswitch=False), c["u"][:40])
    assert np.array_equal(ctx.pbs_multi(c["x"][:40], c["polys"], c["factors"], c["of"][:40]), c["ks0"])
    # one polynomial for every row, one factor given as [N]; nothing to do
    u1, ks1 = MR.multi_reference_rows(kb.ck, c["x"][:4], c["polys"][1:2], c["factors"][DENSE])
    assert np.array_equal(ctx.pbs_multi(c["x"][:4], c["polys"][1], c["factors"][DENSE]), ks1)
    st = ia.Stats()
    assert ctx.pbs_multi(c["x"][:0], c["polys"], c["factors"], stats=st).shape == (0, 7, 38) and st.bootstraps == 0
    with pytest.raises(ia.IeacheError, match="outside"):
        ctx.pbs_multi(c["x"][:2], c["polys"], c["factors"], [0, 2])


def test_every_cut_keeps_rows_with_their_item_and_factor(ia, gpu_ctx):
    kb, ctx = gpu_ctx(37, N)
    c = case37(kb)
    pick = [X1, DENSE, SPARSE]
    x, of, polys, fa, bias = c["x"][:13], c["of"][:13], c["polys"], c["factors"][pick], BIAS[pick]
    u, ks = c["u"][:13][:, pick], c["ks"][:13][:, pick]

    def both():
        return ctx.pbs_multi(x, polys, fa, of, bias), ctx.pbs_multi(x, polys, fa, of, bias, keyswitch=False)

    uncut, uncut_u = both()
    assert np.array_equal(uncut, ks) and np.array_equal(uncut_u, u)
    saved = {k: ctx.get_option(k) for k in ("chunk", "overlap", "overlap_min")}
    try:
        for chunk, pieces in ((5, 13), (7, 7), (2, 13)):  # pieces of max(1, chunk / 3) items: 1, 2 and (chunk < n_factors) 1
            ctx.set_chunk(chunk)
            st = ia.Stats()
            assert np.array_equal(ctx.pbs_multi(x, polys, fa, of, bias, stats=st), uncut), chunk
            assert st.chunks == pieces and st.bootstraps == 13 and st.keyswitch_launches == pieces
            st = ia.Stats()
            assert np.array_equal(ctx.pbs_multi(x, polys, fa, of, bias, keyswitch=False, stats=st), uncut_u), chunk
            assert st.chunks == pieces and st.keyswitch_launches == 0
        ctx.set_option("overlap_min", 2)  # chunk 2: single items alternating between two lanes
        lv = ctx.get_option("overlapped_levels")
        got = both()
        assert np.array_equal(got[0], uncut) and np.array_equal(got[1], uncut_u)
        assert ctx.get_option("overlapped_levels") == lv + 2
        ctx.set_chunk(saved["chunk"])  # the level's two halves, 8 + 5 items
        got = both()
        assert np.array_equal(got[0], uncut) and np.array_equal(got[1], uncut_u)
        assert ctx.get_option("overlapped_levels") == lv + 4
        ctx.set_option("overlap_min", saved["overlap_min"])
        ctx.set_option("overlap", 0)  # one stream
        got = both()
        assert np.array_equal(got[0], uncut) and np.array_equal(got[1], uncut_u)
    finally:
        ctx.set_chunk(saved["chunk"])
        for k in ("overlap", "overlap_min"):
            ctx.set_option(k, saved[k])


def test_exact_paths(ia, gpu_ctx):
    kb, ctx = gpu_ctx(37, N)
    c = case37(kb)
    pick = [ONE, DENSE, SPARSE]
    x, of, polys, fa, bias = c["x"], c["of"], c["polys"], c["factors"][pick], BIAS[pick]
    u, ks = c["u"][:, pick], c["ks"][:, pick]
    saved = {k: ctx.get_option(k) for k in ("exact_fft", "fft_audit")}
    try:
        ctx.set_option("exact_fft", 1)
        assert np.array_equal(ctx.pbs_multi(x[:40], polys, fa, of[:40], bias), ks[:40])
        assert np.array_equal(ctx.pbs_multi(x[:40], polys, fa, of[:40], bias, keyswitch=False), u[:40])
        ctx.set_option("exact_fft", 0)
        # a guard trip: the whole call is repeated on the two-limb kernels and finds tables and factors again
        _, reruns = ctx.fft_guard()
        ctx.set_option("fft_guard_inject", 1)
        assert np.array_equal(ctx.pbs_multi(x[:40], polys, fa, of[:40], bias), ks[:40]) and ctx.fft_guard()[1] == reruns + 1
        ctx.set_option("fft_guard_inject", 1)
        assert np.array_equal(ctx.pbs_multi(x[:40], polys, fa, of[:40], bias, keyswitch=False), u[:40]) and ctx.fft_guard()[1] == reruns + 2
        # the sampled audit re-runs 64 items of the launch on the two-limb kernel and compares their PLAIN extractions
        before = ctx.fft_audit()
        ctx.set_option("fft_audit", 1)
        assert np.array_equal(ctx.pbs_multi(x, polys, fa, of, bias), ks)
        assert np.array_equal(ctx.pbs_multi(x, polys, fa, of, bias, keyswitch=False), u)
        after = ctx.fft_audit()
        assert after["audits"] > before["audits"] and after["gates_compared"] >= before["gates_compared"] + 64
        assert after["mismatches"] == before["mismatches"] == 0
        assert ctx.fft_guard()[1] == reruns + 2
    finally:
        for k, v in saved.items():
            ctx.set_option(k, v)


def device_rows(rows, stride):
    import torch
    d = torch.zeros((rows.shape[0], stride), dtype=torch.int32, device="cuda")
    d[:, : rows.shape[1]] = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    return d


def test_device_form(ia, gpu_ctx):
    import torch
    kb, ctx = gpu_ctx(37, N)
    c = case37(kb)
    pick = [XINV, DENSE, ZERO]
    fa, bias = c["factors"][pick], BIAS[pick]
    d_x = device_rows(c["x"][:8], ctx.lwe_stride)
    d_tv, d_of = torch.from_numpy(c["polys"]).cuda(), torch.from_numpy(c["of"][:8]).cuda()
    d_fa, d_bias = torch.from_numpy(fa).cuda(), torch.from_numpy(bias).cuda()
    d_out = torch.full((8 * 3, ctx.lwe_stride), 7, dtype=torch.int32, device="cuda")
    d_u = torch.full((8 * 3, ctx.extract_stride), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    args = (8, d_x.data_ptr(), d_tv.data_ptr(), 2, d_of.data_ptr(), d_fa.data_ptr(), 3, d_bias.data_ptr())
    st = ia.Stats()
    ctx.pbs_multi_device(*args, d_out.data_ptr(), stats=st)
    assert np.array_equal(d_out.cpu().numpy()[:, :38].reshape(8, 3, 38), c["ks"][:8][:, pick]) and st.bootstraps == 8
    st = ia.Stats()
    ctx.pbs_multi_device(*args, d_u.data_ptr(), keyswitch=False, stats=st)
    assert np.array_equal(d_u.cpu().numpy()[:, :N + 1].reshape(8, 3, N + 1), c["u"][:8][:, pick])
    assert st.bootstraps == 8 and st.keyswitch_launches == 0
    # no index array (row 0 of the table given), no bias
    ctx.pbs_multi_device(8, d_x.data_ptr(), d_tv[1:].data_ptr(), 1, None, d_fa[1:].data_ptr(), 1, None, d_u.data_ptr(), keyswitch=False)
    want, _ = MR.multi_reference_rows(kb.ck, c["x"][:8], c["polys"][1:], fa[1:2])
    assert np.array_equal(d_u.cpu().numpy()[:8, :N + 1], want[:, 0])
    # the inputs are as they were
    assert np.array_equal(d_fa.cpu().numpy(), fa) and np.array_equal(d_tv.cpu().numpy(), c["polys"])
    assert np.array_equal(d_x.cpu().numpy()[:, :38], c["x"][:8]) and np.array_equal(d_bias.cpu().numpy(), bias)
    with pytest.raises(ia.IeacheError, match="overlaps"):  # the output over the factors
        ctx.pbs_multi_device(8, d_x.data_ptr(), d_tv.data_ptr(), 2, None, d_u.data_ptr(), 3, None, d_u.data_ptr(), keyswitch=False)
    with pytest.raises(ia.IeacheError, match="overlaps"):  # ... over the rows: there is no in-place form
        ctx.pbs_multi_device(8, d_out.data_ptr(), d_tv.data_ptr(), 2, None, d_fa.data_ptr(), 3, None, d_out.data_ptr())
    with pytest.raises(ia.IeacheError, match="overlaps"):  # ... over the bias
        ctx.pbs_multi_device(8, d_x.data_ptr(), d_tv.data_ptr(), 2, None, d_fa.data_ptr(), 3, d_out.data_ptr(), d_out.data_ptr())
    with pytest.raises(ia.IeacheError, match="not a device pointer"):
        ctx.pbs_multi_device(8, d_x.data_ptr(), d_tv.data_ptr(), 2, None, fa.ctypes.data, 3, None, d_out.data_ptr())
    with pytest.raises(ia.IeacheError, match="not a device pointer"):
        ctx.pbs_multi_device(8, d_x.data_ptr(), d_tv.data_ptr(), 2, None, d_fa.data_ptr(), 3, bias.ctypes.data, d_out.data_ptr())
    for n_factors in (0, 65):
        with pytest.raises(ia.IeacheError, match="n_factors") as e:
            ctx.pbs_multi_device(8, d_x.data_ptr(), d_tv.data_ptr(), 2, None, d_fa.data_ptr(), n_factors, None, d_out.data_ptr())
        assert e.value.code == -22


@pytest.mark.parametrize("n,ring,kw", [(10, 16, {}), (10, 64, {}),
                                       (12, N, dict(l=2, Bgbit=10, lwe_alpha_min=2.44e-5, tlwe_alpha_min=7.18e-9))])
def test_any_parameter_and_two_limb_kernels(ia, gpu_ctx, n, ring, kw):
    """Toy rings run on k_blind_rotate_generic (fewer coefficients than threads in k_mv_extract); the l = 2 / Bgbit = 10 set at
    N = 1024 on the two-limb 64-lane kernels."""
    kb, ctx = gpu_ctx(n, ring, **kw)
    assert ("generic" in ctx.kernel_variant) == (ring != N)
    rng = np.random.default_rng(910 + ring)
    x, polys = random_rows(rng, 9, n), random_polys(rng, 3, ring)
    of = np.array([0, 1, 2, 2, 1, 0, 1, 1, 2], dtype=np.int32)
    pick = [XINV, DENSE, SPARSE]
    fa, bias = factor_set(rng, ring)[pick], BIAS[pick]
    u, ks = MR.multi_reference_rows(kb.ck, x, polys, fa, of, bias)
    assert np.array_equal(ctx.pbs_multi(x, polys, fa, of, bias), ks)
    assert np.array_equal(ctx.pbs_multi(x, polys, fa, of, bias, keyswitch=False), u)
    chunk = ctx.get_option("chunk")
    try:
        ctx.set_chunk(4)  # single items
        st = ia.Stats()
        assert np.array_equal(ctx.pbs_multi(x, polys, fa, of, bias, stats=st), ks) and st.chunks == 9
    finally:
        ctx.set_chunk(chunk)


def test_warm_host_calls_allocate_nothing(ia, gpu_ctx):
    kb, ctx = gpu_ctx(37, N)
    c = case37(kb)
    x, of, polys, fa = c["x"][:40], c["of"][:40], c["polys"], c["factors"]
    for keyswitch, want in ((True, c["ks"][:40]), (False, c["u"][:40])):
        assert np.array_equal(ctx.pbs_multi(x, polys, fa, of, BIAS, keyswitch=keyswitch), want)
        warm = ctx.get_option("staging_allocations")
        assert np.array_equal(ctx.pbs_multi(x, polys, fa, of, BIAS, keyswitch=keyswitch), want)
        assert np.array_equal(ctx.pbs_multi(x[:7], polys, fa[:3], of[:7], BIAS[:3], keyswitch=keyswitch), want[:7, :3])
        assert ctx.get_option("staging_allocations") == warm


def test_thermometer_and_parity_at_the_product_parameters(ia, gpu_ctx):
    """n = 630: 64 fresh encryptions of m / 8, 16 of each message, through ONE call that rotates the constant polynomial 1/8 and
    multiplies by the factors of w = [0,1,1,1], [0,0,1,1], [0,0,0,1] (m >= 1, 2, 3; |P|^2 = 2) and [0,1,0,1] (parity; 4), bias
    -1/8: output t of message m is a gate bit at 2 (1/8) w_t[m] - 1/8 = +-1/8.  Every GPU row is the composed oracle's and
    every row's phase has the sign w_t[m] dictates -- asserted for the oracle first: zero wrong decodes is the condition for both.
    The largest output phase error against 1/8 is printed (pytest -s): 0.0113 of the torus on the card and for the oracle alike
    (|P|^2 = 2: 0.0102, |P|^2 = 4: 0.0113), the half slot being 0.125."""
    from ieache_amd import tools
    kb, ctx = gpu_ctx(630, N)
    tables = np.array([[0, 1, 1, 1], [0, 0, 1, 1], [0, 0, 0, 1], [0, 1, 0, 1]])
    factors = np.stack([tools.lut_factor_poly(kb.p, w) for w in tables])
    assert [MR.norm2(P) for P in factors] == [2, 2, 2, 4]
    const = np.full(N, 1 << 29, dtype=np.int32)
    bias = np.full(4, -(1 << 29), dtype=np.int32)
    rng = np.random.default_rng(930)
    msgs = np.repeat(np.arange(4), 16)
    x = LR.encrypt_messages(kb.p, kb.lwe_key, msgs, 4, rng)
    want_bits = tables[:, msgs].T  # [64][4]

    def decode(rows):
        return (LR.phases(kb.lwe_key, rows) > 0).astype(np.int64)

    _, ref = MR.multi_reference_rows(kb.ck, x, const[None], factors, None, bias)
    assert np.array_equal(decode(ref), want_bits)
    st = ia.Stats()
    out = ctx.pbs_multi(x, const, factors, bias=bias, stats=st)
    assert st.bootstraps == 64 and st.keyswitch_launches == 1
    assert np.array_equal(out, ref)
    assert np.array_equal(decode(out), want_bits)
    err = np.abs(LR.phases(kb.lwe_key, out) - (2 * want_bits - 1) / 8.0)
    print("largest output phase error against 1/8: %.4f (|P|^2 = 2: %.4f, |P|^2 = 4: %.4f; half slot 0.1250)"
          % (err.max(), err[:, :3].max(), err[:, 3].max()))
