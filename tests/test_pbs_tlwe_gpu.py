"""Blind rotation on a caller's TLWE accumulator (an encrypted table), whole-accumulator output and the public key switch on the
GPU, word for word against the untouched CPU oracle composed in tlwe_reference.py (modswitch -> acc = X^(2N-barb) (A, B) ->
blind_rotate [-> sample_extract [-> keyswitch]]).  Bit-exact cases take uniformly random rows and full-range random TLWE samples
-- no encryption is needed for that -- at n = 37 (the 64-lane kernels accept n = 7 .. 129) and on toy rings, so that the oracle
stays affordable; the private-table test runs at the reference's parameters."""
import numpy as np
import pytest

import lut_reference as LR
import multi_reference as MR
import tlwe_reference as TR

pytestmark = pytest.mark.gpu

N = 1024
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def full_range(rng, shape):
    return rng.integers(INT32_MIN, 1 << 31, size=shape, dtype=np.int64).astype(np.int32)


def random_samples(rng, count, ring):
    """TLWE rows with full-range random A and B, a few words of both halves pinned to the extremes."""
    s = full_range(rng, (count, 2, ring))
    s[0, :, :4] = [INT32_MIN, INT32_MAX, 0, -1]
    s[-1, :, -2:] = [INT32_MAX, INT32_MIN]
    return s


_case = {}


def case37(kb):
    """64 random rows at n = 37, three full-range TLWE samples, a mixed index array, and the oracle's whole accumulators,
    extracted samples and key-switched rows: computed once."""
    if not _case:
        rng = np.random.default_rng(1001)
        x, samples = full_range(rng, (64, 38)), random_samples(rng, 3, N)
        of = rng.integers(0, 3, size=64).astype(np.int32)
        of[:3] = [2, 0, 1]
        ref = TR.tlwe_reference_rows(kb.ck, x, samples, of)
        _case.update(x=x, samples=samples, of=of, acc=ref[TR.ACC], u=ref[TR.EXTRACTED], ks=ref[TR.KEYSWITCHED])
    return _case


def head(c, rows):
    return c["x"][:rows], c["samples"], c["of"][:rows], c["acc"][:rows], c["u"][:rows], c["ks"][:rows]


def test_w64_prologue_word_for_word(ia, gpu_ctx):
    kb, ctx = gpu_ctx(37, N)
    x, samples, of, acc, u, ks = head(case37(kb), 40)
    assert "generic" not in ctx.kernel_variant
    st = ia.Stats()
    assert np.array_equal(ctx.pbs(x, samples, of, tlwe=True, stats=st), ks)
    assert st.bootstraps == 40 and st.levels == 1 and st.keyswitch_launches >= 1
    st = ia.Stats()
    assert np.array_equal(ctx.pbs(x, samples, of, keyswitch=False, tlwe=True, stats=st), u)
    assert st.bootstraps == 40 and st.keyswitch_launches == 0 and st.blind_rotate_launches >= 1
    for keyswitch in (True, False):  # whole accumulators: no key switch either way
        st = ia.Stats()
        out = ctx.pbs(x, samples, of, keyswitch=keyswitch, tlwe=True, accumulator=True, stats=st)
        assert out.shape == (40, 2, N) and np.array_equal(out, acc)
        assert st.bootstraps == 40 and st.levels == 1 and st.keyswitch_launches == 0 and st.blind_rotate_launches >= 1
    # one sample for every row, given as [2][N]; one row; nothing to do
    one = TR.tlwe_reference_rows(kb.ck, x[:8], samples[1:2])
    assert np.array_equal(ctx.pbs(x[:8], samples[1], tlwe=True), one[TR.KEYSWITCHED])
    assert np.array_equal(ctx.pbs(x[:8], samples[1], tlwe=True, accumulator=True), one[TR.ACC])
    assert np.array_equal(ctx.pbs(x[:1], samples, of[:1], tlwe=True, accumulator=True), acc[:1])
    st = ia.Stats()
    assert ctx.pbs(x[:0], samples, of[:0], tlwe=True, stats=st).shape == (0, 38) and st.bootstraps == 0
    assert ctx.pbs(x[:0], samples, tlwe=True, accumulator=True).shape == (0, 2, N)
    with pytest.raises(ia.IeacheError, match="outside"):
        ctx.pbs(x[:2], samples, [0, 3], tlwe=True)


def test_anchors_to_the_calls_that_exist(ia, gpu_ctx):
    kb, ctx = gpu_ctx(37, N)
    x, samples, of, acc, u, ks = head(case37(kb), 24)
    # A = 0: the plain call on B, bit for bit
    polys, zero_mask = samples[:, 1], TR.with_zero_mask(samples[:, 1])
    plain, plain_u = ctx.pbs(x, polys, of), ctx.pbs(x, polys, of, keyswitch=False)
    assert np.array_equal(ctx.pbs(x, zero_mask, of, tlwe=True), plain)
    assert np.array_equal(ctx.pbs(x, zero_mask, of, keyswitch=False, tlwe=True), plain_u)
    rng = np.random.default_rng(1002)
    factors = np.stack([MR.monomial(N, 0), full_range(rng, N)])
    assert np.array_equal(ctx.pbs_multi(x[:8], zero_mask, factors, of[:8], tlwe=True), ctx.pbs_multi(x[:8], polys, factors, of[:8]))
    assert np.array_equal(ctx.pbs_multi(x[:8], zero_mask, factors, of[:8], keyswitch=False, tlwe=True),
                          ctx.pbs_multi(x[:8], polys, factors, of[:8], keyswitch=False))
    # whole accumulators from the constant polynomial: the gate path's rotation
    mu = np.full(N, 1 << 29, dtype=np.int32)
    assert np.array_equal(ctx.pbs(x, mu, accumulator=True), ctx.debug_blind_rotate(x))
    # coefficient 0 of the returned accumulator, extracted in numpy, is the call without key switch; its key switch is the call
    got_acc, got_u, got_ks = (ctx.pbs(x, samples, of, tlwe=True, accumulator=True), ctx.pbs(x, samples, of, keyswitch=False, tlwe=True),
                              ctx.pbs(x, samples, of, tlwe=True))
    assert np.array_equal(TR.extract_coefficient(got_acc), got_u) and np.array_equal(got_u, u)
    assert np.array_equal(ctx.keyswitch(got_u), got_ks) and np.array_equal(ctx.debug_keyswitch(got_u), got_ks) and np.array_equal(got_ks, ks)


def rotated_closed_form(p, barb):
    """X^(2N-barb) p: coefficient j is p[(j + barb) mod N], negated where (j + barb) mod 2N >= N."""
    n = len(p)
    idx = (np.arange(n) + barb) % (2 * n)
    return LR._wrap32(np.where(idx < n, 1, -1) * p[idx % n].astype(np.int64))


@pytest.mark.parametrize("generic", [False, True])
def test_rotation_boundaries_of_both_halves(ia, gpu_ctx, generic):
    """a = 0: every bara_i is 0, no CMux step runs, and the accumulator is the rotated sample itself."""
    kb, ctx = gpu_ctx(37, N)
    barbs = [0, 1, N - 1, N, N + 1, 2 * N - 1]
    x = np.zeros((len(barbs), 38), dtype=np.int32)
    x[:, 37] = LR._wrap32(np.array(barbs, dtype=np.int64) << 21)  # 2N = 2^11 steps
    A = np.arange(1, N + 1, dtype=np.int32)
    B = LR._wrap32(-np.arange(1, N + 1, dtype=np.int64) * 3)
    want = np.stack([np.stack([rotated_closed_form(A, b), rotated_closed_form(B, b)]) for b in barbs])
    assert np.array_equal(want[0], np.stack([A, B])) and want[1][0][N - 1] == -1 and want[1][1][N - 1] == 3
    sample = np.stack([A, B])
    assert np.array_equal(TR.tlwe_reference_rows(kb.ck, x, sample[None])[TR.ACC], want)
    try:
        ctx.force_generic(generic)
        assert ("generic" in ctx.kernel_variant) == generic
        assert np.array_equal(ctx.pbs(x, sample, tlwe=True, accumulator=True), want)
        assert np.array_equal(ctx.pbs(x, sample, keyswitch=False, tlwe=True), TR.extract_coefficient(want))
    finally:
        ctx.force_generic(False)


def test_every_cut_of_a_flat_launch_keeps_the_table_and_the_rows(ia, gpu_ctx):
    kb, ctx = gpu_ctx(37, N)
    x, samples, of, acc, u, ks = head(case37(kb), 13)

    def all_three():
        return (ctx.pbs(x, samples, of, tlwe=True), ctx.pbs(x, samples, of, keyswitch=False, tlwe=True),
                ctx.pbs(x, samples, of, tlwe=True, accumulator=True))

    def check(got):
        assert np.array_equal(got[0], ks) and np.array_equal(got[1], u) and np.array_equal(got[2], acc)

    check(all_three())
    saved = {k: ctx.get_option(k) for k in ("chunk", "overlap", "overlap_min")}
    try:
        ctx.set_chunk(5)  # pieces of 5, 5, 3
        for kw in (dict(), dict(accumulator=True)):
            st = ia.Stats()
            ctx.pbs(x, samples, of, tlwe=True, stats=st, **kw)
            assert st.chunks == 3 and st.bootstraps == 13 and st.keyswitch_launches == (0 if kw else 3)
        check(all_three())
        ctx.set_option("overlap_min", 2)  # ... alternating between two lanes
        lv = ctx.get_option("overlapped_levels")
        check(all_three())
        assert ctx.get_option("overlapped_levels") == lv + 3
        ctx.set_chunk(saved["chunk"])  # the level's two halves, 8 + 5
        check(all_three())
        assert ctx.get_option("overlapped_levels") == lv + 6
        ctx.set_option("overlap_min", saved["overlap_min"])
        ctx.set_option("overlap", 0)  # one stream
        check(all_three())
    finally:
        ctx.set_chunk(saved["chunk"])
        for k in ("overlap", "overlap_min"):
            ctx.set_option(k, saved[k])


@pytest.mark.parametrize("n,ring,kw", [(10, 16, {}), (10, 64, {}),
                                       (12, N, dict(l=2, Bgbit=10, lwe_alpha_min=2.44e-5, tlwe_alpha_min=7.18e-9))])
def test_any_parameter_and_two_limb_kernels(ia, gpu_ctx, n, ring, kw):
    """Toy rings run on k_blind_rotate_generic; the l = 2 / Bgbit = 10 set at N = 1024 on the two-limb 64-lane kernels."""
    kb, ctx = gpu_ctx(n, ring, **kw)
    assert ("generic" in ctx.kernel_variant) == (ring != N)
    rng = np.random.default_rng(1010 + ring)
    x, samples = full_range(rng, (9, n + 1)), random_samples(rng, 3, ring)
    of = np.array([0, 1, 2, 2, 1, 0, 1, 1, 2], dtype=np.int32)
    ref = TR.tlwe_reference_rows(kb.ck, x, samples, of)

    def check():
        assert np.array_equal(ctx.pbs(x, samples, of, tlwe=True), ref[TR.KEYSWITCHED])
        assert np.array_equal(ctx.pbs(x, samples, of, keyswitch=False, tlwe=True), ref[TR.EXTRACTED])
        assert np.array_equal(ctx.pbs(x, samples, of, tlwe=True, accumulator=True), ref[TR.ACC])

    check()
    chunk = ctx.get_option("chunk")
    try:
        ctx.set_chunk(4)
        check()
    finally:
        ctx.set_chunk(chunk)


def device_rows(rows, stride):
    import torch
    d = torch.zeros((rows.shape[0], stride), dtype=torch.int32, device="cuda")
    d[:, : rows.shape[1]] = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    return d


def test_exact_paths(ia, gpu_ctx):
    import torch
    kb, ctx = gpu_ctx(37, N)
    c = case37(kb)
    x, samples, of, acc, u, ks = head(c, 64)
    saved = {k: ctx.get_option(k) for k in ("exact_fft", "fft_audit")}
    try:
        ctx.set_option("exact_fft", 1)
        assert np.array_equal(ctx.pbs(x, samples, of, tlwe=True), ks)
        assert np.array_equal(ctx.pbs(x, samples, of, tlwe=True, accumulator=True), acc)
        ctx.set_option("exact_fft", 0)
        # a guard trip: the whole call is repeated on the two-limb kernels and finds the table again
        _, reruns = ctx.fft_guard()
        ctx.set_option("fft_guard_inject", 1)
        assert np.array_equal(ctx.pbs(x, samples, of, tlwe=True), ks) and ctx.fft_guard()[1] == reruns + 1
        ctx.set_option("fft_guard_inject", 1)
        assert np.array_equal(ctx.pbs(x, samples, of, tlwe=True, accumulator=True), acc) and ctx.fft_guard()[1] == reruns + 2
        # the sampled audit re-runs 64 items of the launch on the two-limb kernel: same table, same rows -- extracted samples
        # for the key-switched call, whole accumulators for the accumulator output
        ctx.set_option("fft_audit", 1)
        for kw, want in ((dict(), ks), (dict(accumulator=True), acc)):
            before = ctx.fft_audit()
            assert np.array_equal(ctx.pbs(x, samples, of, tlwe=True, **kw), want)
            after = ctx.fft_audit()
            assert after["audits"] >= before["audits"] + 1 and after["gates_compared"] >= before["gates_compared"] + 64
            assert after["mismatches"] == before["mismatches"] == 0
        assert ctx.fft_guard()[1] == reruns + 2
        ctx.set_option("fft_audit", saved["fft_audit"])
        # the device form with the output over the input rows: the call cannot be repeated, so it runs on the two-limb
        # kernels from the start
        d_x, d_tv, d_of = device_rows(x[:40], ctx.lwe_stride), torch.from_numpy(samples).cuda(), torch.from_numpy(of[:40]).cuda()
        torch.cuda.synchronize()
        st = ia.Stats()
        ctx.pbs_device(40, d_x.data_ptr(), d_tv.data_ptr(), 3, d_of.data_ptr(), d_x.data_ptr(), tlwe=True, stats=st)
        assert np.array_equal(d_x.cpu().numpy()[:, :38], ks[:40]) and st.bootstraps == 40
        assert np.array_equal(d_tv.cpu().numpy(), samples) and np.array_equal(d_of.cpu().numpy(), of[:40])
        assert ctx.fft_guard()[1] == reruns + 2
        # the device form of accumulator output: packed rows of 2N
        d_x, d_acc = device_rows(x[:40], ctx.lwe_stride), torch.zeros((40, 2, N), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        st = ia.Stats()
        ctx.pbs_device(40, d_x.data_ptr(), d_tv.data_ptr(), 3, d_of.data_ptr(), d_acc.data_ptr(), tlwe=True, accumulator=True, stats=st)
        assert np.array_equal(d_acc.cpu().numpy(), acc[:40]) and st.keyswitch_launches == 0
        assert np.array_equal(d_x.cpu().numpy()[:, :38], x[:40])
        # refusals, all before anything is launched.  Accumulator output has no in-place form:
        with pytest.raises(ia.IeacheError, match="overlaps"):
            ctx.pbs_device(40, d_acc.data_ptr(), d_tv.data_ptr(), 3, None, d_acc.data_ptr(), tlwe=True, accumulator=True)
        with pytest.raises(ia.IeacheError, match="overlaps"):
            ctx.pbs_device(1, d_x.data_ptr(), d_tv.data_ptr(), 3, None, d_x.data_ptr(), accumulator=True)
        # ... and the table's rows are 2N words: an output in its second half -- past the 3 N words of a plain table -- overlaps
        # it (one row of lwe_stride words at word 4N of the table's 6N)
        with pytest.raises(ia.IeacheError, match="overlaps the test polynomials"):
            ctx.pbs_device(1, d_x.data_ptr(), d_tv.data_ptr(), 3, None, d_tv.data_ptr() + 4 * N * 4, tlwe=True)
        with pytest.raises(ia.IeacheError, match="not a device pointer"):
            ctx.pbs_device(8, d_x.data_ptr(), samples.ctypes.data, 3, None, d_acc.data_ptr(), tlwe=True)
    finally:
        for k, v in saved.items():
            ctx.set_option(k, v)


def test_pbs_multi_from_a_tlwe_table(ia, gpu_ctx):
    """One rotation from the TLWE sample, then the factors: schoolbook products of the oracle's accumulator."""
    kb, ctx = gpu_ctx(37, N)
    x, samples, of, acc, u, ks = head(case37(kb), 8)
    rng = np.random.default_rng(1020)
    factors = np.stack([MR.monomial(N, 0), MR.monomial(N, -1), full_range(rng, N)])
    want_u = np.stack([MR.multi_from_accumulator(kb.ck, a, factors, keyswitch=False) for a in acc])
    want_ks = np.stack([np.stack([kb.ck.keyswitch(r) for r in item]) for item in want_u])
    assert np.array_equal(want_u[:, 0], u) and np.array_equal(want_ks[:, 0], ks)  # the factor 1 is pbs itself
    st = ia.Stats()
    assert np.array_equal(ctx.pbs_multi(x, samples, factors, of, tlwe=True, stats=st), want_ks) and st.bootstraps == 8
    assert np.array_equal(ctx.pbs_multi(x, samples, factors, of, keyswitch=False, tlwe=True), want_u)
    # whole accumulators are not an output of the multi-output call, with a context as without one
    assert ia.lib().ieache_pbs_multi(ctx.h, 0, None, None, 1, None, None, 1, None, None, ia.PBS_ACCUMULATOR, None) == -22
    assert "IEACHE_PBS_ACCUMULATOR" in ia.lib().ieache_last_error().decode()


@pytest.mark.parametrize("n,ring,rows", [(37, N, 9), (37, N, 70), (10, 64, 9)])
def test_the_key_switch_alone(ia, gpu_ctx, n, ring, rows):
    import torch
    kb, ctx = gpu_ctx(n, ring)
    u = full_range(np.random.default_rng(1030 + rows + ring), (rows, ring + 1))
    want = np.stack([kb.ck.keyswitch(r) for r in u])
    st = ia.Stats()
    assert np.array_equal(ctx.keyswitch(u, stats=st), want)
    assert st.bootstraps == 0 and st.blind_rotate_launches == 0 and st.keyswitch_launches >= 1 and st.levels == 1 and st.chunks >= 1
    assert np.array_equal(ctx.debug_keyswitch(u), want)
    # a warm host call allocates nothing
    warm = ctx.get_option("staging_allocations")
    assert np.array_equal(ctx.keyswitch(u), want) and np.array_equal(ctx.keyswitch(u[:5]), want[:5])
    assert ctx.get_option("staging_allocations") == warm
    # the device form: rows of extract_stride in, rows of lwe_stride out
    d_u, d_out = device_rows(u, ctx.extract_stride), torch.full((rows, ctx.lwe_stride), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    chunk = ctx.get_option("chunk")
    try:
        for c in (chunk, 4):
            ctx.set_chunk(c)
            d_out.fill_(-1)
            torch.cuda.synchronize()
            st = ia.Stats()
            ctx.keyswitch_device(rows, d_u.data_ptr(), d_out.data_ptr(), stats=st)
            assert np.array_equal(d_out.cpu().numpy()[:, :n + 1], want)
            pieces = -(-rows // c)
            assert st.chunks == pieces and st.keyswitch_launches == pieces and st.bootstraps == 0 and st.levels == 1
            assert rows != 9 or c != 4 or st.chunks == 3
            assert np.array_equal(ctx.keyswitch(u), want)  # the host form under the same cut
    finally:
        ctx.set_chunk(chunk)
    assert np.array_equal(d_u.cpu().numpy()[:, :ring + 1], u)
    # nothing to do; an output over the input
    st = ia.Stats()
    assert ctx.keyswitch(u[:0], stats=st).shape == (0, n + 1) and st.keyswitch_launches == 0
    ctx.keyswitch_device(0, d_u.data_ptr(), d_out.data_ptr())
    with pytest.raises(ia.IeacheError, match="overlaps"):
        ctx.keyswitch_device(rows, d_u.data_ptr(), d_u.data_ptr())
    with pytest.raises(ia.IeacheError, match="not a device pointer"):
        ctx.keyswitch_device(rows, u.ctypes.data, d_out.data_ptr())


def test_a_group_gives_the_one_context_results(ia, gpu_ctx):
    kb, ctx = gpu_ctx(37, N)
    x, samples, of, acc, u, ks = head(case37(kb), 7)
    with ia.Group.from_arrays(kb.p, kb.bk, kb.ksk, [0, 0]) as g:
        stats = []
        out = g.pbs(x, samples, of, tlwe=True, stats=stats)
        assert np.array_equal(out, ctx.pbs(x, samples, of, tlwe=True)) and np.array_equal(out, ks)
        assert [s.bootstraps for s in stats] == [4, 3]
        assert np.array_equal(g.pbs(x, samples, of, keyswitch=False, tlwe=True), u)
        stats = []
        out = g.pbs(x, samples, of, tlwe=True, accumulator=True, stats=stats)
        assert out.shape == (7, 2, N) and np.array_equal(out, ctx.pbs(x, samples, of, tlwe=True, accumulator=True)) and np.array_equal(out, acc)
        assert [s.keyswitch_launches for s in stats] == [0, 0]
        mu = np.full(N, 1 << 29, dtype=np.int32)
        assert np.array_equal(g.pbs(x, mu, accumulator=True), ctx.debug_blind_rotate(x))
        factors = np.stack([MR.monomial(N, 0), MR.monomial(N, -1)])
        assert np.array_equal(g.pbs_multi(x, samples, factors, of, tlwe=True), ctx.pbs_multi(x, samples, factors, of, tlwe=True))


def test_a_private_table_at_the_product_parameters(ia, gpu_ctx):
    """A four-entry permutation table at n = 630, ENCRYPTED under the ring key, on 16 fresh encryptions of m / 8, four of each
    message.  The oracle decodes all 16 to perm[m] first; the card's rows are the oracle's word for word and decode the same,
    and so does coefficient 0 of the phase of the returned accumulators.  Zero wrong decodes is the condition: the four-entry
    budget of DESIGN.md section 7 (14 sigma) carries over, the table's noise being 9e-16 against 1.05e-5."""
    from ieache_amd import tools
    kb, ctx = gpu_ctx(630, N)
    p = 4
    rng = np.random.default_rng(1040)
    perm = rng.permutation(p)
    while np.array_equal(perm, np.arange(p)):
        perm = rng.permutation(p)
    table = tools.lut_test_poly(kb.p, [LR.message_phase(m, p) for m in perm])
    private = tools.tlwe_encrypt(kb.p, kb.tlwe_key, table, 1041)
    assert private.shape == (1, 2, N) and private[0, 0].any() and not np.array_equal(private[0, 1], table)
    msgs = np.repeat(np.arange(p), 4)
    x = LR.encrypt_messages(kb.p, kb.lwe_key, msgs, p, rng)

    def decode(fractions):
        return np.rint(np.asarray(fractions) * 2 * p).astype(np.int64) % (2 * p)

    ref = TR.tlwe_reference_rows(kb.ck, x, private)
    assert np.array_equal(decode(LR.phases(kb.lwe_key, ref[TR.KEYSWITCHED])), perm[msgs])
    st = ia.Stats()
    out = ctx.pbs(x, private, tlwe=True, stats=st)
    assert st.bootstraps == 16 and st.keyswitch_launches == 1
    assert np.array_equal(out, ref[TR.KEYSWITCHED]) and np.array_equal(decode(LR.phases(kb.lwe_key, out)), perm[msgs])
    acc = ctx.pbs(x, private, tlwe=True, accumulator=True)
    assert np.array_equal(acc, ref[TR.ACC])
    coef0 = tools.tlwe_phase(kb.p, kb.tlwe_key, acc)[:, 0].astype(np.float64) / 2.0 ** 32
    assert np.array_equal(decode(coef0), perm[msgs])
    # how far from the slot centres the outputs came, beside the plain table's figure (printed: pytest -s)
    plain = ctx.pbs(x, table)
    assert np.array_equal(decode(LR.phases(kb.lwe_key, plain)), perm[msgs])

    def worst(rows):
        return np.abs(LR.phases(kb.lwe_key, rows) - perm[msgs] / (2.0 * p)).max()

    print("largest output phase error: private table %.5f, plain table %.5f (half slot %.4f)" % (worst(out), worst(plain), 1 / (4.0 * p)))
