"""The programmable bootstrap on the GPU, word for word against the untouched CPU oracle composed in lut_reference.py
(modswitch -> acc = (0, X^(2N-barb) v) -> blind_rotate -> sample_extract -> keyswitch).  Bit-exact cases take uniformly random
rows -- no encryption is needed for that -- at n = 37 (the 64-lane kernels accept n = 7 .. 129) and on toy rings, so that the
oracle stays affordable; the table test runs at the reference's parameters."""
import numpy as np
import pytest

import lut_reference as LR

pytestmark = pytest.mark.gpu

N = 1024


def random_rows(rng, count, n):
    return rng.integers(-(1 << 31), 1 << 31, size=(count, n + 1), dtype=np.int64).astype(np.int32)


def random_polys(rng, count, ring):
    v = rng.integers(-(1 << 31), 1 << 31, size=(count, ring), dtype=np.int64).astype(np.int32)
    v[0, :4] = [-(1 << 31), (1 << 31) - 1, 0, -1]
    return v


def reference(ck, x, polys, of=None):
    """-> (extracted samples [count][N+1], key-switched samples [count][n+1]) of the composed oracle."""
    u = LR.pbs_reference_rows(ck, x, polys, of, keyswitch=False)
    return u, np.stack([ck.keyswitch(r) for r in u])


_case = {}


def case37(kb):
    """64 random rows at n = 37, three full-range polynomials, a mixed index array, and the oracle's outputs: computed once."""
    if not _case:
        rng = np.random.default_rng(801)
        x, polys = random_rows(rng, 64, 37), random_polys(rng, 3, N)
        of = rng.integers(0, 3, size=64).astype(np.int32)
        of[:3] = [2, 0, 1]
        u, ks = reference(kb.ck, x, polys, of)
        _case.update(x=x, polys=polys, of=of, u=u, ks=ks)
    return _case["x"], _case["polys"], _case["of"], _case["u"], _case["ks"]


def test_w64_prologue_word_for_word(ia, gpu_ctx):
    kb, ctx = gpu_ctx(37, N)
    x, polys, of, u, ks = (a[:40] if len(a) == 64 else a for a in case37(kb))
    assert ctx.extract_stride == N + 4 and "generic" not in ctx.kernel_variant
    st = ia.Stats()
    assert np.array_equal(ctx.pbs(x, polys, of, stats=st), ks)
    assert st.bootstraps == 40 and st.levels == 1 and st.keyswitch_launches >= 1
    st = ia.Stats()
    assert np.array_equal(ctx.pbs(x, polys, of, keyswitch=False, stats=st), u)
    assert st.bootstraps == 40 and st.keyswitch_launches == 0 and st.blind_rotate_launches >= 1
    # one polynomial for every row
    u1, ks1 = reference(kb.ck, x[:8], polys[1:2])
    assert np.array_equal(ctx.pbs(x[:8], polys[1]), ks1) and np.array_equal(ctx.pbs(x[:8], polys[1], keyswitch=False), u1)
    assert np.array_equal(ctx.pbs(x[:1], polys, of[:1]), ks[:1])
    # the constant polynomial is the gate bootstrap: the oracle's own, and the gate path of this library
    mu = np.full(N, 1 << 29, dtype=np.int32)
    assert np.array_equal(ctx.pbs(x[:8], mu), np.stack([kb.ck.bootstrap(r) for r in x[:8]]))
    assert np.array_equal(ctx.pbs(x[:8], mu, keyswitch=False), np.stack([kb.ck.bootstrap_woks(r) for r in x[:8]]))
    a, b = x[:20], x[20:40]
    comb = (a.view(np.uint32) + b.view(np.uint32)).astype(np.uint32)
    comb[:, -1] += np.uint32(0xE0000000)  # bootsAND: (0, -1/8) + ca + cb
    assert np.array_equal(ctx.pbs(comb.view(np.int32), mu), ctx.gates(ia.GATE_AND, a, b))
    # nothing to do
    st = ia.Stats()
    assert ctx.pbs(x[:0], polys, of[:0], stats=st).shape == (0, 38) and st.bootstraps == 0
    assert ctx.pbs(x[:0], polys, keyswitch=False).shape == (0, N + 1)
    with pytest.raises(ia.IeacheError, match="outside"):
        ctx.pbs(x[:2], polys, [0, 3])


@pytest.mark.parametrize("generic", [False, True])
def test_rotation_boundaries_of_the_new_init(ia, gpu_ctx, generic):
    """a = 0: every bara_i is 0, no CMux step runs, and the output is the rotated polynomial itself."""
    kb, ctx = gpu_ctx(37, N)
    barbs = [0, 1, N - 1, N, N + 1, 2 * N - 1]
    x = np.zeros((len(barbs), 38), dtype=np.int32)
    x[:, 37] = LR._wrap32(np.array(barbs, dtype=np.int64) << 21)  # 2N = 2^11 steps
    v = np.arange(1, N + 1, dtype=np.int32)
    want = np.zeros((len(barbs), N + 1), dtype=np.int32)
    want[:, N] = [v[b] if b < N else -v[b - N] for b in barbs]
    u, ks = reference(kb.ck, x, v[None])
    assert np.array_equal(u, want)
    try:
        ctx.force_generic(generic)
        assert ("generic" in ctx.kernel_variant) == generic
        assert np.array_equal(ctx.pbs(x, v, keyswitch=False), want)
        assert np.array_equal(ctx.pbs(x, v), ks)
    finally:
        ctx.force_generic(False)


def test_every_cut_of_a_flat_launch_keeps_the_index_with_its_item(ia, gpu_ctx):
    kb, ctx = gpu_ctx(37, N)
    x, polys, of, u, ks = (a[:13] if len(a) == 64 else a for a in case37(kb))
    uncut, uncut_u = ctx.pbs(x, polys, of), ctx.pbs(x, polys, of, keyswitch=False)
    assert np.array_equal(uncut, ks) and np.array_equal(uncut_u, u)
    saved = {k: ctx.get_option(k) for k in ("chunk", "overlap", "overlap_min")}
    try:
        ctx.set_chunk(5)  # pieces of 5, 5, 3
        st = ia.Stats()
        assert np.array_equal(ctx.pbs(x, polys, of, stats=st), ks) and st.chunks == 3 and st.bootstraps == 13
        assert np.array_equal(ctx.pbs(x, polys, of, keyswitch=False), u)
        ctx.set_option("overlap_min", 2)  # ... alternating between two lanes
        lv = ctx.get_option("overlapped_levels")
        assert np.array_equal(ctx.pbs(x, polys, of), ks) and np.array_equal(ctx.pbs(x, polys, of, keyswitch=False), u)
        assert ctx.get_option("overlapped_levels") == lv + 2
        ctx.set_chunk(saved["chunk"])  # the level's two halves, 8 + 5
        assert np.array_equal(ctx.pbs(x, polys, of), ks) and ctx.get_option("overlapped_levels") == lv + 3
        ctx.set_option("overlap_min", saved["overlap_min"])
        ctx.set_option("overlap", 0)  # one stream
        assert np.array_equal(ctx.pbs(x, polys, of), ks) and np.array_equal(ctx.pbs(x, polys, of, keyswitch=False), u)
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
    rng = np.random.default_rng(810 + ring)
    x, polys = random_rows(rng, 9, n), random_polys(rng, 3, ring)
    of = np.array([0, 1, 2, 2, 1, 0, 1, 1, 2], dtype=np.int32)
    u, ks = reference(kb.ck, x, polys, of)
    assert np.array_equal(ctx.pbs(x, polys, of), ks)
    assert np.array_equal(ctx.pbs(x, polys, of, keyswitch=False), u)
    assert ctx.extract_stride == ring + 4
    chunk = ctx.get_option("chunk")
    try:
        ctx.set_chunk(4)
        assert np.array_equal(ctx.pbs(x, polys, of), ks)
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
    x, polys, of, u, ks = case37(kb)
    saved = {k: ctx.get_option(k) for k in ("exact_fft", "fft_audit")}
    try:
        ctx.set_option("exact_fft", 1)
        assert np.array_equal(ctx.pbs(x[:40], polys, of[:40]), ks[:40])
        assert np.array_equal(ctx.pbs(x[:40], polys, of[:40], keyswitch=False), u[:40])
        ctx.set_option("exact_fft", 0)
        # the output over the input rows: the call cannot be repeated, so it runs on the two-limb kernels from the start
        d_x, d_tv, d_of = device_rows(x[:40], ctx.lwe_stride), torch.from_numpy(polys).cuda(), torch.from_numpy(of[:40]).cuda()
        torch.cuda.synchronize()
        st = ia.Stats()
        ctx.pbs_device(40, d_x.data_ptr(), d_tv.data_ptr(), 3, d_of.data_ptr(), d_x.data_ptr(), stats=st)
        assert np.array_equal(d_x.cpu().numpy()[:, :38], ks[:40]) and st.bootstraps == 40
        assert np.array_equal(d_tv.cpu().numpy(), polys) and np.array_equal(d_of.cpu().numpy(), of[:40])
        # device form without the key switch, no index array: rows of extract_stride
        d_x, d_u = device_rows(x[:8], ctx.lwe_stride), torch.zeros((8, ctx.extract_stride), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.pbs_device(8, d_x.data_ptr(), d_tv[2:].data_ptr(), 1, None, d_u.data_ptr(), keyswitch=False)
        assert np.array_equal(d_u.cpu().numpy()[:, :N + 1], LR.pbs_reference_rows(kb.ck, x[:8], polys[2:], keyswitch=False))
        with pytest.raises(ia.IeacheError, match="overlaps"):
            ctx.pbs_device(8, d_u.data_ptr(), d_tv.data_ptr(), 3, None, d_u.data_ptr(), keyswitch=False)
        with pytest.raises(ia.IeacheError, match="not a device pointer"):
            ctx.pbs_device(8, d_x.data_ptr(), polys.ctypes.data, 3, None, d_u.data_ptr())
        # a guard trip: the whole call is repeated on the two-limb kernels and finds the table again
        _, reruns = ctx.fft_guard()
        ctx.set_option("fft_guard_inject", 1)
        assert np.array_equal(ctx.pbs(x[:40], polys, of[:40]), ks[:40]) and ctx.fft_guard()[1] == reruns + 1
        ctx.set_option("fft_guard_inject", 1)
        assert np.array_equal(ctx.pbs(x[:40], polys, of[:40], keyswitch=False), u[:40]) and ctx.fft_guard()[1] == reruns + 2
        # the sampled audit re-runs 64 items of the launch on the two-limb kernel: same table, same rows
        before = ctx.fft_audit()
        ctx.set_option("fft_audit", 1)
        assert np.array_equal(ctx.pbs(x, polys, of), ks) and np.array_equal(ctx.pbs(x, polys, of, keyswitch=False), u)
        after = ctx.fft_audit()
        assert after["audits"] > before["audits"] and after["gates_compared"] >= before["gates_compared"] + 64
        assert after["mismatches"] == before["mismatches"] == 0
        assert ctx.fft_guard()[1] == reruns + 2
    finally:
        for k, v in saved.items():
            ctx.set_option(k, v)


def test_warm_host_calls_allocate_nothing(ia, gpu_ctx):
    kb, ctx = gpu_ctx(37, N)
    x, polys, of, u, ks = case37(kb)
    for keyswitch, want in ((True, ks), (False, u)):
        assert np.array_equal(ctx.pbs(x, polys, of, keyswitch=keyswitch), want)
        warm = ctx.get_option("staging_allocations")
        assert np.array_equal(ctx.pbs(x, polys, of, keyswitch=keyswitch), want)
        assert np.array_equal(ctx.pbs(x[:7], polys[:2], of[:7] % 2, keyswitch=keyswitch), ctx.pbs(x[:7], polys, of[:7] % 2, keyswitch=keyswitch))
        assert ctx.get_option("staging_allocations") == warm


def test_tables_at_the_product_parameters(ia, gpu_ctx):
    """Four-entry tables at n = 630: 16 fresh encryptions of m / 8, four of each message, through a random permutation table and
    then through the identity table.  Every GPU row is the composed oracle's, and every row decodes to the slot the tables
    dictate -- asserted for the oracle first: zero wrong decodes is the condition for both."""
    from ieache_amd import tools
    kb, ctx = gpu_ctx(630, N)
    p = 4
    rng = np.random.default_rng(820)
    perm = rng.permutation(p)
    while np.array_equal(perm, np.arange(p)):
        perm = rng.permutation(p)
    tables = np.stack([tools.lut_test_poly(kb.p, [LR.message_phase(m, p) for m in t]) for t in (perm, np.arange(p))])
    msgs = np.repeat(np.arange(p), 4)
    x = LR.encrypt_messages(kb.p, kb.lwe_key, msgs, p, rng)

    def decode(rows):
        return np.rint(LR.phases(kb.lwe_key, rows) * 2 * p).astype(np.int64) % (2 * p)

    assert np.array_equal(decode(x), msgs)
    ref1 = LR.pbs_reference_rows(kb.ck, x, tables[0:1])
    ref2 = LR.pbs_reference_rows(kb.ck, ref1, tables[1:2])
    assert np.array_equal(decode(ref1), perm[msgs]) and np.array_equal(decode(ref2), perm[msgs])
    st = ia.Stats()
    out1 = ctx.pbs(x, tables, np.zeros(16, dtype=np.int32), stats=st)
    out2 = ctx.pbs(out1, tables, np.ones(16, dtype=np.int32))
    assert st.bootstraps == 16 and st.keyswitch_launches == 1
    assert np.array_equal(out1, ref1) and np.array_equal(out2, ref2)
    assert np.array_equal(decode(out1), perm[msgs]) and np.array_equal(decode(out2), perm[msgs])
    # how far from the slot centres the outputs came, against the half slot of 1/16 (printed: pytest -s)
    err = np.abs(LR.phases(kb.lwe_key, out2) - perm[msgs] / (2.0 * p))
    print("largest output phase error after two tables: %.4f (half slot %.4f)" % (err.max(), 1 / (4.0 * p)))
