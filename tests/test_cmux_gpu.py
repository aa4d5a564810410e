"""The CMux on caller TGSW samples, the CMux tree and the extraction of a coefficient on the GPU (csrc/cmux.hip), word for word
against the C reference (ieache_cmux_reference / ieache_lut_tree_reference, which tests/test_cmux_cpu.py holds to the numpy
restatement and to the oracle) and, once per parameter set, against the numpy restatement itself.  All at N = 1024: that is what the
kernel covers.  The bit-exact cases take random full-range words for samples and rows -- no encryption is needed for that; the
end-to-end test runs at the product parameters and asserts the decoding condition only."""
import numpy as np
import pytest

import cmux_reference as CR
import tlwe_reference as TR

pytestmark = pytest.mark.gpu

N = 1024
G = 4  # rows per workgroup of k_cmux_x1 (kCmuxWaveRows, csrc/cmux_plan.h)
SETS = [{}, {"l": 2, "Bgbit": 10}]
IDS = ["l3_Bg7", "l2_Bg10"]

_words = {}


def words(p, n=5, rows=2 * G + 1):
    """per parameter set, made once and left unchanged: n full-range samples, d1 and d0 rows"""
    key = (p.l, p.Bgbit, n, rows)
    if key not in _words:
        rng = np.random.default_rng(9700 + 10 * p.l + p.Bgbit)
        _words[key] = (CR.full_range(rng, (n, 2 * p.l, 2, N)), CR.full_range(rng, (rows, 2, N)), CR.full_range(rng, (rows, 2, N)))
    return _words[key]


@pytest.fixture
def ctx_of(gpu_ctx):
    """gpu_ctx(4, 1024, ...) whose contexts get the piece cap put back afterwards"""
    used = []

    def make(kw, n=4):
        kb, ctx = gpu_ctx(n, N, **kw)
        used.append(ctx)
        return kb, ctx

    yield make
    for ctx in used:
        ctx.set_option("cmux_piece_rows", 8192)


@pytest.mark.parametrize("kw", SETS, ids=IDS)
def test_flat_call_word_for_word(ia, ctx_of, kw):
    """count 1, G-1, G, G+1, 2G+1 (partial workgroups); sets of 1, 2, 5 samples; sel_of None, all the same, all the last, a
    permutation; d0 given and None."""
    from ieache_amd import tools
    kb, ctx = ctx_of(kw)
    p = kb.p
    C, d1, d0 = words(p)
    rng = np.random.default_rng(9701)
    for n in (1, 2, 5):
        with ctx.tgsw_prepare(C[:n]) as S:
            assert S.n == n
            for count in (1, G - 1, G, G + 1, 2 * G + 1):
                sels = [None, np.zeros(count, dtype=np.int32), np.full(count, n - 1, dtype=np.int32), (rng.permutation(count) % n).astype(np.int32)]
                for sel in sels:
                    st = ia.Stats()
                    got = ctx.cmux(S, d1[:count], d0[:count], sel_of=sel, stats=st)
                    assert np.array_equal(got, tools.cmux_reference(p, C[:n], d1[:count], d0[:count], sel_of=sel)), (n, count, sel)
                    assert st.bootstraps == 0 and st.keyswitch_launches == 0 and st.levels == 1 and st.chunks == 1 and st.total_ms > 0
                assert np.array_equal(ctx.cmux(S, d1[:count]), tools.cmux_reference(p, C[:n], d1[:count])), (n, count)
    # once against the numpy restatement itself, and the pieces of a flat call
    with ctx.tgsw_prepare(C) as S:
        want = CR.cmux_rows(C, d1[:G + 1], d0[:G + 1], p.l, p.Bgbit)
        assert np.array_equal(ctx.cmux(S, d1[:G + 1], d0[:G + 1]), want)
        ctx.set_option("cmux_piece_rows", 2)
        st = ia.Stats()
        assert np.array_equal(ctx.cmux(S, d1[:G + 1], d0[:G + 1], stats=st), want) and st.chunks == 3 and st.levels == 1
        assert ctx.cmux_plan(G + 1)["pieces"] == 3
        assert ctx.cmux(S, d1[:0]).shape == (0, 2, N)
    # bk[i] of the context's own key is a sample: the CMux is the oracle's blind-rotation step
    from np_tfhe import _mul_by_xai
    acc = d0[0]
    with ctx.tgsw_prepare(kb.bk) as S:
        for i, a in ((0, 1), (kb.p.n - 1, N), (1, 2 * N - 1)):
            rot = np.stack([_mul_by_xai(acc[c], a) for c in range(2)])
            assert np.array_equal(ctx.cmux(S, rot[None], acc[None], sel_of=[i])[0], kb.ck.blind_rotate_step(acc, i, a)), (i, a)


@pytest.mark.parametrize("kw", SETS, ids=IDS)
def test_digit_extremes_on_the_card(ia, ctx_of, kw):
    """Every digit -2^(Bgbit-1) (d1 - d0 = -offset) and 2^(Bgbit-1) - 1 against samples of -2^31 and 2^31 - 1 throughout: the
    largest sums the two-limb spectrum meets."""
    from ieache_amd import tools
    from test_cmux_cpu import extreme_rows
    from np_tfhe import _wrap32
    kb, ctx = ctx_of(kw)
    p = kb.p
    d1, samples = extreme_rows(N, p.l, p.Bgbit)
    d0 = np.repeat(CR.full_range(np.random.default_rng(9300), (1, 2, N)), 2, axis=0)
    shifted = _wrap32(d1.astype(np.int64) + d0)
    with ctx.tgsw_prepare(samples) as S:
        for s in range(2):
            sel = np.full(2, s, dtype=np.int32)
            assert np.array_equal(ctx.cmux(S, d1, sel_of=sel), CR.cmux_rows(samples, d1, None, p.l, p.Bgbit, sel_of=sel)), s
            assert np.array_equal(ctx.cmux(S, shifted, d0, sel_of=sel), tools.cmux_reference(p, samples, shifted, d0, sel_of=sel)), s


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_device_form_clamps_and_refuses(ia, ctx_of):
    import torch
    from ieache_amd import tools
    kb, ctx = ctx_of({})
    p = kb.p
    C, d1, d0 = words(p)
    count, n = 2 * G + 1, 5
    sel = np.array([0, 4, 5, -1, 7, 2, 1 << 30, -(1 << 31), 3], dtype=np.int32)
    want = tools.cmux_reference(p, C, d1, d0, sel_of=np.clip(sel, 0, n - 1))
    t1, t0, tsel, tout = dev(d1), dev(d0), dev(sel), torch.full((count, 2, N), -1, dtype=torch.int32, device="cuda")
    tC = dev(C)
    torch.cuda.synchronize()
    with ctx.tgsw_prepare_device(tC.data_ptr(), n) as S:
        st = ia.Stats()
        ctx.cmux_device(S, count, tsel.data_ptr(), t1.data_ptr(), t0.data_ptr(), tout.data_ptr(), stats=st)
        assert np.array_equal(tout.cpu().numpy(), want) and st.chunks == 1 and st.bootstraps == 0
        assert np.array_equal(t1.cpu().numpy(), d1) and np.array_equal(t0.cpu().numpy(), d0)
        # no indices, no d0
        tout.fill_(-1)
        torch.cuda.synchronize()
        ctx.cmux_device(S, count, None, t1.data_ptr(), None, tout.data_ptr())
        assert np.array_equal(tout.cpu().numpy(), tools.cmux_reference(p, C, d1))
        # the host form refuses the index the device form clamps
        with pytest.raises(ia.IeacheError, match=r"sel_of\[2\] = 5") as e:
            ctx.cmux(S, d1, d0, sel_of=sel)
        assert e.value.code == -22
        # overlap, every input
        ctx.cmux_device(S, 0, None, t1.data_ptr(), None, t1.data_ptr())
        for args in ((None, t1.data_ptr(), None, t1.data_ptr() + 4 * N), (None, t1.data_ptr(), t0.data_ptr(), t0.data_ptr()),
                     (tsel.data_ptr(), t1.data_ptr(), None, tsel.data_ptr())):
            with pytest.raises(ia.IeacheError, match="overlaps") as e:
                ctx.cmux_device(S, 2, *args)
            assert e.value.code == -22
        with pytest.raises(ia.IeacheError, match="not a device pointer"):
            ctx.cmux_device(S, 2, None, d1.ctypes.data, None, tout.data_ptr())
        ttab = dev(d1[:8])
        for args in ((2, None, ttab.data_ptr(), 2, None, ttab.data_ptr() + 8 * N),):
            with pytest.raises(ia.IeacheError, match="overlaps"):
                ctx.lut_tree_device(S, 1, *args)
        for depth, n_tables, match in ((-1, 1, "depth"), (13, 1, "depth"), (2, 0, "n_tables")):
            with pytest.raises(ia.IeacheError, match=match) as e:
                ctx.lut_tree_device(S, 1, depth, None, ttab.data_ptr(), n_tables, None, tout.data_ptr())
            assert e.value.code == -22


@pytest.mark.parametrize("kw", SETS, ids=IDS)
def test_tree(ia, ctx_of, kw):
    """depth 0, 1, 2, 4 with 1 and 3 items, one table and two with table_of, selectors implied and explicit; then the same calls
    cut into several pieces by a small cap: the same words."""
    from ieache_amd import tools
    kb, ctx = ctx_of(kw)
    p = kb.p
    C, _, _ = words(p)
    rng = np.random.default_rng(9800)
    T = CR.full_range(rng, (2, 16, 2, N))
    with ctx.tgsw_prepare(C) as S:
        for depth in (0, 1, 2, 4):
            tables = T[:, :1 << depth]
            for count in (1, 3):
                sel = rng.integers(0, 5, size=(count, max(depth, 1))).astype(np.int32) if depth else None
                tof = rng.integers(0, 2, size=count).astype(np.int32)
                tof[0] = 1
                cases = [(tables[:1], None, None), (tables, sel, tof), (tables, None, tof)]
                for tb, so, to in cases:
                    want = tools.lut_tree_reference(p, C, tb, depth, sel_of=so, table_of=to, count=count)
                    ctx.set_option("cmux_piece_rows", 8192)
                    st = ia.Stats()
                    got = ctx.lut_tree(S, tb, depth, sel_of=so, table_of=to, count=count, stats=st)
                    assert np.array_equal(got, want), (depth, count)
                    assert st.bootstraps == 0 and st.keyswitch_launches == 0 and st.levels == depth and st.chunks == 1 and st.total_ms > 0
                    # one item per piece; at depth 4 a cap of 3 is below a single item's 8 level-0 rows, which still runs
                    ctx.set_option("cmux_piece_rows", 3 if depth == 4 else 1)
                    st = ia.Stats()
                    assert np.array_equal(ctx.lut_tree(S, tb, depth, sel_of=so, table_of=to, count=count, stats=st), want), (depth, count)
                    assert st.chunks == count and st.levels == depth and ctx.cmux_plan(count, depth)["pieces"] == count
        # once against the numpy restatement itself
        sel = np.array([[4, 0], [1, 3]], dtype=np.int32)
        assert np.array_equal(ctx.lut_tree(S, T[:, :4], 2, sel_of=sel, table_of=[1, 0]), CR.lut_tree(C, T[:, :4], 2, p.l, p.Bgbit, sel_of=sel, table_of=[1, 0], count=2))
        # host-form refusals
        for kwargs, match in ((dict(sel_of=[[0, 5]]), r"sel_of\[1\] = 5"), (dict(table_of=[2]), r"table_of\[0\] = 2")):
            with pytest.raises(ia.IeacheError, match=match) as e:
                ctx.lut_tree(S, T[:, :4], 2, **kwargs)
            assert e.value.code == -22
        assert ctx.lut_tree(S, T[:, :4], 2, count=0).shape == (0, 2, N)


def test_depth_4_tree_is_four_flat_calls_chained_by_hand(ia, ctx_of):
    """The scratch that swaps roles from level to level is not corrupted: 3 items at depth 4 equal level-by-level flat calls on
    host arrays."""
    kb, ctx = ctx_of({})
    C, _, _ = words(kb.p)
    rng = np.random.default_rng(9801)
    depth, count = 4, 3
    T = CR.full_range(rng, (count, 16, 2, N))
    sel = rng.integers(0, 5, size=(count, depth)).astype(np.int32)
    with ctx.tgsw_prepare(C) as S:
        tree = ctx.lut_tree(S, T, depth, sel_of=sel, table_of=np.arange(count))
        rows = T
        for k in range(depth):
            w = rows.shape[1] // 2
            pairs = rows.reshape(count, w, 2, 2, N)
            rows = ctx.cmux(S, pairs[:, :, 1].reshape(-1, 2, N), pairs[:, :, 0].reshape(-1, 2, N), sel_of=np.repeat(sel[:, k], w)).reshape(count, w, 2, N)
        assert np.array_equal(tree, rows[:, 0])


def torus_distance(a, b):
    d = (np.asarray(a, dtype=np.int64) - np.asarray(b, dtype=np.int64)) & 0xFFFFFFFF
    return np.minimum(d, (1 << 32) - d).astype(np.float64) / 2.0 ** 32


def test_end_to_end_at_the_product_parameters(ia, gpu_ctx):
    """A client-encrypted table of 16 polynomials with coefficients +-1/8, four encrypted selector bits per index, depth 4, all 16
    indices in one call: tlwe_phase of the result is the table entry with every coefficient's error below 2^-8 -- a decoding
    condition, not a measurement (scripts/cmux_rates.py records the largest error) -- and tlwe_extract -> keyswitch ->
    decrypt_bits reads a coefficient back as a bit."""
    from ieache_amd import tools
    kb, ctx = gpu_ctx(630, N)
    p = kb.p
    rng = np.random.default_rng(9900)
    bits = rng.integers(0, 2, size=(16, N)).astype(np.uint8)
    m = np.where(bits == 1, 1 << 29, -(1 << 29)).astype(np.int32)
    table = tools.tlwe_encrypt(p, kb.tlwe_key, m, 81)
    # selector k of every index: a fresh encryption of 0 at 2k, of 1 at 2k + 1
    samples = tools.tgsw_encrypt(p, kb.tlwe_key, [0, 1] * 4, 82)
    sel = np.array([[2 * k + ((i >> k) & 1) for k in range(4)] for i in range(16)], dtype=np.int32)
    with ctx.tgsw_prepare(samples) as S:
        out = ctx.lut_tree(S, table, 4, sel_of=sel)
    assert out.shape == (16, 2, N)
    err = torus_distance(tools.tlwe_phase(p, kb.tlwe_key, out), m)
    print("depth-4 tree at the product parameters: largest phase error %.3e (bound 2^-8 = %.3e)" % (err.max(), 2.0 ** -8))
    assert err.max() < 2.0 ** -8
    assert np.array_equal(out, tools.lut_tree_reference(p, samples, table, 4, sel_of=sel))
    # back among the gates: coefficient j of entry i as an LWE bit
    js = (np.arange(16) * 67 + 5) % N
    js[0], js[1] = 0, N - 1
    lwe = ctx.keyswitch(ctx.tlwe_extract(out, coef_of=js))
    assert np.array_equal(kb.dec(lwe), bits[np.arange(16), js])
    assert np.array_equal(ctx.gates(ia.GATE_AND, lwe, lwe).shape, lwe.shape) and np.array_equal(kb.dec(ctx.gates(ia.GATE_AND, lwe, lwe)), bits[np.arange(16), js])


@pytest.mark.parametrize("n,Nr", [(4, 1024), (5, 64)])
def test_tlwe_extract(ia, gpu_ctx, n, Nr):
    """j = 0, 1, N/2 - 1, N/2, N - 1 against numpy, host and device form; any supported ring."""
    import torch
    kb, ctx = gpu_ctx(n, Nr)
    js = np.array([0, 1, Nr // 2 - 1, Nr // 2, Nr - 1], dtype=np.int32)
    acc = CR.full_range(np.random.default_rng(9950 + Nr), (5, 2, Nr))
    want = np.stack([TR.extract_coefficient(acc[r], int(j)) for r, j in enumerate(js)])
    st = ia.Stats()
    assert np.array_equal(ctx.tlwe_extract(acc, coef_of=js, stats=st), want)
    assert st.bootstraps == 0 and st.keyswitch_launches == 0 and st.levels == 1 and st.chunks == 1
    assert np.array_equal(ctx.tlwe_extract(acc), TR.extract_coefficient(acc, 0))
    stride = ctx.extract_stride
    tacc, tj, tu = dev(acc), dev(np.array([0, 1, Nr // 2 - 1, -3, Nr + 7], dtype=np.int32)), torch.full((5, stride), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.tlwe_extract_device(5, tacc.data_ptr(), tj.data_ptr(), tu.data_ptr())
    got = tu.cpu().numpy()
    clamped = np.stack([TR.extract_coefficient(acc[r], j) for r, j in enumerate([0, 1, Nr // 2 - 1, 0, Nr - 1])])
    assert np.array_equal(got[:, :Nr + 1], clamped) and (got[:, Nr + 1:] == -1).all()
    with pytest.raises(ia.IeacheError, match=r"coef_of\[3\]"):
        ctx.tlwe_extract(acc, coef_of=[0, 1, 2, Nr, 0])
    with pytest.raises(ia.IeacheError, match="overlaps"):
        ctx.tlwe_extract_device(5, tacc.data_ptr(), None, tacc.data_ptr() + 64)
    assert ctx.tlwe_extract(acc[:0]).shape == (0, Nr + 1)


def test_warm_calls_allocate_nothing(ia, ctx_of):
    kb, ctx = ctx_of({})
    C, d1, d0 = words(kb.p)
    T = CR.full_range(np.random.default_rng(9960), (2, 4, 2, N))
    sel = np.array([[0, 1], [2, 3], [4, 4]], dtype=np.int32)
    with ctx.tgsw_prepare(C) as S:
        def calls():
            return (ctx.cmux(S, d1, d0, sel_of=np.arange(len(d1)) % 5), ctx.lut_tree(S, T, 2, sel_of=sel, table_of=[0, 1, 1]),
                    ctx.tlwe_extract(d1, coef_of=np.arange(len(d1))))
        first = calls()
        warm = ctx.get_option("staging_allocations")
        again = calls()
        assert ctx.get_option("staging_allocations") == warm
        assert all(np.array_equal(a, b) for a, b in zip(first, again))
    # a gate call afterwards finds its operand rows as it needs them
    bits = np.array([[0, 1, 1], [1, 1, 0]], dtype=np.uint8)
    assert np.array_equal(kb.dec(ctx.gates(ia.GATE_AND, kb.enc(bits[0], 91), kb.enc(bits[1], 92))), bits[0] & bits[1])
    assert not ctx.set_option_ok("cmux_piece_rows", 0) and not ctx.set_option_ok("cmux_piece_rows", (1 << 20) + 1)


def test_set_lifetime_and_ownership(ia, gpu_ctx, make_keys):
    """A set is freed before use (never used), after use, and after the context that made it is closed; another context refuses
    it; a context whose parameter set the kernels do not cover prepares none."""
    from ieache_amd import tools
    kb, ctx = gpu_ctx(4, N)
    C, d1, d0 = words(kb.p)
    want = tools.cmux_reference(kb.p, C, d1[:2], d0[:2])
    ctx.tgsw_prepare(C).close()
    S = ctx.tgsw_prepare(C)
    assert np.array_equal(ctx.cmux(S, d1[:2], d0[:2]), want)
    other = ia.Context.from_arrays(kb.p, kb.bk, kb.ksk)
    mine = other.tgsw_prepare(C[:1])
    for f in (lambda: other.cmux(S, d1[:2]), lambda: ctx.cmux(mine, d1[:2]), lambda: other.lut_tree(S, d1[:2], 1)):
        with pytest.raises(ia.IeacheError, match="another context") as e:
            f()
        assert e.value.code == -22
    assert np.array_equal(other.cmux(mine, d1[:2], d0[:2]), tools.cmux_reference(kb.p, C[:1], d1[:2], d0[:2]))
    other.close()
    mine.close()       # after its context
    mine.close()       # and twice is nothing
    assert np.array_equal(ctx.cmux(S, d1[:2], d0[:2]), want)
    S.close()
    with pytest.raises(ia.IeacheError, match="no samples"):
        ctx.tgsw_prepare(C[:0])
    ks, small = gpu_ctx(5, 64)
    with pytest.raises(ia.IeacheError, match="N = 1024") as e:
        small.tgsw_prepare(np.zeros((1, 6, 2, 64), dtype=np.int32))
    assert e.value.code == -22
