"""The write at an encrypted index on the GPU (k_demux_x1, csrc/cmux.hip; include/ieache.h section 3g), word for word against the
C reference (ieache_lut_scatter_reference, which tests/test_scatter_cpu.py holds to the numpy restatement) and, once per
parameter set, against the numpy restatement itself.  All at N = 1024: that is what the kernel covers.  The bit-exact cases take
random full-range words -- no encryption is needed for that; the last test runs three replace writes at the product parameters,
word for word and by meaning."""
import numpy as np
import pytest

import cmux_reference as CR
import scatter_reference as SR

pytestmark = pytest.mark.gpu

N = 1024
G = 4  # rows per workgroup of k_demux_x1 (kCmuxWaveRows, csrc/cmux_plan.h)
SETS = [{}, {"l": 2, "Bgbit": 10}]
IDS = ["l3_Bg7", "l2_Bg10"]

_words = {}
_leaves = {}


def words(p):
    """per parameter set, made once and left unchanged: 5 full-range samples, 5 values, 5 memories of 16 rows"""
    key = (p.l, p.Bgbit)
    if key not in _words:
        rng = np.random.default_rng(9750 + 10 * p.l + p.Bgbit)
        _words[key] = (CR.full_range(rng, (5, 2 * p.l, 2, N)), CR.full_range(rng, (5, 2, N)), CR.full_range(rng, (5, 16, 2, N)))
    return _words[key]


def selectors(depth, count, n):
    """explicit indices [count][depth] into a set of n, repeats among them; the same for every caller"""
    rng = np.random.default_rng(9760 + 100 * depth + 10 * count + n)
    sel = rng.integers(0, n, size=(count, max(depth, 1))).astype(np.int32)
    sel[-1, :] = n - 1
    return sel


def leaves(p, n, depth, count, explicit):
    """(sel_of or None, the C reference's leaves [count][2^depth][2][N]) of the first `count` values on the first n samples:
    computed once, shared by the tests below.  With a memory the definition adds it: out = mem + leaves."""
    from ieache_amd import tools
    key = (p.l, p.Bgbit, n, depth, count, explicit)
    if key not in _leaves:
        S, v, _ = words(p)
        sel = selectors(depth, count, n) if explicit else None
        _leaves[key] = (sel, tools.lut_scatter_reference(p, S[:n], v[:count], depth, sel_of=sel))
    return _leaves[key]


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


# (n samples, depth, count, explicit selectors): steps of 1, 2, 3, 4, 5, 6, 8, 12, 24 parents through workgroups of G = 4
CASES = ([(5, d, c, e) for d, c in ((0, 1), (0, 3), (1, 1), (1, 3), (1, 5), (2, 1), (2, 3)) for e in (False, True)] +
         [(5, 4, 1, False), (5, 4, 3, True), (1, 1, 5, False), (1, 2, 3, False)])


@pytest.mark.parametrize("kw", SETS, ids=IDS)
def test_word_for_word(ia, ctx_of, kw):
    """depth 0, 1, 2, 4 with 1 and 3 items and 5 at depth 1; sets of 1 and 5 samples; selectors implied and explicit; mem given
    and None; the stats of section 3g."""
    kb, ctx = ctx_of(kw)
    p = kb.p
    S, v, mem = words(p)
    with ctx.tgsw_prepare(S) as S5, ctx.tgsw_prepare(S[:1]) as S1:
        for n, depth, count, explicit in CASES:
            sel, want = leaves(p, n, depth, count, explicit)
            tg = S5 if n == 5 else S1
            st = ia.Stats()
            got = ctx.lut_scatter(tg, v[:count], depth, sel_of=sel, stats=st)
            assert got.shape == (count, 1 << depth, 2, N) and np.array_equal(got, want), (n, depth, count, explicit)
            assert st.bootstraps == 0 and st.keyswitch_launches == 0 and st.levels == depth and st.chunks == 1 and st.total_ms > 0
            assert st.blind_rotate_launches == max(depth, 1)
            m = mem[:count, :1 << depth]
            st = ia.Stats()
            got = ctx.lut_scatter(tg, v[:count], depth, sel_of=sel, mem=m, count=count, stats=st)
            assert np.array_equal(got, SR.add32(m, want)), (n, depth, count, explicit)
            assert st.levels == depth and st.chunks == 1 and st.blind_rotate_launches == max(depth, 1)
        # once against the numpy restatement itself
        sel = np.array([[4, 0], [1, 3]], dtype=np.int32)
        assert np.array_equal(ctx.lut_scatter(S5, v[:2], 2, sel_of=sel, mem=mem[:2, :4]), SR.lut_scatter(S, v[:2], 2, p.l, p.Bgbit, sel_of=sel, mem=mem[:2, :4]))
        assert ctx.lut_scatter(S5, v[:0], 2).shape == (0, 4, 2, N)


@pytest.mark.parametrize("kw", SETS, ids=IDS)
def test_pieces(ia, ctx_of, kw):
    """One item per piece (cap 1; at depth 4 a cap of 3, below a single item's 8 rows, which still runs): the same words,
    chunks == count, and the plan of a scatter is the tree's."""
    kb, ctx = ctx_of(kw)
    p = kb.p
    S, v, mem = words(p)
    with ctx.tgsw_prepare(S) as S5:
        for depth, count, explicit in ((0, 3, True), (1, 5, True), (2, 3, True), (4, 3, True), (1, 3, False)):
            sel, want = leaves(p, 5, depth, count, explicit)
            m = mem[:count, :1 << depth]
            ctx.set_option("cmux_piece_rows", 3 if depth == 4 else 1)
            for mm, ww in ((None, want), (m, SR.add32(m, want))):
                st = ia.Stats()
                assert np.array_equal(ctx.lut_scatter(S5, v[:count], depth, sel_of=sel, mem=mm, stats=st), ww), (depth, count)
                assert st.chunks == count and st.levels == depth and st.blind_rotate_launches == count * max(depth, 1)
            assert ctx.cmux_plan(count, depth)["pieces"] == count
            ctx.set_option("cmux_piece_rows", 8192)
            assert ctx.cmux_plan(count, depth)["pieces"] == 1


@pytest.mark.parametrize("kw", SETS, ids=IDS)
def test_digit_extremes_on_the_card(ia, ctx_of, kw):
    """Values whose every digit is -2^(Bgbit-1) and 2^(Bgbit-1) - 1 against samples of -2^31 and 2^31 - 1 throughout, depth 2: the
    largest sums the two-limb spectrum meets, in the first step; against the numpy restatement."""
    from test_cmux_cpu import extreme_rows
    kb, ctx = ctx_of(kw)
    p = kb.p
    values, samples = extreme_rows(N, p.l, p.Bgbit)
    mem = CR.full_range(np.random.default_rng(9770), (2, 4, 2, N))
    with ctx.tgsw_prepare(samples) as S:
        for sel in ([[0, 0], [0, 0]], [[1, 1], [1, 1]], [[0, 1], [1, 0]]):
            want = SR.lut_scatter(samples, values, 2, p.l, p.Bgbit, sel_of=sel)
            assert np.array_equal(ctx.lut_scatter(S, values, 2, sel_of=sel), want), sel
            assert np.array_equal(ctx.lut_scatter(S, values, 2, sel_of=sel, mem=mem), SR.add32(mem, want)), sel


def test_depth_4_scatter_is_four_steps_chained_by_hand(ia, ctx_of):
    """The scratch that swaps roles from step to step is not corrupted: 3 items at depth 4 equal the steps done with the flat
    external product Context.cmux(S, p, None, sel_of=...) and host subtraction."""
    kb, ctx = ctx_of({})
    S, v, mem = words(kb.p)
    depth, count = 4, 3
    sel = selectors(depth, count, 5)
    with ctx.tgsw_prepare(S) as S5:
        got = ctx.lut_scatter(S5, v[:count], depth, sel_of=sel, mem=mem[:count])
        rows = v[:count, None]                                   # [count][w][2][N]
        for t in range(depth):
            w = rows.shape[1]
            hi = ctx.cmux(S5, rows.reshape(-1, 2, N), None, sel_of=np.repeat(sel[:, depth - 1 - t], w)).reshape(count, w, 2, N)
            rows = np.stack([SR.sub32(rows, hi), hi], axis=2).reshape(count, 2 * w, 2, N)
        assert np.array_equal(got, SR.add32(mem[:count], rows))
    assert np.array_equal(got, SR.add32(mem[:count], leaves(kb.p, 5, depth, count, True)[1]))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_device_form_in_place_clamps_and_refuses(ia, ctx_of):
    import torch
    from ieache_amd import tools
    kb, ctx = ctx_of({})
    p = kb.p
    S, v, mem = words(p)
    depth, count, n = 2, 3, 5
    sel, lv = leaves(p, n, depth, count, True)
    m = mem[:count, :4]
    want = SR.add32(m, lv)
    tS, tv, tsel, tmem = dev(S), dev(v[:count]), dev(sel), dev(m)
    tout = torch.full((count, 4, 2, N), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with ctx.tgsw_prepare_device(tS.data_ptr(), n) as S5:
        st = ia.Stats()
        ctx.lut_scatter_device(S5, count, depth, tsel.data_ptr(), tv.data_ptr(), tmem.data_ptr(), tout.data_ptr(), stats=st)
        assert np.array_equal(tout.cpu().numpy(), want) and st.chunks == 1 and st.bootstraps == 0 and st.levels == depth
        assert np.array_equal(tmem.cpu().numpy(), m)
        # in place: the same words; values and indices as they were
        ctx.lut_scatter_device(S5, count, depth, tsel.data_ptr(), tv.data_ptr(), tmem.data_ptr(), tmem.data_ptr())
        assert np.array_equal(tmem.cpu().numpy(), want)
        assert np.array_equal(tv.cpu().numpy(), v[:count]) and np.array_equal(tsel.cpu().numpy(), sel)
        # in place at depth 0 and depth 1, no indices
        for d in (0, 1):
            tm = dev(mem[:count, :1 << d])
            torch.cuda.synchronize()
            ctx.lut_scatter_device(S5, count, d, None, tv.data_ptr(), tm.data_ptr(), tm.data_ptr())
            assert np.array_equal(tm.cpu().numpy(), SR.add32(mem[:count, :1 << d], leaves(p, n, d, count, False)[1])), d
        # no memory: the leaves
        tout.fill_(-1)
        torch.cuda.synchronize()
        ctx.lut_scatter_device(S5, count, depth, tsel.data_ptr(), tv.data_ptr(), None, tout.data_ptr())
        assert np.array_equal(tout.cpu().numpy(), lv)
        # explicit bad indices are clamped on the device; the host form names the first
        bad = np.array([[0, 5], [-1, 7], [1 << 30, -(1 << 31)]], dtype=np.int32)
        tbad = dev(bad)
        torch.cuda.synchronize()
        ctx.lut_scatter_device(S5, count, depth, tbad.data_ptr(), tv.data_ptr(), None, tout.data_ptr())
        clamped = tools.lut_scatter_reference(p, S, v[:count], depth, sel_of=np.clip(bad, 0, n - 1))
        assert np.array_equal(tout.cpu().numpy(), clamped)
        with pytest.raises(ia.IeacheError, match=r"sel_of\[1\] = 5") as e:
            ctx.lut_scatter(S5, v[:count], depth, sel_of=bad)
        assert e.value.code == -22
        # refusals: partial overlap with the memory, the output over the values or the indices, a host pointer, the depth
        row = 2 * N * 4
        tbig = torch.zeros((count + 1, 4, 2, N), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.lut_scatter_device(S5, 0, depth, None, tv.data_ptr(), None, tv.data_ptr())
        for args in ((None, tv.data_ptr(), tbig.data_ptr(), tbig.data_ptr() + row),
                     (None, tv.data_ptr(), tbig.data_ptr() + row, tbig.data_ptr()),
                     (None, tv.data_ptr(), None, tv.data_ptr()),
                     (None, tbig.data_ptr() + 5 * row, None, tbig.data_ptr()),
                     (tsel.data_ptr(), tv.data_ptr(), None, tsel.data_ptr())):
            with pytest.raises(ia.IeacheError, match="overlaps") as e:
                ctx.lut_scatter_device(S5, count, depth, *args)
            assert e.value.code == -22
        with pytest.raises(ia.IeacheError, match="not a device pointer") as e:
            ctx.lut_scatter_device(S5, count, depth, None, v.ctypes.data, None, tout.data_ptr())
        assert e.value.code == -22
        for d in (-1, 13):
            with pytest.raises(ia.IeacheError, match="depth") as e:
                ctx.lut_scatter_device(S5, 1, d, None, tv.data_ptr(), None, tout.data_ptr())
            assert e.value.code == -22
        with pytest.raises(ia.IeacheError, match="depth"):
            ctx.lut_scatter(S5, v[:1], 13)
        # a set of another context
        other = ia.Context.from_arrays(kb.p, kb.bk, kb.ksk)
        try:
            for f in (lambda: other.lut_scatter(S5, v[:1], 1), lambda: other.lut_scatter_device(S5, 1, 1, None, tv.data_ptr(), None, tout.data_ptr()),
                      lambda: other.lut_write(S5, mem[:1, :2], 1, v[:1])):
                with pytest.raises(ia.IeacheError, match="another context") as e:
                    f()
                assert e.value.code == -22
        finally:
            other.close()
        assert np.array_equal(tout.cpu().numpy(), clamped)  # and no refused call wrote anything


def test_warm_calls_allocate_nothing(ia, ctx_of):
    kb, ctx = ctx_of({})
    S, v, mem = words(kb.p)
    sel = selectors(2, 3, 5)
    with ctx.tgsw_prepare(S) as S5:
        def calls():
            return (ctx.lut_scatter(S5, v[:3], 2, sel_of=sel, mem=mem[:3, :4]), ctx.lut_scatter(S5, v[:3], 2, sel_of=sel),
                    ctx.lut_write(S5, mem[:3, :4], 2, v[:3], sel_of=sel))
        first = calls()
        warm = ctx.get_option("staging_allocations")
        again = calls()
        assert ctx.get_option("staging_allocations") == warm
        assert all(np.array_equal(a, b) for a, b in zip(first, again))
        # lut_write is the read, the subtraction and the scatter
        from ieache_amd import tools
        old = tools.lut_tree_reference(kb.p, S, mem[:3, :4], 2, sel_of=sel, table_of=np.arange(3))
        assert np.array_equal(first[2], tools.lut_scatter_reference(kb.p, S, SR.sub32(v[:3], old), 2, sel_of=sel, mem=mem[:3, :4]))
    # a gate call afterwards finds its operand rows as it needs them
    bits = np.array([[0, 1, 1], [1, 1, 0]], dtype=np.uint8)
    assert np.array_equal(kb.dec(ctx.gates(ia.GATE_AND, kb.enc(bits[0], 91), kb.enc(bits[1], 92))), bits[0] & bits[1])


def test_three_replace_writes_at_the_product_parameters(ia, gpu_ctx):
    """n = 630, (3, 7): the sequence of test_scatter_cpu.three_writes (addresses 3, 12, 3, fresh selectors each time) through
    Context.lut_write: the memory after each write is the CPU reference's word for word and every coefficient of every slot
    is within 2^-8 of what the slot should hold (a decoding condition; scripts/scatter_rates.py records the largest error).  Then
    lut_tree -> tlwe_extract -> keyswitch -> decrypt reads back bits of the slot written twice and of an untouched one."""
    from ieache_amd import tools
    from test_scatter_cpu import three_writes, torus_distance
    kb, ctx = gpu_ctx(630, N)
    p = kb.p
    seq = three_writes(p, kb.tlwe_key)
    mem = seq["mem0"]
    worst = 0.0
    for w, (samples, sel, new) in enumerate(seq["steps"]):
        with ctx.tgsw_prepare(samples) as S:
            mem = ctx.lut_write(S, mem, 4, new, sel_of=sel)
        assert mem.shape == (1, 16, 2, N) and np.array_equal(mem, seq["mems"][w]), w
        err = torus_distance(tools.tlwe_phase(p, kb.tlwe_key, mem[0]), seq["want"][w])
        worst = max(worst, err.max())
        assert err.max() < 2.0 ** -8, w
    print("three depth-4 replace writes at the product parameters: largest phase error %.3e (bound 2^-8 = %.3e)" % (worst, 2.0 ** -8))
    # back among the gates: slot 3 (written twice) and slot 5 (untouched), 8 coefficients each
    read = tools.tgsw_encrypt(p, kb.tlwe_key, [(a >> k) & 1 for a in (3, 5) for k in range(4)], 201)
    js = np.array([0, N - 1, 5, 72, 139, 206, 273, 340], dtype=np.int32)
    with ctx.tgsw_prepare(read) as S:
        got = ctx.lut_tree(S, mem, 4, sel_of=np.repeat(np.arange(8, dtype=np.int32).reshape(2, 4), 8, axis=0), table_of=np.zeros(16, dtype=np.int32))
    lwe = ctx.keyswitch(ctx.tlwe_extract(got, coef_of=np.tile(js, 2)))
    final = seq["want"][-1]
    assert np.array_equal(kb.dec(lwe), np.concatenate([final[3, js] > 0, final[5, js] > 0]).astype(np.uint8))
    assert np.array_equal(final[5], seq["msg0"][5]) and not np.array_equal(final[3], seq["msg0"][3])
