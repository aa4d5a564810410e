"""Many values into shared memories on the GPU (k_demux_acc, csrc/cmux.hip; include/ieache.h section 3j), word for word against
the C reference (ieache_lut_add_reference, which tests/test_lut_add_cpu.py holds to the numpy restatement and to the existing
references composed) and, for the digit extremes, against the numpy restatement itself.  All at N = 1024: that is what the
kernels cover.  The bit-exact cases take random full-range words -- no encryption is needed for that; the last test runs the
two tallies of tests/test_lut_add_cpu.py at the product parameters, word for word and by meaning."""
import numpy as np
import pytest

import cmux_reference as CR
import lut_add_reference as AR
import scatter_reference as SR

pytestmark = pytest.mark.gpu

N = 1024
G = 4  # rows per workgroup of k_demux_acc (kCmuxWaveRows, csrc/cmux_plan.h)
# (key's gadget, set's gadget or None for the key's): the two fixed builds and the run-time build
SETS = [({}, None), ({"l": 2, "Bgbit": 10}, None), ({}, (6, 5))]
IDS = ["l3_Bg7", "l2_Bg10", "l6_Bg5_rt"]

_words = {}


def words(l, Bgbit):
    """per gadget, made once and left unchanged: 5 full-range samples, 9 values, 2 memories of 16 rows"""
    key = (l, Bgbit)
    if key not in _words:
        rng = np.random.default_rng(9850 + 10 * l + Bgbit)
        _words[key] = (CR.full_range(rng, (5, 2 * l, 2, N)), CR.full_range(rng, (9, 2, N)), CR.full_range(rng, (2, 16, 2, N)))
    return _words[key]


def selectors(depth, steps, count, n=5):
    """explicit indices [count][steps + depth] into a set of n, repeats among them; the same for every caller"""
    rng = np.random.default_rng(9860 + 100 * depth + 10 * count + steps)
    sel = rng.integers(0, n, size=(count, max(depth + steps, 1))).astype(np.int32)
    sel[-1, :] = n - 1
    return sel


@pytest.fixture
def ctx_of(gpu_ctx):
    """gpu_ctx(4, 1024, ...) whose contexts get the piece cap put back afterwards"""
    used = []

    def make(kw):
        kb, ctx = gpu_ctx(4, N, **kw)
        used.append(ctx)
        return kb, ctx

    yield make
    for ctx in used:
        ctx.set_option("cmux_piece_rows", 8192)


def prepared(ctx, kb, gadget):
    """(the reference's parameters, the samples, the values, the memories, the prepared set) of a case of SETS"""
    from ieache_amd import tools
    p = kb.p if gadget is None else tools.with_gadget(kb.p, *gadget)
    S, v, mems = words(p.l, p.Bgbit)
    return p, S, v, mems, (ctx.tgsw_prepare(S) if gadget is None else ctx.tgsw_prepare(S, *gadget))


MEM_OF = np.array([1, 0, 1, 1, 0, 0, 1, 0, 1], dtype=np.int32)
# (selectors explicit, mems given, n_mems, mem_of given)
COMBOS = [(False, False, 1, False), (True, True, 2, True), (True, False, 2, True), (False, True, 1, False)]


def combo_args(combo, depth, steps, count, mems):
    explicit, given, n_mems, mof = combo
    return dict(sel_of=selectors(depth, steps, count) if explicit else None, mems=mems[:n_mems, :1 << depth] if given else None, n_mems=n_mems,
                mem_of=MEM_OF[:count] if mof else None)


@pytest.mark.parametrize("kw,gadget", SETS, ids=IDS)
def test_word_for_word(ia, ctx_of, kw, gadget):
    """depth 0, 1, 2, 4 x steps 0, 3 x counts 1, 3, 5 (5 crosses a workgroup of G = 4 rows); one memory and two with mem_of
    mixed, mem_of None; mems given and None; selectors implied and explicit; the stats of section 3j."""
    from ieache_amd import tools
    kb, ctx = ctx_of(kw)
    p, S, v, mems, tg = prepared(ctx, kb, gadget)
    with tg:
        at = 0
        for depth in (0, 1, 2, 4):
            for steps in (0, 3):
                for count in (1, 3, 5):
                    for combo in COMBOS[2 * (at % 2):2 * (at % 2) + 2]:
                        a = combo_args(combo, depth, steps, count, mems)
                        want = tools.lut_add_reference(p, S, v[:count], depth, steps, **a)
                        st = ia.Stats()
                        got = ctx.lut_add(tg, v[:count], depth, steps, stats=st, **a)
                        assert got.shape == (combo[2], 1 << depth, 2, N) and np.array_equal(got, want), (depth, steps, count, combo)
                        assert st.bootstraps == 0 and st.keyswitch_launches == 0 and st.levels == depth + steps and st.chunks == 1 and st.total_ms > 0
                        assert st.blind_rotate_launches == (1 if steps else 0) + max(depth, 1)
                    at += 1
        # explicit amounts, and no items: the memories unchanged, zeros for none
        am = np.array([2047, 0, 5], dtype=np.int32)
        sel = selectors(1, 3, 3)
        assert np.array_equal(ctx.lut_add(tg, v[:3], 1, 3, sel_of=sel, amounts=am, mems=mems[:1, :2]),
                              tools.lut_add_reference(p, S, v[:3], 1, 3, sel_of=sel, amounts=am, mems=mems[:1, :2]))
        assert np.array_equal(ctx.lut_add(tg, v[:0], 2, 1, mems=mems[:2, :4]), mems[:2, :4])
        assert ctx.lut_add(tg, v[:0], 2, 1, n_mems=3).shape == (3, 4, 2, N) and not ctx.lut_add(tg, v[:0], 2, 1, n_mems=3).any()


@pytest.mark.parametrize("kw,gadget", SETS, ids=IDS)
def test_contention_and_repeat(ia, ctx_of, kw, gadget):
    """9 items at depth 1 whose selectors all name the same sample: every item adds into the same two rows.  The words are the
    reference's, and the same call made twice gives identical arrays (integer adds mod 2^32 have no order)."""
    from ieache_amd import tools
    kb, ctx = ctx_of(kw)
    p, S, v, mems, tg = prepared(ctx, kb, gadget)
    sel = np.full((9, 1), 2, dtype=np.int32)
    want = tools.lut_add_reference(p, S, v, 1, 0, sel_of=sel, mems=mems[:1, :2])
    with tg:
        first = ctx.lut_add(tg, v, 1, 0, sel_of=sel, mems=mems[:1, :2])
        again = ctx.lut_add(tg, v, 1, 0, sel_of=sel, mems=mems[:1, :2])
        # depth 0: nine values into one row
        flat = ctx.lut_add(tg, v, 0, 0, mems=mems[:1, :1])
    assert np.array_equal(first, want) and np.array_equal(again, first)
    assert np.array_equal(flat[0, 0], SR._wrap32(v.astype(np.int64).sum(axis=0) + mems[0, 0]))


@pytest.mark.parametrize("kw,gadget", SETS[:2], ids=IDS[:2])
def test_pieces(ia, ctx_of, kw, gadget):
    """One item per piece (cap 1; at depth 4 a cap of 3, below a single item's 8 rows, which still runs): the items of one memory
    are spread over pieces, the words are the same, chunks == count."""
    from ieache_amd import tools
    kb, ctx = ctx_of(kw)
    p, S, v, mems, tg = prepared(ctx, kb, gadget)
    with tg:
        for depth, steps, count in ((0, 0, 3), (1, 3, 5), (2, 0, 3), (4, 3, 3), (0, 3, 3)):
            a = combo_args(COMBOS[1], depth, steps, count, mems)
            want = tools.lut_add_reference(p, S, v[:count], depth, steps, **a)
            ctx.set_option("cmux_piece_rows", 3 if depth == 4 else 1)
            st = ia.Stats()
            got = ctx.lut_add(tg, v[:count], depth, steps, stats=st, **a)
            assert ctx.cmux_plan(count, depth)["pieces"] == count
            ctx.set_option("cmux_piece_rows", 8192)
            assert np.array_equal(got, want), (depth, steps, count)
            assert st.chunks == count and st.levels == depth + steps and st.blind_rotate_launches == count * ((1 if steps else 0) + max(depth, 1))
            assert ctx.cmux_plan(count, depth)["pieces"] == 1


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_device_form_in_place_conservation_clamps_and_refuses(ia, ctx_of):
    import torch
    from ieache_amd import tools
    kb, ctx = ctx_of({})
    p = kb.p
    S, v, mems = words(p.l, p.Bgbit)
    depth, steps, count, n = 2, 3, 5, 5
    sel, mof, m = selectors(depth, steps, count), MEM_OF[:count], mems[:2, :4]
    want = tools.lut_add_reference(p, S, v[:count], depth, steps, sel_of=sel, mems=m, mem_of=mof)
    tS, tv, tsel, tmof, tmem = dev(S), dev(v[:count]), dev(sel), dev(mof), dev(m)
    tout = torch.full((2, 4, 2, N), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with ctx.tgsw_prepare_device(tS.data_ptr(), n) as S5:
        st = ia.Stats()
        ctx.lut_add_device(S5, count, depth, steps, tsel.data_ptr(), None, tv.data_ptr(), tmem.data_ptr(), 2, tmof.data_ptr(), tout.data_ptr(), stats=st)
        got = tout.cpu().numpy()
        assert np.array_equal(got, want) and st.chunks == 1 and st.bootstraps == 0 and st.levels == depth + steps
        assert st.blind_rotate_launches == 1 + depth and np.array_equal(tmem.cpu().numpy(), m)
        # conservation on the card's own output, no reference involved: what memory m gained is the sum of the rotated values
        # sent to it, and those are the card's own rotation
        turned = ctx.tlwe_rotate(S5, v[:count], steps, sel_of=sel[:, :steps], amounts=tools.rotate_amounts(steps, toward_zero=False, N=N))
        gained = SR._wrap32(SR.sub32(got, m).astype(np.int64).sum(axis=1))
        for mm in (0, 1):
            assert np.array_equal(gained[mm], SR._wrap32(turned[mof == mm].astype(np.int64).sum(axis=0))), mm
        # in place: the same words; values and indices as they were
        ctx.lut_add_device(S5, count, depth, steps, tsel.data_ptr(), None, tv.data_ptr(), tmem.data_ptr(), 2, tmof.data_ptr(), tmem.data_ptr())
        assert np.array_equal(tmem.cpu().numpy(), want)
        assert np.array_equal(tv.cpu().numpy(), v[:count]) and np.array_equal(tsel.cpu().numpy(), sel) and np.array_equal(tmof.cpu().numpy(), mof)
        # no memories: zeros, whatever the output held; no items: the memories copied
        tout.fill_(-1)
        torch.cuda.synchronize()
        ctx.lut_add_device(S5, count, depth, steps, tsel.data_ptr(), None, tv.data_ptr(), None, 2, tmof.data_ptr(), tout.data_ptr())
        assert np.array_equal(tout.cpu().numpy(), SR.sub32(want, m))
        tfresh = dev(m)
        torch.cuda.synchronize()
        ctx.lut_add_device(S5, 0, depth, steps, None, None, None, tfresh.data_ptr(), 2, None, tout.data_ptr())
        assert np.array_equal(tout.cpu().numpy(), m)
        # explicit bad indices and memories are clamped on the device, amounts masked; the host form names the first
        bad = sel.copy()
        bad[0, 0], bad[1, 4], bad[2, 2] = 5, -1, 1 << 30
        badm = np.array([2, -1, 1 << 30, 0, 1], dtype=np.int32)
        am = np.array([2048 + 7, -1, 3], dtype=np.int32)
        tbad, tbadm, tam = dev(bad), dev(badm), dev(am)
        torch.cuda.synchronize()
        ctx.lut_add_device(S5, count, depth, steps, tbad.data_ptr(), tam.data_ptr(), tv.data_ptr(), None, 2, tbadm.data_ptr(), tout.data_ptr())
        clamped = tools.lut_add_reference(p, S, v[:count], depth, steps, sel_of=np.clip(bad, 0, n - 1), amounts=am & 2047, n_mems=2, mem_of=np.clip(badm, 0, 1))
        assert np.array_equal(tout.cpu().numpy(), clamped)
        for match, a in ((r"sel_of\[0\] = 5", dict(sel_of=bad)), (r"mem_of\[0\] = 2", dict(sel_of=sel, n_mems=2, mem_of=badm)),
                         (r"amount_of\[0\] = 2055", dict(sel_of=sel, amounts=am))):
            with pytest.raises(ia.IeacheError, match=match) as e:
                ctx.lut_add(S5, v[:count], depth, steps, **a)
            assert e.value.code == -22
        # refusals: a partly overlapping output, the output over the values or the indices, a host pointer, the ranges
        row = 2 * N * 4
        tbig = torch.zeros((3, 4, 2, N), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for args in ((None, None, tv.data_ptr(), tbig.data_ptr(), 2, None, tbig.data_ptr() + row),
                     (None, None, tv.data_ptr(), tbig.data_ptr() + row, 2, None, tbig.data_ptr()),
                     (None, None, tbig.data_ptr() + 2 * row, None, 2, None, tbig.data_ptr()),
                     (tsel.data_ptr(), None, tv.data_ptr(), None, 1, None, tsel.data_ptr()),
                     (None, None, tv.data_ptr(), None, 1, tmof.data_ptr(), tmof.data_ptr())):
            with pytest.raises(ia.IeacheError, match="overlaps") as e:
                ctx.lut_add_device(S5, count, depth, steps, *args)
            assert e.value.code == -22
        with pytest.raises(ia.IeacheError, match="not a device pointer") as e:
            ctx.lut_add_device(S5, count, depth, steps, None, None, v.ctypes.data, None, 2, None, tout.data_ptr())
        assert e.value.code == -22
        for d, s, nm, match in ((-1, 0, 1, "depth"), (13, 0, 1, "depth"), (1, -1, 1, "steps"), (1, 65, 1, "steps"), (1, 0, 0, "n_mems")):
            with pytest.raises(ia.IeacheError, match=match) as e:
                ctx.lut_add_device(S5, 1, d, s, None, None, tv.data_ptr(), None, nm, None, tout.data_ptr())
            assert e.value.code == -22
        # a set of another context
        other = ia.Context.from_arrays(kb.p, kb.bk, kb.ksk)
        try:
            for f in (lambda: other.lut_add(S5, v[:1], 1), lambda: other.lut_add_device(S5, 1, 1, 0, None, None, tv.data_ptr(), None, 1, None, tout.data_ptr())):
                with pytest.raises(ia.IeacheError, match="another context") as e:
                    f()
                assert e.value.code == -22
        finally:
            other.close()
        assert np.array_equal(tout.cpu().numpy(), clamped)  # and no refused call wrote anything


def test_one_item_is_the_scatter_and_depth_0_is_the_rotation(ia, ctx_of):
    """One item with n_mems = 1 and steps = 0 equals Context.lut_scatter bit for bit; steps > 0 with depth 0 equals
    Context.tlwe_rotate plus the memory; and warm calls allocate nothing."""
    from ieache_amd import tools
    kb, ctx = ctx_of({})
    S, v, mems = words(kb.p.l, kb.p.Bgbit)
    with ctx.tgsw_prepare(S) as S5:
        for depth in (0, 1, 2, 4):
            sel = selectors(depth, 0, 1)
            for so in (None, sel):
                assert np.array_equal(ctx.lut_add(S5, v[:1], depth, 0, sel_of=so, mems=mems[:1, :1 << depth]),
                                      ctx.lut_scatter(S5, v[:1], depth, sel_of=so, mem=mems[:1, :1 << depth])), depth
        sel = selectors(0, 3, 3)
        am = tools.rotate_amounts(3, toward_zero=False, N=N)
        turned = ctx.tlwe_rotate(S5, v[:3], 3, sel_of=sel, amounts=am)
        got = ctx.lut_add(S5, v[:3], 0, 3, sel_of=sel, mems=mems[:, :1], mem_of=[1, 0, 1])
        assert np.array_equal(got[0, 0], SR.add32(mems[0, 0], turned[1])) and np.array_equal(got[1, 0], SR.add32(mems[1, 0], SR.add32(turned[0], turned[2])))

        def calls():
            return (ctx.lut_add(S5, v[:3], 2, 3, mems=mems[:2, :4], mem_of=[1, 0, 1]), ctx.lut_add(S5, v[:5], 1, 0), ctx.lut_add(S5, v[:3], 0, 3))
        first = calls()
        warm = ctx.get_option("staging_allocations")
        again = calls()
        assert ctx.get_option("staging_allocations") == warm
        assert all(np.array_equal(a, b) for a, b in zip(first, again))


@pytest.mark.parametrize("kw,gadget", SETS[:2], ids=IDS[:2])
def test_digit_extremes_on_the_card(ia, ctx_of, kw, gadget):
    """Values whose every digit is -2^(Bgbit-1) and 2^(Bgbit-1) - 1 against samples of -2^31 and 2^31 - 1 throughout, two items
    into one memory at depth 2: the largest sums the two-limb spectrum meets, in the first step; against the numpy restatement."""
    from test_cmux_cpu import extreme_rows
    kb, ctx = ctx_of(kw)
    p = kb.p
    values, samples = extreme_rows(N, p.l, p.Bgbit)
    mem = CR.full_range(np.random.default_rng(9870), (1, 4, 2, N))
    with ctx.tgsw_prepare(samples) as S:
        for sel in ([[0, 0], [0, 0]], [[1, 1], [1, 1]], [[0, 1], [1, 0]]):
            want = AR.lut_add(samples, values, 2, 0, p.l, p.Bgbit, sel_of=sel, mems=mem)
            assert np.array_equal(ctx.lut_add(S, values, 2, 0, sel_of=sel, mems=mem), want), sel


@pytest.mark.parametrize("which", ["coefficients", "slots"])
def test_tally_at_the_product_parameters(ia, gpu_ctx, which):
    """n = 630, (3, 7): the scenario of test_lut_add_cpu.tally through Context.lut_add -- five client-encrypted values into a
    memory of client-encrypted zeros, two addresses equal: the memory is the CPU reference's word for word, every coefficient
    of every slot is within 2^-8 of the plaintext tally (the condition derived in tests/test_lut_add_cpu.py), and the phase
    rounds to the tally."""
    from ieache_amd import tools
    from test_lut_add_cpu import tally
    from test_scatter_cpu import torus_distance
    kb, ctx = gpu_ctx(630, N)
    p = kb.p
    sc = tally(p, kb.tlwe_key, which)
    with ctx.tgsw_prepare(sc["samples"]) as S:
        got = ctx.lut_add(S, sc["values"], sc["depth"], sc["steps"], sel_of=sc["sel_of"], mems=sc["mem0"])
    assert got.shape == (1, 1 << sc["depth"], 2, N) and np.array_equal(got, sc["out"])
    phase = tools.tlwe_phase(p, kb.tlwe_key, got[0])
    err = torus_distance(phase, sc["want"])
    print("%s: five additions on the card: largest phase error %.3e (bound 2^-8 = %.3e)" % (which, err.max(), 2.0 ** -8))
    assert err.max() < 2.0 ** -8
    assert np.array_equal(((phase.astype(np.int64) + (1 << 25)) >> 26) & 63, (sc["want"].astype(np.int64) >> 26) & 63)
