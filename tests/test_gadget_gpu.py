"""TGSW sets with a gadget of their own and the replace write on the GPU (include/ieache.h section 3i; k_cmux_rt / k_demux_rt in
csrc/cmux.hip, k_rotate_rt in csrc/rotate.hip, which take (l, Bgbit) as launch arguments).  Word for word against the C references
with tools.with_gadget parameters (which tests/test_gadget_cpu.py holds to the numpy restatements at these gadgets) on every row
and item, and against the numpy restatements directly on one row or item of each operation (a product of theirs at l = 32 is 128
convolutions).  Shapes: 9 rows -- two
full workgroups of G = 4 rows and a ragged one -- and sets of 5 samples, explicit and implied selectors, full-range words made
once per gadget.  The last test runs the twelve worst-case replace writes of gadget_sequence.py on one memory kept on the card."""
import numpy as np
import pytest

import cmux_reference as CR
import gadget_sequence as GS
import rotate_reference as RR
import scatter_reference as SR

pytestmark = pytest.mark.gpu

N = GS.N
G = 4
ROWS = 2 * G + 1
# the build that shipped takes (l, Bgbit) as launch arguments: every admissible gadget runs
GADGETS = GS.TABLE + GS.RUNTIME_ONLY
IDS = ["l%d_Bg%d" % g for g in GADGETS]

_words = {}


def words(l, Bgbit):
    """per gadget, made once and left unchanged: 5 full-range samples [2l][2][N], 9 rows d1 and d0, 3 memories of 16 rows"""
    if (l, Bgbit) not in _words:
        rng = np.random.default_rng(9850 + 100 * l + Bgbit)
        _words[l, Bgbit] = (CR.full_range(rng, (5, 2 * l, 2, N)), CR.full_range(rng, (ROWS, 2, N)), CR.full_range(rng, (ROWS, 2, N)),
                            CR.full_range(rng, (3, 16, 2, N)))
    return _words[l, Bgbit]


def selectors(shape):
    rng = np.random.default_rng(9860 + 10 * shape[0] + shape[1])
    sel = rng.integers(0, 5, size=shape).astype(np.int32)
    sel[-1, :] = 4
    return sel


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture
def ctx_of(gpu_ctx):
    """gpu_ctx(4, 1024, ...) whose contexts get their options put back afterwards"""
    used = []

    def make(kw=None, n=4):
        kb, ctx = gpu_ctx(n, N, **(kw or {}))
        used.append(ctx)
        return kb, ctx

    yield make
    for ctx in used:
        ctx.set_option("cmux_piece_rows", 8192)
        ctx.set_option("cmux_gadget_runtime", 0)


@pytest.mark.parametrize("l,Bgbit", GADGETS, ids=IDS)
def test_every_operation_word_for_word(ia, ctx_of, l, Bgbit):
    """cmux with and without d0, lut_tree of depth 3 with 3 items sharing 2 tables, lut_scatter of depth 3 in place on the device,
    tlwe_rotate of 3 steps with per-row selectors in place, lut_read of depth 1 + 2 steps with the key switch."""
    import torch
    from ieache_amd import tools
    kb, ctx = ctx_of()
    pg = tools.with_gadget(kb.p, l, Bgbit)
    S, d1, d0, mem = words(l, Bgbit)
    with ctx.tgsw_prepare(S, l, Bgbit) as S5:
        assert (S5.l, S5.Bgbit, S5.n) == (l, Bgbit, 5)
        # flat: explicit selectors with d0, implied without
        sel = selectors((ROWS, 1)).reshape(-1)
        st = ia.Stats()
        got = ctx.cmux(S5, d1, d0, sel_of=sel, stats=st)
        assert np.array_equal(got, tools.cmux_reference(pg, S, d1, d0, sel_of=sel))
        assert st.chunks == 1 and st.levels == 1 and st.bootstraps == 0 and st.blind_rotate_launches == 1
        got0 = ctx.cmux(S5, d1)
        assert np.array_equal(got0, tools.cmux_reference(pg, S, d1))
        # ... the last row (the ragged workgroup) against the numpy restatement itself
        assert np.array_equal(got[-1:], CR.cmux_rows(S, d1[-1:], d0[-1:], l, Bgbit, sel_of=sel[-1:]))
        assert np.array_equal(got0[:1], CR.cmux_rows(S, d1[:1], None, l, Bgbit))
        # tree: 3 items over 2 tables
        sel3 = selectors((3, 3))
        tables, tof = mem[:2, :8], np.array([1, 0, 1], dtype=np.int32)
        assert np.array_equal(ctx.lut_tree(S5, tables, 3, sel_of=sel3, table_of=tof), tools.lut_tree_reference(pg, S, tables, 3, sel_of=sel3, table_of=tof))
        assert np.array_equal(ctx.lut_tree(S5, tables, 3, table_of=tof), tools.lut_tree_reference(pg, S, tables, 3, table_of=tof))
        assert np.array_equal(ctx.lut_tree(S5, tables, 3, sel_of=sel3[:1], table_of=tof[:1]), CR.lut_tree(S, tables, 3, l, Bgbit, sel_of=sel3[:1], table_of=tof[:1]))
        # scatter: in place on the device
        m = mem[:, :8]
        tv, tsel, tm = dev(d1[:3]), dev(sel3), dev(m)
        torch.cuda.synchronize()
        ctx.lut_scatter_device(S5, 3, 3, tsel.data_ptr(), tv.data_ptr(), tm.data_ptr(), tm.data_ptr())
        assert np.array_equal(tm.cpu().numpy(), tools.lut_scatter_reference(pg, S, d1[:3], 3, sel_of=sel3, mem=m))
        assert np.array_equal(ctx.lut_scatter(S5, d1[:3], 3), tools.lut_scatter_reference(pg, S, d1[:3], 3))
        assert np.array_equal(tm.cpu().numpy()[2:], SR.lut_scatter(S, d1[2:3], 3, l, Bgbit, sel_of=sel3[2:], mem=m[2:]))
        # rotation: 9 rows, 3 steps, per-row selectors, in place
        selr = selectors((ROWS, 3))
        tr, tselr = dev(d0), dev(selr)
        torch.cuda.synchronize()
        ctx.tlwe_rotate_device(S5, ROWS, 3, tselr.data_ptr(), None, tr.data_ptr(), tr.data_ptr())
        assert np.array_equal(tr.cpu().numpy(), tools.tlwe_rotate_reference(pg, S, d0, 3, sel_of=selr))
        assert np.array_equal(tr.cpu().numpy()[-1:], RR.tlwe_rotate(S, d0[-1:], 3, l, Bgbit, sel_of=selr[-1:]))
        assert np.array_equal(ctx.tlwe_rotate(S5, d0[:5], 3, amounts=[7, 0, 2047]), tools.tlwe_rotate_reference(pg, S, d0[:5], 3, amounts=[7, 0, 2047]))
        # lookup below the sample, through the key switch
        want = tools.lut_read_reference(pg, S, mem[:2, :2], 1, 2, sel_of=sel3, table_of=tof, ksk=kb.ksk)
        assert np.array_equal(ctx.lut_read(S5, mem[:2, :2], 1, 2, sel_of=sel3, table_of=tof), want)
        assert np.array_equal(ctx.lut_read(S5, mem[:2, :2], 1, 2, sel_of=sel3[:1], table_of=tof[:1], keyswitch=False),
                              RR.lut_read(S, mem[:2, :2], 1, 2, l, Bgbit, sel_of=sel3[:1], table_of=tof[:1]))

        # warm: every call of the family again on this set allocates nothing and gives the same words
        def calls():
            return (ctx.cmux(S5, d1, d0, sel_of=sel), ctx.lut_tree(S5, tables, 3, sel_of=sel3, table_of=tof), ctx.lut_scatter(S5, d1[:3], 3, sel_of=sel3, mem=m),
                    ctx.tlwe_rotate(S5, d0, 3, sel_of=selr), ctx.lut_read(S5, mem[:2, :2], 1, 2, sel_of=sel3, table_of=tof),
                    ctx.lut_write(S5, m, 3, d1[:3], sel_of=sel3))
        first = calls()
        warm = ctx.get_option("staging_allocations")
        again = calls()
        assert ctx.get_option("staging_allocations") == warm
        assert all(np.array_equal(a, b) for a, b in zip(first, again))
        assert np.array_equal(first[0], got) and np.array_equal(first[4], want)


@pytest.mark.parametrize("l,Bgbit", GADGETS, ids=IDS)
def test_digit_extremes_on_the_card(ia, ctx_of, l, Bgbit):
    """Every digit -2^(Bgbit-1) and 2^(Bgbit-1) - 1 (CR.all_digits_word, through test_cmux_cpu.extreme_rows) and the all-ones word
    against samples of -2^31 and 2^31 - 1 throughout: the largest sums the two-limb spectrum meets at this gadget, in the flat
    product, the first step of a scatter and a rotation step."""
    from ieache_amd import tools
    from test_cmux_cpu import extreme_rows
    kb, ctx = ctx_of()
    pg = tools.with_gadget(kb.p, l, Bgbit)
    d1, samples = extreme_rows(N, l, Bgbit)
    d1 = np.concatenate([d1, np.full((1, 2, N), -1, dtype=np.int32)])
    d0 = np.repeat(CR.full_range(np.random.default_rng(9870), (1, 2, N)), 3, axis=0)
    shifted = SR.add32(d1, d0)
    with ctx.tgsw_prepare(samples, l, Bgbit) as S:
        for s in range(2):
            sel = np.full(3, s, dtype=np.int32)
            assert np.array_equal(ctx.cmux(S, d1, sel_of=sel), tools.cmux_reference(pg, samples, d1, sel_of=sel)), s
            assert np.array_equal(ctx.cmux(S, shifted, d0, sel_of=sel), tools.cmux_reference(pg, samples, shifted, d0, sel_of=sel)), s
            sel2 = np.full((3, 2), s, dtype=np.int32)
            assert np.array_equal(ctx.lut_scatter(S, d1, 2, sel_of=sel2), tools.lut_scatter_reference(pg, samples, d1, 2, sel_of=sel2)), s
            assert np.array_equal(ctx.tlwe_rotate(S, d1, 2, sel_of=sel2), tools.tlwe_rotate_reference(pg, samples, d1, 2, sel_of=sel2)), s
        assert np.array_equal(ctx.cmux(S, d1[:1], sel_of=[1]), CR.cmux_rows(samples, d1[:1], None, l, Bgbit, sel_of=[1]))


def test_the_contexts_own_gadget_and_the_other_keys(ia, ctx_of):
    """prepare_gadget at the context's own gadget is prepare: the same words from the shipped builds, and from the run-time
    build under the debug option.  A (6, 5) set works on a context whose key is (2, 10), and so does the key's own."""
    from ieache_amd import tools
    for kw in ({}, {"l": 2, "Bgbit": 10}):
        kb, ctx = ctx_of(kw)
        p = kb.p
        S, d1, d0, mem = words(p.l, p.Bgbit)
        sel3 = selectors((3, 3))
        with ctx.tgsw_prepare(S) as A, ctx.tgsw_prepare(S, p.l, p.Bgbit) as B:
            assert (A.l, A.Bgbit) == (B.l, B.Bgbit) == (p.l, p.Bgbit)

            def calls(T):
                return (ctx.cmux(T, d1, d0), ctx.lut_tree(T, mem[:1, :8], 3, sel_of=sel3), ctx.lut_scatter(T, d1[:3], 3, sel_of=sel3, mem=mem[:, :8]),
                        ctx.tlwe_rotate(T, d0, 3), ctx.lut_write(T, mem[:, :8], 3, d1[:3], sel_of=sel3))
            want = calls(A)
            assert np.array_equal(want[0], tools.cmux_reference(p, S, d1, d0))
            assert np.array_equal(want[4], tools.lut_write_reference(p, S, mem[:, :8], 3, d1[:3], sel_of=sel3))
            assert all(np.array_equal(a, b) for a, b in zip(want, calls(B)))
            ctx.set_option("cmux_gadget_runtime", 1)
            assert all(np.array_equal(a, b) for a, b in zip(want, calls(A)))
            ctx.set_option("cmux_gadget_runtime", 0)
        if p.l == 2:
            S65, e1, e0, _ = words(6, 5)
            with ctx.tgsw_prepare(S65, 6, 5) as T:
                assert np.array_equal(ctx.cmux(T, e1, e0), tools.cmux_reference(tools.with_gadget(p, 6, 5), S65, e1, e0))


def test_refusals(ia, ctx_of, gpu_ctx):
    kb, ctx = ctx_of()
    S, d1, d0, mem = words(6, 5)
    z = lambda l: np.zeros((1, 2 * l, 2, N), dtype=np.int32)
    for l, Bgbit, match in ((3, 11, "l x Bgbit"), (11, 3, "l x Bgbit"), (1, 22, r"2\^32"), (1, 32, "Bgbit must lie"), (4, 0, "Bgbit must lie")):
        with pytest.raises(ia.IeacheError, match=match) as e:
            ctx.tgsw_prepare(z(l), l, Bgbit)
        assert e.value.code == -22, (l, Bgbit)
    # l = 0: there is no sample array of 0 rows to pass through the wrapper; the library names the rule
    from ieache_amd.evaluator import _i32
    assert not ia.lib().ieache_tgsw_prepare_gadget(ctx.h, _i32(z(1)), 1, 0, 7)
    assert "l must be at least 1" in ia.lib().ieache_last_error().decode()
    assert not ia.lib().ieache_tgsw_prepare_gadget_device(ctx.h, dev(z(1)).data_ptr(), 1, 0, 7)
    assert "l must be at least 1" in ia.lib().ieache_last_error().decode()
    with pytest.raises(ia.IeacheError, match="no samples"):
        ctx.tgsw_prepare(S[:0], 6, 5)
    # the wrapper: rows that are no whole number of samples of 2l rows; one of l, Bgbit alone
    with pytest.raises(ValueError, match="2l = 12"):
        ctx.tgsw_prepare(np.zeros((1, 8, 2, N), dtype=np.int32), 6, 5)
    with pytest.raises(ValueError, match="both"):
        ctx.tgsw_prepare(S, l=6)
    # a 64-coefficient ring
    ks, small = gpu_ctx(5, 64)
    with pytest.raises(ia.IeacheError, match="N = 1024") as e:
        small.tgsw_prepare(np.zeros((1, 12, 2, 64), dtype=np.int32), 6, 5)
    assert e.value.code == -22
    # a set used on another context
    other = ia.Context.from_arrays(kb.p, kb.bk, kb.ksk)
    try:
        with ctx.tgsw_prepare(S, 6, 5) as T:
            for f in (lambda: other.cmux(T, d1[:1]), lambda: other.lut_write(T, mem[:1, :2], 1, d1[:1]), lambda: other.tlwe_rotate(T, d1[:1], 1)):
                with pytest.raises(ia.IeacheError, match="another context") as e:
                    f()
                assert e.value.code == -22
    finally:
        other.close()


def test_lut_write_device(ia, ctx_of):
    """depth 0, 1 and 4, 3 items with per-item memories, out of place and in place, equal to tools.lut_write_reference; one item
    per piece; the refusals of section 3i; a warm call allocates nothing."""
    import torch
    from ieache_amd import tools
    kb, ctx = ctx_of()
    l, Bgbit = 6, 5
    pg = tools.with_gadget(kb.p, l, Bgbit)
    S, d1, d0, mem = words(l, Bgbit)
    new = d1[:3]
    tnew = dev(new)
    with ctx.tgsw_prepare(S, l, Bgbit) as S5:
        for depth, explicit in ((0, False), (1, True), (4, True), (4, False)):
            sel = selectors((3, depth)) if explicit else None
            m = mem[:, :1 << depth]
            want = tools.lut_write_reference(pg, S, m, depth, new, sel_of=sel)
            tsel = dev(sel) if explicit else None
            tm, tout = dev(m), torch.full((3, 1 << depth, 2, N), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            args = (S5, 3, depth, tsel.data_ptr() if explicit else None, tnew.data_ptr(), tm.data_ptr())
            st = ia.Stats()
            ctx.lut_write_device(*args, tout.data_ptr(), stats=st)
            assert np.array_equal(tout.cpu().numpy(), want), depth
            assert np.array_equal(tm.cpu().numpy(), m) and np.array_equal(tnew.cpu().numpy(), new)
            assert st.chunks == 1 and st.levels == 2 * depth and st.bootstraps == 0 and st.keyswitch_launches == 0
            assert st.blind_rotate_launches == 2 * max(depth, 1) + 1
            # one item per piece, in place
            ctx.set_option("cmux_piece_rows", 3 if depth == 4 else 1)
            st = ia.Stats()
            ctx.lut_write_device(*args, tm.data_ptr(), stats=st)
            ctx.set_option("cmux_piece_rows", 8192)
            assert np.array_equal(tm.cpu().numpy(), want) and st.chunks == 3, depth
            # the host composition gives the same words
            assert np.array_equal(ctx.lut_write(S5, m, depth, new, sel_of=sel), want), depth
        # warm: the same call again allocates nothing (in place twice: the second writes onto the first's result)
        tm = dev(mem)
        torch.cuda.synchronize()
        ctx.lut_write_device(S5, 3, 4, None, tnew.data_ptr(), tm.data_ptr(), tm.data_ptr())
        warm = ctx.get_option("staging_allocations")
        ctx.lut_write_device(S5, 3, 4, None, tnew.data_ptr(), tm.data_ptr(), tm.data_ptr())
        assert ctx.get_option("staging_allocations") == warm
        once = tools.lut_write_reference(pg, S, mem, 4, new)
        assert np.array_equal(tm.cpu().numpy(), tools.lut_write_reference(pg, S, once, 4, new))
        # refusals: overlap other than out == mem, the output over new or the indices, a host pointer, the depth, no memory
        row = 2 * N * 4
        tsel, tout = dev(selectors((3, 2))), torch.full((4, 4, 2, N), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.lut_write_device(S5, 0, 2, None, tnew.data_ptr(), tout.data_ptr(), tout.data_ptr())
        for a in ((None, tnew.data_ptr(), tout.data_ptr(), tout.data_ptr() + row), (None, tnew.data_ptr(), tout.data_ptr() + row, tout.data_ptr()),
                  (None, tout.data_ptr() + 5 * row, tout.data_ptr(), tout.data_ptr()), (tsel.data_ptr(), tnew.data_ptr(), tout.data_ptr(), tsel.data_ptr())):
            with pytest.raises(ia.IeacheError, match="overlaps") as e:
                ctx.lut_write_device(S5, 3, 2, *a)
            assert e.value.code == -22
        with pytest.raises(ia.IeacheError, match="not a device pointer") as e:
            ctx.lut_write_device(S5, 3, 2, None, new.ctypes.data, tout.data_ptr(), tout.data_ptr())
        assert e.value.code == -22
        for d in (-1, 13):
            with pytest.raises(ia.IeacheError, match="depth") as e:
                ctx.lut_write_device(S5, 1, d, None, tnew.data_ptr(), tout.data_ptr(), tout.data_ptr())
            assert e.value.code == -22
        with pytest.raises(ia.IeacheError, match="null") as e:
            ctx.lut_write_device(S5, 1, 2, None, tnew.data_ptr(), None, tout.data_ptr())
        assert e.value.code == -22
        assert (tout.cpu().numpy() == -1).all()  # and no refused call wrote anything


def lut_write_host(ia, ctx, tgsw, mem, depth, new, sel_of=None, stats=None):
    """ieache_lut_write, the host form of the C ABI, called as it is bound (Context.lut_write stays the composition of the
    tree's and the scatter's host forms) -> (return code, out)"""
    from ieache_amd.evaluator import _i32, _stats_ref
    mem = np.ascontiguousarray(mem, dtype=np.int32)
    new = np.ascontiguousarray(new, dtype=np.int32)
    of = None if sel_of is None else np.ascontiguousarray(sel_of, dtype=np.int32)
    out = np.full_like(mem, -1)
    rc = ia.lib().ieache_lut_write(ctx.h, tgsw.h, new.shape[0], depth, None if of is None else _i32(of), _i32(new), _i32(mem), _i32(out), _stats_ref(stats))
    return rc, out


def test_lut_write_host_form(ia, ctx_of):
    """ieache_lut_write on host arrays: depth 0, 1 and 4, 3 items, explicit and NULL sel_of, word for word
    tools.lut_write_reference; one item per piece; a warm call allocates nothing; an index outside the set is named and
    nothing is written; a set of another context is refused by the host form and by the device form."""
    import torch
    from ieache_amd import tools
    kb, ctx = ctx_of()
    l, Bgbit = 6, 5
    pg = tools.with_gadget(kb.p, l, Bgbit)
    S, d1, d0, mem = words(l, Bgbit)
    new = d1[:3]
    with ctx.tgsw_prepare(S, l, Bgbit) as S5:
        for depth, explicit in ((0, False), (1, True), (1, False), (4, True), (4, False)):
            sel = selectors((3, depth)) if explicit else None
            m = mem[:, :1 << depth].copy()
            want = tools.lut_write_reference(pg, S, m, depth, new, sel_of=sel)
            st = ia.Stats()
            rc, out = lut_write_host(ia, ctx, S5, m, depth, new, sel, stats=st)
            assert rc == 0 and np.array_equal(out, want), (depth, explicit)
            assert np.array_equal(m, mem[:, :1 << depth])  # the caller's memory is read only
            assert st.chunks == 1 and st.levels == 2 * depth and st.bootstraps == 0 and st.blind_rotate_launches == 2 * max(depth, 1) + 1
            ctx.set_option("cmux_piece_rows", 3 if depth == 4 else 1)
            st = ia.Stats()
            rc, out = lut_write_host(ia, ctx, S5, m, depth, new, sel, stats=st)
            ctx.set_option("cmux_piece_rows", 8192)
            assert rc == 0 and np.array_equal(out, want) and st.chunks == 3, (depth, explicit)
        # no items: nothing to do
        assert lut_write_host(ia, ctx, S5, mem[:0, :4], 2, new[:0])[0] == 0
        # warm
        sel = selectors((3, 4))
        first = lut_write_host(ia, ctx, S5, mem, 4, new, sel)[1]
        warm = ctx.get_option("staging_allocations")
        again = lut_write_host(ia, ctx, S5, mem, 4, new, sel)[1]
        assert ctx.get_option("staging_allocations") == warm and np.array_equal(first, again)
        # an index outside the set: the first one is named, IEACHE_EINVAL, nothing written
        bad = np.array([[0, 4], [5, 1], [-1, 7]], dtype=np.int32)
        rc, out = lut_write_host(ia, ctx, S5, mem[:, :4], 2, new, bad)
        assert rc == -22 and "lut_write: sel_of[2] = 5 is outside [0, 5)" in ia.lib().ieache_last_error().decode()
        assert (out == -1).all()
        for d in (-1, 13):
            rc, out = lut_write_host(ia, ctx, S5, mem[:, :1], d, new)
            assert rc == -22 and "depth" in ia.lib().ieache_last_error().decode()
        # ... where the device form clamps an explicit index into the set
        tbad, tnew, tm = dev(bad), dev(new), dev(mem[:, :4])
        torch.cuda.synchronize()
        ctx.lut_write_device(S5, 3, 2, tbad.data_ptr(), tnew.data_ptr(), tm.data_ptr(), tm.data_ptr())
        assert np.array_equal(tm.cpu().numpy(), tools.lut_write_reference(pg, S, mem[:, :4], 2, new, sel_of=np.clip(bad, 0, 4)))
        # a set of another context: both forms of the new call
        other = ia.Context.from_arrays(kb.p, kb.bk, kb.ksk)
        try:
            rc, out = lut_write_host(ia, other, S5, mem[:, :4], 2, new)
            assert rc == -22 and "another context" in ia.lib().ieache_last_error().decode() and (out == -1).all()
            tout = torch.full((3, 4, 2, N), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            with pytest.raises(ia.IeacheError, match="another context") as e:
                other.lut_write_device(S5, 3, 2, None, tnew.data_ptr(), tm.data_ptr(), tout.data_ptr())
            assert e.value.code == -22 and (tout.cpu().numpy() == -1).all()
        finally:
            other.close()


def test_twelve_writes_in_place_at_the_product_parameters(ia, gpu_ctx):
    """n = 630, key at (3, 7), selectors at (6, 5): the sequence of gadget_sequence.write_sequence on ONE memory kept on the device,
    in place, one lut_write_device call per write.  After every write the words are the CPU sequence's and every coefficient of
    every slot is within 2^-8 of what the slot should hold (a decoding condition; the CPU sequence gives at most 7.6e-4)."""
    import torch
    from ieache_amd import tools
    kb, ctx = gpu_ctx(630, N)
    seq = GS.write_sequence(kb.p, kb.tlwe_key, 6, 5)
    tmem, tsel = dev(seq["mem0"]), dev(seq["steps"][0][1])
    errs = []
    for w, (samples, sel, new) in enumerate(seq["steps"]):
        tnew = dev(new)
        torch.cuda.synchronize()
        with ctx.tgsw_prepare(samples, 6, 5) as S:
            ctx.lut_write_device(S, 1, GS.DEPTH, tsel.data_ptr(), tnew.data_ptr(), tmem.data_ptr(), tmem.data_ptr())
        got = tmem.cpu().numpy()
        assert np.array_equal(got, seq["mems"][w]), w
        errs.append(float(GS.torus_distance(tools.tlwe_phase(kb.p, kb.tlwe_key, got[0]), seq["want"][w]).max()))
    print("twelve depth-4 replace writes at address 15, (6, 5) selectors, on the card: largest phase error after write w: " +
          " ".join("%.2e" % e for e in errs) + " (bound 2^-8 = %.3e)" % 2.0 ** -8)
    assert max(errs) < 2.0 ** -8
