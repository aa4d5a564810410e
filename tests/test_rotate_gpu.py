"""The rotation by an encrypted amount and the coefficient-level lookup on the GPU (k_rotate_x1, csrc/rotate.hip; include/ieache.h
section 3h), word for word against the C references (ieache_tlwe_rotate_reference / ieache_lut_read_reference, which
tests/test_rotate_cpu.py holds to the numpy restatement and to the oracle's blind_rotate_step) and, once per parameter set,
against the numpy restatement itself.  All at N = 1024: that is what the kernel covers.  The bit-exact cases take random
full-range words -- no encryption is needed for that; the last test reads and writes a 4 096-coefficient table at the product
parameters, word for word and by meaning."""
import numpy as np
import pytest

import cmux_reference as CR
import rotate_reference as RR

pytestmark = pytest.mark.gpu

N = 1024
G = 4  # rows per workgroup of k_rotate_x1 (kCmuxWaveRows, csrc/cmux_plan.h)
SETS = [{}, {"l": 2, "Bgbit": 10}]
IDS = ["l3_Bg7", "l2_Bg10"]
# every boundary of the 2N-ring, a no-op step and a few amounts between; a prefix of 10 holds all six boundary amounts
AMOUNTS = [1, N - 1, 0, N, N + 1, 2 * N - 1, 5, 1500, N + 513, 77]

_words = {}
_rotated = {}


def words(p):
    """per parameter set, made once and left unchanged: 5 full-range samples, 5 rows, 2 tables of 4 rows"""
    key = (p.l, p.Bgbit)
    if key not in _words:
        rng = np.random.default_rng(9850 + 10 * p.l + p.Bgbit)
        _words[key] = (CR.full_range(rng, (5, 2 * p.l, 2, N)), CR.full_range(rng, (5, 2, N)), CR.full_range(rng, (2, 4, 2, N)))
    return _words[key]


def selectors(width, count, n):
    """explicit indices [count][width] into a set of n, repeats among them and the last index; the same for every caller"""
    rng = np.random.default_rng(9860 + 100 * width + 10 * count + n)
    sel = rng.integers(0, n, size=(count, max(width, 1))).astype(np.int32)
    sel[-1, :] = n - 1
    return sel


def amounts(steps):
    return np.array((AMOUNTS * 7)[:steps], dtype=np.int32)


def rotated(p, n, count, steps, explicit, listed):
    """(sel_of or None, amounts or None, the C reference's rows [count][2][N]) of the first `count` rows on the first n samples:
    computed once, shared by the tests below"""
    from ieache_amd import tools
    key = (p.l, p.Bgbit, n, count, steps, explicit, listed)
    if key not in _rotated:
        S, rows, _ = words(p)
        sel = selectors(steps, count, n) if explicit else None
        am = amounts(steps) if listed else None
        _rotated[key] = (sel, am, tools.tlwe_rotate_reference(p, S[:n], rows[:count], steps, sel_of=sel, amounts=am))
    return _rotated[key]


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


# (n samples, count, steps, explicit selectors, listed amounts): 1, 3 and 5 rows through workgroups of G = 4
CASES = [(5, 1, 0, False, False), (5, 3, 0, True, False),
         (5, 1, 1, False, False), (5, 5, 1, True, True), (1, 3, 1, False, True),
         (5, 3, 2, False, True), (5, 5, 2, True, False), (1, 1, 2, False, False),
         (5, 1, 10, True, True), (5, 3, 10, False, False), (5, 5, 10, True, False), (1, 5, 10, False, True),
         (5, 1, 64, True, True), (5, 5, 64, False, False)]


@pytest.mark.parametrize("kw", SETS, ids=IDS)
def test_word_for_word(ia, ctx_of, kw):
    """steps 0, 1, 2, 10, 64 with 1, 3 and 5 rows; sets of 1 and 5 samples; selectors implied and explicit; the default amounts and
    a list with 0, 1, N - 1, N, N + 1, 2N - 1; the stats of section 3h."""
    kb, ctx = ctx_of(kw)
    p = kb.p
    S, rows, _ = words(p)
    with ctx.tgsw_prepare(S) as S5, ctx.tgsw_prepare(S[:1]) as S1:
        for n, count, steps, explicit, listed in CASES:
            sel, am, want = rotated(p, n, count, steps, explicit, listed)
            st = ia.Stats()
            got = ctx.tlwe_rotate(S5 if n == 5 else S1, rows[:count], steps, sel_of=sel, amounts=am, stats=st)
            assert got.shape == (count, 2, N) and np.array_equal(got, want), (n, count, steps, explicit, listed)
            assert st.bootstraps == 0 and st.keyswitch_launches == 0 and st.levels == steps and st.chunks == 1 and st.total_ms > 0
            assert st.blind_rotate_launches == 1
        assert np.array_equal(rotated(p, 5, 3, 0, True, False)[2], rows[:3])  # steps = 0 copies
        # once against the numpy restatement itself
        sel = np.array([[4, 0, 4], [1, 3, 2]], dtype=np.int32)
        am = [N + 1, 2 * N - 1, 640]
        assert np.array_equal(ctx.tlwe_rotate(S5, rows[:2], 3, sel_of=sel, amounts=am), RR.tlwe_rotate(S, rows[:2], 3, p.l, p.Bgbit, sel_of=sel, amounts=am))
        assert ctx.tlwe_rotate(S5, rows[:0], 2).shape == (0, 2, N)


@pytest.mark.parametrize("kw", SETS, ids=IDS)
def test_pieces(ia, ctx_of, kw):
    """Caps of 1 and 3 rows per piece: the same words, chunks == pieces, one launch per piece whatever the number of steps; the
    item index behind an implied selector and an explicit one's row counts from the call's first row, not the piece's."""
    kb, ctx = ctx_of(kw)
    p = kb.p
    S, rows, _ = words(p)
    with ctx.tgsw_prepare(S) as S5:
        for count, steps, explicit, listed in ((5, 10, True, False), (3, 10, False, False), (5, 2, True, False)):
            sel, am, want = rotated(p, 5, count, steps, explicit, listed)
            for cap in (1, 3):
                ctx.set_option("cmux_piece_rows", cap)
                pieces = -(-count // cap)
                assert ctx.cmux_plan(count)["pieces"] == pieces
                st = ia.Stats()
                assert np.array_equal(ctx.tlwe_rotate(S5, rows[:count], steps, sel_of=sel, amounts=am, stats=st), want), (count, steps, cap)
                assert st.chunks == pieces and st.blind_rotate_launches == pieces and st.levels == steps
            ctx.set_option("cmux_piece_rows", 8192)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_device_form_in_place_clamps_and_refuses(ia, ctx_of):
    import torch
    from ieache_amd import tools
    kb, ctx = ctx_of({})
    p = kb.p
    S, rows, _ = words(p)
    count, steps, n = 5, 10, 5
    sel, am, want = rotated(p, n, count, steps, True, False)
    tS, tin, tsel = dev(S), dev(rows[:count]), dev(sel)
    tout = torch.full((count, 2, N), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with ctx.tgsw_prepare_device(tS.data_ptr(), n) as S5:
        st = ia.Stats()
        ctx.tlwe_rotate_device(S5, count, steps, tsel.data_ptr(), None, tin.data_ptr(), tout.data_ptr(), stats=st)
        assert np.array_equal(tout.cpu().numpy(), want) and st.chunks == 1 and st.bootstraps == 0 and st.levels == steps
        assert np.array_equal(tin.cpu().numpy(), rows[:count])
        # in place: the same words; the indices as they were
        ctx.tlwe_rotate_device(S5, count, steps, tsel.data_ptr(), None, tin.data_ptr(), tin.data_ptr())
        assert np.array_equal(tin.cpu().numpy(), want) and np.array_equal(tsel.cpu().numpy(), sel)
        # in place with listed amounts and implied selectors, in pieces of 3 rows
        sel2, am2, want2 = rotated(p, n, count, steps, False, True)
        tin2, tam = dev(rows[:count]), dev(am2)
        torch.cuda.synchronize()
        ctx.set_option("cmux_piece_rows", 3)
        ctx.tlwe_rotate_device(S5, count, steps, None, tam.data_ptr(), tin2.data_ptr(), tin2.data_ptr())
        ctx.set_option("cmux_piece_rows", 8192)
        assert sel2 is None and np.array_equal(tin2.cpu().numpy(), want2)
        # explicit bad indices are clamped and amounts masked to 2N - 1 on the device; the host form names the first bad one
        bad = np.array([[0, 5], [-1, 7], [1 << 30, -(1 << 31)]], dtype=np.int32)
        bad_am = np.array([2 * N + 3, -1], dtype=np.int32)
        tbad, tbam = dev(bad), dev(bad_am)
        torch.cuda.synchronize()
        ctx.tlwe_rotate_device(S5, 3, 2, tbad.data_ptr(), tbam.data_ptr(), tin.data_ptr(), tout.data_ptr())
        clamped = tools.tlwe_rotate_reference(p, S, want[:3], 2, sel_of=np.clip(bad, 0, n - 1), amounts=bad_am & (2 * N - 1))
        assert np.array_equal(tout.cpu().numpy()[:3], clamped)
        for kws, match in ((dict(sel_of=bad), r"sel_of\[1\] = 5"), (dict(amounts=[3, 2 * N]), r"amount_of\[1\] = 2048"),
                           (dict(amounts=[-1, 3]), r"amount_of\[0\] = -1")):
            with pytest.raises(ia.IeacheError, match=match) as e:
                ctx.tlwe_rotate(S5, rows[:3], 2, **kws)
            assert e.value.code == -22
        # refusals: an output that overlaps the input other than exactly in place, the output over the indices or the amounts,
        # a host pointer, the steps
        row = 2 * N * 4
        tbig = torch.zeros((count + 1, 2, N), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.tlwe_rotate_device(S5, 0, steps, None, None, tin.data_ptr(), tin.data_ptr())
        for args in ((None, None, tbig.data_ptr(), tbig.data_ptr() + row), (None, None, tbig.data_ptr() + row, tbig.data_ptr()),
                     (None, None, tbig.data_ptr(), tbig.data_ptr() + 4), (tsel.data_ptr(), None, tin.data_ptr(), tsel.data_ptr()),
                     (None, tam.data_ptr(), tin.data_ptr(), tam.data_ptr())):
            with pytest.raises(ia.IeacheError, match="overlaps") as e:
                ctx.tlwe_rotate_device(S5, count, steps, *args)
            assert e.value.code == -22
        with pytest.raises(ia.IeacheError, match="not a device pointer") as e:
            ctx.tlwe_rotate_device(S5, count, steps, None, None, rows.ctypes.data, tout.data_ptr())
        assert e.value.code == -22
        for s in (-1, 65):
            with pytest.raises(ia.IeacheError, match="steps") as e:
                ctx.tlwe_rotate_device(S5, 1, s, None, None, tin.data_ptr(), tout.data_ptr())
            assert e.value.code == -22
            with pytest.raises(ia.IeacheError, match="steps"):
                ctx.lut_read_device(S5, 1, 0, s, None, None, tin.data_ptr(), 1, None, tout.data_ptr())
        with pytest.raises(ia.IeacheError, match="steps"):
            ctx.tlwe_rotate(S5, rows[:1], 65)
        # a set of another context
        other = ia.Context.from_arrays(kb.p, kb.bk, kb.ksk)
        try:
            for f in (lambda: other.tlwe_rotate(S5, rows[:1], 1), lambda: other.tlwe_rotate_device(S5, 1, 1, None, None, tin.data_ptr(), tout.data_ptr()),
                      lambda: other.lut_read(S5, rows[:1], 0, 1),
                      lambda: other.lut_read_device(S5, 1, 0, 1, None, None, tin.data_ptr(), 1, None, tout.data_ptr())):
                with pytest.raises(ia.IeacheError, match="another context") as e:
                    f()
                assert e.value.code == -22
        finally:
            other.close()
        assert np.array_equal(tout.cpu().numpy()[:3], clamped)  # and no refused call wrote anything


@pytest.mark.parametrize("kw", SETS, ids=IDS)
def test_lut_read(ia, ctx_of, kw):
    """(depth, steps) = (0, 3), (2, 0), (2, 10), three items over two tables: word for word the C reference and the composition
    lut_tree -> tlwe_rotate -> tlwe_extract -> keyswitch of the existing calls, with and without the key switch; coef != 0 once;
    implied selectors once; one item per piece; the device form's strided rows."""
    import torch
    from ieache_amd import tools
    kb, ctx = ctx_of(kw)
    p = kb.p
    S, _, tables = words(p)
    count, tof = 3, np.array([1, 0, 1], dtype=np.int32)
    with ctx.tgsw_prepare(S) as S5:
        for depth, steps, coef, explicit in ((0, 3, 0, True), (2, 0, 0, True), (2, 10, 0, True), (2, 10, 777, True), (2, 3, 0, False)):
            sel = selectors(depth + steps, count, 5) if explicit else None
            am = amounts(steps) if coef else None
            t = tables[:, :1 << depth]
            common = dict(sel_of=sel, amounts=am, table_of=tof, coef=coef)
            want_u = tools.lut_read_reference(p, S, t, depth, steps, **common)
            want = tools.lut_read_reference(p, S, t, depth, steps, ksk=kb.ksk, **common)
            st = ia.Stats()
            got_u = ctx.lut_read(S5, t, depth, steps, keyswitch=False, stats=st, **common)
            assert got_u.shape == (count, N + 1) and np.array_equal(got_u, want_u), (depth, steps, coef)
            assert st.bootstraps == 0 and st.keyswitch_launches == 0 and st.levels == depth + steps and st.chunks == 1
            st = ia.Stats()
            got = ctx.lut_read(S5, t, depth, steps, stats=st, **common)
            assert got.shape == (count, p.n + 1) and np.array_equal(got, want), (depth, steps, coef)
            assert st.bootstraps == 0 and st.keyswitch_launches == 1 and st.levels == depth + steps and st.chunks == 1
            if explicit:
                # the existing calls composed: the tree by the high selectors, the rotation by the low ones
                picked = ctx.lut_tree(S5, t, depth, sel_of=sel[:, steps:] if depth else None, table_of=tof)
                turned = ctx.tlwe_rotate(S5, picked, steps, sel_of=sel[:, :steps] if steps else None, amounts=am)
                u = ctx.tlwe_extract(turned, coef_of=[coef] * count)
                assert np.array_equal(u, got_u) and np.array_equal(ctx.keyswitch(u), got), (depth, steps, coef)
        # one item per piece
        sel = selectors(12, count, 5)
        want = tools.lut_read_reference(p, S, tables, 2, 10, sel_of=sel, table_of=tof, ksk=kb.ksk)
        ctx.set_option("cmux_piece_rows", 1)
        st = ia.Stats()
        assert np.array_equal(ctx.lut_read(S5, tables, 2, 10, sel_of=sel, table_of=tof, stats=st), want)
        assert st.chunks == count and st.keyswitch_launches == count and st.levels == 12
        ctx.set_option("cmux_piece_rows", 8192)
        # the device form: rows of extract_stride words without the key switch, of lwe_stride words with it
        tt, tsel, ttof = dev(tables), dev(sel), dev(tof)
        stride = N + 4
        tu = torch.full((count, stride), -1, dtype=torch.int32, device="cuda")
        tl = torch.full((count, (p.n + 4) & ~3), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.lut_read_device(S5, count, 2, 10, tsel.data_ptr(), None, tt.data_ptr(), 2, ttof.data_ptr(), tu.data_ptr(), keyswitch=False)
        ctx.lut_read_device(S5, count, 2, 10, tsel.data_ptr(), None, tt.data_ptr(), 2, ttof.data_ptr(), tl.data_ptr())
        assert np.array_equal(tu.cpu().numpy()[:, :N + 1], tools.lut_read_reference(p, S, tables, 2, 10, sel_of=sel, table_of=tof))
        assert np.array_equal(tl.cpu().numpy()[:, :p.n + 1], want)
        assert ctx.lut_read(S5, tables, 2, 10, count=0).shape == (0, p.n + 1)
        with pytest.raises(ia.IeacheError, match=r"coef\[0\] = 1024"):
            ctx.lut_read(S5, tables, 2, 10, coef=1024)
        with pytest.raises(ia.IeacheError, match="overlaps"):
            ctx.lut_read_device(S5, count, 2, 10, tsel.data_ptr(), None, tt.data_ptr(), 2, None, tt.data_ptr() + 64)


def test_warm_calls_allocate_nothing(ia, ctx_of):
    kb, ctx = ctx_of({})
    S, rows, tables = words(kb.p)
    sel = selectors(12, 3, 5)
    with ctx.tgsw_prepare(S) as S5:
        def calls():
            return (ctx.tlwe_rotate(S5, rows[:3], 10, sel_of=sel[:, :10]), ctx.lut_read(S5, tables, 2, 10, sel_of=sel, table_of=[0, 1, 0]),
                    ctx.lut_read(S5, tables, 2, 10, sel_of=sel, table_of=[0, 1, 0], keyswitch=False))
        first = calls()
        warm = ctx.get_option("staging_allocations")
        again = calls()
        assert ctx.get_option("staging_allocations") == warm
        assert all(np.array_equal(a, b) for a, b in zip(first, again))
    # a gate call afterwards finds its operand rows as it needs them
    bits = np.array([[0, 1, 1], [1, 1, 0]], dtype=np.uint8)
    assert np.array_equal(kb.dec(ctx.gates(ia.GATE_AND, kb.enc(bits[0], 91), kb.enc(bits[1], 92))), bits[0] & bits[1])


def test_packed_table_read_and_write_at_the_product_parameters(ia, gpu_ctx):
    """(3, 7), noise 2^-25: the table of test_rotate_cpu.packed_table on the card -- depth 2 and steps 10 over 4 096 coefficients,
    the words the CPU reference's, the addressed message within 2^-8, and within 1/8 through the key switch.  Then the write as a
    composition: a value at coefficient 0 is moved to the addressed coefficient by tlwe_rotate with amounts +2^t and to the
    addressed slot by lut_scatter at depth 2; its phase appears at that (slot, coefficient) and nowhere else beyond 2^-8."""
    from ieache_amd import tools
    from test_rotate_cpu import ADDRESSES, lwe_phase, packed_table, torus_distance
    kb, ctx = gpu_ctx(4, N)
    p = kb.p
    T = packed_table(p, kb.tlwe_key)
    want = np.array([T["msg"][a >> 10, a & 1023] for a in ADDRESSES])
    mu = 1 << 29
    value = tools.tlwe_encrypt(p, kb.tlwe_key, np.eye(1, N, 0, dtype=np.int32)[0] * mu, 321)
    plus = tools.rotate_amounts(10, toward_zero=False)
    with ctx.tgsw_prepare(T["samples"]) as S:
        rows = ctx.lut_read(S, T["table"], 2, 10, sel_of=T["sel_of"], keyswitch=False)
        assert np.array_equal(rows, T["rows"])
        err = torus_distance(lwe_phase(kb.tlwe_key, rows), want)
        print("depth 2 + steps 10 lookup on the card: largest phase error %.3e (bound 2^-8 = %.3e)" % (err.max(), 2.0 ** -8))
        assert err.max() < 2.0 ** -8
        lwe = ctx.lut_read(S, T["table"], 2, 10, sel_of=T["sel_of"])
        assert np.array_equal(lwe, tools.lut_read_reference(p, T["samples"], T["table"], 2, 10, sel_of=T["sel_of"], ksk=kb.ksk))
        assert torus_distance(lwe_phase(kb.lwe_key, lwe), want).max() < 1 / 8
        # the write at an encrypted coefficient, as a composition of tlwe_rotate and lut_scatter
        moved = ctx.tlwe_rotate(S, np.repeat(value, 4, axis=0), 10, sel_of=T["sel_of"][:, :10], amounts=plus)
        leaves = ctx.lut_scatter(S, moved, 2, sel_of=T["sel_of"][:, 10:])
    moved_ref = tools.tlwe_rotate_reference(p, T["samples"], np.repeat(value, 4, axis=0), 10, sel_of=T["sel_of"][:, :10], amounts=plus)
    assert np.array_equal(moved, moved_ref)
    assert np.array_equal(leaves, tools.lut_scatter_reference(p, T["samples"], moved_ref, 2, sel_of=T["sel_of"][:, 10:]))
    for i, a in enumerate(ADDRESSES):
        expect = np.zeros((4, N), dtype=np.int32)
        expect[a >> 10, a & 1023] = mu
        err = torus_distance(tools.tlwe_phase(p, kb.tlwe_key, leaves[i]), expect)
        assert err.shape == (4, N) and err.max() < 2.0 ** -8, (a, err.max())
