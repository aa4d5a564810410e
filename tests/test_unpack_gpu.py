"""The unpacking key switch (k_ksm_window_digits / k_ksm_window_init / k_ksm_window_rows, csrc/keyswitch_mfma.hip) and the read of
an addressed word on the GPU (include/ieache.h section 3m), word for word against the C references (ieache_unpack_reference,
ieache_word_read_reference, which tests/test_unpack_cpu.py holds to the numpy restatement).  The bit-exact cases take random
full-range words -- no encryption is needed for that; the last test reads the table of tests/test_unpack_cpu.py at the product
parameters, word for word and by meaning, and adds the two read words with CIRC_ADD.

Every key-switch family must give the same words: "ks_mfma_min" = 1 sends every run through the fused front end of the MFMA
product, a value above the row count through stored rows and the walk kernels."""
import numpy as np
import pytest

import cmux_reference as CR
import pack_reference as PR
import unpack_reference as UR

pytestmark = pytest.mark.gpu

N = 1024
WINDOWS = [(0, 1, 1), (1023, 1, 1), (0, 1024, 1), (3, 5, 200), (511, 2, 512), (0, 64, 1)]
FUSED, WALKED = 1, 1 << 40  # "ks_mfma_min"
# (key's gadget, set's gadget or None for the key's): the two fixed builds and the run-time build
SETS = [({}, None), ({"l": 2, "Bgbit": 10}, None), ({}, (6, 5))]
IDS = ["l3_Bg7", "l2_Bg10", "l6_Bg5_rt"]

_made = {}


def once(key, make):
    if key not in _made:
        _made[key] = make()
    return _made[key]


def random_samples(n_ring=N):
    return once(("samples", n_ring), lambda: CR.full_range(np.random.default_rng(14000 + n_ring), (3, 2, n_ring)))


@pytest.fixture
def tuned(gpu_ctx):
    """gpu_ctx whose contexts get the options put back as they were found afterwards"""
    used = []

    def make(n=4, n_ring=N, **kw):
        kb, ctx = gpu_ctx(n, n_ring, **kw)
        used.append(ctx)
        return kb, ctx

    yield make
    for ctx in used:
        ctx.set_option("ks_mfma_min", 64)
        ctx.set_option("chunk", 65536)
        ctx.set_option("cmux_piece_rows", 8192)
        ctx.set_option("force_generic", 0)
        ctx.set_packing_key(None)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def runs_of(rows, chunk):
    return -(-rows // min(rows, chunk))


def test_windows_word_for_word_on_every_family(ia, tuned):
    from ieache_amd import tools
    kb, ctx = tuned()
    p, samples = kb.p, random_samples()
    for first, width, spread in WINDOWS:
        for count in (1, 3):
            want = tools.unpack_reference(p, samples[:count], first, width, spread, ksk=kb.ksk)
            for mfma_min in (FUSED, WALKED):
                ctx.set_option("ks_mfma_min", mfma_min)
                st = ia.Stats()
                got = ctx.unpack(samples[:count], first, width, spread, stats=st)
                assert got.shape == (count, width, p.n + 1) and np.array_equal(got, want), (first, width, spread, count, mfma_min)
                assert st.bootstraps == 0 and st.levels == 1 and st.chunks == 1 and st.keyswitch_launches == 1 and st.blind_rotate_launches == 0
                assert st.total_ms > 0 and st.keyswitch_ms > 0
    # ... and against the numpy restatement itself, once
    ctx.set_option("ks_mfma_min", FUSED)
    assert np.array_equal(ctx.unpack(samples[:1], 3, 5, 200), UR.unpack(samples[:1], 3, 5, 200, ksk=kb.ksk, ks=(p.ks_t, p.ks_basebit)))
    # the default threshold, and the any-parameter kernel
    ctx.set_option("ks_mfma_min", 64)
    want = tools.unpack_reference(p, samples, 0, 64, 1, ksk=kb.ksk)
    assert np.array_equal(ctx.unpack(samples, 0, 64, 1), want)
    ctx.set_option("force_generic", 1)
    assert np.array_equal(ctx.unpack(samples, 0, 64, 1), want)
    ctx.set_option("force_generic", 0)
    # one sample [2][N] is one item; no items: nothing to do
    assert np.array_equal(ctx.unpack(samples[1], 0, 64, 1)[0], want[1])
    st = ia.Stats()
    assert ctx.unpack(samples[:0], 0, 1, 1, stats=st).shape == (0, 1, p.n + 1) and st.keyswitch_launches == 0 and st.chunks == 0


def test_padding_edge_and_runs_inside_an_item(ia, tuned):
    """3 items x 171 rows = 513 rows, one past the product's padding of 512; chunks that do not divide the width, so that runs
    begin and end inside an item: the same words, chunks == keyswitch_launches == runs."""
    from ieache_amd import tools
    kb, ctx = tuned()
    p, samples = kb.p, random_samples()
    want = tools.unpack_reference(p, samples, 2, 171, 5, ksk=kb.ksk)
    for mfma_min in (FUSED, WALKED):
        ctx.set_option("ks_mfma_min", mfma_min)
        for chunk in (65536, 512, 200, 7):
            ctx.set_option("chunk", chunk)
            st = ia.Stats()
            got = ctx.unpack(samples, 2, 171, 5, stats=st)
            assert np.array_equal(got, want), (mfma_min, chunk)
            assert st.chunks == runs_of(513, chunk) and st.keyswitch_launches == runs_of(513, chunk) and st.levels == 1, (mfma_min, chunk)
        ctx.set_option("chunk", 65536)
    # a run below the threshold after runs above it: 513 rows in runs of 200, 200, 113 with the product from 150 rows on
    ctx.set_option("ks_mfma_min", 150)
    ctx.set_option("chunk", 200)
    assert np.array_equal(ctx.unpack(samples, 2, 171, 5), want)
    want5 = tools.unpack_reference(p, samples, 3, 5, 200, ksk=kb.ksk)
    ctx.set_option("chunk", 4)
    for mfma_min in (FUSED, WALKED):
        ctx.set_option("ks_mfma_min", mfma_min)
        st = ia.Stats()
        assert np.array_equal(ctx.unpack(samples, 3, 5, 200, stats=st), want5) and st.chunks == 4 and st.keyswitch_launches == 4


def test_no_keyswitch_is_tlwe_extract(ia, tuned):
    from ieache_amd import tools
    kb, ctx = tuned()
    p, samples = kb.p, random_samples()
    for first, width, spread in ((3, 5, 200), (0, 64, 1), (1023, 1, 1)):
        coefs = np.tile(first + spread * np.arange(width, dtype=np.int32), 3)
        st = ia.Stats()
        got = ctx.unpack(samples, first, width, spread, keyswitch=False, stats=st)
        assert got.shape == (3, width, N + 1)
        assert np.array_equal(got.reshape(-1, N + 1), ctx.tlwe_extract(np.repeat(samples, width, axis=0), coef_of=coefs))
        assert np.array_equal(got, tools.unpack_reference(p, samples, first, width, spread))
        assert st.keyswitch_launches == 0 and st.blind_rotate_launches == 0 and st.bootstraps == 0 and st.levels == 1 and st.chunks == 1
        # ... and the key switch of those rows is the call with it
        assert np.array_equal(ctx.keyswitch(got.reshape(-1, N + 1)), ctx.unpack(samples, first, width, spread).reshape(-1, p.n + 1))


def test_device_form_warm_calls_and_refusals(ia, tuned):
    import torch
    from ieache_amd import tools
    kb, ctx = tuned()
    p, samples = kb.p, random_samples()
    first, width, spread = 3, 5, 200
    want = tools.unpack_reference(p, samples, first, width, spread, ksk=kb.ksk)
    want_u = tools.unpack_reference(p, samples, first, width, spread)
    stride, xstride = ctx.lwe_stride, ctx.extract_stride
    tin = dev(samples)
    tout = torch.full((3, width, stride), -1, dtype=torch.int32, device="cuda")
    tu = torch.full((3, width, xstride), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for mfma_min in (FUSED, WALKED):
        ctx.set_option("ks_mfma_min", mfma_min)
        tout.fill_(-1)
        torch.cuda.synchronize()
        st = ia.Stats()
        ctx.unpack_device(3, first, width, spread, tin.data_ptr(), tout.data_ptr(), stats=st)
        assert np.array_equal(tout.cpu().numpy()[:, :, :p.n + 1], want) and np.array_equal(tin.cpu().numpy(), samples)
        assert st.keyswitch_launches == 1 and st.chunks == 1 and st.levels == 1 and st.bootstraps == 0
    ctx.unpack_device(3, first, width, spread, tin.data_ptr(), tu.data_ptr(), keyswitch=False)
    assert np.array_equal(tu.cpu().numpy()[:, :, :N + 1], want_u)
    ctx.unpack_device(0, first, width, spread, tin.data_ptr(), tout.data_ptr())  # no items: a no-op
    # a warm host call allocates nothing, on either path
    for mfma_min in (FUSED, WALKED):
        ctx.set_option("ks_mfma_min", mfma_min)
        ctx.unpack(samples, first, width, spread)
        warm = ctx.get_option("staging_allocations")
        assert np.array_equal(ctx.unpack(samples, first, width, spread), want)
        assert ctx.get_option("staging_allocations") == warm
    # refusals, all before anything is launched
    tbig = torch.zeros((8, 2, N), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    # (the output over the input's first words, inside it, and ending 16 bytes into it)
    for d_in, d_out in ((tbig.data_ptr(), tbig.data_ptr()), (tbig.data_ptr(), tbig.data_ptr() + 8 * N), (tbig.data_ptr() + 8 * N, tbig.data_ptr() + 8 * N - 16)):
        with pytest.raises(ia.IeacheError, match="overlaps") as e:
            ctx.unpack_device(3, first, width, spread, d_in, d_out)
        assert e.value.code == -22
    with pytest.raises(ia.IeacheError, match="not a device pointer") as e:
        ctx.unpack_device(3, first, width, spread, samples.ctypes.data, tout.data_ptr())
    assert e.value.code == -22
    for bad, match in (((-1, 1, 1), "first must"), ((N, 1, 1), "first must"), ((0, 0, 1), "width must"), ((0, 1, 0), "spread must"),
                       ((0, N + 1, 1), "below N"), ((1023, 2, 1), "below N"), ((512, 2, 512), "below N")):
        for f in (lambda: ctx.unpack_device(3, bad[0], bad[1], bad[2], tin.data_ptr(), tout.data_ptr()), lambda: ctx.unpack(samples, *bad)):
            with pytest.raises(ia.IeacheError, match=match) as e:
                f()
            assert e.value.code == -22
    L = ia.lib()
    assert L.ieache_unpack_device(ctx.h, 3, first, width, spread, tin.data_ptr(), 2, tout.data_ptr(), None) == -22
    assert "unknown flag" in L.ieache_last_error().decode()
    assert np.array_equal(tout.cpu().numpy()[:, :, :p.n + 1], want)  # and no refused call wrote anything


@pytest.mark.parametrize("n,n_ring", [(37, 64), (37, 16)])
def test_unpack_on_toy_rings(ia, tuned, n, n_ring):
    """N = 64 has the product, N = 16 does not (the runs' rows are stored whatever "ks_mfma_min" says): unpack runs on any set the
    key switch supports."""
    from ieache_amd import tools
    kb, ctx = tuned(n, n_ring)
    p, samples = kb.p, random_samples(n_ring)
    for first, width, spread in ((0, 1, 1), (n_ring - 1, 1, 1), (0, n_ring, 1), (3, 3, 5), (n_ring // 2 - 1, 2, n_ring // 2)):
        want = tools.unpack_reference(p, samples, first, width, spread, ksk=kb.ksk)
        for mfma_min in (FUSED, WALKED):
            ctx.set_option("ks_mfma_min", mfma_min)
            assert np.array_equal(ctx.unpack(samples, first, width, spread), want), (first, width, spread, mfma_min)
        assert np.array_equal(ctx.unpack(samples, first, width, spread, keyswitch=False), tools.unpack_reference(p, samples, first, width, spread))


def test_unpack_of_pack_is_the_numpy_composition(ia, tuned):
    """unpack(first = shift, spread) reads back what pack(spread, shift) placed: both calls on the card against the numpy
    restatements composed, with a packing key of full-range words."""
    kb, ctx = tuned()
    p = kb.p
    rng = np.random.default_rng(14100)
    pk = PR.full_range(rng, (p.n, 8, 2, N))
    rows = PR.crafted_rows(rng, 16, p.n, 8, 2)
    ctx.set_packing_key(pk)
    m, spread, shift = 8, 3, 5
    packed = ctx.pack(rows.reshape(2, m, p.n + 1), spread=spread, shift=shift)
    want_packed = PR.pack(pk, rows, m, spread, shift)
    assert np.array_equal(packed, want_packed)
    want = UR.unpack(want_packed, shift, m, spread, ksk=kb.ksk, ks=(p.ks_t, p.ks_basebit))
    for mfma_min in (FUSED, WALKED):
        ctx.set_option("ks_mfma_min", mfma_min)
        assert np.array_equal(ctx.unpack(packed, shift, m, spread), want), mfma_min


# ---- the read of an addressed word ----
_words = {}


def words(l, Bgbit):
    """per gadget, made once and left unchanged: 5 full-range samples and two tables of 4 rows"""
    key = (l, Bgbit)
    if key not in _words:
        rng = np.random.default_rng(14200 + 10 * l + Bgbit)
        _words[key] = (CR.full_range(rng, (5, 2 * l, 2, N)), CR.full_range(rng, (2, 4, 2, N)))
    return _words[key]


def selectors(depth, steps, count, n=5):
    rng = np.random.default_rng(14210 + 100 * depth + 10 * count + steps)
    sel = rng.integers(0, n, size=(count, max(depth + steps, 1))).astype(np.int32)
    sel[-1, :] = n - 1
    return sel


def prepared(ctx, kb, gadget):
    from ieache_amd import tools
    p = kb.p if gadget is None else tools.with_gadget(kb.p, *gadget)
    S, tables = words(p.l, p.Bgbit)
    return p, S, tables, (ctx.tgsw_prepare(S) if gadget is None else ctx.tgsw_prepare(S, *gadget))


def launches(depth, steps):
    return max(depth, 1) + (1 if steps else 0)


@pytest.mark.parametrize("kw,gadget", SETS, ids=IDS)
def test_word_read_word_for_word(ia, tuned, kw, gadget):
    """depth 0, 2 x steps 0, 2, 5 x (width, unit) (1, 1), (3, 4), (32, 32) -- at steps 5 the bound unit 2^steps = N; selectors
    implied and explicit and the key-switch family in turn; two tables with table_of; width 1 is lut_read's row; the stats of
    section 3m."""
    from ieache_amd import tools
    kb, ctx = tuned(**kw)
    p, S, tables, tg = prepared(ctx, kb, gadget)
    with tg:
        at = 0
        for depth in (0, 2):
            for steps in (0, 2, 5):
                for width, unit in ((1, 1), (3, 4), (32, 32)):
                    count = (1, 3)[at % 2]
                    sel = selectors(depth, steps, count) if at % 2 else None
                    tof = np.array([1, 0, 1][:count], dtype=np.int32) if at % 3 else None
                    ctx.set_option("ks_mfma_min", (FUSED, WALKED)[(at // 2) % 2])
                    at += 1
                    t = tables[:, :1 << depth]
                    common = dict(sel_of=sel, table_of=tof, count=count)
                    want = tools.word_read_reference(p, S, t, depth, steps, width=width, unit=unit, ksk=kb.ksk, **common)
                    st = ia.Stats()
                    got = ctx.word_read(tg, t, depth, steps, width=width, unit=unit, stats=st, **common)
                    assert got.shape == (count, width, p.n + 1) and np.array_equal(got, want), (depth, steps, width, unit, count)
                    assert st.bootstraps == 0 and st.levels == depth + steps and st.chunks == 1 and st.keyswitch_launches == 1
                    assert st.blind_rotate_launches == launches(depth, steps) and st.total_ms > 0
                    st = ia.Stats()
                    rows = ctx.word_read(tg, t, depth, steps, width=width, unit=unit, keyswitch=False, stats=st, **common)
                    assert rows.shape == (count, width, N + 1) and np.array_equal(rows, tools.word_read_reference(p, S, t, depth, steps, width=width, unit=unit, **common))
                    assert st.keyswitch_launches == 0 and st.blind_rotate_launches == launches(depth, steps) and st.chunks == 1
                    look = ctx.lut_read(tg, t, depth, steps, amounts=tools.rotate_amounts(steps, unit=unit, N=N) if steps else None, coef=0, **common)
                    assert np.array_equal(ctx.word_read(tg, t, depth, steps, width=1, unit=unit, **common)[:, 0], look) and np.array_equal(got[:, 0], look)
        # no items: nothing to do
        assert ctx.word_read(tg, tables, 2, 5, width=3, unit=4, count=0).shape == (0, 3, p.n + 1)


@pytest.mark.parametrize("kw,gadget", SETS[:2], ids=IDS[:2])
def test_word_read_pieces_and_runs(ia, tuned, kw, gadget):
    """"cmux_piece_rows" caps of 1 and 3 (chunks == pieces), and the key switch's own cut inside a piece ("chunk" = 5 over
    items x 3 rows: runs that begin inside an item): the same words."""
    from ieache_amd import tools
    kb, ctx = tuned(**kw)
    p, S, tables, tg = prepared(ctx, kb, gadget)
    count = 5
    tof = np.array([1, 0, 1, 1, 0], dtype=np.int32)
    with tg:
        for depth, steps in ((0, 2), (2, 5)):
            sel = selectors(depth, steps, count)
            t = tables[:, :1 << depth]
            want = tools.word_read_reference(p, S, t, depth, steps, width=3, unit=4, sel_of=sel, table_of=tof, ksk=kb.ksk)
            for cap in (1, 3):
                for mfma_min in (FUSED, WALKED):
                    ctx.set_option("ks_mfma_min", mfma_min)
                    ctx.set_option("cmux_piece_rows", cap)
                    plan = ctx.cmux_plan(count, depth)
                    st = ia.Stats()
                    got = ctx.word_read(tg, t, depth, steps, width=3, unit=4, sel_of=sel, table_of=tof, stats=st)
                    ctx.set_option("cmux_piece_rows", 8192)
                    assert np.array_equal(got, want), (depth, steps, cap, mfma_min)
                    pieces = plan["pieces"]
                    assert pieces == -(-count // plan["items_per_piece"]) and pieces > 1
                    assert st.chunks == pieces and st.keyswitch_launches == pieces and st.blind_rotate_launches == pieces * launches(depth, steps)
            ctx.set_option("chunk", 5)
            st = ia.Stats()
            got = ctx.word_read(tg, t, depth, steps, width=3, unit=4, sel_of=sel, table_of=tof, stats=st)
            ctx.set_option("chunk", 65536)
            assert np.array_equal(got, want) and st.chunks == 1 and st.keyswitch_launches == 3 and st.blind_rotate_launches == launches(depth, steps)


def test_word_read_device_form_clamps_and_refuses(ia, tuned):
    import torch
    from ieache_amd import tools
    kb, ctx = tuned()
    p = kb.p
    S, tables = words(p.l, p.Bgbit)
    depth, steps, width, unit, count, n = 2, 5, 32, 32, 3, 5
    sel, tof = selectors(depth, steps, count), np.array([1, 0, 1], dtype=np.int32)
    want = tools.word_read_reference(p, S, tables, depth, steps, width=width, unit=unit, sel_of=sel, table_of=tof, ksk=kb.ksk)
    want_u = tools.word_read_reference(p, S, tables, depth, steps, width=width, unit=unit, sel_of=sel, table_of=tof)
    tS, tt, tsel, ttof = dev(S), dev(tables), dev(sel), dev(tof)
    tout = torch.full((count, width, ctx.lwe_stride), -1, dtype=torch.int32, device="cuda")
    tu = torch.full((count, width, ctx.extract_stride), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with ctx.tgsw_prepare_device(tS.data_ptr(), n) as S5:
        for mfma_min in (FUSED, WALKED):
            ctx.set_option("ks_mfma_min", mfma_min)
            tout.fill_(-1)
            torch.cuda.synchronize()
            st = ia.Stats()
            ctx.word_read_device(S5, count, depth, steps, width, unit, tsel.data_ptr(), tt.data_ptr(), 2, ttof.data_ptr(), tout.data_ptr(), stats=st)
            assert np.array_equal(tout.cpu().numpy()[:, :, :p.n + 1], want), mfma_min
            assert st.chunks == 1 and st.levels == depth + steps and st.blind_rotate_launches == launches(depth, steps) and st.keyswitch_launches == 1
        assert np.array_equal(tt.cpu().numpy(), tables) and np.array_equal(tsel.cpu().numpy(), sel)
        ctx.word_read_device(S5, count, depth, steps, width, unit, tsel.data_ptr(), tt.data_ptr(), 2, ttof.data_ptr(), tu.data_ptr(), keyswitch=False)
        assert np.array_equal(tu.cpu().numpy()[:, :, :N + 1], want_u)
        # the composition on the card's own calls, no reference involved
        picked = ctx.lut_tree(S5, tables, depth, sel_of=sel[:, steps:], table_of=tof)
        turned = ctx.tlwe_rotate(S5, picked, steps, sel_of=sel[:, :steps], amounts=tools.rotate_amounts(steps, unit=unit, N=N))
        assert np.array_equal(ctx.unpack(turned, 0, width, 1), want)
        # a warm host call allocates nothing
        ctx.word_read(S5, tables, depth, steps, width=width, unit=unit, sel_of=sel, table_of=tof)
        warm = ctx.get_option("staging_allocations")
        assert np.array_equal(ctx.word_read(S5, tables, depth, steps, width=width, unit=unit, sel_of=sel, table_of=tof), want)
        assert ctx.get_option("staging_allocations") == warm
        # explicit bad selectors and table indices are clamped on the device; the host form names the first
        bad, bad_tof = sel.copy(), np.array([2, -1, 1], dtype=np.int32)
        bad[0, 0], bad[1, 4], bad[2, 6] = 5, -1, 1 << 30
        tbad, tbtof = dev(bad), dev(bad_tof)
        torch.cuda.synchronize()
        ctx.word_read_device(S5, count, depth, steps, width, unit, tbad.data_ptr(), tt.data_ptr(), 2, tbtof.data_ptr(), tout.data_ptr())
        clamped = tools.word_read_reference(p, S, tables, depth, steps, width=width, unit=unit, sel_of=np.clip(bad, 0, n - 1), table_of=np.clip(bad_tof, 0, 1),
                                            ksk=kb.ksk)
        assert np.array_equal(tout.cpu().numpy()[:, :, :p.n + 1], clamped)
        for kws, match in ((dict(sel_of=bad, table_of=tof), r"word_read: sel_of\[0\] = 5"), (dict(sel_of=sel, table_of=bad_tof), r"word_read: table_of\[0\] = 2")):
            with pytest.raises(ia.IeacheError, match=match) as e:
                ctx.word_read(S5, tables, depth, steps, width=width, unit=unit, **kws)
            assert e.value.code == -22
        # refusals: the output over the tables, the selectors or the table indices, a host pointer, the scalars, in both forms
        for a in ((None, tt.data_ptr(), 2, None, tt.data_ptr() + 64), (tsel.data_ptr(), tt.data_ptr(), 2, None, tsel.data_ptr()),
                  (None, tt.data_ptr(), 2, ttof.data_ptr(), ttof.data_ptr())):
            with pytest.raises(ia.IeacheError, match="word_read: the output overlaps an input") as e:
                ctx.word_read_device(S5, count, depth, steps, width, unit, *a)
            assert e.value.code == -22
        with pytest.raises(ia.IeacheError, match="d_tables is not a device pointer") as e:
            ctx.word_read_device(S5, count, depth, steps, width, unit, None, tables.ctypes.data, 2, None, tout.data_ptr())
        assert e.value.code == -22
        with pytest.raises(ia.IeacheError, match="d_sel_of is not a device pointer") as e:
            ctx.word_read_device(S5, count, depth, steps, width, unit, sel.ctypes.data, tt.data_ptr(), 2, None, tout.data_ptr())
        assert e.value.code == -22
        with pytest.raises(ia.IeacheError, match="null argument") as e:
            ctx.word_read_device(S5, count, depth, steps, width, unit, None, None, 2, None, tout.data_ptr())
        assert e.value.code == -22
        for d, s, w, u, nt, match in ((-1, 0, 1, 1, 2, "word_read: depth must"), (13, 0, 1, 1, 2, "depth must"), (1, -1, 1, 1, 2, "word_read: steps must"),
                                      (1, 65, 1, 1, 2, "steps must"), (1, 0, 1, 1, 0, "word_read: n_tables must"), (1, 0, 0, 1, 2, "word_read: width must"),
                                      (1, 0, 4, 3, 2, "word_read: unit must"), (1, 3, 4, 129, 2, "exceed N"), (1, 11, 1, 1, 2, "exceed N"),
                                      (1, 6, 32, 32, 2, "word_read: unit x 2\\^steps must not exceed N")):
            with pytest.raises(ia.IeacheError, match=match) as e:
                ctx.word_read_device(S5, 1, d, s, w, u, None, tt.data_ptr(), nt, None, tout.data_ptr())
            assert e.value.code == -22
            if nt and d <= 2:  # (the host form takes n_tables from the array, and a depth-13 table is 64 MB)
                with pytest.raises(ia.IeacheError, match=match) as e:
                    ctx.word_read(S5, tables[:, :1 << max(d, 0)], d, s, width=w, unit=u)
                assert e.value.code == -22
        L = ia.lib()
        assert L.ieache_word_read_device(ctx.h, S5.h, 1, 1, 0, 1, 1, None, tt.data_ptr(), 2, None, 2, tout.data_ptr(), None) == -22
        assert "word_read: unknown flag" in L.ieache_last_error().decode()
        other = ia.Context.from_arrays(kb.p, kb.bk, kb.ksk)
        try:
            for f in (lambda: other.word_read_device(S5, 1, 1, 0, 1, 1, None, tt.data_ptr(), 2, None, tout.data_ptr()),
                      lambda: other.word_read(S5, tables[:, :2], 1, 0)):
                with pytest.raises(ia.IeacheError, match="another context") as e:
                    f()
                assert e.value.code == -22
        finally:
            other.close()
        assert np.array_equal(tout.cpu().numpy()[:, :, :p.n + 1], clamped)  # and no refused call wrote anything


def test_two_words_read_and_added_at_the_product_parameters(ia, gpu_ctx):
    """n = 630, (3, 7): the table of tests/test_unpack_cpu.py.  Two 16-bit words read at encrypted addresses through
    Context.word_read are the CPU reference's word for word and decrypt to the clear words; CIRC_ADD at 16 bits on the two read
    words decrypts to the clear sum mod 2^16.

    Measured on an MI355X (profiles/unpack_rates.txt): the largest distance of a read row's phase from +-1/8 is that file's
    "by meaning" line; a wrong bit needs 1/8."""
    from ieache_amd import tools
    from test_unpack_cpu import word_of, word_table, worst_phase_error
    kb, ctx = gpu_ctx(630, N)
    p = kb.p
    sc = word_table(p, kb.tlwe_key)
    depth, steps, width, unit = sc["depth"], sc["steps"], sc["width"], sc["unit"]
    sel = sc["sel_of"][:2]
    want = tools.word_read_reference(p, sc["samples"], sc["tables"], depth, steps, width=width, unit=unit, sel_of=sel, ksk=kb.ksk)
    with ctx.tgsw_prepare(sc["samples"]) as tg:
        got = ctx.word_read(tg, sc["tables"], depth, steps, width=width, unit=unit, sel_of=sel)
    assert got.shape == (2, 16, p.n + 1) and np.array_equal(got, want)
    clear = [int(sc["clear"][slot, word]) for slot, word in sc["addrs"][:2]]
    for i in range(2):
        print("read %d on the card: largest distance of a row's phase from +-1/8: %.3e (a wrong bit needs 1/8)" % (i, worst_phase_error(kb.lwe_key, got[i], clear[i])))
        assert word_of(kb.dec(got[i])) == clear[i]
    info = ia.circuit_info(ia.CIRC_ADD, 16)
    inp = np.concatenate([got[0], got[1], kb.enc(np.zeros(info.n_inputs - 32, dtype=np.uint8), 93).reshape(-1, p.n + 1)])[None]
    out = ctx.eval_batch(ia.CIRC_ADD, 16, inp)
    assert word_of(kb.dec(out[0])[:16]) == (clear[0] + clear[1]) % (1 << 16)
