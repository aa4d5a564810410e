"""The TLWE projection (k_window_digits, csrc/pack_keyswitch.hip) and the replace write of a window on the GPU (include/ieache.h
section 3l), word for word against the C references (ieache_tlwe_project_reference, ieache_lut_write_coef_reference, which
tests/test_project_cpu.py holds to the numpy restatement).  The bit-exact cases take random full-range words -- no encryption
is needed for that; the last test runs the three writes of tests/test_project_cpu.py at the product parameters, word for word
and by meaning."""
import numpy as np
import pytest

import cmux_reference as CR
import pack_reference as PR
import project_reference as JR

pytestmark = pytest.mark.gpu

N = 1024
T, B = 2, 2  # the decomposition of the bit-exact cases: K = N t = 2 048, 64 K steps
# (key's gadget, set's gadget or None for the key's): the two fixed builds and the run-time build
SETS = [({}, None), ({"l": 2, "Bgbit": 10}, None), ({}, (6, 5))]
IDS = ["l3_Bg7", "l2_Bg10", "l6_Bg5_rt"]

_made = {}


def once(key, make):
    if key not in _made:
        _made[key] = make()
    return _made[key]


def random_key(n_ring=N, t=T):
    return once(("key", n_ring, t), lambda: PR.full_range(np.random.default_rng(12000 + n_ring + t), (n_ring, t, 2, n_ring)))


def random_samples(n_ring=N):
    return once(("samples", n_ring), lambda: CR.full_range(np.random.default_rng(12010 + n_ring), (5, 2, n_ring)))


@pytest.fixture
def keyed(gpu_ctx):
    """gpu_ctx whose contexts get the options and the keys put back as they were found (no key) afterwards"""
    used = []

    def make(n=4, n_ring=N, **kw):
        kb, ctx = gpu_ctx(n, n_ring, **kw)
        used.append(ctx)
        return kb, ctx

    yield make
    for ctx in used:
        ctx.set_projection_key(None)
        ctx.set_packing_key(None)
        ctx.set_option("pack_piece_rows", 4096)
        ctx.set_option("cmux_piece_rows", 8192)


def windows(n_ring):
    """width 1, 3, 32, N x first 0, 5, N - width x dest 0, 7, N - 1, 2N - 1 (the last two cross the negacyclic wrap), the counts
    1, 3, 5 taken in turn so that every width meets every count"""
    out, at = [], 0
    for width in (1, 3, 32, n_ring):
        for first in sorted({0, min(5, n_ring - width), n_ring - width}):
            for dest in (0, 7, n_ring - 1, 2 * n_ring - 1):
                out.append((first, width, dest, (1, 3, 5)[at % 3]))
                at += 1
    return out


def test_windows_word_for_word(ia, keyed):
    from ieache_amd import tools
    kb, ctx = keyed()
    p, pk, samples = kb.p, random_key(), random_samples()
    ctx.set_projection_key(pk, t=T, basebit=B)
    seen = set()
    for first, width, dest, count in windows(N):
        seen.add((width, count))
        st = ia.Stats()
        got = ctx.tlwe_project(samples[:count], first, width, dest, stats=st)
        assert got.shape == (count, 2, N)
        assert np.array_equal(got, tools.tlwe_project_reference(p, pk, samples[:count], first, width, dest, t=T, basebit=B)), (first, width, dest, count)
        pieces = ctx.project_plan(count, width)["pieces"]
        assert pieces == (2 if count * width > 4096 else 1)
        assert st.bootstraps == 0 and st.levels == 1 and st.keyswitch_launches == pieces and st.chunks == pieces and st.total_ms > 0 and st.keyswitch_ms > 0
    assert seen == {(w, c) for w in (1, 3, 32, N) for c in (1, 3, 5)}
    # 5 x 32 rows cross a block of 128 rows; a repeated call gives identical arrays
    first5 = ctx.tlwe_project(samples, 5, 32, 7)
    assert np.array_equal(first5, tools.tlwe_project_reference(p, pk, samples, 5, 32, 7, t=T, basebit=B)) and np.array_equal(ctx.tlwe_project(samples, 5, 32, 7), first5)
    # one sample [2][N] is one item; no items: nothing to do
    assert np.array_equal(ctx.tlwe_project(samples[1], 5, 32, 7)[0], first5[1])
    st = ia.Stats()
    assert ctx.tlwe_project(samples[:0], 0, 1, 0, stats=st).shape == (0, 2, N) and st.keyswitch_launches == 0


def test_crafted_keys_and_digit_extremes(ia, keyed):
    """The keys whose words carry through every byte limb, and samples whose extracted rows have every digit at an extreme --
    on the entries the extraction copies AND on those it negates: A = w throughout makes u[i] = w for i <= c and -w above."""
    from ieache_amd import tools
    kb, ctx = keyed()
    p = kb.p
    prec = 1 << (31 - T * B)
    ones = (0xFFFFFFFF - prec) & 0xFFFFFFFF  # abar = all ones: every digit 2^b - 1
    words = np.array([ones, (-ones) & 0xFFFFFFFF, (-prec) & 0xFFFFFFFF, prec, 0x80000000, 0, 0x7FFFFFFF], dtype=np.uint32).view(np.int32)
    extreme = np.zeros((len(words), 2, N), dtype=np.int32)
    extreme[:, 0, :] = words[:, None]
    extreme[:, 1, :] = CR.full_range(np.random.default_rng(12100), (len(words), N))
    assert JR.window_rows(extreme[:2], 5, 1)[0, 0, 0] == words[0] and JR.window_rows(extreme[:2], 5, 1)[0, 0, 6] == words[1]
    assert (PR.digits(JR.window_rows(extreme[:1], 5, 1)[0], N, T, B)[0, :12] == 3).all() and (PR.digits(JR.window_rows(extreme[1:2], 5, 1)[0], N, T, B)[0, 12:] == 3).all()
    samples = random_samples()
    for name, key in dict(PR.crafted_keys(N, T, N), random=random_key()).items():
        ctx.set_projection_key(key, t=T, basebit=B)
        for rows, first, width, dest in ((samples[:3], 5, 3, 2 * N - 1), (extreme, 5, 3, N - 1), (extreme, N - 32, 32, 7)):
            got = ctx.tlwe_project(rows, first, width, dest)
            assert np.array_equal(got, tools.tlwe_project_reference(p, key, rows, first, width, dest, t=T, basebit=B)), (name, first, width, dest)
    # ... and against the numpy restatement itself, once
    assert np.array_equal(ctx.tlwe_project(extreme, 5, 3, N - 1), JR.project(random_key(), extreme, 5, 3, N - 1, T, B, fast=True))


def test_k_splits_pieces_and_the_other_decompositions(ia, keyed):
    from ieache_amd import tools
    kb, ctx = keyed()
    p, pk, samples = kb.p, random_key(), random_samples()
    ctx.set_projection_key(pk, t=T, basebit=B)
    want = tools.tlwe_project_reference(p, pk, samples[:3], 5, 32, N - 1, t=T, basebit=B)
    # forced K splits 1, 2, 4, 8 give identical words
    for split in (0, 1, 2, 4, 8):
        ctx.set_option("project_split", split)
        assert ctx.get_option("project_split") == split
        plan = ctx.project_plan(3, 32)
        assert plan["k_steps"] == N * T // 32 and plan["pieces"] == 1 and plan["items_per_piece"] == 3 and (plan["k_split"] == split if split else plan["k_split"] in (1, 2, 4, 8))
        assert np.array_equal(ctx.tlwe_project(samples[:3], 5, 32, N - 1), want), split
    assert not ctx.set_option_ok("project_split", 3) and not ctx.set_option_ok("project_split", 16)
    ctx.set_option("project_split", 8)
    ctx.set_projection_key(pk, t=T, basebit=B)  # a new key starts from the automatic choice
    assert ctx.get_option("project_split") == 0
    # "pack_piece_rows" lowered: two pieces, then one item per piece
    for piece_rows, pieces in ((4096, 1), (64, 2), (32, 3), (1, 3)):
        ctx.set_option("pack_piece_rows", piece_rows)
        st = ia.Stats()
        assert np.array_equal(ctx.tlwe_project(samples[:3], 5, 32, N - 1, stats=st), want), piece_rows
        assert ctx.project_plan(3, 32)["pieces"] == pieces and st.keyswitch_launches == pieces and st.chunks == pieces and st.levels == 1
    ctx.set_option("pack_piece_rows", 4096)
    # the same kernel for every accepted decomposition
    for t, b in ((8, 2), (4, 4), (5, 3)):
        key = random_key(N, t)
        ctx.set_projection_key(key, t=t, basebit=b)
        assert np.array_equal(ctx.tlwe_project(samples[:3], 1000, 3, 7), tools.tlwe_project_reference(p, key, samples[:3], 1000, 3, 7, t=t, basebit=b)), (t, b)


@pytest.mark.parametrize("t,b", [(8, 2), (2, 2)])
def test_projection_on_a_toy_ring(ia, keyed, t, b):
    """N = 64: the projection alone runs on any supported set."""
    from ieache_amd import tools
    kb, ctx = keyed(37, 64)
    p, n_ring = kb.p, 64
    pk, samples = random_key(n_ring, t), random_samples(n_ring)
    ctx.set_projection_key(pk, t=t, basebit=b)
    for first, width, dest, count in windows(n_ring):
        got = ctx.tlwe_project(samples[:count], first, width, dest)
        assert np.array_equal(got, tools.tlwe_project_reference(p, pk, samples[:count], first, width, dest, t=t, basebit=b)), (first, width, dest, count)
        assert np.array_equal(got, JR.project(pk, samples[:count], first, width, dest, t, b)), (first, width, dest, count)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_projection_keys_device_form_and_refusals(ia, keyed):
    import torch
    from ieache_amd import tools
    kb, ctx = keyed()
    p, pk, samples = kb.p, random_key(), random_samples()
    ctx.set_projection_key(None)  # nothing set: dropping is no error
    for f in (lambda: ctx.tlwe_project(samples, 0, 1, 0), lambda: ctx.project_plan(1, 1)):
        with pytest.raises(ia.IeacheError, match="no projection key set") as e:
            f()
        assert e.value.code == -22
    # independent of the packing key: a context may hold both, and dropping one leaves the other
    rows = PR.crafted_rows(np.random.default_rng(12200), 33, 4, 8, 2)
    lwe_pk = PR.full_range(np.random.default_rng(12201), (4, 8, 2, N))
    ctx.set_packing_key(lwe_pk)
    packed = ctx.pack(rows, spread=2, shift=3)
    ctx.set_projection_key(pk, t=T, basebit=B)
    want = tools.tlwe_project_reference(p, pk, samples, 5, 3, 7, t=T, basebit=B)
    assert np.array_equal(ctx.tlwe_project(samples, 5, 3, 7), want) and np.array_equal(ctx.pack(rows, spread=2, shift=3), packed)
    ctx.set_packing_key(None)
    assert np.array_equal(ctx.tlwe_project(samples, 5, 3, 7), want)
    ctx.set_packing_key(lwe_pk)
    # refused sets leave the key that is there in place; a second key replaces the first
    for t, b, match in ((16, 2, "below 32"), (8, 5, "pk_basebit"), (0, 2, "pk_t")):
        with pytest.raises(ia.IeacheError, match=match):
            ctx.set_projection_key(np.zeros((N, max(t, 1), 2, N), dtype=np.int32), t=t, basebit=b)
    with pytest.raises(ValueError):
        ctx.set_projection_key(pk[:-1], t=T, basebit=B)
    assert np.array_equal(ctx.tlwe_project(samples, 5, 3, 7), want)
    second = PR.crafted_keys(N, T, N)["varied"]
    ctx.set_projection_key(second, t=T, basebit=B)
    assert np.array_equal(ctx.tlwe_project(samples, 5, 3, 7), tools.tlwe_project_reference(p, second, samples, 5, 3, 7, t=T, basebit=B))
    ctx.set_projection_key(pk, t=T, basebit=B)
    # the device form
    tin, tout = dev(samples), torch.full((5, 2, N), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    st = ia.Stats()
    ctx.tlwe_project_device(5, 5, 3, 7, tin.data_ptr(), tout.data_ptr(), stats=st)
    assert np.array_equal(tout.cpu().numpy(), want) and np.array_equal(tin.cpu().numpy(), samples) and st.keyswitch_launches == 1 and st.chunks == 1
    ctx.tlwe_project_device(0, 5, 3, 7, tin.data_ptr(), tout.data_ptr())  # no items: a no-op
    # a warm host call allocates nothing
    warm = ctx.get_option("staging_allocations")
    ctx.tlwe_project(samples, 5, 3, 7)
    assert ctx.get_option("staging_allocations") == warm
    # refusals, all before anything is launched
    tbig = torch.zeros((6, 2, N), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for d_in, d_out in ((tbig.data_ptr(), tbig.data_ptr()), (tbig.data_ptr(), tbig.data_ptr() + 8 * N), (tbig.data_ptr() + 8 * N, tbig.data_ptr())):
        with pytest.raises(ia.IeacheError, match="overlaps") as e:
            ctx.tlwe_project_device(5, 5, 3, 7, d_in, d_out)
        assert e.value.code == -22
    with pytest.raises(ia.IeacheError, match="not a device pointer") as e:
        ctx.tlwe_project_device(5, 5, 3, 7, samples.ctypes.data, tout.data_ptr())
    assert e.value.code == -22
    for bad, match in (((-1, 1, 0), "first must"), ((N, 1, 0), "first must"), ((0, 0, 0), "width must"), ((5, N - 4, 0), "exceed N"), ((0, N + 1, 0), "exceed N"),
                       ((0, 1, 2 * N), "dest must"), ((0, 1, -1), "dest must")):
        for f in (lambda: ctx.tlwe_project_device(5, bad[0], bad[1], bad[2], tin.data_ptr(), tout.data_ptr()), lambda: ctx.tlwe_project(samples, *bad)):
            with pytest.raises(ia.IeacheError, match=match) as e:
                f()
            assert e.value.code == -22
    assert np.array_equal(tout.cpu().numpy(), want)  # and no refused call wrote anything
    assert ctx.tlwe_project(samples, N - 1, 1, 2 * N - 1).shape == (5, 2, N)


# ---- the replace write of a window ----
_words = {}


def words(l, Bgbit):
    """per gadget, made once and left unchanged: 5 full-range samples, 5 new rows, 5 memories of 4 rows"""
    key = (l, Bgbit)
    if key not in _words:
        rng = np.random.default_rng(12300 + 10 * l + Bgbit)
        _words[key] = (CR.full_range(rng, (5, 2 * l, 2, N)), CR.full_range(rng, (5, 2, N)), CR.full_range(rng, (5, 4, 2, N)))
    return _words[key]


def selectors(depth, steps, count, n=5):
    rng = np.random.default_rng(12310 + 100 * depth + 10 * count + steps)
    sel = rng.integers(0, n, size=(count, max(depth + steps, 1))).astype(np.int32)
    sel[-1, :] = n - 1
    return sel


def prepared(ctx, kb, gadget):
    from ieache_amd import tools
    p = kb.p if gadget is None else tools.with_gadget(kb.p, *gadget)
    S, new, mem = words(p.l, p.Bgbit)
    return p, S, new, mem, (ctx.tgsw_prepare(S) if gadget is None else ctx.tgsw_prepare(S, *gadget))


def launches(depth, steps):
    return 2 * max(depth, 1) + 2 * (1 if steps else 0) + 1


@pytest.mark.parametrize("kw,gadget", SETS, ids=IDS)
def test_write_word_for_word(ia, keyed, kw, gadget):
    """depth 0, 1, 2 x steps 0, 3 x width 1, 4 x counts 1, 3, 5 (5 crosses a workgroup of 4 rows); selectors implied and
    explicit in turn; unit = width and a wider unit; the stats of section 3l."""
    from ieache_amd import tools
    kb, ctx = keyed(**kw)
    pk = random_key()
    ctx.set_projection_key(pk, t=T, basebit=B)
    p, S, new, mem, tg = prepared(ctx, kb, gadget)
    with tg:
        at = 0
        for depth in (0, 1, 2):
            for steps in (0, 3):
                for width in (1, 4):
                    for count in (1, 3, 5):
                        sel = selectors(depth, steps, count) if at % 2 else None
                        unit = None if at % 3 else 2 * width
                        at += 1
                        m = mem[:count, :1 << depth]
                        want = tools.lut_write_coef_reference(p, S, pk, m, depth, steps, new[:count], width=width, unit=unit, sel_of=sel, t=T, basebit=B)
                        st = ia.Stats()
                        got = ctx.lut_write_coef(tg, m, depth, steps, new[:count], width=width, unit=unit, sel_of=sel, stats=st)
                        assert got.shape == (count, 1 << depth, 2, N) and np.array_equal(got, want), (depth, steps, width, unit, count)
                        assert st.bootstraps == 0 and st.levels == 2 * (depth + steps) + 1 and st.chunks == 1 and st.keyswitch_launches == 1
                        assert st.blind_rotate_launches == launches(depth, steps) and st.total_ms > 0
        # no items: nothing to do
        assert ctx.lut_write_coef(tg, mem[:0, :2], 1, 3, new[:0], width=4).shape == (0, 2, 2, N)


@pytest.mark.parametrize("kw,gadget", SETS[:2], ids=IDS[:2])
def test_write_one_item_per_piece(ia, keyed, kw, gadget):
    """Tree pieces of one item ("cmux_piece_rows" = 1), and the projection's own cut inside a piece ("pack_piece_rows" = 4: one
    item of width 4 per run): the same words."""
    from ieache_amd import tools
    kb, ctx = keyed(**kw)
    pk = random_key()
    ctx.set_projection_key(pk, t=T, basebit=B)
    p, S, new, mem, tg = prepared(ctx, kb, gadget)
    with tg:
        for depth, steps, count in ((0, 0, 3), (1, 3, 5), (2, 3, 3)):
            sel = selectors(depth, steps, count)
            m = mem[:count, :1 << depth]
            want = tools.lut_write_coef_reference(p, S, pk, m, depth, steps, new[:count], width=4, sel_of=sel, t=T, basebit=B)
            ctx.set_option("cmux_piece_rows", 1)
            st = ia.Stats()
            got = ctx.lut_write_coef(tg, m, depth, steps, new[:count], width=4, sel_of=sel, stats=st)
            assert ctx.cmux_plan(count, depth)["pieces"] == count
            ctx.set_option("cmux_piece_rows", 8192)
            assert np.array_equal(got, want), (depth, steps, count)
            assert st.chunks == count and st.keyswitch_launches == count and st.blind_rotate_launches == count * launches(depth, steps)
            ctx.set_option("pack_piece_rows", 4)
            st = ia.Stats()
            got = ctx.lut_write_coef(tg, m, depth, steps, new[:count], width=4, sel_of=sel, stats=st)
            ctx.set_option("pack_piece_rows", 4096)
            assert np.array_equal(got, want) and st.chunks == 1 and st.keyswitch_launches == count and st.blind_rotate_launches == launches(depth, steps)


def test_write_device_form_in_place_clamps_and_refuses(ia, keyed):
    import torch
    from ieache_amd import tools
    kb, ctx = keyed()
    p, pk = kb.p, random_key()
    S, new, mem = words(p.l, p.Bgbit)
    depth, steps, width, unit, count, n = 2, 3, 4, 8, 5, 5
    sel = selectors(depth, steps, count)
    want = tools.lut_write_coef_reference(p, S, pk, mem, depth, steps, new, width=width, unit=unit, sel_of=sel, t=T, basebit=B)
    tS, tnew, tsel, tmem = dev(S), dev(new), dev(sel), dev(mem)
    tout = torch.full((count, 4, 2, N), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with ctx.tgsw_prepare_device(tS.data_ptr(), n) as S5:
        args = (tsel.data_ptr(), tnew.data_ptr(), tmem.data_ptr(), tout.data_ptr())
        with pytest.raises(ia.IeacheError, match="no projection key set") as e:
            ctx.lut_write_coef_device(S5, count, depth, steps, width, unit, *args)
        assert e.value.code == -22
        ctx.set_projection_key(pk, t=T, basebit=B)
        # into a second buffer: the memory, the new rows and the selectors as they were
        st = ia.Stats()
        ctx.lut_write_coef_device(S5, count, depth, steps, width, unit, *args, stats=st)
        assert np.array_equal(tout.cpu().numpy(), want) and np.array_equal(tmem.cpu().numpy(), mem)
        assert st.chunks == 1 and st.levels == 2 * (depth + steps) + 1 and st.blind_rotate_launches == launches(depth, steps) and st.keyswitch_launches == 1
        # the composition on the card's own calls, no reference involved
        picked = ctx.lut_tree(S5, mem, depth, sel_of=sel[:, steps:], table_of=np.arange(count, dtype=np.int32), count=count)
        turned = ctx.tlwe_rotate(S5, picked, steps, sel_of=sel[:, :steps], amounts=tools.rotate_amounts(steps, unit=unit, N=N))
        delta = PR._wrap32(new.astype(np.int64) - ctx.tlwe_project(turned, 0, width, 0))
        composed = ctx.lut_add(S5, delta, depth, steps, sel_of=sel, amounts=tools.rotate_amounts(steps, unit=unit, toward_zero=False, N=N), mems=mem,
                               mem_of=np.arange(count, dtype=np.int32))
        assert np.array_equal(composed, want)
        # in place; a repeated call from the same memory gives identical arrays
        ctx.lut_write_coef_device(S5, count, depth, steps, width, unit, tsel.data_ptr(), tnew.data_ptr(), tmem.data_ptr(), tmem.data_ptr())
        assert np.array_equal(tmem.cpu().numpy(), want)
        assert np.array_equal(tnew.cpu().numpy(), new) and np.array_equal(tsel.cpu().numpy(), sel)
        tmem.copy_(dev(mem))
        torch.cuda.synchronize()
        # a warm host call allocates nothing
        ctx.lut_write_coef(S5, mem, depth, steps, new, width=width, unit=unit, sel_of=sel)
        warm = ctx.get_option("staging_allocations")
        assert np.array_equal(ctx.lut_write_coef(S5, mem, depth, steps, new, width=width, unit=unit, sel_of=sel), want)
        assert ctx.get_option("staging_allocations") == warm
        # explicit bad selectors are clamped on the device; the host form names the first
        bad = sel.copy()
        bad[0, 0], bad[1, 4], bad[2, 2] = 5, -1, 1 << 30
        tbad = dev(bad)
        torch.cuda.synchronize()
        ctx.lut_write_coef_device(S5, count, depth, steps, width, unit, tbad.data_ptr(), tnew.data_ptr(), tmem.data_ptr(), tout.data_ptr())
        clamped = tools.lut_write_coef_reference(p, S, pk, mem, depth, steps, new, width=width, unit=unit, sel_of=np.clip(bad, 0, n - 1), t=T, basebit=B)
        assert np.array_equal(tout.cpu().numpy(), clamped)
        with pytest.raises(ia.IeacheError, match=r"sel_of\[0\] = 5") as e:
            ctx.lut_write_coef(S5, mem, depth, steps, new, width=width, unit=unit, sel_of=bad)
        assert e.value.code == -22
        # refusals: a partly overlapping output, the output over the new rows or the selectors, a host pointer, the scalars
        row = 2 * N * 4
        tbig = torch.zeros((2 * count, 4, 2, N), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for a in ((None, tnew.data_ptr(), tbig.data_ptr(), tbig.data_ptr() + row), (None, tnew.data_ptr(), tbig.data_ptr() + row, tbig.data_ptr()),
                  (None, tbig.data_ptr() + 2 * row, tmem.data_ptr(), tbig.data_ptr()), (tsel.data_ptr(), tnew.data_ptr(), tmem.data_ptr(), tsel.data_ptr())):
            with pytest.raises(ia.IeacheError, match="overlaps") as e:
                ctx.lut_write_coef_device(S5, count, depth, steps, width, unit, *a)
            assert e.value.code == -22
        with pytest.raises(ia.IeacheError, match="not a device pointer") as e:
            ctx.lut_write_coef_device(S5, count, depth, steps, width, unit, None, new.ctypes.data, tmem.data_ptr(), tout.data_ptr())
        assert e.value.code == -22
        # a host address for the selectors is refused like any other, even where none would be read (depth = steps = 0)
        with pytest.raises(ia.IeacheError, match="d_sel_of is not a device pointer") as e:
            ctx.lut_write_coef_device(S5, 1, 0, 0, 1, 1, sel.ctypes.data, tnew.data_ptr(), tmem.data_ptr(), tout.data_ptr())
        assert e.value.code == -22
        for d, s, w, u, match in ((-1, 0, 1, 1, "depth must"), (13, 0, 1, 1, "depth must"), (1, -1, 1, 1, "steps must"), (1, 65, 1, 1, "steps must"),
                                  (1, 0, 0, 1, "width must"), (1, 0, 4, 3, "unit must"), (1, 3, 4, 129, "exceed N"), (1, 11, 1, 1, "exceed N")):
            with pytest.raises(ia.IeacheError, match=match) as e:
                ctx.lut_write_coef_device(S5, 1, d, s, w, u, None, tnew.data_ptr(), tmem.data_ptr(), tout.data_ptr())
            assert e.value.code == -22
        other = ia.Context.from_arrays(kb.p, kb.bk, kb.ksk)
        try:
            with pytest.raises(ia.IeacheError, match="another context") as e:
                other.lut_write_coef_device(S5, 1, 1, 0, 1, 1, None, tnew.data_ptr(), tmem.data_ptr(), tout.data_ptr())
            assert e.value.code == -22
        finally:
            other.close()
        assert np.array_equal(tout.cpu().numpy(), clamped)  # and no refused call wrote anything


def test_three_writes_at_the_product_parameters(ia, gpu_ctx):
    """n = 630, (3, 7), the projection key at (8, 2): the three successive writes of tests/test_project_cpu.py through
    Context.lut_write_coef -- each memory is the CPU reference's word for word, every written word within 2^-8 of `new` and every
    other coefficient within 2^-8 of what it held (phases read with tools.tlwe_phase), and a written bit comes back through
    lut_read and decrypt_bits."""
    from ieache_amd import tools
    from test_project_cpu import WRITES, three_writes, torus_distance
    kb, ctx = gpu_ctx(630, N)
    p = kb.p
    pk = tools.projection_keygen(p, kb.tlwe_key, seed=71)
    sc = three_writes(p, kb.tlwe_key, pk)
    depth, steps, width, unit = sc["depth"], sc["steps"], sc["width"], sc["unit"]
    ctx.set_projection_key(pk)
    try:
        with ctx.tgsw_prepare(sc["samples"]) as tg:
            mem = sc["mem0"]
            for i in range(3):
                mem = ctx.lut_write_coef(tg, mem, depth, steps, sc["new"][i], width=width, unit=unit, sel_of=sc["sel_of"][i:i + 1])
                assert mem.shape == (1, 4, 2, N) and np.array_equal(mem, sc["mems"][i]), i
                err = torus_distance(tools.tlwe_phase(p, kb.tlwe_key, mem[0]), sc["want"][i])
                slot, word = WRITES["addrs"][i]
                print("write %d on the card: largest phase error %.3e on the written word, %.3e over the memory (bound 2^-8 = %.3e)"
                      % (i, err[slot, word * unit:word * unit + width].max(), err.max(), 2.0 ** -8))
                assert err.max() < 2.0 ** -8
            # a coefficient of the last written word well away from 0 and 1/2, read at the same encrypted address
            q = next(int(c) for c in range(width) if 4 << 26 <= abs(int(sc["words"][2][c])) <= 28 << 26)
            read = ctx.lut_read(tg, mem, depth, steps, sel_of=sc["sel_of"][2:3], amounts=tools.rotate_amounts(steps, unit=unit, N=N), coef=q)
            assert read.shape == (1, p.n + 1) and kb.dec(read)[0] == (1 if sc["words"][2][q] > 0 else 0)
    finally:
        ctx.set_projection_key(None)
