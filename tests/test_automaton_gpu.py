"""Deterministic automata over words of TGSW-encrypted bits on the GPU (k_automaton_x1, csrc/automaton.hip; include/ieache.h
section 3k), word for word against the C reference (ieache_automaton_reference, which tests/test_automaton_cpu.py holds to the
numpy restatement) and, for the digit extremes, against the numpy restatement itself.  All at N = 1024: that is what the
kernels cover.  The bit-exact cases take random full-range words -- no encryption is needed for that; the last test runs
less_than(8) at the product parameters on client-encrypted letters, by meaning, through the extraction and the key switch."""
import numpy as np
import pytest

import automaton_reference as AR
import cmux_reference as CR

pytestmark = pytest.mark.gpu

N = 1024
G = 4  # waves per workgroup of k_automaton_x1 (kCmuxWaveRows, csrc/cmux_plan.h): states w, w + 4, .. of a step per wave
# (key's gadget, set's gadget or None for the key's): the two fixed builds and the run-time build
SETS = [({}, None), ({"l": 2, "Bgbit": 10}, None), ({}, (6, 5))]
IDS = ["l3_Bg7", "l2_Bg10", "l6_Bg5_rt"]

_words = {}


def words(l, Bgbit):
    """per gadget, made once and left unchanged: 5 full-range samples, 2 sets of finals of 9 rows"""
    key = (l, Bgbit)
    if key not in _words:
        rng = np.random.default_rng(9950 + 10 * l + Bgbit)
        _words[key] = (CR.full_range(rng, (5, 2 * l, 2, N)), CR.full_range(rng, (2, 9, 2, N)))
    return _words[key]


def tables(states, steps):
    """step-dependent random tables with self-loops and next0 == next1 entries; the same for every caller"""
    return AR.random_tables(np.random.default_rng(9960 + 100 * states + steps), steps, states)


def selectors(steps, count, n=5):
    """explicit indices [count][steps] into a set of n, repeats among them; the same for every caller"""
    rng = np.random.default_rng(9970 + 10 * count + steps)
    sel = rng.integers(0, n, size=(count, max(steps, 1))).astype(np.int32)
    sel[-1, :] = n - 1
    return sel


@pytest.fixture
def ctx_of(gpu_ctx):
    """gpu_ctx(4, 1024, ...) whose contexts get the piece cap and the steps per launch put back afterwards"""
    used = []

    def make(kw):
        kb, ctx = gpu_ctx(4, N, **kw)
        used.append(ctx)
        return kb, ctx

    yield make
    for ctx in used:
        ctx.set_option("cmux_piece_rows", 8192)
        ctx.set_option("automaton_steps_per_launch", 0)


def prepared(ctx, kb, gadget):
    """(the reference's parameters, the samples, the finals, the prepared set) of a case of SETS"""
    from ieache_amd import tools
    p = kb.p if gadget is None else tools.with_gadget(kb.p, *gadget)
    S, F = words(p.l, p.Bgbit)
    return p, S, F, (ctx.tgsw_prepare(S) if gadget is None else ctx.tgsw_prepare(S, *gadget))


@pytest.mark.parametrize("kw,gadget", SETS, ids=IDS)
def test_word_for_word(ia, ctx_of, kw, gadget):
    """states 1, 3, 4, 5, 9 (5 and 9 cross the round of G = 4 waves, with idle waves in the last round) x steps 0, 1, 2, 5 (1 reads
    the finals and writes the output with no scratch, 2 has no middle step, 5 uses the buffers in both parities) x count 1, 3 x
    n_out 1, states; selectors implied and explicit, one set of finals and two with final_of; the stats of section 3k."""
    from ieache_amd import tools
    kb, ctx = ctx_of(kw)
    p, S, F, tg = prepared(ctx, kb, gadget)
    with tg:
        at = 0
        for states in (1, 3, 4, 5, 9):
            for steps in (0, 1, 2, 5):
                next0, next1 = tables(states, steps)
                for n_out in (1, states):
                    with ctx.automaton(next0, next1, n_out) as a:
                        assert (a.states, a.steps, a.n_out) == (states, steps, n_out) and 0 <= a.cmuxes <= states * steps
                        for count in (1, 3):
                            explicit = at % 2 == 1
                            so = selectors(steps, count) if explicit else None
                            fo, fin = ((np.arange(count, dtype=np.int32) + 1) % 2, F[:, :states]) if at % 3 else (None, F[1:, :states])
                            want = tools.automaton_reference(p, S, next0, next1, fin, n_out=n_out, sel_of=so, final_of=fo, count=count)
                            st = ia.Stats()
                            got = ctx.automaton_run(tg, a, fin, sel_of=so, final_of=fo, count=count, stats=st)
                            assert got.shape == (count, n_out, 2, N) and np.array_equal(got, want), (states, steps, n_out, count, explicit)
                            assert st.bootstraps == 0 and st.keyswitch_launches == 0 and st.levels == steps and st.chunks == 1 and st.total_ms > 0
                            assert st.blind_rotate_launches == 1 and ctx.automaton_plan(a, count)["launches"] == 1
                            at += 1
        # no items: nothing, and nothing needed
        with ctx.automaton(*tables(3, 2)) as a:
            assert ctx.automaton_run(tg, a, F[:1, :3], count=0).shape == (0, 1, 2, N)


@pytest.mark.parametrize("kw,gadget", SETS, ids=IDS)
def test_chunking(ia, ctx_of, kw, gadget):
    """automaton_steps_per_launch 1, 2 and 0 give identical arrays -- with 1 the hand-off is a kernel boundary -- and the launch
    counts the plan reports."""
    from ieache_amd import tools
    kb, ctx = ctx_of(kw)
    p, S, F, tg = prepared(ctx, kb, gadget)
    states, steps, count = 5, 5, 3
    next0, next1 = tables(states, steps)
    sel = selectors(steps, count)
    want = tools.automaton_reference(p, S, next0, next1, F[:1, :states], n_out=2, sel_of=sel, count=count)
    with tg, ctx.automaton(next0, next1, 2) as a:
        for per, launches in ((1, 5), (2, 3), (0, 1), (5, 1), (4, 2)):
            ctx.set_option("automaton_steps_per_launch", per)
            plan = ctx.automaton_plan(a, count)
            st = ia.Stats()
            got = ctx.automaton_run(tg, a, F[:1, :states], sel_of=sel, count=count, stats=st)
            ctx.set_option("automaton_steps_per_launch", 0)
            assert np.array_equal(got, want), per
            assert plan["launches"] == launches and st.blind_rotate_launches == launches and st.chunks == 1 and st.levels == steps, per
        assert ctx.automaton_plan(a, count) == dict(pieces=1, items_per_piece=3, scratch_rows=30, steps_per_launch=5, launches=1)
    assert not ctx.set_option_ok("automaton_steps_per_launch", -1) and not ctx.set_option_ok("automaton_steps_per_launch", 4097)


@pytest.mark.parametrize("kw,gadget", SETS[:2], ids=IDS[:2])
def test_pieces(ia, ctx_of, kw, gadget):
    """cmux_piece_rows lowered so that every item is its own piece (a cap of 3 is below the 2 x 5 rows of one item, which still
    runs alone): the words are the same and chunks == count; with 2 steps per launch the launches multiply."""
    from ieache_amd import tools
    kb, ctx = ctx_of(kw)
    p, S, F, tg = prepared(ctx, kb, gadget)
    states, steps, count = 5, 5, 3
    next0, next1 = tables(states, steps)
    sel, fo = selectors(steps, count), np.array([1, 0, 1], dtype=np.int32)
    want = tools.automaton_reference(p, S, next0, next1, F[:, :states], n_out=states, sel_of=sel, final_of=fo)
    with tg, ctx.automaton(next0, next1, states) as a:
        for cap, per in ((3, 0), (10, 0), (19, 2)):
            ctx.set_option("cmux_piece_rows", cap)
            ctx.set_option("automaton_steps_per_launch", per)
            plan = ctx.automaton_plan(a, count)
            st = ia.Stats()
            got = ctx.automaton_run(tg, a, F[:, :states], sel_of=sel, final_of=fo, stats=st)
            ctx.set_option("cmux_piece_rows", 8192)
            ctx.set_option("automaton_steps_per_launch", 0)
            assert plan["pieces"] == count and plan["items_per_piece"] == 1 and plan["scratch_rows"] == 10
            assert np.array_equal(got, want), cap
            assert st.chunks == count and st.levels == steps and st.blind_rotate_launches == count * plan["launches"] == count * (3 if per else 1)
        assert ctx.automaton_plan(a, count)["pieces"] == 1


@pytest.mark.parametrize("kw,gadget", SETS[:2], ids=IDS[:2])
def test_a_tree_shaped_automaton_is_lut_tree(ia, ctx_of, kw, gadget):
    """next0 = 2 q, next1 = 2 q + 1 mod Q with the table as finals and the selectors in reverse level order is Context.lut_tree at
    depth 3, word for word: state 0 after three letters b0 b1 b2 is index 4 b0 + 2 b1 + b2, the tree's index with b2 its bit 0."""
    kb, ctx = ctx_of(kw)
    p, S, F, tg = prepared(ctx, kb, gadget)
    Q, depth, count = 8, 3, 3
    q = np.arange(Q, dtype=np.int32)
    next0, next1 = np.tile((2 * q) % Q, (depth, 1)), np.tile((2 * q + 1) % Q, (depth, 1))
    sel = selectors(depth, count)
    with tg, ctx.automaton(next0, next1) as a:
        assert a.cmuxes == 1 + 2 + 4
        got = ctx.automaton_run(tg, a, F[:, :Q], sel_of=sel[:, ::-1], final_of=[0, 1, 0])
        want = ctx.lut_tree(tg, F[:, :Q], depth, sel_of=sel, table_of=[0, 1, 0])
    assert np.array_equal(got[:, 0], want)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_hand_off_under_load(ia, ctx_of):
    """1 100 items -- more than twice the workgroups a device keeps resident (2 per CU) -- of 5 states and 6 steps, each with one
    of 3 selector sequences and the shared finals: many workgroups per CU, the reused scratch rows warm in L1.  The default run
    (every step in one launch, the hand-off inside the workgroup) equals the run with a launch per step in EVERY word, and the
    three distinct results are the reference's (90 reference CMuxes)."""
    import torch
    from ieache_amd import tools
    kb, ctx = ctx_of({})
    p = kb.p
    S, F = words(p.l, p.Bgbit)
    states, steps, count = 5, 6, 1100
    assert count >= 2 * 2 * ctx.get_option("cus")
    next0, next1 = tables(states, steps)
    seqs = selectors(steps, 3)
    which = np.arange(count) % 3
    sel = seqs[which]
    want = tools.automaton_reference(p, S, next0, next1, F[:1, :states], n_out=1, sel_of=seqs)
    tS, tF, tsel = dev(S), dev(F[:1, :states]), dev(sel)
    fused = torch.full((count, 1, 2, N), -1, dtype=torch.int32, device="cuda")
    stepwise = torch.full((count, 1, 2, N), -2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with ctx.tgsw_prepare_device(tS.data_ptr(), 5) as S5, ctx.automaton(next0, next1) as a:
        st = ia.Stats()
        ctx.automaton_run_device(S5, a, count, tsel.data_ptr(), tF.data_ptr(), 1, None, fused.data_ptr(), stats=st)
        assert st.chunks == ctx.automaton_plan(a, count)["pieces"] == 2 and st.blind_rotate_launches == 2
        ctx.set_option("automaton_steps_per_launch", 1)
        st = ia.Stats()
        ctx.automaton_run_device(S5, a, count, tsel.data_ptr(), tF.data_ptr(), 1, None, stepwise.data_ptr(), stats=st)
        ctx.set_option("automaton_steps_per_launch", 0)
        assert st.blind_rotate_launches == 2 * steps
    assert bool(torch.equal(fused, stepwise))
    got = fused.cpu().numpy()
    for s in range(3):
        assert np.array_equal(got[s], want[s]), s
    assert np.array_equal(got, want[which])


@pytest.mark.parametrize("kw,gadget", SETS[:2], ids=IDS[:2])
def test_digit_extremes_on_the_card(ia, ctx_of, kw, gadget):
    """Finals whose every digit is -2^(Bgbit-1) and 2^(Bgbit-1) - 1 (and zeros, so that the differences are those words) against
    samples of -2^31 and 2^31 - 1 throughout, two steps: the largest sums the two-limb spectrum meets, in the first step;
    against the numpy restatement."""
    kb, ctx = ctx_of(kw)
    p = kb.p
    lo, hi = CR.all_digits_word(p.l, p.Bgbit, -(1 << (p.Bgbit - 1))), CR.all_digits_word(p.l, p.Bgbit, (1 << (p.Bgbit - 1)) - 1)
    finals = np.stack([np.zeros((2, N), dtype=np.int32), np.full((2, N), lo, dtype=np.int32), np.full((2, N), hi, dtype=np.int32)])
    samples = np.stack([np.full((2 * p.l, 2, N), -(1 << 31), dtype=np.int32), np.full((2 * p.l, 2, N), (1 << 31) - 1, dtype=np.int32)])
    next0 = np.array([[0, 1, 2], [0, 0, 0]], dtype=np.int32)
    next1 = np.array([[1, 2, 0], [1, 2, 1]], dtype=np.int32)
    with ctx.tgsw_prepare(samples) as S, ctx.automaton(next0, next1, 3) as a:
        for sel in ([[0, 0]], [[1, 1]], [[0, 1]], [[1, 0]]):
            want = AR.run(samples, next0, next1, finals, p.l, p.Bgbit, n_out=3, sel_of=sel)
            assert np.array_equal(ctx.automaton_run(S, a, finals, sel_of=sel), want), sel


def test_device_form_clamps_and_refuses(ia, ctx_of):
    import torch
    from ieache_amd import tools
    kb, ctx = ctx_of({})
    p = kb.p
    S, F = words(p.l, p.Bgbit)
    states, steps, count, n = 4, 5, 3, 5
    next0, next1 = tables(states, steps)
    sel, fo, fin = selectors(steps, count), np.array([1, 0, 1], dtype=np.int32), F[:, :states]
    want = tools.automaton_reference(p, S, next0, next1, fin, n_out=2, sel_of=sel, final_of=fo)
    tS, tF, tsel, tfo = dev(S), dev(fin), dev(sel), dev(fo)
    tout = torch.full((count, 2, 2, N), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with ctx.tgsw_prepare_device(tS.data_ptr(), n) as S5, ctx.automaton(next0, next1, 2) as a:
        st = ia.Stats()
        ctx.automaton_run_device(S5, a, count, tsel.data_ptr(), tF.data_ptr(), 2, tfo.data_ptr(), tout.data_ptr(), stats=st)
        assert np.array_equal(tout.cpu().numpy(), want) and st.chunks == 1 and st.bootstraps == 0 and st.levels == steps and st.blind_rotate_launches == 1
        # the inputs as they were; a warm call allocates nothing
        assert np.array_equal(tF.cpu().numpy(), fin) and np.array_equal(tsel.cpu().numpy(), sel) and np.array_equal(tfo.cpu().numpy(), fo)
        first = ctx.automaton_run(S5, a, fin, sel_of=sel, final_of=fo)
        warm = ctx.get_option("staging_allocations")
        assert np.array_equal(ctx.automaton_run(S5, a, fin, sel_of=sel, final_of=fo), first) and np.array_equal(first, want)
        assert ctx.get_option("staging_allocations") == warm
        # explicit bad selectors and final_of are clamped on the device; the host form names the first
        bad = sel.copy()
        bad[0, 0], bad[1, 4], bad[2, 2] = 5, -1, 1 << 30
        badf = np.array([2, -1, 1 << 30], dtype=np.int32)
        tbad, tbadf = dev(bad), dev(badf)
        torch.cuda.synchronize()
        ctx.automaton_run_device(S5, a, count, tbad.data_ptr(), tF.data_ptr(), 2, tbadf.data_ptr(), tout.data_ptr())
        clamped = tools.automaton_reference(p, S, next0, next1, fin, n_out=2, sel_of=np.clip(bad, 0, n - 1), final_of=np.clip(badf, 0, 1))
        assert np.array_equal(tout.cpu().numpy(), clamped)
        for match, kwargs in ((r"sel_of\[0\] = 5", dict(sel_of=bad)), (r"final_of\[0\] = 2", dict(sel_of=sel, final_of=badf))):
            with pytest.raises(ia.IeacheError, match=match) as e:
                ctx.automaton_run(S5, a, fin, **kwargs)
            assert e.value.code == -22
        # refusals: any overlap of the output with the finals or an index array (there is no in-place form), a host pointer,
        # n_finals, nulls
        row = 2 * N * 4
        tbig = torch.zeros((2 * states + count * 2, 2, N), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for args in ((None, tbig.data_ptr(), 2, None, tbig.data_ptr()),
                     (None, tbig.data_ptr(), 2, None, tbig.data_ptr() + (2 * states - 1) * row),
                     (None, tbig.data_ptr() + row, 2, None, tbig.data_ptr()),
                     (tsel.data_ptr(), tF.data_ptr(), 2, None, tsel.data_ptr()),
                     (None, tF.data_ptr(), 2, tfo.data_ptr(), tfo.data_ptr())):
            with pytest.raises(ia.IeacheError, match="overlaps") as e:
                ctx.automaton_run_device(S5, a, count, *args)
            assert e.value.code == -22
        ctx.automaton_run_device(S5, a, count, None, tbig.data_ptr(), 2, None, tbig.data_ptr() + 2 * states * row)  # adjacent is no overlap
        with pytest.raises(ia.IeacheError, match="not a device pointer") as e:
            ctx.automaton_run_device(S5, a, count, None, fin.ctypes.data, 2, None, tout.data_ptr())
        assert e.value.code == -22
        with pytest.raises(ia.IeacheError, match="n_finals") as e:
            ctx.automaton_run_device(S5, a, count, None, tF.data_ptr(), 0, None, tout.data_ptr())
        assert e.value.code == -22
        for args in ((None, None, 2, None, tout.data_ptr()), (None, tF.data_ptr(), 2, None, None)):
            with pytest.raises(ia.IeacheError, match="null") as e:
                ctx.automaton_run_device(S5, a, count, *args)
            assert e.value.code == -22
        # a bad table is refused at compile time, by name
        worse = next1.copy()
        worse[3, 2] = states
        with pytest.raises(ia.IeacheError, match=r"next1\[3\]\[2\] = 4 is outside \[0, 4\)") as e:
            ctx.automaton(next0, worse)
        assert e.value.code == -22
        # a set or an automaton of another context
        other = ia.Context.from_arrays(kb.p, kb.bk, kb.ksk)
        try:
            with other.automaton(next0, next1, 2) as theirs, other.tgsw_prepare(S) as their_set:
                for f, match in ((lambda: other.automaton_run(S5, theirs, fin), "set was prepared on another context"),
                                 (lambda: other.automaton_run(their_set, a, fin), "automaton was compiled on another context"),
                                 (lambda: ctx.automaton_run_device(S5, theirs, count, None, tF.data_ptr(), 2, None, tout.data_ptr()), "automaton was compiled"),
                                 (lambda: other.automaton_plan(a, 1), "another context")):
                    with pytest.raises(ia.IeacheError, match=match) as e:
                        f()
                    assert e.value.code == -22
            late = other.automaton(next0, next1)
        finally:
            other.close()
        late.close()  # after its context
        assert np.array_equal(tout.cpu().numpy(), clamped)  # and no refused call wrote anything


def test_less_than_at_the_product_parameters(ia, gpu_ctx):
    """n = 630, (3, 7): less_than(8) on pairs that are equal, differ in one bit (the highest, the lowest) and differ anywhere, the
    letters encrypted with tools.tgsw_encrypt, the finals trivial +-1/8.  Before the key switch the phase of coefficient 0 is
    within 1/8 of its message -- the decoding distance of a +-1/8 message, where the sign flips: derived, not tuned -- and after
    tlwe_extract -> keyswitch decrypt_bits equals a < b.  The largest error observed goes into profiles/automaton_rates.txt
    beside the figure of DESIGN.md section 7 (scripts/automaton_rates.py records it; this test prints it)."""
    from ieache_amd import automata as A
    from ieache_amd import tools
    kb, ctx = gpu_ctx(630, N)
    p = kb.p
    bits = 8
    lt = A.less_than(bits)
    pairs = [(0, 0), (255, 255), (77, 77), (128, 0), (0, 128), (1, 0), (0, 1), (100, 101), (101, 100), (37, 200), (200, 37), (127, 128)]
    letters = np.stack([lt.word(a, b) for a, b in pairs])
    samples = tools.tgsw_encrypt(p, kb.tlwe_key, letters.reshape(-1).astype(np.int32), 77)
    with ctx.tgsw_prepare(samples) as tg, ctx.automaton(lt.next0, lt.next1) as a:
        assert (a.states, a.steps) == (5, 2 * bits)
        out = ctx.automaton_run(tg, a, A.final_rows(lt, N), count=len(pairs))  # implied selectors: letter t of item i is sample 16 i + t
    want = np.array([a < b for a, b in pairs])
    phase = tools.tlwe_phase(p, kb.tlwe_key, out[:, 0])[:, 0]
    message = np.where(want, 1 << 29, -(1 << 29))
    d = (phase.astype(np.int64) - message) & 0xFFFFFFFF
    err = np.minimum(d, (1 << 32) - d) / 2.0 ** 32
    print("less_than(8), 16 CMux steps on the card: largest phase error %.3e (decoding distance 1/8 = %.3e)" % (err.max(), 0.125))
    assert err.max() < 1 / 8
    rows = ctx.keyswitch(ctx.tlwe_extract(out[:, 0]))
    assert np.array_equal(tools.decrypt_bits(p, kb.lwe_key, rows).astype(bool), want)
