"""-m gpu: the three safety nets behind "approximate transform, exact product" -- the rounding guard, the sampled audit and the
repeat of the whole call on the two-limb kernels -- on products that are REALLY wrong, through every public entry point.

The inputs are the steered rows of tests/crafted_state.py (worst alignment with 24 random bits off every key word, l = 3 /
Bgbit = 7, n = 3, N = 1024, five rows, a uniform key-switching key) turned into operands of gates, gates3, mux, pbs, pbs_multi,
a netlist, a joint call and a device group by the builders tests/test_crafted_state_cpu.py proves on the oracle.  On them every
guarded one-limb kernel measures 0.5 and the unguarded build 35 returns wrong words (profiles/crafted_state.txt), so nothing
here is injected.  The random bits are those of bits_seed = 622, not of the 11 profiles/crafted_state.txt ran: which words
build 35 rounds wrongly depends on them, and an output reads one word of polynomial b only (below).  So: a guard that trips
did so on the kernel's own arithmetic, a mismatch the audit counts is a row that differs, and a repeat that did not recompute
everything on the two-limb kernels leaves a wrong output behind.

Every result is compared for equality with the CPU oracle.  Each call prints its figures ("safety-nets: ..." lines, `-s` /
`-rP`; profiles/safety_nets.txt is that table) before it asserts.

  Leg A   the guard trips for real: default choice and forced 31 / 32 / 36 / 43, audit off; reruns +1 per call, distance
          >= 1/16, the statistics those of ONE pass.
  Leg B   the audit finds a real difference: build 35 (no guard arithmetic), first without the audit -- the call HAS to return
          a wrong row, or the input shows nothing -- then with fft_audit = 1: mismatches >= 1, reruns +1, the oracle's words.
  Leg B2  the audit window: 200 rows of period 5; a 64-row window holds 12 or 13 copies of each row.
  Leg C   in-place calls cannot repeat: under build 35 they are exact from the start, unaudited.
  Leg D   the rotation of roles between w2r and w1b on 5 gates per CU of crafted rows.
  Old set l = 2 / Bgbit = 10 (worst alignment 0, sums of 2^52): set_option accepts the forcing on the flat path as on the debug
          hook (the choice is br_plan()'s either way), so the leg is here in full -- and wider than pbs and gates, see below.

WHAT THE RUNS FOUND (one MI355X; profiles/safety_nets.txt)
  * At l = 3 / Bgbit = 7 with the random bits of profiles/crafted_state.txt (bits_seed = 11) build 35's wrong words -- 3 per
    row, each the oracle's + 1, 15 per call of five rows: the "30 wrong words" of that profile over its calls after 2 and after
    all steps -- are coefficients 977, 1009 and 1019 of polynomial b of the accumulator.  They arise in step 1 (sums of 2^49.56)
    and step 2 leaves them where they are.  An extracted sample is polynomial a and coefficient 0 of b, and the key switch
    rounds a's words to 16 bits, so a last bit there is lost as well: NO gate, mux, pbs or circuit output shows such a word
    unless it is b[0].  On those rows leg B's precondition measured "wrong rows 0" at every entry point and failed, as it must.
  * So the random bits were searched for an input that does show something: build 35 through debug_blind_rotate on row 0 of
    worst_alignment(3, 7, 1024, 4, bits_seed = s) against the oracle, s = 0 .. 1635.  A seed leaves about one wrong word in each
    polynomial, near coefficients 0 and N - 1 where the sums peak; b[0] is wrong for s = 622 (17 wrong words of b: 0, 14, 19,
    46, 52 one low, twelve from 912 to 1019 one high; a right) and s = 1468 (45).  The legs run on 622: the same construction,
    the same sums, and under build 35 every blind rotation of a crafted row comes out one off in the word an output reads.
  * Every leg also runs at l = 2 / Bgbit = 10 ([l2-Bg10-...]), where build 35's first pass is wrong in every row of every entry
    point's output by far more than a bit.  There the audit counts the differing rows (5 of 5, 64 of a 64-row window, 71 over
    a joint call), the call repeats once and returns the oracle's words.
  * pbs_multi is the one entry point that reads the whole accumulator, and the audit compared plain extractions: under build 35
    the factors X^(N-977), X^(N-1009), X^(N-1019) returned wrong words, the audit counted 0 and the wrong output stood
    (test_audit_compares_the_accumulator_words_a_factor_reads, red before the fix).  BlindRotate::audit now compares whole
    accumulators for multi-output launches.
  * Context.kernel_for_launch named the any-parameter kernel until the context had made a call (legs D and old set); it now
    plans by the options as begin_call() does."""
import collections
import types

import numpy as np
import pytest

import crafted_state as CS
import multi_reference as MR
import np_tfhe
from random_netlists import oracle_netlist

pytestmark = pytest.mark.gpu

GUARD_LIMIT = 1.0 / 16          # past it a call repeats itself (README; kGuardLimit)
LEG_A = [("default", {}), ("31", dict(br_variant=31)), ("32", dict(br_variant=32)), ("36", dict(br_variant=36)), ("43", dict(br_variant=43))]
UNGUARDED = 35                  # k_blind_rotate_w1b without guard arithmetic: one limb, so the audit applies to it
FAMILIES = ("gates", "gates3", "mux", "pbs", "pbs_multi", "netlist", "jobs")
ADD_BITS, ADD_BATCH = 16, 2

# one entry-point call: run(target, stats) -> output(s); ref: the oracle's; one_pass: (bootstraps, levels, keyswitch_launches)
Call = collections.namedtuple("Call", "label run ref one_pass")


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _references(ia, O, case):
    """Everything the oracle says about the five crafted rows of `case`, computed once and read-only."""
    ck = CS.open_oracle(O, case.p, case.bk, case.ksk)
    x, N = case.x, case.p.N
    w = types.SimpleNamespace(case=case, ck=ck, x=x)
    w.ext = _frozen(np.stack([ck.bootstrap_woks(r) for r in x]))
    w.boot = _frozen(np.stack([ck.keyswitch(u) for u in w.ext]))
    w.poly = CS.pbs_constant_poly(N)
    # bootsMUX: half 0 row r, half 1 row r + 1, behind a selector of uniform words
    w.mux_ops = CS.mux_operands(x, np.roll(x, -1, axis=0), np_tfhe.uniform32(np.random.default_rng(21), x.shape))
    w.mux = _frozen(np.stack([ck.mux(*(o[r] for o in w.mux_ops)) for r in range(len(x))]))
    # multi-output: the factors 1 and X, a bias each
    w.factors = np.stack([MR.monomial(N, 0), MR.monomial(N, 1)])
    w.bias = np.array([1 << 27, -(1 << 30)], dtype=np.int32)
    w.multi = {ks: _frozen(np.stack([MR.multi_reference(ck, r, w.poly, w.factors, w.bias, keyswitch=ks) for r in x])) for ks in (True, False)}
    return w


# (l, Bgbit, alignment, bits_seed)
SETS = {"l3-Bg7": (3, 7, 4, CS.B0_BITS_SEED),  # the one-limb kernels' own set; random bits under which build 35 rounds b[0] wrongly
        "l2-Bg10": (2, 10, 0, 11),        # the old set, sums of 2^52: build 35 returns thousands of wrong words
        "l3-Bg7-seed11": (3, 7, 4, 11)}   # the rows of profiles/crafted_state.txt: wrong in three words of b no extraction reads
LEG_SETS = ("l3-Bg7", "l2-Bg10")


@pytest.fixture(scope="module")
def worlds(ia, O):
    """pset -> the case, its oracle references, the crafted netlist and the ADD job that shares the joint call: built on first
    use, shared and read-only."""
    made = {}

    def get(pset):
        if pset not in made:
            l, Bgbit, which, seed = SETS[pset]
            made[pset] = _world(ia, O, CS.worst_alignment(ia, l, Bgbit, 1024, which, ksk=CS.uniform_ksk(ia, 1024), bits_seed=seed))
        return made[pset]

    yield get
    for w in made.values():
        w.cn.close()


def _world(ia, O, case):
    w = _references(ia, O, case)
    w.cn = CS.crafted_netlist(ia)
    w.net_in = _frozen(CS.netlist_inputs(case.x)[None])
    w.net = _frozen(oracle_netlist(w, w.cn, w.net_in[0])[None])
    info = ia.circuit_info(ia.CIRC_ADD, ADD_BITS)
    w.add_info = info
    w.add_in = _frozen(np_tfhe.uniform32(np.random.default_rng(31), (ADD_BATCH, info.n_inputs, case.p.n + 1)))
    w.add = _frozen(np.stack([w.ck.add(r[:ADD_BITS], r[ADD_BITS:2 * ADD_BITS], r[2 * ADD_BITS:2 * ADD_BITS + 1], ADD_BITS)[0] for r in w.add_in]))
    return w


def _calls(ia, w, family, net_batch=1):
    """The entry-point calls of one family on the crafted rows."""
    x, rows = w.x, len(w.x)
    if family == "gates":
        for g, name in ((CS.GATE_OR, "OR"), (CS.GATE_AND, "AND"), (CS.GATE_NAND, "NAND"), (CS.GATE_XOR, "XOR")):
            a, b = CS.gate_operands(g, x)
            yield Call("gates " + name, lambda t, st, g=g, a=a, b=b: t.gates(g, a, b, stats=st), w.boot, (rows, 1, 1))
    elif family == "gates3":
        for g, name in ((CS.GATE_MAJ3, "MAJ3"), (CS.GATE_XOR3, "XOR3")):
            a, b, c = CS.gate_operands(g, x)
            yield Call("gates3 " + name, lambda t, st, g=g, a=a, b=b, c=c: t.gates3(g, a, b, c, stats=st), w.boot, (rows, 1, 1))
    elif family == "mux":  # two rotations and one key-switched row per gate
        yield Call("mux", lambda t, st: t.mux(*w.mux_ops, stats=st), w.mux, (2 * rows, 1, 1))
    elif family == "pbs":
        yield Call("pbs", lambda t, st: t.pbs(x, w.poly, stats=st), w.boot, (rows, 1, 1))
        yield Call("pbs, no key switch", lambda t, st: t.pbs(x, w.poly, keyswitch=False, stats=st), w.ext, (rows, 1, 0))
    elif family == "pbs_multi":
        for ks in (True, False):
            yield Call("pbs_multi, factors 1 and X, bias" + ("" if ks else ", no key switch"),
                       lambda t, st, ks=ks: t.pbs_multi(x, w.poly, w.factors, bias=w.bias, keyswitch=ks, stats=st), w.multi[ks], (rows, 1, 1 if ks else 0))
    elif family == "netlist":  # one piece per level
        rots = sum(g + m for g, m in CS.NETLIST_LEVEL_ITEMS)
        yield Call("eval_netlist", lambda t, st: t.eval_netlist(w.cn, np.repeat(w.net_in, net_batch, axis=0), st), np.repeat(w.net, net_batch, axis=0),
                   (rots * net_batch, 3, 3))
    elif family == "jobs":  # levels of the deeper job; a key switch per job and piece (test_jobs_gpu.py)
        rots, depth = sum(g + m for g, m in CS.NETLIST_LEVEL_ITEMS), w.add_info.sched_levels
        yield Call("eval_jobs [crafted netlist, ADD 16 x %d]" % ADD_BATCH,
                   lambda t, st: t.eval_jobs([(w.cn, np.repeat(w.net_in, net_batch, axis=0)), (ia.CIRC_ADD, ADD_BITS, w.add_in)], st),
                   [np.repeat(w.net, net_batch, axis=0), w.add], (rots * net_batch + w.add_info.bootstraps * ADD_BATCH, max(3, depth), 3 + depth))
    else:
        raise KeyError(family)


def _rows(out):
    """An output, or a joint call's list of them, as rows [.., words] padded to one width."""
    outs = out if isinstance(out, list) else [out]
    width = max(o.shape[-1] for o in outs)
    return np.concatenate([np.pad(o.reshape(-1, o.shape[-1]), ((0, 0), (0, width - o.shape[-1]))) for o in outs])


def _wrong_rows(out, ref):
    """Indices of the rows that differ from the oracle's."""
    return np.flatnonzero((_rows(out) != _rows(ref)).any(axis=1)).tolist()


def _open(ia, case, **options):
    ctx = ia.Context.from_arrays(case.p, case.bk, case.ksk)
    for k, v in options.items():
        ctx.set_option(k, v)
    return ctx


def _one_pass(st):
    return (st.bootstraps, st.levels, st.keyswitch_launches)


def _guard_trips(ia, ctx, leg, opts, call, one_pass=None):
    """Leg A on one call: the oracle's words, exactly one repeat, a published distance past the limit, one pass in the statistics."""
    st = ia.Stats()
    _, r0 = ctx.fft_guard()
    out = call.run(ctx, st)
    d1, r1 = ctx.fft_guard()
    wrong = _wrong_rows(out, call.ref)
    print("safety-nets: %s | %s | %s | distance %.4g | reruns +%d | wrong rows %d | stats %s" % (leg, opts, call.label, d1, r1 - r0, len(wrong), _one_pass(st)))
    assert not wrong, "%s, %s: rows %s differ from the oracle's after the repeat" % (call.label, opts, wrong)
    assert r1 == r0 + 1, "%s, %s: %d repeats of one call" % (call.label, opts, r1 - r0)
    assert d1 >= GUARD_LIMIT, "%s, %s: the guard published %.4g" % (call.label, opts, d1)
    assert _one_pass(st) == (one_pass or call.one_pass), "%s, %s: (bootstraps, levels, keyswitch_launches) are not one pass's" % (call.label, opts)


def _audit_finds(ia, ctx, leg, call):
    """Leg B on one call under build 35: wrong without the audit (the precondition), the oracle's words with it.
    -> (wrong rows of the precondition run, mismatches counted)."""
    ctx.set_option("br_variant", UNGUARDED)
    ctx.set_option("fft_audit", 0)
    r0 = ctx.fft_guard()[1]
    wrong = _wrong_rows(call.run(ctx, None), call.ref)
    print("safety-nets: %s | 35, no audit | %s | wrong rows %d %s | reruns +%d" % (leg, call.label, len(wrong), wrong[:8], ctx.fft_guard()[1] - r0))
    assert wrong, "PRECONDITION: %s under build 35 without the audit returned the oracle's words: this input no longer shows anything" % call.label
    assert ctx.fft_guard()[1] == r0, "build 35 has no guard arithmetic, yet the call repeated itself"
    ctx.set_option("fft_audit", 1)
    a0, r0 = ctx.fft_audit(), ctx.fft_guard()[1]
    out = call.run(ctx, None)
    a1, r1 = ctx.fft_audit(), ctx.fft_guard()[1]
    left = _wrong_rows(out, call.ref)
    print("safety-nets: %s | 35, fft_audit 1 | %s | audits +%d | gates compared +%d | mismatches +%d | reruns +%d | wrong rows %d" % (
        leg, call.label, a1["audits"] - a0["audits"], a1["gates_compared"] - a0["gates_compared"], a1["mismatches"] - a0["mismatches"], r1 - r0, len(left)))
    assert a1["mismatches"] - a0["mismatches"] >= 1, "%s: the audit compared %d rows of a call with wrong rows and counted none" % (
        call.label, a1["gates_compared"] - a0["gates_compared"])
    assert r1 == r0 + 1, "%s: %d repeats" % (call.label, r1 - r0)
    assert not left, "%s: rows %s differ from the oracle's after the repeat" % (call.label, left)
    return wrong, a1["mismatches"] - a0["mismatches"]


# ---- leg A: the guard trips for real ----

# the issue's set under every option, and the old set under the two forced kernels its debug-hook test runs (its default choice
# is the two-limb kernels: nothing trips there).  On the old set a first pass is wrong in the words every entry point returns
# (leg B), so equality with the oracle there is what tells a repeat on the two-limb kernels from one that was not.
LEG_A_CASES = [pytest.param("l3-Bg7", o, id="l3-Bg7-" + i) for i, o in LEG_A] + [pytest.param("l2-Bg10", o, id="l2-Bg10-" + i) for i, o in LEG_A[1:4:2]]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("pset,opts", LEG_A_CASES)
def test_guard_trips_on_the_kernels_own_arithmetic(ia, worlds, pset, opts, family):
    world = worlds(pset)
    with _open(ia, world.case, fft_audit=0, **opts) as ctx:
        for call in _calls(ia, world, family):
            _guard_trips(ia, ctx, "A " + pset, opts or "default", call)


@pytest.mark.parametrize("pset,opts", LEG_A_CASES)
def test_guard_trips_however_the_netlist_levels_are_cut(ia, worlds, pset, opts):
    """Level 0 (four gates and a MUX: six rotation items) in single items -- a MUX's two stay together: 5 + 3 + 2 pieces --, on
    one stream, and as halves on two streams (4 + 2 items; the levels of 4 and 2 items have no second half: joint_plan.h)."""
    world = worlds(pset)
    call = next(_calls(ia, world, "netlist"))
    for cut, pieces in ((dict(chunk=1), 10), (dict(overlap=0), 3), (dict(overlap_min=2), 4)):
        with _open(ia, world.case, fft_audit=0, **opts, **cut) as ctx:
            halves = ctx.get_option("overlapped_levels")
            _guard_trips(ia, ctx, "A " + pset, dict(opts, **cut), call, (call.one_pass[0], 3, pieces))
            assert (ctx.get_option("overlapped_levels") > halves) == ("overlap_min" in cut)


@pytest.mark.parametrize("pset,opts", [LEG_A_CASES[0], LEG_A_CASES[5]])
def test_guard_trips_on_every_member_of_a_group(ia, worlds, pset, opts):
    """Devices (0, 0): rows and expressions are cut 3 + 2 and 1 + 1, every member gets crafted rows, trips its own guard and
    repeats its own share once."""
    w = worlds(pset)
    with ia.Group.from_arrays(w.case.p, w.case.bk, w.case.ksk, (0, 0)) as g:
        g.set_option("fft_audit", 0)
        for k, v in opts.items():
            g.set_option(k, v)
        a, b = CS.gate_operands(CS.GATE_OR, w.x)
        rots, depth = sum(n + m for n, m in CS.NETLIST_LEVEL_ITEMS), w.add_info.sched_levels
        add = w.add_info.bootstraps
        calls = [(Call("group gates OR", lambda t, st: t.gates(CS.GATE_OR, a, b, stats=st), w.boot, None), [(3, 1, 1), (2, 1, 1)]),
                 (Call("group mux", lambda t, st: t.mux(*w.mux_ops, stats=st), w.mux, None), [(6, 1, 1), (4, 1, 1)]),
                 (Call("group pbs", lambda t, st: t.pbs(w.x, w.poly, stats=st), w.boot, None), [(3, 1, 1), (2, 1, 1)])]
        net2, jobs2 = next(_calls(ia, w, "netlist", 2)), next(_calls(ia, w, "jobs", 2))
        calls.append((Call("group " + net2.label, lambda t, st: net2.run(t, st), net2.ref, None), [(rots, 3, 3)] * 2))
        calls.append((Call("group " + jobs2.label, lambda t, st: jobs2.run(t, st), jobs2.ref, None), [(rots + add, max(3, depth), 3 + depth)] * 2))
        for call, shares in calls:
            stats = []
            before = [c.fft_guard()[1] for c in g.contexts]
            out = call.run(g, stats)
            after = [c.fft_guard() for c in g.contexts]
            wrong = _wrong_rows(out, call.ref)
            print("safety-nets: A " + pset + " | group (0, 0) | %s | distance %s | reruns %s | wrong rows %d | stats %s" % (
                call.label, [round(d, 4) for d, _ in after], [r - r0 for (_, r), r0 in zip(after, before)], len(wrong), [_one_pass(s) for s in stats]))
            assert not wrong, (call.label, wrong)
            assert [r for _, r in after] == [r0 + 1 for r0 in before], call.label
            assert all(d >= GUARD_LIMIT for d, _ in after), call.label
            assert [_one_pass(s) for s in stats] == shares, call.label


# ---- leg B: the audit finds a real difference ----

@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("pset", LEG_SETS)
def test_audit_counts_a_row_that_really_differs(ia, worlds, pset, family):
    """[l3-Bg7-*]: every blind rotation of a crafted row is one off in b[0] (module docstring); [l2-Bg10-*]: 5 of 5 rows wrong
    without the audit, mismatches +5 (mux +10, netlist +7 over 3 audits, joint call +71 over 48), reruns +1, the oracle's words.
    For pbs_multi the audit compares the rotation's accumulators, which every factor product is a function of (plain extractions
    do NOT suffice: test_audit_compares_the_accumulator_words_a_factor_reads).  For the joint call the audited part is audits % n_parts (BlindRotate::audit): the context is new and the
    precondition run makes no audit, so the first audited launch -- fft_audit = 1: the first launch, the step of the netlist's
    level 0 and the adder's level 1 -- has audits = 0, n_parts = 2 and takes part 0, the crafted netlist, which is the first job."""
    world = worlds(pset)
    with _open(ia, world.case) as ctx:
        for call in _calls(ia, world, family):
            assert ctx.fft_audit()["audits"] == 0 or family != "jobs"
            _audit_finds(ia, ctx, "B " + pset, call)


WRONG_B_COEFFICIENTS = (977, 1009, 1019)


def test_audit_compares_the_accumulator_words_a_factor_reads(ia, O, worlds):
    """What leg B found at l = 3 / Bgbit = 7 on the rows of bits_seed = 11: build 35's wrong words -- three per row, each the oracle's + 1 -- are
    coefficients 977, 1009 and 1019 of polynomial b of the accumulator (profiles/safety_nets.txt).  An extracted sample holds
    polynomial a and coefficient 0 of b, so gates, mux, pbs and circuits never see them -- but pbs_multi multiplies the whole
    accumulator: the factor X^(N - j) puts -b[j] into the b word of its output.  An audit that compares plain extractions finds
    nothing to count there and lets the wrong output through; it has to compare the accumulators (BlindRotate::audit)."""
    w = worlds("l3-Bg7-seed11")
    N = w.case.p.N
    factors = np.stack([MR.monomial(N, 0)] + [MR.monomial(N, N - j) for j in WRONG_B_COEFFICIENTS])
    ref = np.stack([MR.multi_reference(w.ck, r, w.poly, factors, None, keyswitch=False) for r in w.x])
    assert np.array_equal(ref[:, 0], w.ext)  # the factor 1 is the plain extraction
    call = Call("pbs_multi, no key switch, factors 1 and X^(N-j) for b's wrong coefficients j",
                lambda t, st: t.pbs_multi(w.x, w.poly, factors, keyswitch=False, stats=st), ref, None)
    with _open(ia, w.case) as ctx:
        wrong, _ = _audit_finds(ia, ctx, "B l3-Bg7-seed11, multi-output", call)
        assert not [i for i in wrong if i % 4 == 0], "the plain extractions were wrong too: rows %s" % wrong


@pytest.mark.parametrize("pset", LEG_SETS)
def test_audit_window_lies_on_the_rows_it_names(ia, worlds, pset):
    """Leg B2.  200 rows, row i = crafted row i % 5, one launch, one audit of 64 consecutive rows at an offset that moves.  Any
    64-row window of a period-5 tiling holds 12 or 13 copies of each row, so with w distinct wrong rows (0 < w < 5) the audit has
    to count between 12 w and 13 w; a compare of the wrong rows of `ext` against the sample would count about 64.  With w = 5
    every row of any window is wrong and only 60 <= count <= 64 can be asserted.
    Both sets: the wrong words arise in step 1, which the five rows share, so w = 5."""
    w = worlds(pset)
    x = np.tile(w.x, (40, 1))
    ref = np.tile(w.ext, (40, 1))
    call = Call("pbs, no key switch, 200 rows of period 5", lambda t, st: t.pbs(x, w.poly, keyswitch=False, stats=st), ref, None)
    with _open(ia, w.case) as ctx:
        wrong, counted = _audit_finds(ia, ctx, "B2 " + pset, call)
        distinct = sorted({i % 5 for i in wrong})
        print("safety-nets: B2 " + pset + " | distinct wrong rows %s of 5 | mismatches counted %d | audited rows %d" % (distinct, counted, ctx.fft_audit()["gates_compared"]))
        assert wrong == [i for i in range(200) if i % 5 in distinct], "copies of one row disagree on whether they are wrong"
        assert ctx.fft_audit()["audits"] == 1 and ctx.fft_audit()["gates_compared"] == 64
        if len(distinct) < 5:
            assert 12 * len(distinct) <= counted <= 13 * len(distinct), (distinct, counted)
        else:  # every row of every window is wrong: the window's position cannot show
            assert 60 <= counted <= 64, counted


# ---- leg C: in-place calls ----

def _device_rows(ctx, rows):
    import torch
    d = torch.zeros(rows.shape[:-1] + (ctx.lwe_stride,), dtype=torch.int32, device="cuda")
    d[..., : rows.shape[-1]] = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    return d


@pytest.mark.parametrize("pset", LEG_SETS)
def test_in_place_calls_are_exact_from_the_start(ia, worlds, pset):
    """The output over an input: the first pass would overwrite what a repeat has to read, so the call runs on the two-limb
    kernels at once -- under build 35, whose first pass is wrong on these rows (leg B), with no repeat and no audited launch."""
    import torch
    w = worlds(pset)
    S = w.case.p.n + 1
    a, b = CS.gate_operands(CS.GATE_NAND, w.x)
    with _open(ia, w.case, br_variant=UNGUARDED, fft_audit=1) as ctx:
        d_a, d_b, d_x, d_in = _device_rows(ctx, a), _device_rows(ctx, b), _device_rows(ctx, w.x), _device_rows(ctx, w.net_in)
        d_poly = torch.from_numpy(w.poly).cuda()
        torch.cuda.synchronize()
        calls = [("gates_device NAND over a", lambda: ctx.gates_device(CS.GATE_NAND, 5, d_a.data_ptr(), d_b.data_ptr(), d_a.data_ptr()), lambda: d_a, w.boot),
                 ("pbs_device over x", lambda: ctx.pbs_device(5, d_x.data_ptr(), d_poly.data_ptr(), 1, None, d_x.data_ptr()), lambda: d_x, w.boot),
                 ("eval_netlist_device over its inputs", lambda: ctx.eval_netlist_device(w.cn, 1, d_in.data_ptr(), d_in.data_ptr()),
                  lambda: d_in[:, :3], w.net)]
        for label, run, result, ref in calls:
            before = (ctx.fft_guard()[1], ctx.fft_audit())
            run()
            torch.cuda.synchronize()
            out = result().cpu().numpy()[..., :S]
            after = (ctx.fft_guard()[1], ctx.fft_audit())
            wrong = _wrong_rows(out, ref)
            print("safety-nets: C " + pset + " | 35, fft_audit 1 | %s | reruns +%d | audits +%d | wrong rows %d" % (
                label, after[0] - before[0], after[1]["audits"] - before[1]["audits"], len(wrong)))
            assert not wrong, (label, wrong)
            assert after == before, "%s: an in-place call repeated itself or was audited" % label
        assert np.array_equal(d_b.cpu().numpy()[:, :S], b) and np.array_equal(d_in.cpu().numpy()[0, 3:, :S], w.net_in[0, 3:])


# ---- leg D: rotation of roles ----

def test_guard_trips_inside_a_rotation_of_roles(ia, O):
    """5 gates per CU run as k_blind_rotate_w2r+w1b (mix_plan.h).  The smallest set at which they do is n = 6 with mix_s1 = 1
    (CS.smallest_mixing_set, checked for 256 and 304 CUs by the CPU file): the crafted step 1 then falls into the first phase, on
    two waves for two subsets and on one wave for the third."""
    n, s1 = CS.smallest_mixing_set(ia)
    case = CS.worst_alignment(ia, 3, 7, 1024, 4, n=n, ksk=CS.uniform_ksk(ia, 1024, n))
    ck = CS.open_oracle(O, case.p, case.bk, case.ksk)
    boot = np.stack([ck.bootstrap(r) for r in case.x])
    with _open(ia, case, fft_audit=0, mix_s1=s1) as ctx:
        cus = ctx.get_option("cus")
        gates = 5 * cus
        label = ctx.kernel_for_launch(gates)
        print("safety-nets: D | cus %d | n %d mix_s1 %d | %d gates -> %s" % (cus, n, s1, gates, label))
        assert "k_blind_rotate_w2r+w1b" in label, "no launch on this device mixes: %d gates on %d CUs take %s" % (gates, cus, label)
        a, b = CS.gate_operands(CS.GATE_OR, np.tile(case.x, (cus, 1)))
        call = Call("gates OR x %d as a rotation of roles" % gates, lambda t, st: t.gates(CS.GATE_OR, a, b, stats=st), np.tile(boot, (cus, 1)), (gates, 1, 1))
        mixed = ctx.get_option("mixed_launches")
        _guard_trips(ia, ctx, "D", "default, mix_s1 %d" % s1, call)
        assert ctx.get_option("mixed_launches") > mixed, "no launch on the device mixed"


# ---- the old parameter set ----

@pytest.fixture(scope="module")
def old_world(worlds):
    return worlds("l2-Bg10")


def test_old_parameter_set_accepts_the_forced_kernels(ia, old_world):
    """Legs A and B at this set are the [l2-Bg10-...] cases above (pbs and gates among them); here only that the flat path accepts
    the forcing, as the debug hook does: the context starts on the two-limb kernels and a forced number overrides that."""
    with _open(ia, old_world.case) as ctx:
        assert ctx.get_option("exact_fft") == 1 and ctx.kernel_for_launch(5).startswith("k_blind_rotate_wide<2,10>")
        for variant, name in ((31, "k_blind_rotate_w1b<2,10>"), (36, "k_blind_rotate_w2r<2,10>"), (UNGUARDED, "k_blind_rotate<2,10> br_variant 35")):
            assert ctx.set_option_ok("br_variant", variant), "set_option refuses br_variant %d at l = 2 / Bgbit = 10" % variant
            assert ctx.kernel_for_launch(5) == name


def test_audit_sample_comes_from_the_two_limb_kernels(ia, old_world):
    """The audit's own rotation has to be exact, whatever the launch took.  Forced here: build 24, the latency kernel on the
    ONE-limb spectrum -- the kernel an audit would compare with if br_exact_plan named it instead of its two-limb twin (7).  On
    sums of 2^52 its first pass differs from the exact words in every row; a sample from the same kernel would agree with it word
    for word and count nothing.  (Build 24 is guarded as well: guard and audit both ask for the repeat, and there is one.)"""
    w = old_world
    call = Call("pbs, no key switch, build 24", lambda t, st: t.pbs(w.x, w.poly, keyswitch=False, stats=st), w.ext, (5, 1, 0))
    with _open(ia, w.case, br_variant=24, fft_audit=1) as ctx:
        a0 = ctx.fft_audit()
        _guard_trips(ia, ctx, "B l2-Bg10, sample", dict(br_variant=24, fft_audit=1), call)
        a1 = ctx.fft_audit()
        print("safety-nets: B l2-Bg10, sample | 24, fft_audit 1 | audits +%d | gates compared +%d | mismatches +%d" % (
            a1["audits"] - a0["audits"], a1["gates_compared"] - a0["gates_compared"], a1["mismatches"] - a0["mismatches"]))
        assert a1["audits"] == a0["audits"] + 1 and a1["gates_compared"] == a0["gates_compared"] + 5
        assert a1["mismatches"] - a0["mismatches"] >= 1, "the audit's sample agrees with a one-limb first pass on sums of 2^52"
