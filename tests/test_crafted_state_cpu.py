"""The constructions of tests/crafted_state.py, proved on the CPU before a kernel sees them.

For every case, on the ring it will run at: the accumulator after the steering step is the target; the digits that enter the
crafted step -- restated here from the oracle's own state -- are the claimed ones; the largest exact sum of that step is the
claimed power of two; and the oracle (Goldilocks NTT) and the numpy restatement (int64 convolutions; both exact below 2^62)
agree word for word after every step.  A construction that cannot meet its claim has no place in the GPU file.

What could not be built as first stated, and what stands in its place:
  - l = 1 at the largest Bgbit of a ring, and l x Bgbit = 32: a steered accumulator is the test vector plus a multiple of
    2^(Bgbit-2), so the low Bgbit-1 bits of the decomposed word are fixed and "half - 1" is out of reach for the digits whose
    field covers them.  Those digits take the largest reachable value (Case.pos, asserted below); -half is reachable everywhere.
  - the steering step has amount 1 (acc += d0 x key block, coefficient by coefficient) rather than amount N with a (1 - X) Q
    key: half the granularity, without which "every digit at -half" cannot be reached at (2, 16).
What was added: a fifth worst-alignment input with 24 random bits taken off every key word, because on constant keys the
transform's half-integer outputs all tie to the even exact sum and an unguarded kernel is right by luck.

The last section proves the operand builders tests/test_safety_nets_gpu.py feeds the public entry points with: on the oracle
alone, every builder's gate is the bootstrap of the crafted row it was built for, its blind rotation is the one
oracle_accumulators gives for that row, and the crafted netlist's level 0 bootstraps exactly the crafted rows."""
import hashlib
import types

import numpy as np
import pytest

import crafted_state as CS
import lut_reference as LR
import np_tfhe
import param_lattice as PL
from random_netlists import oracle_gate, oracle_netlist

W64_SETS = [(3, 7, 1024), (2, 10, 1024)]
ALL_SETS = W64_SETS + CS.generic_edge_sets()


def _walk(O, case):
    """Oracle and numpy restatement side by side over every step of every row; -> the oracle's accumulators [rows][n+1][2][N]."""
    p = case.p
    ck = CS.open_oracle(O, p, case.bk, case.ksk)
    bk = np.asarray(case.bk).reshape(p.n, 2 * p.l, 2, p.N)
    out = []
    for r, row in enumerate(case.x):
        bara, barb = ck.modswitch(row)
        acc = ck.blind_rotate_init(barb)
        mine = np.stack([np.zeros(p.N, np.int32), np_tfhe._mul_by_xai(np.full(p.N, CS.MU, np.int32), (2 * p.N - barb) % (2 * p.N))])
        assert np.array_equal(acc, mine), (r, "init")
        accs = [acc]
        for i in range(p.n):
            acc = ck.blind_rotate_step(acc, i, bara[i])
            mine = CS.np_step(mine, bk[i], int(bara[i]), p.l, p.Bgbit)
            assert np.array_equal(acc, mine), (case.name, r, i)
            accs.append(acc)
        out.append(accs)
    return ck, out


def _steered_ids(sets):
    return [pytest.param(l, B, N, cid, id="l%d-Bg%d-N%d-%s" % (l, B, N, cid)) for l, B, N in sets
            for cid, _ in CS.steered_cases(None, l, B, N)]


@pytest.mark.parametrize("l,Bgbit,N,cid", _steered_ids(ALL_SETS))
def test_steered_case_is_what_it_claims(ia, O, l, Bgbit, N, cid):
    assert PL.br_exact(l, Bgbit, N)
    case = dict(CS.steered_cases(ia, l, Bgbit, N))[cid]()
    p, half = case.p, 1 << (Bgbit - 1)
    assert (p.n, case.x.shape) == (3, (5, 4)) and not case.ksk.any() and case.ksk.size == p.ksk_count
    ck, accs = _walk(O, case)
    for r, a in enumerate(accs):
        bara, barb = ck.modswitch(case.x[r])
        assert barb == 0 and bara[0] == 1 and bara[1] == N
        assert np.array_equal(a[1], case.target), r                                      # step 0 steers to the target
        dig = CS.np_step_digits(a[1], N, l, Bgbit)                                         # what step 1 decomposes
        assert np.array_equal(dig, case.digits), r
    assert sorted(int(case.x[r, 2]) for r in range(5)) == sorted(CS.amount_word(a, N) for a in (0, 1, N, 2 * N - 1, 513 % (2 * N)))
    # the digits are the extremes: -half always; half - 1 wherever the field lies above the fixed low bits
    dig = case.digits
    assert list(case.neg) == [-half] * (2 * l)
    for q in range(2 * l):
        lsb = 32 - (q % l + 1) * Bgbit                  # the field's lowest bit; bits below Bgbit - 1 are fixed (to 0 inside a field)
        fixed = max(0, Bgbit - 1 - lsb)
        assert case.pos[q] == half - (1 << fixed), q    # half - 1 wherever the field lies above the fixed bits
        if (l, Bgbit) in ((3, 7), (2, 10)):
            assert case.pos[q] == half - 1
        assert set(np.unique(dig[q]).tolist()) <= {case.neg[q], case.pos[q]}, q
    if cid.startswith("worst"):
        positive = CS.WORST_ALIGNMENTS[int(cid[5:])][1]
        for q in range(2 * l):
            assert dig[q].min() == dig[q].max() == (case.pos[q] if positive else -half), q
    else:
        for q in range(2 * l):
            assert dig[q].min() == -half and dig[q].max() == case.pos[q], q


def _peak(case, two_limb=False):
    """log2 of the largest exact sum of the crafted step: over the whole key words, or over each 16-bit limb."""
    bk1 = np.asarray(case.bk).reshape(case.p.n, 2 * case.p.l, 2, case.p.N)[case.step]
    blocks = CS.limbs(bk1) if two_limb else (bk1,)
    return max(CS.log2_peak(CS.exact_sums(case.digits, b)) for b in blocks)


def test_largest_sums_are_the_claimed_ones(ia):
    """6 x 1024 x 64 x 2^31 = 2^49.58 on the one-limb kernels' set, 2^52 at the old set, and 2^46 per limb at the edge of
    Params::br_exact() on every ring."""
    assert abs(_peak(CS.worst_alignment(ia, 3, 7, 1024, 0)) - 49.58) < 0.01
    assert abs(_peak(CS.worst_alignment(ia, 2, 10, 1024, 0)) - 52) < 0.01
    jittered = CS.worst_alignment(ia, 3, 7, 1024, 4)  # 6 x 1024 x 63 x 2^31 = 2^49.56; the random bits take less than 1 % off it
    assert abs(_peak(jittered) - 49.56) < 0.01 and (CS.exact_sums(jittered.digits, jittered.bk[1]) & 1).any()
    other = CS.worst_alignment(ia, 3, 7, 1024, 4, bits_seed=CS.B0_BITS_SEED)  # other random bits: the same case but for block 1
    assert abs(_peak(other) - 49.56) < 0.01 and (CS.exact_sums(other.digits, other.bk[1]) & 1).any()
    assert not np.array_equal(other.bk[1], jittered.bk[1]) and (np.int64(CS.W_MAX) - other.bk[1] < 1 << 24).all() and (other.bk[1] <= CS.W_MAX).all()
    assert all(np.array_equal(a, b) for a, b in ((other.bk[0], jittered.bk[0]), (other.bk[2], jittered.bk[2]), (other.x, jittered.x), (other.target, jittered.target)))
    for l, Bgbit, N in CS.generic_edge_sets():
        if l == 1:
            assert 2 * N << Bgbit == 1 << 32  # the edge itself
            assert abs(_peak(CS.worst_alignment(ia, l, Bgbit, N, 0), two_limb=True) - 46) < 0.01, N
            assert abs(_peak(CS.worst_alignment(ia, l, Bgbit, N, 2), two_limb=True) - 46) < 0.01, N  # both limbs at once
    # mixed signs: 6144 terms of 2^37 with random signs, standard deviation 2^43.3 and a peak over 2048 coefficients of three
    # to four of them -- every operand at its extreme, the sum no larger than a generated key's
    assert 44 < _peak(CS.extreme_mixed(ia, 3, 7, 1024)) < 46


def test_limb_words_split_as_named():
    lo, hi = CS.limbs([CS.W_MIN, CS.W_MAX, CS.W_BOTH, CS.W_LOW])
    assert lo.tolist() == [0, -1, -(1 << 15), -(1 << 15)] and hi.tolist() == [-(1 << 15), 1 << 15, 1 << 15, 0]


def test_int32_end_words_are_reached_and_walked(ia, O, make_keys):
    case = CS.int32_ends(ia, make_keys(4, 1024).bk)
    N = 1024
    ck, accs = _walk(O, case)
    for r, a in enumerate(accs):
        assert np.array_equal(a[1], case.target), r
    for c in range(2):
        assert set(w - (1 << 32) if w >= 1 << 31 else w for w in (0x80000000, 0x7FFFFFC0, 0, 0xFFFFFFC0)) <= set(case.target[c].tolist())
    seen = set()
    for row in case.x:
        bara, barb = ck.modswitch(row)
        assert barb == 0 and bara[0] == 1
        seen |= set(bara[1:].tolist())
    assert {1, 2 * N - 1, N} <= seen
    # the walk moves the accumulator at every step (no amount 0 after the steering step)
    assert all(not np.array_equal(a[i], a[i + 1]) for a in accs for i in range(4))


def test_boundary_rows_hold_exactly_the_listed_amounts(O, make_keys):
    kb = make_keys(16, 1024)
    x = CS.boundary_amount_rows()
    assert x.shape == (14, 17)
    bara = np.stack([kb.ck.modswitch(r)[0] for r in x])
    for s in range(16):  # every step index meets every amount
        assert sorted(bara[:, s].tolist()) == sorted(CS.BOUNDARY_AMOUNTS), s
    for r in range(14):
        assert bara[r].tolist() == [CS.BOUNDARY_AMOUNTS[(r + s) % 14] for s in range(16)]
        assert kb.ck.modswitch(x[r])[1] == CS.BOUNDARY_AMOUNTS[r]
    # the oracle and the restatement over two of these rows (each holds every amount) and the rounding-edge rows
    from test_param_lattice_gpu import _modswitch_edge_rows
    edge = _modswitch_edge_rows(kb, np.random.default_rng(16))
    case = CS.Case(kb.p, kb.bk, np.concatenate([x[[0, 9]], edge[3:]]), kb.ksk, "boundary amounts", None, None, None, None, None)
    _walk(O, case)


@pytest.mark.parametrize("n,t,bb", [(7, 8, 2), (7, 4, 2), (7, 7, 4), (256, 8, 2)])
def test_keyswitch_references_agree_on_crafted_keys(O, n, t, bb):
    N = 64
    u = PL.edge_rows(np.random.default_rng(n + t), N, t, bb, 66)
    rows = u if n == 7 else u[[0, 66, 67, 68, 69]]
    keys = CS.ks_crafted_keys(n, N, t, bb)
    assert len(keys) == 9
    for label, ksk in keys:
        assert ksk[:, :, 0].any()  # digit-0 rows hold a pattern too
        ck = O.CloudKey(n, N, 1, 3, 7, t, bb, np.zeros((n, 6, 2, N), np.int32), ksk)
        ref = np_tfhe.np_keyswitch(ksk, t, bb, rows)
        for r in range(rows.shape[0]):
            assert np.array_equal(ck.keyswitch(rows[r]), ref[r]), (label, r)
        zero = [1, 2, 4] if n != 7 else [66, 67, 69]
        for r in zero:  # no row subtracted, whatever the d = 0 rows hold
            assert not ref[r, :n].any() and ref[r, n] == rows[r, N], (label, r)
    varied = keys[-1][1]
    assert len(set(varied[:, :, :, 0].ravel().tolist())) == 8 and (varied == varied[..., :1]).all()


# ---- crafted rows as operands of the public entry points ----

def _digest(case):
    return hashlib.sha256(b"".join(np.ascontiguousarray(v).tobytes() for v in (case.bk, case.x, case.ksk, case.digits, case.target))).hexdigest()[:16]


def test_optional_n_and_ksk_leave_existing_callers_their_arrays(ia):
    """The default call is the n = 3, zero-ksk case it was before the arguments existed (digests taken from the file as it was);
    n = 6 keeps the first three key blocks and amounts, adds uniform blocks and a mix of zero and non-zero boundary amounts at
    every further step, and a b word of 0; a uniform ksk goes through unchanged."""
    assert _digest(CS.worst_alignment(ia, 3, 7, 1024, 4)) == "78bb80ccef4bc3d2"
    assert _digest(CS.worst_alignment(ia, 2, 10, 1024, 0)) == "1a9db6f2a2ca1e84"
    for build in (lambda **kw: CS.worst_alignment(ia, 3, 7, 1024, 4, **kw), lambda **kw: CS.extreme_mixed(ia, 3, 7, 1024, **kw)):
        c3, c3n = build(), build(n=3, ksk=None)
        assert _digest(c3) == _digest(c3n) and not c3.ksk.any()
        ksk = CS.uniform_ksk(ia, 1024, 6)
        c6 = build(n=6, ksk=ksk)
        assert (c6.p.n, c6.x.shape, c6.bk.shape) == (6, (5, 7), (6, 6, 2, 1024)) and c6.ksk.size == c6.p.ksk_count
        assert np.array_equal(c6.bk[:3], c3.bk) and np.array_equal(c6.x[:, :3], c3.x[:, :3]) and not c6.x[:, 6].any()
        assert np.array_equal(c6.digits, c3.digits) and np.array_equal(c6.target, c3.target)
        assert np.array_equal(c6.ksk, ksk) and len(np.unique(ksk)) > ksk.size // 2
        for s in range(3, 6):
            amounts = [CS.further_amounts(r, s) for r in range(5)]
            assert c6.x[:, s].tolist() == [CS.amount_word(a, 1024) for a in amounts]
            assert 0 in amounts and any(a in CS.BOUNDARY_AMOUNTS and a for a in amounts), s
            assert len(np.unique(c6.bk[s])) > c6.bk[s].size // 2, s
    assert np.array_equal(CS.uniform_ksk(ia, 1024), CS.uniform_ksk(ia, 1024)) and CS.uniform_ksk(ia, 1024).size == c3.p.ksk_count


@pytest.fixture(scope="module")
def crafted(ia, O):
    """The case the GPU file runs (l = 3 / Bgbit = 7, 24 random bits off every key word, bits_seed B0_BITS_SEED) with a uniform
    ksk, its oracle key, the oracle's final accumulators of the five rows, their extracted samples and their bootstraps."""
    case = CS.worst_alignment(ia, 3, 7, 1024, 4, ksk=CS.uniform_ksk(ia, 1024), bits_seed=CS.B0_BITS_SEED)
    ck = CS.open_oracle(O, case.p, case.bk, case.ksk)
    acc = CS.oracle_accumulators(ck, case.x, (-1,))[-1]
    ext = np.stack([ck.sample_extract(a) for a in acc])
    boot = np.stack([ck.bootstrap(r) for r in case.x])
    for r in range(5):  # the blind rotation IS the bootstrap's: what the gate proofs below rest on
        assert np.array_equal(ck.keyswitch(ext[r]), boot[r]) and np.array_equal(ck.bootstrap_woks(case.x[r]), ext[r]), r
    assert len({bytes(b) for b in boot}) == 5 and boot[:, :3].any()  # the uniform ksk makes every word of the output depend on the rotation
    return case, ck, acc, ext, boot


TWO_INPUT = {CS.GATE_AND: "and", CS.GATE_XOR: "xor", CS.GATE_OR: "or", CS.GATE_NAND: "nand"}


@pytest.mark.parametrize("gate", [CS.GATE_OR, CS.GATE_AND, CS.GATE_NAND, CS.GATE_XOR, CS.GATE_MAJ3, CS.GATE_XOR3])
def test_gate_operands_bootstrap_the_crafted_rows(crafted, gate):
    from test_three_input_gates_gpu import combination
    case, ck, acc, ext, boot = crafted
    ops = CS.gate_operands(gate, case.x)
    assert all(o.dtype == np.int32 and o.shape == case.x.shape for o in ops) and not any(o.any() for o in ops[1:])
    assert np.array_equal(CS.gate_combination(gate, *ops), case.x)
    if gate in TWO_INPUT:
        for r in range(5):
            assert np.array_equal(ck.gate(TWO_INPUT[gate], ops[0][r], ops[1][r]), boot[r]), r
            assert np.array_equal(oracle_gate(ck, gate, ops[0][r], ops[1][r]), boot[r]), r
    else:  # the oracle has no entry point: the combination as the three-input tests state it, then its bootstrap
        x = combination(gate, *ops)
        assert np.array_equal(x, case.x)
        assert np.array_equal(CS.oracle_accumulators(ck, x, (-1,))[-1], acc)
    if gate == CS.GATE_XOR:  # halved operands: the doubled words are the row's
        assert np.array_equal(np_tfhe._wrap32(2 * np_tfhe._u32(ops[0]) + np.array([0] * case.p.n + [0x40000000])), case.x)
    # a gate type's own form against the libtfhe gates random_netlists states (cst, ka, kb) for
    assert np.array_equal(CS.gate_combination(CS.GATE_NAND, case.x, case.x[::-1]),
                          np_tfhe._wrap32(np_tfhe._u32(-case.x.astype(np.int64) - case.x[::-1]) + np.array([0] * case.p.n + [1 << 29])))


def test_mux_operands_bootstrap_two_crafted_rows(crafted):
    case, ck, acc, ext, boot = crafted
    x0, x1 = case.x, np.roll(case.x, -1, axis=0)
    sel = np_tfhe.uniform32(np.random.default_rng(21), case.x.shape)
    for a in (None, sel):
        a_, b, c = CS.mux_operands(x0, x1, a)
        h0, h1 = CS.mux_combinations(a_, b, c)
        assert np.array_equal(h0, x0) and np.array_equal(h1, x1) and (a is None) == (not a_.any())
        for r in range(5):  # boot-gates.cpp: the two extractions and (0, 1/8) added, one key switch
            u = np_tfhe._wrap32(ext[r].astype(np.int64) + ext[(r + 1) % 5])
            u[-1] = np_tfhe._wrap32(int(u[-1]) + CS.MU)
            assert np.array_equal(ck.mux(a_[r], b[r], c[r]), ck.keyswitch(u)), r
            assert np.array_equal(oracle_gate(ck, CS.GATE_MUX, a_[r], b[r], c[r]), ck.keyswitch(u)), r


def test_pbs_with_the_constant_polynomial_is_the_gate_bootstrap(crafted):
    case, ck, acc, ext, boot = crafted
    v = CS.pbs_constant_poly(case.p.N)
    for r in range(5):
        assert np.array_equal(LR.pbs_reference(ck, case.x[r], v), boot[r]) and np.array_equal(LR.pbs_reference(ck, case.x[r], v, keyswitch=False), ext[r])


def test_crafted_netlist_bootstraps_the_crafted_rows_at_level_0(ia, crafted):
    case, ck, acc, ext, boot = crafted
    with CS.crafted_netlist(ia) as cn:
        info = cn.info()
        assert (info.n_inputs, info.n_outputs, info.depth, info.bootstraps) == (7, 3, 3, 12)  # nothing folded: 10 gates, 2 of them MUX
        assert sum(g + m for g, m in CS.NETLIST_LEVEL_ITEMS) == 12 and cn.gates_by_type()[CS.GATE_MUX] == 2
        assert all(r >= 0 for g in cn.gates for r in g[1:]) and all(o >= 0 for o in cn.outputs)  # no netlist constant
        rows = CS.netlist_inputs(case.x)
        assert rows.shape == (7, 4) and not rows[6].any()
        # what level 0 blind-rotates, gate by gate as resolve() combines the wires
        lv0 = [CS.gate_combination(t, rows[a], rows[b]) for t, a, b, _ in CS.NETLIST_GATES[:4]] + list(CS.mux_combinations(rows[6], rows[4], rows[5]))
        assert np.array_equal(np.stack(lv0), CS.netlist_level0_rows(case.x))
        ref = oracle_netlist(types.SimpleNamespace(ck=ck), cn, rows)
        # the level-0 output taken directly is the MUX of rows 4 and 0; the other two depend on every level-0 wire
        u = np_tfhe._wrap32(ext[4].astype(np.int64) + ext[0])
        u[-1] = np_tfhe._wrap32(int(u[-1]) + CS.MU)
        assert np.array_equal(ref[2], ck.keyswitch(u))
        w = [boot[0], boot[1], boot[2], boot[3], ref[2]]                       # wires 7 .. 11
        l1 = [ck.gate("xor", w[0], w[1]), ck.gate("and", w[2], w[3]), ck.mux(w[4], w[0], w[3])]
        assert np.array_equal(ref[0], ck.gate("xor", l1[0], l1[1])) and np.array_equal(ref[1], ck.gate("and", l1[2], w[2]))
        read = {r >> 1 for g in cn.gates[5:] for r in (g[1:] if g[0] == CS.GATE_MUX else g[1:3])}
        assert set(range(7, 12)) <= read                                        # levels 1 and 2 consume every level-0 output


def test_old_set_rows_take_the_same_builders(ia, O):
    """l = 2 / Bgbit = 10 with a uniform ksk: gate operands and the pbs row reach the first worst-alignment rows there too."""
    case = CS.worst_alignment(ia, 2, 10, 1024, 0, ksk=CS.uniform_ksk(ia, 1024))
    ck = CS.open_oracle(O, case.p, case.bk, case.ksk)
    for gate in (CS.GATE_OR, CS.GATE_XOR):
        a, b = CS.gate_operands(gate, case.x)
        assert np.array_equal(CS.gate_combination(gate, a, b), case.x)
        assert np.array_equal(ck.gate(TWO_INPUT[gate], a[0], b[0]), ck.bootstrap(case.x[0]))
    assert np.array_equal(LR.pbs_reference(ck, case.x[4], CS.pbs_constant_poly(1024)), ck.bootstrap(case.x[4]))


def test_smallest_set_at_which_five_gates_per_cu_mix(ia):
    """mix_plan.h: one round of three phases is 2 x 2 mix_s1 + mix_s1 steps and has to leave a step, so n = 6 at mix_s1 = 1 -- on
    256 and on 304 CUs, each alone and together; 5 gates per CU lie inside the 4 .. 7 per CU the rotation of roles takes."""
    assert CS.smallest_mixing_set(ia) == CS.smallest_mixing_set(ia, (256,)) == CS.smallest_mixing_set(ia, (304,)) == (6, 1)
    import ctypes
    out = (ctypes.c_int * 9)()
    for cus in (256, 304):
        assert ia.lib().ieache_debug_mix_plan(cus, 5, 5 * cus, 1, 200, out) == 0      # n = 5: no whole round fits
        assert ia.lib().ieache_debug_mix_plan(cus, 6, 5 * cus, 1, 200, out) == 1 and list(out)[:5] == [3, 2, 1, 2, 1] and out[7] == 5
        assert ia.lib().ieache_debug_mix_plan(cus, 6, 4 * cus, 1, 200, out) == 0      # 4 per CU: every gate fits on two waves
