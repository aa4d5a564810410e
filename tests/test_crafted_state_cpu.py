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
transform's half-integer outputs all tie to the even exact sum and an unguarded kernel is right by luck."""
import numpy as np
import pytest

import crafted_state as CS
import np_tfhe
import param_lattice as PL

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
