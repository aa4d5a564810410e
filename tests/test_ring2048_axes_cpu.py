"""What tests/test_ring2048_axes_gpu.py rests on, as far as it needs no GPU: its crafted rows mod-switch to exactly the amounts
they claim, at every key length it uses; the oracle's accumulators on such a row are those of the numpy restatement of a CMux step
(np_tfhe.np_bootstrap's arithmetic, crafted_state.np_step); the boundary factor's reference is a plain schoolbook product."""
import numpy as np
import pytest

import crafted_state as CS
import multi_reference as MR
import np_tfhe

N = 2048
AXIS_N = (63, 64, 65, 129, 257, 630)


def _key_of_uniform_words(O, n, seed):
    """An oracle key of uniform words (no arithmetic here asks for more), with the smallest key-switch key a set may have."""
    bk = np_tfhe.uniform32(np.random.default_rng(seed), (n, 6, 2, N))
    return bk, O.CloudKey(n, N, 1, 3, 7, 1, 1, bk, np.zeros(N * 2 * (n + 1), dtype=np.int32))


@pytest.mark.parametrize("n", AXIS_N)
def test_crafted_rows_mod_switch_to_their_amounts(O, n):
    """Through the oracle's mod switch and through np_tfhe's: the pattern rows give every step index every one of the eight
    amounts; the isolating rows are zero exactly where they claim."""
    pattern, isolating = CS.axis_pattern_amounts(n, N), CS.axis_isolating_amounts(n, N)
    amounts = np.concatenate([pattern, isolating])
    x = CS.amount_rows(amounts, N)
    assert x.dtype == np.int32 and x.shape == (10, n + 1)
    ck = O.CloudKey(n, N, 1, 3, 7, 1, 1, np.zeros(n * 6 * 2 * N, dtype=np.int32), np.zeros(N * 2 * (n + 1), dtype=np.int32))
    for r in range(10):
        bara, barb = ck.modswitch(x[r])
        assert np.array_equal(bara, amounts[r, :n]) and barb == amounts[r, n], r
        assert [np_tfhe.np_modswitch(int(w), 12) for w in x[r]] == list(amounts[r]), r
        assert x[r, 0] == CS.amount_word(int(amounts[r, 0]), N)
    A = set(CS.axis_amounts(N))
    assert len(A) == 8 and all(set(pattern[:, s]) == A for s in range(n + 1))
    assert sorted(np.flatnonzero(isolating[0])) == sorted({s for s in (63, 64) if s < n - 1} | {n - 1})
    assert isolating[0, n - 1] == 2 * N - 1 and (n <= 64 or isolating[0, 63] == 1) and (n <= 65 or isolating[0, 64] == N + 1)
    assert not isolating[1, 16:32].any() and (np.delete(isolating[1], np.arange(16, 32)) % 2 == 1).all()
    assert len(set(np.delete(isolating[1], np.arange(16, 32)))) == n + 1 - 16


def test_oracle_accumulators_equal_the_numpy_step_on_a_pattern_row(O):
    """n = 129, the largest key length of the GPU file for which the numpy restatement (24 exact convolutions of 2048 x 2048
    terms per step, 27 ms) finishes in a few seconds here (3.5 s; n = 257 takes twice that): pattern row 1 -- amounts 1, N, 2N - 1, 2, N + 1, 0, N - 1,
    2N - 2 in turn -- after 0, 1, 63, 64, 65 steps and after all of them."""
    n = 129
    bk, ck = _key_of_uniform_words(O, n, n)
    amounts = CS.axis_pattern_amounts(n, N)[1]
    x = CS.amount_rows(amounts[None], N)
    steps = [s for s in (0, 1, 63, 64, 65, -1) if s <= n]
    ref = CS.oracle_accumulators(ck, x, steps)
    acc = np.stack([np_tfhe._mul_by_xai(np.full(N, CS.MU, dtype=np.int32) * c, (2 * N - int(amounts[n])) % (2 * N)) for c in (0, 1)])
    for i in range(n + 1):
        for s in steps:
            if (n if s < 0 else s) == i:
                assert np.array_equal(ref[s][0], acc), (s, i)
        if i < n:
            acc = CS.np_step(acc, bk[i], int(amounts[i]), 3, 7)


def test_boundary_factor_reference_is_a_schoolbook_product(O):
    """multi_reference on the factor with non-zero words at coefficients 0, 7, 8, 255, 256, 1023, 1024, 2047 against the
    definition in numpy: coefficient 0 of factor x accumulator extracted, u[j] = (P A)[0] for j = 0 and -(P A)[N - j] above,
    u[N] = (P B)[0] + bias, products as exact integer convolutions reduced mod X^N + 1 and 2^32."""
    BOUNDARY_AT, BOUNDARY_VALUES = CS.BOUNDARY_AT, CS.BOUNDARY_VALUES
    P = CS.boundary_factor(N)
    assert sorted(np.flatnonzero(P)) == list(BOUNDARY_AT) and len(set(BOUNDARY_VALUES)) == 8
    assert P.min() == -(1 << 31) and P.max() == (1 << 31) - 1
    rng = np.random.default_rng(77)
    acc = np_tfhe.uniform32(rng, (2, N))
    bias = np.array([0x12345678], dtype=np.int32)
    ck = O.CloudKey(2, N, 1, 3, 7, 1, 1, np.zeros(2 * 6 * 2 * N, dtype=np.int32), np.zeros(N * 2 * 3, dtype=np.int32))
    got = MR.multi_from_accumulator(ck, acc, P, bias, keyswitch=False)[0]
    prod = []
    for c in range(2):
        full = [0] * (2 * N)
        for j, v in zip(BOUNDARY_AT, BOUNDARY_VALUES):  # Python integers: no intermediate can wrap
            for i in range(N):
                full[i + j] += v * int(acc[c, i])
        prod.append([(full[i] - full[i + N]) & 0xFFFFFFFF for i in range(N)])
    want = [prod[0][0]] + [(-prod[0][N - j]) & 0xFFFFFFFF for j in range(1, N)] + [(prod[1][0] + int(bias[0])) & 0xFFFFFFFF]
    assert np.array_equal(np_tfhe._u32(got), np.array(want, dtype=np.int64))
