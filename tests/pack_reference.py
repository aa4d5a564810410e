"""The packing key switch (include/ieache.h section 3e) restated in numpy, int64 with wrap: the digit matrix [rows][n t] times the
key [n t][2N], then the rotate-and-sum with np_tfhe._mul_by_xai.  Shares no code with the C++ reference or the kernels.

    R_r   = (0, b_r X^0) - sum_{i,j} d_{r,i,j} PK[i][j]
    out_g = sum_{p<m} sum_{q<w} X^(p w + q + shift) R_{g m + p}

The product and the inner sums S_p = sum_q X^q R_p do not depend on the shift or on how rows are grouped, so a test computes
them once (product, spread_sums) and places them many times (place): X^a X^b = X^(a+b) holds exactly in Z_{2^32}[X]/(X^N+1), so
X^(p w + shift) S_p is the definition's inner sum word for word.

Also crafted keys whose words carry through every byte limb, as crafted_state.py has them for the key-switch key."""
import numpy as np

from np_tfhe import _mul_by_xai, _u32, _wrap32

INT32_MIN = -(1 << 31)
# words whose balanced byte limbs sit at their extremes and carry into the next: 127 / -128 in every limb, a carry chain through
# all four, the sign word, the largest word, nothing, and all ones
CARRY_WORDS = np.array([0x7F7F7F7F, 0x80808080, 0x7FFFFF80, 0x80000000, 0x7FFFFFFF, 0, 0xFFFFFFFF], dtype=np.uint32).view(np.int32)


def full_range(rng, shape):
    return rng.integers(INT32_MIN, 1 << 31, size=shape, dtype=np.int64).astype(np.int32)


def digits(rows, n, t, basebit):
    """lweKeySwitch's digits of the rows' a words: [rows][n t] int64, k = i t + j (word for word np_tfhe.np_keyswitch's)."""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.int32))
    abar = (_u32(rows[:, :n]) + (1 << (32 - (1 + basebit * t)))) & 0xFFFFFFFF
    shifts = 32 - (np.arange(t) + 1) * basebit
    return ((abar[:, :, None] >> shifts) & ((1 << basebit) - 1)).reshape(rows.shape[0], n * t)


def product(pk, rows, t, basebit):
    """R [rows][2][N] int32.  pk [n][t][2][N]; |digit| < 2^4, |key| <= 2^31, n t < 2^24 terms: below 2^59, exact in int64."""
    pk = np.asarray(pk, dtype=np.int32)
    n, N = pk.shape[0], pk.shape[3]
    rows = np.atleast_2d(np.asarray(rows, dtype=np.int32))
    R = -(digits(rows, n, t, basebit) @ pk.reshape(n * t, 2 * N).astype(np.int64))
    R[:, N] += rows[:, n]
    return _wrap32(R).reshape(rows.shape[0], 2, N)


def product_fast(pk, rows, t, basebit):
    """product() for the larger shapes: numpy's int64 matrix product runs at ~0.1 G products/s, so the same integers are
    formed as two float64 products on the 16-bit halves of the unsigned key words -- each sum below 15 x 2^16 x n t < 2^44,
    exact in a double -- and recombined in int64.  test_pack_cpu.py holds it equal to product()."""
    pk = np.asarray(pk, dtype=np.int32)
    n, N = pk.shape[0], pk.shape[3]
    rows = np.atleast_2d(np.asarray(rows, dtype=np.int32))
    D = digits(rows, n, t, basebit).astype(np.float64)
    key = _u32(pk.reshape(n * t, 2 * N))
    R = -((D @ (key & 0xFFFF).astype(np.float64)).astype(np.int64) + ((D @ (key >> 16).astype(np.float64)).astype(np.int64) << 16))
    R[:, N] += rows[:, n]
    return _wrap32(R).reshape(rows.shape[0], 2, N)


def spread_sums(R, spread):
    """S [rows][2][N]: S_r = sum_{q < spread} X^q R_r."""
    S = np.zeros(R.shape, dtype=np.int64)
    for r in range(R.shape[0]):
        for c in range(2):
            for q in range(spread):
                S[r, c] += _mul_by_xai(R[r, c], q)
    return _wrap32(S)


def place(S, groups, m, spread, shift):
    """out [groups][2][N] from the first groups x m rows of S = spread_sums(R, spread)."""
    N = S.shape[2]
    out = np.zeros((groups, 2, N), dtype=np.int64)
    for g in range(groups):
        for p in range(m):
            for c in range(2):
                out[g, c] += _mul_by_xai(S[g * m + p, c], (p * spread + shift) % (2 * N))
    return _wrap32(out)


def pack(pk, rows, m, spread=1, shift=0, t=8, basebit=2):
    """The whole definition: rows [groups m][n+1] -> [groups][2][N]."""
    rows = np.asarray(rows, dtype=np.int32).reshape(-1, np.shape(rows)[-1])
    return place(spread_sums(product(pk, rows, t, basebit), spread), rows.shape[0] // m, m, spread, shift)


def crafted_keys(n, t, N):
    """{name: pk [n][t][2][N]}: every word one of CARRY_WORDS ("constant": one word throughout, one key per word), and the
    words varied row by row and along the row ("varied")."""
    keys = {"constant_%08x" % (int(w) & 0xFFFFFFFF): np.full((n, t, 2, N), w, dtype=np.int32) for w in CARRY_WORDS}
    k = np.arange(n * t)[:, None] * 3 + np.arange(2 * N)[None, :]
    keys["varied"] = CARRY_WORDS[k % len(CARRY_WORDS)].reshape(n, t, 2, N)
    return keys


def crafted_rows(rng, count, n, t, basebit):
    """Full-range rows with a few pinned: every digit at its largest (a = -1 - the rounding offset ... all ones after it),
    every digit 0, and the extreme b words."""
    rows = full_range(rng, (count, n + 1))
    ones = np.uint32((0xFFFFFFFF - (1 << (31 - t * basebit))) & 0xFFFFFFFF)
    rows[0, :n] = np.array([ones], dtype=np.uint32).view(np.int32)[0]          # abar = all ones: every digit 2^b - 1
    if count > 1:
        rows[1, :n] = np.array([(-(1 << (31 - t * basebit))) & 0xFFFFFFFF], dtype=np.uint32).view(np.int32)[0]  # abar = 0
        rows[1, n] = INT32_MIN
    rows[0, n] = (1 << 31) - 1
    return rows
