"""Crafted keys and inputs that put the blind-rotation and key-switch kernels at their arithmetic extremes: one set of
constructions, shared by tests/test_crafted_state_cpu.py (which proves on the oracle and on a numpy restatement that every
construction is what it claims to be) and tests/test_crafted_state_gpu.py (which compares the kernels with the oracle on them).

debug_blind_rotate always starts from the test vector (a = 0, b = mu = 2^29 everywhere, for an input whose b word is 0), so
the accumulator cannot be supplied; it is STEERED by the key of step 0:

  step 0, amount 1:  (X - 1) acc = (0, -2^30 X^0).  The only non-zero digit is the first digit of the b polynomial at
                     coefficient 0, d0 = -2^(Bgbit-2), so acc_c = start_c + d0 * bk[0][l][c]: any target T whose distance
                     from the start is a multiple of 2^(Bgbit-2), coefficient by coefficient.
                     (Amount N with a key (1 - X) Q reaches the same states at twice that granularity; amount 1 needs no
                     identity beyond d0 * K, and its finer step is what makes "every digit at -half" reachable at l x Bgbit = 32.)
  step 1, amount N:  (X^N - 1) acc = -2 T pointwise, decomposed against a bk[1] of the case's choice.

The decomposition reads W = -2 T + offset.  Because T = start (mod 2^(Bgbit-2)), the low Bgbit-1 bits of W are those of the
offset whatever the target; every bit above them is free (reachable_field_word).  At l = 3 / Bgbit = 7 and l = 2 / Bgbit = 10
the digit fields lie wholly above those bits, so every digit pattern is reachable.  Where they do not (l = 1 at the largest
Bgbit of a ring; l x Bgbit = 32) the positive extreme is the largest reachable digit instead of half - 1: Case.pos states it
per digit, and the CPU file asserts it."""
import collections

import numpy as np

import np_tfhe
from np_tfhe import _wrap32

MU = 1 << 29
# key words at the ends of the two balanced 16-bit limbs k_bk_to_spectrum splits them into (low = int16(w), high = (w - low) >> 16)
W_MIN, W_MAX = -(1 << 31), (1 << 31) - 1
W_BOTH = 0x7FFF8000               # low -2^15, high +2^15
W_LOW = 0xFFFF8000 - (1 << 32)    # low -2^15, high 0

# p, bk [n][2l][2][N], x [rows][n+1] first, as a caller unpacks them; ksk: all zero.  step: the crafted CMux step (None: no
# single one); digits: [2l][N] that enter it; neg / pos: per digit row, the two values the digits are drawn from;
# target: [2][N] accumulator after step 0 (None where step 0 is not a steering step)
Case = collections.namedtuple("Case", "p bk x ksk name step digits neg pos target")


def amount_word(a, N):
    """The torus word that mod-switches to exactly a (mod 2N)."""
    return int(_wrap32((a % (2 * N)) << (32 - (2 * N).bit_length() + 1)))


def decomposition_offset(l, Bgbit):
    return sum((1 << (Bgbit - 1)) << (32 - q * Bgbit) for q in range(1, l + 1)) & 0xFFFFFFFF


def np_digits(poly, l, Bgbit):
    """tGswTorus32PolynomialDecompH as np_tfhe.np_bootstrap states it: [l][N] int64."""
    w = (np_tfhe._u32(poly) + decomposition_offset(l, Bgbit)) & 0xFFFFFFFF
    return np.stack([((w >> (32 - q * Bgbit)) & ((1 << Bgbit) - 1)) - (1 << (Bgbit - 1)) for q in range(1, l + 1)])


def np_step_digits(acc, amount, l, Bgbit):
    """[2l][N] digits of (X^amount - 1) acc, rows 0 .. l-1 from the a polynomial."""
    tmp = [np_tfhe._mul_by_xai(acc[c], amount).astype(np.int64) - acc[c].astype(np.int64) for c in range(2)]
    return np.concatenate([np_digits(_wrap32(t), l, Bgbit) for t in tmp])


def exact_sums(digits, bk_i):
    """[2][N] int64: sum over rows of digit row * bk_i[row][c] mod X^N + 1, before any wrap.  Exact: at most 2l x N x
    2^(Bgbit-1) x 2^31 <= 2^62 on every set Params::br_exact() admits."""
    N = digits.shape[1]
    out = np.zeros((2, N), dtype=np.int64)
    for row in range(digits.shape[0]):
        for c in range(2):
            full = np.convolve(digits[row].astype(np.int64), bk_i[row, c].astype(np.int64))
            out[c] += full[:N]
            out[c, :N - 1] -= full[N:]
    return out


def np_step(acc, bk_i, amount, l, Bgbit):
    """One CMux step, restated from np_tfhe.np_bootstrap: acc [2][N] int32 -> [2][N] int32."""
    if amount == 0:
        return acc.copy()
    return _wrap32(acc.astype(np.int64) + exact_sums(np_step_digits(acc, amount, l, Bgbit), bk_i))


def limbs(w):
    """The two balanced 16-bit limbs of key words, as k_bk_to_spectrum (blind_rotate.hip) splits them."""
    w = np.asarray(w, dtype=np.int64)
    lo = (w & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int64)
    return lo, (w - lo) >> 16


def log2_peak(sums):
    m = float(np.abs(sums.astype(np.float64)).max())
    return float(np.log2(m)) if m else float("-inf")


# ---- steering ----

def start_acc(N):
    return np.stack([np.zeros(N, dtype=np.int32), np.full(N, MU, dtype=np.int32)])


def steering_block(p, target):
    """bk[0] [2l][2][N] that takes the test vector to `target` [2][N] in a step of amount 1."""
    g = p.Bgbit - 2  # d0 = -2^g
    assert g >= 0
    diff = (np_tfhe._u32(target) - np_tfhe._u32(start_acc(p.N))) & 0xFFFFFFFF
    assert not (diff & ((1 << g) - 1)).any(), "target not reachable: its distance from the test vector is no multiple of 2^(Bgbit-2)"
    blk = np.zeros((2 * p.l, 2, p.N), dtype=np.int32)
    blk[p.l] = _wrap32(-(diff >> g))
    return blk


def reachable_field_word(p, W):
    """The nearest W = -2 T + offset a steered T can give: the low Bgbit-1 bits are the offset's."""
    low = (1 << (p.Bgbit - 1)) - 1
    return (np.asarray(W, dtype=np.int64) & (0xFFFFFFFF ^ low)) | (decomposition_offset(p.l, p.Bgbit) & low)


def target_for_fields(p, W):
    """T [.. N] with -2 T + offset = W (mod 2^32); the free top bit of T is 0."""
    d = (decomposition_offset(p.l, p.Bgbit) - np.asarray(W, dtype=np.int64)) & 0xFFFFFFFF
    assert not (d & 1).any()
    return _wrap32(d >> 1)


def field_word(p, positive):
    """W whose digit q's field is all ones where positive[q] and 0 elsewhere, made reachable.  positive: [l][...] bool."""
    W = np.zeros(np.shape(positive)[1:], dtype=np.int64)
    for q in range(p.l):
        W |= np.where(positive[q], (1 << p.Bgbit) - 1, 0) << (32 - (q + 1) * p.Bgbit)
    return reachable_field_word(p, W)


def extreme_digits(p):
    """(neg, pos): per digit q, the value of a zero field and of an all-ones field after reachable_field_word."""
    ones = np.ones((p.l, 1), dtype=bool)
    return tuple(np_digits(_wrap32(field_word(p, s) - decomposition_offset(p.l, p.Bgbit)), p.l, p.Bgbit)[:, 0].tolist()
                 for s in (~ones, ones))


def _steered_case(ia, name, l, Bgbit, N, positive, block1, seed=5):
    """n = 3, 5 rows: step 0 steers, step 1 (amount N) decomposes -2 T with digit signs `positive` [2][l][N] against block1
    [2l][2][N]; step 2 meets a block of uniform words from the extreme state by amounts 0, 1, N, 2N - 1 and 513."""
    p = ia.default_params().copy(n=3, N=N, l=l, Bgbit=Bgbit)
    W = np.stack([field_word(p, positive[c]) for c in range(2)])
    target = target_for_fields(p, W)
    bk = np.zeros((3, 2 * l, 2, N), dtype=np.int32)
    bk[0] = steering_block(p, target)
    bk[1] = block1
    bk[2] = np_tfhe.uniform32(np.random.default_rng(seed), (2 * l, 2, N))
    x = np.zeros((5, 4), dtype=np.int32)
    x[:, 0], x[:, 1] = amount_word(1, N), amount_word(N, N)
    x[:, 2] = [amount_word(a, N) for a in (0, 1, N, 2 * N - 1, 513 % (2 * N))]
    off = decomposition_offset(l, Bgbit)
    digits = np.concatenate([np_digits(_wrap32(W[c] - off), l, Bgbit) for c in range(2)])
    neg, pos = extreme_digits(p)
    return Case(p, bk, x, np.zeros(p.ksk_count, dtype=np.int32), name, 1, digits, neg * 2, pos * 2, target)


WORST_ALIGNMENTS = (  # (label, every digit positive?, key word)
    ("-half x -2^31", False, W_MIN),            # the largest sum the set allows; high limb only
    ("half-1 x 2^31-1", True, W_MAX),
    ("-half x 0x7FFF8000", False, W_BOTH),      # both limbs at their extremes
    ("-half x 0xFFFF8000", False, W_LOW),       # low limb only
    # the second input with 24 random bits taken off every key word: sums as large (2^49.56), odd ones among them, and a
    # spectrum without the structure of a constant polynomial (whose half-integer transform outputs tie to the even exact sum)
    ("half-1 x (2^31-1 - 24 random bits)", True, None),
)


def worst_alignment(ia, l, Bgbit, N, which):
    """Case 1: every digit of step 1 at one extreme against a constant key block: all 2l x N terms of a coefficient's sum
    that do not wrap have one sign."""
    label, positive, word = WORST_ALIGNMENTS[which]
    block = np.full((2 * l, 2, N), W_MAX if word is None else word, dtype=np.int64)
    if word is None:
        block -= np.random.default_rng(11).integers(0, 1 << 24, size=block.shape)
    return _steered_case(ia, "worst alignment %s, l=%d Bgbit=%d N=%d" % (label, l, Bgbit, N), l, Bgbit, N,
                         np.full((2, l, N), positive), block.astype(np.int32))


def extreme_mixed(ia, l, Bgbit, N, seed=7):
    """Case 2: per coefficient and key row, digits from the two extremes and key words from {-2^31, 2^31 - 1, 0x7FFF8000}."""
    rng = np.random.default_rng(seed)
    positive = rng.integers(0, 2, size=(2, l, N)).astype(bool)
    block = rng.choice(np.array([W_MIN, W_MAX, W_BOTH], dtype=np.int64), size=(2 * l, 2, N)).astype(np.int32)
    return _steered_case(ia, "extreme magnitudes, mixed signs, l=%d Bgbit=%d N=%d" % (l, Bgbit, N), l, Bgbit, N, positive, block)


INT32_END_WORDS = (-(1 << 31), 0x7FFFFFC0, 0, -64)


def int32_ends(ia, gen_bk, N=1024):
    """Case 3 (l = 3 / Bgbit = 7): the accumulator steered to words at the int32 ends, then steps by amounts 1, 2N - 1 and N in
    every order against a generated key (gen_bk [>= 4][6][2][N]): the wrap identities of the rotated decomposition and of the
    32-bit accumulate."""
    p = ia.default_params().copy(n=4, N=N)
    assert (p.l, p.Bgbit) == (3, 7)
    rng = np.random.default_rng(9)
    target = np.stack([np.resize(np.array(INT32_END_WORDS, dtype=np.int64), N), np.resize(np.array(INT32_END_WORDS[1:] + INT32_END_WORDS[:1], dtype=np.int64), N)])
    some = rng.integers(0, N, size=(2, N // 8))
    for c in range(2):  # a scattering of other multiples of 64 between them, so that neighbours differ
        target[c, some[c]] = rng.integers(-(1 << 25), 1 << 25, size=N // 8) * 64
    target = _wrap32(target)
    bk = np.array(gen_bk[:4], dtype=np.int32).reshape(4, 6, 2, N)
    bk[0] = steering_block(p, target)
    amounts = [(1, 2 * N - 1, N), (2 * N - 1, 1, 1), (1, 1, 2 * N - 1), (2 * N - 1, 2 * N - 1, 1), (N + 1, N - 1, 2 * N - 1)]
    x = np.zeros((5, 5), dtype=np.int32)
    x[:, 0] = amount_word(1, N)
    x[:, 1:4] = [[amount_word(a, N) for a in row] for row in amounts]
    return Case(p, bk, x, np.zeros(p.ksk_count, dtype=np.int32), "accumulator words at the int32 ends", None, None, None, None, target)


BOUNDARY_AMOUNTS = (1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 1535, 1536, 2047, 0)


def boundary_amount_rows(n=16, N=1024):
    """Case 4's crafted rows [14][n+1]: row r meets amount BOUNDARY_AMOUNTS[(r + s) % 14] at step s, so every step index meets
    every amount; the b word takes the list's amounts too."""
    L = BOUNDARY_AMOUNTS
    return np.array([[amount_word(L[(r + s) % len(L)], N) for s in range(n)] + [amount_word(L[r], N)] for r in range(len(L))],
                    dtype=np.int32)


# ---- key switch ----

KS_WORDS = (0x80000000, 0x7FFFFFFF, 0x7F7F7F7F, 0x80808080, 0x7FFFFF80, 0xFFFFFF80, 0x00800080, 0xFFFFFFFF)


def ks_crafted_keys(n, N, t, bb):
    """(label, ksk [N][t][base][n+1]): one key per constant word of KS_WORDS -- the digit-0 rows included, which no family
    may subtract -- and one where every (i, j, d) row holds a different one of them."""
    shape = (N, t, 1 << bb, n + 1)
    keys = [("0x%08X" % w, np.full(shape, w, dtype=np.int64).astype(np.uint32).view(np.int32)) for w in KS_WORDS]
    rows = np.arange(N * t * (1 << bb)).reshape(shape[:3]) % len(KS_WORDS)
    varied = np.array(KS_WORDS, dtype=np.int64)[rows].astype(np.uint32).view(np.int32)
    keys.append(("a word per (i, j, d) row", np.ascontiguousarray(np.broadcast_to(varied[..., None], shape))))
    return keys


# ---- the two references on the same arrays ----

def open_oracle(O, p, bk, ksk):
    return O.CloudKey(p.n, p.N, p.k, p.l, p.Bgbit, p.ks_t, p.ks_basebit, bk, ksk)


def open_pair(ia, O, p, bk, ksk):
    """(oracle key, GPU context) on the same arrays; the caller closes the context."""
    return open_oracle(O, p, bk, ksk), ia.Context.from_arrays(p, bk, ksk)


def oracle_accumulators(ck, x, steps_list=(0, 1, 2, -1)):
    """{steps: [rows][2][N]} as debug_blind_rotate(x, steps) must return them."""
    n = ck.n
    want = {s: n if s < 0 else min(s, n) for s in steps_list}
    out = {s: [] for s in steps_list}
    for row in x:
        bara, barb = ck.modswitch(row)
        acc = ck.blind_rotate_init(barb)
        for i in range(n + 1):
            for s, cnt in want.items():
                if cnt == i:
                    out[s].append(acc)
            if i < n:
                acc = ck.blind_rotate_step(acc, i, bara[i])
    return {s: np.stack(v) for s, v in out.items()}


# ---- the sets the two files run ----

def generic_edge_sets():
    """(l, Bgbit, N) for k_blind_rotate_generic: l = 1 at the largest Bgbit Params::br_exact() keeps on the ring (two-limb sums
    of 2^46), and the two l x Bgbit = 32 sets of the lattice file."""
    import param_lattice as PL
    return [(1, PL.largest_bgbit(N), N) for N in (16, 64, 512, 1024)] + [(2, 16, 16), (4, 8, 1024)]


def steered_cases(ia, l, Bgbit, N):
    """Cases 1 and 2 at one set, as (id, builder) so that a test builds only its own (ia may be None where only the ids are read)."""
    out = [("worst%d" % w, lambda w=w: worst_alignment(ia, l, Bgbit, N, w)) for w in range(len(WORST_ALIGNMENTS))]
    return out + [("mixed", lambda: extreme_mixed(ia, l, Bgbit, N))]
