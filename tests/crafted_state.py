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

# p, bk [n][2l][2][N], x [rows][n+1] first, as a caller unpacks them; ksk: all zero unless the builder was given one.  step: the crafted CMux step (None: no
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


FURTHER_AMOUNTS = (0, 1023, 0, 1025, 2047, 64, 0, 1536)


def further_amounts(row, step):
    """The amount row `row` meets at step `step` >= 3 of a case with n > 3: a fixed mix of 0 (the step is skipped) and non-zero
    boundary amounts, shifted from row to row so that every step has both."""
    return FURTHER_AMOUNTS[(3 * row + step) % len(FURTHER_AMOUNTS)]


def uniform_ksk(ia, N, n=3, seed=13):
    """A key-switching key of uniform words for the steered cases' set (n, N): the key switch and the deeper levels of a
    circuit then do real work against the crafted bootstrapping key."""
    p = ia.default_params().copy(n=n, N=N)
    return np_tfhe.uniform32(np.random.default_rng(seed), p.ksk_count)


def _steered_case(ia, name, l, Bgbit, N, positive, block1, seed=5, n=3, ksk=None):
    """5 rows: step 0 steers, step 1 (amount N) decomposes -2 T with digit signs `positive` [2][l][N] against block1
    [2l][2][N]; step 2 meets a block of uniform words from the extreme state by amounts 0, 1, N, 2N - 1 and 513.  n > 3: the
    further key blocks are uniform words and the rows meet them by further_amounts(); the first three steps are those of n = 3,
    array for array.  ksk: None = all zero, or the words of a key for (n, N) (uniform_ksk)."""
    assert n >= 3
    p = ia.default_params().copy(n=n, N=N, l=l, Bgbit=Bgbit)
    W = np.stack([field_word(p, positive[c]) for c in range(2)])
    target = target_for_fields(p, W)
    bk = np.zeros((n, 2 * l, 2, N), dtype=np.int32)
    bk[0] = steering_block(p, target)
    bk[1] = block1
    bk[2] = np_tfhe.uniform32(np.random.default_rng(seed), (2 * l, 2, N))
    if n > 3:  # a generator of their own: bk[2] stays what it is at n = 3
        bk[3:] = np_tfhe.uniform32(np.random.default_rng([seed, n]), (n - 3, 2 * l, 2, N))
    x = np.zeros((5, n + 1), dtype=np.int32)
    x[:, 0], x[:, 1] = amount_word(1, N), amount_word(N, N)
    x[:, 2] = [amount_word(a, N) for a in (0, 1, N, 2 * N - 1, 513 % (2 * N))]
    for s in range(3, n):
        x[:, s] = [amount_word(further_amounts(r, s), N) for r in range(5)]
    off = decomposition_offset(l, Bgbit)
    digits = np.concatenate([np_digits(_wrap32(W[c] - off), l, Bgbit) for c in range(2)])
    neg, pos = extreme_digits(p)
    if ksk is None:
        ksk = np.zeros(p.ksk_count, dtype=np.int32)
    ksk = np.ascontiguousarray(ksk, dtype=np.int32)
    assert ksk.size == p.ksk_count
    return Case(p, bk, x, ksk, name, 1, digits, neg * 2, pos * 2, target)


WORST_ALIGNMENTS = (  # (label, every digit positive?, key word)
    ("-half x -2^31", False, W_MIN),            # the largest sum the set allows; high limb only
    ("half-1 x 2^31-1", True, W_MAX),
    ("-half x 0x7FFF8000", False, W_BOTH),      # both limbs at their extremes
    ("-half x 0xFFFF8000", False, W_LOW),       # low limb only
    # the second input with 24 random bits taken off every key word: sums as large (2^49.56), odd ones among them, and a
    # spectrum without the structure of a constant polynomial (whose half-integer transform outputs tie to the even exact sum)
    ("half-1 x (2^31-1 - 24 random bits)", True, None),
)


# bits_seed of alignment 4 at l = 3 / Bgbit = 7 / N = 1024 under which the unguarded one-limb build (br_variant 35) rounds
# coefficient 0 of polynomial b wrongly in step 1 -- the one word of b a sample extraction reads (tests/test_safety_nets_gpu.py;
# under the default 11 its wrong words are b[977], b[1009], b[1019], which only a multi-output bootstrap can show)
B0_BITS_SEED = 622


def worst_alignment(ia, l, Bgbit, N, which, n=3, ksk=None, bits_seed=11):
    """Case 1: every digit of step 1 at one extreme against a constant key block: all 2l x N terms of a coefficient's sum
    that do not wrap have one sign.  bits_seed: the generator of the random bits of alignment 4 (the sums stay 2^49.56 under any;
    WHICH words an unguarded one-limb kernel rounds wrongly depends on it)."""
    label, positive, word = WORST_ALIGNMENTS[which]
    block = np.full((2 * l, 2, N), W_MAX if word is None else word, dtype=np.int64)
    if word is None:
        block -= np.random.default_rng(bits_seed).integers(0, 1 << 24, size=block.shape)
    return _steered_case(ia, "worst alignment %s, l=%d Bgbit=%d N=%d" % (label, l, Bgbit, N), l, Bgbit, N,
                         np.full((2, l, N), positive), block.astype(np.int32), n=n, ksk=ksk)


def extreme_mixed(ia, l, Bgbit, N, seed=7, n=3, ksk=None):
    """Case 2: per coefficient and key row, digits from the two extremes and key words from {-2^31, 2^31 - 1, 0x7FFF8000}."""
    rng = np.random.default_rng(seed)
    positive = rng.integers(0, 2, size=(2, l, N)).astype(bool)
    block = rng.choice(np.array([W_MIN, W_MAX, W_BOTH], dtype=np.int64), size=(2 * l, 2, N)).astype(np.int32)
    return _steered_case(ia, "extreme magnitudes, mixed signs, l=%d Bgbit=%d N=%d" % (l, Bgbit, N), l, Bgbit, N, positive, block,
                         n=n, ksk=ksk)


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


# ---- rows for the size axes of a ring: long keys, slices that reload their amounts (tests/test_ring2048_axes_*.py) ----

def axis_amounts(N):
    """0 (the step is skipped), 1, 2, N - 1, N, N + 1, 2N - 2, 2N - 1: even and odd amounts on both sides of the sign change."""
    return (0, 1, 2, N - 1, N, N + 1, 2 * N - 2, 2 * N - 1)


def axis_pattern_amounts(n, N):
    """[8][n+1] amounts (the b word's last): row r meets axis_amounts[(r + 3 s) % 8] at step s, so over the eight rows every
    step index -- every lane of a slice of any length -- meets every one of the eight amounts.  A row repeats every 8 steps,
    so a step index that is wrong by a multiple of 8 reads the right amount: the isolating and the uniform rows see those."""
    A = axis_amounts(N)
    return np.array([[A[(r + 3 * s) % 8] for s in range(n)] + [A[(r + 5) % 8]] for r in range(8)], dtype=np.int64)


def axis_isolating_amounts(n, N):
    """[2][n+1] amounts.  Row 0: zero everywhere but 1 at step 63, N + 1 at step 64 (where the key has them) and, set last,
    2N - 1 at step n - 1: lane 63 of a slice, the first step of the next one, the last step of the key.  Row 1: zero over steps
    16 .. 31 -- one whole slice of the default length -- and odd amounts, all different, elsewhere; its b word is odd too."""
    a = np.zeros((2, n + 1), dtype=np.int64)
    for s, amount in ((63, 1), (64, N + 1)):
        if s < n:
            a[0, s] = amount
    a[0, n - 1] = 2 * N - 1
    s = np.arange(n + 1)
    a[1] = (2 * (7 * s + 3) + 1) % (2 * N)
    a[1, 16:min(32, n)] = 0
    return a


def amount_rows(amounts, N):
    """Amounts [rows][n+1] -> the torus words that mod-switch to exactly them."""
    shift = 32 - (2 * N).bit_length() + 1
    return _wrap32((np.asarray(amounts, dtype=np.int64) % (2 * N)) << shift)


# the edges of k_mv_compact's N / 256 = 8 coefficients per thread and of k_mv_extract_2048's j = tid + 256 r at N = 2048
BOUNDARY_AT = (0, 7, 8, 255, 256, 1023, 1024, 2047)
BOUNDARY_VALUES = (-(1 << 31), (1 << 31) - 1, 0x12345679, -0x6789ABCD, 1, -1, 0x40000001, -0x7FFFFFFF)


def boundary_factor(N=2048):
    """A factor polynomial of the multi-output bootstrap that is non-zero exactly at BOUNDARY_AT, full-range and all different."""
    P = np.zeros(N, dtype=np.int32)
    P[list(BOUNDARY_AT)] = np.array(BOUNDARY_VALUES, dtype=np.int64).astype(np.int32)
    return P


def first_difference(got, want):
    """None where the arrays agree, else (index of the first differing word, number of differing words)."""
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    return None if bad.size == 0 else (tuple(int(v) for v in bad[0]), len(bad))


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


# ---- crafted rows as operands of the public entry points ----
# A gate bootstraps a linear combination of its operand rows (csrc/device_common.h: gate_coeffs, resolve, combined_coef):
# (0, cst) + k (a + b [+ c]) word for word mod 2^32, bootsMUX the two combinations (0, -1/8) + a + b and (0, -1/8) - a + c.
# The builders below solve that for operands whose combination IS a crafted row, so that the row reaches the blind rotation
# through gates, gates3, mux, pbs, a netlist level: every public path, not only the debug hook.

GATE_AND, GATE_XOR, GATE_OR, GATE_NAND, GATE_MUX, GATE_MAJ3, GATE_XOR3 = 0, 1, 2, 3, 4, 32, 33
GATE_FORM = {GATE_AND: (0xE0000000, 1), GATE_XOR: (0x40000000, 2), GATE_OR: (0x20000000, 1), GATE_NAND: (0x20000000, -1),
             GATE_MAJ3: (0, 1), GATE_XOR3: (0x80000000, 2)}   # (cst, k) as boot-gates.cpp / DESIGN.md section 7 give them
MUX_CST = 0xE0000000


def _u(rows):
    return np_tfhe._u32(np.asarray(rows, dtype=np.int32))


def _plus_b(rows, word):
    """rows + (0, word): the constant term enters the b word alone."""
    out = _u(rows).copy()
    out[..., -1] = (out[..., -1] + word) & 0xFFFFFFFF
    return out


def gate_combination(gate, a, b, c=None):
    """The row a gate of type `gate` bootstraps from its operand rows: (0, cst) + k (a + b [+ c]) mod 2^32."""
    cst, k = GATE_FORM[gate]
    total = _u(a) + _u(b) + (_u(c) if c is not None else 0)
    return _wrap32(_plus_b(_wrap32(k * total), cst))


def mux_combinations(a, b, c):
    """The two rows bootsMUX(a, b, c) blind-rotates: (0, -1/8) + a + b and (0, -1/8) - a + c."""
    return _wrap32(_plus_b(_wrap32(_u(a) + _u(b)), MUX_CST)), _wrap32(_plus_b(_wrap32(_u(c) - _u(a)), MUX_CST))


def gate_operands(gate, x):
    """(a, b) -- (a, b, c) for MAJ3 / XOR3 -- with gate_combination(gate, ...) == x word for word: a = k^-1 (x - (0, cst)), every
    other operand an all-zero row.  The factor-2 gates (XOR, XOR3) take the halved words; x - (0, cst) has to be even
    everywhere, which the steered rows are (amount words are multiples of 2^21, their b word is 0, cst is even)."""
    cst, k = GATE_FORM[gate]
    d = _plus_b(x, -cst)
    if abs(k) == 2:
        assert not (d & 1).any(), "a factor-2 gate needs even words"
        d = d >> 1
    a = _wrap32(-d if k < 0 else d)
    zero = np.zeros_like(a)
    return (a, zero, zero.copy()) if gate in (GATE_MAJ3, GATE_XOR3) else (a, zero)


def mux_operands(x0, x1, a=None):
    """(a, b, c) with mux_combinations(a, b, c) == (x0, x1): b = x0 - (0, -1/8) - a, c = x1 - (0, -1/8) + a; a: any rows (None: zero)."""
    a = np.zeros_like(np.asarray(x0, dtype=np.int32)) if a is None else np.asarray(a, dtype=np.int32)
    return a, _wrap32(_plus_b(x0, -MUX_CST) - _u(a)), _wrap32(_plus_b(x1, -MUX_CST) + _u(a))


def pbs_constant_poly(N):
    """The programmable bootstrap's test polynomial under which a row is bootstrapped as a gate bootstraps it: 2^29 everywhere."""
    return np.full(N, MU, dtype=np.int32)


# The crafted netlist.  Inputs 0 .. 3: the operands that make OR / AND / NAND / XOR bootstrap rows 0 .. 3; inputs 4, 5: b and c
# of a MUX whose halves are rows 4 and 0; input 6: an all-zero row (every second operand, and the MUX's a).  No netlist
# constant anywhere.  Level 0 is those five gates (six blind rotations, all on crafted rows); levels 1 and 2 consume every
# level-0 output through XOR and AND pairs and a MUX, and one output is a level-0 wire as it stands.
NETLIST_INPUTS = 7
NETLIST_GATES = (  # (type, a, b, c) in wire numbers; wire 7 + i is gate i
    (GATE_OR, 0, 6, 0), (GATE_AND, 1, 6, 0), (GATE_NAND, 2, 6, 0), (GATE_XOR, 3, 6, 0), (GATE_MUX, 6, 4, 5),   # level 0: wires 7 .. 11
    (GATE_XOR, 7, 8, 0), (GATE_AND, 9, 10, 0), (GATE_MUX, 11, 7, 10),                                           # level 1: wires 12 .. 14
    (GATE_XOR, 12, 13, 0), (GATE_AND, 14, 9, 0))                                                                # level 2: wires 15, 16
NETLIST_OUTPUTS = (15, 16, 11)
NETLIST_LEVEL_ITEMS = ((5, 1), (3, 1), (2, 0))   # (gates, of which MUX) per level: 6 + 4 + 2 = 12 blind rotations


def crafted_netlist(ia):
    """-> CompiledNetlist of the gate list above (the caller closes it)."""
    nl = ia.Netlist(NETLIST_INPUTS)
    for t, a, b, c in NETLIST_GATES:
        nl.gate(t, a << 1, b << 1, (c << 1) if t == GATE_MUX else 0)
    return nl.compile([w << 1 for w in NETLIST_OUTPUTS])


def netlist_level0_rows(x):
    """The crafted rows the six blind rotations of level 0 see, in gate order (both halves of the MUX last)."""
    return np.stack([x[0], x[1], x[2], x[3], x[4], x[0]])


def netlist_inputs(x):
    """One expression's input rows [7][n+1] from the five crafted rows x."""
    x = np.asarray(x, dtype=np.int32)
    ops = [gate_operands(g, x[i:i + 1])[0][0] for i, g in enumerate((GATE_OR, GATE_AND, GATE_NAND, GATE_XOR))]
    _, mb, mc = mux_operands(x[4:5], x[0:1])
    return np.stack(ops + [mb[0], mc[0], np.zeros(x.shape[1], dtype=np.int32)])


def smallest_mixing_set(ia, cus_list=(256, 304), ratio=200):
    """(n, mix_s1): the smallest LWE dimension n > 3, and the smallest "mix_s1" there, at which csrc/mix_plan.h
    (ieache_debug_mix_plan, host only) runs a launch of 5 x cus gate instances as a rotation of roles that leaves the ordinary
    slice loop at least a step, on every CU count of cus_list; None if there is none below n = 64."""
    import ctypes
    out = (ctypes.c_int * 9)()
    for n in range(4, 64):
        for s1 in range(1, n):
            if all(ia.lib().ieache_debug_mix_plan(c, n, 5 * c, s1, ratio, out) == 1 and 0 < out[7] < n for c in cus_list):
                return n, s1
    return None


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


def oracle_accumulators_threaded(ck, x, steps_list=(0, 1, 2, -1), threads=16):
    """oracle_accumulators with a host thread per row, for long keys (the oracle's stages take the key read-only and ctypes
    releases the interpreter lock, as multi_reference.multi_reference_rows relies on)."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(threads) as ex:
        per_row = list(ex.map(lambda row: oracle_accumulators(ck, row[None], steps_list), np.asarray(x)))
    return {s: np.concatenate([r[s] for r in per_row]) for s in steps_list}


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
