"""Rounding margin of the one-limb external product, modelled in numpy.

The wide-launch blind rotation multiplies 7-bit digit polynomials with the 32-bit bootstrapping-key polynomials through
ONE double-precision transform (as libtfhe does) and rounds the sum of 2l = 6 products to integers.  This is the same
computation in numpy (pocketfft instead of the kernel's 8x8x8 radix-8 schedule: same precision class), compared with
exact integer arithmetic: the rounded result must be the exact product and the distance to the nearest integer must
stay far below the kernel's guard limit (1/16) -- for random data, for every operand at its extreme magnitude, and for
the worst alignment (all terms of one sign, sum 2^49.6).  tests/test_fft_probe_gpu.py holds the kernel's transform to
this model on the card: its error against an extended-precision reference within a small measured margin of the model's."""
import numpy as np

N = 1024


def _fft_product_sum(digs, bks):
    j = np.arange(N // 2)
    tw = np.exp(1j * np.pi * j / N)
    acc = np.zeros(N // 2, dtype=np.complex128)
    for d, b in zip(digs, bks):
        fd = np.fft.fft((d[: N // 2] + 1j * d[N // 2:]) * tw)
        fb = np.fft.fft((b[: N // 2].astype(np.float64) + 1j * b[N // 2:].astype(np.float64)) * tw)
        acc += fd * fb
    y = np.fft.ifft(acc) * np.conj(tw)
    return np.concatenate([y.real, y.imag])


def _exact_product_sum(digs, bks):
    out = np.zeros(N, dtype=object)
    for d, b in zip(digs, bks):
        full = np.convolve(np.array([int(v) for v in d], dtype=object), np.array([int(v) for v in b], dtype=object))
        res = full[:N].copy()
        res[: N - 1] -= full[N:]
        out += res
    return out


def _check(digs, bks, limit):
    y = _fft_product_sum(digs, bks)
    exact = _exact_product_sum(digs, bks)
    rounded = np.rint(y)
    assert all(int(rounded[i]) == exact[i] for i in range(N))
    dev = float(np.abs(y - rounded).max())
    assert dev < limit, dev
    return dev


def test_random_operands_round_to_the_exact_product():
    rng = np.random.default_rng(1)
    worst = 0.0
    for _ in range(4):
        worst = max(worst, _check(rng.integers(-64, 64, size=(6, N)), rng.integers(-2**31, 2**31, size=(6, N)), 1 / 64))
    assert worst > 0  # the transform is approximate: what is being relied on is the margin, not exactness of the FFT


def test_extreme_magnitudes_and_worst_alignment():
    rng = np.random.default_rng(2)
    _check(rng.choice([-64, 63], size=(6, N)), rng.choice([-2**31, 2**31 - 1], size=(6, N)), 1 / 16)
    # every term of the same sign -- the largest sum the parameters allow (6 x 1024 x 64 x 2^31 = 2^49.6, where a double's
    # grid is 1/8 wide): no margin is left, the computed values sit up to half a step from an integer.  This is the case the
    # guard exists for: it sees a distance far above its limit and the call is repeated on the two-limb kernels.
    digs, bks = np.full((6, N), -64), np.full((6, N), -2**31)
    y = _fft_product_sum(digs, bks)
    exact = _exact_product_sum(digs, bks)
    assert max(abs(float(y[i]) - float(exact[i])) for i in range(N)) <= 1.0
    assert np.abs(y - np.rint(y)).max() > 1 / 16


def test_old_parameter_set_has_less_headroom():
    """l=2, Bgbit=10 (libtfhe 1.0): 10-bit digits, sums up to 2^52 -- why the evaluator keeps that set on the two-limb kernels."""
    rng = np.random.default_rng(3)
    y3 = _fft_product_sum(rng.integers(-64, 64, size=(6, N)), rng.integers(-2**31, 2**31, size=(6, N)))
    y2 = _fft_product_sum(rng.integers(-512, 512, size=(4, N)), rng.integers(-2**31, 2**31, size=(4, N)))
    d3, d2 = np.abs(y3 - np.rint(y3)).max(), np.abs(y2 - np.rint(y2)).max()
    assert d2 > 3 * d3


# ---- the two-limb external product of the any-parameter kernel (k_blind_rotate_generic), over the parameter lattice ----
# Every key polynomial is split into two balanced 16-bit limbs (low in [-2^15, 2^15), high in [-2^15, 2^15]); a CMux step
# multiplies kpl = 2l digit polynomials of magnitude 2^(Bgbit-1) with one limb each through ONE FP64 transform and rounds the
# sum.  The sum's magnitude is at most S = kpl x N x 2^(Bgbit-1) x 2^15.  A set (l, Bgbit, N) is accepted only if, on the
# "extreme magnitudes" and "worst alignment" inputs above, the model rounds to the exact integer product AND its worst
# distance to an integer stays under 1/16, the guard limit.  Params::br_exact() (csrc/params.h) states the outcome once:
# kpl x N x 2^Bgbit <= 2^32 (S <= 2^46, where a double's grid is 2^-7 wide and the model's worst distance is 1/32).

def _fft_product_sum_n(digs, bks, n):
    j = np.arange(n // 2)
    tw = np.exp(1j * np.pi * j / n)
    acc = np.zeros(n // 2, dtype=np.complex128)
    for d, b in zip(digs, bks):
        fd = np.fft.fft((d[: n // 2].astype(np.float64) + 1j * d[n // 2:].astype(np.float64)) * tw)
        fb = np.fft.fft((b[: n // 2].astype(np.float64) + 1j * b[n // 2:].astype(np.float64)) * tw)
        acc += fd * fb
    y = np.fft.ifft(acc) * np.conj(tw)
    return np.concatenate([y.real, y.imag])


def _exact_product_sum_n(digs, bks, n):
    """Exact in int64: the digits are cut at 16 bits, so that no partial sum passes 2^16 x 2^15 x kpl x N <= 2^47."""
    parts = [np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)]
    for d, b in zip(digs, bks):
        d = d.astype(np.int64)
        for part, out in zip((d & 0xFFFF, d >> 16), parts):
            full = np.convolve(part, b.astype(np.int64))
            out += full[:n]
            out[: n - 1] -= full[n:]
    return [int(lo) + (int(hi) << 16) for lo, hi in zip(*parts)]


def two_limb_model(l, Bgbit, n):
    """-> (rounds to the exact product on both inputs, worst distance to an integer)."""
    kpl, half = 2 * l, 1 << (Bgbit - 1)
    rng = np.random.default_rng(2)
    exact, worst = True, 0.0
    for digs, bks in ((rng.choice([-half, half - 1], size=(kpl, n)), rng.choice([-2**15, 2**15], size=(kpl, n))),  # extreme magnitudes
                      (np.full((kpl, n), -half), np.full((kpl, n), -2**15))):                                       # worst alignment
        y = _fft_product_sum_n(digs, bks, n)
        want = _exact_product_sum_n(digs, bks, n)
        rounded = np.rint(y)
        exact = exact and all(int(rounded[i]) == want[i] for i in range(n))
        worst = max(worst, float(np.abs(y - rounded).max()))
    return exact, worst


def br_exact(l, Bgbit, n):
    """Params::br_exact() restated (tests/native/ks_plan_test.cpp holds the C++ to the same boundary)."""
    return Bgbit < 32 and 2 * l * n * (1 << Bgbit) <= 1 << 32


RINGS = (16, 32, 64, 128, 256, 512, 1024)


def lattice_candidates():
    """Every l = 1 set (the only ones whose sums come near the bound) and, for each l >= 2, its largest Bgbit on the largest
    ring and on the smallest: a sum grows with each of kpl, N and Bgbit, so these bound the rest."""
    sets = [(1, b, n) for n in RINGS for b in range(1, 33)]
    sets += [(l, 32 // l, n) for l in range(2, 33) for n in (16, 1024)]
    return sets


def test_two_limb_product_is_exact_on_every_accepted_set():
    accepted = [s for s in lattice_candidates() if br_exact(*s)]
    assert len(accepted) > 200
    for l, Bgbit, n in accepted:
        exact, worst = two_limb_model(l, Bgbit, n)
        assert exact and worst < 1 / 16, (l, Bgbit, n, worst)


def test_the_bound_is_where_the_model_puts_it():
    """The bound is the model's, not a guess: one Bgbit past it the worst distance reaches the guard limit (l = 1, N = 512:
    2^-4 exactly, the grid of a double at 2^48), and from S = 2^51 on the rounded value is no longer the product."""
    for n in RINGS:
        b = max(bg for bg in range(1, 33) if br_exact(1, bg, n))
        assert b == 31 - (n.bit_length() - 1)
        assert two_limb_model(1, b, n)[1] <= 1 / 32
    exact, worst = two_limb_model(1, 23, 512)
    assert exact and worst >= 1 / 16
    for n in RINGS[1:]:
        assert not two_limb_model(1, 32, n)[0]
    # nothing with l >= 2 comes near: l x Bgbit <= 32 keeps those sums at or below 2^42
    assert max(two_limb_model(l, 32 // l, 1024)[1] for l in (2, 3, 4)) < 1 / 256


if __name__ == "__main__":  # the table of profiles/param_lattice.txt
    print("# l Bgbit N  log2(kpl N 2^Bgbit)  accepted  exact  worst distance to an integer")
    for l, Bgbit, n in lattice_candidates():
        exact, worst = two_limb_model(l, Bgbit, n)
        print("%2d %2d %4d  %4.1f  %s  %s  %.3g" % (l, Bgbit, n, np.log2(2 * l * n) + Bgbit, "yes" if br_exact(l, Bgbit, n) else "no ",
                                                   "yes" if exact else "NO ", worst))
