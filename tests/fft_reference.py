"""The 512-point negacyclic transform of the N = 1024 kernels (csrc/fft512.h) as its defining sum in extended precision: what
tests/test_fft_probe_gpu.py measures the kernels against, and what tests/test_fft_reference_cpu.py proves first.

Convention (csrc/tw_roots.h): a polynomial p of 1024 real coefficients is folded to y_j = p[j] + i p[j + 512], twisted by
e^{+i pi j / 1024} and transformed with e^{-2 pi i j k / 512}:

    X_k = sum_j y_j exp(i pi j (1 - 4 k) / 1024),          y_j = (1 / 512) sum_k X_k exp(-i pi j (1 - 4 k) / 1024)

The roots exp(i pi e / 1024), e = 0 .. 2047, come from mpmath at 120 bits and are rounded once to np.longdouble (64-bit
mantissa on x86); the matrix of the sum is indexed by the exact integer j (1 - 4 k) mod 2048, so no angle is ever rounded.
Everything is numpy on clongdouble: sums of 512 terms carry about 2^-60 of relative error, 2^7 below a double's 2^-53.

Also here: the kernels' (register, lane) output order and the any-parameter kernel's bit-reversed order, the balanced 16-bit
limb split of a key word restated from the kernels' three lines, exact negacyclic products in Python integers, and the error of
the numpy double model of tests/test_rounding_model_cpu.py against this reference -- the yardstick the kernels are held to."""
import functools

import mpmath
import numpy as np

import test_rounding_model_cpu as model

N, M = 1024, 512
U53 = 2.0 ** -53  # the unit errors are quoted in
IMPULSE_SLOTS = (0, 1, 63, 64, 65, 511, 512, 513, 1023)  # coefficient indices: >= 512 are the imaginary slots


def _longdouble(x):
    """An mpmath real, rounded to np.longdouble through two doubles (106 bits carried, 64 kept)."""
    hi = float(x)
    return np.longdouble(hi) + np.longdouble(float(x - hi))


@functools.lru_cache(maxsize=None)
def roots(n=N):
    """exp(i pi e / n) for e = 0 .. 2n - 1, clongdouble; cospi / sinpi make the multiples of pi/2 exact."""
    with mpmath.workprec(120):
        out = np.empty(2 * n, dtype=np.clongdouble)
        for e in range(2 * n):
            t = mpmath.mpf(e) / n
            out[e] = _longdouble(mpmath.cospi(t)) + 1j * _longdouble(mpmath.sinpi(t))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def forward_matrix(n=N):
    """F[k, j] = exp(i pi j (1 - 4 k) / n), [n/2][n/2] clongdouble."""
    m = n // 2
    k, j = np.arange(m, dtype=np.int64)[:, None], np.arange(m, dtype=np.int64)[None, :]
    F = roots(n)[(j * (1 - 4 * k)) % (2 * n)]
    F.setflags(write=False)
    return F


def fold(p):
    """[.. n] real coefficients -> [.. n/2] clongdouble y_j = p[j] + i p[j + n/2]"""
    p = np.asarray(p)
    m = p.shape[-1] // 2
    return p[..., :m].astype(np.longdouble) + 1j * p[..., m:].astype(np.longdouble)


def unfold(y):
    return np.concatenate([y.real, y.imag], axis=-1)


def forward(y):
    """[.. n/2] complex -> [.. n/2] clongdouble spectrum X_k, k natural"""
    y = np.asarray(y, dtype=np.clongdouble)
    return (forward_matrix(2 * y.shape[-1]) @ y[..., None])[..., 0]


def inverse(X):
    """The inverse with the 1/(n/2) and the untwist: [.. n/2] spectrum -> [.. n/2] clongdouble y_j"""
    X = np.asarray(X, dtype=np.clongdouble)
    m = X.shape[-1]
    return (np.conj(forward_matrix(2 * m)).T @ X[..., None])[..., 0] / np.longdouble(m)


def impulse(slot):
    """y of the polynomial X^slot: 1 at j = slot, or i at j = slot - 512"""
    y = np.zeros(M, dtype=np.complex128)
    y[slot % M] = 1.0 if slot < M else 1.0j
    return y


def impulse_spectrum(slot):
    """Closed form: one root of unity per k, times i for an imaginary slot."""
    k = np.arange(M, dtype=np.int64)
    X = roots()[((slot % M) * (1 - 4 * k)) % (2 * N)]
    return X if slot < M else 1j * X


# ---- orders ----
# fft512_forward: out[k2][lane] = X[k0 + 8 k1 + 64 k2] with lane = 8 k0 + k1
REG_LANE = np.array([[(lane >> 3) + 8 * (lane & 7) + 64 * k2 for lane in range(64)] for k2 in range(8)])


def to_reg_lane(X):
    """[.. 512] natural -> [.. 8][64] as the forward transform leaves it in registers"""
    return np.asarray(X)[..., REG_LANE]


def from_reg_lane(out):
    out = np.asarray(out)
    X = np.empty(out.shape[:-2] + (M,), dtype=out.dtype)
    X[..., REG_LANE] = out
    return X


def bit_reversed(m):
    """indices r with r[i] = bit reversal of i over log2(m) bits: the any-parameter kernel stores X[r[i]] at i"""
    bits = m.bit_length() - 1
    assert 1 << bits == m
    return np.array([int(format(i, "0%db" % bits)[::-1], 2) if bits else 0 for i in range(m)])


# ---- the key's limbs ----
def limb_split(w):
    """k_bk_to_spectrum's three lines: lo = (int16_t)(w & 0xFFFF); hi = ((int64_t)w - lo) >> 16.  w: int32 words (any integer
    array holding them, or their unsigned bit patterns) -> (lo, hi) int64."""
    w = np.asarray(w, dtype=np.int64)
    w = ((w + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)  # as int32
    lo = (w & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int64)
    return lo, (w - lo) >> 16


# ---- exact products ----
def exact_product_sum(digs, bks):
    """sum over rows of digs[row] * bks[row] mod X^n + 1 in Python integers, as test_rounding_model_cpu._exact_product_sum"""
    n = len(digs[0])
    out = np.zeros(n, dtype=object)
    for d, b in zip(digs, bks):
        full = np.convolve(np.array([int(v) for v in d], dtype=object), np.array([int(v) for v in b], dtype=object))
        res = full[:n].copy()
        res[: n - 1] -= full[n:]
        out += res
    return out


def reference_product_sum(digs, bks):
    """The same through the reference transform: forward, pointwise product, inverse -> [n] longdouble"""
    acc = 0
    for d, b in zip(digs, bks):
        acc = acc + forward(fold(d)) * forward(fold(b))
    return unfold(inverse(acc))


# ---- the numpy double model and error measures ----
def model_forward(p):
    """The transform of test_rounding_model_cpu._fft_product_sum_n (numpy double, pocketfft) of coefficients p [n] -> X_k"""
    p = np.asarray(p)
    m = p.shape[-1] // 2
    tw = np.exp(1j * np.pi * np.arange(m) / (2 * m))
    return np.fft.fft((p[:m].astype(np.float64) + 1j * p[m:].astype(np.float64)) * tw)


def spectrum_errors(X, ref):
    """(relative L2 error, largest single error over rms |ref|), both in units of 2^-53.  X: complex128; ref: clongdouble."""
    d = np.abs(np.asarray(X).astype(np.clongdouble) - ref)
    a = np.abs(ref)
    l2 = float(np.sqrt((d * d).sum() / (a * a).sum()))
    peak = float(d.max() / np.sqrt((a * a).mean()))
    return l2 / U53, peak / U53


def model_product_sum(digs, bks):
    n = len(digs[0])
    return model._fft_product_sum_n(np.asarray(digs), np.asarray(bks), n)


def rounding_distance(y):
    """largest distance of the pre-rounding doubles from an integer"""
    y = np.asarray(y, dtype=np.float64)
    return float(np.abs(y - np.rint(y)).max())


def rounds_to(y, exact):
    y = np.rint(np.asarray(y, dtype=np.float64))
    return all(int(y[i]) == exact[i] for i in range(len(exact)))
