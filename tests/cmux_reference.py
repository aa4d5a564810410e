"""The external product, the CMux and the CMux tree of include/ieache.h section 3f restated in numpy: exact integer arithmetic
(int64 convolutions where the sums fit, Python integers where they do not), sharing no code with the C reference
(csrc/tfhe_host.cpp) or the kernels.  Test support only."""
import numpy as np

from np_tfhe import _wrap32


def full_range(rng, shape):
    """int32 words over the whole range, the extremes included"""
    return rng.integers(-(1 << 31), 1 << 31, size=shape, dtype=np.int64).astype(np.int32)


def offset(l, Bgbit):
    return sum((1 << (Bgbit - 1)) << (32 - q * Bgbit) for q in range(1, l + 1)) & 0xFFFFFFFF


def digits(poly, l, Bgbit):
    """[l][N] signed digits q = 1 .. l of a polynomial of int32 words"""
    w = ((np.asarray(poly, dtype=np.int64) & 0xFFFFFFFF) + offset(l, Bgbit)) & 0xFFFFFFFF
    return np.stack([((w >> (32 - q * Bgbit)) & ((1 << Bgbit) - 1)) - (1 << (Bgbit - 1)) for q in range(1, l + 1)])


def negacyclic(small, big, exact_int64):
    """small x big mod X^N + 1 over the integers (before any wrap)"""
    N = small.shape[0]
    if exact_int64:
        full = np.convolve(small.astype(np.int64), big.astype(np.int64))
    else:
        full = np.convolve(small.astype(object), big.astype(object))
    res = full[:N].copy()
    res[:N - 1] -= full[N:]
    return res


def external_product(C, d, l, Bgbit):
    """C [2l][2][N] (.) d [2][N] -> [2][N] int32 words"""
    C = np.asarray(C, dtype=np.int32)
    d = np.asarray(d, dtype=np.int32)
    N = d.shape[-1]
    fits = 2 * l * N * (1 << (Bgbit - 1)) * (1 << 31) < (1 << 62)
    acc = [0, 0]
    for c in range(2):
        dig = digits(d[c], l, Bgbit)
        for q in range(l):
            for o in range(2):
                acc[o] = acc[o] + negacyclic(dig[q], C[c * l + q, o], fits)
    return np.stack([_wrap32(np.array([int(v) & 0xFFFFFFFF for v in a], dtype=np.int64)) for a in acc])


def cmux(C, d1, d0, l, Bgbit):
    """d0 + C (.) (d1 - d0); d0 None: zeros"""
    d1 = np.asarray(d1, dtype=np.int32)
    d0 = np.zeros_like(d1) if d0 is None else np.asarray(d0, dtype=np.int32)
    diff = _wrap32(d1.astype(np.int64) - d0.astype(np.int64))
    return _wrap32(d0.astype(np.int64) + external_product(C, diff, l, Bgbit).astype(np.int64))


def cmux_rows(samples, d1, d0, l, Bgbit, sel_of=None, clamp=False):
    """the flat call: row i with sample sel_of[i] (None: i mod n; clamp: indices clamped into the set as the device does)"""
    n = len(samples)
    out = []
    for i in range(len(d1)):
        s = i % n if sel_of is None else int(sel_of[i])
        if clamp:
            s = min(max(s, 0), n - 1)
        out.append(cmux(samples[s], d1[i], None if d0 is None else d0[i], l, Bgbit))
    return np.stack(out) if out else np.zeros((0,) + tuple(np.shape(d1)[1:]), dtype=np.int32)


def lut_tree(samples, tables, depth, l, Bgbit, sel_of=None, table_of=None, count=1):
    """the tree: item i folds tables[table_of[i]] by selectors sel_of[i][k] (None: (i depth + k) mod n), bit 0 first"""
    n = len(samples)
    out = []
    for i in range(count):
        rows = list(np.asarray(tables[0 if table_of is None else int(table_of[i])], dtype=np.int32))
        assert len(rows) == 1 << depth
        for k in range(depth):
            s = (i * depth + k) % n if sel_of is None else int(np.asarray(sel_of).reshape(-1, depth)[i, k])
            rows = [cmux(samples[s], rows[2 * j + 1], rows[2 * j], l, Bgbit) for j in range(len(rows) // 2)]
        out.append(rows[0])
    return np.stack(out)


def all_digits_word(l, Bgbit, digit):
    """the int32 word x whose every digit dig_q(x) is `digit` (-2^(Bgbit-1) .. 2^(Bgbit-1) - 1); the bits below the last
    digit's field are zero"""
    half = 1 << (Bgbit - 1)
    w = sum((digit + half) << (32 - q * Bgbit) for q in range(1, l + 1))
    x = (w - offset(l, Bgbit)) & 0xFFFFFFFF
    return int(np.array([x], dtype=np.uint32).view(np.int32)[0])
