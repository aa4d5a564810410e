"""The unpacking key switch and the read of an addressed word of include/ieache.h section 3m restated in numpy: the extraction
rule written out, the LWE key switch as a digit walk in int64, and word_read composed from cmux_reference.lut_tree and
rotate_reference.tlwe_rotate.  Exact integer arithmetic, sharing no code with the C reference (csrc/tfhe_host.cpp) or the
kernels.  Test support only."""
import numpy as np

import cmux_reference as CR
import rotate_reference as RR


def wrap32(x):
    return (np.asarray(x, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def window_rows(samples, first, width, spread):
    """[count][2][N] -> [count][width][N + 1]: row (i, q) is the extracted row of coefficient c = first + q spread of sample i:
    entry j is A[c - j] for j <= c and -A[N + c - j] above, the last word B[c]"""
    samples = np.asarray(samples, dtype=np.int32).reshape(-1, 2, np.asarray(samples).shape[-1])
    count, _, N = samples.shape
    out = np.zeros((count, width, N + 1), dtype=np.int64)
    j = np.arange(N)
    for q in range(width):
        c = first + q * spread
        assert 0 <= c < N
        A = samples[:, 0, :].astype(np.int64)
        out[:, q, :N] = np.where(j <= c, A[:, (c - j) % N], -A[:, (N + c - j) % N])
        out[:, q, N] = samples[:, 1, c]
    return wrap32(out)


def keyswitch(ksk, t, basebit, u):
    """lweKeySwitch as a walk: per row out = (0, .., 0, u[N]), then for every coefficient i and position j the row
    ksk[i][j][digit] subtracted where the digit -- bits [32 - (j+1) basebit, 32 - j basebit) of u[i] + 2^(31 - t basebit) -- is
    not 0.  ksk [N][t][base][n+1], u [..][N+1] -> [..][n+1]."""
    ksk = np.asarray(ksk, dtype=np.int32)
    u = np.asarray(u, dtype=np.int32)
    N, n1 = ksk.shape[0], ksk.shape[3]
    flat = u.reshape(-1, N + 1)
    out = np.zeros((flat.shape[0], n1), dtype=np.int64)
    out[:, n1 - 1] = flat[:, N]
    key = ksk.astype(np.int64)
    abar = (flat[:, :N].astype(np.int64) + (1 << (32 - (1 + basebit * t)))) & 0xFFFFFFFF
    for r in range(flat.shape[0]):
        for j in range(t):
            d = (abar[r] >> (32 - (j + 1) * basebit)) & ((1 << basebit) - 1)
            i = np.nonzero(d)[0]
            out[r] -= key[i, j, d[i]].sum(axis=0)
    return wrap32(out).reshape(u.shape[:-1] + (n1,))


def unpack(samples, first, width, spread, ksk=None, ks=None):
    """-> [count][width][n+1] with ksk and ks = (t, basebit); the extracted rows [count][width][N+1] without"""
    u = window_rows(samples, first, width, spread)
    return u if ksk is None else keyswitch(ksk, ks[0], ks[1], u)


def word_amounts(steps, unit, N):
    return [(2 * N - ((unit << t) % (2 * N))) % (2 * N) for t in range(steps)]


def word_read(samples, tables, depth, steps, width, unit, l, Bgbit, sel_of=None, table_of=None, count=1, ksk=None, ks=None):
    """the tree by selectors steps .. steps+depth-1 of each item, the rotation by selectors 0 .. steps-1 with the amounts
    2N - unit 2^t, and the window (0, width, 1) of the rotated rows unpacked"""
    tables = np.asarray(tables, dtype=np.int32)
    n, N = len(samples), tables.shape[-1]
    stride = depth + steps
    if stride == 0:
        of = np.zeros((count, 1), dtype=np.int64)
    else:
        of = (np.arange(count * stride).reshape(count, stride) % n) if sel_of is None else np.asarray(sel_of).reshape(count, stride)
    picked = CR.lut_tree(samples, tables, depth, l, Bgbit, sel_of=of[:, steps:steps + depth] if depth else None, table_of=table_of, count=count)
    turned = RR.tlwe_rotate(samples, picked, steps, l, Bgbit, sel_of=of, amounts=word_amounts(steps, unit, N), stride=stride)
    return unpack(turned, 0, width, 1, ksk=ksk, ks=ks)
