"""The rotation by an encrypted amount and the coefficient-level lookup of include/ieache.h section 3h restated in numpy on top of
cmux_reference.external_product, with an explicit negacyclic monomial shift: exact integer arithmetic, sharing no code with
the C reference (csrc/tfhe_host.cpp) or the kernels.  Test support only."""
import numpy as np

import cmux_reference as CR
from np_tfhe import _wrap32, np_keyswitch


def monomial(row, a):
    """X^a row for a in [0, 2N): coefficient j takes +/- coefficient j - a mod 2N of the 2N-ring [row, -row]"""
    row = np.asarray(row, dtype=np.int32)
    N = row.shape[-1]
    src = (np.arange(N) - int(a)) % (2 * N)
    taken = row[..., src % N].astype(np.int64)
    return _wrap32(np.where(src >= N, -taken, taken))


def default_amounts(steps, N):
    """a_t = 2N - 2^t mod 2N: 0 once 2^t reaches 2N"""
    return [(2 * N - (1 << t)) % (2 * N) for t in range(steps)]


def rotate_step(C, acc, a, l, Bgbit):
    """acc + C (.) (X^a acc - acc)"""
    diff = _wrap32(monomial(acc, a).astype(np.int64) - acc.astype(np.int64))
    return _wrap32(acc.astype(np.int64) + CR.external_product(C, diff, l, Bgbit).astype(np.int64))


def tlwe_rotate(samples, rows, steps, l, Bgbit, sel_of=None, amounts=None, stride=None, clamp=False):
    """row i through steps 0 .. steps-1 with sample sel_of[i][t] (None: (i stride + t) mod n; clamp: as the device clamps)"""
    rows = np.asarray(rows, dtype=np.int32)
    n, N = len(samples), rows.shape[-1]
    stride = steps if stride is None else stride
    am = default_amounts(steps, N) if amounts is None else [int(a) for a in amounts]
    of = None if sel_of is None else np.asarray(sel_of).reshape(-1, max(stride, 1))
    out = []
    for i in range(rows.shape[0]):
        acc = rows[i]
        for t in range(steps):
            s = (i * stride + t) % n if of is None else int(of[i, t])
            if clamp:
                s = min(max(s, 0), n - 1)
            acc = rotate_step(samples[s], acc, am[t] % (2 * N), l, Bgbit)
        out.append(acc)
    return np.stack(out) if out else np.zeros((0, 2, N), dtype=np.int32)


def extract(row, j):
    """coefficient j of a TLWE sample as an extracted row [N + 1]"""
    A, B = np.asarray(row[0], dtype=np.int64), row[1]
    N = A.shape[0]
    i = np.arange(N)
    return _wrap32(np.concatenate([np.where(i <= j, A[(j - i) % N], -A[(N + j - i) % N]), [int(B[j])]]))


def lut_read(samples, tables, depth, steps, l, Bgbit, sel_of=None, amounts=None, table_of=None, coef=0, count=1, ksk=None, ks=None):
    """the lookup: the tree by selectors steps .. steps+depth-1, the rotation by selectors 0 .. steps-1, coefficient `coef`,
    and np_keyswitch with ks = (t, basebit) where ksk is given"""
    n = len(samples)
    stride = depth + steps
    of = (np.arange(count * stride).reshape(count, max(stride, 1)) % n) if sel_of is None else np.asarray(sel_of).reshape(count, max(stride, 1))
    picked = CR.lut_tree(samples, tables, depth, l, Bgbit, sel_of=of[:, steps:steps + depth] if depth else None, table_of=table_of, count=count)
    turned = tlwe_rotate(samples, picked, steps, l, Bgbit, sel_of=of, amounts=amounts, stride=stride)
    u = np.stack([extract(r, coef) for r in turned])
    return u if ksk is None else np_keyswitch(ksk, ks[0], ks[1], u)
