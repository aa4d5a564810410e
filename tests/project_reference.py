"""The TLWE projection and the replace write of a window (include/ieache.h section 3l) restated in numpy: the extraction by the
rule of section 3f, pack_reference.pack on the parameter set with n := N, and the write composed from cmux_reference.lut_tree,
rotate_reference.tlwe_rotate and lut_add_reference.lut_add.  It shares no code with the C references (csrc/tfhe_host.cpp) or the
kernels.  Test support only."""
import numpy as np

import cmux_reference as CR
import lut_add_reference as AR
import pack_reference as PR
import rotate_reference as RR
from np_tfhe import _wrap32


def extract(sample, j):
    """coefficient j of a TLWE sample [2][N] as an extracted row [N + 1]: u[i] = A[j - i] for i <= j, -A[N + j - i] above, u[N] = B[j]"""
    A, B = np.asarray(sample[0], dtype=np.int64), np.asarray(sample[1], dtype=np.int64)
    N = A.shape[0]
    u = np.empty(N + 1, dtype=np.int64)
    for i in range(N):
        u[i] = A[j - i] if i <= j else -A[N + j - i]
    u[N] = B[j]
    return _wrap32(u)


def window_rows(samples, first, width):
    """the extracted rows of the windows: [count][width][N + 1]"""
    samples = np.asarray(samples, dtype=np.int32)
    return np.stack([np.stack([extract(s, first + q) for q in range(width)]) for s in samples])


def project(pk, samples, first, width, dest, t=8, basebit=2, fast=False):
    """the call: pk [N][t][2][N], samples [count][2][N] -> [count][2][N], one group of `width` rows per sample, spread 1.
    fast: pack_reference.product_fast in place of the int64 product (tests/test_pack_cpu.py holds the two equal)."""
    samples = np.asarray(samples, dtype=np.int32)
    N = samples.shape[-1]
    rows = window_rows(samples, first, width).reshape(-1, N + 1)
    if not fast:
        return PR.pack(pk, rows, width, spread=1, shift=dest, t=t, basebit=basebit)
    return PR.place(PR.spread_sums(PR.product_fast(pk, rows, t, basebit), 1), samples.shape[0], width, 1, dest)


def amounts(steps, unit, N, toward_zero):
    w = [(unit << s) % (2 * N) for s in range(steps)]
    return [(2 * N - a) % (2 * N) for a in w] if toward_zero else w


def lut_write_coef(samples, pk, mem, depth, steps, new, width, unit, l, Bgbit, sel_of=None, t=8, basebit=2, fast=False):
    """mem [count][2^depth][2][N], new [count][2][N]; selectors sel_of [count][steps + depth], the low bits first (None: (i
    (steps + depth) + k) mod n) -> the new memories"""
    mem = np.asarray(mem, dtype=np.int32)
    new = np.asarray(new, dtype=np.int32)
    n, count, N, stride = len(samples), mem.shape[0], mem.shape[-1], depth + steps
    if stride == 0:
        of = np.zeros((count, 1), dtype=np.int64)  # no selectors at all
    else:
        of = (np.arange(count * stride).reshape(count, stride) % n) if sel_of is None else np.asarray(sel_of).reshape(count, stride)
    picked = CR.lut_tree(samples, mem, depth, l, Bgbit, sel_of=of[:, steps:steps + depth] if depth else None, table_of=np.arange(count), count=count)
    turned = RR.tlwe_rotate(samples, picked, steps, l, Bgbit, sel_of=of, amounts=amounts(steps, unit, N, True), stride=stride)
    old = project(pk, turned, 0, width, 0, t, basebit, fast)
    delta = _wrap32(new.astype(np.int64) - old.astype(np.int64))
    return AR.lut_add(samples, delta, depth, steps, l, Bgbit, sel_of=of if stride else None, amounts=amounts(steps, unit, N, False), mems=mem,
                      mem_of=np.arange(count))
