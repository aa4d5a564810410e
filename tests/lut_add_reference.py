"""Many values into shared memories (include/ieache.h section 3j) restated in numpy from rotate_reference.tlwe_rotate and
scatter_reference.demux: the rotation by the low selectors with the write's amounts, the demux by the high ones, the leaves
summed per memory.  It shares no code with the C reference (csrc/tfhe_host.cpp) or the kernels.  Test support only."""
import numpy as np

import rotate_reference as RR
import scatter_reference as SR


def default_amounts(steps, N):
    """a_t = +2^t mod 2N: coefficient 0 goes to the encrypted position; 0 once 2^t reaches 2N"""
    return [(1 << t) % (2 * N) for t in range(steps)]


def lut_add(samples, values, depth, steps, l, Bgbit, sel_of=None, amounts=None, mems=None, n_mems=1, mem_of=None, clamp=False):
    """item i: selectors sel_of[i] ([count][steps + depth], the low bits first; None: (i (steps + depth) + t) mod n; clamp: as
    the device clamps indices and memories) -> [n_mems][2^depth][2][N]"""
    values = np.asarray(values, dtype=np.int32)
    n, N, count, stride = len(samples), values.shape[-1], len(values), depth + steps
    if stride == 0:
        of = np.zeros((count, 1), dtype=np.int64)  # no selectors at all
    else:
        of = (np.arange(count * stride).reshape(count, stride) % n) if sel_of is None else np.asarray(sel_of).reshape(count, stride)
    if clamp:
        of = np.clip(of, 0, n - 1)
    am = default_amounts(steps, N) if amounts is None else [int(a) for a in amounts]
    if mems is not None:
        mems = np.asarray(mems, dtype=np.int32).reshape(-1, 1 << depth, 2, N)
        n_mems = mems.shape[0]
    out = np.zeros((n_mems, 1 << depth, 2, N), dtype=np.int32) if mems is None else mems.copy()
    turned = RR.tlwe_rotate(samples, values, steps, l, Bgbit, sel_of=of, amounts=am, stride=stride)
    for i in range(count):
        m = 0 if mem_of is None else int(np.asarray(mem_of).reshape(-1)[i])
        if clamp:
            m = min(max(m, 0), n_mems - 1)
        out[m] = SR.add32(out[m], SR.demux(samples, turned[i], [int(s) for s in of[i, steps:steps + depth]], l, Bgbit))
    return out
