"""The write at an encrypted index of include/ieache.h section 3g restated in numpy on cmux_reference.external_product: the demux
from the most significant selector down, the memory added to the leaves.  It shares no code with the C reference
(csrc/tfhe_host.cpp) or the kernels.  Test support only."""
import numpy as np

from cmux_reference import external_product
from np_tfhe import _wrap32


def sub32(a, b):
    return _wrap32(np.asarray(a, dtype=np.int64) - np.asarray(b, dtype=np.int64))


def add32(a, b):
    return _wrap32(np.asarray(a, dtype=np.int64) + np.asarray(b, dtype=np.int64))


def demux(samples, v, sels, l, Bgbit):
    """the 2^depth leaves of one item: sels[k] is the sample of bit k of the index; the row at position j becomes
    hi = C (.) row at 2 j + 1 and row - hi at 2 j, selector depth - 1 first"""
    rows = [np.asarray(v, dtype=np.int32)]
    for k in reversed(range(len(sels))):
        nxt = []
        for p in rows:
            hi = external_product(samples[sels[k]], p, l, Bgbit)
            nxt += [sub32(p, hi), hi]
        rows = nxt
    return np.stack(rows)


def lut_scatter(samples, values, depth, l, Bgbit, sel_of=None, mem=None, clamp=False):
    """the call: item i with samples sel_of[i][k] (None: (i depth + k) mod n; clamp: indices clamped into the set as the device
    does) -> mem[i] + leaves, [count][2^depth][2][N]"""
    n = len(samples)
    values = np.asarray(values, dtype=np.int32)
    out = []
    for i in range(len(values)):
        if sel_of is None:
            sels = [(i * depth + k) % n for k in range(depth)]
        else:
            sels = [int(s) for s in np.asarray(sel_of).reshape(-1, max(depth, 1))[i, :depth]]
            if clamp:
                sels = [min(max(s, 0), n - 1) for s in sels]
        leaves = demux(samples, values[i], sels, l, Bgbit)
        out.append(leaves if mem is None else add32(np.asarray(mem)[i], leaves))
    return np.stack(out) if out else np.zeros((0, 1 << depth) + values.shape[1:], dtype=np.int32)
