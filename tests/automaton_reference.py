"""The automaton evaluation of include/ieache.h section 3k restated in numpy on the CMux of cmux_reference.py: exact integer
arithmetic, sharing no code with the C reference (csrc/tfhe_host.cpp) or the kernels.  Every state of every step is computed --
no liveness, no copies -- so it also checks that the kernel's two shortcuts change nothing.  Test support only."""
import numpy as np

import cmux_reference as CR


def run(samples, next0, next1, finals, l, Bgbit, n_out=1, sel_of=None, final_of=None, count=1, clamp=False):
    """samples [n][2l][2][N], tables [steps][states], finals [n_finals][states][2][N] -> [count][n_out][2][N]; item i's letter t
    is sample sel_of[i][t] (None: (i steps + t) mod n; clamp: indices clamped as the device does), its finals finals[final_of[i]]
    (None: 0)"""
    next0, next1 = np.asarray(next0, dtype=np.int64), np.asarray(next1, dtype=np.int64)
    steps, states = next0.shape
    finals = np.asarray(finals, dtype=np.int32).reshape(-1, states, 2, np.shape(finals)[-1])
    n = len(samples)
    out = []
    for i in range(count):
        f = 0 if final_of is None else int(final_of[i])
        if clamp:
            f = min(max(f, 0), len(finals) - 1)
        v = [finals[f, q] for q in range(states)]
        for t in reversed(range(steps)):
            s = (i * steps + t) % n if sel_of is None else int(np.asarray(sel_of).reshape(-1, steps)[i, t])
            if clamp:
                s = min(max(s, 0), n - 1)
            v = [CR.cmux(samples[s], v[next1[t, q]], v[next0[t, q]], l, Bgbit) for q in range(states)]
        out.append(np.stack(v[:n_out]))
    return np.stack(out)


def random_tables(rng, steps, states):
    """step-dependent random tables with self-loops, next0 == next1 entries and states nothing leads to among them"""
    next0 = rng.integers(0, states, size=(steps, states)).astype(np.int32)
    next1 = rng.integers(0, states, size=(steps, states)).astype(np.int32)
    for t in range(steps):
        next0[t, t % states] = t % states                     # a self-loop on letter 0
        next1[t, (t + 1) % states] = next0[t, (t + 1) % states]  # a state whose letters agree
    return next0, next1
