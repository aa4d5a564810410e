#!/usr/bin/env python3
"""Blind rotations per second of a worked-example netlist (ieache_amd.netlists) over a batch, or -- for comparison on the same
card in the same run -- of a built-in circuit kind.

    python scripts/netlist_rate.py minmax 32 1024
    python scripts/netlist_rate.py divmod 32 64 --balanced
    python scripts/netlist_rate.py --builtin 4 32 1024        # CIRC_MUL
    python scripts/netlist_rate.py --builtin 1 16 4096        # CIRC_ADD

The rate is ieache_stats.bootstraps / ieache_stats.total_ms (GPU timeline) of each warm call; median and spread over --calls
calls after --warm unrecorded ones.  Random operands: the gate sequence does not depend on the data.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", help="compare | minmax | divmod, or with --builtin the circuit kind number")
    ap.add_argument("bits", type=int)
    ap.add_argument("batch", type=int)
    ap.add_argument("--builtin", action="store_true")
    ap.add_argument("--balanced", action="store_true")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warm", type=int, default=4, help="unrecorded calls first (pipe_auto tries both stream modes in four)")
    ap.add_argument("--n", type=int, default=0, help="LWE dimension (0 = the default parameter set)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    import ieache_amd as ia
    from ieache_amd import tools
    p = ia.default_params()
    if a.n:
        p = p.copy(n=a.n)
    k = tools.keygen_raw(p, (1, 2, 3))
    rng = np.random.default_rng(1)
    with ia.Context.from_arrays(p, k["bk"], k["ksk"], device=a.device) as ctx:
        if a.builtin:
            kind = int(a.what)
            info = ia.circuit_info(kind, a.bits)
            bits = np.zeros((a.batch, info.n_inputs), dtype=np.uint8)
            bits[:, :2 * a.bits] = rng.integers(0, 2, size=(a.batch, 2 * a.bits))
            inp = tools.encrypt_bits(p, k["lwe_key"], bits, 9)
            ctx.prepare(kind, a.bits, a.batch)
            run = lambda st: ctx.eval_batch(kind, a.bits, inp, st)  # noqa: E731
            name = "builtin%d" % kind
        else:
            from ieache_amd import netlists
            cn = getattr(netlists, a.what)(a.bits, balanced=a.balanced)
            info = cn.info()
            bits = rng.integers(0, 2, size=(a.batch, info.n_inputs)).astype(np.uint8)
            inp = tools.encrypt_bits(p, k["lwe_key"], bits, 9)
            ctx.prepare_netlist(cn, a.batch)
            run = lambda st: ctx.eval_netlist(cn, inp, st)  # noqa: E731
            name = a.what + ("_balanced" if a.balanced else "")
        for _ in range(a.warm):
            run(None)
        rates, ms = [], []
        for _ in range(a.calls):
            st = ia.Stats()
            out = run(st)
            assert st.bootstraps == a.batch * info.bootstraps
            rates.append(st.bootstraps / (st.total_ms * 1e-3))
            ms.append(st.total_ms)
        if not a.builtin:  # and the answers are right
            dec = tools.decrypt_bits(p, k["lwe_key"], out[:8])
            assert all(np.array_equal(dec[e], cn.simulate(bits[e])) for e in range(min(8, a.batch)))
        print(json.dumps({"circuit": name, "bits": a.bits, "batch": a.batch, "n": p.n, "rotations_per_expression": int(info.bootstraps),
                          "levels": int(info.sched_levels), "widest_level_rotations": int(info.sched_max_width) * a.batch,
                          "mean_level_rotations": round(info.bootstraps * a.batch / max(info.sched_levels, 1), 1),
                          "total_ms_median": round(float(np.median(ms)), 3), "rotations_per_s_median": round(float(np.median(rates))),
                          "rotations_per_s_min": round(min(rates)), "rotations_per_s_max": round(max(rates)), "calls": a.calls,
                          "pipelined_evals": ctx.get_option("pipelined_evals"), "mixed_launches": ctx.get_option("mixed_launches")}))


if __name__ == "__main__":
    main()
