#!/usr/bin/env python3
"""Flat programmable-bootstrap calls beside flat gate calls of the same size, on one card in one run:

  * Context.pbs of 256 / 1 024 / 8 192 rows (a four-entry table, mixed row indices) and Context.gates (AND) of as many
    gates, by turns; bootstraps/s from ieache_stats.total_ms, the GPU timeline of a warm call;
  * the same pbs call without the key switch;
  * the decode of the table's outputs, checked before anything is timed.

    python scripts/pbs_rates.py [--out profiles/pbs_rates.txt] [--calls 5]

Median and range over --calls recorded calls after --warm unrecorded ones."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pbs_rates.txt"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--sizes", default="256,1024,8192")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]

    import ieache_amd as ia
    from ieache_amd import tools
    p = ia.default_params()
    k = tools.keygen_raw(p, (1, 2, 3))
    rng = np.random.default_rng(1)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    entries = 4
    perm = np.array([2, 0, 3, 1])

    def value(m):  # m / (2 entries) on the torus: below 1/2, so it fits an int32
        return (int(m) << 32) // (2 * entries)

    tables = np.stack([tools.lut_test_poly(p, [value(m) for m in t]) for t in (perm, np.arange(entries))])
    s = np.asarray(k["lwe_key"][: p.n], dtype=np.int64)

    def decode(rows):
        ph = ((rows[:, p.n].astype(np.int64) - rows[:, : p.n].astype(np.int64) @ s) & 0xFFFFFFFF) / 2.0 ** 32
        return np.rint(ph * 2 * entries).astype(np.int64) % (2 * entries)

    with ia.Context.from_arrays(p, k["bk"], k["ksk"], device=a.device) as ctx:
        say("flat programmable bootstraps against flat gate calls: n = %d, N = %d, %d CUs, %s" % (p.n, p.N, ctx.get_option("cus"), ctx.kernel_variant))
        say("bootstraps/s from ieache_stats.total_ms of warm host calls (%d unrecorded, then %d recorded, the three calls by turns): "
            "median [min .. max]" % (a.warm, a.calls))
        say()
        for count in sizes:
            bits = rng.integers(0, 2, size=(2, count)).astype(np.uint8)
            ga, gb = tools.encrypt_bits(p, k["lwe_key"], bits[0], 461), tools.encrypt_bits(p, k["lwe_key"], bits[1], 462)
            # table inputs: fresh encryptions of 1/8 moved to the message phases m / 8
            msgs = rng.integers(0, entries, size=count)
            x = tools.encrypt_bits(p, k["lwe_key"], np.ones(count, dtype=np.uint8), 463)
            b = x[:, p.n].astype(np.int64) - (1 << 29) + np.array([value(m) for m in msgs], dtype=np.int64)
            x[:, p.n] = (b & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
            of = rng.integers(0, 2, size=count).astype(np.int32)
            calls = (("gates AND", lambda st: ctx.gates(ia.GATE_AND, ga, gb, st)),
                     ("pbs", lambda st: ctx.pbs(x, tables, of, stats=st)),
                     ("pbs, no key switch", lambda st: ctx.pbs(x, tables, of, keyswitch=False, stats=st)))
            out = ctx.pbs(x, tables, of)
            want = np.where(of == 0, perm[msgs], msgs)
            wrong = int(np.sum(decode(out) != want))
            assert np.array_equal(tools.decrypt_bits(p, k["lwe_key"], ctx.gates(ia.GATE_AND, ga, gb)), bits[0] & bits[1])
            ms = {label: [] for label, _ in calls}
            launches = {}
            for i in range(a.warm + a.calls):
                for label, f in calls:
                    st = ia.Stats()
                    f(st)
                    assert st.bootstraps == count
                    launches[label] = (st.blind_rotate_launches, st.keyswitch_launches)
                    if i >= a.warm:
                        ms[label].append(st.total_ms)
            say("%d rows (kernel of a launch of this size: %s); %d of %d table outputs decode wrong" % (count, ctx.kernel_for_launch(count), wrong, count))
            base = float(np.median(ms["gates AND"]))
            for label, _ in calls:
                m, lo, hi = float(np.median(ms[label])), min(ms[label]), max(ms[label])
                say("  %-20s %9.3f ms [%.3f .. %.3f]   %9.0f bootstraps/s [%.0f .. %.0f]   %.3f of the gate call's time   (%d blind-rotation, %d key-switch launches)"
                    % (label, m, lo, hi, count / (m * 1e-3), count / (hi * 1e-3), count / (lo * 1e-3), m / base, launches[label][0], launches[label][1]))
            say()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
