#!/usr/bin/env python3
"""One batch through a plain context, through device groups on one card, and through every distinct device of the node:

  * add16 x 4 096 and mul32 x 64 (the reference's parameters) through Context, Group {0}, Group {0,0} and -- when the node
    has several devices -- Group {0,1,...}, by turns;
  * WALL time of the whole host call (time.perf_counter around it: staging, threads, evaluation, download), since a group's
    members report their own GPU timelines and no one of them is the call's;
  * the outputs of every group compared word for word with the context's before anything is timed.

    python scripts/group_rates.py [--out profiles/group_rates.txt] [--calls 5]

Median and range over --calls recorded calls after --warm unrecorded ones.  On ONE card the figures are expected to be close:
the chip is already full with one context.  The file is the record; nothing else states a group's speed."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_rates.txt"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--add16", type=int, default=4096)
    ap.add_argument("--mul32", type=int, default=64)
    a = ap.parse_args()
    assert a.calls >= 5, "the median of at least 5 calls"

    import ieache_amd as ia
    from ieache_amd import tools
    p = ia.default_params()
    k = tools.keygen_raw(p, (1, 2, 3))
    rng = np.random.default_rng(1)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def inputs(kind, bits, batch, seed):
        info = ia.circuit_info(kind, bits)
        inb = np.zeros((batch, info.n_inputs), dtype=np.uint8)
        inb[:, :2 * bits] = rng.integers(0, 2, size=(batch, 2 * bits))
        return tools.encrypt_bits(p, k["lwe_key"], inb, seed), info

    n_dev = ia.device_count()
    device_lists = [(0,), (0, 0)] + ([tuple(range(n_dev))] if n_dev > 1 else [])
    ctx = ia.Context.from_arrays(p, k["bk"], k["ksk"], device=0)
    groups = [ia.Group.from_arrays(p, k["bk"], k["ksk"], d) for d in device_lists]
    try:
        say("device groups against a plain context: n = %d, N = %d, %d device(s), %d CUs on device 0, %s"
            % (p.n, p.N, n_dev, ctx.get_option("cus"), ctx.kernel_variant))
        say("wall time of the whole host call, warm (%d unrecorded, then %d recorded, the callers by turns): median [min .. max]" % (a.warm, a.calls))
        say("br_mix of the members: " + "; ".join("%s: %s" % (g.devices, [c.get_option("br_mix") for c in g.contexts]) for g in groups))
        say()
        for name, kind, bits, batch in (("add16", ia.CIRC_ADD, 16, a.add16), ("mul32", ia.CIRC_MUL, 32, a.mul32)):
            inp, info = inputs(kind, bits, batch, 471 + bits)
            callers = [("context", lambda: ctx.eval_batch(kind, bits, inp))]
            callers += [("group %s" % (g.devices,), lambda g=g: g.eval_batch(kind, bits, inp)) for g in groups]
            ctx.prepare(kind, bits, batch)
            want = ctx.eval_batch(kind, bits, inp)
            for g in groups:
                g.prepare(kind, bits, batch)
                assert np.array_equal(g.eval_batch(kind, bits, inp), want), g.devices
            s = {label: [] for label, _ in callers}
            for i in range(a.warm + a.calls):
                for label, f in callers:
                    t0 = time.perf_counter()
                    f()
                    dt = time.perf_counter() - t0
                    if i >= a.warm:
                        s[label].append(dt)
            total = batch * info.bootstraps
            say("%s x %d: %d bootstraps per call; every group's output equals the context's word for word" % (name, batch, total))
            base = float(np.median(s["context"]))
            for label, _ in callers:
                m, lo, hi = float(np.median(s[label])), min(s[label]), max(s[label])
                say("  %-28s %9.1f ms [%.1f .. %.1f]   %9.0f bootstraps/s [%.0f .. %.0f]   %.3f of the context's time"
                    % (label, m * 1e3, lo * 1e3, hi * 1e3, total / m, total / hi, total / lo, m / base))
            say()
    finally:
        for g in groups:
            g.close()
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
