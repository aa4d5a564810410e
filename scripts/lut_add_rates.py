#!/usr/bin/env python3
"""What many values into ONE shared memory in one call (Context.lut_add_device, include/ieache.h section 3j) cost beside what
the call replaces, on one card in one run at the product parameters (n = 630, N = 1024, l = 3, Bgbit = 7):
(count, depth, steps) = (64, 10, 0), (1 024, 4, 0), (1 024, 4, 10), (4 096, 0, 10).  What it replaces is
Context.lut_scatter_device of the same items with no memory -- count x 2^depth rows of leaves the caller then has to sum, a
sum that is NOT timed here -- and, where steps > 0, Context.tlwe_rotate_device before it.

The last demux step of lut_add adds its rows with integer atomics instead of storing them.  Where steps == 0 its time is
taken as lut_add(depth) minus lut_scatter(depth - 1) of the same items (the steps before the last are exactly that scatter),
the storing step's as lut_scatter(depth) minus lut_scatter(depth - 1), and the added bytes per second follow:
count x 2^depth x 8 KB over that time.

No rate is promised; the record is the deliverable.  Every figure is ieache_stats.total_ms, the GPU timeline (HIP events) of the
whole call, of warm device-form calls on buffers made once: the forms of a case by turns, the order rotated from round to
round, median [min .. max] of --calls recorded rounds after --warm unrecorded ones.

    python scripts/lut_add_rates.py [--out profiles/lut_add_rates.txt] [--calls 7]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((64, 10, 0), (1024, 4, 0), (1024, 4, 10), (4096, 0, 10))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lut_add_rates.txt"))
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    import torch
    import ieache_amd as ia
    from ieache_amd import tools
    p = ia.default_params()
    k = tools.keygen_raw(p, (1, 2, 3))
    rng = np.random.default_rng(1)
    lines = []
    dev = "cuda:%d" % a.device
    N = p.N

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def words(shape):
        return rng.integers(-(1 << 31), 1 << 31, size=shape, dtype=np.int64).astype(np.int32)

    def by_turns(forms):
        """{name: f -> ms} -> {name: (median, min, max)}: every round runs each form once, starting one form further on"""
        names = list(forms)
        times = {n: [] for n in names}
        for r in range(a.warm + a.calls):
            for q in range(len(names)):
                n = names[(r + q) % len(names)]
                t = forms[n]()
                if r >= a.warm:
                    times[n].append(t)
        return {n: (float(np.median(t)), min(t), max(t)) for n, t in times.items()}

    with ia.Context.from_arrays(p, k["bk"], k["ksk"], device=a.device) as ctx:
        say("many values into ONE shared memory (lut_add_device) beside what it replaces (tlwe_rotate_device where steps > 0, then lut_scatter_device "
            "with no memory; the caller's sum of the leaves is not timed): n = %d, N = %d, l = %d, Bgbit = %d, %d CUs" % (p.n, N, p.l, p.Bgbit, ctx.get_option("cus")))
        say("ieache_stats.total_ms (HIP events around the whole call) of warm device-form calls, the forms of a case by turns in rotating order "
            "(%d unrecorded rounds, then %d recorded): median [min .. max]" % (a.warm, a.calls))
        say()

        # ---- the words first: a small call against the CPU reference ----
        S, v, mems = words((5, 2 * p.l, 2, N)), words((5, 2, N)), words((2, 4, 2, N))
        mof = np.array([1, 0, 1, 1, 0], dtype=np.int32)
        with ctx.tgsw_prepare(S) as tg:
            same = bool(np.array_equal(ctx.lut_add(tg, v, 2, 3, mems=mems, mem_of=mof), tools.lut_add_reference(p, S, v, 2, 3, mems=mems, mem_of=mof)))
        say("5 items x depth 2 x steps 3 into two memories, full-range words: equal to the CPU reference: %s" % same)
        say()

        for items, depth, steps in CASES:
            bits = depth + steps
            d_set = torch.from_numpy(words((bits, 2 * p.l, 2, N))).to(dev)  # any words are a sample to the arithmetic
            d_val = torch.from_numpy(words((items, 2, N))).to(dev)
            d_mem = torch.from_numpy(words((1 << depth, 2, N))).to(dev)
            d_leaves = torch.zeros((items << depth, 2, N), dtype=torch.int32, device=dev)
            d_rows = torch.zeros((items, 2, N), dtype=torch.int32, device=dev)
            sel = np.tile(np.arange(bits, dtype=np.int32), (items, 1))
            d_sel = torch.from_numpy(sel).to(dev)
            d_low = torch.from_numpy(np.ascontiguousarray(sel[:, :steps])).to(dev) if steps else None
            d_high = torch.from_numpy(np.ascontiguousarray(sel[:, steps:])).to(dev) if depth else None
            d_am = torch.from_numpy(tools.rotate_amounts(steps, toward_zero=False, N=N)).to(dev) if steps else None
            torch.cuda.synchronize()
            ptr = lambda t: t.data_ptr() if t is not None else None
            with ctx.tgsw_prepare_device(d_set.data_ptr(), bits) as tg:
                def add():
                    st = ia.Stats()
                    ctx.lut_add_device(tg, items, depth, steps, d_sel.data_ptr(), None, d_val.data_ptr(), d_mem.data_ptr(), 1, None, d_mem.data_ptr(), stats=st)
                    assert st.levels == bits and st.bootstraps == 0
                    return st.total_ms

                def scatter_at(d):
                    def f():
                        st = ia.Stats()
                        ctx.lut_scatter_device(tg, items, d, ptr(d_high), d_rows.data_ptr() if steps else d_val.data_ptr(), None, d_leaves.data_ptr(), stats=st)
                        assert st.levels == d and st.bootstraps == 0
                        return st.total_ms
                    return f

                def rotate():
                    st = ia.Stats()
                    ctx.tlwe_rotate_device(tg, items, steps, d_low.data_ptr(), d_am.data_ptr(), d_val.data_ptr(), d_rows.data_ptr(), stats=st)
                    return st.total_ms

                forms = {"lut_add_device, in place": add, "lut_scatter_device, no memory": scatter_at(depth)}
                if steps:
                    forms["tlwe_rotate_device"] = rotate
                elif depth:
                    forms["lut_scatter_device, depth - 1"] = scatter_at(depth - 1)
                t = by_turns(forms)
            products = items * ((1 << depth) - 1 + steps)
            plan = ctx.cmux_plan(items, depth)
            added = items * (8192 << depth)
            say("%d items x depth %d x steps %d into one memory of %d row%s (%d external products, %d piece%s, %.0f MB of leaves)"
                % (items, depth, steps, 1 << depth, "" if depth == 0 else "s", products, plan["pieces"], "" if plan["pieces"] == 1 else "s", added / 2.0 ** 20))
            for name, (m, lo, hi) in t.items():
                say("  %-34s %9.3f ms [%.3f .. %.3f]" % (name, m, lo, hi))
            am = t["lut_add_device, in place"][0]
            old = t["lut_scatter_device, no memory"][0] + (t["tlwe_rotate_device"][0] if steps else 0.0)
            say("  lut_add_device takes %.2f x the time of what it replaces (%.3f ms, before the caller's sum of %.0f MB)" % (am / old, old, added / 2.0 ** 20))
            if depth == 0:
                say("  all %d items add into ONE row: %.0f MB of atomic adds onto 8 KB, %.1f GB/s of added bytes for the whole call (rotation included)"
                    % (items, added / 2.0 ** 20, added / (am * 1e-3) / 1e9))
            elif not steps:
                before = t["lut_scatter_device, depth - 1"][0]
                last_add, last_store = am - before, t["lut_scatter_device, no memory"][0] - before
                say("  last step alone: adding %.3f ms, %.1f GB/s of added bytes; storing %.3f ms, %.1f GB/s of stored bytes"
                    % (last_add, added / (last_add * 1e-3) / 1e9, last_store, added / (last_store * 1e-3) / 1e9))
            else:
                say("  whole call: %.1f GB/s of added bytes (rotation and the steps before the last included)" % (added / (am * 1e-3) / 1e9))
            del d_leaves
            say()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
