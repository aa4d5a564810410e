#!/usr/bin/env python3
"""What the TLWE projection (Context.tlwe_project_device) and the replace write of a window (Context.lut_write_coef_device,
include/ieache.h section 3l) cost beside the calls they stand next to, on one card in one run at the product parameters
(n = 630, N = 1024, l = 3, Bgbit = 7; packing and projection keys at (8, 2)):

  tlwe_project_device of 32 / 1 024 / 4 096 rows in all, as items of width 1 and of width 32, beside pack_device of as many
  LWE rows (groups of 32): the same product kernel on K = N t = 8 192 against K = n t = 5 040, with the window digits written
  from the samples instead of from stored rows;
  lut_write_coef_device, in place, at 1 024 items x depth 4 x steps 5 x width 32 and at 64 items x depth 10 x steps 10 x
  width 1, beside lut_write_device (the replace write of whole slots, by the depth selectors) and lut_add_device (one memory
  per item) of the same items.

No rate is promised; the record is the deliverable.  Every figure is ieache_stats.total_ms, the GPU timeline (HIP events) of the
whole call, of warm device-form calls on buffers made once: the forms of a case by turns, the order rotated from round to
round, median [min .. max] of --calls recorded rounds after --warm unrecorded ones.

    python scripts/project_rates.py [--out profiles/project_rates.txt] [--calls 7]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROJECT_ROWS = (32, 1024, 4096)
WRITES = ((1024, 4, 5, 32), (64, 10, 10, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "project_rates.txt"))
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
        say("the TLWE projection and the replace write of a window beside their neighbours: n = %d, N = %d, l = %d, Bgbit = %d, keys at (8, 2), %d CUs"
            % (p.n, N, p.l, p.Bgbit, ctx.get_option("cus")))
        say("ieache_stats.total_ms (HIP events around the whole call) of warm device-form calls, the forms of a case by turns in rotating order "
            "(%d unrecorded rounds, then %d recorded): median [min .. max]" % (a.warm, a.calls))
        say()
        proj_key, pack_key = words((N, 8, 2, N)), words((p.n, 8, 2, N))  # any words are a key to the arithmetic
        ctx.set_projection_key(proj_key)
        ctx.set_packing_key(pack_key)

        # ---- the words first: small calls against the CPU references ----
        S, v, mem = words((5, 2 * p.l, 2, N)), words((3, 2, N)), words((3, 4, 2, N))
        same = bool(np.array_equal(ctx.tlwe_project(v, 5, 3, 2047), tools.tlwe_project_reference(p, proj_key, v, 5, 3, 2047)))
        say("3 samples projected onto (first 5, width 3, dest 2047), full-range words: equal to the CPU reference: %s" % same)
        with ctx.tgsw_prepare(S) as tg:
            same = bool(np.array_equal(ctx.lut_write_coef(tg, mem, 2, 3, v, width=4, unit=8),
                                       tools.lut_write_coef_reference(p, S, proj_key, mem, 2, 3, v, width=4, unit=8)))
        say("3 items x depth 2 x steps 3 x width 4, full-range words: equal to the CPU reference: %s" % same)
        say()

        # ---- the projection beside pack_device of as many rows ----
        for rows in PROJECT_ROWS:
            d_rows = torch.zeros((rows, ctx.lwe_stride), dtype=torch.int32, device=dev)
            d_rows[:, :p.n + 1] = torch.from_numpy(words((rows, p.n + 1))).to(dev)
            d_in = torch.from_numpy(words((rows, 2, N))).to(dev)
            d_out = torch.zeros((rows, 2, N), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()

            def project(width):
                def f():
                    st = ia.Stats()
                    ctx.tlwe_project_device(rows // width, 5, width, 7, d_in.data_ptr(), d_out.data_ptr(), stats=st)
                    assert st.levels == 1 and st.bootstraps == 0
                    return st.total_ms
                return f

            def pack():
                st = ia.Stats()
                ctx.pack_device(rows // 32, 32, 1, 7, d_rows.data_ptr(), d_out.data_ptr(), stats=st)
                return st.total_ms

            t = by_turns({"tlwe_project_device, width 1": project(1), "tlwe_project_device, width 32": project(32), "pack_device, groups of 32": pack})
            say("%d rows in all (projection: K = %d, split %d / %d; packing: K = %d, split %d)"
                % (rows, N * 8, ctx.project_plan(rows, 1)["k_split"], ctx.project_plan(rows // 32, 32)["k_split"], p.n * 8, ctx.pack_plan(rows // 32, 32)["k_split"]))
            for name, (m, lo, hi) in t.items():
                say("  %-34s %9.3f ms [%.3f .. %.3f]  %8.2f us per row" % (name, m, lo, hi, 1e3 * m / rows))
            say()

        # ---- the replace write of a window beside the replace write of a slot and lut_add ----
        for items, depth, steps, width in WRITES:
            bits = depth + steps
            d_set = torch.from_numpy(words((bits, 2 * p.l, 2, N))).to(dev)
            d_new = torch.from_numpy(words((items, 2, N))).to(dev)
            d_mem = torch.from_numpy(words((items << depth, 2, N))).to(dev)
            sel = np.tile(np.arange(bits, dtype=np.int32), (items, 1))
            d_sel = torch.from_numpy(sel).to(dev)
            d_high = torch.from_numpy(np.ascontiguousarray(sel[:, steps:])).to(dev)
            d_own = torch.arange(items, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            with ctx.tgsw_prepare_device(d_set.data_ptr(), bits) as tg:
                def write_coef():
                    st = ia.Stats()
                    ctx.lut_write_coef_device(tg, items, depth, steps, width, width, d_sel.data_ptr(), d_new.data_ptr(), d_mem.data_ptr(), d_mem.data_ptr(), stats=st)
                    assert st.levels == 2 * bits + 1 and st.bootstraps == 0
                    return st.total_ms, st.keyswitch_ms

                def write_slot():
                    st = ia.Stats()
                    ctx.lut_write_device(tg, items, depth, d_high.data_ptr(), d_new.data_ptr(), d_mem.data_ptr(), d_mem.data_ptr(), stats=st)
                    return st.total_ms

                def add():
                    st = ia.Stats()
                    ctx.lut_add_device(tg, items, depth, steps, d_sel.data_ptr(), None, d_new.data_ptr(), d_mem.data_ptr(), items, d_own.data_ptr(), d_mem.data_ptr(), stats=st)
                    return st.total_ms

                ks = []

                def write_coef_total():
                    total, part = write_coef()
                    ks.append(part)
                    return total

                t = by_turns({"lut_write_coef_device, in place": write_coef_total, "lut_write_device, in place": write_slot, "lut_add_device, in place": add})
            say("%d items x depth %d x steps %d x width %d, one memory of %d row%s per item (%d piece%s)"
                % (items, depth, steps, width, 1 << depth, "" if depth == 0 else "s", ctx.cmux_plan(items, depth)["pieces"], "" if ctx.cmux_plan(items, depth)["pieces"] == 1 else "s"))
            for name, (m, lo, hi) in t.items():
                say("  %-34s %9.3f ms [%.3f .. %.3f]" % (name, m, lo, hi))
            wc = t["lut_write_coef_device, in place"][0]
            say("  of lut_write_coef_device the projection's launches take %.3f ms (median); the call takes %.2f x lut_write_device's time and %.2f x lut_add_device's"
                % (float(np.median(ks[a.warm:])), wc / t["lut_write_device, in place"][0], wc / t["lut_add_device, in place"][0]))
            say()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
