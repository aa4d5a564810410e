#!/usr/bin/env python3
"""What a rotation by caller selectors (Context.tlwe_rotate_device, include/ieache.h section 3h) costs per step beside the two-limb
blind rotation's step on the same number of rows, and what the coefficient-level lookup (Context.lut_read_device) costs beside
the CMux tree of its depth (Context.lut_tree_device), on one card in one run at the product parameters (n = 630, N = 1024, l = 3,
Bgbit = 7):

  * tlwe_rotate_device of 1, 1 024 and 16 384 rows at steps = 10, in place, with ten selectors shared by every row and with ten
    selectors of its own per row (implied indices into a set of 1 024 samples), beside
  * the per-step time of the two-limb rotation on the same rows: "exact_fft" = 1, Context.pbs_device(..., tlwe=True,
    accumulator=True), total_ms / n, and
  * lut_read_device at (depth 4, steps 10), with and without its key switch, beside lut_tree_device of depth 4 on the same
    1 024 items, one table per item.

No rate is promised; the record is the deliverable.  Every figure is ieache_stats.total_ms, the GPU timeline (HIP events) of the
whole call, of warm device-form calls on buffers made once; median [min .. max] of --calls recorded calls after --warm
unrecorded ones.  Before anything is timed a client-encrypted table of 4 samples is read at depth 2 + steps 10 at 16 addresses,
compared with the CPU reference and decoded; the largest phase error seen goes into the file.

    python scripts/rotate_rates.py [--out profiles/rotate_rates.txt] [--calls 5]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rotate_rates.txt"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
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
    steps = 10

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def full_range(shape):
        return torch.from_numpy(rng.integers(-(1 << 31), 1 << 31, size=shape, dtype=np.int64).astype(np.int32)).to(dev)

    def timed(f):
        t = [f() for _ in range(a.warm + a.calls)][a.warm:]
        return float(np.median(t)), min(t), max(t)

    with ia.Context.from_arrays(p, k["bk"], k["ksk"], device=a.device) as ctx:
        say("rotation by caller selectors (tlwe_rotate_device) beside the two-limb blind rotation's step, and the coefficient-level lookup "
            "(lut_read_device) beside the CMux tree: n = %d, N = %d, l = %d, Bgbit = %d, %d CUs" % (p.n, N, p.l, p.Bgbit, ctx.get_option("cus")))
        say("ieache_stats.total_ms (HIP events around the whole call) of warm device-form calls (%d unrecorded, then %d recorded): median [min .. max]"
            % (a.warm, a.calls))
        say()

        # ---- correctness and noise first ----
        msg = ((np.arange(4 * N, dtype=np.int64) * 0x9E3779B1 + 7) & 0xFFFFFFFF).astype(np.uint32).view(np.int32).reshape(4, N)
        table = tools.tlwe_encrypt(p, k["tlwe_key"], msg, 311)
        addrs = [0, 4095, 1686, 2561] + [int(v) for v in rng.integers(0, 4096, size=12)]
        samples = tools.tgsw_encrypt(p, k["tlwe_key"], [(ad >> t) & 1 for ad in addrs for t in range(12)], 312)
        sel = np.arange(12 * len(addrs), dtype=np.int32).reshape(len(addrs), 12)
        with ctx.tgsw_prepare(samples) as S:
            u = ctx.lut_read(S, table, 2, steps, sel_of=sel, keyswitch=False)
            lwe = ctx.lut_read(S, table, 2, steps, sel_of=sel)
        same = bool(np.array_equal(u, tools.lut_read_reference(p, samples, table, 2, steps, sel_of=sel)))
        want = np.array([msg[ad >> 10, ad & 1023] for ad in addrs])

        def err_of(rows, key):
            rows = rows.astype(np.int64)
            ph = (rows[:, -1] - rows[:, :-1] @ np.asarray(key, dtype=np.int64)) & 0xFFFFFFFF
            d = (ph - want.astype(np.int64)) & 0xFFFFFFFF
            return np.minimum(d, (1 << 32) - d) / 2.0 ** 32

        e, eks = err_of(u, k["tlwe_key"]), err_of(lwe, k["lwe_key"])
        say("a client-encrypted table of 4 samples (4 096 distinct messages, alpha = %.3e) read at depth 2 + steps 10 by tgsw_encrypt'ed address "
            "bits at 16 addresses (0, 4095, 14 others; 12 external products each): words equal to the CPU reference: %s; phase error of the extracted "
            "row max %.3e, rms %.3e (decoding condition of the tests: 2^-8 = %.3e; DESIGN.md section 7 derives key noise of standard deviation "
            "3.0e-4 for 12 products plus a truncation ramp of at most 1.2e-4 per address bit that is 1); after the key switch max %.3e (a gate "
            "input's condition: 1/8)" % (p.tlwe_alpha_min, same, e.max(), float(np.sqrt(np.mean(e ** 2))), 2.0 ** -8, eks.max()))
        say()

        # ---- the rotation beside the blind rotation's step ----
        d_set = full_range((1024, 2 * p.l, 2, N))  # any words are a sample to the arithmetic
        torch.cuda.synchronize()
        shared = ctx.tgsw_prepare_device(d_set.data_ptr(), steps)  # the first ten samples: selector t of every row is sample t
        per_row = ctx.tgsw_prepare_device(d_set.data_ptr(), 1024)  # implied indices: row r, step t takes sample (10 r + t) mod 1 024
        del d_set
        for rows in (1, 1024, 16384):
            d_rows, d_out = full_range((rows, 2, N)), torch.zeros((rows, 2, N), dtype=torch.int32, device=dev)
            x = torch.zeros((rows, ctx.lwe_stride), dtype=torch.int32, device=dev)
            x[:, : p.n + 1] = full_range((rows, p.n + 1))
            tv = full_range((1, 2, N))
            sel_shared = torch.from_numpy(np.tile(np.arange(steps, dtype=np.int32), (rows, 1))).to(dev)
            torch.cuda.synchronize()

            def rotate_call(tgsw, sel_ptr):
                def f():
                    st = ia.Stats()
                    ctx.tlwe_rotate_device(tgsw, rows, steps, sel_ptr, None, d_rows.data_ptr(), d_rows.data_ptr(), stats=st)
                    assert st.bootstraps == 0 and st.levels == steps and st.blind_rotate_launches == st.chunks
                    return st.total_ms
                return f

            def rotation():
                st = ia.Stats()
                ctx.pbs_device(rows, x.data_ptr(), tv.data_ptr(), 1, None, d_out.data_ptr(), tlwe=True, accumulator=True, stats=st)
                assert st.bootstraps == rows
                return st.total_ms

            ctx.set_option("exact_fft", 1)
            rm, rlo, rhi = timed(rotation)
            ctx.set_option("exact_fft", 0)
            step = rm / p.n
            say("%d row%s" % (rows, "" if rows == 1 else "s"))
            say("  %-62s %9.3f ms [%.3f .. %.3f] / %d steps = %.4f ms per step   %10.0f rows/s per step"
                % ("two-limb rotation (exact_fft = 1, accumulator=True)", rm, rlo, rhi, p.n, step, rows / (step * 1e-3)))
            for label, tgsw, sel_ptr in (("tlwe_rotate_device, %d steps, selectors shared by all rows" % steps, shared, sel_shared.data_ptr()),
                                         ("tlwe_rotate_device, %d steps, selectors per row (1 024 samples)" % steps, per_row, None)):
                tm, lo, hi = timed(rotate_call(tgsw, sel_ptr))
                say("  %-62s %9.3f ms [%.3f .. %.3f] / %d steps = %.4f ms per step   %10.0f rows/s per step   %.2f x the rotation's step"
                    % (label, tm, lo, hi, steps, tm / steps, rows / (tm / steps * 1e-3), tm / steps / step))
            del d_rows, d_out, x
            say()
        shared.close()
        per_row.close()

        # ---- the lookup beside the tree ----
        items, depth = 1024, 4
        d_sel = full_range((depth + steps, 2 * p.l, 2, N))
        d_tables = full_range((items, 1 << depth, 2, N))
        sel_read = torch.from_numpy(np.tile(np.arange(depth + steps, dtype=np.int32), (items, 1))).to(dev)
        sel_tree = torch.from_numpy(np.tile(np.arange(steps, steps + depth, dtype=np.int32), (items, 1))).to(dev)
        table_of = torch.arange(items, dtype=torch.int32, device=dev)
        d_row = torch.zeros((items, 2, N), dtype=torch.int32, device=dev)
        d_u = torch.zeros((items, N + 4), dtype=torch.int32, device=dev)
        d_lwe = torch.zeros((items, ctx.lwe_stride), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        with ctx.tgsw_prepare_device(d_sel.data_ptr(), depth + steps) as S:
            def tree():
                st = ia.Stats()
                ctx.lut_tree_device(S, items, depth, sel_tree.data_ptr(), d_tables.data_ptr(), items, table_of.data_ptr(), d_row.data_ptr(), stats=st)
                assert st.levels == depth and st.bootstraps == 0
                return st.total_ms

            def read(ks):
                def f():
                    st = ia.Stats()
                    ctx.lut_read_device(S, items, depth, steps, sel_read.data_ptr(), None, d_tables.data_ptr(), items, table_of.data_ptr(),
                                        (d_lwe if ks else d_u).data_ptr(), keyswitch=ks, stats=st)
                    assert st.levels == depth + steps and st.bootstraps == 0 and (st.keyswitch_launches > 0) == ks
                    return st.total_ms
                return f

            tm, tlo, thi = timed(tree)
            um, ulo, uhi = timed(read(False))
            km, klo, khi = timed(read(True))
        plan = ctx.cmux_plan(items, depth)
        say("%d items x (depth %d, steps %d): %d-bit tables of %d samples, one per item (%.0f MB), %d piece%s"
            % (items, depth, steps, N << depth, 1 << depth, items * (8192 << depth) / 2.0 ** 20, plan["pieces"], "" if plan["pieces"] == 1 else "s"))
        say("  %-62s %9.3f ms [%.3f .. %.3f]   %10.0f lookups/s" % ("lut_tree_device, depth %d (a sample per item)" % depth, tm, tlo, thi, items / (tm * 1e-3)))
        say("  %-62s %9.3f ms [%.3f .. %.3f]   %10.0f lookups/s   %.2f x the tree" % ("lut_read_device without the key switch (an extracted row per item)", um, ulo, uhi, items / (um * 1e-3), um / tm))
        say("  %-62s %9.3f ms [%.3f .. %.3f]   %10.0f lookups/s   %.2f x the tree" % ("lut_read_device (an LWE row per item)", km, klo, khi, items / (km * 1e-3), km / tm))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
