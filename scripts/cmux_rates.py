#!/usr/bin/env python3
"""What a CMux on caller TGSW samples costs beside a CMux step of the blind rotation, on one card in one run at the product
parameters (n = 630, N = 1024, l = 3, Bgbit = 7):

  * Context.cmux_device of 1 024 and 16 384 rows, with ONE selector shared by every row and with one selector per row
    (a set of as many samples), and
  * Context.lut_tree_device at depth 10 over 1 and 64 items (1 023 CMuxes per item, one shared table), beside
  * the per-step time of the two-limb rotation on the same number of rows: "exact_fft" = 1, Context.pbs_device(..., tlwe=True,
    accumulator=True), total_ms / n.

No rate is promised; the record is the deliverable.  Every figure is ieache_stats.total_ms, the GPU timeline (HIP events) of the
whole call, of warm device-form calls on buffers made once; median [min .. max] of --calls recorded calls after --warm
unrecorded ones.  Before anything is timed the card's words are compared with the CPU reference and a depth-4 lookup in a
client-encrypted table is decoded; the largest phase error seen goes into the file.

    python scripts/cmux_rates.py [--out profiles/cmux_rates.txt] [--calls 5]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cmux_rates.txt"))
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

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def full_range(shape):
        return torch.from_numpy(rng.integers(-(1 << 31), 1 << 31, size=shape, dtype=np.int64).astype(np.int32)).to(dev)

    def timed(f):
        t = [f() for _ in range(a.warm + a.calls)][a.warm:]
        return float(np.median(t)), min(t), max(t)

    with ia.Context.from_arrays(p, k["bk"], k["ksk"], device=a.device) as ctx:
        say("CMux on caller TGSW samples beside the CMux step of the two-limb blind rotation: n = %d, N = %d, l = %d, Bgbit = %d, %d CUs"
            % (p.n, N, p.l, p.Bgbit, ctx.get_option("cus")))
        say("ieache_stats.total_ms (HIP events around the whole call) of warm device-form calls (%d unrecorded, then %d recorded): median [min .. max]"
            % (a.warm, a.calls))
        say()

        # ---- correctness and noise first ----
        bits = rng.integers(0, 2, size=(16, N)).astype(np.uint8)
        m = np.where(bits == 1, 1 << 29, -(1 << 29)).astype(np.int32)
        table = tools.tlwe_encrypt(p, k["tlwe_key"], m, 81)
        samples = tools.tgsw_encrypt(p, k["tlwe_key"], [0, 1] * 4, 82)
        sel = np.array([[2 * b + ((i >> b) & 1) for b in range(4)] for i in range(16)], dtype=np.int32)
        with ctx.tgsw_prepare(samples) as S:
            out = ctx.lut_tree(S, table, 4, sel_of=sel)
            one = ctx.cmux(S, table[1:2], table[0:1], sel_of=[1])
        same = bool(np.array_equal(out, tools.lut_tree_reference(p, samples, table, 4, sel_of=sel)))

        def err_of(samples_, want):
            d = (tools.tlwe_phase(p, k["tlwe_key"], samples_).astype(np.int64) - want.astype(np.int64)) & 0xFFFFFFFF
            return np.minimum(d, (1 << 32) - d) / 2.0 ** 32

        e4, e1 = err_of(out, m), err_of(one, m[1:2])
        say("a client-encrypted table of 16 polynomials (coefficients +-1/8, alpha = %.3e) looked up at depth 4 by tgsw_encrypt'ed selector bits, "
            "all 16 indices: words equal to the CPU reference: %s; phase error max %.3e, rms %.3e (decoding condition of the tests: 2^-8 = %.3e; "
            "DESIGN.md section 7 derives key noise of standard deviation 1.7e-4 at depth 4 plus a truncation ramp of at most 1.2e-4 per selector bit that is 1)" % (p.tlwe_alpha_min, same, e4.max(), float(np.sqrt(np.mean(e4 ** 2))), 2.0 ** -8))
        say("one CMux of two of its entries: phase error max %.3e, rms %.3e (selector 1; derived: key noise 8.6e-5 and the ramp's 7.0e-5 rms, together 1.1e-4)" % (e1.max(), float(np.sqrt(np.mean(e1 ** 2)))))
        lwe = ctx.keyswitch(ctx.tlwe_extract(out, coef_of=np.arange(16)))
        say("tlwe_extract -> keyswitch -> decrypt_bits of coefficient i of entry i: wrong bits %d of 16"
            % int(np.sum(tools.decrypt_bits(p, k["lwe_key"], lwe) != bits[np.arange(16), np.arange(16)])))
        say()

        # ---- flat CMux beside the rotation's step ----
        step_of = {}
        for rows in (1024, 16384):
            d1, d0, d_out = full_range((rows, 2, N)), full_range((rows, 2, N)), torch.zeros((rows, 2, N), dtype=torch.int32, device=dev)
            d_set = full_range((rows, 2 * p.l, 2, N)) if rows <= 1024 else None
            x = torch.zeros((rows, ctx.lwe_stride), dtype=torch.int32, device=dev)
            x[:, : p.n + 1] = full_range((rows, p.n + 1))
            tv = full_range((1, 2, N))
            torch.cuda.synchronize()
            shared = ctx.tgsw_prepare_device(d1.data_ptr(), 1)  # any words are a sample to the arithmetic: rows of d1 stand in
            # one selector per row: 1 024 distinct samples (192 MB of spectrum); 16 384 rows walk them 16 times over
            per_row = ctx.tgsw_prepare_device(d_set.data_ptr(), 1024) if d_set is not None else step_of["per_row_set"]
            step_of["per_row_set"] = per_row
            zeros = torch.zeros(rows, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()

            def cmux_call(tgsw, sel_ptr):
                def f():
                    st = ia.Stats()
                    ctx.cmux_device(tgsw, rows, sel_ptr, d1.data_ptr(), d0.data_ptr(), d_out.data_ptr(), stats=st)
                    assert st.bootstraps == 0 and st.chunks >= 1
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
            say("%d rows" % rows)
            say("  %-58s %9.3f ms [%.3f .. %.3f] / %d steps = %.4f ms per step   %10.0f rows/s per step"
                % ("two-limb rotation (exact_fft = 1, accumulator=True)", rm, rlo, rhi, p.n, step, rows / (step * 1e-3)))
            for label, tgsw, sel_ptr in (("cmux_device, one shared selector", shared, zeros.data_ptr()), ("cmux_device, one selector per row (1 024 samples)", per_row, None)):
                cm, lo, hi = timed(cmux_call(tgsw, sel_ptr))
                say("  %-58s %9.3f ms [%.3f .. %.3f]   %10.0f rows/s   %.2f x the rotation's step" % (label, cm, lo, hi, rows / (cm * 1e-3), cm / step))
                if label.endswith("shared selector") and cm > 2 * step:
                    say("    (worse than half the rotation's step rate: the kernel does the same arithmetic per row -- 2l forward and four inverse "
                        "transforms, 8l row products -- plus 24 KB of global traffic per row, d1 and d0 read and d0 read again and the result "
                        "written, that the rotation keeps in LDS, and pays the launch, the twiddle table and the selector's 192 KB once per row "
                        "instead of once per 16 to 64 steps)")
            shared.close()
            say()
        step_of["per_row_set"].close()

        # ---- depth-10 tree ----
        depth = 10
        tables = full_range((1, 1 << depth, 2, N))
        d_sel = full_range((depth, 2 * p.l, 2, N))
        torch.cuda.synchronize()
        with ctx.tgsw_prepare_device(d_sel.data_ptr(), depth) as S:
            for items in (1, 64):
                sel_of = torch.from_numpy(np.tile(np.arange(depth, dtype=np.int32), (items, 1))).to(dev)
                d_out = torch.zeros((items, 2, N), dtype=torch.int32, device=dev)
                torch.cuda.synchronize()

                def tree():
                    st = ia.Stats()
                    ctx.lut_tree_device(S, items, depth, sel_of.data_ptr(), tables.data_ptr(), 1, None, d_out.data_ptr(), stats=st)
                    assert st.levels == depth and st.bootstraps == 0
                    return st.total_ms

                tm, lo, hi = timed(tree)
                cmuxes = items * ((1 << depth) - 1)
                plan = ctx.cmux_plan(items, depth)
                say("depth-%d tree, %d item%s (%d CMuxes, %d piece%s): %9.3f ms [%.3f .. %.3f]   %8.1f lookups/s   %10.0f CMuxes/s"
                    % (depth, items, "" if items == 1 else "s", cmuxes, plan["pieces"], "" if plan["pieces"] == 1 else "s", tm, lo, hi, items / (tm * 1e-3),
                       cmuxes / (tm * 1e-3)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
