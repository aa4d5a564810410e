#!/usr/bin/env python3
"""What a linear layer on encrypted rows (Context.lwe_linear_device, include/ieache.h section 3n) costs on one card in one run at
the product parameters (n = 630, N = 1024, l = 3, Bgbit = 7), with both kernels, beside the programmable bootstrap of the rows
it feeds:

  LWE rows   batch 1 024, 784 -> 32
  LWE rows   batch 4 096,   4 -> 1
  LWE rows   batch    64, 1 024 -> 1 024
  TLWE rows  batch    16,  64 -> 64
  LWE rows   batch 1 024,  64 -> n_out for n_out = 1, 2, 4, 8, 16, 32: where the MFMA product overtakes the simple kernel, which is
             what kLinearMfmaMinOut (csrc/linear_plan.h) is set from

No rate is promised; the record is the deliverable.  Every figure is ieache_stats.total_ms, the GPU timeline (HIP events) of the
whole call, of warm device-form calls on buffers made once: the kernels of a shape by turns, the order rotated from round to
round, median [min .. max] of --calls recorded rounds after --warm unrecorded ones.  Bytes moved are x once plus out once plus W,
what a perfect kernel would move; the streaming figure they are held against is the 6.29 TB/s a float4 copy reaches on this card
(8.0 TB/s on paper).  pbs_device runs on the batch x n_out rows the call produced, once warm and once recorded: it is seconds
long at the larger shapes.

    python scripts/linear_rates.py [--out profiles/linear_rates.txt] [--calls 5] [--no-pbs]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STREAM_TBS = 6.29
SHAPES = (("lwe", 1024, 32, 784), ("lwe", 4096, 1, 4), ("lwe", 64, 1024, 1024), ("tlwe", 16, 64, 64))
SWEEP = tuple(("lwe", 1024, n_out, 64) for n_out in (1, 2, 4, 8, 16, 32))
PBS_ROWS_MAX = 65536


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_rates.txt"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-pbs", action="store_true", help="leave the bootstrap's times out (they are most of the run)")
    a = ap.parse_args()

    import torch
    import ieache_amd as ia
    from ieache_amd import tools
    import linear_reference as LN
    p = ia.default_params()
    k = tools.keygen_raw(p, (1, 2, 3))
    rng = np.random.default_rng(1)
    lines = []
    dev = "cuda:%d" % a.device

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def by_turns(forms):
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
        say("linear layers on encrypted rows beside the bootstrap they feed: n = %d, N = %d, l = %d, Bgbit = %d, %d CUs" % (p.n, p.N, p.l, p.Bgbit, ctx.get_option("cus")))
        say("ieache_stats.total_ms (HIP events around the whole call) of warm device-form calls, the two kernels of a shape by turns in rotating order "
            "(%d unrecorded rounds, then %d recorded): median [min .. max]; GB/s = (x + out + W bytes) / median, against %.2f TB/s of a streaming copy"
            % (a.warm, a.calls, STREAM_TBS))
        say()
        # the words first: a small call of each kernel against the numpy restatement
        x, W, b = LN.full_range(rng, (3, 33, p.n + 1)), LN.weight_cases(rng, 33, 33)["full"], LN.full_range(rng, 33)
        for kern in (1, 2):
            ctx.set_option("linear_kernel", kern)
            say("3 x (33 -> 33) on full-range LWE rows, kernel %d: equal to the numpy restatement: %s" % (kern, bool(np.array_equal(ctx.lwe_linear(x, W, b), LN.linear(x, W, b, p.n)))))
        say()
        tv = torch.full((p.N,), 1 << 29, dtype=torch.int32, device=dev)
        crossover = []
        for rows, batch, n_out, n_in in SHAPES + SWEEP:
            stride = LN.stride_of(p.n, p.N, rows)
            d_x = torch.from_numpy(LN.full_range(rng, (batch * n_in, stride))).to(dev)
            d_w = torch.from_numpy(rng.integers(-128, 128, size=(n_out, n_in)).astype(np.int8)).to(dev)
            d_b = None if rows == "tlwe" else torch.from_numpy(LN.full_range(rng, n_out)).to(dev)
            d_out = torch.zeros((batch * n_out, stride), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            moved = 4.0 * stride * batch * (n_in + n_out) + n_out * n_in

            def run(kern):
                def f():
                    ctx.set_option("linear_kernel", kern)
                    st = ia.Stats()
                    ctx.lwe_linear_device(rows, batch, n_out, n_in, d_w.data_ptr(), None if d_b is None else d_b.data_ptr(), d_x.data_ptr(), d_out.data_ptr(), stats=st)
                    assert st.bootstraps == 0 and st.levels == 1 and st.chunks == 1
                    return st.total_ms
                return f

            t = by_turns({"k_linear_simple": run(1), "k_linear_mfma": run(2)})
            ctx.set_option("linear_kernel", 0)
            plan = ctx.linear_plan(rows, batch, n_out, n_in)
            say("%s rows, batch %d, %d -> %d (%.1f MB in, %.1f MB out; the plan takes kernel %d, %d tile(s) per wave, %d K steps)"
                % (rows.upper(), batch, n_in, n_out, 4e-6 * stride * batch * n_in, 4e-6 * stride * batch * n_out, plan["kernel"], plan["wave_tiles"], plan["k_steps"]))
            for name, (m, lo, hi) in t.items():
                say("  %-16s %9.3f ms [%.3f .. %.3f]  %8.1f GB/s = %5.1f %% of the streaming figure" % (name, m, lo, hi, moved / m / 1e6, moved / m / 1e6 / (10 * STREAM_TBS)))
            if (rows, batch, n_out, n_in) in SWEEP:
                crossover.append((n_out, t["k_linear_simple"][0], t["k_linear_mfma"][0]))
            if not a.no_pbs and rows == "lwe" and batch * n_out <= PBS_ROWS_MAX:
                count = batch * n_out
                d_boot = torch.zeros((count, stride), dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                ms = []
                for _ in range(2):
                    st = ia.Stats()
                    ctx.pbs_device(count, d_out.data_ptr(), tv.data_ptr(), 1, None, d_boot.data_ptr(), stats=st)
                    ms.append(st.total_ms)
                best = min(v[0] for v in t.values())
                say("  pbs_device of the %d rows it feeds: %.1f ms (second call); the faster linear kernel is %.2f %% of that" % (count, ms[1], 100 * best / ms[1]))
            say()
        say("the crossover at batch 1 024, n_in = 64 (simple / MFMA, ms): " + ", ".join("n_out %d: %.3f / %.3f" % c for c in crossover))
        first = next((c[0] for c in crossover if c[2] < c[1]), None)
        ctx.set_option("linear_kernel", 0)
        taken = next(n_out for n_out in range(1, 65537) if ctx.linear_plan("lwe", 1024, n_out, 64)["kernel"] == 2)
        say("the MFMA product is the faster from n_out = %s on; csrc/linear_plan.h takes it from n_out = %d (kLinearMfmaMinOut)"
            % (first if first is not None else "(never in this sweep)", taken))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
