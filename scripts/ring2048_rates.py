#!/usr/bin/env python3
"""What a blind rotation on the ring of degree 2048 costs, on one card in one run at n = 630, l = 3, Bgbit = 7:

  k_blind_rotate_h2 (csrc/blind_rotate_h2.hip: a CMux step as two products on the ring of degree 1024) beside
  k_blind_rotate_generic on the same N = 2048 context ("force_generic"), at 64, 1 024 and 4 096 rows;
  k_blind_rotate_x1 -- the two-limb kernel of N = 1024 with one wave per gate -- with the same n and gadget, same rows.

No rate is promised; the record is the deliverable.  On paper an N = 2048 step is about 3.3 x k_blind_rotate_x1's: four times the
forward transforms and row products, twice the inverse ones.  Every figure is ieache_stats.blind_rotate_ms, HIP events around the
blind-rotation launches of a warm pbs_device call without key switch, on buffers made once: the three kernels by turns, the
order rotated from round to round, median [min .. max] of --calls recorded rounds after --warm unrecorded ones.  Key words are
uniform random words: any words are a key to the arithmetic, and a rotation amount is zero (a skipped step) once in 2N.

    python scripts/ring2048_rates.py [--out profiles/ring2048_rates.txt] [--calls 7]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = (64, 1024, 4096)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ring2048_rates.txt"))
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--n", type=int, default=630)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    import torch
    import ieache_amd as ia
    rng = np.random.default_rng(2048)
    dev = "cuda:%d" % a.device
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def words(shape):
        return rng.integers(-(1 << 31), 1 << 31, size=shape, dtype=np.int64).astype(np.int32)

    def open_context(N):
        p = ia.default_params().copy(n=a.n, N=N)
        return p, ia.Context.from_arrays(p, words(p.bk_count), np.zeros(p.ksk_count, dtype=np.int32), device=a.device)

    p2, big = open_context(2048)
    p1, small = open_context(1024)
    with big, small:
        small.set_option("exact_fft", 1)
        small.set_option("br_variant", 9)  # k_blind_rotate_x1 at every launch size
        say("blind rotation on the ring of degree 2048 beside the any-parameter kernel and beside N = 1024: n = %d, l = %d, Bgbit = %d, %d CUs"
            % (p2.n, p2.l, p2.Bgbit, big.get_option("cus")))
        say("ieache_stats.blind_rotate_ms (HIP events around the blind-rotation launches) of warm pbs_device calls without key switch, the kernels by "
            "turns in rotating order (%d unrecorded rounds, then %d recorded): median [min .. max]" % (a.warm, a.calls))
        say("key forms: N = 2048 even / odd half spectra %.0f MB, N = 1024 two-limb spectrum %.0f MB"
            % (p2.n * 2 * p2.l * 2 * 4 * 512 * 16 / 1e6, p1.n * 2 * p1.l * 4 * 512 * 16 / 1e6))
        say()
        for rows in ROWS:
            bufs = {}
            for p, ctx in ((p2, big), (p1, small)):
                bufs[p.N] = (torch.from_numpy(words((rows, ctx.lwe_stride))).to(dev), torch.full((p.N,), 1 << 29, dtype=torch.int32, device=dev),
                             torch.zeros((rows, ctx.extract_stride), dtype=torch.int32, device=dev))
            torch.cuda.synchronize()

            def run(ctx, N, fg, name):
                d_x, d_v, d_u = bufs[N]
                ctx.set_option("force_generic", fg)
                assert ctx.kernel_for_launch(rows).startswith(name), ctx.kernel_for_launch(rows)
                st = ia.Stats()
                ctx.pbs_device(rows, d_x.data_ptr(), d_v.data_ptr(), 1, None, d_u.data_ptr(), keyswitch=False, stats=st)
                return st.blind_rotate_ms

            forms = {"k_blind_rotate_h2, N = 2048": lambda: run(big, 2048, 0, "k_blind_rotate_h2"),
                     "k_blind_rotate_generic, N = 2048": lambda: run(big, 2048, 1, "k_blind_rotate_generic"),
                     "k_blind_rotate_x1, N = 1024": lambda: run(small, 1024, 0, "k_blind_rotate_x1")}
            names = list(forms)
            times = {n: [] for n in names}
            for r in range(a.warm + a.calls):
                for q in range(len(names)):
                    n = names[(r + q) % len(names)]
                    t = forms[n]()
                    if r >= a.warm:
                        times[n].append(t)
            med = {n: float(np.median(t)) for n, t in times.items()}
            say("%d rows" % rows)
            for n in names:
                say("  %-36s %10.3f ms [%.3f .. %.3f]  %8.3f us per row and CMux step" % (n, med[n], min(times[n]), max(times[n]), 1e3 * med[n] / rows / a.n))
            say("  h2 takes %.2f x the time of x1 at N = 1024 (on paper 3.3 x); the any-parameter kernel takes %.2f x the time of h2"
                % (med[names[0]] / med[names[2]], med[names[1]] / med[names[0]]))
            say()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
