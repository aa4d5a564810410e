#!/usr/bin/env python3
"""What a write at an encrypted index (Context.lut_scatter_device, include/ieache.h section 3g) costs beside the lookup
(Context.lut_tree_device) of the same items and depth, on one card in one run at the product parameters (n = 630, N = 1024,
l = 3, Bgbit = 7): items x depth = 1 x 10, 64 x 10 and a flat batch of 1 024 x 4.  Both run the same number of external
products (2^depth - 1 per item); the scatter writes twice the rows and, in its last step, reads the memory it adds to.  Every
item has a memory block of its own, written in place (d_out == d_mem), and the lookup beside it reads one table per item.

No rate is promised; the record is the deliverable.  Every figure is ieache_stats.total_ms, the GPU timeline (HIP events) of the
whole call, of warm device-form calls on buffers made once; median [min .. max] of --calls recorded calls after --warm
unrecorded ones.  Before anything is timed, three replace writes (Context.lut_write, addresses 3, 12, 3, fresh selectors each
time) into a client-encrypted 16-slot memory are compared with the CPU reference and decoded; the largest phase error seen
goes into the file.

    python scripts/scatter_rates.py [--out profiles/scatter_rates.txt] [--calls 5]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scatter_rates.txt"))
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

    def sign_poly(shape):
        return np.where(rng.integers(0, 2, size=shape) == 1, 1 << 29, -(1 << 29)).astype(np.int32)

    def wrap_sub(x, y):
        return ((x.astype(np.int64) - y.astype(np.int64)) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)

    with ia.Context.from_arrays(p, k["bk"], k["ksk"], device=a.device) as ctx:
        say("write at an encrypted index (lut_scatter_device) beside the lookup (lut_tree_device): n = %d, N = %d, l = %d, Bgbit = %d, %d CUs"
            % (p.n, N, p.l, p.Bgbit, ctx.get_option("cus")))
        say("ieache_stats.total_ms (HIP events around the whole call) of warm device-form calls (%d unrecorded, then %d recorded): median [min .. max]"
            % (a.warm, a.calls))
        say()

        # ---- correctness and noise first ----
        msg = sign_poly((16, N))
        mem = tools.tlwe_encrypt(p, k["tlwe_key"], msg, 171)[None]
        ref = mem
        sel = np.arange(4, dtype=np.int32)[None]
        same, errs = True, []
        for w, addr in enumerate((3, 12, 3)):
            samples = tools.tgsw_encrypt(p, k["tlwe_key"], [(addr >> b) & 1 for b in range(4)], 181 + w)
            m = sign_poly(N)
            new = tools.tlwe_encrypt(p, k["tlwe_key"], m, 191 + w)
            with ctx.tgsw_prepare(samples) as S:
                mem = ctx.lut_write(S, mem, 4, new, sel_of=sel)
            old = tools.lut_tree_reference(p, samples, ref, 4, sel_of=sel, table_of=[0])
            ref = tools.lut_scatter_reference(p, samples, wrap_sub(new, old), 4, sel_of=sel, mem=ref)
            same = same and bool(np.array_equal(mem, ref))
            msg[addr] = m
            d = (tools.tlwe_phase(p, k["tlwe_key"], mem[0]).astype(np.int64) - msg.astype(np.int64)) & 0xFFFFFFFF
            errs.append(np.minimum(d, (1 << 32) - d) / 2.0 ** 32)
        say("a client-encrypted memory of 16 polynomials (coefficients +-1/8, alpha = %.3e), three replace writes at depth 4 (addresses 3, 12, 3; fresh "
            "tgsw_encrypt'ed selector bits each): words equal to the CPU reference: %s; largest phase error over all slots after write 1, 2, 3: "
            "%.3e, %.3e, %.3e (rms %.3e after the third; decoding condition of the tests: 2^-8 = %.3e; DESIGN.md section 7 derives the growth)"
            % (p.tlwe_alpha_min, same, errs[0].max(), errs[1].max(), errs[2].max(), float(np.sqrt(np.mean(errs[2] ** 2))), 2.0 ** -8))
        say()

        # ---- scatter beside the tree ----
        for items, depth in ((1, 10), (64, 10), (1024, 4)):
            d_set = full_range((depth, 2 * p.l, 2, N))  # any words are a sample to the arithmetic
            d_mem = full_range((items, 1 << depth, 2, N))
            d_val = full_range((items, 2, N))
            d_out = torch.zeros((items, 2, N), dtype=torch.int32, device=dev)
            sel_of = torch.from_numpy(np.tile(np.arange(depth, dtype=np.int32), (items, 1))).to(dev)
            table_of = torch.arange(items, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            with ctx.tgsw_prepare_device(d_set.data_ptr(), depth) as S:
                def tree():
                    st = ia.Stats()
                    ctx.lut_tree_device(S, items, depth, sel_of.data_ptr(), d_mem.data_ptr(), items, table_of.data_ptr(), d_out.data_ptr(), stats=st)
                    assert st.levels == depth and st.bootstraps == 0
                    return st.total_ms

                def scatter():
                    st = ia.Stats()
                    ctx.lut_scatter_device(S, items, depth, sel_of.data_ptr(), d_val.data_ptr(), d_mem.data_ptr(), d_mem.data_ptr(), stats=st)
                    assert st.levels == depth and st.bootstraps == 0
                    return st.total_ms

                tm, tlo, thi = timed(tree)
                sm, slo, shi = timed(scatter)
            products = items * ((1 << depth) - 1)
            plan = ctx.cmux_plan(items, depth)
            say("%d item%s x depth %d (%d external products, %d piece%s, %.0f MB of memory)"
                % (items, "" if items == 1 else "s", depth, products, plan["pieces"], "" if plan["pieces"] == 1 else "s", items * (8192 << depth) / 2.0 ** 20))
            say("  %-44s %9.3f ms [%.3f .. %.3f]   %10.1f lookups/s   %10.0f products/s" % ("lut_tree_device, one table per item", tm, tlo, thi, items / (tm * 1e-3), products / (tm * 1e-3)))
            say("  %-44s %9.3f ms [%.3f .. %.3f]   %10.1f writes/s    %10.0f products/s   %.2f x the lookup"
                % ("lut_scatter_device, in place", sm, slo, shi, items / (sm * 1e-3), products / (sm * 1e-3), sm / tm))
            del d_mem
            say()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
