#!/usr/bin/env python3
"""What the packing key switch costs beside the work that produced its rows, on one card in one run at the reference's
parameters (n = 630, N = 1024, packing decomposition t = 8, b = 2):

  * Context.pack_device of (groups, m) = (1, 32), (1, 256), (1, 1 024), (16, 256), (8, 1 024) at spread 1, and of (64, 4) at the
    table layout (tools.lut_pack_layout), beside
  * Context.keyswitch_device of the same number of rows, and
  * a gate call (AND) of the same number of rows.

The last two are a comparison, not a pass mark.  Every figure is ieache_stats.total_ms, the GPU timeline (HIP events) of the
whole call, of warm device-form calls on buffers made once, the forms by turns in rotating order; median [min .. max] of
--calls recorded calls after --warm unrecorded ones.  The K split the plan chose (Context.pack_plan) is recorded, and every K
split beside it at each size.  Before anything is timed the card's words are compared with the CPU reference, and the decode of packed gate
outputs and of a cloud-built table is checked; the largest phase errors seen go into the file.

    python scripts/pack_rates.py [--out profiles/pack_rates.txt] [--calls 7]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1, 32, False), (1, 256, False), (1, 1024, False), (16, 256, False), (8, 1024, False), (64, 4, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_rates.txt"))
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    import torch
    import ieache_amd as ia
    from ieache_amd import tools
    p = ia.default_params()
    k = tools.keygen_raw(p, (1, 2, 3))
    pk = tools.packing_keygen(p, k["lwe_key"], k["tlwe_key"], seed=5)
    rng = np.random.default_rng(1)
    lines = []
    dev = "cuda:%d" % a.device

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def by_turns(forms):
        rec = {label: [] for label, _ in forms}
        for i in range(a.warm + a.calls):
            r = i % len(forms)  # the order rotates from round to round, so that no form always follows the same one
            for label, f in forms[r:] + forms[:r]:
                ms = f()
                if i >= a.warm:
                    rec[label].append(ms)
        return rec

    def line(label, t, rows, base=None):
        m = float(np.median(t))
        say("  %-44s %8.3f ms [%.3f .. %.3f]   %10.0f rows/s%s" % (label, m, min(t), max(t), rows / (m * 1e-3),
                                                                  "" if base is None else "   %.3f of the gate call" % (m / base)))

    with ia.Context.from_arrays(p, k["bk"], k["ksk"], device=a.device) as ctx:
        cus = ctx.get_option("cus")
        ctx.set_packing_key(pk)
        say("Packing key switch beside the key switch alone and a gate call of the same rows: n = %d, N = %d, (t, b) = (8, 2), %d CUs, %s"
            % (p.n, p.N, cus, ctx.kernel_variant))
        say("Shipped: two kernels (product k_pack_gemm, then placement k_pack_place); the fused epilogue was not built, so there is no A/B of it.")
        say("ieache_stats.total_ms (HIP events around the whole call) of warm device-form calls (%d unrecorded, then %d recorded, the forms by turns "
            "in rotating order): median [min .. max]" % (a.warm, a.calls))
        say()

        # ---- correctness and noise first: gate outputs packed, a cloud-built table looked up ----
        bits = rng.integers(0, 2, size=(2, 1024)).astype(np.uint8)
        outs = ctx.gates(ia.GATE_XOR, tools.encrypt_bits(p, k["lwe_key"], bits[0], 11), tools.encrypt_bits(p, k["lwe_key"], bits[1], 12))
        want = bits[0] ^ bits[1]
        packed = ctx.pack(outs)
        same = bool(np.array_equal(packed[:, :, :], tools.pack_reference(p, pk, outs)))
        phase = tools.tlwe_phase(p, k["tlwe_key"], packed)[0].astype(np.float64) / 2.0 ** 32
        err = np.abs(phase - np.where(want == 1, 0.125, -0.125))
        say("1 024 XOR outputs packed at spread 1 (m w = 1 024): words equal to the CPU reference: %s; wrong decodes %d; phase error "
            "max %.3e, rms %.3e (margin 1/8; DESIGN.md section 7 derives a standard deviation of about 1.3e-4 + 0.8e-4 before the rows' own noise)"
            % (same, int(np.sum((phase > 0) != (want == 1))), err.max(), float(np.sqrt(np.mean(err ** 2)))))
        spread, shift = tools.lut_pack_layout(p, 4)
        f_bits = np.array([1, 0, 0, 1], dtype=np.uint8)
        entries = ctx.gates(ia.GATE_AND, tools.encrypt_bits(p, k["lwe_key"], f_bits, 13), tools.encrypt_bits(p, k["lwe_key"], np.ones(4, dtype=np.uint8), 14))
        table = ctx.pack(entries, spread=spread, shift=shift)
        v = tools.lut_test_poly(p, np.where(f_bits == 1, 1 << 29, -(1 << 29)).astype(np.int32))
        d = (tools.tlwe_phase(p, k["tlwe_key"], table)[0].astype(np.int64) - v.astype(np.int64)) & 0xFFFFFFFF
        terr = np.minimum(d, (1 << 32) - d) / 2.0 ** 32
        msgs = np.repeat(np.arange(4), 16)
        x = tools.encrypt_bits(p, k["lwe_key"], np.ones(len(msgs), dtype=np.uint8), 15)
        b = x[:, p.n].astype(np.int64) - (1 << 29) + (msgs.astype(np.int64) << 29)
        x[:, p.n] = (b & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
        looked = tools.decrypt_bits(p, k["lwe_key"], ctx.pbs(x, table, tlwe=True))
        say("a table of 4 gate outputs packed at the table layout (spread %d, shift %d): phase error against lut_test_poly max %.3e; "
            "64 lookups through pbs(tlwe=True): wrong decodes %d" % (spread, shift, terr.max(), int(np.sum(looked != f_bits[msgs]))))
        say()

        # ---- rates ----
        for groups, m, table_layout in SHAPES:
            rows = groups * m
            spread, shift = tools.lut_pack_layout(p, m) if table_layout else (1, 0)
            d_rows = torch.zeros((rows, ctx.lwe_stride), dtype=torch.int32, device=dev)
            d_rows[:, : p.n + 1] = torch.from_numpy(rng.integers(-(1 << 31), 1 << 31, size=(rows, p.n + 1), dtype=np.int64).astype(np.int32)).to(dev)
            d_b = d_rows.clone()
            d_out = torch.zeros((groups, 2, p.N), dtype=torch.int32, device=dev)
            d_u = torch.zeros((rows, ctx.extract_stride), dtype=torch.int32, device=dev)
            d_u[:, : p.N + 1] = torch.from_numpy(rng.integers(-(1 << 31), 1 << 31, size=(rows, p.N + 1), dtype=np.int64).astype(np.int32)).to(dev)
            d_ks, d_gate = torch.zeros((rows, ctx.lwe_stride), dtype=torch.int32, device=dev), torch.zeros((rows, ctx.lwe_stride), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()

            def pack_call(split):
                def f():
                    ctx.set_option("pack_split", split)
                    st = ia.Stats()
                    ctx.pack_device(groups, m, spread, shift, d_rows.data_ptr(), d_out.data_ptr(), stats=st)
                    assert st.bootstraps == 0 and st.keyswitch_launches >= 1
                    return st.total_ms
                return f

            def ks_call():
                st = ia.Stats()
                ctx.keyswitch_device(rows, d_u.data_ptr(), d_ks.data_ptr(), stats=st)
                return st.total_ms

            def gate_call():
                st = ia.Stats()
                ctx.gates_device(ia.GATE_AND, rows, d_rows.data_ptr(), d_b.data_ptr(), d_gate.data_ptr(), stats=st)
                assert st.bootstraps == rows
                return st.total_ms

            ctx.set_option("pack_split", 0)
            plan = ctx.pack_plan(groups, m)
            forms = [("pack, K split by the plan (%d)" % plan["k_split"], pack_call(0))] + [("pack, K split %d" % s, pack_call(s)) for s in (1, 2, 4, 8)]
            rec = by_turns(forms + [("keyswitch_device", ks_call), ("gate call (AND)", gate_call)])
            ctx.set_option("pack_split", 0)
            say("groups %d x m %d = %d rows, %s (spread %d, shift %d); pieces %d"
                % (groups, m, rows, "table layout" if table_layout else "spread 1", spread, shift, plan["pieces"]))
            base = float(np.median(rec["gate call (AND)"]))
            for label, _ in forms:
                line(label, rec[label], rows, base)
            line("keyswitch_device, the same rows", rec["keyswitch_device"], rows, base)
            line("gate call (AND), the same rows", rec["gate call (AND)"], rows)
            say()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
