#!/usr/bin/env python3
"""The full-adder circuit kinds (IEACHE_CIRC_*_FA: MAJ3 / XOR3 gates) against the reference's kinds, on one card in one run:

  * gate ops/s and expressions/s of add16 x 4096 and mul32 x 1024, reference kind and FA kind by turns;
  * single-expression latency of 32-bit A+B and A*B;
  * the noise the three-input gates see: smallest distance of a combined input phase to its decision boundary over 4 096
    gates of each type whose operands are bootstrapped outputs.

    python scripts/fa_rates.py [--out profiles/fa_circuits.txt] [--calls 3]

Rates are ieache_stats.bootstraps (resp. the batch) over ieache_stats.total_ms, the GPU timeline of a warm call; median and
range over --calls calls.  The decrypted results of the two kinds are compared before anything is timed."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAJ3, XOR3 = 32, 33


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fa_circuits.txt"))
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    import ieache_amd as ia
    from ieache_amd import tools
    p = ia.default_params()
    k = tools.keygen_raw(p, (1, 2, 3))
    rng = np.random.default_rng(1)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def operands(kind, bits, batch, seed):
        info = ia.circuit_info(kind, bits)
        b = np.zeros((batch, info.n_inputs), dtype=np.uint8)
        b[:, :2 * bits] = rng.integers(0, 2, size=(batch, 2 * bits))
        return b, tools.encrypt_bits(p, k["lwe_key"], b, seed)

    with ia.Context.from_arrays(p, k["bk"], k["ksk"], device=a.device) as ctx:
        say("full-adder circuit kinds against the reference's kinds: n = %d, N = %d, %d CUs, %s"
            % (p.n, p.N, ctx.get_option("cus"), ctx.kernel_variant))
        say("rates from ieache_stats.total_ms of warm calls (%d unrecorded, then %d recorded, the two kinds by turns): median [min .. max]"
            % (a.warm, a.calls))
        resident = ctx.get_option("resident_gates")
        say("the card holds %d gate instances at once (one wave per gate): a level is issued as launches of whole rounds of that many, "
            "so the gate rate of a circuit follows how its levels fill rounds" % resident)
        say()
        for name, ref_kind, fa_kind, bits, batch in (("add16", ia.CIRC_ADD, ia.CIRC_ADD_FA, 16, 4096),
                                                      ("mul32", ia.CIRC_MUL, ia.CIRC_MUL_FA, 32, 1024),
                                                      ("add32 single expression", ia.CIRC_ADD, ia.CIRC_ADD_FA, 32, 1),
                                                      ("mul32 single expression", ia.CIRC_MUL, ia.CIRC_MUL_FA, 32, 1)):
            _, inp = operands(ref_kind, bits, batch, 9)
            kinds = (("reference", ref_kind), ("full adder", fa_kind))
            outs = {}
            for label, kind in kinds:
                ctx.prepare(kind, bits, batch)
                for _ in range(a.warm if batch > 1 else 4):
                    outs[label] = ctx.eval_batch(kind, bits, inp)
            dec = {label: tools.decrypt_bits(p, k["lwe_key"], out) for label, out in outs.items()}
            assert np.array_equal(dec["reference"], dec["full adder"]), name
            ms = {label: [] for label, _ in kinds}
            wall = {label: [] for label, _ in kinds}
            for _ in range(a.calls if batch > 1 else 7):
                for label, kind in kinds:
                    st = ia.Stats()
                    t0 = time.perf_counter()
                    ctx.eval_batch(kind, bits, inp, st)
                    wall[label].append((time.perf_counter() - t0) * 1e3)
                    assert st.bootstraps == batch * ia.circuit_info(kind, bits).bootstraps
                    ms[label].append(st.total_ms)
            say("%s x %d" % (name, batch) if batch > 1 else name)
            med = {}
            for label, kind in kinds:
                info = ia.circuit_info(kind, bits)
                m, lo, hi = float(np.median(ms[label])), min(ms[label]), max(ms[label])
                med[label] = m
                boots = info.bootstraps * batch
                say("  %-10s %6d bootstraps/expression, %4d levels, mean level %7.0f gate instances = %.2f rounds (widest %d)"
                    % (label, info.bootstraps, info.sched_levels, boots / info.sched_levels, boots / info.sched_levels / resident,
                       info.sched_max_width * batch))
                if batch > 1:
                    say("             %9.3f ms [%.3f .. %.3f]   %10.0f gate ops/s [%.0f .. %.0f]   %9.1f expressions/s"
                        % (m, lo, hi, boots / (m * 1e-3), boots / (hi * 1e-3), boots / (lo * 1e-3), batch / (m * 1e-3)))
                else:
                    say("             %9.3f ms GPU timeline [%.3f .. %.3f], %.3f ms host wall clock (median of %d)"
                        % (m, lo, hi, float(np.median(wall[label])), len(wall[label])))
            r_info, f_info = ia.circuit_info(ref_kind, bits), ia.circuit_info(fa_kind, bits)
            say("  bootstrap ratio %.2f, time ratio %.2f%s" % (r_info.bootstraps / f_info.bootstraps, med["reference"] / med["full adder"],
                                                                "" if batch == 1 else ", gate rate of the full-adder kind %.2f of the reference kind's"
                                                                % ((f_info.bootstraps / med["full adder"]) / (r_info.bootstraps / med["reference"]))))
            say()

        # noise: operands that are themselves bootstrapped outputs, as the wires of a circuit are
        cnt = 4096
        raw = rng.integers(0, 2, size=(2, 3 * cnt)).astype(np.uint8)
        layer1 = ctx.gates(ia.GATE_XOR, tools.encrypt_bits(p, k["lwe_key"], raw[0], 451), tools.encrypt_bits(p, k["lwe_key"], raw[1], 452))
        b1 = (raw[0] ^ raw[1]).reshape(3, cnt)
        x = layer1.reshape(3, cnt, -1).view(np.uint32)
        s = np.asarray(k["lwe_key"][: p.n], dtype=np.int64)
        say("noise margins: %d gates of each type on bootstrapped operands, phases computed with the secret key" % cnt)
        for gate, label, mult, cst, nominal in ((MAJ3, "MAJ3", 1, 0, 1 / 8), (XOR3, "XOR3", 2, 1 << 31, 1 / 4)):
            want = (b1.sum(axis=0) >= 2) if gate == MAJ3 else (b1[0] ^ b1[1] ^ b1[2])
            out = ctx.gates3(gate, layer1.reshape(3, cnt, -1)[0], layer1.reshape(3, cnt, -1)[1], layer1.reshape(3, cnt, -1)[2])
            wrong = int(np.sum(tools.decrypt_bits(p, k["lwe_key"], out) != want.astype(np.uint8)))
            comb = (np.uint32(mult) * (x[0] + x[1] + x[2])).astype(np.uint32)
            comb[:, -1] += np.uint32(cst)
            comb = comb.view(np.int32)
            phase = ((comb[:, p.n].astype(np.int64) - comb[:, : p.n].astype(np.int64) @ s) & 0xFFFFFFFF) / 2.0 ** 32
            dist = np.abs((phase + 0.25) % 0.5 - 0.25)
            say("  %s: %d of %d outputs decrypt wrong; distance of the combined input phase to the decision boundary: smallest %.4f, "
                "mean %.4f, sd %.4f (nominal %.4f; the test asks for more than %.4f)"
                % (label, wrong, cnt, dist.min(), dist.mean(), dist.std(), nominal, nominal / 2))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
