#!/usr/bin/env python3
"""What an automaton over encrypted words costs (Context.automaton_run_device, include/ieache.h section 3k) with every step of
an item inside ONE launch, beside the same call with a launch per step (option automaton_steps_per_launch = 1: the hand-off a
kernel boundary) and beside a CMux tree (Context.lut_tree_device) of about the same CMux count, on one card in one run at the
product parameters (n = 630, N = 1024, l = 3, Bgbit = 7): states 2, 6, 16 x steps 16, 64, 256 x 1, 64, 1 024 items, every state
live and a CMux (next0 = q, next1 = q + 1 mod states, n_out = states); then less_than(32) for 1 and 1 024 pairs beside
netlists.compare(32) as a gate call on the same context; then the phase error of less_than(8) on client-encrypted letters
beside the figure of DESIGN.md section 7.

No rate is promised; the record is the deliverable.  Every figure is ieache_stats.total_ms, the GPU timeline (HIP events) of the
whole call, of warm device-form calls on buffers made once: the forms of a case by turns, the order rotated from round to
round, median [min .. max] of --calls recorded rounds after --warm unrecorded ones.

    python scripts/automaton_rates.py [--out profiles/automaton_rates.txt] [--calls 7]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STATES, STEPS, ITEMS = (2, 6, 16), (16, 64, 256), (1, 64, 1024)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "automaton_rates.txt"))
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    import torch
    import ieache_amd as ia
    from ieache_amd import automata, netlists, tools
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
        say("automata over encrypted words (automaton_run_device), every step of an item in one launch, beside a launch per step "
            "(automaton_steps_per_launch = 1) and a CMux tree (lut_tree_device) of about the same CMux count: n = %d, N = %d, l = %d, Bgbit = %d, %d CUs"
            % (p.n, N, p.l, p.Bgbit, ctx.get_option("cus")))
        say("ieache_stats.total_ms (HIP events around the whole call) of warm device-form calls, the forms of a case by turns in rotating order "
            "(%d unrecorded rounds, then %d recorded): median [min .. max]" % (a.warm, a.calls))
        say()

        # ---- the words first: a small call against the CPU reference, fused and with a launch per step ----
        S, F = words((5, 2 * p.l, 2, N)), words((1, 5, 2, N))
        n0 = rng.integers(0, 5, size=(6, 5)).astype(np.int32)
        n1 = rng.integers(0, 5, size=(6, 5)).astype(np.int32)
        with ctx.tgsw_prepare(S) as tg, ctx.automaton(n0, n1, 5) as au:
            want = tools.automaton_reference(p, S, n0, n1, F, n_out=5, count=3)
            same = bool(np.array_equal(ctx.automaton_run(tg, au, F, count=3), want))
            ctx.set_option("automaton_steps_per_launch", 1)
            same1 = bool(np.array_equal(ctx.automaton_run(tg, au, F, count=3), want))
            ctx.set_option("automaton_steps_per_launch", 0)
        say("3 items x 5 states x 6 steps, full-range words: equal to the CPU reference: %s (one launch), %s (a launch per step)" % (same, same1))
        say()

        d_set = torch.from_numpy(words((max(STEPS), 2 * p.l, 2, N))).to(dev)  # any words are a sample to the arithmetic
        torch.cuda.synchronize()
        slower = []
        with ctx.tgsw_prepare_device(d_set.data_ptr(), max(STEPS)) as tg:
            for states in STATES:
                q = np.arange(states, dtype=np.int32)
                d_fin = torch.from_numpy(words((states, 2, N))).to(dev)
                for steps in STEPS:
                    depth = int(round(np.log2(states * steps + 1)))
                    d_table = torch.from_numpy(words((1 << depth, 2, N))).to(dev)
                    with ctx.automaton(np.tile(q, (steps, 1)), np.tile((q + 1) % states, (steps, 1)), states) as au:
                        assert au.cmuxes == states * steps
                        for items in ITEMS:
                            d_out = torch.zeros((items, states, 2, N), dtype=torch.int32, device=dev)
                            d_tree = torch.zeros((items, 2, N), dtype=torch.int32, device=dev)
                            torch.cuda.synchronize()

                            def run(per):
                                def f():
                                    ctx.set_option("automaton_steps_per_launch", per)
                                    st = ia.Stats()
                                    ctx.automaton_run_device(tg, au, items, None, d_fin.data_ptr(), 1, None, d_out.data_ptr(), stats=st)
                                    ctx.set_option("automaton_steps_per_launch", 0)
                                    assert st.levels == steps and st.bootstraps == 0
                                    return st.total_ms
                                return f

                            def tree():
                                st = ia.Stats()
                                ctx.lut_tree_device(tg, items, depth, None, d_table.data_ptr(), 1, None, d_tree.data_ptr(), stats=st)
                                return st.total_ms

                            plan = ctx.automaton_plan(au, items)
                            t = by_turns({"one launch": run(0), "a launch per step": run(1), "lut_tree depth %d" % depth: tree})
                            cm = items * states * steps
                            say("%d items x %d states x %d steps (%d CMuxes, %d piece%s of %d launch%s; the tree: %d CMuxes)"
                                % (items, states, steps, cm, plan["pieces"], "" if plan["pieces"] == 1 else "s", plan["launches"],
                                   "" if plan["launches"] == 1 else "es", items * ((1 << depth) - 1)))
                            for name, (m, lo, hi) in t.items():
                                say("  %-22s %10.3f ms [%.3f .. %.3f]  %8.3f us per CMux" % (name, m, lo, hi, 1e3 * m / (items * ((1 << depth) - 1) if name.startswith("lut") else cm)))
                            ratio = t["a launch per step"][0] / t["one launch"][0]
                            say("  a launch per step takes %.2f x the time of one launch" % ratio)
                            if ratio < 1.0:
                                slower.append((items, states, steps, ratio))
                            del d_out, d_tree
                    del d_table
        say()
        say("shapes where one launch is NOT the faster of the two: %s" % (", ".join("%d x %d x %d (%.2f)" % s for s in slower) if slower else "none"))
        say()

        # ---- less_than(32) beside the bootstrapped comparison netlist on the same context ----
        bits = 32
        lt = automata.less_than(bits)
        nl = netlists.compare(bits)
        fin = torch.from_numpy(automata.final_rows(lt, N)).to(dev)
        d_letters = torch.from_numpy(words((2 * bits, 2 * p.l, 2, N))).to(dev)
        torch.cuda.synchronize()
        with ctx.tgsw_prepare_device(d_letters.data_ptr(), 2 * bits) as tg, ctx.automaton(lt.next0, lt.next1) as au:
            for pairs in (1, 1024):
                d_out = torch.zeros((pairs, 1, 2, N), dtype=torch.int32, device=dev)
                in_bits = rng.integers(0, 2, size=(pairs, 2 * bits)).astype(np.uint8)
                in_lwe = tools.encrypt_bits(p, k["lwe_key"], in_bits, 5)
                stride = p.lwe_stride
                padded = np.zeros((pairs, 2 * bits, stride), dtype=np.int32)
                padded[:, :, :p.n + 1] = in_lwe
                d_in = torch.from_numpy(padded).to(dev)
                d_gate = torch.zeros((pairs, 2, stride), dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                ctx.prepare_netlist(nl, pairs)

                def run(per):
                    def f():
                        ctx.set_option("automaton_steps_per_launch", per)
                        st = ia.Stats()
                        ctx.automaton_run_device(tg, au, pairs, None, fin.data_ptr(), 1, None, d_out.data_ptr(), stats=st)
                        ctx.set_option("automaton_steps_per_launch", 0)
                        return st.total_ms
                    return f

                def gates():
                    st = ia.Stats()
                    ctx.eval_netlist_device(nl, pairs, d_in.data_ptr(), d_gate.data_ptr(), stats=st)
                    return st.total_ms

                t = by_turns({"one launch": run(0), "a launch per step": run(1), "netlists.compare(32)": gates})
                say("less_than(32) for %d pair%s: %d steps x 5 states, %d live CMuxes per pair; the netlist: %d bootstraps per pair (both outputs, A < B and A == B)"
                    % (pairs, "" if pairs == 1 else "s", au.steps, au.cmuxes, nl.info().bootstraps))
                for name, (m, lo, hi) in t.items():
                    say("  %-22s %10.3f ms [%.3f .. %.3f]" % (name, m, lo, hi))
                say("  the gate netlist takes %.1f x the time of the automaton (which still needs tlwe_extract and one key switch per pair to rejoin the gates)"
                    % (t["netlists.compare(32)"][0] / t["one launch"][0]))
                del d_out, d_in, d_gate
        say()

        # ---- by meaning: the phase error of less_than(8) on client-encrypted letters ----
        lt8 = automata.less_than(8)
        pairs = [(0, 0), (255, 255), (77, 77), (128, 0), (0, 128), (1, 0), (0, 1), (100, 101), (101, 100), (37, 200), (200, 37), (127, 128)]
        letters = np.stack([lt8.word(x, y) for x, y in pairs]).reshape(-1).astype(np.int32)
        samples = tools.tgsw_encrypt(p, k["tlwe_key"], letters, 77)
        with ctx.tgsw_prepare(samples) as tg, ctx.automaton(lt8.next0, lt8.next1) as au:
            out = ctx.automaton_run(tg, au, automata.final_rows(lt8, N), count=len(pairs))
        want = np.array([x < y for x, y in pairs])
        phase = tools.tlwe_phase(p, k["tlwe_key"], out[:, 0])[:, 0]
        d = (phase.astype(np.int64) - np.where(want, 1 << 29, -(1 << 29))) & 0xFFFFFFFF
        err = np.minimum(d, (1 << 32) - d) / 2.0 ** 32
        bits_out = tools.decrypt_bits(p, k["lwe_key"], ctx.keyswitch(ctx.tlwe_extract(out[:, 0]))).astype(bool)
        say("less_than(8) on %d pairs of client-encrypted letters (tools.tgsw_encrypt, alpha = %.3g), trivial +-1/8 finals, 16 CMux steps:" % (len(pairs), p.tlwe_alpha_min))
        say("  largest phase error of coefficient 0 before the key switch: %.3e; decoding distance 1/8 = 1.250e-01; DESIGN.md section 7 derives a standard "
            "deviation of sqrt(16) x 8.6e-5 = 3.4e-4 plus a truncation ramp of at most 16 x 1.2e-4 = 1.9e-3 for 16 steps at (3, 7)" % err.max())
        say("  after tlwe_extract -> keyswitch, decrypt_bits equals a < b on every pair: %s" % bool(np.array_equal(bits_out, want)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
