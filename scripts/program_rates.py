#!/usr/bin/env python3
"""Word programs (ieache_program_compile) against the same expressions as one built-in call per operator, at the product
parameters (n = 630), on one GPU:

  * a*b + c*d at 32 bits (two reference multipliers, one 64-bit reference addition) as one program, against its three calls;
  * the sum of 8 x 32-bit operands mod 2^32 as one SUM, full-adder and Kogge-Stone tail, against seven CIRC_ADD calls and
    against seven CIRC_ADD_FA calls (each fed the previous one's ciphertext);
  * maximum(a + b, c) at 32 bits (no built-in counterpart: the program alone);
  * batches 1 and 8; the whole call timed by the evaluator's own GPU event timers (ieache_stats.total_ms; a leg of several
    calls is the sum over them), warm, the ways taken by turns; median and range of --calls recorded turns;
  * every program's decryption compared with the integers, and a*b + c*d word for word with its three calls, before anything
    is timed.

    python scripts/program_rates.py [--out profiles/program_rates.txt] [--calls 7]

The file is the record: DESIGN and README quote it, nothing else states a rate."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "program_rates.txt"))
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--batches", default="1,8")
    a = ap.parse_args()
    assert a.calls >= 7, "the median of at least 7 turns"

    import ieache_amd as ia
    from ieache_amd import tools
    p = ia.default_params()
    k = tools.keygen_raw(p, (1, 2, 3))
    rng = np.random.default_rng(1)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def encrypt(values, widths, seed):
        bits = np.array([[(v >> j) & 1 for v, w in zip(row, widths) for j in range(w)] for row in values], dtype=np.uint8)
        return tools.encrypt_bits(p, k["lwe_key"], bits, seed)

    def decrypt(out):
        return [sum(int(b) << j for j, b in enumerate(row)) for row in tools.decrypt_bits(p, k["lwe_key"], out)]

    def timed(ways, title, detail):
        ms = {label: [] for label, _ in ways}
        for i in range(a.warm + a.calls):
            for label, f in ways:
                t = f()
                if i >= a.warm:
                    ms[label].append(t)
        say("%s -- %s" % (title, detail))
        base = float(np.median(ms[ways[-1][0]])) if len(ways) > 1 else None
        for label, _ in ways:
            m, lo, hi = float(np.median(ms[label])), min(ms[label]), max(ms[label])
            say("  %-34s %9.1f ms [%.1f .. %.1f]%s" % (label, m, lo, hi, "   %.3f of the last line's time" % (m / base) if base else ""))
        say()

    def program_way(ctx, compiled, inp):
        def f():
            st = ia.Stats()
            ctx.eval_netlist(compiled, inp, st)
            return st.total_ms
        return f

    with ia.Context.from_arrays(p, k["bk"], k["ksk"], device=0) as ctx:
        say("word programs against one built-in call per operator: n = %d, N = %d, %d CUs, %s" % (p.n, p.N, ctx.get_option("cus"), ctx.kernel_variant))
        say("GPU time of the whole call (ieache_stats.total_ms; several calls: the sum over them), warm: %d unrecorded turns, then %d recorded, "
            "the ways by turns; median [min .. max]" % (a.warm, a.calls))
        say()
        zero_carry = lambda batch: encrypt([[0]] * batch, (32,), 9)  # noqa: E731
        for batch in (int(b) for b in a.batches.split(",")):
            # ---- a*b + c*d ----
            prog = ia.WordProgram()
            ra, rb, rc, rd, carry = (prog.input(32) for _ in range(5))
            compiled = prog.compile([prog.add(prog.mul(ra, rb, carry), prog.mul(rc, rd, carry), carry)])
            values = [[int(v) for v in rng.integers(0, 1 << 32, size=4)] + [0] for _ in range(batch)]
            inp = encrypt(values, (32,) * 5, 100 + batch)
            A, B, Cc, D, cy = (inp[:, 32 * i:32 * (i + 1)] for i in range(5))
            ab_in, cd_in = np.concatenate([A, B, cy], axis=1), np.concatenate([Cc, D, cy], axis=1)

            def three_calls(keep=None):
                ms, st = 0.0, ia.Stats()
                ab = ctx.eval_batch(ia.CIRC_MUL, 32, ab_in, st)
                ms += st.total_ms
                cd = ctx.eval_batch(ia.CIRC_MUL, 32, cd_in, st)
                ms += st.total_ms
                out = ctx.eval_batch(ia.CIRC_ADD, 64, np.concatenate([ab, cd, cy], axis=1), st)
                if keep is not None:
                    keep.append(out)
                return ms + st.total_ms
            ctx.prepare_netlist(compiled, batch)
            kept, st = [], ia.Stats()
            three_calls(kept)
            got = ctx.eval_netlist(compiled, inp, st)
            assert np.array_equal(got, kept[0]), "a*b + c*d: the program and its three calls differ"
            assert decrypt(got) == [(v[0] * v[1] + v[2] * v[3]) % (1 << 64) for v in values]
            info = compiled.info()
            timed([("one program", program_way(ctx, compiled, inp)), ("three calls (mul32, mul32, add64)", three_calls)],
                  "a*b + c*d, 32-bit operands, batch %d" % batch,
                  "program: %d bootstraps, %d levels; the calls: %d + %d + %d levels; same ciphertext"
                  % (info.bootstraps, st.levels, ia.circuit_info(ia.CIRC_MUL, 32).depth, ia.circuit_info(ia.CIRC_MUL, 32).depth,
                     ia.circuit_info(ia.CIRC_ADD, 64).depth))

            # ---- the sum of eight words ----
            values = [[int(v) for v in rng.integers(0, 1 << 32, size=8)] for _ in range(batch)]
            inp = encrypt(values, (32,) * 8, 200 + batch)
            words = [inp[:, 32 * i:32 * (i + 1)] for i in range(8)]
            cy = zero_carry(batch)
            want = [sum(v) % (1 << 32) for v in values]

            def seven_calls(kind):
                def f(keep=None):
                    ms, st, acc = 0.0, ia.Stats(), words[0]
                    for w in words[1:]:
                        acc = ctx.eval_batch(kind, 32, np.concatenate([acc, w, cy], axis=1), st)
                        ms += st.total_ms
                    if keep is not None:
                        keep.append(acc)
                    return ms
                return f
            ways, shapes = [], []
            for label, family in (("one SUM, full-adder tail", 3), ("one SUM, Kogge-Stone tail", 1)):
                prog = ia.WordProgram()
                compiled = prog.compile([prog.sum([prog.input(32) for _ in range(8)], 32, family=family)])
                ctx.prepare_netlist(compiled, batch)
                assert decrypt(ctx.eval_netlist(compiled, inp)) == want, label
                ways.append((label, program_way(ctx, compiled, inp)))
                shapes.append("%s: %d bootstraps, %d levels" % (label, compiled.info().bootstraps, compiled.info().depth))
            for label, kind in (("seven CIRC_ADD_FA calls", ia.CIRC_ADD_FA), ("seven CIRC_ADD calls", ia.CIRC_ADD)):
                kept = []
                seven_calls(kind)(kept)
                assert decrypt(kept[0]) == want, label
                ways.append((label, seven_calls(kind)))
                shapes.append("%s: %d bootstraps, %d levels" % (label, 7 * ia.circuit_info(kind, 32).bootstraps, 7 * ia.circuit_info(kind, 32).depth))
            timed(ways, "sum of 8 x 32-bit operands mod 2^32, batch %d" % batch, "; ".join(shapes))

            # ---- maximum(a + b, c) ----
            prog = ia.WordProgram()
            ra, rb, rc = prog.input(32), prog.input(32), prog.input(32)
            compiled = prog.compile([prog.maximum(ra + rb, rc)])
            values = [[int(v) for v in rng.integers(0, 1 << 32, size=3)] for _ in range(batch)]
            inp = encrypt(values, (32,) * 3, 300 + batch)
            ctx.prepare_netlist(compiled, batch)
            assert decrypt(ctx.eval_netlist(compiled, inp)) == [max((v[0] + v[1]) % (1 << 32), v[2]) for v in values]
            timed([("one program", program_way(ctx, compiled, inp))], "maximum(a + b, c), 32-bit operands, batch %d" % batch,
                  "%d bootstraps, %d levels (reference addition, XNOR / MUX comparison, MUX selection); no built-in counterpart"
                  % (compiled.info().bootstraps, compiled.info().depth))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
