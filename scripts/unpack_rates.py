#!/usr/bin/env python3
"""What the unpacking key switch (Context.unpack_device) and the read of an addressed word (Context.word_read_device,
include/ieache.h section 3m) cost beside the calls they replace, on one card in one run at the product parameters
(n = 630, N = 1024, l = 3, Bgbit = 7):

  unpack_device of 1 024 x 32 rows and of 64 x 1 rows, beside the same rows stored first -- unpack_device with
  IEACHE_UNPACK_NO_KEYSWITCH, then keyswitch_device -- and beside tlwe_extract_device + keyswitch_device, which takes one
  sample per ROW;
  word_read_device at 1 024 items x depth 4 x steps 5 x width 32, beside `width` lut_read_device calls of the same items and
  beside lut_write_coef_device of the same shape.

No rate is promised; the record is the deliverable.  Every figure is ieache_stats.total_ms, the GPU timeline (HIP events) of the
whole call, of warm device-form calls on buffers made once: the forms of a case by turns, the order rotated from round to
round, median [min .. max] of --calls recorded rounds after --warm unrecorded ones.  The last lines read the by-meaning table of
tests/test_unpack_cpu.py on the card and record how far the read rows' phases come from +-1/8.

    python scripts/unpack_rates.py [--out profiles/unpack_rates.txt] [--calls 5]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

UNPACKS = ((1024, 32), (64, 1))
READ = (1024, 4, 5, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unpack_rates.txt"))
    ap.add_argument("--calls", type=int, default=5)
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
        say("the unpacking key switch and the read of an addressed word beside their neighbours: n = %d, N = %d, l = %d, Bgbit = %d, %d CUs"
            % (p.n, N, p.l, p.Bgbit, ctx.get_option("cus")))
        say("ieache_stats.total_ms (HIP events around the whole call) of warm device-form calls, the forms of a case by turns in rotating order "
            "(%d unrecorded rounds, then %d recorded): median [min .. max]" % (a.warm, a.calls))
        say()

        # ---- the words first: small calls against the CPU references ----
        S, v, tab = words((5, 2 * p.l, 2, N)), words((3, 2, N)), words((2, 4, 2, N))
        same = bool(np.array_equal(ctx.unpack(v, 3, 100, 7), tools.unpack_reference(p, v, 3, 100, 7, ksk=k["ksk"])))
        say("3 samples unpacked over (first 3, width 100, spread 7), full-range words: equal to the CPU reference: %s" % same)
        with ctx.tgsw_prepare(S) as tg:
            same = bool(np.array_equal(ctx.word_read(tg, tab, 2, 3, width=32, unit=32, table_of=[1, 0, 1]),
                                       tools.word_read_reference(p, S, tab, 2, 3, width=32, unit=32, table_of=[1, 0, 1], ksk=k["ksk"])))
        say("3 items x depth 2 x steps 3 x width 32, full-range words: equal to the CPU reference: %s" % same)
        say()

        # ---- unpack beside the same rows stored first ----
        for count, width in UNPACKS:
            rows = count * width
            d_in = torch.from_numpy(words((count, 2, N))).to(dev)
            d_each = d_in.repeat_interleave(width, dim=0).contiguous()  # tlwe_extract_device takes one sample per row
            d_coef = torch.arange(width, dtype=torch.int32, device=dev).repeat(count).contiguous()
            d_u = torch.zeros((rows, ctx.extract_stride), dtype=torch.int32, device=dev)
            d_out = torch.zeros((rows, ctx.lwe_stride), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()

            def fused():
                st = ia.Stats()
                ctx.unpack_device(count, 0, width, 1, d_in.data_ptr(), d_out.data_ptr(), stats=st)
                assert st.levels == 1 and st.bootstraps == 0 and st.keyswitch_launches == 1
                return st.total_ms

            def stored():
                s1, s2 = ia.Stats(), ia.Stats()
                ctx.unpack_device(count, 0, width, 1, d_in.data_ptr(), d_u.data_ptr(), keyswitch=False, stats=s1)
                ctx.keyswitch_device(rows, d_u.data_ptr(), d_out.data_ptr(), stats=s2)
                return s1.total_ms + s2.total_ms

            def extracted():
                s1, s2 = ia.Stats(), ia.Stats()
                ctx.tlwe_extract_device(rows, d_each.data_ptr(), d_coef.data_ptr(), d_u.data_ptr(), stats=s1)
                ctx.keyswitch_device(rows, d_u.data_ptr(), d_out.data_ptr(), stats=s2)
                return s1.total_ms + s2.total_ms

            t = by_turns({"unpack_device": fused, "unpack_device(no key switch) + keyswitch_device": stored,
                          "tlwe_extract_device + keyswitch_device": extracted})
            say("%d samples x %d coefficients = %d rows (the extracted rows: %.1f MB)" % (count, width, rows, rows * ctx.extract_stride * 4 / 1e6))
            for name, (m, lo, hi) in t.items():
                say("  %-48s %9.3f ms [%.3f .. %.3f]  %8.2f us per row" % (name, m, lo, hi, 1e3 * m / rows))
            say("  unpack_device takes %.3f x the time of the same rows stored first" % (t["unpack_device"][0] / t["unpack_device(no key switch) + keyswitch_device"][0]))
            say()

        # ---- the read of a word beside `width` lookups and beside the write of the same shape ----
        items, depth, steps, width = READ
        bits = depth + steps
        ctx.set_projection_key(words((N, 8, 2, N)))  # any words are a key to the arithmetic
        d_set = torch.from_numpy(words((bits, 2 * p.l, 2, N))).to(dev)
        d_tab = torch.from_numpy(words((1 << depth, 2, N))).to(dev)
        d_new = torch.from_numpy(words((items, 2, N))).to(dev)
        d_mem = torch.from_numpy(words((items << depth, 2, N))).to(dev)
        d_sel = torch.from_numpy(np.tile(np.arange(bits, dtype=np.int32), (items, 1))).to(dev)
        d_am = torch.from_numpy(tools.rotate_amounts(steps, unit=width, N=N)).to(dev)
        d_out = torch.zeros((items * width, ctx.lwe_stride), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        with ctx.tgsw_prepare_device(d_set.data_ptr(), bits) as tg:
            ks = []

            def word_read():
                st = ia.Stats()
                ctx.word_read_device(tg, items, depth, steps, width, width, d_sel.data_ptr(), d_tab.data_ptr(), 1, None, d_out.data_ptr(), stats=st)
                assert st.levels == bits and st.bootstraps == 0
                ks.append(st.keyswitch_ms)
                return st.total_ms

            def lookups():
                total = 0.0
                for q in range(width):
                    st = ia.Stats()
                    ctx.lut_read_device(tg, items, depth, steps, d_sel.data_ptr(), d_am.data_ptr(), d_tab.data_ptr(), 1, None,
                                        d_out.data_ptr() + q * items * ctx.lwe_stride * 4, coef=q, stats=st)
                    total += st.total_ms
                return total

            def write_coef():
                st = ia.Stats()
                ctx.lut_write_coef_device(tg, items, depth, steps, width, width, d_sel.data_ptr(), d_new.data_ptr(), d_mem.data_ptr(), d_mem.data_ptr(), stats=st)
                return st.total_ms

            t = by_turns({"word_read_device": word_read, "%d lut_read_device calls" % width: lookups, "lut_write_coef_device, in place": write_coef})
        ctx.set_projection_key(None)
        say("%d items x depth %d x steps %d x width %d = %d rows (%d piece%s)"
            % (items, depth, steps, width, items * width, ctx.cmux_plan(items, depth)["pieces"], "" if ctx.cmux_plan(items, depth)["pieces"] == 1 else "s"))
        for name, (m, lo, hi) in t.items():
            say("  %-48s %9.3f ms [%.3f .. %.3f]" % (name, m, lo, hi))
        wr = t["word_read_device"][0]
        say("  of word_read_device the key switch's launches take %.3f ms (median); the call takes %.3f x the time of the %d lookups and %.2f x lut_write_coef_device's"
            % (float(np.median(ks[a.warm:])), wr / t["%d lut_read_device calls" % width][0], width, wr / t["lut_write_coef_device, in place"][0]))
        say()

        # ---- by meaning: the table of tests/test_unpack_cpu.py read on the card ----
        from test_unpack_cpu import word_of, word_table, worst_phase_error
        sc = word_table(p, k["tlwe_key"])
        with ctx.tgsw_prepare(sc["samples"]) as tg:
            got = ctx.word_read(tg, sc["tables"], sc["depth"], sc["steps"], width=sc["width"], unit=sc["unit"], sel_of=sc["sel_of"])
        want = tools.word_read_reference(p, sc["samples"], sc["tables"], sc["depth"], sc["steps"], width=sc["width"], unit=sc["unit"], sel_of=sc["sel_of"],
                                         ksk=k["ksk"])
        clear = [int(sc["clear"][slot, word]) for slot, word in sc["addrs"]]
        worst = max(worst_phase_error(k["lwe_key"], got[i], clear[i]) for i in range(len(clear)))
        right = all(word_of(tools.decrypt_bits(p, k["lwe_key"], got[i])) == clear[i] for i in range(len(clear)))
        say("by meaning: %d sixteen-bit words of a client-encrypted table of 4 samples x 64 words (bits at +-1/8) read at encrypted addresses: equal to the "
            "CPU reference: %s; every word decrypts to the clear one: %s; largest distance of a read row's phase from +-1/8: %.3e (a wrong bit needs 1.25e-01)"
            % (len(clear), bool(np.array_equal(got, want)), right, worst))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
