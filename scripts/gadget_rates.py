#!/usr/bin/env python3
"""What a TGSW set with a gadget of its own (Context.tgsw_prepare(samples, l, Bgbit), include/ieache.h section 3i) costs beside a
set at the key's gadget, on one card in one run at the product parameters (n = 630, N = 1024, key at l = 3, Bgbit = 7).  Per gadget:
  * 16 384 CMuxes with ONE selector shared by every row (Context.cmux_device),
  * 1 024 depth-4 replace writes in place (Context.lut_write_device, every item a memory of its own),
  * 16 384 rows x 10 rotation steps in place (Context.tlwe_rotate_device).
The first line is (3, 7) on the builds it always had; the second (3, 7) again on the builds that take (l, Bgbit) as launch
arguments, through the unstable debug option "cmux_gadget_runtime"; then the gadgets only those builds serve.  The digit rows of
a product scale with 2l and its four inverse transforms do not, so no rate is promised: the record is the deliverable, and the
ratios to the first line of the same run are what to quote.  The first line also carries lut_scatter_device of 1 024 x depth 4 in
place, the figure scripts/scatter_rates.py records, and its 16 384 CMuxes are the figure of scripts/cmux_rates.py: run those two
from the parent commit on the same box and pass their files with --parent to have both numbers set side by side.

Every figure is ieache_stats.total_ms, the GPU timeline (HIP events) of the whole call, of warm device-form calls on buffers made
once; median [min .. max] of --calls recorded calls after --warm unrecorded ones, and one whole line runs unrecorded before
the first.  The last line repeats the first, to show what the run itself drifts by.  Words are random: any words are a sample to the
arithmetic.

    python scripts/gadget_rates.py [--out profiles/gadget_rates.txt] [--calls 5] [--parent cmux_rates.txt scatter_rates.txt]"""
import argparse
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GADGETS = [(4, 6), (6, 5), (8, 4), (4, 8), (16, 2), (2, 10)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gadget_rates.txt"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--parent", nargs=2, metavar=("CMUX_RATES", "SCATTER_RATES"), help="files written by the parent commit's scripts on the same box")
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
    ROWS, ITEMS, DEPTH, STEPS = 16384, 1024, 4, 10

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def full_range(shape):
        return torch.from_numpy(rng.integers(-(1 << 31), 1 << 31, size=shape, dtype=np.int64).astype(np.int32)).to(dev)

    def timed(f):
        t = [f() for _ in range(a.warm + a.calls)][a.warm:]
        return float(np.median(t)), min(t), max(t)

    with ia.Context.from_arrays(p, k["bk"], k["ksk"], device=a.device) as ctx:
        say("TGSW sets with a gadget of their own beside the key's: n = %d, N = %d, key at l = %d, Bgbit = %d, %d CUs" % (p.n, N, p.l, p.Bgbit, ctx.get_option("cus")))
        say("ieache_stats.total_ms (HIP events around the whole call) of warm device-form calls (%d unrecorded, then %d recorded): median [min .. max]"
            % (a.warm, a.calls))
        say("columns: %d CMuxes, one shared selector | %d depth-%d replace writes in place (lut_write_device) | %d rows x %d rotation steps in place"
            % (ROWS, ITEMS, DEPTH, ROWS, STEPS))
        say()
        d_rows, d_zero, d_out = full_range((ROWS, 2, N)), full_range((ROWS, 2, N)), torch.zeros((ROWS, 2, N), dtype=torch.int32, device=dev)
        d_mem, d_new = full_range((ITEMS, 1 << DEPTH, 2, N)), full_range((ITEMS, 2, N))
        shared = torch.zeros(ROWS, dtype=torch.int32, device=dev)
        sel_of = torch.from_numpy(np.tile(np.arange(DEPTH, dtype=np.int32), (ITEMS, 1))).to(dev)  # scatter_rates.py's selectors
        base, first = None, {}

        def line(l, Bgbit, label, runtime, record=True):
            nonlocal base
            d_set = full_range((STEPS, 2 * l, 2, N))
            torch.cuda.synchronize()
            ctx.set_option("cmux_gadget_runtime", 1 if runtime else 0)
            with ctx.tgsw_prepare_device(d_set.data_ptr(), STEPS, l, Bgbit) as S:
                def stat(f):
                    def g():
                        st = ia.Stats()
                        f(st)
                        assert st.bootstraps == 0
                        return st.total_ms
                    return timed(g)
                c = stat(lambda st: ctx.cmux_device(S, ROWS, shared.data_ptr(), d_rows.data_ptr(), d_zero.data_ptr(), d_out.data_ptr(), stats=st))
                w = stat(lambda st: ctx.lut_write_device(S, ITEMS, DEPTH, None, d_new.data_ptr(), d_mem.data_ptr(), d_mem.data_ptr(), stats=st))
                r = stat(lambda st: ctx.tlwe_rotate_device(S, ROWS, STEPS, None, None, d_rows.data_ptr(), d_rows.data_ptr(), stats=st))
                if record and l == p.l and Bgbit == p.Bgbit and not runtime:
                    first.setdefault("scatter", []).append(stat(lambda st: ctx.lut_scatter_device(S, ITEMS, DEPTH, sel_of.data_ptr(), d_new.data_ptr(), d_mem.data_ptr(), d_mem.data_ptr(), stats=st)))
                    first.setdefault("cmux", []).append(c)
            ctx.set_option("cmux_gadget_runtime", 0)
            if not record:
                return
            if base is None:
                base = (c[0], w[0], r[0])
            say("(%2d, %2d) %-22s %8.3f ms [%.3f .. %.3f] %5.2fx | %8.3f ms [%.3f .. %.3f] %5.2fx | %9.3f ms [%.3f .. %.3f] %5.2fx"
                % (l, Bgbit, label, c[0], c[1], c[2], c[0] / base[0], w[0], w[1], w[2], w[0] / base[1], r[0], r[1], r[2], r[0] / base[2]))

        line(p.l, p.Bgbit, "", False, record=False)  # one whole line unrecorded: the card's clocks and the caches settle on it
        line(p.l, p.Bgbit, "shipped builds", False)
        line(p.l, p.Bgbit, "run-time builds", True)
        for l, Bgbit in GADGETS:
            line(l, Bgbit, "shipped builds" if (l, Bgbit) == (2, 10) else "run-time builds", False)
        line(p.l, p.Bgbit, "shipped builds, again", False)
        say()
        say("(x: the ratio to the first line.  2l digit rows per product: 6 at (3, 7), 8 at (4, 6) and (4, 8), 12 at (6, 5), 16 at (8, 4), 32 at (16, 2), 4 at (2, 10).)")
        say()
        # this run's own spread of a figure: from the smallest to the largest recorded call of the first line and of its repeat
        spread = {k: (min(t[1] for t in v), max(t[2] for t in v)) for k, v in first.items()}
        cm, sc = spread["cmux"], spread["scatter"]
        say("the dispatch where nothing changed, (3, 7) on the shipped builds, first line and its repeat, this run's own spread: cmux_device %d rows, one "
            "shared selector %.3f .. %.3f ms (medians %s); lut_scatter_device %d items x depth %d in place %.3f .. %.3f ms (medians %s)"
            % (ROWS, cm[0], cm[1], ", ".join("%.3f" % t[0] for t in first["cmux"]), ITEMS, DEPTH, sc[0], sc[1], ", ".join("%.3f" % t[0] for t in first["scatter"])))
        if a.parent:
            num = r"\s+([0-9.]+) ms \[([0-9.]+) \.\. ([0-9.]+)\]"
            with open(a.parent[0]) as f:
                text = f.read()
            m = re.search(r"cmux_device, one shared selector" + num, text[text.index("16384 rows"):] if "16384 rows" in text else "")
            with open(a.parent[1]) as f:
                text = f.read()
            s = re.search(r"lut_scatter_device, in place" + num, text[text.index("1024 items x depth 4"):] if "1024 items x depth 4" in text else "")
            say("the parent commit's scripts on the same box: cmux_rates.py, 16384 rows, shared selector: %s; scatter_rates.py, 1024 items x depth 4, in place: %s"
                % ("%s ms [%s .. %s]" % m.groups() if m else "line not found", "%s ms [%s .. %s]" % s.groups() if s else "line not found"))
            for what, found, (lo, hi) in (("cmux_device", m, cm), ("lut_scatter_device", s, sc)):
                if found:
                    plo, phi = float(found.group(2)), float(found.group(3))
                    say("  %s: the parent's calls %.3f .. %.3f ms %s this run's spread %.3f .. %.3f ms"
                        % (what, plo, phi, "overlap" if plo <= hi and lo <= phi else ("lie ABOVE" if plo > hi else "lie BELOW"), lo, hi))
        else:
            say("the parent commit's scripts on the same box: not measured")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
