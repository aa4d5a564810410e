#!/usr/bin/env python3
"""Host time per call of the seven calls on a caller TGSW set (include/ieache.h sections 3f to 3j), one build of libieache.so
beside another, on one card in one command:

    python scripts/set_calls_ab.py parent_a=<libieache.so> parent_b=<a copy of it> new=<libieache.so> [--rounds 7] [--out FILE]

Every round starts one fresh process per library (IEACHE_LIBRARY), the order rotated from round to round.  A process takes

  * the host wall time (time.perf_counter around the call, which ends in a stream synchronise) of each call in both forms at
    count = 1, depth 2, steps 2 -- the overhead case: the median of --calls warm calls, in microseconds;
  * ieache_stats.total_ms and the wall time of one product-size device-form case per call family, the cases of cmux_rates.py,
    scatter_rates.py, rotate_rates.py, gadget_rates.py and lut_add_rates.py: the median of 3 warm calls, in milliseconds.

The first two names are the same library loaded twice: the span of their rounds, min .. max over both, is what the card and the
host do to a figure on their own.  Each line gives median [min .. max] over the rounds per name and says whether the last
name's median lies within that span; the exit status is 1 if one does not."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COUNT, DEPTH, STEPS = 1, 2, 2


def child(keys, calls):
    import torch
    import ieache_amd as ia
    p = ia.default_params()
    k = np.load(keys)
    rng = np.random.default_rng(1)
    N = p.N
    out = {}

    def words(*shape):
        return rng.integers(-(1 << 31), 1 << 31, size=shape, dtype=np.int64).astype(np.int32)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def wall(f, n, warm):
        t = []
        for i in range(warm + n):
            t0 = time.perf_counter()
            f()
            t.append(time.perf_counter() - t0)
        return float(np.median(t[warm:]))

    with ia.Context.from_arrays(p, k["bk"], k["ksk"]) as ctx:
        # ---- the overhead case ----
        S = words(DEPTH + STEPS, 2 * p.l, 2, N)
        sel_d, sel_s, sel_ds = np.zeros((1, DEPTH), np.int32), np.zeros((1, STEPS), np.int32), np.zeros((1, DEPTH + STEPS), np.int32)
        am = np.array([1, 2], np.int32)
        row, leaves = words(1, 2, N), words(1, 1 << DEPTH, 2, N)
        with ctx.tgsw_prepare(S) as tg:
            host = {
                "cmux": lambda: ctx.cmux(tg, row, row, sel_of=[0]),
                "lut_tree": lambda: ctx.lut_tree(tg, leaves, DEPTH, sel_of=sel_d),
                "lut_scatter": lambda: ctx.lut_scatter(tg, row, DEPTH, sel_of=sel_d, mem=leaves),
                "tlwe_rotate": lambda: ctx.tlwe_rotate(tg, row, STEPS, sel_of=sel_s, amounts=am),
                "lut_read": lambda: ctx.lut_read(tg, leaves, DEPTH, STEPS, sel_of=sel_ds, amounts=am),
                "lut_add": lambda: ctx.lut_add(tg, row, DEPTH, STEPS, sel_of=sel_ds, amounts=am, mems=leaves),
            }
            d_row, d_leaves, d_out = dev(row), dev(leaves), torch.zeros((1 << DEPTH, 2, N), dtype=torch.int32, device="cuda")
            d_sel, d_am, d_lwe = dev(sel_ds), dev(am), torch.zeros((1, max(ctx.lwe_stride, N + 1)), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            P = lambda t: t.data_ptr()
            device = {
                "cmux": lambda: ctx.cmux_device(tg, 1, P(d_sel), P(d_row), P(d_row), P(d_out)),
                "lut_tree": lambda: ctx.lut_tree_device(tg, 1, DEPTH, P(d_sel), P(d_leaves), 1, None, P(d_out)),
                "lut_scatter": lambda: ctx.lut_scatter_device(tg, 1, DEPTH, P(d_sel), P(d_row), P(d_leaves), P(d_out)),
                "lut_write": lambda: ctx.lut_write_device(tg, 1, DEPTH, P(d_sel), P(d_row), P(d_leaves), P(d_out)),
                "tlwe_rotate": lambda: ctx.tlwe_rotate_device(tg, 1, STEPS, P(d_sel), P(d_am), P(d_row), P(d_out)),
                "lut_read": lambda: ctx.lut_read_device(tg, 1, DEPTH, STEPS, P(d_sel), P(d_am), P(d_leaves), 1, None, P(d_lwe)),
                "lut_add": lambda: ctx.lut_add_device(tg, 1, DEPTH, STEPS, P(d_sel), P(d_am), P(d_row), P(d_leaves), 1, None, P(d_out)),
            }
            # the C entry of the host replace write: Context.lut_write composes read and scatter and never reaches it
            L, I = ia.lib(), ia.evaluator._i32
            w_out = np.zeros_like(leaves)
            host["lut_write"] = lambda: ia.evaluator.check(L.ieache_lut_write(ctx.h, tg.h, 1, DEPTH, I(sel_d), I(row), I(leaves), I(w_out), None))
            for name in ("cmux", "lut_tree", "lut_scatter", "lut_write", "tlwe_rotate", "lut_read", "lut_add"):
                out["%-11s host form    wall us" % name] = 1e6 * wall(host[name], calls, 5)
                out["%-11s device form  wall us" % name] = 1e6 * wall(device[name], calls, 5)

        # ---- one product-size case per rate script ----
        def product(label, f):
            st = ia.Stats()
            ms, ws = [], []
            for i in range(4):
                t0 = time.perf_counter()
                f(st)
                ws.append(1e3 * (time.perf_counter() - t0))
                ms.append(st.total_ms)
            out[label + "  total_ms"], out[label + "  wall ms"] = float(np.median(ms[1:])), float(np.median(ws[1:]))

        rows, items, depth, steps = 16384, 1024, 4, 10
        d_set = dev(words(depth + steps, 2 * p.l, 2, N))
        d_rows, d_out = dev(words(rows, 2, N)), torch.zeros((rows, 2, N), dtype=torch.int32, device="cuda")
        d_mem, d_val = dev(words(items, 1 << depth, 2, N)), dev(words(items, 2, N))
        zeros = torch.zeros(rows, dtype=torch.int32, device="cuda")
        sel = dev(np.tile(np.arange(depth + steps, dtype=np.int32), (items, 1)))
        sel_depth = dev(np.tile(np.arange(depth, dtype=np.int32), (items, 1)))
        torch.cuda.synchronize()
        with ctx.tgsw_prepare_device(P(d_set), depth + steps) as tg:
            product("cmux_rates:    cmux_device, 16 384 rows, one shared selector",
                    lambda st: ctx.cmux_device(tg, rows, P(zeros), P(d_rows), P(d_rows), P(d_out), stats=st))
            product("scatter_rates: lut_scatter_device, 1 024 items x depth 4, in place",
                    lambda st: ctx.lut_scatter_device(tg, items, depth, P(sel_depth), P(d_val), P(d_mem), P(d_mem), stats=st))
            product("rotate_rates:  tlwe_rotate_device, 16 384 rows x 10 steps, in place",
                    lambda st: ctx.tlwe_rotate_device(tg, rows, steps, None, None, P(d_rows), P(d_rows), stats=st))
            product("gadget_rates:  lut_write_device, 1 024 items x depth 4, in place",
                    lambda st: ctx.lut_write_device(tg, items, depth, None, P(d_val), P(d_mem), P(d_mem), stats=st))
            product("lut_add_rates: lut_add_device, 1 024 items x depth 4 x 10 steps, one memory",
                    lambda st: ctx.lut_add_device(tg, items, depth, steps, P(sel), None, P(d_val), P(d_mem), 1, None, P(d_mem), stats=st))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*", help="name=path, the two selves of the one library first and the other library last")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=201)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_calls_refactor.txt"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.calls)
    libs = [s.split("=", 1) for s in a.libs]
    assert len(libs) == 3, "three name=path pairs"
    from ieache_amd import tools
    import ieache_amd as ia
    k = tools.keygen_raw(ia.default_params(), (1, 2, 3))
    found = {name: {} for name, _ in libs}
    with tempfile.TemporaryDirectory() as tmp:
        keys = os.path.join(tmp, "keys.npz")
        np.savez(keys, bk=k["bk"], ksk=k["ksk"])
        for r in range(a.rounds):
            for q in range(len(libs)):
                name, path = libs[(r + q) % len(libs)]
                env = dict(os.environ, IEACHE_LIBRARY=os.path.abspath(path))
                run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", keys, "--calls", str(a.calls)], env=env, timeout=240,
                                     stdout=subprocess.PIPE, text=True, check=True)
                got = json.loads([l for l in run.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
                for line, v in got.items():
                    found[name].setdefault(line, []).append(v)
                print("round %d %s done" % (r, name), flush=True)
    names = [n for n, _ in libs]
    lines = ["host time of the calls on a TGSW set, %s beside %s (one library under two names: %s, %s)" % (names[2], names[0], names[0], names[1]),
             "command: python scripts/set_calls_ab.py %s --rounds %d --calls %d" % (" ".join("%s=<%s>" % (n, os.path.basename(os.path.dirname(os.path.abspath(p))) + "/libieache.so") for n, p in libs), a.rounds, a.calls),
             "%d rounds, a fresh process per library and round, the order rotated; toy lines: count = %d, depth %d, steps %d, median of %d warm calls per "
             "process; every figure below: median [min .. max] over the rounds" % (a.rounds, COUNT, DEPTH, STEPS, a.calls), ""]
    outside = 0
    for line in found[names[0]]:
        span = found[names[0]][line] + found[names[1]][line]
        lo, hi = min(span), max(span)
        m = float(np.median(found[names[2]][line]))
        ok = lo <= m <= hi
        outside += not ok
        lines.append(line)
        for n in names:
            v = found[n][line]
            lines.append("    %-10s %10.3f [%.3f .. %.3f]" % (n, float(np.median(v)), min(v), max(v)))
        lines.append("    %s median %s the span of %s and %s, %.3f .. %.3f" % (names[2], "within" if ok else "OUTSIDE", names[0], names[1], lo, hi))
    lines.append("")
    lines.append("%d of %d lines outside" % (outside, len(found[names[0]])))
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 1 if outside else 0


if __name__ == "__main__":
    sys.exit(main())
