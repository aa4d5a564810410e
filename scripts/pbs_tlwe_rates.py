#!/usr/bin/env python3
"""What the TLWE-table form, the accumulator output and the key switch alone cost beside the calls they sit next to, on one
card in one run at the reference's parameters (n = 630):

  * Context.pbs of 1 024 / 4 096 rows from an ENCRYPTED four-entry table (tlwe=True) against the same rows from the plain
    table, by turns, on the default two streams and on one stream ("overlap" = 0);
  * the whole rotated accumulators as the result (accumulator=True) against the extracted samples (keyswitch=False);
  * Context.keyswitch_device of 8 192 rows against the key-switch share (ieache_stats.keyswitch_ms) the same build reports
    for a gate call of 8 192 gates.

Every figure is ieache_stats.total_ms, the GPU timeline (HIP events) of the whole call, of warm device-form calls on buffers made
once; the decode of the table forms' outputs (host calls) is checked before anything is timed.

    python scripts/pbs_tlwe_rates.py [--out profiles/pbs_tlwe_rates.txt] [--calls 7]

Median and range over --calls recorded calls after --warm unrecorded ones."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pbs_tlwe_rates.txt"))
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--ks-rows", type=int, default=8192)
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]

    import torch
    import ieache_amd as ia
    from ieache_amd import tools
    p = ia.default_params()
    k = tools.keygen_raw(p, (1, 2, 3))
    rng = np.random.default_rng(1)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    entries = 4
    perm = np.array([2, 0, 3, 1])
    table = tools.lut_test_poly(p, (perm << 29).astype(np.int32))  # message m at phase m / 8
    private = tools.tlwe_encrypt(p, k["tlwe_key"], table, 7)
    s = np.asarray(k["lwe_key"][: p.n], dtype=np.int64)

    def decode(rows):
        ph = (rows[..., p.n].astype(np.int64) - rows[..., : p.n].astype(np.int64) @ s) & 0xFFFFFFFF
        return np.rint(ph / 2.0 ** 32 * 2 * entries).astype(np.int64) % (2 * entries)

    def median_line(label, t, base, rows):
        m, lo, hi = float(np.median(t)), min(t), max(t)
        say("  %-34s %9.3f ms [%.3f .. %.3f]   %9.0f rows/s   %.4f of the call beside it" % (label, m, lo, hi, rows / (m * 1e-3), m / base))

    def by_turns(forms):
        rec = {label: [] for label, _ in forms}
        for i in range(a.warm + a.calls):
            r = i % len(forms)  # the order rotates from round to round, so that no form always follows the same one
            for label, f in forms[r:] + forms[:r]:
                ms = f()
                if i >= a.warm:
                    rec[label].append(ms)
        return rec

    with ia.Context.from_arrays(p, k["bk"], k["ksk"], device=a.device) as ctx:
        say("TLWE tables, accumulator output and the key switch alone beside the plain calls: n = %d, N = %d, %d CUs, %s"
            % (p.n, p.N, ctx.get_option("cus"), ctx.kernel_variant))
        say("ieache_stats.total_ms (HIP events around the whole call) of warm device-form calls (%d unrecorded, then %d recorded, the forms by turns in rotating order): "
            "median [min .. max]" % (a.warm, a.calls))
        say()
        for count, overlap in [(c, o) for c in sizes for o in (1, 0)]:
            # "overlap" = 0: every launch on one stream -- the mode per-kernel comparisons are taken in; with the default two
            # streams a wide call runs as level halves side by side, and how the halves share the chip moves from form to form
            ctx.set_option("overlap", overlap)
            msgs = rng.integers(0, entries, size=count)
            x = tools.encrypt_bits(p, k["lwe_key"], np.ones(count, dtype=np.uint8), 463)  # 1/8, moved to the phases m / 8
            b = x[:, p.n].astype(np.int64) - (1 << 29) + (msgs.astype(np.int64) << 29)
            x[:, p.n] = (b & 0xFFFFFFFF).astype(np.uint32).view(np.int32)

            # device forms on buffers made once: nothing is copied between the timed calls, so every form finds the chip in
            # the state the previous call left it in (after the 32 MB download of a host call with accumulator output the next
            # call starts on a chip that has idled, and measures about 1 ms longer at 4 096 rows whatever its form)
            dev = "cuda:%d" % a.device
            d_x = torch.zeros((count, ctx.lwe_stride), dtype=torch.int32, device=dev)
            d_x[:, : p.n + 1] = torch.from_numpy(x).to(dev)
            d_tv = {False: torch.from_numpy(table).to(dev), True: torch.from_numpy(private).to(dev)}
            d_out = torch.zeros((count, 2 * p.N), dtype=torch.int32, device=dev)  # the longest rows of the five forms
            torch.cuda.synchronize()

            def call(**kw):
                def f():
                    st = ia.Stats()
                    ctx.pbs_device(count, d_x.data_ptr(), d_tv[bool(kw.get("tlwe"))].data_ptr(), 1, None, d_out.data_ptr(), stats=st, **kw)
                    assert st.bootstraps == count
                    return st.total_ms
                return f

            wrong = [int(np.sum(decode(ctx.pbs(x, tv, tlwe=t)) != perm[msgs])) for tv, t in ((table, False), (private, True))]
            say("%d rows, %s (kernel of a launch of %d rows: %s); wrong decodes: plain table %d, TLWE table %d"
                % (count, "two streams (default)" if overlap else "one stream (overlap = 0)", count, ctx.kernel_for_launch(count), wrong[0], wrong[1]))
            rec = by_turns([("plain table", call()), ("TLWE table", call(tlwe=True)),
                            ("extracted samples (no key switch)", call(keyswitch=False)), ("whole accumulators", call(accumulator=True)),
                            ("whole accumulators, TLWE table", call(tlwe=True, accumulator=True))])
            base = float(np.median(rec["plain table"]))
            median_line("plain table", rec["plain table"], base, count)
            median_line("TLWE table", rec["TLWE table"], base, count)
            base = float(np.median(rec["extracted samples (no key switch)"]))
            for label in ("extracted samples (no key switch)", "whole accumulators", "whole accumulators, TLWE table"):
                median_line(label, rec[label], base, count)
            say()

        ctx.set_option("overlap", 1)
        rows = a.ks_rows
        bits = rng.integers(0, 2, size=(2, rows)).astype(np.uint8)
        ga, gb = (tools.encrypt_bits(p, k["lwe_key"], bits[i], 470 + i) for i in range(2))
        d_u = torch.zeros((rows, ctx.extract_stride), dtype=torch.int32, device="cuda:%d" % a.device)
        d_u[:, : p.N + 1] = torch.from_numpy(rng.integers(-(1 << 31), 1 << 31, size=(rows, p.N + 1), dtype=np.int64).astype(np.int32)).to(d_u.device)
        d_out = torch.zeros((rows, ctx.lwe_stride), dtype=torch.int32, device=d_u.device)
        torch.cuda.synchronize()

        def gate_call():
            st = ia.Stats()
            ctx.gates(ia.GATE_AND, ga, gb, stats=st)
            return (st.total_ms, st.keyswitch_ms, st.keyswitch_launches)

        def ks_call():
            st = ia.Stats()
            ctx.keyswitch_device(rows, d_u.data_ptr(), d_out.data_ptr(), stats=st)
            assert st.bootstraps == 0
            return (st.total_ms, st.keyswitch_ms, st.keyswitch_launches)

        rec = by_turns([("gates", gate_call), ("keyswitch", ks_call)])
        g_tot, g_ks = (float(np.median([r[i] for r in rec["gates"]])) for i in (0, 1))
        k_tot, k_ks = (float(np.median([r[i] for r in rec["keyswitch"]])) for i in (0, 1))
        say("the key switch of %d rows" % rows)
        say("  gate call of %d AND gates:        total %9.3f ms, of which key switch (keyswitch_ms, %d launches, each stream's own time) %9.3f ms"
            % (rows, g_tot, rec["gates"][-1][2], g_ks))
        say("  Context.keyswitch_device:           total %9.3f ms [%.3f .. %.3f], key-switch launches (%d) %9.3f ms   %9.0f rows/s   %.3f of the gate call's share"
            % (k_tot, min(r[0] for r in rec["keyswitch"]), max(r[0] for r in rec["keyswitch"]), rec["keyswitch"][-1][2], k_ks, rows / (k_tot * 1e-3),
               k_tot / g_ks if g_ks > 0 else float("nan")))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
