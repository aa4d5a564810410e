#!/usr/bin/env python3
"""One multi-output programmable bootstrap beside the single-output calls that give the same outputs, on one card in one run:

  * Context.pbs_multi of 1 024 / 4 096 rows with 2 and with 4 factors (thermometer and parity tables of 2-bit messages, the
    constant polynomial 1/8, bias -1/8) against 2 and 4 Context.pbs calls of the same rows, one table each, by turns;
    output rows/s from ieache_stats.total_ms, the GPU timeline (HIP events) of a warm call;
  * the share of the multi call spent in the blind rotation, in the key switch, and in what is left -- k_mv_compact,
    k_mv_extract and, every "fft_audit"-th launch, the audit (total - blind_rotate_ms - keyswitch_ms);
  * the decode of both forms' outputs, checked before anything is timed.

    python scripts/pbs_multi_rates.py [--out profiles/pbs_multi_rates.txt] [--calls 5]

Median and range over --calls recorded calls after --warm unrecorded ones."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TABLES = np.array([[0, 1, 1, 1], [0, 1, 0, 1], [0, 0, 1, 1], [0, 0, 0, 1]])  # m >= 1, parity, m >= 2, m >= 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pbs_multi_rates.txt"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--sizes", default="1024,4096")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]

    import ieache_amd as ia
    from ieache_amd import tools
    p = ia.default_params()
    k = tools.keygen_raw(p, (1, 2, 3))
    rng = np.random.default_rng(1)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    mu = 1 << 29
    const = np.full(p.N, mu, dtype=np.int32)
    factors = np.stack([tools.lut_factor_poly(p, w) for w in TABLES])
    polys = np.stack([tools.lut_test_poly(p, np.where(w != 0, mu, -mu)) for w in TABLES])  # the same tables for Context.pbs
    s = np.asarray(k["lwe_key"][: p.n], dtype=np.int64)

    def bits(rows):
        ph = (rows[..., p.n].astype(np.int64) - rows[..., : p.n].astype(np.int64) @ s) & 0xFFFFFFFF
        return ((ph > 0) & (ph < (1 << 31))).astype(np.int64)

    with ia.Context.from_arrays(p, k["bk"], k["ksk"], device=a.device) as ctx:
        say("one multi-output programmable bootstrap against single-output calls: n = %d, N = %d, %d CUs, %s"
            % (p.n, p.N, ctx.get_option("cus"), ctx.kernel_variant))
        say("from ieache_stats of warm host calls (%d unrecorded, then %d recorded, the two forms by turns): median [min .. max]" % (a.warm, a.calls))
        say("rest = total - rotation - key switch: k_mv_compact, k_mv_extract and, when one falls due, the audit; negative where a call's two")
        say("streams ran rotation and key switch side by side (level halves on two lanes: each share is then a stream's own time)")
        say()
        for count in sizes:
            # fresh encryptions of 1/8 moved to the message phases m / 8
            msgs = rng.integers(0, 4, size=count)
            x = tools.encrypt_bits(p, k["lwe_key"], np.ones(count, dtype=np.uint8), 463)
            b = x[:, p.n].astype(np.int64) - mu + (msgs.astype(np.int64) << 29)
            x[:, p.n] = (b & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
            for nf in (2, 4):
                bias = np.full(nf, -mu, dtype=np.int32)
                want = TABLES[:nf, msgs].T

                def multi():
                    st = ia.Stats()
                    out = ctx.pbs_multi(x, const, factors[:nf], bias=bias, stats=st)
                    assert st.bootstraps == count
                    return out, (st.total_ms, st.blind_rotate_ms, st.keyswitch_ms, st.blind_rotate_launches, st.keyswitch_launches)

                def singles():  # the only way without the multi-output call: one rotation per table
                    outs, tot = [], np.zeros(5)
                    for t in range(nf):
                        st = ia.Stats()
                        outs.append(ctx.pbs(x, polys[t], stats=st))
                        assert st.bootstraps == count
                        tot += (st.total_ms, st.blind_rotate_ms, st.keyswitch_ms, st.blind_rotate_launches, st.keyswitch_launches)
                    return np.stack(outs, axis=1), tuple(tot)

                wrong = [int(np.sum(bits(f()[0]) != want)) for f in (multi, singles)]
                rec = {"multi": [], "singles": []}
                for i in range(a.warm + a.calls):
                    for label, f in (("multi", multi), ("singles", singles)):
                        r = f()[1]
                        if i >= a.warm:
                            rec[label].append(r)
                say("%d rows x %d tables = %d output rows (kernel of a launch of %d rows: %s); wrong decodes: multi %d, singles %d"
                    % (count, nf, count * nf, count, ctx.kernel_for_launch(count), wrong[0], wrong[1]))
                base = float(np.median([r[0] for r in rec["singles"]]))
                for label in ("multi", "singles"):
                    t = [r[0] for r in rec[label]]
                    m, lo, hi = float(np.median(t)), min(t), max(t)
                    br, ks = float(np.median([r[1] for r in rec[label]])), float(np.median([r[2] for r in rec[label]]))
                    say("  %-8s %9.3f ms [%.3f .. %.3f]   %9.0f output rows/s [%.0f .. %.0f]   %.3f of the singles' time   rotation %.1f %%, key switch %.1f %%, "
                        "rest (extraction stage, audit) %.1f %%   (%d blind-rotation, %d key-switch launches)"
                        % (label, m, lo, hi, count * nf / (m * 1e-3), count * nf / (hi * 1e-3), count * nf / (lo * 1e-3), m / base,
                           100 * br / m, 100 * ks / m, 100 * (m - br - ks) / m, rec[label][-1][3], rec[label][-1][4]))
                say()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
