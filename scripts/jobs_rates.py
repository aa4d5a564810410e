#!/usr/bin/env python3
"""Several circuits' batches evaluated together, level by level (ieache_eval_jobs), against the same jobs evaluated one after
another (ieache_eval_batch), at the product parameters (n = 630):

  * {ADD, SUB, MUL} 32-bit x 8 each; {MUL32 x 8, MUL64 x 4, MULADD64 x 4}; {ADD32 x 64, MUL32 x 8}; and a wide set,
    {MUL32 x 64, ADD32 x 64}, where joining should NOT pay;
  * the whole call timed by the evaluator's own GPU event timers (ieache_stats.total_ms; the sequential leg is the sum over its
    calls), warm, the two ways taken by turns; median and range of --calls recorded turns;
  * every joint output compared word for word with the sequential one before anything is timed.

    python scripts/jobs_rates.py [--out profiles/jobs_rates.txt] [--calls 7]
    python scripts/jobs_rates.py --sequential-only --library /path/to/another/libieache.so [--out ...]

--sequential-only needs none of the joint symbols, so it runs against ANOTHER build of the library -- the parent commit's: the
baseline -- loaded beside this one (keys and ciphertexts still come from this build's host tools, which the evaluation does
not touch).  The same leg on this build stands beside it in the full run, to show that single calls did not move.
The file is the record: DESIGN, README and the daemon's rule (csrc/joint_plan.h) quote it, nothing else states a rate."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CIRC_ADD, CIRC_SUB, CIRC_MUL, CIRC_MULADD = 1, 2, 4, 5
SETS = [
    ("three operators, narrow", [("add32", CIRC_ADD, 32, 8), ("sub32", CIRC_SUB, 32, 8), ("mul32", CIRC_MUL, 32, 8)]),
    ("three multipliers", [("mul32", CIRC_MUL, 32, 8), ("mul64", CIRC_MUL, 64, 4), ("muladd64", CIRC_MULADD, 64, 4)]),
    ("many additions beside a few multiplications", [("add32", CIRC_ADD, 32, 64), ("mul32", CIRC_MUL, 32, 8)]),
    ("wide on their own (joining should not pay)", [("mul32", CIRC_MUL, 32, 64), ("add32", CIRC_ADD, 32, 64)]),
]


class OtherBuild:
    """ieache_eval_batch of another build of the library through a binding of its own: only symbols every build has"""

    def __init__(self, path, ia, p, bk, ksk):
        self.ia, self.L = ia, C.CDLL(path)
        L = self.L
        i32p = C.POINTER(C.c_int32)
        L.ieache_ctx_create_raw.restype = C.c_void_p
        L.ieache_ctx_create_raw.argtypes = [C.c_void_p, i32p, i32p, C.c_int]
        L.ieache_ctx_destroy.argtypes = [C.c_void_p]
        L.ieache_prepare_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_size_t]
        L.ieache_eval_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_size_t, i32p, i32p, C.c_void_p]
        L.ieache_last_error.restype = C.c_char_p
        L.ieache_version.restype = C.c_char_p
        self.p = p
        self.h = L.ieache_ctx_create_raw(C.byref(p), bk.ctypes.data_as(i32p), ksk.ctypes.data_as(i32p), 0)
        if not self.h:
            raise RuntimeError(L.ieache_last_error().decode())

    def prepare(self, kind, bits, batch):
        assert self.L.ieache_prepare_batch(self.h, kind, bits, batch) == 0, self.L.ieache_last_error()

    def eval_batch(self, kind, bits, in_lwe, stats):
        info = self.ia.circuit_info(kind, bits)
        out = np.zeros((in_lwe.shape[0], info.n_outputs, self.p.n + 1), dtype=np.int32)
        i32p = C.POINTER(C.c_int32)
        rc = self.L.ieache_eval_batch(self.h, kind, bits, in_lwe.shape[0], in_lwe.ctypes.data_as(i32p), out.ctypes.data_as(i32p), C.byref(stats))
        assert rc == 0, self.L.ieache_last_error()
        return out

    def close(self):
        self.L.ieache_ctx_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--sets", default="0,1,2,3", help="which of the job sets, by index")
    ap.add_argument("--sequential-only", action="store_true")
    ap.add_argument("--library", default=None, help="--sequential-only: the build to evaluate with (default: this one)")
    a = ap.parse_args()
    assert a.calls >= 7, "the median of at least 7 turns"
    assert not a.library or a.sequential_only, "--library goes with --sequential-only"
    out_path = a.out or os.path.join(ROOT, "profiles", "jobs_rates_sequential.txt" if a.sequential_only else "jobs_rates.txt")

    import ieache_amd as ia
    from ieache_amd import tools
    p = ia.default_params()
    k = tools.keygen_raw(p, (1, 2, 3))
    bk, ksk = np.ascontiguousarray(k["bk"], dtype=np.int32), np.ascontiguousarray(k["ksk"], dtype=np.int32)
    rng = np.random.default_rng(1)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def inputs(kind, bits, batch, seed):
        info = ia.circuit_info(kind, bits)
        inb = np.zeros((batch, info.n_inputs), dtype=np.uint8)
        inb[:, :2 * bits] = rng.integers(0, 2, size=(batch, 2 * bits))
        return tools.encrypt_bits(p, k["lwe_key"], inb, seed), info

    ctx = OtherBuild(a.library, ia, p, bk, ksk) if a.library else ia.Context.from_arrays(p, bk, ksk, device=0)
    try:
        if a.sequential_only:
            say("the jobs of each set one after another through ieache_eval_batch: n = %d, N = %d; library: %s"
                % (p.n, p.N, os.path.basename(a.library) + " (" + ctx.L.ieache_version().decode() + ")" if a.library else "this build"))
        else:
            say("several circuits' batches together (ieache_eval_jobs) against one after another (ieache_eval_batch): n = %d, N = %d, %d CUs, %s"
                % (p.n, p.N, ctx.get_option("cus"), ctx.kernel_variant))
        say("GPU time of the whole call (ieache_stats.total_ms; sequential: the sum over its calls), warm: %d unrecorded turns, then %d "
            "recorded, the ways by turns; median [min .. max]" % (a.warm, a.calls))
        say()
        for si in (int(x) for x in a.sets.split(",")):
            title, members = SETS[si]
            jobs, gates = [], 0
            for j, (name, kind, bits, batch) in enumerate(members):
                inp, info = inputs(kind, bits, batch, 600 + 10 * si + j)
                jobs.append((kind, bits, inp))
                gates += batch * info.bootstraps
                ctx.prepare(kind, bits, batch)

            def sequential():
                outs, ms = [], 0.0
                for kind, bits, inp in jobs:
                    st = ia.Stats()
                    outs.append(ctx.eval_batch(kind, bits, inp, st))
                    ms += st.total_ms
                return outs, ms

            def joint():
                st = ia.Stats()
                outs = ctx.eval_jobs(jobs, st)
                return outs, st.total_ms, st

            ways = [("one after another", sequential)]
            want, _ = sequential()
            shape = ""
            if not a.sequential_only:
                ctx.prepare_jobs([(kind, bits, len(inp)) for kind, bits, inp in jobs])
                got, _, st = joint()
                assert all(np.array_equal(g, w) for g, w in zip(got, want)), title
                shape = "; joint call: %d levels, %d pieces, %d rotation launches" % (st.levels, st.chunks, st.blind_rotate_launches)
                ways.append(("together", lambda: joint()[:2]))
            ms = {label: [] for label, _ in ways}
            for i in range(a.warm + a.calls):
                for label, f in ways:
                    t = f()[1]
                    if i >= a.warm:
                        ms[label].append(t)
            say("set %d, %s: %s -- %d gates%s" % (si, title, " + ".join("%s x %d" % (m[0], m[3]) for m in members), gates, shape))
            base = float(np.median(ms["one after another"]))
            for label, _ in ways:
                m, lo, hi = float(np.median(ms[label])), min(ms[label]), max(ms[label])
                say("  %-20s %9.1f ms [%.1f .. %.1f]   %8.0f gates/s [%.0f .. %.0f]   %.3f of the sequential time"
                    % (label, m, lo, hi, gates / m * 1e3, gates / hi * 1e3, gates / lo * 1e3, m / base))
            say()
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
