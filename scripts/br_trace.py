"""The launches a fixed set of calls makes, for comparing two builds of the library (development aid: the check behind a
host-side refactoring of the blind rotation).
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/br_trace.py run     (a run of its own, no counters)
  python scripts/br_trace.py summary DIR/.../*_kernel_trace.csv > summary.txt
`run`: flat gates of 200, 400, 900, 1 100, 1 400, 2 300 and 4 096 instances at the product parameters, by launch size and with
exact_fft = 1; a MUX call; a call with the audit on every launch; a call after fft_guard_inject; a debug blind rotation of
three steps; add16 x 4 096 and a MUX-bearing netlist.  pipe_auto = 0 (its trials choose a stream mode by host wall time:
two runs of the same code would differ) and fixed seeds.
`summary`: per stream in order of first use, the list of (kernel, grid, workgroup, LDS bytes) with repeats folded, and a
digest of the unfolded list: two builds that make the same launches in the same order give the same text."""
import csv
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = (200, 400, 900, 1100, 1400, 2300, 4096)


def run():
    import numpy as np
    import ieache_amd as ia
    from ieache_amd import tools

    p = ia.default_params()
    k = tools.keygen_raw(p, (1, 2, 3))
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2, size=(3, 4096)).astype(np.uint8)
    a, b, c = (tools.encrypt_bits(p, k["lwe_key"], bits[i], 20 + i) for i in range(3))
    h = hashlib.sha256()
    with ia.Context.from_arrays(p, k["bk"], k["ksk"], device=0) as ctx:
        assert ctx.set_option_ok("pipe_auto", 0)
        for exact in (0, 1):
            ctx.set_option("exact_fft", exact)
            for n in SIZES:
                print("gates", n, "exact_fft", exact, ctx.kernel_for_launch(n), flush=True)
                h.update(ctx.gates(ia.GATE_XOR, a[:n], b[:n]).tobytes())
        ctx.set_option("exact_fft", 0)
        h.update(ctx.mux(a[:700], b[:700], c[:700]).tobytes())
        ctx.set_option("fft_audit", 1)
        h.update(ctx.gates(ia.GATE_AND, a[:1400], b[:1400]).tobytes())
        ctx.set_option("fft_audit", 64)
        ctx.set_option("fft_guard_inject", 1)
        h.update(ctx.gates(ia.GATE_AND, a[:900], b[:900]).tobytes())
        h.update(ctx.debug_blind_rotate(a[:300], 3).tobytes())
        info = ia.circuit_info(ia.CIRC_ADD, 16)
        inp = tools.encrypt_bits(p, k["lwe_key"], rng.integers(0, 2, size=(4096, info.n_inputs)).astype(np.uint8), 30)
        h.update(ctx.eval_batch(ia.CIRC_ADD, 16, inp).tobytes())
        nl = ia.Netlist(3)
        x, y, z = nl.input(0), nl.input(1), nl.input(2)
        t = nl.XNOR(x, ia.NOT(y))
        m = nl.MUX(t, y, ia.NOT(z))
        cn = nl.compile([t, m, nl.ORYN(m, x), nl.NOR(ia.TRUE, m)])
        h.update(ctx.eval_netlist(cn, np.stack([a[:600], b[:600], c[:600]], axis=1)).tobytes())
        print("audits", ctx.fft_audit(), "guard", ctx.fft_guard(), "mixed_launches", ctx.get_option("mixed_launches"),
              "overlapped_levels", ctx.get_option("overlapped_levels"), "pipelined_evals", ctx.get_option("pipelined_evals"))
    print("outputs sha256", h.hexdigest())


def summary(path):
    streams, order = {}, []
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r["Start_Timestamp"]))
    for r in rows:
        s = r.get("Stream_Id") or r.get("Queue_Id")
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").replace("ieache::", "")
        rec = (name, "x".join(r["Grid_Size_" + d] if "Grid_Size_" + d in r else r["Grid_Size"] for d in "XYZ"),
               "x".join(r["Workgroup_Size_" + d] if "Workgroup_Size_" + d in r else r["Workgroup_Size"] for d in "XYZ"), r["LDS_Block_Size"])
        if s not in streams:
            streams[s] = []
            order.append(s)
        streams[s].append(rec)
    print("%d kernel launches on %d streams" % (len(rows), len(order)))
    for i, s in enumerate(order):
        recs = streams[s]
        print("stream %d: %d launches, sha256 %s" % (i, len(recs), hashlib.sha256(repr(recs).encode()).hexdigest()[:16]))
        j = 0
        while j < len(recs):
            e = j
            while e < len(recs) and recs[e] == recs[j]:
                e += 1
            print("  %5d x %s grid %s wg %s lds %s" % ((e - j,) + recs[j]))
            j = e


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "summary":
        summary(sys.argv[2])
    elif len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    else:
        sys.exit(__doc__)
