"""Every Circuit the built-in kinds and build_netlist can produce, every refusal and the whole circuit_level_cap table, as
64-bit digests (tests/native/circuit_digest.cpp: one line per (kind, width) over its 24 configurations of folding, balancing
and level cap; `circuit_digest -v` lists them singly) against tests/golden/circuit_digests.txt -- the program's output at commit
d888306, before the circuit code was restructured into a kind table, named schedule steps and one cache.  The golden file is
the definition of "unchanged" for circuit.cpp: it is never regenerated from newer code."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_circuit_and_level_cap_matches_the_recorded_digests(tmp_path):
    exe = tmp_path / "circuit_digest"
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "native", "circuit_digest.cpp"),
                           os.path.join(ROOT, "ie-ache_amd", "csrc", "circuit.cpp"), "-o", str(exe)])
    env = {k: v for k, v in os.environ.items() if k != "IEACHE_SCHEDULE"}
    r = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    got = r.stdout.splitlines()
    with open(os.path.join(ROOT, "tests", "golden", "circuit_digests.txt")) as f:
        want = f.read().splitlines()
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            print("first differing line, %d:\n  golden: %s\n  now:    %s" % (i + 1, w, g))
            break
    assert got == want, "%d lines against the golden file's %d" % (len(got), len(want))
    assert r.returncode == 0, r.stdout[-2000:]
    print("CIRCUIT_DIGEST_OK lines=%d" % len(got))
