"""finalize_circuit's slot allocation, level layout and schedules on thousands of random DAGs and on the reference's own adder
and multiplier, executed piece by piece on symbolic values, under AddressSanitizer + UBSan (tests/native/circuit_store_test.cpp).
This is the test that holds the wire store's invariant: a level's output slots are disjoint from every slot the level reads."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 4 000 random DAGs and 4 reference DAGs, each as ASAP levels and under five level caps of the balanced schedule
CIRCUITS = (4000 + 4) * 6


def test_piecewise_execution_of_the_slot_table_under_asan_ubsan(tmp_path):
    exe = tmp_path / "circuit_store_test"
    csrc = os.path.join(ROOT, "ie-ache_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "native", "circuit_store_test.cpp"),
                           os.path.join(csrc, "circuit.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    m = re.search(r"^CIRCUIT_STORE_OK circuits=(\d+)$", r.stdout, re.M)
    assert m and int(m.group(1)) == CIRCUITS, r.stdout[-4000:]
    print(m.group(0))
