"""The wire store under circuits that hold MAJ3 / XOR3 gates: slot allocation with the third operand counted as a read, on
thousands of random DAGs and on add16_fa / mul32_fa, every schedule, executed piece by piece forwards and backwards, under
AddressSanitizer + UBSan (tests/native/gate3_store_test.cpp)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 3 000 random DAGs and the recorded add16_fa (plain, folded), each as ASAP levels and under five level caps of the balanced
# schedule; ADD / SUB / RSUB_FA at 16 bits and mul32_fa under five level widths as build_circuit gives them, plain and folded
CIRCUITS = (3000 + 2) * 6 + 2 * (3 + 5)


def test_piecewise_execution_with_three_input_gates_under_asan_ubsan(tmp_path):
    exe = tmp_path / "gate3_store_test"
    csrc = os.path.join(ROOT, "ie-ache_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "native", "gate3_store_test.cpp"),
                           os.path.join(csrc, "circuit.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("IEACHE_SCHEDULE", None)
    r = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    m = re.search(r"^GATE3_STORE_OK circuits=(\d+) gate3=(\d+)$", r.stdout, re.M)
    assert m and int(m.group(1)) == CIRCUITS and int(m.group(2)) > 100000, r.stdout[-4000:]
    print(m.group(0))
