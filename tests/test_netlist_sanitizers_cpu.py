"""The item arithmetic of MUX-bearing circuit levels and the netlist constructor under AddressSanitizer + UBSan (host code:
GPU sanitizers are not available on the pool)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_level_item_arithmetic_and_netlist_validation_under_asan_ubsan(tmp_path):
    exe = tmp_path / "level_items_test"
    csrc = os.path.join(ROOT, "ie-ache_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "native", "level_items_test.cpp"),
                           os.path.join(csrc, "circuit.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "LEVEL_ITEMS_OK" in r.stdout, r.stdout[-4000:]
