"""Which key-switch kernel takes a launch, and cut how (csrc/ks_plan.h: free of HIP), against a table derived by hand, under
AddressSanitizer + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ks_plan_table_under_asan_ubsan(tmp_path):
    exe = tmp_path / "ks_plan_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "native", "ks_plan_test.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "KS_PLAN_OK" in r.stdout, r.stdout[-4000:]
