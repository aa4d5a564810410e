"""The evaluator's option table and scoped-assignment guard under AddressSanitizer + UBSan (host code: the table is free of
HIP, and Evaluator::set_option / get_option / the environment pass are loops over it)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_table_and_scoped_set_under_asan_ubsan(tmp_path):
    exe = tmp_path / "evaluator_options_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "native", "evaluator_options_test.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "EVALUATOR_OPTIONS_OK" in r.stdout, r.stdout[-4000:]
