"""What a call on a caller TGSW set is (csrc/set_calls.h: the scalars and their refusal, the arguments as plain data) without a
GPU, under AddressSanitizer + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_set_calls_under_asan_ubsan(tmp_path):
    """tests/native/set_calls_test.cpp: a stand-alone program over csrc/set_calls.h -- for each of the eight calls (the seven of
    sections 3f to 3j, and lut_write_coef of section 3l with its width, unit and window mark) every scalar rule with its exact
    message and the first-failing order, the words of every argument (2^20 items at depth 12 among them), and which arguments are
    optional, which may be the output, and every bound."""
    exe = tmp_path / "set_calls_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "native", "set_calls_test.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "SET_CALLS_OK" in r.stdout, r.stdout[-4000:]
