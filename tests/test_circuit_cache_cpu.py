"""CircuitCache (ie-ache_amd/csrc/circuit_cache.h), the one cache of built circuits behind a context and the daemon: LRU eviction
of level-capped variants, held circuits outliving their eviction, and the selection rule, as plain host C++ under
AddressSanitizer + UBSan (tests/native/circuit_cache_test.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_circuit_cache_under_asan_ubsan(tmp_path):
    exe = tmp_path / "circuit_cache_test"
    csrc = os.path.join(ROOT, "ie-ache_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "native", "circuit_cache_test.cpp"),
                           os.path.join(csrc, "circuit.cpp"), "-pthread", "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for args, marker in (([], "CIRCUIT_CACHE_OK"), (["asap"], "CIRCUIT_CACHE_ASAP_OK")):
        r = subprocess.run([str(exe)] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert r.returncode == 0 and marker in r.stdout.split(), r.stdout[-4000:]
