"""The runner that cuts a device group's call -- and the daemon's round -- into slices on host threads (csrc/group_run.h:
free of HIP), as a stand-alone program under AddressSanitizer + UBSan and, built a second time, under ThreadSanitizer; and
its slices against ieache_shard_slice."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "group_run_test.cpp")

BUILDS = {
    "asan_ubsan": (["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                   {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"}),
    "tsan": (["-fsanitize=thread"], {"TSAN_OPTIONS": "halt_on_error=1"}),
}


def _build(tmp_path, which):
    flags, env = BUILDS[which]
    exe = tmp_path / ("group_run_test_" + which)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fno-omit-frame-pointer"] + flags + [SRC, "-o", str(exe)])
    return exe, dict(os.environ, **env)


@pytest.mark.parametrize("which", sorted(BUILDS))
def test_run_sliced_under_sanitizers(tmp_path, which):
    exe, env = _build(tmp_path, which)
    r = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "GROUP_RUN_OK" in r.stdout, r.stdout[-4000:]


def test_its_slices_are_ieache_shard_slice(tmp_path, ia):
    exe, env = _build(tmp_path, "asan_ubsan")
    out = subprocess.run([str(exe), "--slices"], env=env, stdout=subprocess.PIPE, text=True, timeout=60, check=True).stdout
    L = ia.lib()
    first, count = C.c_size_t(0), C.c_size_t(0)
    lines = out.split("\n")[:-1]
    assert len(lines) == 41 * sum(range(1, 10))
    for line in lines:
        total, parts, part, want_first, want_count = (int(x) for x in line.split())
        assert L.ieache_shard_slice(total, parts, part, C.byref(first), C.byref(count)) == 0
        assert (first.value, count.value) == (want_first, want_count), line
