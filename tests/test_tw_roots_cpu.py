"""The resident form of the transform's second inter-pass twiddles (csrc/tw_roots.h, taken by k_blind_rotate_w1b) holds, for
every lane, exactly the table entries the table form reads: tests/native/tw_roots_test.cpp on the host."""
import os
import subprocess


def test_resident_twiddles_are_the_table_entries(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "tw_roots_test"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(root, "ie-ache_amd", "csrc"),
                           os.path.join(root, "tests", "native", "tw_roots_test.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 mismatches" in r.stdout
