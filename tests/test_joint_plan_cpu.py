"""The arithmetic of a joint evaluation (csrc/joint_plan.h: step -> parts, joint item -> part, the piece cut with the
gate-boundary rule inside a part, the scratch of the widest step, the daemon's rule) as a stand-alone program under
AddressSanitizer + UBSan: thousands of random job lists, with and without MUX levels, odd chunk values and parts of one item."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "joint_plan_test.cpp")
FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"}


def build(tmp_path):
    exe = tmp_path / "joint_plan_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fno-omit-frame-pointer"] + FLAGS + [SRC, "-o", str(exe)])
    return exe, dict(os.environ, **ENV)


def test_joint_plan_under_sanitizers(tmp_path):
    exe, env = build(tmp_path)
    r = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    m = re.search(r"JOINT_PLAN_OK (\d+) job lists", r.stdout)
    assert m and int(m.group(1)) >= 5000, r.stdout[-4000:]


def test_the_header_is_free_of_hip():
    """joint_plan.h compiles with a plain host compiler (the test above has just done that) and includes nothing of the device."""
    with open(os.path.join(ROOT, "ie-ache_amd", "csrc", "joint_plan.h")) as f:
        text = f.read()
    assert "hip/" not in text and "__global__" not in text
    assert set(re.findall(r'#include [<"]([^>"]+)[>"]', text)) == {"algorithm", "cstddef", "cstdint", "level_items.h"}
