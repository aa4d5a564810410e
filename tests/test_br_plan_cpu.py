"""Which blind-rotation kernel takes a launch, sliced how, with how many gates per workgroup, and whether as a rotation of
roles (csrc/br_plan.h: free of HIP), against the table of what the evaluator and the launcher decided before the header
existed, under AddressSanitizer + UBSan; and the variant table's builds against the launch rows of blind_rotate_w64.hip."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ie-ache_amd", "csrc")


def _build(tmp_path):
    exe = tmp_path / "br_plan_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "native", "br_plan_test.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return exe, env


def test_br_plan_table_under_asan_ubsan(tmp_path):
    exe, env = _build(tmp_path)
    r = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and "BR_PLAN_OK" in r.stdout, r.stdout[-4000:]


def test_both_variant_tables_hold_the_same_builds(tmp_path):
    """kBrVariants (br_plan.h) against kLaunchRows (blind_rotate_w64.hip, whose static_assert says the same to the
    compiler): the same (number, gates per workgroup) pairs, each once."""
    exe, env = _build(tmp_path)
    out = subprocess.run([str(exe), "--builds"], env=env, stdout=subprocess.PIPE, text=True, timeout=60, check=True).stdout
    named = sorted(tuple(int(x) for x in line.split(":")) for line in out.split())
    with open(os.path.join(CSRC, "br_plan.h")) as f:
        consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr int32_t (kVariant\w+) = (\d+);", f.read())}
    with open(os.path.join(CSRC, "blind_rotate_w64.hip")) as f:
        text = f.read()
    table = text[text.index("kLaunchRows[] = {"):]
    table = table[:table.index("};")]
    launched = []
    for m in re.finditer(r"^\s*\{(\d+|kVariant\w+)(?: \+ (\d+))?, (\d+),", table, re.M):
        base = int(m.group(1)) if m.group(1).isdigit() else consts[m.group(1)]
        launched.append((base + int(m.group(2) or 0), int(m.group(3))))
    assert len(launched) == table.count("{") - 1 == 22  # every row of the table was read ("= {" is the one other brace)
    assert sorted(launched) == named and len(set(launched)) == len(launched)
