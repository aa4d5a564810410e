"""scripts/isa_same.py: the classifier behind "this refactoring left the kernels' code alone", pinned on hand-written
assembly (no compiler involved): identical streams, exchanged sources of a commutative instruction, and real differences
(an extra instruction, exchanged sources of a subtraction, another register count, a kernel only one side has)."""
import importlib.util
import io
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "scripts", "isa_same.py")
spec = importlib.util.spec_from_file_location("isa_same", SCRIPT)
isa_same = importlib.util.module_from_spec(spec)
spec.loader.exec_module(isa_same)


def kernel(name, body, vgpr=12, ordinal=0, lds=0):
    return """\t.globl\t%(n)s ; -- Begin function %(n)s
\t.p2align\t8
\t.type\t%(n)s,@function
%(n)s: ; @%(n)s
; %%bb.0:
%(b)s
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel %(n)s
\t\t.amdhsa_group_segment_fixed_size %(l)d
\t\t.amdhsa_private_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr %(v)d
\t\t.amdhsa_next_free_sgpr 8
\t\t.amdhsa_accum_offset 12
\t.end_amdhsa_kernel
\t.text
.Lfunc_end%(o)d:
\t.size\t%(n)s, .Lfunc_end%(o)d-%(n)s
""" % dict(n=name, b=body, v=vgpr, o=ordinal, l=lds)


BODY = """\ts_load_dwordx2 s[2:3], s[0:1], 0x0 ; a comment
\tv_mul_f64 v[2:3], v[4:5], v[6:7]
.LBB%d_1: ; =>This Inner Loop Header: Depth=1
\tv_fma_f64 v[8:9], v[2:3], v[4:5], v[8:9]
\tv_sub_u32_e32 v1, v0, v10
\ts_cbranch_scc1 .LBB%d_1"""


def run(old, new):
    out = io.StringIO()
    rc = isa_same.compare(old, new, out)
    return rc, out.getvalue()


def test_identical_kernels_whatever_the_comments_directives_and_function_ordinals():
    old = kernel("_Z1aPd", BODY % (0, 0)) + kernel("_Z1bPd", BODY % (1, 1), ordinal=1)
    new = kernel("_Z1bPd", (BODY % (0, 0)).replace("; a comment", "; another"), ordinal=0) + "\t.p2align 4\n" + kernel("_Z1aPd", BODY % (1, 1), ordinal=1)
    rc, text = run(old, new)
    assert rc == 0
    assert [l.split()[0] for l in text.splitlines()[1:3]] == ["identical", "identical"] and "2 kernels: 2 identical, 0 identical up to" in text
    assert "6/6" in text and "12/12" in text  # instruction count (the label is none) and VGPRs of both sides


def test_exchanged_sources_of_a_commutative_instruction_are_their_own_class():
    old = kernel("_Z1aPd", BODY % (0, 0))
    new = kernel("_Z1aPd", (BODY % (0, 0)).replace("v_mul_f64 v[2:3], v[4:5], v[6:7]", "v_mul_f64 v[2:3], v[6:7], v[4:5]"))
    rc, text = run(old, new)
    assert rc == 0
    assert text.splitlines()[1].startswith("swapped") and "(1 exchanged)" in text
    assert "1 kernels: 0 identical, 1 identical up to exchanged sources of a commutative instruction, 0 different" in text
    # the first two sources of a fused multiply-add commute as well; its addend does not
    fma = kernel("_Z1aPd", (BODY % (0, 0)).replace("v_fma_f64 v[8:9], v[2:3], v[4:5], v[8:9]", "v_fma_f64 v[8:9], v[4:5], v[2:3], v[8:9]"))
    assert run(old, fma)[0] == 0 and "swapped" in run(old, fma)[1]
    bad = kernel("_Z1aPd", (BODY % (0, 0)).replace("v_fma_f64 v[8:9], v[2:3], v[4:5], v[8:9]", "v_fma_f64 v[8:9], v[2:3], v[8:9], v[4:5]"))
    assert run(old, bad)[0] == 1 and "DIFFERENT" in run(old, bad)[1]


ADD3 = "\tv_add3_u32 v8, v8, v18, v14\n"


def test_the_three_sources_of_an_integer_add_commute():
    old = kernel("_Z1aPd", ADD3 + BODY % (0, 0))
    rc, text = run(old, kernel("_Z1aPd", ADD3.replace("v8, v18, v14", "v14, v18, v8") + BODY % (0, 0)))
    assert rc == 0 and text.splitlines()[1].startswith("swapped") and "(1 exchanged)" in text
    # the same destination and the same multiset of sources, nothing less: another source is another sum
    for other in ("v14, v18, v9", "v8, v8, v18", "v18, v14, v14"):
        rc, text = run(old, kernel("_Z1aPd", ADD3.replace("v8, v18, v14", other) + BODY % (0, 0)))
        assert rc == 1 and text.splitlines()[1].startswith("DIFFERENT"), other
    rc, text = run(old, kernel("_Z1aPd", ADD3.replace("v8, v8, v18, v14", "v14, v8, v18, v8") + BODY % (0, 0)))
    assert rc == 1 and "DIFFERENT" in text


def test_three_source_operations_whose_sources_do_not_all_commute_stay_strict():
    for mnem in ("v_and_or_b32", "v_xad_u32", "v_lshl_add_u32"):
        line = "\t%s v8, v9, v18, v14\n" % mnem
        old = kernel("_Z1aPd", line + BODY % (0, 0))
        for other in ("v14, v18, v9", "v18, v9, v14", "v9, v14, v18"):
            rc, text = run(old, kernel("_Z1aPd", line.replace("v9, v18, v14", other) + BODY % (0, 0)))
            assert rc == 1 and text.splitlines()[1].startswith("DIFFERENT"), (mnem, other)


def test_real_differences_fail():
    old = kernel("_Z1aPd", BODY % (0, 0))
    extra = kernel("_Z1aPd", (BODY % (0, 0)).replace("\tv_sub_u32", "\tv_mov_b32_e32 v11, v1\n\tv_sub_u32"))
    rc, text = run(old, extra)
    assert rc == 1 and text.splitlines()[1].startswith("DIFFERENT") and "6/7" in text
    # a subtraction does not commute, another destination is another instruction, another branch target another loop
    for a, b in (("v_sub_u32_e32 v1, v0, v10", "v_sub_u32_e32 v1, v10, v0"),
                 ("v_mul_f64 v[2:3], v[4:5], v[6:7]", "v_mul_f64 v[4:5], v[2:3], v[6:7]"),
                 ("s_cbranch_scc1 .LBB0_1", "s_cbranch_scc1 .LBB0_2")):
        rc, text = run(old, kernel("_Z1aPd", (BODY % (0, 0)).replace(a, b)))
        assert rc == 1 and "DIFFERENT" in text, (a, b)
    # the same instructions with another register count or LDS size: reported and refused
    rc, text = run(old, kernel("_Z1aPd", BODY % (0, 0), vgpr=13))
    assert rc == 1 and "12/13" in text and "RESOURCES DIFFER: next_free_vgpr 12/13" in text and text.splitlines()[1].startswith("identical")
    rc, text = run(old, kernel("_Z1aPd", BODY % (0, 0), lds=1024))
    assert rc == 1 and "0/1024" in text
    # a kernel only one side has
    rc, text = run(old, old + kernel("_Z1cPd", BODY % (1, 1), ordinal=1))
    assert rc == 1 and "only in the new file" in text


def test_command_line(tmp_path):
    a, b = tmp_path / "old.s", tmp_path / "new.s"
    a.write_text(kernel("_Z1aPd", BODY % (0, 0)))
    b.write_text(kernel("_Z1aPd", BODY % (0, 0)))
    assert subprocess.run([sys.executable, SCRIPT, str(a), str(b)], capture_output=True).returncode == 0
    b.write_text(kernel("_Z1aPd", (BODY % (0, 0)).replace("\tv_sub_u32", "\tv_nop\n\tv_sub_u32")))
    r = subprocess.run([sys.executable, SCRIPT, str(a), str(b)], capture_output=True, text=True)
    assert r.returncode == 1 and "DIFFERENT" in r.stdout
