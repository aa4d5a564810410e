"""Are the kernels of two hipcc -S outputs the same code? (development aid: the check behind a source-only refactoring)
usage: isa_same.py old.s new.s
  hipcc <the Makefile's flags> --cuda-device-only -S file.hip -o file.s   at both commits
Kernels are paired by mangled name.  Comments and every directive except the .amdhsa_* resource block are dropped, block
labels lose the function ordinal (.LBB12_3 -> .LBB_3), and each kernel is put in one of three classes:
  identical   the same instruction stream
  swapped     the same stream up to exchanged sources of a commutative instruction (v_mul_f64 v[0:1], v[2:3], v[4:5] against
              v_mul_f64 v[0:1], v[4:5], v[2:3]; the three sources of v_add3_u32 in any order): same opcode, same destination,
              same position, same count
  DIFFERENT   anything else, or a kernel only one file has
with the instruction counts and .amdhsa_next_free_vgpr / _sgpr / group_segment_fixed_size / private_segment_fixed_size
(VGPRs, SGPRs, static LDS, scratch) of both.  Exit status 1 if a kernel is DIFFERENT or any .amdhsa_* value differs."""
import re
import sys

RESOURCES = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")
# two-source operations whose sources may be exchanged, and three-source ones whose first two may
COMMUTE2 = re.compile(r"^[vs]_(pk_)?(add|mul|mul_lo|mul_hi|and|or|xor|xnor|max|min)_[a-z]*\d+(_e32|_e64)?$")
COMMUTE3 = re.compile(r"^v_(pk_)?(fma|mad)_[a-z]*\d+(_e64)?$")
# ... and the one three-source operation ALL of whose sources commute, the integer add; v_xad_u32, v_and_or_b32 and
# v_lshl_add_u32 treat their sources differently and stay strict
COMMUTE_ALL3 = re.compile(r"^v_add3_u32(_e64)?$")


def parse(text):
    """-> {kernel: (instructions, {amdhsa directive: value})}; an instruction is (mnemonic, [operands]), a label (label, None)"""
    code, res, cur, hsa = {}, {}, None, None
    for raw in text.split("\n"):
        line = raw.split(";")[0].split("//")[0].strip()
        if not line:
            continue
        m = re.match(r"^([A-Za-z_][\w$.]*):$", line)
        if m and not line.startswith(".L"):
            cur = m.group(1)
            code[cur] = []
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        if line.startswith(".amdhsa_kernel"):
            hsa = line.split()[1]
            res[hsa] = {}
            continue
        if line.startswith(".end_amdhsa_kernel"):
            hsa = None
            continue
        if hsa is not None and line.startswith(".amdhsa_"):
            key, _, val = line[len(".amdhsa_"):].partition(" ")
            res[hsa][key] = val.strip()
            continue
        if cur is None:
            continue
        line = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", line)
        if line.endswith(":"):
            code[cur].append((line, None))
        elif not line.startswith("."):
            mnem, _, ops = line.partition(" ")
            code[cur].append((mnem, [o.strip() for o in ops.split(",")] if ops.strip() else []))
    return {k: (code[k], res[k]) for k in code if k in res}


def swapped_sources(a, b):
    (ma, oa), (mb, ob) = a, b
    if ma != mb or oa is None or ob is None or len(oa) != len(ob):
        return False
    if COMMUTE2.match(ma) and len(oa) == 3:
        return oa[0] == ob[0] and oa[1] == ob[2] and oa[2] == ob[1]
    if COMMUTE3.match(ma) and len(oa) >= 4:
        return oa[0] == ob[0] and oa[1] == ob[2] and oa[2] == ob[1] and oa[3:] == ob[3:]
    if COMMUTE_ALL3.match(ma) and len(oa) == 4:
        return oa[0] == ob[0] and sorted(oa[1:]) == sorted(ob[1:])
    return False


def classify(old, new):
    """-> ("identical" | "swapped" | "DIFFERENT", number of instructions that differ only by exchanged sources)"""
    if old == new:
        return "identical", 0
    if len(old) != len(new):
        return "DIFFERENT", 0
    swaps = 0
    for a, b in zip(old, new):
        if a == b:
            continue
        if not swapped_sources(a, b):
            return "DIFFERENT", 0
        swaps += 1
    return "swapped", swaps


def count(instrs):
    return sum(1 for _, ops in instrs if ops is not None)


def compare(old_text, new_text, out=sys.stdout):
    old, new = parse(old_text), parse(new_text)
    bad = 0
    tally = {"identical": 0, "swapped": 0, "DIFFERENT": 0}
    out.write("%-10s %13s %11s %11s %15s %11s  kernel\n" % ("class", "instructions", "vgpr", "sgpr", "lds", "scratch"))
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            out.write("%-10s only in the %s file  %s\n" % ("DIFFERENT", "old" if name in old else "new", name))
            tally["DIFFERENT"] += 1
            bad += 1
            continue
        (ci, ri), (cj, rj) = old[name], new[name]
        cls, swaps = classify(ci, cj)
        tally[cls] += 1
        cols = ["%d/%d" % (count(ci), count(cj))] + ["%s/%s" % (ri.get(k, "?"), rj.get(k, "?")) for k in RESOURCES]
        note = " (%d exchanged)" % swaps if swaps else ""
        other = sorted(k for k in set(ri) | set(rj) if ri.get(k) != rj.get(k))
        if other:
            note += " RESOURCES DIFFER: " + ", ".join("%s %s/%s" % (k, ri.get(k, "?"), rj.get(k, "?")) for k in other)
        out.write("%-10s %13s %11s %11s %15s %11s  %s%s\n" % ((cls,) + tuple(cols) + (name, note)))
        if cls == "DIFFERENT" or other:
            bad += 1
    out.write("%d kernels: %d identical, %d identical up to exchanged sources of a commutative instruction, %d different; "
              "%d to look at\n" % (sum(tally.values()), tally["identical"], tally["swapped"], tally["DIFFERENT"], bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(compare(open(sys.argv[1]).read(), open(sys.argv[2]).read()))
