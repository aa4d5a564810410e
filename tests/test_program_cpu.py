"""Word programs (include/ieache.h section 3d, ie-ache_amd/programs.py) on the host: the compiler under AddressSanitizer + UBSan
(tests/native/program_test.cpp), the one-instruction programs against the built-in kinds through the C ABI, random programs
against Python integers, the shape of SUM, the export of any compiled netlist, and every refusal.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import random_netlists as rn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF, KS, CSA, FA = 0, 1, 2, 3
MAJ3, XOR3 = 32, 33


def test_program_compiler_under_asan_ubsan(tmp_path):
    exe = tmp_path / "program_test"
    csrc = os.path.join(ROOT, "ie-ache_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "native", "program_test.cpp"),
                           os.path.join(csrc, "circuit.cpp"), os.path.join(csrc, "program.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "PROGRAM_OK" in r.stdout, r.stdout[-4000:]


# ---- anchor: a one-instruction program is the built-in kind ----

def info_get(ia, kind, bits):
    """ieache_circuit_info_get: the fields it writes (through `folded`)."""
    info = ia.CircuitInfo()
    L = ia.lib()
    L.ieache_circuit_info_get.argtypes = [C.c_int, C.c_int, C.POINTER(ia.CircuitInfo)]
    assert L.ieache_circuit_info_get(kind, bits, C.byref(info)) == 0
    return info


V01_FIELDS = ("n_inputs", "n_outputs", "n_slots", "depth", "max_width", "bootstraps", "n_and", "n_xor", "sched_max_width", "folded")


def same_as_kind(ia, compiled, kind, bits, fold=False):
    want, got = info_get(ia, kind, bits), compiled.info()
    for f in V01_FIELDS:
        if f != "folded":  # ieache_netlist_info reports 0: the flag says what a CONTEXT option did
            assert getattr(got, f) == getattr(want, f), (kind, bits, f)
    full = ia.circuit_info(kind, bits)
    assert got.sched_levels == full.sched_levels
    for t in list(range(ia.GATE_TYPES)) + [MAJ3, XOR3]:
        assert compiled.gate_count(t) == ia.circuit_gate_count(kind, bits, t), (kind, bits, t)
    rng = np.random.default_rng([kind, bits])
    for v in rng.integers(0, 2, size=(64, want.n_inputs)).astype(np.uint8):
        assert np.array_equal(compiled.simulate(v), ia.circuit_simulate(kind, bits, v)), (kind, bits)


def kind_rows(ia):
    return [(ia.CIRC_ADD, "add", REF), (ia.CIRC_SUB, "sub", REF), (ia.CIRC_RSUB, "rsub", REF), (ia.CIRC_MUL, "mul", REF),
            (ia.CIRC_ADD_KS, "add", KS), (ia.CIRC_SUB_KS, "sub", KS), (ia.CIRC_RSUB_KS, "rsub", KS), (ia.CIRC_MUL_WALLACE, "mul", CSA),
            (ia.CIRC_ADD_FA, "add", FA), (ia.CIRC_SUB_FA, "sub", FA), (ia.CIRC_RSUB_FA, "rsub", FA), (ia.CIRC_MUL_FA, "mul", FA)]


@pytest.mark.parametrize("row", range(12))
def test_one_instruction_program_is_the_builtin_kind(ia, row):
    """Given the caller's carry word, under the schedule and folding the kind itself is built with: the slack-balanced schedule
    for the 64-bit multipliers, folding for MUL_WALLACE (the one kind that is built folded whatever the caller asks)."""
    kind, op, family = kind_rows(ia)[row]
    for bits in ((32, 64) if op == "mul" else (1, 7, 16, 32)):
        p = ia.WordProgram(family=family)
        a, b, carry = p.input(bits), p.input(bits), p.input(32)
        compiled = p.compile([getattr(p, op)(a, b, carry)], fold=kind == ia.CIRC_MUL_WALLACE, balanced=op == "mul" and bits >= 64)
        same_as_kind(ia, compiled, kind, bits)


def test_two_instruction_programs_are_the_chain_kinds(ia):
    for bits in (8, 32):  # (A + B) - C
        p = ia.WordProgram()
        a, b, carry, c = p.input(bits), p.input(bits), p.input(32), p.input(bits)
        same_as_kind(ia, p.compile([p.sub(p.add(a, b, carry), c, carry)]), ia.circ_chain(ia.CIRC_ADD, ia.CIRC_SUB), bits)
    p = ia.WordProgram()  # A * B + C
    a, b, carry, c = p.input(32), p.input(32), p.input(32), p.input(64)
    same_as_kind(ia, p.compile([p.add(p.mul(a, b, carry), c, carry)]), ia.CIRC_MULADD, 32)
    p = ia.WordProgram()  # flip = 0: C - (B - A), C's own carry word
    a, b, carry, c, carry2 = p.input(16), p.input(16), p.input(32), p.input(16), p.input(32)
    same_as_kind(ia, p.compile([p.sub(c, p.rsub(a, b, carry), carry2)]), ia.circ_chain(ia.CIRC_RSUB, ia.CIRC_SUB, flip=False), 16)


# ---- arithmetic: random programs against Python integers ----

class RandomProgram:
    """3 .. 12 instructions over widths 1 .. 12 (multipliers at 32).  Every register carries the Python function of the input
    values that it must equal, and the set of instructions whose GATES or inputs its samples come from: a sum without folding
    must not meet one wire twice in a column, so its operands are chosen with disjoint origins."""

    def __init__(self, ia, seed):
        self.ia, self.rng = ia, np.random.default_rng([seed, 4242])
        self.p = ia.WordProgram(family=int(self.rng.choice([REF, KS, FA])))
        self.regs = []  # (Register, f(input values) -> int, origins)
        self.inputs = []
        self.ops = set()
        for _ in range(2):
            self.input(int(self.rng.integers(1, 13)))
        n = int(self.rng.integers(3, 13))
        while len(self.p) < n:
            self.step()

    def input(self, width):
        i = len(self.inputs)
        r = self.p.input(width)
        self.inputs.append(width)
        return self.put(r, lambda v, i=i: v[i], {("in", i)})

    def put(self, reg, f, origins, fresh=False):
        mask = (1 << reg.width) - 1
        self.regs.append((reg, lambda v, f=f, mask=mask: f(v) & mask, {("gate", reg.index)} if fresh else set(origins)))
        return self.regs[-1]

    def pick(self, width=None):
        c = [r for r in self.regs if width is None or r[0].width == width]
        return c[int(self.rng.integers(0, len(c)))] if c else None

    def to_width(self, r, width):
        reg, f, o = r
        if reg.width == width:
            return r
        if reg.width < width:
            return self.put(reg.zext(width), f, o)
        return self.put(reg.slice(0, width), f, o)

    def step(self):
        rng, p = self.rng, self.p
        op = str(rng.choice(["input", "const", "zext", "slice", "shl", "not", "concat", "and", "or", "xor", "andbit", "add", "sub", "rsub",
                             "mul", "sum", "lt", "eq", "select", "minmax", "dot"]))
        self.ops.add(op)
        x = self.pick()
        xr, xf, xo = x
        w = xr.width
        if op == "input":
            return self.input(int(rng.integers(1, 13)))
        if op == "const":
            width = int(rng.integers(1, 13))
            value = (1 << width) - 1 if rng.random() < 0.3 else int(rng.integers(0, 1 << width))
            return self.put(p.const(width, value), lambda v, value=value: value, set())
        if op == "zext":
            return self.to_width(x, int(rng.integers(w, 13)) if w < 13 else w + 1)
        if op == "slice":
            first = int(rng.integers(0, w))
            count = int(rng.integers(1, w - first + 1))
            return self.put(xr.slice(first, count), lambda v: xf(v) >> first, xo)
        if op == "shl":
            k = int(rng.integers(0, w + 2))
            return self.put(xr << k, lambda v: xf(v) << k, xo)
        if op == "not":
            return self.put(~xr, lambda v: ~xf(v), xo)
        if op == "concat":
            yr, yf, yo = self.pick()
            if w + yr.width > 64:
                return None
            return self.put(xr.concat(yr), lambda v: xf(v) | (yf(v) << w), xo | yo)
        if op in ("and", "or", "xor", "lt", "eq", "minmax", "add", "sub", "rsub"):
            y = self.to_width(self.pick(), w)
            yr, yf = y[0], y[1]
            if op == "and":
                return self.put(xr & yr, lambda v: xf(v) & yf(v), None, True)
            if op == "or":
                return self.put(xr | yr, lambda v: xf(v) | yf(v), None, True)
            if op == "xor":
                return self.put(xr ^ yr, lambda v: xf(v) ^ yf(v), None, True)
            if op == "lt":
                return self.put(xr.lt(yr), lambda v: int(xf(v) < yf(v)), None, True)
            if op == "eq":
                return self.put(xr.eq(yr), lambda v: int(xf(v) == yf(v)), None, True)
            if op == "minmax":
                if rng.random() < 0.5:
                    return self.put(p.minimum(xr, yr), lambda v: min(xf(v), yf(v)), None, True)
                return self.put(p.maximum(xr, yr), lambda v: max(xf(v), yf(v)), None, True)
            # the word operators, in a family of their own choice; a carry word now and then: the adders take bit 0 of it as carry-in
            # (the reference's SUB / RSUB too: they add the complement with it), the opt-in SUB / RSUB ignore it
            family = int(rng.choice([REF, KS, FA, -1]))
            if (p.family if family < 0 else family) == FA and xo & y[2]:
                family = KS  # x + x on full adders is XOR3(x, x, carry): refused without folding, as it must be
            carry, cf = None, (lambda v: 0)
            c = self.pick()
            if rng.random() < 0.4 and not (c[2] & (xo | y[2])):  # a full adder would meet an operand's sample again in its carry-in
                carry, cf = self.to_width(c, 32)[0], (lambda v, g=c[1]: g(v) & 1)
            used = p.family if family < 0 else family
            reads_carry = op == "add" or used == REF
            sign = {"add": (1, 1), "sub": (1, -1), "rsub": (-1, 1)}[op]
            build = getattr(p, op)
            return self.put(build(xr, yr, carry, None if family < 0 else family),
                            lambda v: sign[0] * xf(v) + sign[1] * yf(v) + (cf(v) if reads_carry else 0), None, True)
        if op == "andbit":
            b = self.pick()
            bit = self.put(b[0].slice(0, 1), b[1], b[2])
            return self.put(xr.and_bit(bit[0]), lambda v: xf(v) if bit[1](v) else 0, None, True)
        if op == "mul":
            if any(r[0].width == 64 for r in self.regs) and rng.random() < 0.7:
                return None  # one multiplier per program is plenty
            y = self.pick()
            a, b = self.to_width(x, 32), self.to_width(y, 32)
            family = int(rng.choice([REF, CSA, FA]))
            return self.put(p.mul(a[0], b[0], None, family), lambda v: a[1](v) * b[1](v), None, True)
        if op == "select":
            c = self.pick()
            cond = self.put(c[0].slice(0, 1), c[1], c[2])
            y = self.to_width(self.pick(), w)
            return self.put(p.select(cond[0], xr, y[0]), lambda v: xf(v) if cond[1](v) else y[1](v), None, True)
        if op == "sum":
            k = int(rng.integers(2, 7))
            chosen, seen = [], set()
            for i in rng.permutation(len(self.regs)):
                reg, f, o = self.regs[int(i)]
                if len(chosen) < k and not (o & seen):
                    chosen.append((reg, f, int(rng.integers(0, 4))))
                    seen |= o
            if len(chosen) < 2:
                return None
            width = int(rng.integers(1, 13))
            family = int(rng.choice([FA, KS]))
            return self.put(p.sum([(r, s) for r, _, s in chosen], width, family), lambda v: sum(f(v) << s for _, f, s in chosen), None, True)
        if op == "dot":
            pairs = [(self.pick(), self.to_width(self.pick(), int(rng.integers(1, 5)))) for _ in range(int(rng.integers(1, 3)))]
            width = int(rng.integers(1, 13))
            return self.put(p.dot([(a[0], b[0]) for a, b in pairs], width), lambda v: sum(a[1](v) * b[1](v) for a, b in pairs), None, True)
        raise AssertionError(op)

    def outputs(self):
        others = self.regs[int(self.rng.integers(0, len(self.regs)))]
        return [self.regs[-1], others]

    def input_bits(self, values):
        return np.array([(v >> j) & 1 for v, w in zip(values, self.inputs) for j in range(w)], dtype=np.uint8)


def check_program(rp, compiled_pair, seed):
    outs = rp.outputs_
    rng = np.random.default_rng([seed, 99])
    for _ in range(8):
        values = [int(rng.integers(0, 1 << w)) for w in rp.inputs]
        want = np.array([(f(values) >> j) & 1 for reg, f, _ in outs for j in range(reg.width)], dtype=np.uint8)
        for compiled in compiled_pair:
            assert np.array_equal(compiled.simulate(rp.input_bits(values)), want), (seed, values)


def make_random_program(ia, seed):
    rp = RandomProgram(ia, seed)
    rp.outputs_ = rp.outputs()
    regs = [r[0] for r in rp.outputs_]
    return rp, (rp.p.compile(regs), rp.p.compile(regs, fold=True))


def test_random_programs_compute_what_python_integers_compute(ia):
    """2 000 seeded programs, 8 input vectors each, unfolded and folded: both equal the integers mod 2^width."""
    ops = set()
    for seed in range(2000):
        rp, pair = make_random_program(ia, seed)
        check_program(rp, pair, seed)
        assert pair[1].info().bootstraps <= pair[0].info().bootstraps
        ops |= rp.ops
    assert len(ops) == 21, ops  # every opcode and helper was drawn


# ---- the shape of SUM ----

def wallace_stages(k):
    s, w = 0, 2
    while w < k:
        s, w = s + 1, w * 3 // 2
    return s


@pytest.mark.parametrize("family", [FA, KS])
@pytest.mark.parametrize("width", [6, 32])
def test_sum_is_a_carry_save_tree_and_one_addition(ia, family, width):
    """Depth: Wallace's stage count plus the stand-alone addition's.  Bootstraps: each compressor cell is two gates and takes one
    sample out of its column, so k rows go down to two in at most width x (k - 2) cells; with the addition, a full-adder ripple of
    2 x width gates, that is the bound 2 x width x (k - 1).  The Kogge-Stone addition is more than 2 x width gates by itself (454
    at 32 bits, so the k = 2 sum, which is just that addition, cannot meet 2 x width): there the bound is the same one with the
    stand-alone Kogge-Stone addition's count in the ripple's place."""
    add = ia.circuit_info(ia.CIRC_ADD_FA if family == FA else ia.CIRC_ADD_KS, width)
    assert family != FA or add.bootstraps == 2 * width
    for k in (2, 3, 4, 5, 8, 9, 13):
        p = ia.WordProgram()
        compiled = p.compile([p.sum([p.input(width) for _ in range(k)], width, family=family)])
        info = compiled.info()
        assert info.depth == wallace_stages(k) + add.depth, (k, info.depth)
        assert info.bootstraps <= 2 * width * (k - 2) + add.bootstraps, (k, info.bootstraps)
        assert info.bootstraps == len(compiled.gates)
        for t, a, b, c in compiled.gates:
            if t in (MAJ3, XOR3):
                wires = [r >> 1 for r in (a, b, c) if r >= 0]
                assert len(set(wires)) == len(wires), (k, t, a, b, c)
        assert compiled.gate_count(MAJ3) > 0 or k == 2 and family == KS
        rng = np.random.default_rng([k, width, family])
        for _ in range(4):
            values = [int(v) for v in rng.integers(0, 1 << width, size=k)]
            bits = np.array([(v >> j) & 1 for v in values for j in range(width)], dtype=np.uint8)
            assert sum(int(b) << j for j, b in enumerate(compiled.simulate(bits))) == sum(values) % (1 << width)


# ---- export ----

def recreated(ia, compiled, balanced=False):
    nl = ia.Netlist(compiled.info().n_inputs)
    for g in compiled.gates:
        nl.gate(*g)
    return nl.compile(compiled.outputs, balanced=balanced)


def same_netlist(a, b, seed):
    assert bytes(a.info()) == bytes(b.info())
    assert a.gates_by_type() == b.gates_by_type() and a.gate_count(MAJ3) == b.gate_count(MAJ3) and a.gate_count(XOR3) == b.gate_count(XOR3)
    for v in np.random.default_rng([seed, 5]).integers(0, 2, size=(16, a.info().n_inputs)).astype(np.uint8):
        assert np.array_equal(a.simulate(v), b.simulate(v))


@pytest.mark.parametrize("params", [(5, 64), (16, 1024)])
def test_export_of_created_netlists_is_what_was_recorded(ia, params):
    for seed, family in rn.corpus(params):
        nl, gates, outputs = rn.generate(seed, family)
        for balanced in (False, True):
            compiled = nl.compile(outputs, balanced=balanced)
            got_gates, got_outputs = ia.netlist_export(compiled)
            assert got_gates == [tuple(g) for g in gates] and got_outputs == list(outputs), (seed, family)
            same_netlist(recreated(ia, compiled, balanced), compiled, seed)


def test_export_of_programs_compiles_to_the_same_netlist(ia):
    for seed in range(200):
        rp, pair = make_random_program(ia, seed)
        for compiled in pair:  # unfolded, and the gates after folding
            assert compiled.n_inputs == sum(rp.inputs) and len(compiled.gates) == sum(compiled.gates_by_type()) + compiled.gate_count(MAJ3) + \
                compiled.gate_count(XOR3)
            same_netlist(recreated(ia, compiled), compiled, seed)
    p = ia.WordProgram()
    compiled = p.compile([p.mul(p.input(64), p.input(64), family=FA)], balanced=True)
    same_netlist(recreated(ia, compiled, balanced=True), compiled, 0)


def test_export_counts_before_it_writes(ia):
    nl, gates, outputs = rn.generate(1000, "window")
    compiled = nl.compile(outputs)
    L = ia.lib()
    assert L.ieache_netlist_export(compiled.h, None, 0, None, 0) == len(gates)
    buf = np.full((len(gates), 4), 77, dtype=np.int32)
    outs = np.full(len(outputs), 77, dtype=np.int32)
    i32p = C.POINTER(C.c_int32)
    assert L.ieache_netlist_export(compiled.h, buf.ctypes.data_as(C.c_void_p), len(gates) - 1, outs.ctypes.data_as(i32p), len(outputs) - 1) == len(gates)
    assert (buf == 77).all() and (outs == 77).all()  # too small: nothing written
    assert L.ieache_netlist_export(None, None, 0, None, 0) < 0


# ---- refusals, each with its instruction ----

def refusal(ia, build, *parts):
    p = ia.WordProgram()
    outs = build(p)
    with pytest.raises(ia.IeacheError) as e:
        p.compile(outs if isinstance(outs, list) else [outs])
    for part in parts:
        assert part in str(e.value), str(e.value)


def test_refusals_name_the_instruction(ia):
    from ieache_amd.programs import Register

    def forward(p):  # a register referred to before it exists
        a = p.input(4)
        return a & Register(p, 5, 4)
    refusal(ia, forward, "program: instruction 1:", "does not exist")
    refusal(ia, lambda p: p.input(4) ^ p.input(5), "program: instruction 2:", "width mismatch")
    refusal(ia, lambda p: p.input(4).lt(p.input(3)), "program: instruction 2:", "width mismatch")
    refusal(ia, lambda p: p.add(p.input(4), p.input(4), p.input(8)), "program: instruction 3:", "carry word")
    refusal(ia, lambda p: p.input(16) * p.input(16), "program: instruction 2:", "width 16")  # a width the kind table refuses
    refusal(ia, lambda p: p.mul(p.input(32), p.input(32), family=KS), "program: instruction 2:", "no such operator")
    refusal(ia, lambda p: p.input(200).concat(p.input(200)) + p.input(400), "program: instruction 4:", "width 400")
    refusal(ia, lambda p: p.input(513), "program: instruction 0:", "outside 1 .. 512")
    refusal(ia, lambda p: p.input(300).concat(p.input(300)), "program: instruction 2:", "outside 1 .. 512")
    refusal(ia, lambda p: p.sum([p.input(4), p.input(4)], 513), "program: instruction 2:", "outside 1 .. 512")
    refusal(ia, lambda p: p.sum([p.input(4), p.input(4)], 0), "program: instruction 2:", "outside 1 .. 512")
    refusal(ia, lambda p: p.sum([p.input(512)] * ((1 << 20) + 8), 512), "program: instruction 1:", "2^30")
    refusal(ia, lambda p: [p.input(4)][:0], "program:", "no outputs")

    def twice(p):  # one wire twice in a MAJ3 / XOR3
        a = p.input(4)
        return p.sum([a, (a, 1), (a, 0)], 6)
    refusal(ia, twice, "program: instruction 1:", "same wire twice")
    p = ia.WordProgram()
    folded = p.compile([twice(p)], fold=True)  # with folding the same program is lowered instead
    assert sum(int(b) << j for j, b in enumerate(folded.simulate(np.array([1, 0, 1, 1], dtype=np.uint8)))) == 13 * 4
    with pytest.raises(ia.IeacheError):  # a refusal leaves the message, not a handle
        ia.WordProgram().compile([])
    assert ia.lib().ieache_last_error().decode().startswith("program:")
