"""Host logic of the three-input gates MAJ3 / XOR3 and of the full-adder circuits built on them (no GPU, no ciphertexts):
truth tables through the netlist ABI, what the ABI refuses, the statistics of the four IEACHE_CIRC_*_FA kinds derived on paper,
their plaintext semantics against Python integers, and the noise budget of DESIGN.md section 7."""
import ctypes as C
import itertools

import numpy as np
import pytest

from test_circuits_cpu import APP_C

MAJ3, XOR3 = 32, 33
TRUTH3 = {MAJ3: lambda a, b, c: int(a + b + c >= 2), XOR3: lambda a, b, c: a ^ b ^ c}
ALL_BITS = [tuple((v >> i) & 1 for i in range(3)) for v in range(8)]


def operand_forms(ia, nl):
    """Plain, negated and both constants in every position; never the same wire twice."""
    a, b, c = nl.input(0), nl.input(1), nl.input(2)
    N, T, F = ia.NOT, ia.TRUE, ia.FALSE
    forms = [(a, b, c), (N(a), b, c), (a, N(b), c), (a, b, N(c)), (N(a), N(b), N(c)), (c, a, b), (b, N(c), a)]
    for k in (T, F):
        forms += [(k, b, c), (a, k, c), (a, b, k), (k, N(b), c), (N(a), k, N(c))]
    forms += [(T, F, c), (a, T, T), (F, b, F), (T, T, T), (F, F, F), (F, T, F)]
    return forms


def ref_bit(r, bits):
    return (1 if r == -1 else 0) if r < 0 else bits[r >> 1] ^ (r & 1)


@pytest.mark.parametrize("gate", [MAJ3, XOR3])
def test_truth_tables_through_the_netlist_simulation(ia, gate):
    assert (ia.GATE_MAJ3, ia.GATE_XOR3) == (MAJ3, XOR3)
    nl = ia.Netlist(3)
    forms = operand_forms(ia, nl)
    outs = [nl.gate(gate, *f) for f in forms]
    cn = nl.compile(outs)
    info = cn.info()
    assert info.depth == 1 and info.bootstraps == len(forms) == info.max_width  # one rotation each, all in one level
    for bits in ALL_BITS:
        got = cn.simulate(bits)
        assert list(got) == [TRUTH3[gate](*(ref_bit(r, bits) for r in f)) for f in forms], bits


def test_a_three_input_gate_feeds_later_gates_and_counts_its_third_read(ia):
    """c is an operand like a and b: it sets the gate's level, and its wire stays alive until the gate has read it."""
    nl = ia.Netlist(4)
    a, b, c, d = (nl.input(i) for i in range(4))
    x = nl.AND(a, b)
    y = nl.XOR(x, c)          # level 2
    m = nl.MAJ3(a, b, y)      # level 3 only through its third operand
    s = nl.XOR3(d, ia.NOT(m), x)
    out = nl.MUX(s, m, ia.NOT(y))
    cn = nl.compile([out, s, m])
    assert cn.info().depth == 5 and cn.info().bootstraps == 4 + 2
    for v in range(16):
        bits = [(v >> i) & 1 for i in range(4)]
        x_, y_ = bits[0] & bits[1], (bits[0] & bits[1]) ^ bits[2]
        m_ = TRUTH3[MAJ3](bits[0], bits[1], y_)
        s_ = bits[3] ^ (1 - m_) ^ x_
        assert list(cn.simulate(bits)) == [m_ if s_ else 1 - y_, s_, m_]


def test_refusals(ia):
    def compiled(gates, n_inputs=3):
        nl = ia.Netlist(n_inputs)
        for g in gates:
            nl.gate(*g)
        return nl.compile([(n_inputs + len(gates) - 1) << 1])

    a, b, c = 0, 2, 4
    # the same WIRE twice, whatever the signs; constants may repeat
    for t in (MAJ3, XOR3):
        for ops in ((a, a, c), (a, b, a), (a, b, b ^ 1), (a ^ 1, a, a)):
            with pytest.raises(ia.IeacheError, match="gate 1"):
                compiled([(0, a, b, 0), (t,) + ops])
        compiled([(t, ia.TRUE, ia.TRUE, a)])
        compiled([(t, ia.FALSE, b, ia.FALSE)])
        with pytest.raises(ia.IeacheError, match="gate 0: operand c"):  # the third operand is checked like the others
            compiled([(t, a, b, 6 << 1)])
    # the codes between the libtfhe types and the two new ones name nothing
    for t in list(range(11, 32)) + [34]:
        with pytest.raises(ia.IeacheError, match="gate 0: unknown gate type %d" % t):
            compiled([(t, a, b, 0)])
    # the flat entry points take the two new types only (checked before anything else, so no context is needed to see it)
    L = ia.lib()
    for t in (ia.GATE_AND, ia.GATE_XOR, ia.GATE_MUX, ia.GATE_ORYN, 11, 31, 34, -1):
        assert L.ieache_gates3(None, t, 0, None, None, None, None, None) == -22
        assert b"three-input" in L.ieache_last_error()
        assert L.ieache_gates3_device(None, t, 0, None, None, None, None, None) == -22
    # ... and the two-input ones still refuse them
    for t in (MAJ3, XOR3):
        assert L.ieache_gates(None, t, 0, None, None, None, None) == -22


def test_netlist_info_still_fills_eleven_counts(ia):
    nl = ia.Netlist(3)
    a, b, c = nl.input(0), nl.input(1), nl.input(2)
    m = nl.MAJ3(a, b, c)
    x = nl.XOR3(a, ia.NOT(b), ia.TRUE)
    x2 = nl.XOR3(m, x, c)
    g = nl.NOR(m, x2)
    u = nl.MUX(g, m, x)
    cn = nl.compile([u])
    assert ia.GATE_TYPES == 11
    # a buffer of 11 counts and a guard word behind it: ieache_netlist_info writes the 11 and nothing else
    buf = (C.c_int64 * 12)(*([-7] * 12))
    info = ia.CircuitInfo()
    assert ia.lib().ieache_netlist_info(cn.h, C.byref(info), buf) == 0
    assert list(buf) == [0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, -7]
    assert cn.gates_by_type() == list(buf)[:11]
    for t in range(11):
        assert cn.gate_count(t) == buf[t]
    assert cn.gate_count(MAJ3) == 1 and cn.gate_count(XOR3) == 2
    assert info.bootstraps == 1 + 2 + 1 + 2 == sum(buf[:11]) + 1 + cn.gate_count(MAJ3) + cn.gate_count(XOR3)  # the MUX is two
    for t in (-1, 11, 31, 34):
        with pytest.raises(ia.IeacheError):
            cn.gate_count(t)


def test_adder_fa_worked_example(ia):
    from ieache_amd import netlists
    from ieache_amd.tools import bits_to_int, int_to_bits
    cn = netlists.adder_fa(8)
    assert cn.info().bootstraps == 16 and cn.info().depth == 8
    assert (cn.gate_count(MAJ3), cn.gate_count(XOR3), cn.gate_count(0), cn.gate_count(1)) == (7, 7, 1, 1)
    rng = np.random.default_rng(3)
    for a, b in [(0, 0), (255, 255), (255, 1), (170, 85)] + [tuple(int(v) for v in rng.integers(0, 256, 2)) for _ in range(40)]:
        assert bits_to_int(cn.simulate(np.concatenate([int_to_bits(a, 8), int_to_bits(b, 8)]))) == a + b


# ---- the built-in kinds ----
# Derived on paper (csrc/circuit.cpp: full_adder_ripple, full_adder_mul):
#   ADD_FA / SUB_FA / RSUB_FA, b bits: one XOR3 and one MAJ3 per bit, the top carry included as in the reference's add();
#     the carry chain is one level per bit, a level holds that bit's two gates.  (The constant carry-in of SUB / RSUB is an
#     operand like any other unless constants are folded.)
#   MUL_FA, n bits: n*n ANDs, all in level 1; rows 1 .. n-1 of the array hold n-1 full adders each (the top cell of a row has two
#     constant-zero operands and is a wire), one level per row; the ripple over the last two rows has n-1 cells (its top cell is
#     a wire as well), one level each: n*n + 2 (n-1)^2 + 2 (n-1) = 3 n*n - 2 n bootstraps, 1 + (n-1) + (n-1) levels.
FA_REFERENCE = {16: 1, 17: 2, 18: 3, 19: 4}


def fa_stats(kind, bits):
    """(bootstraps, and, xor, depth, max_width, maj3, xor3)"""
    if kind == 19:
        n = bits
        return (3 * n * n - 2 * n, n * n, 0, 2 * n - 1, n * n, n * (n - 1), n * (n - 1))
    return (2 * bits, 0, 0, bits, 2, bits, bits)


FA_CASES = [(k, b) for k in (16, 17, 18) for b in (1, 16, 32, 64, 128, 256)] + [(19, 32), (19, 64), (19, 128)]


@pytest.mark.parametrize("kind,bits", FA_CASES)
def test_full_adder_kind_statistics(ia, kind, bits):
    assert (ia.CIRC_ADD_FA, ia.CIRC_SUB_FA, ia.CIRC_RSUB_FA, ia.CIRC_MUL_FA) == (16, 17, 18, 19)
    info = ia.circuit_info(kind, bits)
    n_maj3, n_xor3 = ia.circuit_gate_count(kind, bits, MAJ3), ia.circuit_gate_count(kind, bits, XOR3)
    assert (info.bootstraps, info.n_and, info.n_xor, info.depth, info.max_width, n_maj3, n_xor3) == fa_stats(kind, bits)
    assert info.bootstraps == info.n_and + n_maj3 + n_xor3
    assert info.n_inputs == 2 * bits + 32 and info.n_outputs == (2 * bits if kind == 19 else bits)
    ref = (FA_REFERENCE[kind], bits)
    if ref in APP_C:
        assert info.reference_bootstraps == APP_C[ref][0]
    assert info.reference_bootstraps == ia.circuit_info(*ref).bootstraps
    if (kind, bits) == (16, 16):
        assert (info.bootstraps, info.reference_bootstraps, info.depth) == (32, 80, 16)
    if (kind, bits) == (19, 32):
        assert (info.bootstraps, info.reference_bootstraps, info.depth) == (3008, 11264, 63)


def test_widths_and_chains_the_new_kinds_refuse(ia):
    for bits in (0, 16, 48, 256):
        with pytest.raises(ia.IeacheError):
            ia.circuit_info(19, bits)
    for kind in (16, 17, 18):
        with pytest.raises(ia.IeacheError):
            ia.circuit_info(kind, 0)
    for kind in (10, 11, 15, 20, 31, 64):  # the codes around the new ones still name nothing
        with pytest.raises(ia.IeacheError):
            ia.circuit_info(kind, 32)
    # a chain's stage kinds are 1 .. 4: there is no code that would name an _FA stage
    assert all(ia.circ_chain(k1, k2, f) not in (16, 17, 18, 19) for k1 in range(1, 5) for k2 in range(1, 5) for f in (True, False))


@pytest.mark.parametrize("key", sorted(APP_C))
def test_existing_kinds_keep_their_statistics(ia, key):
    info = ia.circuit_info(*key)
    assert (info.bootstraps, info.n_and, info.n_xor, info.depth, info.max_width) == APP_C[key]
    assert ia.circuit_gate_count(key[0], key[1], MAJ3) == 0 and ia.circuit_gate_count(key[0], key[1], XOR3) == 0
    assert ia.circuit_gate_count(key[0], key[1], 0) == info.n_and and ia.circuit_gate_count(key[0], key[1], 1) == info.n_xor


def run_kind(ia, kind, bits, a, b, carry_bits=0, fold=False):
    from ieache_amd.tools import bits_to_int, int_to_bits
    x = np.zeros(2 * bits + 32, dtype=np.uint8)
    x[:bits], x[bits:2 * bits], x[2 * bits:] = int_to_bits(a, bits), int_to_bits(b, bits), int_to_bits(carry_bits, 32)
    return bits_to_int(ia.circuit_simulate(kind, bits, x, fold))


def rand_int(rng, bits):
    return int.from_bytes(rng.bytes(bits // 8), "little")


@pytest.mark.parametrize("bits", [16, 32, 64])
def test_add_sub_rsub_fa_against_python_integers(ia, bits):
    rng = np.random.default_rng(bits)
    m = 1 << bits
    cases = [(0, 0), (1, m - 1), (m - 1, m - 1), (m - 1, 0), (0, m - 1), (1 << (bits - 2), 1 << (bits - 2)), (m >> 1, m >> 1)]
    cases += [(rand_int(rng, bits), rand_int(rng, bits)) for _ in range(40)]
    for a, b in cases:
        for fold in (False, True):
            assert run_kind(ia, 16, bits, a, b, fold=fold) == (a + b) % m
            assert run_kind(ia, 17, bits, a, b, fold=fold) == (a - b) % m
            assert run_kind(ia, 18, bits, a, b, fold=fold) == (b - a) % m
        # bit 0 of the carry word is the carry-in, as in the reference's add(); the other 31 samples are not read
        assert run_kind(ia, 16, bits, a, b, carry_bits=1) == (a + b + 1) % m == run_kind(ia, 1, bits, a, b, carry_bits=1)
        assert run_kind(ia, 16, bits, a, b, carry_bits=0xFFFFFFFE) == (a + b) % m


EDGE32 = [0, 1, 2, 3, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF, 0x55555555, 0xAAAAAAAA, 0x0000FFFF, 0xFFFF0000, 1 << 30]


def test_mul32_fa_against_python_integers(ia):
    rng = np.random.default_rng(32)
    for a, b in itertools.product(EDGE32, EDGE32):
        assert run_kind(ia, 19, 32, a, b) == a * b, (a, b)
    for _ in range(200):
        a, b = rand_int(rng, 32), rand_int(rng, 32)
        assert run_kind(ia, 19, 32, a, b) == a * b, (a, b)
    for a, b in [(0xFFFFFFFF, 0xFFFFFFFF), (0, 5), (0x80000000, 2), (0x12345678, 0x9ABCDEF0)]:
        assert run_kind(ia, 19, 32, a, b, fold=True) == a * b
        assert run_kind(ia, 19, 32, a, b, carry_bits=0xFFFFFFFF) == a * b  # a multiplier has no carry-in


def test_mul64_fa_against_python_integers(ia):
    rng = np.random.default_rng(64)
    m = 1 << 64
    pairs = [(0, 0), (m - 1, m - 1), (m - 1, 1), (1 << 62, 1 << 62)] + [(rand_int(rng, 64), rand_int(rng, 64)) for _ in range(16)]
    assert len(pairs) == 20
    for a, b in pairs:
        assert run_kind(ia, 19, 64, a, b) == a * b, (a, b)


def test_mul128_fa_builds_and_multiplies(ia):
    m = 1 << 128
    assert run_kind(ia, 19, 128, m - 1, m - 1) == (m - 1) ** 2
    assert run_kind(ia, 19, 128, 0x0123456789ABCDEF0F1E2D3C4B5A6978, 0xFEDCBA9876543210A5A5A5A55A5A5A5A) == \
        0x0123456789ABCDEF0F1E2D3C4B5A6978 * 0xFEDCBA9876543210A5A5A5A55A5A5A5A


def test_folding_lowers_a_constant_operand(ia):
    """fold on: the constant carry-in of SUB / RSUB makes bit 0 an OR and an XNOR (= a free NOT of XOR), the half adders of
    MUL_FA's first row and of its ripple become AND / XOR; nothing else changes."""
    for kind in (17, 18):
        plain, folded = ia.circuit_info(kind, 32), ia.circuit_info(kind, 32, fold=True)
        assert folded.bootstraps == plain.bootstraps == 64 and folded.n_xor == 1 and folded.n_and == 0
        assert ia.circuit_gate_count(kind, 32, MAJ3, fold=True) == 31 and ia.circuit_gate_count(kind, 32, XOR3, fold=True) == 31
        assert ia.circuit_gate_count(kind, 32, ia.GATE_OR, fold=True) == 1
    f = ia.circuit_info(19, 32, fold=True)
    # row 1 (31 cells) and the ripple's first cell have a constant-zero operand: 32 MAJ3 -> AND, 32 XOR3 -> XOR
    assert (f.bootstraps, f.n_and, f.n_xor) == (3008, 1024 + 32, 32)
    assert ia.circuit_gate_count(19, 32, MAJ3, fold=True) == 32 * 31 - 32 == ia.circuit_gate_count(19, 32, XOR3, fold=True)
    # ADD_FA has no constant to fold
    a, af = ia.circuit_info(16, 32), ia.circuit_info(16, 32, fold=True)
    assert (a.bootstraps, a.depth) == (af.bootstraps, af.depth)


def test_noise_budget(ia):
    """DESIGN.md section 7.  A gate's input phase is the combination's nominal phase plus, per operand wire, that wire's noise
    (variance V, and the per-key offset delta that all wires share and that therefore adds coherently) times its multiplier,
    plus the rounding of the n + 1 coefficients to 2N = 2048 steps: each is uniform on a step, and the mask coefficients count
    where the key bit is one -- (1 + ones) / 12 / 2048^2.  Distance to the nearest decision boundary over the standard
    deviation, with the offset at 4 of its own standard deviations against the gate."""
    from test_golden_cpu import predicted_gate_output_noise
    p = ia.default_params()
    V, offset_sd = predicted_gate_output_noise(p)
    delta = 4 * offset_sd
    rounding = (1 + p.n / 2) / 12.0 / (2.0 * p.N) ** 2
    assert abs(V - 1.05e-5) < 0.03e-5 and abs(offset_sd - 1.2e-3) < 0.05e-3 and abs(rounding - 6.3e-6) < 0.1e-6

    def sigmas(margin, multiplier, wires):
        return (margin - multiplier * wires * delta) / np.sqrt(multiplier ** 2 * wires * V + rounding)

    maj3, xor3 = sigmas(1 / 8, 1, 3), sigmas(1 / 4, 2, 3)
    and2, xor2 = sigmas(1 / 8, 1, 2), sigmas(1 / 4, 2, 2)
    assert abs(maj3 - 18) < 0.6 and abs(xor3 - 19) < 0.6 and abs(and2 - 22) < 0.6 and abs(xor2 - 24) < 0.6
    assert maj3 >= 15 and xor3 >= 15
    assert maj3 >= 0.75 * and2 and xor3 >= 0.75 * and2
    # the same wire three times adds its noise coherently: why netlists refuse a repeated wire
    # (about 13 sigma before the offset is taken off, 11 after)
    assert 12 < (1 / 4) / np.sqrt(36 * V + rounding) < 14 and (1 / 4 - 6 * delta) / np.sqrt(36 * V + rounding) < 0.65 * xor3
