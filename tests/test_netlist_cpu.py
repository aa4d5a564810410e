"""Caller-defined netlists on the host: the C ABI's create / info / simulate / destroy, validation, the worked examples of
ieache_amd.netlists against Python integers, and the built-in circuits' statistics, which the new gate types must not move."""
import ctypes as C
import itertools

import numpy as np
import pytest


def test_symbols_and_a_hand_written_netlist(ia):
    L = ia.lib()
    for name in ("ieache_netlist_create", "ieache_netlist_destroy", "ieache_netlist_info", "ieache_netlist_simulate",
                 "ieache_prepare_netlist", "ieache_eval_netlist", "ieache_eval_netlist_device"):
        assert hasattr(L, name), name
    assert (ia.GATE_MUX, ia.GATE_NOR, ia.GATE_XNOR, ia.GATE_ANDNY, ia.GATE_ANDYN, ia.GATE_ORNY, ia.GATE_ORYN) == (4, 5, 6, 7, 8, 9, 10)
    # eight gates, through the C ABI itself.  Wires: inputs 0..2, gates 3..10
    W = lambda w: w << 1  # noqa: E731  IEACHE_NET_WIRE
    gates = np.array([
        (ia.GATE_XNOR, W(0), W(1), 0),        # 3  level 1
        (ia.GATE_AND, W(0) ^ 1, W(2), 0),     # 4  level 1
        (ia.GATE_MUX, W(3), W(2), W(4) ^ 1),  # 5  level 2 (2 rotations)
        (ia.GATE_NOR, W(3), W(4), 0),         # 6  level 2
        (ia.GATE_MUX, W(5), W(6), -1),        # 7  level 3 (2 rotations)
        (ia.GATE_ORYN, W(5), W(0), 0),        # 8  level 3
        (ia.GATE_XOR, W(6), -2, 0),           # 9  level 3
        (ia.GATE_MUX, W(7), W(8), W(9)),      # 10 level 4 (2 rotations)
    ], dtype=np.int32)
    outs = np.array([W(10), W(7) ^ 1, W(1), -1], dtype=np.int32)
    i32p = C.POINTER(C.c_int32)
    h = L.ieache_netlist_create(3, gates.ctypes.data_as(C.c_void_p), 8, outs.ctypes.data_as(i32p), 4, 0)
    assert h, L.ieache_last_error()
    try:
        info, by_type = ia.CircuitInfo(), (C.c_int64 * 11)()
        assert L.ieache_netlist_info(h, C.byref(info), by_type) == 0
        assert (info.n_inputs, info.n_outputs, info.depth, info.sched_levels) == (3, 4, 4, 4)
        # in blind rotations: levels of 2, 3, 4, 2
        assert info.bootstraps == 11 and info.reference_bootstraps == 11 and info.max_width == 4 and info.sched_max_width == 4
        assert list(by_type) == [1, 1, 0, 0, 3, 1, 1, 0, 0, 0, 1]
        assert info.n_and == 2 and info.n_xor == 1  # the NOR runs as an AND of negated operands
        u8p = C.POINTER(C.c_uint8)
        for v in range(8):
            a, b, c = v & 1, (v >> 1) & 1, (v >> 2) & 1
            g3, g4 = 1 - (a ^ b), (1 - a) & c
            g5, g6 = (c if g3 else 1 - g4), 1 - (g3 | g4)
            g7, g8, g9 = (g6 if g5 else 1), g5 | (1 - a), g6
            g10 = g8 if g7 else g9
            bits, out = np.array([a, b, c], dtype=np.uint8), np.zeros(4, dtype=np.uint8)
            assert L.ieache_netlist_simulate(h, bits.ctypes.data_as(u8p), out.ctypes.data_as(u8p)) == 0
            assert list(out) == [g10, 1 - g7, b, 1], v
    finally:
        L.ieache_netlist_destroy(h)
    L.ieache_netlist_destroy(None)


TRUTH = {0: lambda a, b: a & b, 1: lambda a, b: a ^ b, 2: lambda a, b: a | b, 3: lambda a, b: 1 - (a & b), 5: lambda a, b: 1 - (a | b),
         6: lambda a, b: 1 - (a ^ b), 7: lambda a, b: (1 - a) & b, 8: lambda a, b: a & (1 - b), 9: lambda a, b: (1 - a) | b,
         10: lambda a, b: a | (1 - b)}


def test_truth_tables_of_all_eleven_types(ia):
    nl = ia.Netlist(3)
    x = [nl.input(i) for i in range(3)]

    def operand_forms(ref, value):
        """(reference, function of the input bits) for a wire, its negation and both constants"""
        return [(ref, lambda v: v[value]), (ia.NOT(ref), lambda v: 1 - v[value]), (ia.TRUE, lambda v: 1), (ia.FALSE, lambda v: 0)]

    outs, expect = [], []
    for t, f in TRUTH.items():
        for (ra, fa), (rb, fb) in itertools.product(operand_forms(x[0], 0), operand_forms(x[1], 1)):
            outs.append(nl.gate(t, ra, rb))
            expect.append(lambda v, f=f, fa=fa, fb=fb: f(fa(v), fb(v)))
    for (ra, fa), (rb, fb), (rc, fc) in itertools.product(operand_forms(x[0], 0), operand_forms(x[1], 1), operand_forms(x[2], 2)):
        outs.append(nl.MUX(ra, rb, rc))
        expect.append(lambda v, fa=fa, fb=fb, fc=fc: fb(v) if fa(v) else fc(v))
    for balanced in (False, True):
        with nl.compile(outs, balanced=balanced) as cn:
            assert cn.info().bootstraps == 160 + 2 * 64 and cn.gates_by_type() == [16] * 4 + [64] + [16] * 6
            for v in itertools.product((0, 1), repeat=3):
                assert list(cn.simulate(v)) == [e(v) for e in expect], v


@pytest.mark.parametrize("gates,outputs,n_inputs,needle", [
    ([(0, 0, 3 << 1, 0)], [0], 3, "gate 0"),                        # refers to its own output
    ([(0, 0, 2, 0), (4, 0, 2, 5 << 1)], [0], 3, "gate 1"),          # third operand not defined yet
    ([(0, 0, 2, 0), (11, 0, 2, 0)], [0], 3, "gate 1"),              # type out of range
    ([(-1, 0, 2, 0)], [0], 3, "gate 0"),
    ([(0, 0, 2, 0), (1, 0, 2, 2)], [0], 3, "gate 1"),               # third operand on a two-input gate
    ([(0, 0, -3, 0)], [0], 3, "gate 0"),                            # not a reference
    ([(0, 0, 2, 0)], [4 << 1], 3, "gate 1"),                        # output out of range: names the first gate that does not exist
    ([], [-1], 0, "input"),
    ([(0, 0, 2, 0)], [], 3, "output"),
])
def test_validation_names_the_gate(ia, gates, outputs, n_inputs, needle):
    L = ia.lib()
    g = np.array(gates, dtype=np.int32).reshape(-1, 4)
    o = np.array(outputs, dtype=np.int32)
    h = L.ieache_netlist_create(n_inputs, g.ctypes.data_as(C.c_void_p), len(gates), o.ctypes.data_as(C.POINTER(C.c_int32)), len(outputs), 0)
    assert not h and needle in L.ieache_last_error().decode(), L.ieache_last_error()
    nl = ia.Netlist(n_inputs)
    for t, a, b, c in gates:
        nl.gate(t, a, b, c)
    with pytest.raises(ia.IeacheError) as e:
        nl.compile(outputs)
    assert e.value.code == -22 and needle in str(e.value)


def test_sizes_and_flags_are_checked_before_anything_is_read(ia):
    L = ia.lib()
    o = np.array([0], dtype=np.int32)
    op = o.ctypes.data_as(C.POINTER(C.c_int32))
    # 2^30 gates would overflow the wire numbering: refused on the count alone, naming the first gate without a wire number
    assert not L.ieache_netlist_create(3, o.ctypes.data_as(C.c_void_p), 1 << 30, op, 1, 0) and b"gate 1073741821" in L.ieache_last_error()
    assert not L.ieache_netlist_create(3, None, 0, op, 1, 2) and b"flag" in L.ieache_last_error()
    info = ia.CircuitInfo()
    assert L.ieache_netlist_info(None, C.byref(info), None) == -22


def _bits(v, n):
    return [(v >> i) & 1 for i in range(n)]


def _expected(name, a, b, n):
    if name == "compare":
        return [int(a < b), int(a == b)]
    if name == "minmax":
        return _bits(min(a, b), n) + _bits(max(a, b), n)
    q, r = divmod(a, b) if b else ((1 << n) - 1, a)
    return _bits(q, n) + _bits(r, n)


@pytest.mark.parametrize("name", ["compare", "minmax", "divmod"])
def test_worked_examples_against_python_integers(ia, name):
    from ieache_amd import netlists
    rng = np.random.default_rng(12)
    for n, pairs in ((4, list(itertools.product(range(16), repeat=2))),
                     (32, [(int(a), int(b)) for a, b in rng.integers(0, 1 << 32, size=(200, 2))] + [(7, 0), (0, 0), (1 << 31, 1 << 31)])):
        plain, balanced = getattr(netlists, name)(n), getattr(netlists, name)(n, balanced=True)
        pi, bi = plain.info(), balanced.info()
        assert pi.bootstraps == bi.bootstraps and pi.depth == bi.depth and bi.sched_max_width <= pi.sched_max_width == pi.max_width
        assert pi.bootstraps == sum(plain.gates_by_type()) + plain.gates_by_type()[ia.GATE_MUX]
        for a, b in pairs:
            bits = np.array(_bits(a, n) + _bits(b, n), dtype=np.uint8)
            want = _expected(name, a, b, n)
            assert list(plain.simulate(bits)) == want and list(balanced.simulate(bits)) == want, (n, a, b)
        # the reported ASAP depth and width, in blind rotations, are what the gate list gives when levelised by hand
        by_level = {}
        level = [0] * (plain.n_inputs + len(plain.gates))
        for g, (t, ra, rb, rc) in enumerate(plain.gates):
            lv = 1 + max([level[r >> 1] for r in ((ra, rb, rc) if t == ia.GATE_MUX else (ra, rb)) if r >= 0] or [0])
            level[plain.n_inputs + g] = lv
            by_level[lv] = by_level.get(lv, 0) + (2 if t == ia.GATE_MUX else 1)
        assert max(by_level) == pi.depth and max(by_level.values()) == pi.max_width
    assert netlists.minmax(32).info().bootstraps == 224 and netlists.compare(32).info().bootstraps == 128


def test_add_recorded_as_a_netlist_matches_the_built_in(ia):
    bits = 16
    nl = ia.Netlist(2 * bits + 32)
    carry, sums = nl.input(2 * bits), []
    for i in range(bits):  # Cloud/cloud.c: add()
        x, y = nl.input(i), nl.input(bits + i)
        axc = nl.XOR(x, carry)
        bxc = nl.XOR(y, carry)
        sums.append(nl.XOR(x, bxc))
        axc = nl.AND(axc, bxc)
        carry = nl.XOR(carry, axc)
    cn = nl.compile(sums)
    ref, got = ia.circuit_info(ia.CIRC_ADD, bits), cn.info()
    for f in ("n_inputs", "n_outputs", "n_slots", "depth", "max_width", "bootstraps", "n_and", "n_xor", "sched_max_width", "sched_levels"):
        assert getattr(ref, f) == getattr(got, f), f
    rng = np.random.default_rng(13)
    for _ in range(50):
        inb = np.zeros(2 * bits + 32, dtype=np.uint8)
        inb[:2 * bits + 1] = rng.integers(0, 2, size=2 * bits + 1)
        assert np.array_equal(cn.simulate(inb), ia.circuit_simulate(ia.CIRC_ADD, bits, inb))


# (kind, bits): (n_inputs, n_outputs, n_slots, depth, max_width, bootstraps, n_and, n_xor, sched_max_width, sched_levels), as computed
# before circuits could hold MUX / XNOR gates
BUILT_IN = {
    (1, 16): (64, 16, 64, 48, 2, 80, 16, 64, 2, 48),
    (1, 32): (96, 32, 96, 96, 2, 160, 32, 128, 2, 96),
    (1, 64): (160, 64, 160, 192, 2, 320, 64, 256, 2, 192),
    (1, 128): (288, 128, 288, 384, 2, 640, 128, 512, 2, 384),
    (2, 16): (64, 16, 64, 50, 4, 160, 32, 128, 4, 50),
    (2, 32): (96, 32, 96, 98, 4, 320, 64, 256, 4, 98),
    (2, 64): (160, 64, 160, 194, 4, 640, 128, 512, 4, 194),
    (2, 128): (288, 128, 288, 386, 4, 1280, 256, 1024, 4, 386),
    (3, 16): (64, 16, 64, 50, 4, 160, 32, 128, 4, 50),
    (3, 32): (96, 32, 96, 98, 4, 320, 64, 256, 4, 98),
    (3, 64): (160, 64, 160, 194, 4, 640, 128, 512, 4, 194),
    (3, 128): (288, 128, 288, 386, 4, 1280, 256, 1024, 4, 386),
    (4, 32): (96, 64, 1121, 255, 1056, 11264, 3072, 8192, 1056, 255),
    (4, 64): (160, 128, 1610, 449, 4160, 35296, 10336, 24960, 122, 449),
    (5, 32): (160, 64, 1186, 257, 1057, 11584, 3136, 8448, 1057, 257),
    (5, 64): (288, 128, 1770, 451, 4161, 35936, 10464, 25472, 124, 451),
    (6, 16): (64, 16, 88, 11, 32, 182, 100, 82, 32, 11),
    (6, 32): (96, 32, 194, 13, 64, 454, 260, 194, 64, 13),
    (6, 64): (160, 64, 418, 15, 128, 1094, 644, 450, 128, 15),
    (7, 16): (64, 16, 88, 11, 32, 182, 100, 82, 32, 11),
    (7, 32): (96, 32, 194, 13, 64, 454, 260, 194, 64, 13),
    (7, 64): (160, 64, 418, 15, 128, 1094, 644, 450, 128, 15),
    (8, 16): (64, 16, 88, 11, 32, 182, 100, 82, 32, 11),
    (8, 32): (96, 32, 194, 13, 64, 454, 260, 194, 64, 13),
    (8, 64): (160, 64, 418, 15, 128, 1094, 644, 450, 128, 15),
    (9, 32): (96, 64, 1654, 37, 1024, 6637, 3477, 3160, 1024, 37),
    (9, 64): (160, 128, 4572, 43, 4096, 25960, 13362, 12598, 1588, 43),
    (36, 16): (80, 16, 80, 50, 6, 240, 48, 192, 6, 50),
    (36, 32): (128, 32, 128, 98, 6, 480, 96, 384, 6, 98),
    (36, 64): (224, 64, 224, 194, 6, 960, 192, 768, 6, 194),
    (35, 32): (160, 64, 1186, 257, 1057, 11584, 3136, 8448, 1057, 257),
    (35, 64): (288, 128, 1770, 451, 4161, 35936, 10464, 25472, 124, 451),
    (61, 32): (160, 64, 899, 259, 82, 11584, 3136, 8448, 82, 259),
    (61, 64): (256, 128, 2231, 453, 169, 35936, 10464, 25472, 116, 453),
}


def test_built_in_circuits_are_unchanged(ia):
    for (kind, bits), want in BUILT_IN.items():
        i = ia.circuit_info(kind, bits)
        got = (i.n_inputs, i.n_outputs, i.n_slots, i.depth, i.max_width, i.bootstraps, i.n_and, i.n_xor, i.sched_max_width, i.sched_levels)
        assert got == want, (kind, bits)
