"""Random gate netlists for the wire store and the level executor, and the references they are checked against.

generate(seed, family) records a small DAG through ieache_amd.Netlist; each family aims at one way slot allocation, level
layout or the executor's piece cutting can go wrong.  walk_bits() is the plain wire-by-wire truth-table walk (no slots, no
levels); oracle_netlist() walks the same gate list on ciphertexts, one libtfhe gate after the other.  corpus(params) is the
fixed list of (seed, family) the CPU and GPU tests share.  Plain Python: no fixtures, no GPU."""
import numpy as np

FAMILIES = ("window", "long_lived", "dead", "mux_only", "mixed", "same_wire", "constants", "empty")
MAX_INPUTS, MAX_GATES, MAX_OUTPUTS = 6, 40, 7
FALSE, TRUE = -2, -1
MUX = 4
TWO_INPUT_TYPES = (0, 1, 2, 3, 5, 6, 7, 8, 9, 10)

TWO_INPUT = {0: "and", 1: "xor", 2: "or", 3: "nand"}
# libtfhe boot-gates.cpp: (constant term, multiplier of ca, multiplier of cb) of the gates the oracle has no entry point for
LINEAR = {5: (-1 << 29, -1, -1), 6: (-2 << 29, -2, -2), 7: (-1 << 29, -1, 1), 8: (-1 << 29, 1, -1), 9: (1 << 29, -1, 1), 10: (1 << 29, 1, -1)}

TRUTH = {0: lambda a, b: a & b, 1: lambda a, b: a ^ b, 2: lambda a, b: a | b, 3: lambda a, b: 1 - (a & b), 5: lambda a, b: 1 - (a | b),
         6: lambda a, b: 1 - (a ^ b), 7: lambda a, b: (1 - a) & b, 8: lambda a, b: a & (1 - b), 9: lambda a, b: (1 - a) | b,
         10: lambda a, b: a | (1 - b)}


# ---- ciphertext reference ----

def _neg(row):
    return (0 - row.view(np.uint32)).view(np.int32)


def oracle_gate(ck, t, a, b, c=None):
    if t in TWO_INPUT:
        return ck.gate(TWO_INPUT[t], a, b)
    if t == 4:
        return ck.mux(a, b, c)
    cst, ka, kb = LINEAR[t]
    x = (np.uint32(ka & 0xFFFFFFFF) * a.view(np.uint32) + np.uint32(kb & 0xFFFFFFFF) * b.view(np.uint32)).astype(np.uint32)
    x[-1:] += np.uint32(cst & 0xFFFFFFFF)
    return ck.bootstrap(x.view(np.int32))


def oracle_netlist(kb, cn, rows):
    """The compiled netlist `cn` on one expression's input rows, one libtfhe gate after the other."""
    ck = kb.ck
    wires = [np.ascontiguousarray(r) for r in rows]

    def ref(r):
        if r < 0:
            return ck.constant(1 if r == -1 else 0)
        return _neg(wires[r >> 1]) if r & 1 else wires[r >> 1]

    for t, a, b, c in cn.gates:
        wires.append(oracle_gate(ck, t, ref(a), ref(b), ref(c) if t == 4 else None))
    return np.stack([ref(o) for o in cn.outputs])


# ---- plaintext reference ----

def walk_bits(n_inputs, gates, outputs, in_bits):
    """Output bits of the recorded gate list on one vector of input bits: every wire computed once, in recording order."""
    wires = [int(v) & 1 for v in in_bits]
    assert len(wires) == n_inputs

    def ref(r):
        if r < 0:
            return 1 if r == TRUE else 0
        return wires[r >> 1] ^ (r & 1)

    for t, a, b, c in gates:
        wires.append((ref(b) if ref(a) else ref(c)) if t == MUX else TRUTH[t](ref(a), ref(b)))
    return np.array([ref(o) for o in outputs], dtype=np.uint8)


def all_input_bits(n_inputs):
    return np.array([[(v >> i) & 1 for i in range(n_inputs)] for v in range(1 << n_inputs)], dtype=np.uint8)


# ---- structure of a recorded gate list, computed without the product ----

def operands(gate):
    t, a, b, c = gate
    return (a, b, c) if t == MUX else (a, b)


def wire_levels(n_inputs, gates):
    """ASAP level of every wire (inputs 0)."""
    level = [0] * n_inputs
    for g in gates:
        level.append(1 + max([level[r >> 1] for r in operands(g) if r >= 0] or [0]))
    return level


def properties(n_inputs, gates, outputs):
    """What a case exercises, from its recorded gates alone."""
    level = wire_levels(n_inputs, gates)
    read = set(r >> 1 for g in gates for r in operands(g) if r >= 0)
    out_wires = set(o >> 1 for o in outputs if o >= 0)
    by_level = {}
    for i, g in enumerate(gates):
        by_level.setdefault(level[n_inputs + i], []).append(g[0])
    longest = 0
    for i, g in enumerate(gates):
        for r in operands(g):
            if r >= 0:
                longest = max(longest, level[n_inputs + i] - level[r >> 1])
    return {
        "gates": len(gates),
        "depth": max(level) if gates else 0,
        "mux_only_level": any(all(t == MUX for t in ts) for ts in by_level.values()),
        "dead_gate": any(n_inputs + i not in read and n_inputs + i not in out_wires for i in range(len(gates))),
        "unread_input": any(w not in read for w in range(n_inputs)),
        "unread_input_is_output": any(w not in read and w in out_wires for w in range(n_inputs)),
        "level1_output_nobody_reads": any(level[n_inputs + i] == 1 and n_inputs + i in out_wires and n_inputs + i not in read
                                          for i in range(len(gates))),
        "longest_life": longest,  # levels between a wire's production and its last read by a gate
        "same_wire_gate": any(len(set(r >> 1 for r in operands(g) if r >= 0)) < sum(r >= 0 for r in operands(g)) for g in gates),
        "two_constant_gate": any(sum(r < 0 for r in operands(g)) >= 2 for g in gates),
        "types": set(g[0] for g in gates),
        "negated_operand": any(r >= 0 and r & 1 for g in gates for r in operands(g)),
    }


# ---- the generator ----

class _Recorder:
    def __init__(self, rng, n_inputs):
        from ieache_amd import Netlist
        self.rng, self.nl, self.n_inputs = rng, Netlist(n_inputs), n_inputs
        self.gates = []

    @property
    def n_wires(self):
        return self.n_inputs + len(self.gates)

    def gate(self, t, a, b, c=0):
        assert len(self.gates) < MAX_GATES
        a, b, c = int(a), int(b), int(c) if t == MUX else 0
        self.gates.append((int(t), a, b, c))
        return self.nl.gate(t, a, b, c)

    def signed(self, wire, p_neg=0.3):
        return (int(wire) << 1) | int(self.rng.random() < p_neg)

    def any_type(self, p_mux=0.25):
        return MUX if self.rng.random() < p_mux else int(self.rng.choice(TWO_INPUT_TYPES))

    def from_pool(self, pool, t=None, p_neg=0.3):
        t = self.any_type() if t is None else t
        return self.gate(t, *(self.signed(self.rng.choice(pool), p_neg) for _ in range(3 if t == MUX else 2)))

    def finish(self, outputs):
        outputs = [int(o) for o in outputs][:MAX_OUTPUTS]
        assert 1 <= len(outputs) and len(self.gates) <= MAX_GATES and self.n_inputs <= MAX_INPUTS
        return self.nl, list(self.gates), outputs


def _usual_outputs(r, keep=()):
    """The last wires, one of them twice and once negated, an input, a constant -- after the ones the family insists on."""
    rng, last = r.rng, r.n_wires - 1
    outs = list(keep)
    outs += [last << 1, (last << 1) | 1, last << 1]
    outs += [r.signed(rng.integers(0, r.n_inputs)), TRUE if rng.random() < 0.5 else FALSE]
    while len(outs) < MAX_OUTPUTS:
        outs.append(r.signed(rng.integers(r.n_inputs, r.n_wires)))
    return outs


def _window(r):
    # deep and narrow: every operand among the last few wires, so slots are recycled level after level
    n_gates, width = int(r.rng.integers(28, MAX_GATES + 1)), int(r.rng.integers(2, 4))
    for _ in range(n_gates):
        r.from_pool(np.arange(max(0, r.n_wires - width), r.n_wires), t=r.any_type(0.15))
    return _usual_outputs(r)


def _long_lived(r):
    # one operand keeps the circuit deep, the others come from anywhere: wires are read many levels after they are made
    for _ in range(int(r.rng.integers(24, MAX_GATES + 1))):
        t = r.any_type(0.2)
        ops = [r.signed(r.n_wires - 1 - int(r.rng.integers(0, 2)))] + [r.signed(r.rng.integers(0, r.n_wires)) for _ in range(2 if t == MUX else 1)]
        r.rng.shuffle(ops)
        r.gate(t, *ops)
    return _usual_outputs(r)


def _dead(r):
    # the last input is read by nobody and is an output; the one before is read by nobody at all.  Gate 0 sits in level 1, is
    # an output and nothing else: its slot has to survive every later level.  Some later gates are read by nobody.
    live_inputs = list(range(r.n_inputs - 2))
    first = r.gate(int(r.rng.choice(TWO_INPUT_TYPES)), r.signed(live_inputs[0]), r.signed(live_inputs[-1]))
    pool, dead = list(live_inputs), []
    for _ in range(int(r.rng.integers(24, MAX_GATES))):
        w = r.from_pool(np.array(pool[-4:] + pool[:2]), t=r.any_type(0.2)) >> 1
        if r.rng.random() < 0.3:
            dead.append(w)  # nobody will read it
        else:
            pool.append(w)
    assert dead
    return _usual_outputs(r, keep=[first, ((r.n_inputs - 1) << 1) | int(r.rng.integers(0, 2))])


def _mux_only(r):
    for _ in range(int(r.rng.integers(20, MAX_GATES + 1))):
        ops = [r.signed(r.rng.integers(max(0, r.n_wires - 8), r.n_wires)) for _ in range(3)]
        if r.rng.random() < 0.15:
            ops[int(r.rng.integers(0, 3))] = TRUE if r.rng.random() < 0.5 else FALSE
        r.gate(MUX, *ops)
    return _usual_outputs(r)


def _mixed(r):
    # every one of the eleven types at least once, in random order, then anything
    types = list(TWO_INPUT_TYPES) + [MUX, MUX]
    r.rng.shuffle(types)
    types += [r.any_type(0.3) for _ in range(int(r.rng.integers(15, MAX_GATES - len(types) + 1)))]
    for t in types:
        r.from_pool(np.arange(max(0, r.n_wires - 16), r.n_wires), t=t, p_neg=0.5)
    return _usual_outputs(r)


def _same_wire(r):
    rng = r.rng
    for k in range(int(rng.integers(20, MAX_GATES + 1))):
        a = int(rng.integers(max(0, r.n_wires - 6), r.n_wires))
        b = int(rng.integers(0, r.n_wires))
        form = k % 6
        if form == 0:    # gate(a, a), either sign
            s = r.signed(a)
            r.gate(int(rng.choice(TWO_INPUT_TYPES)), s, s)
        elif form == 1:  # gate(a, NOT a)
            s = r.signed(a)
            r.gate(int(rng.choice(TWO_INPUT_TYPES)), s, s ^ 1)
        elif form == 2:  # MUX(a, a, a)
            r.gate(MUX, a << 1, a << 1, r.signed(a))
        elif form == 3:  # MUX(a, b, b)
            s = r.signed(b)
            r.gate(MUX, r.signed(a), s, s)
        elif form == 4:  # MUX(a, a, b) / MUX(a, b, a)
            ops = [r.signed(a), r.signed(b)]
            r.gate(MUX, a << 1, *(ops if rng.random() < 0.5 else ops[::-1]))
        else:
            r.from_pool(np.arange(max(0, r.n_wires - 6), r.n_wires))
    return _usual_outputs(r)


def _constants(r):
    rng = r.rng
    const = lambda: TRUE if rng.random() < 0.5 else FALSE  # noqa: E731
    wire = lambda: r.signed(rng.integers(max(0, r.n_wires - 6), r.n_wires))  # noqa: E731
    for k in range(int(rng.integers(22, MAX_GATES + 1))):
        form = k % 8
        t2 = int(rng.choice(TWO_INPUT_TYPES))
        if form == 0:
            r.gate(t2, const(), wire())
        elif form == 1:
            r.gate(t2, wire(), const())
        elif form == 2:
            r.gate(t2, const(), const())
        elif form == 3:
            r.gate(MUX, const(), wire(), wire())
        elif form == 4:
            r.gate(MUX, wire(), const(), wire())
        elif form == 5:
            r.gate(MUX, wire(), wire(), const())
        elif form == 6:
            r.gate(MUX, *[(const(), const(), wire()), (wire(), const(), const()), (const(), const(), const())][int(rng.integers(0, 3))])
        else:
            r.from_pool(np.arange(max(0, r.n_wires - 6), r.n_wires))
    return _usual_outputs(r, keep=[TRUE, FALSE])


def _empty(r):
    outs = [0, 1, TRUE, FALSE, ((r.n_inputs - 1) << 1) | 1, (r.n_inputs - 1) << 1]
    outs.append(r.signed(r.rng.integers(0, r.n_inputs)))
    return outs


_BUILDERS = {"window": (_window, 2, 4), "long_lived": (_long_lived, 4, 6), "dead": (_dead, 5, 6), "mux_only": (_mux_only, 3, 5),
             "mixed": (_mixed, 3, 6), "same_wire": (_same_wire, 2, 4), "constants": (_constants, 2, 4), "empty": (_empty, 1, 6)}
assert tuple(_BUILDERS) == FAMILIES


def generate(seed, family):
    """-> (ieache_amd.Netlist, recorded gates [(type, a, b, c)], output references).  At most 6 inputs, 40 gates, 7 outputs;
    the same (seed, family) always gives the same netlist."""
    rng = np.random.default_rng(seed)
    build, lo, hi = _BUILDERS[family]
    r = _Recorder(rng, int(rng.integers(lo, hi + 1)))
    return r.finish(build(r))


# ---- the cases the CPU and the GPU tests share ----

BATCH = 8


def corpus(params):
    """The fixed (seed, family) list for a parameter set (n, N): 24 cases on the any-parameter kernels, 6 on the 64-lane ones."""
    if tuple(params) == (5, 64):
        return [(1000 + 10 * k + i, f) for i in range(3) for k, f in enumerate(FAMILIES)]
    if tuple(params) == (16, 1024):
        return [(2000 + k, f) for k, f in enumerate(("mixed", "mux_only", "dead", "long_lived", "window", "constants"))]
    raise KeyError(params)


def compared_with_oracle(params):
    """Expressions of the batch the GPU test compares word for word with oracle_netlist (a libtfhe gate takes the CPU 13 ms at
    (16, 1024): there the others are compared with the default run)."""
    return tuple(range(BATCH)) if tuple(params) == (5, 64) else (0, BATCH - 1)


def case_inputs(kb, seed, n_inputs):
    """-> (bits [BATCH][n_inputs], their encryptions): what both tests feed case `seed`."""
    bits = np.random.default_rng([seed, 77]).integers(0, 2, size=(BATCH, n_inputs)).astype(np.uint8)
    return bits, kb.enc(bits, seed)
