"""Word programs on the GPU: a one-instruction program is the built-in kind's ciphertext, independent operators of one program
share levels, every expression equals a walk of the exported gate list on the untouched CPU oracle, and a compiled program goes
through every route a netlist goes through.  The oracle walk is random_netlists.oracle_netlist with the two three-input gates
(test_three_input_gates_gpu.oracle_netlist3): the compressors of SUM are MAJ3 / XOR3."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from random_netlists import _neg, oracle_gate
from test_three_input_gates_gpu import COMBINATION, combination, oracle_netlist3

pytestmark = pytest.mark.gpu

KS, FA = 1, 3


def encrypt_values(kb, widths, values, seed):
    """values [batch][len(widths)] integers -> (input bits [batch][sum(widths)], their encryptions)"""
    bits = np.array([[(v >> j) & 1 for v, w in zip(row, widths) for j in range(w)] for row in values], dtype=np.uint8)
    return bits, kb.enc(bits, seed)


def random_values(widths, batch, seed):
    rng = np.random.default_rng(seed)
    return [[int(rng.integers(0, 1 << min(w, 62))) for w in widths] for _ in range(batch)]


def decrypted_ints(kb, out, widths):
    """output rows [batch][sum(widths)] -> [batch][len(widths)] integers"""
    dec = kb.dec(out)
    res = []
    for row in dec:
        vals, at = [], 0
        for w in widths:
            vals.append(sum(int(b) << j for j, b in enumerate(row[at:at + w])))
            at += w
        res.append(vals)
    return res


# ---- anchor on the card ----

def test_one_instruction_programs_give_the_builtin_ciphertext(ia, gpu_ctx):
    kb, ctx = gpu_ctx(4, 1024)
    for kind, op, bits in ((ia.CIRC_ADD, "add", 8), (ia.CIRC_SUB, "sub", 8), (ia.CIRC_MUL, "mul", 32)):
        p = ia.WordProgram()
        a, b, carry = p.input(bits), p.input(bits), p.input(32)
        compiled = p.compile([getattr(p, op)(a, b, carry)])
        _, inp = encrypt_values(kb, (bits, bits, 32), random_values((bits, bits, 32), 3, [kind, bits]), 11 + kind)
        st, sk = ia.Stats(), ia.Stats()
        assert np.array_equal(ctx.eval_netlist(compiled, inp, st), ctx.eval_batch(kind, bits, inp, sk)), op
        assert st.bootstraps == sk.bootstraps == 3 * compiled.info().bootstraps
    p = ia.WordProgram()  # (A + B) - C is the chain kind
    a, b, carry, c = p.input(8), p.input(8), p.input(32), p.input(8)
    compiled = p.compile([p.sub(p.add(a, b, carry), c, carry)])
    _, inp = encrypt_values(kb, (8, 8, 32, 8), random_values((8, 8, 32, 8), 3, 5), 21)
    assert np.array_equal(ctx.eval_netlist(compiled, inp), ctx.eval_batch(ia.circ_chain(ia.CIRC_ADD, ia.CIRC_SUB), 8, inp))


# ---- parallel branches ----

def test_independent_products_share_levels(ia, gpu_ctx):
    """a*b + c*d as one program against its three built-in calls chained by hand: the same words, the same bootstraps, and
    fewer levels than the three calls one after the other -- the two products run side by side and the addition starts on
    their low words while the high ones are still being made."""
    kb, ctx = gpu_ctx(4, 1024)
    p = ia.WordProgram()
    a, b, c, d, carry = (p.input(32) for _ in range(5))
    compiled = p.compile([p.add(p.mul(a, b, carry), p.mul(c, d, carry), carry)])
    values = [[0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0], [123456789, 987654321, 55555, 4000000000, 0]]
    _, inp = encrypt_values(kb, (32,) * 5, values, 31)
    A, B, Cc, D, cy = (inp[:, 32 * i:32 * (i + 1)] for i in range(5))
    s1, s2, s3, st = ia.Stats(), ia.Stats(), ia.Stats(), ia.Stats()
    ab = ctx.eval_batch(ia.CIRC_MUL, 32, np.concatenate([A, B, cy], axis=1), s1)
    cd = ctx.eval_batch(ia.CIRC_MUL, 32, np.concatenate([Cc, D, cy], axis=1), s2)
    want = ctx.eval_batch(ia.CIRC_ADD, 64, np.concatenate([ab, cd, cy], axis=1), s3)
    got = ctx.eval_netlist(compiled, inp, st)
    assert np.array_equal(got, want)
    assert st.bootstraps == s1.bootstraps + s2.bootstraps + s3.bootstraps
    assert max(s1.levels, s2.levels, s3.levels) <= st.levels < s1.levels + s2.levels + s3.levels, (st.levels, s1.levels, s3.levels)
    assert decrypted_ints(kb, got, (64,)) == [[(r[0] * r[1] + r[2] * r[3]) % (1 << 64)] for r in values]


# ---- against the oracle, gate by gate ----

_programs = {}


def oracle_programs(ia):
    """name -> (compiled program, input widths, output widths, f(values) -> expected output integers): compiled once"""
    if _programs:
        return _programs
    for name, family in (("sum5_fa", FA), ("sum5_ks", KS)):
        p = ia.WordProgram()
        xs = [p.input(6) for _ in range(5)]
        _programs[name] = (p.compile([p.sum(xs, 9, family=family)]), (6,) * 5, (9,), lambda v: [sum(v) % 512])
    p = ia.WordProgram()
    a, b, c = p.input(6), p.input(6), p.input(6)
    _programs["max_of_sum"] = (p.compile([p.maximum(a + b, c)]), (6, 6, 6), (6,), lambda v: [max((v[0] + v[1]) % 64, v[2])])
    p = ia.WordProgram()
    a, b, s, c, d = p.input(4), p.input(4), p.input(1), p.input(4), p.input(4)
    outs = [a.lt(b), a.eq(b), p.select(s, a, b), p.dot([(a, b), (c, d)], 8)]
    _programs["compare_select_dot"] = (p.compile(outs), (4, 4, 1, 4, 4), (1, 1, 4, 8),
                                       lambda v: [int(v[0] < v[1]), int(v[0] == v[1]), v[0] if v[2] else v[1], (v[0] * v[1] + v[3] * v[4]) % 256])
    return _programs


PROGRAM_NAMES = ("sum5_fa", "sum5_ks", "max_of_sum", "compare_select_dot")


@pytest.mark.parametrize("name", PROGRAM_NAMES)
@pytest.mark.parametrize("n,N,compared", [(5, 64, (0, 1, 2, 3)), (4, 1024, (0, 3))])
def test_every_expression_equals_the_oracle_walk(ia, gpu_ctx, n, N, compared, name):
    kb, ctx = gpu_ctx(n, N)
    compiled, widths, out_widths, expect = oracle_programs(ia)[name]
    values = random_values(widths, 4, [len(name), n])
    values[1] = [(1 << w) - 1 for w in widths]  # every carry there is
    if name == "compare_select_dot":
        values[2][1] = values[2][0]  # equal operands
    _, inp = encrypt_values(kb, widths, values, 41 + n)
    out = ctx.eval_netlist(compiled, inp)
    with ThreadPoolExecutor(4) as ex:
        ref = list(ex.map(lambda e: oracle_netlist3(kb, compiled, inp[e]), compared))
    for e, r in zip(compared, ref):
        assert np.array_equal(out[e], r), (name, e)
    assert decrypted_ints(kb, out, out_widths) == [expect(v) for v in values]


# ---- every route a netlist takes ----

def test_a_program_through_jobs_group_chunks_and_level_halves(ia, gpu_ctx):
    kb, ctx = gpu_ctx(4, 1024)
    compiled, widths, out_widths, expect = oracle_programs(ia)["max_of_sum"]
    values = random_values(widths, 6, 61)
    _, inp = encrypt_values(kb, widths, values, 62)
    ref = ctx.eval_netlist(compiled, inp)
    assert decrypted_ints(kb, ref, out_widths) == [expect(v) for v in values]
    # one program and one built-in kind in ONE joint call
    _, add_in = encrypt_values(kb, (8, 8, 32), random_values((8, 8, 32), 3, 63), 64)
    add_ref = ctx.eval_batch(ia.CIRC_ADD, 8, add_in)
    st = ia.Stats()
    joint = ctx.eval_jobs([(compiled, inp), (ia.CIRC_ADD, 8, add_in)], st)
    assert np.array_equal(joint[0], ref) and np.array_equal(joint[1], add_ref)
    assert st.bootstraps == 6 * compiled.info().bootstraps + 3 * ia.circuit_info(ia.CIRC_ADD, 8).bootstraps
    # two members on one card
    with ia.Group.from_arrays(kb.p, kb.bk, kb.ksk, (0, 0)) as g:
        assert np.array_equal(g.eval_netlist(compiled, inp), ref)
    saved = {k: ctx.get_option(k) for k in ("chunk", "overlap", "overlap_min")}
    try:
        ctx.set_option("overlap", 0)
        ctx.set_option("chunk", 7)  # pieces of 7 rotation items: levels are cut, and a MUX (two items) lies across two pieces
        st = ia.Stats()
        assert np.array_equal(ctx.eval_netlist(compiled, inp, st), ref) and st.chunks > st.levels
        ctx.set_option("chunk", saved["chunk"])
        ctx.set_option("overlap", 1)
        ctx.set_option("overlap_min", 4)
        halves = ctx.get_option("overlapped_levels")
        assert np.array_equal(ctx.eval_netlist(compiled, inp), ref) and ctx.get_option("overlapped_levels") > halves
    finally:
        for k, v in saved.items():
            ctx.set_option(k, v)


# ---- at the product parameters ----

def oracle_walk_by_levels(kb, walks, pool):
    """oracle_netlist3 for several (compiled, input rows) at once, level by level, the gates of a level on `pool`: a gate of the
    oracle at n = 630 takes the CPU half a second, and the gates of one level are independent."""
    ck = kb.ck
    state = []
    for compiled, rows in walks:
        level = [0] * compiled.n_inputs  # ASAP level of every wire
        for t, a, b, c in compiled.gates:
            read = (a, b, c) if t == 4 or t in COMBINATION else (a, b)
            level.append(1 + max([level[r >> 1] for r in read if r >= 0] or [0]))
        wires = [np.ascontiguousarray(r) for r in rows] + [None] * len(compiled.gates)
        state.append((compiled, wires, level))

    def ref(wires, r):
        if r < 0:
            return ck.constant(1 if r == -1 else 0)
        return _neg(wires[r >> 1]) if r & 1 else wires[r >> 1]

    def run(job):
        wires, (t, a, b, c) = job
        if t in COMBINATION:
            return ck.bootstrap(combination(t, ref(wires, a), ref(wires, b), ref(wires, c)))
        return oracle_gate(ck, t, ref(wires, a), ref(wires, b), ref(wires, c) if t == 4 else None)

    for L in range(1, max(max(lv) for _, _, lv in state) + 1):
        jobs = [(wires, g, compiled.n_inputs + i) for compiled, wires, lv in state for i, g in enumerate(compiled.gates)
                if lv[compiled.n_inputs + i] == L]
        for (wires, _, w), row in zip(jobs, pool.map(run, [(j[0], j[1]) for j in jobs])):
            wires[w] = row
    return [np.stack([ref(wires, o) for o in compiled.outputs]) for compiled, wires, _ in state]


def test_sum_and_maximum_at_product_parameters(ia, gpu_ctx):
    """n = 630, N = 1024: the sum of four 8-bit operands (10 bits, full-adder tail) and maximum(a + b, c) at 8 bits on full
    adders, two expressions each: no wrong decryption, and expression 0 of both word for word the oracle's walk of the export.
    52 + 40 = 92 gates per expression (108 blind rotations: 16 of the gates are MUX)."""
    kb, ctx = gpu_ctx(630, 1024)
    p = ia.WordProgram()
    total = p.compile([p.sum([p.input(8) for _ in range(4)], 10)])
    q = ia.WordProgram(family=FA)
    a, b, c = q.input(8), q.input(8), q.input(8)
    largest = q.compile([q.maximum(a + b, c)])
    assert len(total.gates) + len(largest.gates) == N_GATES_AT_PRODUCT_PARAMETERS < 400
    sum_values = [[255, 255, 255, 255], [200, 17, 96, 3]]
    max_values = [[200, 100, 43], [7, 8, 250]]
    _, sum_in = encrypt_values(kb, (8,) * 4, sum_values, 71)
    _, max_in = encrypt_values(kb, (8,) * 3, max_values, 72)
    sum_out, max_out = ctx.eval_netlist(total, sum_in), ctx.eval_netlist(largest, max_in)
    assert decrypted_ints(kb, sum_out, (10,)) == [[sum(v)] for v in sum_values]
    assert decrypted_ints(kb, max_out, (8,)) == [[max((v[0] + v[1]) % 256, v[2])] for v in max_values]
    with ThreadPoolExecutor(16) as pool:
        sum_ref, max_ref = oracle_walk_by_levels(kb, [(total, sum_in[0]), (largest, max_in[0])], pool)
    assert np.array_equal(sum_out[0], sum_ref) and np.array_equal(max_out[0], max_ref)


N_GATES_AT_PRODUCT_PARAMETERS = 92
