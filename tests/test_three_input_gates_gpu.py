"""The three-input gates MAJ3 / XOR3 on the GPU: flat calls, netlist levels under every way the executor cuts a level, the
full-adder circuit kinds, and the noise the gates see at the reference's parameters.  The reference is the untouched CPU oracle:
the gate's linear combination in numpy (as random_netlists.oracle_gate does for the gates libtfhe's entry points do not cover),
then the oracle's bootstrap."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from random_netlists import _neg, oracle_gate
from test_three_input_gates_cpu import ALL_BITS, EDGE32, TRUTH3, operand_forms

pytestmark = pytest.mark.gpu

MAJ3, XOR3 = 32, 33
COMBINATION = {MAJ3: (1, 0), XOR3: (2, 1 << 31)}  # multiplier of ca + cb + cc, constant term


def combination(t, a, b, c):
    """The sample a MAJ3 / XOR3 gate bootstraps, rows of n + 1."""
    k, cst = COMBINATION[t]
    x = (np.uint32(k) * (a.view(np.uint32) + b.view(np.uint32) + c.view(np.uint32))).astype(np.uint32)
    x[..., -1] += np.uint32(cst)
    return x.view(np.int32)


def oracle_gates3(ck, t, a, b, c):
    """Rows of gates through the oracle (its bootstrap is the code a single gate runs; independent rows go to host threads)."""
    x = np.ascontiguousarray(combination(t, a, b, c)).reshape(-1, a.shape[-1])
    if len(x) < 4:
        return np.stack([ck.bootstrap(r) for r in x]) if len(x) else x
    with ThreadPoolExecutor(16) as ex:
        return np.stack(list(ex.map(ck.bootstrap, x)))


def oracle_netlist3(kb, cn, rows):
    """random_netlists.oracle_netlist with the two new types: one expression, one oracle gate after the other."""
    ck = kb.ck
    wires = [np.ascontiguousarray(r) for r in rows]

    def ref(r):
        if r < 0:
            return ck.constant(1 if r == -1 else 0)
        return _neg(wires[r >> 1]) if r & 1 else wires[r >> 1]

    for t, a, b, c in cn.gates:
        if t in COMBINATION:
            wires.append(ck.bootstrap(combination(t, ref(a), ref(b), ref(c))))
        else:
            wires.append(oracle_gate(ck, t, ref(a), ref(b), ref(c) if t == 4 else None))
    return np.stack([ref(o) for o in cn.outputs])


def device_rows(ctx, rows):
    import torch
    d = torch.zeros((rows.shape[0], ctx.lwe_stride), dtype=torch.int32, device="cuda")
    d[:, : rows.shape[1]] = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    return d


# ---- flat calls ----

_flat = {}


def flat_case(kb):
    """All 8 input rows x 3 at the reference's parameters, and the oracle's outputs of both gates: computed once."""
    if "ref" not in _flat:
        bits = np.array(ALL_BITS * 3, dtype=np.uint8)  # [24][3]
        rows = [kb.enc(bits[:, i], 401 + i) for i in range(3)]
        _flat["bits"], _flat["rows"] = bits, rows
        _flat["ref"] = {t: oracle_gates3(kb.ck, t, *rows) for t in (MAJ3, XOR3)}
    return _flat["bits"], _flat["rows"], _flat["ref"]


@pytest.mark.parametrize("gate", [MAJ3, XOR3])
def test_flat_calls_word_for_word(ia, gpu_ctx, gate):
    kb, ctx = gpu_ctx(630, 1024)
    bits, (a, b, c), ref = flat_case(kb)
    st = ia.Stats()
    out = ctx.gates3(gate, a, b, c, st)
    assert np.array_equal(out, ref[gate])
    assert st.bootstraps == 24 and st.levels == 1 and st.keyswitch_launches == 1  # one rotation, one key-switch row per gate
    assert list(kb.dec(out)) == [TRUTH3[gate](*r) for r in bits]
    for i in (0, 23):
        assert np.array_equal(ctx.gates3(gate, a[i:i + 1], b[i:i + 1], c[i:i + 1]), ref[gate][i:i + 1]), i
    try:
        ctx.set_option("exact_fft", 1)
        assert np.array_equal(ctx.gates3(gate, a, b, c), ref[gate])
        assert np.array_equal(ctx.gates3(gate, a[:1], b[:1], c[:1]), ref[gate][:1])
    finally:
        ctx.set_option("exact_fft", 0)
    # count 0
    e = np.zeros((0, kb.p.n + 1), np.int32)
    st = ia.Stats()
    assert ctx.gates3(gate, e, e, e, st).shape == (0, kb.p.n + 1) and st.bootstraps == 0


@pytest.mark.parametrize("gate", [MAJ3, XOR3])
def test_flat_calls_in_place(ia, gpu_ctx, gate):
    """The output over each of the three operands: such a call cannot be repeated, so it runs on the two-limb kernels."""
    import torch
    kb, ctx = gpu_ctx(630, 1024)
    _, rows, ref = flat_case(kb)
    S = kb.p.n + 1
    for over in range(3):
        d = [device_rows(ctx, r) for r in rows]
        torch.cuda.synchronize()
        ctx.gates3_device(gate, 24, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[over].data_ptr())
        assert np.array_equal(d[over].cpu().numpy()[:, :S], ref[gate]), over
        for other in range(3):
            if other != over:
                assert np.array_equal(d[other].cpu().numpy()[:, :S], rows[other])
    d = [device_rows(ctx, r) for r in rows]
    with pytest.raises(ia.IeacheError, match="not a device pointer"):
        ctx.gates3_device(gate, 24, d[0].data_ptr(), d[1].data_ptr(), rows[2].ctypes.data, d[0].data_ptr())
    with pytest.raises(ia.IeacheError, match="three-input"):
        ctx.gates3_device(ia.GATE_AND, 24, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[0].data_ptr())
    with pytest.raises(ia.IeacheError):
        ctx.gates_device(gate, 24, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr())


@pytest.mark.parametrize("n,N,generic", [(6, 64, False), (4, 1024, True)])
def test_flat_calls_on_the_any_parameter_kernels(ia, gpu_ctx, n, N, generic):
    kb, ctx = gpu_ctx(n, N)
    bits = np.random.default_rng(40).integers(0, 2, size=(40, 3)).astype(np.uint8)
    a, b, c = (kb.enc(bits[:, i], 411 + i) for i in range(3))
    try:
        ctx.force_generic(generic)
        for gate in (MAJ3, XOR3):
            out = ctx.gates3(gate, a, b, c)
            assert np.array_equal(out, oracle_gates3(kb.ck, gate, a, b, c)), gate
            assert list(kb.dec(out)) == [TRUTH3[gate](*r) for r in bits]
    finally:
        ctx.force_generic(False)


# ---- netlists ----

def mixed_level_netlist(ia):
    """Level 1: MAJ3 and XOR3 with plain, negated and constant operands in every position, two-input gates and MUX gates.
    Level 2: a MUX fed by three-input gates, a three-input gate fed by a MUX and by three-input gates.  Level 3: one on both."""
    nl = ia.Netlist(3)
    a, b, c = nl.input(0), nl.input(1), nl.input(2)
    forms = operand_forms(ia, nl)
    outs, first = [], {}
    for i, f in enumerate(forms):  # interleaved, so that pieces of a level hold both types
        for t in (MAJ3, XOR3) if i % 2 else (XOR3, MAJ3):
            first.setdefault(t, len(outs))
            outs.append(nl.gate(t, *f))
        if i % 5 == 0:
            outs.append(nl.gate((0, 1, 6, 9)[i // 5 % 4], f[0], f[1]))
    m1 = nl.MUX(a, b, ia.NOT(c))
    m2 = nl.MUX(ia.NOT(c), ia.TRUE, a)
    maj, xor = outs[first[MAJ3]], outs[first[XOR3]]
    fed = nl.MUX(maj, ia.NOT(xor), m1)
    deep = nl.XOR3(m2, ia.NOT(maj), xor)
    deep2 = nl.MAJ3(deep, fed, ia.FALSE)
    return nl.compile(outs + [m1, m2, fed, deep, deep2]), forms


_net = {}


def netlist_case(ia, kb, ctx):
    if "ref" not in _net:
        cn, forms = mixed_level_netlist(ia)
        bits = np.array(ALL_BITS, dtype=np.uint8)
        inp = kb.enc(bits, 421)
        with ThreadPoolExecutor(8) as ex:
            ref = np.stack(list(ex.map(lambda e: oracle_netlist3(kb, cn, inp[e]), range(8))))
        _net.update(cn=cn, forms=forms, bits=bits, inp=inp, ref=ref)
    return _net["cn"], _net["bits"], _net["inp"], _net["ref"]


def test_netlist_levels_word_for_word_however_they_are_cut(ia, gpu_ctx):
    kb, ctx = gpu_ctx(4, 1024)
    cn, bits, inp, ref = netlist_case(ia, kb, ctx)
    info = cn.info()
    n3 = 2 * len(_net["forms"])
    assert cn.gate_count(MAJ3) == n3 // 2 + 1 and cn.gate_count(XOR3) == n3 // 2 + 1 and cn.gate_count(ia.GATE_MUX) == 3
    assert info.depth == 3 and info.bootstraps == len(cn.gates) + 3  # every gate one rotation, a MUX two
    st = ia.Stats()
    out = ctx.eval_netlist(cn, inp, st)
    assert np.array_equal(out, ref)
    assert st.bootstraps == 8 * info.bootstraps and st.levels == 3
    assert np.array_equal(kb.dec(out), np.stack([cn.simulate(v) for v in bits]))
    saved = {k: ctx.get_option(k) for k in ("chunk", "overlap", "overlap_min", "pipe_min", "pipe_auto", "exact_fft")}
    try:
        for chunk in (1, 3):
            ctx.set_chunk(chunk)
            assert np.array_equal(ctx.eval_netlist(cn, inp[:2]), ref[:2]), chunk
        ctx.set_chunk(saved["chunk"])
        ctx.set_option("overlap", 0)  # one stream
        assert np.array_equal(ctx.eval_netlist(cn, inp), ref)
        ctx.set_option("overlap", 1)
        ctx.set_option("pipe_auto", 0)
        ctx.set_option("overlap_min", 16)  # level halves on two lanes
        lv = ctx.get_option("overlapped_levels")
        assert np.array_equal(ctx.eval_netlist(cn, inp), ref) and ctx.get_option("overlapped_levels") > lv
        ctx.set_option("overlap_min", saved["overlap_min"])
        ctx.set_option("pipe_min", 1)  # expression pipelines, an odd batch as well
        pe = ctx.get_option("pipelined_evals")
        assert np.array_equal(ctx.eval_netlist(cn, inp), ref)
        assert np.array_equal(ctx.eval_netlist(cn, inp[:3]), ref[:3]) and ctx.get_option("pipelined_evals") == pe + 2
        ctx.set_option("pipe_min", saved["pipe_min"])
        ctx.set_option("pipe_auto", saved["pipe_auto"])
        ctx.set_option("exact_fft", 1)
        assert np.array_equal(ctx.eval_netlist(cn, inp), ref)
        ctx.set_option("exact_fft", saved["exact_fft"])
        ctx.force_generic(True)  # the any-parameter kernels
        assert np.array_equal(ctx.eval_netlist(cn, inp), ref)
        ctx.force_generic(False)
        assert np.array_equal(ctx.eval_netlist(cn, inp[5:6]), ref[5:6])  # batch 1
        st = ia.Stats()
        assert ctx.eval_netlist(cn, inp[:0], st).shape == (0, len(cn.outputs), kb.p.n + 1) and st.bootstraps == 0
    finally:
        ctx.set_chunk(saved["chunk"])
        ctx.force_generic(False)
        for k in ("overlap", "overlap_min", "pipe_min", "pipe_auto", "exact_fft"):
            ctx.set_option(k, saved[k])


def test_guard_repeat_on_a_three_input_level(ia, gpu_ctx):
    kb, ctx = gpu_ctx(4, 1024)
    cn, bits, inp, ref = netlist_case(ia, kb, ctx)
    reps = ctx.get_option("cus") // 64 + 2  # level 1 then holds more than one gate per CU: it takes a one-limb kernel
    big, want = np.concatenate([inp] * reps), np.concatenate([ref] * reps)
    assert np.array_equal(ctx.eval_netlist(cn, big), want)
    auto = ctx.get_option("pipe_auto")
    try:
        ctx.set_option("pipe_auto", 0)  # (a batch of this size would otherwise be timed in both stream modes first)
        _, reruns = ctx.fft_guard()
        ctx.set_option("fft_guard_inject", 1)
        assert np.array_equal(ctx.eval_netlist(cn, big), want) and ctx.fft_guard()[1] == reruns + 1
    finally:
        ctx.set_option("pipe_auto", auto)


# ---- circuits ----

def circuit_inputs(ia, kb, kind, bits, values, seed, carry_in=None):
    from ieache_amd.tools import int_to_bits
    inb = np.zeros((len(values), 2 * bits + 32), dtype=np.uint8)
    for e, (a, b) in enumerate(values):
        inb[e, :bits], inb[e, bits:2 * bits] = int_to_bits(a, bits), int_to_bits(b, bits)
        if carry_in is not None:
            inb[e, 2 * bits] = carry_in[e]
    return kb.enc(inb, seed)


def ints(dec):
    from ieache_amd.tools import bits_to_int
    return [bits_to_int(d) for d in dec]


@pytest.mark.parametrize("bits", [16, 32])
def test_add_sub_rsub_fa_decrypt_as_the_reference_kinds(ia, gpu_ctx, bits):
    kb, ctx = gpu_ctx(4, 1024)
    m = 1 << bits
    vals = [(m - 1, 1), (m - 1, m - 1), (0, 0), (0x9ABCDEF0 % m, 0x12345678 % m)]
    inp = circuit_inputs(ia, kb, ia.CIRC_ADD_FA, bits, vals, 431)
    for fa, rc, f in ((ia.CIRC_ADD_FA, ia.CIRC_ADD, lambda a, b: a + b), (ia.CIRC_SUB_FA, ia.CIRC_SUB, lambda a, b: a - b),
                      (ia.CIRC_RSUB_FA, ia.CIRC_RSUB, lambda a, b: b - a)):
        st = ia.Stats()
        out = ctx.eval_batch(fa, bits, inp, st)
        info = ia.circuit_info(fa, bits)
        assert st.levels == info.depth == bits and st.bootstraps == info.bootstraps * 4 == 2 * bits * 4
        assert ints(kb.dec(out)) == [f(a, b) % m for a, b in vals]
        assert np.array_equal(kb.dec(out), kb.dec(ctx.eval_batch(rc, bits, inp)))
    # a carry word whose bit 0 is set: ADD_FA takes it as the carry-in, as the reference's add() does
    inp1 = circuit_inputs(ia, kb, ia.CIRC_ADD_FA, bits, vals, 432, carry_in=[1, 0, 1, 1])
    out = ctx.eval_batch(ia.CIRC_ADD_FA, bits, inp1)
    assert ints(kb.dec(out)) == [(a + b + k) % m for (a, b), k in zip(vals, [1, 0, 1, 1])]
    assert np.array_equal(kb.dec(out), kb.dec(ctx.eval_batch(ia.CIRC_ADD, bits, inp1)))


def test_mul_fa_decrypts_as_the_reference_multiplier(ia, gpu_ctx):
    kb, ctx = gpu_ctx(4, 1024)
    vals = [(0xFFFFFFFF, 0xFFFFFFFF), (0xDEADBEEF, 0x12345678), (0, 12345), (1 << 30, 1 << 30)]
    assert all(v in EDGE32 for v in (0xFFFFFFFF, 0, 1 << 30))
    inp = circuit_inputs(ia, kb, ia.CIRC_MUL_FA, 32, vals, 433)
    st = ia.Stats()
    out = ctx.eval_batch(ia.CIRC_MUL_FA, 32, inp, st)
    info = ia.circuit_info(ia.CIRC_MUL_FA, 32)
    assert st.levels == info.depth == 63 and st.bootstraps == info.bootstraps * 4 == 3008 * 4
    assert ints(kb.dec(out)) == [a * b for a, b in vals]
    assert np.array_equal(kb.dec(out), kb.dec(ctx.eval_batch(ia.CIRC_MUL, 32, inp)))


def test_full_adder_kinds_through_the_file_contract(ia, tmp_path):
    from ieache_amd import tools
    from test_gpu_parity import _run_file_contract
    p = ia.default_params().copy(n=6, N=64)
    tools.keygen_files(tmp_path, p)
    saved = {k: os.environ.get(k) for k in ("IEACHE_MULTIPLIER", "IEACHE_ADDER")}
    try:
        os.environ["IEACHE_MULTIPLIER"] = "full-adder"
        os.environ["IEACHE_ADDER"] = "full-adder"
        rc, size, ok = _run_file_contract(ia, tmp_path, 4, 3, 64, 0xFEDCBA9876543210, 0, 0x0F1E2D3C4B5A6978, 2)
        assert rc == 0 and ok
        code, bit_size, words = tools.verif(tmp_path)
        assert (code, bit_size) == (2, 128)
        assert sum(w << (32 * i) for i, w in enumerate(words[:4])) == 0xFEDCBA9876543210 * 0x0F1E2D3C4B5A6978
        assert (tmp_path / "averagestandard.txt").exists()
        rc, size, ok = _run_file_contract(ia, tmp_path, 2, 2, 32, 0x12345678, 0, 0x9ABCDEF0, 0)
        assert rc == 0 and ok
        code, bit_size, words = tools.verif(tmp_path)
        assert (code, bit_size) == (0, 32) and words[0] == (0x12345678 - 0x9ABCDEF0) % (1 << 32) and words[1:] == [0] * 8
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_add16_fa_at_product_parameters(ia, gpu_ctx):
    """64 sums at n = 630, and expression 0 word for word against a replay of its 32 gates on the oracle."""
    kb, ctx = gpu_ctx(630, 1024)
    rng = np.random.default_rng(44)
    vals = [(int(a), int(b)) for a, b in rng.integers(0, 1 << 16, size=(64, 2))]
    vals[:3] = [(0xFFFF, 1), (0xFFFF, 0xFFFF), (0, 0)]
    inp = circuit_inputs(ia, kb, ia.CIRC_ADD_FA, 16, vals, 441)
    st = ia.Stats()
    out = ctx.eval_batch(ia.CIRC_ADD_FA, 16, inp, st)
    assert st.bootstraps == 64 * 32 and st.levels == 16
    assert ints(kb.dec(out)) == [(a + b) & 0xFFFF for a, b in vals]
    x, y, carry = inp[0, :16], inp[0, 16:32], inp[0, 32]
    replayed = 0
    with ThreadPoolExecutor(2) as ex:
        for i in range(16):  # a bit's two gates side by side; the carry chain itself is sequential
            s, carry = ex.map(kb.ck.bootstrap, [combination(XOR3, x[i], y[i], carry), combination(MAJ3, x[i], y[i], carry)])
            assert np.array_equal(out[0, i], s), i
            replayed += 2
    assert replayed == 32


def phases(p, lwe_key, samples):
    """Phase b - <a, s> of each sample, as a fraction of the torus in [0, 1)."""
    s = np.asarray(lwe_key[: p.n], dtype=np.int64)
    return (((samples[:, p.n].astype(np.int64) - samples[:, : p.n].astype(np.int64) @ s) & 0xFFFFFFFF) / 2.0 ** 32)


def boundary_distance(phase):
    """Distance of a phase to the nearer of the two decision boundaries of a gate bootstrap, 0 and 1/2."""
    return np.abs((phase + 0.25) % 0.5 - 0.25)


def test_noise_of_three_input_gates_on_bootstrapped_inputs(ia, gpu_ctx):
    """4 096 MAJ3 and 4 096 XOR3 gates at the reference's parameters whose operands are outputs of a first layer of gates,
    i.e. carry a bootstrap's noise and the key's offset as the wires of a circuit do.  Every output decrypts right; the outputs'
    own noise is the prediction for any gate (it does not depend on the inputs); and the phase each gate actually bootstrapped
    -- computed with the secret key -- keeps more than half of its nominal distance (1/8 for MAJ3, 1/4 for XOR3) to the
    decision boundary."""
    from test_golden_cpu import phase_errors, predicted_gate_output_noise
    kb, ctx = gpu_ctx(630, 1024)
    var, offset_sd = predicted_gate_output_noise(kb.p, np.sum(kb.tlwe_key))
    cnt = 4096
    rng = np.random.default_rng(45)
    raw = rng.integers(0, 2, size=(2, 3 * cnt)).astype(np.uint8)
    layer1 = ctx.gates(ia.GATE_XOR, kb.enc(raw[0], 451), kb.enc(raw[1], 452))
    b1 = (raw[0] ^ raw[1]).reshape(3, cnt)
    assert np.array_equal(kb.dec(layer1), b1.reshape(-1))
    a, b, c = layer1.reshape(3, cnt, -1)
    errors = []
    for gate, nominal in ((MAJ3, 1 / 8), (XOR3, 1 / 4)):
        want = np.array([TRUTH3[gate](*r) for r in b1.T], dtype=np.uint8)
        out = ctx.gates3(gate, a, b, c)
        assert np.array_equal(kb.dec(out), want)
        e = phase_errors(kb.p, kb.lwe_key, out, want)
        assert np.max(np.abs(e)) < 1.0 / 32
        errors.append(e - np.mean(e))
        dist = boundary_distance(phases(kb.p, kb.lwe_key, combination(gate, a, b, c)))
        print("%s: smallest distance of a combined input phase to the decision boundary %.4f of nominal %.4f (mean %.4f)"
              % ("MAJ3" if gate == MAJ3 else "XOR3", dist.min(), nominal, dist.mean()))
        assert dist.min() > nominal / 2, (gate, dist.min())
    e = np.concatenate(errors)
    print("output variance %.4g, predicted %.4g" % (np.var(e), var))
    assert 0.94 * var < np.var(e) < 1.06 * var, (np.var(e), var)
