"""-m gpu: the HIP path through the C ABI against the CPU oracle.

P2 (bit-exact): every LWE coefficient the GPU produces equals the exact-integer
oracle's.  P1: outputs decrypt to integer arithmetic.  """
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_extension_loaded_and_device_present(ia):
    assert os.path.exists(ia.library_path())
    assert ia.device_count() >= 1


@pytest.mark.parametrize("n,N", [(5, 64), (8, 256), (16, 1024)])
def test_blind_rotate_stage_bit_exact(gpu_ctx, n, N):
    kb, ctx = gpu_ctx(n, N)
    x = kb.enc(np.random.default_rng(n).integers(0, 2, size=6), 7)
    x[5] = 0  # all bara_i = 0: every CMux step is skipped
    for steps in (0, 1, 3, -1):
        acc = ctx.debug_blind_rotate(x, steps)
        for i in range(x.shape[0]):
            bara, barb = kb.ck.modswitch(x[i])
            ref = kb.ck.blind_rotate_init(barb)
            for s in range(kb.p.n if steps < 0 else steps):
                ref = kb.ck.blind_rotate_step(ref, s, bara[s])
            assert np.array_equal(ref, acc[i]), (steps, i)


@pytest.mark.parametrize("n,N", [(5, 64), (8, 256), (16, 1024), (630, 1024)])
def test_keyswitch_stage_bit_exact(ia, gpu_ctx, n, N):
    kb, ctx = gpu_ctx(n, N)
    rng = np.random.default_rng(0)
    u = rng.integers(-2 ** 31, 2 ** 31, size=(5, N + 1), dtype=np.int64).astype(np.int32)
    u[3] = 0                # every digit zero except the rounding offset's
    u[4, :N] = -(1 << 15)   # a_i + 2^15 wraps to 0: no row subtracted at all
    out = ctx.debug_keyswitch(u)
    for i in range(u.shape[0]):
        assert np.array_equal(kb.ck.keyswitch(u[i]), out[i]), i
    assert not out[4, :n].any() and out[4, n] == u[4, N]
    if N % 8 == 0 and n >= 8:  # the hand-scheduled sliced kernel (large launches) on the same edge rows, against the oracle
        ctx.set_option("ks_sliced_min", 1)
        for gates, sl in ((4, 0), (8, 0), (16, 3), (32, 0)):
            ctx.set_option("ks_gates", gates)
            ctx.set_option("ks_slice", sl)
            assert np.array_equal(ctx.debug_keyswitch(u), out), (gates, sl)
        ctx.set_option("ks_gates", 0)
        ctx.set_option("ks_slice", 0)
        ctx.set_option("ks_sliced_min", 576)
    # the int8 MFMA product (launches of >= 64 gates) on the same edge rows, against the oracle: every K split
    ctx.set_option("ks_mfma_min", 1)
    # the product's loop takes two digit groups (eight coefficients of B fragments) per trip: a split must hold whole trips.
    # The largest such split is N / 8 -- correct -- and the next power of two (one group per split) is refused when set
    largest = min(64, N // 8)
    for split in (0, 1, 2, 4, 8, largest):
        ctx.set_option("ks_mfma_split", split)
        assert np.array_equal(ctx.debug_keyswitch(u), out), split
    if 2 * largest <= 64:
        with pytest.raises(ia.IeacheError):
            ctx.set_option("ks_mfma_split", 2 * largest)
        assert ctx.get_option("ks_mfma_split") == largest  # a refused value changes nothing
    ctx.set_option("ks_mfma_split", 0)
    ctx.set_option("ks_mfma_min", 64)


@pytest.mark.parametrize("n,N", [(5, 64), (16, 1024)])
def test_gates_bit_exact_and_truth_tables(ia, gpu_ctx, n, N):
    kb, ctx = gpu_ctx(n, N)
    a_bits = np.array([0, 0, 1, 1] * 3, dtype=np.uint8)
    b_bits = np.array([0, 1, 0, 1] * 3, dtype=np.uint8)
    a, b = kb.enc(a_bits, 11), kb.enc(b_bits, 12)
    for name, gt, f in (("and", ia.GATE_AND, a_bits & b_bits), ("xor", ia.GATE_XOR, a_bits ^ b_bits),
                        ("or", ia.GATE_OR, a_bits | b_bits), ("nand", ia.GATE_NAND, 1 - (a_bits & b_bits))):
        st = ia.Stats()
        out = ctx.gates(gt, a, b, st)
        assert st.bootstraps == 12
        assert np.array_equal(kb.dec(out), f), name
        for i in range(12):
            assert np.array_equal(kb.ck.gate(name, a[i], b[i]), out[i]), (name, i)


def test_full_size_gates_match_golden_and_oracle(ia, O, gpu_ctx):
    """n=630, N=1024: committed KAT + a batch that must decrypt correctly."""
    z = np.load(os.path.join(G, "full_gate_kat.npz"))
    kb, ctx = gpu_ctx(630, 1024, seed=tuple(int(v) for v in z["seed"]))
    assert np.array_equal(ctx.gates(ia.GATE_AND, z["ca"], z["cb"]), z["gate_and"])
    assert np.array_equal(ctx.gates(ia.GATE_XOR, z["ca"], z["cb"]), z["gate_xor"])
    rng = np.random.default_rng(1)
    bits = rng.integers(0, 2, size=(2, 300)).astype(np.uint8)
    a, b = kb.enc(bits[0], 21), kb.enc(bits[1], 22)
    out = ctx.gates(ia.GATE_XOR, a, b)
    assert np.array_equal(kb.dec(out), bits[0] ^ bits[1])
    for i in (0, 299):
        assert np.array_equal(kb.ck.gate("xor", a[i], b[i]), out[i])
    # chunked launches give the same bits
    ctx.set_chunk(64)
    assert np.array_equal(ctx.gates(ia.GATE_XOR, a, b), out)
    ctx.set_chunk(16384)


def test_toy_golden_vectors(ia):
    z = np.load(os.path.join(G, "toy_vectors.npz"))
    n, N, k, l, Bgbit, t, bb = (int(v) for v in z["params"])
    p = ia.default_params().copy(n=n, N=N, k=k, l=l, Bgbit=Bgbit, ks_t=t, ks_basebit=bb)
    with ia.Context.from_arrays(p, z["bk"], z["ksk"]) as ctx:
        for g, gt in (("and", ia.GATE_AND), ("xor", ia.GATE_XOR), ("or", ia.GATE_OR), ("nand", ia.GATE_NAND)):
            assert np.array_equal(ctx.gates(gt, z["ca"], z["cb"]), z["gate_" + g]), g
        assert np.array_equal(ctx.debug_blind_rotate(z["ca"][3:4], 0)[0], z["acc0"])
        assert np.array_equal(ctx.debug_blind_rotate(z["ca"][3:4], 1)[0], z["acc1"])
        assert np.array_equal(ctx.debug_blind_rotate(z["ca"][3:4], -1)[0], z["accn"])
        assert np.array_equal(ctx.debug_keyswitch(z["extracted"])[0], z["keyswitched"])
        # add(nb_bits=4) through the generalised ADD circuit: inputs x, y, carry word
        inp = np.concatenate([z["add_x"], z["add_y"], np.repeat(z["add_c"], 32, axis=0)])[None]
        out = ctx.eval_batch(ia.CIRC_ADD, 4, inp)
        assert np.array_equal(out[0], z["add_sum"])


def _inputs(kb, kind, bits, values, seed):
    """values: list of (a, b[, c]) -> encrypted circuit inputs [batch][n_inputs][n+1]."""
    import ieache_amd as ia
    from ieache_amd.tools import int_to_bits
    info = ia.circuit_info(kind, bits)
    inb = np.zeros((len(values), info.n_inputs), dtype=np.uint8)
    for e, v in enumerate(values):
        inb[e, :bits] = int_to_bits(v[0], bits)
        inb[e, bits:2 * bits] = int_to_bits(v[1], bits)
        if kind == 5:
            inb[e, 2 * bits + 32:] = int_to_bits(v[2], 2 * bits)
    return kb.enc(inb, seed)


def _oracle_values(kb, op, neg, bits, inp, threads=1):
    """Run the oracle's sequential cloud.c restatement on one expression's inputs (threads != 1: the same
    gate stream with independent gates on several host threads, see tests/test_oracle_cpu.py)."""
    S = kb.p.n + 1
    W = bits // 32
    o1 = np.zeros((8, 32, S), np.int32)
    o2 = np.zeros((8, 32, S), np.int32)
    o1[:W] = inp[:bits].reshape(W, 32, S)
    o2[:W] = inp[bits:2 * bits].reshape(W, 32, S)
    rc, out = kb.ck.cloud_values(op, neg, bits, o1, o2, inp[2 * bits:2 * bits + 32], threads=threads)
    assert rc == 0
    return out


@pytest.mark.parametrize("kind,op,neg,bits", [(1, 1, 0, 32), (1, 1, 0, 64), (2, 2, 0, 32), (2, 2, 0, 128), (3, 1, 1, 64),
                                              (1, 1, 0, 256), (2, 1, 2, 256)])
def test_add_sub_circuits_bit_exact(ia, gpu_ctx, kind, op, neg, bits):
    kb, ctx = gpu_ctx(4, 1024)
    from ieache_amd.tools import bits_to_int
    rng = np.random.default_rng(bits + kind)
    m = 1 << bits
    vals = [(int.from_bytes(rng.bytes(bits // 8), "little"), int.from_bytes(rng.bytes(bits // 8), "little")) for _ in range(3)]
    vals += [(m - 1, 1), (1 << (bits - 2), 1 << (bits - 2))]  # carry through every bit; process.c operands
    inp = _inputs(kb, kind, bits, vals, 5)
    st = ia.Stats()
    out = ctx.eval_batch(kind, bits, inp, st)
    info = ia.circuit_info(kind, bits)
    assert st.bootstraps == info.bootstraps * len(vals) and st.levels == info.depth
    dec = kb.dec(out)
    for e, (a, b) in enumerate(vals):
        exp = {1: a + b, 2: a - b, 3: b - a}[kind] % m
        assert bits_to_int(dec[e]) == exp
    ref = _oracle_values(kb, op, neg, bits, inp[0])
    assert np.array_equal(ref[:bits // 32].reshape(bits, -1), out[0])


def test_add16_generalisation_bit_exact(ia, gpu_ctx):
    """BASELINE.json configs[1]: add(..., nb_bits=16, ...) (cloud.c:18)."""
    kb, ctx = gpu_ctx(4, 1024)
    from ieache_amd.tools import bits_to_int
    vals = [(0xFFFF, 1), (0x1234, 0xEDCB), (0, 0), (40000, 30000)]
    inp = _inputs(kb, 1, 16, vals, 6)
    out = ctx.eval_batch(1, 16, inp)
    dec = kb.dec(out)
    for e, (a, b) in enumerate(vals):
        assert bits_to_int(dec[e]) == (a + b) & 0xFFFF
        s, _ = kb.ck.add(inp[e, :16], inp[e, 16:32], inp[e, 32:33], 16)
        assert np.array_equal(s, out[e])


def test_mul32_bit_exact(ia, gpu_ctx):
    kb, ctx = gpu_ctx(4, 1024)
    from ieache_amd.tools import bits_to_int
    vals = [(0xFFFFFFFF, 0xFFFFFFFF), (1 << 30, 1 << 30), (0xDEADBEEF, 0x12345678)]
    inp = _inputs(kb, 4, 32, vals, 8)
    st = ia.Stats()
    out = ctx.eval_batch(4, 32, inp, st)
    assert st.bootstraps == 11264 * 3 and st.levels == 255
    dec = kb.dec(out)
    for e, (a, b) in enumerate(vals):
        assert bits_to_int(dec[e]) == a * b
    ref = _oracle_values(kb, 4, 0, 32, inp[2])
    assert np.array_equal(ref[:2].reshape(64, -1), out[2])


def _two_stage_oracle(kb, k1, k2, flip, bits, inp):
    """compute() then compute_final() with the oracle: stage 1 on (A, B), then stage 2 on
    (answer, C) or (C, answer) exactly as a second ./cloud run would (cloud_oracle.c orc_cloud_values)."""
    S = kb.p.n + 1
    opneg = {1: (1, 0), 2: (2, 0), 3: (1, 1), 4: (4, 0)}  # circuit kind -> (operator, sign routing) of main()
    w2 = 2 * bits if k1 == 4 else bits
    op, neg = opneg[k1]
    st1 = _oracle_values(kb, op, neg, bits, inp, threads=0)  # [9][32][S]; words past the result are the carry word
    C = np.zeros((8, 32, S), np.int32)
    C[:w2 // 32] = inp[2 * bits + 32:2 * bits + 32 + w2].reshape(w2 // 32, 32, S)
    ans = np.ascontiguousarray(st1[:8])
    carry = inp[2 * bits:2 * bits + 32] if flip else inp[2 * bits + 32 + w2:2 * bits + 64 + w2]
    op, neg = opneg[k2]
    o1, o2 = (ans, C) if flip else (C, ans)
    rc, st2 = kb.ck.cloud_values(op, neg, w2, o1, o2, carry, threads=0)
    assert rc == 0
    nw = (2 * w2 if k2 == 4 else w2) // 32
    return st2[:nw].reshape(nw * 32, S)


def _chain_inputs(kb, ia, k1, k2, flip, bits, a, b, c, seed):
    from ieache_amd.tools import int_to_bits
    info = ia.circuit_info(ia.circ_chain(k1, k2, flip), bits)
    w2 = 2 * bits if k1 == 4 else bits
    inb = np.zeros((1, info.n_inputs), dtype=np.uint8)
    inb[0, :bits] = int_to_bits(a, bits)
    inb[0, bits:2 * bits] = int_to_bits(b, bits)
    inb[0, 2 * bits + 32:2 * bits + 32 + w2] = int_to_bits(c, w2)
    return kb.enc(inb, seed)


def test_mul64_and_muladd_fast_kernels(ia, gpu_ctx):
    """BASELINE configs[3]'s circuit: 64-bit MUL (2x mul64 + split) and the fused a*b+c, on the N=1024 ring so
    the two-wave blind rotation, the latency kernel and the hand-scheduled key switch carry the whole DAG
    (the oracle replays its own sequential gate stream on all host cores)."""
    kb, ctx = gpu_ctx(4, 1024)
    assert "radix8" in ctx.kernel_variant
    from ieache_amd.tools import bits_to_int
    a, b, c = 0xFEDCBA9876543210, 0x0F1E2D3C4B5A6978, (1 << 127) | 0x1234567890ABCDEF
    inp = _inputs(kb, 4, 64, [(a, b), (1 << 62, 1 << 62)], 9)
    st = ia.Stats()
    out = ctx.eval_batch(4, 64, inp, st)
    assert st.bootstraps == 2 * 35296 and st.levels == 449
    dec = kb.dec(out)
    assert bits_to_int(dec[0]) == a * b and bits_to_int(dec[1]) == 1 << 124
    S = kb.p.n + 1
    o1 = np.zeros((8, 32, S), np.int32)
    o2 = np.zeros((8, 32, S), np.int32)
    o1[:2], o2[:2] = inp[0, :64].reshape(2, 32, S), inp[0, 64:128].reshape(2, 32, S)
    rc, ref = kb.ck.cloud_values(4, 0, 64, o1, o2, inp[0, 128:160], threads=0)
    assert rc == 0 and np.array_equal(ref[:4].reshape(128, -1), out[0])
    inp = _inputs(kb, 5, 64, [(a, b, c)], 10)
    st = ia.Stats()
    out = ctx.eval_batch(5, 64, inp, st)
    assert st.bootstraps == 35936 and st.levels == 451
    assert bits_to_int(kb.dec(out)[0]) == (a * b + c) % (1 << 128)
    assert np.array_equal(_two_stage_oracle(kb, 4, 1, True, 64, inp[0]), out[0])


def test_mul128_fast_kernels(ia, gpu_ctx):
    """BASELINE configs[4]'s circuit (depth 1601, 121 184 bootstraps per expression) on the N=1024 ring."""
    kb, ctx = gpu_ctx(4, 1024)
    from ieache_amd.tools import bits_to_int
    a = (1 << 126) | 0xFFFFFFFFFFFFFFFFFFFFFFFF
    b = (1 << 127) | 0x123456789ABCDEF0FEDCBA9
    inp = _inputs(kb, 4, 128, [(a, b), (1 << 126, 1 << 126)], 12)
    st = ia.Stats()
    out = ctx.eval_batch(4, 128, inp, st)
    assert st.levels == 1601 and st.bootstraps == 2 * 121184
    dec = kb.dec(out)
    assert bits_to_int(dec[0]) == a * b and bits_to_int(dec[1]) == 1 << 252  # process.c:152-163
    S = kb.p.n + 1
    o1 = np.zeros((8, 32, S), np.int32)
    o2 = np.zeros((8, 32, S), np.int32)
    o1[:4], o2[:4] = inp[0, :128].reshape(4, 32, S), inp[0, 128:256].reshape(4, 32, S)
    rc, ref = kb.ck.cloud_values(4, 0, 128, o1, o2, inp[0, 256:288], threads=0)
    assert rc == 0 and np.array_equal(ref[:8].reshape(256, -1), out[0])


@pytest.mark.parametrize("k1,k2,flip,bits", [(4, 1, True, 32),    # A*B+C on 32-bit operands (AC058.pdf Fig. 7 "A+B*C")
                                             (1, 2, True, 32),    # A+B-C
                                             (2, 2, True, 64),    # A-B-C
                                             (1, 1, False, 32),   # C+(A+B): answer as operand 2, C's own carry word
                                             (4, 3, False, 32),   # A*B-C as (-C)+answer
                                             (4, 4, True, 32),    # A*B*C: 32-bit MUL then 64-bit MUL (46 560 bootstraps)
                                             (4, 1, True, 128)])  # 128-bit a*b+c: MUL128 then a 256-bit ADD
def test_chained_operators_bit_exact(ia, gpu_ctx, k1, k2, flip, bits):
    """compute() + compute_final() (dragonfly_cipher_cloud.py:1219-1327) as ONE DAG equals the
    oracle's two ./cloud runs bit for bit, and decrypts to the integer expression."""
    kb, ctx = gpu_ctx(4, 1024)
    from ieache_amd.tools import bits_to_int
    rng = np.random.default_rng(1000 * k1 + 100 * k2 + bits)
    m = 1 << bits
    w2 = 2 * bits if k1 == 4 else bits
    a, b = (int.from_bytes(rng.bytes(bits // 8), "little") for _ in range(2))
    c = int.from_bytes(rng.bytes(w2 // 8), "little")
    kind = ia.circ_chain(k1, k2, flip)
    inp = _chain_inputs(kb, ia, k1, k2, flip, bits, a, b, c, 70 + k1 + k2)
    st = ia.Stats()
    out = ctx.eval_batch(kind, bits, inp, st)
    info = ia.circuit_info(kind, bits)
    assert st.bootstraps == info.bootstraps and st.levels == info.depth
    f = {1: lambda x, y, mm: (x + y) % mm, 2: lambda x, y, mm: (x - y) % mm, 3: lambda x, y, mm: (y - x) % mm,
         4: lambda x, y, mm: x * y}
    s1 = f[k1](a, b, m)
    exp = f[k2](s1, c, 1 << w2) if flip else f[k2](c, s1, 1 << w2)
    assert bits_to_int(kb.dec(out)[0]) == exp
    assert np.array_equal(_two_stage_oracle(kb, k1, k2, flip, bits, inp[0]), out[0])
    if (k1, k2, flip) == (4, 1, True):  # CIRC_MULADD is the same DAG under its round-1 code
        assert np.array_equal(ctx.eval_batch(ia.CIRC_MULADD, bits, inp), out)


@pytest.mark.parametrize("n,N", [(5, 64), (16, 1024)])
def test_mux_gate_bit_exact(ia, gpu_ctx, n, N):
    """bootsMUX(a,b,c) = a ? b : c (named by BASELINE.json's north_star; cloud.c never calls it): two blind
    rotations without key switch, one key switch -- against the oracle's restatement of boot-gates.cpp."""
    kb, ctx = gpu_ctx(n, N)
    a_bits = np.array([0, 0, 0, 0, 1, 1, 1, 1] * 2, dtype=np.uint8)
    b_bits = np.array([0, 0, 1, 1, 0, 0, 1, 1] * 2, dtype=np.uint8)
    c_bits = np.array([0, 1, 0, 1, 0, 1, 0, 1] * 2, dtype=np.uint8)
    a, b, c = kb.enc(a_bits, 81), kb.enc(b_bits, 82), kb.enc(c_bits, 83)
    st = ia.Stats()
    out = ctx.mux(a, b, c, st)
    assert st.bootstraps == 32 and st.keyswitch_launches == 1
    assert np.array_equal(kb.dec(out), np.where(a_bits == 1, b_bits, c_bits))
    for i in range(16):
        assert np.array_equal(kb.ck.mux(a[i], b[i], c[i]), out[i]), i
    ctx.set_chunk(6)  # ragged chunks of 3 gates = 6 blind rotations
    assert np.array_equal(ctx.mux(a, b, c), out)
    ctx.set_chunk(16384)
    if N == 1024:     # large launches: two-wave blind rotation + hand-scheduled key switch
        reps = 70
        big = ctx.mux(np.tile(a, (reps, 1)), np.tile(b, (reps, 1)), np.tile(c, (reps, 1)))
        assert np.array_equal(big, np.tile(out, (reps, 1)))
    assert ctx.mux(a[:0], b[:0], c[:0]).shape[0] == 0


def test_constant_folded_circuits_decrypt_identically(ia, gpu_ctx):
    """Opt-in fold_constants: fewer bootstraps, same plaintext; the default path is untouched."""
    kb, ctx = gpu_ctx(4, 1024)
    from ieache_amd.tools import bits_to_int
    vals = [(0xFFFFFFFF, 0xFFFFFFFF), (0xDEADBEEF, 0x12345678), (0, 0x9ABCDEF0), (1 << 30, 1 << 30)]
    inp = _inputs(kb, 4, 32, vals, 8)
    ref = ctx.eval_batch(4, 32, inp)
    ctx.set_option("fold_constants", 1)
    try:
        st = ia.Stats()
        out = ctx.eval_batch(4, 32, inp, st)
        info = ia.circuit_info(4, 32, fold=True)
        assert st.bootstraps == info.bootstraps * len(vals) == 7568 * len(vals) and info.reference_bootstraps == 11264
        assert np.array_equal(kb.dec(out), kb.dec(ref))
        assert [bits_to_int(d) for d in kb.dec(out)] == [a * b for a, b in vals]
        sub = _inputs(kb, 2, 64, [(5, 9), (1 << 63, 1)], 18)
        assert [bits_to_int(d) for d in kb.dec(ctx.eval_batch(2, 64, sub))] == [(5 - 9) % (1 << 64), (1 << 63) - 1]
    finally:
        ctx.set_option("fold_constants", 0)
    assert np.array_equal(ctx.eval_batch(4, 32, inp), ref)  # default again: the reference's own gate list
    with pytest.raises(ia.IeacheError):
        ctx.set_option("fold_constants", 2)


def test_mul32_at_product_parameters_matches_golden(ia, gpu_ctx):
    """BASELINE configs[2]'s circuit at n=630: all 64 output samples of one encrypted 32-bit multiplication
    equal what the oracle's sequential mul32 produced offline (tests/golden/mul32_n630.json, made by
    make_golden.py mul32_n630: 11 264 exact bootstraps)."""
    import hashlib
    from ieache_amd.tools import bits_to_int, int_to_bits
    g = json.load(open(os.path.join(G, "mul32_n630.json")))
    kb, ctx = gpu_ctx(630, 1024, seed=tuple(g["key_seed"]))
    inb = np.zeros(96, dtype=np.uint8)
    inb[:32], inb[32:64] = int_to_bits(g["a"], 32), int_to_bits(g["b"], 32)
    inp = kb.enc(inb, g["encrypt_seed"])
    assert hashlib.sha256(np.ascontiguousarray(inp).tobytes()).hexdigest() == g["input_sha256"]
    st = ia.Stats()
    out = ctx.eval_batch(4, 32, inp[None], st)[0]
    assert st.bootstraps == 11264 == g["bootstraps"] and st.levels == 255
    assert bits_to_int(kb.dec(out)) == g["a"] * g["b"]
    assert out[0].tolist() == g["first_sample"] and out[-1].tolist() == g["last_sample"]
    assert hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest() == g["output_sha256"]
    # the same expression inside a batch wide enough for the two-wave kernel and the sliced key switch
    batch = np.repeat(inp[None], 24, axis=0)
    outs = ctx.eval_batch(4, 32, batch)
    assert all(np.array_equal(outs[e], out) for e in range(24))
    # the guard's repeat path on the golden: an (injected) guard trip re-runs the whole call on the two-limb kernels ...
    r0 = ctx.fft_guard()[1]
    ctx.set_option("fft_guard_inject", 1)
    out2 = ctx.eval_batch(4, 32, inp[None])[0]
    assert ctx.fft_guard()[1] == r0 + 1
    assert hashlib.sha256(np.ascontiguousarray(out2).tobytes()).hexdigest() == g["output_sha256"]
    # ... and so does a row the sampled audit finds different (every launch audited here)
    ctx.set_option("fft_audit", 1)
    ctx.set_option("fft_audit_inject", 1)
    a0 = ctx.fft_audit()
    out3 = ctx.eval_batch(4, 32, inp[None])[0]
    a1 = ctx.fft_audit()
    ctx.set_option("fft_audit", 64)
    assert ctx.fft_guard()[1] == r0 + 2 and a1["mismatches"] == a0["mismatches"] + 1 and a1["audits"] > a0["audits"]
    assert hashlib.sha256(np.ascontiguousarray(out3).tobytes()).hexdigest() == g["output_sha256"]
    # the provably exact two-limb transform from the start: same bits
    ctx.set_option("exact_fft", 1)
    out4 = ctx.eval_batch(4, 32, inp[None])[0]
    ctx.set_option("exact_fft", 0)
    assert hashlib.sha256(np.ascontiguousarray(out4).tobytes()).hexdigest() == g["output_sha256"] and ctx.fft_guard()[1] == r0 + 2


def test_muladd64_at_product_parameters_matches_golden(ia, gpu_ctx):
    """BASELINE configs[3]'s circuit at n=630: the fused 64-bit a*b+c (35 936 bootstraps, 451 levels) equals, sample for
    sample, what the oracle's two sequential cloud.c runs produced offline (tests/golden/muladd64_n630.json)."""
    import hashlib
    from ieache_amd.tools import bits_to_int, int_to_bits
    path = os.path.join(G, "muladd64_n630.json")
    g = json.load(open(path))
    kb, ctx = gpu_ctx(630, 1024, seed=tuple(g["key_seed"]))
    inb = np.zeros(2 * 64 + 32 + 128, dtype=np.uint8)
    inb[:64], inb[64:128], inb[160:] = int_to_bits(g["a"], 64), int_to_bits(g["b"], 64), int_to_bits(g["c"], 128)
    inp = kb.enc(inb, g["encrypt_seed"])
    assert hashlib.sha256(np.ascontiguousarray(inp).tobytes()).hexdigest() == g["input_sha256"]
    st = ia.Stats()
    out = ctx.eval_batch(ia.CIRC_MULADD, 64, inp[None], st)[0]
    assert st.bootstraps == 35936 == g["bootstraps"] and st.levels == 451
    assert bits_to_int(kb.dec(out)) == (g["a"] * g["b"] + g["c"]) % (1 << 128)
    assert out[0].tolist() == g["first_sample"] and out[-1].tolist() == g["last_sample"]
    assert hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest() == g["output_sha256"]


def test_misc_product_parameter_vectors(ia, gpu_ctx):
    """n=630 vectors for the paths the big goldens do not touch: a chained ADD -> SUB, the (-A)+B branch, OR / NAND / MUX
    (tests/golden/misc_n630.json, made by the oracle offline)."""
    import hashlib
    from ieache_amd.tools import int_to_bits
    g = json.load(open(os.path.join(G, "misc_n630.json")))
    kb, ctx = gpu_ctx(630, 1024, seed=tuple(g["key_seed"]))
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    v = g["addsub32"]
    inb = np.zeros(128, dtype=np.uint8)
    inb[:32], inb[32:64], inb[96:128] = int_to_bits(v["a"], 32), int_to_bits(v["b"], 32), int_to_bits(v["c"], 32)
    inp = kb.enc(inb, v["encrypt_seed"])
    assert sha(inp) == v["input_sha256"]
    out = ctx.eval_batch(ia.circ_chain(ia.CIRC_ADD, ia.CIRC_SUB), 32, inp[None])[0]
    assert out[0].tolist() == v["first_sample"] and sha(out) == v["output_sha256"]
    v = g["rsub64"]
    inb = np.zeros(160, dtype=np.uint8)
    inb[:64], inb[64:128] = int_to_bits(v["a"], 64), int_to_bits(v["b"], 64)
    inp = kb.enc(inb, v["encrypt_seed"])
    assert sha(inp) == v["input_sha256"]
    out = ctx.eval_batch(ia.CIRC_RSUB, 64, inp[None])[0]
    assert out[-1].tolist() == v["last_sample"] and sha(out) == v["output_sha256"]
    v = g["gates"]
    bits = np.array([[0, 0, 0, 0, 1, 1, 1, 1], [0, 0, 1, 1, 0, 0, 1, 1], [0, 1, 0, 1, 0, 1, 0, 1]], dtype=np.uint8)
    ga, gb, gc = (kb.enc(bits[i], v["encrypt_seeds"][i]) for i in range(3))
    assert sha(ctx.gates(ia.GATE_OR, ga, gb)) == v["or_sha256"]
    assert sha(ctx.gates(ia.GATE_NAND, ga, gb)) == v["nand_sha256"]
    mux = ctx.mux(ga, gb, gc)
    assert mux[0].tolist() == v["mux_first_sample"] and sha(mux) == v["mux_sha256"]


def test_mul128_at_product_parameters_matches_golden(ia, gpu_ctx):
    """BASELINE configs[4]'s circuit at n=630: one 128-bit multiplication (121 184 bootstraps, 1 601 levels) against the
    oracle's sequential run (tests/golden/mul128_n630.json)."""
    import hashlib
    from ieache_amd.tools import bits_to_int, int_to_bits
    g = json.load(open(os.path.join(G, "mul128_n630.json")))
    kb, ctx = gpu_ctx(630, 1024, seed=tuple(g["key_seed"]))
    inb = np.zeros(2 * 128 + 32, dtype=np.uint8)
    inb[:128], inb[128:256] = int_to_bits(g["a"], 128), int_to_bits(g["b"], 128)
    inp = kb.enc(inb, g["encrypt_seed"])
    assert hashlib.sha256(np.ascontiguousarray(inp).tobytes()).hexdigest() == g["input_sha256"]
    st = ia.Stats()
    out = ctx.eval_batch(ia.CIRC_MUL, 128, inp[None], st)[0]
    assert st.bootstraps == 121184 == g["bootstraps"] and st.levels == 1601
    assert bits_to_int(kb.dec(out)) == g["a"] * g["b"]
    assert out[0].tolist() == g["first_sample"] and out[-1].tolist() == g["last_sample"]
    assert hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest() == g["output_sha256"]


def test_noise_margin_of_bootstrapped_outputs(ia, gpu_ctx):
    """SURVEY section 7 step 1 at the product parameter set: the phase error of bootstrapped outputs against
    the analytic variance of TFHE gate bootstrapping (Keygen/keygen.c:22-23's set: sigma_bk = 2^-25, sigma_ks =
    2^-15, l = 3, Bg = 2^7, t = 8, basebit = 2).  The external product here is exact, so there is no FFT term:
      Var = n (k+1) l N (Bg/2)^2 sigma_bk^2 + n (1 + kN) eps^2 [eps = 1/(2 Bg^l)]      blind rotation
          + kN t sigma_ks^2 (1 - 1/base) + kN 2^(-2(t basebit + 1)) / 12 * ...           key switch (rounding is tiny)
    4 096 gates: the maximum error must stay under 1/16 (what the next gate needs), the empirical
    deviation must sit at the analytic one."""
    z = np.load(os.path.join(G, "full_gate_kat.npz"))
    kb, ctx = gpu_ctx(630, 1024, seed=tuple(int(v) for v in z["seed"]))
    p = kb.p
    rng = np.random.default_rng(8)
    cnt = 4096
    bits = rng.integers(0, 2, size=(2, cnt)).astype(np.uint8)
    a, b = kb.enc(bits[0], 91), kb.enc(bits[1], 92)
    errs = []
    for gt, truth in ((ia.GATE_AND, bits[0] & bits[1]), (ia.GATE_XOR, bits[0] ^ bits[1])):
        out = ctx.gates(gt, a, b)
        ph = (out[:, -1].astype(np.int64) - (out[:, :-1].astype(np.int64) * kb.lwe_key.astype(np.int64)).sum(1)) & 0xFFFFFFFF
        ph = np.where(ph >= 2 ** 31, ph - 2 ** 32, ph).astype(np.float64) / 2.0 ** 32
        assert np.array_equal((ph > 0).astype(np.uint8), truth)
        errs.append(ph - np.where(truth == 1, 0.125, -0.125))
    err = np.concatenate(errs)
    Bg, eps = 2.0 ** p.Bgbit, 1.0 / (2.0 * 2.0 ** (p.Bgbit * p.l))
    var_br = p.n * (p.k + 1) * p.l * p.N * (Bg / 2) ** 2 * p.tlwe_alpha_min ** 2 + p.n * (1 + p.k * p.N) * eps ** 2
    base = 1 << p.ks_basebit
    var_ks = p.k * p.N * p.ks_t * p.lwe_alpha_min ** 2 * (1 - 1.0 / base) + p.k * p.N * (2.0 ** -(p.ks_t * p.ks_basebit + 1)) ** 2 / 3
    sigma = (var_br + var_ks) ** 0.5
    # the decomposition digits are uniform in [-Bg/2, Bg/2): E[d^2] = Bg^2/12, so the bound above (worst-case
    # digits) overestimates the blind-rotation part by 3x; the measured deviation must sit between the two
    sigma_typ = (var_br / 3 + var_ks) ** 0.5
    assert 0.6 * sigma_typ < err.std() < 1.15 * sigma, (err.std(), sigma_typ, sigma)
    # not zero-mean: tGswTorus32PolynomialDecompH truncates (its offset carries no half-ulp), so every CMux
    # step drops a residual of mean 2^-22 per coefficient, coherent over the N coefficients of a polynomial
    # (N 2^-22 = 1.2e-4 per active step, signs scrambled by the later rotations).  The oracle does the same --
    # the GPU result is bit-identical to it -- and the key-dependent common part stays far inside sigma.
    assert abs(err.mean()) < 0.5 * sigma, (err.mean(), sigma)
    assert np.abs(err).max() < min(1.0 / 16, 6 * sigma), (np.abs(err).max(), sigma)
    print("noise margin: std %.3e (analytic typical %.3e, worst-case %.3e), mean %.3e, max |err| %.3e of 1/16 = %.3e"
          % (err.std(), sigma_typ, sigma, err.mean(), np.abs(err).max(), 1 / 16))


def test_stream_ordering_entry_point(ia, gpu_ctx):
    """include/ieache.h "Streams": inputs produced on another stream are ordered by ieache_ctx_wait_stream."""
    import torch
    kb, ctx = gpu_ctx(4, 1024)
    inp = _inputs(kb, 1, 32, [(123456789, 987654321), (7, 9), (0xFFFFFFFF, 1)], 13)
    host = ctx.eval_batch(1, 32, inp)
    stride = ctx.lwe_stride
    side = torch.cuda.Stream()
    d_out = torch.zeros((3, 32, stride), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        junk = torch.randn(4096, 4096, device="cuda")
        for _ in range(20):  # keep the side stream busy so the copy below completes late
            junk = junk @ junk * 1e-4
        d_in = torch.zeros((3, 96, stride), dtype=torch.int32, device="cuda")
        d_in[:, :, :kb.p.n + 1] = torch.from_numpy(inp).cuda()
    ctx.wait_stream(side.cuda_stream)  # no host-side synchronize between producer and evaluator
    ctx.eval_batch_device(1, 32, 3, d_in.data_ptr(), d_out.data_ptr())
    assert np.array_equal(d_out.cpu().numpy()[:, :, :kb.p.n + 1], host)
    ctx.wait_stream(None)


def test_device_buffer_api_matches_host_api(ia, gpu_ctx):
    import torch
    kb, ctx = gpu_ctx(4, 1024)
    inp = _inputs(kb, 1, 32, [(123456789, 987654321), (7, 9)], 13)
    host = ctx.eval_batch(1, 32, inp)
    stride = ctx.lwe_stride
    d_in = torch.zeros((2, 96, stride), dtype=torch.int32, device="cuda")
    d_in[:, :, :kb.p.n + 1] = torch.from_numpy(inp).cuda()
    d_out = torch.zeros((2, 32, stride), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.eval_batch_device(1, 32, 2, d_in.data_ptr(), d_out.data_ptr())
    assert np.array_equal(d_out.cpu().numpy()[:, :, :kb.p.n + 1], host)
    # keys handed over as device pointers (the RCCL-broadcast path)
    bk = torch.from_numpy(np.ascontiguousarray(kb.bk)).cuda()
    ksk = torch.from_numpy(np.ascontiguousarray(kb.ksk)).cuda()
    torch.cuda.synchronize()
    with ia.Context.from_device_pointers(kb.p, bk.data_ptr(), ksk.data_ptr()) as ctx2:
        assert np.array_equal(ctx2.eval_batch(1, 32, inp), host)


def _run_file_contract(ia, tmp_path, op_code, operator, bits, a, sa, b, sb, use_subprocess=False, ctx=None):
    from ieache_amd import tools
    tools.alice(tmp_path, sa, bits, a, seed=31)
    tools.alice(tmp_path, sb, bits, b, seed=32, append=True)
    rc, size, ok = ia.compute(operator, tmp_path, ctx=ctx, use_subprocess=use_subprocess, failure_size=64 * (4 * 6 + 16))
    return rc, size, ok


def test_cloud_file_contract_end_to_end(ia, O, tmp_path):
    """keygen -> alice x2 -> compute() -> verif, on the reference's canned operands
    (tests/golden/plaintext_kats.json from Client1/process.c), every sign case."""
    from ieache_amd import tools
    p = ia.default_params().copy(n=6, N=64)
    tools.keygen_files(tmp_path, p)
    S = 4 * p.n + 16
    kats = json.load(open(os.path.join(G, "plaintext_kats.json")))
    _, bk, ksk = tools.read_cloud_key(tmp_path / "cloud.key")
    ck = O.CloudKey(p.n, p.N, p.k, p.l, p.Bgbit, p.ks_t, p.ks_basebit, bk, ksk)
    with ia.Context.from_file(tmp_path / "cloud.key") as ctx:
        for kat in kats:
            if kat["bits"] == 128 and kat["op"] == 4 and (kat["sa"], kat["sb"]) != (0, 0):
                continue  # one sign case of the deepest circuit is enough
            operator = {1: 1, 2: 2, 4: 3}[kat["op"]]
            rc, size, ok = _run_file_contract(ia, tmp_path, kat["op"], operator, kat["bits"], int(kat["a"]), kat["sa"],
                                              int(kat["b"]), kat["sb"], ctx=ctx)
            assert rc == kat["exit"]
            if rc == 126:  # Cannot multiply 256 bit number (cloud.c:860-864): 64 samples only
                assert size == 64 * S and not ok
                continue
            assert size == 352 * S and ok
            code, bit_size, words = tools.verif(tmp_path)
            assert bit_size == (2 * kat["bits"] if kat["op"] == 4 else kat["bits"])
            # value words = the magnitude circuit main() dispatches to (SURVEY 8a truth table)
            a_mag, b_mag, m = int(kat["a"]), int(kat["b"]), 1 << kat["bits"]
            neg = {0: 0, 2: 1}[kat["sa"]] + kat["sb"]
            if kat["op"] == 4:
                mag = a_mag * b_mag
            elif (kat["op"] == 1 and neg in (0, 3)) or (kat["op"] == 2 and neg in (1, 2)):
                mag = (a_mag + b_mag) % m
            elif (kat["op"] == 2 and neg == 0) or (kat["op"] == 1 and neg == 2):
                mag = (a_mag - b_mag) % m
            else:
                mag = (b_mag - a_mag) % m
            nw = bit_size // 32
            assert sum(w << (32 * i) for i, w in enumerate(words[:nw])) == mag, kat
            assert code == {0: 0, 1: 1, 2: 2, 3: 4}[neg] and words[nw:] == [0] * (9 - nw)
            # verif.c reads mixed-sign sums as two's complement, so it is only right while
            # |result| < 2^(bits-1); process.c's 2^(bits-2) operands sit exactly on that edge
            if abs(int(kat["expect"])) < (1 << (bit_size - 1)):
                assert tools.verif_interpret(kat["op"], code, bit_size, words) == int(kat["expect"]), kat
            # P2 through the file boundary: value samples equal the oracle's on the same cloud.data
            data = tools.read_samples(tmp_path / "cloud.data", p.n).reshape(22, 32, p.n + 1)
            rc2, ref = ck.cloud_values(kat["op"], neg, kat["bits"], data[2:10], data[13:21], data[10])
            ans = tools.read_samples(tmp_path / "answer.data", p.n).reshape(11, 32, p.n + 1)
            assert rc2 == 0 and np.array_equal(ans[2:], ref), kat
        # cloud.c reads exactly 22 arrays of 32 samples (:703-766; the 22nd, ciphertextcarry2, is read and never
        # used); anything a caller left behind them is not looked at, a shorter file is an I/O error
        _run_file_contract(ia, tmp_path, 1, 1, 32, 77, 0, 23, 0, ctx=ctx)
        good = (tmp_path / "cloud.data").read_bytes()
        assert len(good) == 704 * S and tools.verif_interpret(1, *tools.verif(tmp_path)) == 100
        (tmp_path / "cloud.data").write_bytes(good + good[:32 * S])  # a 23rd word
        rc, size, ok = ia.compute(1, tmp_path, ctx=ctx, failure_size=64 * S)
        assert (rc, ok) == (0, True) and tools.verif_interpret(1, *tools.verif(tmp_path)) == 100
        (tmp_path / "cloud.data").write_bytes(good[:-S])              # last sample of the 22nd word missing
        with pytest.raises(ia.IeacheError):
            ctx.cloud_run(tmp_path)
    # the `cloud` executable shim honours the same contract (exit code, files in cwd)
    rc, size, ok = _run_file_contract(ia, tmp_path, 1, 1, 32, 1 << 30, 0, 1 << 30, 0, use_subprocess=True)
    assert (rc, ok) == (0, True)
    assert tools.verif_interpret(1, *tools.verif(tmp_path)) == 1 << 31
    assert (tmp_path / "timings.txt").exists()
    rc, size, ok = _run_file_contract(ia, tmp_path, 4, 3, 256, 5, 0, 5, 0, use_subprocess=True)
    assert rc == 126 and size == 64 * S
    # chaining (compute_final): (a*b) then + c through answer.data -> cloud.data
    _run_file_contract(ia, tmp_path, 4, 3, 32, 1000, 0, 2000, 0)
    tools.alice(tmp_path, 0, 32, 77, seed=33)  # third operand alone in cloud.data
    rc, size, ok = ia.compute_final(1, tmp_path, flip=True, failure_size=64 * S)
    assert rc == 0 and ok
    code, bit_size, words = tools.verif(tmp_path)
    assert bit_size == 64 and tools.verif_interpret(1, code, bit_size, words) == 1000 * 2000 + 77
    assert (tmp_path / "averagestandard.txt").exists()  # MUL timing log (cloud.c:2467-2471)


def test_host_entry_points_keep_their_staging_rows(ia, gpu_ctx):
    """The host-buffer entry points (ieache_eval_batch -- what `cloud` and `cloudd` evaluate through --, ieache_gates, ieache_mux)
    stage operands and results in device rows the evaluator keeps between calls: a warm call (same or smaller size) makes no
    hipMalloc / hipFree -- each a device-wide synchronisation -- and a larger one grows the rows once.  Results do not depend on
    what an earlier, larger call left in the rows."""
    kb, ctx = gpu_ctx(4, 1024)
    rng = np.random.default_rng(5)
    vals = [(int(x), int(y)) for x, y in rng.integers(0, 1 << 16, size=(6, 2))]
    inp = _inputs(kb, 1, 16, vals, 19)
    big = ctx.eval_batch(1, 16, inp)                      # first use (or growth) of the operand and result rows
    n0 = ctx.get_option("staging_allocations")
    assert np.array_equal(ctx.eval_batch(1, 16, inp), big) and ctx.get_option("staging_allocations") == n0
    small = ctx.eval_batch(1, 16, inp[2:4])               # a smaller batch in the same rows, stale rows behind it
    assert np.array_equal(small, big[2:4]) and ctx.get_option("staging_allocations") == n0
    a, b, c = kb.enc(rng.integers(0, 2, size=40), 1), kb.enc(rng.integers(0, 2, size=40), 2), kb.enc(rng.integers(0, 2, size=40), 3)
    g1, m1 = ctx.gates(ia.GATE_NAND, a, b), ctx.mux(a, b, c)
    n1 = ctx.get_option("staging_allocations")
    assert np.array_equal(ctx.gates(ia.GATE_NAND, a, b), g1) and np.array_equal(ctx.mux(a, b, c), m1)
    assert np.array_equal(ctx.gates(ia.GATE_NAND, a[:7], b[:7]), g1[:7]) and ctx.get_option("staging_allocations") == n1
    for i in (0, 39):
        assert np.array_equal(kb.ck.gate("nand", a[i], b[i]), g1[i]) and np.array_equal(kb.ck.mux(a[i], b[i], c[i]), m1[i])
    inp2 = _inputs(kb, 1, 16, vals * 40, 19)              # 240 expressions: the rows grow (once), results unchanged
    out2 = ctx.eval_batch(1, 16, inp2)
    n2 = ctx.get_option("staging_allocations")
    assert n2 > n1 and np.array_equal(out2[:6], big) and np.array_equal(kb.dec(out2[234:]), kb.dec(big))
    assert np.array_equal(ctx.eval_batch(1, 16, inp2), out2) and ctx.get_option("staging_allocations") == n2
    assert ctx.eval_batch(1, 16, inp[:0]).shape[0] == 0


def test_cloud_file_contract_at_product_parameters(ia, tmp_path):
    """The ./cloud process contract at n=630 (cloud.c:650-917), through the `cloud` EXECUTABLE: keygen from the documented
    seeds, `alice` twice, operator.txt, ./cloud in that directory, `verif` -- BASELINE configs[0] (16-bit a+b, zero-extended in
    the 32-bit word), 32-bit SUBs (a > b and a < b), a 64-bit ADD, a 32-bit MUL, and the sign branches of main() (first /
    second / both operands negative: (-A)+B as B-A, A-(-B) as A+B at 64 bits, -(A+B) at 128 bits, (-A)-(-B) as B-A), a 256-bit ADD, a 128-bit SUB with borrows across words, 64- and 128-bit MULs with negative operands, and compute() followed by
    compute_final() ((a + b) - c through answer.data -> cloud.data).  2536-byte samples, the 114 MB key file through the codec, the fast
    kernels behind ieache_cloud_run; the 288 value samples of answer.data equal what the oracle's orc_cloud_values made of
    the same cloud.data (tests/golden/cloud_n630.json, make_golden.py cloud_n630).  A 256-bit MUL exits 126 and leaves
    exactly the 162 304 bytes the reference's caller tests for (Cloud/dragonfly_cipher_cloud.py:1295, cloud.c:860-864)."""
    import hashlib
    from ieache_amd import tools
    g = json.load(open(os.path.join(G, "cloud_n630.json")))
    p = ia.default_params()
    S = p.n + 1

    def digest(*arrays):
        h = hashlib.sha256()
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())
        return h.hexdigest()

    tools.keygen_files(tmp_path, p, seed=tuple(g["key_seed"]), nbit_seed=tuple(g["nbit_seed"]))
    assert os.path.getsize(tmp_path / "cloud.key") > 113_000_000
    _, bk, ksk = tools.read_cloud_key(tmp_path / "cloud.key")
    assert digest(bk, ksk) == g["cloud_key_sha256"]
    del bk, ksk
    assert g["sample_bytes"] == 2536 == 4 * p.n + 16
    for name, c in g["cases"].items():
        tools.alice(tmp_path, c["sign_a"], c["bits"], c["a"], seed=c["seed_a"])
        tools.alice(tmp_path, c["sign_b"], c["bits"], c["b"], seed=c["seed_b"], append=True)
        assert os.path.getsize(tmp_path / "cloud.data") == 704 * 2536
        assert digest(tools.read_samples(tmp_path / "cloud.data", p.n)) == c["cloud_data_sha256"], name
        if (tmp_path / "answer.data").exists():
            os.remove(tmp_path / "answer.data")
        rc, size, ok = ia.compute({1: 1, 2: 2, 4: 3}[c["operator"]], tmp_path, use_subprocess=True)
        assert (rc, ok) == (0, True) and size == 892672 == 352 * 2536, name
        ans = tools.read_samples(tmp_path / "answer.data", p.n)
        val = ans[64:]  # [neg, bit] are fresh encryptions (cloud.c:822-826); r1..r8 + the carry-word filler follow
        assert val.shape == (288, S)
        assert val[0].tolist() == c["first_value_sample"] and val[-1].tolist() == c["last_value_sample"], name
        assert digest(val) == c["value_samples_sha256"], name
        code, bit_size, words = tools.verif(tmp_path)
        assert bit_size == (2 * c["bits"] if c["operator"] == 4 else c["bits"])
        assert tools.verif_interpret(c["operator"], code, bit_size, words) == c["expect"], name
    # compute() then compute_final() through the files (dragonfly_cipher_cloud.py:1219-1327): (a + b) - c, the second run's
    # operands being the first run's answer words; value samples against the oracle's second stage
    ch = g.get("chain")
    if ch:
        c1 = g["cases"][ch["first"]]
        tools.alice(tmp_path, c1["sign_a"], c1["bits"], c1["a"], seed=c1["seed_a"])
        tools.alice(tmp_path, c1["sign_b"], c1["bits"], c1["b"], seed=c1["seed_b"], append=True)
        os.remove(tmp_path / "answer.data")
        assert ia.compute(1, tmp_path, use_subprocess=True)[::2] == (0, True)
        tools.alice(tmp_path, 0, ch["bits"], ch["c"], seed=ch["seed_c"])   # the third operand alone in cloud.data
        rc, size, ok = ia.compute_final(ch["operator"], tmp_path, flip=True, use_subprocess=True)
        assert (rc, ok) == (0, True) and size == 892672
        val = tools.read_samples(tmp_path / "answer.data", p.n)[64:]
        assert val[0].tolist() == ch["first_value_sample"] and val[-1].tolist() == ch["last_value_sample"]
        assert digest(val) == ch["value_samples_sha256"]
        code, bit_size, words = tools.verif(tmp_path)
        assert bit_size == ch["bits"] and tools.verif_interpret(ch["operator"], code, bit_size, words) == ch["expect"]
    # 256-bit operands cannot be multiplied: exit code 126 and the 64 metadata samples only
    tools.alice(tmp_path, 0, 256, 5, seed=1)
    tools.alice(tmp_path, 0, 256, 7, seed=2, append=True)
    os.remove(tmp_path / "answer.data")
    rc, size, ok = ia.compute(3, tmp_path, use_subprocess=True)
    assert rc == 126 and size == 162304 and not ok


def _inplace_gates(ia, ctx, a, b):
    """gates_device with the output written over the first operand."""
    import torch
    stride = ctx.lwe_stride
    da = torch.zeros((a.shape[0], stride), dtype=torch.int32, device="cuda")
    db = torch.zeros_like(da)
    da[:, : a.shape[1]] = torch.from_numpy(a).cuda()
    db[:, : b.shape[1]] = torch.from_numpy(b).cuda()
    torch.cuda.synchronize()
    ctx.gates_device(ia.GATE_AND, a.shape[0], da.data_ptr(), db.data_ptr(), da.data_ptr())
    return da.cpu().numpy()[:, : a.shape[1]]


def test_kernel_variants_agree_bit_for_bit(ia, gpu_ctx):
    """Fast (two-waves-per-gate, sliced), latency (2L-waves-per-gate) and generic kernels, every slice
    size, both key-switch kernels: all must produce identical bits (and the oracle's)."""
    kb, ctx = gpu_ctx(16, 1024)
    assert "radix8" in ctx.kernel_variant
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2, size=(2, 2304)).astype(np.uint8)
    a, b = kb.enc(bits[0], 41), kb.enc(bits[1], 42)
    ref = ctx.gates(ia.GATE_AND, a, b)                     # defaults: slice 16, sliced key switch (>= 576 gates)
    assert np.array_equal(kb.dec(ref), bits[0] & bits[1])
    for i in (0, 1, 2303):
        assert np.array_equal(kb.ck.gate("and", a[i], b[i]), ref[i])
    for sl in (1, 5, 16, 64):                              # n=16: 16, 4, 1, 1 launches; 5 leaves a ragged last slice
        ctx.set_option("br_slice", sl)
        assert np.array_equal(ctx.gates(ia.GATE_AND, a, b), ref), sl
    ctx.set_option("br_slice", 0)
    for variant in (9, 12):                                # two limbs: one wave per gate (round 4);
        ctx.set_option("br_variant", variant)              # two waves per gate with every transpose through LDS
        assert np.array_equal(ctx.gates(ia.GATE_AND, a[:301], b[:301]), ref[:301]), variant   # ragged last workgroup of 4 gates
    ctx.set_option("br_variant", 9)
    for sl in (1, 5, 64):
        ctx.set_option("br_slice", sl)
        assert np.array_equal(ctx.gates(ia.GATE_AND, a[:301], b[:301]), ref[:301]), sl
    ctx.set_option("br_slice", 0)
    ctx.set_option("br_variant", 7)                        # 2L-waves-per-gate (latency) kernel, forced for every launch size
    for sl in (16, 5, 4096):                               # sliced, ragged, whole rotation in one launch
        ctx.set_option("br_slice", sl)
        assert np.array_equal(ctx.gates(ia.GATE_AND, a[:600], b[:600]), ref[:600]), sl
    ctx.set_option("br_slice", 0)
    # the one-limb kernels, each forced for this launch size: 31 / 32 / 35 k_blind_rotate_w1b (guard on one coefficient in four /
    # on every one / none), 36 / 37 k_blind_rotate_w2r, 38 / 39 k_blind_rotate_wide4, 43 / 44 k_blind_rotate_w4r, 24 round 2's
    # latency kernel on one limb; ragged last workgroup of 4 gates
    for variant in (24, 31, 32, 35, 36, 37, 38, 39, 43, 44):
        ctx.set_option("br_variant", variant)
        assert np.array_equal(ctx.gates(ia.GATE_AND, a[:301], b[:301]), ref[:301]), variant
    for variant in (31,):
        ctx.set_option("br_variant", variant)
        for sl in (1, 5, 64):
            ctx.set_option("br_slice", sl)
            assert np.array_equal(ctx.gates(ia.GATE_AND, a[:301], b[:301]), ref[:301]), (variant, sl)
    ctx.set_option("br_slice", 0)
    ctx.set_option("br_variant", 0)
    dev, reruns = ctx.fft_guard()
    assert 0 < dev < 1 / 16 and reruns == 0                # rounding stayed far from the 0.5 that would flip a bit
    ctx.set_option("exact_fft", 1)                         # two-limb (provably exact) kernel for every launch size
    assert np.array_equal(ctx.gates(ia.GATE_AND, a, b), ref)
    # ... which kernel by launch size: 2L waves per gate up to one per CU, two waves per gate up to four per CU, one wave per
    # gate above ("exact_one_wave_min" moves that boundary)
    cus = ctx.get_option("cus")                            # 256 on an MI355X: the boundaries below are per CU
    one_wave_min = ctx.get_option("exact_one_wave_min")
    assert one_wave_min == 4 * cus + 1
    assert [ctx.kernel_for_launch(c).split("<")[0] for c in (cus - 56, cus + 44, 4 * cus, 4 * cus + 1)] == \
        ["k_blind_rotate_wide", "k_blind_rotate_w2", "k_blind_rotate_w2", "k_blind_rotate_x1"]
    ctx.set_option("exact_one_wave_min", 0)
    assert ctx.kernel_for_launch(300).startswith("k_blind_rotate_x1") and np.array_equal(ctx.gates(ia.GATE_AND, a[:300], b[:300]), ref[:300])
    ctx.set_option("exact_one_wave_min", one_wave_min)
    ctx.set_option("exact_fft", 0)
    ctx.set_option("fft_guard_inject", 1)                  # a tripped guard makes the call repeat itself on the two-limb kernel
    assert np.array_equal(ctx.gates(ia.GATE_AND, a, b), ref)
    assert ctx.fft_guard()[1] == 1
    assert np.array_equal(ctx.gates(ia.GATE_AND, a, b), ref) and ctx.fft_guard()[1] == 1
    # in-place call: it could not be repeated (the first attempt overwrites its inputs), so it runs on the two-limb kernels
    # from the start -- right bits, no rerun counted, and an injected guard trip is simply folded away
    ctx.set_option("fft_guard_inject", 1)
    assert np.array_equal(_inplace_gates(ia, ctx, a[:600], b[:600]), ref[:600]) and ctx.fft_guard()[1] == 1
    # the sampled audit: with fft_audit = 1 every one-limb launch has 64 of its gates re-run on the two-limb kernel and compared
    base = ctx.fft_audit()
    ctx.set_option("fft_audit", 1)
    assert np.array_equal(ctx.gates(ia.GATE_AND, a, b), ref)           # one launch of 2304 gates: one audit of 64
    assert np.array_equal(ctx.gates(ia.GATE_AND, a[:37], b[:37]), ref[:37])  # latency kernel on one limb: all 37 audited
    au = ctx.fft_audit()
    assert au["audits"] == base["audits"] + 2 and au["gates_compared"] == base["gates_compared"] + 64 + 37
    assert au["mismatches"] == base["mismatches"] == 0 and ctx.fft_guard()[1] == 1
    ctx.set_option("fft_audit_inject", 1)                  # a differing row makes the call repeat itself on the two-limb kernels
    assert np.array_equal(ctx.gates(ia.GATE_AND, a, b), ref)
    au2 = ctx.fft_audit()
    assert au2["mismatches"] == 1 and au2["audits"] == au["audits"] + 1 and ctx.fft_guard()[1] == 2
    ctx.set_option("exact_fft", 1)                         # nothing to audit on the two-limb kernels
    ctx.gates(ia.GATE_AND, a[:600], b[:600])
    assert ctx.fft_audit() == au2
    ctx.set_option("exact_fft", 0)
    ctx.set_option("fft_audit", 64)
    ctx.set_option("one_limb_min", 0)                      # one-limb kernel down to a single gate
    ctx.set_option("br_wide_max", 0)
    assert np.array_equal(ctx.gates(ia.GATE_AND, a[:1], b[:1]), ref[:1])
    assert np.array_equal(ctx.gates(ia.GATE_AND, a[:7], b[:7]), ref[:7])
    ctx.set_option("one_limb_min", 257)
    ctx.set_option("br_wide_max", 256)
    # policy: launches of <= br_wide_max gates take the wide kernel by themselves (default = CU count)
    assert np.array_equal(ctx.gates(ia.GATE_AND, a[:200], b[:200]), ref[:200])
    ctx.set_option("br_wide_max", 0)
    assert np.array_equal(ctx.gates(ia.GATE_AND, a[:200], b[:200]), ref[:200])
    ctx.set_option("br_wide_max", 1 << 20)
    assert np.array_equal(ctx.gates(ia.GATE_AND, a, b), ref)
    ctx.set_option("br_wide_max", 256)
    # key switch: the defaults above took the int8 MFMA product (>= 64 gates per launch); its K splits, ragged gate blocks ...
    for split, cnt in ((1, 2304), (2, 2304), (4, 513), (8, 64), (8, 65), (0, 1000)):
        ctx.set_option("ks_mfma_split", split)
        assert np.array_equal(ctx.gates(ia.GATE_AND, a[:cnt], b[:cnt]), ref[:cnt]), (split, cnt)
    ctx.set_option("ks_mfma_split", 0)
    ctx.set_option("ks_mfma_min", 1)                       # ... and down to a single gate
    for cnt in (1, 5, 37):
        assert np.array_equal(ctx.gates(ia.GATE_AND, a[:cnt], b[:cnt]), ref[:cnt]), cnt
    # now every walk kernel: the hand-scheduled sliced one (round 2's default from 576 gates) ...
    ctx.set_option("ks_mfma_min", 1 << 40)
    assert np.array_equal(ctx.gates(ia.GATE_AND, a, b), ref)
    # ... and the others
    ctx.set_option("ks_sliced_min", 1 << 40)
    ctx.set_option("ks_batch_min", 1 << 40)                # per-gate vectorised key switch
    assert np.array_equal(ctx.gates(ia.GATE_AND, a, b), ref)
    for splits in (1, 2, 16, 64):                          # per-gate kernel with a gate's walk cut into several workgroups
        ctx.set_option("ks_split_max", splits)             # (tiny launches; partial sums meet through atomic adds)
        for cnt in (1, 5, 37, 200):
            assert np.array_equal(ctx.gates(ia.GATE_AND, a[:cnt], b[:cnt]), ref[:cnt]), (splits, cnt)
    ctx.set_option("ks_split_max", 16)
    ctx.set_option("ks_batch_min", 1)                      # gate-batched key switch even for tiny launches
    assert np.array_equal(ctx.gates(ia.GATE_AND, a[:37], b[:37]), ref[:37])  # ragged last group of 16
    ctx.set_option("ks_batch_min", 4096)
    ctx.set_option("ks_sliced_min", 1)                     # sliced key switch: 8 / 16 / 32 gates per workgroup,
    for gates, sl, cnt in ((8, 0, 2304), (16, 5, 2304), (32, 64, 2304), (32, 1024, 37), (8, 3, 1), (4, 0, 2304), (4, 7, 5),
                           (0, 0, 2304)):
        ctx.set_option("ks_gates", gates)                  # whole walk or ragged slices, ragged last groups
        ctx.set_option("ks_slice", sl)
        assert np.array_equal(ctx.gates(ia.GATE_AND, a[:cnt], b[:cnt]), ref[:cnt]), (gates, sl, cnt)
    ctx.set_option("ks_gates", 0)
    ctx.set_option("ks_slice", 0)
    ctx.set_option("ks_sliced_min", 576)
    ctx.set_option("ks_mfma_min", 64)
    with pytest.raises(ia.IeacheError):
        ctx.set_option("ks_gates", 12)
    for bad in (3, 5, 48):                                 # K splits that do not divide the walk are refused when set, not mid-evaluation
        with pytest.raises(ia.IeacheError):
            ctx.set_option("ks_mfma_split", bad)
    ctx.force_generic(True)
    assert ctx.kernel_variant == "generic-radix2"
    assert np.array_equal(ctx.gates(ia.GATE_AND, a[:64], b[:64]), ref[:64])
    ctx.force_generic(False)
    for gone in (13, 20, 41, 61):                          # kernels of earlier rounds that lost their A/B (csrc/attic), and no kernel at all
        with pytest.raises(ia.IeacheError):
            ctx.set_option("br_variant", gone)
    with pytest.raises(ia.IeacheError):
        ctx.set_option("br_slice", 4097)
    with pytest.raises(ia.IeacheError):
        ctx.set_option("no_such_knob", 1)


def test_flat_mux_cuts_guard_and_audit(ia, gpu_ctx):
    """A flat MUX call under everything a flat gate call goes through: odd and minimal chunks (pieces are whole gates: 3, 1 and
    1 of them), the sampled audit, a guard repeat, the two-limb and the any-parameter kernels, an in-place device call and warm
    staging rows.  37 gates = 74 blind rotations: a ragged last piece, and room for an audit's 64 consecutive items.  Every
    row equals the oracle's bootsMUX.  (Companion of test_mux_gate_bit_exact; it stands here because it adds guard repeats and
    an audit mismatch to the session's shared context, whose counts test_kernel_variants_agree_bit_for_bit reads from zero.)"""
    import torch
    kb, ctx = gpu_ctx(16, 1024)
    rng = np.random.default_rng(37)
    bits = rng.integers(0, 2, size=(3, 37)).astype(np.uint8)
    a, b, c = kb.enc(bits[0], 84), kb.enc(bits[1], 85), kb.enc(bits[2], 86)
    want = np.stack([kb.ck.mux(a[i], b[i], c[i]) for i in range(37)])
    assert np.array_equal(kb.dec(want), np.where(bits[0] == 1, bits[1], bits[2]))
    try:
        for chunk, pieces in ((7, 13), (2, 37), (1, 37)):
            ctx.set_chunk(chunk)
            st = ia.Stats()
            assert np.array_equal(ctx.mux(a, b, c, st), want), chunk
            assert st.keyswitch_launches == pieces and st.bootstraps == 74, (chunk, st.keyswitch_launches, st.bootstraps)
    finally:
        ctx.set_chunk(16384)
    reruns, base = ctx.fft_guard()[1], ctx.fft_audit()
    try:
        ctx.set_option("fft_audit", 1)
        ctx.set_option("fft_audit_inject", 1)      # a differing audited row: the call repeats itself on the two-limb kernels
        assert np.array_equal(ctx.mux(a, b, c), want)
        assert ctx.fft_audit()["mismatches"] == base["mismatches"] + 1 and ctx.fft_guard()[1] == reruns + 1
    finally:
        ctx.set_option("fft_audit", 64)            # (the two injection hooks clear themselves when they have been used)
    ctx.set_option("fft_guard_inject", 1)          # a tripped guard: one more repeat
    assert np.array_equal(ctx.mux(a, b, c), want) and ctx.fft_guard()[1] == reruns + 2
    try:
        ctx.set_option("exact_fft", 1)
        assert np.array_equal(ctx.mux(a, b, c), want) and ctx.fft_guard()[1] == reruns + 2
    finally:
        ctx.set_option("exact_fft", 0)
    try:
        ctx.force_generic(True)
        assert np.array_equal(ctx.mux(a, b, c), want)
    finally:
        ctx.force_generic(False)
    # in place, d_out == d_a: it could not be repeated, so it runs on the two-limb kernels from the start -- no rerun counted
    d = [torch.zeros((37, ctx.lwe_stride), dtype=torch.int32, device="cuda") for _ in range(3)]
    for t, rows in zip(d, (a, b, c)):
        t[:, : rows.shape[1]] = torch.from_numpy(rows).cuda()
    torch.cuda.synchronize()
    ctx.mux_device(37, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[0].data_ptr())
    assert np.array_equal(d[0].cpu().numpy()[:, : a.shape[1]], want) and ctx.fft_guard()[1] == reruns + 2
    n0 = ctx.get_option("staging_allocations")    # the host calls above have grown the rows: a warm one allocates nothing
    assert np.array_equal(ctx.mux(a, b, c), want) and ctx.get_option("staging_allocations") == n0


def test_level_overlap_on_two_streams_same_bits(ia, gpu_ctx):
    """Option "overlap": a level of at least overlap_min gate instances is issued as pieces alternating between two streams of the
    context (own scratch per stream, one key copy, event join before the next level).  Same launches on the same gate instances:
    every output word equals the one-stream run's and the oracle's -- flat gates and circuits, odd sizes, pieces smaller than
    half a level (chunk), an audit on every launch of both streams."""
    kb, ctx = gpu_ctx(16, 1024)
    assert ctx.get_option("overlap") == 1 and ctx.get_option("overlap_min") == 16 * ctx.get_option("cus")
    rng = np.random.default_rng(77)
    bits = rng.integers(0, 2, size=(2, 4999)).astype(np.uint8)
    a, b = kb.enc(bits[0], 31), kb.enc(bits[1], 32)
    ctx.set_option("overlap", 0)
    ref = ctx.gates(ia.GATE_XOR, a, b)
    assert np.array_equal(kb.dec(ref), bits[0] ^ bits[1])
    for i in (0, 2499, 2500, 4998):
        assert np.array_equal(kb.ck.gate("xor", a[i], b[i]), ref[i])
    ctx.set_option("overlap", 1)
    audit0 = ctx.fft_audit()  # counts over the (shared) context's life
    try:
        for omin, chunk, audit in ((4096, 65536, 64), (2, 65536, 1), (1000, 700, 64), (2, 1, 0)):
            ctx.set_option("overlap_min", omin)
            ctx.set_chunk(chunk)
            ctx.set_option("fft_audit", audit)
            n = 4999 if chunk > 1 else 37  # chunk 1: one gate per piece, 37 pieces on alternating streams
            before = ctx.get_option("overlapped_levels")
            st = ia.Stats()
            out = ctx.gates(ia.GATE_XOR, a[:n], b[:n], st)
            assert np.array_equal(out, ref[:n]), (omin, chunk)
            assert ctx.get_option("overlapped_levels") == before + 1 and st.bootstraps == n
            pieces = -(-n // min(chunk, (((n + 1) // 2) + 3) & ~3))
            assert st.chunks == pieces and st.keyswitch_launches == pieces, (st.chunks, pieces)
        audit1 = ctx.fft_audit()
        assert audit1["mismatches"] == audit0["mismatches"] and audit1["audits"] >= audit0["audits"] + 2  # both streams' launches audited
        # below overlap_min nothing changes: one stream, one piece
        ctx.set_option("overlap_min", 5000)
        ctx.set_chunk(65536)
        before = ctx.get_option("overlapped_levels")
        st = ia.Stats()
        assert np.array_equal(ctx.gates(ia.GATE_XOR, a, b, st), ref) and st.chunks == 1
        assert ctx.get_option("overlapped_levels") == before
        # a circuit: every level of add16 x 40 (40 or 80 gate instances) on two streams, against the sequential oracle
        vals = [(int(x), int(y)) for x, y in rng.integers(0, 1 << 16, size=(40, 2))]
        inp = _inputs(kb, 1, 16, vals, 9)
        ctx.set_option("overlap", 0)
        cref = ctx.eval_batch(1, 16, inp)
        ctx.set_option("overlap", 1)
        ctx.set_option("overlap_min", 40)
        before = ctx.get_option("overlapped_levels")
        st = ia.Stats()
        cout = ctx.eval_batch(1, 16, inp, st)
        assert np.array_equal(cout, cref) and ctx.get_option("overlapped_levels") == before + 48 and st.chunks == 96
        s, _ = kb.ck.add(inp[7, :16], inp[7, 16:32], inp[7, 32:33], 16)
        assert np.array_equal(s, cout[7])
        assert ctx.get_option("pipelined_evals") == 0  # 80 x 40 gate instances over 48 levels is below pipe_min (8 per CU and level)
        # ... and as two PIPELINES: the batch cut into two halves of expressions, each through all 48 levels on its own stream with
        # no join in between ("pipe_min" lowered so that this small batch qualifies); odd batches, two expressions, chunked pieces
        ctx.set_option("pipe_min", 1)
        for nb, chunk in ((40, 65536), (39, 65536), (2, 65536), (40, 7)):
            ctx.set_chunk(chunk)
            before, lv = ctx.get_option("pipelined_evals"), ctx.get_option("overlapped_levels")
            st = ia.Stats()
            pout = ctx.eval_batch(1, 16, inp[:nb], st)
            assert np.array_equal(pout, cref[:nb]), (nb, chunk)
            assert ctx.get_option("pipelined_evals") == before + 1 and ctx.get_option("overlapped_levels") == lv
            assert st.levels == 48 and st.bootstraps == 80 * nb and st.chunks >= 96
        ctx.set_chunk(65536)
        # a tripped guard / a differing audited row under pipelines: the call repeats itself on the two-limb kernels (as pipelines too)
        reruns = ctx.fft_guard()[1]
        ctx.set_option("fft_guard_inject", 1)
        assert np.array_equal(ctx.eval_batch(1, 16, inp), cref) and ctx.fft_guard()[1] == reruns + 1
        ctx.set_option("fft_audit", 1)
        ctx.set_option("fft_audit_inject", 1)
        assert np.array_equal(ctx.eval_batch(1, 16, inp), cref) and ctx.fft_guard()[1] == reruns + 2
        ctx.set_option("fft_audit", 64)
        for lanes, nb in ((3, 40), (4, 39), (4, 3)):       # more pipelines ("pipe_lanes"): ragged slices; never more than expressions
            ctx.set_option("pipe_lanes", lanes)
            st = ia.Stats()
            assert np.array_equal(ctx.eval_batch(1, 16, inp[:nb], st), cref[:nb]), (lanes, nb)
            assert st.chunks == 48 * min(lanes, nb) and st.bootstraps == 80 * nb
        ctx.set_option("pipe_lanes", 2)
        assert not ctx.set_option_ok("pipe_lanes", 5) and not ctx.set_option_ok("pipe_lanes", 1)
        # "pipe_auto": a mean level between pipe_min / 8 and pipe_min (here 3 200 gate instances over 48 levels against pipe_min 300)
        # is tried both ways -- evaluations 1 and 3 without pipelines, 2 and 4 with -- and then stays with the faster mode;
        # every one of them gives the same bits
        ctx.set_option("pipe_min", 300)
        ctx.set_option("pipe_auto", 1)  # (re)starts the trials
        p0, t0 = ctx.get_option("pipelined_evals"), ctx.get_option("tuned_evals")
        seen = []
        for i in range(6):
            before = ctx.get_option("pipelined_evals")
            assert np.array_equal(ctx.eval_batch(1, 16, inp), cref), i
            seen.append(ctx.get_option("pipelined_evals") - before)
        assert seen[:4] == [0, 1, 0, 1] and seen[4] == seen[5] and ctx.get_option("tuned_evals") == t0 + 4, seen
        ctx.set_option("pipe_auto", 0)  # off: below pipe_min there are no pipelines
        before = ctx.get_option("pipelined_evals")
        assert np.array_equal(ctx.eval_batch(1, 16, inp), cref) and ctx.get_option("pipelined_evals") == before
        ctx.set_option("pipe_auto", 1)
        ctx.set_option("pipe_min", 1)
        before = ctx.get_option("pipelined_evals")
        assert np.array_equal(ctx.eval_batch(1, 16, inp[:1]), cref[:1]) and ctx.get_option("pipelined_evals") == before  # one expression: one stream
        ctx.set_option("exact_fft", 1)
        assert np.array_equal(ctx.eval_batch(1, 16, inp), cref) and ctx.get_option("pipelined_evals") == before + 1
        ctx.set_option("exact_fft", 0)
        ctx.set_option("pipe_min", 8 * ctx.get_option("cus"))
        # the exact (two-limb) kernels and the MUX gate (never overlapped: its two rotations feed one key switch) are unaffected
        ctx.set_option("exact_fft", 1)
        assert np.array_equal(ctx.eval_batch(1, 16, inp), cref)
        ctx.set_option("exact_fft", 0)
        c = kb.enc(rng.integers(0, 2, size=100).astype(np.uint8), 33)
        m1 = ctx.mux(a[:100], b[:100], c)
        ctx.set_option("overlap", 0)
        assert np.array_equal(ctx.mux(a[:100], b[:100], c), m1)
    finally:
        ctx.set_option("overlap", 1)
        ctx.set_option("overlap_min", 16 * ctx.get_option("cus"))
        ctx.set_option("pipe_min", 8 * ctx.get_option("cus"))
        ctx.set_chunk(65536)
        ctx.set_option("fft_audit", 64)
    assert not ctx.set_option_ok("overlap", 2) and not ctx.set_option_ok("overlap_min", 1)


def test_level_overlap_at_product_parameters(ia, gpu_ctx):
    """n=630: 4 608 XOR gates as one launch (overlap 0) and as two halves of 2 304 on two streams: identical words, oracle on samples,
    and the exact two-limb kernels under overlap as well."""
    kb, ctx = gpu_ctx(630, 1024)
    rng = np.random.default_rng(78)
    bits = rng.integers(0, 2, size=(2, 4608)).astype(np.uint8)
    a, b = kb.enc(bits[0], 41), kb.enc(bits[1], 42)
    ctx.set_option("overlap", 0)
    ref = ctx.gates(ia.GATE_XOR, a, b)
    ctx.set_option("overlap", 1)
    before = ctx.get_option("overlapped_levels")
    st = ia.Stats()
    out = ctx.gates(ia.GATE_XOR, a, b, st)
    assert ctx.get_option("overlapped_levels") == before + 1 and st.chunks == 2
    assert np.array_equal(out, ref) and np.array_equal(kb.dec(out), bits[0] ^ bits[1])
    for i in (0, 2303, 2304, 4607):
        assert np.array_equal(kb.ck.gate("xor", a[i], b[i]), out[i]), i
    ctx.set_option("exact_fft", 1)
    try:
        assert np.array_equal(ctx.gates(ia.GATE_XOR, a, b), ref)
    finally:
        ctx.set_option("exact_fft", 0)


def test_edge_cases_empty_batch_and_chunking(ia, gpu_ctx):
    kb, ctx = gpu_ctx(4, 1024)
    info = ia.circuit_info(ia.CIRC_ADD, 32)
    empty = ctx.eval_batch(ia.CIRC_ADD, 32, np.zeros((0, info.n_inputs, kb.p.n + 1), np.int32))
    assert empty.shape == (0, 32, kb.p.n + 1)
    assert ctx.gates(ia.GATE_AND, np.zeros((0, kb.p.n + 1), np.int32), np.zeros((0, kb.p.n + 1), np.int32)).shape[0] == 0
    vals = [(0xFFFFFFFF, 0xFFFFFFFF), (0, 0), (1, 0xFFFFFFFF), (0x80000000, 0x80000000), (12345, 67890)]
    inp = _inputs(kb, 2, 32, vals, 17)
    ref = ctx.eval_batch(ia.CIRC_SUB, 32, inp)
    # ieache_prepare_batch: allocations ahead of an evaluation -- idempotent, for a batch larger and smaller than the last one, an
    # empty batch, an unknown circuit refused; the evaluation after it produces the same bits
    for b in (len(vals), 64, 0, len(vals)):
        ctx.prepare(ia.CIRC_SUB, 32, b)
    with pytest.raises(ia.IeacheError):
        ctx.prepare(99, 32, 4)
    assert np.array_equal(ctx.eval_batch(ia.CIRC_SUB, 32, inp), ref)
    ctx.set_chunk(7)  # every level split into ragged chunks
    st = ia.Stats()
    assert np.array_equal(ctx.eval_batch(ia.CIRC_SUB, 32, inp, st), ref)
    assert st.chunks > st.levels
    ctx.set_chunk(16384)
    ctx.force_generic(True)  # generic kernels on a whole circuit
    assert np.array_equal(ctx.eval_batch(ia.CIRC_SUB, 32, inp), ref)
    ctx.force_generic(False)
    with pytest.raises(ia.IeacheError):
        ctx.eval_batch_device(99, 32, 1, 1, 1)  # unknown circuit kind: refused before any pointer is touched
    with pytest.raises(ia.IeacheError, match="not a device pointer"):
        ctx.eval_batch_device(ia.CIRC_ADD, 32, 1, 4096, 8192)  # stray addresses never reach a kernel
    host = np.zeros((1, 96, kb.p.n + 1), np.int32)
    with pytest.raises(ia.IeacheError, match="not a device pointer"):
        ctx.eval_batch_device(ia.CIRC_ADD, 32, 1, host.ctypes.data, host.ctypes.data)


def test_kogge_stone_adders_decrypt_identically(ia, gpu_ctx):
    """Opt-in parallel-prefix adders: same plaintext as the reference's ripple adders, fewer levels."""
    kb, ctx = gpu_ctx(4, 1024)
    from ieache_amd.tools import bits_to_int
    vals = [(0xFFFFFFFF, 1), (0x12345678, 0x9ABCDEF0), (0, 0), (0x80000000, 0x80000000)]
    inp = _inputs(kb, 1, 32, vals, 23)
    for ks_kind, rc_kind, f in ((ia.CIRC_ADD_KS, ia.CIRC_ADD, lambda a, b: a + b), (ia.CIRC_SUB_KS, ia.CIRC_SUB, lambda a, b: a - b),
                                (ia.CIRC_RSUB_KS, ia.CIRC_RSUB, lambda a, b: b - a)):
        st = ia.Stats()
        out = ctx.eval_batch(ks_kind, 32, inp, st)
        ref = ctx.eval_batch(rc_kind, 32, inp)
        assert st.levels == 13
        assert np.array_equal(kb.dec(out), kb.dec(ref))
        assert [bits_to_int(d) for d in kb.dec(out)] == [f(a, b) & 0xFFFFFFFF for a, b in vals]


def test_carry_save_multiplier_decrypts_identically(ia, gpu_ctx, tmp_path):
    """Opt-in CIRC_MUL_WALLACE / IEACHE_MULTIPLIER=wallace: same plaintext as the reference's shift-add multipliers,
    37 / 43 levels instead of 255 / 449."""
    kb, ctx = gpu_ctx(4, 1024)
    from ieache_amd.tools import bits_to_int
    for bits, levels in ((32, 37), (64, 43)):
        m = 1 << bits
        vals = [(m - 1, m - 1), (0xDEADBEEF % m, 0x12345678), (0, 12345), (1 << (bits - 2), 1 << (bits - 2))]
        inp = _inputs(kb, ia.CIRC_MUL_WALLACE, bits, vals, 27)
        st = ia.Stats()
        out = ctx.eval_batch(ia.CIRC_MUL_WALLACE, bits, inp, st)
        info = ia.circuit_info(ia.CIRC_MUL_WALLACE, bits)
        assert st.levels == info.depth == levels and st.bootstraps == info.bootstraps * len(vals)
        assert [bits_to_int(d) for d in kb.dec(out)] == [a * b for a, b in vals]
        if bits == 32:
            assert np.array_equal(kb.dec(out), kb.dec(ctx.eval_batch(ia.CIRC_MUL, bits, inp)))
    # through the process contract
    from ieache_amd import tools
    p = ia.default_params().copy(n=6, N=64)
    tools.keygen_files(tmp_path, p)
    os.environ["IEACHE_MULTIPLIER"] = "wallace"
    try:
        rc, size, ok = _run_file_contract(ia, tmp_path, 4, 3, 64, 0xFEDCBA9876543210, 0, 0x0F1E2D3C4B5A6978, 2)
    finally:
        del os.environ["IEACHE_MULTIPLIER"]
    assert rc == 0 and ok
    code, bit_size, words = tools.verif(tmp_path)
    assert (code, bit_size) == (2, 128)
    assert sum(w << (32 * i) for i, w in enumerate(words[:4])) == 0xFEDCBA9876543210 * 0x0F1E2D3C4B5A6978
    assert (tmp_path / "averagestandard.txt").exists()


def test_batch_aware_level_width_same_bits(ia, gpu_ctx):
    """"level_quantum" re-levels the 64/128-bit multipliers for the batch at hand (here 32 expressions: levels of 64 gates
    = exactly one round of the 2 048 gates the one-wave kernel keeps resident); the DAG is the same, so every output sample is."""
    kb, ctx = gpu_ctx(4, 1024)
    rng = np.random.default_rng(16)
    vals = [(int.from_bytes(rng.bytes(8), "little"), int.from_bytes(rng.bytes(8), "little")) for _ in range(32)]
    inp = _inputs(kb, 4, 64, vals, 33)
    resident = 8 * 256
    cap = ia.circuit_level_cap(4, 64, 32, resident)
    assert cap == 64
    st = ia.Stats()
    out = ctx.eval_batch(4, 64, inp, st)
    assert st.levels == ia.circuit_info(4, 64, level_cap=cap).sched_levels > 449 and st.bootstraps == 32 * 35296
    ctx.set_option("level_quantum", 0)
    try:
        st0 = ia.Stats()
        ref = ctx.eval_batch(4, 64, inp, st0)
    finally:
        ctx.set_option("level_quantum", 1)
    assert st0.levels == 449 and np.array_equal(out, ref)
    from ieache_amd.tools import bits_to_int
    assert [bits_to_int(d) for d in kb.dec(out)] == [a * b for a, b in vals]
    # the ASAP-scheduled 32-bit multiplier at a small batch: 58 expressions get levels of 35 gates (58 x 35 = one round)
    vals32 = [(int(rng.integers(0, 2**32)), int(rng.integers(0, 2**32))) for _ in range(58)]
    inp32 = _inputs(kb, 4, 32, vals32, 34)
    st = ia.Stats()
    out32 = ctx.eval_batch(4, 32, inp32, st)
    assert st.levels == ia.circuit_info(4, 32, level_cap=35).sched_levels == 334 and st.bootstraps == 58 * 11264
    ctx.set_option("level_quantum", 0)
    try:
        st0 = ia.Stats()
        ref32 = ctx.eval_batch(4, 32, inp32, st0)
    finally:
        ctx.set_option("level_quantum", 1)
    assert st0.levels == 255 and np.array_equal(out32, ref32)
    assert [bits_to_int(d) for d in kb.dec(out32)] == [a * b for a, b in vals32]


def test_full_size_random_gates_bit_exact_soak(ia, gpu_ctx):
    """A wider bit-exact sweep at n=630, N=1024: random gate types and operands, including
    operands that are themselves bootstrapped outputs and NOT-ed inputs (the oracle takes ~0.4 s/gate)."""
    z = np.load(os.path.join(G, "full_gate_kat.npz"))
    kb, ctx = gpu_ctx(630, 1024, seed=tuple(int(v) for v in z["seed"]))
    reruns0 = ctx.fft_guard()[1]  # the context is shared with tests that inject guard trips
    rng = np.random.default_rng(77)
    n_g = 24
    bits = rng.integers(0, 2, size=(2, n_g)).astype(np.uint8)
    a, b = kb.enc(bits[0], 51), kb.enc(bits[1], 52)
    a[::3] = (0 - a[::3].astype(np.int64)).astype(np.int32)      # bootsNOT of every third operand
    abits = bits[0].copy()
    abits[::3] ^= 1
    first = ctx.gates(ia.GATE_XOR, a, b)                          # level 1
    second = ctx.gates(ia.GATE_AND, first, b)                     # level 2 consumes bootstrapped outputs
    assert np.array_equal(kb.dec(first), abits ^ bits[1])
    assert np.array_equal(kb.dec(second), (abits ^ bits[1]) & bits[1])
    for i in range(n_g):
        r1 = kb.ck.gate("xor", a[i], b[i])
        assert np.array_equal(r1, first[i]), i
        assert np.array_equal(kb.ck.gate("and", r1, b[i]), second[i]), i
    # the same gates on the kernel wide launches take (one wave per gate, one-limb spectrum, rounding guard) and on the
    # two-wave two-limb kernel: 24 gates go to the latency kernel unless told otherwise
    for opts in ({"one_limb_min": 0, "br_wide_max": 0, "two_wave_max": 0}, {"two_wave_max": 1024}, {"exact_fft": 1}):
        for k, v in opts.items():
            ctx.set_option(k, v)
        f2 = ctx.gates(ia.GATE_XOR, a, b)
        assert np.array_equal(f2, first) and np.array_equal(ctx.gates(ia.GATE_AND, f2, b), second), opts
    dev, reruns = ctx.fft_guard()
    assert 0 < dev < 1 / 32 and reruns == reruns0
    ctx.set_option("exact_fft", 0)
    cus = ctx.get_option("cus")
    ctx.set_option("one_limb_min", cus + 1)
    ctx.set_option("br_wide_max", cus)
    ctx.set_option("two_wave_max", 5 * cus)


def test_one_limb_kernels_match_two_limb_over_many_gates(ia, gpu_ctx):
    """The guarded one-limb kernels against the provably exact two-limb ones at n=630 on 16 384 gates per level, five levels
    deep (each level's operands are the previous level's bootstrapped outputs): every sample identical, the guard silent
    with its maximum far below the limit.  (GPU against GPU: the oracle takes 0.4 s per gate; it pins the two-limb kernels
    in the tests above.)"""
    z = np.load(os.path.join(G, "full_gate_kat.npz"))
    kb, ctx = gpu_ctx(630, 1024, seed=tuple(int(v) for v in z["seed"]))
    reruns0 = ctx.fft_guard()[1]  # the context is shared with tests that inject guard trips
    rng = np.random.default_rng(630)
    cnt = 16384
    bits = rng.integers(0, 2, size=(2, cnt)).astype(np.uint8)
    a, b = kb.enc(bits[0], 71), kb.enc(bits[1], 72)
    results = {}
    for exact in (1, 0):
        ctx.set_option("exact_fft", exact)
        x, y, plain_x, plain_y = a, b, bits[0], bits[1]
        outs = []
        for level, gate in enumerate((ia.GATE_XOR, ia.GATE_AND, ia.GATE_OR, ia.GATE_NAND, ia.GATE_XOR)):
            o = ctx.gates(gate, x, y)
            outs.append(o)
            x, y = o, np.roll(x, 1, axis=0)                 # next level: this level's outputs against shifted operands
        results[exact] = outs
    for lvl, (e, f) in enumerate(zip(results[1], results[0])):
        assert np.array_equal(e, f), lvl
    dev, reruns = ctx.fft_guard()
    assert 0 < dev < 1 / 32 and reruns == reruns0
    assert np.array_equal(kb.dec(results[0][0]), bits[0] ^ bits[1])
    # a mid-size launch (two waves per gate) and a narrow one (latency kernel) of the same gates; the names the library
    # reports for those launch sizes (bench.py labels each leg's roofline record with them)
    names = [ctx.kernel_for_launch(c).split("<")[0] for c in (200, 400, 900, cnt)]
    assert names[0] == "k_blind_rotate_wide4" and names[3] == "k_blind_rotate_w1b" and len(set(names)) == 4, names
    assert ctx.kernel_for_launch(900).endswith("<3,7>")
    ctx.set_option("exact_fft", 1)
    assert [ctx.kernel_for_launch(c).split("<")[0] for c in (200, 900, cnt)] == ["k_blind_rotate_wide", "k_blind_rotate_w2", "k_blind_rotate_x1"]
    ctx.set_option("exact_fft", 0)
    mid = ctx.gates(ia.GATE_XOR, a[:900], b[:900])
    assert np.array_equal(mid, results[1][0][:900])
    four = ctx.gates(ia.GATE_XOR, a[:400], b[:400])      # four waves per gate (one to two gates per CU), whole rotation in one launch
    narrow = ctx.gates(ia.GATE_XOR, a[:200], b[:200])    # the latency kernel
    assert np.array_equal(four, results[1][0][:400]) and np.array_equal(narrow, results[1][0][:200])
    # ... and each of those launch-size regimes (k_blind_rotate_w2r, _w4r, _wide4) against the ORACLE itself at n = 630:
    # 640 of those 900 gates, the oracle's exact back-end on all host cores (~0.3 s per gate and core)
    ref = kb.ck.gates_batch("xor", a[:640], b[:640], threads=0)
    assert np.array_equal(ref, mid[:640])
    assert np.array_equal(ref[:400], four) and np.array_equal(ref[:200], narrow)
    assert np.array_equal(ref, results[0][0][:640])      # and the wide-launch kernel's first level
    # round 5: the one-wave-per-gate kernels built for 1 .. 4 gates per workgroup ("wg_gates"; by default three while a launch
    # holds at most six gates per CU), one-limb (k_blind_rotate_w1b) and two-limb (k_blind_rotate_x1): 1 400 gates of the same
    # level against the oracle's 640 and, beyond them, against the 16 384-gate launch above; ragged last workgroups (1 400 = 3 x 466 + 2)
    cus = ctx.get_option("cus")
    assert ctx.get_option("wg_gates") == 0 and ctx.get_option("wg3_max") == 6 * cus
    # Launches of 4 .. 7 and of 8 .. 10.5 gates per CU run as a ROTATION OF ROLES by default ("br_mix"): the gates in three
    # subsets on three streams, two of them on two waves per gate while the third takes one, roles rotating, no kernel of its own --
    # k_blind_rotate_w2r and k_blind_rotate_w1b on sub-ranges of steps.  Both size ranges, forced geometries (1 of 2 / 1 of 3
    # subsets on two waves), ragged subsets, turn lengths that do and do not divide the rotation, against the oracle's
    # 640 gates and the 16 384-gate launch above; and the same sizes with the rotation switched off.
    assert ctx.get_option("br_mix") == 1
    assert [ctx.kernel_for_launch(c).split("<")[0] for c in (4 * cus, 4 * cus + 1, 7 * cus, 7 * cus + 1, 8 * cus, 8 * cus + 1, 21 * cus // 2, 21 * cus // 2 + 1)] == \
        ["k_blind_rotate_w2r", "k_blind_rotate_w2r+w1b", "k_blind_rotate_w2r+w1b", "k_blind_rotate_w1b", "k_blind_rotate_w1b",
         "k_blind_rotate_w2r+w1b", "k_blind_rotate_w2r+w1b", "k_blind_rotate_w1b"]
    for c, geometry in ((1100, "2 of 3"), (1301, "2 of 3"), (1536, "2 of 3"), (1790, "2 of 3"), (2300, "2 of 3"), (2688, "2 of 3")):
        assert geometry in ctx.kernel_for_launch(c), (c, ctx.kernel_for_launch(c))
        before = ctx.get_option("mixed_launches")
        st = ia.Stats()
        o = ctx.gates(ia.GATE_XOR, a[:c], b[:c], st)
        assert ctx.get_option("mixed_launches") == before + 1 and st.blind_rotate_launches > 20 and st.chunks == 1
        assert np.array_equal(o[:640], ref) and np.array_equal(o, results[1][0][:c]), c
    for fk, ftw in ((2, 1), (3, 1)):                       # forced geometries ("mix_k" / "mix_tw": measurement aids)
        ctx.set_option("mix_k", fk)
        ctx.set_option("mix_tw", ftw)
        assert ("%d of %d" % (ftw, fk)) in ctx.kernel_for_launch(1301)
        assert np.array_equal(ctx.gates(ia.GATE_XOR, a[:1301], b[:1301]), results[1][0][:1301]), (fk, ftw)
    ctx.set_option("mix_k", 0)
    ctx.set_option("mix_tw", 0)
    for s1, ratio, wg in ((7, 150, 4), (64, 400, 3), (630, 100, 1)):  # (630: no whole round fits -- the plain kernels take the launch)
        ctx.set_option("mix_s1", s1)
        ctx.set_option("mix_ratio", ratio)
        ctx.set_option("mix_wg", wg)
        assert np.array_equal(ctx.gates(ia.GATE_XOR, a[:1301], b[:1301]), results[1][0][:1301]), (s1, ratio, wg)
    ctx.set_option("mix_s1", 16)
    ctx.set_option("mix_ratio", 200)
    ctx.set_option("mix_wg", 2)
    # the audit after a rotation of roles (every launch audited here), and a guard trip during one: repeated on the two-limb kernel
    ctx.set_option("fft_audit", 1)
    au0, reruns = ctx.fft_audit(), ctx.fft_guard()[1]
    assert np.array_equal(ctx.gates(ia.GATE_XOR, a[:1301], b[:1301]), results[1][0][:1301])
    au1 = ctx.fft_audit()
    assert au1["audits"] == au0["audits"] + 1 and au1["mismatches"] == au0["mismatches"] and ctx.fft_guard()[1] == reruns
    ctx.set_option("fft_guard_inject", 1)
    assert np.array_equal(ctx.gates(ia.GATE_XOR, a[:1301], b[:1301]), results[1][0][:1301]) and ctx.fft_guard()[1] == reruns + 1
    ctx.set_option("fft_audit", 64)
    ctx.set_option("br_mix", 0)
    assert ctx.kernel_for_launch(1400).split("<")[0] == "k_blind_rotate_w1b" and ctx.kernel_for_launch(1100).split("<")[0] == "k_blind_rotate_w2r"
    before = ctx.get_option("mixed_launches")
    assert np.array_equal(ctx.gates(ia.GATE_XOR, a[:1100], b[:1100]), results[1][0][:1100]) and ctx.get_option("mixed_launches") == before
    for exact in (0, 1):
        ctx.set_option("exact_fft", exact)
        ctx.set_option("two_wave_max", 0)                  # one wave per gate at this size (the default below 5 per CU is two)
        assert ctx.kernel_for_launch(1400).split("<")[0] == ("k_blind_rotate_x1" if exact else "k_blind_rotate_w1b")
        for wg in (0, 1, 2, 3, 4):
            ctx.set_option("wg_gates", wg)
            o = ctx.gates(ia.GATE_XOR, a[:1400], b[:1400])
            assert np.array_equal(o[:640], ref) and np.array_equal(o, results[1][0][:1400]), (exact, wg)
        ctx.set_option("wg_gates", 0)
        ctx.set_option("two_wave_max", 5 * cus)
    ctx.set_option("exact_fft", 0)
    ctx.set_option("br_mix", 1)
    with pytest.raises(ia.IeacheError):
        ctx.set_option("wg_gates", 5)


def test_full_config_add16_batch4096_decrypts(ia, gpu_ctx):
    """BASELINE.json configs[1] at full size (n=630, 4096 ciphertext pairs, 327 680 bootstraps): every one
    of the 4096 sums must decrypt to a+b mod 2^16 (the size-independent property), and a sampled
    expression must equal the oracle bit for bit."""
    z = np.load(os.path.join(G, "full_gate_kat.npz"))
    kb, ctx = gpu_ctx(630, 1024, seed=tuple(int(v) for v in z["seed"]))
    from ieache_amd.tools import bits_to_int
    rng = np.random.default_rng(4096)
    B, bits = 4096, 16
    info = ia.circuit_info(ia.CIRC_ADD, bits)
    inb = rng.integers(0, 2, size=(B, info.n_inputs), dtype=np.uint8)
    inb[:, 2 * bits:] = 0                                   # carry word encrypts 0 (alice.c:147-149)
    inb[0, :2 * bits] = 1                                   # 0xFFFF + 0xFFFF: carries through every bit
    inb[1, :2 * bits] = 0
    inp = kb.enc(inb, 404)
    st = ia.Stats()
    out = ctx.eval_batch(ia.CIRC_ADD, bits, inp, st)
    assert st.bootstraps == 80 * B and st.levels == 48
    dec = kb.dec(out)
    w = 1 << np.arange(bits, dtype=np.int64)
    a = (inb[:, :bits] * w).sum(1)
    b = (inb[:, bits:2 * bits] * w).sum(1)
    got = (dec.astype(np.int64) * w).sum(1)
    assert np.array_equal(got, (a + b) & 0xFFFF)
    # sixteen sampled expressions against the ORACLE bit for bit: the first and the last slot, the carry-through slot, the
    # all-zero slot and twelve random ones -- cloud.c's add() (cloud.c:18-51) replayed level by level so that the sixteen
    # expressions' gates of a level run as one batch on all host cores (1 280 oracle bootstraps)
    sample = sorted({0, 1, B - 1, 1234} | set(int(v) for v in np.random.default_rng(16).choice(B, size=14, replace=False)))[:16]
    ref = _oracle_add_batch(kb.ck, inp[sample, :bits], inp[sample, bits:2 * bits], inp[sample, 2 * bits], bits)
    for q, e in enumerate(sample):
        assert np.array_equal(ref[q], out[e]), e


def _oracle_add_batch(ck, x, y, c, bits):
    """cloud.c add() (cloud.c:18-51; oracle/cloud_oracle.c orc_add) on E independent expressions at once: the same five gates
    per bit in the same dependency order, each level's gates of all expressions as one orc_gates_batch call.
    x, y: [E][bits][n+1], c: [E][n+1] (the carry-in sample) -> sum [E][bits][n+1]"""
    E = x.shape[0]
    carry = np.ascontiguousarray(c)
    out = np.zeros_like(x)
    for i in range(bits):
        both = ck.gates_batch("xor", np.concatenate([x[:, i], y[:, i]]), np.concatenate([carry, carry]), threads=0)  # :30, :32
        axc, bxc = both[:E], both[E:]
        out[:, i] = ck.gates_batch("xor", x[:, i], bxc, threads=0)        # :38
        axc = ck.gates_batch("and", axc, bxc, threads=0)                  # :40
        carry = ck.gates_batch("xor", carry, axc, threads=0)              # :43
    return out


def test_full_config_mul32_batch1024_slot0_matches_golden(ia, gpu_ctx):
    """BASELINE.json configs[2] at full size -- the bench leg's geometry: 32-bit shift-add MUL x 1024 expressions, levels of
    up to 1 056 x 1 024 gate instances cut into 65 536-gate launches (11.5 M bootstraps) -- with the golden vector's operand
    pair in slot 0: that slot's 64 output samples must hash to tests/golden/mul32_n630.json (the oracle's bits, through the
    chunked widest-launch path), and every one of the 1 024 products must decrypt to a * b."""
    import hashlib
    from ieache_amd.tools import bits_to_int, int_to_bits
    g = json.load(open(os.path.join(G, "mul32_n630.json")))
    kb, ctx = gpu_ctx(630, 1024, seed=tuple(g["key_seed"]))
    B = 1024
    rng = np.random.default_rng(1024)
    inb = rng.integers(0, 2, size=(B, 96), dtype=np.uint8)
    inb[:, 64:] = 0                                         # the carry word encrypts 0 (alice.c:147-149)
    inb[0, :32], inb[0, 32:64] = int_to_bits(g["a"], 32), int_to_bits(g["b"], 32)
    inb[1, :64] = 1                                         # 0xFFFFFFFF x 0xFFFFFFFF
    inp = kb.enc(inb, 2048)
    gold_in = kb.enc(inb[0], g["encrypt_seed"])
    assert hashlib.sha256(np.ascontiguousarray(gold_in).tobytes()).hexdigest() == g["input_sha256"]
    inp[0] = gold_in
    widest = ia.circuit_info(4, 32).max_width * B
    assert widest > 65536 and ctx.kernel_for_launch(65536).startswith("k_blind_rotate_w1b")
    st = ia.Stats()
    out = ctx.eval_batch(4, 32, inp, st)
    assert st.bootstraps == 11264 * B and st.chunks > st.levels == 255   # the wide levels were cut into several launches
    assert hashlib.sha256(np.ascontiguousarray(out[0]).tobytes()).hexdigest() == g["output_sha256"]
    w = 1 << np.arange(32, dtype=np.uint64)
    a = (inb[:, :32].astype(np.uint64) * w).sum(1)
    b = (inb[:, 32:64].astype(np.uint64) * w).sum(1)
    dec = kb.dec(out)
    for e in range(B):
        assert bits_to_int(dec[e]) == int(a[e]) * int(b[e]), e
    assert ctx.fft_guard()[0] < 1 / 32


def test_old_libtfhe_parameter_set_on_fast_kernel(ia, gpu_ctx):
    """libtfhe 1.0's default set (l=2, Bgbit=10 -- the paper's 78 MiB keys) also runs on the
    wave-per-polynomial kernel; parameters always come from the key header."""
    kb, ctx = gpu_ctx(12, 1024, l=2, Bgbit=10, lwe_alpha_min=2.44e-5, tlwe_alpha_min=7.18e-9)
    assert "radix8" in ctx.kernel_variant
    a_bits = np.array([0, 0, 1, 1] * 4, dtype=np.uint8)
    b_bits = np.array([0, 1, 0, 1] * 4, dtype=np.uint8)
    a, b = kb.enc(a_bits, 61), kb.enc(b_bits, 62)
    out = ctx.gates(ia.GATE_XOR, a, b)
    assert np.array_equal(kb.dec(out), a_bits ^ b_bits)
    for i in range(16):
        assert np.array_equal(kb.ck.gate("xor", a[i], b[i]), out[i]), i
    ctx.set_option("br_wide_max", 0)  # 16 gates took the 2L = 4 waves-per-gate kernel; now the two-wave one
    assert np.array_equal(ctx.gates(ia.GATE_XOR, a, b), out)
    # this set's sums (4 x 1024 x 2^9 x 2^31 = 2^52) leave the one-limb transform too little FP64 headroom: the context
    # stays on the two-limb kernels and says so; forced, the one-limb kernels still agree (or trip the guard and repeat)
    assert ctx.kernel_variant == "x1x64-radix8-twolimb" and ctx.fft_guard() == (0.0, 0)
    with pytest.raises(ia.IeacheError):
        ctx.set_option("exact_fft", 0)
    for variant in (31, 36):
        ctx.set_option("br_variant", variant)
        assert np.array_equal(ctx.gates(ia.GATE_XOR, a, b), out), variant
    ctx.set_option("br_variant", 0)
    ctx.set_option("br_wide_max", 256)
    # a wide launch of this set takes the two-limb one-wave-per-gate kernel (k_blind_rotate_x1<2,10>): against the oracle on
    # sampled gates and against the two-waves-per-gate kernel on all of them (ragged last workgroup)
    wide_bits = np.random.default_rng(210).integers(0, 2, size=(2, 1101)).astype(np.uint8)
    wa, wb = kb.enc(wide_bits[0], 64), kb.enc(wide_bits[1], 65)
    assert ctx.kernel_for_launch(1101) == "k_blind_rotate_x1<2,10>"
    wout = ctx.gates(ia.GATE_AND, wa, wb)
    assert np.array_equal(kb.dec(wout), wide_bits[0] & wide_bits[1])
    for i in (0, 517, 1100):
        assert np.array_equal(kb.ck.gate("and", wa[i], wb[i]), wout[i]), i
    for wg in (1, 2, 3, 4):                                # its builds for 1 .. 4 gates per workgroup (ragged last workgroups)
        ctx.set_option("wg_gates", wg)
        assert np.array_equal(ctx.gates(ia.GATE_AND, wa, wb), wout), wg
    ctx.set_option("wg_gates", 0)
    one_wave_min = ctx.get_option("exact_one_wave_min")
    ctx.set_option("exact_one_wave_min", 1 << 40)
    assert ctx.kernel_for_launch(1101) == "k_blind_rotate_w2<2,10>" and np.array_equal(ctx.gates(ia.GATE_AND, wa, wb), wout)
    ctx.set_option("exact_one_wave_min", one_wave_min)
    x = kb.enc([1, 0, 1], 63)
    acc = ctx.debug_blind_rotate(x, 3)
    for i in range(3):
        bara, barb = kb.ck.modswitch(x[i])
        ref = kb.ck.blind_rotate_init(barb)
        for s_ in range(3):
            ref = kb.ck.blind_rotate_step(ref, s_, bara[s_])
        assert np.array_equal(ref, acc[i])
    ctx.force_generic(True)
    assert np.array_equal(ctx.gates(ia.GATE_XOR, a, b), out)
    ctx.force_generic(False)


def test_resident_key_daemon(ia, O, tmp_path, sock_dir):
    """`cloudd` keeps the cloud key on the GPU and serves the ./cloud contract over a
    local socket; results equal the in-process run and the oracle, bit for bit."""
    import ctypes as C
    import signal
    import subprocess
    from ieache_amd import daemon, tools
    p = ia.default_params().copy(n=6, N=64)
    S = 4 * p.n + 16
    tools.keygen_files(tmp_path, p)
    sock = sock_dir / "cloudd.sock"
    proc = daemon.spawn(sock, tmp_path / "cloud.key")
    try:
        assert daemon.ping(sock)[0] == 0
        # RUN_DIR through compute(): 2^30 + 2^30, then the oracle on the same cloud.data
        rc, size, ok = _run_file_contract_daemon(ia, tmp_path, sock, 1, 32, 1 << 30, 0, 1 << 30, 0)
        assert (rc, size, ok) == (0, 352 * S, True)
        assert tools.verif_interpret(1, *tools.verif(tmp_path)) == 1 << 31
        _, bk, ksk = tools.read_cloud_key(tmp_path / "cloud.key")
        ck = O.CloudKey(p.n, p.N, p.k, p.l, p.Bgbit, p.ks_t, p.ks_basebit, bk, ksk)
        data = tools.read_samples(tmp_path / "cloud.data", p.n).reshape(22, 32, p.n + 1)
        rc2, ref = ck.cloud_values(1, 0, 32, data[2:10], data[13:21], data[10])
        ans = tools.read_samples(tmp_path / "answer.data", p.n).reshape(11, 32, p.n + 1)
        assert rc2 == 0 and np.array_equal(ans[2:], ref)
        # RUN_DATA: the same bytes over the socket give the same value samples back
        raw = (tmp_path / "cloud.data").read_bytes()
        rc, log, answer = daemon.run_data(sock, 1, raw)
        assert rc == 0 and len(answer) == 352 * S and "Computation Time" in log
        (tmp_path / "answer_sock.data").write_bytes(answer)
        ans2 = tools.read_samples(tmp_path / "answer_sock.data", p.n).reshape(11, 32, p.n + 1)
        assert np.array_equal(ans2[2:], ref)
        # MUL appends averagestandard.txt (cloud.c:2467-2471); 256-bit MUL is refused with 126 and 64 samples
        rc, size, ok = _run_file_contract_daemon(ia, tmp_path, sock, 3, 32, 12345, 0, 678, 2)
        assert rc == 0 and ok and (tmp_path / "averagestandard.txt").exists()
        code, bit_size, words = tools.verif(tmp_path)
        assert (code, bit_size, words[0] | words[1] << 32) == (2, 64, 12345 * 678)
        rc, size, ok = _run_file_contract_daemon(ia, tmp_path, sock, 3, 256, 5, 0, 5, 0)
        assert (rc, size, ok) == (126, 64 * S, False)
        # the `cloud` shim hands over to the daemon when IEACHE_DAEMON is set
        tools.alice(tmp_path, 0, 32, 1000, seed=41)
        tools.alice(tmp_path, 0, 32, 234, seed=42, append=True)
        (tmp_path / "operator.txt").write_text("2")
        exe = os.path.join(os.path.dirname(ia.library_path()), "cloud")
        r = subprocess.run([exe], cwd=tmp_path, env=dict(os.environ, IEACHE_DAEMON=str(sock)), capture_output=True, timeout=120)
        assert r.returncode == 0 and b"Computation Time" in r.stdout and b"daemon" not in r.stderr
        assert tools.verif_interpret(2, *tools.verif(tmp_path)) == 766
        # failures are answered, not fatal: missing directory, truncated cloud.data, unknown request
        rc, log = daemon.run_dir(sock, tmp_path / "no_such_dir")
        assert rc == -5 and "nbit.key" in log
        rc, log, answer = daemon.run_data(sock, 1, raw[:1000])
        assert rc == -5 and answer == b""
        assert daemon.request(sock, 99)[0] == -22
        assert daemon.ping(sock)[0] == 0
        # a directory holding a different cloud.key (a new session): the daemon switches keys
        other = tmp_path / "session2"
        other.mkdir()
        seed = (C.c_uint32 * 3)(7, 8, 9)
        assert ia.lib().ieache_keygen_files(os.fsencode(other), C.byref(p), seed, 3, None, 0) == 0
        tools.alice(other, 0, 32, 40, seed=51)
        tools.alice(other, 0, 32, 2, seed=52, append=True)
        rc, size, ok = ia.compute(1, other, daemon_socket=sock, failure_size=64 * S)
        assert rc == 0 and ok and tools.verif_interpret(1, *tools.verif(other)) == 42
        assert daemon.shutdown(sock) == 0
        assert proc.wait(timeout=60) == 0 and not sock.exists()
    finally:
        if proc.poll() is None:
            proc.send_signal(signal.SIGTERM)
            try:
                proc.wait(timeout=30)
            except subprocess.TimeoutExpired:
                proc.kill()


@pytest.mark.parametrize("devices", [None, (0, 0)])
def test_daemon_batches_concurrent_requests(ia, O, tmp_path, sock_dir, devices):
    """cloudd --batch-window-ms: requests of several clients that arrive together are answered together, those asking
    for the same circuit as ONE level-batched evaluation.  Every client still gets exactly its own answer: the value
    samples equal a one-at-a-time run (and the oracle) bit for bit.
    devices (0, 0): cloudd --devices 0,0 -- two evaluators (two contexts on this box's one card, the way an 8-GPU node would
    list 0,...,7); the round's same-circuit jobs are cut into contiguous slices, one per evaluator, run concurrently and
    answered in request order: same answers, bit for bit."""
    import signal
    import threading
    from ieache_amd import daemon, tools
    p = ia.default_params().copy(n=6, N=64)
    S = 4 * p.n + 16
    tools.keygen_files(tmp_path, p)
    _, bk, ksk = tools.read_cloud_key(tmp_path / "cloud.key")
    ck = O.CloudKey(p.n, p.N, p.k, p.l, p.Bgbit, p.ks_t, p.ks_basebit, bk, ksk)
    # eight clients: six 32-bit additions (one circuit), one subtraction, one 64-bit multiplication
    jobs = []
    for i in range(8):
        d = tmp_path / ("client%d" % i)
        d.mkdir()
        for f in ("cloud.key", "nbit.key", "secret.key"):
            os.link(tmp_path / f, d / f)
        operator, bits, a, b = (1, 32, 1000 + i, 77 * i) if i < 6 else ((2, 32, 5000, 123) if i == 6 else (3, 64, (1 << 40) + 9, (1 << 33) + 5))
        tools.alice(d, 0, bits, a, seed=100 + i)
        tools.alice(d, 0, bits, b, seed=200 + i, append=True)
        jobs.append((d, operator, bits, a, b))
    sock = sock_dir / "cloudd.sock"
    proc = daemon.spawn(sock, tmp_path / "cloud.key", batch_window_ms=400, max_batch=64, devices=devices)
    try:
        results = [None] * 8
        barrier = threading.Barrier(8)

        def client(i):
            d, operator, bits, a, b = jobs[i]
            barrier.wait()
            if i % 2:  # RUN_DATA: bytes over the socket
                rc, log, ans = daemon.run_data(sock, {1: 1, 2: 2, 3: 4}[operator], (d / "cloud.data").read_bytes())
                (d / "answer.data").write_bytes(ans)
                results[i] = (rc, log)
            else:      # RUN_DIR: what the `cloud` shim sends
                (d / "operator.txt").write_text({1: "1", 2: "2", 3: "4"}[operator])
                results[i] = daemon.run_dir(sock, d)

        threads = [threading.Thread(target=client, args=(i,)) for i in range(8)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=300)
        st = daemon.stats(sock)
        assert st["batched_requests"] == 8 and st["largest_batch"] >= 2 and st["evaluations"] < 8, st
        assert st["devices"] == (len(devices) if devices else 1) and sum(st["device_jobs"]) == 8, st
        if devices:  # the six additions (or whatever part of them shared a round) went to both evaluators
            assert st["sharded_evaluations"] >= 1 and min(st["device_jobs"]) >= 1, st
        else:
            assert st["sharded_evaluations"] == 0 and st["device_jobs"] == [8], st
        together = 0
        for i, (d, operator, bits, a, b) in enumerate(jobs):
            rc, log = results[i]
            assert rc == 0 and "Computation Time" in log, (i, log)
            together += "evaluated together" in log
            assert (d / "answer.data").stat().st_size == 352 * S
            code, bit_size, words = tools.verif(d)
            exp = {1: a + b, 2: a - b, 3: a * b}[operator]
            assert tools.verif_interpret({1: 1, 2: 2, 3: 4}[operator], code, bit_size, words) == exp, i
            data = tools.read_samples(d / "cloud.data", p.n).reshape(22, 32, p.n + 1)
            rc2, ref = ck.cloud_values({1: 1, 2: 2, 3: 4}[operator], 0, bits, data[2:10], data[13:21], data[10])
            ans = tools.read_samples(d / "answer.data", p.n).reshape(11, 32, p.n + 1)
            assert rc2 == 0 and np.array_equal(ans[2:], ref), i
        assert together >= 2
        if devices:
            assert any("on 2 devices" in results[i][1] for i in range(8))
        # failures inside a round are answered individually and do not take the round down
        bad = threading.Thread(target=lambda: results.__setitem__(0, daemon.run_data(sock, 1, b"short")))
        good = threading.Thread(target=lambda: results.__setitem__(1, daemon.run_data(sock, 1, (jobs[1][0] / "cloud.data").read_bytes())))
        bad.start()
        good.start()
        bad.join(timeout=120)
        good.join(timeout=120)
        assert results[0][0] == -5 and results[1][0] == 0 and len(results[1][2]) == 352 * S
        # a peer that connects during a round and then sends nothing misses the receive deadline (the batching window,
        # 400 ms here) and is dropped: the request that opened the round is answered without waiting for it
        import socket
        import time
        first = threading.Thread(target=lambda: results.__setitem__(2, daemon.run_data(sock, 1, (jobs[2][0] / "cloud.data").read_bytes())))
        t0 = time.perf_counter()
        first.start()
        time.sleep(0.1)
        staller = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
        staller.connect(os.fspath(sock))
        staller.sendall(b"\x01\x02\x03")  # a fragment of a header, then silence
        first.join(timeout=120)
        took = time.perf_counter() - t0
        assert results[2][0] == 0 and len(results[2][2]) == 352 * S and took < 30, took
        assert staller.recv(16) == b""       # the daemon closed the stalled connection
        staller.close()
        assert daemon.ping(sock)[0] == 0
        assert daemon.shutdown(sock) == 0
        assert proc.wait(timeout=60) == 0
    finally:
        if proc.poll() is None:
            proc.send_signal(signal.SIGTERM)
            try:
                proc.wait(timeout=30)
            except subprocess.TimeoutExpired:
                proc.kill()


def _run_file_contract_daemon(ia, tmp_path, sock, operator, bits, a, sa, b, sb):
    from ieache_amd import tools
    tools.alice(tmp_path, sa, bits, a, seed=31)
    tools.alice(tmp_path, sb, bits, b, seed=32, append=True)
    return ia.compute(operator, tmp_path, daemon_socket=sock, failure_size=64 * (4 * 6 + 16))


def test_bench_two_rank_flow_on_one_gpu(tmp_path):
    """The N>1 path of bench.py end to end, started the way the driver starts it -- `python bench.py --gpus 2` with NO
    torch.distributed.run environment, so bench.py launches its own ranks -- (key broadcast, batch sharding,
    max-over-ranks timing, one JSON line from rank 0), rehearsed with CPU collectives so that both ranks can share this
    box's one GPU."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--full",
           "--batch", "48", "--backend", "gloo", "--no-cpu-baseline", "--legs", "mul32,muladd64", "--mul32-batch", "6",
           "--muladd64-batch", "2", "--extras", "--details", str(tmp_path / "details.json")]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "TORCHELASTIC_RUN_ID")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=tmp_path,
                       env=dict(env, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) < 6000, r.stdout[-2000:]      # ONE compact line (bench.LINE_LIMIT) ...
    line = json.loads(lines[0])
    out = json.load(open(tmp_path / "details.json"))                        # ... and the full record it summarises
    assert line["details"] == str(tmp_path / "details.json") and line["value"] == pytest.approx(out["value"], rel=1e-5)
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["value"] > 0 and "cpu_baseline" not in line
    assert line["config"]["batch_per_gpu"] == 48 and line["config"]["parallelism"] == "batch-sharded x2"
    assert line["config"]["collective_backend"] == "gloo" and len(line["config"]["per_rank_gate_ops_per_s"]) == 2
    lrf = line["roofline"]
    assert lrf["bound"] == "fp64_valu" and 0 < lrf["frac"] < 1 and abs(lrf["achieved"] / lrf["peak"] - lrf["frac"]) < 1e-4 and "note" not in lrf
    assert line["mul32"]["batch_per_gpu"] == 6 and line["mul32_per_s"] > 0 and line["muladd64"]["roofline_frac"] > 0 and "mul128" not in line
    assert line["mul32"]["folded"]["mul32_per_s"] > 0 and line["mul32"]["carry_save"]["mul32_per_s"] > 0
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["value"] > 0
    rf = out["roofline"]
    assert "cpu_baseline" not in out and rf["bound"] == "fp64_valu" and 0 < rf["frac"] == rf["frac_algorithmic_flops"] < 1
    assert abs(rf["achieved"] / rf["peak"] - rf["frac"]) < 1e-9 and rf["algorithmic_flops_per_gate"] == 630 * 233472
    # the other legs ran on both ranks too (their passes contain barriers: a rank skipping one would hang the other)
    m = out["mul32"]
    assert m["batch_per_gpu"] == 6 and len(m["per_rank_gate_ops_per_s"]) == 2 and m["mul32_per_s"] == out["mul32_per_s"] > 0
    assert m["passes"] == 2 and len(m["per_pass_gate_ops_per_s"]) == 2     # the metric's own leg is timed twice
    assert m["folded"]["executed_bootstraps_per_expr"] == 7568 and m["carry_save"]["levels"] == 37
    ma = out["muladd64"]
    assert ma["batch_per_gpu"] == 2 and ma["bootstraps_per_expr"] == 35936 and ma["roofline"]["frac"] > 0 and "mul128" not in out


@pytest.mark.gpu
def test_bench_default_command_shape_with_three_ranks_on_one_gpu(tmp_path):
    """First-contact rehearsal of the multi-GPU job: the --full command shape -- every leg: add16 steps, the exact leg, mul32,
    muladd64, mul128 -- with `--gpus 3`, started by bench.py itself, ranks wrapping onto this box's one GPU, CPU
    collectives.  Three, not eight: this pool allows at most six processes on a card, and this test process and the launcher's
    agent count too (a six-rank attempt was killed by the box's process guard; four ran, at the limit); the eight-rank plumbing runs on CPU in
    tests/test_multirank_cpu.py.  One JSON line, every per-rank list three long, the key broadcast timed, inside the time box."""
    import subprocess
    import sys
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "3", "--full", "--backend", "gloo", "--batch", "64", "--legs",
           "mul32,muladd64,mul128", "--mul32-batch", "8", "--muladd64-batch", "4", "--mul128-batch", "2", "--no-cpu-baseline",
           "--details", str(tmp_path / "details.json")]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "TORCHELASTIC_RUN_ID")}
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=tmp_path,
                       env=dict(env, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0"))
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) < 6000, r.stdout[-2000:]
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                "data", "config", "roofline", "metric_leg", "exact", "mul32", "muladd64", "mul128"):
        assert key in line, key
    assert line["n_gpus"] == 3 and len(line["config"]["per_rank_gate_ops_per_s"]) == 3 and line["exact"]["bit_identical_to_primary_leg"] is True
    out = json.load(open(tmp_path / "details.json"))
    assert out["n_gpus"] == 3 and out["scaling"] == "weak" and out["value"] > 0 and wall < 300, wall
    cfg = out["config"]
    assert cfg["key_broadcast_s"] > 0 and cfg["collective_backend"] == "gloo" and cfg["parallelism"] == "batch-sharded x3"
    assert len(cfg["per_rank_gate_ops_per_s"]) == 3
    for leg in ("mul32", "muladd64", "mul128", "exact"):
        assert len(out[leg]["per_rank_gate_ops_per_s"]) == 3 and out[leg]["gate_ops_per_s"] > 0, leg
    assert out["exact"]["bit_identical_to_primary_leg"] is True and out["exact"]["roofline"]["algorithmic_flops_per_gate"] == 630 * 328704
    assert out["metric_leg"]["mul32_per_s"] == out["mul32_per_s"] > 0 and "skipped_legs" not in out


@pytest.mark.gpu
def test_bench_collectives_on_rccl_with_one_rank(ia, tmp_path):
    """The collective calls of the N>1 job on RCCL itself, as far as one GPU allows: IEACHE_DIST_SINGLE=1 makes bench.py
    form a process group of ONE rank on backend "nccl" (= RCCL), so init_process_group(device_id=...), the device-side
    broadcast of BK / KSK / the LWE key, the barriers, all_gather and all_reduce of the timing path all run on the GPU.
    --dump-outputs: the file holds the timed step's output samples (they decrypt, under bench.py's key, to the sums of its fixed
    edge operands in slots 0-3)."""
    import subprocess
    import sys
    from ieache_amd import tools
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", "--full", "--batch", "64",
           "--backend", "nccl", "--no-cpu-baseline", "--legs", "mul32", "--mul32-batch", "4", "--dump-outputs", str(tmp_path / "dump")]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "TORCHELASTIC_RUN_ID")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=tmp_path,
                       env=dict(env, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", IEACHE_DIST_SINGLE="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    cfg = out["config"]
    assert out["n_gpus"] == 1 and cfg["rccl_ranks"] == 1 and cfg["collective_backend"] == "nccl" and cfg["key_broadcast_s"] > 0
    assert len(cfg["per_rank_gate_ops_per_s"]) == 1 and out["value"] > 0 and out["mul32_per_s"] > 0 and out["mul32"]["expressions_per_s"] > 0
    assert out["metric_leg"]["passes"] == 2 and len(lines[0]) < 6000
    p = ia.default_params()
    dump = np.load(tmp_path / "dump" / "add16_out.npy")
    assert dump.dtype == np.float64 and dump.shape == (64, ia.circuit_info(ia.CIRC_ADD, 16).n_outputs, p.n + 1)
    assert np.array_equal(dump, dump.astype(np.int32))
    lwe_key = tools.keygen_raw(p, (314, 1592, 657), with_cloud=False)["lwe_key"]
    dec = tools.decrypt_bits(p, lwe_key, dump.astype(np.int32))
    assert [tools.bits_to_int(dec[e]) for e in range(4)] == [0, 2, 0xFFFE, 0x8000]   # 0+0, 1+1, 2 (2^16-1), 2 x 2^14


def test_bench_plain_run_stops_at_the_timed_steps(tmp_path):
    """`python bench.py --gpus 1 --steps K --warmup W` without --full: set-up, warm-up, the K timed steps, the line.  No exact leg, no
    further workload, no CPU baseline, the roofline object priced on the timed steps themselves; and the whole process, start to
    exit, spends less than 30 s outside its K + W steps (a --full run spends minutes there)."""
    import subprocess
    import sys
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--details", str(tmp_path / "details.json")]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "TORCHELASTIC_RUN_ID")}
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=tmp_path, env=env)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) < 6000, r.stdout[-2000:]
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                "data", "config", "roofline", "fft_guard", "details"):
        assert key in line, key
    for key in ("exact", "mul32", "muladd64", "mul128", "metric_leg", "mul32_per_s", "cpu_baseline", "skipped_legs"):
        assert key not in line, key
    assert line["steps"] == 2 and line["warmup"] == 1 and line["config"]["batch_per_gpu"] == 4096 and line["unit"] == "gate ops/s"
    assert line["value"] == pytest.approx(80 * 4096 / (line["ms_per_step"] * 1e-3), rel=1e-4)
    assert line["roofline"]["mode"] == "timed region" and 0 < line["roofline"]["frac"] < 1
    assert wall - 3 * line["ms_per_step"] * 1e-3 < 30, (wall, line["ms_per_step"])
    assert "--legs" in subprocess.run(cmd + ["--legs", "mul32"], capture_output=True, text=True, timeout=60, cwd=tmp_path, env=env).stderr


def test_output_noise_matches_the_published_variance(ia, gpu_ctx):
    """The algorithm pinned without a libtfhe binary: 16 384 bootstrapped gate outputs at the reference's parameters carry the
    noise the published analysis predicts for libtfhe's conventions (tests/test_golden_cpu.py: predicted_gate_output_noise) --
    blind rotation 4.69e-6 + truncating decomposition 1.5e-6 + key switch 4.29e-6 about a per-key offset -- to within 6 %
    (sample variance of 16 384 values: +-1.1 % at one sigma).  A decomposition that ROUNDED would measure 15 % lower, a missing
    digit row 8 % lower, a key-switch base of 8 instead of 4 15 % higher: the bits the kernels produce are those of THIS algorithm.
    Both kernel families, two gate types (the output noise must not depend on the gate or on the inputs)."""
    from test_golden_cpu import predicted_gate_output_noise, phase_errors
    z = np.load(os.path.join(G, "full_gate_kat.npz"))
    kb, ctx = gpu_ctx(630, 1024, seed=tuple(int(v) for v in z["seed"]))
    var, offset_sd = predicted_gate_output_noise(kb.p, np.sum(kb.tlwe_key))
    rng = np.random.default_rng(99)
    cnt = 16384
    bits = rng.integers(0, 2, size=(2, cnt)).astype(np.uint8)
    a, b = kb.enc(bits[0], 171), kb.enc(bits[1], 172)
    means = []
    for exact, gate, want_bits in ((0, ia.GATE_XOR, bits[0] ^ bits[1]), (1, ia.GATE_NAND, 1 - (bits[0] & bits[1]))):
        ctx.set_option("exact_fft", exact)
        out = ctx.gates(gate, a, b)
        ctx.set_option("exact_fft", 0)
        assert np.array_equal(kb.dec(out), want_bits)
        e = phase_errors(kb.p, kb.lwe_key, out, want_bits)
        assert np.max(np.abs(e)) < 1.0 / 32                       # 1/8 is a wrong bit; 4.5 sigma of 16 384 draws is 0.016
        assert 0.94 * var < np.var(e) < 1.06 * var, (exact, np.var(e), var)
        means.append(float(np.mean(e)))
        assert abs(means[-1]) < 4 * offset_sd, means
        # the offset is the same for outputs of either sign (it is additive key-switch-key noise, not a scaling of the message)
        m1, m0 = np.mean(e[want_bits == 1]), np.mean(e[want_bits == 0])
        assert abs(m1 - m0) < 6 * np.sqrt(2 * var / (cnt / 2)), (m1, m0)
    assert abs(means[0] - means[1]) < 6 * np.sqrt(2 * var / cnt), means  # one key, one offset
