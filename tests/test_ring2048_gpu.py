"""-m gpu: a context on the ring of degree 2048, word for word against the CPU oracle (pinned against np_tfhe at these sets by
tests/test_ring2048_cpu.py), every case on both kernels of that ring: k_blind_rotate_h2 (csrc/blind_rotate_h2.hip: one CMux step
as two products on the ring of degree 1024) and, under "force_generic", k_blind_rotate_generic with the any-parameter key switch.

Every key has n <= 16 and no launch more than 16 items: the size axes are tests/test_ring2048_axes_gpu.py's.  The odd rotation amounts, where the even and odd halves of the accumulator change places, are what the
crafted rows aim at; tests/native/ring_split_test.cpp holds the identity itself."""
import contextlib

import numpy as np
import pytest

import crafted_state as CS
import np_tfhe
import param_lattice as PL

pytestmark = pytest.mark.gpu
N = 2048
NEVER = 1 << 40
KERNELS = pytest.mark.parametrize("fg", [0, 1], ids=["h2", "generic"])
AMOUNTS = (0, 1, 2, N - 1, N, N + 1, 2 * N - 2, 2 * N - 1)


@contextlib.contextmanager
def _context(ia, p, bk, ksk, fg):
    """A context on the arrays with the kernel of the case forced or not; says which kernel a launch takes."""
    with ia.Context.from_arrays(p, bk, ksk) as ctx:
        ctx.set_option("force_generic", fg)
        want = "k_blind_rotate_generic" if fg else "k_blind_rotate_h2<%d,%d>" % (p.l, p.Bgbit)
        assert ctx.kernel_for_launch(5) == want and ctx.kernel_for_launch(5000) == want
        assert ctx.kernel_variant == ("generic-radix2" if fg else "h2x64-radix8-twolimb")
        yield ctx


def _check_accumulators(ctx, ck, x, steps=(0, 1, 2, -1)):
    ref = CS.oracle_accumulators(ck, x, steps)
    for s in steps:
        acc = ctx.debug_blind_rotate(x, s)
        bad = np.argwhere(acc != ref[s])
        assert bad.size == 0, "steps %d: %d words differ, first at (row, polynomial, coefficient) %s" % (s, len(bad), bad[0])


# ---- mod switch, single steps at crafted amounts, the whole rotation ----

@KERNELS
def test_mod_switch_and_steps_at_crafted_amounts(ia, make_keys, fg):
    """Rows whose coefficients mod-switch to exactly 0, 1, 2, N - 1, N, N + 1, 2N - 2, 2N - 1 -- every row meets another of them
    at every step, the b word too, so the starting accumulator is rotated by even and odd amounts -- and rows on the rounding
    edges of the mod switch to 2N = 4096.  Accumulators after 0 steps (the mod switch of b and the start), 1, 2 and all steps."""
    kb = make_keys(8, N)
    n = kb.p.n
    x = np.array([[CS.amount_word(AMOUNTS[(r + 3 * s) % 8], N) for s in range(n)] + [CS.amount_word(AMOUNTS[(r + 5) % 8], N)] for r in range(8)],
                 dtype=np.int32)
    for r in range(8):
        bara, barb = kb.ck.modswitch(x[r])
        assert bara[0] == AMOUNTS[r] and bara[1] == AMOUNTS[(r + 3) % 8] and barb == AMOUNTS[(r + 5) % 8]
    half = 1 << 19  # half a mod-switch step: 2^32 / 4096 / 2
    edge = np.zeros((4, n + 1), dtype=np.int32)
    edge[0] = -1                 # + half wraps: amount 0 everywhere
    edge[1] = 0x7FFFFFFF         # rounds up to N
    edge[2] = -(half + 1)        # the last value that still rounds to 2N - 1
    edge[3] = np.resize(np.array([-1, 0x7FFFFFFF, -(half + 1), -half, half - 1, half, 12345], dtype=np.int64), n + 1).astype(np.int32)
    assert not kb.ck.modswitch(edge[0])[0].any() and (kb.ck.modswitch(edge[1])[0] == N).all() and (kb.ck.modswitch(edge[2])[0] == 2 * N - 1).all()
    x = np.concatenate([x, edge, kb.enc([0, 1, 1], 7)])
    with _context(ia, kb.p, kb.bk, kb.ksk, fg) as ctx:
        _check_accumulators(ctx, kb.ck, x)


# ---- crafted state: the br_exact() edge with every term of one sign ----

EDGE_CASES = [("worst%d" % w, lambda ia, w=w: CS.worst_alignment(ia, 1, 20, N, w)) for w in range(len(CS.WORST_ALIGNMENTS))]
EDGE_CASES += [("mixed", lambda ia: CS.extreme_mixed(ia, 1, 20, N)), ("worst0-l3", lambda ia: CS.worst_alignment(ia, 3, 7, N, 0)),
               ("mixed-l2", lambda ia: CS.extreme_mixed(ia, 2, 10, N))]


@KERNELS
@pytest.mark.parametrize("name,build", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_steered_state_at_the_exactness_edge(ia, O, fg, name, build):
    """tests/crafted_state.py's construction at N = 2048: step 0 (amount 1, odd: the halves change places) steers the
    accumulator so that step 1 (amount N) decomposes into digits at their extremes against key words at theirs; l = 1 /
    Bgbit = 20 is the edge of Params::br_exact(): 2 x 2048 x 2^19 x 2^31 = 2^62, two-limb sums of 2^46."""
    case = build(ia)
    p = case.p
    assert PL.br_exact(p.l, p.Bgbit, N) and (p.l != 1 or not PL.br_exact(1, p.Bgbit + 1, N))
    if name == "worst0":
        assert CS.log2_peak(CS.exact_sums(case.digits, case.bk[1])) > 61.99  # every unwrapped term of one sign: 2^62
    ck = CS.open_oracle(O, p, case.bk, case.ksk)
    assert np.array_equal(CS.oracle_accumulators(ck, case.x[:1], (1,))[1][0], case.target)  # the steering step does what it claims
    with _context(ia, p, case.bk, case.ksk, fg) as ctx:
        _check_accumulators(ctx, ck, case.x)


# ---- gadgets ----

@KERNELS
@pytest.mark.parametrize("l,Bgbit", [(3, 7), (2, 10), (4, 6), (8, 4)])
def test_gadgets(ia, make_keys, fg, l, Bgbit):
    """(l, Bgbit) as launch arguments of the one build: 6, 4, 8 and 16 digit rows.  The any-parameter kernel takes up to l = 4
    on this ring; at l = 8 its 16 rows of 16 KiB do not fit a CU, which a forced launch says."""
    kb = make_keys(5, N, l=l, Bgbit=Bgbit)
    rng = np.random.default_rng(l)
    x = np.concatenate([kb.enc([0, 1], 3), np_tfhe.uniform32(rng, (3, kb.p.n + 1))])
    a, b = kb.enc([0, 1, 1], 4), kb.enc([1, 1, 0], 5)
    with _context(ia, kb.p, kb.bk, kb.ksk, fg) as ctx:
        if fg and l == 8:
            with pytest.raises(ia.IeacheError, match="exceeds the 160 KiB LDS"):
                ctx.debug_blind_rotate(x, -1)
            with pytest.raises(ia.IeacheError, match="exceeds the 160 KiB LDS"):
                ctx.gates(ia.GATE_XOR, a, b)
            return
        _check_accumulators(ctx, kb.ck, x, steps=(1, -1))
        out = ctx.gates(ia.GATE_XOR, a, b)
        for i in range(3):
            assert np.array_equal(kb.ck.gate("xor", a[i], b[i]), out[i]), i


# ---- partial workgroups, slices ----

@KERNELS
def test_row_counts_and_a_slice_that_cuts_the_rotation(ia, make_keys, fg):
    kb = make_keys(9, N)
    bits = np.random.default_rng(9).integers(0, 2, size=(2, 5)).astype(np.uint8)
    a, b = kb.enc(bits[0], 11), kb.enc(bits[1], 12)
    ref = np.stack([kb.ck.gate("and", a[i], b[i]) for i in range(5)])
    with _context(ia, kb.p, kb.bk, kb.ksk, fg) as ctx:
        for sl in (0, 5, 1, 64):  # the default; 5 + 4 steps; a launch per step; longer than the rotation
            ctx.set_option("br_slice", sl)
            for cnt in (1, 3, 5):
                st = ia.Stats()
                assert np.array_equal(ctx.gates(ia.GATE_AND, a[:cnt], b[:cnt], stats=st), ref[:cnt]), (sl, cnt)
                if not fg:
                    assert st.as_dict()["blind_rotate_launches"] == {0: 1, 5: 2, 1: 9, 64: 1}[sl]
        assert np.array_equal(kb.dec(ref), bits[0] & bits[1])
        audit = ctx.fft_audit()
        assert audit["audits"] == 0 and audit["mismatches"] == 0  # exact by construction: nothing is audited on this ring


# ---- every gate ----

TWO_INPUT = {  # (ka, kb, constant): boot-gates.cpp
    "GATE_AND": (1, 1, 0xE0000000), "GATE_XOR": (2, 2, 0x40000000), "GATE_OR": (1, 1, 0x20000000), "GATE_NAND": (-1, -1, 0x20000000),
    "GATE_XNOR": (-2, -2, 0xC0000000), "GATE_NOR": (-1, -1, 0xE0000000), "GATE_ANDNY": (-1, 1, 0xE0000000), "GATE_ANDYN": (1, -1, 0xE0000000),
    "GATE_ORNY": (-1, 1, 0x20000000), "GATE_ORYN": (1, -1, 0x20000000)}
TRUTH = {"GATE_AND": lambda a, b: a & b, "GATE_XOR": lambda a, b: a ^ b, "GATE_OR": lambda a, b: a | b, "GATE_NAND": lambda a, b: 1 - (a & b),
         "GATE_XNOR": lambda a, b: 1 - (a ^ b), "GATE_NOR": lambda a, b: 1 - (a | b), "GATE_ANDNY": lambda a, b: (1 - a) & b,
         "GATE_ANDYN": lambda a, b: a & (1 - b), "GATE_ORNY": lambda a, b: (1 - a) | b, "GATE_ORYN": lambda a, b: a | (1 - b)}


@KERNELS
def test_every_gate(ia, make_keys, fg):
    """The ten two-input gates, bootsMUX, MAJ3 and XOR3 on the four / eight combinations of their inputs: the oracle's
    bootstrap of the gate's linear combination, sample for sample, and the truth table."""
    kb = make_keys(8, N)
    bits = np.array([[(v >> k) & 1 for v in range(8)] for k in range(3)], dtype=np.uint8)
    a, b, c = (kb.enc(bits[k], 21 + k) for k in range(3))
    with _context(ia, kb.p, kb.bk, kb.ksk, fg) as ctx:
        for name, (ka, kbb, cst) in TWO_INPUT.items():
            out = ctx.gates(getattr(ia, name), a[:4], b[:4])
            comb = np_tfhe._wrap32(CS._plus_b(np_tfhe._wrap32(ka * a[:4].astype(np.int64) + kbb * b[:4].astype(np.int64)), cst))
            for i in range(4):
                assert np.array_equal(kb.ck.bootstrap(comb[i]), out[i]), (name, i)
            assert np.array_equal(kb.dec(out), TRUTH[name](bits[0, :4], bits[1, :4])), name
        out = ctx.mux(a, b, c)
        for i in range(8):
            assert np.array_equal(kb.ck.mux(a[i], b[i], c[i]), out[i]), ("mux", i)
        assert np.array_equal(kb.dec(out), np.where(bits[0] == 1, bits[1], bits[2]))
        for gate, truth in ((ia.GATE_MAJ3, (bits.sum(axis=0) >= 2)), (ia.GATE_XOR3, bits[0] ^ bits[1] ^ bits[2])):
            out = ctx.gates3(gate, a, b, c)
            comb = CS.gate_combination(gate, a, b, c)
            for i in range(8):
                assert np.array_equal(kb.ck.bootstrap(comb[i]), out[i]), (gate, i)
            assert np.array_equal(kb.dec(out), truth.astype(np.uint8)), gate


@KERNELS
def test_four_bit_adder_through_the_level_executor(ia, make_keys, fg):
    from ieache_amd import tools
    kb = make_keys(8, N)
    bits = 4
    info = ia.circuit_info(ia.CIRC_ADD, bits)
    vals = [(9, 5), (15, 1), (7, 7)]
    inb = np.zeros((len(vals), info.n_inputs), dtype=np.uint8)
    for e, (u, v) in enumerate(vals):
        inb[e, :bits], inb[e, bits:2 * bits] = tools.int_to_bits(u, bits), tools.int_to_bits(v, bits)
    inp = kb.enc(inb, 31)
    with _context(ia, kb.p, kb.bk, kb.ksk, fg) as ctx:
        out = ctx.eval_batch(ia.CIRC_ADD, bits, inp)
        nl = ia.Netlist(2)
        nl_out = nl.gate(ia.GATE_XOR, nl.input(0), nl.input(1))
        with nl.compile([nl_out, nl.gate(ia.GATE_MUX, nl_out, nl.input(0), ia.NOT(nl.input(1)))]) as cn:
            net = ctx.eval_netlist(cn, inp[:, :2])
    for e, (u, v) in enumerate(vals):
        ref, _ = kb.ck.add(inp[e, :bits], inp[e, bits:2 * bits], inp[e, 2 * bits:2 * bits + 1], bits)
        assert np.array_equal(ref, out[e]), e
        assert tools.bits_to_int(kb.dec(out[e])) == (u + v) % 16
        x0, x1 = inb[e, 0], inb[e, 1]
        assert list(kb.dec(net[e])) == [x0 ^ x1, (x0 if x0 ^ x1 else 1 - x1)]
        assert np.array_equal(net[e, 0], kb.ck.gate("xor", inp[e, 0], inp[e, 1]))


# ---- programmable bootstrap ----

def _start(rows, barb):
    """X^(2N - barb) rows, rows [..][N]: the accumulator polynomials a programmable bootstrap starts from."""
    idx = (np.arange(N) - (2 * N - barb)) % (2 * N)
    r = np.asarray(rows, dtype=np.int32)[..., idx % N].astype(np.int64)
    return np.where(idx < N, r, -r).astype(np.int32)


@KERNELS
def test_programmable_bootstrap_in_its_three_forms(ia, O, make_keys, fg):
    """A caller polynomial, a table of TLWE samples and the accumulator as the result, with and without the key switch; two
    factors through pbs_multi; keyswitch and tlwe_extract on what they return."""
    from ieache_amd import tools
    kb = make_keys(8, N)
    p, ck = kb.p, kb.ck
    x = np.concatenate([kb.enc([1, 0, 1], 41), np_tfhe.uniform32(np.random.default_rng(41), (2, p.n + 1))])
    v = (np.arange(1, N + 1, dtype=np.int64) * 0x01234567 & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    const = np.full(N, 1 << 29, dtype=np.int32)
    sample = np.stack([v[::-1], v])
    of = [0, 1, 1, 0, 1]
    accs = []
    for i in range(5):
        bara, barb = ck.modswitch(x[i])
        accs.append((ck.blind_rotate(np.ascontiguousarray(np.stack([np.zeros(N, np.int32), _start(v, barb)])), bara),
                     ck.blind_rotate(np.ascontiguousarray(_start(sample, barb)), bara)))
    factors = np.stack([np.eye(1, N, 0, dtype=np.int32)[0], tools.lut_factor_poly(p, [0, 1, 0, 1, 1, 0, 1, 0])])
    bias = np.array([0, -(1 << 29)], dtype=np.int32)
    with _context(ia, p, kb.bk, kb.ksk, fg) as ctx:
        out = ctx.pbs(x, np.stack([const, v]), of)
        ext = ctx.pbs(x, np.stack([const, v]), of, keyswitch=False)
        assert np.array_equal(ctx.keyswitch(ext), out)
        for i in range(5):
            want = ck.bootstrap(x[i]) if of[i] == 0 else ck.keyswitch(ck.sample_extract(accs[i][0]))
            assert np.array_equal(want, out[i]), i
            if of[i]:
                assert np.array_equal(ck.sample_extract(accs[i][0]), ext[i]), i
        got = ctx.pbs(x, sample, tlwe=True, accumulator=True)
        for i in range(5):
            assert np.array_equal(got[i], accs[i][1]), i
        assert np.array_equal(ctx.pbs(x, sample, tlwe=True), np.stack([ck.keyswitch(ck.sample_extract(a[1])) for a in accs]))
        coef = [0, 1, N - 1, 1024, 77]
        rows = ctx.tlwe_extract(got, coef_of=coef)
        for i, c in enumerate(coef):  # u[j] = A[c - j] up to c and -A[N + c - j] above, u[N] = B[c]
            j = np.arange(N)
            A = accs[i][1][0].astype(np.int64)
            want = np.append(np.where(j <= c, A[(c - j) % N], -A[(N + c - j) % N]), accs[i][1][1][c])
            assert np.array_equal(rows[i], np_tfhe._wrap32(want)), (i, c)
        assert np.array_equal(rows[0], ck.sample_extract(accs[0][1]))
        multi = ctx.pbs_multi(x, np.stack([const, v]), factors, of, bias)
        assert np.array_equal(multi[:, 0], out)
        for i in (1, 3):
            acc = accs[i][0] if of[i] else ck.blind_rotate(np.ascontiguousarray(np.stack([np.zeros(N, np.int32), _start(const, ck.modswitch(x[i])[1])])),
                                                            ck.modswitch(x[i])[0])
            u = ck.sample_extract(np.stack([O.negacyclic_mul(factors[1], acc[c], mode=O.POLYMUL_SCHOOLBOOK) for c in range(2)]))
            u[N] = np.uint32((int(u[N]) + int(bias[1])) & 0xFFFFFFFF).astype(np.int32)
            assert np.array_equal(ck.keyswitch(u), multi[i, 1]), i


@KERNELS
def test_sixteen_entry_table_by_meaning(ia, O, make_keys, fg):
    """What the ring is for: a 16-entry table through pbs, every input value decrypted.  The key's noise is set low (the mod
    switch alone moves a phase by at most 9 / 8192 of the torus at n = 8; a slot is 1 / 32 wide)."""
    from ieache_amd import tools
    kb = make_keys(8, N, lwe_alpha_min=2.0 ** -30, tlwe_alpha_min=2.0 ** -40)
    p = kb.p
    rng = np.random.default_rng(16)
    table = (((np.arange(16, dtype=np.int64) * 5 + 3) % 16 - 8) << 27)
    table[0] = 0  # slot 0 straddles phase 0, where the negacyclic sign flips
    key = kb.lwe_key.astype(np.int64)
    x = np.zeros((16, p.n + 1), dtype=np.int32)
    for m in range(16):
        a = np_tfhe.uniform32(rng, p.n).astype(np.int64)
        x[m, :p.n] = a
        x[m, p.n] = np_tfhe._wrap32(int((a * key).sum()) + (m << 27) + int(rng.integers(-1 << 12, 1 << 12)))
    with _context(ia, p, kb.bk, kb.ksk, fg) as ctx:
        out = ctx.pbs(x, tools.lut_test_poly(p, table.astype(np.int32)))
    for m in range(16):
        ph = int(np_tfhe._wrap32(int(out[m, p.n]) - int((out[m, :p.n].astype(np.int64) * key).sum())))
        assert abs(ph - int(table[m])) < 1 << 25, (m, ph, int(table[m]))
        assert np.array_equal(out[m], kb.ck.keyswitch(kb.ck.sample_extract(
            kb.ck.blind_rotate(np.ascontiguousarray(np.stack([np.zeros(N, np.int32), _start(tools.lut_test_poly(p, table.astype(np.int32)), kb.ck.modswitch(x[m])[1])])),
                               kb.ck.modswitch(x[m])[0])))), m


# ---- key switch ----

def test_key_switch_families_on_the_edge_rows(ia, make_keys):
    """N = 2048 words per extracted sample through every family ks_support() allows: 70 rows (66 random + the four edge rows of
    param_lattice.edge_rows), 5 and 1 of them; the sliced walk takes the ring in two launches of 1 024 coefficients."""
    kb = make_keys(7, N)
    p = kb.p
    u = PL.edge_rows(np.random.default_rng(15), N, p.ks_t, p.ks_basebit, 66)
    ref = np.stack([kb.ck.keyswitch(r) for r in u])
    assert np.array_equal(np_tfhe.np_keyswitch(kb.ksk, p.ks_t, p.ks_basebit, u), ref)
    for r in (66, 67, 69):  # no row subtracted: (0, b')
        assert not ref[r, :p.n].any() and ref[r, p.n] == u[r, N]
    base = dict(force_generic=0, ks_mfma_min=NEVER, ks_sliced_min=NEVER, ks_batch_min=NEVER)
    fams = [("generic", dict(base, force_generic=1)), ("per-gate", dict(base, ks_split_max=1)), ("per-gate, split", dict(base, ks_split_max=16)),
            ("batched", dict(base, ks_batch_min=1)), ("sliced 4", dict(base, ks_sliced_min=1, ks_gates=4)),
            ("sliced 32, slice 600", dict(base, ks_sliced_min=1, ks_gates=32, ks_slice=600)),
            ("mfma", dict(base, ks_mfma_min=1, ks_mfma_split=1)), ("mfma split 8", dict(base, ks_mfma_min=1, ks_mfma_split=8))]
    with ia.Context.from_arrays(p, kb.bk, kb.ksk) as ctx:
        assert np.array_equal(ctx.debug_keyswitch(u), ref) and np.array_equal(ctx.keyswitch(u), ref)
        for label, opts in fams:
            for k, val in opts.items():
                ctx.set_option(k, val)
            for rows in (slice(0, 70), slice(65, 70), slice(68, 69)):
                out = ctx.debug_keyswitch(u[rows])
                bad = np.argwhere(out != ref[rows])
                assert bad.size == 0, "%s, rows %s: %d words differ, first at (row, column) %s" % (label, rows, len(bad), bad[0])


# ---- what such a context refuses ----

def _raw_arrays(p):
    return np.zeros(p.bk_count, dtype=np.int32), np.zeros(p.ksk_count, dtype=np.int32)


def test_lds_refusals_at_context_creation(ia):
    """Before any launch: a gadget of more than 16 rows stays on the any-parameter kernel, whose 32 rows of 16 KiB no CU holds;
    a key-switch digit list of N x t = 2048 x 31 words does not fit either.  N = 4096 is no supported ring."""
    for kw in (dict(l=16, Bgbit=2), dict(ks_t=31, ks_basebit=1), dict(ks_t=19, ks_basebit=1)):
        p = ia.default_params().copy(n=3, N=N, **kw)
        with pytest.raises(ia.IeacheError, match="exceeds the 160 KiB LDS"):
            ia.Context.from_arrays(p, *_raw_arrays(p))
    p = ia.default_params().copy(n=3, N=4096)
    with pytest.raises(ia.IeacheError, match="unsupported TFHE parameter set"):
        ia.Context.from_arrays(p, *_raw_arrays(p))
    p = ia.default_params().copy(n=3, N=N, ks_t=18, ks_basebit=1)  # 155 664 bytes: accepted
    with ia.Context.from_arrays(p, *_raw_arrays(p)) as ctx:
        assert ctx.kernel_for_launch(1) == "k_blind_rotate_h2<3,7>"


def test_calls_of_the_1024_ring_keep_their_refusals(ia, make_keys):
    """tgsw_prepare (and with it every call on a TGSW set) is N = 1024 only and says so as before; the packing key switch --
    and the projection and unpack, which are that unit on n := N -- refuses its key with a message."""
    from ieache_amd import tools
    kb = make_keys(4, N)
    p = kb.p
    with ia.Context.from_arrays(p, kb.bk, kb.ksk) as ctx:
        with pytest.raises(ia.IeacheError, match="the CMux kernels cover N = 1024"):
            ctx.tgsw_prepare(np.zeros((1, 2 * p.l, 2, N), dtype=np.int32))
        with pytest.raises(ia.IeacheError, match="covers rings up to N = 1024"):
            ctx.set_packing_key(np.zeros((p.n, 8, 2, N), dtype=np.int32))
        with pytest.raises(ia.IeacheError, match="covers rings up to N = 1024"):
            ctx.set_projection_key(np.zeros((N, 1, 2, N), dtype=np.int32), t=1, basebit=2)
        a = kb.enc([1, 0], 3)
        assert np.array_equal(ctx.gates(ia.GATE_NAND, a, a[::-1])[0], kb.ck.gate("nand", a[0], a[1]))  # and goes on working


def test_group_of_one_device(ia, make_keys):
    kb = make_keys(8, N)
    a, b = kb.enc([0, 1, 1], 51), kb.enc([1, 1, 0], 52)
    with ia.Group.from_arrays(kb.p, kb.bk, kb.ksk, [0]) as grp:
        out = grp.gates(ia.GATE_OR, a, b)
        const = np.full(N, 1 << 29, dtype=np.int32)
        boot = grp.pbs(a, const)
    for i in range(3):
        assert np.array_equal(out[i], kb.ck.gate("or", a[i], b[i])) and np.array_equal(boot[i], kb.ck.bootstrap(a[i])), i
