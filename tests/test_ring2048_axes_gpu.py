"""-m gpu: the ring of degree 2048 along its SIZE axes, where tests/test_ring2048_gpu.py (arithmetic: crafted amounts, the
br_exact() edge, gadgets, gates) stays at n <= 16 and at most 16 items.  Index arithmetic, not rounding: key lengths 63 .. 630, so
that a slice of k_blind_rotate_h2 reaches lanes 16 .. 63 of its amounts, reloads them at steps other than 0, parks and re-reads
its accumulator up to 65 times, k_h2_prologue takes its second trip (n >= 256) and a key block is fetched at a high step index;
launches wider than the chip, scratch grown by a later call, calls cut by "chunk"; k_mv_extract_2048 on the whole factor set of
tests/test_pbs_multi_gpu.py; the key switch from 2048-word samples around n = 256.

Every comparison is exact equality with the CPU oracle (pinned against np_tfhe on this ring by tests/test_ring2048_cpu.py and,
for the rows used here, by tests/test_ring2048_axes_cpu.py), or with an uncut / one-stream run that is itself compared with it.
Every case forces its kernel and asserts which one a launch takes, as tests/test_ring2048_gpu.py does.

Wall time on an MI355X, same run, each file in a pytest process of its own: this file 10.0 s (52 cases, key generation and CPU
references included), tests/test_ring2048_gpu.py 5.5 s (40 cases)."""
import contextlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import crafted_state as CS
import multi_reference as MR
import np_tfhe
import param_lattice as PL
from test_pbs_multi_gpu import BIAS, DENSE, ONE, SPARSE, X1, XHALF, XINV, ZERO, factor_set, random_polys, random_rows, without_bias
from test_ring2048_gpu import KERNELS, N, NEVER, _context

pytestmark = pytest.mark.gpu
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
AXIS_N = (63, 64, 65, 129, 257)
ROW_NAMES = ["pattern %d" % r for r in range(8)] + ["isolating 63/64/n-1", "isolating zero slice 16..31", "uniform 0", "uniform 1",
                                                     "bit 0", "bit 1", "bit 1'"]


def _launches(steps, sl):
    """Launches of k_blind_rotate_h2 for `steps` CMux steps under "br_slice" sl (0: br_slice_default = 16)."""
    return -(-steps // (sl or 16))


# ---- 1. blind rotation over n and over slices ----

_axis = {}


def axis_case(kb):
    """The 15 rows of a key length and the oracle's accumulators after every step count of the case, computed once per n."""
    n = kb.p.n
    if n not in _axis:
        rng = np.random.default_rng(2048 + n)
        a, b = kb.enc([0, 1, 1], 7), kb.enc([1, 1, 0], 8)
        x = np.concatenate([CS.amount_rows(CS.axis_pattern_amounts(n, N), N), CS.amount_rows(CS.axis_isolating_amounts(n, N), N),
                            np_tfhe.uniform32(rng, (2, n + 1)), a])
        steps = [s for s in dict.fromkeys((0, 1, 63, 64, 65, n - 1, -1)) if s <= n]
        _axis[n] = dict(x=x, steps=steps, ref=CS.oracle_accumulators_threaded(kb.ck, x, steps), a=a, b=b,
                        xor=kb.ck.gates_batch("xor", a, b, threads=3))
    return _axis[n]


def _run_axis(ia, kb, fg, sl):
    n = kb.p.n
    c = axis_case(kb)
    with _context(ia, kb.p, kb.bk, kb.ksk, fg) as ctx:
        ctx.set_option("br_slice", sl)
        for s in c["steps"]:
            diff = CS.first_difference(ctx.debug_blind_rotate(c["x"], s), c["ref"][s])
            if diff:
                (row, poly, coef), count = diff
                pytest.fail("n %d, slice %d, steps %d: %d words differ, first in row %d (%s), polynomial %d, coefficient %d"
                            % (n, sl, s, count, row, ROW_NAMES[row], poly, coef))
        # the same rotation through the entries that report Stats: the accumulator a programmable bootstrap returns, and a gate
        st = ia.Stats()
        acc = ctx.pbs(c["x"], CS.pbs_constant_poly(N), accumulator=True, stats=st)
        diff = CS.first_difference(acc, c["ref"][-1])
        assert diff is None, "n %d, slice %d, pbs accumulator: first at (row, polynomial, coefficient) %s of %d words" % ((n, sl) + diff)
        if not fg:
            assert st.blind_rotate_launches == _launches(n, sl), (n, sl)
        st = ia.Stats()
        out = ctx.gates(ia.GATE_XOR, c["a"], c["b"], stats=st)
        assert np.array_equal(out, c["xor"]), (n, sl)
        if not fg:
            assert st.blind_rotate_launches == _launches(n, sl), (n, sl)


def test_launch_counts_the_cases_expect():
    assert [_launches(129, 0), _launches(129, 64), _launches(65, 1), _launches(257, 7), _launches(64, 64), _launches(65, 64)] == [9, 3, 65, 37, 1, 2]


@KERNELS
@pytest.mark.parametrize("sl", [0, 7, 64])
@pytest.mark.parametrize("n", AXIS_N)
def test_blind_rotation_over_n_and_slices(ia, make_keys, fg, n, sl):
    """debug_blind_rotate(x, s) word for word for s in {0, 1, 63, 64, 65, n - 1, all} (those <= n) under "br_slice" 0 (the
    default, 16), 7 and 64.  Rows: the eight crafted-amount rows of test_mod_switch_and_steps_at_crafted_amounts continued to
    n + 1 words (every step index meets 0, even, odd and 2N - 1 amounts); a row that is zero but at steps 63, 64 and n - 1 and a
    row that skips exactly the default slice 16 .. 31, which a wrong lane index or reload offset changes and nothing else does;
    two uniform rows and three encrypted bits.  n = 63, 64, 65: lane 63 of a slice and the step after it; 129: three slices of
    64; 257: the second trip of k_h2_prologue's loop, the b word written by thread 1 of it, key blocks up to index 256, and
    br_bara_stride() = 264 with padding.  On h2 the entries that report Stats take ceil(n / S) launches."""
    _run_axis(ia, make_keys(n, N), fg, sl)


@KERNELS
def test_a_launch_per_step_at_n_65(ia, make_keys, fg):
    """"br_slice" = 1: 65 launches, the accumulator parked and re-read between every two steps."""
    _run_axis(ia, make_keys(65, N), fg, 1)


# ---- 2. whole gates at realistic key lengths ----

_gates257 = {}


def gates257_case(kb):
    if not _gates257:
        bits = np.array([[(v >> k) & 1 for v in range(8)] for k in range(3)], dtype=np.uint8)
        a, b, c = (kb.enc(bits[k], 61 + k) for k in range(3))
        with ThreadPoolExecutor(8) as ex:
            mux = np.stack(list(ex.map(lambda i: kb.ck.mux(a[i], b[i], c[i]), range(8))))
        _gates257.update(bits=bits, a=a, b=b, c=c, mux=mux, **{g: kb.ck.gates_batch(g, a[:4], b[:4], threads=4) for g in ("and", "xor")})
    return _gates257


@KERNELS
def test_gates_at_n_257(ia, make_keys, fg):
    """AND, XOR and bootsMUX on every combination of their inputs at n = 257: the oracle's samples, and the truth tables."""
    kb = make_keys(257, N)
    c = gates257_case(kb)
    bits = c["bits"]
    with _context(ia, kb.p, kb.bk, kb.ksk, fg) as ctx:
        for gate, name, truth in ((ia.GATE_AND, "and", bits[0, :4] & bits[1, :4]), (ia.GATE_XOR, "xor", bits[0, :4] ^ bits[1, :4])):
            st = ia.Stats()
            out = ctx.gates(gate, c["a"][:4], c["b"][:4], stats=st)
            assert np.array_equal(out, c[name]), name
            assert np.array_equal(kb.dec(out), truth), name
            if not fg:
                assert st.blind_rotate_launches == _launches(257, 0) == 17
        out = ctx.mux(c["a"], c["b"], c["c"])
        assert np.array_equal(out, c["mux"])
        assert np.array_equal(kb.dec(out), np.where(bits[0] == 1, bits[1], bits[2]))


def test_xor_and_a_caller_polynomial_at_n_630(ia, make_keys):
    """The key length a ring of this degree is used with, on h2, three rows: XOR, and pbs with a full-range caller polynomial.
    ks_t = 4 / ks_basebit = 2 keeps the key-switch key at 83 MB (the default 8 / 2 is 165 MB, 4 / 4 would be 331 MB); the
    bootstrapping key's spectra are 242 MB on the device.  On the CPU, key generation takes 2.0 s and the six references, on host threads, 1.1 s."""
    kb = make_keys(630, N, ks_t=4, ks_basebit=2)
    p, ck = kb.p, kb.ck
    assert p.ksk_count * 4 < 100e6
    a, b = kb.enc([0, 1, 1], 71), kb.enc([1, 1, 0], 72)
    v = (np.arange(1, N + 1, dtype=np.int64) * 0x01234567 & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    x = np.concatenate([a[1:], np_tfhe.uniform32(np.random.default_rng(630), (1, p.n + 1))])
    with ThreadPoolExecutor(6) as ex:
        want_pbs = ex.map(lambda i: ck.keyswitch(ck.sample_extract(MR.accumulator(ck, x[i], v))), range(3))
        want_xor = ex.map(lambda i: ck.gate("xor", a[i], b[i]), range(3))
        want_pbs, want_xor = np.stack(list(want_pbs)), np.stack(list(want_xor))
    with _context(ia, p, kb.bk, kb.ksk, 0) as ctx:
        st = ia.Stats()
        out = ctx.gates(ia.GATE_XOR, a, b, stats=st)
        assert np.array_equal(out, want_xor) and st.blind_rotate_launches == _launches(630, 0) == 40
        assert np.array_equal(kb.dec(out), [1, 0, 1])
        assert np.array_equal(ctx.pbs(x, v), want_pbs)


# ---- 3. launch width, scratch growth, cuts, two lanes ----

_wide = {}


def wide_case(kb):
    """520 pairs of encrypted bits at n = 8 -- more than two gates per CU of a 256-CU chip -- and the oracle's XOR of each."""
    if not _wide:
        bits = np.random.default_rng(520).integers(0, 2, size=(2, 520)).astype(np.uint8)
        a, b = kb.enc(bits[0], 81), kb.enc(bits[1], 82)
        _wide.update(bits=bits, a=a, b=b, ref=kb.ck.gates_batch("xor", a, b, threads=16))
    return _wide


@KERNELS
def test_scratch_grown_by_a_later_wider_call(ia, make_keys, fg):
    """One context: XOR on 1, 520, 3 and 520 rows.  The second call grows the blind-rotation state a first, small call
    reserved; the third uses the larger block for fewer items (amounts at item x nb, accumulators at item x 2N, the amounts
    behind the accumulators of the ITEMS OF THE LAUNCH); the launch of 520 workgroups is wider than the chip."""
    kb = make_keys(8, N)
    c = wide_case(kb)
    with _context(ia, kb.p, kb.bk, kb.ksk, fg) as ctx:
        assert ctx.get_option("cus") < 520
        for cnt in (1, 520, 3, 520):
            st = ia.Stats()
            out = ctx.gates(ia.GATE_XOR, c["a"][:cnt], c["b"][:cnt], stats=st)
            diff = CS.first_difference(out, c["ref"][:cnt])
            assert diff is None, "%d rows: first at (row, word) %s of %d words" % ((cnt,) + diff)
            assert st.bootstraps == cnt and st.chunks == 1
        assert np.array_equal(kb.dec(out), c["bits"][0] ^ c["bits"][1])


@KERNELS
def test_calls_cut_by_chunk(ia, make_keys, fg):
    """The 520 rows in pieces of 7 (75 pieces, the last of 2) and of 200 (3 pieces): the uncut result, which is the oracle's."""
    kb = make_keys(8, N)
    c = wide_case(kb)
    with _context(ia, kb.p, kb.bk, kb.ksk, fg) as ctx:
        uncut = ctx.gates(ia.GATE_XOR, c["a"], c["b"])
        assert np.array_equal(uncut, c["ref"])
        saved = ctx.get_option("chunk")
        try:
            for chunk in (7, 200):
                ctx.set_chunk(chunk)
                st = ia.Stats()
                out = ctx.gates(ia.GATE_XOR, c["a"], c["b"], stats=st)
                diff = CS.first_difference(out, uncut)
                assert diff is None, "chunk %d: first at (row, word) %s of %d words" % ((chunk,) + diff)
                assert st.chunks == -(-520 // chunk) and st.bootstraps == 520
                if not fg:
                    assert st.blind_rotate_launches == st.chunks and st.keyswitch_launches == st.chunks
        finally:
            ctx.set_chunk(saved)


@KERNELS
def test_levels_under_overlap_min_2(ia, make_keys, fg):
    """A netlist with a MUX over 8 expressions and the 4-bit adder over 4, with "overlap_min" = 2 and with "overlap" = 0 (one
    stream): the same samples, and the oracle's.  The level executor never takes two lanes on this ring: plan_level
    (csrc/evaluator.hip) hands levels to two lanes only where the 64-lane kernels of N = 1024 serve the context (br_supported()),
    so "overlapped_levels" stays where it is, which is asserted -- a change there has to come with a test of its own."""
    from ieache_amd import tools
    kb = make_keys(8, N)
    ck = kb.ck
    bits = np.array([[(v >> k) & 1 for k in range(3)] for v in range(8)], dtype=np.uint8)
    inp = kb.enc(bits, 91)
    nl = ia.Netlist(3)
    w_x = nl.gate(ia.GATE_XOR, nl.input(0), nl.input(1))
    w_m = nl.gate(ia.GATE_MUX, w_x, nl.input(0), nl.input(2))
    w_o = nl.gate(ia.GATE_AND, w_m, w_x)
    want = []
    for e in range(8):
        x = ck.gate("xor", inp[e, 0], inp[e, 1])
        m = ck.mux(x, inp[e, 0], inp[e, 2])
        want.append(np.stack([x, m, ck.gate("and", m, x)]))
    want = np.stack(want)
    width = 4
    info = ia.circuit_info(ia.CIRC_ADD, width)
    vals = [(9, 5), (15, 1), (7, 7), (0, 15)]
    inb = np.zeros((len(vals), info.n_inputs), dtype=np.uint8)
    for e, (u, v) in enumerate(vals):
        inb[e, :width], inb[e, width:2 * width] = tools.int_to_bits(u, width), tools.int_to_bits(v, width)
    add_in = kb.enc(inb, 92)
    add_want = np.stack([ck.add(add_in[e, :width], add_in[e, width:2 * width], add_in[e, 2 * width:2 * width + 1], width)[0] for e in range(len(vals))])
    with _context(ia, kb.p, kb.bk, kb.ksk, fg) as ctx, nl.compile([w_x, w_m, w_o]) as cn:
        saved = {k: ctx.get_option(k) for k in ("overlap", "overlap_min")}
        levels = ctx.get_option("overlapped_levels")
        try:
            ctx.set_option("overlap_min", 2)
            net, add = ctx.eval_netlist(cn, inp), ctx.eval_batch(ia.CIRC_ADD, width, add_in)
            assert ctx.get_option("overlapped_levels") == levels
            ctx.set_option("overlap", 0)
            assert np.array_equal(ctx.eval_netlist(cn, inp), net) and np.array_equal(ctx.eval_batch(ia.CIRC_ADD, width, add_in), add)
        finally:
            for k, v in saved.items():
                ctx.set_option(k, v)
    assert np.array_equal(net, want) and np.array_equal(add, add_want)
    x0, x1, x2 = bits.T
    assert np.array_equal(np.stack([kb.dec(r) for r in net]), np.stack([x0 ^ x1, np.where(x0 ^ x1, x0, x2), np.where(x0 ^ x1, x0, x2) & (x0 ^ x1)], axis=1))
    assert [tools.bits_to_int(kb.dec(r)) for r in add] == [(u + v) % 16 for u, v in vals]


# ---- 4. multi-output extraction, the 2048-word build ----

BOUNDARY = 7  # index in the factor set below
BIAS8 = np.append(BIAS, np.int32(-0x0FEDCBA9))
PICKS = [[ONE], [DENSE, ZERO], [ONE, X1, XHALF, XINV, SPARSE]]
_multi = {}


def multi_case(kb):
    """40 uniform rows at n = 9, two full-range test polynomials with a mixed index array, the seven factors of
    test_pbs_multi_gpu.factor_set at ring 2048 and the boundary factor, a non-zero bias each; the oracle's rows with and
    without the bias: computed once."""
    if not _multi:
        rng = np.random.default_rng(2901)
        x, polys = random_rows(rng, 40, 9), random_polys(rng, 2, N)
        of = rng.integers(0, 2, size=40).astype(np.int32)
        of[:2] = [1, 0]
        factors = np.concatenate([factor_set(rng, N), CS.boundary_factor(N)[None]])
        u, ks = MR.multi_reference_rows(kb.ck, x, polys, factors, of, BIAS8)
        u0 = u.copy()
        u0[..., -1] = np_tfhe._wrap32(u[..., -1].astype(np.int64) - BIAS8[None, :].astype(np.int64))
        ks0 = np.stack([[kb.ck.keyswitch(r) for r in item] for item in u0])
        _multi.update(x=x, polys=polys, of=of, factors=factors, u=u, ks=ks, u0=u0, ks0=ks0)
    return _multi


def _check_multi(ia, ctx, c, count, pick):
    """test_pbs_multi_gpu.test_w64_kernels_word_for_word's body on this ring."""
    x, of, fa = c["x"][:count], c["of"][:count], c["factors"][pick]
    for bias, u, ks in ((BIAS8[pick], c["u"], c["ks"]), (None, c["u0"], c["ks0"])):
        st = ia.Stats()
        out = ctx.pbs_multi(x, c["polys"], fa, of, bias, stats=st)
        assert out.shape == (count, len(pick), 10)
        diff = CS.first_difference(out, ks[:count][:, pick])
        assert diff is None, "key-switched, bias %s: first at (row, factor, word) %s of %d words" % ((bias is not None,) + diff)
        assert st.bootstraps == count and st.levels == 1 and st.keyswitch_launches >= 1
        st = ia.Stats()
        out = ctx.pbs_multi(x, c["polys"], fa, of, bias, keyswitch=False, stats=st)
        assert out.shape == (count, len(pick), N + 1)
        diff = CS.first_difference(out, u[:count][:, pick])
        assert diff is None, "extracted, bias %s: first at (row, factor, word) %s of %d words" % ((bias is not None,) + diff)
        assert st.bootstraps == count and st.keyswitch_launches == 0 and st.blind_rotate_launches >= 1
    if ONE in pick:  # the factor 1 without bias is the single-output bootstrap of the same rows, bit for bit
        t = pick.index(ONE)
        assert np.array_equal(ctx.pbs_multi(x, c["polys"], fa, of)[:, t], ctx.pbs(x, c["polys"], of))
        assert np.array_equal(ctx.pbs_multi(x, c["polys"], fa, of, keyswitch=False)[:, t], ctx.pbs(x, c["polys"], of, keyswitch=False))
    if ZERO in pick:  # the all-zero factor: (0, bias) before the key switch
        t = pick.index(ZERO)
        out = ctx.pbs_multi(x, c["polys"], fa, of, BIAS8[pick], keyswitch=False)[:, t]
        assert not out[:, :N].any() and (out[:, N] == BIAS8[ZERO]).all()


@pytest.mark.parametrize("pick", PICKS, ids=["1", "2", "5"])
def test_multi_output_word_for_word(ia, make_keys, pick):
    """The three factor picks of tests/test_pbs_multi_gpu.py on 1, 3, 5 and 40 rows, with and without bias, with and without
    the key switch, accumulators from k_blind_rotate_h2."""
    kb = make_keys(9, N)
    c = multi_case(kb)
    with _context(ia, kb.p, kb.bk, kb.ksk, 0) as ctx:
        for count in (1, 3, 5, 40):
            _check_multi(ia, ctx, c, count, pick)


def test_multi_output_from_the_any_parameter_kernel(ia, make_keys):
    """One pick under "force_generic": the accumulators k_mv_extract_2048 reads then come from k_blind_rotate_generic."""
    kb = make_keys(9, N)
    c = multi_case(kb)
    with _context(ia, kb.p, kb.bk, kb.ksk, 1) as ctx:
        for count in (1, 40):
            _check_multi(ia, ctx, c, count, PICKS[2])


def test_boundary_factor_and_the_whole_set(ia, make_keys):
    """A factor with non-zero words exactly at coefficients 0, 7, 8, 255, 256, 1023, 1024 and 2047, alone and between two
    others, and all eight factors in one call."""
    kb = make_keys(9, N)
    c = multi_case(kb)
    with _context(ia, kb.p, kb.bk, kb.ksk, 0) as ctx:
        for pick in ([BOUNDARY], [X1, BOUNDARY, DENSE], list(range(8))):
            _check_multi(ia, ctx, c, 5, pick)


def test_factor_limit(ia, make_keys):
    """64 dense full-range factors (kMultiMaxFactors) on two rows; 65 are refused."""
    kb = make_keys(9, N)
    rng = np.random.default_rng(2964)
    x, v = random_rows(rng, 2, 9), random_polys(rng, 1, N)
    factors = rng.integers(INT32_MIN, 1 << 31, size=(65, N), dtype=np.int64).astype(np.int32)
    bias = rng.integers(INT32_MIN, 1 << 31, size=65, dtype=np.int64).astype(np.int32)
    u, ks = MR.multi_reference_rows(kb.ck, x, v, factors[:64], None, bias[:64])
    with _context(ia, kb.p, kb.bk, kb.ksk, 0) as ctx:
        assert CS.first_difference(ctx.pbs_multi(x, v, factors[:64], bias=bias[:64], keyswitch=False), u) is None
        assert CS.first_difference(ctx.pbs_multi(x, v, factors[:64], bias=bias[:64]), ks) is None
        with pytest.raises(ia.IeacheError, match="n_factors must be 1 .. 64") as e:
            ctx.pbs_multi(x, v, factors, bias=bias)
        assert e.value.code == -22


def test_every_cut_of_a_multi_output_call(ia, make_keys):
    """test_every_cut_keeps_rows_with_their_item_and_factor's cuts on this ring: 13 rows, three factors, "chunk" 5, 7 and 2."""
    kb = make_keys(9, N)
    c = multi_case(kb)
    pick = [X1, DENSE, BOUNDARY]
    x, of, polys, fa, bias = c["x"][:13], c["of"][:13], c["polys"], c["factors"][pick], BIAS8[pick]
    with _context(ia, kb.p, kb.bk, kb.ksk, 0) as ctx:
        uncut, uncut_u = ctx.pbs_multi(x, polys, fa, of, bias), ctx.pbs_multi(x, polys, fa, of, bias, keyswitch=False)
        assert np.array_equal(uncut, c["ks"][:13][:, pick]) and np.array_equal(uncut_u, c["u"][:13][:, pick])
        saved = ctx.get_option("chunk")
        try:
            for chunk, pieces in ((5, 13), (7, 7), (2, 13)):  # pieces of max(1, chunk / 3) items: 1, 2 and (chunk < n_factors) 1
                ctx.set_chunk(chunk)
                st = ia.Stats()
                assert np.array_equal(ctx.pbs_multi(x, polys, fa, of, bias, stats=st), uncut), chunk
                assert st.chunks == pieces and st.bootstraps == 13 and st.keyswitch_launches == pieces
                st = ia.Stats()
                assert np.array_equal(ctx.pbs_multi(x, polys, fa, of, bias, keyswitch=False, stats=st), uncut_u), chunk
                assert st.chunks == pieces and st.keyswitch_launches == 0
        finally:
            ctx.set_chunk(saved)


# ---- 5. key switch from 2048-word samples over n ----

KS_SETS = [(255, 4, 2), (256, 1, 4), (257, 8, 2)]  # n = 255: the last single-load row (lwe_stride 256); 8 / 2 is the default


def _ks_bundle(ia, O, make_keys, n, t, bb):
    """(p, bk, ksk, ck).  n = 257 is the generated key of cases 1 and 2; the others are uniform words, which is all a key
    switch sees, under an all-zero bootstrapping key."""
    if (t, bb) == (8, 2):
        kb = make_keys(n, N)
        return kb.p, kb.bk, kb.ksk, kb.ck
    p = ia.default_params().copy(n=n, N=N, ks_t=t, ks_basebit=bb)
    bk, ksk = np.zeros(p.bk_count, dtype=np.int32), np_tfhe.uniform32(np.random.default_rng(n), p.ksk_count)
    return p, bk, ksk, CS.open_oracle(O, p, bk, ksk)


@pytest.mark.parametrize("n,t,bb", KS_SETS, ids=["n%d-t%d-bb%d" % s for s in KS_SETS])
def test_key_switch_families_around_n_256(ia, O, make_keys, n, t, bb):
    """test_key_switch_families_on_the_edge_rows at n = 255, 256, 257 -- output rows of 256, 260 and 260 words: one and two
    16-byte loads per key row and lane -- under the same eight option sets, on 70, 5 and 1 rows."""
    p, bk, ksk, ck = _ks_bundle(ia, O, make_keys, n, t, bb)
    assert (p.ks_t, p.ks_basebit) == (t, bb) and (t, bb) in PL.KS_DECOMPS
    u = PL.edge_rows(np.random.default_rng(n), N, t, bb, 66)
    with ThreadPoolExecutor(16) as ex:
        ref = np.stack(list(ex.map(ck.keyswitch, u)))
    assert np.array_equal(np_tfhe.np_keyswitch(np.reshape(ksk, (N, t, 1 << bb, n + 1)), t, bb, u[64:]), ref[64:])
    for r in (66, 67, 69):  # no row subtracted: (0, b')
        assert not ref[r, :n].any() and ref[r, n] == u[r, N]
    base = dict(force_generic=0, ks_mfma_min=NEVER, ks_sliced_min=NEVER, ks_batch_min=NEVER)
    fams = [("generic", dict(base, force_generic=1)), ("per-gate", dict(base, ks_split_max=1)), ("per-gate, split", dict(base, ks_split_max=16)),
            ("batched", dict(base, ks_batch_min=1)), ("sliced 4", dict(base, ks_sliced_min=1, ks_gates=4)),
            ("sliced 32, slice 600", dict(base, ks_sliced_min=1, ks_gates=32, ks_slice=600)),
            ("mfma", dict(base, ks_mfma_min=1, ks_mfma_split=1)), ("mfma split 8", dict(base, ks_mfma_min=1, ks_mfma_split=8))]
    with ia.Context.from_arrays(p, bk, ksk) as ctx:
        assert ctx.kernel_for_launch(5) == "k_blind_rotate_h2<3,7>"
        assert np.array_equal(ctx.debug_keyswitch(u), ref) and np.array_equal(ctx.keyswitch(u), ref)
        for label, opts in fams:
            for k, val in opts.items():
                ctx.set_option(k, val)
            for rows in (slice(0, 70), slice(65, 70), slice(68, 69)):
                diff = CS.first_difference(ctx.debug_keyswitch(u[rows]), ref[rows])
                assert diff is None, "n %d, %s, rows %s: first at (row, column) %s of %d words" % ((n, label, rows) + diff)
