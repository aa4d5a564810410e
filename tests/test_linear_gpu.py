"""Linear layers on encrypted rows on the GPU (k_linear_simple, k_linear_mfma; csrc/lwe_linear.hip; include/ieache.h section 3n),
word for word against the numpy restatement of the definition (linear_reference.py).  Every comparison runs with "linear_kernel"
forced to the simple kernel (1), to the MFMA product (2) and left to the plan (0).  The bit-exact cases take full-range random
and crafted rows -- no encryption is needed for that; the compositions and the end-to-end test run on keys and assert meanings."""
from fractions import Fraction as F

import numpy as np
import pytest

import linear_reference as LN
import lut_reference as LR
import np_tfhe

pytestmark = pytest.mark.gpu

KERNELS = (1, 2, 0)
GUARD_ROWS = 3
_garbage = np.random.default_rng(15999)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture
def lin(gpu_ctx):
    """gpu_ctx whose contexts get "linear_kernel" put back as it was found (0) afterwards"""
    used = []

    def make(n, N):
        kb, ctx = gpu_ctx(n, N)
        used.append(ctx)
        return kb, ctx

    yield make
    for ctx in used:
        ctx.set_option("linear_kernel", 0)


def expected_kernel(forced, n_out):
    """csrc/linear_plan.h: left to the plan, two outputs or more take the product (kLinearMfmaMinOut, from profiles/linear_rates.txt)"""
    return forced if forced else (2 if n_out >= 2 else 1)


def device_form(ctx, rows, x, W, bias=None, stats=None):
    """The device form on rows of the kind's stride: input padding filled with garbage, the output pre-filled with -1 and
    followed by guard rows.  Checks that every padding word of the output is zero and the guards intact -> the data words."""
    import torch
    p = ctx.params
    words, stride = LN.words_of(p.n, p.N, rows), LN.stride_of(p.n, p.N, rows)
    batch, n_in = x.shape[:2]
    n_out = W.shape[0]
    hx = LN.full_range(_garbage, (batch, n_in, stride))
    hx[..., :words] = x
    tx, tw = dev(hx), dev(np.ascontiguousarray(W, dtype=np.int8))
    tb = None if bias is None else dev(np.asarray(bias, dtype=np.int32))
    tout = torch.full((batch * n_out + GUARD_ROWS, stride), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.lwe_linear_device(rows, batch, n_out, n_in, tw.data_ptr(), None if tb is None else tb.data_ptr(), tx.data_ptr(), tout.data_ptr(), stats=stats)
    got = tout.cpu().numpy()
    assert (got[batch * n_out:] == -1).all(), "a guard row after the output was written"
    body = got[:batch * n_out].reshape(batch, n_out, stride)
    assert not body[..., words:].any(), "a padding word of an output row is not zero"
    return body[..., :words]


def both_forms(ia, ctx, rows, x, W, bias, want, what):
    """device and host form under each kernel choice against `want`; the plan names the kernel; the stats are a linear call's"""
    n_out, n_in = W.shape
    for k in KERNELS:
        ctx.set_option("linear_kernel", k)
        plan = ctx.linear_plan(rows, x.shape[0], n_out, n_in)
        assert plan["kernel"] == expected_kernel(k, n_out) and plan["k_steps"] == -(-n_in // 32), (what, k, plan)
        st = ia.Stats()
        got = device_form(ctx, rows, x, W, bias, stats=st)
        bad = np.argwhere(got != want)
        assert bad.size == 0, "%s, kernel option %d, device form: %d words differ, first at (b, i, w) = %s" % (what, k, len(bad), bad[0])
        assert (st.bootstraps, st.blind_rotate_launches, st.keyswitch_launches, st.levels, st.chunks) == (0, 0, 0, 1, 1) and st.total_ms > 0
        st = ia.Stats()
        host = ctx.lwe_linear(x, W, bias, rows=rows, stats=st)
        assert np.array_equal(host, got), "%s, kernel option %d: the host form differs from the device form" % (what, k)
        assert (st.bootstraps, st.blind_rotate_launches, st.keyswitch_launches, st.levels, st.chunks) == (0, 0, 0, 1, 1) and st.total_ms > 0
    ctx.set_option("linear_kernel", 0)


@pytest.mark.parametrize("batch", [1, 3])
def test_tile_edges(ia, lin, batch):
    """LWE rows at (37, 64): 38 words in rows of 40.  Every n_in around the K step of 32 and the half-step of 16, every n_out
    around the tile of 32, and one output: what the automatic choice leaves to the simple kernel."""
    kb, ctx = lin(37, 64)
    rng = np.random.default_rng(15000 + batch)
    x = LN.full_range(rng, (batch, 65, 38))
    W = LN.weight_cases(rng, 65, 65)["full"]
    bias = LN.full_range(rng, 65)
    for n_in in (1, 15, 16, 17, 31, 32, 33, 64, 65):
        for n_out in (1, 2, 7, 8, 31, 32, 33, 65):  # 2: where the automatic choice changes kernels
            xs, Ws, bs = np.ascontiguousarray(x[:, :n_in]), np.ascontiguousarray(W[:n_out, :n_in]), bias[:n_out]
            want = LN.linear(xs, Ws, bs, 37)
            for k in KERNELS:
                ctx.set_option("linear_kernel", k)
                assert np.array_equal(device_form(ctx, "lwe", xs, Ws, bs), want), (n_in, n_out, k)
    ctx.set_option("linear_kernel", 2)
    assert ctx.lwe_linear(x[:, :33], W[:33, :33], bias[:33]).shape == (batch, 33, 38)
    assert np.array_equal(ctx.lwe_linear(x[:, :33], W[:33, :33], bias[:33]), LN.linear(x[:, :33], W[:33, :33], bias[:33], 37))


@pytest.mark.parametrize("n,N", [(5, 16), (37, 64), (130, 1024)])
def test_row_shapes(ia, lin, n, N):
    """All three kinds at (n_out, n_in) = (33, 33), batch 3: rows of 6, 17 and 32 words (less than, and exactly, one column
    block), 38 / 65 / 128, and 131 / 1 025 / 2 048 (whole blocks); the bias on the bias word only."""
    kb, ctx = lin(n, N)
    rng = np.random.default_rng(15100 + n + N)
    for rows in LN.KINDS:
        words, at = LN.words_of(n, N, rows), LN.bias_word(n, N, rows)
        assert words == {(5, 16): (6, 17, 32), (37, 64): (38, 65, 128), (130, 1024): (131, 1025, 2048)}[(n, N)][LN.KINDS.index(rows)]
        x = LN.full_range(rng, (3, 33, words))
        W = LN.weight_cases(rng, 33, 33)["full"]
        bias = None if at is None else LN.full_range(rng, 33)
        both_forms(ia, ctx, rows, x, W, bias, LN.linear(x, W, bias, at), "%s rows at (%d, %d)" % (rows, n, N))
        if at is not None:
            ctx.set_option("linear_kernel", 2)
            diff = LN.wrap32(device_form(ctx, rows, x, W, bias).astype(np.int64) - device_form(ctx, rows, x, W, None))
            assert not np.delete(diff, at, axis=2).any() and np.array_equal(diff[:, :, at], np.broadcast_to(bias, (3, 33)))
            ctx.set_option("linear_kernel", 0)


def test_tlwe_rows_on_the_ring_of_degree_2048(ia, lin):
    kb, ctx = lin(8, 2048)
    rng = np.random.default_rng(15200)
    x = LN.full_range(rng, (3, 33, 4096))
    W = LN.weight_cases(rng, 33, 33)["full"]
    both_forms(ia, ctx, "tlwe", x, W, None, LN.linear(x, W), "TLWE rows at N = 2048")
    xe = LN.full_range(rng, (2, 5, 2049))
    be = LN.full_range(rng, 9)
    both_forms(ia, ctx, "extracted", xe, W[:9, :5], be, LN.linear(xe, W[:9, :5], be, 2048), "extracted rows at N = 2048")


def test_crafted_data(ia, lin):
    """The identity on asymmetric rows returns them (a transposed operand or result map does not); ones at the corners of W;
    the crafted words, which carry through every byte limb, against the extreme weights."""
    kb, ctx = lin(37, 64)
    rng = np.random.default_rng(15300)
    for n_out, n_in in ((33, 33), (65, 40), (40, 65)):
        x = LN.asymmetric_rows(2, n_in, 38)
        cases = LN.weight_cases(rng, n_out, n_in)
        eye = LN.linear(x, cases["identity"])
        assert np.array_equal(eye[:, :min(n_out, n_in)], x[:, :min(n_out, n_in)]) and not eye[:, n_in:].any()
        both_forms(ia, ctx, "lwe", x, cases["identity"], None, eye, "identity %d x %d" % (n_out, n_in))
        both_forms(ia, ctx, "lwe", x, cases["corners"], None, LN.linear(x, cases["corners"]), "corners %d x %d" % (n_out, n_in))
    xc = LN.crafted_rows(rng, (2, 65, 128))
    for name, W in LN.weight_cases(rng, 33, 65).items():
        both_forms(ia, ctx, "tlwe", xc, W, None, LN.linear(xc, W), "crafted words, weights '%s'" % name)
    for word in LN.CRAFTED_WORDS:
        xw = LN.constant_rows(word, (1, 64, 38))
        for name in ("min", "max"):
            W = LN.weight_cases(rng, 8, 64)[name]
            both_forms(ia, ctx, "lwe", xw, W, None, LN.linear(xw, W), "word %08x, weights '%s'" % (word, name))


@pytest.mark.parametrize("n_out", [1, 33])
def test_the_largest_sum(ia, lin, n_out):
    """n_in = 65 536 on 6-word rows (2 MB of x): every weight -128 on words whose four balanced limbs are -128 -- each limb's
    accumulator ends at 2^30, the bound IEACHE_LINEAR_MAX_DIM stands for -- then +127 on limbs of +127, then random rows."""
    kb, ctx = lin(5, 16)
    rng = np.random.default_rng(15400 + n_out)
    bias = LN.full_range(rng, n_out)
    for word, weight in ((0x7F7F7F80, -128), (0x7F7F7F7F, 127), (None, None)):
        x = LN.full_range(rng, (1, 65536, 6)) if word is None else LN.constant_rows(word, (1, 65536, 6))
        W = LN.weight_cases(rng, n_out, 65536)["full"] if weight is None else np.full((n_out, 65536), weight, dtype=np.int8)
        both_forms(ia, ctx, "lwe", x, W, bias, LN.linear(x, W, bias, 5), "n_in = 65536, word %s" % word)
    # one more input is refused, by both forms, before anything is read
    x = np.zeros((1, 65537, 6), dtype=np.int32)
    W = np.zeros((n_out, 65537), dtype=np.int8)
    with pytest.raises(ia.IeacheError, match="1 .. 65536") as e:
        ctx.lwe_linear(x, W)
    assert e.value.code == -22
    with pytest.raises(ia.IeacheError, match="1 .. 65536"):
        ctx.lwe_linear_device("lwe", 1, n_out, 65537, 0, None, 0, 0)


def test_stats_refusals_and_the_empty_call(ia, lin):
    import torch
    kb, ctx = lin(37, 64)
    stride = ctx.lwe_stride
    rng = np.random.default_rng(15500)
    x, W, bias = LN.full_range(rng, (2, 5, 38)), LN.weight_cases(rng, 9, 5)["full"], LN.full_range(rng, 9)
    tx, tw, tb = dev(np.pad(x, ((0, 0), (0, 0), (0, stride - 38)))), dev(W), dev(bias)
    tout = torch.full((2 * 9 + GUARD_ROWS, 2 * 64), -1, dtype=torch.int32, device="cuda")  # room for TLWE rows too
    torch.cuda.synchronize()
    ptr = lambda t: t.data_ptr()
    # batch == 0 writes nothing and names no memory
    st = ia.Stats()
    ctx.lwe_linear_device("lwe", 0, 9, 5, ptr(tw), ptr(tb), ptr(tx), ptr(tout), stats=st)
    ctx.lwe_linear_device("lwe", 0, 9, 5, None, None, None, None)
    assert (tout.cpu().numpy() == -1).all() and st.bootstraps == 0 and st.chunks == 0
    assert ctx.lwe_linear(x[:0], W, bias).shape == (0, 9, 38)

    def refused(match, f, *a, **kw):
        with pytest.raises(ia.IeacheError, match=match) as e:
            f(*a, **kw)
        assert e.value.code == -22

    call = ctx.lwe_linear_device
    refused("unknown rows kind", call, 3, 2, 9, 5, ptr(tw), ptr(tb), ptr(tx), ptr(tout))
    refused("unknown rows kind", call, -1, 2, 0, 5, None, None, None, None)
    refused("1 .. 65536", call, "lwe", 2, 0, 5, ptr(tw), ptr(tb), ptr(tx), ptr(tout))
    refused("1 .. 65536", call, "tlwe", 2, 9, 0, ptr(tw), ptr(tb), ptr(tx), ptr(tout))
    refused("TLWE rows have no bias word", call, "tlwe", 1, 9, 5, ptr(tw), ptr(tb), None, None)
    refused("lwe_linear: null argument", call, "lwe", 2, 9, 5, None, ptr(tb), ptr(tx), ptr(tout))
    refused("lwe_linear: null argument", call, "lwe", 2, 9, 5, ptr(tw), ptr(tb), None, ptr(tout))
    refused("lwe_linear: null argument", call, "lwe", 2, 9, 5, ptr(tw), ptr(tb), ptr(tx), None)
    # overlap: the output over x (the whole, its last word, one word into the output's end), over W, over the bias
    x_words, out_words = 2 * 5 * stride, 2 * 9 * stride
    for d_out in (ptr(tx), ptr(tx) + 4 * (x_words - 1), ptr(tx) - 4 * (out_words - 1)):
        refused("overlaps an input", call, "lwe", 2, 9, 5, ptr(tw), ptr(tb), ptr(tx), d_out)
    refused("overlaps an input", call, "lwe", 2, 9, 5, ptr(tw), ptr(tb), ptr(tx), ptr(tw) + 44)
    refused("overlaps an input", call, "lwe", 2, 9, 5, ptr(tw), ptr(tb), ptr(tx), ptr(tb) + 32)
    refused("overlaps an input", call, "lwe", 2, 9, 5, ptr(tout) + 64, ptr(tb), ptr(tx), ptr(tout))
    # a host pointer to the device form
    refused("not a device pointer", call, "lwe", 2, 9, 5, W.ctypes.data, ptr(tb), ptr(tx), ptr(tout))
    refused("not a device pointer", call, "lwe", 2, 9, 5, ptr(tw), ptr(tb), x.ctypes.data, ptr(tout))
    assert (tout.cpu().numpy() == -1).all(), "a refused call wrote"
    # the host form's refusals
    refused("unknown rows kind", ctx.lwe_linear, x, W, bias, rows=5)
    refused("TLWE rows have no bias word", ctx.lwe_linear, np.zeros((1, 5, 128), dtype=np.int32), W, bias, rows="tlwe")
    with pytest.raises(ValueError, match="-128 .. 127"):
        ctx.lwe_linear(x, W.astype(np.int64) * 2)
    refused("unknown rows kind", ctx.linear_plan, 3, 1, 1, 1)
    refused("1 .. 65536", ctx.linear_plan, "lwe", 1, 65537, 1)
    # the option: 0, 1, 2 and nothing else
    for v in (-1, 3, 100):
        assert not ctx.set_option_ok("linear_kernel", v)
    assert ctx.get_option("linear_kernel") == 0
    for v in (1, 2, 0):
        ctx.set_option("linear_kernel", v)
        assert ctx.get_option("linear_kernel") == v
    # the plan's figures: 40 words = 2 column blocks; 9 outputs = one tile; 5 inputs = one K step
    assert ctx.linear_plan("lwe", 2, 9, 5) == dict(kernel=2, col_blocks=2, wave_tiles=1, k_steps=1)
    assert ctx.linear_plan("tlwe", 2, 1, 65) == dict(kernel=1, col_blocks=4, wave_tiles=1, k_steps=3)
    assert ctx.linear_plan("tlwe", 2, 2, 65)["kernel"] == 2
    assert ctx.linear_plan("extracted", 1, 65, 64)["wave_tiles"] == 4 and ctx.linear_plan("extracted", 1, 64, 64)["wave_tiles"] == 2
    # a warm host call allocates nothing
    ctx.lwe_linear(x, W, bias)
    before = ctx.get_option("staging_allocations")
    ctx.lwe_linear(x, W, bias)
    assert ctx.get_option("staging_allocations") == before


def lwe_phases(lwe_key, rows):
    return LR.phases(lwe_key, rows)


def test_sums_of_extracted_rows_before_one_key_switch(ia, lin):
    """EXTRACTED rows: weighted sums of pbs(..., keyswitch=False) outputs with a bias, then ONE key switch, against the same
    composed from the references -- the C reference of the sum and the oracle's key switch -- word for word."""
    from ieache_amd import tools
    kb, ctx = lin(37, 64)
    p = kb.p
    rng = np.random.default_rng(15600)
    x = LN.full_range(rng, (12, p.n + 1))
    v = LN.full_range(rng, p.N)
    u = ctx.pbs(x, v, keyswitch=False)  # [12][N+1]
    assert np.array_equal(u, LR.pbs_reference_rows(kb.ck, x, v, keyswitch=False))
    W = np.array([[1, 1, 0, 0], [1, -1, 2, -2], [127, -128, 5, 0]])
    bias = np.array([1 << 29, -(1 << 29), 12345], dtype=np.int32)
    sums_ref = tools.lwe_linear_reference(p, u.reshape(3, 4, p.N + 1), W, bias, "extracted")
    want = np.stack([kb.ck.keyswitch(row) for row in sums_ref.reshape(-1, p.N + 1)]).reshape(3, 3, p.n + 1)
    for k in KERNELS:
        ctx.set_option("linear_kernel", k)
        sums = ctx.lwe_linear(u.reshape(3, 4, p.N + 1), W, bias, rows="extracted")
        assert np.array_equal(sums, sums_ref), k
        assert np.array_equal(ctx.keyswitch(sums.reshape(-1, p.N + 1)).reshape(3, 3, p.n + 1), want), k


def test_slot_wise_arithmetic_on_packed_samples(ia, lin):
    """pack, then the TLWE kind: slot k of output i carries sum_j W[i][j] x (phase of row (j, k)), what the LWE kind gives on the
    rows themselves, up to the packing noise of DESIGN.md section 7: per packed sample m w n t E[d^2] alpha^2 of key noise plus
    (n / 2) 2^(-2tb) / 12 of rounding, here m w = 16, n = 130, (t, b) = (8, 2), alpha = 2^-25; the sums weigh it with ||w||_2.
    Six of those deviations.  unpack without its key switch hands the same slots out as rows, exactly."""
    from ieache_amd import tools
    kb, ctx = lin(130, 1024)
    p = kb.p
    m, n_in = 16, 5
    rng = np.random.default_rng(15700)
    rows = LN.full_range(rng, (n_in, m, p.n + 1))
    W = np.array([[1, 1, 1, 1, 1], [3, -2, 0, 1, -1], [-128, 127, 64, -64, 1]])
    sigma_pack = np.sqrt(m * p.n * 8 * 3.5 * p.tlwe_alpha_min ** 2 + (p.n / 2) * 2.0 ** -32 / 12)
    pk = tools.packing_keygen(p, kb.lwe_key, kb.tlwe_key, seed=157)
    try:
        ctx.set_packing_key(pk)
        packed = ctx.pack(rows)  # [n_in][2][N]: sample j holds rows (j, 0 .. m-1) on slots 0 .. m-1
        assert np.array_equal(packed, tools.pack_reference(p, pk, rows))
        by_slot = np.ascontiguousarray(rows.transpose(1, 0, 2))  # [m][n_in][n+1]
        for k in KERNELS:
            ctx.set_option("linear_kernel", k)
            on_samples = ctx.lwe_linear(packed.reshape(1, n_in, 2 * p.N), W, rows="tlwe")[0].reshape(3, 2, p.N)
            on_rows = ctx.lwe_linear(by_slot, W)  # [m][3][n+1]
            assert np.array_equal(on_samples, LN.linear(packed.reshape(1, n_in, 2 * p.N), W)[0].reshape(3, 2, p.N))
            ph_samples = tools.tlwe_phase(p, kb.tlwe_key, on_samples)[:, :m]  # [3][m] Torus32
            ph_rows = lwe_phases(kb.lwe_key, on_rows).T  # [3][m] fractions
            d = ph_samples.astype(np.float64) / 2.0 ** 32 - ph_rows
            d -= np.round(d)
            for i in range(3):
                bound = 6 * np.sqrt(float((W[i].astype(np.int64) ** 2).sum())) * sigma_pack
                print("kernel option %d, output %d: largest slot error %.3e, bound %.3e" % (k, i, np.abs(d[i]).max(), bound))
                assert np.abs(d[i]).max() < bound, (k, i)
            # the way back: the slots as extracted rows under the ring key carry exactly those phases
            back = ctx.unpack(on_samples, first=0, width=m, keyswitch=False)  # [3][m][N+1]
            ring = LN.wrap32(back[..., p.N].astype(np.int64) - (back[..., :p.N].astype(np.int64) * np.asarray(kb.tlwe_key[:p.N], dtype=np.int64)).sum(-1))
            assert np.array_equal(ring, ph_samples)
    finally:
        ctx.set_packing_key(None)


def encrypt_phases(p, lwe_key, phases, rng):
    """fresh LWE encryptions of the given fractions of the torus with the parameter set's noise -> [..][n+1]"""
    phases = np.asarray(phases, dtype=object)
    flat = phases.reshape(-1)
    a = np_tfhe.uniform32(rng, (len(flat), p.n))
    e = np_tfhe.gaussian32(rng, p.lwe_alpha_min, len(flat)).astype(np.int64)
    mu = np.array([int(round(F(t) * (1 << 32))) for t in flat], dtype=np.int64)
    out = np.zeros((len(flat), p.n + 1), dtype=np.int32)
    out[:, :p.n] = a
    out[:, p.n] = LN.wrap32((a.astype(np.int64) * np.asarray(lwe_key[:p.n], dtype=np.int64)).sum(-1) + mu + e)
    return out.reshape(phases.shape + (p.n + 1,))


def test_two_dense_layers_at_the_product_parameters(ia, lin):
    """n = 630, N = 1024, (3, 7): 16 fresh inputs of fan-in 8 at +-1/32 -> a sign layer of 4 neurons (weights +-1, bias 1/32, outputs
    +-1/10: at least 12 sigma on fresh inputs) -> the worked fan-in-4 neuron of DESIGN.md section 7 (weights 1, 1, -1, -1, bias
    1/20, about 7.2 sigma) -> decode.  First the composition of references (the C reference of the sums, the oracle's stages on host
    threads), then the card through Dense.run: its rows equal the reference's word for word, and neither has a wrong decode."""
    from ieache_amd import layers
    kb, ctx = lin(630, 1024)
    p = kb.p
    assert (p.N, p.l, p.Bgbit, p.ks_t, p.ks_basebit) == (1024, 3, 7, 8, 2)
    T = layers.torus
    rng = np.random.default_rng(15800)
    W1 = np.array([[1, 1, 1, 1, -1, -1, -1, -1], [1, -1, 1, -1, 1, -1, 1, -1], [1, 1, -1, -1, 1, 1, -1, -1], [-1, 1, 1, -1, 1, -1, -1, 1]])
    first = layers.sign_layer(W1, [T(F(1, 32))] * 4, inputs=(F(-1, 32), F(1, 32)), mu=T(F(1, 10)))
    second = layers.sign_layer([[1, 1, -1, -1]], [T(F(1, 20))], inputs=(F(-1, 10), F(1, 10)), mu=T(F(1, 8)))
    signs = rng.integers(0, 2, size=(16, 8)) * 2 - 1
    clear1 = first.run_clear([[F(int(s), 32) for s in row] for row in signs])  # [16][4] words: +-1/10
    clear2 = second.run_clear([[F(int(w), 1 << 32) for w in row] for row in clear1])[:, 0]
    want_bits = (clear2 > 0).astype(np.uint8)
    assert 0 < want_bits.sum() < 16  # both answers occur
    x = encrypt_phases(p, kb.lwe_key, [[F(int(s), 32) for s in row] for row in signs], rng)  # [16][8][n+1]
    pbs = lambda rows, v: LR.pbs_reference_rows(kb.ck, rows, v)
    mid_ref = first.run_reference(p, x, pbs)                      # [16][4][n+1]
    out_ref = second.run_reference(p, mid_ref, pbs)               # [16][1][n+1]
    assert np.array_equal((lwe_phases(kb.lwe_key, mid_ref) > 0), clear1 > 0), "the reference composition decodes a first-layer output wrong"
    assert np.array_equal(kb.dec(out_ref[:, 0]), want_bits), "the reference composition decodes wrong"
    for k in KERNELS:
        ctx.set_option("linear_kernel", k)
        mid = first.run(ctx, x)
        out = second.run(ctx, mid)
        assert np.array_equal(mid, mid_ref) and np.array_equal(out, out_ref), "kernel option %d: the card's rows differ from the reference's" % k
        assert np.array_equal(kb.dec(out[:, 0]), want_bits)
    err = np.abs(lwe_phases(kb.lwe_key, out_ref[:, 0]) - np.where(want_bits == 1, 0.125, -0.125)).max()
    print("largest output phase error %.4f against the decoding margin of 0.125" % err)
