"""The packing key switch on the GPU (csrc/pack_keyswitch.hip) word for word against the numpy restatement of the definition
(pack_reference.py).  All bit-exact cases take random full-range key arrays and rows -- no encryption is needed for that -- so
the reference stays cheap; the end-to-end tests run at the reference's parameters and assert the decoding margin only."""
import numpy as np
import pytest

import lut_reference as LR
import pack_reference as PR

pytestmark = pytest.mark.gpu


def SHIFTS(N):
    return [0, 1, N - 1, N, N + 1, 2 * N - 1]


_keys = {}


def random_key(p, t, b):
    """one full-range random key per (n, N, t, b), shared by the tests"""
    k = (p.n, p.N, t, b)
    if k not in _keys:
        _keys[k] = PR.full_range(np.random.default_rng(8000 + 7 * p.n + p.N + 31 * t + b), (p.n, t, 2, p.N))
    return _keys[k]


def splits_allowed(p, t):
    """csrc/pack_plan.h: 1, 2, 4, 8, none longer than the walk of ceil(n t / 32) K steps"""
    return [k for k in (1, 2, 4, 8) if k <= -(-p.n * t // 32)]


@pytest.fixture
def keyed(gpu_ctx):
    """gpu_ctx whose contexts get the packing options and the key put back as they were found (no key) afterwards"""
    used = []

    def make(n, N):
        kb, ctx = gpu_ctx(n, N)
        used.append(ctx)
        return kb, ctx

    yield make
    for ctx in used:
        ctx.set_packing_key(None)
        ctx.set_option("pack_piece_rows", 4096)


def rows_as_groups(ctx, rows, **kw):
    """every row a group of its own: out_g = R_g, the product alone"""
    return ctx.pack(rows[:, None, :], **kw)


# n t against the K step of 32: at (8, 2) 40, 296 and 1 040 all end in a partly padded step; n = 130 at (16, 1) is 65 whole steps,
# n = 5 at (4, 4) and (5, 3) a walk shorter than one step
@pytest.mark.parametrize("n,N", [(5, 1024), (37, 1024), (130, 1024), (37, 16), (37, 64)])
def test_product_word_for_word(ia, keyed, n, N):
    kb, ctx = keyed(n, N)
    p = kb.p
    rng = np.random.default_rng(8100 + n + N)
    # (8, 2): tile edges and past one block of rows
    rows = PR.crafted_rows(rng, 513, n, 8, 2)
    pk = random_key(p, 8, 2)
    R = PR.product_fast(pk, rows, 8, 2)
    ctx.set_packing_key(pk)
    for count in (1, 31, 32, 33, 127, 128, 129, 513):
        st = ia.Stats()
        assert np.array_equal(rows_as_groups(ctx, rows[:count], stats=st), R[:count]), count
        assert st.bootstraps == 0 and st.levels == 1 and st.keyswitch_launches == 1 and st.chunks == 1 and st.total_ms > 0 and st.keyswitch_ms > 0
    # the same kernel for every accepted decomposition: 33 rows each
    for t, b in [(4, 4), (5, 3), (16, 1), (31, 1)]:
        rows_tb = PR.crafted_rows(rng, 33, n, t, b)
        pk_tb = random_key(p, t, b)
        ctx.set_packing_key(pk_tb, t=t, basebit=b)
        assert np.array_equal(rows_as_groups(ctx, rows_tb), PR.product_fast(pk_tb, rows_tb, t, b)), (t, b)
    # crafted keys whose words carry through every byte limb, 129 rows
    for name, key in PR.crafted_keys(n, 8, N).items():
        ctx.set_packing_key(key)
        assert np.array_equal(rows_as_groups(ctx, rows[:129]), PR.product_fast(key, rows[:129], 8, 2)), name


@pytest.mark.parametrize("n,N,t,b", [(5, 1024, 8, 2), (37, 1024, 8, 2), (130, 1024, 8, 2), (37, 64, 31, 1), (5, 16, 4, 4)])
def test_every_k_split_gives_the_same_words(ia, keyed, n, N, t, b):
    kb, ctx = keyed(n, N)
    p = kb.p
    rows = PR.crafted_rows(np.random.default_rng(8200 + n), 129, n, t, b)
    pk = random_key(p, t, b)
    want = PR.product_fast(pk, rows, t, b)
    ctx.set_packing_key(pk, t=t, basebit=b)
    allowed = splits_allowed(p, t)
    assert allowed[0] == 1 and (n * t > 32) == (len(allowed) > 1)
    for split in [0] + allowed:
        ctx.set_option("pack_split", split)
        assert ctx.get_option("pack_split") == split
        plan = ctx.pack_plan(129, 1)
        assert plan["k_steps"] == -(-n * t // 32) and plan["pieces"] == 1 and (plan["k_split"] == split if split else plan["k_split"] in allowed)
        assert np.array_equal(rows_as_groups(ctx, rows), want), split
    for split in (3, 16) + tuple(k for k in (2, 4, 8) if k not in allowed):
        assert not ctx.set_option_ok("pack_split", split)
    # a new key starts from the automatic choice: a forced split belongs to the walk of the key it was set for
    ctx.set_option("pack_split", allowed[-1])
    ctx.set_packing_key(pk, t=t, basebit=b)
    assert ctx.get_option("pack_split") == 0


@pytest.mark.parametrize("N", [16, 64, 1024])
def test_placement(ia, keyed, N):
    n = 37
    kb, ctx = keyed(n, N)
    p = kb.p
    pk = random_key(p, 8, 2)
    ms = [m for m in (1, 2, 33, N) if m <= N]
    rows = PR.crafted_rows(np.random.default_rng(8300 + N), 3 * N, n, 8, 2)
    R = PR.product_fast(pk, rows, 8, 2)
    ctx.set_packing_key(pk)
    for m in ms:
        for spread in sorted({1, N // m}):
            S = PR.spread_sums(R[:3 * m], spread)
            for shift in SHIFTS(N):
                for groups in (1, 3):
                    got = ctx.pack(rows[:groups * m].reshape(groups, m, n + 1), spread=spread, shift=shift)
                    assert got.shape == (groups, 2, N)
                    assert np.array_equal(got, PR.place(S, groups, m, spread, shift)), (m, spread, shift, groups)
    # m = N at spread 1: the last coefficient, and the wrap sign at shift 1 -- row N - 1 lands on coefficient 0, negated
    one = np.zeros((N, n + 1), dtype=np.int32)  # a = 0: every digit is 0 at (8, 2), R_r = (0, b_r)
    one[:, n] = np.arange(1, N + 1)
    at0, at1 = ctx.pack(one, spread=1, shift=0)[0], ctx.pack(one, spread=1, shift=1)[0]
    digit0 = PR.product_fast(pk, one[:1], 8, 2)[0]
    assert not PR.digits(one[:1], n, 8, 2).any() and not digit0[0].any() and digit0[1, 0] == 1 and not digit0[1, 1:].any()
    assert not at0[0].any() and np.array_equal(at0[1], np.arange(1, N + 1))
    assert at1[1, 0] == -N and np.array_equal(at1[1, 1:], np.arange(1, N)) and not at1[0].any()
    # a single row list [m][n+1] is one group; m may be given for flat rows
    assert np.array_equal(ctx.pack(rows[:6], m=2), ctx.pack(rows[:6].reshape(3, 2, n + 1)))
    st = ia.Stats()
    assert ctx.pack(rows[:0].reshape(0, 2, n + 1), stats=st).shape == (0, 2, N) and st.keyswitch_launches == 0


def device_rows(rows, stride):
    import torch
    d = torch.zeros((rows.shape[0], stride), dtype=torch.int32, device="cuda")
    d[:, : rows.shape[1]] = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    return d


def test_pieces_host_and_device_form(ia, keyed):
    import torch
    n, N = 37, 1024
    kb, ctx = keyed(n, N)
    pk = random_key(kb.p, 8, 2)
    rows = PR.crafted_rows(np.random.default_rng(8400), 5 * 33, n, 8, 2).reshape(5, 33, n + 1)
    ctx.set_packing_key(pk)
    spread, shift = 31, N + 1
    st = ia.Stats()
    whole = ctx.pack(rows, spread=spread, shift=shift, stats=st)
    assert st.keyswitch_launches == 1 and st.chunks == 1
    assert np.array_equal(whole, PR.pack(pk, rows.reshape(-1, n + 1), 33, spread=spread, shift=shift))
    d_rows, d_out = device_rows(rows.reshape(-1, n + 1), ctx.lwe_stride), torch.full((5, 2, N), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for piece_rows, pieces in ((4096, 1), (100, 2), (64, 5), (1, 5)):
        ctx.set_option("pack_piece_rows", piece_rows)
        st = ia.Stats()
        assert np.array_equal(ctx.pack(rows, spread=spread, shift=shift, stats=st), whole)
        assert st.keyswitch_launches == pieces and st.chunks == pieces and st.bootstraps == 0 and st.levels == 1
        assert ctx.pack_plan(5, 33)["pieces"] == pieces
        d_out.fill_(-1)
        torch.cuda.synchronize()
        st = ia.Stats()
        ctx.pack_device(5, 33, spread, shift, d_rows.data_ptr(), d_out.data_ptr(), stats=st)
        assert np.array_equal(d_out.cpu().numpy(), whole) and st.keyswitch_launches == pieces
        assert np.array_equal(d_rows.cpu().numpy()[:, :n + 1], rows.reshape(-1, n + 1))
    assert not ctx.set_option_ok("pack_piece_rows", 0) and not ctx.set_option_ok("pack_piece_rows", 4097)
    # a warm host call allocates nothing
    warm = ctx.get_option("staging_allocations")
    ctx.pack(rows, spread=spread, shift=shift)
    assert ctx.get_option("staging_allocations") == warm
    # refusals of the device form, all before anything is launched
    ctx.pack_device(0, 33, spread, shift, d_rows.data_ptr(), d_out.data_ptr())
    with pytest.raises(ia.IeacheError, match="overlaps"):
        ctx.pack_device(1, 33, 1, 0, d_rows.data_ptr(), d_rows.data_ptr() + 64)
    with pytest.raises(ia.IeacheError, match="not a device pointer"):
        ctx.pack_device(5, 33, spread, shift, rows.ctypes.data, d_out.data_ptr())
    for bad, match in (((0, 1, 0), "m must"), ((33, 0, 0), "spread must"), ((33, 32, 0), "exceed N"), ((1025, 1, 0), "exceed N"),
                       ((33, 1, 2 * N), "shift"), ((33, 1, -1), "shift")):
        with pytest.raises(ia.IeacheError, match=match) as e:
            ctx.pack_device(1, bad[0], bad[1], bad[2], d_rows.data_ptr(), d_out.data_ptr())
        assert e.value.code == -22
    with pytest.raises(ia.IeacheError, match="exceed N"):
        ctx.pack(rows, spread=32)
    assert ctx.pack(rows, spread=31, shift=2 * N - 1).shape == (5, 2, N)


def test_replacing_and_dropping_the_key(ia, keyed):
    n, N = 37, 1024
    kb, ctx = keyed(n, N)
    p = kb.p
    bits = np.random.default_rng(8500).integers(0, 2, size=(2, 40)).astype(np.uint8)
    a, b = kb.enc(bits[0], 51), kb.enc(bits[1], 52)
    before = ctx.gates(ia.GATE_NAND, a, b)
    rows = PR.crafted_rows(np.random.default_rng(8501), 33, n, 8, 2)
    ctx.set_packing_key(None)  # nothing set: dropping is no error
    with pytest.raises(ia.IeacheError, match="no packing key set") as e:
        ctx.pack(rows)
    assert e.value.code == -22
    first, second = random_key(p, 8, 2), random_key(p, 5, 3)
    ctx.set_packing_key(first)
    assert np.array_equal(ctx.pack(rows, spread=2, shift=3), PR.pack(first, rows, 33, spread=2, shift=3))
    ctx.set_packing_key(second, t=5, basebit=3)
    assert np.array_equal(ctx.pack(rows, spread=2, shift=3), PR.pack(second, rows, 33, spread=2, shift=3, t=5, basebit=3))
    assert np.array_equal(ctx.gates(ia.GATE_NAND, a, b), before)
    # refused sets leave the key that is there in place
    for t, bb, match in ((16, 2, "below 32"), (8, 5, "pk_basebit"), (0, 2, "pk_t")):
        with pytest.raises(ia.IeacheError, match=match):
            ctx.set_packing_key(np.zeros((n, max(t, 1), 2, N), dtype=np.int32), t=t, basebit=bb)
    with pytest.raises(ValueError):
        ctx.set_packing_key(first[:-1])
    assert np.array_equal(ctx.pack(rows, spread=2, shift=3), PR.pack(second, rows, 33, spread=2, shift=3, t=5, basebit=3))
    ctx.set_packing_key(None)
    with pytest.raises(ia.IeacheError, match="no packing key set"):
        ctx.pack(rows)
    with pytest.raises(ia.IeacheError, match="no packing key set"):
        ctx.pack_plan(1, 33)
    # the scratch went with the key: a key set again starts from nothing and gives the same words
    ctx.set_packing_key(first)
    assert np.array_equal(ctx.pack(rows, spread=2, shift=3), PR.pack(first, rows, 33, spread=2, shift=3))
    ctx.set_packing_key(None)
    assert np.array_equal(ctx.gates(ia.GATE_NAND, a, b), before)
    # a context of its own that never had a key
    with ia.Context.from_arrays(p, kb.bk, kb.ksk) as fresh:
        with pytest.raises(ia.IeacheError, match="no packing key set"):
            fresh.pack(rows)
        assert np.array_equal(fresh.gates(ia.GATE_NAND, a, b), before)


def torus_distance(a, b):
    d = (np.asarray(a, dtype=np.int64) - np.asarray(b, dtype=np.int64)) & 0xFFFFFFFF
    return np.minimum(d, (1 << 32) - d).astype(np.float64) / 2.0 ** 32


def test_end_to_end_at_the_reference_parameters(ia, keyed):
    """(a) gate outputs packed at spread 1 decode through tlwe_phase; (b) four gate-output entries packed at the table layout are
    a table for pbs(..., tlwe=True): encrypted indices 0 .. 3 come out as f[idx], for two tables.  Both assert the decoding
    margin only; the largest phase errors are printed (pytest -s; scripts/pack_rates.py records them)."""
    from ieache_amd import tools
    kb, ctx = keyed(630, 1024)
    p, N = kb.p, 1024
    pk = tools.packing_keygen(p, kb.lwe_key, kb.tlwe_key, seed=61)
    ctx.set_packing_key(pk)
    rng = np.random.default_rng(8600)
    # (a) 256 XOR outputs, one TLWE sample
    bits = rng.integers(0, 2, size=(2, 256)).astype(np.uint8)
    outs = ctx.gates(ia.GATE_XOR, kb.enc(bits[0], 62), kb.enc(bits[1], 63))
    want = bits[0] ^ bits[1]
    assert np.array_equal(kb.dec(outs), want)
    packed = ctx.pack(outs)
    assert packed.shape == (1, 2, N) and np.array_equal(packed, tools.pack_reference(p, pk, outs))
    phase = tools.tlwe_phase(p, kb.tlwe_key, packed)[0].astype(np.float64) / 2.0 ** 32
    err_bits, err_rest = np.abs(phase[:256] - np.where(want == 1, 0.125, -0.125)).max(), np.abs(phase[256:]).max()
    print("pack 256 gate outputs: largest phase error %.3e on the bits, %.3e elsewhere (margin 1/8)" % (err_bits, err_rest))
    assert err_bits < 1 / 8 and err_rest < 1 / 8
    assert np.array_equal((phase[:256] > 0).astype(np.uint8), want)
    # (b) tables of four entries that are themselves gate outputs
    spread, shift = tools.lut_pack_layout(p, 4)
    msgs = np.repeat(np.arange(4), 4)
    x = LR.encrypt_messages(p, kb.lwe_key, msgs, 4, rng)
    for f_bits in ([1, 0, 0, 1], [0, 1, 1, 1]):
        f_bits = np.array(f_bits, dtype=np.uint8)
        entries = ctx.gates(ia.GATE_AND, kb.enc(f_bits, 64), kb.enc(np.ones(4, dtype=np.uint8), 65))
        table = ctx.pack(entries, spread=spread, shift=shift)
        f = np.where(f_bits == 1, 1 << 29, -(1 << 29)).astype(np.int32)
        err = torus_distance(tools.tlwe_phase(p, kb.tlwe_key, table)[0], tools.lut_test_poly(p, f)).max()
        out = ctx.pbs(x, table, tlwe=True)
        out_err = np.abs(LR.phases(kb.lwe_key, out) - np.where(f_bits[msgs] == 1, 0.125, -0.125)).max()
        print("cloud-built table %s: largest phase error of the table %.3e, of the lookups %.3e (margin 1/8)" % (f_bits.tolist(), err, out_err))
        assert err < 1 / 8 and out_err < 1 / 8
        assert np.array_equal(kb.dec(out), f_bits[msgs])

