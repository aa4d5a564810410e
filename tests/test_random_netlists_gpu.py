"""Random netlists on the GPU: the wire store and the level executor (run_items, resolve, k_level_combine, k_gather_outputs)
under every way a level is cut.  Every comparison is exact: output words against the CPU oracle walked gate by gate
(tests/test_random_netlists_cpu.py has shown that it decrypts to the plain wire walk on these very inputs), and every cut
-- pieces of one and three rotation items, level halves on two lanes, expression pipelines, the two-limb kernels, the
any-parameter kernels, batches of one and none -- against the default run.  A store whose level writes a slot the same level
still reads gives the right words as long as a level is one piece; it is the cuts that show it."""
import numpy as np
import pytest

import random_netlists as rn

pytestmark = pytest.mark.gpu

SMALL, LARGE = (5, 64), (16, 1024)
CASES = [(p, seed, family) for p in (SMALL, LARGE) for seed, family in rn.corpus(p)]
OPTIONS = ("chunk", "overlap", "overlap_min", "pipe_min", "pipe_auto", "exact_fft")


def test_the_corpus_is_the_one_the_cpu_tests_proved():
    assert len(rn.corpus(SMALL)) == 24 and len(rn.corpus(LARGE)) == 6 and len(CASES) == 30


def _expected_passthrough(kb, outs, inp_e):
    """Rows of the outputs that are not gates: an input row, its negation, a constant."""
    rows = {}
    for i, o in enumerate(outs):
        if o < 0:
            rows[i] = kb.ck.constant(1 if o == rn.TRUE else 0)
        elif (o >> 1) < inp_e.shape[0]:
            rows[i] = rn._neg(inp_e[o >> 1]) if o & 1 else inp_e[o >> 1]
    return rows


@pytest.mark.parametrize("params,seed,family", CASES, ids=["%d-%d-%d-%s" % (p[0], p[1], s, f) for p, s, f in CASES])
def test_random_netlist_under_every_cut(ia, gpu_ctx, params, seed, family):
    kb, ctx = gpu_ctx(*params)
    w64 = ctx.kernel_variant != "generic-radix2"  # lanes and pipelines exist on the 64-lane kernels only
    assert w64 == (params == LARGE)
    nl, gates, outs = rn.generate(seed, family)
    cn = nl.compile(outs)
    info = cn.info()
    bits, inp = rn.case_inputs(kb, seed, nl.n_inputs)
    B, S = rn.BATCH, kb.p.n + 1
    st = ia.Stats()
    ref = ctx.eval_netlist(cn, inp, st)
    assert ref.shape == (B, len(outs), S)
    assert st.bootstraps == B * info.bootstraps == B * (len(gates) + sum(g[0] == rn.MUX for g in gates))
    assert st.levels == info.sched_levels == info.depth
    if family == "empty":
        assert st.bootstraps == 0 and st.levels == 0 and len(gates) == 0
    # word for word against the oracle, and the bits of the plain wire walk
    for e in rn.compared_with_oracle(params):
        assert np.array_equal(rn.oracle_netlist(kb, cn, inp[e]), ref[e]), e
    assert np.array_equal(kb.dec(ref), np.stack([rn.walk_bits(nl.n_inputs, gates, outs, v) for v in bits]))
    # outputs that name an input, its negation or a constant are that row, in every expression
    for e in range(B):
        for i, row in _expected_passthrough(kb, outs, inp[e]).items():
            assert np.array_equal(ref[e, i], row), (e, i)
    if family == "empty":
        assert all(o < 0 or (o >> 1) < nl.n_inputs for o in outs)  # ... which is all of them here

    has_levels = info.depth > 0
    saved = {k: ctx.get_option(k) for k in OPTIONS}

    def restore():
        ctx.set_chunk(saved["chunk"])
        ctx.force_generic(False)
        for k in OPTIONS[1:]:
            ctx.set_option(k, saved[k])

    def same(batch=B):
        got = ctx.eval_netlist(cn, inp[:batch])
        return got.shape == ref[:batch].shape and np.array_equal(got, ref[:batch])

    try:
        # pieces that end inside levels and inside expressions; one rotation item at a time
        for chunk in (1, 3):
            ctx.set_chunk(chunk)
            assert same(), chunk
        restore()
        # one stream, then level halves on two lanes (no pipelines: a level is halved only when the lanes are not taken)
        ctx.set_option("overlap", 0)
        assert same()
        ctx.set_option("overlap", 1)
        ctx.set_option("pipe_auto", 0)
        ctx.set_option("pipe_min", 1 << 40)
        ctx.set_option("overlap_min", 2)
        lv = ctx.get_option("overlapped_levels")
        assert same()
        # every level of a batch of 8 holds at least 8 rotation items: two pieces of at least 4
        assert (ctx.get_option("overlapped_levels") > lv) == (w64 and has_levels)
        if w64 and has_levels:
            assert ctx.get_option("overlapped_levels") == lv + info.sched_levels
        ctx.set_chunk(3)
        assert same()
        restore()
        # expression-half pipelines, forced on; an odd batch; pieces inside a pipeline's share
        ctx.set_option("pipe_auto", 0)
        ctx.set_option("pipe_min", 1)
        pe = ctx.get_option("pipelined_evals")
        assert same() and same(3)
        assert ctx.get_option("pipelined_evals") == pe + (2 if w64 and has_levels else 0)
        ctx.set_chunk(3)
        assert same() and same(3)
        assert ctx.get_option("pipelined_evals") == pe + (4 if w64 and has_levels else 0)
        restore()
        ctx.set_option("exact_fft", 1)
        assert same()
        restore()
        if params == LARGE:
            ctx.force_generic(True)
            assert same(2)
            restore()
        # batches of one and of none
        assert same(1)
        st0 = ia.Stats()
        none = ctx.eval_netlist(cn, inp[:0], st0)
        assert none.shape == (0, len(outs), S) and st0.bootstraps == 0
    finally:
        restore()
    # schedule independence: the same DAG, every gate a deterministic bootstrap
    with nl.compile(outs, balanced=True) as cb:
        assert np.array_equal(ctx.eval_netlist(cb, inp), ref)
        try:
            ctx.set_chunk(1)
            assert np.array_equal(ctx.eval_netlist(cb, inp), ref)
        finally:
            ctx.set_chunk(saved["chunk"])
    cn.close()


def test_guard_repeat_restages_recycled_input_slots(ia, gpu_ctx):
    """A deep narrow netlist recycles its input slots after the first levels.  When the rounding guard trips, the evaluation
    runs again on the two-limb kernels: the inputs the first attempt overwrote in the store have to be staged again."""
    kb, ctx = gpu_ctx(*LARGE)
    seed, family = next(c for c in rn.corpus(LARGE) if c[1] == "window")
    nl, gates, outs = rn.generate(seed, family)
    cn = nl.compile(outs)
    assert cn.info().n_slots < nl.n_inputs + len(gates) // 2  # slots are reused, the inputs' among them
    # the narrowest level is one rotation item per expression: more expressions than CUs, so that every level's launch takes
    # a one-limb kernel
    batch = ctx.get_option("cus") + 8
    bits = np.random.default_rng([seed, 78]).integers(0, 2, size=(batch, nl.n_inputs)).astype(np.uint8)
    inp = kb.enc(bits, seed + 1)
    ref = ctx.eval_netlist(cn, inp)
    assert np.array_equal(kb.dec(ref), np.stack([rn.walk_bits(nl.n_inputs, gates, outs, v) for v in bits]))
    for e in (0, batch - 1):
        assert np.array_equal(rn.oracle_netlist(kb, cn, inp[e]), ref[e]), e
    _, reruns = ctx.fft_guard()
    ctx.set_option("fft_guard_inject", 1)
    st = ia.Stats()
    again = ctx.eval_netlist(cn, inp, st)
    assert ctx.fft_guard()[1] == reruns + 1
    assert np.array_equal(again, ref) and st.bootstraps == batch * cn.info().bootstraps
    cn.close()


def test_device_entry_with_padded_rows(ia, gpu_ctx):
    import torch
    kb, ctx = gpu_ctx(*LARGE)
    seed, family = next(c for c in rn.corpus(LARGE) if c[1] == "mixed")
    nl, gates, outs = rn.generate(seed, family)
    cn = nl.compile(outs)
    bits, inp = rn.case_inputs(kb, seed, nl.n_inputs)
    B, S, stride = rn.BATCH, kb.p.n + 1, ctx.lwe_stride
    assert stride > S  # there are padding words
    host = ctx.eval_netlist(cn, inp)
    assert np.array_equal(rn.oracle_netlist(kb, cn, inp[0]), host[0])
    assert np.array_equal(kb.dec(host), np.stack([rn.walk_bits(nl.n_inputs, gates, outs, v) for v in bits]))
    rows = np.full((B, nl.n_inputs, stride), 0x5A5A5A5A, dtype=np.int32)  # padding the evaluation must neither use nor pass on
    rows[:, :, :S] = inp
    d_in = torch.from_numpy(rows).cuda()
    d_out = torch.full((B, len(outs), stride), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    auto = ctx.get_option("pipe_auto")
    try:
        ctx.set_option("pipe_auto", 0)
        ctx.prepare_netlist(cn, B)
        n0 = ctx.get_option("staging_allocations")
        ctx.eval_netlist_device(cn, B, d_in.data_ptr(), d_out.data_ptr())
        first = d_out.cpu().numpy().copy()
        d_out.fill_(-1)
        torch.cuda.synchronize()
        ctx.eval_netlist_device(cn, B, d_in.data_ptr(), d_out.data_ptr())
        assert ctx.get_option("staging_allocations") == n0
    finally:
        ctx.set_option("pipe_auto", auto)
    second = d_out.cpu().numpy()
    assert np.array_equal(first[:, :, :S], host) and np.array_equal(second, first)
    assert not first[:, :, S:].any()
    assert np.array_equal(d_in.cpu().numpy(), rows)  # the inputs are the caller's: untouched
    cn.close()
