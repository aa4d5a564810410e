"""Device groups on the card (include/ieache.h section 2b): one, two and three contexts on device 0 -- and two distinct devices
where the machine has them -- driven from concurrent host threads by one call.  Every result is compared WORD FOR WORD with
the single context's: a member's slice goes through the same circuit and kernels, so no tolerance applies.  Keys: (4, 1024),
the 64-lane kernel family with four CMux steps per rotation; flat calls and netlists once more at (5, 64), the any-parameter
kernels."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ONE_CARD = [(0,), (0, 0), (0, 0, 0)]


@pytest.fixture(scope="module")
def groups(ia, gpu_ctx):
    """(n, N, devices) -> (keys, the reference Context, a Group on those devices); groups are kept for the module."""
    made = {}

    def make(n, N, devices):
        kb, ctx = gpu_ctx(n, N)
        if any(d >= ia.device_count() for d in devices):
            pytest.skip("devices %s need %d GPUs" % (devices, max(devices) + 1))
        if (n, N, devices) not in made:
            made[(n, N, devices)] = ia.Group.from_arrays(kb.p, kb.bk, kb.ksk, devices)
        return kb, ctx, made[(n, N, devices)]

    yield make
    for g in made.values():
        g.close()


def add16_inputs(kb, vals, seed):
    from ieache_amd.tools import int_to_bits
    inb = np.zeros((len(vals), 16 + 16 + 32), dtype=np.uint8)  # A, B, A's carry word (zero)
    for e, (a, b) in enumerate(vals):
        inb[e, :16], inb[e, 16:32] = int_to_bits(a, 16), int_to_bits(b, 16)
    return kb.enc(inb, seed)


@pytest.fixture(scope="module")
def add16(ia, gpu_ctx):
    """Case 1's batch, computed once: 37 sixteen-bit additions, their inputs, and what the single context gives."""
    kb, ctx = gpu_ctx(4, 1024)
    rng = np.random.default_rng(37)
    vals = [(int(a), int(b)) for a, b in rng.integers(0, 1 << 16, size=(37, 2))]
    vals[7], vals[36] = (0xFFFF, 1), (0x8000, 0x8000)  # the carry through every bit; process.c's operands close the batch
    inp = add16_inputs(kb, vals, 41)
    st = ia.Stats()
    want = ctx.eval_batch(ia.CIRC_ADD, 16, inp, st)
    want.setflags(write=False)
    return vals, inp, want, st.bootstraps


@pytest.mark.parametrize("devices", ONE_CARD + [(0, 1)])
def test_eval_batch_ragged_equals_the_context(ia, groups, add16, devices):
    from ieache_amd.tools import bits_to_int
    kb, ctx, g = groups(4, 1024, devices)
    vals, inp, want, bootstraps = add16
    assert len(g) == len(devices) and g.devices == devices
    stats = []
    out = g.eval_batch(ia.CIRC_ADD, 16, inp, stats=stats)
    assert np.array_equal(out, want)
    assert len(stats) == len(g) and sum(s.bootstraps for s in stats) == bootstraps
    assert [s.bootstraps * 37 // bootstraps for s in stats] == {1: [37], 2: [19, 18], 3: [13, 12, 12]}[len(g)]  # contiguous, the first parts longer
    for e, d in enumerate(kb.dec(out)):
        assert bits_to_int(d) == (vals[e][0] + vals[e][1]) & 0xFFFF, e
    # the oracle's add() replay: the first expression of a slice (19 opens member 1's of two, 13 member 1's of three), the last
    # of the batch, and the carry through every bit
    for e in (19, 13, 36, 7):
        s, _ = kb.ck.add(inp[e, :16], inp[e, 16:32], inp[e, 32:33], 16)
        assert np.array_equal(s, out[e]), e


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)])
def test_mul32_on_members_that_share_a_card(ia, groups, devices):
    from ieache_amd.tools import bits_to_int, int_to_bits
    kb, ctx, g = groups(4, 1024, devices)
    vals = [(0xFFFFFFFF, 0xFFFFFFFF), (0x12345678, 0x9ABCDEF0), (3, 5)]
    info = ia.circuit_info(ia.CIRC_MUL, 32)
    inb = np.zeros((3, info.n_inputs), dtype=np.uint8)
    for e, (a, b) in enumerate(vals):
        inb[e, :32], inb[e, 32:64] = int_to_bits(a, 32), int_to_bits(b, 32)
    inp = kb.enc(inb, 43)
    want = ctx.eval_batch(ia.CIRC_MUL, 32, inp)
    g.prepare(ia.CIRC_MUL, 32, 3)
    out = g.eval_batch(ia.CIRC_MUL, 32, inp)
    assert np.array_equal(out, want)
    assert [bits_to_int(d) for d in kb.dec(out)] == [a * b for a, b in vals]


def test_fewer_expressions_than_members(ia, groups, add16):
    kb, ctx, g = groups(4, 1024, (0, 0, 0))
    vals, inp, want, _ = add16
    st, stats = ia.Stats(), []
    assert np.array_equal(ctx.eval_batch(ia.CIRC_ADD, 16, inp[:2], st), want[:2])
    out = g.eval_batch(ia.CIRC_ADD, 16, inp[:2], stats=stats)
    assert np.array_equal(out, want[:2])
    assert len(stats) == 3 and bytes(stats[2]) == bytes(ia.Stats())  # all zero: no rows, no call
    assert stats[0].bootstraps + stats[1].bootstraps == st.bootstraps and stats[0].bootstraps == stats[1].bootstraps > 0
    # and none at all: member 0 alone makes the (empty) call
    empty = g.eval_batch(ia.CIRC_ADD, 16, inp[:0], stats=stats)
    assert empty.shape == (0, 16, kb.p.n + 1) and all(bytes(s) == bytes(ia.Stats()) for s in stats)


def mux_netlist(ia):
    nl = ia.Netlist(3)
    a, b, c = nl.input(0), nl.input(1), nl.input(2)
    x = nl.XNOR(a, ia.NOT(b))
    m = nl.MUX(x, b, ia.NOT(c))
    return nl.compile([x, m, nl.ORYN(m, a), nl.MAJ3(a, m, c)])


@pytest.mark.parametrize("n,N,devices", [(4, 1024, (0, 0)), (4, 1024, (0, 0, 0)), (5, 64, (0, 0, 0))])
def test_one_compiled_netlist_shared_by_all_members(ia, groups, n, N, devices):
    from ieache_amd import netlists
    kb, ctx, g = groups(n, N, devices)
    rng = np.random.default_rng(5)
    for cn in (netlists.adder_fa(4), mux_netlist(ia)):
        info = cn.info()
        bits = rng.integers(0, 2, size=(5, info.n_inputs)).astype(np.uint8)
        inp = kb.enc(bits, 47)
        want = ctx.eval_netlist(cn, inp)
        assert np.array_equal(kb.dec(want), np.stack([cn.simulate(b) for b in bits]))
        g.prepare_netlist(cn, 5)
        stats = []
        first = g.eval_netlist(cn, inp, stats=stats)
        again = g.eval_netlist(cn, inp)
        assert np.array_equal(first, want) and np.array_equal(again, first)
        assert sum(s.bootstraps for s in stats) == 5 * info.bootstraps and all(s.bootstraps for s in stats)
        cn.close()


@pytest.mark.parametrize("n,N,devices", [(4, 1024, (0, 0)), (4, 1024, (0, 0, 0)), (5, 64, (0, 0))])
def test_the_five_flat_calls_at_counts_that_do_not_divide(ia, groups, n, N, devices):
    from ieache_amd import tools
    kb, ctx, g = groups(n, N, devices)
    p = kb.p
    rng = np.random.default_rng(n)
    bits = rng.integers(0, 2, size=(3, 7)).astype(np.uint8)
    a, b, c = (kb.enc(bits[i], 51 + i) for i in range(3))
    for t in (ia.GATE_AND, ia.GATE_XOR):
        stats = []
        assert np.array_equal(g.gates(t, a, b, stats=stats), ctx.gates(t, a, b)), t
        assert [s.bootstraps for s in stats] == ([4, 3] if len(g) == 2 else [3, 2, 2])
    assert np.array_equal(kb.dec(g.gates(ia.GATE_XOR, a, b)), bits[0] ^ bits[1])
    assert np.array_equal(g.gates3(ia.GATE_MAJ3, a, b, c), ctx.gates3(ia.GATE_MAJ3, a, b, c))
    assert np.array_equal(g.mux(a[:5], b[:5], c[:5]), ctx.mux(a[:5], b[:5], c[:5]))
    # two test polynomials, taken in an order that no slice start repeats: a member that read poly_of from row 0 instead of
    # its own first row (rows 4 .. 6 of two members; 3 .. 4 and 5 .. 6 of three) would take other polynomials
    tv = np.stack([np.full(p.N, 1 << 29, dtype=np.int32),
                   (np.arange(1, p.N + 1, dtype=np.int64) * 0x01234567 & 0xFFFFFFFF).astype(np.uint32).view(np.int32)])
    of = [0, 1, 1, 1, 0, 1, 0]
    want = ctx.pbs(a, tv, of)
    assert not np.array_equal(want, ctx.pbs(a, tv, of[1:] + [1]))  # the indices matter
    assert np.array_equal(g.pbs(a, tv, of), want)
    extracted = ctx.pbs(a, tv, of, keyswitch=False)
    assert extracted.shape == (7, p.N + 1) and np.array_equal(g.pbs(a, tv, of, keyswitch=False), extracted)
    # two factors and a bias; output rows [count][n_factors]: a member's slice starts at row first x n_factors
    factors = np.stack([np.eye(1, p.N, 0, dtype=np.int32)[0], tools.lut_factor_poly(p, [0, 1, 0, 1])])
    bias = np.array([0, -(1 << 29)], dtype=np.int64).astype(np.int32)
    want = ctx.pbs_multi(a[:5], tv, factors, of[:5], bias)
    stats = []
    assert np.array_equal(g.pbs_multi(a[:5], tv, factors, of[:5], bias, stats=stats), want)
    assert sum(s.bootstraps for s in stats) == 5
    assert np.array_equal(g.pbs_multi(a[:5], tv, factors, of[:5], bias, keyswitch=False), ctx.pbs_multi(a[:5], tv, factors, of[:5], bias, keyswitch=False))


def test_options_reach_every_member_or_none(ia, groups, add16):
    vals, inp, want, _ = add16
    _, _, alone = groups(4, 1024, (0,))
    kb, ctx, g = groups(4, 1024, (0, 0))
    # members that share a card leave the rotation of roles alone; a member with the card to itself keeps it
    assert [c.get_option("br_mix") for c in g.contexts] == [0, 0] and alone.contexts[0].get_option("br_mix") == 1
    before = [{o: c.get_option(o) for o in ("exact_fft", "chunk", "br_mix", "fold_constants")} for c in g.contexts]
    try:
        g.set_option("exact_fft", 1)
        assert [c.get_option("exact_fft") for c in g.contexts] == [1, 1]
        assert np.array_equal(g.eval_batch(ia.CIRC_ADD, 16, inp), want)  # the two-limb kernels give the same bits
        g.set_option("exact_fft", 0)
        g.set_option("br_mix", 1)  # the rule may be overridden
        assert [c.get_option("br_mix") for c in g.contexts] == [1, 1]
        g.set_option("br_mix", 0)
        # a value the row refuses raises and changes no member; so does a name no table has
        g.contexts[1].set_option("chunk", 4096)
        for name, value in (("chunk", -1), ("chunk", 0), ("no_such_option", 1), ("cus", 1)):
            with pytest.raises(ia.IeacheError) as e:
                g.set_option(name, value)
            assert e.value.code == -22
            assert [c.get_option("chunk") for c in g.contexts] == [before[0]["chunk"], 4096]
        g.set_option("chunk", 7)
        assert [c.get_option("chunk") for c in g.contexts] == [7, 7]
        assert np.array_equal(g.eval_batch(ia.CIRC_ADD, 16, inp[:5]), want[:5])
    finally:
        for c, old in zip(g.contexts, before):
            for name, value in old.items():
                c.set_option(name, value)
    assert [{o: c.get_option(o) for o in before[0]} for c in g.contexts] == before


def test_a_failed_call_leaves_the_group_usable(ia, groups, add16):
    vals, inp, want, _ = add16
    kb, ctx, g = groups(4, 1024, (0, 0))
    L = ia.lib()
    i32p = C.POINTER(C.c_int32)
    out = np.zeros_like(want)
    # an argument error is found before any thread starts, and reads as the context form's
    assert L.ieache_group_eval_batch(g.h, 999, 16, 37, inp.ctypes.data_as(i32p), out.ctypes.data_as(i32p), None) == -22
    assert L.ieache_last_error() == b"unsupported circuit kind/bits"
    assert np.array_equal(g.eval_batch(ia.CIRC_ADD, 16, inp), want)
    a = kb.enc(np.ones(7, dtype=np.uint8), 61)
    tv = np.full((2, kb.p.N), 1 << 29, dtype=np.int32)
    bad = [0, 1, 0, 1, 0, 9, 0]  # row 5 is row 1 of member 1's slice (rows 4 .. 6)
    with pytest.raises(ia.IeacheError) as e:
        g.pbs(a, tv, bad)
    assert e.value.code == -22 and "pbs: poly_of[5] = 9" in str(e.value) and "member" not in str(e.value)
    # The same error raised INSIDE a member, on a thread that is not the caller's: with the shared check switched off (a test
    # hook) member 1's own call finds the index, at its own row number, while member 0 evaluates its rows; code and message
    # arrive on the calling thread.  A host-side argument check: nothing reaches the GPU from the failing member.
    g.set_option("precheck", 0)
    try:
        with pytest.raises(ia.IeacheError) as e:
            g.pbs(a, tv, bad)
        assert e.value.code == -22 and "member 1 (device 0): pbs: poly_of[1] = 9" in str(e.value)
        # both members fail: the lowest-numbered one is reported
        with pytest.raises(ia.IeacheError) as e:
            g.pbs(a, tv[:0].reshape(0, kb.p.N), None)
        assert e.value.code == -22 and "member 0 (device 0): pbs: n_polys must be at least 1" in str(e.value)
    finally:
        g.set_option("precheck", 1)
    assert np.array_equal(g.pbs(a, tv, bad[:5] + [1, 0]), ctx.pbs(a, tv, bad[:5] + [1, 0]))
    assert np.array_equal(g.eval_batch(ia.CIRC_ADD, 16, inp), want)


def test_lifetime_of_groups_and_their_borrowed_contexts(ia, gpu_ctx, add16):
    kb, ctx = gpu_ctx(4, 1024)
    vals, inp, want, _ = add16
    for _ in range(2):
        g = ia.Group.from_arrays(kb.p, kb.bk, kb.ksk, (0, 0, 0))
        views = g.contexts
        assert len(views) == 3 and all(v.h for v in views) and len({v.h for v in views}) == 3
        assert np.array_equal(g.eval_batch(ia.CIRC_ADD, 16, inp[:4]), want[:4])
        views[1].close()  # a borrowed view forgets its handle; the member lives on in the group
        assert np.array_equal(g.eval_batch(ia.CIRC_ADD, 16, inp[:4]), want[:4])
        g.close()
        assert g.h is None and all(v.h is None for v in views)
        g.close()  # closing twice, and the views' own finalisers, destroy nothing a second time
        del views, g
    with ia.Group.from_arrays(kb.p, kb.bk, kb.ksk, (0, 0, 0)) as g:
        assert np.array_equal(g.eval_batch(ia.CIRC_ADD, 16, inp[:7]), want[:7])
        assert [c.get_option("br_mix") for c in g.contexts] == [0, 0, 0]
    assert np.array_equal(ctx.eval_batch(ia.CIRC_ADD, 16, inp[:3]), want[:3])  # the single context never noticed
