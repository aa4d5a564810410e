"""-m gpu: every kernel family over the parameter sets a key header may carry (Params::supported(), csrc/params.h), bit for
bit against the CPU oracle -- which tests/test_param_lattice_cpu.py pins at the same decompositions -- and, for the key
switch, against the plain numpy statement of it (np_tfhe.np_keyswitch) as well.

Which family a forced option selects is what tests/native/ks_plan_test.cpp states for these very sets; nothing here probes it.
Sweep contexts are opened on keys from make_keys and closed again, so that a few dozen of them do not stay open."""
import contextlib

import numpy as np
import pytest

import np_tfhe
import param_lattice as PL

pytestmark = pytest.mark.gpu
NEVER = 1 << 40


@contextlib.contextmanager
def _options(ctx, **kw):
    """Options set for the block and put back after it, whatever happens inside."""
    old = {k: ctx.get_option(k) for k in kw}
    try:
        for k, v in kw.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            ctx.set_option(k, v)


# ---- key switch ----

def _ks_families(n, t, bb):
    """(label, options) for every key-switch family ks_support() allows the set (csrc/ks_plan.h; the boundaries are those of
    tests/native/ks_plan_test.cpp: a walk kernel needs n <= 1023; gate-batched base 4 with t = 4, 8; sliced and MFMA t = 8)."""
    walk = ((n + 4) // 4 + 63) // 64 <= 4
    base = dict(force_generic=0, ks_mfma_min=NEVER, ks_sliced_min=NEVER, ks_batch_min=NEVER)
    fams = [("generic", dict(base, force_generic=1))]
    if walk:
        fams += [("per-gate, splits %d" % s, dict(base, ks_split_max=s)) for s in (1, 16)]
        if bb == 2 and t in (4, 8):
            fams.append(("batched", dict(base, ks_batch_min=1)))
        if (t, bb) == (8, 2):
            fams += [("sliced, %d gates, slice %d" % (g, sl), dict(base, ks_sliced_min=1, ks_gates=g, ks_slice=sl))
                     for g in (4, 32) for sl in (0, 24)]  # 24: N = 64 in slices of 24, 24 and a ragged 16
    if (t, bb) == (8, 2):
        fams += [("mfma, split %d" % s, dict(base, ks_mfma_min=1, ks_mfma_split=s)) for s in (1, 8)]
    return fams


def _check_keyswitch(ia, kb):
    """debug_keyswitch of 70 rows (66 random + the four edge rows), and of 5 and 1 of them, through every family."""
    p = kb.p
    t, bb, N, n = p.ks_t, p.ks_basebit, p.N, p.n
    u = PL.edge_rows(np.random.default_rng(n + t), N, t, bb, 66)
    ref = np.stack([kb.ck.keyswitch(r) for r in u])
    assert np.array_equal(np_tfhe.np_keyswitch(kb.ksk, t, bb, u), ref)  # the two references agree before the GPU is asked
    for r in (66, 67, 69):  # no row subtracted: (0, b')
        assert not ref[r, :n].any() and ref[r, n] == u[r, N]
    with ia.Context.from_arrays(p, kb.bk, kb.ksk) as ctx:
        assert np.array_equal(ctx.debug_keyswitch(u), ref), "no option set"  # 70 rows: whatever the plan picks unforced
        for label, opts in _ks_families(n, t, bb):
            with _options(ctx, **opts):
                for rows in (slice(0, 70), slice(65, 70), slice(68, 69)):  # 70 (ragged groups, MFMA padding), 5, 1 (every digit base - 1)
                    out = ctx.debug_keyswitch(u[rows])
                    bad = np.argwhere(out != ref[rows])
                    assert bad.size == 0, "%s, rows %s: %d words differ, first at (row, column) %s" % (label, rows, len(bad), bad[0])


@pytest.mark.parametrize("n", [3, 7, 31, 32, 63, 255, 256, 511, 512, 767, 768, 1023, 1024, 1100])
def test_keyswitch_stage_over_n(ia, make_keys, n):
    """Output rows of every width: one to four dwordx4 loads per key row (n = 255 | 256, 511 | 512, 767 | 768), b' in .w with no
    padding column (n % 4 == 3), MFMA coefficient blocks ending on a row (stride % 32 == 0: n = 31, 63, 255 ...), and past the
    walk kernels (n >= 1024: the generic kernel, whose columns beyond 768 were never written before it looped over them)."""
    _check_keyswitch(ia, make_keys(n, 64))


@pytest.mark.parametrize("n", [7, 256])
@pytest.mark.parametrize("t,bb", PL.KS_DECOMPS)
def test_keyswitch_stage_over_decomposition(ia, make_keys, t, bb, n):
    """basebit 1, 3, 4; t x basebit = 31 (rounding offset 1); t = 4 on the gate-batched kernel; a single digit (t = 1)."""
    _check_keyswitch(ia, make_keys(n, 64, ks_t=t, ks_basebit=bb))


def test_keyswitch_stage_with_the_longest_digit_list(ia, make_keys):
    """t = 31 at N = 1024: 131 KB of LDS for the digit list of the generic and per-gate kernels (the dynamic-LDS opt-in)."""
    _check_keyswitch(ia, make_keys(4, 1024, ks_t=31, ks_basebit=1))


# ---- generic blind rotation ----

def _modswitch_edge_rows(kb, rng):
    """LWE samples for the blind rotation: encryptions, an all-zero row (every CMux step skipped), and rows whose coefficients
    sit on the mod-switch edges: rounding up to 2N (wraps to 0), to N (X^N = -1), and to 2N - 1."""
    n, N = kb.p.n, kb.p.N
    half = 1 << (31 - (2 * N).bit_length() + 1)  # half a mod-switch step
    x = np.concatenate([kb.enc(rng.integers(0, 2, size=3), 7), np.zeros((5, n + 1), dtype=np.int32)])
    x[4] = -1                   # + half wraps: 0 everywhere, b included
    x[5] = 0x7FFFFFFF           # rounds up to N
    x[6] = -(half + 1)          # the last value that still rounds to 2N - 1
    x[7] = np.resize(np.array([-1, 0x7FFFFFFF, -(half + 1), -half, half - 1, 12345], dtype=np.int64), n + 1).astype(np.int32)
    bara = [kb.ck.modswitch(r) for r in x]
    assert not bara[4][0].any() and bara[4][1] == 0 and (bara[5][0] == N).all() and (bara[6][0] == 2 * N - 1).all()
    return x


def _check_blind_rotate(ia, kb):
    x = _modswitch_edge_rows(kb, np.random.default_rng(kb.p.n))
    n = kb.p.n
    with ia.Context.from_arrays(kb.p, kb.bk, kb.ksk) as ctx:
        assert ctx.kernel_variant == "generic-radix2"
        for steps in (0, 1, -1):
            acc = ctx.debug_blind_rotate(x, steps)
            for i in range(x.shape[0]):
                bara, barb = kb.ck.modswitch(x[i])
                ref = kb.ck.blind_rotate_init(barb)
                for s in range(n if steps < 0 else min(steps, n)):
                    ref = kb.ck.blind_rotate_step(ref, s, bara[s])
                assert np.array_equal(ref, acc[i]), (n, steps, i)


@pytest.mark.parametrize("N", PL.BR_RINGS)
@pytest.mark.parametrize("l,Bgbit", PL.BR_DECOMPS + [(1, 0)], ids=lambda v: str(v))
def test_generic_blind_rotation_over_the_decomposition(ia, make_keys, l, Bgbit, N):
    """k_blind_rotate_generic where it never ran: l = 1 (rows 2 - 3 of F are outputs only), kpl > 4, N = 16 (fewer points than
    a wave) .. 512, digits of up to 2^26 (Bgbit 0 here = the largest the exactness bound keeps on this ring)."""
    if Bgbit == 0:
        Bgbit = PL.largest_bgbit(N)
    for n in (1, 5, 9):
        _check_blind_rotate(ia, make_keys(n, N, l=l, Bgbit=Bgbit))


@pytest.mark.parametrize("l,Bgbit", PL.BR_DECOMPS_1024)
def test_generic_blind_rotation_on_the_full_ring_without_force(ia, make_keys, l, Bgbit):
    """N = 1024 sets that are not br_supported(): the generic kernel serves them unforced; (4, 8) needs more than 64 KiB of LDS."""
    for n in (1, 5, 9):
        _check_blind_rotate(ia, make_keys(n, 1024, l=l, Bgbit=Bgbit))


# ---- the 64-lane kernels over n ----

def _check_variants(ia, kb, variants, slices=(0,)):
    """37 XOR gates (ragged workgroups) on each forced variant: all equal to the two-limb latency kernel's (variant 7), whose
    first and last gate equal the oracle's."""
    rng = np.random.default_rng(kb.p.n)
    bits = rng.integers(0, 2, size=(2, 37)).astype(np.uint8)
    a, b = kb.enc(bits[0], 71), kb.enc(bits[1], 72)
    with ia.Context.from_arrays(kb.p, kb.bk, kb.ksk) as ctx:
        assert "radix8" in ctx.kernel_variant
        with _options(ctx, br_variant=7):
            ref = ctx.gates(ia.GATE_XOR, a, b)
        for i in (0, 36):
            assert np.array_equal(kb.ck.gate("xor", a[i], b[i]), ref[i]), i
        assert np.array_equal(ctx.gates(ia.GATE_XOR, a, b), ref), "by launch size"
        for sl in slices:
            for v in variants:
                with _options(ctx, br_variant=v, br_slice=sl):
                    assert np.array_equal(ctx.gates(ia.GATE_XOR, a, b), ref), (v, sl)
        if kb.p.l == 3:
            dev, reruns = ctx.fft_guard()
            assert 0 < dev < 1 / 16 and reruns == 0


@pytest.mark.parametrize("n", [7, 9, 63, 65, 67, 129])
def test_64_lane_kernels_over_n(ia, make_keys, n):
    """The `chosen` rows of kBrVariants, two-limb (0, 7, 9, 12) and one-limb (31, 36, 38, 43), at LWE dimensions that are no
    multiple of 8 (the padding of br_bara_stride) and just past a 64-step reload of the rotation amounts (65, 67, 129)."""
    _check_variants(ia, make_keys(n, 1024), (0, 7, 9, 12, 31, 36, 38, 43), slices=(0, 1, 64, 67) if n == 67 else (0,))


def test_64_lane_two_limb_kernels_on_the_old_parameter_set(ia, make_keys):
    """l = 2 / Bgbit = 10 at n = 9 on every two-limb variant (test_old_libtfhe_parameter_set_on_fast_kernel forces 31 and 36)."""
    _check_variants(ia, make_keys(9, 1024, l=2, Bgbit=10, lwe_alpha_min=2.44e-5, tlwe_alpha_min=7.18e-9), (0, 7, 9, 12))


# ---- whole gates ----

@pytest.mark.parametrize("pset", PL.GATE_SETS, ids=lambda s: "n%d-N%d-l%d-Bg%d-t%d-bb%d" % s)
def test_whole_gates_at_unusual_sets(ia, make_keys, pset):
    """AND, XOR and bootsMUX, sample for sample against the oracle (pinned at these sets on the CPU): an unusual (l, Bgbit)
    with an unusual (ks_t, ks_basebit), n % 4 == 3."""
    n, N, l, Bgbit, t, bb = pset
    kb = make_keys(n, N, l=l, Bgbit=Bgbit, ks_t=t, ks_basebit=bb)
    bits = np.random.default_rng(N + l).integers(0, 2, size=(3, 9)).astype(np.uint8)
    a, b, c = (kb.enc(bits[i], 81 + i) for i in range(3))
    with ia.Context.from_arrays(kb.p, kb.bk, kb.ksk) as ctx:
        for name, gt in (("and", ia.GATE_AND), ("xor", ia.GATE_XOR)):
            out = ctx.gates(gt, a, b)
            for i in range(9):
                assert np.array_equal(kb.ck.gate(name, a[i], b[i]), out[i]), (name, i)
        out = ctx.mux(a, b, c)
        for i in range(9):
            assert np.array_equal(kb.ck.mux(a[i], b[i], c[i]), out[i]), ("mux", i)


# ---- refusals (host-side: nothing here launches anything) ----

def _raw_arrays(p):
    return np.zeros(p.bk_count, dtype=np.int32), np.zeros(p.ksk_count, dtype=np.int32)


@pytest.mark.parametrize("N,l,Bgbit,t,bb", PL.REFUSED_SETS)
def test_sets_outside_supported_are_refused_at_context_creation(ia, N, l, Bgbit, t, bb):
    p = ia.default_params().copy(n=3, N=N, l=l, Bgbit=Bgbit, ks_t=t, ks_basebit=bb)
    with pytest.raises(ia.IeacheError, match="unsupported TFHE parameter set"):
        ia.Context.from_arrays(p, *_raw_arrays(p))


def test_sets_past_the_lds_of_a_cu_are_refused_at_context_creation(ia):
    """l = 10 / Bgbit = 3 at N = 1024 is inside supported() but the generic blind rotation would need 20 x 512 double2 = 160 KiB
    of LDS for its digit spectra alone.  (The key switch's twin of this refusal cannot be reached from a supported set: its list
    is N x t words, 131 088 bytes at most -- tests/native/ks_plan_test.cpp -- and that set runs above.)"""
    p = ia.default_params().copy(n=3, N=1024, l=10, Bgbit=3)
    with pytest.raises(ia.IeacheError, match="exceeds the 160 KiB LDS"):
        ia.Context.from_arrays(p, *_raw_arrays(p))
    p = ia.default_params().copy(n=3, N=512, l=10, Bgbit=3)  # the same decomposition one ring down fits (80 KiB) and is accepted
    with ia.Context.from_arrays(p, *_raw_arrays(p)) as ctx:
        assert ctx.kernel_variant == "generic-radix2"
