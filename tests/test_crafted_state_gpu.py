"""-m gpu: every blind-rotation and key-switch kernel at its arithmetic extremes, word for word against the CPU oracle.

The inputs are the constructions of tests/crafted_state.py, each proved on the CPU by tests/test_crafted_state_cpu.py: sums
of 2^49.58 on the one-limb kernels (where the rounding guard has to trip on the kernel's own arithmetic and the call repeat
itself), 2^52 at the old parameter set, 2^46 per limb on the any-parameter kernel at the edge of Params::br_exact(),
accumulator words at the int32 ends, every rotation amount at which the byte-offset arithmetic of the rotated decomposition
changes a high bit, and key-switch keys whose int8 limb split carries through every byte.

Every assertion is equality with the oracle; the guard's counters are recorded (printed, `pytest -s` / `-rP`, as
"crafted-state: ..." lines: profiles/crafted_state.txt), not asserted -- a guarded kernel has to return the oracle's words
whether or not it repeated itself.  The one exception is stated where it stands: on the first worst-alignment input some
kernel that watches every coefficient has to count a repeat, or the input is not the one the CPU file described."""
import functools

import numpy as np
import pytest

import crafted_state as CS
import np_tfhe
import param_lattice as PL
from test_param_lattice_gpu import _ks_families, _modswitch_edge_rows, _options

pytestmark = pytest.mark.gpu

STEPS = (0, 1, 2, -1)
TWO_LIMB = [("variant %d" % v, dict(br_variant=v)) for v in (7, 9, 12)] + [("variant 0, exact_fft", dict(br_variant=0, exact_fft=1))]
ONE_LIMB_VARIANTS = (24, 31, 32, 36, 37, 38, 39, 43, 44)
EVERY_COEFFICIENT = (32, 37, 39, 44)   # the guard on every rounded coefficient
UNGUARDED = 35                          # k_blind_rotate_w1b without guard arithmetic


def _first_difference(out, ref):
    bad = np.argwhere(out != ref)
    if bad.size == 0:
        return None
    at = tuple(int(v) for v in bad[0])
    return "%d words differ, first at (row, polynomial, coefficient) %s: %d, oracle %d" % (len(bad), at, out[at], ref[at])


def _run(ctx, x, ref, name, label, opts):
    """debug_blind_rotate after 0, 1, 2 and all steps under `opts` -> (first difference or None, guard pair, wrong words)."""
    with _options(ctx, **opts):
        before = ctx.fft_guard()
        outs = {s: ctx.debug_blind_rotate(x, s) for s in STEPS}
        after = ctx.fft_guard()
    wrong = sum(int((outs[s] != ref[s]).sum()) for s in STEPS)
    pair = (after[0], after[1] - before[1])
    print("crafted-state: %s | %s | largest distance so far %.4g | reruns added %d | wrong words %d" % (name, label, pair[0], pair[1], wrong))
    for s in STEPS:
        d = _first_difference(outs[s], ref[s])
        if d:
            return "%s, %s, after %s steps: %s; guard (largest distance, reruns added) = %s" % (name, label, "all" if s < 0 else s, d, pair), pair, wrong
    return None, pair, wrong


def _check_64_lane(ia, O, name, p, bk, ksk, x, runs, unguarded=True):
    """Every run of `runs` (label, options) equals the oracle; the unguarded one-limb kernel is run and counted, not asserted.
    -> {label: guard pair}."""
    ck, ctx = CS.open_pair(ia, O, p, bk, ksk)
    with ctx:
        assert "radix8" in ctx.kernel_variant
        ref = CS.oracle_accumulators(ck, x, STEPS)
        pairs, failures = {}, []
        for label, opts in runs:
            failed, pairs[label], _ = _run(ctx, x, ref, name, label, opts)
            if failed:
                failures.append(failed)
        if unguarded:
            _, _, wrong = _run(ctx, x, ref, name, "variant %d (no guard; counted only)" % UNGUARDED, dict(br_variant=UNGUARDED))
            pairs["unguarded wrong words"] = wrong
        assert not failures, "\n".join(failures)
    return pairs


def _one_limb_runs(slices=(0,)):
    runs = []
    for sl in slices:
        tag = "" if sl == 0 else ", br_slice %d" % sl
        runs += [(label + tag, dict(opts, br_slice=sl)) for label, opts in TWO_LIMB]
        runs += [("variant %d%s" % (v, tag), dict(br_variant=v, br_slice=sl)) for v in ONE_LIMB_VARIANTS]
        runs.append(("by launch size" + tag, dict(br_slice=sl)))
    return runs


# ---- 64-lane kernels, l = 3 / Bgbit = 7 ----

@pytest.mark.parametrize("cid", [c for c, _ in CS.steered_cases(None, 3, 7, 1024)])
def test_64_lane_kernels_at_extreme_sums(ia, O, cid):
    """Cases 1 and 2: sums of up to 2^49.58 (worst0), where a double's grid is 1/8 wide and the one-limb transform alone is
    not to be trusted (worst4: the build without a guard returns wrong words); the guarded kernels must notice and the call
    return the oracle's words all the same."""
    case = dict(CS.steered_cases(ia, 3, 7, 1024))[cid]()
    runs = _one_limb_runs() + [("any-parameter kernel", dict(force_generic=1))]
    pairs = _check_64_lane(ia, O, case.name, case.p, case.bk, case.ksk, case.x, runs)
    if cid == "worst0":
        assert any(pairs["variant %d" % v][1] > 0 for v in EVERY_COEFFICIENT), \
            "no kernel that watches every coefficient repeated itself on sums of 2^49.58: %s" % pairs


def test_64_lane_kernels_on_accumulator_words_at_the_int32_ends(ia, O, make_keys):
    """Case 3: 0x80000000, 0x7FFFFFC0, 0 and -64 in the accumulator, then steps by 1, 2N - 1 and N against a generated key."""
    case = CS.int32_ends(ia, make_keys(4, 1024).bk)
    _check_64_lane(ia, O, case.name, case.p, case.bk, case.ksk, case.x, _one_limb_runs())


@functools.lru_cache(maxsize=None)
def _boundary_rows(kb):
    x = np.concatenate([CS.boundary_amount_rows(), _modswitch_edge_rows(kb, np.random.default_rng(16))])
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("br_slice", [0, 1, 5])
def test_64_lane_kernels_at_boundary_rotation_amounts(ia, O, make_keys, br_slice):
    """Case 4: amounts 1, 63 .. 65, 511 .. 513, 1023 .. 1025, 1535, 1536, 2047 and 0 at every step index, on every kernel, as
    the first, the last and the only step of a launch (slices of 5 and 1; 0: the kernel's own slice)."""
    kb = make_keys(16, 1024)
    runs = _one_limb_runs((br_slice,))
    if br_slice == 0:
        runs.append(("variant 7, br_slice 4096", dict(br_variant=7, br_slice=4096)))
    _check_64_lane(ia, O, "boundary amounts", kb.p, kb.bk, kb.ksk, _boundary_rows(kb), runs, unguarded=br_slice == 0)


# ---- the old set: l = 2 / Bgbit = 10 ----

@pytest.mark.parametrize("cid", [c for c, _ in CS.steered_cases(None, 2, 10, 1024)])
def test_old_parameter_set_at_extreme_sums(ia, O, cid):
    """Sums of up to 2^52, past the 2^51 where adding 1.5 x 2^52 stops rounding to the nearest integer: the default path
    (two-limb) is exact by construction; the forced one-limb kernels have to trip their guard and repeat."""
    case = dict(CS.steered_cases(ia, 2, 10, 1024))[cid]()
    runs = [("by launch size", {}), ("variant 31", dict(br_variant=31)), ("variant 36", dict(br_variant=36))]
    _check_64_lane(ia, O, case.name, case.p, case.bk, case.ksk, case.x, runs)


# ---- k_blind_rotate_generic at the edge of br_exact() ----

def _generic_ids():
    return [pytest.param(l, B, N, cid, id="l%d-Bg%d-N%d-%s" % (l, B, N, cid)) for l, B, N in CS.generic_edge_sets()
            for cid, _ in CS.steered_cases(None, l, B, N)]


@pytest.mark.parametrize("l,Bgbit,N,cid", _generic_ids())
def test_generic_kernel_at_the_edge_of_the_exactness_bound(ia, O, l, Bgbit, N, cid):
    """2l x N x 2^Bgbit = 2^32 with every term of one sign and both limbs at +-2^15: the kernel has no guard, so equality with
    the oracle is the whole test.  Forced, and as the plan picks it unforced (none of these sets is br_supported())."""
    case = dict(CS.steered_cases(ia, l, Bgbit, N))[cid]()
    ck, ctx = CS.open_pair(ia, O, case.p, case.bk, case.ksk)
    with ctx:
        assert ctx.kernel_variant == "generic-radix2"
        ref = CS.oracle_accumulators(ck, case.x, STEPS)
        for label, opts in (("no option", {}), ("force_generic", dict(force_generic=1))):
            with _options(ctx, **opts):
                for s in STEPS:
                    d = _first_difference(ctx.debug_blind_rotate(case.x, s), ref[s])
                    assert d is None, "%s, %s, after %s steps: %s" % (case.name, label, "all" if s < 0 else s, d)


# ---- key switch on crafted keys ----

@pytest.mark.parametrize("n,t,bb", [(7, 8, 2), (256, 8, 2), (7, 4, 2), (256, 4, 2), (7, 7, 4)])
def test_keyswitch_families_on_crafted_keys(ia, O, n, t, bb):
    """Key words whose four balanced int8 limbs carry through every byte (0x7F7F7F7F, 0x80808080, 0x7FFFFF80 ...), constant
    and varied row by row, d = 0 rows included, against inputs with every digit at base - 1: every family, 70 / 5 / 1 rows."""
    N = 64
    p = ia.default_params().copy(n=n, N=N, ks_t=t, ks_basebit=bb)
    u = PL.edge_rows(np.random.default_rng(n + t), N, t, bb, 66)
    bk = np.zeros(p.bk_count, dtype=np.int32)
    for name, ksk in CS.ks_crafted_keys(n, N, t, bb):
        ck, ctx = CS.open_pair(ia, O, p, bk, ksk)
        with ctx:
            ref = np.stack([ck.keyswitch(r) for r in u])
            assert np.array_equal(np_tfhe.np_keyswitch(ksk, t, bb, u), ref), name  # the two references agree before the GPU is asked
            assert np.array_equal(ctx.debug_keyswitch(u), ref), "key %s, no option set" % name
            for label, opts in _ks_families(n, t, bb):
                with _options(ctx, **opts):
                    for rows in (slice(0, 70), slice(65, 70), slice(68, 69)):
                        bad = np.argwhere(ctx.debug_keyswitch(u[rows]) != ref[rows])
                        assert bad.size == 0, "key %s, %s, rows %s: %d words differ, first at (row, column) %s" % (
                            name, label, rows, len(bad), bad[0])
