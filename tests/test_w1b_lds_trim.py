"""-m gpu: k_blind_rotate_w1b with six of its seven second inter-pass twiddles resident in registers and the first BK block of
a row requested inside the forward transform -- word for word against the two-limb kernels (exact_fft = 1) and, on a sample,
the CPU oracle, at n = 630, N = 1024, l = 3.  (A form of the kernel that also carried polynomial 0's unrotated operands from
one step's update to the next step's decomposition measured within noise and is not kept; the cases that pin
what such a change can break -- launch boundaries, skipped steps -- stay.)

What can go wrong, and the smallest shape that shows it:
  gates 1, 3      a partial workgroup of the four-gate build; the three-gate build (wg_gates 3) full and partial
  gates 5         one full workgroup and a partial one
  gates 2 049     forced onto the kernel: a second round of workgroups on a chip that holds 2 048 waves
  slices          whatever a wave keeps across steps is set up once per launch: a rotation in launches of 1, 16, 17 and 64 steps
  amount 0        a skipped step must leave accumulator and kept state alone: as the first step of a launch, in the middle of
                  one, twice in a row, and across a launch boundary; amounts 1, 1023, 1024, 2047 for the wrap and the sign
  guard           the largest rounding distance of a fixed input equals the one the table-form build published for it
                  (tests/golden/w1b_guard.json, recorded by running guard_figures() below on the library of the commit before
                  the resident form): the arithmetic is the same instruction for instruction, so the figure is too -- also
                  with the running maximum kept as a float between steps"""
import json
import os

import numpy as np
import pytest

import crafted_state as CS
from test_param_lattice_gpu import _options

pytestmark = pytest.mark.gpu

W1B, W1B_EVERY = 31, 32          # guard on one rounded coefficient in four / on every one
TWO_LIMB = dict(br_variant=0, exact_fft=1)
ROWS = 2049
SAMPLE = (0, 4, 2048)
SLICES = (1, 16, 17, 64)
CRAFTED_STEPS = (10, 18, 40, -1)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "w1b_guard.json")


def _rows(n, rows, seed):
    return np.random.default_rng(seed).integers(-(1 << 31), 1 << 31, size=(rows, n + 1), dtype=np.int64).astype(np.int32)


def _crafted_rows(n, N):
    """Six rows of random amounts with the cases of the docstring written over them (step: amount)."""
    x = _rows(n, 6, 99)
    plans = [
        {0: 0, 7: 0, 8: 0, 9: 0, 16: 0, 17: 1, 33: 1023, 34: 1024, 35: 2047},     # first step of the launch, middle, consecutive, first of slice 16's second launch
        {0: 1, 1: 0, 15: 0, 16: 0, 17: 0, 18: 2047, 63: 0, 64: 0, 65: 1024},       # consecutive across the boundaries of slices 16, 17 and 64
        {0: 1024, 1: 1024, 2: 0, 3: 1023, 4: 1, 5: 0, 6: 0, 7: 2047, 8: 2047},
        {s: 0 for s in range(0, 40)},                                              # nothing happens for 40 steps, then random amounts
        {s: (0 if s % 2 else 1) for s in range(0, 40)},                            # every other step skipped
        {n - 1: 0, n - 2: 0, n - 3: 1, 0: 2047},                                   # the rotation ends on skipped steps
    ]
    for row, plan in zip(x, plans):
        for step, a in plan.items():
            row[step] = CS.amount_word(a, N)
    return x


@pytest.fixture(scope="module")
def world(ia, O, gpu_ctx):
    """The inputs and every reference, computed once: the two-limb kernels on all rows, the oracle on the sample rows and on
    the crafted rows.  Nothing below writes to them."""
    kb, ctx = gpu_ctx(630, 1024)
    assert (kb.p.n, kb.p.N, kb.p.l) == (630, 1024, 3)
    x, xc = _rows(kb.p.n, ROWS, 630), _crafted_rows(kb.p.n, kb.p.N)
    with _options(ctx, **TWO_LIMB):
        ref = ctx.debug_blind_rotate(x, -1)
        refc = {s: ctx.debug_blind_rotate(xc, s) for s in CRAFTED_STEPS}
    ora = CS.oracle_accumulators(kb.ck, x[list(SAMPLE)], (-1,))[-1]
    orac = CS.oracle_accumulators(kb.ck, xc, CRAFTED_STEPS)
    assert np.array_equal(ref[list(SAMPLE)], ora), "the two-limb kernels differ from the oracle: no reference to test against"
    for s in CRAFTED_STEPS:
        assert np.array_equal(refc[s], orac[s]), "the two-limb kernels differ from the oracle on the crafted rows after %d steps" % s
    for a in (x, xc, ref, ora, *refc.values()):
        a.setflags(write=False)
    return dict(kb=kb, ctx=ctx, x=x, xc=xc, ref=ref, ora=ora, refc=refc)


def _differs(out, ref):
    bad = np.argwhere(out != ref)
    return None if bad.size == 0 else "%d words differ, first at (row, polynomial, coefficient) %s" % (len(bad), tuple(int(v) for v in bad[0]))


@pytest.mark.parametrize("wg", [0, 3, 4])
@pytest.mark.parametrize("gates", [1, 3, 5])
def test_partial_workgroups(world, gates, wg):
    ctx = world["ctx"]
    with _options(ctx, br_variant=W1B, wg_gates=wg):
        assert ctx.kernel_for_launch(gates).startswith("k_blind_rotate_w1b")
        out = ctx.debug_blind_rotate(world["x"][:gates], -1)
    assert _differs(out, world["ref"][:gates]) is None, _differs(out, world["ref"][:gates])
    assert np.array_equal(out[0], world["ora"][0])


def test_second_round_of_workgroups(world):
    ctx = world["ctx"]
    with _options(ctx, br_variant=W1B, wg_gates=4):
        out = ctx.debug_blind_rotate(world["x"], -1)
    assert _differs(out, world["ref"]) is None, _differs(out, world["ref"])
    assert np.array_equal(out[list(SAMPLE)], world["ora"])


@pytest.mark.parametrize("variant", [W1B, W1B_EVERY])
@pytest.mark.parametrize("br_slice", SLICES)
def test_rotation_in_slices(world, br_slice, variant):
    ctx = world["ctx"]
    with _options(ctx, br_variant=variant, br_slice=br_slice):
        out = ctx.debug_blind_rotate(world["x"][:5], -1)
    assert _differs(out, world["ref"][:5]) is None, _differs(out, world["ref"][:5])


@pytest.mark.parametrize("br_slice", SLICES)
def test_skipped_steps_and_wrapping_amounts(world, br_slice):
    ctx = world["ctx"]
    for steps in CRAFTED_STEPS:
        with _options(ctx, br_variant=W1B, br_slice=br_slice):
            out = ctx.debug_blind_rotate(world["xc"], steps)
        d = _differs(out, world["refc"][steps])
        assert d is None, "after %s steps in launches of %d: %s" % ("all" if steps < 0 else steps, br_slice, d)


def guard_figures(ia, kb, x):
    """{variant: largest rounding distance (hex float) a fresh context publishes after rotating x on that build}."""
    out = {}
    for variant in (W1B, W1B_EVERY):
        with ia.Context.from_arrays(kb.p, kb.bk, kb.ksk) as ctx:
            ctx.set_option("br_variant", variant)
            ctx.debug_blind_rotate(x, -1)
            dev, reruns = ctx.fft_guard()
            assert reruns == 0
            out[str(variant)] = float(dev).hex()
    return out


def test_guard_maximum_is_the_table_form_builds(ia, world):
    want = json.load(open(GOLDEN))
    got = guard_figures(ia, world["kb"], world["x"][:5])
    print("w1b guard maxima:", got, "recorded:", want)
    assert got == {k: want[k] for k in got}
