"""-m gpu: k_blind_rotate_w1b with its forward transforms in the exchange form (csrc/fft512.h, XLANE = 2: lane bit 3 exchanged
at one DPP move per dword) against the same kernel built with the v_cndmask form (ieache_debug_forward_path(1)) and against the
two-limb kernel k_blind_rotate_x1, accumulators word for word, at n = 630, N = 1024, l = 3.

Shapes: one 16-step slice of 8 gates (two whole workgroups of the four-gate build) and one of 3 gates, on the three-per-workgroup
build and as a short workgroup of the four-gate build.  Inputs are random gate inputs with the amounts 0 (a skipped step: as the
first step, in the middle, twice in a row), 1, 1023, 1024 and 2047 (the negacyclic sign and the wrap) written over some steps."""
import numpy as np
import pytest

import crafted_state as CS
from test_param_lattice_gpu import _options

pytestmark = pytest.mark.gpu

W1B, X1 = 31, 9
STEPS = 16


def _rows(n, N):
    x = np.random.default_rng(950).integers(-(1 << 31), 1 << 31, size=(8, n + 1), dtype=np.int64).astype(np.int32)
    plans = [
        {0: 0, 5: 0, 6: 0, 9: 1, 10: 1023, 11: 1024, 12: 2047},
        {0: 2047, 1: 1024, 2: 0, 3: 1023, 4: 1, 15: 0},
        {s: (0 if s % 2 else 1) for s in range(STEPS)},
        {0: 1, 1: 1, 14: 1024, 15: 2047},
        {},
        {7: 0, 8: 1023},
        {3: 1024, 4: 1024, 5: 2047, 6: 2047},
        {s: 0 for s in range(STEPS - 1)},
    ]
    for row, plan in zip(x, plans):
        for step, a in plan.items():
            row[step] = CS.amount_word(a, N)
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def world(gpu_ctx):
    kb, ctx = gpu_ctx(630, 1024)
    assert (kb.p.n, kb.p.N, kb.p.l) == (630, 1024, 3)
    x = _rows(kb.p.n, kb.p.N)
    with _options(ctx, br_variant=X1, br_slice=STEPS):
        assert ctx.kernel_for_launch(8).startswith("k_blind_rotate_x1")
        two_limb = ctx.debug_blind_rotate(x, STEPS)
    two_limb.setflags(write=False)
    return dict(ctx=ctx, x=x, two_limb=two_limb)


def _differs(out, ref):
    bad = np.argwhere(out != ref)
    return None if bad.size == 0 else "%d words differ, first at (row, polynomial, coefficient) %s" % (len(bad), tuple(int(v) for v in bad[0]))


@pytest.mark.parametrize("gates, wg", [(8, 4), (3, 3), (3, 4)])
def test_exchange_form_gives_the_cndmask_forms_words(ia, world, gates, wg):
    ctx, x = world["ctx"], world["x"][:gates]
    out = {}
    try:
        for path in (2, 1):
            ia.debug_forward_path(path)
            with _options(ctx, br_variant=W1B, br_slice=STEPS, wg_gates=wg):
                assert ctx.kernel_for_launch(gates).startswith("k_blind_rotate_w1b")
                out[path] = ctx.debug_blind_rotate(x, STEPS)
    finally:
        ia.debug_forward_path(2)  # the default
    d = _differs(out[2], out[1])
    assert d is None, "exchange form against the v_cndmask form: " + d
    d = _differs(out[2], world["two_limb"][:gates])
    assert d is None, "exchange form against k_blind_rotate_x1: " + d
