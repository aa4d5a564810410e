"""The 512-point transform of the N = 1024 kernels, its twiddle table and the prepared key spectra, as they run on the card,
against the extended-precision reference of tests/fft_reference.py (proved in tests/test_fft_reference_cpu.py).

Every word-for-word test of the suite sees this code after rounding; here the doubles are read back before it, through the
probe of csrc/fft_probe.h (Context.debug_twiddles / debug_fft512 / debug_spectrum), so that a twiddle off at the 2^-40 level,
a cheaper sincospi or a consistent but wrong permutation fails here while every rounded word is still right.

The bounds.  Figures measured on an MI355X are recorded, per form and input, in profiles/fft_probe.txt (this file's own
output under pytest -s); the constants below follow from them by rule:
  TWIDDLE_UNITS   the next whole unit of 2^-53 above the largest error of a table entry against mpmath (measured: 0.661); at
                  most 4, the OpenCL full-profile limit for sinpi / cospi (an assumption: ROCm's own statement is not at hand)
  MARGIN_*        (relative L2, largest single error): kernel error over the numpy double model's error on the same input
                  (tests/test_rounding_model_cpu.py's transform), per group of measurements the smallest power of two that
                  leaves a factor 1.5 over the largest ratio measured in the group; at most 4 -- beyond that the kernel would
                  not be in the model's precision class.  The margin is there because the two
                  factorisations round differently, not to hide drift.
  impulse bound   derived, not measured: impulse_bound_units()"""
import ctypes as C

import numpy as np
import pytest

import crafted_state as CS
import fft_reference as R

pytestmark = pytest.mark.gpu

N, M = R.N, R.M
N_CTX = 3  # key blocks: 3 x 6 x 2 = 36 polynomials

TWIDDLE_UNITS = 1              # measured 0.661
MARGIN_FORWARD = (2.0, 2.0)    # largest ratios measured over forms x inputs: 0.985, 1.254
MARGIN_INVERSE = (2.0, 2.0)    # 1.105, 1.224
MARGIN_KEY = (4.0, 4.0)        # 1.487, 2.614: the constant polynomial 2^31 - 1, whose spectrum spans 2^9 in magnitude
MARGIN_GENERIC = (4.0, 4.0)    # k_bk_to_spectrum (radix-2, host-made roots): 1.625, 2.096
MARGIN_DISTANCE = 2.0          # rounding distance of a composed product over the model's: 1.000
GUARD_LIMIT = 1 / 16   # kGuardLimit (csrc/br_step.h)


def impulse_bound_units():
    """|probe - closed form| of a unit impulse, in units of 2^-53.  An impulse reaches each output as a product of unit-modulus
    factors: the three chained rotations cos (1 + i tan) of the first pass (dft8_twist_fwd), the first-set twiddle, the W8
    power of the second pass, the second-set twiddle, the W8 power of the third pass -- the three multiplications by a root (pass
    1's, the two table entries) and the two in-register W8 powers between them.  Seven factors, each within TWIDDLE_UNITS of its
    true value (the constants are correctly rounded doubles: within one unit), and seven complex multiplications whose FMA
    pairs round twice per component: at most 2 units in modulus each.  First order: 7 TWIDDLE_UNITS + 14."""
    return 7 * TWIDDLE_UNITS + 14


# ---- the key: the crafted tests' own words, the limb ends, random words ----
def key_words(p):
    rng = np.random.default_rng(17)
    polys = np.zeros((p.n * 2 * p.l * 2, N), dtype=np.int64)
    polys[0], polys[1], polys[2], polys[3] = CS.W_BOTH, CS.W_MIN, CS.W_MAX, -1
    polys[4] = rng.choice(np.array([0x7FFF8000, 0xFFFF8000, 0x80000000, 0x00008000, 0x80008000, 0x7FFF7FFF]), size=N)  # limbs at +-2^15
    polys[5] = rng.choice(np.array([CS.W_MIN, CS.W_MAX, CS.W_BOTH, CS.W_LOW]), size=N)
    polys[6:] = rng.integers(-2**31, 2**31, size=(len(polys) - 6, N))
    polys[7, ::3] = CS.W_BOTH  # special words among random ones
    polys[7, 1::5] = -1
    return (((polys + 2**31) & 0xFFFFFFFF) - 2**31).astype(np.int32)


FORWARD_INPUTS = {  # name -> [1024] coefficients
    "int32": lambda rng: rng.integers(-2**31, 2**31, size=N),
    "7-bit digits": lambda rng: rng.integers(-64, 64, size=N),
    "10-bit digits": lambda rng: rng.integers(-512, 512, size=N),
    "limbs at +-2^15": lambda rng: rng.choice([-2**15, 2**15], size=N),
    "all -2^31": lambda rng: np.full(N, -2**31),
    "all -64": lambda rng: np.full(N, -64),
    "alternating +-2^31": lambda rng: np.where(np.arange(N) % 2 == 0, 2**31 - 1, -2**31),
}


def fold64(p):
    p = np.asarray(p)
    return p[..., :M].astype(np.float64) + 1j * p[..., M:].astype(np.float64)


class World:
    def __init__(self, ia, ctx, p, bk):
        self.ia, self.ctx, self.p, self.bk = ia, ctx, p, bk
        self.polys = bk.reshape(-1, N)
        rng = np.random.default_rng(1)
        self.names = sorted(FORWARD_INPUTS)
        self.inputs = np.stack([FORWARD_INPUTS[k](rng) for k in self.names])
        self.ref = R.forward(R.fold(self.inputs))                                     # [inputs][512] clongdouble, computed once
        self.model = [R.spectrum_errors(R.model_forward(q), r) for q, r in zip(self.inputs, self.ref)]
        self._fwd = {}

    def forward(self, form):
        """probe output of the precision inputs, raw [inputs][8][64]"""
        if form not in self._fwd:
            self._fwd[form] = self.ctx.debug_fft512(form, fold64(self.inputs))
            self._fwd[form].setflags(write=False)
        return self._fwd[form]

    def forward_figures(self, form):
        """[(name, kernel l2, kernel peak, model l2, model peak)] in units of 2^-53"""
        X = R.from_reg_lane(self.forward(form))
        return [(k,) + R.spectrum_errors(X[i], self.ref[i]) + self.model[i] for i, k in enumerate(self.names)]


@pytest.fixture(scope="module")
def world(ia):
    assert ia.device_count() > 0, "gpu-marked test needs a HIP device"
    p = ia.default_params().copy(n=N_CTX, N=N)
    bk = key_words(p).reshape(p.n, 2 * p.l, 2, N)
    ctx = ia.Context.from_arrays(p, bk, np.zeros(p.ksk_count, dtype=np.int32))
    yield World(ia, ctx, p, bk)
    ctx.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- twiddles ----
def twiddle_exponents():
    """entry -> e with value exp(i pi e / 1024) (csrc/tw_roots.h)"""
    e = np.empty(576, dtype=np.int64)
    for idx in range(512):
        k, lane = idx >> 6, idx & 63
        e[idx] = (lane * (1 - 4 * k)) % 2048
    for idx in range(64):
        k, p0 = idx >> 3, idx & 7
        e[512 + idx] = (-32 * p0 * k) % 2048
    return e


def twiddle_error_units(tw):
    """largest error of a component of an entry against the mpmath root, in units of 2^-53"""
    want = R.roots()[twiddle_exponents()]
    d = tw.astype(np.clongdouble) - want
    return float(max(np.abs(d.real).max(), np.abs(d.imag).max())) / R.U53


def test_twiddle_tables_are_one_table_exact_on_the_axes_and_within_the_bound(world):
    t0, t1, t2 = (world.ctx.debug_twiddles(w) for w in (0, 1, 2))
    assert np.array_equal(bits(t0), bits(t1)), "the CMux family's table differs from the blind rotation's"
    assert np.array_equal(bits(t0), bits(t2)), "a table built in a 64-thread kernel differs from the context's"
    e = twiddle_exponents()
    axes = {0: 1, 512: 1j, 1024: -1, 1536: -1j}
    on_axis = [i for i in range(576) if int(e[i]) in axes]
    assert len(on_axis) == 8 + 16  # lane 0 of the first set; p0 k a multiple of 16 (p0 = 0, k = 0, 4 x 4) of the second
    for i in on_axis:
        assert t0[i] == axes[int(e[i])], (i, t0[i])
    err = twiddle_error_units(t0)
    print("twiddle table: largest error %.3f units of 2^-53" % err)
    assert TWIDDLE_UNITS <= 4
    assert err <= TWIDDLE_UNITS, err


# ---- forward: layout ----
@pytest.mark.parametrize("form", range(5))
def test_forward_sends_impulses_to_the_documented_layout(world, form):
    """A wrong permutation, transpose or twiddle index moves whole outputs: an error of order 1, 2^53 units."""
    y = np.stack([R.impulse(s) for s in R.IMPULSE_SLOTS])
    out = world.ctx.debug_fft512(form, y)
    worst = 0.0
    for i, slot in enumerate(R.IMPULSE_SLOTS):
        d = np.abs(R.from_reg_lane(out[i]).astype(np.clongdouble) - R.impulse_spectrum(slot))
        worst = max(worst, float(d.max()) / R.U53)
        assert float(d.max()) / R.U53 <= impulse_bound_units(), (slot, int(d.argmax()), float(d.max()) / R.U53)
    print("form %d: impulses within %.2f units of the closed form (bound %d)" % (form, worst, impulse_bound_units()))


# ---- forward: precision ----
@pytest.mark.parametrize("form", range(5))
def test_forward_is_in_the_models_precision_class(world, form):
    assert max(MARGIN_FORWARD + MARGIN_INVERSE + MARGIN_KEY + MARGIN_GENERIC) <= 4
    bad = []
    for name, kl2, kpeak, ml2, mpeak in world.forward_figures(form):
        print("form %d %-20s kernel l2 %.3f peak %.3f | model l2 %.3f peak %.3f | ratio %.3f %.3f" % (form, name, kl2, kpeak, ml2, mpeak, kl2 / ml2, kpeak / mpeak))
        if not (kl2 <= MARGIN_FORWARD[0] * ml2 and kpeak <= MARGIN_FORWARD[1] * mpeak):
            bad.append((name, kl2, kpeak, ml2, mpeak))
    assert not bad, bad


def test_counts_one_four_and_five_give_the_batchs_bits(world):
    """A full workgroup, a ragged one and a lone wave: the transform of a row does not depend on its neighbours (a tile per
    wave, one table per workgroup)."""
    y = fold64(world.inputs)
    for form in range(5):
        whole = world.forward(form)
        for count in (1, 4, 5):
            assert np.array_equal(bits(world.ctx.debug_fft512(form, y[:count])), bits(whole[:count])), (form, count)
    spec = world.forward(0).reshape(-1, M)
    whole = world.ctx.debug_fft512(5, spec[:6])
    for count in (1, 4, 5):
        assert np.array_equal(bits(world.ctx.debug_fft512(5, spec[:count])), bits(whole[:count])), count


# ---- forms agree ----
def test_every_forward_form_returns_the_same_bits(world):
    """The forms differ in data movement, root storage and the hook only; under -ffp-contract=on contraction follows the source
    expression, which they share."""
    y = np.concatenate([fold64(world.inputs), np.stack([R.impulse(s) for s in R.IMPULSE_SLOTS]), fold64(world.polys[:8])])
    first = world.ctx.debug_fft512(0, y)
    for form in range(1, 5):
        out = world.ctx.debug_fft512(form, y)
        diff = np.argwhere(bits(out) != bits(first))
        assert diff.size == 0, (form, diff[:4].tolist())


def test_every_inverse_form_returns_the_same_bits(world):
    spec = np.concatenate([world.forward(0), world.ctx.debug_fft512(0, fold64(world.polys[:9]))]).reshape(-1, M)
    assert len(spec) % 2 == 0
    first = world.ctx.debug_fft512(5, spec)
    for form in (6, 7):
        out = world.ctx.debug_fft512(form, spec)
        diff = np.argwhere(bits(out) != bits(first))
        assert diff.size == 0, (form, diff[:4].tolist())


def test_inverse_undoes_the_reference_forward(world):
    """The inverse on its own, against the defining sum: the exactly representable spectrum nearest the reference's goes in, the
    reference inverse of THAT spectrum is what must come out, to the forward's margin over the model's own inverse."""
    spec = R.to_reg_lane(world.ref).astype(np.complex128)  # [inputs][8][64]
    want = R.inverse(R.from_reg_lane(spec))                # [inputs][512] clongdouble
    for form in (5, 6):
        pad = spec if len(spec) % 2 == 0 else np.concatenate([spec, spec[:1]])
        got = world.ctx.debug_fft512(form, pad)[:len(spec)].reshape(len(spec), M)
        for i, name in enumerate(world.names):
            tw = np.exp(1j * np.pi * np.arange(M) / N)
            mod = np.fft.ifft(R.from_reg_lane(spec[i])) * np.conj(tw)
            kl2, kpeak = R.spectrum_errors(got[i], want[i])
            ml2, mpeak = R.spectrum_errors(mod, want[i])
            print("form %d inverse %-20s kernel l2 %.3f peak %.3f | model l2 %.3f peak %.3f | ratio %.3f %.3f" % (form, name, kl2, kpeak, ml2, mpeak, kl2 / ml2, kpeak / mpeak))
            assert kl2 <= MARGIN_INVERSE[0] * ml2 and kpeak <= MARGIN_INVERSE[1] * mpeak, (form, name)


# ---- tied to production ----
def test_one_limb_key_spectrum_is_the_probes_forward_of_the_key(world):
    got = world.ctx.debug_spectrum(1, 0, len(world.polys))
    want = world.ctx.debug_fft512(0, fold64(world.polys))
    assert np.array_equal(bits(got), bits(want))
    _check_against_reference("one-limb", R.from_reg_lane(got[:8]), world.polys[:8])


def test_two_limb_key_spectrum_is_the_probes_forward_of_the_limbs(world):
    got = world.ctx.debug_spectrum(0, 0, len(world.polys))  # [poly][limb][8][64]
    lo, hi = R.limb_split(world.polys)
    assert np.array_equal(bits(got[:, 0]), bits(world.ctx.debug_fft512(0, fold64(lo))))
    assert np.array_equal(bits(got[:, 1]), bits(world.ctx.debug_fft512(0, fold64(hi))))
    _check_against_reference("two-limb low", R.from_reg_lane(got[:8, 0]), lo[:8])
    _check_against_reference("two-limb high", R.from_reg_lane(got[:8, 1]), hi[:8])
    part = world.ctx.debug_spectrum(0, 5, 3)  # a window that starts inside the key
    assert np.array_equal(bits(part), bits(got[5:8]))


def _check_against_reference(label, X, polys, margin=MARGIN_KEY):
    """X [polys][n/2] in natural order against the reference, to the margin over the model at that n"""
    bad = []
    for i, p in enumerate(polys):
        if not np.any(p):
            assert not np.any(X[i]), (label, i)
            continue
        ref, mod = R.forward(R.fold(p)), R.model_forward(p)
        (kl2, kpeak), (ml2, mpeak) = R.spectrum_errors(X[i], ref), R.spectrum_errors(mod, ref)
        print("%s polynomial %d: kernel l2 %.3f peak %.3f | model l2 %.3f peak %.3f | ratio %.3f %.3f" % (label, i, kl2, kpeak, ml2, mpeak, kl2 / ml2, kpeak / mpeak))
        if not (kl2 <= margin[0] * ml2 and kpeak <= margin[1] * mpeak):
            bad.append((label, i, kl2, kpeak, ml2, mpeak))
    assert not bad, bad


@pytest.mark.parametrize("n_ring,force", [(16, False), (64, False), (1024, True)])
def test_generic_key_spectrum_against_the_reference(ia, n_ring, force):
    """k_bk_to_spectrum's form (host-made twiddles, radix-2, bit-reversed out) on the rings the any-parameter kernel runs."""
    p = ia.default_params().copy(n=2, N=n_ring)
    rng = np.random.default_rng(23)
    polys = rng.integers(-2**31, 2**31, size=(p.n * 2 * p.l * 2, n_ring))
    polys[0], polys[1], polys[2] = CS.W_BOTH, CS.W_MIN, -1
    polys[3, ::2] = CS.W_LOW
    polys = (((polys + 2**31) & 0xFFFFFFFF) - 2**31).astype(np.int32)
    with ia.Context.from_arrays(p, polys.reshape(p.n, 2 * p.l, 2, n_ring), np.zeros(p.ksk_count, dtype=np.int32)) as ctx:
        if force:
            ctx.set_option("force_generic", 1)
            assert ctx.kernel_variant == "generic-radix2"
        got = ctx.debug_spectrum(2, 0, 6)  # [poly][limb][n/2]
    lo, hi = R.limb_split(polys[:6])
    order = R.bit_reversed(n_ring // 2)  # stored[i] = X[order[i]]; a bit reversal is its own inverse
    _check_against_reference("generic N=%d low" % n_ring, got[:, 0][:, order], lo, MARGIN_GENERIC)
    _check_against_reference("generic N=%d high" % n_ring, got[:, 1][:, order], hi, MARGIN_GENERIC)


# ---- inverse and the rounding margin ----
def probe_product_sum(ctx, digs, bks):
    """A step's product composed of the probe's transforms: forward of the digit polynomials (form 1) and of the key
    polynomials (form 0, as the key is prepared), inverse (form 5) -> the [1024] doubles a kernel would round.  The
    multiply-accumulate between them is numpy's complex128, NOT the kernel's FMA order: what is measured is the two transforms."""
    fd = ctx.debug_fft512(1, fold64(np.asarray(digs)))
    fb = ctx.debug_fft512(0, fold64(np.asarray(bks)))
    acc = (fd * fb).sum(axis=0)
    y = ctx.debug_fft512(5, acc[None])[0].reshape(M)  # out[r][lane] = y_{64 r + lane}
    return np.concatenate([y.real, y.imag])


def one_limb_inputs():
    """test_rounding_model_cpu's three, at (l, Bgbit) = (3, 7)"""
    rng1, rng2 = np.random.default_rng(1), np.random.default_rng(2)
    return [("random", rng1.integers(-64, 64, size=(6, N)), rng1.integers(-2**31, 2**31, size=(6, N))),
            ("extreme magnitudes", rng2.choice([-64, 63], size=(6, N)), rng2.choice([-2**31, 2**31 - 1], size=(6, N))),
            ("worst alignment", np.full((6, N), -64), np.full((6, N), -2**31))]


def two_limb_inputs(l, Bgbit, n=N):
    """two_limb_model's two, drawn as it draws them"""
    kpl, half = 2 * l, 1 << (Bgbit - 1)
    rng = np.random.default_rng(2)
    return [("extreme magnitudes", rng.choice([-half, half - 1], size=(kpl, n)), rng.choice([-2**15, 2**15], size=(kpl, n))),
            ("worst alignment", np.full((kpl, n), -half), np.full((kpl, n), -2**15))]


def product_figures(ctx, digs, bks):
    """-> (kernel distance, kernel rounds exactly, model distance, model rounds exactly, log2 of the largest exact sum)"""
    exact = R.exact_product_sum(digs, bks)
    yk, ym = probe_product_sum(ctx, digs, bks), R.model_product_sum(digs, bks)
    peak = float(np.log2(max(abs(int(v)) for v in exact)))
    return R.rounding_distance(yk), R.rounds_to(yk, exact), R.rounding_distance(ym), R.rounds_to(ym, exact), peak


def test_one_limb_products_keep_the_rounding_margin(world):
    """The one-limb product at (3, 7): rounding gives the exact product wherever the model's does, the distance stays within
    MARGIN_DISTANCE of the model's, and the project's own limits hold whatever the margin: below the guard limit on random
    and extreme operands, ABOVE it at the worst alignment (2^49.58) -- the case the guard exists for."""
    for name, digs, bks in one_limb_inputs():
        dk, ek, dm, em, peak = product_figures(world.ctx, digs, bks)
        print("one-limb %-20s sums 2^%.2f: kernel distance %.5f exact %s | model %.5f exact %s | ratio %.3f" % (name, peak, dk, ek, dm, em, dk / dm if dm else float("inf")))
        assert ek or not em, name
        assert dk <= MARGIN_DISTANCE * dm, (name, dk, dm)
        if name == "worst alignment":
            assert dk > GUARD_LIMIT, dk
        else:
            assert ek and dk < GUARD_LIMIT, (name, dk)


@pytest.mark.parametrize("l,Bgbit", [(3, 7), (2, 10), (1, 21)])
def test_two_limb_products_are_exact_with_margin(world, l, Bgbit):
    """The two-limb product on two_limb_model's inputs, (1, 21, 1024) being the 2^46 edge of Params::br_exact(): exact, within
    MARGIN_DISTANCE of the model's distance, and below 1/32 whatever the margin."""
    for name, digs, bks in two_limb_inputs(l, Bgbit):
        dk, ek, dm, em, peak = product_figures(world.ctx, digs, bks)
        print("two-limb (%d, %d) %-20s sums 2^%.2f: kernel distance %.4g exact %s | model %.4g exact %s | ratio %.3f" % (l, Bgbit, name, peak, dk, ek, dm, em, dk / dm if dm else float("inf")))
        assert ek or not em, name
        assert ek and dk < 1 / 32, (name, dk)
        assert dk <= MARGIN_DISTANCE * dm, (name, dk, dm)


# ---- refusals ----
def _refused(ia, rc, reason):
    assert rc == -22, rc
    msg = ia.lib().ieache_last_error().decode()
    assert reason in msg, msg


def test_refusals_name_the_reason_and_write_nothing(ia, world):
    L, h = ia.lib(), world.ctx.h
    f64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    inp = np.ones((2, 512, 2))
    out = np.full((2, 512, 2), 7.0)
    tw = np.full((576, 2), 7.0)
    for form in (-1, 8):
        _refused(ia, L.ieache_debug_fft512(h, form, 2, f64(inp), f64(out)), "unknown form")
    for form in (6, 7):
        _refused(ia, L.ieache_debug_fft512(h, form, 1, f64(inp), f64(out)), "even count")
    _refused(ia, L.ieache_debug_fft512(h, 0, 2, None, f64(out)), "null")
    _refused(ia, L.ieache_debug_fft512(h, 0, 2, f64(inp), None), "null")
    _refused(ia, L.ieache_debug_fft512(None, 0, 2, f64(inp), f64(out)), "null")
    _refused(ia, L.ieache_debug_twiddles(h, 0, None), "null")
    _refused(ia, L.ieache_debug_twiddles(h, 3, f64(tw)), "which")
    _refused(ia, L.ieache_debug_spectrum(h, 0, 0, 1, None), "null")
    _refused(ia, L.ieache_debug_spectrum(h, 3, 0, 1, f64(out)), "which")
    _refused(ia, L.ieache_debug_spectrum(h, 1, len(world.polys), 1, f64(out)), "outside the key")
    _refused(ia, L.ieache_debug_spectrum(h, 1, len(world.polys) - 1, 2, f64(out)), "outside the key")
    p = ia.default_params().copy(n=2, N=64)
    with ia.Context.from_arrays(p, np.zeros(p.bk_count, dtype=np.int32), np.zeros(p.ksk_count, dtype=np.int32)) as small:
        _refused(ia, L.ieache_debug_fft512(small.h, 0, 2, f64(inp), f64(out)), "N = 1024")
        _refused(ia, L.ieache_debug_twiddles(small.h, 0, f64(tw)), "N = 1024")
        _refused(ia, L.ieache_debug_twiddles(small.h, 2, f64(tw)), "N = 1024")
        _refused(ia, L.ieache_debug_spectrum(small.h, 0, 0, 1, f64(out)), "N = 1024")
        _refused(ia, L.ieache_debug_spectrum(small.h, 1, 0, 1, f64(out)), "N = 1024")
    assert (out == 7.0).all() and (tw == 7.0).all() and (inp == 1.0).all()
