"""tests/fft_reference.py proved before the card is asked anything (tests/test_fft_probe_gpu.py holds the kernels to it): the
extended-precision transform reproduces exact integer negacyclic products, its (register, lane) order is the closed form on
unit impulses, the limb split recombines, and the numpy double model's own error against it is a few units of 2^-53."""
import numpy as np
import pytest

import fft_reference as R

N, M = R.N, R.M


def test_roots_are_exact_on_the_axes_and_unit_length():
    r = R.roots()
    assert r.dtype == np.clongdouble and np.finfo(np.longdouble).nmant >= 63, "the reference needs an extended long double"
    for e, want in ((0, 1), (512, 1j), (1024, -1), (1536, -1j)):
        assert r[e] == want
    assert float(np.abs(np.abs(r) - 1).max()) < 2.0 ** -62
    assert np.array_equal(r[1024:], -r[:1024]) and np.array_equal(r[1:1024][::-1].real, -r[1:1024].real)


def test_forward_product_inverse_reproduces_exact_negacyclic_products():
    """Full-range int32 against 7-bit digits, six products summed as a CMux step sums them: |sums| reach 2^44.  Observed on
    default_rng(1): the reference is within 2^-17.0 of the exact integers (2^-60 of the largest sum, 2^43.4), where a double
    transform leaves 2^-8.  Asserted a few bits looser: 2^-15."""
    rng = np.random.default_rng(1)
    digs, bks = rng.integers(-64, 64, size=(6, N)), rng.integers(-2**31, 2**31, size=(6, N))
    exact = R.exact_product_sum(digs, bks)
    y = R.reference_product_sum(digs, bks)
    err = max(abs(float(y[i] - np.longdouble(int(exact[i])))) for i in range(N))
    print("reference product: largest error %.3g = 2^%.1f at largest sum 2^%.1f" % (err, np.log2(err), np.log2(max(abs(int(v)) for v in exact))))
    assert err < 2.0 ** -15
    assert R.rounds_to(y.astype(np.float64), exact)
    # one product of a single polynomial pair, and the inverse undoing the forward on its own
    y1 = R.unfold(R.inverse(R.forward(R.fold(bks[0]))))
    assert float(np.abs(y1 - bks[0].astype(np.longdouble)).max()) < 2.0 ** -25  # 2^31 x 2^-60 = 2^-29 expected


def test_reg_lane_order_round_trips_and_matches_the_closed_form_on_impulses():
    X = np.arange(M) + 1j * np.arange(M)[::-1]
    assert np.array_equal(R.from_reg_lane(R.to_reg_lane(X)), X)
    assert sorted(R.REG_LANE.ravel().tolist()) == list(range(M))
    batch = np.stack([X, X[::-1]])
    assert np.array_equal(R.from_reg_lane(R.to_reg_lane(batch)), batch)
    r = R.roots()
    for slot in R.IMPULSE_SLOTS:
        out = R.to_reg_lane(R.forward(R.impulse(slot)))
        closed = R.impulse_spectrum(slot)
        j, v = slot % M, (1 if slot < M else 1j)
        for k2 in range(8):  # the documented layout, index by index: x[k2] = X[k0 + 8 k1 + 64 k2] at lane = 8 k0 + k1
            for k0 in range(8):
                for k1 in range(8):
                    k = k0 + 8 * k1 + 64 * k2
                    want = v * r[(j * (1 - 4 * k)) % 2048]
                    assert out[k2, 8 * k0 + k1] == want == closed[k], (slot, k2, k0, k1)


def test_bit_reversed_order():
    assert R.bit_reversed(8).tolist() == [0, 4, 2, 6, 1, 5, 3, 7]
    assert R.bit_reversed(1).tolist() == [0]
    b = R.bit_reversed(512)
    assert sorted(b.tolist()) == list(range(512)) and np.array_equal(b[b], np.arange(512)) and b[1] == 256


def test_limb_split_recombines_and_stays_balanced():
    words = [0, -1, 0x7FFF8000, 0x7FFF7FFF, 0x80000000, 0x00008000, 0xFFFF8000]
    lo, hi = R.limb_split(words)
    assert lo.tolist() == [0, -1, -32768, 32767, 0, -32768, -32768]
    assert hi.tolist() == [0, 0, 32768, 32767, -32768, 1, 0]
    rng = np.random.default_rng(4)
    w = np.concatenate([np.array(words, dtype=np.int64), rng.integers(-2**31, 2**31, size=4096)])
    lo, hi = R.limb_split(w)
    assert np.array_equal((lo + (hi << 16)) & 0xFFFFFFFF, w & 0xFFFFFFFF)
    assert lo.min() >= -2**15 and lo.max() < 2**15 and hi.min() >= -2**15 and hi.max() <= 2**15
    assert hi.max() == 2**15 and lo.min() == -2**15  # the ends are met


MODEL_INPUTS = {
    "int32": lambda rng: rng.integers(-2**31, 2**31, size=N),
    "7-bit digits": lambda rng: rng.integers(-64, 64, size=N),
    "16-bit limbs": lambda rng: rng.integers(-2**15, 2**15, size=N),
    "all -2^31": lambda rng: np.full(N, -2**31),
}


@pytest.mark.parametrize("name", sorted(MODEL_INPUTS))
def test_the_numpy_model_is_a_few_units_from_the_reference(name):
    """The yardstick itself: the model's relative L2 spectrum error is a small multiple of 2^-53 (nine radix-2 stages of
    roundings that add in quadrature: sqrt(9) x O(1)), its largest single error some times that.  Bounds from that reasoning,
    16 and 64 units: what a transform of the double-precision class cannot exceed, and a float twiddle (2^29 units) would."""
    p = MODEL_INPUTS[name](np.random.default_rng(1))
    l2, peak = R.spectrum_errors(R.model_forward(p), R.forward(R.fold(p)))
    print("model error on %s: relative L2 %.2f, largest %.2f (units of 2^-53)" % (name, l2, peak))
    assert 0 < l2 < 16 and l2 <= peak < 64


def test_probe_entries_are_exported_and_refuse_null_before_any_device_work(ia):
    """The three entries of the transform probe (include/ieache.h): present, and a null context or array is IEACHE_EINVAL with
    the reason named and nothing written -- no GPU needed to say so."""
    import ctypes as C
    L = ia.lib()
    out = np.full(8, 7.0)
    f64 = out.ctypes.data_as(C.POINTER(C.c_double))
    for rc in (L.ieache_debug_twiddles(None, 0, f64), L.ieache_debug_fft512(None, 0, 1, f64, f64), L.ieache_debug_spectrum(None, 0, 0, 1, f64)):
        assert rc == -22 and "null" in L.ieache_last_error().decode()
    assert (out == 7.0).all()
    assert ia.FFT_FORWARD_FORMS == (0, 1, 2, 3, 4) and ia.FFT_INVERSE_FORMS == (5, 6, 7) and ia.FFT_PAIRED_FORMS == (6, 7)


def test_model_product_distance_matches_the_rounding_model():
    rng = np.random.default_rng(1)
    digs, bks = rng.integers(-64, 64, size=(6, N)), rng.integers(-2**31, 2**31, size=(6, N))
    y = R.model_product_sum(digs, bks)
    assert R.rounds_to(y, R.exact_product_sum(digs, bks)) and 0 < R.rounding_distance(y) < 1 / 64
