"""Linear layers on encrypted rows (include/ieache.h section 3n) without a GPU: the symbols, the rules of csrc/linear_plan.h in
their order and words through the entry points (with a NULL context where a rule needs none), the C reference
ieache_lwe_linear_reference against the numpy restatement (linear_reference.py) word for word on random and crafted inputs, the
plan in a stand-alone program under AddressSanitizer + UBSan, and ie-ache_amd/layers.py: run_clear against integer arithmetic and
the margins of DESIGN.md section 7."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction as F

import numpy as np
import pytest

import linear_reference as LN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLARED = {"ieache_lwe_linear": 10, "ieache_lwe_linear_device": 10, "ieache_lwe_linear_reference": 9, "ieache_debug_linear_plan": 6}
SETS = [(5, 16), (37, 64), (130, 1024)]


def test_every_symbol_is_declared_exported_and_bound(ia):
    with open(os.path.join(ROOT, "include", "ieache.h")) as f:
        text = f.read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = {m.group(1): m.group(2) for m in re.finditer(r"^int\s+(ieache_(?:lwe_linear|debug_linear)[a-z_]*)\s*\(([^;]*)\)\s*;", hdr, re.M)}
    assert set(declared) == set(DECLARED)
    raw, L = C.CDLL(ia.library_path()), ia.lib()
    for name, n_params in DECLARED.items():
        assert len(declared[name].split(",")) == n_params, name
        assert hasattr(raw, name), name
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n_params, name
    for name in ("lwe_linear", "lwe_linear_device", "linear_plan"):
        assert callable(getattr(ia.Context, name)), name
    from ieache_amd import tools, layers
    assert callable(tools.lwe_linear_reference) and callable(layers.Dense) and callable(layers.sign_layer) and callable(layers.bivariate)
    assert (ia.ROWS_LWE, ia.ROWS_EXTRACTED, ia.ROWS_TLWE, ia.LINEAR_MAX_DIM) == (0, 1, 2, 65536)
    for line in ("#define IEACHE_ROWS_LWE 0", "#define IEACHE_ROWS_EXTRACTED 1", "#define IEACHE_ROWS_TLWE 2", "#define IEACHE_LINEAR_MAX_DIM 65536"):
        assert line in hdr
    assert "There is no group form and no cloudd" in text[text.index("3n. Linear layers"):text.index("4. CPU tools around the path")]


def test_rules_in_order_and_in_words(ia):
    """Rules 1 to 3 need no context: a NULL one gets their messages.  Every argument after the rule under test is wrong too, so
    the message that comes back shows the order."""
    L = ia.lib()
    p = ia.default_params().copy(n=5, N=16)
    w = np.ones((2, 3), dtype=np.int8)
    bias = np.zeros(2, dtype=np.int32)
    x = np.zeros((1, 3, 6), dtype=np.int32)
    out = np.zeros((1, 2, 6), dtype=np.int32)
    i8, i32 = (lambda a: a.ctypes.data_as(C.POINTER(C.c_int8))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)))

    def said(rc):
        assert rc == -22
        return L.ieache_last_error().decode()

    forms = [lambda *a: L.ieache_lwe_linear(None, *a, None), lambda *a: L.ieache_lwe_linear_reference(C.byref(p), *a),
             lambda *a: L.ieache_lwe_linear_reference(None, *a)]
    for f in forms:
        assert "unknown rows kind" in said(f(3, 1, 0, 0, None, i32(bias), None, None))
        assert "unknown rows kind" in said(f(-1, 1, 2, 3, i8(w), None, i32(x), i32(out)))
        assert "n_out and n_in must lie in 1 .. 65536" in said(f(2, 1, 0, 3, None, i32(bias), None, None))
        assert "n_out and n_in must lie in 1 .. 65536" in said(f(2, 1, 2, 65537, None, i32(bias), None, None))
        assert "n_out and n_in must lie in 1 .. 65536" in said(f(0, 0, 65537, 3, i8(w), None, i32(x), i32(out)))
        assert "TLWE rows have no bias word" in said(f(2, 1, 2, 3, None, i32(bias), None, None))
        assert "TLWE rows have no bias word" in said(f(2, 0, 2, 3, i8(w), i32(bias), i32(x), i32(out)))
    # the device form hands its pointers over as addresses
    dev = lambda *a: L.ieache_lwe_linear_device(None, *a, None)
    assert "unknown rows kind" in said(dev(7, 1, 0, 0, None, bias.ctypes.data, None, None))
    assert "1 .. 65536" in said(dev(2, 1, 65537, 1, None, bias.ctypes.data, None, None))
    assert "TLWE rows have no bias word" in said(dev(2, 1, 2, 3, None, bias.ctypes.data, None, None))
    plan = (C.c_int64 * 4)()
    assert "unknown rows kind" in said(L.ieache_debug_linear_plan(None, 3, 1, 0, 0, plan))
    assert "1 .. 65536" in said(L.ieache_debug_linear_plan(None, 0, 1, 0, 1, plan))
    # rule 4: with scalars that pass, the NULL context -- and for the reference, which has none, the NULL arrays of a call with rows
    for f in forms[:1] + [dev]:
        assert said(f(0, 1, 2, 3, w.ctypes.data_as(C.c_void_p) if f is dev else i8(w), None, None, None)) == "lwe_linear: null argument"
    assert said(L.ieache_debug_linear_plan(None, 0, 1, 1, 1, plan)) == "lwe_linear: null argument"
    ref = forms[1]
    assert said(forms[2](0, 1, 2, 3, i8(w), None, i32(x), i32(out))) == "lwe_linear: null argument"  # no parameter set
    assert said(ref(0, 1, 2, 3, None, None, i32(x), i32(out))) == "lwe_linear: null argument"
    assert said(ref(0, 1, 2, 3, i8(w), None, None, i32(out))) == "lwe_linear: null argument"
    assert said(ref(0, 1, 2, 3, i8(w), i32(bias), i32(x), None)) == "lwe_linear: null argument"
    assert ref(0, 1, 2, 3, i8(w), None, i32(x), i32(out)) == 0 and ref(0, 1, 2, 3, i8(w), i32(bias), i32(x), i32(out)) == 0
    assert ref(0, 0, 2, 3, None, None, None, None) == 0  # batch == 0 is a no-op
    assert "unsupported" in said(L.ieache_lwe_linear_reference(C.byref(p.copy(N=8)), 0, 1, 2, 3, i8(w), None, i32(x), i32(out)))
    # the Python wrappers refuse weights outside int8 before the library is called
    from ieache_amd import tools
    for bad in (128, -129):
        with pytest.raises(ValueError, match="-128 .. 127"):
            tools.lwe_linear_reference(p, x, [[bad, 0, 0]])
    assert tools.lwe_linear_reference(p, x, np.array([[127, -128, 0]], dtype=np.int64)).shape == (1, 1, 6)
    with pytest.raises(ValueError, match="one word per output"):
        tools.lwe_linear_reference(p, x, w, bias=[1, 2, 3])


@pytest.mark.parametrize("n,N", SETS)
def test_reference_is_the_definition(ia, n, N):
    from ieache_amd import tools
    p = ia.default_params().copy(n=n, N=N)
    rng = np.random.default_rng(14000 + n + N)
    for rows in LN.KINDS:
        words, at = LN.words_of(n, N, rows), LN.bias_word(n, N, rows)
        for batch, n_out, n_in in ((1, 1, 1), (3, 7, 33), (2, 33, 17)):
            bias = None if at is None else LN.full_range(rng, n_out)
            for x in (LN.full_range(rng, (batch, n_in, words)), LN.crafted_rows(rng, (batch, n_in, words))):
                for name, W in LN.weight_cases(rng, n_out, n_in).items():
                    got = tools.lwe_linear_reference(p, x, W, bias, rows)
                    assert got.shape == (batch, n_out, words) and np.array_equal(got, LN.linear(x, W, bias, at)), (rows, batch, n_out, n_in, name)
            # the bias lands on the bias word only
            if at is not None:
                W = LN.weight_cases(rng, n_out, n_in)["full"]
                x = LN.full_range(rng, (batch, n_in, words))
                with_b, without = tools.lwe_linear_reference(p, x, W, bias, rows), tools.lwe_linear_reference(p, x, W, None, rows)
                diff = LN.wrap32(with_b.astype(np.int64) - without)
                assert not np.delete(diff, at, axis=2).any() and np.array_equal(diff[:, :, at], np.broadcast_to(bias, (batch, n_out)))
        # the identity returns x
        x = LN.asymmetric_rows(2, 9, words)
        assert np.array_equal(tools.lwe_linear_reference(p, x, np.eye(9, dtype=np.int8), None, rows), x)
        assert tools.lwe_linear_reference(p, x[:0], np.eye(9, dtype=np.int8), None, rows).shape == (0, 9, words)


def test_reference_at_the_largest_sum(ia):
    """n_in = 65 536 with every weight -128 and every balanced limb of every word -128: each limb column sums to 2^30."""
    from ieache_amd import tools
    p = ia.default_params().copy(n=5, N=16)
    assert LN.balanced_limbs(0x7F7F7F80) == [-128] * 4 and LN.balanced_limbs(0x7F7F7F7F) == [127] * 4
    for v in LN.CRAFTED_WORDS:
        assert sum(b << (8 * k) for k, b in enumerate(LN.balanced_limbs(v))) & 0xFFFFFFFF == v
    x = LN.constant_rows(0x7F7F7F80, (1, 65536, 6))
    W = np.full((2, 65536), -128, dtype=np.int8)
    W[1, ::2] = 127
    bias = np.array([1, -1], dtype=np.int32)
    got = tools.lwe_linear_reference(p, x, W, bias, "lwe")
    assert np.array_equal(got, LN.linear(x, W, bias, 5))
    assert int(got[0, 0, 0]) & 0xFFFFFFFF == (65536 * -128 * 0x7F7F7F80) & 0xFFFFFFFF


def test_linear_plan_under_asan_ubsan(tmp_path):
    """tests/native/linear_plan_test.cpp: a stand-alone program over csrc/linear_plan.h, run as its own executable."""
    exe = tmp_path / "linear_plan_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "native", "linear_plan_test.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "LINEAR_PLAN_OK" in r.stdout, r.stdout[-4000:]


# ---- ie-ache_amd/layers.py ----
def test_run_clear_is_integer_arithmetic(ia):
    from ieache_amd import layers
    T = layers.torus
    assert T(0) == 0 and T(F(1, 8)) == 1 << 29 and T(F(-1, 8)) == -(1 << 29) and T(F(1, 2)) == -(1 << 31) and T(F(7, 8)) == -(1 << 29)
    # the worked neuron of DESIGN.md section 7 on all sixteen sign patterns: the sign of 1/20 + (a + b - c - d) / 10
    d = layers.sign_layer([[1, 1, -1, -1]], [T(F(1, 20))], inputs=[F(-1, 10), F(1, 10)], mu=T(F(1, 10)))
    signs = [[1 if (k >> j) & 1 else -1 for j in range(4)] for k in range(16)]
    got = d.run_clear([[F(s, 10) for s in row] for row in signs])
    for row, word in zip(signs, got[:, 0]):
        twentieths = 1 + 2 * (row[0] + row[1] - row[2] - row[3])  # the clear phase in twentieths: -7 .. 9, never 0 or 10
        assert word == (T(F(1, 10)) if twentieths > 0 else -T(F(1, 10))), row
    assert sorted({int(round(float(t) * 20)) for t in d.reachable_phases(0)}) == [1, 5, 9, 13, 17]  # 0.05, 0.25, 0.45, -0.35, -0.15
    # a random integer layer on message slots: p = 4 messages per input, the table of the sums mod 8
    p = ia.default_params()
    from ieache_amd import tools
    table = np.array([T(F(m, 16)) for m in range(8)], dtype=np.int64).astype(np.int32)
    W = np.array([[1, 1, 0], [1, 0, 1], [0, 1, 1]])
    layer = layers.Dense(W, None, tools.lut_test_poly(p, table), inputs=[F(m, 16) for m in range(4)], slots=(F(1, 16), F(1, 32)))
    rng = np.random.default_rng(14100)
    msgs = rng.integers(0, 4, size=(20, 3))
    got = layer.run_clear([[F(int(m), 16) for m in row] for row in msgs])
    assert np.array_equal(got, np.array([[T(F(int(s), 16)) for s in (W @ row)] for row in msgs]))
    # bivariate: x p + y through one table of p^2 entries
    mul = layers.bivariate(lambda a, b: (a * b) % 4, 4, p, scale=1 << 28)
    assert mul.W.tolist() == [[4, 1]] and mul.bias is None and float(mul.gap(0)) == 1 / 64
    for a in range(4):
        for b in range(4):
            assert mul.run_clear([[F(a, 32), F(b, 32)]])[0, 0] == ((a * b) % 4) << 28


def test_margin_reproduces_the_design_table(ia):
    """DESIGN.md section 7, "Linear layers": (gap - |sum w| 4 sigma_delta) / sqrt(||w||^2 V + rounding) at the gate parameters,
    from the figures the document already carries.  The worked neuron must keep 7 sigma: at 7 sigma 4 096 decodes expect
    about 1e-8 failures."""
    from test_golden_cpu import predicted_gate_output_noise
    from ieache_amd import layers
    T = layers.torus
    p = ia.default_params()
    V, sigma_delta = predicted_gate_output_noise(p)
    rounding = (1 + p.n / 2) / 12.0 / (2.0 * p.N) ** 2
    assert abs(V - 1.05e-5) < 0.03e-5 and abs(sigma_delta - 1.2e-3) < 0.05e-3 and abs(rounding - 6.3e-6) < 0.1e-6
    table = [  # weights, bias, inputs, gap, sigmas in the document
        ([[1]], 0, (F(-1, 8), F(1, 8)), F(1, 8), 29.3),
        ([[1, 1]], F(-1, 8), (F(-1, 8), F(1, 8)), F(1, 8), 22.1),
        ([[1, 1, -1, -1]], F(1, 20), (F(-1, 10), F(1, 10)), F(1, 20), 7.2),
        ([[2, -2, 1, -1]], F(1, 28), (F(-1, 14), F(1, 14)), F(1, 28), 3.4),
        ([[1, 1, 1, 1, -1, -1, -1, -1]], F(1, 40), (F(-1, 20), F(1, 20)), F(1, 40), 2.6),
    ]
    for W, bias, inputs, gap, sigmas in table:
        d = layers.sign_layer(W, [T(bias)], inputs=inputs)
        assert abs(d.gap(0) - gap) < F(1, 1 << 31), W
        got = d.margin(V, sigma_delta, rounding)
        w = np.array(W[0], dtype=np.float64)
        assert abs(got - (float(gap) - abs(w.sum()) * 4 * sigma_delta) / np.sqrt((w ** 2).sum() * V + rounding)) < 1e-6
        print("weights %s: gap %.4f, margin %.2f sigma (the document says %.1f)" % (W[0], float(gap), got, sigmas))
        assert abs(got - sigmas) < 0.15, W
    worked = layers.sign_layer(table[2][0], [T(table[2][1])], inputs=table[2][2])
    assert worked.margin(V, sigma_delta, rounding) >= 7.0
    # the first layer of the end-to-end test: fan-in 8 on FRESH inputs (alpha = 2^-15, no offset of a key switch)
    fresh = layers.sign_layer([[1, 1, 1, 1, -1, -1, -1, -1]], [T(F(1, 32))], inputs=(F(-1, 32), F(1, 32)))
    assert fresh.margin(p.lwe_alpha_min ** 2, 0.0, rounding) >= 12.0
    # a layer's margin is its worst neuron's
    two = layers.sign_layer([[1, 1, -1, -1], [1, 1, 1, 1]], [T(F(1, 20))] * 2, inputs=(F(-1, 10), F(1, 10)))
    m = two.neuron_margins(V, sigma_delta, rounding)
    assert two.margin(V, sigma_delta, rounding) == min(m) and m[1] < m[0]
