"""The rotation by an encrypted amount and the coefficient-level lookup (include/ieache.h section 3h) without a GPU: the C references
ieache_tlwe_rotate_reference / ieache_lut_read_reference against the numpy restatement (rotate_reference.py) word for word, three
steps against the untouched oracle's blind_rotate_step, single steps and a 4 096-coefficient table by meaning at the product
parameters, the refusals that need no device (output overlap and a set of another context need one: tests/test_rotate_gpu.py),
the declarations, and the C references in a stand-alone program under AddressSanitizer + UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cmux_reference as CR
import rotate_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def params(ia, N, l, Bgbit, n=4):
    return ia.default_params().copy(n=n, N=N, l=l, Bgbit=Bgbit)


def torus_distance(a, b):
    d = (np.asarray(a, dtype=np.int64) - np.asarray(b, dtype=np.int64)) & 0xFFFFFFFF
    return np.minimum(d, (1 << 32) - d).astype(np.float64) / 2.0 ** 32


@pytest.mark.parametrize("N", [64, 1024])
@pytest.mark.parametrize("l,Bgbit", [(3, 7), (2, 10)])
def test_reference_is_the_definition_word_for_word(ia, N, l, Bgbit):
    """Full-range random words; steps 0, 1, 3; selectors implied and explicit with repeats and the last index; amounts default and
    explicit; the lookup at (depth, steps) = (1, 2) against its restatement, with and without the key switch."""
    from ieache_amd import tools
    p = params(ia, N, l, Bgbit)
    rng = np.random.default_rng(9800 + N + 100 * l + Bgbit)
    n = 3
    S = CR.full_range(rng, (n, 2 * l, 2, N))
    rows = CR.full_range(rng, (2, 2, N))
    for steps in (0, 1, 3):
        sel = rng.integers(0, n, size=(2, max(steps, 1))).astype(np.int32)
        sel[-1, :] = n - 1
        am = rng.integers(0, 2 * N, size=steps).astype(np.int32)
        for so in (None, sel):
            for a in (None, am):
                got = tools.tlwe_rotate_reference(p, S, rows, steps, sel_of=so, amounts=a)
                assert got.shape == (2, 2, N) and got.dtype == np.int32
                assert np.array_equal(got, RR.tlwe_rotate(S, rows, steps, l, Bgbit, sel_of=so, amounts=a)), (steps, so is None, a is None)
    assert np.array_equal(tools.tlwe_rotate_reference(p, S, rows, 0), rows)
    assert tools.tlwe_rotate_reference(p, S, rows[:0], 2).shape == (0, 2, N)
    # the default amounts are what rotate_amounts names
    assert np.array_equal(tools.tlwe_rotate_reference(p, S, rows, 3), tools.tlwe_rotate_reference(p, S, rows, 3, amounts=tools.rotate_amounts(3, N=N)))
    tables = CR.full_range(rng, (2, 2, 2, N))
    ksk = CR.full_range(rng, (N, p.ks_t, 1 << p.ks_basebit, p.n + 1))
    sel = np.array([[2, 0, 1], [1, 1, 2]], dtype=np.int32)
    for so in (None, sel):
        kw = dict(sel_of=so, table_of=[1, 0], coef=5, count=2)
        got = tools.lut_read_reference(p, S, tables, 1, 2, **kw)
        assert got.shape == (2, N + 1) and np.array_equal(got, RR.lut_read(S, tables, 1, 2, l, Bgbit, **kw))
        got = tools.lut_read_reference(p, S, tables, 1, 2, ksk=ksk, **kw)
        assert got.shape == (2, p.n + 1) and np.array_equal(got, RR.lut_read(S, tables, 1, 2, l, Bgbit, ksk=ksk, ks=(p.ks_t, p.ks_basebit), **kw))


@pytest.mark.parametrize("kw", [{}, {"l": 2, "Bgbit": 10}], ids=["l3_Bg7", "l2_Bg10"])
def test_three_steps_are_three_blind_rotation_steps_of_the_oracle(ia, make_keys, kw):
    """The independent pin: with the set = rows bk[i] of a seeded key, a 3-step rotation IS oracle.blind_rotate_step three times."""
    from ieache_amd import tools
    kb = make_keys(4, 1024, **kw)
    N = kb.p.N
    acc = CR.full_range(np.random.default_rng(9810), (2, N))
    for sel, am in (([0, 1, 2], [1, N + 3, 2 * N - 1]), ([3, 3, 1], [N, 0, 77])):
        want = acc
        for i, a in zip(sel, am):
            want = kb.ck.blind_rotate_step(want, i, a)  # the step of amount 0 included: the oracle leaves the accumulator as it is
        assert np.array_equal(tools.tlwe_rotate_reference(kb.p, kb.bk, acc, 3, sel_of=[sel], amounts=am)[0], want), (sel, am)
    assert np.array_equal(kb.ck.blind_rotate_step(acc, 2, 0), acc)


def test_single_steps_by_meaning(ia, make_keys):
    """Amounts 0, 1, N - 1, N, N + 1, 2N - 1 as single steps at (3, 7): with the selector an encryption of 1 the phase is the
    input's shifted and negated as X^a says, with an encryption of 0 it is unchanged, each within 2^-8."""
    from ieache_amd import tools
    kb = make_keys(4, 1024)
    p, N = kb.p, 1024
    msg = ((np.arange(N, dtype=np.int64) * 0x9E3779B1 + 12345) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    sample = tools.tlwe_encrypt(p, kb.tlwe_key, msg, 301)
    bits = tools.tgsw_encrypt(p, kb.tlwe_key, [0, 1], 302)
    for a in (0, 1, N - 1, N, N + 1, 2 * N - 1):
        for b in (0, 1):
            got = tools.tlwe_rotate_reference(p, bits, sample, 1, sel_of=[[b]], amounts=[a])
            want = RR.monomial(msg, a) if b else msg
            err = torus_distance(tools.tlwe_phase(p, kb.tlwe_key, got)[0], want).max()
            assert err < 2.0 ** -8, (a, b, err)


ADDRESSES = (0, 4095, 1686, 2561)
_table = {}


def packed_table(p, tlwe_key):
    """The by-meaning case, made once and left unchanged: a client-encrypted table of 4 samples with distinct messages on all
    1 024 coefficients, and for each of the addresses 0, all-ones and two others its 12 bits as FRESH TGSW samples (bit t of the
    address at index t: the 10 coefficient bits first, then the 2 sample bits).
    -> dict(msg [4][N], table [4][2][N], samples [48][2l][2][N], sel_of [4][12], rows = lut_read_reference without key switch)"""
    from ieache_amd import tools
    key = np.asarray(tlwe_key).tobytes()
    if key not in _table:
        N = p.N
        msg = ((np.arange(4 * N, dtype=np.int64) * 0x9E3779B1 + 7) & 0xFFFFFFFF).astype(np.uint32).view(np.int32).reshape(4, N)
        assert len(set(msg.ravel().tolist())) == 4 * N
        table = tools.tlwe_encrypt(p, tlwe_key, msg, 311)
        samples = tools.tgsw_encrypt(p, tlwe_key, [(a >> t) & 1 for a in ADDRESSES for t in range(12)], 312)
        sel_of = np.arange(48, dtype=np.int32).reshape(4, 12)
        rows = tools.lut_read_reference(p, samples, table, 2, 10, sel_of=sel_of, count=4)
        _table[key] = dict(msg=msg, table=table, samples=samples, sel_of=sel_of, rows=rows)
    return _table[key]


def lwe_phase(lwe_key, rows):
    rows = np.asarray(rows, dtype=np.int64)
    return ((rows[:, -1] - rows[:, :-1] @ np.asarray(lwe_key, dtype=np.int64)) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def test_packed_table_lookup_at_the_product_parameters(ia, make_keys):
    """N = 1024, l = 3, Bgbit = 7, noise 2^-25: depth 2 and steps 10 address every one of 4 096 coefficients; for the addresses 0,
    4095 and two others the phase of the extracted row is the addressed coefficient's message within 2^-8, the project's
    decoding condition (DESIGN.md section 7 derives 1.44e-3 of ramp plus 5 sigma = 1.5e-3 for the 12 products; this table gives
    the figures profiles/rotate_rates.txt records).  Through the key switch the condition is a gate input's, 1/8.  Not run at
    (2, 10): section 7's stated limit."""
    from ieache_amd import tools
    kb = make_keys(4, 1024)
    p = kb.p
    assert (p.N, p.l, p.Bgbit) == (1024, 3, 7) and p.tlwe_alpha_min == 2.0 ** -25
    T = packed_table(p, kb.tlwe_key)
    want = np.array([T["msg"][a >> 10, a & 1023] for a in ADDRESSES])
    # an extracted row is an LWE sample under the ring key: phase = b - <a, key>
    err = torus_distance(lwe_phase(kb.tlwe_key, T["rows"]), want)
    print("depth 2 + steps 10 lookup at addresses %s: phase errors %s, largest %.3e (bound 2^-8 = %.3e)"
          % (ADDRESSES, " ".join("%.3e" % e for e in err), err.max(), 2.0 ** -8))
    assert err.max() < 2.0 ** -8
    # the same rows are the stages composed by hand
    picked = tools.lut_tree_reference(p, T["samples"], T["table"], 2, sel_of=T["sel_of"][:, 10:], table_of=[0] * 4)
    turned = tools.tlwe_rotate_reference(p, T["samples"], picked, 10, sel_of=T["sel_of"][:, :10])
    assert np.array_equal(tools.tlwe_extract_reference(p, turned), T["rows"])
    assert torus_distance(tools.tlwe_phase(p, kb.tlwe_key, turned)[:, 0], want).max() < 2.0 ** -8
    # one case with the key switch on
    lwe = tools.lut_read_reference(p, T["samples"], T["table"], 2, 10, sel_of=T["sel_of"][2:3], ksk=kb.ksk)
    assert lwe.shape == (1, p.n + 1) and torus_distance(lwe_phase(kb.lwe_key, lwe), want[2:3]).max() < 1 / 8


def refused(ia, match, f, *a, **kw):
    with pytest.raises(ia.IeacheError, match=match) as e:
        f(*a, **kw)
    assert e.value.code == -22


def test_refusals_without_a_device(ia):
    from ieache_amd import tools
    from ieache_amd.evaluator import _i32, check
    p = params(ia, 16, 3, 7)
    S = np.zeros((2, 6, 2, 16), dtype=np.int32)
    v = np.zeros((2, 2, 16), dtype=np.int32)
    t = np.zeros((1, 2, 2, 16), dtype=np.int32)
    assert tools.tlwe_rotate_reference(p, S, v, 2, sel_of=[[1, 0], [0, 1]], amounts=[31, 0]).shape == (2, 2, 16)
    refused(ia, r"amount_of\[1\] = 32", tools.tlwe_rotate_reference, p, S, v, 2, amounts=[31, 32])
    refused(ia, r"amount_of\[0\] = -1", tools.tlwe_rotate_reference, p, S, v, 2, amounts=[-1, 32])
    refused(ia, r"sel_of\[1\] = 2", tools.tlwe_rotate_reference, p, S, v, 2, sel_of=[[1, 2], [0, 0]])
    refused(ia, r"sel_of\[2\] = -1", tools.tlwe_rotate_reference, p, S, v, 2, sel_of=[[1, 0], [-1, 0]])
    refused(ia, "steps", tools.tlwe_rotate_reference, p, S, v, 65)
    refused(ia, "steps", tools.tlwe_rotate_reference, p, S, v, -1)
    refused(ia, "unsupported", tools.tlwe_rotate_reference, p.copy(N=8), S, v, 1)
    assert tools.tlwe_rotate_reference(p, S, v, 64).shape == (2, 2, 16)
    refused(ia, r"sel_of\[3\] = 2", tools.lut_read_reference, p, S, t, 1, 2, sel_of=[[1, 0, 0], [2, 0, 0]])
    refused(ia, r"amount_of\[0\] = 32", tools.lut_read_reference, p, S, t, 1, 1, amounts=[32])
    refused(ia, r"table_of\[0\] = 1", tools.lut_read_reference, p, S, t, 1, 1, table_of=[1])
    refused(ia, r"coef\[0\] = 16", tools.lut_read_reference, p, S, t, 1, 1, coef=16)
    refused(ia, "steps", tools.lut_read_reference, p, S, t, 1, 65)
    L, pc, out = ia.lib(), C.byref(p), np.zeros((1, 17), dtype=np.int32)
    refused(ia, "depth", lambda: check(L.ieache_lut_read_reference(pc, _i32(S), 2, None, 1, 13, 1, None, None, _i32(t), 1, None, 0, 1, _i32(out))))
    refused(ia, "no samples", lambda: check(L.ieache_tlwe_rotate_reference(pc, _i32(S), 0, 1, 1, None, None, _i32(v), _i32(v))))
    refused(ia, "null", lambda: check(L.ieache_tlwe_rotate_reference(pc, _i32(S), 2, 1, 1, None, None, None, _i32(v))))
    refused(ia, "needs ksk", lambda: check(L.ieache_lut_read_reference(pc, _i32(S), 2, None, 1, 1, 1, None, None, _i32(t), 1, None, 0, 0, _i32(out))))
    refused(ia, "unknown flag", lambda: check(L.ieache_lut_read_reference(pc, _i32(S), 2, None, 1, 1, 1, None, None, _i32(t), 1, None, 0, 2, _i32(out))))


def test_rotate_amounts():
    from ieache_amd import tools
    assert tools.rotate_amounts(12).tolist() == [2047, 2046, 2044, 2040, 2032, 2016, 1984, 1920, 1792, 1536, 1024, 0]
    assert tools.rotate_amounts(4, toward_zero=False).tolist() == [1, 2, 4, 8]
    assert tools.rotate_amounts(3, unit=4).tolist() == [2044, 2040, 2032] and tools.rotate_amounts(2, unit=3, toward_zero=False, N=16).tolist() == [3, 6]
    assert tools.rotate_amounts(0).shape == (0,) and tools.rotate_amounts(3).dtype == np.int32


def test_references_under_asan_ubsan(tmp_path):
    """tlwe_rotate_reference / lut_read_reference of csrc/tfhe_host.cpp in a stand-alone program
    (tests/native/rotate_reference_test.cpp): exact-size buffers, a 2-step rotation at N = 64 against a schoolbook product,
    the boundary amounts, in place, both defaults, the lookup against its stages."""
    csrc = os.path.join(ROOT, "ie-ache_amd", "csrc")
    exe = tmp_path / "rotate_reference_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I", csrc, os.path.join(ROOT, "tests", "native", "rotate_reference_test.cpp"),
                           os.path.join(csrc, "tfhe_host.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "ROTATE_REFERENCE_OK" in r.stdout, r.stdout[-4000:]


# name -> number of parameters as include/ieache.h declares them (all return int)
DECLARED = {"ieache_tlwe_rotate": 9, "ieache_tlwe_rotate_device": 9, "ieache_tlwe_rotate_reference": 9,
            "ieache_lut_read": 14, "ieache_lut_read_device": 14, "ieache_lut_read_reference": 15}


def test_every_symbol_is_declared_exported_and_bound(ia):
    with open(os.path.join(ROOT, "include", "ieache.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = {m.group(1): m.group(2) for m in re.finditer(r"^int\s+(ieache_(?:tlwe_rotate|lut_read)[a-z_]*)\s*\(([^;]*)\)\s*;", hdr, re.M)}
    assert set(declared) == set(DECLARED)
    raw, L = C.CDLL(ia.library_path()), ia.lib()
    for name, n_params in DECLARED.items():
        assert len(declared[name].split(",")) == n_params, name
        assert hasattr(raw, name), name
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n_params, name  # the binding passes what the header declares
    assert len(L.ieache_tlwe_rotate.argtypes) == len(L.ieache_tlwe_rotate_device.argtypes)
    assert len(L.ieache_lut_read.argtypes) == len(L.ieache_lut_read_device.argtypes)
    for name in ("tlwe_rotate", "tlwe_rotate_device", "lut_read", "lut_read_device"):
        assert callable(getattr(ia.Context, name)), name
    from ieache_amd import tools
    assert callable(tools.tlwe_rotate_reference) and callable(tools.lut_read_reference)
    assert ia.ROTATE_MAX_STEPS == 64 and ia.LUT_READ_NO_KEYSWITCH == 1
