"""The unpacking key switch and the read of an addressed word (include/ieache.h section 3m) without a GPU: the C references
(ieache_unpack_reference, ieache_word_read_reference) against the numpy restatement (unpack_reference.py) word for word and
against the references they are composed of, the window rule and the cut (csrc/unpack_plan.h) in a stand-alone program under
AddressSanitizer + UBSan, the symbols, the refusals, and the read by meaning at the product parameters.

The by-meaning table holds bits as +-1/8, the gate encoding: a read row decrypts right while its phase stays within 1/8 of its
message, and the test prints how far the reference's rows come from that."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cmux_reference as CR
import unpack_reference as UR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLARED = {"ieache_unpack": 9, "ieache_unpack_device": 9, "ieache_unpack_reference": 9, "ieache_word_read": 14, "ieache_word_read_device": 14,
            "ieache_word_read_reference": 15}
WINDOWS_1024 = [(0, 1, 1), (1023, 1, 1), (0, 1024, 1), (3, 5, 200), (511, 2, 512), (0, 64, 1)]


def torus_distance(a, b):
    d = (np.asarray(a, dtype=np.int64) - np.asarray(b, dtype=np.int64)) & 0xFFFFFFFF
    return np.minimum(d, (1 << 32) - d).astype(np.float64) / 2.0 ** 32


def test_every_symbol_is_declared_exported_and_bound(ia):
    with open(os.path.join(ROOT, "include", "ieache.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = {m.group(1): m.group(2) for m in re.finditer(r"^int\s+(ieache_(?:unpack|word_read)[a-z_]*)\s*\(([^;]*)\)\s*;", hdr, re.M)}
    assert set(declared) == set(DECLARED)
    raw, L = C.CDLL(ia.library_path()), ia.lib()
    for name, n_params in DECLARED.items():
        assert len(declared[name].split(",")) == n_params, name
        assert hasattr(raw, name), name
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n_params, name  # the binding passes what the header declares
    for name in ("unpack", "unpack_device", "word_read", "word_read_device"):
        assert callable(getattr(ia.Context, name)), name
    from ieache_amd import tools
    assert callable(tools.unpack_reference) and callable(tools.word_read_reference)
    assert ia.UNPACK_NO_KEYSWITCH == 1 and "#define IEACHE_UNPACK_NO_KEYSWITCH 1" in hdr


def toy_windows(N):
    return [(0, 1, 1), (N - 1, 1, 1), (0, N, 1), (3, 3, 5), (N // 2 - 1, 2, N // 2), (1, N // 4, 3)]


@pytest.mark.parametrize("N,t,b", [(16, 8, 2), (64, 8, 2), (64, 5, 3)])
def test_unpack_reference_is_the_definition_on_toy_rings(ia, N, t, b):
    from ieache_amd import tools
    p = ia.default_params().copy(n=5, N=N, ks_t=t, ks_basebit=b)
    rng = np.random.default_rng(13000 + N + 10 * t + b)
    ksk = CR.full_range(rng, (N, t, 1 << b, p.n + 1))
    samples = CR.full_range(rng, (3, 2, N))
    for first, width, spread in toy_windows(N):
        u = tools.unpack_reference(p, samples, first, width, spread)
        assert u.shape == (3, width, N + 1) and np.array_equal(u, UR.window_rows(samples, first, width, spread)), (first, width, spread)
        got = tools.unpack_reference(p, samples, first, width, spread, ksk=ksk)
        assert got.shape == (3, width, p.n + 1) and np.array_equal(got, UR.unpack(samples, first, width, spread, ksk=ksk, ks=(t, b))), (first, width, spread)
        # the definition spelled out: tlwe_extract_reference of each coefficient, then the key switch lut_read_reference uses --
        # the lookup of depth = steps = 0 over the sample as its one table
        for q in range(width):
            coef = np.full(3, first + q * spread, dtype=np.int32)
            assert np.array_equal(u[:, q], tools.tlwe_extract_reference(p, samples, coef))
        for i in range(3):
            S = CR.full_range(rng, (1, 2 * p.l, 2, N))
            for q in (0, width - 1):
                row = tools.lut_read_reference(p, S, samples[i:i + 1], 0, 0, coef=first + q * spread, ksk=ksk, count=1)
                assert np.array_equal(got[i, q], row[0])
    assert tools.unpack_reference(p, samples[:0], 0, 1, 1, ksk=ksk).shape == (0, 1, p.n + 1)


def test_unpack_reference_at_1024(ia):
    from ieache_amd import tools
    p = ia.default_params().copy(n=6)
    N = p.N
    rng = np.random.default_rng(13100)
    ksk = CR.full_range(rng, (N, p.ks_t, 1 << p.ks_basebit, p.n + 1))
    samples = CR.full_range(rng, (2, 2, N))
    for first, width, spread in WINDOWS_1024:
        keep = sorted({0, width // 2, width - 1})  # the walk in numpy is slow: the whole window extracted, three rows of it switched
        u = tools.unpack_reference(p, samples, first, width, spread)
        assert np.array_equal(u, UR.window_rows(samples, first, width, spread)), (first, width, spread)
        got = tools.unpack_reference(p, samples, first, width, spread, ksk=ksk)
        assert np.array_equal(got[:, keep], UR.keyswitch(ksk, p.ks_t, p.ks_basebit, u[:, keep])), (first, width, spread)


def read_case(rng, p, n_set, n_tables, depth):
    return CR.full_range(rng, (n_set, 2 * p.l, 2, p.N)), CR.full_range(rng, (n_tables, 1 << depth, 2, p.N))


@pytest.mark.parametrize("N", [16, 64])
def test_word_read_reference_is_the_composition_on_toy_rings(ia, N):
    """depth 0, 2 x steps 0, 2 x (width, unit) (1, 1), (3, 4) x counts 1, 3; selectors implied and explicit; two tables."""
    from ieache_amd import tools
    p = ia.default_params().copy(n=5, N=N)
    rng = np.random.default_rng(13200 + N)
    ksk = CR.full_range(rng, (N, p.ks_t, 1 << p.ks_basebit, p.n + 1))
    at = 0
    for depth in (0, 2):
        for steps in (0, 2):
            for width, unit in ((1, 1), (3, 4)):
                for count in (1, 3):
                    S, tables = read_case(rng, p, 5, 2, depth)
                    sel = rng.integers(0, 5, size=(count, max(depth + steps, 1))).astype(np.int32) if at % 2 else None
                    tof = rng.integers(0, 2, size=count).astype(np.int32) if at % 3 else None
                    at += 1
                    kw = dict(sel_of=sel, table_of=tof, count=count)
                    got = tools.word_read_reference(p, S, tables, depth, steps, width=width, unit=unit, ksk=ksk, **kw)
                    want = UR.word_read(S, tables, depth, steps, width, unit, p.l, p.Bgbit, ksk=ksk, ks=(p.ks_t, p.ks_basebit), **kw)
                    assert got.shape == (count, width, p.n + 1) and np.array_equal(got, want), (depth, steps, width, unit, count)
                    rows = tools.word_read_reference(p, S, tables, depth, steps, width=width, unit=unit, **kw)
                    assert rows.shape == (count, width, N + 1) and np.array_equal(rows, UR.word_read(S, tables, depth, steps, width, unit, p.l, p.Bgbit, **kw))
                    # width 1 is lut_read with coef 0 and the amounts 2N - unit 2^t
                    one = tools.word_read_reference(p, S, tables, depth, steps, width=1, unit=unit, ksk=ksk, **kw)
                    look = tools.lut_read_reference(p, S, tables, depth, steps, amounts=tools.rotate_amounts(steps, unit=unit, N=N), coef=0, ksk=ksk, **kw)
                    assert np.array_equal(one[:, 0], look) and np.array_equal(one[:, 0], got[:, 0])


def test_word_read_reference_at_1024(ia):
    from ieache_amd import tools
    p = ia.default_params().copy(n=6)
    N = p.N
    rng = np.random.default_rng(13300)
    ksk = CR.full_range(rng, (N, p.ks_t, 1 << p.ks_basebit, p.n + 1))
    S, tables = read_case(rng, p, 3, 1, 1)
    sel = np.array([[2, 0, 1], [1, 1, 0]], dtype=np.int32)
    got = tools.word_read_reference(p, S, tables, 1, 2, width=3, unit=4, sel_of=sel, ksk=ksk)
    assert np.array_equal(got, UR.word_read(S, tables, 1, 2, 3, 4, p.l, p.Bgbit, sel_of=sel, count=2, ksk=ksk, ks=(p.ks_t, p.ks_basebit)))
    look = tools.lut_read_reference(p, S, tables, 1, 2, sel_of=sel, amounts=tools.rotate_amounts(2, unit=4, N=N), coef=0, ksk=ksk)
    assert np.array_equal(got[:, 0], look)


def refused(ia, match, f, *a, **kw):
    with pytest.raises(ia.IeacheError, match=match) as e:
        f(*a, **kw)
    assert e.value.code == -22


def test_refusals(ia):
    """Each bound at its last accepted and its first refused value, for both references."""
    from ieache_amd import tools
    p = ia.default_params().copy(n=5, N=16)
    rng = np.random.default_rng(13400)
    ksk = CR.full_range(rng, (16, p.ks_t, 1 << p.ks_basebit, 6))
    S, tables = read_case(rng, p, 3, 2, 1)
    un = lambda first, width, spread, **kw: tools.unpack_reference(p, tables[0], first, width, spread, ksk=ksk, **kw)
    assert un(15, 1, 1).shape == (2, 1, 6) and un(0, 16, 1).shape == (2, 16, 6) and un(7, 2, 8).shape == (2, 2, 6)
    refused(ia, "first must", un, -1, 1, 1)
    refused(ia, "first must", un, 16, 1, 1)
    refused(ia, "width must", un, 0, 0, 1)
    refused(ia, "spread must", un, 0, 1, 0)
    refused(ia, "below N", un, 0, 17, 1)
    refused(ia, "below N", un, 8, 2, 8)
    refused(ia, "below N", un, 15, 2, 1)
    refused(ia, "unsupported", tools.unpack_reference, p.copy(N=8), np.zeros((1, 2, 8), dtype=np.int32), 0, 1, 1)
    L = ia.lib()
    out = np.zeros((2, 1, 17), dtype=np.int32)
    flat = np.ascontiguousarray(tables[0])
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.ieache_unpack_reference(C.byref(p), None, 2, 0, 1, 1, i32(flat), 2, i32(out)) == -22 and "unknown flag" in L.ieache_last_error().decode()
    assert L.ieache_unpack_reference(C.byref(p), None, 2, 0, 1, 1, i32(flat), 0, i32(out)) == -22 and "needs ksk" in L.ieache_last_error().decode()
    rd = lambda depth, steps, width, unit, sel=None, tof=None, **kw: tools.word_read_reference(
        p, S, tables[:, :1 << max(min(depth, 1), 0)] if depth <= 1 else np.zeros((2, 1 << depth, 2, 16), dtype=np.int32), depth, steps, width=width,
        unit=unit, sel_of=sel, table_of=tof, ksk=ksk, **kw)
    assert rd(1, 2, 4, 4).shape == (1, 4, 6) and rd(0, 4, 1, 1).shape == (1, 1, 6) and rd(0, 0, 16, 16).shape == (1, 16, 6)
    refused(ia, "word_read: unit must be at least width", rd, 1, 0, 4, 3)
    refused(ia, "word_read: unit x 2\\^steps must not exceed N", rd, 1, 3, 4, 4)
    refused(ia, "must not exceed N", rd, 0, 5, 1, 1)
    refused(ia, "must not exceed N", rd, 0, 0, 17, 17)
    refused(ia, "word_read: width must", rd, 1, 0, 0, 1)
    refused(ia, "word_read: depth must", rd, -1, 0, 1, 1)
    refused(ia, "depth must", rd, 13, 0, 1, 1)
    refused(ia, "word_read: steps must", rd, 0, -1, 1, 1)
    refused(ia, "steps must", rd, 0, 65, 1, 1)
    refused(ia, r"word_read: sel_of\[1\] = 3", rd, 1, 1, 1, 1, sel=np.array([[0, 3]], dtype=np.int32))
    refused(ia, r"sel_of\[0\] = -1", rd, 1, 1, 1, 1, sel=np.array([[-1, 0]], dtype=np.int32))
    refused(ia, r"word_read: table_of\[0\] = 2", rd, 1, 1, 1, 1, tof=np.array([2], dtype=np.int32))


def test_unpack_plan_under_asan_ubsan(tmp_path):
    """tests/native/unpack_plan_test.cpp: a stand-alone program over csrc/unpack_plan.h, run as its own executable."""
    exe = tmp_path / "unpack_plan_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "native", "unpack_plan_test.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "UNPACK_PLAN_OK" in r.stdout, r.stdout[-4000:]


# ---- by meaning, at the product parameters ----
WORDS = dict(depth=2, steps=6, width=16, unit=16, addrs=[(2, 37), (3, 63), (0, 0), (1, 5)])
_table = {}


def word_table(p, tlwe_key):
    """The scenario, made once and left unchanged: a client-encrypted table of 4 samples x 64 sixteen-bit words, bit b of a word
    at +-1/8 on coefficient 16 word + b, and the address bits of the reads as ONE set of TGSW samples, selectors laid out
    [steps low bits][depth high bits].  -> dict(depth, steps, width, unit, addrs, clear [4][64], tables [1][4][2][N], samples,
    sel_of [reads][8])"""
    from ieache_amd import tools
    key = np.asarray(tlwe_key).tobytes()
    if key not in _table:
        depth, steps, width, unit, addrs = (WORDS[k] for k in ("depth", "steps", "width", "unit", "addrs"))
        N, bits = p.N, depth + steps
        assert unit << steps == N
        rng = np.random.default_rng(13500)
        clear = rng.integers(0, 1 << 16, size=(1 << depth, 1 << steps))
        plain = np.zeros((1 << depth, N), dtype=np.int64)
        for b in range(width):
            plain[:, b::unit] = np.where((clear >> b) & 1, 1 << 29, -(1 << 29))
        tables = tools.tlwe_encrypt(p, tlwe_key, UR.wrap32(plain), 91)[None]
        flat = [slot << steps | word for slot, word in addrs]
        samples = tools.tgsw_encrypt(p, tlwe_key, [(a >> s) & 1 for a in flat for s in range(bits)], 92)
        sel_of = np.arange(len(addrs) * bits, dtype=np.int32).reshape(len(addrs), bits)
        _table[key] = dict(depth=depth, steps=steps, width=width, unit=unit, addrs=addrs, clear=clear, tables=tables, samples=samples, sel_of=sel_of)
    return _table[key]


def lwe_phase(lwe_key, rows):
    rows = np.asarray(rows, dtype=np.int32)
    return UR.wrap32(rows[..., -1].astype(np.int64) - (rows[..., :-1].astype(np.int64) * np.asarray(lwe_key, dtype=np.int64)).sum(axis=-1))


def word_of(bits):
    return sum(int(b) << i for i, b in enumerate(bits))


def worst_phase_error(lwe_key, rows, word):
    want = np.array([(1 << 29) if (word >> b) & 1 else -(1 << 29) for b in range(rows.shape[0])], dtype=np.int64)
    return torus_distance(lwe_phase(lwe_key, rows), UR.wrap32(want)).max()


def test_word_read_by_meaning(ia, make_keys):
    """n = 630, (3, 7): four words read at encrypted (slot, word) addresses through the C reference; every decrypted word is the
    clear one."""
    from ieache_amd import tools
    kb = make_keys(630, 1024)
    p = kb.p
    assert (p.N, p.l, p.Bgbit, p.ks_t, p.ks_basebit) == (1024, 3, 7, 8, 2)
    sc = word_table(p, kb.tlwe_key)
    got = tools.word_read_reference(p, sc["samples"], sc["tables"], sc["depth"], sc["steps"], width=sc["width"], unit=sc["unit"], sel_of=sc["sel_of"],
                                    ksk=kb.ksk)
    assert got.shape == (len(sc["addrs"]), 16, p.n + 1)
    for i, (slot, word) in enumerate(sc["addrs"]):
        clear = int(sc["clear"][slot, word])
        print("read %d at slot %d word %d: largest distance of a row's phase from +-1/8: %.3e (a wrong bit needs 1/8 = 1.25e-01)"
              % (i, slot, word, worst_phase_error(kb.lwe_key, got[i], clear)))
        assert word_of(kb.dec(got[i])) == clear, (slot, word)
