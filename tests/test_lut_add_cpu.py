"""Many values into shared memories (include/ieache.h section 3j) without a GPU: the C reference ieache_lut_add_reference against
the numpy restatement (lut_add_reference.py) and against the three existing C references composed, one item against
lut_scatter_reference, the conservation of the leaves, every refusal, the declarations, two tallies at the product
parameters by meaning, and the C reference in a stand-alone program under AddressSanitizer + UBSan.

No planning code was added (csrc/cmux_plan.h's tree plan for (count, depth) is the cut, unchanged), so there is no native
program for a plan here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cmux_reference as CR
import lut_add_reference as AR
import scatter_reference as SR
from test_scatter_cpu import params, refused, torus_distance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLARED = {"ieache_lut_add": 13, "ieache_lut_add_device": 13, "ieache_lut_add_reference": 13}


def composed(tools, p, S, v, depth, steps, sel_of=None, amounts=None, mems=None, n_mems=1, mem_of=None):
    """the definition written out with the three existing C references: tlwe_rotate, lut_scatter with no memory, a sum"""
    count, n, stride = len(v), len(S), depth + steps
    if sel_of is None:
        of = (np.arange(count * stride) % n).astype(np.int32).reshape(count, stride)
    else:
        of = np.asarray(sel_of, dtype=np.int32)
    am = tools.rotate_amounts(steps, toward_zero=False, N=p.N) if amounts is None else amounts
    w = tools.tlwe_rotate_reference(p, S, v, steps, sel_of=of[:, :steps] if steps else None, amounts=am) if steps else v
    leaves = tools.lut_scatter_reference(p, S, w, depth, sel_of=of[:, steps:steps + depth] if depth else None)
    out = np.zeros((n_mems, 1 << depth, 2, p.N), dtype=np.int32) if mems is None else np.array(mems, dtype=np.int32)
    for i in range(count):
        m = 0 if mem_of is None else int(mem_of[i])
        out[m] = SR.add32(out[m], leaves[i])
    return out


@pytest.mark.parametrize("l,Bgbit", [(3, 7), (2, 10), (6, 5)])
def test_reference_is_the_definition_word_for_word(ia, l, Bgbit):
    """N = 64, full-range words: depth 0 .. 2 x steps 0 and 3, 1 and 3 items, one and two memories, every optional argument given
    and left out; against the numpy restatement and against the existing references composed."""
    from ieache_amd import tools
    N, n = 64, 4
    p = params(ia, N, l, Bgbit)
    rng = np.random.default_rng(9800 + 10 * l + Bgbit)
    S = CR.full_range(rng, (n, 2 * l, 2, N))
    for depth in range(3):
        for steps in (0, 3):
            for count in (1, 3):
                v = CR.full_range(rng, (count, 2, N))
                mems = CR.full_range(rng, (2, 1 << depth, 2, N))
                sel = rng.integers(0, n, size=(count, max(depth + steps, 1))).astype(np.int32)
                am = rng.integers(0, 2 * N, size=steps).astype(np.int32)
                mof = np.array([1, 0, 1][:count], dtype=np.int32)
                for kw in (dict(), dict(sel_of=sel), dict(mems=mems[:1]), dict(sel_of=sel, amounts=am, mems=mems, mem_of=mof), dict(n_mems=2, mem_of=mof)):
                    got = tools.lut_add_reference(p, S, v, depth, steps, **kw)
                    n_mems = 2 if "mem_of" in kw else 1
                    assert got.shape == (n_mems, 1 << depth, 2, N) and got.dtype == np.int32
                    assert np.array_equal(got, AR.lut_add(S, v, depth, steps, l, Bgbit, **kw)), (depth, steps, count, sorted(kw))
                    assert np.array_equal(got, composed(tools, p, S, v, depth, steps, **kw)), (depth, steps, count, sorted(kw))
    # no items: the memories unchanged, zeros for none
    assert np.array_equal(tools.lut_add_reference(p, S, v[:0], 2, 1, mems=mems), mems)
    assert not tools.lut_add_reference(p, S, v[:0], 2, 1, n_mems=3).any()


@pytest.mark.parametrize("l,Bgbit", [(3, 7), (2, 10)])
def test_one_item_conservation_and_in_place_at_n1024(ia, l, Bgbit):
    """For ANY words at N = 1024: one item with steps = 0 is lut_scatter_reference bit for bit; steps > 0 with depth 0 is the
    rotation plus the memory; the leaves are conserved -- sum_j out[m][j] - sum_j mems[m][j] is the sum of the rotated values
    sent to m, word for word; out may be mems."""
    from ieache_amd import tools
    N = 1024
    p = params(ia, N, l, Bgbit)
    rng = np.random.default_rng(9810 + l)
    S = CR.full_range(rng, (3, 2 * l, 2, N))
    v = CR.full_range(rng, (3, 2, N))
    mems = CR.full_range(rng, (2, 4, 2, N))
    sel = np.array([[2, 0, 1, 1], [1, 1, 0, 2], [0, 2, 2, 0]], dtype=np.int32)
    one = tools.lut_add_reference(p, S, v[:1], 2, 0, sel_of=sel[:1, :2], mems=mems[:1])
    assert np.array_equal(one, tools.lut_scatter_reference(p, S, v[:1], 2, sel_of=sel[:1, :2], mem=mems[:1]))
    am = tools.rotate_amounts(2, toward_zero=False, N=N)
    turned = tools.tlwe_rotate_reference(p, S, v, 2, sel_of=sel[:, :2], amounts=am)
    assert np.array_equal(tools.lut_add_reference(p, S, v[:1], 0, 2, sel_of=sel[:1, :2], mems=mems[:1, :1]), SR.add32(mems[:1, :1], turned[:1, None]))
    mof = np.array([1, 0, 1], dtype=np.int32)
    out = tools.lut_add_reference(p, S, v, 2, 2, sel_of=sel, mems=mems, mem_of=mof)
    gained = SR._wrap32(SR.sub32(out, mems).astype(np.int64).sum(axis=1))
    assert np.array_equal(gained[0], turned[1]) and np.array_equal(gained[1], SR.add32(turned[0], turned[2]))
    # depth 0, steps 0: a plain sum
    assert np.array_equal(tools.lut_add_reference(p, S, v, 0, 0, mems=mems[:1, :1])[0, 0], SR._wrap32(v.astype(np.int64).sum(axis=0) + mems[0, 0]))
    from ieache_amd.evaluator import _i32, check
    inplace = mems.copy()
    check(ia.lib().ieache_lut_add_reference(C.byref(p), _i32(S), 3, 3, 2, 2, _i32(sel), None, _i32(v), _i32(inplace), 2, _i32(mof), _i32(inplace)))
    assert np.array_equal(inplace, out)


def test_refusals_without_a_device(ia):
    from ieache_amd import tools
    from ieache_amd.evaluator import _i32, check
    p = params(ia, 16, 3, 7)
    S = np.zeros((2, 6, 2, 16), dtype=np.int32)
    v = np.zeros((2, 2, 16), dtype=np.int32)
    assert tools.lut_add_reference(p, S, v, 1, 2, sel_of=[[1, 0, 1], [0, 1, 0]], amounts=[31, 0], n_mems=2, mem_of=[1, 0]).shape == (2, 2, 2, 16)
    refused(ia, r"lut_add: sel_of\[2\] = 2", tools.lut_add_reference, p, S, v, 1, 2, sel_of=[[1, 0, 2], [0, 0, 0]])
    refused(ia, r"lut_add: sel_of\[3\] = -1", tools.lut_add_reference, p, S, v, 1, 2, sel_of=[[1, 0, 1], [-1, 0, 0]])
    refused(ia, r"lut_add: amount_of\[1\] = 32", tools.lut_add_reference, p, S, v, 1, 2, amounts=[31, 32])
    refused(ia, r"lut_add: amount_of\[0\] = -1", tools.lut_add_reference, p, S, v, 1, 2, amounts=[-1, 0])
    refused(ia, r"lut_add: mem_of\[1\] = 2", tools.lut_add_reference, p, S, v, 1, 0, n_mems=2, mem_of=[1, 2])
    refused(ia, r"lut_add: mem_of\[0\] = -1", tools.lut_add_reference, p, S, v, 1, 0, n_mems=2, mem_of=[-1, 0])
    refused(ia, r"lut_add: mem_of\[0\] = 1", tools.lut_add_reference, p, S, v, 1, 0, mem_of=[1, 0])
    refused(ia, "lut_add: depth", tools.lut_add_reference, p, S, v, -1)
    refused(ia, "lut_add: steps", tools.lut_add_reference, p, S, v, 1, 65)
    refused(ia, "lut_add: steps", tools.lut_add_reference, p, S, v, 1, -1)
    refused(ia, "n_mems must be at least 1", tools.lut_add_reference, p, S, v, 1, 0, n_mems=0)
    refused(ia, "unsupported", tools.lut_add_reference, p.copy(N=8), S, v, 1)
    L, pc, out = ia.lib(), C.byref(p), np.zeros((1, 1, 2, 16), dtype=np.int32)
    refused(ia, "lut_add: depth", lambda: check(L.ieache_lut_add_reference(pc, _i32(S), 2, 1, 13, 0, None, None, _i32(v), None, 1, None, _i32(out))))
    refused(ia, "no samples", lambda: check(L.ieache_lut_add_reference(pc, _i32(S), 0, 1, 0, 0, None, None, _i32(v), None, 1, None, _i32(out))))
    refused(ia, "null", lambda: check(L.ieache_lut_add_reference(pc, _i32(S), 2, 1, 0, 0, None, None, None, None, 1, None, _i32(out))))
    refused(ia, "null", lambda: check(L.ieache_lut_add_reference(pc, _i32(S), 2, 1, 0, 0, None, None, _i32(v), None, 1, None, None)))
    # the two forms that need a context: well-formed arguments get as far as the missing context and set
    refused(ia, "null argument", lambda: check(L.ieache_lut_add(None, None, 1, 0, 0, None, None, _i32(v), None, 1, None, _i32(out), None)))
    refused(ia, "null argument", lambda: check(L.ieache_lut_add_device(None, None, 1, 0, 0, None, None, None, None, 1, None, None, None)))


def test_reference_under_asan_ubsan(tmp_path):
    """lut_add_reference of csrc/tfhe_host.cpp in a stand-alone program (tests/native/lut_add_reference_test.cpp): exact-size
    buffers, l x Bgbit = 32, Bgbit = 1, 64 steps, depth 0, steps 0, every optional array given and null, mems given / null / the
    output itself, no items; the result against the rotation's and the scatter's references summed by hand."""
    csrc = os.path.join(ROOT, "ie-ache_amd", "csrc")
    exe = tmp_path / "lut_add_reference_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I", csrc, os.path.join(ROOT, "tests", "native", "lut_add_reference_test.cpp"),
                           os.path.join(csrc, "tfhe_host.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "LUT_ADD_REFERENCE_OK" in r.stdout, r.stdout[-4000:]


def test_every_symbol_is_declared_exported_and_bound(ia):
    with open(os.path.join(ROOT, "include", "ieache.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = {m.group(1): m.group(2) for m in re.finditer(r"^int\s+(ieache_lut_add[a-z_]*)\s*\(([^;]*)\)\s*;", hdr, re.M)}
    assert set(declared) == set(DECLARED)
    raw, L = C.CDLL(ia.library_path()), ia.lib()
    for name, n_params in DECLARED.items():
        assert len(declared[name].split(",")) == n_params, name
        assert hasattr(raw, name), name
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n_params, name  # the binding passes what the header declares
    assert len(L.ieache_lut_add.argtypes) == len(L.ieache_lut_add_device.argtypes)
    for name in ("lut_add", "lut_add_device"):
        assert callable(getattr(ia.Context, name)), name
    from ieache_amd import tools
    assert callable(tools.lut_add_reference)


# ---- by meaning at the product parameters ----
# Five additions of multiples of 1/64 into memories of client-encrypted zeros, two of the five addresses equal.  The number of
# additions and the addresses are chosen so that DESIGN.md section 7's DERIVED bound already sits within the decoding condition
# tests/test_scatter_gpu.py's last test uses (every coefficient within 2^-8 = 3.9e-3 of what it should hold), before anything
# is run: at (3, 7) and alpha = 2^-25 a product adds key noise sigma = 8.6e-5 and, per selector bit that is 1, a truncation
# ramp of at most 1.2e-4; k additions of depth + steps products each put at most k (depth + steps) products' key noise into a
# slot and, with addresses of at most two 1-bits, at most 2 k ramps:
#   slots:        depth 4, steps 0, k = 5:  10 x 1.2e-4 + 5 sqrt(20) x 8.6e-5 = 1.2e-3 + 1.9e-3 = 3.1e-3 < 3.9e-3
#   coefficients: depth 2, steps 3, k = 5:  10 x 1.2e-4 + 5 sqrt(25) x 8.6e-5 = 1.2e-3 + 2.2e-3 = 3.4e-3 < 3.9e-3
# (all-ones addresses, 4 or 5 ramps per addition, would not fit: 5 x 4 x 1.2e-4 + 1.9e-3 = 4.3e-3).
TALLIES = {"slots": dict(depth=4, steps=0, addrs=(3, 12, 3, 5, 10)), "coefficients": dict(depth=2, steps=3, addrs=(9, 20, 9, 6, 17))}
_tallies = {}


def tally(p, tlwe_key, which):
    """The scenario, made once and left unchanged: a memory of 2^depth client-encrypted zeros, five client-encrypted values --
    "slots": whole polynomials of multiples of 1/64 added to slot addr; "coefficients": the amount c/64 on coefficient 0, moved
    to coefficient addr % 8 of slot addr // 8 -- with the address bits of all five as ONE set of TGSW samples, selectors laid
    out [steps low bits][depth high bits], and the plaintext tally.
    -> dict(depth, steps, samples, sel_of, values, mem0, want [2^depth][N], out: the CPU reference's memory)"""
    from ieache_amd import tools
    key = (np.asarray(tlwe_key).tobytes(), which)
    if key not in _tallies:
        sc = TALLIES[which]
        depth, steps, addrs = sc["depth"], sc["steps"], sc["addrs"]
        N, bits = p.N, sc["depth"] + sc["steps"]
        assert all(bin(a).count("1") <= 2 for a in addrs) and len(set(addrs)) == len(addrs) - 1
        rng = np.random.default_rng(9820 + depth)
        mem0 = tools.tlwe_encrypt(p, tlwe_key, np.zeros((1 << depth, N), dtype=np.int32), 211)[None]
        want = np.zeros((1 << depth, N), dtype=np.int64)
        msgs = np.zeros((len(addrs), N), dtype=np.int64)
        for i, a in enumerate(addrs):
            if steps:
                msgs[i, 0] = int(rng.integers(1, 8)) << 26
                want[a >> steps, a & ((1 << steps) - 1)] += msgs[i, 0]
            else:
                msgs[i] = rng.integers(-8, 8, size=N) << 26
                want[a] += msgs[i]
        values = tools.tlwe_encrypt(p, tlwe_key, msgs.astype(np.int32), 221)
        samples = tools.tgsw_encrypt(p, tlwe_key, [(a >> t) & 1 for a in addrs for t in range(bits)], 231)
        sel_of = np.arange(len(addrs) * bits, dtype=np.int32).reshape(len(addrs), bits)
        out = tools.lut_add_reference(p, samples, values, depth, steps, sel_of=sel_of, mems=mem0)
        _tallies[key] = dict(depth=depth, steps=steps, samples=samples, sel_of=sel_of, values=values, mem0=mem0,
                             want=SR._wrap32(want), out=out)
    return _tallies[key]


@pytest.mark.parametrize("which", sorted(TALLIES))
def test_tally_at_the_product_parameters(ia, which):
    """N = 1024, (3, 7), TGSW and TLWE noise 2^-25: after the five additions every coefficient of every slot is within 2^-8 of the
    plaintext tally (the condition derived above; a condition and not a measurement -- the largest error is printed).  The slot
    addressed twice holds the sum of two values."""
    from ieache_amd import tools
    p = ia.default_params()
    assert (p.N, p.l, p.Bgbit) == (1024, 3, 7) and p.tlwe_alpha_min == 2.0 ** -25
    k = tools.keygen_raw(p, (1, 2, 3), with_cloud=False)
    sc = tally(p, k["tlwe_key"], which)
    assert sc["out"].shape == (1, 1 << sc["depth"], 2, p.N)
    err = torus_distance(tools.tlwe_phase(p, k["tlwe_key"], sc["out"][0]), sc["want"])
    print("%s: five additions, depth %d steps %d: largest phase error %.3e (bound 2^-8 = %.3e)" % (which, sc["depth"], sc["steps"], err.max(), 2.0 ** -8))
    assert err.shape == (1 << sc["depth"], p.N) and err.max() < 2.0 ** -8
    # decoded: the phase rounded to multiples of 1/64 is the tally itself
    phase = tools.tlwe_phase(p, k["tlwe_key"], sc["out"][0]).astype(np.int64)
    assert np.array_equal(((phase + (1 << 25)) >> 26) & 63, (sc["want"].astype(np.int64) >> 26) & 63)
    assert np.count_nonzero(sc["want"]) > 0
