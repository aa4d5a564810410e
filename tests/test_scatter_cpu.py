"""The write at an encrypted index (include/ieache.h section 3g) without a GPU: the C reference ieache_lut_scatter_reference against
the numpy restatement (scatter_reference.py) word for word, the exact invariants of the definition at N = 1024, three replace
writes into a 16-slot memory at the product parameters by meaning, the refusals that need no device, the declarations, and
the C reference in a stand-alone program under AddressSanitizer + UBSan.

No planning code was added for the scatter (csrc/cmux_plan.h's tree plan is the cut, unchanged; test_cmux_cpu.py runs it under
AddressSanitizer + UBSan), so there is no native program for a plan here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cmux_reference as CR
import scatter_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the two device sets on both toy rings, and one more set of the lattice on each
TOY_SETS = [(16, 3, 7), (16, 2, 10), (16, 1, 27), (64, 3, 7), (64, 2, 10), (64, 4, 8)]


def params(ia, N, l, Bgbit, n=4):
    return ia.default_params().copy(n=n, N=N, l=l, Bgbit=Bgbit)


@pytest.mark.parametrize("N,l,Bgbit", TOY_SETS)
def test_reference_is_the_definition_word_for_word_on_toy_rings(ia, N, l, Bgbit):
    """Full-range random words; depth 0 .. 3, count 1 and 3, selectors implied and explicit with repeats, mem given and None."""
    from ieache_amd import tools
    p = params(ia, N, l, Bgbit)
    rng = np.random.default_rng(9000 + N + 100 * l + Bgbit)
    n = 4
    S = CR.full_range(rng, (n, 2 * l, 2, N))
    for depth in range(4):
        for count in (1, 3):
            v = CR.full_range(rng, (count, 2, N))
            mem = CR.full_range(rng, (count, 1 << depth, 2, N))
            sel = rng.integers(0, n, size=(count, max(depth, 1))).astype(np.int32)
            sel[-1, :] = n - 1  # one sample for every bit of the last item
            for so in (None, sel):
                for m in (None, mem):
                    got = tools.lut_scatter_reference(p, S, v, depth, sel_of=so, mem=m)
                    assert got.shape == (count, 1 << depth, 2, N) and got.dtype == np.int32
                    assert np.array_equal(got, SR.lut_scatter(S, v, depth, l, Bgbit, sel_of=so, mem=m)), (depth, count, so is None, m is None)
    assert tools.lut_scatter_reference(p, S, v[:0], 2).shape == (0, 4, 2, N)


@pytest.mark.parametrize("l,Bgbit", [(3, 7), (2, 10)])
def test_exact_invariants_at_n1024(ia, l, Bgbit):
    """For ANY words: the leaves of an item sum to its value word for word (sum_j (out[j] - mem[j]) == v, depth 3); at depth 1
    row 1 is the external product cmux_reference(C, v, None) and row 0 is v minus it; depth 0 is mem + v; out may be mem."""
    from ieache_amd import tools
    p = params(ia, 1024, l, Bgbit)
    rng = np.random.default_rng(9100 + l)
    S = CR.full_range(rng, (3, 2 * l, 2, 1024))
    v = CR.full_range(rng, (2, 2, 1024))
    mem = CR.full_range(rng, (2, 8, 2, 1024))
    sel = np.array([[2, 0, 1], [1, 1, 0]], dtype=np.int32)
    out = tools.lut_scatter_reference(p, S, v, 3, sel_of=sel, mem=mem)
    leaves = SR.sub32(out, mem)
    assert np.array_equal(SR._wrap32(leaves.astype(np.int64).sum(axis=1)), v)
    assert np.array_equal(leaves, tools.lut_scatter_reference(p, S, v, 3, sel_of=sel))
    # one item against the numpy restatement on the ring the kernels cover
    assert np.array_equal(out[1], SR.lut_scatter(S, v[1:], 3, l, Bgbit, sel_of=sel[1:], mem=mem[1:])[0])
    one = tools.lut_scatter_reference(p, S, v, 1, sel_of=[[2], [0]])
    hi = tools.cmux_reference(p, S, v, None, sel_of=[2, 0])
    assert np.array_equal(one[:, 1], hi) and np.array_equal(one[:, 0], SR.sub32(v, hi))
    assert np.array_equal(tools.lut_scatter_reference(p, S, v, 0, mem=mem[:, :1]), SR.add32(mem[:, :1], v[:, None]))
    assert np.array_equal(tools.lut_scatter_reference(p, S, v, 0), v[:, None])
    # in place through the raw call: out is mem itself
    from ieache_amd.evaluator import _i32, check
    inplace = mem.copy()
    check(ia.lib().ieache_lut_scatter_reference(C.byref(p), _i32(S), 3, 2, 3, _i32(sel), _i32(v), _i32(inplace), _i32(inplace)))
    assert np.array_equal(inplace, out)


def torus_distance(a, b):
    d = (np.asarray(a, dtype=np.int64) - np.asarray(b, dtype=np.int64)) & 0xFFFFFFFF
    return np.minimum(d, (1 << 32) - d).astype(np.float64) / 2.0 ** 32


WRITE_ADDRS = (3, 12, 3)
_writes = {}


def three_writes(p, tlwe_key):
    """The end-to-end sequence, made once and left unchanged: a 16-slot memory of +-1/8 polynomials under the ring key (noise
    the key's, 2^-25), and for each of the writes at addresses 3, 12, 3 four FRESH selector samples (bit k of the address at
    index k), the new +-1/8 polynomial and its fresh encryption; then, on the CPU reference, the memory after each write as
    Context.lut_write forms it (lut_tree with the item's own table, a wrapping subtraction, lut_scatter).
    -> dict(msg0, mem0, steps = [(samples, sel_of, new)], mems = [memory after write w], want = [messages [16][N] after write w])"""
    from ieache_amd import tools
    key = np.asarray(tlwe_key).tobytes()
    if key not in _writes:
        N = p.N
        rng = np.random.default_rng(9700)
        msg0 = msg = np.where(rng.integers(0, 2, size=(16, N)) == 1, 1 << 29, -(1 << 29)).astype(np.int32)
        mem0 = mem = tools.tlwe_encrypt(p, tlwe_key, msg, 171)[None]
        steps, mems, want = [], [], []
        sel = np.arange(4, dtype=np.int32)[None]
        for w, addr in enumerate(WRITE_ADDRS):
            samples = tools.tgsw_encrypt(p, tlwe_key, [(addr >> k) & 1 for k in range(4)], 181 + w)
            m = np.where(rng.integers(0, 2, size=N) == 1, 1 << 29, -(1 << 29)).astype(np.int32)
            new = tools.tlwe_encrypt(p, tlwe_key, m, 191 + w)
            old = tools.lut_tree_reference(p, samples, mem, 4, sel_of=sel, table_of=[0])
            mem = tools.lut_scatter_reference(p, samples, SR.sub32(new, old), 4, sel_of=sel, mem=mem)
            msg = msg.copy()
            msg[addr] = m
            steps.append((samples, sel, new))
            mems.append(mem)
            want.append(msg)
        _writes[key] = dict(msg0=msg0, mem0=mem0, steps=steps, mems=mems, want=want)
    return _writes[key]


def test_three_replace_writes_at_the_product_parameters(ia):
    """N = 1024, l = 3, Bgbit = 7, TGSW and TLWE noise 2^-25: after each of the writes at 3, 12, 3 every coefficient of every slot
    is within 2^-8 of what the slot should hold -- the decoding condition test_cmux's tree test uses, a condition and not a
    measurement.  DESIGN.md section 7 derives what to expect (about 1e-3 after three writes; this sequence gives 9.8e-4, 9.6e-4,
    1.21e-3, a numpy model of the definition with other draws 8.4e-4, 8.7e-4, 1.19e-3).  Not run at (2, 10): one depth-4 write
    there exceeds 2^-8 (section 7)."""
    from ieache_amd import tools
    p = ia.default_params()
    assert (p.N, p.l, p.Bgbit) == (1024, 3, 7) and p.tlwe_alpha_min == 2.0 ** -25
    k = tools.keygen_raw(p, (1, 2, 3), with_cloud=False)
    seq = three_writes(p, k["tlwe_key"])
    assert np.array_equal(tools.tlwe_phase(p, k["tlwe_key"], seq["mem0"][0]) > 0, seq["msg0"] > 0)
    for w, (mem, want) in enumerate(zip(seq["mems"], seq["want"])):
        err = torus_distance(tools.tlwe_phase(p, k["tlwe_key"], mem[0]), want)
        print("after write %d (address %d): largest phase error %.3e (bound 2^-8 = %.3e)" % (w + 1, WRITE_ADDRS[w], err.max(), 2.0 ** -8))
        assert err.shape == (16, p.N) and err.max() < 2.0 ** -8, w
    # the slot written twice holds the third value, not the first; an untouched slot what it held
    assert not np.array_equal(seq["want"][0][3], seq["want"][2][3]) and np.array_equal(seq["want"][2][5], seq["msg0"][5])


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
    assert tools.lut_scatter_reference(p, S, v, 2, sel_of=[[1, 0], [0, 1]]).shape == (2, 4, 2, 16)
    refused(ia, r"sel_of\[1\] = 2", tools.lut_scatter_reference, p, S, v, 2, sel_of=[[1, 2], [0, 0]])
    refused(ia, r"sel_of\[2\] = -1", tools.lut_scatter_reference, p, S, v, 2, sel_of=[[1, 0], [-1, 0]])
    refused(ia, "depth", tools.lut_scatter_reference, p, S, v, -1)
    refused(ia, "unsupported", tools.lut_scatter_reference, p.copy(N=8), S, v, 1)
    L, pc, out = ia.lib(), C.byref(p), np.zeros((1, 2, 16), dtype=np.int32)
    refused(ia, "depth", lambda: check(L.ieache_lut_scatter_reference(pc, _i32(S), 2, 1, 13, None, _i32(v), None, _i32(out))))
    refused(ia, "no samples", lambda: check(L.ieache_lut_scatter_reference(pc, _i32(S), 0, 1, 0, None, _i32(v), None, _i32(out))))
    refused(ia, "null", lambda: check(L.ieache_lut_scatter_reference(pc, _i32(S), 2, 1, 0, None, None, None, _i32(out))))


def test_reference_under_asan_ubsan(tmp_path):
    """lut_scatter_reference of csrc/tfhe_host.cpp in a stand-alone program (tests/native/scatter_reference_test.cpp):
    exact-size buffers, l x Bgbit = 32, the largest Bgbit, Bgbit = 1, mem given / null / the output itself, the steps against
    flat external products chained by hand."""
    csrc = os.path.join(ROOT, "ie-ache_amd", "csrc")
    exe = tmp_path / "scatter_reference_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I", csrc, os.path.join(ROOT, "tests", "native", "scatter_reference_test.cpp"),
                           os.path.join(csrc, "tfhe_host.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "SCATTER_REFERENCE_OK" in r.stdout, r.stdout[-4000:]


# name -> number of parameters as include/ieache.h declares them (all return int)
DECLARED = {"ieache_lut_scatter": 9, "ieache_lut_scatter_device": 9, "ieache_lut_scatter_reference": 9}


def test_every_symbol_is_declared_exported_and_bound(ia):
    with open(os.path.join(ROOT, "include", "ieache.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = {m.group(1): m.group(2) for m in re.finditer(r"^int\s+(ieache_lut_scatter[a-z_]*)\s*\(([^;]*)\)\s*;", hdr, re.M)}
    assert set(declared) == set(DECLARED)
    raw, L = C.CDLL(ia.library_path()), ia.lib()
    for name, n_params in DECLARED.items():
        assert len(declared[name].split(",")) == n_params, name
        assert hasattr(raw, name), name
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n_params, name  # the binding passes what the header declares
    # the device form carries the host form's arguments, pointers opaque
    assert len(L.ieache_lut_scatter.argtypes) == len(L.ieache_lut_scatter_device.argtypes)
    for name in ("lut_scatter", "lut_scatter_device", "lut_write"):
        assert callable(getattr(ia.Context, name)), name
    from ieache_amd import tools
    assert callable(tools.lut_scatter_reference)
