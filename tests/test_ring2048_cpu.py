"""Rings of degree 2048, the parts that need no GPU: the references of tests/test_ring2048_gpu.py pinned against each other, the
gate Params::supported() (csrc/params.h) through the C ABI, the even / odd identity the N = 2048 CMux step rests on
(tests/native/ring_split_test.cpp), and the LDS needs by which a context refuses a set at creation
(tests/native/ring2048_plan_test.cpp; the refusals themselves need a device and are in the GPU file)."""
import os
import subprocess

import numpy as np
import pytest

import np_tfhe
import param_lattice as PL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, N, l, Bgbit, ks_t, ks_basebit); the last lies on the edge of Params::br_exact(): 2 x 2048 x 2^20 = 2^32
ORACLE_SETS = [(4, 2048, 3, 7, 8, 2), (3, 2048, 4, 6, 8, 2), (3, 4096, 2, 10, 8, 2), (5, 2048, 1, 20, 8, 2)]


@pytest.mark.parametrize("pset", ORACLE_SETS, ids=lambda s: "n%d-N%d-l%d-Bg%d-t%d-bb%d" % s)
def test_oracle_equals_numpy_restatement_on_the_larger_rings(O, pset):
    """The C oracle and np_tfhe (numpy int64, exact convolutions) word for word: a bootstrap of any phase, two gates, and the
    stages the GPU file compares one by one composed to the same sample.  N = 4096 is a ring the references serve and the
    evaluator refuses."""
    n, N, l, Bgbit, t, bb = pset
    assert PL.br_exact(l, Bgbit, N)
    K = np_tfhe.ToyKeys(n=n, N=N, l=l, Bgbit=Bgbit, ks_t=t, ks_basebit=bb, seed=n + N + l + t)
    ck = O.CloudKey(n, N, 1, l, Bgbit, t, bb, K.bk, K.ksk)
    a, b = K.encrypt_bits([1, 0]), K.encrypt_bits([1, 1])
    rnd = np_tfhe.uniform32(np.random.default_rng(N + l), n + 1)
    ref = np_tfhe.np_bootstrap(K, rnd)
    assert np.array_equal(ck.bootstrap(rnd), ref)
    assert np.array_equal(ck.gate("and", a[0], b[0]), np_tfhe.np_gate(K, "and", a[0], b[0]))
    assert np.array_equal(ck.gate("xor", a[1], b[1]), np_tfhe.np_gate(K, "xor", a[1], b[1]))
    bara, barb = ck.modswitch(rnd)
    assert barb == np_tfhe.np_modswitch(int(rnd[n]), (2 * N).bit_length() - 1)
    assert [int(v) for v in bara] == [np_tfhe.np_modswitch(int(w), (2 * N).bit_length() - 1) for w in rnd[:n]]
    acc = ck.blind_rotate_init(barb)
    for i in range(n):
        acc = ck.blind_rotate_step(acc, i, bara[i])
    u = ck.sample_extract(acc)
    assert np.array_equal(ck.keyswitch(u), ref)
    assert np.array_equal(np_tfhe.np_keyswitch(K.ksk, t, bb, u)[0], ref)


def test_ring_2048_is_accepted_and_nothing_above_it(ia):
    """Params::supported() through the C ABI (the key generator asks it before it draws anything): N = 2048 with the gadgets of
    the GPU file and on the br_exact() edge; N = 4096, N = 1000 and one Bgbit past the edge refused."""
    from ieache_amd import tools
    base = ia.default_params()
    for l, Bgbit in ((3, 7), (2, 10), (4, 6), (8, 4), (1, 20), (2, 16)):
        k = tools.keygen_raw(base.copy(n=3, N=2048, l=l, Bgbit=Bgbit), (1, 2, 3), with_cloud=False)
        assert k["tlwe_key"].shape == (2048,) and set(np.unique(k["tlwe_key"])) <= {0, 1}
    for kw in (dict(N=4096), dict(N=4096, l=2, Bgbit=10), dict(N=1000), dict(N=3072), dict(N=2048, l=1, Bgbit=21), dict(N=2048, l=3, Bgbit=11)):
        with pytest.raises(ia.IeacheError, match="unsupported parameter set"):
            tools.keygen_raw(base.copy(n=3, **kw), (1, 2, 3), with_cloud=False)


@pytest.mark.parametrize("N,l,Bgbit,t,bb", PL.REFUSED_SETS)
def test_every_refused_set_of_the_lattice_stays_refused(ia, N, l, Bgbit, t, bb):
    from ieache_amd import tools
    p = ia.default_params().copy(n=3, N=N, l=l, Bgbit=Bgbit, ks_t=t, ks_basebit=bb)
    with pytest.raises(ia.IeacheError, match="unsupported parameter set"):
        tools.keygen_raw(p, (1, 2, 3), with_cloud=False)


def test_key_files_of_a_2048_ring_round_trip(ia, tmp_path):
    """The codec asks the same gate: a cloud key written at N = 2048 is read back with its header, and the same file with
    N: 4096 in the header is refused when the header is read."""
    from ieache_amd import tools
    p = ia.default_params().copy(n=2, N=2048, l=2, Bgbit=10, ks_t=2, ks_basebit=2)
    tools.keygen_files(tmp_path, p, seed=(1, 2, 3), nbit_seed=(4, 5))
    q, bk, ksk = tools.read_cloud_key(tmp_path / "cloud.key")
    assert bytes(q) == bytes(p) and bk.size == p.bk_count and ksk.size == p.ksk_count
    raw = (tmp_path / "cloud.key").read_bytes()
    assert raw.count(b"N: 2048\n") == 1
    (tmp_path / "refused.key").write_bytes(raw.replace(b"N: 2048\n", b"N: 4096\n"))
    with pytest.raises(ia.IeacheError, match="not supported"):
        tools.read_cloud_key(tmp_path / "refused.key")


def test_lookup_polynomials_at_the_larger_ring(ia):
    """lut_test_poly / lut_factor_poly lay a 16-entry table out over N = 2048: slots of N / 16 coefficients, centred on their
    messages, the half slot that wraps negated."""
    from ieache_amd import tools
    p = ia.default_params().copy(n=3, N=2048)
    table = (np.arange(16, dtype=np.int64) << 27).astype(np.int32)
    v = tools.lut_test_poly(p, table)
    assert v.shape == (2048,)
    rot = np.concatenate([v[-64:].astype(np.int64) * -1, v[:-64].astype(np.int64)])  # X^64 v: slot m on [128 m, 128 m + 128)
    assert np.array_equal(rot.reshape(16, 128), np.repeat(table.astype(np.int64)[:, None], 128, axis=1))
    assert tools.lut_factor_poly(p, np.arange(16, dtype=np.int32)).shape == (2048,)


def _native(tmp_path, name, token, opt="-O1", include=True):
    exe = tmp_path / name
    cmd = ["g++", "-std=c++17", opt, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    if include:
        cmd += ["-I", os.path.join(ROOT, "ie-ache_amd", "csrc")]
    subprocess.check_call(cmd + [os.path.join(ROOT, "tests", "native", name + ".cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and token in r.stdout, r.stdout[-4000:]


def test_even_odd_split_of_the_ring_under_asan_ubsan(tmp_path):
    """The product on the halves and the rotation rule against the direct negacyclic ones, amounts 0, 1, 2, 2047, 2048, 2049, 4094
    and 4095, random and extreme polynomials (-O2: some thirty schoolbook products of 2048 x 2048 terms)."""
    _native(tmp_path, "ring_split_test", "RING_SPLIT_OK", opt="-O2", include=False)


def test_lds_needs_and_refusals_at_2048_under_asan_ubsan(tmp_path):
    """csrc/br_plan.h and csrc/ks_plan.h on the larger ring: the any-parameter blind rotation fits a CU's LDS up to l = 4, the
    key switch's digit list up to t = 18; past either, context creation refuses (the GPU file sees the messages)."""
    _native(tmp_path, "ring2048_plan_test", "RING2048_PLAN_OK")
