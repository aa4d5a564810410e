"""The references of tests/test_param_lattice_gpu.py, pinned before the GPU is compared with them.

The GPU file runs every kernel family over parameter sets far from libtfhe's two (tests/param_lattice.py).  Its reference is
the C oracle, which until now had a second witness only at l = 3 / Bgbit = 7 / t = 8 / basebit = 2.  Here the oracle is
compared sample for sample with np_tfhe.np_bootstrap (numpy int64 / exact convolutions, written from the spec alone) at every
decomposition the GPU file uses, on toy rings; and the plain numpy statement of the key switch, the GPU file's second
reference at large n, is compared with both."""
import numpy as np
import pytest

import np_tfhe
import param_lattice as PL


def _id(s):
    return "n%d-N%d-l%d-Bg%d-t%d-bb%d" % s


@pytest.mark.parametrize("pset", PL.cpu_sets(), ids=_id)
def test_oracle_equals_numpy_restatement_at_every_lattice_set(O, pset):
    n, N, l, Bgbit, t, bb = pset
    assert PL.br_exact(l, Bgbit, N)
    K = np_tfhe.ToyKeys(n=n, N=N, l=l, Bgbit=Bgbit, ks_t=t, ks_basebit=bb, seed=n + N + l + t)
    ck = O.CloudKey(n, N, 1, l, Bgbit, t, bb, K.bk, K.ksk)
    a, b = K.encrypt_bits([1, 0]), K.encrypt_bits([1, 1])
    rnd = np_tfhe.uniform32(np.random.default_rng(N + l), n + 1)  # any phase: the bits are compared, not the decryption
    assert np.array_equal(ck.gate("and", a[0], b[0]), np_tfhe.np_gate(K, "and", a[0], b[0]))
    assert np.array_equal(ck.gate("xor", a[1], b[1]), np_tfhe.np_gate(K, "xor", a[1], b[1]))
    ref = np_tfhe.np_bootstrap(K, rnd)
    assert np.array_equal(ck.bootstrap(rnd), ref)
    # the stages the GPU file compares one by one compose to the same sample
    bara, barb = ck.modswitch(rnd)
    acc = ck.blind_rotate_init(barb)
    for i in range(n):
        acc = ck.blind_rotate_step(acc, i, bara[i])
    u = ck.sample_extract(acc)
    assert np.array_equal(ck.keyswitch(u), ref)
    assert np.array_equal(np_tfhe.np_keyswitch(K.ksk, t, bb, u)[0], ref)


@pytest.mark.parametrize("t,bb", PL.KS_DECOMPS)
def test_numpy_keyswitch_statement_equals_oracle_on_edge_rows(O, t, bb):
    n, N = 6, 32
    rng = np.random.default_rng(t * 8 + bb)
    ksk = np_tfhe.uniform32(rng, (N, t, 1 << bb, n + 1))  # digit-0 rows hold noise: neither reference may read them
    ck = O.CloudKey(n, N, 1, 3, 7, t, bb, np.zeros((n, 6, 2, N), np.int32), ksk)
    u = PL.edge_rows(rng, N, t, bb, 5)
    out = np_tfhe.np_keyswitch(ksk, t, bb, u)
    for r in range(u.shape[0]):
        assert np.array_equal(ck.keyswitch(u[r]), out[r]), r
    # the edge rows are what they are meant to be: no row subtracted (5, 6, 8), the row of digit base - 1 at every position (7)
    for r in (5, 6, 8):
        assert not out[r, :n].any() and out[r, n] == u[r, N], r
    want = -ksk[:, :, (1 << bb) - 1].astype(np.int64).sum(axis=(0, 1))
    want[n] += int(u[7, N])
    assert np.array_equal(np_tfhe._wrap32(want), out[7])
