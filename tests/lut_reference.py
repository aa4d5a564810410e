"""The programmable bootstrap's reference: the untouched CPU oracle's separately callable stages, composed in numpy.

    modswitch -> acc = (0, X^(2N - barb) * v) -> blind_rotate -> sample_extract [-> keyswitch]

which is libtfhe's tfhe_blindRotateAndExtract_FFT from the test polynomial v (plus lweKeySwitch): the oracle's own bootstrap with
v in place of the constant polynomial.  Test support only.  Also here: a numpy restatement of the same steps that shares no
code with the oracle (toy rings only), the table -> polynomial rule of include/ieache.h, and the decode of a table's output."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import np_tfhe
from np_tfhe import _mul_by_xai, _negacyclic, _u32, _wrap32, np_keyswitch, np_modswitch


def rotated_test_poly(v, barb):
    """testvectbis = X^(2N - barb) * v mod X^N + 1."""
    v = np.ascontiguousarray(v, dtype=np.int32)
    N = v.shape[0]
    return _mul_by_xai(v, (2 * N - int(barb)) % (2 * N))


def pbs_reference(ck, x, v, keyswitch=True):
    """One row through the oracle's stages from the test polynomial v -> LWE sample [n+1], or the extracted sample [N+1]."""
    bara, barb = ck.modswitch(x)
    acc = np.zeros((2, ck.N), dtype=np.int32)
    acc[1] = rotated_test_poly(v, barb)
    u = ck.sample_extract(ck.blind_rotate(acc, bara))
    return ck.keyswitch(u) if keyswitch else u


def pbs_reference_rows(ck, x, polys, poly_of=None, keyswitch=True, threads=16):
    """Rows x [count][n+1] with polys [n_polys][N] and one row index per x row (None: polynomial 0), on host threads (the
    oracle's stages take the key read-only and ctypes releases the interpreter lock)."""
    x = np.ascontiguousarray(x, dtype=np.int32).reshape(-1, ck.n + 1)
    polys = np.ascontiguousarray(polys, dtype=np.int32).reshape(-1, ck.N)
    of = np.zeros(len(x), dtype=np.int64) if poly_of is None else np.asarray(poly_of)
    width = (ck.n if keyswitch else ck.N) + 1
    if not len(x):
        return np.zeros((0, width), dtype=np.int32)
    with ThreadPoolExecutor(threads) as ex:
        return np.stack(list(ex.map(lambda i: pbs_reference(ck, x[i], polys[of[i]], keyswitch), range(len(x)))))


def np_pbs(K, x, v, keyswitch=True):
    """np_tfhe.np_bootstrap's steps with the test polynomial as an argument: exact integer arithmetic on the raw key arrays K
    (anything with n, N, l, Bgbit, ks_t, ks_basebit, bk [n][2l][2][N], ksk [N][t][base][n+1])."""
    n, N, l, Bgbit = K.n, K.N, K.l, K.Bgbit
    log2_2N = (2 * N).bit_length() - 1
    barb = np_modswitch(x[n], log2_2N)
    bara = [np_modswitch(x[i], log2_2N) for i in range(n)]
    acc = [np.zeros(N, dtype=np.int32), _mul_by_xai(np.asarray(v, dtype=np.int32), (2 * N - barb) % (2 * N))]
    Bg, half = 1 << Bgbit, 1 << (Bgbit - 1)
    offset = sum(half << (32 - p * Bgbit) for p in range(1, l + 1)) & 0xFFFFFFFF
    for i in range(n):
        if bara[i] == 0:
            continue
        tmp = [_wrap32(_mul_by_xai(acc[u], bara[i]).astype(np.int64) - acc[u].astype(np.int64)) for u in range(2)]
        rows = []
        for u in range(2):
            w = (_u32(tmp[u]) + offset) & 0xFFFFFFFF
            for p in range(1, l + 1):
                rows.append(((w >> (32 - p * Bgbit)) & (Bg - 1)) - half)
        prod = [np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)]
        for row, dec in enumerate(rows):
            for c in range(2):
                prod[c] += _negacyclic(dec.astype(np.int64), K.bk[i, row, c]).astype(np.int64)
        acc = [_wrap32(acc[c].astype(np.int64) + prod[c]) for c in range(2)]
    u = np.zeros(N + 1, dtype=np.int32)
    u[0] = acc[0][0]
    u[1:N] = _wrap32(-acc[0][N - 1:0:-1].astype(np.int64))
    u[N] = acc[1][0]
    if not keyswitch:
        return u
    return np_keyswitch(np.asarray(K.ksk).reshape(N, K.ks_t, 1 << K.ks_basebit, n + 1), K.ks_t, K.ks_basebit, u)[0]


def lut_poly(N, table):
    """include/ieache.h's rule: v[j] = f[((j + N/(2p)) p) div N] for j < N - N/(2p), -f[0] on the last N/(2p) coefficients."""
    f = np.asarray(table, dtype=np.int64)
    p = len(f)
    assert N % (2 * p) == 0
    h = N // (2 * p)
    v = np.empty(N, dtype=np.int64)
    for j in range(N):
        v[j] = f[(j + h) * p // N] if j < N - h else -f[0]
    return _wrap32(v)


def message_phase(m, p):
    """Torus32 phase of message m of a p-entry table: m / (2p), padding bit clear."""
    return int(_wrap32((int(m) << 32) // (2 * p)))


def encrypt_messages(p_set, lwe_key, msgs, p, rng):
    """Fresh LWE encryptions of m / (2p) under lwe_key with the parameter set's noise -> [count][n+1]."""
    n = p_set.n
    msgs = np.asarray(msgs)
    a = np_tfhe.uniform32(rng, (len(msgs), n))
    e = np_tfhe.gaussian32(rng, p_set.lwe_alpha_min, len(msgs)).astype(np.int64)
    mu = np.array([int(message_phase(m, p)) for m in msgs], dtype=np.int64)
    out = np.zeros((len(msgs), n + 1), dtype=np.int32)
    out[:, :n] = a
    out[:, n] = _wrap32((a.astype(np.int64) * np.asarray(lwe_key[:n], dtype=np.int64)).sum(-1) + mu + e)
    return out


def phases(lwe_key, samples):
    """Phase b - <a, s> of each sample as a fraction of the torus in [-1/2, 1/2)."""
    s = np.asarray(samples, dtype=np.int32)
    n = s.shape[-1] - 1
    ph = _wrap32(s[..., n].astype(np.int64) - (s[..., :n].astype(np.int64) * np.asarray(lwe_key[:n], dtype=np.int64)).sum(-1))
    return ph.astype(np.float64) / 2.0 ** 32
