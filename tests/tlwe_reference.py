"""Blind rotation on a caller's TLWE accumulator: the untouched CPU oracle's separately callable stages, composed in numpy.

    modswitch -> acc = (X^(2N - barb) * A, X^(2N - barb) * B) -> blind_rotate [-> sample_extract [-> keyswitch]]

which is libtfhe's tfhe_blindRotate_FFT on the accumulator X^(2N - barb) * (A, B) (plus tLweExtractLweSample and lweKeySwitch):
lut_reference.pbs_reference with an A half of the caller's.  The oracle's blind_rotate takes any [2][N] accumulator.  Test
support only.  Also here: a numpy restatement of the same steps that shares no code with the oracle (toy rings only), the
numpy extraction of a coefficient of an accumulator, and TLWE encryption / phase in numpy."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import lut_reference as LR
from np_tfhe import _mul_by_xai, _negacyclic, _u32, _wrap32, np_keyswitch, np_modswitch

ACC, EXTRACTED, KEYSWITCHED = "acc", "extracted", "keyswitched"


def rotated_sample(sample, barb):
    """X^(2N - barb) * (A, B): both polynomials by the same amount with the same negacyclic rule."""
    sample = np.ascontiguousarray(sample, dtype=np.int32).reshape(2, -1)
    return np.stack([LR.rotated_test_poly(sample[c], barb) for c in range(2)])


def tlwe_reference(ck, x, sample, what=KEYSWITCHED):
    """One row through the oracle's stages from the TLWE sample [2][N] -> the whole accumulator [2][N], the extracted sample
    [N+1] or the LWE sample [n+1]."""
    bara, barb = ck.modswitch(x)
    acc = ck.blind_rotate(rotated_sample(sample, barb), bara)
    if what == ACC:
        return acc
    u = ck.sample_extract(acc)
    return ck.keyswitch(u) if what == KEYSWITCHED else u


def tlwe_reference_rows(ck, x, samples, poly_of=None, threads=16):
    """Rows x [count][n+1] with samples [n_polys][2][N] and one index per row (None: sample 0), on host threads ->
    dict(acc [count][2][N], extracted [count][N+1], keyswitched [count][n+1]): one rotation per row, its later stages shared."""
    x = np.ascontiguousarray(x, dtype=np.int32).reshape(-1, ck.n + 1)
    samples = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, 2, ck.N)
    of = np.zeros(len(x), dtype=np.int64) if poly_of is None else np.asarray(poly_of)

    def one(i):
        acc = tlwe_reference(ck, x[i], samples[of[i]], ACC)
        u = ck.sample_extract(acc)
        return acc, u, ck.keyswitch(u)

    if not len(x):
        return {ACC: np.zeros((0, 2, ck.N), np.int32), EXTRACTED: np.zeros((0, ck.N + 1), np.int32), KEYSWITCHED: np.zeros((0, ck.n + 1), np.int32)}
    with ThreadPoolExecutor(threads) as ex:
        rows = list(ex.map(one, range(len(x))))
    return {ACC: np.stack([r[0] for r in rows]), EXTRACTED: np.stack([r[1] for r in rows]), KEYSWITCHED: np.stack([r[2] for r in rows])}


def with_zero_mask(polys):
    """Plain polynomials [count][N] as TLWE samples with A = 0: [count][2][N]."""
    polys = np.ascontiguousarray(polys, dtype=np.int32)
    return np.stack([np.zeros_like(polys), polys], axis=-2)


def extract_coefficient(acc, j=0):
    """The LWE sample [..., N+1] of coefficient j of accumulators [..., 2, N], as every bootstrap here extracts:
    u[i] = A[j - i] for i <= j, -A[N + j - i] otherwise; u[N] = B[j]."""
    acc = np.asarray(acc, dtype=np.int32)
    N = acc.shape[-1]
    A = acc[..., 0, :].astype(np.int64)
    i = np.arange(N)
    u = np.where(i <= j, A[..., (j - i) % N], -A[..., (N + j - i) % N])
    return np.concatenate([_wrap32(u), acc[..., 1, j:j + 1]], axis=-1)


def np_tlwe_pbs(K, x, sample, what=KEYSWITCHED):
    """lut_reference.np_pbs with an acc[0] of the caller's: exact integer arithmetic on the raw key arrays K (anything with n, N,
    l, Bgbit, ks_t, ks_basebit, bk [n][2l][2][N], ksk [N][t][base][n+1])."""
    n, N, l, Bgbit = K.n, K.N, K.l, K.Bgbit
    log2_2N = (2 * N).bit_length() - 1
    barb = np_modswitch(x[n], log2_2N)
    bara = [np_modswitch(x[i], log2_2N) for i in range(n)]
    sample = np.asarray(sample, dtype=np.int32).reshape(2, N)
    acc = [_mul_by_xai(sample[c], (2 * N - barb) % (2 * N)) for c in range(2)]
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
    if what == ACC:
        return np.stack(acc)
    u = np.zeros(N + 1, dtype=np.int32)
    u[0] = acc[0][0]
    u[1:N] = _wrap32(-acc[0][N - 1:0:-1].astype(np.int64))
    u[N] = acc[1][0]
    if what == EXTRACTED:
        return u
    return np_keyswitch(np.asarray(K.ksk).reshape(N, K.ks_t, 1 << K.ks_basebit, n + 1), K.ks_t, K.ks_basebit, u)[0]


def np_tlwe_phase(tlwe_key, samples):
    """B - A s, negacyclic and mod 2^32, of samples [..., 2, N] under the binary ring key [N] -> [..., N]."""
    samples = np.asarray(samples, dtype=np.int32)
    N = samples.shape[-1]
    flat = samples.reshape(-1, 2, N)
    s = np.asarray(tlwe_key[:N], dtype=np.int64)
    out = np.stack([_wrap32(r[1].astype(np.int64) - _negacyclic(s, r[0]).astype(np.int64)) for r in flat])
    return out.reshape(samples.shape[:-2] + (N,))
