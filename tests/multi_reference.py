"""The multi-output programmable bootstrap's reference: the untouched CPU oracle's separately callable stages, composed in numpy.

    modswitch -> acc = (0, X^(2N - barb) * v) -> blind_rotate -> for each factor P: negacyclic_mul(P, acc[c]) on both polynomials
              -> sample_extract -> + bias on b [-> keyswitch]

The products take the oracle's SCHOOLBOOK back-end: exact with wraparound for full-range factors (its NTT back-end is exact only
for small first operands).  Test support only.  Also here: the table -> factor rule of include/ieache.h in numpy, and the noise
budget of DESIGN.md section 7 for outputs whose rotation noise a factor has multiplied."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import lut_reference as LR
from np_tfhe import _wrap32
from oracle import oracle as O


def accumulator(ck, x, v):
    """The oracle's whole accumulator [2][N] of row x blind-rotated from the test polynomial v."""
    bara, barb = ck.modswitch(x)
    acc = np.zeros((2, ck.N), dtype=np.int32)
    acc[1] = LR.rotated_test_poly(v, barb)
    return ck.blind_rotate(acc, bara)


def multi_from_accumulator(ck, acc, factors, bias=None, keyswitch=True):
    """-> [n_factors][n+1] (or [N+1]): each factor times both polynomials of acc, coefficient 0 extracted, bias on b."""
    out = []
    for t, P in enumerate(np.ascontiguousarray(factors, dtype=np.int32).reshape(-1, ck.N)):
        prod = np.stack([O.negacyclic_mul(P, acc[c], mode=O.POLYMUL_SCHOOLBOOK) for c in range(2)])
        u = ck.sample_extract(prod)
        if bias is not None:
            u[ck.N] = _wrap32(int(u[ck.N]) + int(bias[t]))
        out.append(ck.keyswitch(u) if keyswitch else u)
    return np.stack(out)


def multi_reference(ck, x, v, factors, bias=None, keyswitch=True):
    """One row -> [n_factors][n+1], or the extracted samples [n_factors][N+1]."""
    return multi_from_accumulator(ck, accumulator(ck, x, v), factors, bias, keyswitch)


def multi_reference_rows(ck, x, polys, factors, poly_of=None, bias=None, threads=16):
    """Rows x [count][n+1] -> (extracted samples [count][n_factors][N+1], key-switched [count][n_factors][n+1]), on host threads
    (the oracle's stages take the key read-only and ctypes releases the interpreter lock)."""
    x = np.ascontiguousarray(x, dtype=np.int32).reshape(-1, ck.n + 1)
    polys = np.ascontiguousarray(polys, dtype=np.int32).reshape(-1, ck.N)
    factors = np.ascontiguousarray(factors, dtype=np.int32).reshape(-1, ck.N)
    of = np.zeros(len(x), dtype=np.int64) if poly_of is None else np.asarray(poly_of)

    def one(i):
        u = multi_reference(ck, x[i], polys[of[i]], factors, bias, keyswitch=False)
        return u, np.stack([ck.keyswitch(r) for r in u])

    with ThreadPoolExecutor(threads) as ex:
        both = list(ex.map(one, range(len(x))))
    return np.stack([b[0] for b in both]), np.stack([b[1] for b in both])


def monomial(N, power, coef=1):
    """coef * X^power as a factor polynomial; power may be negative or >= N (X^N = -1)."""
    P = np.zeros(N, dtype=np.int64)
    e = power % (2 * N)
    P[e % N] = -coef if e >= N else coef
    return _wrap32(P)


def factor_poly(N, table):
    """include/ieache.h's rule in numpy: P = v (1 - X) with v = lut_poly(table): P[0] = v[0] + v[N-1], P[j] = v[j] - v[j-1]."""
    v = LR.lut_poly(N, table).astype(np.int64)
    return _wrap32(v - np.concatenate([-v[-1:], v[:-1]]))


def norm2(P):
    """Squared Euclidean norm of a factor: what it multiplies the rotation's share of the output variance by."""
    return int((np.asarray(P, dtype=np.int64) ** 2).sum())


def keyswitch_variance(p):
    """The key switch's share of predicted_gate_output_noise's variance (test_golden_cpu.py: the part that varies from output
    to output under one key)."""
    base = 1 << p.ks_basebit
    return p.N * p.k * p.ks_t * ((base - 1.0) / base) ** 2 * p.lwe_alpha_min ** 2


def output_variance(p, V, n2):
    """Variance of an output of the multi-output bootstrap: the rotation's share of V times |P|^2, the key switch's once."""
    ks = keyswitch_variance(p)
    return n2 * (V - ks) + ks


def margin(p, V, offset_sd, entries, k, n2):
    """DESIGN.md section 7's margin of a table of `entries` slots whose input is k such outputs added up:
    (1/(4 entries) - k 4 offset_sd) / sqrt(k V_out(|P|^2) + rounding)."""
    rounding = (1 + p.n / 2) / 12.0 / (2.0 * p.N) ** 2
    return (1.0 / (4 * entries) - k * 4 * offset_sd) / np.sqrt(k * output_variance(p, V, n2) + rounding)
