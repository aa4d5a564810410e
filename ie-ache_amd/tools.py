"""CPU tools around the Cloud path: key generation, operand encryption and
answer decryption -- what the reference's Keygen/keygen.c:22-51,
Client1/alice.c:116-191 and Output/verif.c:41-179 do through libtfhe.  All of
it runs inside libieache.so's host code (no GPU, no oracle)."""
import ctypes as C
import os

import numpy as np

from .evaluator import Params, check, lib, _i32


def _u32(seq):
    if seq is None:
        return None, 0
    arr = (C.c_uint32 * len(seq))(*seq)
    return arr, len(seq)


def keygen_raw(params, seed=(314, 1592, 657), with_cloud=True):
    """-> dict(lwe_key [n], tlwe_key [kN], bk, ksk) as numpy int32 (bk/ksk None if with_cloud=False)."""
    s, ns = _u32(seed)
    lwe = np.zeros(params.n, dtype=np.int32)
    tlwe = np.zeros(params.k * params.N, dtype=np.int32)
    bk = np.zeros(params.bk_count, dtype=np.int32) if with_cloud else None
    ksk = np.zeros(params.ksk_count, dtype=np.int32) if with_cloud else None
    check(lib().ieache_keygen_raw(C.byref(params), s, ns, _i32(lwe), _i32(tlwe),
                                  _i32(bk) if with_cloud else None, _i32(ksk) if with_cloud else None))
    if with_cloud:
        kpl = (params.k + 1) * params.l
        bk = bk.reshape(params.n, kpl, params.k + 1, params.N)
        ksk = ksk.reshape(params.k * params.N, params.ks_t, 1 << params.ks_basebit, params.n + 1)
    return {"lwe_key": lwe, "tlwe_key": tlwe, "bk": bk, "ksk": ksk}


def keygen_files(directory, params=None, seed=None, nbit_seed=None):
    """keygen.c: writes secret.key, cloud.key, nbit.key into `directory`."""
    s, ns = _u32(seed)
    b, nb = _u32(nbit_seed)
    check(lib().ieache_keygen_files(os.fsencode(directory), C.byref(params) if params is not None else None,
                                    s, ns, b, nb))


def encrypt_bits(params, lwe_key, bits, seed):
    bits = np.ascontiguousarray(bits, dtype=np.uint8)
    lwe_key = np.ascontiguousarray(lwe_key, dtype=np.int32)
    out = np.zeros(bits.shape + (params.n + 1,), dtype=np.int32)
    check(lib().ieache_encrypt_bits(C.byref(params), _i32(lwe_key), bits.ctypes.data_as(C.POINTER(C.c_uint8)),
                                    bits.size, seed, _i32(out)))
    return out


def decrypt_bits(params, lwe_key, samples):
    samples = np.ascontiguousarray(samples, dtype=np.int32)
    lwe_key = np.ascontiguousarray(lwe_key, dtype=np.int32)
    shape = samples.shape[:-1]
    bits = np.zeros(shape, dtype=np.uint8)
    check(lib().ieache_decrypt_bits(C.byref(params), _i32(lwe_key), _i32(samples), int(np.prod(shape, dtype=np.int64)),
                                    bits.ctypes.data_as(C.POINTER(C.c_uint8))))
    return bits


def lut_test_poly(params, table):
    """Test polynomial [N] of a lookup table of Torus32 values for Context.pbs: messages m < len(table) encoded at phase
    m / (2 len(table)), every slot centred on its message (ieache_lut_test_poly; 2 len(table) must divide N)."""
    f = np.ascontiguousarray(table, dtype=np.int32).reshape(-1)
    v = np.zeros(params.N, dtype=np.int32)
    check(lib().ieache_lut_test_poly(C.byref(params), f.shape[0], _i32(f), _i32(v)))
    return v


def lut_factor_poly(params, table):
    """Factor polynomial [N] of a lookup table of small INTEGERS for Context.pbs_multi: P = v (1 - X) with v laid out as
    lut_test_poly lays a table out (ieache_lut_factor_poly; 2 len(table) must divide N).  After a rotation from the constant
    polynomial c, a message m < len(table) comes out as 2 c table[m] (+ bias)."""
    w = np.ascontiguousarray(table, dtype=np.int32).reshape(-1)
    P = np.zeros(params.N, dtype=np.int32)
    check(lib().ieache_lut_factor_poly(C.byref(params), w.shape[0], _i32(w), _i32(P)))
    return P


def tlwe_encrypt(params, tlwe_key, polys, seed, alpha=None):
    """TLWE encryptions under the ring key of polys [count][N] (or one [N]) -> [count][2][N], A then B with B = A s + poly + e:
    an encrypted table for Context.pbs(..., tlwe=True).  alpha None: the parameter set's tlwe_alpha_min; seed as for
    encrypt_bits (0: kernel entropy)."""
    polys = np.ascontiguousarray(polys, dtype=np.int32).reshape(-1, params.N)
    tlwe_key = np.ascontiguousarray(tlwe_key, dtype=np.int32)
    out = np.zeros((polys.shape[0], 2, params.N), dtype=np.int32)
    check(lib().ieache_tlwe_encrypt(C.byref(params), _i32(tlwe_key), _i32(polys), polys.shape[0], 0.0 if alpha is None else float(alpha),
                                    seed, _i32(out)))
    return out


def tlwe_phase(params, tlwe_key, samples):
    """Exact phase B - A s (negacyclic, mod 2^32) of TLWE samples [count][2][N] (or one [2][N]) -> [count][N]: the table behind
    an encryption, or the polynomial a returned accumulator (Context.pbs(..., accumulator=True)) holds."""
    samples = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, 2, params.N)
    tlwe_key = np.ascontiguousarray(tlwe_key, dtype=np.int32)
    phase = np.zeros((samples.shape[0], params.N), dtype=np.int32)
    check(lib().ieache_tlwe_phase(C.byref(params), _i32(tlwe_key), _i32(samples), samples.shape[0], _i32(phase)))
    return phase


def packing_keygen(params, lwe_key, tlwe_key, t=8, basebit=2, alpha=None, seed=0):
    """The packing key [n][t][2][N] for Context.set_packing_key: PK[i][j] a TLWE encryption under the ring key of the constant
    polynomial lwe_key[i] 2^(32 - (j+1) basebit).  Needs both secret keys.  alpha None: tlwe_alpha_min; seed as for tlwe_encrypt."""
    lwe_key = np.ascontiguousarray(lwe_key, dtype=np.int32)
    tlwe_key = np.ascontiguousarray(tlwe_key, dtype=np.int32)
    out = np.zeros((params.n, max(int(t), 0), 2, params.N), dtype=np.int32)
    check(lib().ieache_packing_keygen(C.byref(params), _i32(lwe_key), _i32(tlwe_key), int(t), int(basebit), 0.0 if alpha is None else float(alpha),
                                      seed, _i32(out)))
    return out


def pack_reference(params, pk, rows, m=None, spread=1, shift=0, t=8, basebit=2):
    """CPU reference of Context.pack on raw arrays (ieache_pack_reference; no GPU, no context): pk [n][t][2][N],
    rows [groups][m][n+1] (or [m][n+1]; or any [..][n+1] with m given) -> [groups][2][N]."""
    pk = np.ascontiguousarray(pk, dtype=np.int32)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    if m is None:
        m = rows.shape[-2]
    m = int(m)
    rows = rows.reshape(-1, params.n + 1)
    groups = rows.shape[0] // m if m >= 1 else 0
    out = np.zeros((groups, 2, params.N), dtype=np.int32)
    check(lib().ieache_pack_reference(C.byref(params), int(t), int(basebit), _i32(pk), groups, m, int(spread), int(shift), _i32(rows), _i32(out)))
    return out


def projection_params(params):
    """The parameter set on which the projection is the packing key switch: n := N (the source key is the ring key)."""
    return params.copy(n=params.N)


def projection_keygen(params, tlwe_key, t=8, basebit=2, alpha=None, seed=0):
    """The projection key [N][t][2][N] for Context.set_projection_key: packing_keygen on projection_params(params) with the ring
    key's N words as the source key (include/ieache.h section 3l).  Needs the ring key only."""
    return packing_keygen(projection_params(params), tlwe_key, tlwe_key, t=t, basebit=basebit, alpha=alpha, seed=seed)


def tlwe_project_reference(params, pk, tlwe, first=0, width=1, dest=0, t=8, basebit=2):
    """CPU reference of Context.tlwe_project on raw arrays (ieache_tlwe_project_reference: the references of tlwe_extract and
    pack composed; no GPU, any supported set): pk [N][t][2][N], tlwe [count][2][N] (or one) -> [count][2][N]."""
    pk = np.ascontiguousarray(pk, dtype=np.int32)
    tlwe = np.ascontiguousarray(tlwe, dtype=np.int32).reshape(-1, 2, params.N)
    out = np.zeros_like(tlwe)
    check(lib().ieache_tlwe_project_reference(C.byref(params), int(t), int(basebit), _i32(pk), tlwe.shape[0], int(first), int(width), int(dest),
                                              _i32(tlwe), _i32(out)))
    return out


def lut_write_coef_reference(params, samples, pk, mem, depth, steps, new, width=1, unit=None, sel_of=None, t=8, basebit=2):
    """CPU reference of Context.lut_write_coef on raw arrays (ieache_lut_write_coef_reference: the references of lut_tree,
    tlwe_rotate, tlwe_project and lut_add composed), arguments as there; pk [N][t][2][N] or None (refused: no key)."""
    depth, steps, width = int(depth), int(steps), int(width)
    unit = width if unit is None else int(unit)
    kpl = (params.k + 1) * params.l
    samples = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, kpl, 2, params.N)
    pk = None if pk is None else np.ascontiguousarray(pk, dtype=np.int32)
    mem = np.ascontiguousarray(mem, dtype=np.int32).reshape(-1, 1 << max(depth, 0), 2, params.N)
    new = np.ascontiguousarray(new, dtype=np.int32).reshape(-1, 2, params.N)
    count = mem.shape[0]
    of = None if sel_of is None else np.ascontiguousarray(sel_of, dtype=np.int32).reshape(-1, max(depth + steps, 1))
    assert new.shape[0] == count and (of is None or depth + steps < 1 or of.shape[0] == count)
    out = np.zeros_like(mem)
    check(lib().ieache_lut_write_coef_reference(C.byref(params), _i32(samples), samples.shape[0], int(t), int(basebit), None if pk is None else _i32(pk),
                                                count, depth, steps, width, unit, None if of is None else _i32(of), _i32(new), _i32(mem), _i32(out)))
    return out


def lut_pack_layout(params, entries):
    """(spread, shift) with which Context.pack of `entries` encrypted table entries f[e] gives an encryption of exactly
    lut_test_poly(f): a table for Context.pbs(..., tlwe=True) built from encrypted results.  2 entries must divide N."""
    entries = int(entries)
    if entries < 1 or params.N % (2 * entries):
        raise ValueError("lut_pack_layout: 2 x entries must divide N")
    return params.N // entries, 2 * params.N - params.N // (2 * entries)


def tgsw_encrypt(params, tlwe_key, mu, seed, alpha=None):
    """TGSW samples under the ring key of the int32 messages mu [count] (or one; selector bits are 0 / 1) -> [count][2l][2][N]:
    what Context.tgsw_prepare takes, made by the routine key generation makes BK_i with.  alpha None: tlwe_alpha_min; seed as for
    tlwe_encrypt."""
    mu = np.ascontiguousarray(mu, dtype=np.int32).reshape(-1)
    tlwe_key = np.ascontiguousarray(tlwe_key, dtype=np.int32)
    out = np.zeros((mu.shape[0], (params.k + 1) * params.l, 2, params.N), dtype=np.int32)
    check(lib().ieache_tgsw_encrypt(C.byref(params), _i32(tlwe_key), _i32(mu), mu.shape[0], 0.0 if alpha is None else float(alpha), seed, _i32(out)))
    return out


def trivial_tlwe(polys):
    """Plain polynomials [count][N] (or one [N]) as noiseless TLWE samples with A = 0: [count][2][N]."""
    polys = np.ascontiguousarray(polys, dtype=np.int32)
    polys = polys.reshape(-1, polys.shape[-1])
    return np.ascontiguousarray(np.stack([np.zeros_like(polys), polys], axis=1))


def cmux_reference(params, samples, d1, d0=None, sel_of=None):
    """CPU reference of Context.cmux on raw arrays (ieache_cmux_reference; no GPU, no context, any supported set):
    samples [n][2l][2][N], d1 / d0 [count][2][N] -> [count][2][N]."""
    kpl = (params.k + 1) * params.l
    samples = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, kpl, 2, params.N)
    d1 = np.ascontiguousarray(d1, dtype=np.int32).reshape(-1, 2, params.N)
    d0 = None if d0 is None else np.ascontiguousarray(d0, dtype=np.int32).reshape(-1, 2, params.N)
    of = None if sel_of is None else np.ascontiguousarray(sel_of, dtype=np.int32).reshape(-1)
    assert (d0 is None or d0.shape == d1.shape) and (of is None or of.shape[0] == d1.shape[0])
    out = np.zeros_like(d1)
    check(lib().ieache_cmux_reference(C.byref(params), _i32(samples), samples.shape[0], d1.shape[0], None if of is None else _i32(of), _i32(d1),
                                      None if d0 is None else _i32(d0), _i32(out)))
    return out


def lut_tree_reference(params, samples, tables, depth, sel_of=None, table_of=None, count=None):
    """CPU reference of Context.lut_tree on raw arrays (ieache_lut_tree_reference), arguments as there."""
    depth = int(depth)
    kpl = (params.k + 1) * params.l
    samples = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, kpl, 2, params.N)
    tables = np.ascontiguousarray(tables, dtype=np.int32).reshape(-1, 1 << max(depth, 0), 2, params.N)
    of = None if sel_of is None else np.ascontiguousarray(sel_of, dtype=np.int32).reshape(-1, max(depth, 1))
    tof = None if table_of is None else np.ascontiguousarray(table_of, dtype=np.int32).reshape(-1)
    if count is None:
        count = tof.shape[0] if tof is not None else (of.shape[0] if of is not None and depth > 0 else 1)
    out = np.zeros((count, 2, params.N), dtype=np.int32)
    check(lib().ieache_lut_tree_reference(C.byref(params), _i32(samples), samples.shape[0], count, depth, None if of is None else _i32(of),
                                          _i32(tables), tables.shape[0], None if tof is None else _i32(tof), _i32(out)))
    return out


def lut_scatter_reference(params, samples, values, depth, sel_of=None, mem=None, count=None):
    """CPU reference of Context.lut_scatter on raw arrays (ieache_lut_scatter_reference; any supported set), arguments as there."""
    depth = int(depth)
    kpl = (params.k + 1) * params.l
    samples = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, kpl, 2, params.N)
    values = np.ascontiguousarray(values, dtype=np.int32).reshape(-1, 2, params.N)
    n = values.shape[0] if count is None else int(count)
    of = None if sel_of is None else np.ascontiguousarray(sel_of, dtype=np.int32).reshape(-1, max(depth, 1))
    mem = None if mem is None else np.ascontiguousarray(mem, dtype=np.int32).reshape(-1, 1 << max(depth, 0), 2, params.N)
    assert values.shape[0] == n and (of is None or depth < 1 or of.shape[0] == n) and (mem is None or mem.shape[0] == n)
    out = np.zeros((n, 1 << max(depth, 0), 2, params.N), dtype=np.int32)
    check(lib().ieache_lut_scatter_reference(C.byref(params), _i32(samples), samples.shape[0], n, depth, None if of is None else _i32(of),
                                             _i32(values), None if mem is None else _i32(mem), _i32(out)))
    return out


def lut_write_reference(params, samples, mem, depth, new, sel_of=None):
    """CPU reference of Context.lut_write / lut_write_device on raw arrays: the composition of the two C references -- the tree
    over each item's own memory, the wrapping subtraction, the scatter of the difference.  Arguments as Context.lut_write."""
    depth = int(depth)
    mem = np.ascontiguousarray(mem, dtype=np.int32).reshape(-1, 1 << max(depth, 0), 2, params.N)
    new = np.ascontiguousarray(new, dtype=np.int32).reshape(-1, 2, params.N)
    count = mem.shape[0]
    assert new.shape[0] == count
    old = lut_tree_reference(params, samples, mem, depth, sel_of=sel_of, table_of=np.arange(count, dtype=np.int32), count=count)
    delta = ((new.astype(np.int64) - old.astype(np.int64)) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    return lut_scatter_reference(params, samples, delta, depth, sel_of=sel_of, mem=mem, count=count)


def with_gadget(params, l, Bgbit):
    """A copy of `params` with the gadget (l, Bgbit): what tgsw_encrypt and every *_reference here take for a TGSW set with a
    gadget of its own (Context.tgsw_prepare(samples, l, Bgbit)).  `params` itself is left alone."""
    return params.copy(l=int(l), Bgbit=int(Bgbit))


def rotate_amounts(steps, unit=1, toward_zero=True, N=1024):
    """The public amounts of Context.tlwe_rotate / lut_read for address bits of weight unit 2^t, t = 0 .. steps-1, mod 2N:
    2N - unit 2^t (toward_zero: coefficient unit sum b_t 2^t comes to position 0 -- the read; unit = 1 is the calls' default) or
    unit 2^t (coefficient 0 goes to that position -- the write) -> int32 [steps].  N: the ring's degree."""
    two_n = 2 * int(N)
    w = np.array([(int(unit) << t) % two_n for t in range(int(steps))], dtype=np.int64)
    return ((two_n - w) % two_n if toward_zero else w).astype(np.int32)


def tlwe_rotate_reference(params, samples, rows, steps, sel_of=None, amounts=None):
    """CPU reference of Context.tlwe_rotate on raw arrays (ieache_tlwe_rotate_reference; no GPU, any supported set), arguments as
    there."""
    steps = int(steps)
    kpl = (params.k + 1) * params.l
    samples = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, kpl, 2, params.N)
    rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 2, params.N)
    of = None if sel_of is None else np.ascontiguousarray(sel_of, dtype=np.int32).reshape(-1, max(steps, 1))
    am = None if amounts is None else np.ascontiguousarray(amounts, dtype=np.int32).reshape(-1)
    assert (of is None or steps < 1 or of.shape[0] == rows.shape[0]) and (am is None or am.shape[0] == max(steps, 0))
    out = np.zeros_like(rows)
    check(lib().ieache_tlwe_rotate_reference(C.byref(params), _i32(samples), samples.shape[0], rows.shape[0], steps, None if of is None else _i32(of),
                                             None if am is None else _i32(am), _i32(rows), _i32(out)))
    return out


def lut_read_reference(params, samples, tables, depth, steps, sel_of=None, amounts=None, table_of=None, coef=0, ksk=None, count=None):
    """CPU reference of Context.lut_read on raw arrays (ieache_lut_read_reference), arguments as there; ksk: the key-switch key
    [N][t][base][n+1] as keygen_raw gives it -> [count][n+1], or None: no key switch, the extracted rows [count][N+1]."""
    depth, steps = int(depth), int(steps)
    kpl = (params.k + 1) * params.l
    samples = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, kpl, 2, params.N)
    tables = np.ascontiguousarray(tables, dtype=np.int32).reshape(-1, 1 << max(depth, 0), 2, params.N)
    of = None if sel_of is None else np.ascontiguousarray(sel_of, dtype=np.int32).reshape(-1, max(depth + steps, 1))
    am = None if amounts is None else np.ascontiguousarray(amounts, dtype=np.int32).reshape(-1)
    tof = None if table_of is None else np.ascontiguousarray(table_of, dtype=np.int32).reshape(-1)
    ksk = None if ksk is None else np.ascontiguousarray(ksk, dtype=np.int32)
    if count is None:
        count = tof.shape[0] if tof is not None else (of.shape[0] if of is not None and depth + steps > 0 else 1)
    assert am is None or am.shape[0] == max(steps, 0)
    out = np.zeros((count, (params.N if ksk is None else params.n) + 1), dtype=np.int32)
    check(lib().ieache_lut_read_reference(C.byref(params), _i32(samples), samples.shape[0], None if ksk is None else _i32(ksk), count, depth, steps,
                                          None if of is None else _i32(of), None if am is None else _i32(am), _i32(tables), tables.shape[0],
                                          None if tof is None else _i32(tof), int(coef), 1 if ksk is None else 0, _i32(out)))
    return out


def lut_add_reference(params, samples, values, depth, steps=0, sel_of=None, amounts=None, mems=None, n_mems=1, mem_of=None):
    """CPU reference of Context.lut_add on raw arrays (ieache_lut_add_reference: the references of tlwe_rotate and lut_scatter
    composed and the leaves summed per memory; no GPU, any supported set), arguments as there -> [n_mems][2^depth][2][N]."""
    depth, steps = int(depth), int(steps)
    kpl = (params.k + 1) * params.l
    samples = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, kpl, 2, params.N)
    values = np.ascontiguousarray(values, dtype=np.int32).reshape(-1, 2, params.N)
    count = values.shape[0]
    of = None if sel_of is None else np.ascontiguousarray(sel_of, dtype=np.int32).reshape(-1, max(depth + steps, 1))
    am = None if amounts is None else np.ascontiguousarray(amounts, dtype=np.int32).reshape(-1)
    mof = None if mem_of is None else np.ascontiguousarray(mem_of, dtype=np.int32).reshape(-1)
    if mems is not None:
        mems = np.ascontiguousarray(mems, dtype=np.int32).reshape(-1, 1 << max(depth, 0), 2, params.N)
        n_mems = mems.shape[0]
    n_mems = int(n_mems)
    assert (of is None or depth + steps < 1 or of.shape[0] == count) and (am is None or am.shape[0] == max(steps, 0))
    assert mof is None or mof.shape[0] == count
    out = np.zeros((max(n_mems, 0), 1 << max(depth, 0), 2, params.N), dtype=np.int32)
    check(lib().ieache_lut_add_reference(C.byref(params), _i32(samples), samples.shape[0], count, depth, steps, None if of is None else _i32(of),
                                         None if am is None else _i32(am), _i32(values), None if mems is None else _i32(mems), n_mems,
                                         None if mof is None else _i32(mof), _i32(out)))
    return out


def automaton_check(next0, next1, n_out=1):
    """ieache_automaton_check: the validation of Context.automaton with no context and no GPU; raises IeacheError naming the
    first rule broken."""
    from .evaluator import automaton_tables
    next0, next1 = automaton_tables(next0, next1)
    check(lib().ieache_automaton_check(next0.shape[1], next0.shape[0], int(n_out), _i32(next0), _i32(next1)))


def automaton_reference(params, samples, next0, next1, finals, n_out=1, sel_of=None, final_of=None, count=None):
    """CPU reference of Context.automaton_run on raw arrays (ieache_automaton_reference: the CMux reference composed; no GPU,
    any supported set): samples [n][2l][2][N], tables [steps][states], finals [n_finals][states][2][N] -> [count][n_out][2][N]."""
    from .evaluator import automaton_tables
    next0, next1 = automaton_tables(next0, next1)
    steps, states = next0.shape
    kpl = (params.k + 1) * params.l
    samples = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, kpl, 2, params.N)
    finals = np.ascontiguousarray(finals, dtype=np.int32).reshape(-1, max(states, 1), 2, params.N)
    of = None if sel_of is None else np.ascontiguousarray(sel_of, dtype=np.int32).reshape(-1, max(steps, 1))
    fof = None if final_of is None else np.ascontiguousarray(final_of, dtype=np.int32).reshape(-1)
    if count is None:
        count = fof.shape[0] if fof is not None else (of.shape[0] if of is not None and steps > 0 else 1)
    assert (fof is None or fof.shape[0] == count) and (of is None or steps < 1 or of.shape[0] == count)
    out = np.zeros((count, max(int(n_out), 0), 2, params.N), dtype=np.int32)
    check(lib().ieache_automaton_reference(C.byref(params), _i32(samples), samples.shape[0], states, steps, int(n_out), _i32(next0), _i32(next1), count,
                                           None if of is None else _i32(of), _i32(finals), finals.shape[0], None if fof is None else _i32(fof), _i32(out)))
    return out


def lwe_linear_reference(params, x, W, bias=None, rows="lwe"):
    """CPU reference of Context.lwe_linear (ieache_lwe_linear_reference; no GPU, no context): x [batch][n_in][words], W an
    integer matrix [n_out][n_in] in -128 .. 127, bias [n_out] or None, rows "lwe" / "extracted" / "tlwe" -> [batch][n_out][words]."""
    from .evaluator import linear_rows_kind, linear_row_words, linear_weights, _i8, _opt
    kind = linear_rows_kind(rows)
    W, bias = linear_weights(W, bias)
    x = np.ascontiguousarray(x, dtype=np.int32)
    words = linear_row_words(params, kind)
    if words is not None:
        if x.ndim < 2 or x.shape[-1] != words or x.shape[-2] != W.shape[1]:
            raise ValueError("lwe_linear: x must be [batch][n_in = %d][words = %d]" % (W.shape[1], words))
        x = x.reshape(-1, W.shape[1], words)
    out = np.zeros((x.shape[0], W.shape[0], x.shape[-1]), dtype=np.int32)
    check(lib().ieache_lwe_linear_reference(C.byref(params), kind, x.shape[0], W.shape[0], W.shape[1], _i8(W), _opt(bias), _i32(x), _i32(out)))
    return out


def tlwe_extract_reference(params, tlwe, coef_of=None):
    """CPU reference of Context.tlwe_extract (ieache_tlwe_extract_reference): tlwe [count][2][N] -> [count][N+1]."""
    tlwe = np.ascontiguousarray(tlwe, dtype=np.int32).reshape(-1, 2, params.N)
    of = None if coef_of is None else np.ascontiguousarray(coef_of, dtype=np.int32).reshape(-1)
    assert of is None or of.shape[0] == tlwe.shape[0]
    u = np.zeros((tlwe.shape[0], params.N + 1), dtype=np.int32)
    check(lib().ieache_tlwe_extract_reference(C.byref(params), tlwe.shape[0], _i32(tlwe), None if of is None else _i32(of), _i32(u)))
    return u


def unpack_reference(params, tlwe, first=0, width=1, spread=1, ksk=None):
    """CPU reference of Context.unpack on raw arrays (ieache_unpack_reference: the references of tlwe_extract and the key switch
    composed; no GPU, any supported set): tlwe [count][2][N]; ksk: the key-switch key [N][t][base][n+1] as keygen_raw gives it
    -> [count][width][n+1], or None: no key switch, the extracted rows [count][width][N+1]."""
    tlwe = np.ascontiguousarray(tlwe, dtype=np.int32).reshape(-1, 2, params.N)
    ksk = None if ksk is None else np.ascontiguousarray(ksk, dtype=np.int32)
    out = np.zeros((tlwe.shape[0], max(int(width), 0), (params.N if ksk is None else params.n) + 1), dtype=np.int32)
    check(lib().ieache_unpack_reference(C.byref(params), None if ksk is None else _i32(ksk), tlwe.shape[0], int(first), int(width), int(spread),
                                        _i32(tlwe), 1 if ksk is None else 0, _i32(out)))
    return out


def word_read_reference(params, samples, tables, depth, steps, width=1, unit=None, sel_of=None, table_of=None, ksk=None, count=None):
    """CPU reference of Context.word_read on raw arrays (ieache_word_read_reference: the references of lut_tree, tlwe_rotate and
    unpack composed), arguments as there; ksk as for unpack_reference."""
    depth, steps, width = int(depth), int(steps), int(width)
    unit = width if unit is None else int(unit)
    kpl = (params.k + 1) * params.l
    samples = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, kpl, 2, params.N)
    tables = np.ascontiguousarray(tables, dtype=np.int32).reshape(-1, 1 << max(depth, 0), 2, params.N)
    of = None if sel_of is None else np.ascontiguousarray(sel_of, dtype=np.int32).reshape(-1, max(depth + steps, 1))
    tof = None if table_of is None else np.ascontiguousarray(table_of, dtype=np.int32).reshape(-1)
    ksk = None if ksk is None else np.ascontiguousarray(ksk, dtype=np.int32)
    if count is None:
        count = tof.shape[0] if tof is not None else (of.shape[0] if of is not None and depth + steps > 0 else 1)
    out = np.zeros((count, max(width, 0), (params.N if ksk is None else params.n) + 1), dtype=np.int32)
    check(lib().ieache_word_read_reference(C.byref(params), _i32(samples), samples.shape[0], None if ksk is None else _i32(ksk), count, depth, steps,
                                           width, unit, None if of is None else _i32(of), _i32(tables), tables.shape[0],
                                           None if tof is None else _i32(tof), 1 if ksk is None else 0, _i32(out)))
    return out


def int_to_bits(value, nbits):
    return np.array([(int(value) >> i) & 1 for i in range(nbits)], dtype=np.uint8)


def bits_to_int(bits):
    return sum(int(b) << i for i, b in enumerate(np.asarray(bits).reshape(-1)))


def read_secret_key(path):
    p = Params()
    check(lib().ieache_read_secret_key(os.fsencode(path), C.byref(p), None, None))
    lwe = np.zeros(p.n, dtype=np.int32)
    tlwe = np.zeros(p.k * p.N, dtype=np.int32)
    check(lib().ieache_read_secret_key(os.fsencode(path), C.byref(p), _i32(lwe), _i32(tlwe)))
    return p, lwe, tlwe


def read_cloud_key(path):
    p = Params()
    check(lib().ieache_read_cloud_key(os.fsencode(path), C.byref(p), None, None))
    bk = np.zeros(p.bk_count, dtype=np.int32)
    ksk = np.zeros(p.ksk_count, dtype=np.int32)
    check(lib().ieache_read_cloud_key(os.fsencode(path), C.byref(p), _i32(bk), _i32(ksk)))
    return p, bk, ksk


def write_cloud_key(path, params, bk, ksk):
    bk = np.ascontiguousarray(bk, dtype=np.int32)
    ksk = np.ascontiguousarray(ksk, dtype=np.int32)
    check(lib().ieache_write_cloud_key(os.fsencode(path), C.byref(params), _i32(bk), _i32(ksk)))


def write_secret_key(path, params, lwe_key, tlwe_key, bk, ksk):
    arrs = [np.ascontiguousarray(a, dtype=np.int32) for a in (lwe_key, tlwe_key, bk, ksk)]
    check(lib().ieache_write_secret_key(os.fsencode(path), C.byref(params), *[_i32(a) for a in arrs]))


def read_samples(path, n, first=0, count=None):
    if count is None:
        count = os.path.getsize(path) // (4 * n + 16) - first
    out = np.zeros((count, n + 1), dtype=np.int32)
    check(lib().ieache_read_samples(os.fsencode(path), n, first, count, _i32(out)))
    return out


def write_samples(path, rows, append=False):
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    n = rows.shape[-1] - 1
    check(lib().ieache_write_samples(os.fsencode(path), n, rows.size // (n + 1), _i32(rows), int(append)))


def alice(directory, sign_code, bit_size, value, seed, append=False, cloud_data="cloud.data"):
    """alice.c: encrypt one operand (magnitude `value`, sign code 0/1/2) into cloud.data."""
    words = [(int(value) >> (32 * w)) & 0xFFFFFFFF for w in range(8)]
    arr = (C.c_uint32 * 8)(*words)
    d = os.fspath(directory)
    check(lib().ieache_alice(os.fsencode(os.path.join(d, "secret.key")), os.fsencode(os.path.join(d, "nbit.key")),
                             os.fsencode(os.path.join(d, cloud_data)), int(append), sign_code, bit_size, arr, seed))


def verif(directory, answer_data="answer.data"):
    """verif.c decrypt step -> (sign_code, bit_size, [9 words])."""
    d = os.fspath(directory)
    code, bits = C.c_uint32(), C.c_uint32()
    words = (C.c_uint32 * 9)()
    check(lib().ieache_verif(os.fsencode(os.path.join(d, "secret.key")), os.fsencode(os.path.join(d, "nbit.key")),
                             os.fsencode(os.path.join(d, answer_data)), C.byref(code), C.byref(bits), words))
    return code.value, bits.value, list(words)


def verif_interpret(op, sign_code, bit_size, words):
    """Output/verif.c's reconstruction rules -> Python int.

    op: operator.txt code (1 add, 2 sub, 4 mul).  Words are LSW first
    (verif.c:229).  ADD (verif.c:120-179): codes 0/4 read the magnitude
    unsigned (4 negates); codes 1/2 read two's complement.  SUB
    (verif.c:733-789): code 2 unsigned, otherwise two's complement, code 1
    negates.  MUL (verif.c:1409-1435): unsigned, codes 1/2 negate."""
    nwords = bit_size // 32
    total = 0
    for w in reversed(range(nwords)):
        total = (total << 32) | (words[w] & 0xFFFFFFFF)
    top = 1 << (bit_size - 1)

    def twos(v):
        return v - (1 << bit_size) if v & top else v

    if op == 1:
        if sign_code in (0, 4):
            return -total if sign_code == 4 else total
        return twos(total)
    if op == 2:
        v = total if sign_code == 2 else twos(total)
        return -v if sign_code == 1 else v
    if op == 4:
        return -total if sign_code in (1, 2) else total
    raise ValueError("unknown operator code %r" % (op,))
