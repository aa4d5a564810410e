"""TGSW sets with a gadget of their own and the replace write (include/ieache.h section 3i) without a GPU: tools.with_gadget, the C
references at the gadgets such a set may carry against the numpy restatements word for word (the definition the card is held
to in tests/test_gadget_gpu.py), the sequence of twelve worst-case replace writes by meaning at (6, 5) and at the key's (3, 7),
tools.lut_write_reference against its composition written out, and the declarations."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cmux_reference as CR
import gadget_sequence as GS
import rotate_reference as RR
import scatter_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = GS.N
GADGETS = GS.TABLE + GS.RUNTIME_ONLY  # every gadget tests/test_gadget_gpu.py runs


def test_with_gadget_round_trips_and_leaves_its_argument_alone(ia):
    from ieache_amd import tools
    p = ia.default_params()
    before = bytes(p)
    q = tools.with_gadget(p, 6, 5)
    assert (q.l, q.Bgbit) == (6, 5) and bytes(p) == before and q is not p
    assert [getattr(q, f) for f, _ in p._fields_ if f not in ("l", "Bgbit")] == [getattr(p, f) for f, _ in p._fields_ if f not in ("l", "Bgbit")]
    back = tools.with_gadget(q, p.l, p.Bgbit)
    assert bytes(back) == before and (q.l, q.Bgbit) == (6, 5)
    # what the samples of such a set look like: 2l rows
    key = np.zeros(N, dtype=np.int32)
    assert tools.tgsw_encrypt(q.copy(N=N), key, [1], 7).shape == (1, 12, 2, N)


@pytest.mark.parametrize("l,Bgbit", GADGETS, ids=["l%d_Bg%d" % g for g in GADGETS])
def test_references_are_the_definition_at_every_gadget(ia, l, Bgbit):
    """N = 1024, full-range words: cmux with and without d0, lut_scatter of depth 2 onto a memory, tlwe_rotate of 2 steps."""
    from ieache_amd import tools
    p = tools.with_gadget(ia.default_params().copy(n=4, N=N), l, Bgbit)
    rng = np.random.default_rng(9800 + 100 * l + Bgbit)
    S = CR.full_range(rng, (2, 2 * l, 2, N))
    d1, d0 = CR.full_range(rng, (1, 2, N)), CR.full_range(rng, (1, 2, N))
    assert np.array_equal(tools.cmux_reference(p, S, d1, d0, sel_of=[1]), CR.cmux_rows(S, d1, d0, l, Bgbit, sel_of=[1]))
    mem = CR.full_range(rng, (1, 4, 2, N))
    sel = np.array([[1, 0]], dtype=np.int32)
    assert np.array_equal(tools.lut_scatter_reference(p, S, d1, 2, sel_of=sel, mem=mem), SR.lut_scatter(S, d1, 2, l, Bgbit, sel_of=sel, mem=mem))
    assert np.array_equal(tools.tlwe_rotate_reference(p, S, d0, 2, sel_of=sel), RR.tlwe_rotate(S, d0, 2, l, Bgbit, sel_of=sel))


def test_twelve_worst_case_writes_survive_at_6_5_and_not_at_3_7(ia, make_keys):
    """The sequence of gadget_sequence.write_sequence through tools.lut_write_reference.  With (6, 5) selectors every coefficient
    of every slot is within 2^-8 of what the slot should hold after EVERY write: a decoding condition (the reference gives at most
    7.6e-4 on these seeds).  With the key's own (3, 7) the same sequence is above 2^-8 after write 12 (4.33e-3; it crosses at
    write 11, 4.02e-3): deterministic integer arithmetic on committed seeds, and the reason a set carries its gadget."""
    kb = make_keys(630, N)
    fine = GS.write_sequence(kb.p, kb.tlwe_key, 6, 5)["errs"]
    coarse = GS.write_sequence(kb.p, kb.tlwe_key, 3, 7)["errs"]
    print("largest phase error after write w, selectors at (6, 5): " + " ".join("%.2e" % e for e in fine))
    print("largest phase error after write w, selectors at (3, 7): " + " ".join("%.2e" % e for e in coarse))
    assert len(fine) == len(coarse) == 12
    assert max(fine) < 2.0 ** -8
    assert coarse[-1] > 2.0 ** -8


@pytest.mark.parametrize("l,Bgbit", [(3, 7), (6, 5)])
def test_lut_write_reference_is_the_composition_written_out(ia, l, Bgbit):
    from ieache_amd import tools
    p = tools.with_gadget(ia.default_params().copy(n=4, N=N), l, Bgbit)
    rng = np.random.default_rng(9900 + l)
    S = CR.full_range(rng, (5, 2 * l, 2, N))
    for depth, sel in ((0, None), (1, None), (2, np.array([[4, 0], [1, 3], [2, 2]], dtype=np.int32))):
        mem, new = CR.full_range(rng, (3, 1 << depth, 2, N)), CR.full_range(rng, (3, 2, N))
        old = tools.lut_tree_reference(p, S, mem, depth, sel_of=sel, table_of=np.arange(3, dtype=np.int32), count=3)
        want = tools.lut_scatter_reference(p, S, SR.sub32(new, old), depth, sel_of=sel, mem=mem, count=3)
        got = tools.lut_write_reference(p, S, mem, depth, new, sel_of=sel)
        assert got.shape == (3, 1 << depth, 2, N) and np.array_equal(got, want), depth
    # depth 0 replaces the one slot word for word
    assert np.array_equal(tools.lut_write_reference(p, S, mem[:, :1], 0, new), new[:, None])


# name -> (result, number of parameters) as include/ieache.h declares them
DECLARED = {"ieache_tgsw_prepare_gadget": ("ieache_tgsw*", 5), "ieache_tgsw_prepare_gadget_device": ("ieache_tgsw*", 5),
            "ieache_tgsw_gadget": ("int", 3), "ieache_lut_write": ("int", 9), "ieache_lut_write_device": ("int", 9)}


def test_every_symbol_is_declared_exported_and_bound(ia):
    with open(os.path.join(ROOT, "include", "ieache.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = {m.group(2): (m.group(1).replace(" ", ""), m.group(3)) for m in
                re.finditer(r"^([a-z_0-9]+ ?\*?)\s*(ieache_(?:tgsw_prepare_gadget|tgsw_gadget|lut_write)[a-z_]*)\s*\(([^;]*)\)\s*;", hdr, re.M)}
    assert set(declared) == set(DECLARED)
    raw, L = C.CDLL(ia.library_path()), ia.lib()
    for name, (result, n_params) in DECLARED.items():
        assert declared[name][0] == result and len(declared[name][1].split(",")) == n_params, name
        assert hasattr(raw, name), name
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n_params, name
        assert (fn.restype is C.c_void_p) == (result != "int"), name
    assert len(L.ieache_lut_write.argtypes) == len(L.ieache_lut_write_device.argtypes)
    assert L.ieache_tgsw_prepare_gadget.argtypes[:3] == L.ieache_tgsw_prepare.argtypes
    for name in ("tgsw_prepare", "tgsw_prepare_device", "lut_write", "lut_write_device"):
        assert callable(getattr(ia.Context, name)), name
    from ieache_amd import tools
    assert callable(tools.lut_write_reference) and callable(tools.with_gadget)
