"""Device groups behind the C ABI (include/ieache.h section 2b), as far as a machine without a GPU can tell: every symbol is
exported and bound with its declared shape, the creation arguments are judged before the first HIP call -- so the refusals
read the same here as on the card --, and every group form refuses a NULL group."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (result, number of parameters) as include/ieache.h declares them
DECLARED = {
    "ieache_group_create": ("ieache_group*", 3),
    "ieache_group_create_raw": ("ieache_group*", 5),
    "ieache_group_destroy": ("void", 1),
    "ieache_group_size": ("int", 1),
    "ieache_group_device": ("int", 2),
    "ieache_group_ctx": ("ieache_ctx*", 2),
    "ieache_group_set_option": ("int", 3),
    "ieache_group_prepare_batch": ("int", 4),
    "ieache_group_eval_batch": ("int", 7),
    "ieache_group_prepare_netlist": ("int", 3),
    "ieache_group_eval_netlist": ("int", 6),
    "ieache_group_gates": ("int", 7),
    "ieache_group_gates3": ("int", 8),
    "ieache_group_mux": ("int", 7),
    "ieache_group_pbs": ("int", 9),
    "ieache_group_pbs_multi": ("int", 12),
}


def _header():
    with open(os.path.join(ROOT, "include", "ieache.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_every_group_symbol_is_declared_exported_and_bound(ia):
    hdr = _header()
    assert re.search(r"#define\s+IEACHE_GROUP_MAX_DEVICES\s+16\b", hdr) and ia.GROUP_MAX_DEVICES == 16
    assert "typedef struct ieache_group ieache_group;" in hdr
    declared = {m.group(2): (m.group(1).replace(" ", ""), m.group(3)) for m in
                re.finditer(r"^([a-z_0-9]+ ?\*?)\s*(ieache_group_[a-z_0-9]+)\s*\(([^;]*)\)\s*;", hdr, re.M)}
    assert set(declared) == set(DECLARED)
    raw, L = C.CDLL(ia.library_path()), ia.lib()
    for name, (result, n_params) in DECLARED.items():
        got_result, params = declared[name]
        assert got_result == result, name
        assert len(params.split(",")) == n_params, name
        assert params.split(",")[0].strip() in ("ieache_group* g", "const ieache_group* g") or name.startswith("ieache_group_create"), name
        assert hasattr(raw, name), name
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n_params, name  # the Python binding passes what the header declares
        assert (fn.restype is None) == (result == "void") and (fn.restype is C.c_void_p) == result.endswith("*"), name
    # the evaluating forms carry the context form's arguments behind the group, and the statistics last
    for name in ("eval_batch", "eval_netlist", "gates", "gates3", "mux", "pbs", "pbs_multi"):
        ctx_form, group_form = getattr(L, "ieache_" + name), getattr(L, "ieache_group_" + name)
        assert list(group_form.argtypes[1:]) == list(ctx_form.argtypes[1:]), name
        assert re.search(r"ieache_stats\* stats\s*\)\s*;", declared["ieache_group_" + name][1] + ");"), name
    assert ia.Group is ia.evaluator.Group


@pytest.fixture(scope="module")
def toy_key(ia):
    from ieache_amd import tools
    p = ia.default_params().copy(n=4, N=64)
    k = tools.keygen_raw(p, (1, 2, 3))
    return p, np.ascontiguousarray(k["bk"], dtype=np.int32), np.ascontiguousarray(k["ksk"], dtype=np.int32)


def _create_raw(ia, p, bk, ksk, devices, n):
    L = ia.lib()
    i32p = C.POINTER(C.c_int32)
    arr = None if devices is None else (C.c_int * max(len(devices), 1))(*devices)
    h = L.ieache_group_create_raw(C.byref(p), bk.ctypes.data_as(i32p), ksk.ctypes.data_as(i32p), arr, n)
    return h, L.ieache_last_error().decode()


@pytest.mark.parametrize("devices,n,names", [
    ([0], 0, "n_devices"),
    (list(range(17)), 17, "n_devices"),
    (None, 1, "devices"),
    ([0, -1], 2, "devices[1]"),
])
def test_creation_refuses_a_bad_device_list_before_any_hip_call(ia, toy_key, devices, n, names):
    p, bk, ksk = toy_key
    h, msg = _create_raw(ia, p, bk, ksk, devices, n)
    assert not h and names in msg, msg
    assert "HIP" not in msg and "member" not in msg, msg  # nobody asked the runtime
    # the file form judges the list before it opens the file
    arr = None if devices is None else (C.c_int * max(len(devices), 1))(*devices)
    assert not ia.lib().ieache_group_create(b"/nonexistent/cloud.key", arr, n)
    assert names in ia.lib().ieache_last_error().decode()


def test_creation_refuses_an_unsupported_parameter_set_before_any_hip_call(ia, toy_key):
    p, bk, ksk = toy_key
    h, msg = _create_raw(ia, p.copy(k=2), bk, ksk, [0], 1)
    assert not h and "parameter set" in msg and "HIP" not in msg and "member" not in msg, msg
    with pytest.raises(ia.IeacheError) as e:
        ia.Group.from_arrays(p.copy(N=48), np.zeros(p.copy(N=48).bk_count, np.int32), np.zeros(p.copy(N=48).ksk_count, np.int32), [0, 0])
    assert e.value.code == -22 and "parameter set" in str(e.value)
    # a missing file is an I/O error that names the file, once the list has passed
    assert not ia.lib().ieache_group_create(b"/nonexistent/cloud.key", (C.c_int * 2)(0, 0), 2)
    assert "/nonexistent/cloud.key" in ia.lib().ieache_last_error().decode()
    assert not ia.lib().ieache_group_create(None, (C.c_int * 1)(0), 1) and "cloud_key_path" in ia.lib().ieache_last_error().decode()


def test_a_valid_list_naming_a_device_that_is_not_there_fails_cleanly(ia, toy_key):
    """Index device_count() is the first device the machine does not have -- 0 on a machine without a GPU, where the runtime
    itself reports no device: creation fails in the first member, names member and device, and leaves nothing behind."""
    p, bk, ksk = toy_key
    absent = ia.device_count()
    h, msg = _create_raw(ia, p, bk, ksk, [absent, absent], 2)
    assert not h and msg.startswith("member 0 (device %d): " % absent) and "device" in msg.split(": ", 1)[1], msg
    with pytest.raises(ia.IeacheError) as e:
        ia.Group.from_arrays(p, bk, ksk, (absent,))
    assert e.value.code == -19
    assert not _create_raw(ia, p, bk, ksk, [absent], 1)[0]  # and again


def test_group_forms_refuse_a_null_group(ia):
    L = ia.lib()
    EINVAL = -22
    calls = {
        "ieache_group_size": (None,),
        "ieache_group_device": (None, 0),
        "ieache_group_set_option": (None, b"chunk", 1),
        "ieache_group_prepare_batch": (None, ia.CIRC_ADD, 16, 1),
        "ieache_group_eval_batch": (None, ia.CIRC_ADD, 16, 0, None, None, None),
        "ieache_group_prepare_netlist": (None, None, 1),
        "ieache_group_eval_netlist": (None, None, 0, None, None, None),
        "ieache_group_gates": (None, ia.GATE_AND, 0, None, None, None, None),
        "ieache_group_gates3": (None, ia.GATE_MAJ3, 0, None, None, None, None, None),
        "ieache_group_mux": (None, 0, None, None, None, None, None),
        "ieache_group_pbs": (None, 0, None, None, 1, None, None, 0, None),
        "ieache_group_pbs_multi": (None, 0, None, None, 1, None, None, 1, None, None, 0, None),
    }
    assert set(calls) | {"ieache_group_create", "ieache_group_create_raw", "ieache_group_destroy", "ieache_group_ctx"} == set(DECLARED)
    for name, args in calls.items():
        assert getattr(L, name)(*args) == EINVAL, name
        assert "null group" in L.ieache_last_error().decode(), name
    assert L.ieache_group_ctx(None, 0) is None and "null group" in L.ieache_last_error().decode()
    L.ieache_group_destroy(None)  # like free(NULL)
