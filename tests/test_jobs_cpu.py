"""Several circuits' batches in one call (include/ieache.h section 3c), as far as a machine without a GPU can tell: the new
symbols are exported and bound with their declared shapes, the arguments capi.cpp can judge without a device are refused the
same way here as on the card, and a device group cuts a job list by ieache_shard_slice's rule."""
import ctypes as C
import os
import re

import numpy as np

from test_joint_plan_cpu import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22


def _text(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_every_new_symbol_is_declared_exported_and_bound(ia):
    hdr = _text("include", "ieache.h")
    assert "typedef ieache_stats ieache_eval_stats;" in hdr
    assert re.search(r"typedef struct ieache_job \{\s*int kind, bits;\s*const struct ieache_netlist\* netlist;\s*size_t batch;\s*"
                     r"const int32_t\* in_lwe;\s*int32_t\* out_lwe;\s*\} ieache_job;", hdr)
    for decl in ("int ieache_prepare_jobs(ieache_ctx* ctx, const ieache_job* jobs, size_t n_jobs);",
                 "int ieache_eval_jobs(ieache_ctx* ctx, const ieache_job* jobs, size_t n_jobs, ieache_eval_stats* stats);",
                 "int ieache_eval_jobs_device(ieache_ctx* ctx, const ieache_job* jobs, size_t n_jobs, ieache_eval_stats* stats);"):
        assert decl in hdr, decl
    # the group form lives with the group
    assert re.search(r'extern "C" int ieache_group_eval_jobs\(ieache_group\* g, const ieache_job\* jobs, size_t n_jobs, ieache_stats\* stats',
                     _text("ie-ache_amd", "csrc", "group.h"))
    raw, L = C.CDLL(ia.library_path()), ia.lib()
    for name, n_params in (("ieache_prepare_jobs", 3), ("ieache_eval_jobs", 4), ("ieache_eval_jobs_device", 4), ("ieache_group_eval_jobs", 4)):
        assert hasattr(raw, name), name
        assert len(getattr(L, name).argtypes) == n_params, name
    # ieache_job as the binding lays it out: two ints, a pointer, a size, two pointers
    assert C.sizeof(ia.Job) == 8 + 4 * C.sizeof(C.c_void_p)
    assert [f[0] for f in ia.Job._fields_] == ["kind", "bits", "netlist", "batch", "in_lwe", "out_lwe"]
    assert ia.Job.netlist.offset == 8 and ia.Job.batch.offset == 8 + C.sizeof(C.c_void_p)
    assert hasattr(ia.Context, "eval_jobs") and hasattr(ia.Context, "eval_jobs_device") and hasattr(ia.Context, "prepare_jobs")
    assert hasattr(ia.Group, "eval_jobs")
    # the daemon's option
    assert "--joint" in _text("ie-ache_amd", "csrc", "cloudd_main.cpp") and "bool joint = true;" in _text("ie-ache_amd", "csrc", "daemon.h")


def test_arguments_are_refused_without_a_device(ia):
    L = ia.lib()
    rows = np.zeros(4, dtype=np.int32)
    jobs = (ia.Job * 3)()
    for j in jobs:
        j.kind, j.bits, j.batch, j.in_lwe, j.out_lwe = ia.CIRC_ADD, 16, 2, rows.ctypes.data, rows.ctypes.data
    for call, tail in ((L.ieache_eval_jobs, (None,)), (L.ieache_eval_jobs_device, (None,)), (L.ieache_prepare_jobs, ())):
        # no context: refused, whatever the jobs are -- also none
        assert call(None, jobs, 3, *tail) == EINVAL and L.ieache_last_error() == b"null argument"
        assert call(None, None, 0, *tail) == EINVAL and L.ieache_last_error() == b"null argument"
        # a job list that is not there
        assert call(None, None, 2, *tail) == EINVAL and L.ieache_last_error() == b"null argument"
    # a NULL row pointer with a batch names its job, before the context is looked at; with batch 0 the pointers are not read
    jobs[1].out_lwe = None
    for call in (L.ieache_eval_jobs, L.ieache_eval_jobs_device):
        assert call(None, jobs, 3, None) == EINVAL and L.ieache_last_error() == b"job 1: null argument"
    jobs[1].batch = 0
    jobs[2].in_lwe = None
    assert L.ieache_eval_jobs(None, jobs, 3, None) == EINVAL and L.ieache_last_error() == b"job 2: null argument"
    assert L.ieache_prepare_jobs(None, jobs, 3) == EINVAL and L.ieache_last_error() == b"null argument"  # preparing reads no rows
    # the group form: a NULL group first
    assert L.ieache_group_eval_jobs(None, jobs, 3, None) == EINVAL and b"null group" in L.ieache_last_error()
    assert L.ieache_group_eval_jobs(None, None, 0, None) == EINVAL and b"null group" in L.ieache_last_error()


def test_a_group_cuts_a_job_list_by_ieache_shard_slice(tmp_path, ia):
    """shard_jobs (csrc/group_run.h), what ieache_group_eval_jobs and the daemon cut a job list with: every job a member keeps
    starts `first` expressions into the job's rows and holds `count` of them -- ieache_shard_slice's -- and jobs whose slice is
    empty are dropped (the program checks the pointers and the order itself)."""
    exe, env = build(tmp_path)
    import subprocess
    out = subprocess.run([str(exe), "--slices"], env=env, stdout=subprocess.PIPE, text=True, timeout=60, check=True).stdout
    L = ia.lib()
    first, count = C.c_size_t(0), C.c_size_t(0)
    lines = out.split("\n")[:-1]
    seen = set()
    for line in lines:
        batch, parts, part, got_first, got_count = (int(x) for x in line.split())
        assert L.ieache_shard_slice(batch, parts, part, C.byref(first), C.byref(count)) == 0
        assert (first.value, count.value) == (got_first, got_count) and got_count > 0, line
        seen.add((batch, parts, part))
    # nothing kept that should have been dropped, nothing dropped that should have been kept
    for parts in range(1, 6):
        for batch in (5, 1, 0, 7, parts, 2 * parts + 1):
            for part in range(parts):
                L.ieache_shard_slice(batch, parts, part, C.byref(first), C.byref(count))
                assert ((batch, parts, part) in seen) == (count.value > 0), (batch, parts, part)
