"""Several circuits' batches in one call, evaluated together level by level (include/ieache.h section 3c; csrc/joint_plan.h).
The reference of every assertion is the SAME job run alone through eval_batch / eval_netlist, word for word: a job's gates go
through the same kernels' arithmetic whatever they share their launches with, so no tolerance applies.  One job per test is
also compared with the CPU oracle directly, so that the chain to the oracle does not rest on the code under test alone.
Keys: (4, 1024), the 64-lane kernels with four CMux steps per rotation; (5, 64), the any-parameter kernel."""
import ctypes as C
import os
import signal
import subprocess
import threading

import numpy as np
import pytest

from random_netlists import oracle_netlist

pytestmark = pytest.mark.gpu

OPTIONS = ("chunk", "overlap", "overlap_min", "exact_fft", "fft_audit")


def job_inputs(ia, kb, kind, bits, batch, seed):
    """random operands A, B of a CIRC_* job (every other input word zero, as the process contract leaves them)"""
    info = ia.circuit_info(kind, bits)
    rng = np.random.default_rng(seed)
    inb = np.zeros((batch, info.n_inputs), dtype=np.uint8)
    inb[:, :2 * bits] = rng.integers(0, 2, size=(batch, 2 * bits))
    return kb.enc(inb, seed)


def netlist_inputs(kb, cn, batch, seed):
    rng = np.random.default_rng(seed)
    return kb.enc(rng.integers(0, 2, size=(batch, cn.info().n_inputs)).astype(np.uint8), seed)


def alone(ia, ctx, job, stats=None):
    """the job through the single-circuit call"""
    if len(job) == 2:
        return ctx.eval_netlist(job[0], job[1], stats)
    return ctx.eval_batch(job[0], job[1], job[2], stats)


def oracle_add(kb, inp_row, bits):
    s, _ = kb.ck.add(inp_row[:bits], inp_row[bits:2 * bits], inp_row[2 * bits:2 * bits + 1], bits)
    return s


class Saved:
    """the options a test moves, put back whatever happens"""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.saved = {k: self.ctx.get_option(k) for k in OPTIONS}
        return self.ctx

    def __exit__(self, *a):
        for k, v in self.saved.items():
            self.ctx.set_option(k, v)


@pytest.fixture(scope="module")
def mixed(ia, gpu_ctx):
    """Four jobs of different kinds, widths, depths and batches -- three-input gates among them -- and what each gives alone
    with every launch on one stream: computed once, read-only."""
    kb, ctx = gpu_ctx(4, 1024)
    jobs = [(ia.CIRC_ADD, 16, job_inputs(ia, kb, ia.CIRC_ADD, 16, 3, 71)),
            (ia.CIRC_SUB, 32, job_inputs(ia, kb, ia.CIRC_SUB, 32, 2, 72)),
            (ia.CIRC_MUL, 32, job_inputs(ia, kb, ia.CIRC_MUL, 32, 1, 73)),
            (ia.CIRC_ADD_FA, 32, job_inputs(ia, kb, ia.CIRC_ADD_FA, 32, 5, 74))]
    with Saved(ctx):
        ctx.set_option("overlap", 0)
        stats = [ia.Stats() for _ in jobs]
        want = [alone(ia, ctx, j, s) for j, s in zip(jobs, stats)]
    for w in want:
        w.setflags(write=False)
    return jobs, want, stats


def test_different_depths_and_kinds_share_every_level(ia, gpu_ctx, mixed):
    kb, ctx = gpu_ctx(4, 1024)
    jobs, want, single = mixed
    depth = [ia.circuit_info(k, b).sched_levels for k, b, _ in jobs]
    # alone: a piece per level, each job its own (a lone small batch may even run a re-levelled variant with more levels)
    assert all(s.chunks == s.levels >= d for s, d in zip(single, depth))
    with Saved(ctx):
        ctx.set_option("overlap", 0)
        ctx.prepare_jobs([(k, b, len(x)) for k, b, x in jobs])
        st = ia.Stats()
        out = ctx.eval_jobs(jobs, st)
    for i, (o, w) in enumerate(zip(out, want)):
        assert np.array_equal(o, w), i
    assert st.levels == max(depth) == ia.circuit_info(ia.CIRC_MUL, 32).sched_levels
    assert st.bootstraps == sum(s.bootstraps for s in single)
    # structural: ONE piece per joint level -- the launches are shared -- where the separate runs issue the sum of their depths
    assert st.chunks == st.levels and sum(s.chunks for s in single) >= sum(depth) > st.chunks
    # a prologue-free count of the sharing: the rotation launches of the joint call are those of its deepest job, not the sum
    assert st.blind_rotate_launches < sum(s.blind_rotate_launches for s in single)
    assert st.keyswitch_launches == sum(depth)  # one key switch per job and piece
    for e in range(3):  # the chain to the oracle, not through the code under test
        assert np.array_equal(oracle_add(kb, jobs[0][2][e], 16), out[0][e]), e


@pytest.fixture(scope="module")
def with_mux(ia, gpu_ctx):
    """minimum / maximum of 4-bit numbers (MUX levels) x 3 beside ADD 16-bit x 2, and their single runs"""
    from ieache_amd import netlists
    kb, ctx = gpu_ctx(4, 1024)
    cn = netlists.minmax(4)
    assert cn.gates_by_type()[ia.GATE_MUX] > 0
    jobs = [(cn, netlist_inputs(kb, cn, 3, 81)), (ia.CIRC_ADD, 16, job_inputs(ia, kb, ia.CIRC_ADD, 16, 2, 82))]
    want = [alone(ia, ctx, j) for j in jobs]
    for w in want:
        w.setflags(write=False)
    yield cn, jobs, want
    cn.close()


@pytest.mark.parametrize("chunk", [7, 8])
def test_mux_levels_with_pieces_that_end_inside_parts(ia, gpu_ctx, with_mux, chunk):
    kb, ctx = gpu_ctx(4, 1024)
    cn, jobs, want = with_mux
    with Saved(ctx):
        ctx.set_option("overlap", 0)
        ctx.set_chunk(chunk)
        st = ia.Stats()
        out = ctx.eval_jobs(jobs, st)
        assert st.chunks > st.levels  # pieces do end inside the joint levels
    assert np.array_equal(out[0], want[0]) and np.array_equal(out[1], want[1])
    assert st.bootstraps == 3 * cn.info().bootstraps + 2 * ia.circuit_info(ia.CIRC_ADD, 16).bootstraps
    assert np.array_equal(kb.dec(out[0]), np.stack([cn.simulate(b) for b in kb.dec(jobs[0][1])]))
    assert np.array_equal(oracle_netlist(kb, cn, jobs[0][1][1]), out[0][1])
    assert np.array_equal(oracle_add(kb, jobs[1][2][0], 16), out[1][0])


def test_level_halves_on_two_lanes(ia, gpu_ctx, with_mux):
    kb, ctx = gpu_ctx(4, 1024)
    cn, jobs, want = with_mux
    with Saved(ctx):
        ctx.set_option("overlap", 1)
        ctx.set_option("overlap_min", 8)  # joint levels of 8 items and more fork
        lv = ctx.get_option("overlapped_levels")
        out = ctx.eval_jobs(jobs)
        assert ctx.get_option("overlapped_levels") > lv
        ctx.set_chunk(3)  # ... and more than two pieces alternate between the lanes
        again = ctx.eval_jobs(jobs)
    for o in (out, again):
        assert np.array_equal(o[0], want[0]) and np.array_equal(o[1], want[1])
    assert np.array_equal(oracle_add(kb, jobs[1][2][1], 16), out[1][1])


def test_one_job_and_empty_jobs(ia, gpu_ctx, mixed):
    kb, ctx = gpu_ctx(4, 1024)
    jobs, want, single = mixed
    st = ia.Stats()
    out = ctx.eval_jobs([jobs[0]], st)
    assert len(out) == 1 and np.array_equal(out[0], want[0]) and st.bootstraps == single[0].bootstraps and st.levels == single[0].levels
    assert np.array_equal(oracle_add(kb, jobs[0][2][2], 16), out[0][2])
    # a batch of 0 among others is skipped
    empty = (ia.CIRC_MUL, 32, jobs[2][2][:0])
    out = ctx.eval_jobs([jobs[0], empty, jobs[3]], st)
    assert np.array_equal(out[0], want[0]) and out[1].shape[0] == 0 and np.array_equal(out[2], want[3])
    assert st.levels == max(single[0].levels, single[3].levels) and st.bootstraps == single[0].bootstraps + single[3].bootstraps
    # only empty ones, and none at all
    assert ctx.eval_jobs([empty], st)[0].shape[0] == 0 and bytes(st) == bytes(ia.Stats())
    assert ctx.eval_jobs([], st) == [] and bytes(st) == bytes(ia.Stats())
    assert ia.lib().ieache_eval_jobs(ctx.h, None, 0, None) == 0
    assert ia.lib().ieache_prepare_jobs(ctx.h, None, 0) == 0


def test_exact_path_guard_and_audit(ia, gpu_ctx, with_mux):
    kb, ctx = gpu_ctx(4, 1024)
    cn, jobs, want = with_mux

    def same(out):
        return np.array_equal(out[0], want[0]) and np.array_equal(out[1], want[1])

    with Saved(ctx):
        ctx.set_option("exact_fft", 1)
        assert same(ctx.eval_jobs(jobs))
        ctx.set_option("exact_fft", 0)
        reruns = ctx.fft_guard()[1]
        ctx.set_option("fft_guard_inject", 1)  # a tripped guard repeats the WHOLE joint call on the two-limb kernels, once
        out = ctx.eval_jobs(jobs)
        assert same(out) and ctx.fft_guard()[1] == reruns + 1
        assert same(ctx.eval_jobs(jobs)) and ctx.fft_guard()[1] == reruns + 1
        assert np.array_equal(oracle_add(kb, jobs[1][2][0], 16), out[1][0])
        # the audit: one decision per joint piece; with fft_audit = 1 every piece that took a one-limb kernel is sampled
        ctx.set_option("fft_audit", 1)
        before = ctx.fft_audit()
        st = ia.Stats()
        assert same(ctx.eval_jobs(jobs, st))
        after = ctx.fft_audit()
        assert after["gates_compared"] > before["gates_compared"] and after["mismatches"] == before["mismatches"]
        assert before["audits"] < after["audits"] <= before["audits"] + st.chunks  # never more than one per piece
        ctx.set_option("fft_audit_inject", 1)  # a differing row: a mismatch, and a repeat on the two-limb kernels
        assert same(ctx.eval_jobs(jobs))
        assert ctx.fft_audit()["mismatches"] == after["mismatches"] + 1 and ctx.fft_guard()[1] == reruns + 2


def device_rows(rows, stride):
    import torch
    d = torch.zeros(rows.shape[:-1] + (stride,), dtype=torch.int32, device="cuda")
    d[..., : rows.shape[-1]] = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    return d


def test_overlapping_ranges_run_on_the_two_limb_kernels(ia, gpu_ctx, mixed):
    """Device form: job 0's output over job 1's input.  The call cannot be repeated, so it runs on the two-limb kernels from
    the start -- no launch of it is audited -- and gives what the jobs give from a copy of the inputs."""
    import torch
    kb, ctx = gpu_ctx(4, 1024)
    jobs, want, _ = mixed
    S, stride = kb.p.n + 1, ctx.lwe_stride
    (ka, ba, xa), (kc, bc, xc) = jobs[0], jobs[3]
    d_a, d_c = device_rows(xa, stride), device_rows(xc, stride)
    d_out_a = torch.zeros(want[0].shape[:-1] + (stride,), dtype=torch.int32, device="cuda")
    d_out_c = torch.zeros(want[3].shape[:-1] + (stride,), dtype=torch.int32, device="cuda")
    assert want[0].shape[0] * want[0].shape[1] <= xc.shape[0] * xc.shape[1]  # job 0's output fits inside job 3's input
    torch.cuda.synchronize()
    with Saved(ctx):
        ctx.set_option("fft_audit", 1)
        a0 = ctx.fft_audit()["audits"]
        ctx.eval_jobs_device([(ka, ba, len(xa), d_a.data_ptr(), d_out_a.data_ptr()), (kc, bc, len(xc), d_c.data_ptr(), d_out_c.data_ptr())])
        a1 = ctx.fft_audit()["audits"]
        assert a1 > a0  # disjoint ranges: one-limb launches, audited
        assert np.array_equal(d_out_a.cpu().numpy()[..., :S], want[0]) and np.array_equal(d_out_c.cpu().numpy()[..., :S], want[3])
        reruns = ctx.fft_guard()[1]
        ctx.eval_jobs_device([(ka, ba, len(xa), d_a.data_ptr(), d_c.data_ptr()), (kc, bc, len(xc), d_c.data_ptr(), d_out_c.data_ptr())])
        assert ctx.fft_audit()["audits"] == a1 and ctx.fft_guard()[1] == reruns
    n_rows = want[0].shape[0] * want[0].shape[1]
    got_a = d_c.cpu().numpy().reshape(-1, stride)[:n_rows, :S].reshape(want[0].shape)
    assert np.array_equal(got_a, want[0]) and np.array_equal(d_out_c.cpu().numpy()[..., :S], want[3])
    assert np.array_equal(oracle_add(kb, xa[1], 16), got_a[1])
    with pytest.raises(ia.IeacheError, match="not a device pointer"):
        ctx.eval_jobs_device([(ka, ba, len(xa), xa.ctypes.data, d_out_a.data_ptr())])


def test_a_bad_job_fails_the_whole_call_before_anything_runs(ia, gpu_ctx, mixed):
    kb, ctx = gpu_ctx(4, 1024)
    jobs, want, _ = mixed
    L = ia.lib()
    arr = (ia.Job * 3)()
    ins = [np.ascontiguousarray(jobs[i][2]) for i in (0, 1, 3)]
    outs = [np.full_like(want[i], 7) for i in (0, 1, 3)]
    for i, (k, b) in enumerate(((ia.CIRC_ADD, 16), (ia.CIRC_SUB, 32), (999, 32))):
        arr[i].kind, arr[i].bits, arr[i].batch = k, b, len(ins[i])
        arr[i].in_lwe, arr[i].out_lwe = ins[i].ctypes.data, outs[i].ctypes.data
    st = ia.Stats()
    assert L.ieache_eval_jobs(ctx.h, arr, 3, C.byref(st)) == -22
    assert L.ieache_last_error().startswith(b"job 2: unsupported circuit kind/bits")
    assert all((o == 7).all() for o in outs)  # every output untouched
    assert L.ieache_prepare_jobs(ctx.h, arr, 3) == -22 and L.ieache_last_error().startswith(b"job 2:")
    arr[1].in_lwe = None
    assert L.ieache_eval_jobs(ctx.h, arr, 3, None) == -22 and L.ieache_last_error() == b"job 1: null argument"
    # the context is as usable as before
    out = ctx.eval_jobs([jobs[0], jobs[1]])
    assert np.array_equal(out[0], want[0]) and np.array_equal(out[1], want[1])
    assert np.array_equal(oracle_add(kb, jobs[0][2][0], 16), out[0][0])


def test_any_parameter_path_two_jobs_of_different_depth(ia, gpu_ctx):
    from ieache_amd import netlists
    kb, ctx = gpu_ctx(5, 64)
    cn = netlists.minmax(3)
    jobs = [(ia.CIRC_ADD, 16, job_inputs(ia, kb, ia.CIRC_ADD, 16, 2, 91)), (cn, netlist_inputs(kb, cn, 3, 92))]
    single = [ia.Stats(), ia.Stats()]
    want = [alone(ia, ctx, j, s) for j, s in zip(jobs, single)]
    assert single[0].levels != single[1].levels
    st = ia.Stats()
    saved = ctx.get_option("chunk")
    try:
        out = ctx.eval_jobs(jobs, st)
        ctx.set_chunk(5)
        cut = ctx.eval_jobs(jobs)
    finally:
        ctx.set_chunk(saved)
    for o in (out, cut):
        assert np.array_equal(o[0], want[0]) and np.array_equal(o[1], want[1])
    assert st.levels == max(s.levels for s in single) and st.bootstraps == sum(s.bootstraps for s in single)
    assert np.array_equal(oracle_add(kb, jobs[0][2][1], 16), out[0][1])
    assert np.array_equal(oracle_netlist(kb, cn, jobs[1][1][2]), out[1][2])
    cn.close()


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)])
def test_group_cuts_every_job_over_its_members(ia, gpu_ctx, devices):
    kb, ctx = gpu_ctx(4, 1024)
    jobs = [(ia.CIRC_ADD, 16, job_inputs(ia, kb, ia.CIRC_ADD, 16, 5, 95)),
            (ia.CIRC_ADD_FA, 32, job_inputs(ia, kb, ia.CIRC_ADD_FA, 32, 1, 96)),
            (ia.CIRC_SUB, 32, job_inputs(ia, kb, ia.CIRC_SUB, 32, 0, 97))]
    single = ia.Stats()
    want = ctx.eval_jobs(jobs, single)
    assert np.array_equal(want[0], alone(ia, ctx, jobs[0])) and np.array_equal(want[1], alone(ia, ctx, jobs[1]))
    with ia.Group.from_arrays(kb.p, kb.bk, kb.ksk, devices) as g:
        stats = []
        out = g.eval_jobs(jobs, stats=stats)
        assert len(out) == 3 and all(np.array_equal(o, w) for o, w in zip(out, want)) and out[2].shape[0] == 0
        assert len(stats) == len(devices) and sum(s.bootstraps for s in stats) == single.bootstraps
        # 5 and 1 expressions: member 0 takes 3 + 1 (2 + 1 of three members), the last member the rest of the first job alone
        per_add, per_fa = ia.circuit_info(ia.CIRC_ADD, 16).bootstraps, ia.circuit_info(ia.CIRC_ADD_FA, 32).bootstraps
        shares = {2: [3 * per_add + per_fa, 2 * per_add], 3: [2 * per_add + per_fa, 2 * per_add, per_add]}[len(devices)]
        assert [s.bootstraps for s in stats] == shares
        assert g.eval_jobs([], stats=stats) == [] and all(bytes(s) == bytes(ia.Stats()) for s in stats)
        assert np.array_equal(g.eval_jobs([jobs[1]])[0], want[1])
    assert np.array_equal(oracle_add(kb, jobs[0][2][4], 16), out[0][4])  # the last member's own expression


@pytest.fixture(scope="module")
def six_clients(ia, O, tmp_path_factory):
    """Six requests -- A+B, A-B and AxB at 32 bits, two of each -- under one toy key, and every answer's value samples as the
    CPU oracle gives them."""
    from ieache_amd import tools
    root = tmp_path_factory.mktemp("jobs_daemon")
    p = ia.default_params().copy(n=6, N=64)
    tools.keygen_files(root, p)
    _, bk, ksk = tools.read_cloud_key(root / "cloud.key")
    ck = O.CloudKey(p.n, p.N, p.k, p.l, p.Bgbit, p.ks_t, p.ks_basebit, bk, ksk)
    jobs = []
    for i in range(6):
        d = root / ("client%d" % i)
        d.mkdir()
        for f in ("cloud.key", "nbit.key", "secret.key"):
            os.link(root / f, d / f)
        operator, a, b = (1, 2, 4)[i % 3], 70000 + 13 * i, 999 + 7 * i
        tools.alice(d, 0, 32, a, seed=300 + i)
        tools.alice(d, 0, 32, b, seed=400 + i, append=True)
        data = tools.read_samples(d / "cloud.data", p.n).reshape(22, 32, p.n + 1)
        rc, ref = ck.cloud_values(operator, 0, 32, data[2:10], data[13:21], data[10])
        assert rc == 0
        jobs.append((d, operator, a, b, ref))
    # every request served alone, one round each (no batching window: nothing waits)
    import shutil
    import tempfile
    from ieache_amd import daemon
    sdir = tempfile.mkdtemp(prefix="ia-")
    proc = daemon.spawn(os.path.join(sdir, "s.sock"), root / "cloud.key")
    try:
        served_alone = []
        for (d, *_), (rc, log, ans) in zip(jobs, _serve_round(daemon, os.path.join(sdir, "s.sock"), jobs, together=False)):
            assert rc == 0, log
            served_alone.append(_value_samples(tools, p, d / "alone.data", ans))
        st = daemon.stats(os.path.join(sdir, "s.sock"))
        assert st["evaluations"] == 6 and st["joint_rounds"] == 0 and st["joint_requests"] == 0  # rounds of one circuit: as ever
        assert daemon.shutdown(os.path.join(sdir, "s.sock")) == 0 and proc.wait(timeout=60) == 0
    finally:
        if proc.poll() is None:
            proc.kill()
        shutil.rmtree(sdir, ignore_errors=True)
    return root, p, jobs, served_alone


def _value_samples(tools, p, path, answer):
    """The 9 x 32 value samples of an answer.data.  (The 64 metadata samples before them are FRESH encryptions under the nbit
    key, as in the reference: no two servings of a request agree on them; tools.verif decrypts them below.)"""
    path.write_bytes(answer)
    return tools.read_samples(path, p.n).reshape(11, 32, p.n + 1)[2:].copy()


def _serve_round(daemon, sock, jobs, together):
    """the six requests at once (together) or one after another -> [(rc, log, answer bytes)]"""
    results = [None] * len(jobs)
    barrier = threading.Barrier(len(jobs))

    def client(i):
        if together:
            barrier.wait()
        results[i] = daemon.run_data(sock, jobs[i][1], (jobs[i][0] / "cloud.data").read_bytes())

    if together:
        threads = [threading.Thread(target=client, args=(i,)) for i in range(len(jobs))]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=300)
    else:
        for i in range(len(jobs)):
            client(i)
    return results


@pytest.mark.parametrize("joint", [1, 0])
def test_daemon_joins_a_round_of_several_circuits(ia, sock_dir, six_clients, joint):
    from ieache_amd import daemon, tools
    root, p, jobs, served_alone = six_clients
    sock = sock_dir / "cloudd.sock"
    proc = daemon.spawn(sock, root / "cloud.key", batch_window_ms=400, max_batch=64, joint=joint)
    try:
        results = _serve_round(daemon, sock, jobs, together=True)
        st = daemon.stats(sock)
        jointly = 0
        for i, (d, operator, a, b, ref) in enumerate(jobs):
            rc, log, ans = results[i]
            assert rc == 0 and "Computation Time" in log, (i, log)
            samples = _value_samples(tools, p, d / "answer.data", ans)
            assert np.array_equal(samples, served_alone[i]), i  # word for word the answer of the same request served alone
            assert np.array_equal(samples, ref), i  # ... and the oracle's
            code, bit_size, words = tools.verif(d)
            assert tools.verif_interpret(operator, code, bit_size, words) == {1: a + b, 2: a - b, 4: a * b}[operator], i
            jointly += "evaluated jointly" in log
        assert st["batched_requests"] == 6 and st["evaluations"] < 6, st
        if joint:
            assert st["joint_rounds"] > 0 and st["joint_requests"] >= 2 and jointly == st["joint_requests"], st
            assert any("evaluated jointly, level by level, with circuit " in results[i][1] for i in range(6))
        else:
            assert st["joint_rounds"] == 0 and st["joint_requests"] == 0 and jointly == 0, st
        assert daemon.shutdown(sock) == 0
        assert proc.wait(timeout=60) == 0
    finally:
        if proc.poll() is None:
            proc.send_signal(signal.SIGTERM)
            try:
                proc.wait(timeout=30)
            except subprocess.TimeoutExpired:
                proc.kill()
