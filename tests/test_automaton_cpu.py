"""Deterministic automata over words of encrypted bits without a GPU (include/ieache.h section 3k): the C reference
(ieache_automaton_reference) against the numpy restatement (automaton_reference.py) word for word, the worked examples of
ieache_amd.automata against plain Python on every input of a small width, one of them by meaning through the reference with
encrypted letters, the refusals of ieache_automaton_check, and the plan (csrc/automaton_plan.h) under AddressSanitizer + UBSan."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import automaton_reference as AR
import cmux_reference as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def params(ia, N, l, Bgbit, n=4):
    return ia.default_params().copy(n=n, N=N, l=l, Bgbit=Bgbit)


# both libtfhe gadgets and (6, 5), on toy rings and once each on the ring the kernels cover
@pytest.mark.parametrize("N,l,Bgbit,states,steps", [(16, 3, 7, 5, 4), (16, 2, 10, 3, 5), (64, 6, 5, 4, 3), (16, 3, 7, 1, 3), (64, 2, 10, 9, 2),
                                                    (1024, 3, 7, 3, 2), (1024, 2, 10, 2, 2), (1024, 6, 5, 2, 1)])
def test_reference_is_the_definition_word_for_word(ia, N, l, Bgbit, states, steps):
    """Full-range random words for samples and finals; random step-dependent tables with self-loops and next0 == next1 entries;
    selectors implied and explicit; one and two sets of finals; n_out 1 and states; steps == 0 copies the finals."""
    from ieache_amd import tools
    p = params(ia, N, l, Bgbit)
    rng = np.random.default_rng(9900 + N + 100 * l + Bgbit + states)
    n, count = 3, 2
    C = CR.full_range(rng, (n, 2 * l, 2, N))
    F = CR.full_range(rng, (2, states, 2, N))
    next0, next1 = AR.random_tables(rng, steps, states)
    assert (next0 == next1).any() and (next0 != next1).any() or states == 1
    sel = rng.integers(0, n, size=(count, steps)).astype(np.int32)
    for n_out, so, fo in ((1, None, None), (states, sel, [1, 0])):
        got = tools.automaton_reference(p, C, next0, next1, F, n_out=n_out, sel_of=so, final_of=fo, count=count)
        want = AR.run(C, next0, next1, F, l, Bgbit, n_out=n_out, sel_of=so, final_of=fo, count=count)
        assert got.shape == (count, n_out, 2, N) and np.array_equal(got, want), (n_out, so is None)
    empty = np.zeros((0, states), dtype=np.int32)
    assert np.array_equal(tools.automaton_reference(p, C, empty, empty, F, n_out=states, final_of=[1, 0, 1]), F[[1, 0, 1]])


def every_word(steps):
    return itertools.product((0, 1), repeat=steps)


def test_worked_examples_on_every_input_of_a_small_width(ia):
    from ieache_amd import automata as A
    bits = 4
    lt, eq = A.less_than(bits), A.equals(bits)
    assert lt.next0.shape == (2 * bits, 5) and lt.next0.shape[1] <= 6 and not np.array_equal(lt.next0[0], lt.next0[1])
    for a in range(1 << bits):
        for b in range(1 << bits):
            word = lt.word(a, b)
            assert list(word[0::2]) == [(a >> i) & 1 for i in reversed(range(bits))] and list(word[1::2]) == [(b >> i) & 1 for i in reversed(range(bits))]
            assert A.message(lt, A.run_clear(lt, word)) == (1 / 8 if a < b else -1 / 8), (a, b)
            assert A.message(eq, A.run_clear(eq, eq.word(a, b))) == (1 / 8 if a == b else -1 / 8), (a, b)
    for pattern in ([1], [0, 1], [1, 1, 0], [1, 0, 1, 0], [0, 0, 0]):
        c = A.contains(pattern, 7)
        assert c.next0.shape == (7, len(pattern) + 1)
        for word in every_word(7):
            found = any(list(word[i:i + len(pattern)]) == pattern for i in range(7 - len(pattern) + 1))
            assert A.message(c, A.run_clear(c, c.word(word))) == (1 / 8 if found else -1 / 8), (pattern, word)
    for k in (1, 2, 3, 5, 7):
        r, h = A.remainder(k, 6), A.remainder(k, 6, one_hot=True)
        for value in range(64):
            q = A.run_clear(r, r.word(value))
            assert q == value % k and A.message(r, q) == (value % k) / (2 * k) and h.finals[A.run_clear(h, h.word(value))] == (value % k, 1, 8)
        rows = A.final_rows(h, 16)
        assert rows.shape == (k, 2, 16) and all(rows[q, 1, q] == 1 << 29 and np.count_nonzero(rows[q]) == 1 for q in range(k))
    for k in (1, 2, 4):
        t = A.at_least(k, 6)
        for word in every_word(6):
            assert A.message(t, A.run_clear(t, t.word(word))) == (1 / 8 if sum(word) >= k else -1 / 8), (k, word)
    rows = A.final_rows(lt, 16)
    assert rows[3, 1, 0] == 1 << 29 and rows[0, 1, 0] == -(1 << 29) and not rows[:, 0].any() and np.count_nonzero(rows) == 5
    third = A.final_rows(A.remainder(3, 2), 16)
    assert [int(v) for v in third[:, 1, 0]] == [0, 715827883, 1431655765]  # 0, 1/6, 2/6 of 2^32, rounded to nearest
    # every builder's tables pass the library's validation
    from ieache_amd import tools
    for w in (lt, eq, A.contains([1, 0, 1], 9), A.remainder(5, 8), A.at_least(3, 8)):
        tools.automaton_check(w.next0, w.next1, w.n_out)


def torus_distance(a, b):
    d = (np.asarray(a, dtype=np.int64) - np.asarray(b, dtype=np.int64)) & 0xFFFFFFFF
    return np.minimum(d, (1 << 32) - d).astype(np.float64) / 2.0 ** 32


def test_less_than_by_meaning_on_a_small_ring(ia):
    """N = 64, (3, 7), letters encrypted at a small noise: for pairs that differ high, low, in one bit and not at all, the phase
    of coefficient 0 of the output is within 1/8 -- the decoding distance of a +-1/8 message -- of the verdict's message."""
    from ieache_amd import automata as A
    from ieache_amd import tools
    p = params(ia, 64, 3, 7)
    k = tools.keygen_raw(p, (8, 9), with_cloud=False)
    bits = 3
    lt = A.less_than(bits)
    pairs = [(0, 0), (5, 5), (3, 4), (4, 3), (6, 7), (7, 6), (0, 7), (2, 2)]
    letters = np.concatenate([lt.word(a, b) for a, b in pairs])
    C = tools.tgsw_encrypt(p, k["tlwe_key"], letters.astype(np.int32), 75, alpha=2.0 ** -30)
    out = tools.automaton_reference(p, C, lt.next0, lt.next1, A.final_rows(lt, 64), count=len(pairs))
    phase = tools.tlwe_phase(p, k["tlwe_key"], out[:, 0])
    for i, (a, b) in enumerate(pairs):
        want = (1 << 29) if a < b else -(1 << 29)
        assert torus_distance(phase[i, 0], want) < 1 / 8, (a, b)
        assert torus_distance(phase[i, 1:], 0).max() < 1 / 8


def refused(ia, match, f, *a, **kw):
    with pytest.raises(ia.IeacheError, match=match) as e:
        f(*a, **kw)
    assert e.value.code == -22


def test_check_refuses_each_bad_scalar_and_names_a_bad_entry(ia):
    from ieache_amd import tools
    from ieache_amd.evaluator import _i32, check
    L = ia.lib()
    ok = np.zeros((3, 4), dtype=np.int32)
    tools.automaton_check(ok, ok + 3, 4)
    tools.automaton_check(np.zeros((0, 64), dtype=np.int32), np.zeros((0, 64), dtype=np.int32), 64)
    wide = np.zeros((1, 65), dtype=np.int32)
    refused(ia, r"states must lie in 1 \.\. 64", tools.automaton_check, wide, wide)
    refused(ia, "states", lambda: check(L.ieache_automaton_check(0, 3, 1, _i32(ok), _i32(ok))))
    refused(ia, r"steps must lie in 0 \.\. 4096", lambda: check(L.ieache_automaton_check(4, 4097, 1, _i32(ok), _i32(ok))))
    refused(ia, "steps", lambda: check(L.ieache_automaton_check(4, -1, 1, _i32(ok), _i32(ok))))
    refused(ia, r"n_out must lie in 1 \.\. states", tools.automaton_check, ok, ok, 0)
    refused(ia, "n_out", tools.automaton_check, ok, ok, 5)
    refused(ia, "null transition table", lambda: check(L.ieache_automaton_check(4, 3, 1, None, _i32(ok))))
    bad = ok.copy()
    bad[2, 1] = 4
    refused(ia, r"next1\[2\]\[1\] = 4 is outside \[0, 4\)", tools.automaton_check, ok, bad)
    refused(ia, r"next0\[2\]\[1\] = 4", tools.automaton_check, bad, bad)
    neg = ok.copy()
    neg[0, 3] = -1
    refused(ia, r"next0\[0\]\[3\] = -1", tools.automaton_check, neg, bad)
    # the reference refuses the same, then its own indices
    p = params(ia, 16, 3, 7)
    S, F = np.zeros((2, 6, 2, 16), dtype=np.int32), np.zeros((2, 4, 2, 16), dtype=np.int32)
    assert tools.automaton_reference(p, S, ok, ok + 3, F, n_out=2, sel_of=[[0, 1, 1]], final_of=[1]).shape == (1, 2, 2, 16)
    refused(ia, r"next1\[2\]\[1\] = 4", tools.automaton_reference, p, S, ok, bad, F)
    refused(ia, r"sel_of\[1\] = 2", tools.automaton_reference, p, S, ok, ok, F, sel_of=[[0, 2, 1]])
    refused(ia, r"final_of\[0\] = 2", tools.automaton_reference, p, S, ok, ok, F, final_of=[2])
    refused(ia, "unsupported", tools.automaton_reference, p.copy(N=8), S, ok, ok, F)
    assert ia.AUTOMATON_MAX_STATES == 64 and ia.AUTOMATON_MAX_STEPS == 4096


def test_automaton_plan_under_asan_ubsan(tmp_path):
    """tests/native/automaton_plan_test.cpp: a stand-alone program over csrc/automaton_plan.h -- every item in exactly one piece,
    the cap respected or the item alone, the step chunks covering all steps once in order, the live masks against a brute-force
    walk, the CMux count."""
    exe = tmp_path / "automaton_plan_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "native", "automaton_plan_test.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "AUTOMATON_PLAN_OK" in r.stdout, r.stdout[-4000:]
