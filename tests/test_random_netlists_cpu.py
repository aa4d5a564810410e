"""The random netlist corpus on the host: the compiled netlists simulate to the plain wire walk under both schedules, the
corpus holds what its families promise, and the ciphertext oracle decrypts to the wire walk on exactly the inputs and
expressions tests/test_random_netlists_gpu.py will compare -- so a red GPU test there is the card's, not the reference's."""
import numpy as np
import pytest

import random_netlists as rn

PARAMS = [(5, 64), (16, 1024)]
SIZES = {(5, 64): 24, (16, 1024): 6}


def test_corpus_sizes_and_families():
    for params in PARAMS:
        cases = rn.corpus(params)
        assert len(cases) == SIZES[params] == len(set(cases)) and cases == rn.corpus(params)
    assert set(f for _, f in rn.corpus((5, 64))) == set(rn.FAMILIES)
    assert {"mixed", "mux_only", "dead", "long_lived", "window"} <= set(f for _, f in rn.corpus((16, 1024)))
    for seed, family in rn.corpus((5, 64)) + rn.corpus((16, 1024)):
        nl, gates, outs = rn.generate(seed, family)
        again = rn.generate(seed, family)
        assert (gates, outs) == again[1:] and nl.n_inputs == again[0].n_inputs
        assert 1 <= nl.n_inputs <= rn.MAX_INPUTS and len(gates) <= rn.MAX_GATES and 1 <= len(outs) <= rn.MAX_OUTPUTS
        assert len(nl) == len(gates)


@pytest.mark.parametrize("params", PARAMS)
def test_simulation_equals_the_wire_walk_under_both_schedules(ia, params):
    ran = 0
    for seed, family in rn.corpus(params):
        nl, gates, outs = rn.generate(seed, family)
        bits = rn.all_input_bits(nl.n_inputs)
        want = np.stack([rn.walk_bits(nl.n_inputs, gates, outs, v) for v in bits])
        by_type = [sum(1 for g in gates if g[0] == t) for t in range(11)]
        for balanced in (False, True):
            with nl.compile(outs, balanced=balanced) as cn:
                assert cn.gates == gates and cn.outputs == outs
                got = np.stack([cn.simulate(v) for v in bits])
                assert np.array_equal(got, want), (seed, family, balanced)
                info = cn.info()
                assert info.bootstraps == len(gates) + by_type[rn.MUX], (seed, family)
                assert cn.gates_by_type() == by_type, (seed, family)
                p = rn.properties(nl.n_inputs, gates, outs)
                assert info.depth == p["depth"] and info.n_inputs == nl.n_inputs and info.n_outputs == len(outs)
        ran += 1
    assert ran == len(rn.corpus(params)) == SIZES[params]


def _props(params):
    out = []
    for seed, family in rn.corpus(params):
        nl, gates, outs = rn.generate(seed, family)
        out.append((family, rn.properties(nl.n_inputs, gates, outs)))
    return out


def test_the_corpus_contains_what_its_families_promise():
    small, large = _props((5, 64)), _props((16, 1024))
    for props in (small, large):
        for family, p in props:
            # per family: every case of it has the family's trait
            if family == "empty":
                assert p["gates"] == 0 and p["depth"] == 0
            else:
                assert p["gates"] >= 20 and p["depth"] >= 2, family
            if family == "mux_only":
                assert p["types"] == {rn.MUX} and p["mux_only_level"]
            if family == "dead":
                assert p["dead_gate"] and p["unread_input"] and p["unread_input_is_output"] and p["level1_output_nobody_reads"]
                assert p["depth"] >= 5  # the level-1 output outlives several levels of recycling
            if family == "long_lived":
                assert p["longest_life"] >= 5
            if family == "window":
                assert p["depth"] >= 10
            if family == "mixed":
                assert p["types"] == set(range(11)) and p["negated_operand"]
            if family == "same_wire":
                assert p["same_wire_gate"]
            if family == "constants":
                assert p["two_constant_gate"]
    # over the small corpus as a whole (the issue's list)
    for key in ("mux_only_level", "dead_gate", "unread_input", "same_wire_gate", "two_constant_gate"):
        assert any(p[key] for _, p in small), key
    assert any(p["longest_life"] >= 5 for _, p in small) and any(p["gates"] == 0 for _, p in small)
    # the large one keeps the traits the executor's cuts are aimed at
    assert any(p["mux_only_level"] for _, p in large) and any(p["dead_gate"] for _, p in large)
    assert any(p["longest_life"] >= 5 for _, p in large)


@pytest.mark.parametrize("params", PARAMS)
def test_the_oracle_decrypts_to_the_wire_walk_on_the_gpu_tests_inputs(ia, make_keys, params):
    kb = make_keys(*params)
    ran = 0
    for seed, family in rn.corpus(params):
        nl, gates, outs = rn.generate(seed, family)
        with nl.compile(outs) as cn:
            bits, inp = rn.case_inputs(kb, seed, nl.n_inputs)
            assert inp.shape == (rn.BATCH, nl.n_inputs, params[0] + 1) and np.array_equal(kb.dec(inp), bits)
            for e in rn.compared_with_oracle(params):
                want = rn.walk_bits(nl.n_inputs, gates, outs, bits[e])
                assert np.array_equal(kb.dec(rn.oracle_netlist(kb, cn, inp[e])), want), (seed, family, e)
        ran += 1
    assert ran == len(rn.corpus(params)) == SIZES[params]
