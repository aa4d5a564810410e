"""The corpus of tests/levelled_programs.py: the conditions the GPU tests rely on, asserted, and the MEANING of the reference
interpreter -- the plumbing the GPU side shares -- against a plain integer model on real encryptions.  No GPU.

Corpus conditions (test_corpus_conditions): every call kind stands after a call on more items, after one on fewer, directly
after an option change and directly after a gate step; every memory-updating call occurs in place and out of place, in place at
least half of the time; word_read follows a lut_write_coef on more items and lut_write_coef follows word_read (the coef_idx
layout); every kind that fills the lane's extracted rows follows every other such kind; every option value of the table is set.

Meaning (test_reference_interpreter_by_meaning): on MEANING -- three programs on the key's gadget (3, 7), one each on (2, 10)
and on the run-time set (6, 5) -- the state is client-encrypted (messages on the grid of eighths, selector bits as TGSW samples,
real packing and projection keys), the reference interpreter runs beside levelled_programs.Model, and after EVERY step the rows
the step wrote decrypt to the model's words; so does the whole final state.  A gate whose argument sits on a decision boundary
(phase 0 or 1/2 exactly, which sums of eighths reach) has no right bit: there the model takes the reference's, and the test
asserts that most gate rows are decided by the model.

The bound: a decoding to eighths goes wrong at 1/16; the reference's own largest phase error must stay within half of that,
1/32 of the torus.  Measured on the CPU with MAX_UPDATES = 6 memory-updating steps per program at most (largest over the steps of
each program):

    mixed 0    (3, 7)      5.9e-3        memory 2   (3, 7)      8.9e-3        way_back 3 (3, 7)      5.4e-3
    mixed 1    (2, 10)     6.5e-3        grow 5     (6, 5) rt   6.9e-3

so the cap stands: the largest, 8.9e-3, is under a third of the bound 3.125e-2.  Were a drawn program to exceed it, MAX_UPDATES
goes down; the assertion stays.
"""
import numpy as np
import pytest

import levelled_programs as LP

MEANING = [(0, "mixed", 0), (2, "memory", 0), (3, "way_back", 0), (1, "mixed", 1), (5, "grow", 2)]
BOUND = 1.0 / 32


def programs():
    return {(seed, family): LP.program(seed, family) for seed, family in LP.corpus()}


def test_generation_is_deterministic():
    for (seed, family), steps in programs().items():
        assert steps == LP.program(seed, family) and len(steps) >= 10
        assert steps != LP.program(seed + 100, family)
    assert len(LP.corpus()) == 6 and {f for _, f in LP.corpus()} == set(LP.FAMILIES)


def test_steps_name_rows_inside_the_state_and_outputs_apart_from_inputs():
    """every operand lies inside its entry; the output shares rows with an input only where it is that input exactly (the in-place
    forms); the scalars lie in the ranges levelled_programs states"""
    st = LP.initial_state(LP.set_params(__import__("ieache_amd").default_params().copy(n=LP.KEY_N), None))
    for steps in programs().values():
        for s in steps:
            if s["op"] == "option":
                assert s["name"] == "force_generic" and s["value"] in (0, 1) or s["value"] in LP.OPTION_VALUES[s["name"]]
                continue
            assert s["count"] in LP.COUNTS and 0 <= s.get("depth", 0) <= 3 and 0 <= s.get("steps", 0) <= 3 and 1 <= s.get("width", 1) <= 5
            assert s.get("unit", 1) << s.get("steps", 0) <= LP.N and s.get("m", 1) <= 5 and s.get("states", 1) <= 4 and s.get("letters", 0) <= 5
            entry, first, rows = s["out"]
            assert 0 <= first and first + rows <= st[entry].shape[0] and rows > 0
            for ref in s["args"].values():
                if ref is None:
                    continue
                assert 0 <= ref[1] and ref[1] + ref[2] <= st[ref[0]].shape[0], s
                if ref[0] == entry and ref[1] < first + rows and first < ref[1] + ref[2]:
                    assert (ref[1], ref[2]) == (first, rows) and (s.get("inplace") or s["kind"] == "tlwe_rotate"), s


def test_force_generic_only_around_the_key_switching_calls():
    for steps in programs().values():
        for i, s in enumerate(steps):
            if s["op"] == "option" and s["name"] == "force_generic" and s["value"] == 1:
                assert steps[i + 1]["kind"] in LP.KS_CALLS and steps[i + 2] == {"op": "option", "name": "force_generic", "value": 0}


def test_corpus_conditions():
    after_larger, after_smaller, after_option, after_gate = set(), set(), set(), set()
    in_place, out_of_place, ext_pairs, options_set = set(), set(), set(), set()
    read_after_bigger_write = write_after_read = False
    updates = updates_in_place = 0
    for steps in programs().values():
        before = last = last_filler = None  # the step before; the call or gate step before; the last step that fills the extracted rows
        write_counts, read_seen = [], False
        for s in steps:
            if s["op"] == "option":
                options_set.add((s["name"], s["value"]))
                before = s
                continue
            kind = s["kind"]
            if last is not None and last["count"] > s["count"]:
                after_larger.add(kind)
            if last is not None and last["count"] < s["count"]:
                after_smaller.add(kind)
            if before is not None and before["op"] == "option":
                after_option.add(kind)
            if before is not None and before["op"] == "gate":
                after_gate.add(kind)
            if kind in LP.UPDATES:
                (in_place if s["inplace"] else out_of_place).add(kind)
                updates += 1
                updates_in_place += bool(s["inplace"])
                assert (s["out"][0] == s["args"]["mems" if kind == "lut_add" else "mem"][0]) == s["inplace"]
            if kind == "word_read":
                read_after_bigger_write |= any(c > s["count"] for c in write_counts)
                read_seen = True
            if kind == "lut_write_coef":
                write_after_read |= read_seen
                write_counts.append(s["count"])
            if kind in LP.EXT_FILLERS:
                if last_filler is not None:
                    ext_pairs.add((last_filler, kind))
                last_filler = kind
            before = last = s
        assert sum(s.get("kind") in LP.UPDATES for s in steps) <= LP.MAX_UPDATES
    kinds = set(LP.KINDS)
    assert after_larger >= kinds, kinds - after_larger
    assert after_smaller >= kinds, kinds - after_smaller
    assert after_option >= kinds, kinds - after_option
    assert after_gate >= kinds, kinds - after_gate
    assert in_place == set(LP.UPDATES) == out_of_place and 2 * updates_in_place >= updates
    assert read_after_bigger_write and write_after_read
    want_pairs = {(a, b) for a in LP.EXT_FILLERS for b in LP.EXT_FILLERS if a != b}
    assert ext_pairs >= want_pairs, want_pairs - ext_pairs
    want_options = {(name, v) for name, values in LP.OPTION_VALUES.items() for v in values} | {("force_generic", 0), ("force_generic", 1)}
    assert options_set >= want_options, want_options - options_set


def test_way_back_reads_outgrow_the_extracted_rows_reserved_before_them():
    """UnpackRows::reserve is the one place that sizes the lane's extracted rows for unpack and word_read.  In four programs a run
    of such a call walks more stored rows than any earlier step of the program reserved (gate steps reserve their items, MUX twice
    that, lut_read its items; a run of at least "ks_mfma_min" rows stores none): on a context of its own
    (test_every_program_on_a_fresh_context) that call is the first to need them."""
    outgrown = set()
    for key, steps in programs().items():
        opt, high = {"chunk": 65536, "ks_mfma_min": 64, "force_generic": 0}, 0
        for s in steps:
            if s["op"] == "option":
                opt[s["name"]] = s["value"]
                continue
            kind, c = s["kind"], s["count"]
            need = {"gates": c, "mux": 2 * c, "lut_read": c}.get(kind, 0)
            if kind in ("unpack", "word_read"):
                run = min(c * s["width"], opt["chunk"])
                need = run if opt["force_generic"] or run < opt["ks_mfma_min"] else 0
                if need > high:
                    outgrown.add(key)
            high = max(high, need)
    assert len(outgrown) >= 4, outgrown


def test_strip_options_keeps_the_calls():
    for steps in programs().values():
        bare = LP.strip_options(steps)
        assert all(s["op"] != "option" for s in bare) and bare == [s for s in steps if s["op"] in ("call", "gate")]


def oracle_gate(kb):
    def gate(kind, a, b, c):
        return np.stack([kb.ck.gate("nand", a[i], b[i]) if kind == "gates" else kb.ck.mux(a[i], b[i], c[i]) for i in range(len(a))])
    return gate


def oracle_keyswitch(kb):
    return lambda u: np.stack([kb.ck.keyswitch(row) for row in u])


def run_by_meaning(kb, gadget, seed, family, run=None):
    """The reference interpreter beside the model on an encrypted state; run(steps, state, writes): what else to put through the
    steps (the GPU test's card).  -> (largest phase error over every step's rows and the final state, model, writes, final)"""
    steps = LP.program(seed, family)
    state, model = LP.encrypted_state(kb, gadget, seed)
    writes, final = LP.run_reference(steps, state, LP.set_params(kb.p, gadget), kb.ksk, oracle_gate(kb), oracle_keyswitch(kb))
    worst = 0.0
    for i, s in enumerate(steps):
        if s["op"] == "option":
            continue
        model.step(s, LP.to_grid(kb, writes[i]) if s["op"] == "gate" else None)
        err = LP.decoded_error(kb, s["out"][0], writes[i], model.get(s["out"]))
        assert err <= BOUND, "%s decrypts %.4f of the torus from the model (bound 1/32)" % (LP.describe(i, s), err)
        worst = max(worst, err)
    for entry in ("mem", "tab", "tlwe", "lwe", "ext"):
        err = LP.decoded_error(kb, entry, final[entry], model.m[entry])
        assert err <= BOUND, "final %s decrypts %.4f of the torus from the model (bound 1/32)" % (entry, err)
        worst = max(worst, err)
    return worst, model, writes, final


@pytest.mark.parametrize("seed,family,which", MEANING, ids=["%s%d_%s" % (f, s, LP.IDS[w]) for s, f, w in MEANING])
def test_reference_interpreter_by_meaning(make_keys, seed, family, which):
    kw, gadget = LP.SETS[which]
    kb = make_keys(LP.KEY_N, LP.N, **kw)
    worst, model, _writes, _final = run_by_meaning(kb, gadget, seed, family)
    print("%s %d on %s: largest phase error of the reference %.3e of the torus (bound 1/32 = %.3e); %d of %d gate rows on a decision boundary"
          % (family, seed, LP.IDS[which], worst, BOUND, model.adopted, model.gate_rows))
    assert worst <= BOUND
    assert 2 * model.adopted <= model.gate_rows  # most gate rows are the model's own
