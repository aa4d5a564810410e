"""Random sequences of levelled calls on ONE context (tests/levelled_programs.py): cmux, lut_tree, lut_scatter, lut_write,
tlwe_rotate, lut_read, lut_add, automaton_run, tlwe_extract, pack, tlwe_project, lut_write_coef, unpack, word_read and keyswitch,
with NAND and MUX gate steps and option changes between them, in orders and at sizes a seed drew -- all through
Evaluator::run_pieces on lane 0 and its scratch (the extracted rows, the key switch's digits, the CMux rows and tree buffers,
coef_idx, coef_old, the two PackScratch).  Each call's own file compares it with the C reference on a buffer that is fresh or
was left by a call of the same kind; here a call follows calls of other kinds, larger and smaller, under other options.

The state stays on the card in one tensor, every entry between guard words, LWE rows at the padded stride.  After EVERY step the
rows the step wrote equal the reference interpreter's word for word and nothing else in the tensor changed -- entries only read,
guards, padding words (those of the rows a step wrote may have become zero: a key switch writes its rows whole, "the padding as
zero", include/ieache.h; every other row's padding keeps its guard pattern); a failure names the step.  Gate steps have no C reference in ieache_amd.tools: theirs is the same gate
call issued on the same rows through the host form before the program starts (and, on client-encrypted rows in the last test,
the CPU oracle's).  Every comparison is exact."""
import threading

import numpy as np
import pytest

import levelled_programs as LP

pytestmark = pytest.mark.gpu

CORPUS = LP.corpus()
CORPUS_IDS = ["%s%d" % (family, seed) for seed, family in CORPUS]
# (A, B): B runs first on the context, then A, which must give what it gives alone
ORDERS = [((5, "grow"), (4, "shrink")), ((4, "shrink"), (5, "grow")), ((0, "mixed"), (1, "mixed")), ((1, "mixed"), (0, "mixed"))]


def trace(what):
    print(what, flush=True)


def setup(gpu_ctx, which):
    kw, gadget = LP.SETS[which]
    kb, ctx = gpu_ctx(LP.KEY_N, LP.N, **kw)
    return kb, ctx, gadget


def keyswitch_of(kb):
    return lambda u: np.stack([kb.ck.keyswitch(row) for row in u])


def reference(kb, ctx, which, seed, family):
    """(steps, state, writes, final) of a corpus program on a set, computed once per session and left unchanged.  Its gate steps
    are the host gate calls on the reference's own rows, issued here -- before any program runs."""
    def make():
        gadget = LP.SETS[which][1]
        steps, state = LP.program(seed, family), LP.initial_state(LP.set_params(kb.p, gadget))

        def gate(kind, a, b, c):
            return ctx.gates(LP.GATE_NAND, a, b) if kind == "gates" else ctx.mux(a, b, c)
        writes, final = LP.run_reference(steps, state, LP.set_params(kb.p, gadget), kb.ksk, gate, keyswitch_of(kb))
        return steps, state, writes, final
    return LP.once(("reference", which, seed, family), make)


def same_state(got, want):
    for name, a in got.items():
        assert np.array_equal(a, want[name]), "entry %s differs" % name


@pytest.mark.parametrize("which", range(3), ids=LP.IDS)
@pytest.mark.parametrize("seed,family", CORPUS, ids=CORPUS_IDS)
def test_every_step_against_the_reference(gpu_ctx, seed, family, which):
    kb, ctx, gadget = setup(gpu_ctx, which)
    steps, state, writes, final = reference(kb, ctx, which, seed, family)
    found = {name: ctx.get_option(name) for name in list(LP.OPTION_VALUES) + ["force_generic"]}
    got = LP.run_context(steps, state, ctx, gadget, writes=writes, log=trace)
    same_state(got, final)
    # options(): every option is back as it was found, and the keys are gone
    assert {name: ctx.get_option(name) for name in found} == found
    with pytest.raises(Exception, match="no packing key set"):
        ctx.pack(np.zeros((1, kb.p.n + 1), dtype=np.int32))


@pytest.mark.parametrize("seed,family", CORPUS, ids=CORPUS_IDS)
def test_every_program_on_a_fresh_context(ia, gpu_ctx, seed, family):
    """The session's contexts have run whatever ran before this file, and a buffer only grows: a call that reserves too little
    shows on a context whose buffers are as small as the program's own calls left them.  Each program on a context of its own."""
    kb, ctx, gadget = setup(gpu_ctx, 0)
    steps, state, writes, final = reference(kb, ctx, 0, seed, family)
    fresh = ia.Context.from_arrays(kb.p, kb.bk, kb.ksk)
    try:
        same_state(LP.run_context(steps, state, fresh, gadget, writes=writes, log=trace), final)
    finally:
        fresh.close()


@pytest.mark.parametrize("which", range(3), ids=LP.IDS)
def test_order_independence(gpu_ctx, which):
    """B, then A on the same context: A ends where it ends alone.  Then once more behind a warm-up pass of the corpus's largest
    program, after which no buffer grows and no reallocation synchronises the device for anybody: the same words."""
    kb, ctx, gadget = setup(gpu_ctx, which)
    for warm in (False, True):
        for a, b in ORDERS:
            if warm:
                steps, state, _w, _f = reference(kb, ctx, which, *LP.largest_program())
                LP.run_context(steps, state, ctx, gadget)
            steps_b, state_b, _w, final_b = reference(kb, ctx, which, *b)
            same_state(LP.run_context(steps_b, state_b, ctx, gadget), final_b)
            steps_a, state_a, writes_a, final_a = reference(kb, ctx, which, *a)
            trace("%s after %s%s" % (a, b, ", warm" if warm else ""))
            same_state(LP.run_context(steps_a, state_a, ctx, gadget, writes=writes_a, log=trace), final_a)


@pytest.mark.parametrize("which", range(3), ids=LP.IDS)
@pytest.mark.parametrize("seed,family", CORPUS, ids=CORPUS_IDS)
def test_option_independence(gpu_ctx, seed, family, which):
    """the program without its option steps, under the defaults: the same final state"""
    kb, ctx, gadget = setup(gpu_ctx, which)
    steps, state, _writes, final = reference(kb, ctx, which, seed, family)
    bare = LP.strip_options(steps)
    assert len(bare) < len(steps) or family == "memory"
    same_state(LP.run_context(bare, state, ctx, gadget, log=trace), final)


@pytest.mark.parametrize("which", range(3), ids=LP.IDS)
def test_two_contexts_on_one_card_from_two_host_threads(ia, gpu_ctx, which):
    """the session's context and a second one on the same card, each running another program at the same time from a host thread
    of its own: each ends where the program ends single-threaded"""
    kb, ctx, gadget = setup(gpu_ctx, which)
    jobs = [reference(kb, ctx, which, 0, "mixed"), reference(kb, ctx, which, 3, "way_back")]
    other = ia.Context.from_arrays(kb.p, kb.bk, kb.ksk)
    try:
        results, errors = [None, None], []

        def work(slot, context):
            try:
                steps, state, writes, _final = jobs[slot]
                results[slot] = LP.run_context(steps, state, context, gadget, writes=writes)
            except BaseException as e:  # noqa: BLE001 -- handed to the main thread, which raises it
                errors.append(e)
        threads = [threading.Thread(target=work, args=(slot, context)) for slot, context in enumerate((ctx, other))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if errors:
            raise errors[0]
        for slot in range(2):
            same_state(results[slot], jobs[slot][3])
    finally:
        other.close()


@pytest.mark.parametrize("seed,family,which", [(0, "mixed", 0), (3, "way_back", 0), (1, "mixed", 1)], ids=["mixed0_l3_Bg7", "way_back3_l3_Bg7", "mixed1_l2_Bg10"])
def test_gate_steps_and_meaning_on_client_encrypted_rows(gpu_ctx, seed, family, which):
    """The meaning programs of tests/test_levelled_programs_cpu.py on the card: every step, the NAND and MUX steps on rows that
    came the way back included, equals the reference interpreter word for word -- the gate steps' reference is the CPU oracle here
    -- and every gate step's rows decrypt to the model's bits."""
    from test_levelled_programs_cpu import run_by_meaning
    kb, ctx, gadget = setup(gpu_ctx, which)
    steps = LP.program(seed, family)
    state, _model = LP.encrypted_state(kb, gadget, seed)
    _worst, model, writes, final = run_by_meaning(kb, gadget, seed, family)
    # the same gate calls on the same rows, issued before the program starts
    at = {k: v.copy() for k, v in state.items() if k == "lwe"}
    for i, s in enumerate(steps):
        if s["op"] == "gate":
            a, b, c = (LP._fetch(at, s["args"].get(name)) for name in ("a", "b", "c"))
            early = ctx.gates(LP.GATE_NAND, a, b) if s["kind"] == "gates" else ctx.mux(a, b, c)
            assert np.array_equal(early, writes[i]), LP.describe(i, s)
        if s["op"] != "option" and s["out"][0] == "lwe":
            at["lwe"][s["out"][1]:s["out"][1] + s["out"][2]] = writes[i]
    got = LP.run_context(steps, state, ctx, gadget, writes=writes, log=trace)
    same_state(got, final)
    assert model.gate_rows > 0
    for entry in ("mem", "tab", "tlwe", "lwe", "ext"):
        assert LP.decoded_error(kb, entry, got[entry], model.m[entry]) <= 1.0 / 32
