// csrc/set_calls.h on its own (no HIP): for each of the eight calls on a set the refusal of its scalars -- exact messages, the
// first failing rule when two are broken -- the words of every argument at a few scalars, and which arguments are optional,
// which one may be the output, and every bound.  The expectations restate include/ieache.h sections 3f to 3j, and 3l for the
// eighth (lut_write_coef, whose block is write_coef() below), on purpose: they are the second statement that keeps the header's honest.  Built with AddressSanitizer + UBSan by tests/test_set_calls_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../ie-ache_amd/csrc/set_calls.h"

using namespace ieache;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);        \
            exit(1);                                                   \
        }                                                              \
    } while (0)

static const int N = 1024;
static const size_t ROW = 2048, LWE = 632, N_SET = 5;  // words of a TLWE row and of lut_read's output row; samples of the set
static const int kSeven = kCallLutWriteCoef;  // the calls of sections 3f to 3j, which the three blocks after this one walk
static_assert(kSeven == 7 && kSetCallKinds == 8, "seven calls sized by (count, depth, steps, n_sets) alone, and the write of a window");
// every scalar refusal at the test's ring
static std::string set_call_refusal(const SetCall& c) { return ieache::set_call_refusal(c, N); }

static const SetArg& arg(SetCallKind k, const char* name) {
    const SetCallShape& s = kSetCalls[k];
    for (int i = 0; i < s.n_args; i++)
        if (!strcmp(s.args[i].name, name)) return s.args[i];
    printf("FAIL: %s has no argument %s\n", s.name, name);
    exit(1);
}
static size_t words(const SetCall& c, const char* name) { return set_arg_words(c, arg(c.kind, name), N, c.kind == kCallLutRead ? LWE : ROW); }
static bool is(const std::string& got, const char* want) {
    if (got != want) printf("got \"%s\", want \"%s\"\n", got.c_str(), want);
    return got == want;
}
static SetCall call(SetCallKind k, size_t count, int32_t depth = 0, int32_t steps = 0, int32_t n_sets = 1, int32_t flags = 0) {
    SetCall c{k};
    c.count = count, c.depth = depth, c.steps = steps, c.n_sets = n_sets, c.flags = flags;
    return c;
}

// one argument as the issue's table gives it: (call, name, kind, optional, may be the output, is the output, bound or -1)
struct Want {
    SetCallKind k;
    const char* name;
    SetArgKind kind;
    bool optional, alias, output;
    int64_t bound;
};
static const int32_t N_SETS = 3;  // n_tables / n_mems of the calls whose bounds are asked
static const Want kWant[] = {
    {kCallCmux, "d_sel_of", kArgIndices, true, false, false, 5},        {kCallCmux, "d_d1", kArgRows, false, false, false, -1},
    {kCallCmux, "d_d0", kArgRows, true, false, false, -1},              {kCallCmux, "d_out", kArgRows, false, false, true, -1},
    {kCallLutTree, "d_sel_of", kArgIndices, true, false, false, 5},     {kCallLutTree, "d_tables", kArgRows, false, false, false, -1},
    {kCallLutTree, "d_table_of", kArgIndices, true, false, false, 3},   {kCallLutTree, "d_out", kArgRows, false, false, true, -1},
    {kCallLutScatter, "d_sel_of", kArgIndices, true, false, false, 5},  {kCallLutScatter, "d_values", kArgRows, false, false, false, -1},
    {kCallLutScatter, "d_mem", kArgRows, true, true, false, -1},        {kCallLutScatter, "d_out", kArgRows, false, false, true, -1},
    {kCallLutWrite, "d_sel_of", kArgIndices, true, false, false, 5},    {kCallLutWrite, "d_new", kArgRows, false, false, false, -1},
    {kCallLutWrite, "d_mem", kArgRows, false, true, false, -1},         {kCallLutWrite, "d_out", kArgRows, false, false, true, -1},
    {kCallTlweRotate, "d_sel_of", kArgIndices, true, false, false, 5},  {kCallTlweRotate, "d_amount_of", kArgIndices, true, false, false, 2048},
    {kCallTlweRotate, "d_in", kArgRows, false, true, false, -1},        {kCallTlweRotate, "d_out", kArgRows, false, false, true, -1},
    {kCallLutRead, "d_sel_of", kArgIndices, true, false, false, 5},     {kCallLutRead, "d_amount_of", kArgIndices, true, false, false, 2048},
    {kCallLutRead, "d_tables", kArgRows, false, false, false, -1},      {kCallLutRead, "d_table_of", kArgIndices, true, false, false, 3},
    {kCallLutRead, "d_out", kArgRows, false, false, true, -1},  // coef, one index under N, is no pointer: the forms check SetCall::coef
    {kCallLutAdd, "d_sel_of", kArgIndices, true, false, false, 5},      {kCallLutAdd, "d_amount_of", kArgIndices, true, false, false, 2048},
    {kCallLutAdd, "d_values", kArgRows, false, false, false, -1},       {kCallLutAdd, "d_mems", kArgRows, true, true, false, -1},
    {kCallLutAdd, "d_mem_of", kArgIndices, true, false, false, 3},      {kCallLutAdd, "d_out", kArgRows, false, false, true, -1},
};

static void shapes() {
    const char* names[kSeven] = {"cmux", "lut_tree", "lut_scatter", "lut_write", "tlwe_rotate", "lut_read", "lut_add"};
    const int n_args[kSeven] = {4, 4, 4, 4, 4, 5, 6};
    int seen[kSeven] = {};
    for (int k = 0; k < kSeven; k++) {
        CHECK(!strcmp(kSetCalls[k].name, names[k]) && kSetCalls[k].n_args == n_args[k] && n_args[k] <= kSetCallMaxArgs);
        CHECK(&set_call_output(call((SetCallKind)k, 1)) == &kSetCalls[k].args[n_args[k] - 1]);
    }
    for (const Want& w : kWant) {
        // in the order of the signature: entry i of a call's expectations is its argument i
        const SetArg& a = kSetCalls[w.k].args[seen[w.k]++];
        CHECK(&a == &arg(w.k, w.name));
        const SetCall c = call(w.k, 2, 1, 1, N_SETS);
        CHECK(a.kind == w.kind && (a.need == kOptional) == w.optional && (a.role == kMayBeOutput) == w.alias && (a.role == kOutput) == w.output);
        CHECK(set_arg_required(c, a) == !w.optional);
        CHECK((a.bound == kBoundNone) == (w.bound < 0));
        if (w.bound >= 0) CHECK(set_arg_bound(c, a, N, N_SET) == w.bound);
    }
    for (int k = 0; k < kSeven; k++) CHECK(seen[k] == n_args[k]);
    // lut_add's values are required only with items, and an empty lut_add touches its memories and its output; nothing else is so
    const SetArg& v = arg(kCallLutAdd, "d_values");
    CHECK(v.need == kWithItems && !set_arg_required(call(kCallLutAdd, 0), v) && set_arg_required(call(kCallLutAdd, 1), v));
    for (int k = 0; k < kSeven; k++)
        for (int i = 0; i < kSetCalls[k].n_args; i++) {
            const SetArg& a = kSetCalls[k].args[i];
            CHECK(a.empty_too == (k == kCallLutAdd && (!strcmp(a.name, "d_mems") || !strcmp(a.name, "d_out"))));
            if (&a != &v) CHECK(a.need != kWithItems);
        }
}

static void refusals() {
    for (int k = 0; k < kSeven; k++) {
        const SetCallKind kind = (SetCallKind)k;
        const std::string name = kSetCalls[k].name;
        const bool has_depth = k != kCallCmux && k != kCallTlweRotate, has_steps = k == kCallTlweRotate || k == kCallLutRead || k == kCallLutAdd;
        const char* sets = k == kCallLutTree || k == kCallLutRead ? "n_tables" : k == kCallLutAdd ? "n_mems" : nullptr;
        const std::string depth_msg = name + ": depth must lie in 0 .. 12", steps_msg = name + ": steps must lie in 0 .. 64";
        const std::string sets_msg = name + ": " + (sets ? sets : "") + " must be at least 1";
        for (int32_t d : {-1, 0, 12, 13}) CHECK(is(set_call_refusal(call(kind, 1, d)), has_depth && (d < 0 || d > 12) ? depth_msg.c_str() : ""));
        for (int32_t t : {-1, 0, 64, 65}) CHECK(is(set_call_refusal(call(kind, 1, 0, t)), has_steps && (t < 0 || t > 64) ? steps_msg.c_str() : ""));
        for (int32_t n : {0, 1}) CHECK(is(set_call_refusal(call(kind, 1, 0, 0, n)), sets && n < 1 ? sets_msg.c_str() : ""));
        CHECK(is(set_call_refusal(call(kind, 0, 12, 64, 1)), ""));
        // every unknown flag bit of lut_read; the known one passes; the other calls take no flags, and a SetCall of theirs has none
        for (int bit = 0; bit < 32; bit++)
            CHECK(is(set_call_refusal(call(kCallLutRead, 1, 0, 0, 1, (int32_t)(1u << bit))), bit == 0 ? "" : "lut_read: unknown flag"));
        CHECK(is(set_call_refusal(call(kCallLutRead, 1, 0, 0, 1, 3)), "lut_read: unknown flag"));
        // two at once: depth before steps before the count before the flags
        if (has_depth && has_steps) CHECK(is(set_call_refusal(call(kind, 1, 13, 65, 0, k == kCallLutRead ? 2 : 0)), depth_msg.c_str()));
        if (has_depth && sets) CHECK(is(set_call_refusal(call(kind, 1, -1, 0, 0)), depth_msg.c_str()));
        if (has_steps && sets) CHECK(is(set_call_refusal(call(kind, 1, 0, 65, 0, k == kCallLutRead ? 2 : 0)), steps_msg.c_str()));
        if (k == kCallLutRead) CHECK(is(set_call_refusal(call(kind, 1, 0, 0, 0, 2)), sets_msg.c_str()));
    }
    CHECK(is(set_call_refusal(call(kCallLutTree, 1, 13)), "lut_tree: depth must lie in 0 .. 12"));
    CHECK(is(set_call_refusal(call(kCallLutAdd, 1, 0, 0, 0)), "lut_add: n_mems must be at least 1"));
    CHECK(is(set_call_refusal(call(kCallLutRead, 1, 0, -1, 0)), "lut_read: steps must lie in 0 .. 64"));
}

static void sizes() {
    // count = 0: only what does not scale with the items holds anything
    CHECK(words(call(kCallCmux, 0), "d_sel_of") == 0 && words(call(kCallCmux, 0), "d_d1") == 0 && words(call(kCallCmux, 0), "d_out") == 0);
    CHECK(words(call(kCallLutTree, 0, 2, 0, 3), "d_tables") == 24576 && words(call(kCallLutTree, 0, 2, 0, 3), "d_out") == 0);
    CHECK(words(call(kCallLutScatter, 0, 2), "d_mem") == 0 && words(call(kCallLutScatter, 0, 2), "d_out") == 0);
    CHECK(words(call(kCallLutWrite, 0, 2), "d_mem") == 0 && words(call(kCallLutWrite, 0, 2), "d_new") == 0);
    CHECK(words(call(kCallTlweRotate, 0, 0, 10), "d_amount_of") == 10 && words(call(kCallTlweRotate, 0, 0, 10), "d_sel_of") == 0);
    CHECK(words(call(kCallLutRead, 0, 2, 10, 3), "d_tables") == 24576 && words(call(kCallLutRead, 0, 2, 10, 3), "d_out") == 0);
    CHECK(words(call(kCallLutRead, 0, 2, 10, 3), "d_amount_of") == 10 && words(call(kCallLutRead, 0, 2, 10, 3), "d_table_of") == 0);
    CHECK(words(call(kCallLutAdd, 0, 2, 10, 3), "d_mems") == 24576 && words(call(kCallLutAdd, 0, 2, 10, 3), "d_out") == 24576);
    CHECK(words(call(kCallLutAdd, 0, 2, 10, 3), "d_values") == 0 && words(call(kCallLutAdd, 0, 2, 10, 3), "d_mem_of") == 0);
    // count = 1, depth 0, steps 0
    for (int k = 0; k < kSeven; k++) {
        const SetCall c = call((SetCallKind)k, 1);
        CHECK(words(c, "d_sel_of") == (k == kCallCmux ? 1u : 0u));
        CHECK(words(c, "d_out") == (k == kCallLutRead ? LWE : ROW));
    }
    CHECK(words(call(kCallCmux, 1), "d_d1") == 2048 && words(call(kCallCmux, 1), "d_d0") == 2048);
    CHECK(words(call(kCallLutTree, 1), "d_tables") == 2048 && words(call(kCallLutTree, 1), "d_table_of") == 1);
    CHECK(words(call(kCallLutScatter, 1), "d_values") == 2048 && words(call(kCallLutScatter, 1), "d_mem") == 2048);
    CHECK(words(call(kCallLutWrite, 1), "d_new") == 2048 && words(call(kCallLutWrite, 1), "d_mem") == 2048);
    CHECK(words(call(kCallTlweRotate, 1), "d_amount_of") == 0 && words(call(kCallTlweRotate, 1), "d_in") == 2048);
    CHECK(words(call(kCallLutRead, 1), "d_amount_of") == 0 && words(call(kCallLutRead, 1), "d_tables") == 2048 && words(call(kCallLutRead, 1), "d_table_of") == 1);
    CHECK(words(call(kCallLutAdd, 1), "d_values") == 2048 && words(call(kCallLutAdd, 1), "d_mems") == 2048 && words(call(kCallLutAdd, 1), "d_mem_of") == 1);
    // depth 12 with three tables or memories, seven items, and (where taken) 64 steps: 3 x 4096 rows are 25 165 824 words
    CHECK(words(call(kCallLutTree, 7, 12, 0, 3), "d_tables") == 25165824 && words(call(kCallLutTree, 7, 12, 0, 3), "d_sel_of") == 84);
    CHECK(words(call(kCallLutTree, 7, 12, 0, 3), "d_table_of") == 7 && words(call(kCallLutTree, 7, 12, 0, 3), "d_out") == 14336);
    CHECK(words(call(kCallLutRead, 7, 12, 64, 3), "d_tables") == 25165824 && words(call(kCallLutRead, 7, 12, 64, 3), "d_sel_of") == 532);
    CHECK(words(call(kCallLutRead, 7, 12, 64, 3), "d_amount_of") == 64 && words(call(kCallLutRead, 7, 12, 64, 3), "d_out") == 4424);
    CHECK(words(call(kCallLutAdd, 7, 12, 64, 3), "d_mems") == 25165824 && words(call(kCallLutAdd, 7, 12, 64, 3), "d_out") == 25165824);
    CHECK(words(call(kCallLutAdd, 7, 12, 64, 3), "d_sel_of") == 532 && words(call(kCallLutAdd, 7, 12, 64, 3), "d_values") == 14336);
    CHECK(words(call(kCallLutScatter, 7, 12), "d_out") == 58720256 && words(call(kCallLutScatter, 7, 12), "d_sel_of") == 84);
    CHECK(words(call(kCallLutWrite, 7, 12), "d_mem") == 58720256 && words(call(kCallLutWrite, 7, 12), "d_new") == 14336);
    CHECK(words(call(kCallTlweRotate, 7, 0, 64), "d_sel_of") == 448 && words(call(kCallTlweRotate, 7, 0, 64), "d_out") == 14336);
    // 2^20 items at depth 12: 2^32 rows of 2^11 words, formed in size_t without wrapping
    static_assert(sizeof(size_t) == 8, "the products below need 64 bits");
    const size_t M = (size_t)1 << 20;
    CHECK(words(call(kCallLutScatter, M, 12), "d_out") == 8796093022208u && words(call(kCallLutScatter, M, 12), "d_mem") == 8796093022208u);
    CHECK(words(call(kCallLutWrite, M, 12), "d_out") == 8796093022208u && words(call(kCallLutWrite, M, 12), "d_sel_of") == 12582912u);
    CHECK(words(call(kCallLutScatter, M, 12), "d_values") == 2147483648u && words(call(kCallCmux, M), "d_out") == 2147483648u);
    CHECK(words(call(kCallLutTree, M, 12, 0, 3), "d_sel_of") == 12582912u && words(call(kCallLutTree, M, 12, 0, 3), "d_out") == 2147483648u);
    CHECK(words(call(kCallLutRead, M, 12, 64, 3), "d_sel_of") == 79691776u && words(call(kCallLutRead, M, 12, 64, 3), "d_out") == 662700032u);
    CHECK(words(call(kCallLutAdd, M, 12, 64, 3), "d_sel_of") == 79691776u && words(call(kCallLutAdd, M, 12, 64, 3), "d_out") == 25165824u);
    CHECK(words(call(kCallTlweRotate, M, 0, 64), "d_sel_of") == 67108864u && words(call(kCallTlweRotate, M, 0, 64), "d_in") == 2147483648u);
    // a scalar a call does not take never enters its sizes
    CHECK(words(call(kCallCmux, 3, 5, 7, 9), "d_sel_of") == 3 && words(call(kCallTlweRotate, 3, 5, 2), "d_sel_of") == 6);
    CHECK(words(call(kCallLutTree, 3, 2, 7, 1), "d_sel_of") == 6 && words(call(kCallLutScatter, 3, 2, 7), "d_sel_of") == 6);
}

// The eighth call, the replace write of a window (include/ieache.h section 3l): lut_write's arguments with `steps` more selectors
// per item, the scalars width and unit, and the projection key (which the forms ask the context for: `window` marks it).
static SetCall coef_call(size_t count, int32_t depth, int32_t steps, int32_t width, int32_t unit) {
    SetCall c = call(kCallLutWriteCoef, count, depth, steps);
    c.width = width, c.unit = unit;
    return c;
}
static void write_coef() {
    const SetCallShape& s = kSetCalls[kCallLutWriteCoef];
    CHECK(!strcmp(s.name, "lut_write_coef") && s.n_args == 4 && s.depth && s.steps && !s.sets && s.known_flags == 0 && s.window && !strcmp(s.in_place, "write"));
    for (int k = 0; k < kSeven; k++) CHECK(!kSetCalls[k].window);
    // the arguments in the order of the signature: sel_of optional and bounded by the set; new, mem and out needed only with
    // items; mem may be the output exactly and is staged at the result; nothing is touched by a call without items
    const char* names[4] = {"d_sel_of", "d_new", "d_mem", "d_out"};
    for (int i = 0; i < 4; i++) CHECK(!strcmp(s.args[i].name, names[i]) && !s.args[i].empty_too);
    CHECK(&set_call_output(coef_call(1, 0, 0, 1, 1)) == &s.args[3] && s.args[3].role == kOutput && s.args[3].kind == kArgRows);
    const SetArg &sel = s.args[0], &fresh = s.args[1], &mem = s.args[2], &out = s.args[3];
    CHECK(sel.kind == kArgIndices && sel.need == kOptional && sel.role == kInput && sel.size == kSizeSelectors);
    CHECK(set_arg_bound(coef_call(3, 2, 2, 1, 1), sel, N, N_SET) == (int64_t)N_SET);
    CHECK(fresh.kind == kArgRows && fresh.role == kInput && fresh.bound == kBoundNone && fresh.stage == kAtRowsA);
    CHECK(mem.kind == kArgRows && mem.role == kMayBeOutput && mem.bound == kBoundNone && mem.stage == kAtResult);
    for (const SetArg* a : {&fresh, &mem, &out}) {
        CHECK(a->need == kWithItems && set_arg_required(coef_call(1, 0, 0, 1, 1), *a) && !set_arg_required(coef_call(0, 0, 0, 1, 1), *a));
    }
    CHECK(!set_arg_required(coef_call(1, 0, 0, 1, 1), sel));
    // every scalar rule with its exact message
    const char *depth_msg = "lut_write_coef: depth must lie in 0 .. 12", *steps_msg = "lut_write_coef: steps must lie in 0 .. 64";
    const char *width_msg = "lut_write_coef: width must be at least 1", *unit_msg = "lut_write_coef: unit must be at least width";
    const char* span_msg = "lut_write_coef: unit x 2^steps must not exceed N";
    for (int32_t d : {-1, 0, 12, 13}) CHECK(is(set_call_refusal(coef_call(1, d, 0, 1, 1)), d < 0 || d > 12 ? depth_msg : ""));
    for (int32_t t : {-1, 65}) CHECK(is(set_call_refusal(coef_call(1, 0, t, 1, 1)), steps_msg));
    for (int32_t w : {-1, 0}) CHECK(is(set_call_refusal(coef_call(1, 0, 0, w, 1)), width_msg));
    CHECK(is(set_call_refusal(coef_call(1, 0, 0, 4, 3)), unit_msg) && is(set_call_refusal(coef_call(1, 0, 0, 4, 4)), ""));
    // unit 2^steps against N = 1024: 10 steps of unit 1 and 5 of unit 32 fill a sample; one more, or steps the shift cannot take, do not
    CHECK(is(set_call_refusal(coef_call(1, 12, 10, 1, 1)), "") && is(set_call_refusal(coef_call(1, 4, 5, 32, 32)), "") && is(set_call_refusal(coef_call(0, 0, 0, 1024, 1024)), ""));
    CHECK(is(set_call_refusal(coef_call(1, 0, 11, 1, 1)), span_msg) && is(set_call_refusal(coef_call(1, 0, 5, 32, 33)), span_msg));
    CHECK(is(set_call_refusal(coef_call(1, 0, 31, 1, 1)), span_msg) && is(set_call_refusal(coef_call(1, 0, 64, 1, 1)), span_msg));
    CHECK(is(set_call_refusal(coef_call(1, 0, 1, 1, 2147483647)), span_msg) && is(set_call_refusal(coef_call(1, 0, 0, 1, 1025)), span_msg));
    CHECK(is(ieache::set_call_refusal(coef_call(1, 0, 6, 1, 1), 64), "") && is(ieache::set_call_refusal(coef_call(1, 0, 7, 1, 1), 64), span_msg));  // N is the ring's
    // the first failing rule: depth, steps, width, unit, unit x 2^steps
    CHECK(is(set_call_refusal(coef_call(1, 13, 65, 0, -1)), depth_msg) && is(set_call_refusal(coef_call(1, 0, 65, 0, -1)), steps_msg));
    CHECK(is(set_call_refusal(coef_call(1, 0, 11, 0, -1)), width_msg) && is(set_call_refusal(coef_call(1, 0, 11, 2, 1)), unit_msg));
    CHECK(is(set_call_refusal(coef_call(1, 0, 11, 2, 2)), span_msg));
    // n_sets, flags and coef are not this call's
    SetCall odd = coef_call(1, 0, 0, 1, 1);
    odd.n_sets = 0, odd.flags = 6, odd.coef = -1;
    CHECK(is(set_call_refusal(odd), ""));
    // the words of each argument: no items; 3 items at depth 2 with 2 steps; one item at depth 0 with no steps; 2^20 items at depth 12
    CHECK(words(coef_call(0, 2, 2, 1, 1), "d_sel_of") == 0 && words(coef_call(0, 2, 2, 1, 1), "d_new") == 0 && words(coef_call(0, 2, 2, 1, 1), "d_mem") == 0 &&
          words(coef_call(0, 2, 2, 1, 1), "d_out") == 0);
    const SetCall c = coef_call(3, 2, 2, 1, 1);
    CHECK(words(c, "d_sel_of") == 12 && words(c, "d_new") == 6144 && words(c, "d_mem") == 24576 && words(c, "d_out") == 24576);
    CHECK(words(coef_call(1, 0, 0, 1, 1), "d_sel_of") == 0 && words(coef_call(1, 0, 0, 1, 1), "d_new") == 2048 && words(coef_call(1, 0, 0, 1, 1), "d_mem") == 2048 &&
          words(coef_call(1, 0, 0, 1, 1), "d_out") == 2048);
    const SetCall big = coef_call((size_t)1 << 20, 12, 10, 1, 1);
    CHECK(words(big, "d_sel_of") == 23068672u && words(big, "d_new") == 2147483648u && words(big, "d_mem") == 8796093022208u && words(big, "d_out") == 8796093022208u);
    // width and unit never enter a size
    CHECK(words(coef_call(3, 2, 2, 32, 64), "d_sel_of") == 12 && words(coef_call(3, 2, 2, 32, 64), "d_mem") == 24576);
}

int main() {
    shapes();
    refusals();
    sizes();
    write_coef();
    printf("SET_CALLS_OK\n");
    return 0;
}
