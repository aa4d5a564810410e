// The calls on caller TGSW sets (include/ieache.h sections 3f to 3j and 3l: cmux, lut_tree, lut_scatter, lut_write, tlwe_rotate,
// lut_read, lut_add, lut_write_coef; and word_read of 3m, stated beside the table as kWordRead): THE statement of what such a call
// is -- its scalars and their refusal, and its arguments as plain data.
// The C ABI's device, host and reference forms (capi.cpp) and the evaluator's prelude (Evaluator::begin_set_call) loop over
// this table; nothing else states a size, a bound or a rule of these calls.  How a call is cut into pieces is cmux_plan.h.
// Free of HIP so that the CPU tests can check it (tests/native/set_calls_test.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <string>

#include "cmux_plan.h"
#include "project_plan.h"
#include "unpack_plan.h"

namespace ieache {

enum SetCallKind : int32_t { kCallCmux, kCallLutTree, kCallLutScatter, kCallLutWrite, kCallTlweRotate, kCallLutRead, kCallLutAdd, kCallLutWriteCoef, kSetCallKinds };
// The scalars of a call; what a call does not take stays as it is here.
struct SetCall {
    SetCallKind kind;
    size_t count = 0;
    int32_t depth = 0, steps = 0;
    int32_t n_sets = 1;  // n_tables (lut_tree, lut_read) or n_mems (lut_add)
    int32_t flags = 0, coef = 0;  // lut_read; coef is an index under N that the host and reference forms check after the arrays
    int32_t width = 0, unit = 0;  // lut_write_coef: the window's words and the distance between two addressed words
    bool word = false;  // word_read (section 3m): lut_read's kind and pointer arguments under kWordRead's statement below, `width`
                        // and `unit` in place of coef and the amounts (amount_of is null), count x width output rows
};

enum SetArgKind : int8_t { kArgRows, kArgIndices };
enum SetArgSize : int8_t { kSizeItems, kSizeSelectors, kSizeSteps, kSizeTables, kSizeLeaves, kSizeWords };  // rows or indices: set_arg_units
enum SetArgNeed : int8_t { kOptional, kRequired, kWithItems };  // kWithItems: null is allowed in a call without items
enum SetArgBound : int8_t { kBoundNone, kBoundSet, kBound2N, kBoundSets };  // exclusive: the set's n, 2N, n_sets
enum SetArgRole : int8_t { kInput, kMayBeOutput, kOutput };  // kMayBeOutput: the one input that may coincide exactly with the output
// where the host form stages an input: a slot for indices, one for rows, or the result rows themselves (the call then runs in place)
enum SetArgStage : int8_t { kAtNone, kAtSelectors, kAtIndicesA, kAtIndicesB, kAtRowsA, kAtRowsB, kAtTables, kAtResult };
struct SetArg {
    const char* name;  // as require_device_pointer reports it; the host forms' messages drop the "d_"
    SetArgKind kind;
    SetArgSize size;
    SetArgNeed need;
    SetArgBound bound;
    SetArgRole role;
    SetArgStage stage;
    // a call without items touches it as well (lut_add copies or zero-fills its memories): its pointer is checked at count == 0, and first
    bool empty_too;
};
constexpr int kSetCallMaxArgs = 6;
struct SetCallShape {
    const char* name;      // as the messages spell it
    bool depth, steps;     // the scalars it takes
    const char* sets;      // what it calls n_sets, or null
    int32_t known_flags;
    const char* in_place;  // what the overlap refusal calls the accepted alias, or null
    int n_args;
    SetArg args[kSetCallMaxArgs];  // in the order of the signature; the output is the last
    bool window = false;   // it takes width and unit and needs the context's projection key: "<name>: no projection key set"
                           // after the context, set and null checks and before the scalars, which write_coef_error judges
};

// an index array: always optional
constexpr SetArg arg_indices(const char* name, SetArgSize size, SetArgBound bound, SetArgStage stage) {
    return {name, kArgIndices, size, kOptional, bound, kInput, stage, false};
}
constexpr SetArg arg_rows(const char* name, SetArgSize size, SetArgNeed need, SetArgStage stage, SetArgRole role = kInput, bool empty_too = false) {
    return {name, kArgRows, size, need, kBoundNone, role, stage, empty_too};
}
constexpr SetArg kSelOf = arg_indices("d_sel_of", kSizeSelectors, kBoundSet, kAtSelectors), kTables = arg_rows("d_tables", kSizeTables, kRequired, kAtTables);
constexpr SetArg kAmountOf = arg_indices("d_amount_of", kSizeSteps, kBound2N, kAtIndicesB);  // lut_read, lut_add
constexpr SetArg kTableOf = arg_indices("d_table_of", kSizeItems, kBoundSets, kAtIndicesA);
constexpr SetArg arg_out(SetArgSize size, bool empty_too = false) { return arg_rows("d_out", size, kRequired, kAtNone, kOutput, empty_too); }
constexpr SetCallShape kSetCalls[kSetCallKinds] = {
    {"cmux", false, false, nullptr, 0, nullptr, 4,
     {arg_indices("d_sel_of", kSizeItems, kBoundSet, kAtSelectors), arg_rows("d_d1", kSizeItems, kRequired, kAtRowsA),
      arg_rows("d_d0", kSizeItems, kOptional, kAtRowsB), arg_out(kSizeItems)}},
    {"lut_tree", true, false, "n_tables", 0, nullptr, 4, {kSelOf, kTables, kTableOf, arg_out(kSizeItems)}},
    {"lut_scatter", true, false, nullptr, 0, "write", 4,
     {kSelOf, arg_rows("d_values", kSizeItems, kRequired, kAtRowsA), arg_rows("d_mem", kSizeLeaves, kOptional, kAtResult, kMayBeOutput), arg_out(kSizeLeaves)}},
    {"lut_write", true, false, nullptr, 0, "write", 4,
     {kSelOf, arg_rows("d_new", kSizeItems, kRequired, kAtRowsA), arg_rows("d_mem", kSizeLeaves, kRequired, kAtResult, kMayBeOutput), arg_out(kSizeLeaves)}},
    {"tlwe_rotate", false, true, nullptr, 0, "rotation", 4,
     {kSelOf, arg_indices("d_amount_of", kSizeSteps, kBound2N, kAtIndicesA), arg_rows("d_in", kSizeItems, kRequired, kAtRowsA, kMayBeOutput),
      arg_out(kSizeItems)}},
    // the output: rows of the words the caller of set_arg_words names, key-switched or extracted ones; the one known flag is
    // IEACHE_LUT_READ_NO_KEYSWITCH (capi.cpp asserts that the header's and the evaluator's are this one)
    {"lut_read", true, true, "n_tables", 1, nullptr, 5, {kSelOf, kAmountOf, kTables, kTableOf, arg_out(kSizeItems)}},
    {"lut_add", true, true, "n_mems", 0, "write", 6,
     {kSelOf, kAmountOf, arg_rows("d_values", kSizeItems, kWithItems, kAtRowsA), arg_rows("d_mems", kSizeTables, kOptional, kAtResult, kMayBeOutput, true),
      arg_indices("d_mem_of", kSizeItems, kBoundSets, kAtIndicesA), arg_out(kSizeTables, true)}},
    // lut_write's arguments with `steps` more selectors per item; a call without items takes null rows, the output included
    {"lut_write_coef", true, true, nullptr, 0, "write", 4,
     {kSelOf, arg_rows("d_new", kSizeItems, kWithItems, kAtRowsA), arg_rows("d_mem", kSizeLeaves, kWithItems, kAtResult, kMayBeOutput),
      arg_rows("d_out", kSizeLeaves, kWithItems, kAtNone, kOutput)}, true},
};
// word_read, the statement beside the table (the table's size is fixed by the tests): lut_read's arguments, whose amounts the
// call makes itself from `unit` -- so d_amount_of is always null -- and an output of count x width rows; its scalars are
// word_read_error's (unpack_plan.h), the one known flag IEACHE_UNPACK_NO_KEYSWITCH.  A SetCall with `word` set names it.
constexpr SetCallShape kWordRead = {"word_read", true, true, "n_tables", kUnpackNoKeyswitch, nullptr, 5, {kSelOf, kAmountOf, kTables, kTableOf, arg_out(kSizeWords)}};
inline const SetCallShape& set_call_shape(const SetCall& c) { return c.word ? kWordRead : kSetCalls[c.kind]; }
using SetPtrs = std::initializer_list<const void*>;  // a call's pointer arguments in the order of `args`: entry i is begin()[i]
inline const SetArg& set_call_output(const SetCall& c) { return set_call_shape(c).args[set_call_shape(c).n_args - 1]; }

// The first rule the scalars break as the message of the refusal, or empty: depth, then steps, then the table or memory count,
// then the flags; a call with a window: write_coef_error's rules in its order and words (project_plan.h); word_read:
// word_read_error's (unpack_plan.h).  N: the ring's.
static_assert(kCmuxMaxDepth == 12 && kRotateMaxSteps == 64, "the messages below spell the limits out");
inline std::string set_call_refusal(const SetCall& c, int32_t N) {
    const SetCallShape& s = set_call_shape(c);
    if (c.word) {
        const char* e = word_read_error(N, c.depth, c.steps, c.n_sets, c.flags, c.width, c.unit);
        return e ? std::string(e) : std::string();
    }
    if (s.window) {
        const char* e = write_coef_error(N, c.depth, c.steps, c.width, c.unit);
        return e ? std::string(e) : std::string();
    }
    const bool depth = s.depth && (c.depth < 0 || c.depth > kCmuxMaxDepth), steps = s.steps && (c.steps < 0 || c.steps > kRotateMaxSteps);
    const bool sets = s.sets && c.n_sets < 1;
    if (!depth && !steps && !sets && !(c.flags & ~s.known_flags)) return std::string();  // no string is built for a call that passes
    const std::string who = std::string(s.name) + ": ";
    if (depth) return who + "depth must lie in 0 .. 12";
    if (steps) return who + "steps must lie in 0 .. 64";
    return sets ? who + s.sets + " must be at least 1" : who + "unknown flag";
}

// rows (of kArgRows) or indices `a` holds in a call whose scalars passed set_call_refusal
inline size_t set_arg_units(const SetCall& c, const SetArg& a) {
    const SetCallShape& s = set_call_shape(c);
    const size_t depth = s.depth ? (size_t)c.depth : 0, steps = s.steps ? (size_t)c.steps : 0;
    switch (a.size) {
    case kSizeItems: return c.count;
    case kSizeSelectors: return c.count * (depth + steps);
    case kSizeSteps: return steps;
    case kSizeTables: return (size_t)c.n_sets << depth;
    case kSizeWords: return c.count * (size_t)c.width;
    default: return c.count << depth;  // kSizeLeaves
    }
}
// ... and its words on the device: rows have 2N, the output's `out_row_words` (2N as well, but for lut_read's LWE rows)
inline size_t set_arg_words(const SetCall& c, const SetArg& a, int32_t N, size_t out_row_words) {
    return set_arg_units(c, a) * (a.kind != kArgRows ? 1 : a.role == kOutput ? out_row_words : (size_t)2 * (size_t)N);
}
// the exclusive bound of an index array's entries; n_set: the samples of the set
inline int64_t set_arg_bound(const SetCall& c, const SetArg& a, int32_t N, size_t n_set) {
    return a.bound == kBoundSet ? (int64_t)n_set : a.bound == kBound2N ? 2 * (int64_t)N : a.bound == kBoundSets ? c.n_sets : 0;
}
// whether a null `a` is refused in this call
inline bool set_arg_required(const SetCall& c, const SetArg& a) { return a.need == kRequired || (a.need == kWithItems && c.count > 0); }

}  // namespace ieache
