// The way back from the levelled memory to the gates (include/ieache.h section 3m): the unpacking key switch -- a window of
// coefficients of TLWE samples as LWE rows, the partner of pack -- and the read of an addressed word built on it (word_read, the
// partner of lut_write_coef): which calls are accepted and how their rows are cut: THE statement of it.  Free of HIP so that the
// CPU tests can check it (tests/native/unpack_plan_test.cpp).
//
//   row r of a call = (item r / width, q = r % width): the extracted row of coefficient first + q spread of sample `item`,
//   key-switched by lweKeySwitch (ks_plan.h chooses the kernel) or, with kUnpackNoKeyswitch, handed out as it is.
//
//   k_ksm_window         where the run's plan is the MFMA product: the transposed digits and the initial output rows of the
//                        run's rows straight from the samples -- what k_ksm_digits and k_ksm_init make from stored rows
//   k_ksm_window_rows    every other family, and kUnpackNoKeyswitch: the run's extracted rows, stored
//
// The count x width rows are cut into runs of at most `chunk` rows, as every flat call's are; a run may begin and end inside an
// item.  word_read is cut into the tree's pieces for (count, depth) (cmux_plan.h) and unpacks the items x width rows of a piece
// in such runs.
#pragma once
#include "cmux_plan.h"
#include "project_plan.h"

namespace ieache {

constexpr int32_t kUnpackNoKeyswitch = 1;  // IEACHE_UNPACK_NO_KEYSWITCH: the one flag of both calls

// The public window of a call: coefficients first + q spread, q < width.
struct UnpackWindow {
    int32_t first = 0, width = 1, spread = 1;
};
inline int32_t unpack_coef(const UnpackWindow& w, int64_t q) { return (int32_t)(w.first + q * w.spread); }

// Why the window of an unpack call is refused, or null: first in [0, N), width >= 1, spread >= 1, first + (width - 1) spread < N.
inline const char* unpack_window_error(int32_t N, int32_t first, int32_t width, int32_t spread) {
    if (first < 0 || first >= N) return "unpack: first must lie in [0, N)";
    if (width < 1) return "unpack: width must be at least 1";
    if (spread < 1) return "unpack: spread must be at least 1";
    if ((int64_t)first + ((int64_t)width - 1) * spread >= N) return "unpack: first + (width - 1) x spread must stay below N";
    return nullptr;
}
inline const char* unpack_call_error(int32_t N, int32_t first, int32_t width, int32_t spread, int32_t flags) {
    if (const char* e = unpack_window_error(N, first, width, spread)) return e;
    return flags & ~kUnpackNoKeyswitch ? "unpack: unknown flag" : nullptr;
}

// rows of `items` items, and their cut into runs of at most `chunk` rows (chunk < 1: one run)
inline int64_t unpack_rows(int64_t items, int32_t width) { return items * (int64_t)width; }
inline Cut unpack_runs(int64_t items, int32_t width, int64_t chunk) {
    const int64_t rows = unpack_rows(items, width);
    return cut_in_runs(rows, chunk < 1 || chunk > rows ? rows : chunk);
}

// Why the scalars of a word read are refused, or null: lut_read's rules in lut_read's order (depth, steps, n_tables, flags),
// then the window's, which are the write's (word_window_rule, project_plan.h).
static_assert(kCmuxMaxDepth == 12 && kRotateMaxSteps == 64, "the messages below spell the limits out");
inline const char* word_read_error(int32_t N, int32_t depth, int32_t steps, int32_t n_tables, int32_t flags, int32_t width, int32_t unit) {
    if (depth < 0 || depth > kCmuxMaxDepth) return "word_read: depth must lie in 0 .. 12";
    if (steps < 0 || steps > kRotateMaxSteps) return "word_read: steps must lie in 0 .. 64";
    if (n_tables < 1) return "word_read: n_tables must be at least 1";
    if (flags & ~kUnpackNoKeyswitch) return "word_read: unknown flag";
    switch (word_window_rule(N, steps, width, unit)) {
    case 1: return "word_read: width must be at least 1";
    case 2: return "word_read: unit must be at least width";
    case 3: return "word_read: unit x 2^steps must not exceed N";
    default: return nullptr;
    }
}

}  // namespace ieache
