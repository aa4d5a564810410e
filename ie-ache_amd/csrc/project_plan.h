// The TLWE projection (TLWE sample -> TLWE sample carrying a window of its coefficients and nothing else; include/ieache.h
// section 3l) and the replace write of a window (lut_write_coef): which calls are accepted and how they are cut: THE statement
// of it.  Free of HIP so that the CPU tests can check it (tests/native/project_plan_test.cpp).
//
// The projection is the packing key switch of section 3e on the parameter set with n := N (project_params) and the ring key as
// its source key: the extracted key of a TLWE sample is the ring key itself.  Every rule of pack_plan.h therefore holds with
// that set -- pack_set_error is the refusal of a decomposition, pack_plan the cut, with an ITEM (a sample and its `width`
// extracted rows) where a packing call has a group of m rows:
//
//   k_window_digits  per piece: the digits of the `width` extracted rows of each sample in k_pack_gemm's A layout, and
//                    R = (0, B[first + q] X^0); the extracted rows themselves are never stored
//   k_pack_gemm      per piece, unchanged, K = N t
//   k_pack_place     per piece, unchanged: one group per item, m = width, spread = 1, shift = dest
//
// Pieces are whole items with items x width rows within "pack_piece_rows" (an item of N <= 1 024 rows fits a piece of the
// default 4 096).  The replace write is cut into the tree's pieces for (count, depth) (cmux_plan.h); inside a piece of `items`
// items the projection runs in runs of at most project_plan(...).groups_per_piece items (project_runs).
#pragma once
#include "cmux_plan.h"
#include "pack_plan.h"

namespace ieache {

// the parameter set the packing unit sees for a projection: the source key is the ring key, N words
inline Params project_params(const Params& p) {
    Params q = p;
    q.n = p.N;
    return q;
}
// Why a decomposition (t, b) is refused for the projection key, or null: pack_set_error on n := N.
inline const char* project_set_error(const Params& p, int32_t t, int32_t b) { return pack_set_error(project_params(p), t, b); }

// Why the window of a call is refused, or null: first in [0, N), width >= 1 with first + width <= N, dest in [0, 2N).
inline const char* project_call_error(const Params& p, int32_t first, int32_t width, int32_t dest) {
    if (first < 0 || first >= p.N) return "tlwe_project: first must lie in [0, N)";
    if (width < 1) return "tlwe_project: width must be at least 1";
    if ((int64_t)first + width > p.N) return "tlwe_project: first + width must not exceed N";
    if (dest < 0 || dest >= 2 * p.N) return "tlwe_project: dest must lie in [0, 2N)";
    return nullptr;
}

// A projection of `items` samples onto windows of `width` coefficients: pack_plan with an item as the group.
inline PackPlan project_plan(const Params& p, int32_t t, int64_t items, int32_t width, int64_t piece_rows_opt, int32_t split_opt, int64_t cus) {
    return pack_plan(project_params(p), t, items, width, piece_rows_opt, split_opt, cus);
}
// runs of the projection inside a piece of `items` items of a replace write whose plan `pl` was made for the largest piece
inline int64_t project_runs(const PackPlan& pl, int64_t items) { return cut_in_runs(items, pl.groups_per_piece).pieces; }

// Why the scalars of a replace write of a window are refused, or null: depth and steps as for lut_add, width >= 1,
// width <= unit, unit 2^steps <= N (so that every word lies inside one sample and the amounts stay below N).  THE statement
// of these rules: the call's row of set_calls.h refuses by it (set_call_refusal).
static_assert(kCmuxMaxDepth == 12 && kRotateMaxSteps == 64, "the messages below spell the limits out");
// Which rule the window of an addressed word breaks, for steps >= 0: 0 none, 1 width < 1, 2 unit < width, 3 unit 2^steps > N.
// The write states its messages below, the read of such a word (word_read, unpack_plan.h) its own under its name.
inline int word_window_rule(int32_t N, int32_t steps, int32_t width, int32_t unit) {
    if (width < 1) return 1;
    if (unit < width) return 2;
    return steps > 30 || ((int64_t)unit << steps) > N ? 3 : 0;
}
inline const char* write_coef_error(int32_t N, int32_t depth, int32_t steps, int32_t width, int32_t unit) {
    if (depth < 0 || depth > kCmuxMaxDepth) return "lut_write_coef: depth must lie in 0 .. 12";
    if (steps < 0 || steps > kRotateMaxSteps) return "lut_write_coef: steps must lie in 0 .. 64";
    switch (word_window_rule(N, steps, width, unit)) {
    case 1: return "lut_write_coef: width must be at least 1";
    case 2: return "lut_write_coef: unit must be at least width";
    case 3: return "lut_write_coef: unit x 2^steps must not exceed N";
    default: return nullptr;
    }
}
// the public amount of step t of the two rotations: the read brings coefficient unit sum b_t 2^t to position 0, the write
// takes position 0 back there.  unit 2^t < N for t < steps by write_coef_error.
inline int32_t write_coef_amount(const Params& p, int32_t unit, int32_t t, bool toward_zero) {
    const int32_t w = (int32_t)(((int64_t)unit << t) & (2 * p.N - 1));
    return toward_zero ? (2 * p.N - w) & (2 * p.N - 1) : w;
}

}  // namespace ieache
