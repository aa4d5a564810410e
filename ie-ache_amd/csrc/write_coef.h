// The small passes of the replace write of a window (lut_write_coef; include/ieache.h section 3l, project_plan.h): none of
// them is a step of the definition, each prepares or joins two.  Kernels: write_coef.hip.  The evaluator's device is current.
#pragma once
#include <cstdint>

#include "device_buffer.h"

namespace ieache {

// Once per call: the public amounts of the two rotations, toward [steps] = 2N - unit 2^t (the read) and back [steps] =
// unit 2^t (the write), and own [count] = 0, 1, .. -- item i writes memory i.
void launch_write_coef_tables(hipStream_t stream, int32_t unit, int32_t steps, int32_t two_n, int64_t count, int32_t* toward, int32_t* back,
                              int32_t* own);
// Per piece: selectors steps .. steps + depth - 1 of items item0 .. item0 + items - 1 as explicit indices tree_sel
// [items][depth] -- the rule of every call on a set: an implied selector is its position mod n_set, an explicit one is clamped.
void launch_write_coef_indices(hipStream_t stream, const int32_t* sel_of, int64_t item0, int64_t items, int32_t depth, int32_t steps, int32_t n_set,
                               int32_t* tree_sel);
// Per piece: delta_i = fresh_i - old_i mod 2^32 on all 2N words, in place over old [items][2][N].
void launch_write_coef_delta(hipStream_t stream, int64_t items, int32_t N, const int32_t* fresh, int32_t* old_to_delta);

}  // namespace ieache
