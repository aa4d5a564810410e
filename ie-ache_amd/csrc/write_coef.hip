// The small passes of the replace write of a window (write_coef.h).  Plain integer kernels: a word is read and written by one
// thread, nothing is shared.
#include "write_coef.h"

#include <hip/hip_runtime.h>

namespace ieache {

namespace {

__global__ __launch_bounds__(256) void k_write_coef_tables(int32_t unit, int32_t steps, int32_t two_n, int64_t count, int32_t* __restrict__ toward,
                                                           int32_t* __restrict__ back, int32_t* __restrict__ own) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q < steps) {
        const int32_t w = (int32_t)(((int64_t)unit << q) & (two_n - 1));  // steps <= 30 (write_coef_error)
        back[q] = w;
        toward[q] = (two_n - w) & (two_n - 1);
    }
    if (q < count) own[q] = (int32_t)q;
}

__global__ __launch_bounds__(256) void k_write_coef_indices(const int32_t* __restrict__ sel_of, int64_t item0, int64_t items, int32_t depth,
                                                            int32_t steps, int32_t n_set, int32_t* __restrict__ tree_sel) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= items * depth) return;
    const int64_t item = q / depth, k = q - item * depth;
    const int64_t at = (item0 + item) * (depth + steps) + steps + k;
    int64_t sel;
    if (sel_of == nullptr) {
        sel = at % n_set;
    } else {
        sel = (int64_t)sel_of[at];
        sel = sel < 0 ? 0 : (sel >= n_set ? n_set - 1 : sel);
    }
    tree_sel[q] = (int32_t)sel;
}

__global__ __launch_bounds__(256) void k_write_coef_delta(const int32_t* __restrict__ fresh, int32_t* old_to_delta, int32_t words) {
    const size_t at = (size_t)blockIdx.x * words;
    for (int32_t q = threadIdx.x; q < words; q += 256) old_to_delta[at + q] = (int32_t)((uint32_t)fresh[at + q] - (uint32_t)old_to_delta[at + q]);
}

}  // namespace

void launch_write_coef_tables(hipStream_t stream, int32_t unit, int32_t steps, int32_t two_n, int64_t count, int32_t* toward, int32_t* back,
                              int32_t* own) {
    const int64_t n = count > steps ? count : steps;
    if (n <= 0) return;
    hipLaunchKernelGGL(k_write_coef_tables, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, unit, steps, two_n, count, toward, back, own);
}

void launch_write_coef_indices(hipStream_t stream, const int32_t* sel_of, int64_t item0, int64_t items, int32_t depth, int32_t steps, int32_t n_set,
                               int32_t* tree_sel) {
    const int64_t words = items * depth;
    if (words <= 0) return;
    hipLaunchKernelGGL(k_write_coef_indices, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, sel_of, item0, items, depth, steps, n_set,
                       tree_sel);
}

void launch_write_coef_delta(hipStream_t stream, int64_t items, int32_t N, const int32_t* fresh, int32_t* old_to_delta) {
    if (items <= 0) return;
    hipLaunchKernelGGL(k_write_coef_delta, dim3((unsigned)items), dim3(256), 0, stream, fresh, old_to_delta, 2 * N);
}

}  // namespace ieache
