// Linear layers on encrypted rows (include/ieache.h section 3n), the one door: the kernels and the prepared weight fragments are
// behind this object; what a call is and how it is tiled is linear_plan.h.  Kernels: lwe_linear.hip.
#pragma once
#include "device_buffer.h"
#include "linear_plan.h"

namespace ieache {

// One per evaluator.  All methods expect the evaluator's device to be current.
struct LweLinear {
    void init(const Params& p) { p_ = p; }
    // the plan of a call under "linear_kernel" = kernel_opt
    LinearPlan plan(int32_t rows, int32_t n_out, int32_t n_in, int32_t kernel_opt) const { return linear_plan(linear_rows(p_, rows), n_out, n_in, kernel_opt); }
    // One call on `stream`: d_x [batch][n_in] rows and d_out [batch][n_out] rows of the kind's stride, d_w [n_out][n_in] int8,
    // d_bias [n_out] or null.  Every word of d_out up to the stride is written.  The product copies W into the unit's scratch
    // first (grown here when the call needs more: the stream is then idle, every call ends with it so).  Throws
    // std::invalid_argument for a call linear_call_error refuses.
    void launch(hipStream_t stream, const LinearPlan& pl, int32_t rows, size_t batch, int32_t n_out, int32_t n_in, const int8_t* d_w,
                const int32_t* d_bias, const Torus32* d_x, Torus32* d_out);

private:
    Params p_;
    dev::DeviceBuffer<int8_t> frags_;  // W as A fragments of the product, the last call's
};

}  // namespace ieache
