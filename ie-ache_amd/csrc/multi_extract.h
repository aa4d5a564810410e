// Multi-output extraction, the one door: the stage between a blind rotation that leaves its whole accumulators and the key
// switch of a multi-output programmable bootstrap (Carpov, Izabachene, Mollimard, CT-RSA 2019).  For every item (A, B) and
// every factor polynomial P_t it forms the extracted sample of coefficient 0 of (P_t A, P_t B), negacyclic and mod 2^32, plus
// bias[t] on the b term -- one row of N + 4 words per (item, factor), item-major -- and the plain extraction of (A, B) for
// the sampled audit of the rotation.  Kernels: multi_extract.hip.  include/ieache.h states the convention.
#pragma once
#include "device_buffer.h"
#include "device_common.h"

namespace ieache {

constexpr int32_t kMultiMaxFactors = 64;  // IEACHE_PBS_MULTI_MAX_FACTORS

// Per-stream scratch: the accumulators a piece's blind rotation leaves, [items][2][N], and the rows of its extracted samples,
// [items x factors][N + 4] (not used where the caller's rows take them directly).
struct MvScratch {
    dev::DeviceBuffer<Torus32> acc;
    dev::DeviceBuffer<Torus32> rows;
};

// One per evaluator.  All methods expect the evaluator's device to be current.
struct MultiExtract {
    void init(const Params& p);
    // Room for a piece of `items` accumulators and `rows` extracted samples ahead of time (an allocation is a device-wide
    // synchronisation); cap: the most items / rows a piece is expected to take.
    void reserve(MvScratch& scratch, size_t items, size_t rows, size_t cap_items, size_t cap_rows);
    // Once per call, on `stream`, before any extract(): the factors [n_factors][N] (device) become, per factor, the count
    // and the ascending list of (index, coefficient) pairs of its nonzero coefficients.  The host never reads the factors.
    // The lists belong to the evaluator, not to a lane: every stream that extracts is ordered after this one.
    void compact(hipStream_t stream, const int32_t* d_factors, int32_t n_factors);
    // acc [cnt][2][N] -> ext_plain [cnt] rows (the plain extraction: what a blind rotation with `ext` would have written) and
    // rows [cnt x n_factors], rows of N + 4 words, all of them written (the three padding words as zero).
    // d_bias: [n_factors] on the device or null.
    void extract(hipStream_t stream, const Torus32* acc, int64_t cnt, int32_t n_factors, const Torus32* d_bias, Torus32* ext_plain,
                 Torus32* rows);

private:
    int32_t N_ = 0;
    dev::DeviceBuffer<int32_t> counts_;  // [kMultiMaxFactors]
    dev::DeviceBuffer<int2> pairs_;      // [kMultiMaxFactors][N]: a dense factor is legal
};

}  // namespace ieache
