// Multi-output extraction on MI355X (gfx950): see multi_extract.h.
//
// Everything here is arithmetic mod 2^32 on uint32 -- products, sums, the negacyclic sign -- so there is nothing to round and
// the result does not depend on the order in which the terms are added: any schedule gives the same bits.
#include "multi_extract.h"

#include <stdexcept>

namespace ieache {

namespace {

using namespace dev;

constexpr int kMvThreads = 256;
constexpr int32_t kMvMaxN = 1024, kMvMaxN2 = 2048;  // the two builds of k_mv_extract; 2048: Params::supported()

// One workgroup per factor: count and ascending (index, coefficient) list of its nonzero coefficients.  Thread i looks at the
// ceil(N / 256) consecutive coefficients from i x that on; an inclusive scan of the threads' counts places each thread's pairs.
__global__ __launch_bounds__(kMvThreads) void k_mv_compact(const int32_t* __restrict__ factors, int32_t N, int32_t* __restrict__ counts,
                                                           int2* __restrict__ pairs) {
    __shared__ int32_t s_scan[kMvThreads];
    const int tid = threadIdx.x;
    const int32_t* P = factors + (size_t)blockIdx.x * N;
    int2* list = pairs + (size_t)blockIdx.x * N;
    const int32_t per = (N + kMvThreads - 1) / kMvThreads, j0 = tid * per;
    int32_t mine = 0;
    for (int32_t q = 0; q < per; q++) mine += (j0 + q < N && P[j0 + q] != 0) ? 1 : 0;
    s_scan[tid] = mine;
    __syncthreads();
    for (int off = 1; off < kMvThreads; off <<= 1) {
        const int32_t below = tid >= off ? s_scan[tid - off] : 0;
        __syncthreads();
        s_scan[tid] += below;
        __syncthreads();
    }
    int32_t pos = s_scan[tid] - mine;  // <= N - mine: the list holds N pairs
    for (int32_t q = 0; q < per; q++) {
        const int32_t j = j0 + q;
        if (j < N && P[j] != 0) list[pos++] = make_int2(j, P[j]);
    }
    if (tid == kMvThreads - 1) counts[blockIdx.x] = s_scan[tid];
}

// term of coefficient index i in (-N, 2N) of the negacyclic extension of a polynomial in LDS: p[i] for 0 <= i < N, -p[i + N]
// below, -p[i - N] above (i is taken mod 2N, so any int32 i is in range)
__device__ __forceinline__ uint32_t ext_coef(const int32_t* p, int32_t i, int32_t N) {
    const int32_t s = i & (2 * N - 1);
    const uint32_t v = (uint32_t)p[s & (N - 1)];
    return (s & N) ? 0u - v : v;
}

// One workgroup per item.  The item's accumulator (A, B) is read once into LDS; then, for the plain extraction (t = -1: the
// factor 1, no bias, into ext_plain) and for every factor t, one extracted row is formed in extracted order
//     u[j] = -sum_k c_k Aext[N - j - j_k]   (j < N; j = 0 gives +A'[0] through Aext[N] = -A[0])
//     u[N] = sum_k c_k Bext[-j_k] + bias[t]
// over the factor's list (j_k, c_k).  Thread i owns coefficients i, i + 256, ...: for one list entry consecutive threads read
// consecutive LDS words (no bank conflict), and the entry itself is the same for the whole workgroup (a scalar load).  The row
// goes through LDS once more so that it leaves in 16-byte stores.  N < 256: the threads past N hold no coefficient.
// Stated once and built twice, so that the build for rings up to 1024 keeps its code: per thread MAXN / 256 coefficients of a row.
#define MV_EXTRACT_KERNEL(NAME, MAXN) \
__global__ __launch_bounds__(kMvThreads) void NAME(const Torus32* __restrict__ acc, int32_t N, int32_t n_factors,                                         \
                                                           const int32_t* __restrict__ counts, const int2* __restrict__ pairs,                            \
                                                           const Torus32* __restrict__ bias, Torus32* __restrict__ ext_plain,                             \
                                                           Torus32* __restrict__ rows) {                                                                  \
    __shared__ __align__(16) int32_t s_acc[2 * MAXN];  /* A | B */                                                                                        \
    __shared__ __align__(16) int32_t s_row[MAXN + 4];                                                                                                     \
    __shared__ uint32_t s_part[kMvThreads / 64];                                                                                                          \
    const int tid = threadIdx.x;                                                                                                                          \
    const int64_t item = blockIdx.x;                                                                                                                      \
    const int32_t R = (N + 4) >> 2;  /* 16-byte words of a row; word N / 4 holds the b term and the padding */                                            \
    {                                                                                                                                                     \
        const int4* src = reinterpret_cast<const int4*>(acc + (size_t)item * 2 * N);                                                                      \
        for (int32_t v = tid; v < (N >> 1); v += kMvThreads) reinterpret_cast<int4*>(s_acc)[v] = src[v];                                                  \
    }                                                                                                                                                     \
    __syncthreads();                                                                                                                                      \
    const int32_t* A = s_acc;                                                                                                                             \
    const int32_t* B = s_acc + N;                                                                                                                         \
    for (int32_t t = -1; t < n_factors; t++) {                                                                                                            \
        const int32_t len = t < 0 ? 1 : counts[t];                                                                                                        \
        const int2* list = pairs + (size_t)(t < 0 ? 0 : t) * N;                                                                                           \
        uint32_t a[(MAXN / kMvThreads)];                                                                                                                  \
_Pragma("unroll")                                                                                                                                         \
        for (int r = 0; r < (MAXN / kMvThreads); r++) a[r] = 0;                                                                                           \
        for (int32_t k = 0; k < len; k++) {                                                                                                               \
            const int2 e = t < 0 ? make_int2(0, 1) : list[k];                                                                                             \
_Pragma("unroll")                                                                                                                                         \
            for (int r = 0; r < (MAXN / kMvThreads); r++) {                                                                                               \
                const int32_t j = tid + kMvThreads * r;                                                                                                   \
                if (j < N) a[r] += (uint32_t)e.y * ext_coef(A, N - j - e.x, N);                                                                           \
            }                                                                                                                                             \
        }                                                                                                                                                 \
        uint32_t b = 0;                                                                                                                                   \
        for (int32_t k = tid; k < len; k += kMvThreads) {                                                                                                 \
            const int2 e = t < 0 ? make_int2(0, 1) : list[k];                                                                                             \
            b += (uint32_t)e.y * ext_coef(B, -e.x, N);                                                                                                    \
        }                                                                                                                                                 \
        for (int m = 32; m > 0; m >>= 1) b += (uint32_t)__shfl_xor((int)b, m, 64);                                                                        \
        __syncthreads();  /* the previous row has left s_row / s_part */                                                                                  \
_Pragma("unroll")                                                                                                                                         \
        for (int r = 0; r < (MAXN / kMvThreads); r++) {                                                                                                   \
            const int32_t j = tid + kMvThreads * r;                                                                                                       \
            if (j < N) s_row[j] = (int32_t)(0u - a[r]);                                                                                                   \
        }                                                                                                                                                 \
        if ((tid & 63) == 0) s_part[tid >> 6] = b;                                                                                                        \
        __syncthreads();                                                                                                                                  \
        uint32_t bt = (t >= 0 && bias) ? (uint32_t)bias[t] : 0u;                                                                                          \
_Pragma("unroll")                                                                                                                                         \
        for (int w = 0; w < kMvThreads / 64; w++) bt += s_part[w];                                                                                        \
        int4* dst = reinterpret_cast<int4*>(t < 0 ? ext_plain + (size_t)item * (N + 4) : rows + ((size_t)item * n_factors + t) * (N + 4));                \
        for (int32_t v = tid; v < R; v += kMvThreads) dst[v] = v == (N >> 2) ? make_int4((int32_t)bt, 0, 0, 0) : reinterpret_cast<const int4*>(s_row)[v]; \
    }                                                                                                                                                     \
}
MV_EXTRACT_KERNEL(k_mv_extract, kMvMaxN)            // N <= 1024
MV_EXTRACT_KERNEL(k_mv_extract_2048, kMvMaxN2)      // N = 2048: twice the LDS and the registers
#undef MV_EXTRACT_KERNEL

}  // namespace

void MultiExtract::init(const Params& p) {
    if (p.N > kMvMaxN2 || (p.N & 3)) throw std::invalid_argument("multi-output extraction: ring degree outside 4 .. 2048");
    N_ = p.N;
}

void MultiExtract::reserve(MvScratch& scratch, size_t items, size_t rows, size_t cap_items, size_t cap_rows) {
    scratch.acc.reserve(items, cap_items, (size_t)2 * N_ * 4);
    if (rows) scratch.rows.reserve(rows, cap_rows, (size_t)(N_ + 4) * 4);
}

void MultiExtract::compact(hipStream_t stream, const int32_t* d_factors, int32_t n_factors) {
    if (n_factors < 1 || n_factors > kMultiMaxFactors || !d_factors) throw std::invalid_argument("multi-output extraction: 1 .. 64 factors");
    if (!counts_) counts_.allocate(kMultiMaxFactors);
    if (!pairs_) pairs_.allocate((size_t)kMultiMaxFactors * N_);
    hipLaunchKernelGGL(k_mv_compact, dim3((unsigned)n_factors), dim3(kMvThreads), 0, stream, d_factors, N_, counts_, pairs_);
    HIP_CHECK(hipGetLastError());
}

void MultiExtract::extract(hipStream_t stream, const Torus32* acc, int64_t cnt, int32_t n_factors, const Torus32* d_bias, Torus32* ext_plain,
                           Torus32* rows) {
    if (n_factors < 1 || n_factors > kMultiMaxFactors || !counts_ || !pairs_) throw std::logic_error("multi-output extraction before its factor lists");
    if (cnt < 1) return;
    hipLaunchKernelGGL(N_ > kMvMaxN ? k_mv_extract_2048 : k_mv_extract, dim3((unsigned)cnt), dim3(kMvThreads), 0, stream, acc, N_, n_factors, counts_,
                       pairs_, d_bias, ext_plain, rows);
    HIP_CHECK(hipGetLastError());
}

}  // namespace ieache
