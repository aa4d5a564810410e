// Packing key switch: LWE rows into one TLWE sample, as an int8 matrix product on the MFMA pipe (include/ieache.h section 3e,
// DESIGN.md section 4.5).
//
//   R_r   = (0, b_r X^0) - sum_{i < n} sum_{j < t} d_{r,i,j} PK[i][j]              (scalar x [2][N], mod 2^32)
//   out_g = sum_{p < m} sum_{q < w} X^(p w + q + shift) R_{g m + p}                (negacyclic, mod 2^32)
//
// The first line is the sibling of keyswitch_mfma.hip's product, with the digit as a VALUE instead of a one-hot row choice:
//
//   C[r][c] = sum_k A[r][k] * B[k][c],   k = (i, j) flattened,  A[r][k] = d_{r,i,j}  (int8, 0 .. 2^b - 1)
//                                                               B[k][(c, limb)] = byte `limb` of PK[i][j][c]  (int8)
//
// with the key words cut into four BALANCED byte limbs (v = b0 + 2^8 b1 + 2^16 b2 + 2^24 b3 mod 2^32, each in [-128, 127]).
// A limb column accumulates n t products of magnitude <= (2^b - 1) 128, below 2^31 for every accepted set (pack_set_error), so
// the MFMA's int32 accumulators are exact and R = (0, b) - sum_limb (C_limb << 8 limb) mod 2^32 is the integer definition
// whatever the order of summation: no rounding, nothing to guard or audit.  There is no table in LDS and one kernel for every
// (t, b): the digit pre-pass writes values.
//
// A wave owns four 32-row tiles x 32 columns x 4 limbs = 16 accumulator tiles and walks its share of the K steps alone.  Per
// step it reads 4 KiB of B, stored at key load in the operand order of the instruction (one coalesced 1 KiB
// global_load_dwordx4 per limb), and one 1 KiB row of digits per tile: [K step][row][32] bytes, so the 32 rows of a tile are
// contiguous.  Which lane / byte of an operand register is "k" does not matter as long as A and B agree: both use
// k = 32 step + 16 (lane / 32) + byte.  K splits meet in R through integer atomic adds, order-free mod 2^32.
// The second line is k_pack_place: 32 output words per workgroup, the m w reads of R of each cut over eight threads; it writes
// every word of out.
// The projection of section 3l is the same product and placement on the parameter set with n := N: its rows are the extracted
// rows of a window of a TLWE sample, which k_window_digits turns into digits without storing them (Pack::launch_window).
#include "pack.h"

#include <hip/hip_runtime.h>

#include <stdexcept>

namespace ieache {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// ---- key preparation: PK [K][2N] int32 -> B fragments [K step][column block][4 limbs][64 lanes][16 bytes]; k >= K: zero rows ----
__global__ __launch_bounds__(256) void k_pack_prepare(const int32_t* __restrict__ pk, int8_t* __restrict__ limbs, int64_t K, int32_t cols,
                                                      int32_t ncb) {
    const int32_t s = blockIdx.x, cb = blockIdx.y;
    int8_t* dst = limbs + ((size_t)s * ncb + cb) * 4096;
    for (int idx = threadIdx.x; idx < 1024; idx += 256) {  // (lane, byte) of one fragment; the four limbs of a key word together
        const int lane = idx >> 4, e = idx & 15;
        const int32_t c = cb * 32 + (lane & 31);           // < cols: cols = 32 ncb
        const int64_t k = (int64_t)s * kPackKStep + 16 * (lane >> 5) + e;
        int64_t r = k < K ? (int64_t)pk[(size_t)k * cols + c] : 0;
#pragma unroll
        for (int limb = 0; limb < 4; limb++) {
            const int8_t b = (int8_t)(r & 0xFF);  // balanced: the remainder in [-128, 127]
            dst[limb * 1024 + idx] = b;
            r = (r - b) >> 8;                     // exact division
        }
    }
}

// ---- per piece: digits d_{r,i,j} of abar = a_i + 2^(31 - t b) as bytes, [K step][padded row][32]; rows past the piece and
// k >= n t are zero.  One workgroup per padded row, a thread per dword of four digits. ----
__global__ __launch_bounds__(256) void k_pack_digits(const Torus32* __restrict__ rows, uint32_t* __restrict__ dig, int64_t nrows, int64_t rpad,
                                                     int32_t stride, int32_t K, int32_t t, int32_t basebit, int32_t k_steps) {
    const int64_t r = (int64_t)blockIdx.x;
    const Torus32* a = rows + (size_t)r * stride;
    const uint32_t prec = 1u << (31 - t * basebit), mask = (1u << basebit) - 1u;
    for (int32_t q = threadIdx.x; q < k_steps * 8; q += 256) {
        uint32_t v = 0;
        if (r < nrows) {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int32_t k = 4 * q + e;
                if (k < K) {
                    const int32_t i = k / t, j = k - i * t;
                    v |= ((((uint32_t)a[i] + prec) >> (32 - (j + 1) * basebit)) & mask) << (8 * e);
                }
            }
        }
        dig[((size_t)(q >> 3) * rpad + r) * 8 + (q & 7)] = v;
    }
}

// ---- per piece: R rows start as (0, b X^0) ----
__global__ __launch_bounds__(256) void k_pack_init(const Torus32* __restrict__ rows, uint32_t* __restrict__ R, int32_t stride, int32_t n, int32_t N) {
    const int64_t r = (int64_t)blockIdx.x;
    const uint32_t b = (uint32_t)rows[(size_t)r * stride + n];
    uint32_t* dst = R + (size_t)r * 2 * N;
    for (int32_t q = threadIdx.x; q < 2 * N; q += 256) dst[q] = q == N ? b : 0u;
}

// ---- per piece of a projection (include/ieache.h section 3l; project_plan.h): what k_pack_digits and k_pack_init do, for rows that
// are never stored.  Row r of the piece is coefficient c = first + r % width of sample r / width, whose extracted row is
// u[i] = A[c - i] for i <= c and -A[N + c - i] above (k_tlwe_extract's rule), u[N] = B[c]: the digits of abar = u[i] + 2^(31 - t b)
// -- of the NEGATED word where the rule negates, not the negated digits -- go straight into the product's A layout, and
// R_r = (0, B[c] X^0).  A workgroup owns 32 consecutive padded rows and (blockIdx.y) a share of the K steps; thread (row, w)
// writes dword w of each of those steps of its row, so a step's store is 1 KiB contiguous.  The rows of a sample read it through the caches: it comes from memory once.  Rows past
// the piece and k >= N t get zero digits. ----
constexpr int kWindowRows = 32, kWindowStepParts = 16;
__global__ __launch_bounds__(kWindowRows * 8) void k_window_digits(const Torus32* __restrict__ tlwe, uint32_t* __restrict__ dig, uint32_t* __restrict__ R,
                                                                   int64_t nrows, int64_t rpad, int32_t N, int32_t first, int32_t width, int32_t t,
                                                                   int32_t basebit, int32_t k_steps) {
    const int64_t r0 = (int64_t)blockIdx.x * kWindowRows;  // < rpad by the grid: rpad is a whole number of blocks of 128 rows
    const int32_t rr = threadIdx.x >> 3, w = threadIdx.x & 7;
    const int64_t r = r0 + rr;
    const bool live = r < nrows;
    const int64_t item = live ? r / width : 0;
    const int32_t c = first + (live ? (int32_t)(r - item * width) : 0);  // < N: first + width <= N
    const uint32_t* A = reinterpret_cast<const uint32_t*>(tlwe) + (size_t)item * 2 * N;
    const uint32_t prec = 1u << (31 - t * basebit), mask = (1u << basebit) - 1u;
    const int32_t K = N * t;  // < 2^15: t < 32, N <= 1024
    // blockIdx.y takes its share of the K steps (consecutive, together every step once: gridDim.y <= k_steps), so that a thread's
    // chain of dependent loads stays short: 256 steps in one thread made a piece of 32 rows latency-bound
    const int32_t s0 = (int32_t)(k_steps * blockIdx.y / gridDim.y), s1 = (int32_t)(k_steps * (blockIdx.y + 1) / gridDim.y);
    for (int32_t s = s0; s < s1; s++) {
        uint32_t v = 0;
        if (live) {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int32_t k = s * kPackKStep + 4 * w + e;
                if (k < K) {
                    const int32_t i = k / t, j = k - i * t;                        // i < N
                    const uint32_t u = i <= c ? A[c - i] : 0u - A[N + c - i];      // indices in [0, N) either way
                    v |= (((u + prec) >> (32 - (j + 1) * basebit)) & mask) << (8 * e);
                }
            }
        }
        dig[((size_t)s * rpad + r) * 8 + w] = v;
    }
    if (blockIdx.y != 0) return;  // R is written once per row
    for (int32_t q = 0; q < kWindowRows; q++) {
        const int64_t row = r0 + q;
        if (row >= nrows) break;
        const int64_t it = row / width;
        const uint32_t b = reinterpret_cast<const uint32_t*>(tlwe)[(size_t)it * 2 * N + N + first + (int32_t)(row - it * width)];
        uint32_t* dst = R + (size_t)row * 2 * N;
        for (int32_t x = threadIdx.x; x < 2 * N; x += kWindowRows * 8) dst[x] = x == N ? b : 0u;
    }
}

// ---- the product.  grid: one wave per (column block, K split, block of 128 rows), streams fastest as in k_ksm_gemm ----
__global__ __launch_bounds__(64) void k_pack_gemm(const v4i* __restrict__ limbs, const v4i* __restrict__ dig, uint32_t* __restrict__ R, int64_t nrows,
                                                  int64_t rpad, int32_t k_steps, int32_t ncb, int32_t ksplit, int32_t cols) {
    const int lane = threadIdx.x;
    const int32_t streams = ncb * ksplit;
    const int32_t st = blockIdx.x % streams;
    const int64_t row0 = (int64_t)(blockIdx.x / streams) * kPackBlockRows;
    const int32_t cb = st % ncb, ks = st / ncb;
    // pack_split_first (pack_plan.h, host code) spelled out
    const int32_t s0 = (int32_t)((int64_t)k_steps * ks / ksplit), s1 = (int32_t)((int64_t)k_steps * (ks + 1) / ksplit);
    const int m = lane & 31, grp = lane >> 5;

    v16i acc[kPackWaveTiles][4];
#pragma unroll
    for (int t = 0; t < kPackWaveTiles; t++)
#pragma unroll
        for (int l = 0; l < 4; l++)
#pragma unroll
            for (int v = 0; v < 16; v++) acc[t][l][v] = 0;

    // a row of digits is two 16-byte words; tile t of the block starts 64 words on (rpad is a whole number of blocks)
    const v4i* ap = dig + ((size_t)row0 + m) * 2 + grp;
    const v4i* bp = limbs + (size_t)cb * 256 + lane;
    const size_t a_step = (size_t)rpad * 2, b_step = (size_t)ncb * 256;
    v4i a[kPackWaveTiles], b[4], an[kPackWaveTiles], bn[4];
#pragma unroll
    for (int t = 0; t < kPackWaveTiles; t++) an[t] = ap[(size_t)s0 * a_step + t * 64];
#pragma unroll
    for (int l = 0; l < 4; l++) bn[l] = bp[(size_t)s0 * b_step + l * 64];
#pragma unroll 1
    for (int32_t s = s0; s < s1; s++) {
#pragma unroll
        for (int t = 0; t < kPackWaveTiles; t++) a[t] = an[t];
#pragma unroll
        for (int l = 0; l < 4; l++) b[l] = bn[l];
        if (s + 1 < s1) {  // the next step's operands are requested before this step's products are issued
#pragma unroll
            for (int t = 0; t < kPackWaveTiles; t++) an[t] = ap[(size_t)(s + 1) * a_step + t * 64];
#pragma unroll
            for (int l = 0; l < 4; l++) bn[l] = bp[(size_t)(s + 1) * b_step + l * 64];
        }
#pragma unroll
        for (int t = 0; t < kPackWaveTiles; t++)
#pragma unroll
            for (int l = 0; l < 4; l++) acc[t][l] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[t], b[l], acc[t][l], 0, 0, 0);
    }
    // epilogue: D[row][col] of a 32x32 tile sits in register v of lane: col = lane % 32, row = 8 (v / 4) + 4 (lane / 32) + v % 4
    const int32_t col = cb * 32 + m;  // < cols
#pragma unroll
    for (int t = 0; t < kPackWaveTiles; t++) {
#pragma unroll
        for (int v = 0; v < 16; v++) {
            const int64_t r = row0 + t * 32 + 8 * (v >> 2) + 4 * grp + (v & 3);
            if (r < nrows) {
                const uint32_t sum = (uint32_t)acc[t][0][v] + ((uint32_t)acc[t][1][v] << 8) + ((uint32_t)acc[t][2][v] << 16) + ((uint32_t)acc[t][3][v] << 24);
                // atomic adds without a return even where no K split shares the word: a plain read-modify-write waits for its
                // load and measured slower
                if (sum) atomicAdd(R + (size_t)r * cols + col, 0u - sum);
            }
        }
    }
}

// ---- placement: word (c, x) of out_g = sum over the group's m w pairs u = p w + q of coefficient x of X^(u + shift) R_{g m + p}[c];
// coefficient x of X^a P is P[x - a] for 0 <= x - a < N mod 2N and -P[x - a - N] otherwise.  A workgroup owns 32 output words
// (2N is a whole number of them); eight threads per word take an eighth of the pairs each -- a single group of 1 024 rows would
// otherwise be 2 048 threads of 1 024 dependent-latency loads -- and meet in LDS.  Every word of out is written. ----
constexpr int kPlaceWords = 32, kPlaceParts = 8;
__global__ __launch_bounds__(kPlaceWords * kPlaceParts) void k_pack_place(const uint32_t* __restrict__ R, uint32_t* __restrict__ out, int32_t N,
                                                                          int32_t m, int32_t spread, int32_t shift) {
    __shared__ uint32_t sums[kPlaceParts][kPlaceWords];
    const int xl = threadIdx.x & (kPlaceWords - 1), part = threadIdx.x / kPlaceWords;
    const int32_t idx = blockIdx.x * kPlaceWords + xl;  // < 2N by the grid
    const int64_t g = (int64_t)blockIdx.y;
    const int32_t c = idx >= N ? 1 : 0, x = idx & (N - 1);
    const uint32_t* base = R + ((size_t)g * m * 2 + c) * N;
    const int32_t pairs = m * spread;  // <= N
    int32_t u = (int32_t)((int64_t)pairs * part / kPlaceParts);
    const int32_t u1 = (int32_t)((int64_t)pairs * (part + 1) / kPlaceParts);
    int32_t p = u / spread, q = u - p * spread;
    uint32_t acc = 0;
    for (; u < u1; u++) {
        const int32_t j = (x - u - shift) & (2 * N - 1);  // two's complement: the residue mod 2N of a negative difference too
        const uint32_t v = base[(size_t)p * 2 * N + (j & (N - 1))];
        acc += (j & N) ? 0u - v : v;
        if (++q == spread) {
            q = 0;
            p++;
        }
    }
    sums[part][xl] = acc;
    __syncthreads();
    if (part == 0) {
#pragma unroll
        for (int k = 1; k < kPlaceParts; k++) acc += sums[k][xl];
        out[(size_t)g * 2 * N + idx] = acc;
    }
}

}  // namespace

void Pack::set_key(int32_t t, int32_t basebit, const int32_t* pk, hipStream_t stream) {
    if (!pk) {
        limbs_.reset();
        t_ = basebit_ = 0;
        return;
    }
    if (const char* e = pack_set_error(p_, t, basebit)) throw std::invalid_argument(e);
    const int64_t K = pack_k(p_, t);
    const int32_t cols = 2 * p_.N, ncb = pack_col_blocks(p_), k_steps = pack_k_steps(p_, t);
    dev::DeviceBuffer<int32_t> words;  // the int32 key: scratch of this call
    words.allocate((size_t)K * cols);
    HIP_CHECK(hipMemcpy(words, pk, (size_t)K * cols * 4, hipMemcpyHostToDevice));
    std::unique_ptr<dev::DeviceBuffer<int8_t>> limbs(new dev::DeviceBuffer<int8_t>);
    limbs->allocate(pack_limb_bytes(p_, t));
    hipLaunchKernelGGL(k_pack_prepare, dim3((unsigned)k_steps, (unsigned)ncb), dim3(256), 0, stream, (const int32_t*)words, (int8_t*)*limbs, K,
                       cols, ncb);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(stream));
    limbs_ = std::move(limbs);  // the first key goes here
    t_ = t;
    basebit_ = basebit;
}

void Pack::reserve(PackScratch& scratch, const PackPlan& pl) {
    scratch.r.reserve_exact(pl.r_bytes);
    scratch.digits.reserve_exact(pl.digit_bytes);
}

void Pack::launch(PackScratch& scratch, hipStream_t stream, const PackPlan& pl, int64_t groups, int32_t m, int32_t spread, int32_t shift,
                  const Torus32* rows, int32_t stride, Torus32* out) {
    if (!limbs_) throw std::invalid_argument("pack: no packing key set");
    const int64_t nrows = groups * m, rpad = pack_padded_rows(nrows);
    if (nrows <= 0) return;
    if (!pack_split_ok(pl.k_steps, pl.ksplit) || pl.k_steps != pack_k_steps(p_, t_)) throw std::invalid_argument("pack: plan of another key");
    if ((size_t)nrows * 2 * (size_t)p_.N * 4 > scratch.r.items() || (size_t)pl.k_steps * (size_t)rpad * kPackKStep > scratch.digits.items())
        throw std::invalid_argument("pack: piece larger than the reserved scratch");
    const int32_t N = p_.N, ncb = pack_col_blocks(p_);
    const int64_t row_blocks = rpad / kPackBlockRows;
    uint32_t* R = reinterpret_cast<uint32_t*>((char*)scratch.r);
    uint32_t* dig = reinterpret_cast<uint32_t*>((char*)scratch.digits);
    hipLaunchKernelGGL(k_pack_digits, dim3((unsigned)rpad), dim3(256), 0, stream, rows, dig, nrows, rpad, stride, (int32_t)pack_k(p_, t_), t_,
                       basebit_, pl.k_steps);
    hipLaunchKernelGGL(k_pack_init, dim3((unsigned)nrows), dim3(256), 0, stream, rows, R, stride, p_.n, N);
    hipLaunchKernelGGL(k_pack_gemm, dim3((unsigned)(row_blocks * ncb * pl.ksplit)), dim3(64), 0, stream,
                       reinterpret_cast<const v4i*>((const int8_t*)*limbs_), reinterpret_cast<const v4i*>(dig), R, nrows, rpad, pl.k_steps, ncb,
                       pl.ksplit, 2 * N);
    hipLaunchKernelGGL(k_pack_place, dim3((unsigned)(2 * N / kPlaceWords), (unsigned)groups), dim3(kPlaceWords * kPlaceParts), 0, stream, R,
                       reinterpret_cast<uint32_t*>(out), N, m, spread, shift);
}

void Pack::launch_window(PackScratch& scratch, hipStream_t stream, const PackPlan& pl, int64_t items, int32_t first, int32_t width, int32_t dest,
                         const Torus32* tlwe, Torus32* out) {
    if (!limbs_) throw std::invalid_argument("tlwe_project: no projection key set");
    if (p_.n != p_.N) throw std::logic_error("tlwe_project: the unit was not initialised on the n := N parameter set");
    if (const char* e = project_call_error(p_, first, width, dest)) throw std::invalid_argument(e);
    const int64_t nrows = items * width, rpad = pack_padded_rows(nrows);
    if (nrows <= 0) return;
    if (!pack_split_ok(pl.k_steps, pl.ksplit) || pl.k_steps != pack_k_steps(p_, t_)) throw std::invalid_argument("tlwe_project: plan of another key");
    if ((size_t)nrows * 2 * (size_t)p_.N * 4 > scratch.r.items() || (size_t)pl.k_steps * (size_t)rpad * kPackKStep > scratch.digits.items())
        throw std::invalid_argument("tlwe_project: piece larger than the reserved scratch");
    const int32_t N = p_.N, ncb = pack_col_blocks(p_);
    const int64_t row_blocks = rpad / kPackBlockRows;
    uint32_t* R = reinterpret_cast<uint32_t*>((char*)scratch.r);
    uint32_t* dig = reinterpret_cast<uint32_t*>((char*)scratch.digits);
    const int32_t step_parts = pl.k_steps < kWindowStepParts ? pl.k_steps : kWindowStepParts;
    hipLaunchKernelGGL(k_window_digits, dim3((unsigned)(rpad / kWindowRows), (unsigned)step_parts), dim3(kWindowRows * 8), 0, stream, tlwe, dig, R, nrows,
                       rpad, N, first, width, t_, basebit_, pl.k_steps);
    hipLaunchKernelGGL(k_pack_gemm, dim3((unsigned)(row_blocks * ncb * pl.ksplit)), dim3(64), 0, stream,
                       reinterpret_cast<const v4i*>((const int8_t*)*limbs_), reinterpret_cast<const v4i*>(dig), R, nrows, rpad, pl.k_steps, ncb,
                       pl.ksplit, 2 * N);
    hipLaunchKernelGGL(k_pack_place, dim3((unsigned)(2 * N / kPlaceWords), (unsigned)items), dim3(kPlaceWords * kPlaceParts), 0, stream, R,
                       reinterpret_cast<uint32_t*>(out), N, width, 1, dest);
}

}  // namespace ieache
