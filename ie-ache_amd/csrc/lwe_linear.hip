// Linear layers on encrypted rows: a public int8 matrix times LWE rows (include/ieache.h section 3n).
//
//   out[b][i][w] = sum_{j < n_in} W[i][j] x[b][j][w]  +  [w == bias word] bias[i]      (mod 2^32)
//
// k_linear_simple is the definition with a thread per output word.  k_linear_mfma is the same sum as an exact product on the
// int8 MFMA pipe, the sibling of k_pack_gemm (pack_keyswitch.hip) with the limb split on the DATA side instead of the key side:
//
//   C_limb[i][w] = sum_j A[i][j] * B_limb[j][w],     A[i][j] = W[i][j]  (int8),   B_limb[j][w] = balanced byte `limb` of x[b][j][w]
//
// A word v is cut in registers: u = (v + 0x80808080) ^ 0x80808080 has bytes that, read as signed, are limbs b_k in [-128, 127]
// with v = sum_k b_k 2^(8k) mod 2^32 (adding 0x80 to every byte and flipping its top bit is subtracting 128 from the unsigned
// byte; the carries of the addition are the borrows of the balanced form -- the offset trick of the gadget decomposition).  A
// limb column accumulates n_in products of magnitude <= 2^14, at most 2^30 for n_in <= 65 536 (linear_plan.h), so the int32
// accumulators are exact and out = sum_limb (C_limb << 8 limb) + bias mod 2^32 is the definition whatever the order of
// summation: nothing is rounded, nothing to guard or audit.
//
// A wave owns 32 consecutive words of one batch element and T output tiles of 32: 4 limbs x T accumulator tiles, four MFMAs per
// tile and K step of 32 inputs.  Per step a lane reads the word of its column from sixteen consecutive input rows (a half-wave's
// loads of one row are 128 contiguous bytes), gathers byte k of the sixteen into limb k's 16-byte fragment with byte permutes,
// and reads one aligned 16-byte A fragment per tile from the weights k_linear_prepare laid out in operand order, zero beyond
// n_out and n_in.  Rows j >= n_in are read clamped: the data is valid and the weight is zero.  Operand and C/D lane maps are
// k_pack_gemm's: k = 32 step + 16 (lane / 32) + byte on both operands; D[row][col] in register v of lane: col = lane % 32,
// row = 8 (v / 4) + 4 (lane / 32) + v % 4 -- the column is the lane, so a register of a half-wave stores 32 consecutive words of
// one output row.
#include "lwe_linear.h"

#include <hip/hip_runtime.h>

#include <stdexcept>

namespace ieache {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// ---- the definition: a thread per word of out (w fastest, so a row's loads and stores are coalesced); the padding as zero ----
__global__ __launch_bounds__(256) void k_linear_simple(const int8_t* __restrict__ W, const uint32_t* __restrict__ x, const int32_t* __restrict__ bias,
                                                       uint32_t* __restrict__ out, int64_t total, int32_t n_out, int32_t n_in, int32_t words,
                                                       int32_t stride, int32_t bias_word) {
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {  // total = batch n_out stride
        const int64_t row = idx / stride;
        const int32_t w = (int32_t)(idx - row * stride);
        const int64_t b = row / n_out;
        const int32_t i = (int32_t)(row - b * n_out);
        uint32_t acc = 0;
        if (w < words) {
            const uint32_t* xp = x + (size_t)b * n_in * stride + w;
            const int8_t* wp = W + (size_t)i * n_in;
            for (int32_t j = 0; j < n_in; j++) acc += (uint32_t)(int32_t)wp[j] * xp[(size_t)j * stride];  // wrap-around is the definition
            if (bias && w == bias_word) acc += (uint32_t)bias[i];
        }
        out[idx] = acc;
    }
}

// ---- W [n_out][n_in] int8 -> A fragments [padded tile][K step][64 lanes][16 bytes]: byte e of lane (m, grp) is
// W[32 tile + m][32 step + 16 grp + e], zero outside the matrix.  A thread per dword of one fragment set. ----
__global__ __launch_bounds__(256) void k_linear_prepare(const int8_t* __restrict__ W, uint32_t* __restrict__ frags, int32_t n_out, int32_t n_in,
                                                        int32_t k_steps) {
    const int32_t s = blockIdx.x, tile = blockIdx.y;
    const int lane = threadIdx.x >> 2, q = threadIdx.x & 3;
    const int32_t i = tile * kLinearTile + (lane & 31);
    uint32_t v = 0;
    if (i < n_out) {
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int32_t j = s * kLinearTile + 16 * (lane >> 5) + 4 * q + e;
            if (j < n_in) v |= (uint32_t)(uint8_t)W[(size_t)i * n_in + j] << (8 * e);
        }
    }
    frags[((size_t)tile * k_steps + s) * 256 + threadIdx.x] = v;
}

// byte k of four words as one dword, k = 0 .. 3: the 4 x 4 byte transpose in eight permutes (v_perm_b32: selector values 0 .. 3
// name the bytes of the SECOND operand, 4 .. 7 those of the first)
__device__ __forceinline__ void limb_dwords(uint32_t u0, uint32_t u1, uint32_t u2, uint32_t u3, uint32_t d[4]) {
    const uint32_t p01 = __builtin_amdgcn_perm(u1, u0, 0x05010400u);  // u0.b0 u1.b0 u0.b1 u1.b1
    const uint32_t p23 = __builtin_amdgcn_perm(u3, u2, 0x05010400u);
    const uint32_t q01 = __builtin_amdgcn_perm(u1, u0, 0x07030602u);  // u0.b2 u1.b2 u0.b3 u1.b3
    const uint32_t q23 = __builtin_amdgcn_perm(u3, u2, 0x07030602u);
    d[0] = __builtin_amdgcn_perm(p23, p01, 0x05040100u);
    d[1] = __builtin_amdgcn_perm(p23, p01, 0x07060302u);
    d[2] = __builtin_amdgcn_perm(q23, q01, 0x05040100u);
    d[3] = __builtin_amdgcn_perm(q23, q01, 0x07060302u);
}

// ---- the product.  grid: x = batch x column blocks, y = groups of T output tiles; one wave each.  The kernel streams x, so
// the builds with fewer accumulators are held to the registers that keep more waves on a SIMD: 4 / T of them ----
template <int T>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4 / T, 4 / T))) void k_linear_mfma(const v4i* __restrict__ frags, const uint32_t* __restrict__ x, const int32_t* __restrict__ bias,
                                                    uint32_t* __restrict__ out, int32_t n_out, int32_t n_in, int32_t words, int32_t stride,
                                                    int32_t bias_word, int32_t ncb, int32_t k_steps) {
    const int lane = threadIdx.x;
    const int c = lane & 31, grp = lane >> 5;
    const int64_t b = blockIdx.x / ncb;
    const int32_t cb = (int32_t)(blockIdx.x - b * ncb);
    const int32_t tile0 = blockIdx.y * T;
    const int32_t w = cb * kLinearTile + c;
    // a column past the row's words reads the last word (valid memory) and stores zero, or nothing past the stride
    const uint32_t* xp = x + (size_t)b * n_in * stride + (w < words ? w : words - 1);
    const v4i* ap = frags + (size_t)tile0 * k_steps * 64 + lane;  // tile t, step s: ap[(t k_steps + s) 64]

    v16i acc[T][4];
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int l = 0; l < 4; l++)
#pragma unroll
            for (int v = 0; v < 16; v++) acc[t][l][v] = 0;

    uint32_t xv[16], xn[16];
    v4i a[T], an[T];
    const int32_t last = n_in - 1;
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const int32_t j = 16 * grp + e;
        xn[e] = xp[(size_t)(j < last ? j : last) * stride];
    }
#pragma unroll
    for (int t = 0; t < T; t++) an[t] = ap[(size_t)t * k_steps * 64];
#pragma unroll 1
    for (int32_t s = 0; s < k_steps; s++) {
#pragma unroll
        for (int e = 0; e < 16; e++) xv[e] = xn[e];
#pragma unroll
        for (int t = 0; t < T; t++) a[t] = an[t];
        if (s + 1 < k_steps) {  // the next step's operands are requested before this step's products are issued
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int32_t j = (s + 1) * kLinearTile + 16 * grp + e;
                xn[e] = xp[(size_t)(j < last ? j : last) * stride];
            }
#pragma unroll
            for (int t = 0; t < T; t++) an[t] = ap[((size_t)t * k_steps + s + 1) * 64];
        }
        v4i bl[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            uint32_t d[4];
            limb_dwords((xv[4 * q] + 0x80808080u) ^ 0x80808080u, (xv[4 * q + 1] + 0x80808080u) ^ 0x80808080u,
                        (xv[4 * q + 2] + 0x80808080u) ^ 0x80808080u, (xv[4 * q + 3] + 0x80808080u) ^ 0x80808080u, d);
#pragma unroll
            for (int l = 0; l < 4; l++) bl[l][q] = (int)d[l];
        }
#pragma unroll
        for (int t = 0; t < T; t++)
#pragma unroll
            for (int l = 0; l < 4; l++) acc[t][l] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[t], bl[l], acc[t][l], 0, 0, 0);
    }
    if (w >= stride) return;
    uint32_t* op = out + (size_t)b * n_out * stride + w;
#pragma unroll
    for (int t = 0; t < T; t++) {
#pragma unroll
        for (int v = 0; v < 16; v++) {
            const int32_t i = (tile0 + t) * kLinearTile + 8 * (v >> 2) + 4 * grp + (v & 3);
            if (i < n_out) {
                uint32_t sum = (uint32_t)acc[t][0][v] + ((uint32_t)acc[t][1][v] << 8) + ((uint32_t)acc[t][2][v] << 16) + ((uint32_t)acc[t][3][v] << 24);
                if (bias && w == bias_word) sum += (uint32_t)bias[i];
                op[(size_t)i * stride] = w < words ? sum : 0u;
            }
        }
    }
}

template <int T>
void launch_mfma(hipStream_t stream, const LinearPlan& pl, const LinearRows& r, size_t batch, int32_t n_out, int32_t n_in, const int8_t* frags,
                 const int32_t* d_bias, const Torus32* d_x, Torus32* d_out) {
    hipLaunchKernelGGL(k_linear_mfma<T>, dim3((unsigned)(batch * (size_t)pl.col_blocks), (unsigned)pl.tile_groups), dim3(64), 0, stream,
                       reinterpret_cast<const v4i*>(frags), reinterpret_cast<const uint32_t*>(d_x), d_bias, reinterpret_cast<uint32_t*>(d_out), n_out, n_in,
                       r.words, r.stride, r.bias_word, pl.col_blocks, pl.k_steps);
}

}  // namespace

void LweLinear::launch(hipStream_t stream, const LinearPlan& pl, int32_t rows, size_t batch, int32_t n_out, int32_t n_in, const int8_t* d_w,
                       const int32_t* d_bias, const Torus32* d_x, Torus32* d_out) {
    LinearCall c;
    c.rows = rows, c.batch = batch, c.n_out = n_out, c.n_in = n_in, c.w = d_w, c.bias = d_bias, c.x = d_x, c.out = d_out, c.device = true;
    if (const char* e = linear_call_error(p_, c)) throw std::invalid_argument(e);
    if (batch == 0) return;
    const LinearRows r = linear_rows(p_, rows);
    const LinearPlan want = linear_plan(r, n_out, n_in, pl.kernel);
    if (pl.kernel != want.kernel || pl.col_blocks != want.col_blocks || pl.wave_tiles != want.wave_tiles || pl.k_steps != want.k_steps ||
        pl.tile_groups != want.tile_groups || pl.frag_bytes != want.frag_bytes)
        throw std::invalid_argument("lwe_linear: plan of another call");
    if (pl.kernel == kLinearSimple) {
        const int64_t total = (int64_t)batch * n_out * r.stride;
        const int64_t blocks = (total + 255) / 256;
        hipLaunchKernelGGL(k_linear_simple, dim3((unsigned)(blocks < ((int64_t)1 << 30) ? blocks : (int64_t)1 << 30)), dim3(256), 0, stream, d_w,
                           reinterpret_cast<const uint32_t*>(d_x), d_bias, reinterpret_cast<uint32_t*>(d_out), total, n_out, n_in, r.words, r.stride,
                           r.bias_word);
        return;
    }
    if (batch * (size_t)pl.col_blocks > (size_t)INT32_MAX) throw std::invalid_argument("lwe_linear: batch x column blocks exceeds a launch");
    frags_.reserve_exact(pl.frag_bytes);
    hipLaunchKernelGGL(k_linear_prepare, dim3((unsigned)pl.k_steps, (unsigned)pl.padded_tiles()), dim3(256), 0, stream, d_w,
                       reinterpret_cast<uint32_t*>((int8_t*)frags_), n_out, n_in, pl.k_steps);
    switch (pl.wave_tiles) {
    case 1: launch_mfma<1>(stream, pl, r, batch, n_out, n_in, frags_, d_bias, d_x, d_out); break;
    case 2: launch_mfma<2>(stream, pl, r, batch, n_out, n_in, frags_, d_bias, d_x, d_out); break;
    default: launch_mfma<4>(stream, pl, r, batch, n_out, n_in, frags_, d_bias, d_x, d_out); break;
    }
}

}  // namespace ieache
