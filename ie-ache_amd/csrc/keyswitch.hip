// LWE key switch (K5): the walk kernels and the unit's host side (keyswitch.h).
//
//   out = (0, b') - sum_{i < N} sum_{j < t} KSK[i][j][digit_j(a'_i)]        (int32, wraparound; lwe-keyswitch-functions.cpp)
//
// Which kernel takes a launch is decided in ks_plan.h and nowhere else; launch() below dispatches on its answer.
#include "keyswitch.h"

#include "keyswitch_dev.h"

namespace ieache {

namespace {

constexpr int kThreads = 256;

using namespace dev;

// ---- K5, generic: one workgroup per gate instance ----
// LDS: u [N+1] | list [N*t] | count
__global__ __launch_bounds__(kThreads) void k_keyswitch_generic(DevKeys K, WorkDesc W, const Torus32* ext,
                                                                Torus32* flat_out) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int32_t N = K.N, n = K.n, t = K.ks_t, basebit = K.ks_basebit, stride = K.stride;
    int32_t* u = reinterpret_cast<int32_t*>(smem);
    uint32_t* list = reinterpret_cast<uint32_t*>(u + N + 4);
    __shared__ uint32_t s_count;
    const int64_t item = (int64_t)blockIdx.x;
    const Torus32* src = ext + (size_t)item * (N + 4);
    if (threadIdx.x == 0) s_count = 0;
    for (int32_t j = threadIdx.x; j <= N; j += blockDim.x) u[j] = src[j];
    __syncthreads();
    const uint32_t prec_offset = 1u << (32 - (1 + basebit * t));
    const uint32_t mask = (1u << basebit) - 1;
    for (int32_t idx = threadIdx.x; idx < N * t; idx += blockDim.x) {
        const int32_t i = idx / t, j = idx - i * t;
        const uint32_t d = ks_digit((uint32_t)u[i] + prec_offset, j, basebit, mask);
        if (d) list[atomicAdd(&s_count, 1u)] = ((uint32_t)idx << basebit) + d;  // row index [i][j][d]
    }
    __syncthreads();
    const uint32_t cnt = s_count;
    // subtraction mod 2^32 commutes, so the (non-deterministic) list order does not matter
    Torus32* out = flat_out ? flat_out + (size_t)item * stride : resolve(W, W.item0 + item, stride).out;
    const uint32_t bprime = (uint32_t)u[N];
    // every column of the row, kThreads at a time (any n: the list is walked once per pass of columns)
    for (int32_t q = threadIdx.x; q < stride; q += kThreads) {
        uint32_t r = 0;
        for (uint32_t e = 0; e < cnt; e++) r -= (uint32_t)K.ksk[(size_t)list[e] * stride + q];
        out[q] = q <= n ? (int32_t)(r + (q == n ? bprime : 0u)) : 0;
    }
}

// ---- K5, vectorised: one 512-thread workgroup per gate instance ----
// The non-zero digits are compacted into a row list; the 8 waves take list
// entries round-robin, each wave subtracting whole 16-byte-per-lane row pieces
// (NLD dwordx4 loads cover one padded KSK row), four rows in flight per wave;
// the 8 partial sums meet in LDS.  Subtraction mod 2^32 commutes, so neither the
// list order nor the split changes a single bit.
// LDS: u [N+4] | list [N*t] | part [8][stride]
constexpr int kKsThreads = 512;
template <int NLD>
__global__ __launch_bounds__(kKsThreads) void k_keyswitch_vec(DevKeys K, WorkDesc W, const Torus32* ext,
                                                              Torus32* flat_out, int32_t splits) {
    // splits > 1 (launches of a handful of gates, where one workgroup per gate leaves the chip idle and the walk's
    // latency is what counts): blockIdx.y takes coefficients [y*N/splits, (y+1)*N/splits) and ADDS its share to an
    // output row that k_keyswitch_init has set to (0, ..., 0, b); int32 addition commutes, so the bits do not change
    extern __shared__ __align__(16) unsigned char smem[];
    const int32_t N = K.N, n = K.n, t = K.ks_t, basebit = K.ks_basebit, stride = K.stride;
    int32_t* u = reinterpret_cast<int32_t*>(smem);
    uint32_t* list = reinterpret_cast<uint32_t*>(u + N + 4);
    int4* part = reinterpret_cast<int4*>(list + (size_t)N * t);
    __shared__ uint32_t s_count;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t item = (int64_t)blockIdx.x;
    const Torus32* src = ext + (size_t)item * (N + 4);
    if (tid == 0) s_count = 0;
    for (int32_t j = tid; j <= N; j += kKsThreads) u[j] = src[j];
    __syncthreads();
    const uint32_t prec_offset = 1u << (32 - (1 + basebit * t));
    const uint32_t mask = (1u << basebit) - 1;
    const int32_t idx0 = splits > 1 ? (int32_t)blockIdx.y * (N / splits) * t : 0;
    const int32_t idx1 = splits > 1 ? idx0 + (N / splits) * t : N * t;
    for (int32_t idx = idx0 + tid; idx < idx1; idx += kKsThreads) {
        const int32_t i = idx / t, j = idx - i * t;
        const uint32_t d = ks_digit((uint32_t)u[i] + prec_offset, j, basebit, mask);
        if (d) list[atomicAdd(&s_count, 1u)] = ((uint32_t)idx << basebit) + d;  // row index [i][j][d]
    }
    __syncthreads();
    const uint32_t cnt = s_count;
    const int32_t nvec = stride >> 2;
    int4 acc[NLD];
#pragma unroll
    for (int v = 0; v < NLD; v++) acc[v] = make_int4(0, 0, 0, 0);
    const int4* kbase = reinterpret_cast<const int4*>(K.ksk);
    uint32_t e = wave;
    for (; e + 24 < cnt; e += 32) {  // four rows (e, e+8, e+16, e+24) in flight
        int4 r[4][NLD];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int4* row = kbase + (size_t)list[e + 8 * q] * nvec;
#pragma unroll
            for (int v = 0; v < NLD; v++)
                r[q][v] = (lane + 64 * v < nvec) ? row[lane + 64 * v] : make_int4(0, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int v = 0; v < NLD; v++) {
                acc[v].x -= r[q][v].x;
                acc[v].y -= r[q][v].y;
                acc[v].z -= r[q][v].z;
                acc[v].w -= r[q][v].w;
            }
    }
    for (; e < cnt; e += 8) {
        const int4* row = kbase + (size_t)list[e] * nvec;
#pragma unroll
        for (int v = 0; v < NLD; v++)
            if (lane + 64 * v < nvec) {
                const int4 rr = row[lane + 64 * v];
                acc[v].x -= rr.x;
                acc[v].y -= rr.y;
                acc[v].z -= rr.z;
                acc[v].w -= rr.w;
            }
    }
#pragma unroll
    for (int v = 0; v < NLD; v++)
        if (lane + 64 * v < nvec) part[(size_t)wave * nvec + lane + 64 * v] = acc[v];
    __syncthreads();
    Torus32* out = flat_out ? flat_out + (size_t)item * stride : resolve(W, W.item0 + item, stride).out;
    const int32_t* parti = reinterpret_cast<const int32_t*>(part);
    for (int32_t q = tid; q < stride; q += kKsThreads) {
        uint32_t v = 0;
#pragma unroll
        for (int w = 0; w < 8; w++) v += (uint32_t)parti[(size_t)w * stride + q];
        if (splits > 1) {
            if (q <= n) atomicAdd(reinterpret_cast<uint32_t*>(out) + q, v);
            continue;
        }
        if (q == n) v += (uint32_t)u[N];
        out[q] = q <= n ? (int32_t)v : 0;
    }
}

// output rows of a split key switch: (0, ..., 0, b) with b the extracted sample's last word
__global__ __launch_bounds__(256) void k_keyswitch_init(DevKeys K, WorkDesc W, const Torus32* ext, Torus32* flat_out) {
    const int64_t item = (int64_t)blockIdx.x;
    const int32_t n = K.n, stride = K.stride;
    Torus32* out = ks_out_row(W, flat_out, item, stride);
    const Torus32 b = ext[(size_t)item * (K.N + 4) + K.N];
    for (int32_t q = threadIdx.x; q < stride; q += 256) out[q] = q == n ? b : 0;
}

// ---- K5, gate-batched: one workgroup per G gate instances ----
// The key-switch key does not fit the L2s (83 MB), so K5 is bound by how many KSK bytes
// are fetched per gate.  Here a workgroup walks ALL (i, j) positions once, loads the
// three candidate rows [i][j][1..3] and lets each of its G gates subtract the one its
// digit selects: 3 x 2.5 KB x N x t / G bytes per gate instead of ~0.75 x 2.5 KB x N x t.
// One wave per 64 int4 columns of a row (3 waves at n=630), each lane owning one column
// for all G gates, so no partial sums cross waves.  The t digits of a'_i are packed into
// one word per gate, pulled into SGPRs once per i; the digit (wave-uniform) indexes a 4-row
// register table {0, r1, r2, r3} through the SGPR-indexed VGPR mode (s_set_gpr_idx), which is
// 3x cheaper than v_cndmask chains or scalar branches.  Subtraction mod 2^32 commutes, so the
// result is bit-identical to the other kernels.
// LDS: dw [G][N] u16 | bprime [G]
template <int G>
__global__ __launch_bounds__(256) void k_keyswitch_batch(DevKeys K, WorkDesc W, const Torus32* ext, Torus32* flat_out,
                                                         int64_t items) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int32_t N = K.N, n = K.n, t = K.ks_t, basebit = K.ks_basebit, stride = K.stride;
    uint16_t* dw = reinterpret_cast<uint16_t*>(smem);
    int32_t* bprime = reinterpret_cast<int32_t*>(dw + (size_t)G * N);
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int64_t item0 = (int64_t)blockIdx.x * G;
    const int32_t gcount = (int32_t)(items - item0 < G ? items - item0 : G);
    const uint32_t prec_offset = 1u << (32 - (1 + basebit * t));
    const uint32_t mask = (1u << basebit) - 1;
    // pack the digits of every a'_i of every gate: digit j sits at bits [j*basebit, (j+1)*basebit)
    for (int32_t idx = tid; idx < G * N; idx += nthreads) {
        const int32_t g = idx / N, i = idx - g * N;
        uint32_t packed = 0;
        if (g < gcount) {
            const uint32_t a = (uint32_t)ext[(size_t)(item0 + g) * (N + 4) + i] + prec_offset;
            for (int32_t j = 0; j < t; j++) packed |= ((a >> (32 - (j + 1) * basebit)) & mask) << (j * basebit);
        }
        dw[idx] = (uint16_t)packed;
    }
    if (tid < G) bprime[tid] = tid < gcount ? ext[(size_t)(item0 + tid) * (N + 4) + N] : 0;
    __syncthreads();

    const int32_t nvec = stride >> 2;
    const int32_t col = tid;  // one int4 column per thread
    const bool active = col < nvec;
    const int4* kbase = reinterpret_cast<const int4*>(K.ksk) + (active ? col : 0);  // idle lanes shadow column 0
    const size_t rowpitch = (size_t)nvec;  // int4 per row; rows [pos][d] are consecutive
    int4 acc[G];
#pragma unroll
    for (int g = 0; g < G; g++) acc[g] = make_int4(0, 0, 0, 0);

    // Walk i (the extracted coefficient), then its t digits.  The packed digits of a'_i of all
    // G gates are pulled into SGPRs once per i.  Candidate rows are requested two positions
    // ahead into a ring of three named row sets (the walk is latency-bound otherwise).
    const size_t npos = (size_t)N * t;
#define KS_LOAD(A, B, C, POS)                                        \
    {                                                                \
        size_t pp_ = (POS);                                          \
        if (pp_ >= npos) pp_ = npos - 1;                             \
        const int4* row_ = kbase + pp_ * 4 * rowpitch;               \
        A = row_[1 * rowpitch];                                      \
        B = row_[2 * rowpitch];                                      \
        C = row_[3 * rowpitch];                                      \
    }
#define KS_USE(A, B, C, SH)                                                        \
    {                                                                              \
        const int32_t tab_[16] = {0, 0, 0, 0, A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w, C.x, C.y, C.z, C.w}; \
        _Pragma("unroll") for (int g = 0; g < G; g++) {                            \
            const uint32_t d_ = ((dg[g] >> (SH)) & mask) * 4;  /* uniform: SGPR-indexed register read */ \
            acc[g].x -= tab_[d_ + 0];                                              \
            acc[g].y -= tab_[d_ + 1];                                              \
            acc[g].z -= tab_[d_ + 2];                                              \
            acc[g].w -= tab_[d_ + 3];                                              \
        }                                                                          \
    }
    int4 a1, a2, a3, b1, b2, b3, c1, c2, c3;
    KS_LOAD(a1, a2, a3, 0)
    KS_LOAD(b1, b2, b3, 1)
    size_t pos = 0;
    for (int32_t i = 0; i < N; i++) {
        uint32_t dg[G];
#pragma unroll
        for (int g = 0; g < G; g++) dg[g] = __builtin_amdgcn_readfirstlane((uint32_t)dw[g * N + i]);
        int32_t sh = 0;
        for (int32_t j = 0; j < t; j++, pos++, sh += basebit) {
            KS_LOAD(c1, c2, c3, pos + 2)
            KS_USE(a1, a2, a3, sh)
            a1 = b1; a2 = b2; a3 = b3;
            b1 = c1; b2 = c2; b3 = c3;
        }
    }
#undef KS_LOAD
#undef KS_USE
    if (active) {
#pragma unroll
        for (int g = 0; g < G; g++) {
            if (g < gcount) {
                int4 v = acc[g];
                if (col == (n >> 2)) {  // the column holding b'
                    const int32_t bp = bprime[g];
                    switch (n & 3) {
                        case 0: v.x += bp; break;
                        case 1: v.y += bp; break;
                        case 2: v.z += bp; break;
                        default: v.w += bp; break;
                    }
                }
                Torus32* out = flat_out ? flat_out + (size_t)(item0 + g) * stride : resolve(W, W.item0 + item0 + g, stride).out;
                reinterpret_cast<int4*>(out)[col] = v;
            }
        }
    }
}

// NLD = 1 .. 4 dwordx4 loads cover one padded KSK row
using VecKernel = void (*)(DevKeys, WorkDesc, const Torus32*, Torus32*, int32_t);
VecKernel vec_kernel(int nld) {
    return nld == 1 ? k_keyswitch_vec<1> : nld == 2 ? k_keyswitch_vec<2> : nld == 3 ? k_keyswitch_vec<3> : k_keyswitch_vec<4>;
}

}  // namespace

void KeySwitch::init(const Params& p, const DevKeys& K) {
    p_ = p;
    K_ = K;
    sup_ = ks_support(p);
    if (sup_.generic_lds > kKsLdsMax) throw std::invalid_argument("parameter set exceeds the 160 KiB LDS of a CU");
    // (per context, on the context's device: the sizes depend on the parameter set)
    allow_dynamic_lds((const void*)k_keyswitch_generic, sup_.generic_lds, "k_keyswitch_generic");
    if (sup_.batch) allow_dynamic_lds((const void*)k_keyswitch_batch<16>, sup_.batch_lds, "k_keyswitch_batch");
    if (sup_.nld > 0) allow_dynamic_lds((const void*)vec_kernel(sup_.nld), sup_.vec_lds, "k_keyswitch_vec");
}

void KeySwitch::load_key(const int32_t* d_ksk_padded, hipStream_t stream) {
    K_.ksk = d_ksk_padded;
    if (!sup_.mfma) return;
    if (!limbs_) limbs_.allocate(ks_limb_matrix_bytes(p_));
    ksm::prepare(p_, d_ksk_padded, limbs_, stream);
    HIP_CHECK(hipGetLastError());
}

// the grown() policy in bytes
void KeySwitch::reserve(KsScratch& scratch, int64_t cnt, const EvalOptions& opt, bool force_generic) {
    if (const size_t need = ks_scratch_bytes(sup_, p_, opt, limbs_ != nullptr, force_generic, cnt))
        scratch.digits.reserve(need, ks_digit_scratch_bytes(p_, opt.chunk), 1, ks_digit_scratch_bytes(p_, 4096));
}

void KeySwitch::launch(KsScratch& scratch, hipStream_t stream, const WorkDesc& w, int64_t cnt, const Torus32* ext, Torus32* flat_out,
                       const EvalOptions& opt, bool force_generic) {
    const KsPlan pl = ks_plan(sup_, p_, opt, limbs_ != nullptr, force_generic, cnt);
    const dim3 grid((unsigned)cnt);
    switch (pl.family) {
        case KsFamily::Mfma:
            reserve(scratch, cnt, opt, force_generic);  // in place already unless the caller did not reserve
            ksm::launch(p_, K_, w, cnt, ext, flat_out, limbs_, scratch.digits, pl.ksplit, pl.xcd_map, stream);
            break;
        case KsFamily::Sliced:
            kss::launch(p_, K_, w, cnt, ext, flat_out, pl.slice, pl.gates_per_wg, stream);
            break;
        case KsFamily::Batched:
            hipLaunchKernelGGL(k_keyswitch_batch<16>, dim3((unsigned)((cnt + 15) / 16)), dim3(64 * sup_.nld), sup_.batch_lds, stream, K_, w, ext,
                               flat_out, cnt);
            break;
        case KsFamily::PerGate:
            if (pl.splits > 1) hipLaunchKernelGGL(k_keyswitch_init, grid, dim3(256), 0, stream, K_, w, ext, flat_out);
            hipLaunchKernelGGL(vec_kernel(sup_.nld), dim3((unsigned)cnt, (unsigned)pl.splits), dim3(kKsThreads), sup_.vec_lds, stream, K_, w, ext,
                               flat_out, pl.splits);
            break;
        case KsFamily::Generic:
            hipLaunchKernelGGL(k_keyswitch_generic, grid, dim3(kThreads), sup_.generic_lds, stream, K_, w, ext, flat_out);
            break;
    }
}

bool KeySwitch::window_needs_rows(int64_t cnt, const EvalOptions& opt, bool force_generic) const {
    return cnt > 0 && ks_plan(sup_, p_, opt, limbs_ != nullptr, force_generic, cnt).family != KsFamily::Mfma;
}

void KeySwitch::extract_window(hipStream_t stream, int64_t cnt, const KsWindowRows& rows, Torus32* u, int32_t stride) {
    ksm::extract_window(p_, cnt, rows, u, stride, stream);
}

void KeySwitch::launch_window(KsScratch& scratch, hipStream_t stream, int64_t cnt, const KsWindowRows& rows, Torus32* ext, Torus32* out_rows,
                              const EvalOptions& opt, bool force_generic) {
    if (cnt <= 0) return;
    const KsPlan pl = ks_plan(sup_, p_, opt, limbs_ != nullptr, force_generic, cnt);
    if (pl.family == KsFamily::Mfma) {
        reserve(scratch, cnt, opt, force_generic);  // in place already unless the caller did not reserve
        ksm::launch_window(p_, K_, cnt, rows, out_rows, limbs_, scratch.digits, pl.ksplit, pl.xcd_map, stream);
        return;
    }
    if (!ext) throw std::invalid_argument("key switch of a window: no rows to store the extracted samples in");
    ksm::extract_window(p_, cnt, rows, ext, p_.N + 4, stream);
    launch(scratch, stream, dev::WorkDesc{}, cnt, ext, out_rows, opt, force_generic);
}

}  // namespace ieache
