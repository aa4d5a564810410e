// Blind rotation on the ring of degree 2048 (blind_rotate_h2.h): one CMux step as two external products on the ring of degree
// 1024, on the 512-point transform of fft512.h.  DESIGN.md section 4.15.
//
// A polynomial of Z[X]/(X^2048 + 1) is p = p_e(Y) + X p_o(Y) with Y = X^2, both halves in Z[Y]/(Y^1024 + 1).  For a digit
// polynomial d and a key polynomial k
//     (d k)_e = d_e k_e + (Y d_o) k_o        (d k)_o = d_e k_o + d_o k_e
// where Y d_o is d_o moved up one coefficient with the negacyclic sign on the one that wraps: an index and one negated digit.
// X^a acts on the halves as Y^(a/2) on each for even a; for odd a the halves change places:
//     new even = Y^((a+1)/2) p_o             new odd = Y^((a-1)/2) p_e
// The decomposition is coefficient by coefficient, so the digits of the halves of (X^a - 1) acc are the halves of its digits.
//
// Schedule: one workgroup of two waves per gate instance.  Wave 0 owns the EVEN halves of both output polynomials, wave 1 the
// ODD halves.  Each transforms the 4l digit rows it needs -- (accumulator polynomial c, half dh, digit q); wave 0 reads the odd
// half's digits one coefficient down, which is the Y shift -- and multiplies each with the four blocks (output polynomial,
// limb) of the key half dh ^ wave of row (c, q): k_blind_rotate_x1's step with twice the rows, four spectrum sums in 128
// VGPRs, two interleaved inverse pairs, limbs recombined as lo + (hi << 16).  Both waves read all four accumulator halves
// and each writes its own two, so a step has two workgroup barriers: before the update and after it.  The accumulator
// (16 KiB, de-interleaved: [c][half][1024]) lives in LDS and is parked in coefficient order in the state block between slices.
// Every rounded sum is 4l x 1024 products of a digit (2^(Bgbit-1)) and a limb (2^15): <= 2^46 under Params::br_exact().
#include "blind_rotate_h2.h"

#include <stdexcept>

#include "blind_rotate_w64.h"
#include "br_step.h"

namespace ieache {
namespace h2 {

using namespace dev;
using namespace w64;  // kN = 1024 and kM = 512 are the HALF ring's here

namespace {

constexpr int kN2 = 2 * kN;                                   // the ring's degree
constexpr int kBlockBytes = kM * (int)sizeof(double2);        // one spectrum: 8 KiB
constexpr int kHalfBytes = 4 * kBlockBytes;                   // q = 2 c + limb of one half of one row
constexpr int kRowBytes = 2 * kHalfBytes;                     // even half, odd half

// ---- key preparation: BK polynomial -> the two-limb spectra of its even and of its odd half ----
// bkf layout: [n][2l rows][half][q = 2 c + limb][k2 = 8][lane = 64]
__global__ __launch_bounds__(64) void k_bk_to_spectrum_h2(const Torus32* bk_raw, double2* bkf) {
    __shared__ __align__(16) double2 sT[kTile];
    __shared__ __align__(16) double2 sTw[kTwElems];
    const int lane = threadIdx.x;
    build_twiddles(sTw, lane, 64);
    __syncthreads();
    const LaneRoots R = make_roots(sTw, lane);
    const size_t poly = blockIdx.x;  // (i * 2l + row) * 2 + c
    const Torus32* src = bk_raw + poly * kN2;
    const size_t irow = poly >> 1, c = poly & 1;
#pragma unroll 1
    for (int hl = 0; hl < 4; hl++) {
        const int half = hl >> 1, limb = hl & 1;
        double2 x[8];
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const int32_t v0 = src[2 * (64 * r + lane) + half], v1 = src[2 * (64 * r + lane + kM) + half];
            const int32_t lo0 = (int16_t)(v0 & 0xFFFF), lo1 = (int16_t)(v1 & 0xFFFF);
            const int32_t e0 = limb ? (int32_t)(((int64_t)v0 - lo0) >> 16) : lo0;
            const int32_t e1 = limb ? (int32_t)(((int64_t)v1 - lo1) >> 16) : lo1;
            x[r] = make_double2((double)e0, (double)e1);
        }
        fft512_forward<true>(x, sT, lane, R);
        double2* dst = bkf + ((((irow * 2 + half) * 4) + c * 2 + limb) * 8) * 64 + lane;
#pragma unroll
        for (int k2 = 0; k2 < 8; k2++) dst[k2 * 64] = x[k2];
    }
}

// ---- K0..K2: gate pre-combination, mod switch to 2N = 4096, accumulator = X^(2N - barb) times the constant polynomial, the
// item's test polynomial or (a table of TLWE samples) both halves of its sample; coefficient order ----
__global__ __launch_bounds__(256) void k_h2_prologue(DevKeys K, WorkDesc W, uint16_t* st_bara, int32_t nb, int32_t* st_acc) {
    __shared__ int32_t s_barb;
    const int tid = threadIdx.x;
    const int32_t n = K.n;
    const int64_t item = (int64_t)blockIdx.x;
    const GateInst g = resolve(W, W.item0 + item, K.stride);
    uint16_t* bara = st_bara + (size_t)item * nb;
    for (int32_t i = tid; i <= n; i += 256) {
        const int32_t bar = modswitch2N(combined_coef(g, i, n), 12);
        if (i < n)
            bara[i] = (uint16_t)bar;
        else
            s_barb = bar;
    }
    __syncthreads();
    const int32_t a0 = (2 * kN2 - s_barb) & (2 * kN2 - 1);
    int32_t* acc = st_acc + (size_t)item * 2 * kN2;
    const bool tlwe = W.flat_type == kFlatRawTlwe;
    const Torus32* v = test_poly_row(W, W.item0 + item, tlwe ? 2 * kN2 : kN2);
    for (int32_t j = tid; j < kN2; j += 256) {
        acc[j] = (v && tlwe) ? rot_coef(v, j, a0, kN2) : 0;
        if (v)
            acc[kN2 + j] = rot_coef(tlwe ? v + kN2 : v, j, a0, kN2);
        else
            acc[kN2 + j] = ((j - a0) & (2 * kN2 - 1)) < kN2 ? kMU : -kMU;
    }
}

// word (c, m) of the accumulator in coefficient order, from the de-interleaved LDS form [c][half][1024]
__device__ __forceinline__ int32_t& acc_word(int32_t* acc, int c, int32_t m) { return acc[(2 * c + (m & 1)) * kN + (m >> 1)]; }

// One digit row of this wave: the digit at shift `sh` of the decomposed words, negated in coefficient 0 where the row is a Y
// shift (sign0 = -1 in lane 0, 1 elsewhere), transformed, times the four blocks [q = 2 c + limb] at byte offset brow of the
// step's resource, added into the four sums.  digit_row_two_limb_rt (br_step.h) with the sign and without the FIRST form.
__device__ __forceinline__ void digit_row_h2(double2 (&s)[4][8], const uint32_t (&v0)[8], const uint32_t (&v1)[8], int sh, int bgbit, double sign0,
                                             __amdgpu_buffer_rsrc_t bk_rsrc, int lane16, int brow, double2* sT, int lane, const LaneRoots& R) {
    double2 x[8], bA[8], bB[8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int32_t e0 = __builtin_amdgcn_sbfe((int32_t)v0[r], sh, bgbit), e1 = __builtin_amdgcn_sbfe((int32_t)v1[r], sh, bgbit);
        x[r] = make_double2((double)e0, (double)e1);
    }
    x[0].x *= sign0;
    __builtin_amdgcn_sched_barrier(0);
    auto req = [&]() { load_bk_block(bA, bk_rsrc, lane16, brow); };
    fft512_forward<true, 1, decltype(req), true>(x, sT, lane, R, req);
    load_bk_block(bB, bk_rsrc, lane16, brow + kBlockBytes);
    __builtin_amdgcn_sched_barrier(0);
    mac_row<false>(s[0], x, bA);
    __builtin_amdgcn_sched_barrier(0);
    load_bk_block(bA, bk_rsrc, lane16, brow + 2 * kBlockBytes);
    __builtin_amdgcn_sched_barrier(0);
    mac_row<false>(s[1], x, bB);
    __builtin_amdgcn_sched_barrier(0);
    load_bk_block(bB, bk_rsrc, lane16, brow + 3 * kBlockBytes);
    __builtin_amdgcn_sched_barrier(0);
    mac_row<false>(s[2], x, bA);
    mac_row<false>(s[3], x, bB);
}

// ---- K3 (+K4): CMux steps [i0, i1), i1 - i0 <= 64, of every gate instance; (l, bgbit) launch arguments, 2l <= 16 ----
__global__ __launch_bounds__(128) void k_blind_rotate_h2(DevKeys K, const double2* __restrict__ bkf, const uint16_t* __restrict__ st_bara, int32_t nb,
                                                         int32_t* st_acc, int32_t i0, int32_t i1, Torus32* ext, const double2* __restrict__ gtw, int l,
                                                         int bgbit) {
    __shared__ __align__(16) int32_t acc[2 * kN2];  // [c][half][1024]
    __shared__ __align__(16) double2 sT_all[2 * kTile];
    __shared__ __align__(16) double2 sTw[kTwElems];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // 0: the even halves of the outputs, 1: the odd halves
    double2* sT = sT_all + wave * kTile;
    const int64_t item = (int64_t)blockIdx.x;
    const uint16_t* __restrict__ bara = st_bara + (size_t)item * nb;
    int32_t* gacc = st_acc + (size_t)item * 2 * kN2;
    load_twiddles(sTw, gtw, tid, 128);
    {   // four consecutive coefficients e o e o -> two words of each half
        const int4* src = reinterpret_cast<const int4*>(gacc);
#pragma unroll
        for (int r = 0; r < 2 * kN2 / 4 / 128; r++) {
            const int v = 128 * r + tid;  // words 4v .. 4v + 3 of polynomial v / 512
            const int4 w = src[v];
            const int c = v >> 9, m = (v & 511) * 2;
            *reinterpret_cast<int2*>(&acc[(2 * c) * kN + m]) = make_int2(w.x, w.z);
            *reinterpret_cast<int2*>(&acc[(2 * c + 1) * kN + m]) = make_int2(w.y, w.w);
        }
    }
    __syncthreads();
    const LaneRoots R = make_roots(sTw, lane);

    const int step_bytes = 2 * l * kRowBytes;
    const size_t step_elems = (size_t)step_bytes / sizeof(double2);
    const int lane16 = bk_lane_offset(lane);
    const uint32_t dec_offset = decomposition_offset_rt(l, bgbit);
    const int32_t my_a = lane_amounts(bara, i0, i1, lane);
#pragma unroll 1
    for (int32_t i = i0; i < i1; i++) {
        const int32_t a = __builtin_amdgcn_readlane(my_a, i - i0);
        if (a == 0) continue;  // uniform over the workgroup; exact arithmetic makes the step a no-op
        // BK_i alone behind the resource: nothing past the step can be read, and offsets stay below 2^21 for any n
        const __amdgpu_buffer_rsrc_t bk_rsrc = bk_resource(bkf + (size_t)i * step_elems, 1, step_bytes);
        double2 s[4][8];
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int r = 0; r < 8; r++) s[q][r] = make_double2(0.0, 0.0);
#pragma unroll 1
        for (int g = 0; g < 4; g++) {
            const int c = g >> 1, dh = g & 1;
            // half dh of X^a acc_c is Y^t of half src (the halves change places for odd a)
            const int src = dh ^ (a & 1);
            const int32_t t = (a & 1) ? (dh ? (a - 1) >> 1 : (a + 1) >> 1) : a >> 1;  // 0 .. 2048: taken mod 2048 below (Y^2048 = 1)
            const int32_t sft = (wave == 0 && dh == 1) ? 1 : 0;                       // the Y shift of d_o in the even output
            const int32_t* rot = acc + (2 * c + src) * kN;
            const int32_t* own = acc + (2 * c + dh) * kN;
            uint32_t v0[8], v1[8];
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const int32_t m0 = (64 * r + lane - sft) & (kN - 1), m1 = m0 ^ kM;  // coefficient j - sft, j = 64 r + lane and j + 512
                const int32_t r0 = (m0 - t) & (2 * kN - 1), r1 = (m1 - t) & (2 * kN - 1);  // in the ring [half, -half] of 2048
                const uint32_t x0 = (uint32_t)rot[r0 & (kN - 1)], x1 = (uint32_t)rot[r1 & (kN - 1)];
                const uint32_t n0 = (r0 & kN) ? 0u - x0 : x0, n1 = (r1 & kN) ? 0u - x1 : x1;
                v0[r] = ((n0 - (uint32_t)own[m0]) + dec_offset) ^ dec_offset;
                v1[r] = ((n1 - (uint32_t)own[m1]) + dec_offset) ^ dec_offset;
            }
            const double sign0 = (sft && lane == 0) ? -1.0 : 1.0;  // coefficient 0 of Y d_o is -d_o[1023]
            const int brow0 = (c * l * 2 + (dh ^ wave)) * kHalfBytes;  // row c l + q, key half dh ^ wave: + q kRowBytes
#pragma unroll 1
            for (int q = 0; q < l; q++)
                digit_row_h2(s, v0, v1, 32 - (q + 1) * bgbit, bgbit, sign0, bk_rsrc, lane16, brow0 + q * kRowBytes, sT, lane, R);
        }
        __syncthreads();  // the partner has read this wave's halves for the last time in this step
#pragma unroll
        for (int c = 0; c < 2; c++) {
            fft512_inverse_pair<true>(s[2 * c], s[2 * c + 1], sT, lane, R);
            uint32_t* accc = reinterpret_cast<uint32_t*>(acc) + (2 * c + wave) * kN;
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const uint32_t d0 = join_limbs(s[2 * c][r].x, s[2 * c + 1][r].x, r), d1 = join_limbs(s[2 * c][r].y, s[2 * c + 1][r].y, r);
                const int32_t j = 64 * r + lane;
                __hip_atomic_fetch_add(&accc[j], d0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                __hip_atomic_fetch_add(&accc[j + kM], d1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            }
        }
        __syncthreads();  // both halves updated before the next step reads them
    }
    if (ext) {  // K4: u = (a'_0 = A_0, a'_j = -A_{N-j}; b' = B_0), a row of N + 4 words
        Torus32* u = ext + (size_t)item * (kN2 + 4);
        for (int32_t j = tid; j <= kN2; j += 128)
            u[j] = j == 0 ? acc_word(acc, 0, 0) : (j == kN2 ? acc_word(acc, 1, 0) : (int32_t)(0u - (uint32_t)acc_word(acc, 0, kN2 - j)));
    } else {
        int4* dst = reinterpret_cast<int4*>(gacc);
#pragma unroll
        for (int r = 0; r < 2 * kN2 / 4 / 128; r++) {
            const int v = 128 * r + tid;
            const int c = v >> 9, m = (v & 511) * 2;
            const int2 e = *reinterpret_cast<const int2*>(&acc[(2 * c) * kN + m]), o = *reinterpret_cast<const int2*>(&acc[(2 * c + 1) * kN + m]);
            dst[v] = make_int4(e.x, o.x, e.y, o.y);
        }
    }
}

}  // namespace

size_t spectrum_elems(const Params& p) { return (size_t)p.n * p.kpl() * 2 * 4 * kM; }

void prepare_spectrum(const Params& p, const Torus32* d_bk_raw, double2* d_bkf, hipStream_t stream) {
    const size_t npoly = (size_t)p.n * p.kpl() * 2;
    hipLaunchKernelGGL(k_bk_to_spectrum_h2, dim3((unsigned)npoly), dim3(64), 0, stream, d_bk_raw, d_bkf);
}

int launch(const Params& p, const DevKeys& K, const double2* bkf, const double2* twiddles, const BrPlan& plan, hipStream_t stream, const BrPart* parts,
           size_t n_parts, void* state, Torus32* ext, int32_t steps, Torus32* dbg_acc) {
    if (!br_h2_supported(p) || !plan.h2 || !bkf || !twiddles) throw std::logic_error("blind rotation on the ring of degree 2048: not this plan's kernel");
    int64_t items = 0;
    for (size_t q = 0; q < n_parts; q++) {
        if (parts[q].cnt < 1) throw std::logic_error("blind-rotation launch: an empty part");
        items += parts[q].cnt;
    }
    if (items < 1) throw std::logic_error("blind-rotation launch without items");
    const int32_t S = plan.slice;
    if (S < 1 || S > 64) throw std::logic_error("blind-rotation plan: slice length out of the kernel's range");  // one amount per lane
    const int32_t nb = br_bara_stride(p);
    const int32_t nsteps = steps < 0 ? p.n : (steps < p.n ? steps : p.n);
    int32_t* st_acc = reinterpret_cast<int32_t*>(state);
    uint16_t* st_bara = reinterpret_cast<uint16_t*>(st_acc + (size_t)items * 2 * kN2);
    int64_t off = 0;
    for (size_t q = 0; q < n_parts; q++) {
        hipLaunchKernelGGL(k_h2_prologue, dim3((unsigned)parts[q].cnt), dim3(256), 0, stream, K, parts[q].W, st_bara + (size_t)off * nb, nb,
                           st_acc + (size_t)off * 2 * kN2);
        off += parts[q].cnt;
    }
    int launches = 0;
    auto slice = [&](int32_t i0, int32_t i1, Torus32* e) {
        hipLaunchKernelGGL(k_blind_rotate_h2, dim3((unsigned)items), dim3(128), 0, stream, K, bkf, st_bara, nb, st_acc, i0, i1, e, twiddles, (int)p.l,
                           (int)p.Bgbit);
        launches++;
    };
    for (int32_t i0 = 0; i0 < nsteps; i0 += S) {
        const int32_t i1 = i0 + S < nsteps ? i0 + S : nsteps;
        slice(i0, i1, i1 == nsteps ? ext : nullptr);  // the last slice extracts instead of parking the accumulator
    }
    if (nsteps == 0 && ext) slice(0, 0, ext);  // degenerate (steps == 0): extraction straight from the initial accumulator
    if (dbg_acc) (void)hipMemcpyAsync(dbg_acc, st_acc, (size_t)items * 2 * kN2 * 4, hipMemcpyDeviceToDevice, stream);
    return launches;
}

}  // namespace h2
}  // namespace ieache
