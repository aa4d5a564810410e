// Blind rotation for the N=1024 ring (tfhe_blindRotate_FFT of libtfhe), on 64-lane wavefronts.
//
// Same mathematics as k_blind_rotate_generic, re-laid out for CDNA4:
//   * the 512-point complex transform is 8 x 8 x 8: three radix-8 passes done entirely in registers (8 points per lane),
//     separated by two register<->lane transposes -- through a padded, bank-conflict-free LDS tile per wave, or cross-lane
//     with v_permlane*_swap / v_cndmask_b32_dpp (the forward lane-high one, by default);
//   * the spectrum stays in registers between the forward transform, the point-wise multiply-accumulate with BK_i and the
//     inverse transform; BK_i is stored in exactly the (register, lane) order the forward transform leaves its output in, so
//     every BK load is one coalesced 1 KiB load per wave, issued ahead of its MACs;
//   * the CMux step index is the OUTER loop of the evaluator: one launch advances every gate of a chunk by a slice of steps,
//     so all resident workgroups read the same BK blocks while they are hot in the XCD's L2;
//   * the accumulator (2 x 1024 int32) lives in LDS only because the X^a rotation needs arbitrary shifts; twiddles come from a
//     9 KiB LDS table.
//   * the 512-point complex transform is 8 x 8 x 8 (fft512.h) with the register part of the negacyclic twist folded into its
//     first / last radix-8 pass.
// One kernel per launch-size regime (which one takes a launch: br_plan.h):
//   k_blind_rotate_w1b    one wave per gate            launches of more than 5 gates per CU (the throughput kernel)
//   k_blind_rotate_w2r    two waves per gate           2 .. 5 gates per CU
//   k_blind_rotate_w4r    four waves per gate          1 .. 2 gates per CU
//   k_blind_rotate_wide4  2L = 6 waves per gate        at most one gate per CU (single expressions: the reference's own mode)
// all on the ONE-limb spectrum (libtfhe's own product, rounded to the exact integer under a rounding guard and a sampled
// audit), and on the TWO-limb spectrum (exact by construction: "exact_fft", repeats, audits)
//   k_blind_rotate_x1     one wave per gate            more than 4 gates per CU (round 4)
//   k_blind_rotate_w2     two waves per gate           1 .. 4 gates per CU
//   k_blind_rotate_wide   2L waves per gate            at most one gate per CU
// The pieces of a CMux step the kernels share (guard publication, digit conversion, row product, epilogue, ...) are in
// br_step.h, with the list of what each kernel still writes out itself and why.
// Kernels and template flags that lost their A/B: attic/ (not built by default).
#include "blind_rotate_w64.h"

#include <cstdio>
#include <algorithm>
#include <stdexcept>
#include <type_traits>
#include <vector>

#include "br_step.h"
#include "fft_probe.h"
#include "mix_plan.h"

namespace ieache {
namespace w64 {

using namespace dev;

namespace {

// ---- key preparation: BK polynomial -> two-limb spectrum in the w64 register/lane order ----
// bkf layout: [n][2L rows][q = 2*c + limb][k2 = 8][lane = 64]
__global__ __launch_bounds__(64) void k_bk_to_spectrum_w64(const Torus32* bk_raw, double2* bkf) {
    __shared__ __align__(16) double2 sT[kTile];
    __shared__ __align__(16) double2 sTw[kTwElems];
    const int lane = threadIdx.x;
    build_twiddles(sTw, lane, 64);
    __syncthreads();
    const LaneRoots R = make_roots(sTw, lane);
    const size_t poly = blockIdx.x;  // (i * 2L + row) * 2 + c
    const Torus32* src = bk_raw + poly * kN;
    const size_t irow = poly >> 1, c = poly & 1;
#pragma unroll 1
    for (int limb = 0; limb < 2; limb++) {
        double2 x[8];
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const int32_t v0 = src[64 * r + lane], v1 = src[64 * r + lane + kM];
            const int32_t lo0 = (int16_t)(v0 & 0xFFFF), lo1 = (int16_t)(v1 & 0xFFFF);
            const int32_t e0 = limb ? (int32_t)(((int64_t)v0 - lo0) >> 16) : lo0;
            const int32_t e1 = limb ? (int32_t)(((int64_t)v1 - lo1) >> 16) : lo1;
            x[r] = make_double2((double)e0, (double)e1);  // untwisted: the first radix-8 pass applies e^{i pi r/16} itself
        }
        fft512_forward<true>(x, sT, lane, R);
        double2* dst = bkf + ((irow * 4 + c * 2 + limb) * 8) * 64 + lane;
#pragma unroll
        for (int k2 = 0; k2 < 8; k2++) dst[k2 * 64] = x[k2];
    }
}

// ---- key preparation, one-limb form: BK polynomial -> spectrum of its 32-bit coefficients ----
// bkf1 layout: [n][2L rows][c = 2][k2 = 8][lane = 64]   (half the two-limb form: 61.9 MB at n = 630)
__global__ __launch_bounds__(64) void k_bk_to_spectrum_w64_1(const Torus32* bk_raw, double2* bkf1) {
    __shared__ __align__(16) double2 sT[kTile];
    __shared__ __align__(16) double2 sTw[kTwElems];
    const int lane = threadIdx.x;
    build_twiddles(sTw, lane, 64);
    __syncthreads();
    const LaneRoots R = make_roots(sTw, lane);
    const size_t poly = blockIdx.x;  // (i * 2L + row) * 2 + c
    const Torus32* src = bk_raw + poly * kN;
    double2 x[8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const double2 v = make_double2((double)src[64 * r + lane], (double)src[64 * r + lane + kM]);
        x[r] = v;
    }
    fft512_forward<true>(x, sT, lane, R);
    double2* dst = bkf1 + (poly * 8) * 64 + lane;
#pragma unroll
    for (int k2 = 0; k2 < 8; k2++) dst[k2 * 64] = x[k2];
}

// ---- K0..K2: gate pre-combination, mod-switch, test-vector init ----
// One 128-thread workgroup per gate instance.  Writes the rotation amounts
// bara[n] (u16, row stride nb) and the initial accumulator [2][1024] to the
// blind-rotation state in HBM, from where the sliced kernel below picks up.
// TV: a programmable bootstrap -- the accumulator starts from the item's row of W.tv (device_common.h) instead of the constant
// polynomial; the TV = false build is the gate path's prologue, instruction for instruction what it was without the template.
template <bool TV>
__global__ __launch_bounds__(128) void k_br_prologue(DevKeys K, WorkDesc W, uint16_t* st_bara, int32_t nb, int32_t* st_acc) {
    __shared__ int32_t s_barb;
    const int tid = threadIdx.x;
    const int32_t n = K.n;
    const int64_t item = (int64_t)blockIdx.x;
    const GateInst g = resolve(W, W.item0 + item, K.stride);
    uint16_t* bara = st_bara + (size_t)item * nb;
    for (int32_t i = tid; i <= n; i += 128) {
        const int32_t bar = modswitch2N(combined_coef(g, i, n), 11);
        if (i < n)
            bara[i] = (uint16_t)bar;
        else
            s_barb = bar;
    }
    __syncthreads();
    // acc = (0, X^{2N-barb} * (mu,...,mu)), or (0, X^{2N-barb} * v) for the item's test polynomial v
    const int32_t a0 = (2 * kN - s_barb) & (2 * kN - 1);
    int32_t* acc = st_acc + (size_t)item * 2 * kN;
    const Torus32* v = TV ? test_poly_row(W, W.item0 + item, kN) : nullptr;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int32_t j = 128 * r + tid;
        acc[j] = 0;
        if (TV)
            acc[kN + j] = rot_coef(v, j, a0, kN);
        else
            acc[kN + j] = ((j - a0) & (2 * kN - 1)) < kN ? kMU : -kMU;
    }
}

// The third build: a programmable bootstrap from a table of TLWE samples (W.flat_type == kFlatRawTlwe, rows of 2N words, A
// then B) -- the accumulator starts from X^{2N-barb} * (A, B), both halves rotated by the same amount with the same rule.  A
// kernel of its own, so that the two builds above keep their names and their code.
__global__ __launch_bounds__(128) void k_br_prologue_tlwe(DevKeys K, WorkDesc W, uint16_t* st_bara, int32_t nb, int32_t* st_acc) {
    __shared__ int32_t s_barb;
    const int tid = threadIdx.x;
    const int32_t n = K.n;
    const int64_t item = (int64_t)blockIdx.x;
    const GateInst g = resolve(W, W.item0 + item, K.stride);
    uint16_t* bara = st_bara + (size_t)item * nb;
    for (int32_t i = tid; i <= n; i += 128) {
        const int32_t bar = modswitch2N(combined_coef(g, i, n), 11);
        if (i < n)
            bara[i] = (uint16_t)bar;
        else
            s_barb = bar;
    }
    __syncthreads();
    const int32_t a0 = (2 * kN - s_barb) & (2 * kN - 1);
    int32_t* acc = st_acc + (size_t)item * 2 * kN;
    const Torus32* v = test_poly_row(W, W.item0 + item, 2 * kN);
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int32_t j = 128 * r + tid;
        acc[j] = rot_coef(v, j, a0, kN);
        acc[kN + j] = rot_coef(v + kN, j, a0, kN);
    }
}

// ---- K3 (+K4): CMux steps [i0, i1) for every gate instance of the launch ----
// One 128-thread workgroup (two waves) per gate instance.  The step index is the
// OUTER loop of the evaluator: a chunk of gates is advanced S steps per launch, so
// all resident workgroups read the same S blocks BK_i0..BK_i1 while those are hot
// in the XCD's L2 (with the whole blind rotation in one launch, workgroups drift
// apart in i and each streams its own BK_i from Infinity Cache/HBM: measured 51 MB
// of fetch per gate).  The accumulator lives in HBM between launches (8 KB per gate).
// Wave w decomposes accumulator polynomial w (its 3 digit rows -> 3 forward
// transforms), owns the spectrum-domain sums of OUTPUT polynomial w (both
// limbs) and inverse-transforms them.  Each forward spectrum is handed to the
// partner wave through the producing wave's own (then idle) transpose tile.
// dynamic LDS: sT [2][kTile] double2 | tw [kTwElems] double2 | acc [2][1024] int32
// XLANE = 1: the forward transforms' lane-high transpose cross-lane (the default); 0: every transpose through LDS (round 1)
template <int L, int BGBIT, int XLANE = 1>
__global__ __launch_bounds__(128, 2) void k_blind_rotate_w2(DevKeys K, const double2* __restrict__ bkf,
                                                           const uint16_t* __restrict__ st_bara, int32_t nb,
                                                           int32_t* st_acc, int32_t i0, int32_t i1, Torus32* ext,
                                                           const double2* __restrict__ gtw) {
    extern __shared__ __align__(16) unsigned char smem[];
    double2* sT_all = reinterpret_cast<double2*>(smem);
    double2* sTw = sT_all + 2 * kTile;
    int32_t* acc = reinterpret_cast<int32_t*>(sTw + kTwElems);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double2* sT = sT_all + wave * kTile;
    const double2* sTp = sT_all + (wave ^ 1) * kTile;
    const int64_t item = (int64_t)blockIdx.x;
    const uint16_t* __restrict__ bara = st_bara + (size_t)item * nb;
    int32_t* gacc = st_acc + (size_t)item * 2 * kN;
    load_twiddles(sTw, gtw, tid, 128);
    const LaneRoots R = make_roots(sTw, lane);
    copy_acc<128>(acc, gacc, tid);
    __syncthreads();

    uint32_t dec_offset = decomposition_offset<L, BGBIT>();
    int32_t* accw = acc + wave * kN;  // the polynomial this wave decomposes and updates

    // this slice's rotation amounts: one per lane, fetched once, then read with readlane
    // (a dependent global load at the head of every step costs ~2-3k cycles)
    const int32_t my_a = lane_amounts(bara, i0, i1, lane);
#pragma unroll 1
    for (int32_t i = i0; i < i1; i++) {
        const int32_t a = __builtin_amdgcn_readlane(my_a, i - i0);
        if (a == 0) continue;  // workgroup-uniform; exact arithmetic makes the step a no-op
        // BK_i rows [2L][4][8][64]; this wave reads outputs o = 2*wave, 2*wave+1 of every row
        const double2* __restrict__ bki = bkf + (size_t)i * (2 * L * 4 * kM) + (size_t)(2 * wave) * kM + lane;
        double2 s[2][8];  // written (not accumulated into) by digit 0's own-row products below
        // (X^a - 1) * acc_w at this lane's 16 coefficients, plus the decomposition offset
        uint32_t v0[8], v1[8];
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const int32_t j = 64 * r + lane;
            // (x + C) ^ C with C = sum_q halfBg << shift_q: digit q's field then holds digit ^ halfBg, whose
            // sign-extended BGBIT-bit value IS digit - halfBg (one v_bfe_i32 per digit below)
            v0[r] = (((uint32_t)rot_coef(accw, j, a, kN) - (uint32_t)accw[j]) + dec_offset) ^ dec_offset;
            v1[r] = (((uint32_t)rot_coef(accw, j + kM, a, kN) - (uint32_t)accw[j + kM]) + dec_offset) ^ dec_offset;
        }
        auto digit_row = [&](const int q, auto first) {
            constexpr bool FIRST = decltype(first)::value;  // digit 0: its own-row products initialise s
            const int sh = 32 - (q + 1) * BGBIT;
            const double2* __restrict__ bown = bki + (size_t)(wave * L + q) * (4 * kM);
            const double2* __restrict__ bpar = bki + (size_t)((wave ^ 1) * L + q) * (4 * kM);
            double2 x[8];
            digits_to_double2<BGBIT>(x, v0, v1, sh);
            // BK loads are issued well ahead of their use (each is an L2 round trip of ~700 cycles):
            //   bA = own row, limb 0      before the transform
            //   bB = own row, limb 1      } right after it, consumed behind bA's MACs
            //   bC = partner row, limb 0  }
            //   bD = partner row, limb 1  after bA is consumed (reuses its registers)
            double2 bA[8], bB[8], bC[8];
#pragma unroll
            for (int k = 0; k < 8; k++) bA[k] = bown[k * 64];
            __builtin_amdgcn_sched_barrier(0);
            fft512_forward<true, XLANE>(x, sT, lane, R);
            // hand the spectrum to the partner wave through our own (now idle) tile
#pragma unroll
            for (int k = 0; k < 8; k++) sT[k * 64 + lane] = x[k];
#pragma unroll
            for (int k = 0; k < 8; k++) bB[k] = bown[(8 + k) * 64];
#pragma unroll
            for (int k = 0; k < 8; k++) bC[k] = bpar[k * 64];
            __builtin_amdgcn_sched_barrier(0);
            mac_row<FIRST>(s[0], x, bA);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < 8; k++) bA[k] = bpar[(8 + k) * 64];  // bD
            __builtin_amdgcn_sched_barrier(0);
            mac_row<FIRST>(s[1], x, bB);
            __syncthreads();
            // partner's row
#pragma unroll
            for (int k = 0; k < 8; k++) x[k] = sTp[k * 64 + lane];
            mac_row<false>(s[0], x, bC);
            mac_row<false>(s[1], x, bA);
            __syncthreads();  // partner has read our tile before the next transform reuses it
        };
        digit_row(0, std::true_type{});
#pragma unroll 1
        for (int q = 1; q < L; q++) digit_row(q, std::false_type{});
        // back to coefficients, round, recombine the two limbs, accumulate into polynomial `wave`
        fft512_inverse_pair<true>(s[0], s[1], sT, lane, R);
#pragma unroll
        for (int r = 0; r < 8; r++) {
            double unused = 0.0;
            const uint32_t l0 = round_coef(s[0][r].x, untwist_gain(r), false, unused), l1 = round_coef(s[0][r].y, untwist_gain(r), false, unused);
            const uint32_t h0 = round_coef(s[1][r].x, untwist_gain(r), false, unused), h1 = round_coef(s[1][r].y, untwist_gain(r), false, unused);
            const int32_t j = 64 * r + lane;
            accw[j] = (int32_t)((uint32_t)accw[j] + l0 + (h0 << 16));
            accw[j + kM] = (int32_t)((uint32_t)accw[j + kM] + l1 + (h1 << 16));
        }
        // wave w reads and updates only polynomial w, and the partner is done with this wave's tile since the
        // last digit's second barrier: nothing crosses waves here, so no barrier (round 1's cost 0.3-0.4 %)
    }
    __syncthreads();  // the epilogue below reads both polynomials with all threads
    finish_slice<128>(ext, item, acc, gacc, tid);
}


// ---- K3 (+K4), throughput form (rounds 2-3): ONE wave per gate instance on the ONE-limb spectrum ----
// The two-limb product (k_blind_rotate_x1 / _w2 / _wide below) is exact by construction (every rounded sum stays below 2^35
// of the 2^53 an FP64 mantissa holds) and pays for it with a second inverse transform and a second set of row products per
// output polynomial.  libtfhe itself multiplies with ONE double-precision transform of the 32-bit coefficients; the sums then
// reach 2^49.6 in the worst case and ~2^43 on real data, where the transform's rounding error is ~2^-9 of an integer step
// (largest seen: 0.0156) -- far from the 0.5 that would change a rounded coefficient, but not provably so.
// This kernel takes that form and WATCHES the error: the distance to the nearest integer of inverse-transformed coefficients
// is folded into a running maximum, published per launch (guard[1], float bits) and counted (guard[0]) when it exceeds
// kGuardLimit; the evaluator then repeats the call on the two-limb kernels, and audits a sample of every K-th launch bit for
// bit (evaluator.hip).  With 6 forward + 2 inverse transforms and 12 row products per step the whole step fits ONE wave: no
// spectra cross waves, the step has no workgroup barrier at all, and a SIMD's two resident waves belong to unrelated gates
// that never wait for each other.  Four gates share a workgroup only for the twiddle table.
//   * the accumulators stand FIRST in the workgroup's LDS, each polynomial on a 4 KiB boundary, so the byte address of
//     coefficient (j - a) mod N is one v_and_or_b32 of a per-step lane value plus 256 r, and the address of coefficient
//     j + 512 is that address ^ 2048; the negacyclic sign is a v_bfe_i32 of the same per-step value;
//   * (X^a - 1) acc + offset is formed as (rot ^ m) + ((offset - acc_j) - m)  (v_xad_u32);
//   * BK_i through buffer loads: the first block of a row requested inside its forward transform, once the first twiddle
//     set's 32 registers are free (fft512_forward's MID hook), the second behind the transform;
//   * second inter-pass twiddles resident for the whole kernel (fft512.h): the four odd ones, signed, for the forward
//     transforms (XLANE = 2 below: a forward transform reads 11 twiddles from the LDS table instead of 15), or six of the
//     seven for both directions (XLANE = 1: 9 instead of 15; all seven do not fit: the <3,7> builds then spill 5 VGPRs);
//   * the unrotated operands of a decomposition are read back from LDS, which the compiler pairs as ds_read2st64_b32;
//     carrying polynomial 0's from the update (ds_add_rtn_u32) measured within noise and is not kept;
//   * the rounding guard's running maximum between steps is a float (what is published; rounding is monotone, so the
//     figure is the same), and the epilogue forms its addresses again instead of sharing the prologue's: with these the
//     kernel holds 256 VGPRs without scratch;
//   * the forward transforms' lane-high transpose cross-lane, every other transpose through the gate's padded LDS tile; the
//     two inverse transforms interleaved through that one tile; ds_add_u32 update;
//   * XLANE = 2: that transpose in the exchange form (fft512.h): lane bit 3 at one v_mov_b32_dpp per dword instead of two
//     v_cndmask_b32_dpp, 96 vector instructions fewer per step (3 143 -> 3 047, profiles/xlane3_isa_mix.txt).  A lane then
//     gathers the inputs of the relabelled position xl_pi(lane) -- the decomposition reads through `plane`, the update behind
//     the inverse transforms stays in the lanes' own order -- and holds two signed cosines, a second table base and a second
//     tile base across the step loop.  For those registers only the four ODD second twiddles are resident (LaneRootsExchange,
//     16 VGPRs), with the form's per-lane sign, so the inverse pair reads the whole set from the table: 321 LDS instructions
//     per step against 303, and every ds_read_b32 of the decomposition is a 2-way bank conflict (lanes l and l ^ 8 gather
//     dwords 32 apart).  Still +1.6 % (profiles/xlane3_ab.txt).  With one even entry resident as well the <3,7> builds spill
//     6 VGPRs.  XLANE = 1: v_cndmask_b32_dpp pairs and six resident twiddles (LaneRootsResident), the form before;
//   * GUARD = 2 watches ONE rounded coefficient in four (registers r = 0 and r = 4 of both output polynomials), 1 every one,
//     0 none (measurement only); DIAG: s_memtime phase stamps on stderr (br_variant 49).
// Measured and dropped (profiles/r3_w1_ab.txt; source in git history, see attic/README.md): software-pipelined rows, both
// forward transposes cross-lane, twiddles through the buffer path, an L2 prefetch of the next step's BK blocks.
// dynamic LDS: acc [4][2][1024] int32 | sT [4][kTile] double2 | tw [kTwElems] double2          (78 848 B -> 2 per CU)
template <int L, int BGBIT, int GUARD, bool DIAG = false, int G = kW1Gates, int XLANE = 2>
__global__ __launch_bounds__(64 * G, 2) void k_blind_rotate_w1b(DevKeys K, const double2* __restrict__ bkf1,
                                                                       const uint16_t* __restrict__ st_bara, int32_t nb,
                                                                       int32_t* st_acc, int64_t items, int32_t i0, int32_t i1,
                                                                       Torus32* ext, unsigned* guard,
                                                                       const double2* __restrict__ gtw, unsigned long long* diag = nullptr) {
    extern __shared__ __align__(16) unsigned char smem[];
    int32_t* acc_all = reinterpret_cast<int32_t*>(smem);
    double2* sT_all = reinterpret_cast<double2*>(smem + (size_t)G * 2 * kN * 4);
    double2* sTw = sT_all + G * kTile;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double2* sT = sT_all + wave * kTile;
    int32_t* acc = acc_all + wave * 2 * kN;
    const int64_t item = (int64_t)blockIdx.x * G + wave;
    static_assert(XLANE == 1 || XLANE == 2, "the forward transforms' lane-high transpose: v_cndmask pairs (1) or the exchange form (2)");
    using Roots = typename std::conditional<XLANE == 2, LaneRootsExchange, LaneRootsResident>::type;
    load_twiddles(sTw, gtw, tid, 64 * G);
    __syncthreads();  // the only workgroup barrier
    if (item >= items) return;
    const Roots R = make_roots<Roots>(sTw, lane);  // resident second twiddles: 16 VGPRs (XLANE = 2) or 24 for the whole kernel
    // the position whose inputs this lane gathers: the exchange form takes them relabelled (tw_roots.h); the update below, behind
    // the inverse transforms, is in the lanes' own order either way
    const int plane = XLANE == 2 ? xl_pi(lane) : lane;
    const uint16_t* __restrict__ bara = st_bara + (size_t)item * nb;
    int32_t* gacc = st_acc + (size_t)item * 2 * kN;
    {
        const int4* src = reinterpret_cast<const int4*>(gacc);
        int4* dst = reinterpret_cast<int4*>(acc);
#pragma unroll
        for (int r = 0; r < 8; r++) dst[64 * r + lane] = src[64 * r + lane];
    }
    wave_sync();

    constexpr uint32_t halfBg = 1u << (BGBIT - 1);
    uint32_t dec_offset = 0;
#pragma unroll
    for (int q = 1; q <= L; q++) dec_offset += halfBg << (32 - q * BGBIT);
    // the launch's largest distance is published as a float: kept as one between steps (rounding is monotone, so the
    // maximum of the rounded distances is the rounded maximum), one VGPR instead of two across the step loop
    float dev_maxf = 0.0f;
    constexpr int kRowBytes = 2 * kM * (int)sizeof(double2), kStepBytes = 2 * L * kRowBytes;
    const __amdgpu_buffer_rsrc_t bk_rsrc = bk_resource(bkf1, K.n, kStepBytes);
    const int lane16 = bk_lane_offset(lane);
    const unsigned char* accb = reinterpret_cast<const unsigned char*>(acc_all);  // LDS offset 0 of the workgroup
    const uint32_t pb0 = (uint32_t)wave * (2 * kN * 4);                            // this gate's polynomial 0; polynomial 1 at + 4096

    unsigned long long tsum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tlast = 0;
    if (DIAG) tlast = stamp();
    const int32_t my_a = lane_amounts(bara, i0, i1, lane);
#pragma unroll 1
    for (int32_t i = i0; i < i1; i++) {
        const int32_t a = __builtin_amdgcn_readlane(my_a, i - i0);
        if (a == 0) continue;  // wave-uniform; exact arithmetic makes the step a no-op
        const int bki = i * kStepBytes;
        double2 s[2][8];
        uint32_t v0[8], v1[8];
        double dev_max = 0.0;  // of this step
        // byte offset of coefficient (lane - a) in the 2N-ring [acc, -acc]: bits 2..11 address, bit 12 = negate
        const uint32_t jb4 = ((uint32_t)(plane - a) & (2 * kN - 1)) << 2;
        auto decompose = [&](const uint32_t pb) {
            const int32_t* accp = reinterpret_cast<const int32_t*>(accb + pb);
            decompose_rotated(v0, v1, accb, accp, pb, jb4, plane, dec_offset);
        };
        auto digit_row = [&](const int sh, const int brow, auto first) {
            constexpr bool FIRST = decltype(first)::value;
            double2 x[8], bA[8], bB[8];
            // the first block of the row is requested once the first twiddle set's 32 registers are free (the resident second
            // set has taken the room the request used to have before the transform); passes 2 and 3 cover its latency
            auto request_a = [&]() { load_bk_block(bA, bk_rsrc, lane16, brow); };
            digits_to_double2<BGBIT>(x, v0, v1, sh);
            __builtin_amdgcn_sched_barrier(0);
            stamp_phase<DIAG>(tsum, tlast, 1);
            fft512_forward<true, XLANE>(x, sT, lane, R, request_a);
            stamp_phase<DIAG>(tsum, tlast, 2);
            load_bk_block(bB, bk_rsrc, lane16, brow + kRowBytes / 2);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < 8; k++) s[0][k] = mac<FIRST>(s[0][k], x[k], bA[k]);
#pragma unroll
            for (int k = 0; k < 8; k++) s[1][k] = mac<FIRST>(s[1][k], x[k], bB[k]);
            stamp_phase<DIAG>(tsum, tlast, 3);
        };
        decompose(pb0);
        stamp_phase<DIAG>(tsum, tlast, 0);
        digit_row(32 - BGBIT, bki, std::true_type{});
#pragma unroll 1
        for (int row = 1; row < L; row++) digit_row(32 - (row + 1) * BGBIT, bki + row * kRowBytes, std::false_type{});
        decompose(pb0 + 4096u);
        stamp_phase<DIAG>(tsum, tlast, 0);
#pragma unroll 1
        for (int row = L; row < 2 * L; row++) digit_row(32 - (row - L + 1) * BGBIT, bki + row * kRowBytes, std::false_type{});
        fft512_inverse_pair<true>(s[0], s[1], sT, lane, R);
        stamp_phase<DIAG>(tsum, tlast, 4);
#pragma unroll
        for (int c = 0; c < 2; c++) {
            uint32_t* accc = reinterpret_cast<uint32_t*>(acc) + c * kN;
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const bool watched = GUARD == 1 || (GUARD == 2 && (r & 3) == 0);
                const uint32_t d0 = round_coef(s[c][r].x, untwist_gain(r), watched, dev_max), d1 = round_coef(s[c][r].y, untwist_gain(r), watched, dev_max);
                const int32_t j = 64 * r + lane;
                // ds_add_u32 (no return): one LDS instruction instead of read, add, write
                __hip_atomic_fetch_add(&accc[j], d0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                __hip_atomic_fetch_add(&accc[j + kM], d1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            }
        }
        if (GUARD) dev_maxf = fmaxf(dev_maxf, (float)dev_max);
        wave_sync();
        stamp_phase<DIAG>(tsum, tlast, 5);
    }
    if (DIAG && diag && lane == 0) {
#pragma unroll
        for (int t = 0; t < 8; t++) atomicAdd(&diag[(wave & 1) * 8 + t], tsum[t]);
    }
    // the epilogue forms its addresses from the lane number again: shared with the prologue's they would be 12 VGPRs held
    // across the step loop, which has none to spare
    int elane = lane;
    asm volatile("" : "+v"(elane));
    if (GUARD) publish_guard((double)dev_maxf, guard, elane);
    finish_slice<64>(ext, item, acc, gacc, elane);
}

// ---- K3 (+K4), throughput form of the PROVABLY EXACT product, round 4: one wave per gate on the TWO-limb spectrum ----
// k_blind_rotate_w2 (above) gives the two-limb product -- BK split into balanced 16-bit limbs, every rounded sum below 2^35
// of the 2^53 an FP64 mantissa holds, so rounding recovers the integer whatever the transform's schedule -- to two waves
// per gate that exchange every forward spectrum through LDS: six workgroup barriers per CMux step.  This is that product on
// k_blind_rotate_w1b's mapping: ONE wave owns a gate, four gates share a workgroup for the twiddle table only, no barrier
// and nothing crossing waves inside a step, BK through buffer loads with the block index in the scalar offset, accumulators
// first in LDS on 4 KiB boundaries (rotation address = one v_and_or of a per-step lane value), ds_add_u32 update.
// Per step and gate: 2L forward transforms (the digits, as in the one-limb kernels), 4 x 2L row products into FOUR
// spectrum sums s[2 c + limb] (128 VGPRs), four inverse transforms (two interleaved pairs through the gate's one tile),
// the two limbs of an output recombined as lo + (hi << 16) mod 2^32.  With the sums taking half the register file, only two
// BK blocks are in flight at a time: block 0 of a row is requested inside its forward transform (once the second twiddle
// set is consumed), block q + 2 when block q has been multiplied; the second decomposition's addresses and sign masks are
// recomputed rather than kept from the first (46 registers).  No guard: nothing here can round wrongly.
// dynamic LDS as k_blind_rotate_w1b: acc [4][2][1024] int32 | sT [4][kTile] double2 | tw [kTwElems] double2   (78 848 B -> 2 per CU)
template <int L, int BGBIT, int G = kW1Gates>
__global__ __launch_bounds__(64 * G, 2) void k_blind_rotate_x1(DevKeys K, const double2* __restrict__ bkf,
                                                                      const uint16_t* __restrict__ st_bara, int32_t nb,
                                                                      int32_t* st_acc, int64_t items, int32_t i0, int32_t i1,
                                                                      Torus32* ext, const double2* __restrict__ gtw) {
    extern __shared__ __align__(16) unsigned char smem[];
    int32_t* acc_all = reinterpret_cast<int32_t*>(smem);
    double2* sT_all = reinterpret_cast<double2*>(smem + (size_t)G * 2 * kN * 4);
    double2* sTw = sT_all + G * kTile;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double2* sT = sT_all + wave * kTile;
    int32_t* acc = acc_all + wave * 2 * kN;
    const int64_t item = (int64_t)blockIdx.x * G + wave;
    load_twiddles(sTw, gtw, tid, 64 * G);
    __syncthreads();  // the only workgroup barrier
    if (item >= items) return;
    const LaneRoots R = make_roots(sTw, lane);
    const uint16_t* __restrict__ bara = st_bara + (size_t)item * nb;
    int32_t* gacc = st_acc + (size_t)item * 2 * kN;
    {
        const int4* src = reinterpret_cast<const int4*>(gacc);
        int4* dst = reinterpret_cast<int4*>(acc);
#pragma unroll
        for (int r = 0; r < 8; r++) dst[64 * r + lane] = src[64 * r + lane];
    }
    wave_sync();

    constexpr uint32_t halfBg = 1u << (BGBIT - 1);
    uint32_t dec_offset = 0;
#pragma unroll
    for (int q = 1; q <= L; q++) dec_offset += halfBg << (32 - q * BGBIT);
    constexpr int kBlockBytes = kM * (int)sizeof(double2), kRowBytes = 4 * kBlockBytes, kStepBytes = 2 * L * kRowBytes;
    const __amdgpu_buffer_rsrc_t bk_rsrc = bk_resource(bkf, K.n, kStepBytes);
    const int lane16 = bk_lane_offset(lane);
    const unsigned char* accb = reinterpret_cast<const unsigned char*>(acc_all);  // LDS offset 0 of the workgroup
    const uint32_t pb0 = (uint32_t)wave * (2 * kN * 4);                            // this gate's polynomial 0; polynomial 1 at + 4096

    const int32_t my_a = lane_amounts(bara, i0, i1, lane);
#pragma unroll 1
    for (int32_t i = i0; i < i1; i++) {
        const int32_t a = __builtin_amdgcn_readlane(my_a, i - i0);
        if (a == 0) continue;  // wave-uniform; exact arithmetic makes the step a no-op
        const int bki = i * kStepBytes;  // BK_i rows [2L][q = 2 c + limb][8][64] double2
        double2 s[4][8];
        uint32_t v0[8], v1[8];
        // byte offset of coefficient (lane - a) in the 2N-ring [acc, -acc]: bits 2..11 address, bit 12 = negate
        const uint32_t jb4 = ((uint32_t)(lane - a) & (2 * kN - 1)) << 2;
        auto decompose = [&](const uint32_t pb, const uint32_t jb) {
            const int32_t* accp = reinterpret_cast<const int32_t*>(accb + pb);
            decompose_rotated(v0, v1, accb, accp, pb, jb, lane, dec_offset);
        };
        auto digit_row = [&](const int sh, const int brow, auto first) {
            digit_row_two_limb<BGBIT, decltype(first)::value>(s, v0, v1, sh, bk_rsrc, lane16, brow, sT, lane, R);
        };
        decompose(pb0, jb4);
        digit_row(32 - BGBIT, bki, std::true_type{});
#pragma unroll 1
        for (int row = 1; row < L; row++) digit_row(32 - (row + 1) * BGBIT, bki + row * kRowBytes, std::false_type{});
        // opaque copy: the addresses and sign masks of the second decomposition are recomputed (~50 integer instructions) rather
        // than kept from the first one across three digit rows -- 46 registers this kernel does not have (they were spilled)
        uint32_t jb4b = jb4;
        asm volatile("" : "+v"(jb4b));
        decompose(pb0 + 4096u, jb4b);
#pragma unroll 1
        for (int row = L; row < 2 * L; row++) digit_row(32 - (row - L + 1) * BGBIT, bki + row * kRowBytes, std::false_type{});
        // back to coefficients: s[2 c] / s[2 c + 1] hold the low / high limb sums of output polynomial c
#pragma unroll
        for (int c = 0; c < 2; c++) {
            fft512_inverse_pair<true>(s[2 * c], s[2 * c + 1], sT, lane, R);
            uint32_t* accc = reinterpret_cast<uint32_t*>(acc) + c * kN;
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const uint32_t d0 = join_limbs(s[2 * c][r].x, s[2 * c + 1][r].x, r), d1 = join_limbs(s[2 * c][r].y, s[2 * c + 1][r].y, r);
                const int32_t j = 64 * r + lane;
                __hip_atomic_fetch_add(&accc[j], d0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                __hip_atomic_fetch_add(&accc[j + kM], d1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            }
        }
        wave_sync();
    }
    finish_slice<64>(ext, item, acc, gacc, lane);
}

// ---- K3 (+K4), mid-size launches, round 3: two waves per gate, the ROWS split between them ----
// k_blind_rotate_w2s (below) splits a gate by OUTPUT polynomial: wave w owns output w, so each of its three forward
// spectra has to reach the partner through LDS -- two workgroup barriers per digit row, six per step, and a lone wave per
// SIMD spends them waiting.  Here the split is by ROW of BK_i: wave w decomposes accumulator polynomial w, transforms its
// three digits and multiplies each with BOTH output blocks of its own rows (k_blind_rotate_w1's digit row, three times
// instead of six), keeping two partial spectrum sums.  Only then do the waves meet: each hands the partial sum of the
// OTHER output to its partner through its own (idle) tile, adds what it receives, inverse-transforms output w and updates
// accumulator polynomial w -- two barriers per step.  The next step's decomposition reads polynomial w only, so nothing
// else crosses waves.  Arithmetic differs from k_blind_rotate_w1 only in the order of two exact-after-rounding FP64 sums.
// dynamic LDS: acc [2][1024] int32 | sT [2][kTile] double2 | tw [kTwElems] double2       (35 840 B -> 4 per CU)
template <int L, int BGBIT, int GUARD>
__global__ __launch_bounds__(128, 2) void k_blind_rotate_w2r(DevKeys K, const double2* __restrict__ bkf1,
                                                            const uint16_t* __restrict__ st_bara, int32_t nb,
                                                            int32_t* st_acc, int32_t i0, int32_t i1, Torus32* ext,
                                                            unsigned* guard, const double2* __restrict__ gtw) {
    extern __shared__ __align__(16) unsigned char smem[];
    int32_t* acc = reinterpret_cast<int32_t*>(smem);
    double2* sT_all = reinterpret_cast<double2*>(smem + (size_t)2 * kN * 4);
    double2* sTw = sT_all + 2 * kTile;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double2* sT = sT_all + wave * kTile;
    const double2* sTp = sT_all + (wave ^ 1) * kTile;
    const int64_t item = (int64_t)blockIdx.x;
    const uint16_t* __restrict__ bara = st_bara + (size_t)item * nb;
    int32_t* gacc = st_acc + (size_t)item * 2 * kN;
    load_twiddles(sTw, gtw, tid, 128);
    const LaneRoots R = make_roots(sTw, lane);
    {
        const int4* src = reinterpret_cast<const int4*>(gacc);
        int4* dst = reinterpret_cast<int4*>(acc);
#pragma unroll
        for (int r = 0; r < 4; r++) dst[128 * r + tid] = src[128 * r + tid];
    }
    __syncthreads();

    constexpr uint32_t halfBg = 1u << (BGBIT - 1);
    uint32_t dec_offset = 0;
#pragma unroll
    for (int q = 1; q <= L; q++) dec_offset += halfBg << (32 - q * BGBIT);
    double dev_max = 0.0;
    constexpr int kRowBytes = 2 * kM * (int)sizeof(double2), kStepBytes = 2 * L * kRowBytes;
    const __amdgpu_buffer_rsrc_t bk_rsrc = bk_resource(bkf1, K.n, kStepBytes);
    const int lane16 = bk_lane_offset(lane);
    const unsigned char* accb = reinterpret_cast<const unsigned char*>(acc);  // LDS offset 0 of the workgroup
    const uint32_t pb = (uint32_t)wave * (kN * 4);                             // this wave's polynomial
    const int32_t* accp = acc + wave * kN;
    uint32_t* accu = reinterpret_cast<uint32_t*>(acc) + wave * kN;

    int32_t my_a = 0;  // the rotation amounts of 64 steps at a time, one per lane (a launch may be the whole rotation)
#pragma unroll 1
    for (int32_t i = i0; i < i1; i++) {
        if (((i - i0) & 63) == 0) my_a = (i + lane < i1) ? (int32_t)bara[i + lane] : 0;
        const int32_t a = __builtin_amdgcn_readlane(my_a, (i - i0) & 63);
        if (a == 0) continue;  // workgroup-uniform
        const int bki = i * kStepBytes + wave * L * kRowBytes;  // this wave's rows of BK_i
        double2 s[2][8];
        uint32_t v0[8], v1[8];
        const uint32_t jb4 = ((uint32_t)(lane - a) & (2 * kN - 1)) << 2;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const uint32_t t = jb4 + 256u * r;
            const uint32_t o0 = (t & 4092u) | pb, o1 = o0 ^ 2048u;
            const int32_t m0 = __builtin_amdgcn_sbfe((int32_t)t, 12, 1), m1 = __builtin_amdgcn_sbfe((int32_t)(t + 2048u), 12, 1);
            const uint32_t rv0 = *reinterpret_cast<const uint32_t*>(accb + o0), rv1 = *reinterpret_cast<const uint32_t*>(accb + o1);
            const uint32_t pv0 = (uint32_t)accp[64 * r + lane], pv1 = (uint32_t)accp[64 * r + lane + kM];
            v0[r] = ((rv0 ^ (uint32_t)m0) + ((dec_offset - pv0) - (uint32_t)m0)) ^ dec_offset;
            v1[r] = ((rv1 ^ (uint32_t)m1) + ((dec_offset - pv1) - (uint32_t)m1)) ^ dec_offset;
        }
        auto digit_row = [&](const int sh, const int brow, auto first) {
            constexpr bool FIRST = decltype(first)::value;
            double2 x[8], bA[8], bB[8];
            load_bk_block(bA, bk_rsrc, lane16, brow);
            digits_to_double2<BGBIT>(x, v0, v1, sh);
            __builtin_amdgcn_sched_barrier(0);
            fft512_forward<true, 1>(x, sT, lane, R);
            load_bk_block(bB, bk_rsrc, lane16, brow + kRowBytes / 2);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < 8; k++) s[0][k] = mac<FIRST>(s[0][k], x[k], bA[k]);
#pragma unroll
            for (int k = 0; k < 8; k++) s[1][k] = mac<FIRST>(s[1][k], x[k], bB[k]);
        };
        digit_row(32 - BGBIT, bki, std::true_type{});
#pragma unroll 1
        for (int q = 1; q < L; q++) digit_row(32 - (q + 1) * BGBIT, bki + q * kRowBytes, std::false_type{});
        // the partial sum of the partner's output goes to the partner through this wave's tile (idle since the last transform)
        double2 y[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const double2 mine = wave ? s[1][k] : s[0][k], theirs = wave ? s[0][k] : s[1][k];
            sT[k * 64 + lane] = theirs;
            y[k] = mine;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const double2 z = sTp[k * 64 + lane];
            y[k] = cadd(y[k], z);
        }
        __syncthreads();  // the partner has read this wave's tile before the inverse transform reuses it
        fft512_inverse<true>(y, sT, lane, R);
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const bool watched = GUARD == 1 || (GUARD == 2 && (r & 3) == 0);
            const uint32_t d0 = round_coef(y[r].x, untwist_gain(r), watched, dev_max), d1 = round_coef(y[r].y, untwist_gain(r), watched, dev_max);
            const int32_t j = 64 * r + lane;
            __hip_atomic_fetch_add(&accu[j], d0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            __hip_atomic_fetch_add(&accu[j + kM], d1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
        wave_sync();  // wave w reads and updates only polynomial w: nothing crosses waves here
    }
    __syncthreads();  // the epilogue below reads both polynomials with all threads
    if (GUARD) publish_guard(dev_max, guard, lane);
    finish_slice<128>(ext, item, acc, gacc, tid);
}

// ---- K3 (+K4), one to two gates per CU, round 3: FOUR waves per gate, the rows split 2 : 1 : 2 : 1 ----
// Launches of 257 .. 512 gate instances leave every SIMD a single wave under k_blind_rotate_w2r, and a lone wave issues a
// vector instruction only every 6-7 cycles.  Here a gate is one 256-thread workgroup (two per CU: two waves per SIMD):
//   wave 2p     ("heavy", polynomial p): digits 0 .. L-2 of accumulator polynomial p -- L-1 forward transforms, each
//               multiplied with BOTH output blocks of its BK row (two partial spectrum sums, as in k_blind_rotate_w1b);
//   wave 2p + 1 ("light"): digit L-1 the same way, then the inverse transform of OUTPUT polynomial p.
// One hand-over per step: every wave passes on the partial sums it does not invert -- through its own (idle) tile and,
// for the heavy waves' second sum, one of two extra 8 KiB slots -- barrier, the light waves add the three sums they
// receive, inverse-transform (scratch: the tile they have just emptied, which nobody else reads), round and ds_add_u32
// into "their" accumulator polynomial, barrier.  Arithmetic differs from the other kernels only in the order of exact-
// after-rounding FP64 sums.
// dynamic LDS: acc [2][1024] int32 | sT [4][kTile] double2 | X [2][8][64] double2 | tw [kTwElems] double2   (70 656 B -> 2 per CU)
template <int L, int BGBIT, int GUARD>
__global__ __launch_bounds__(256, 2) void k_blind_rotate_w4r(DevKeys K, const double2* __restrict__ bkf1,
                                                            const uint16_t* __restrict__ st_bara, int32_t nb,
                                                            int32_t* st_acc, int32_t i0, int32_t i1, Torus32* ext,
                                                            unsigned* guard, const double2* __restrict__ gtw, int32_t flip_period) {
    extern __shared__ __align__(16) unsigned char smem[];
    int32_t* acc = reinterpret_cast<int32_t*>(smem);
    double2* sT_all = reinterpret_cast<double2*>(smem + (size_t)2 * kN * 4);
    double2* sX = sT_all + 4 * kTile;
    double2* sTw = sX + 2 * 8 * 64;
    const int tid = threadIdx.x, lane = tid & 63;
    // The two workgroups that share a CU (observed: workgroup i and i + #CUs) swap the heavy and the light role within each
    // wave pair, so that every SIMD hosts one heavy and one light wave instead of two of a kind waiting for each other's phase.
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6) ^ (int)((blockIdx.x / (unsigned)flip_period) & 1u);
    const int pol = wave >> 1;
    const bool light = wave & 1;
    double2* sT = sT_all + wave * kTile;
    const int64_t item = (int64_t)blockIdx.x;
    const uint16_t* __restrict__ bara = st_bara + (size_t)item * nb;
    int32_t* gacc = st_acc + (size_t)item * 2 * kN;
    load_twiddles(sTw, gtw, tid, 256);
    const LaneRoots R = make_roots(sTw, lane);
    {
        const int4* src = reinterpret_cast<const int4*>(gacc);
        int4* dst = reinterpret_cast<int4*>(acc);
#pragma unroll
        for (int r = 0; r < 2; r++) dst[256 * r + tid] = src[256 * r + tid];
    }
    __syncthreads();

    constexpr uint32_t halfBg = 1u << (BGBIT - 1);
    uint32_t dec_offset = 0;
#pragma unroll
    for (int q = 1; q <= L; q++) dec_offset += halfBg << (32 - q * BGBIT);
    double dev_max = 0.0;
    constexpr int kRowBytes = 2 * kM * (int)sizeof(double2), kStepBytes = 2 * L * kRowBytes;
    const __amdgpu_buffer_rsrc_t bk_rsrc = bk_resource(bkf1, K.n, kStepBytes);
    const int lane16 = bk_lane_offset(lane);
    const unsigned char* accb = reinterpret_cast<const unsigned char*>(acc);
    const uint32_t pb = (uint32_t)pol * (kN * 4);
    const int32_t* accp = acc + pol * kN;
    uint32_t* accu = reinterpret_cast<uint32_t*>(acc) + pol * kN;
    const int q0 = light ? L - 1 : 0, q1 = light ? L : (L > 1 ? L - 1 : 1);  // this wave's digits [q0, q1)
    // where the partial sums go: `keep` stays (light waves: the output they invert), `give0` / `give1` are handed over
    //   wave 0: s[0] -> tile 0 (for wave 1), s[1] -> slot 0 (for wave 3)      wave 1: s[1] -> tile 1 (for wave 3)
    //   wave 2: s[1] -> tile 2 (for wave 3), s[0] -> slot 1 (for wave 1)      wave 3: s[0] -> tile 3 (for wave 1)
    double2* slot_extra = sX + pol * (8 * 64);
    const double2* in_a = light ? (pol == 0 ? sT_all + 0 * kTile : sX + 0 * (8 * 64)) : nullptr;        // wave 1: tile 0 ; wave 3: slot 0
    const double2* in_b = light ? (pol == 0 ? sX + 1 * (8 * 64) : sT_all + 1 * kTile) : nullptr;        // wave 1: slot 1 ; wave 3: tile 1
    const double2* in_c = light ? (pol == 0 ? sT_all + 3 * kTile : sT_all + 2 * kTile) : nullptr;       // wave 1: tile 3 ; wave 3: tile 2
    double2* scratch = sT_all + (pol == 0 ? 0 : 2) * kTile;  // the heavy partner's tile: after the hand-over only this light wave reads it

    int32_t my_a = 0;  // the rotation amounts of 64 steps at a time, one per lane (a launch may be the whole rotation)
#pragma unroll 1
    for (int32_t i = i0; i < i1; i++) {
        if (((i - i0) & 63) == 0) my_a = (i + lane < i1) ? (int32_t)bara[i + lane] : 0;
        const int32_t a = __builtin_amdgcn_readlane(my_a, (i - i0) & 63);
        if (a == 0) continue;  // workgroup-uniform
        const int bki = i * kStepBytes + pol * L * kRowBytes;  // the rows of this wave's polynomial
        double2 s[2][8];
        uint32_t v0[8], v1[8];
        const uint32_t jb4 = ((uint32_t)(lane - a) & (2 * kN - 1)) << 2;
        decompose_rotated(v0, v1, accb, accp, pb, jb4, lane, dec_offset);
        auto digit_row = [&](const int sh, const int brow, auto first) {
            constexpr bool FIRST = decltype(first)::value;
            double2 x[8], bA[8], bB[8];
            load_bk_block(bA, bk_rsrc, lane16, brow);
            digits_to_double2<BGBIT>(x, v0, v1, sh);
            __builtin_amdgcn_sched_barrier(0);
            fft512_forward<true, 1>(x, sT, lane, R);
            load_bk_block(bB, bk_rsrc, lane16, brow + kRowBytes / 2);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < 8; k++) s[0][k] = mac<FIRST>(s[0][k], x[k], bA[k]);
#pragma unroll
            for (int k = 0; k < 8; k++) s[1][k] = mac<FIRST>(s[1][k], x[k], bB[k]);
        };
        digit_row(32 - (q0 + 1) * BGBIT, bki + q0 * kRowBytes, std::true_type{});
#pragma unroll 1
        for (int q = q0 + 1; q < q1; q++) digit_row(32 - (q + 1) * BGBIT, bki + q * kRowBytes, std::false_type{});
        // hand-over: the sum for this wave's own polynomial's output goes to (or stays with) the light wave of that polynomial
        double2 y[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const double2 own = pol ? s[1][k] : s[0][k], other = pol ? s[0][k] : s[1][k];
            if (light) {
                y[k] = own;
                sT[k * 64 + lane] = other;          // for the other polynomial's light wave
            } else {
                sT[k * 64 + lane] = own;            // for this polynomial's light wave
                slot_extra[k * 64 + lane] = other;  // for the other polynomial's light wave
            }
        }
        __syncthreads();
        if (light) {
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const double2 za = in_a[k * 64 + lane], zb = in_b[k * 64 + lane], zc = in_c[k * 64 + lane];
                y[k] = cadd(cadd(y[k], za), cadd(zb, zc));
            }
            fft512_inverse<true>(y, scratch, lane, R);
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const bool watched = GUARD == 1 || (GUARD == 2 && (r & 3) == 0);
                const uint32_t d0 = round_coef(y[r].x, untwist_gain(r), watched, dev_max), d1 = round_coef(y[r].y, untwist_gain(r), watched, dev_max);
                const int32_t j = 64 * r + lane;
                __hip_atomic_fetch_add(&accu[j], d0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                __hip_atomic_fetch_add(&accu[j + kM], d1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            }
        }
        __syncthreads();  // accumulator complete; every handed-over sum consumed; the tiles are scratch again
    }
    if (GUARD && light) publish_guard(dev_max, guard, lane);
    finish_slice<256>(ext, item, acc, gacc, tid);
}

// ---- K3 (+K4), latency-oriented: 2L waves per gate instance ----
// For narrow levels (a single expression, the reference's own mode) the time of a level is the
// LATENCY of one blind rotation, and two waves walking 3 forward + 2 inverse transforms one after
// the other leave most of the CU idle.  Here one workgroup of 2L waves takes one gate: wave w
// (w = p*L + q) decomposes digit q of polynomial p and transforms it -- all 2L forward transforms
// at once -- and publishes the spectrum in its own tile; waves 0..3 then each own ONE spectrum
// accumulator (output polynomial w>>1, limb w&1), MAC all 2L rows into it, inverse-transform it and
// add their share to the accumulator polynomial in LDS with ds_add_u32 (addition mod 2^32
// commutes, so the two limb waves need no ordering).  Three barriers per step.
// Same arithmetic as k_blind_rotate_w2 up to the order of exact-after-rounding FP64 sums, so the
// integers it produces are identical.
// dynamic LDS: sT [2L][kTile] double2 | tw [kTwElems] double2 | acc [2][1024] int32 | bara [i1-i0] u16
// LIMBS = 1: the same kernel on the one-limb spectrum [n][2L][2][8][64] -- waves 0 and 1 own the two output polynomials,
// half the BK bytes and LDS reads per step, guarded rounding (`guard`, see k_blind_rotate_w1).
template <int L, int BGBIT, bool DIAG, int LIMBS = 2>
__global__ __launch_bounds__(128 * L) void k_blind_rotate_wide(DevKeys K, const double2* __restrict__ bkf,
                                                             const uint16_t* __restrict__ st_bara, int32_t nb,
                                                             int32_t* st_acc, int32_t i0, int32_t i1, Torus32* ext,
                                                             unsigned long long* diag, const double2* __restrict__ gtw,
                                                             unsigned* guard) {
    constexpr int RS = 2 * LIMBS * kM;  // double2 elements per BK row
    constexpr int NW = 2 * L, NT = 64 * NW;
    extern __shared__ __align__(16) unsigned char smem[];
    double2* sT_all = reinterpret_cast<double2*>(smem);
    double2* sTw = sT_all + NW * kTile;
    int32_t* acc = reinterpret_cast<int32_t*>(sTw + kTwElems);
    uint16_t* s_bara = reinterpret_cast<uint16_t*>(acc + 2 * kN);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double2* sT = sT_all + wave * kTile;
    const int64_t item = (int64_t)blockIdx.x;
    int32_t* gacc = st_acc + (size_t)item * 2 * kN;
    load_twiddles(sTw, gtw, tid, NT);
    const LaneRoots R = make_roots(sTw, lane);
    {
        copy_acc_strided<NT>(acc, gacc, tid);
        const uint16_t* bara = st_bara + (size_t)item * nb;
        for (int idx = tid; idx < i1 - i0; idx += NT) s_bara[idx] = bara[i0 + idx];
    }
    __syncthreads();

    constexpr uint32_t halfBg = 1u << (BGBIT - 1);
    uint32_t dec_offset = 0;
#pragma unroll
    for (int q = 1; q <= L; q++) dec_offset += halfBg << (32 - q * BGBIT);
    const int pw = wave / L, qw = wave - pw * L;  // forward role: digit qw of polynomial pw
    const int sh = 32 - (qw + 1) * BGBIT;
    const int32_t* accp = acc + pw * kN;
    const bool is_out = wave < 2 * LIMBS;         // inverse role: output polynomial wave>>1, limb wave&1 (one limb: polynomial wave)
    uint32_t* acco = reinterpret_cast<uint32_t*>(acc) + (LIMBS == 2 ? (wave >> 1) : wave) * kN;
    const int lsh = LIMBS == 2 ? (wave & 1) * 16 : 0;
    double dev_max = 0.0;
    unsigned long long tsum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tlast = 0;
    if (DIAG) tlast = stamp();

#pragma unroll 1
    for (int32_t i = i0; i < i1; i++) {
        const int32_t a = __builtin_amdgcn_readfirstlane((int32_t)s_bara[i - i0]);
        if (a == 0) continue;  // workgroup-uniform
        // BK_i rows [2L][4][8][64]: this wave (as an output owner) reads block `wave` of every row.
        // One CU takes 64 B/clk from its vector-memory path, i.e. >= 3 000 cycles for the 192 KiB of a
        // step, so the loads are issued in three instalments spread over the step: rows 0,1 now (they
        // fly under the decomposition and the transform), rows 2,3 after the transform, rows 4,5 once
        // rows 0,1 are consumed.
        const double2* __restrict__ bki = bkf + (size_t)i * (2 * L * RS) + (size_t)wave * kM + lane;
        double2 bA[2][8], bB[2][8], s[8];
        if (is_out) {
#pragma unroll
            for (int k = 0; k < 8; k++) {
                bA[0][k] = bki[(size_t)0 * RS + k * 64];
                bA[1][k] = bki[(size_t)1 * RS + k * 64];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        int32_t lane_o = lane;
        asm volatile("" : "+v"(lane_o));  // opaque: keeps 16 per-coefficient LDS addresses from being hoisted (and spilled)
        // all 32 LDS reads first, then the arithmetic: left to itself the compiler waits for every read
        // before issuing the next one (16 exposed LDS round trips = 2 000 cycles per step)
        uint32_t rv0[8], rv1[8], pv0[8], pv1[8];
        const int32_t jb = (lane_o - a) & (2 * kN - 1);
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const int32_t j = 64 * r + lane_o;
            rv0[r] = (uint32_t)accp[(jb + 64 * r) & (kN - 1)];        // X^a * acc at j      (sign applied below)
            rv1[r] = (uint32_t)accp[(jb + 64 * r + kM) & (kN - 1)];   //            at j + 512
            pv0[r] = (uint32_t)accp[j];
            pv1[r] = (uint32_t)accp[j + kM];
        }
        __builtin_amdgcn_sched_barrier(0);
        double2 x[8];
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const uint32_t n0 = 0u - (((uint32_t)(jb + 64 * r) >> 10) & 1u);        // all ones where the rotation wrapped
            const uint32_t n1 = 0u - (((uint32_t)(jb + 64 * r + kM) >> 10) & 1u);
            const uint32_t u0 = ((rv0[r] ^ n0) - n0) - pv0[r] + dec_offset;
            const uint32_t u1 = ((rv1[r] ^ n1) - n1) - pv1[r] + dec_offset;
            // digit - halfBg = sign-extended field of (u ^ (halfBg << sh))
            const int32_t e0 = __builtin_amdgcn_sbfe((int32_t)(u0 ^ (halfBg << sh)), sh, BGBIT);
            const int32_t e1 = __builtin_amdgcn_sbfe((int32_t)(u1 ^ (halfBg << sh)), sh, BGBIT);
            x[r] = make_double2((double)e0, (double)e1);  // untwisted: the first radix-8 pass applies e^{i pi r/16} itself
        }
        stamp_phase<DIAG>(tsum, tlast, 0);
        fft512_forward<true>(x, sT, lane, R);
        stamp_phase<DIAG>(tsum, tlast, 1);
#pragma unroll
        for (int k = 0; k < 8; k++) sT[k * 64 + lane] = x[k];  // publish
        __builtin_amdgcn_sched_barrier(0);
        if (is_out) {
#pragma unroll
            for (int k = 0; k < 8; k++) {
                bB[0][k] = bki[(size_t)2 * RS + k * 64];
                bB[1][k] = bki[(size_t)3 * RS + k * 64];
            }
        }
        stamp_phase<DIAG>(tsum, tlast, 2);
        __syncthreads();  // A: all 2L spectra are in their tiles
        stamp_phase<DIAG>(tsum, tlast, 3);
        if (is_out) {
#pragma unroll
            for (int k = 0; k < 8; k++) s[k] = make_double2(0.0, 0.0);
#define IEACHE_MAC_ROW(row, B)                                                                          \
    {                                                                                                   \
        const double2* sp = sT_all + (row) * kTile + lane;                                              \
        _Pragma("unroll") for (int k = 0; k < 8; k++) {                                                 \
            const double2 y = sp[k * 64];                                                               \
            s[k] = make_double2(fma(y.x, B[k].x, fma(-y.y, B[k].y, s[k].x)), fma(y.x, B[k].y, fma(y.y, B[k].x, s[k].y))); \
        }                                                                                               \
    }
            IEACHE_MAC_ROW(0, bA[0])
            IEACHE_MAC_ROW(1, bA[1])
            if (NW > 4) {
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    bA[0][k] = bki[(size_t)4 * RS + k * 64];
                    bA[1][k] = bki[(size_t)5 * RS + k * 64];
                }
            }
            IEACHE_MAC_ROW(2, bB[0])
            IEACHE_MAC_ROW(3, bB[1])
            if (NW > 4) {
                IEACHE_MAC_ROW(4, bA[0])
                IEACHE_MAC_ROW(5, bA[1])
            }
#undef IEACHE_MAC_ROW
        }
        stamp_phase<DIAG>(tsum, tlast, 4);
        __syncthreads();  // B: every spectrum has been consumed, tiles are scratch again
        stamp_phase<DIAG>(tsum, tlast, 5);
        if (is_out) {
            fft512_inverse<true>(s, sT, lane, R);
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const uint32_t c0 = round_coef(s[r].x, untwist_gain(r), LIMBS == 1, dev_max) << lsh;
                const uint32_t c1 = round_coef(s[r].y, untwist_gain(r), LIMBS == 1, dev_max) << lsh;
                const int32_t j = 64 * r + lane;
                atomicAdd(&acco[j], c0);       // ds_add_u32; the partner limb adds its share to the same word
                atomicAdd(&acco[j + kM], c1);
            }
        }
        stamp_phase<DIAG>(tsum, tlast, 6);
        __syncthreads();  // C: accumulator complete before the next decomposition
        stamp_phase<DIAG>(tsum, tlast, 7);
    }
    if (LIMBS == 1 && guard && is_out) publish_guard(dev_max, guard, lane);
    if (DIAG && diag && lane == 0 && (wave == 0 || wave == 4)) {
#pragma unroll
        for (int t = 0; t < 8; t++) atomicAdd(&diag[(wave >> 2) * 8 + t], tsum[t]);
    }
    if (ext) {
        Torus32* u = ext + (size_t)item * (kN + 4);
        for (int32_t j = tid; j <= kN; j += NT)
            u[j] = j == 0 ? acc[0] : (j == kN ? acc[kN] : (int32_t)(0u - (uint32_t)acc[kN - j]));
    } else {
        const int4* src = reinterpret_cast<const int4*>(acc);
        int4* dst = reinterpret_cast<int4*>(gacc);
        for (int idx = tid; idx < 2 * kN / 4; idx += NT) dst[idx] = src[idx];
    }
}


// ---- K3 (+K4), latency-oriented, round 3: 2L waves per gate, FOUR output waves on half the rows each ----
// k_blind_rotate_wide on the one-limb spectrum leaves the six row products and the inverse transform of an output
// polynomial to ONE wave (two output waves; the other four idle for half of the step), and its tiles serve both as the
// published spectra and as the inverse transforms' scratch (barrier B).  Here waves 0..3 are output waves (one per SIMD):
// output wave (c, h) = (w & 1, w >> 1) multiplies the L published spectra of accumulator polynomial h with block c of
// their BK rows -- its L blocks are requested one row at a time across the forward phase (at the top of the step, behind the
// decomposition's LDS reads, inside the forward transform: a wave that queues all 24 requests first starts its forward work
// that much later; -3 ... -6 % per rotation, profiles/r4_narrow_ab.txt) and arrive under the forward transform --, inverse-transforms that PARTIAL sum in a scratch tile of its own (no barrier B), rounds it and adds it
// into accumulator polynomial c with ds_add_u32.  Each partial sum is an integer polynomial and addition mod 2^32
// commutes, so the two halves of an output need no ordering.  Two barriers per step (spectra published / accumulator
// updated).  Same rounded integers as every other kernel here.
// dynamic LDS: acc [2][1024] int32 | sT [2L + 4][kTile] double2 | tw [kTwElems] double2 | bara [i1-i0] u16
template <int L, int BGBIT, int GUARD>
__global__ __launch_bounds__(128 * L) void k_blind_rotate_wide4(DevKeys K, const double2* __restrict__ bkf1,
                                                              const uint16_t* __restrict__ st_bara, int32_t nb,
                                                              int32_t* st_acc, int32_t i0, int32_t i1, Torus32* ext,
                                                              unsigned* guard, const double2* __restrict__ gtw) {
    constexpr int NW = 2 * L, NT = 64 * NW;
    extern __shared__ __align__(16) unsigned char smem[];
    int32_t* acc = reinterpret_cast<int32_t*>(smem);
    double2* sT_all = reinterpret_cast<double2*>(smem + (size_t)2 * kN * 4);
    double2* sTw = sT_all + (NW + 4) * kTile;
    uint16_t* s_bara = reinterpret_cast<uint16_t*>(sTw + kTwElems);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double2* sT = sT_all + wave * kTile;                  // forward scratch, then this wave's published spectrum
    double2* sTi = sT_all + (NW + (wave & 3)) * kTile;    // inverse scratch of output wave `wave`
    const int64_t item = (int64_t)blockIdx.x;
    int32_t* gacc = st_acc + (size_t)item * 2 * kN;
    load_twiddles(sTw, gtw, tid, NT);
    const LaneRoots R = make_roots(sTw, lane);
    {
        const int4* src = reinterpret_cast<const int4*>(gacc);
        int4* dst = reinterpret_cast<int4*>(acc);
        for (int idx = tid; idx < 2 * kN / 4; idx += NT) dst[idx] = src[idx];
        const uint16_t* bara = st_bara + (size_t)item * nb;
        for (int idx = tid; idx < i1 - i0; idx += NT) s_bara[idx] = bara[i0 + idx];
    }
    __syncthreads();

    constexpr uint32_t halfBg = 1u << (BGBIT - 1);
    uint32_t dec_offset = 0;
#pragma unroll
    for (int q = 1; q <= L; q++) dec_offset += halfBg << (32 - q * BGBIT);
    const int pw = wave / L, qw = wave - pw * L;  // forward role: digit qw of polynomial pw = row `wave` of BK_i
    const int sh = 32 - (qw + 1) * BGBIT;
    const bool is_out = wave < 4;
    const int oc = wave & 1, oh = (wave >> 1) & 1;  // output role: block oc of the rows of polynomial oh
    uint32_t* acco = reinterpret_cast<uint32_t*>(acc) + oc * kN;
    const unsigned char* accb = reinterpret_cast<const unsigned char*>(acc);
    const uint32_t pb = (uint32_t)pw * (kN * 4);
    const int32_t* accp = acc + pw * kN;
    double dev_max = 0.0;

#pragma unroll 1
    for (int32_t i = i0; i < i1; i++) {
        const int32_t a = __builtin_amdgcn_readfirstlane((int32_t)s_bara[i - i0]);
        if (a == 0) continue;  // workgroup-uniform
        // BK_i rows [2L][2][8][64]: this output wave's L blocks, one row per request point
        const double2* __restrict__ bki = bkf1 + (size_t)i * (2 * L * 2 * kM) + (size_t)(oh * L) * (2 * kM) + (size_t)oc * kM + lane;
        double2 bk[L][8];
        auto request = [&](int q) {
            if (is_out) {
#pragma unroll
                for (int k = 0; k < 8; k++) bk[q][k] = bki[(size_t)q * (2 * kM) + k * 64];
            }
        };
        request(0);
        __builtin_amdgcn_sched_barrier(0);
        int32_t lane_o = lane;
        asm volatile("" : "+v"(lane_o));  // opaque: keeps the per-coefficient LDS addresses from being hoisted out of the step loop
        const uint32_t jb4 = ((uint32_t)(lane_o - a) & (2 * kN - 1)) << 2;
        uint32_t rv0[8], rv1[8], pv0[8], pv1[8];
#pragma unroll
        for (int r = 0; r < 8; r++) {   // all 32 LDS reads first, then the arithmetic
            const uint32_t t = jb4 + 256u * r;
            const uint32_t o0 = (t & 4092u) | pb, o1 = o0 ^ 2048u;
            rv0[r] = *reinterpret_cast<const uint32_t*>(accb + o0);
            rv1[r] = *reinterpret_cast<const uint32_t*>(accb + o1);
            pv0[r] = (uint32_t)accp[64 * r + lane_o];
            pv1[r] = (uint32_t)accp[64 * r + lane_o + kM];
        }
        __builtin_amdgcn_sched_barrier(0);
        request(1);
        __builtin_amdgcn_sched_barrier(0);
        double2 x[8];
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const uint32_t t = jb4 + 256u * r;
            const uint32_t m0 = (uint32_t)__builtin_amdgcn_sbfe((int32_t)t, 12, 1), m1 = (uint32_t)__builtin_amdgcn_sbfe((int32_t)(t + 2048u), 12, 1);
            const uint32_t u0 = (rv0[r] ^ m0) + ((dec_offset - pv0[r]) - m0);
            const uint32_t u1 = (rv1[r] ^ m1) + ((dec_offset - pv1[r]) - m1);
            // digit - halfBg = sign-extended field of (u ^ (halfBg << sh))
            const int32_t e0 = __builtin_amdgcn_sbfe((int32_t)(u0 ^ (halfBg << sh)), sh, BGBIT);
            const int32_t e1 = __builtin_amdgcn_sbfe((int32_t)(u1 ^ (halfBg << sh)), sh, BGBIT);
            x[r] = make_double2((double)e0, (double)e1);  // untwisted: the first radix-8 pass applies e^{i pi r/16} itself
        }
        if (L > 2)
            fft512_forward<true, 0>(x, sT, lane, R, [&]() {
#pragma unroll
                for (int q = 2; q < L; q++) request(q);
            });
        else
            fft512_forward<true>(x, sT, lane, R);
#pragma unroll
        for (int k = 0; k < 8; k++) sT[k * 64 + lane] = x[k];  // publish
        __syncthreads();  // A: all 2L spectra are in their tiles
        if (is_out) {
            double2 s[8];
#pragma unroll
            for (int q = 0; q < L; q++) {
                const double2* sp = sT_all + (oh * L + q) * kTile + lane;
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const double2 y = sp[k * 64];
                    s[k] = q == 0 ? mac<true>(s[k], y, bk[0][k]) : mac<false>(s[k], y, bk[q][k]);
                }
            }
            fft512_inverse<true>(s, sTi, lane, R);
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const bool watched = GUARD == 1 || (GUARD == 2 && (r & 3) == 0);
                const uint32_t d0 = round_coef(s[r].x, untwist_gain(r), watched, dev_max), d1 = round_coef(s[r].y, untwist_gain(r), watched, dev_max);
                const int32_t j = 64 * r + lane;
                atomicAdd(&acco[j], d0);  // ds_add_u32; the other half of this output adds to the same word
                atomicAdd(&acco[j + kM], d1);
            }
        }
        __syncthreads();  // C: accumulator complete before the next decomposition; every published spectrum consumed
    }
    if (GUARD && is_out) publish_guard(dev_max, guard, lane);
    if (ext) {
        Torus32* u = ext + (size_t)item * (kN + 4);
        for (int32_t j = tid; j <= kN; j += NT)
            u[j] = j == 0 ? acc[0] : (j == kN ? acc[kN] : (int32_t)(0u - (uint32_t)acc[kN - j]));
    } else {
        const int4* src = reinterpret_cast<const int4*>(acc);
        int4* dst = reinterpret_cast<int4*>(gacc);
        for (int idx = tid; idx < 2 * kN / 4; idx += NT) dst[idx] = src[idx];
    }
}

// the transforms' twiddle table (fft512.h), built once per context
__global__ __launch_bounds__(128) void k_build_twiddle_table(double2* tw) { build_twiddles(tw, threadIdx.x, 128); }

}  // namespace

size_t spectrum_elems(const Params& p) { return (size_t)p.n * p.kpl() * 4 * kM; }
size_t spectrum1_elems(const Params& p) { return (size_t)p.n * p.kpl() * 2 * kM; }
size_t twiddle_table_elems() { return kTwElems; }

void build_twiddle_table(double2* d_tw, hipStream_t stream) {
    hipLaunchKernelGGL(k_build_twiddle_table, dim3(1), dim3(128), 0, stream, d_tw);
}

void prepare_spectrum(const Params& p, const Torus32* d_bk_raw, double2* d_bkf, hipStream_t stream) {
    const size_t npoly = (size_t)p.n * p.kpl() * 2;
    hipLaunchKernelGGL(k_bk_to_spectrum_w64, dim3((unsigned)npoly), dim3(64), 0, stream, d_bk_raw, d_bkf);
}

void prepare_spectrum1(const Params& p, const Torus32* d_bk_raw, double2* d_bkf1, hipStream_t stream) {
    const size_t npoly = (size_t)p.n * p.kpl() * 2;
    hipLaunchKernelGGL(k_bk_to_spectrum_w64_1, dim3((unsigned)npoly), dim3(64), 0, stream, d_bk_raw, d_bkf1);
}

// diagnostic builds (br_variant 8 / 49): per-segment s_memtime sums, printed per launch() call
static void diag_report(hipStream_t stream, unsigned long long* buf, const char* tag, const char* const* names, int nnames, double denom) {
    unsigned long long h[16];
    (void)hipStreamSynchronize(stream);
    (void)hipMemcpy(h, buf, sizeof h, hipMemcpyDeviceToHost);
    (void)hipMemset(buf, 0, sizeof h);
    for (int w = 0; w < 2; w++) {
        double tot = 0;
        for (int t = 0; t < nnames; t++) tot += (double)h[w * 8 + t];
        fprintf(stderr, "[br-diag %s] slot %d: %.0f memtime ticks per step:", tag, w, tot / denom);
        for (int t = 0; t < nnames; t++) fprintf(stderr, " %s=%.0f", names[t], (double)h[w * 8 + t] / denom);
        fprintf(stderr, "\n");
    }
}

// ---- the launch half of the variant table: one row per build of a br_variant number (br_plan.h: kBrVariants) ----
// one launch: CMux steps [i0, i1) of `items` gate instances, parameter set l
struct Slice {
    int32_t l;
    int64_t items;
    hipStream_t stream;
    const DevKeys& K;
    const Tables& t;
    const uint16_t* st_bara;
    int32_t nb;
    int32_t* st_acc;
    int32_t i0, i1;
    Torus32* ext;
    int32_t flip;  // k_blind_rotate_w4r: BrPlan::w4r_flip
};
constexpr int kTwoLWaves = 0;
struct LaunchRow {
    int32_t number;     // "br_variant": a row of kBrVariants
    int gates;          // per workgroup: the variant's default build, or one of its smaller ones
    int threads;        // per workgroup; kTwoLWaves: 128 L (2L waves per gate)
    size_t (*lds)(int L, int32_t nb, int gates);  // dynamic LDS of a launch
    size_t allow;       // bytes of dynamic LDS to be allowed first; 0: the launch fits the default 64 KiB
    void (*launch)(const LaunchRow&, const Slice&);
};
static LdsGrant& granted(const LaunchRow& v, int param_set);  // ... remembered per kernel (parameter set) and device

template <class T>
struct as_is {
    using type = T;
};
// `grant`: the opt-in of this kernel; a row's own unless the row launches a second build (go_w1b)
template <class PS, class... P>
static void launch_row_granted(PS, const LaunchRow& v, const Slice& s, LdsGrant& grant, void (*kernel)(P...), typename as_is<P>::type... args) {
    if (v.allow) {
        char what[96];  // the instantiation, for the message of a refused opt-in
        snprintf(what, sizeof what, "%s<%d,%d> (br_variant %d, %d gates per workgroup)", br_variant(v.number)->name, PS::L, PS::BGBIT, (int)v.number, v.gates);
        allow_dynamic_lds_once(grant, (const void*)kernel, v.allow, what);
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)((s.items + v.gates - 1) / v.gates)), dim3(v.threads == kTwoLWaves ? 128 * PS::L : v.threads),
                       v.lds(PS::L, s.nb, v.gates), s.stream, args...);
}
template <class PS, class... P>
static void launch_row(PS ps, const LaunchRow& v, const Slice& s, void (*kernel)(P...), typename as_is<P>::type... args) {
    launch_row_granted(ps, v, s, granted(v, PS::index), kernel, args...);
}
// one launcher per kernel (their argument lists differ), instantiated for both parameter sets
template <int XLANE>
static void go_w2(const LaunchRow& v, const Slice& s) {
    with_param_set(s.l, [&](auto ps) {
        launch_row(ps, v, s, k_blind_rotate_w2<ps.L, ps.BGBIT, XLANE>, s.K, s.t.bkf, s.st_bara, s.nb, s.st_acc, s.i0, s.i1, s.ext, s.t.twiddles);
    });
}
template <int G>
static void go_x1(const LaunchRow& v, const Slice& s) {
    with_param_set(s.l, [&](auto ps) {
        launch_row(ps, v, s, k_blind_rotate_x1<ps.L, ps.BGBIT, G>, s.K, s.t.bkf, s.st_bara, s.nb, s.st_acc, s.items, s.i0, s.i1, s.ext, s.t.twiddles);
    });
}
template <bool DIAG, int LIMBS>
static void go_wide(const LaunchRow& v, const Slice& s) {
    with_param_set(s.l, [&](auto ps) {
        launch_row(ps, v, s, k_blind_rotate_wide<ps.L, ps.BGBIT, DIAG, LIMBS>, s.K, LIMBS == 2 ? s.t.bkf : s.t.bkf1, s.st_bara, s.nb, s.st_acc,
                   s.i0, s.i1, s.ext, DIAG ? s.t.diag : nullptr, s.t.twiddles, LIMBS == 2 ? nullptr : s.t.guard);
    });
}
// The forward transforms' lane-high transpose takes the exchange form (XLANE = 2: +1.6 %, profiles/xlane3_ab.txt) but in the
// stamped l = 2 build, which does not hold it without scratch.  The default-guard builds have the v_cndmask form (1) beside
// them, as the partner of an A/B and of tests/test_xlane_exchange_gpu.py, launched while probe::w1b_forward_path() says so.
template <int GUARD, bool DIAG = false, int G = kW1Gates>
static void go_w1b(const LaunchRow& v, const Slice& s) {
    with_param_set(s.l, [&](auto ps) {
        constexpr int XL = (DIAG && ps.L == 2) ? 1 : 2;
        if constexpr (GUARD == 2 && !DIAG) {
            if (probe::w1b_forward_path() == 1) {
                static LdsGrant partner;  // per instantiation: G and the parameter set
                launch_row_granted(ps, v, s, partner, k_blind_rotate_w1b<ps.L, ps.BGBIT, GUARD, DIAG, G, 1>, s.K, s.t.bkf1, s.st_bara, s.nb, s.st_acc,
                                   s.items, s.i0, s.i1, s.ext, s.t.guard, s.t.twiddles, nullptr);
                return;
            }
        }
        launch_row(ps, v, s, k_blind_rotate_w1b<ps.L, ps.BGBIT, GUARD, DIAG, G, XL>, s.K, s.t.bkf1, s.st_bara, s.nb, s.st_acc, s.items, s.i0, s.i1,
                   s.ext, s.t.guard, s.t.twiddles, DIAG ? s.t.diag : nullptr);
    });
}
template <int GUARD>
static void go_w2r(const LaunchRow& v, const Slice& s) {
    with_param_set(s.l, [&](auto ps) {
        launch_row(ps, v, s, k_blind_rotate_w2r<ps.L, ps.BGBIT, GUARD>, s.K, s.t.bkf1, s.st_bara, s.nb, s.st_acc, s.i0, s.i1, s.ext, s.t.guard, s.t.twiddles);
    });
}
template <int GUARD>
static void go_w4r(const LaunchRow& v, const Slice& s) {
    with_param_set(s.l, [&](auto ps) {
        launch_row(ps, v, s, k_blind_rotate_w4r<ps.L, ps.BGBIT, GUARD>, s.K, s.t.bkf1, s.st_bara, s.nb, s.st_acc, s.i0, s.i1, s.ext, s.t.guard, s.t.twiddles,
                   s.flip);
    });
}
template <int GUARD>
static void go_wide4(const LaunchRow& v, const Slice& s) {
    with_param_set(s.l, [&](auto ps) {
        launch_row(ps, v, s, k_blind_rotate_wide4<ps.L, ps.BGBIT, GUARD>, s.K, s.t.bkf1, s.st_bara, s.nb, s.st_acc, s.i0, s.i1, s.ext, s.t.guard, s.t.twiddles);
    });
}

constexpr size_t kAccBytes = (size_t)2 * kN * 4, kCuLds = 160 * 1024;
// LDS per workgroup: 4 gates -> 2 workgroups per CU, 3 -> 2, 2 -> 3, 1 -> 6
constexpr size_t lds_bytes_w1(int wg_gates) { return (size_t)(wg_gates * kTile + kTwElems) * sizeof(double2) + (size_t)wg_gates * 2 * kN * 4; }
static size_t lds_w1(int, int32_t, int gates) { return lds_bytes_w1(gates); }
static size_t lds_w2(int, int32_t, int) { return (size_t)(2 * kTile + kTwElems) * sizeof(double2) + kAccBytes; }
static size_t lds_w4(int, int32_t, int) { return (size_t)(4 * kTile + 2 * 8 * 64 + kTwElems) * sizeof(double2) + kAccBytes; }
static size_t lds_wide(int L, int32_t nb, int) { return (size_t)(2 * L * kTile + kTwElems) * sizeof(double2) + kAccBytes + (size_t)nb * 2; }
static size_t lds_wide4(int L, int32_t nb, int) { return (size_t)((2 * L + 4) * kTile + kTwElems) * sizeof(double2) + kAccBytes + (size_t)nb * 2; }

// What a number means (kernel, limbs, slice lengths, which builds exist) is its row in kBrVariants; the rows here with
// fewer gates per workgroup than the variant's default are the builds a launch that does not fill the chip takes.
static constexpr LaunchRow kLaunchRows[] = {
    // number, gates per workgroup, threads, LDS, allow, launcher
    // ---- two limbs: exact by construction ----
    {0, 1, 128, lds_w2, 0, go_w2<1>},
    {kVariantTwoWavesLds, 1, 128, lds_w2, 0, go_w2<0>},
    {kVariantExactOneWave, 4, 256, lds_w1, lds_bytes_w1(4), go_x1<4>},
    {kVariantExactOneWave, 3, 192, lds_w1, lds_bytes_w1(3), go_x1<3>},
    {kVariantExactOneWave, 2, 128, lds_w1, lds_bytes_w1(2), go_x1<2>},
    {kVariantExactOneWave, 1, 64, lds_w1, lds_bytes_w1(1), go_x1<1>},
    {kVariantWide, 1, kTwoLWaves, lds_wide, kCuLds, go_wide<false, 2>},
    {kVariantWideStamps, 1, kTwoLWaves, lds_wide, kCuLds, go_wide<true, 2>},
    // ---- one limb, guarded ----
    {kVariantWideOneLimb, 1, kTwoLWaves, lds_wide, kCuLds, go_wide<false, 1>},
    {kVariantOneLimbDefault, 4, 256, lds_w1, lds_bytes_w1(4), go_w1b<2>},
    {kVariantOneLimbDefault, 3, 192, lds_w1, lds_bytes_w1(3), go_w1b<2, false, 3>},
    {kVariantOneLimbDefault, 2, 128, lds_w1, lds_bytes_w1(2), go_w1b<2, false, 2>},
    {kVariantOneLimbDefault, 1, 64, lds_w1, lds_bytes_w1(1), go_w1b<2, false, 1>},
    {kVariantOneLimbDefault + 1, 4, 256, lds_w1, lds_bytes_w1(4), go_w1b<1>},
    {kVariantOneLimbDefault + 4, 4, 256, lds_w1, lds_bytes_w1(4), go_w1b<0>},
    {kVariantOneLimbStamps, 4, 256, lds_w1, lds_bytes_w1(4), go_w1b<2, true>},
    {kVariantOneLimbTwoWaves, 1, 128, lds_w2, 0, go_w2r<2>},
    {kVariantOneLimbTwoWaves + 1, 1, 128, lds_w2, 0, go_w2r<1>},
    {kVariantOneLimbFourWaves, 1, 256, lds_w4, kCuLds, go_w4r<2>},
    {kVariantOneLimbFourWaves + 1, 1, 256, lds_w4, kCuLds, go_w4r<1>},
    {kVariantWideHandoverOneLimb, 1, kTwoLWaves, lds_wide4, kCuLds, go_wide4<2>},
    {kVariantWideHandoverOneLimb + 1, 1, kTwoLWaves, lds_wide4, kCuLds, go_wide4<1>},
};
constexpr size_t kLaunchRowCount = sizeof kLaunchRows / sizeof kLaunchRows[0];
static LdsGrant g_granted[kLaunchRowCount][2];
static LdsGrant& granted(const LaunchRow& v, int param_set) { return g_granted[&v - kLaunchRows][param_set]; }

// every launch row is a build kBrVariants names, and every build it names has exactly one launch row
constexpr bool launch_rows_match_variants() {
    for (const LaunchRow& r : kLaunchRows)
        if (!br_variant_build(r.number, r.gates)) return false;
    for (const BrVariant& v : kBrVariants)
        for (int g = v.wg_builds ? 1 : v.gates; g <= v.gates; g++) {
            int rows = 0;
            for (const LaunchRow& r : kLaunchRows) rows += r.number == v.number && r.gates == g;
            if (rows != 1) return false;
        }
    return true;
}
static_assert(launch_rows_match_variants(), "kLaunchRows and kBrVariants (br_plan.h) name different variants or builds");

// one slice of CMux steps on the kernel `variant` names, wg gates per workgroup where the kernel is built for that
static void launch_slice(int variant, int wg, const Slice& s) {
    const BrVariant* v = br_variant(variant);
    if (!v) throw std::invalid_argument("unknown blind-rotation variant");
    const int gates = br_variant_build(variant, wg) ? wg : v->gates;
    for (const LaunchRow& r : kLaunchRows)
        if (r.number == variant && r.gates == gates) return r.launch(r, s);
}

// A mid-size launch (more gates than fit two waves each, fewer than fill the chip with one wave each) as a ROTATION OF ROLES:
// the items are cut into mix.k contiguous subsets, each driven by its own stream; in phase t the subsets t .. t + tw - 1
// (mod k) advance s2 CMux steps on the two-waves-per-gate kernel while the others advance s1 steps on the one-wave-per-gate
// kernel, so that all eight wave slots of every CU work (a gate is one sequential chain of steps: with one wave per gate
// 1 536 gates can keep only 1 536 of the chip's 2 048 slots busy).  After `cycles` rounds of k phases every subset has done
// cycles x (tw s2 + (k - tw) s1) steps; the caller's ordinary slice loop finishes the rotation from there on the main stream.
// Same kernels, same arithmetic per step: bit-identical to any other schedule.  Returns the kernel launches issued.
static int launch_mixed_phases(const Params& p, const DevKeys& K, const Tables& tab, int64_t items, int32_t* st_acc, uint16_t* st_bara,
                               int32_t nb, const BrPlan& plan, const BrLanes& on, int32_t* steps_done) {
    int launches = 0;
    const int k = plan.mix.k, tw = plan.mix.tw;
    const MixSteps& ms = plan.mix_steps;
    auto ok = [](hipError_t e) {  // a failed record / wait would leave the streams unordered: stop here rather than compute on stale state
        if (e != hipSuccess) throw std::runtime_error(std::string("rotation of roles: ") + hipGetErrorString(e));
    };
    // contiguous subsets of whole workgroups of the one-wave kernel (4 gates) -- and of 3, the other workgroup size
    const int64_t per = mix_subset_size(items, k);
    std::vector<int32_t> pos(k, 0);
    hipStream_t main = on.streams[0];
    ok(hipEventRecord(on.ev[0], main));  // the prologue is on the main stream
    for (int j = 1; j < k; j++) ok(hipStreamWaitEvent(on.streams[j], on.ev[0], 0));
    const int32_t rounds = ms.cycles + ((ms.tail_s1 > 0 && ms.tail_s2 > 0) ? 1 : 0);
    int32_t total = 0;
    for (int32_t c = 0; c < rounds; c++) {
        // the last round may be a shortened one (tail_s1 / tail_s2) that takes the rotation close to its end
        const int32_t s1c = c < ms.cycles ? ms.s1 : ms.tail_s1, s2c = c < ms.cycles ? ms.s2 : ms.tail_s2;
        total += tw * s2c + (k - tw) * s1c;
        for (int t = 0; t < k; t++) {
            for (int j = 0; j < k; j++) {
                const int64_t off = (int64_t)j * per, m = std::min<int64_t>(per, items - off);
                if (m <= 0) continue;
                const bool two = ((j - t) % k + k) % k < tw;
                int32_t todo = two ? s2c : s1c;
                while (todo > 0) {  // the one-wave kernel takes at most 64 steps per launch (one rotation amount per lane)
                    const int32_t s = two ? todo : std::min<int32_t>(todo, 64);
                    const int v = two ? kVariantOneLimbTwoWaves : kVariantOneLimbDefault;
                    launch_slice(v, plan.mix_wg, Slice{p.l, m, on.streams[j], K, tab, st_bara + (size_t)off * nb, nb,
                                                       st_acc + (size_t)off * 2 * kN, pos[j], pos[j] + s, nullptr, plan.w4r_flip});
                    pos[j] += s;
                    todo -= s;
                    launches++;
                }
            }
            if (plan.mix_sync && !(c == rounds - 1 && t == k - 1)) {
                // phase boundary: nobody starts the next phase before everybody has finished this one (the roles change)
                for (int j = 0; j < k; j++) ok(hipEventRecord(on.ev[j], on.streams[j]));
                for (int j = 0; j < k; j++)
                    for (int q = 0; q < k; q++)
                        if (q != j) ok(hipStreamWaitEvent(on.streams[j], on.ev[q], 0));
            }
        }
    }
    for (int j = 1; j < k; j++) {  // join: the main stream finishes the rotation
        ok(hipEventRecord(on.ev[j], on.streams[j]));
        ok(hipStreamWaitEvent(main, on.ev[j], 0));
    }
    *steps_done = total;
    return launches;
}

int launch(const Params& p, const DevKeys& K, const Tables& t, const BrPlan& plan, const BrLanes& mix, hipStream_t stream,
           const BrPart* parts, size_t n_parts, void* state, Torus32* ext, int32_t steps, Torus32* dbg_acc) {
    int64_t items = 0;
    for (size_t q = 0; q < n_parts; q++) {
        if (parts[q].cnt < 1) throw std::logic_error("blind-rotation launch: an empty part");
        items += parts[q].cnt;
    }
    if (items < 1) throw std::logic_error("blind-rotation launch without items");
    const BrVariant* row = br_variant(plan.variant);
    if (plan.generic || !row) throw std::invalid_argument("unknown blind-rotation variant");
    if (row->limbs == 1 && (!t.bkf1 || !t.guard)) throw std::runtime_error("one-limb blind rotation without its spectrum / guard word");
    const int32_t nb = br_bara_stride(p);
    const int32_t nsteps = steps < 0 ? p.n : (steps < p.n ? steps : p.n);
    // not decisions, the kernels' bounds: a slice's rotation amounts fit a lane each unless the kernel has long_slices (every
    // slice ends at nsteps <= nb at the latest); a rotation of roles leaves the loop below a step, runs on the launch's own
    // stream and on streams that exist
    const int32_t S = plan.slice;
    if (S < 1 || (!row->long_slices && S > 64)) throw std::logic_error("blind-rotation plan: slice length out of the kernel's range");
    const int k = plan.mix.k;
    if (k && (k < 2 || k > kMaxLanes || plan.mix.tw < 1 || plan.mix.tw >= k || row->limbs != 1 || plan.mix_steps.s1 < 1 || plan.mix_steps.s2 < 1 ||
              plan.mix_steps.cycles < 1 || plan.mix_steps.covered >= nsteps || mix.streams[0] != stream))
        throw std::logic_error("blind-rotation plan: rotation of roles outside what the launch can run");
    for (int j = 0; j < k; j++)
        if (!mix.streams[j] || !mix.ev[j]) throw std::logic_error("blind-rotation plan: rotation of roles without its streams");
    if ((plan.variant == kVariantOneLimbStamps || plan.variant == kVariantWideStamps) && !t.diag) throw std::logic_error("diagnostic blind-rotation build without its stamp buffer");
    int launches = 0;
    // state block: [items][2][1024] int32 accumulators, then [items][nb] u16 rotation amounts
    int32_t* st_acc = reinterpret_cast<int32_t*>(state);
    uint16_t* st_bara = reinterpret_cast<uint16_t*>(st_acc + (size_t)items * 2 * kN);
    // the prologue writes row (block index) of what it is given: a part's rows start `off` rows into the state block
    int64_t off = 0;
    for (size_t q = 0; q < n_parts; q++) {
        const WorkDesc& W = parts[q].W;
        uint16_t* bara = st_bara + (size_t)off * nb;
        int32_t* acc = st_acc + (size_t)off * 2 * kN;
        if (!W.gates && W.tv && W.flat_type == kFlatRawTlwe)  // a programmable bootstrap from TLWE samples
            hipLaunchKernelGGL(k_br_prologue_tlwe, dim3((unsigned)parts[q].cnt), dim3(128), 0, stream, K, W, bara, nb, acc);
        else if (!W.gates && W.tv)  // a programmable bootstrap (BlindRotate::launch has checked the table)
            hipLaunchKernelGGL(k_br_prologue<true>, dim3((unsigned)parts[q].cnt), dim3(128), 0, stream, K, W, bara, nb, acc);
        else
            hipLaunchKernelGGL(k_br_prologue<false>, dim3((unsigned)parts[q].cnt), dim3(128), 0, stream, K, W, bara, nb, acc);
        off += parts[q].cnt;
    }
    auto one = [&](int v, int32_t i0, int32_t i1, Torus32* e) {
        launch_slice(v, plan.wg_gates, Slice{p.l, items, stream, K, t, st_bara, nb, st_acc, i0, i1, e, plan.w4r_flip});
    };
    int32_t first = 0;
    if (k) launches += launch_mixed_phases(p, K, t, items, st_acc, st_bara, nb, plan, mix, &first);
    for (int32_t i0 = first; i0 < nsteps; i0 += S) {
        const int32_t i1 = i0 + S < nsteps ? i0 + S : nsteps;
        launches++;
        one(plan.variant, i0, i1, (i1 == nsteps) ? ext : nullptr);  // the last slice extracts instead of storing the accumulator
    }
    const double denom = (double)items * (nsteps > 0 ? nsteps : 1);
    if (plan.variant == kVariantOneLimbStamps) {
        static const char* names[6] = {"decomposition (x2)", "digits+cvt+twist (x6)", "forward transform (x6)", "2nd BK block + products (x6)", "inverse pair", "round+update"};
        diag_report(stream, t.diag, "w1b, waves by parity", names, 6, denom / 2.0);  // each of the two slots collects half of the waves
    } else if (plan.variant == kVariantWideStamps) {
        static const char* names[8] = {"head+decompose", "fwdFFT", "publish+BK issue", "barrier A", "MAC rows", "barrier B", "invFFT+update", "barrier C"};
        diag_report(stream, t.diag, "wide, waves 0 / 4", names, 8, denom);
    }
    if (nsteps == 0 && ext) one(kVariantTwoWavesLds, 0, 0, ext);  // degenerate (steps == 0): extraction straight from the initial accumulator
    if (dbg_acc)
        (void)hipMemcpyAsync(dbg_acc, st_acc, (size_t)items * 2 * kN * 4, hipMemcpyDeviceToDevice, stream);
    return launches;
}

}  // namespace w64
}  // namespace ieache
