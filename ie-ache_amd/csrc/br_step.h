// The pieces of one CMux step that the blind-rotation kernels of blind_rotate_w64.hip share, each stated once:
//   acc += round( IFFT( sum over rows  FFT(digit_q((X^a - 1) acc_p + offset)) * BK_i[row] ) )
// A kernel there is a SCHEDULE over these pieces -- which wave owns which rows, what crosses waves through which tile,
// where the BK loads are issued relative to the transforms, where the barriers stand -- and nothing here decides any of
// that: every function is a forced inline over the caller's registers.  The rule for moving a piece in here: the kernel's
// code must not change (scripts/isa_same.py on hipcc -S output before and after: identical, or identical up to exchanged
// sources of a commutative instruction, all resource figures equal).  With this compiler that holds per piece AND per
// kernel, and not for every combination; where a move reordered so much as two scalar instructions the kernel keeps its
// open-coded copy:
//   piece                         used by                                open-coded in
//   guard publication             _w1b _w2r _w4r _wide _wide4            --
//   digit conversion              _w2 _w1b _x1 _w2r _w4r                 (_wide / _wide4 extract one digit per wave: signed field only)
//   row product (mac / mac_row)   all but _wide                          _wide (IEACHE_MAC_ROW: the helper moves its stamped build, br_variant 8)
//   epilogue (finish_slice)       _w2 _w1b _x1 _w2r _w4r                 _wide _wide4 (strided copy: reorders their epilogue)
//   BK buffer resource            _w1b _x1 _w2r _w4r                     --
//   phase stamps                  _w1b _wide                             --
//   rotated decomposition         _w1b _x1 _w4r                          _w2r (reschedules it); _wide4 reads first, combines later
//   amounts, once per slice       _w2 _w1b _x1                           every-64-steps form: _w2r _w4r (reschedules both)
//   accumulator load              _w2 _wide                              _w1b _x1 _wide4 (changes instruction count), _w2r _w4r (with the others above)
//   decomposition offset          _w2                                    the other six (_w1b _x1 _wide _wide4 alone, _w2r _w4r in combination)
//   round + ds_add_u32 update     --                                     all (a shared form reorders the GUARD = 2 builds of _w2r / _w4r)
//   two-limb digit row            _x1 k_cmux_x1 k_demux_x1 k_rotate_x1   --
//   limb recombination            _x1 k_cmux_x1 k_demux_x1 k_rotate_x1   -- (k_cmux_x1: the three sources of 16 v_add3_u32 come out in another order)
//   ... with a run-time digit width k_cmux_rt k_demux_rt k_rotate_rt      -- (digit_row_two_limb_rt, decomposition_offset_rt: siblings, the rows above keep their code)
// k_cmux_x1 / k_demux_x1 (cmux.hip) and k_rotate_x1 (rotate.hip) are the CMux family: _x1's step on caller TGSW samples.  What
// only they share is cmux_step.h, under the same rule:
//   selector rule                 k_demux_x1 k_rotate_x1 k_read_indices  k_cmux_x1 (its flat form implies another position than it reads: any shared form moves it)
//   index clamp                   k_cmux_x1 k_tlwe_extract               k_cmux_copy (one instruction fewer), the selector rule itself (narrowed to 32 bits in k_demux_x1)
//   wave prologue                 k_cmux_x1 k_demux_x1 k_rotate_x1       --
//   row resource / row word       k_cmux_x1 k_demux_x1                   --
//   loop over the digit rows      --                                     k_cmux_x1 k_demux_x1 (one helper over the loop moves both)
// The transform itself is fft512.h / dft8_twist.h.
#pragma once
#include "device_common.h"
#include "fft512.h"

namespace ieache {
namespace w64 {
namespace {

using namespace dev;

constexpr int kW1Gates = 4;              // gates (= waves) per workgroup of the one-wave-per-gate kernels: they share the twiddle table only
// Rounding guard of the one-limb kernels.  round_coef() folds the distance to the nearest integer of the watched inverse-
// transformed coefficients into a per-lane running maximum; publish_guard() makes it the launch's: guard[1] is the largest
// distance seen (float bits: non-negative floats order like unsigned integers), guard[0] counts the waves that saw more than
// kGuardLimit -- 1/16 of an integer step, where 1/2 would change a rounded coefficient and real data stay near 2^-9
// (DESIGN.md section 3).  A non-zero count makes the evaluator repeat the call on the two-limb kernels.
constexpr float kGuardLimit = 0.0625f;
__device__ __forceinline__ void publish_guard(double dev_max, unsigned* guard, int lane) {
    float m = (float)dev_max;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) {
        const unsigned bits = __float_as_uint(m);
        if (bits > __builtin_nontemporal_load(&guard[1])) atomicMax(&guard[1], bits);
        if (m > kGuardLimit) atomicAdd(&guard[0], 1u);
    }
}

// ---- state block <-> LDS, sample extract ----
// One gate's accumulator [2][1024] int32 as 512 int4, NT threads (a divisor of 512), in registers' order ...
template <int NT>
__device__ __forceinline__ void copy_acc(int32_t* to, const int32_t* from, int tid) {
    const int4* src = reinterpret_cast<const int4*>(from);
    int4* dst = reinterpret_cast<int4*>(to);
#pragma unroll
    for (int r = 0; r < 2 * kN / 4 / NT; r++) dst[NT * r + tid] = src[NT * r + tid];
}
// ... or as a strided loop (the 2L-waves kernels: 384 threads for L = 3)
template <int NT>
__device__ __forceinline__ void copy_acc_strided(int32_t* to, const int32_t* from, int tid) {
    const int4* src = reinterpret_cast<const int4*>(from);
    int4* dst = reinterpret_cast<int4*>(to);
    for (int idx = tid; idx < 2 * kN / 4; idx += NT) dst[idx] = src[idx];
}
// After a slice: the last one extracts the LWE sample (K4: b = acc[1][0], a_j = -acc[0][N - j], a row of N + 4 words),
// every other one stores the accumulator back to the state block.
template <int NT>
__device__ __forceinline__ void finish_slice(Torus32* ext, int64_t item, const int32_t* acc, int32_t* gacc, int tid) {
    if (ext) {
        Torus32* u = ext + (size_t)item * (kN + 4);
        for (int32_t j = tid; j <= kN; j += NT)
            u[j] = j == 0 ? acc[0] : (j == kN ? acc[kN] : (int32_t)(0u - (uint32_t)acc[kN - j]));
    } else {
        const int4* src = reinterpret_cast<const int4*>(acc);
        int4* dst = reinterpret_cast<int4*>(gacc);
#pragma unroll
        for (int r = 0; r < 2 * kN / 4 / NT; r++) dst[NT * r + tid] = src[NT * r + tid];
    }
}

// ---- rotation amounts ----
// One amount per lane for the 64 steps from i on, read back with v_readlane: a dependent global load at the head of every
// step costs ~2-3k cycles.  The one-wave kernels and k_blind_rotate_w2 fetch once per slice (slices of at most 64 steps);
// k_blind_rotate_w2r / _w4r fetch again every 64 steps, so a launch may be the whole rotation.
__device__ __forceinline__ int32_t lane_amounts(const uint16_t* __restrict__ bara, int32_t i, int32_t i1, int lane) {
    return (i + lane < i1) ? (int32_t)bara[i + lane] : 0;
}

// ---- BK through the buffer path (load_bk_block, fft512.h) ----
// resource over the whole spectrum: n steps of step_bytes; the step and row go into the scalar offset, the lane's 16 bytes
// are the only vector operand
__device__ __forceinline__ __amdgpu_buffer_rsrc_t bk_resource(const double2* bkf, int32_t n, int step_bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<double2*>(bkf), (short)0, n * step_bytes, 0x00020000);
}
__device__ __forceinline__ int bk_lane_offset(int lane) { return lane * (int)sizeof(double2); }

// ---- decomposition ----
// C = sum_q halfBg << shift_q.  (x + C) ^ C leaves digit q's field holding digit ^ halfBg, whose sign-extended BGBIT-bit
// value IS digit - halfBg: one v_bfe_i32 per digit (signed_digit below).
template <int L, int BGBIT>
__device__ __forceinline__ uint32_t decomposition_offset() {
    constexpr uint32_t halfBg = 1u << (BGBIT - 1);
    uint32_t dec_offset = 0;
#pragma unroll
    for (int q = 1; q <= L; q++) dec_offset += halfBg << (32 - q * BGBIT);
    return dec_offset;
}
template <int BGBIT>
__device__ __forceinline__ int32_t signed_digit(uint32_t v, int sh) {
    return __builtin_amdgcn_sbfe((int32_t)v, sh, BGBIT);  // v_bfe_i32
}
// one digit of this lane's 16 coefficients, as the forward transform's input
template <int BGBIT>
__device__ __forceinline__ void digits_to_double2(double2 (&x)[8], const uint32_t (&v0)[8], const uint32_t (&v1)[8], int sh) {
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int32_t e0 = signed_digit<BGBIT>(v0[r], sh), e1 = signed_digit<BGBIT>(v1[r], sh);
        x[r] = make_double2((double)e0, (double)e1);  // untwisted: the first radix-8 pass applies e^{i pi r/16} itself
    }
}

// (X^a - 1) acc + offset where the accumulators stand FIRST in the workgroup's LDS, each polynomial on a 4 KiB boundary
// (accb = LDS offset 0, pb = the polynomial's byte offset).  Lane value per step: the byte offset of coefficient (lane - a)
// in the 2N-ring [acc, -acc] -- bits 2..11 address, bit 12 = negate.  For register r, t = that + 256 r: the byte address of
// coefficient (j - a) mod N is one v_and_or_b32 (t & 4092 | pb), the address of coefficient j + 512 is that address ^ 2048,
// and the negacyclic sign m (all ones where the rotation wrapped) is a v_bfe_i32 of t, resp. t + 2048.
// ... for this lane's 16 coefficients of the polynomial at accp = accb + pb, ^ offset: every digit's field ready for signed_digit
__device__ __forceinline__ void decompose_rotated(uint32_t (&v0)[8], uint32_t (&v1)[8], const unsigned char* accb, const int32_t* accp,
                                                  uint32_t pb, uint32_t jb4, int lane, uint32_t dec_offset) {
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const uint32_t t = jb4 + 256u * r;
        const uint32_t o0 = (t & 4092u) | pb, o1 = o0 ^ 2048u;
        const int32_t m0 = __builtin_amdgcn_sbfe((int32_t)t, 12, 1), m1 = __builtin_amdgcn_sbfe((int32_t)(t + 2048u), 12, 1);
        const uint32_t rv0 = *reinterpret_cast<const uint32_t*>(accb + o0), rv1 = *reinterpret_cast<const uint32_t*>(accb + o1);
        const uint32_t pv0 = (uint32_t)accp[64 * r + lane], pv1 = (uint32_t)accp[64 * r + lane + kM];
        // +/- rot - acc_j + offset, formed as (rot ^ m) + ((offset - acc_j) - m)  (v_xad_u32); then ^ offset: every digit's field
        // is ready for signed_digit
        v0[r] = ((rv0 ^ (uint32_t)m0) + ((dec_offset - pv0) - (uint32_t)m0)) ^ dec_offset;
        v1[r] = ((rv1 ^ (uint32_t)m1) + ((dec_offset - pv1) - (uint32_t)m1)) ^ dec_offset;
    }
}

// ---- spectrum row product ----
// s (+)= x * b; FIRST: the product initialises the sum (digit 0 of a step), so nothing has to be zeroed
template <bool FIRST>
__device__ __forceinline__ double2 mac(double2 s, double2 x, double2 b) {
    return FIRST ? cmulx<false>(x, b) : make_double2(fma(x.x, b.x, fma(-x.y, b.y, s.x)), fma(x.x, b.y, fma(x.y, b.x, s.y)));
}
// ... for the 8 registers of a row
template <bool FIRST>
__device__ __forceinline__ void mac_row(double2 (&s)[8], const double2 (&x)[8], const double2 (&b)[8]) {
#pragma unroll
    for (int k = 0; k < 8; k++) s[k] = mac<FIRST>(s[k], x[k], b[k]);
}

// ---- one digit row on the two-limb spectrum (k_blind_rotate_x1 and the CMux family: cmux.hip, rotate.hip) ----
// The digit at shift `sh` of the decomposed words, transformed, times the row's four blocks [q = 2 c + limb] at byte offset
// brow of the resource, into the four sums s[q].  With the sums taking half the register file only two BK blocks are in
// flight at a time: block 0 is requested inside the forward transform (once the second twiddle set is consumed), block 1
// behind it, block q + 2 when block q has been multiplied (re-requesting register by register, right behind the products
// that consumed each one, measured the same: profiles/r4_x1_ab.txt).
template <int BGBIT, bool FIRST>
__device__ __forceinline__ void digit_row_two_limb(double2 (&s)[4][8], const uint32_t (&v0)[8], const uint32_t (&v1)[8], int sh,
                                                   __amdgpu_buffer_rsrc_t bk_rsrc, int lane16, int brow, double2* sT, int lane, const LaneRoots& R) {
    constexpr int kBlockBytes = kM * (int)sizeof(double2);
    double2 x[8], bA[8], bB[8];
    digits_to_double2<BGBIT>(x, v0, v1, sh);
    __builtin_amdgcn_sched_barrier(0);
    auto req = [&]() { load_bk_block(bA, bk_rsrc, lane16, brow); };  // block 0: output 0, low limb
    fft512_forward<true, 1, decltype(req), true>(x, sT, lane, R, req);
    load_bk_block(bB, bk_rsrc, lane16, brow + kBlockBytes);          // block 1: output 0, high limb
    __builtin_amdgcn_sched_barrier(0);
    mac_row<FIRST>(s[0], x, bA);
    __builtin_amdgcn_sched_barrier(0);
    load_bk_block(bA, bk_rsrc, lane16, brow + 2 * kBlockBytes);      // block 2: output 1, low limb
    __builtin_amdgcn_sched_barrier(0);
    mac_row<FIRST>(s[1], x, bB);
    __builtin_amdgcn_sched_barrier(0);
    load_bk_block(bB, bk_rsrc, lane16, brow + 3 * kBlockBytes);      // block 3: output 1, high limb
    __builtin_amdgcn_sched_barrier(0);
    mac_row<FIRST>(s[2], x, bA);
    mac_row<FIRST>(s[3], x, bB);
}
// ---- the same with the gadget (l, Bgbit) a launch argument (the run-time builds of the CMux family: cmux.hip, rotate.hip) ----
// Siblings, not a parameter of the pieces above: those keep their code.  l and bgbit are wave-uniform (SGPRs); the width operand
// of v_bfe_i32 may be a register, the offset is formed once per wave.
__device__ __forceinline__ uint32_t decomposition_offset_rt(int l, int bgbit) {
    const uint32_t halfBg = 1u << (bgbit - 1);
    uint32_t dec_offset = 0;
#pragma unroll 1
    for (int q = 1; q <= l; q++) dec_offset += halfBg << (32 - q * bgbit);
    return dec_offset;
}
template <bool FIRST>
__device__ __forceinline__ void digit_row_two_limb_rt(double2 (&s)[4][8], const uint32_t (&v0)[8], const uint32_t (&v1)[8], int sh, int bgbit,
                                                      __amdgpu_buffer_rsrc_t bk_rsrc, int lane16, int brow, double2* sT, int lane, const LaneRoots& R) {
    constexpr int kBlockBytes = kM * (int)sizeof(double2);
    double2 x[8], bA[8], bB[8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int32_t e0 = __builtin_amdgcn_sbfe((int32_t)v0[r], sh, bgbit), e1 = __builtin_amdgcn_sbfe((int32_t)v1[r], sh, bgbit);
        x[r] = make_double2((double)e0, (double)e1);
    }
    __builtin_amdgcn_sched_barrier(0);
    auto req = [&]() { load_bk_block(bA, bk_rsrc, lane16, brow); };
    fft512_forward<true, 1, decltype(req), true>(x, sT, lane, R, req);
    load_bk_block(bB, bk_rsrc, lane16, brow + kBlockBytes);
    __builtin_amdgcn_sched_barrier(0);
    mac_row<FIRST>(s[0], x, bA);
    __builtin_amdgcn_sched_barrier(0);
    load_bk_block(bA, bk_rsrc, lane16, brow + 2 * kBlockBytes);
    __builtin_amdgcn_sched_barrier(0);
    mac_row<FIRST>(s[1], x, bB);
    __builtin_amdgcn_sched_barrier(0);
    load_bk_block(bB, bk_rsrc, lane16, brow + 3 * kBlockBytes);
    __builtin_amdgcn_sched_barrier(0);
    mac_row<FIRST>(s[2], x, bA);
    mac_row<FIRST>(s[3], x, bB);
}

// ... and a coefficient back from its two inverse-transformed limb sums: lo + (hi << 16) mod 2^32, register q's gain folded
// into the rounding.  Nothing to watch: every rounded sum is below 2^37 of the 2^53 an FP64 mantissa holds.
__device__ __forceinline__ uint32_t join_limbs(double lo, double hi, int q) {
    double unused = 0.0;
    return round_coef(lo, untwist_gain(q), false, unused) + (round_coef(hi, untwist_gain(q), false, unused) << 16);
}

// ---- phase stamps of the diagnostic builds (br_variant 8 / 49): s_memtime ticks since the last stamp, summed per segment ----
template <bool DIAG>
__device__ __forceinline__ void stamp_phase(unsigned long long (&tsum)[8], unsigned long long& tlast, int idx) {
    if (DIAG) {
        const unsigned long long t_ = stamp();
        tsum[idx] += t_ - tlast;
        tlast = t_;
    }
}

}  // namespace
}  // namespace w64
}  // namespace ieache
