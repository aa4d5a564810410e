// The CMux on TGSW samples the caller supplies (include/ieache.h section 3f): out = d0 + C_sel [.] (d1 - d0), the external
// product of libtfhe's tGswExternMulToTLwe on the provably exact two-limb spectrum -- k_blind_rotate_x1's step
// (blind_rotate_w64.hip) with the operand taken from global memory instead of a rotating LDS accumulator and the key block
// chosen per row.  Built from the pieces of br_step.h and fft512.h, which that kernel uses too, and of cmux_step.h.
// N = 1024, k = 1; libtfhe's two (l, Bgbit) as template arguments (k_cmux_x1, k_demux_x1) and every other admissible gadget of a
// set as launch arguments (k_cmux_rt, k_demux_rt: section 3i); the extraction kernel at the end takes any set.
// k_demux_x1 is the same product as a demultiplexer: the write at an encrypted index (section 3g); k_demux_acc is its last step
// with the children added into shared memories by atomic adds: many values into one memory in one call (section 3j).
#include "cmux.h"

#include <atomic>
#include <memory>
#include <stdexcept>
#include <type_traits>

#include "blind_rotate_w64.h"
#include "cmux_step.h"

namespace ieache {

using namespace dev;
using namespace w64;

namespace {

// ---- one CMux per wave ----
// Per row: 2L forward transforms of the digits of d1 - d0, 4 x 2L row products against block `sel` of the set's spectrum into
// the four sums s[2 c + limb], two interleaved pairs of inverse transforms, the limbs recombined as lo + (hi << 16) mod 2^32,
// d0 added, vector stores.  Every rounded sum stays below 2L x 1024 x 2^(BGBIT-1) x 2^15 <= 2^37 of the 2^53 an FP64 mantissa
// holds, so the words are exact for ANY caller words: no guard.
//   * there is no rotation, so no LDS accumulator: the lane reads its 16 coefficients of d1 and d0 per polynomial (j = 64 r +
//     lane and j + 512: the forward transform's own (register, lane) order, 256 contiguous bytes per load) straight into
//     registers and forms ((d1 - d0) + offset) ^ offset, every digit's field ready for signed_digit;
//   * d0 is NOT kept across the products (32 registers the four sums leave no room for): the epilogue reads it again (16 more
//     loads per polynomial, which the caches are left to serve; kept in registers it spilled);
//   * the selector, the row rule and with them every base address are wave-uniform: the spectrum block goes into the buffer
//     resource's base (sel x step bytes), the rows of a block into the scalar offset, as for BK_i;
//   * BK loads as in k_blind_rotate_x1: block 0 of a row requested inside its forward transform, block q + 2 when block q has
//     been multiplied; forward transforms' lane-high transpose cross-lane, everything else through the wave's tile.
// G = 4 rows per workgroup share the twiddle table only; one workgroup barrier (after the table is in LDS).
// hipcc reports 252 VGPRs, no scratch, for both parameter sets -> 2 waves per SIMD, 8 rows per CU, the bound stated to the
// compiler as __launch_bounds__(256, 2); LDS is static: sT [4][kTile] | tw [kTwElems] double2 = 46 080 B, three workgroups' worth
// per CU, so the registers bind, not the LDS.  G = 8 would halve the table copies per row and changes nothing else; not measured.
template <int L, int BGBIT, int G = kCmuxWaveRows>
__global__ __launch_bounds__(64 * G, 2) void k_cmux_x1(CmuxRows A, const double2* __restrict__ bkf, const double2* __restrict__ gtw) {
    __shared__ __align__(16) double2 sT_all[G * kTile];
    __shared__ __align__(16) double2 sTw[kTwElems];
    const WaveRow W = wave_prologue<G>(sT_all, sTw, gtw);
    const int lane = W.lane;
    double2* sT = W.sT;
    const int64_t r = W.r;
    if (r >= A.rows) return;
    const LaneRoots R = make_roots(sTw, lane);

    // row r -> (d1, d0, selector): all wave-uniform
    const int32_t* p1;
    const int32_t* p0;
    int64_t sel;
    bool implied;
    if (A.depth < 0) {
        p1 = A.src + (size_t)r * 2 * kN;
        p0 = A.src0 ? A.src0 + (size_t)r * 2 * kN : nullptr;
        implied = A.sel_of == nullptr;
        sel = implied ? A.item0 + r : (int64_t)A.sel_of[r];
    } else {
        const int64_t item = r / A.width, pair = r - item * A.width;
        int64_t block = item;
        if (A.shared) block = clamp_index(A.table_of ? (int64_t)A.table_of[A.item0 + item] : 0, A.n_tables);
        p0 = A.src + ((size_t)block * 2 * A.width + 2 * (size_t)pair) * 2 * kN;
        p1 = p0 + 2 * kN;
        const int64_t at = (A.item0 + item) * A.depth + A.level;
        implied = A.sel_of == nullptr;
        sel = implied ? at : (int64_t)A.sel_of[at];
    }
    // selector_at's rule (cmux_step.h), open-coded: the flat form reads the piece's array at r but implies the call's item0 + r
    if (implied)
        sel %= A.n_set;
    else
        sel = clamp_index(sel, A.n_set);
    int32_t* po = A.dst + (size_t)r * 2 * kN;
    // d0 = zeros: the loads read d1's words instead and a wave-uniform mask clears them -- no branch per load
    const uint32_t keep0 = p0 ? 0xFFFFFFFFu : 0u;
    if (!p0) p0 = p1;
    // rows through the buffer path as well: resource (the row's 8 KB, so nothing past it can be touched) and word offset in
    // SGPRs, the lane's 4 bytes the only vector operand -- as plain global accesses the 48 of them each got a 64-bit vector
    // address, which the kernel spilled
    const __amdgpu_buffer_rsrc_t r1 = row_resource(p1), r0 = row_resource(p0), ro = row_resource(po);
    const int lane4 = lane * 4;

    constexpr int kBlockBytes = kM * (int)sizeof(double2), kRowBytes = 4 * kBlockBytes, kStepBytes = 2 * L * kRowBytes;
    // the resource covers the selected sample only: its rows [2L][q = 2 c + limb][8][64] double2
    const __amdgpu_buffer_rsrc_t bk_rsrc = bk_resource(bkf + (size_t)sel * (kStepBytes / sizeof(double2)), 1, kStepBytes);
    const int lane16 = bk_lane_offset(lane);
    const uint32_t dec_offset = decomposition_offset<L, BGBIT>();

    double2 s[4][8];
    uint32_t v0[8], v1[8];
    auto decompose = [&](const int c) {
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int j = c * kN + 64 * q;
            const uint32_t a0 = row_word(r0, lane4, j) & keep0, a1 = row_word(r0, lane4, j + kM) & keep0;
            v0[q] = ((row_word(r1, lane4, j) - a0) + dec_offset) ^ dec_offset;
            v1[q] = ((row_word(r1, lane4, j + kM) - a1) + dec_offset) ^ dec_offset;
        }
    };
    auto digit_row = [&](const int sh, const int brow, auto first) {
        digit_row_two_limb<BGBIT, decltype(first)::value>(s, v0, v1, sh, bk_rsrc, lane16, brow, sT, lane, R);
    };
    decompose(0);
    digit_row(32 - BGBIT, 0, std::true_type{});
    // ONE loop over the other 2L - 1 rows, the second decomposition inside it: as two loops, the L = 2 build (one trip each) became
    // straight-line code whose BK requests the compiler gathered at the top and spilled (287 VGPRs)
#pragma unroll 1
    for (int row = 1; row < 2 * L; row++) {
        const int c = row >= L ? 1 : 0, q = row - c * L;
        if (q == 0) decompose(1);
        digit_row(32 - (q + 1) * BGBIT, row * kRowBytes, std::false_type{});
    }
    // opaque copy: d0 is read AGAIN below.  Through the same pointer the compiler would keep the 32 words it loaded for the
    // decompositions alive across every product instead -- registers this kernel does not have (they were spilled)
    const int32_t* p0e = p0;
    asm volatile("" : "+s"(p0e));
    const __amdgpu_buffer_rsrc_t r0e = row_resource(p0e);
    // back to coefficients: s[2 c] / s[2 c + 1] hold the low / high limb sums of output polynomial c
#pragma unroll
    for (int c = 0; c < 2; c++) {
        fft512_inverse_pair<true>(s[2 * c], s[2 * c + 1], sT, lane, R);
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const uint32_t e0 = join_limbs(s[2 * c][q].x, s[2 * c + 1][q].x, q), e1 = join_limbs(s[2 * c][q].y, s[2 * c + 1][q].y, q);
            const int j = c * kN + 64 * q;
            const uint32_t a0 = row_word(r0e, lane4, j) & keep0, a1 = row_word(r0e, lane4, j + kM) & keep0;
            __builtin_amdgcn_raw_buffer_store_b32(a0 + e0, ro, lane4, j * 4, 0);
            __builtin_amdgcn_raw_buffer_store_b32(a1 + e1, ro, lane4, (j + kM) * 4, 0);
        }
    }
}

// ---- one demux step per wave: the scatter of include/ieache.h section 3g ----
// Parent row p splits into hi = C_sel [.] p (child 2 r + 1) and lo = p - hi (child 2 r): k_cmux_x1's body with no d0 -- the
// digits are those of p itself -- and another epilogue.  What the two share is stated once -- the wave prologue, the selector
// rule and the rows of cmux_step.h, the digit row and the limb recombination of br_step.h -- and each keeps its own
// decomposition, its three-line loop over the digit rows (one helper over that loop moved both kernels' code) and its epilogue.
//   * p is NOT kept across the products; the epilogue reads it again through an opaque copy of its pointer, for k_cmux_x1's
//     reason (kept live, its 32 words were spilled);
//   * the last step of a scatter adds the memory: base rows 2 r and 2 r + 1 are read here and the sums stored, so no separate
//     add pass moves 2 x 16 KB per parent more than the products do.  base null (no memory, or an earlier step) is a
//     wave-uniform branch around those loads;
//   * IN PLACE (base == dst) is sound: child row c of parent r is words [2 r + c][j], and the lane that stores word j of it is
//     the only lane of the whole launch that reads word j of base row 2 r + c (rows are disjoint between waves, j = 64 q' + lane
//     belongs to one lane), and its load stands before its store in program order on the same buffer path, which the compiler
//     does not exchange (the two may alias).  No other word of base is touched by anyone.  The parent rows never overlap dst:
//     they are the caller's values, which the host refuses over the output, or the other scratch buffer.
// Rows through 8 KB buffer resources as in k_cmux_x1, so nothing past a row can be touched whatever the indices hold.
template <int L, int BGBIT, int G = kCmuxWaveRows>
__global__ __launch_bounds__(64 * G, 2) void k_demux_x1(DemuxRows A, const double2* __restrict__ bkf, const double2* __restrict__ gtw) {
    __shared__ __align__(16) double2 sT_all[G * kTile];
    __shared__ __align__(16) double2 sTw[kTwElems];
    const WaveRow W = wave_prologue<G>(sT_all, sTw, gtw);
    const int lane = W.lane;
    double2* sT = W.sT;
    const int64_t r = W.r;
    if (r >= A.rows) return;
    const LaneRoots R = make_roots(sTw, lane);

    // row r -> (parent, children, base rows, selector): all wave-uniform
    const int64_t item = r / A.width;
    const int64_t sel = selector_at(A.sel_of, (A.item0 + item) * A.depth + (A.depth - 1 - A.step), A.n_set);
    const int32_t* pp = A.src + (size_t)r * 2 * kN;
    int32_t* po = A.dst + (size_t)r * 4 * kN;
    const bool add = A.base != nullptr;
    const int32_t* pb = add ? A.base + (size_t)r * 4 * kN : pp;  // never read when !add: any valid row will do for the resource
    const __amdgpu_buffer_rsrc_t rp = row_resource(pp);
    const int lane4 = lane * 4;

    constexpr int kBlockBytes = kM * (int)sizeof(double2), kRowBytes = 4 * kBlockBytes, kStepBytes = 2 * L * kRowBytes;
    const __amdgpu_buffer_rsrc_t bk_rsrc = bk_resource(bkf + (size_t)sel * (kStepBytes / sizeof(double2)), 1, kStepBytes);
    const int lane16 = bk_lane_offset(lane);
    const uint32_t dec_offset = decomposition_offset<L, BGBIT>();

    double2 s[4][8];
    uint32_t v0[8], v1[8];
    auto decompose = [&](const int c) {
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int j = c * kN + 64 * q;
            v0[q] = (row_word(rp, lane4, j) + dec_offset) ^ dec_offset;
            v1[q] = (row_word(rp, lane4, j + kM) + dec_offset) ^ dec_offset;
        }
    };
    auto digit_row = [&](const int sh, const int brow, auto first) {
        digit_row_two_limb<BGBIT, decltype(first)::value>(s, v0, v1, sh, bk_rsrc, lane16, brow, sT, lane, R);
    };
    decompose(0);
    digit_row(32 - BGBIT, 0, std::true_type{});
    // one loop over the other 2L - 1 rows, as in k_cmux_x1 and for its reason
#pragma unroll 1
    for (int row = 1; row < 2 * L; row++) {
        const int c = row >= L ? 1 : 0, q = row - c * L;
        if (q == 0) decompose(1);
        digit_row(32 - (q + 1) * BGBIT, row * kRowBytes, std::false_type{});
    }
    // opaque copies: the parent is read AGAIN below, and the children's and the base rows' addresses are formed only now
    const int32_t* ppe = pp;
    asm volatile("" : "+s"(ppe));
    asm volatile("" : "+s"(po));
    asm volatile("" : "+s"(pb));
    const __amdgpu_buffer_rsrc_t rpe = row_resource(ppe);
    const __amdgpu_buffer_rsrc_t ro0 = row_resource(po), ro1 = row_resource(po + 2 * kN);
    const __amdgpu_buffer_rsrc_t rb0 = row_resource(pb), rb1 = row_resource(pb + 2 * kN);
#pragma unroll
    for (int c = 0; c < 2; c++) {
        fft512_inverse_pair<true>(s[2 * c], s[2 * c + 1], sT, lane, R);
        uint32_t h0[8], h1[8];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            h0[q] = join_limbs(s[2 * c][q].x, s[2 * c + 1][q].x, q);
            h1[q] = join_limbs(s[2 * c][q].y, s[2 * c + 1][q].y, q);
        }
        if (add) {
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const int j = c * kN + 64 * q;
                const uint32_t p0 = row_word(rpe, lane4, j), p1 = row_word(rpe, lane4, j + kM);
                const uint32_t b00 = row_word(rb0, lane4, j), b01 = row_word(rb0, lane4, j + kM);
                const uint32_t b10 = row_word(rb1, lane4, j), b11 = row_word(rb1, lane4, j + kM);
                __builtin_amdgcn_raw_buffer_store_b32(b00 + (p0 - h0[q]), ro0, lane4, j * 4, 0);
                __builtin_amdgcn_raw_buffer_store_b32(b01 + (p1 - h1[q]), ro0, lane4, (j + kM) * 4, 0);
                __builtin_amdgcn_raw_buffer_store_b32(b10 + h0[q], ro1, lane4, j * 4, 0);
                __builtin_amdgcn_raw_buffer_store_b32(b11 + h1[q], ro1, lane4, (j + kM) * 4, 0);
            }
        } else {
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const int j = c * kN + 64 * q;
                const uint32_t p0 = row_word(rpe, lane4, j), p1 = row_word(rpe, lane4, j + kM);
                __builtin_amdgcn_raw_buffer_store_b32(p0 - h0[q], ro0, lane4, j * 4, 0);
                __builtin_amdgcn_raw_buffer_store_b32(p1 - h1[q], ro0, lane4, (j + kM) * 4, 0);
                __builtin_amdgcn_raw_buffer_store_b32(h0[q], ro1, lane4, j * 4, 0);
                __builtin_amdgcn_raw_buffer_store_b32(h1[q], ro1, lane4, (j + kM) * 4, 0);
            }
        }
    }
}

// ---- the two kernels once more with the set's gadget (l, bgbit) as launch arguments ----
// A set prepared with a gadget of its own (ieache_tgsw_prepare_gadget) that is not one of the two above runs here.  The bodies
// are k_cmux_x1's and k_demux_x1's line for line -- what those say about registers, the buffer path, the opaque copies and the
// write in place holds here and is not repeated -- with four differences, all wave-uniform: the decomposition offset comes
// from decomposition_offset_rt, the digit row is digit_row_two_limb_rt (the width of its v_bfe_i32 a register), the bytes
// of a sample in the set are 2 l kRowBytes computed once, and the row loop runs to 2 l.  They are copies and not a parameter
// of the kernels above because those must keep their code (br_step.h's rule).  Exactness: 2 l x 1024 x 2^(bgbit-1) x 2^15 <= 2^46
// of 2^53 for every gadget the door admits (l bgbit <= 32, 2 l N 2^bgbit <= 2^32), so no guard here either.
template <int G = kCmuxWaveRows>
__global__ __launch_bounds__(64 * G, 2) void k_cmux_rt(CmuxRows A, const double2* __restrict__ bkf, const double2* __restrict__ gtw, int l, int bgbit) {
    __shared__ __align__(16) double2 sT_all[G * kTile];
    __shared__ __align__(16) double2 sTw[kTwElems];
    const WaveRow W = wave_prologue<G>(sT_all, sTw, gtw);
    const int lane = W.lane;
    double2* sT = W.sT;
    const int64_t r = W.r;
    if (r >= A.rows) return;
    const LaneRoots R = make_roots(sTw, lane);

    const int32_t* p1;
    const int32_t* p0;
    int64_t sel;
    bool implied;
    if (A.depth < 0) {
        p1 = A.src + (size_t)r * 2 * kN;
        p0 = A.src0 ? A.src0 + (size_t)r * 2 * kN : nullptr;
        implied = A.sel_of == nullptr;
        sel = implied ? A.item0 + r : (int64_t)A.sel_of[r];
    } else {
        const int64_t item = r / A.width, pair = r - item * A.width;
        int64_t block = item;
        if (A.shared) block = clamp_index(A.table_of ? (int64_t)A.table_of[A.item0 + item] : 0, A.n_tables);
        p0 = A.src + ((size_t)block * 2 * A.width + 2 * (size_t)pair) * 2 * kN;
        p1 = p0 + 2 * kN;
        const int64_t at = (A.item0 + item) * A.depth + A.level;
        implied = A.sel_of == nullptr;
        sel = implied ? at : (int64_t)A.sel_of[at];
    }
    if (implied)
        sel %= A.n_set;
    else
        sel = clamp_index(sel, A.n_set);
    int32_t* po = A.dst + (size_t)r * 2 * kN;
    const uint32_t keep0 = p0 ? 0xFFFFFFFFu : 0u;
    if (!p0) p0 = p1;
    const __amdgpu_buffer_rsrc_t r1 = row_resource(p1), r0 = row_resource(p0), ro = row_resource(po);
    const int lane4 = lane * 4;

    constexpr int kBlockBytes = kM * (int)sizeof(double2), kRowBytes = 4 * kBlockBytes;
    const int rows2l = 2 * l, step_bytes = rows2l * kRowBytes;
    const __amdgpu_buffer_rsrc_t bk_rsrc = bk_resource(bkf + (size_t)sel * ((size_t)step_bytes / sizeof(double2)), 1, step_bytes);
    const int lane16 = bk_lane_offset(lane);
    const uint32_t dec_offset = decomposition_offset_rt(l, bgbit);

    double2 s[4][8];
    uint32_t v0[8], v1[8];
    auto decompose = [&](const int c) {
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int j = c * kN + 64 * q;
            const uint32_t a0 = row_word(r0, lane4, j) & keep0, a1 = row_word(r0, lane4, j + kM) & keep0;
            v0[q] = ((row_word(r1, lane4, j) - a0) + dec_offset) ^ dec_offset;
            v1[q] = ((row_word(r1, lane4, j + kM) - a1) + dec_offset) ^ dec_offset;
        }
    };
    decompose(0);
    digit_row_two_limb_rt<true>(s, v0, v1, 32 - bgbit, bgbit, bk_rsrc, lane16, 0, sT, lane, R);
#pragma unroll 1
    for (int row = 1; row < rows2l; row++) {
        const int c = row >= l ? 1 : 0, q = row - c * l;
        if (q == 0) decompose(1);
        digit_row_two_limb_rt<false>(s, v0, v1, 32 - (q + 1) * bgbit, bgbit, bk_rsrc, lane16, row * kRowBytes, sT, lane, R);
    }
    const int32_t* p0e = p0;
    asm volatile("" : "+s"(p0e));
    const __amdgpu_buffer_rsrc_t r0e = row_resource(p0e);
#pragma unroll
    for (int c = 0; c < 2; c++) {
        fft512_inverse_pair<true>(s[2 * c], s[2 * c + 1], sT, lane, R);
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const uint32_t e0 = join_limbs(s[2 * c][q].x, s[2 * c + 1][q].x, q), e1 = join_limbs(s[2 * c][q].y, s[2 * c + 1][q].y, q);
            const int j = c * kN + 64 * q;
            const uint32_t a0 = row_word(r0e, lane4, j) & keep0, a1 = row_word(r0e, lane4, j + kM) & keep0;
            __builtin_amdgcn_raw_buffer_store_b32(a0 + e0, ro, lane4, j * 4, 0);
            __builtin_amdgcn_raw_buffer_store_b32(a1 + e1, ro, lane4, (j + kM) * 4, 0);
        }
    }
}

template <int G = kCmuxWaveRows>
__global__ __launch_bounds__(64 * G, 2) void k_demux_rt(DemuxRows A, const double2* __restrict__ bkf, const double2* __restrict__ gtw, int l, int bgbit) {
    __shared__ __align__(16) double2 sT_all[G * kTile];
    __shared__ __align__(16) double2 sTw[kTwElems];
    const WaveRow W = wave_prologue<G>(sT_all, sTw, gtw);
    const int lane = W.lane;
    double2* sT = W.sT;
    const int64_t r = W.r;
    if (r >= A.rows) return;
    const LaneRoots R = make_roots(sTw, lane);

    const int64_t item = r / A.width;
    const int64_t sel = selector_at(A.sel_of, (A.item0 + item) * A.depth + (A.depth - 1 - A.step), A.n_set);
    const int32_t* pp = A.src + (size_t)r * 2 * kN;
    int32_t* po = A.dst + (size_t)r * 4 * kN;
    const bool add = A.base != nullptr;
    const int32_t* pb = add ? A.base + (size_t)r * 4 * kN : pp;
    const __amdgpu_buffer_rsrc_t rp = row_resource(pp);
    const int lane4 = lane * 4;

    constexpr int kBlockBytes = kM * (int)sizeof(double2), kRowBytes = 4 * kBlockBytes;
    const int rows2l = 2 * l, step_bytes = rows2l * kRowBytes;
    const __amdgpu_buffer_rsrc_t bk_rsrc = bk_resource(bkf + (size_t)sel * ((size_t)step_bytes / sizeof(double2)), 1, step_bytes);
    const int lane16 = bk_lane_offset(lane);
    const uint32_t dec_offset = decomposition_offset_rt(l, bgbit);

    double2 s[4][8];
    uint32_t v0[8], v1[8];
    auto decompose = [&](const int c) {
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int j = c * kN + 64 * q;
            v0[q] = (row_word(rp, lane4, j) + dec_offset) ^ dec_offset;
            v1[q] = (row_word(rp, lane4, j + kM) + dec_offset) ^ dec_offset;
        }
    };
    decompose(0);
    digit_row_two_limb_rt<true>(s, v0, v1, 32 - bgbit, bgbit, bk_rsrc, lane16, 0, sT, lane, R);
#pragma unroll 1
    for (int row = 1; row < rows2l; row++) {
        const int c = row >= l ? 1 : 0, q = row - c * l;
        if (q == 0) decompose(1);
        digit_row_two_limb_rt<false>(s, v0, v1, 32 - (q + 1) * bgbit, bgbit, bk_rsrc, lane16, row * kRowBytes, sT, lane, R);
    }
    const int32_t* ppe = pp;
    asm volatile("" : "+s"(ppe));
    asm volatile("" : "+s"(po));
    asm volatile("" : "+s"(pb));
    const __amdgpu_buffer_rsrc_t rpe = row_resource(ppe);
    const __amdgpu_buffer_rsrc_t ro0 = row_resource(po), ro1 = row_resource(po + 2 * kN);
    const __amdgpu_buffer_rsrc_t rb0 = row_resource(pb), rb1 = row_resource(pb + 2 * kN);
#pragma unroll
    for (int c = 0; c < 2; c++) {
        fft512_inverse_pair<true>(s[2 * c], s[2 * c + 1], sT, lane, R);
        uint32_t h0[8], h1[8];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            h0[q] = join_limbs(s[2 * c][q].x, s[2 * c + 1][q].x, q);
            h1[q] = join_limbs(s[2 * c][q].y, s[2 * c + 1][q].y, q);
        }
        if (add) {
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const int j = c * kN + 64 * q;
                const uint32_t p0 = row_word(rpe, lane4, j), p1 = row_word(rpe, lane4, j + kM);
                const uint32_t b00 = row_word(rb0, lane4, j), b01 = row_word(rb0, lane4, j + kM);
                const uint32_t b10 = row_word(rb1, lane4, j), b11 = row_word(rb1, lane4, j + kM);
                __builtin_amdgcn_raw_buffer_store_b32(b00 + (p0 - h0[q]), ro0, lane4, j * 4, 0);
                __builtin_amdgcn_raw_buffer_store_b32(b01 + (p1 - h1[q]), ro0, lane4, (j + kM) * 4, 0);
                __builtin_amdgcn_raw_buffer_store_b32(b10 + h0[q], ro1, lane4, j * 4, 0);
                __builtin_amdgcn_raw_buffer_store_b32(b11 + h1[q], ro1, lane4, (j + kM) * 4, 0);
            }
        } else {
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const int j = c * kN + 64 * q;
                const uint32_t p0 = row_word(rpe, lane4, j), p1 = row_word(rpe, lane4, j + kM);
                __builtin_amdgcn_raw_buffer_store_b32(p0 - h0[q], ro0, lane4, j * 4, 0);
                __builtin_amdgcn_raw_buffer_store_b32(p1 - h1[q], ro0, lane4, (j + kM) * 4, 0);
                __builtin_amdgcn_raw_buffer_store_b32(h0[q], ro1, lane4, j * 4, 0);
                __builtin_amdgcn_raw_buffer_store_b32(h1[q], ro1, lane4, (j + kM) * 4, 0);
            }
        }
    }
}

// ---- the accumulating demux step: the LAST step of a piece of lut_add (include/ieache.h section 3j) ----
// k_demux_x1's body -- prologue, selector rule, decomposition, digit rows, inverse transforms, the parent read again through an
// opaque copy -- with a third epilogue: child c of parent r of item i is not stored at 2 r + c of the piece's own rows but
// ADDED into row 2 j + c of the memory the item names (DemuxAccRows: the rule, no pointer tables, everything wave-uniform), with
// integer atomic adds that return nothing.
//   * nothing of `out` is read, so any number of waves of any number of launches may add into one row: the sums are mod 2^32,
//     which is commutative and associative, so the words are determined whatever the order the adds arrive in (what
//     k_pack_gemm's K splits rest on) -- no float, no order, no run-to-run difference;
//   * one atomic instruction of the wave covers words 64 q + lane of a row half: 256 contiguous bytes, the shape the adds run
//     fastest in; the rows are again 8 KB buffer resources, the memory index clamped, so nothing past a row of `out` can be
//     touched whatever mem_of holds;
//   * a new kernel and not a flag of k_demux_x1, which must keep its code (br_step.h's rule).  Being new it states the body
//     ONCE for the three builds: L > 0 takes the compile-time digit row, L == 0 the run-time one (k_demux_rt's differences).
// hipcc: the register and LDS figures are in DESIGN.md section 4.11; __launch_bounds__(256, 2) as the family's.
template <int L, int BGBIT, int G>
__device__ __forceinline__ void demux_acc_body(const DemuxAccRows& A, const double2* __restrict__ bkf, const double2* __restrict__ gtw, const int l,
                                               const int bgbit, double2* sT_all, double2* sTw) {
    const WaveRow W = wave_prologue<G>(sT_all, sTw, gtw);
    const int lane = W.lane;
    double2* sT = W.sT;
    const int64_t r = W.r;
    if (r >= A.rows) return;
    const LaneRoots R = make_roots(sTw, lane);

    // row r -> (parent, the two rows of the item's memory, selector): all wave-uniform
    const int64_t item = r / A.width, j = r - item * A.width;
    const int64_t sel = selector_at(A.sel_of, item * A.depth + (A.depth - 1 - A.step), A.n_set);
    const int64_t m0 = A.mem_of ? (int64_t)A.mem_of[item] : 0;
    const int64_t m = m0 < 0 ? 0 : (m0 >= A.n_mems ? A.n_mems - 1 : m0);
    const int32_t* pp = A.src + (size_t)r * 2 * kN;
    int32_t* po = A.out + (((size_t)m << A.depth) + 2 * (size_t)j) * 2 * kN;
    const __amdgpu_buffer_rsrc_t rp = row_resource(pp);
    const int lane4 = lane * 4;

    constexpr int kBlockBytes = kM * (int)sizeof(double2), kRowBytes = 4 * kBlockBytes;
    const int rows2l = L > 0 ? 2 * L : 2 * l, half = L > 0 ? L : l, width = L > 0 ? BGBIT : bgbit, step_bytes = rows2l * kRowBytes;
    const __amdgpu_buffer_rsrc_t bk_rsrc = bk_resource(bkf + (size_t)sel * ((size_t)step_bytes / sizeof(double2)), 1, step_bytes);
    const int lane16 = bk_lane_offset(lane);
    uint32_t dec_offset;
    if constexpr (L > 0)
        dec_offset = decomposition_offset<L, BGBIT>();
    else
        dec_offset = decomposition_offset_rt(l, bgbit);

    double2 s[4][8];
    uint32_t v0[8], v1[8];
    auto decompose = [&](const int c) {
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int jj = c * kN + 64 * q;
            v0[q] = (row_word(rp, lane4, jj) + dec_offset) ^ dec_offset;
            v1[q] = (row_word(rp, lane4, jj + kM) + dec_offset) ^ dec_offset;
        }
    };
    auto digit_row = [&](const int sh, const int brow, auto first) {
        if constexpr (L > 0)
            digit_row_two_limb<BGBIT, decltype(first)::value>(s, v0, v1, sh, bk_rsrc, lane16, brow, sT, lane, R);
        else
            digit_row_two_limb_rt<decltype(first)::value>(s, v0, v1, sh, bgbit, bk_rsrc, lane16, brow, sT, lane, R);
    };
    decompose(0);
    digit_row(32 - width, 0, std::true_type{});
    // one loop over the other rows, as in k_cmux_x1 and for its reason
#pragma unroll 1
    for (int row = 1; row < rows2l; row++) {
        const int c = row >= half ? 1 : 0, q = row - c * half;
        if (q == 0) decompose(1);
        digit_row(32 - (q + 1) * width, row * kRowBytes, std::false_type{});
    }
    // opaque copies: the parent is read AGAIN below, and the memory rows' addresses are formed only now
    const int32_t* ppe = pp;
    asm volatile("" : "+s"(ppe));
    asm volatile("" : "+s"(po));
    const __amdgpu_buffer_rsrc_t rpe = row_resource(ppe);
    const __amdgpu_buffer_rsrc_t ro0 = row_resource(po), ro1 = row_resource(po + 2 * kN);
#pragma unroll
    for (int c = 0; c < 2; c++) {
        fft512_inverse_pair<true>(s[2 * c], s[2 * c + 1], sT, lane, R);
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const uint32_t h0 = join_limbs(s[2 * c][q].x, s[2 * c + 1][q].x, q), h1 = join_limbs(s[2 * c][q].y, s[2 * c + 1][q].y, q);
            const int jj = c * kN + 64 * q;
            const uint32_t p0 = row_word(rpe, lane4, jj), p1 = row_word(rpe, lane4, jj + kM);
            // the results are not used: the adds are issued in the form that returns nothing
            (void)__builtin_amdgcn_raw_ptr_buffer_atomic_add_i32((int)(p0 - h0), ro0, lane4, jj * 4, 0);
            (void)__builtin_amdgcn_raw_ptr_buffer_atomic_add_i32((int)(p1 - h1), ro0, lane4, (jj + kM) * 4, 0);
            (void)__builtin_amdgcn_raw_ptr_buffer_atomic_add_i32((int)h0, ro1, lane4, jj * 4, 0);
            (void)__builtin_amdgcn_raw_ptr_buffer_atomic_add_i32((int)h1, ro1, lane4, (jj + kM) * 4, 0);
        }
    }
}

template <int L, int BGBIT, int G = kCmuxWaveRows>
__global__ __launch_bounds__(64 * G, 2) void k_demux_acc(DemuxAccRows A, const double2* __restrict__ bkf, const double2* __restrict__ gtw) {
    __shared__ __align__(16) double2 sT_all[G * kTile];
    __shared__ __align__(16) double2 sTw[kTwElems];
    demux_acc_body<L, BGBIT, G>(A, bkf, gtw, L, BGBIT, sT_all, sTw);
}
template <int G = kCmuxWaveRows>
__global__ __launch_bounds__(64 * G, 2) void k_demux_acc_rt(DemuxAccRows A, const double2* __restrict__ bkf, const double2* __restrict__ gtw, int l,
                                                            int bgbit) {
    __shared__ __align__(16) double2 sT_all[G * kTile];
    __shared__ __align__(16) double2 sTw[kTwElems];
    demux_acc_body<0, 0, G>(A, bkf, gtw, l, bgbit, sT_all, sTw);
}

// ---- lut_add at depth 0: out[mem_of[i]][0] += v_i, the same order-free adds; a wave's instruction covers 256 contiguous bytes ----
__global__ __launch_bounds__(256) void k_demux_acc0(const int32_t* __restrict__ values, const int32_t* __restrict__ mem_of, int32_t n_mems,
                                                    int32_t* out) {
    const int64_t i = blockIdx.x;
    const int64_t m0 = mem_of ? (int64_t)mem_of[i] : 0;
    const int64_t m = m0 < 0 ? 0 : (m0 >= n_mems ? n_mems - 1 : m0);
    const uint32_t* v = reinterpret_cast<const uint32_t*>(values) + (size_t)i * 2 * kN;
    uint32_t* dst = reinterpret_cast<uint32_t*>(out) + (size_t)m * 2 * kN;
    for (int q = threadIdx.x; q < 2 * kN; q += 256) atomicAdd(dst + q, v[q]);
}

// ---- the subtraction of a replace write (include/ieache.h section 3i): delta_i = new_i - old_i mod 2^32, in place over old ----
// A pass of its own over the piece's [items][2][N] words between the tree and the scatter: 16 KB read and 8 KB written per item,
// against the 2^depth rows of 8 KB the scatter's last step moves.
__global__ __launch_bounds__(256) void k_write_delta(const int32_t* __restrict__ fresh, int32_t* old_to_delta) {
    const size_t at = (size_t)blockIdx.x * 2 * kN;
    for (int q = threadIdx.x; q < 2 * kN; q += 256) old_to_delta[at + q] = (int32_t)((uint32_t)fresh[at + q] - (uint32_t)old_to_delta[at + q]);
}

// ---- a scatter of depth 0: out_i = mem_i + v_i (mem null: v_i).  out == mem is sound: a word is read by the thread that stores it ----
__global__ __launch_bounds__(256) void k_demux_add(const int32_t* __restrict__ values, const int32_t* mem, int32_t* out) {
    const size_t at = (size_t)blockIdx.x * 2 * kN;
    for (int q = threadIdx.x; q < 2 * kN; q += 256) out[at + q] = (int32_t)((uint32_t)values[at + q] + (mem ? (uint32_t)mem[at + q] : 0u));
}

// ---- a tree of depth 0: out_i = row 0 of its table ----
__global__ __launch_bounds__(256) void k_cmux_copy(const int32_t* __restrict__ tables, int32_t n_tables, const int32_t* __restrict__ table_of,
                                                   int64_t item0, int32_t* __restrict__ out) {
    const int64_t i = blockIdx.x;
    const int64_t t0 = table_of ? (int64_t)table_of[item0 + i] : 0;
    const int64_t t = t0 < 0 ? 0 : (t0 >= n_tables ? n_tables - 1 : t0);  // clamp_index (cmux_step.h), open-coded: the helper moves this kernel's code
    const int4* src = reinterpret_cast<const int4*>(tables + (size_t)t * 2 * kN);
    int4* dst = reinterpret_cast<int4*>(out + (size_t)i * 2 * kN);
    for (int q = threadIdx.x; q < 2 * kN / 4; q += 256) dst[q] = src[q];
}

// ---- coefficient j of a TLWE sample as an extracted row: u[i] = A[j - i] for i <= j, -A[N + j - i] otherwise, u[N] = B[j] ----
__global__ __launch_bounds__(256) void k_tlwe_extract(const int32_t* __restrict__ tlwe, const int32_t* __restrict__ coef_of, int32_t* __restrict__ u,
                                                      int32_t N, int32_t stride) {
    const int64_t row = blockIdx.x;
    const int32_t j = clamp_index(coef_of ? coef_of[row] : 0, N);
    const int32_t* A = tlwe + (size_t)row * 2 * N;
    int32_t* dst = u + (size_t)row * stride;
    for (int32_t i = threadIdx.x; i <= N; i += 256)
        dst[i] = i == N ? A[N + j] : (i <= j ? A[j - i] : (int32_t)(0u - (uint32_t)A[N + j - i]));
}

std::atomic<uint64_t> g_next_id{1};

// The intermediates of a tree or a scatter piece alternate between the two scratch buffers: A or B by the parity of the
// distance from the widest one (items x 2^(depth-1) rows: what level 0 of a tree and step depth - 2 of a scatter write),
// so that it lands in A and the sizes are cmux_plan.h's.
void check_scratch(const CmuxScratch& scratch, int64_t items, int32_t depth, const char* refusal) {
    const size_t widest = (size_t)(items << (depth - 1)) * 2 * kN;
    if ((depth >= 2 && scratch.a.items() < widest) || (depth >= 3 && scratch.b.items() < widest / 2)) throw std::invalid_argument(refusal);
}
int32_t* scratch_rows(CmuxScratch& scratch, int32_t from_widest) { return from_widest % 2 == 0 ? (int32_t*)scratch.a : (int32_t*)scratch.b; }

}  // namespace

void Cmux::init(const Params& p, int device, const int64_t* runtime_always) {
    p_ = p;
    runtime_always_ = runtime_always;
    device_ = device;
    id_ = g_next_id.fetch_add(1);
}

TgswSet* Cmux::prepare(const int32_t* d_samples, size_t n, hipStream_t stream) {
    if (!br_supported(p_)) throw std::invalid_argument("tgsw_prepare: the CMux kernels cover N = 1024, k = 1 with (l, Bgbit) = (3, 7) or (2, 10) only");
    return prepare(d_samples, n, p_.l, p_.Bgbit, stream);
}

const double2* Cmux::twiddles(hipStream_t stream) {
    if (!tw_) {
        tw_.allocate(twiddle_table_elems());
        build_twiddle_table(tw_, stream);
        HIP_CHECK(hipGetLastError());
    }
    return tw_;
}

TgswSet* Cmux::prepare(const int32_t* d_samples, size_t n, int32_t l, int32_t Bgbit, hipStream_t stream) {
    if (const char* why = gadget_refusal(p_, l, Bgbit)) throw std::invalid_argument(why);
    if (!d_samples || n < 1) throw std::invalid_argument("tgsw_prepare: no samples");
    if (n > ((size_t)1 << 20)) throw std::invalid_argument("tgsw_prepare: more than 2^20 samples");
    twiddles(stream);
    std::unique_ptr<TgswSet> set(new TgswSet);
    Params as_key = p_;
    as_key.n = (int32_t)n;  // the spectrum kernel sees n samples where the bootstrapping key has n blocks BK_i
    as_key.l = l;           // ... of the set's 2l rows: it works per polynomial and knows no gadget
    as_key.Bgbit = Bgbit;
    set->spectrum.allocate(spectrum_elems(as_key));
    prepare_spectrum(as_key, d_samples, set->spectrum, stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(stream));
    set->n = n;
    set->l = l;
    set->Bgbit = Bgbit;
    set->owner = id_;
    set->device = device_;
    return set.release();
}

void Cmux::check_owner(const TgswSet& set) const {
    if (set.owner != id_ || !set.spectrum || set.n < 1) throw std::invalid_argument("the TGSW set was prepared on another context");
}

void Cmux::reserve(CmuxScratch& scratch, const CmuxPlan& pl) {
    scratch.a.reserve_exact((size_t)pl.a_rows * 2 * kN);
    scratch.b.reserve_exact((size_t)pl.b_rows * 2 * kN);
}

void Cmux::launch(const TgswSet& set, hipStream_t stream, CmuxRows rows) {
    launch_rows(set, stream, rows, [](auto ps) {
        if constexpr (decltype(ps)::L == 0)
            return k_cmux_rt<>;
        else
            return k_cmux_x1<ps.L, ps.BGBIT>;
    });
}

int Cmux::launch_tree(const TgswSet& set, CmuxScratch& scratch, hipStream_t stream, int64_t item0, int64_t items, int32_t depth,
                      const int32_t* sel_of, const int32_t* tables, int32_t n_tables, const int32_t* table_of, int32_t* out) {
    check_owner(set);
    if (items <= 0) return 0;
    if (depth < 0 || depth > kCmuxMaxDepth || n_tables < 1) throw std::invalid_argument("lut_tree: depth or n_tables out of range");
    if (depth == 0) {
        hipLaunchKernelGGL(k_cmux_copy, dim3((unsigned)items), dim3(256), 0, stream, tables, n_tables, table_of, item0, out);
        return 1;
    }
    return launch_levels(set, scratch, stream, item0, items, depth, sel_of, tables, true, n_tables, table_of, out,
                         "lut_tree: piece larger than the reserved scratch");
}

int Cmux::launch_levels(const TgswSet& set, CmuxScratch& scratch, hipStream_t stream, int64_t item0, int64_t items, int32_t depth,
                        const int32_t* sel_of, const int32_t* src, bool shared, int32_t n_tables, const int32_t* table_of, int32_t* out,
                        const char* refusal) {
    check_scratch(scratch, items, depth, refusal);
    for (int32_t k = 0; k < depth; k++) {
        CmuxRows R;
        R.depth = depth;
        R.level = k;
        R.width = 1 << (depth - 1 - k);
        R.rows = items * R.width;
        R.item0 = item0;
        R.sel_of = sel_of;
        R.src = src;
        R.shared = shared && k == 0;
        R.table_of = table_of;
        R.n_tables = n_tables;
        R.dst = k == depth - 1 ? out : scratch_rows(scratch, k);  // the last level writes the caller's rows; level 0 the widest
        launch(set, stream, R);
        src = R.dst;
    }
    return depth;
}

int Cmux::launch_own_tree(const TgswSet& set, CmuxScratch& scratch, hipStream_t stream, int64_t item0, int64_t items, int32_t depth,
                          const int32_t* sel_of, const int32_t* mem, int32_t* out, const char* refusal) {
    if (depth == 0) {
        HIP_CHECK(hipMemcpyAsync(out, mem, (size_t)items * 2 * kN * 4, hipMemcpyDeviceToDevice, stream));
        return 1;
    }
    // tables [items][2^depth] with table_of[i] = i, which is the tree's level 0 unshared
    return launch_levels(set, scratch, stream, item0, items, depth, sel_of, mem, false, 1, nullptr, out, refusal);
}

void Cmux::launch_demux(const TgswSet& set, hipStream_t stream, DemuxRows rows) {
    launch_rows(set, stream, rows, [](auto ps) {
        if constexpr (decltype(ps)::L == 0)
            return k_demux_rt<>;
        else
            return k_demux_x1<ps.L, ps.BGBIT>;
    });
}

int Cmux::launch_scatter(const TgswSet& set, CmuxScratch& scratch, hipStream_t stream, int64_t item0, int64_t items, int32_t depth,
                         const int32_t* sel_of, const int32_t* values, const int32_t* mem, int32_t* out) {
    check_owner(set);
    if (items <= 0) return 0;
    if (depth < 0 || depth > kCmuxMaxDepth) throw std::invalid_argument("lut_scatter: depth out of range");
    if (depth == 0) {
        hipLaunchKernelGGL(k_demux_add, dim3((unsigned)items), dim3(256), 0, stream, values, mem, out);
        return 1;
    }
    check_scratch(scratch, items, depth, "lut_scatter: piece larger than the reserved scratch");
    const int32_t* src = values;
    for (int32_t t = 0; t < depth; t++) {
        DemuxRows R;
        R.depth = depth;
        R.step = t;
        R.width = 1 << t;
        R.rows = items * R.width;
        R.item0 = item0;
        R.sel_of = sel_of;
        R.src = src;
        const bool last = t == depth - 1;
        R.dst = last ? out : scratch_rows(scratch, depth - 2 - t);  // the last step writes the caller's rows over the memory; step depth - 2 the widest
        R.base = last ? mem : nullptr;
        launch_demux(set, stream, R);
        src = R.dst;
    }
    return depth;
}

void Cmux::launch_demux_acc(const TgswSet& set, hipStream_t stream, DemuxAccRows rows) {
    // the rule that keeps 2 j + c inside a memory: only the last step of a scatter accumulates
    if (rows.rows > 0 && (rows.depth < 1 || rows.depth > kCmuxMaxDepth || rows.step != rows.depth - 1 || rows.width != 1 << (rows.depth - 1) ||
                          rows.rows % rows.width != 0 || rows.n_mems < 1))
        throw std::invalid_argument("lut_add: the accumulating step is the last step of a scatter");
    launch_rows(set, stream, rows, [](auto ps) {
        if constexpr (decltype(ps)::L == 0)
            return k_demux_acc_rt<>;
        else
            return k_demux_acc<ps.L, ps.BGBIT>;
    });
}

int Cmux::launch_scatter_acc(const TgswSet& set, CmuxScratch& scratch, hipStream_t stream, int64_t items, int32_t depth, const int32_t* tree_sel,
                             const int32_t* src, const int32_t* mem_of, int32_t n_mems, int32_t* out) {
    check_owner(set);
    if (items <= 0) return 0;
    if (depth < 0 || depth > kCmuxMaxDepth || n_mems < 1) throw std::invalid_argument("lut_add: depth or n_mems out of range");
    if (depth == 0) {
        hipLaunchKernelGGL(k_demux_acc0, dim3((unsigned)items), dim3(256), 0, stream, src, mem_of, n_mems, out);
        return 1;
    }
    check_scratch(scratch, items, depth, "lut_add: piece larger than the reserved scratch");
    for (int32_t t = 0; t < depth - 1; t++) {
        DemuxRows R;
        R.depth = depth;
        R.step = t;
        R.width = 1 << t;
        R.rows = items * R.width;
        R.sel_of = tree_sel;  // the piece's own array: item0 stays 0
        R.src = src;
        R.dst = scratch_rows(scratch, depth - 2 - t);  // launch_scatter's buffers: step depth - 2 the widest, in A
        launch_demux(set, stream, R);
        src = R.dst;
    }
    DemuxAccRows R;
    R.depth = depth;
    R.step = depth - 1;
    R.width = 1 << (depth - 1);
    R.rows = items * R.width;
    R.sel_of = tree_sel;
    R.mem_of = mem_of;
    R.n_mems = n_mems;
    R.src = src;
    R.out = out;
    launch_demux_acc(set, stream, R);
    return depth;
}

int Cmux::launch_write(const TgswSet& set, CmuxScratch& scratch, hipStream_t stream, int64_t item0, int64_t items, int32_t depth, const int32_t* sel_of,
                       const int32_t* fresh, const int32_t* mem, int32_t* out) {
    check_owner(set);
    if (items <= 0) return 0;
    if (depth < 0 || depth > kCmuxMaxDepth) throw std::invalid_argument("lut_write: depth out of range");
    if (scratch.rows.items() < (size_t)items * 2 * kN) throw std::invalid_argument("lut_write: piece larger than the reserved scratch");
    int32_t* delta = scratch.rows;
    const int launches = launch_own_tree(set, scratch, stream, item0, items, depth, sel_of, mem, delta, "lut_write: piece larger than the reserved scratch");
    launch_delta(stream, items, fresh, delta);
    return launches + 1 + launch_scatter(set, scratch, stream, item0, items, depth, sel_of, delta, mem, out);
}

void Cmux::launch_delta(hipStream_t stream, int64_t items, const int32_t* fresh, int32_t* old_to_delta) {
    if (items <= 0) return;
    hipLaunchKernelGGL(k_write_delta, dim3((unsigned)items), dim3(256), 0, stream, fresh, old_to_delta);
}

void Cmux::launch_extract(hipStream_t stream, int64_t count, const int32_t* tlwe, const int32_t* coef_of, int32_t* u, int32_t stride) {
    if (count <= 0) return;
    hipLaunchKernelGGL(k_tlwe_extract, dim3((unsigned)count), dim3(256), 0, stream, tlwe, coef_of, u, p_.N, stride);
}

}  // namespace ieache
