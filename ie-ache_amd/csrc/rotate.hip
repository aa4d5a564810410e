// The rotation of a TLWE sample by an encrypted amount (include/ieache.h section 3h): for t = 0 .. steps - 1
//   acc <- acc + C_t [.] (X^(a_t) acc - acc),
// the blind rotation's own step with the selector a TGSW sample of the caller's set instead of BK_i and the amount public.  It
// is the last stage of vertical packing: after a CMux tree has chosen one of 2^d samples, this brings one of its N coefficients
// to a public position.  k_rotate_x1 is k_blind_rotate_x1 (blind_rotate_w64.hip) with the key block chosen per row and step;
// built from the pieces of br_step.h and fft512.h, and of cmux_step.h, which it shares with the kernels of cmux.hip.
// N = 1024, k = 1; libtfhe's two (l, Bgbit) as template arguments (k_rotate_x1), every other admissible gadget of a set as launch
// arguments (k_rotate_rt: include/ieache.h section 3i).
#include "cmux.h"

#include <stdexcept>
#include <type_traits>

#include "blind_rotate_w64.h"
#include "cmux_step.h"

namespace ieache {

using namespace dev;
using namespace w64;

namespace {

// ---- one row per wave, every step of it inside the launch ----
// What stays as in k_blind_rotate_x1: one wave owns a row, G = 4 rows share a workgroup for the twiddle table only (one workgroup
// barrier, after the table is in LDS), the accumulator [2][1024] stands first in LDS on a 4 KiB boundary so that the rotated
// decomposition addresses it with one v_and_or of a per-step lane value, 2L forward transforms of the digits, 8L row products
// on the two-limb spectrum into four sums, two interleaved pairs of inverse transforms, the limbs recombined as
// lo + (hi << 16), the wavefront-scope ds_add update and wave_sync, and the loop over the steps.  Every rounded sum stays
// below 2^37 of the 2^53 an FP64 mantissa holds, so the words are exact for ANY caller words: no guard, no audit.
// What differs:
//   * the key block is chosen per row AND per step.  Lane t holds step t's amount (11 bits) and selector index (below 2^20, what
//     a set may hold) in ONE register, fetched once ahead of the loop like the blind rotation's amounts and read back per step
//     with v_readlane: the step loop has no register to spare for a second vector;
//   * the selected sample goes into the buffer resource's BASE, rebuilt per step with num_records = one sample's bytes, as in
//     k_cmux_x1: a set may hold 2^20 samples of 192 KB, which the 32-bit scalar offset that addresses BK_i cannot reach.  The rows
//     of the sample go into the scalar offset.  Nothing past the selected sample can be touched whatever the indices hold: an
//     explicit index is clamped into the set, an implied one taken mod n_set, an amount masked to 2N - 1;
//   * the amounts come from the call's shared [steps] array (null: 2N - 2^t, which brings coefficient sum b_t 2^t to position 0);
//   * the accumulator is loaded from src + r and stored to dst + r after the last step.
// IN PLACE (dst == src) is sound: the wave copies its WHOLE row into LDS (the sixteen 16-byte loads per lane below, then
// wave_sync) before the step loop starts, nothing in the loop reads global memory but the set and nothing in it writes
// global memory at all, and the stores after the loop write row r only -- a row no other wave of the launch reads or writes
// (rows are disjoint between waves).  So every load of a row precedes every store to it, in one wave's program order.
// Everything that selects memory is wave-uniform scalar arithmetic; there are no pointer tables; stores are vector stores.
// dynamic LDS as k_blind_rotate_x1: acc [4][2][1024] int32 | sT [4][kTile] double2 | tw [kTwElems] double2   (78 848 B -> 2 per CU)
template <int L, int BGBIT, int G = kCmuxWaveRows>
__global__ __launch_bounds__(64 * G, 2) void k_rotate_x1(RotateRows A, const double2* __restrict__ bkf, const double2* __restrict__ gtw) {
    extern __shared__ __align__(16) unsigned char smem[];
    int32_t* acc_all = reinterpret_cast<int32_t*>(smem);
    double2* sT_all = reinterpret_cast<double2*>(smem + (size_t)G * 2 * kN * 4);
    double2* sTw = sT_all + G * kTile;
    const WaveRow W = wave_prologue<G>(sT_all, sTw, gtw);
    const int lane = W.lane, wave = W.wave;
    double2* sT = W.sT;
    int32_t* acc = acc_all + wave * 2 * kN;
    const int64_t r = W.r;
    if (r >= A.rows) return;
    const LaneRoots R = make_roots(sTw, lane);
    {
        const int4* src = reinterpret_cast<const int4*>(A.src + (size_t)r * 2 * kN);
        int4* dst = reinterpret_cast<int4*>(acc);
#pragma unroll
        for (int q = 0; q < 8; q++) dst[64 * q + lane] = src[64 * q + lane];
    }
    wave_sync();

    // lane t: (selector << 11) | amount of step t; amount 0 beyond the last step
    int32_t my_step = 0;
    if (lane < A.steps) {
        const int64_t sel = selector_at(A.sel_of, (A.item0 + r) * A.sel_stride + lane, A.n_set);
        const int32_t a = A.amount_of ? A.amount_of[lane] : (lane < 11 ? 2 * kN - (1 << lane) : 0);
        my_step = ((int32_t)sel << 11) | (a & (2 * kN - 1));
    }

    const uint32_t dec_offset = decomposition_offset<L, BGBIT>();
    constexpr int kBlockBytes = kM * (int)sizeof(double2), kRowBytes = 4 * kBlockBytes, kStepBytes = 2 * L * kRowBytes;
    const int lane16 = bk_lane_offset(lane);
    const unsigned char* accb = reinterpret_cast<const unsigned char*>(acc_all);  // LDS offset 0 of the workgroup
    const uint32_t pb0 = (uint32_t)wave * (2 * kN * 4);                            // this row's polynomial 0; polynomial 1 at + 4096

#pragma unroll 1
    for (int32_t t = 0; t < A.steps; t++) {
        const int32_t both = __builtin_amdgcn_readlane(my_step, t);
        const int32_t a = both & (2 * kN - 1);
        if (a == 0) continue;  // wave-uniform; exact arithmetic makes the step a no-op
        // the resource covers the selected sample only: its rows [2L][q = 2 c + limb][8][64] double2
        const __amdgpu_buffer_rsrc_t bk_rsrc = bk_resource(bkf + (size_t)(both >> 11) * (kStepBytes / sizeof(double2)), 1, kStepBytes);
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
        digit_row(32 - BGBIT, 0, std::true_type{});
#pragma unroll 1
        for (int row = 1; row < L; row++) digit_row(32 - (row + 1) * BGBIT, row * kRowBytes, std::false_type{});
        // opaque copy, as in k_blind_rotate_x1: the second decomposition's addresses and sign masks are recomputed, not kept
        uint32_t jb4b = jb4;
        asm volatile("" : "+v"(jb4b));
        decompose(pb0 + 4096u, jb4b);
#pragma unroll 1
        for (int row = L; row < 2 * L; row++) digit_row(32 - (row - L + 1) * BGBIT, row * kRowBytes, std::false_type{});
        // back to coefficients: s[2 c] / s[2 c + 1] hold the low / high limb sums of output polynomial c
#pragma unroll
        for (int c = 0; c < 2; c++) {
            fft512_inverse_pair<true>(s[2 * c], s[2 * c + 1], sT, lane, R);
            uint32_t* accc = reinterpret_cast<uint32_t*>(acc) + c * kN;
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const uint32_t d0 = join_limbs(s[2 * c][q].x, s[2 * c + 1][q].x, q), d1 = join_limbs(s[2 * c][q].y, s[2 * c + 1][q].y, q);
                const int32_t j = 64 * q + lane;
                __hip_atomic_fetch_add(&accc[j], d0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                __hip_atomic_fetch_add(&accc[j + kM], d1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            }
        }
        wave_sync();
    }
    // the epilogue forms its addresses from the lane number again (k_blind_rotate_w1b's remedy): shared with the prologue's
    // they would be held across the step loop, which has no register to spare
    int elane = lane;
    asm volatile("" : "+v"(elane));
    {
        const int4* src = reinterpret_cast<const int4*>(acc);
        int4* dst = reinterpret_cast<int4*>(A.dst + (size_t)r * 2 * kN);
#pragma unroll
        for (int q = 0; q < 8; q++) dst[64 * q + elane] = src[64 * q + elane];
    }
}

// ---- the same kernel with the set's gadget (l, bgbit) as launch arguments ----
// k_rotate_x1's body line for line -- what it says about the packed step word, the resource per step and the rotation in place
// holds here -- with the wave-uniform differences of k_cmux_rt (cmux.hip): decomposition_offset_rt, digit_row_two_limb_rt,
// the bytes of a sample 2 l kRowBytes, the row loops to l and 2 l.  A copy because k_rotate_x1 must keep its code.
template <int G = kCmuxWaveRows>
__global__ __launch_bounds__(64 * G, 2) void k_rotate_rt(RotateRows A, const double2* __restrict__ bkf, const double2* __restrict__ gtw, int l, int bgbit) {
    extern __shared__ __align__(16) unsigned char smem[];
    int32_t* acc_all = reinterpret_cast<int32_t*>(smem);
    double2* sT_all = reinterpret_cast<double2*>(smem + (size_t)G * 2 * kN * 4);
    double2* sTw = sT_all + G * kTile;
    const WaveRow W = wave_prologue<G>(sT_all, sTw, gtw);
    const int lane = W.lane, wave = W.wave;
    double2* sT = W.sT;
    int32_t* acc = acc_all + wave * 2 * kN;
    const int64_t r = W.r;
    if (r >= A.rows) return;
    const LaneRoots R = make_roots(sTw, lane);
    {
        const int4* src = reinterpret_cast<const int4*>(A.src + (size_t)r * 2 * kN);
        int4* dst = reinterpret_cast<int4*>(acc);
#pragma unroll
        for (int q = 0; q < 8; q++) dst[64 * q + lane] = src[64 * q + lane];
    }
    wave_sync();

    int32_t my_step = 0;
    if (lane < A.steps) {
        const int64_t sel = selector_at(A.sel_of, (A.item0 + r) * A.sel_stride + lane, A.n_set);
        const int32_t a = A.amount_of ? A.amount_of[lane] : (lane < 11 ? 2 * kN - (1 << lane) : 0);
        my_step = ((int32_t)sel << 11) | (a & (2 * kN - 1));
    }

    const uint32_t dec_offset = decomposition_offset_rt(l, bgbit);
    constexpr int kBlockBytes = kM * (int)sizeof(double2), kRowBytes = 4 * kBlockBytes;
    const int rows2l = 2 * l, step_bytes = rows2l * kRowBytes;
    const int lane16 = bk_lane_offset(lane);
    const unsigned char* accb = reinterpret_cast<const unsigned char*>(acc_all);
    const uint32_t pb0 = (uint32_t)wave * (2 * kN * 4);

#pragma unroll 1
    for (int32_t t = 0; t < A.steps; t++) {
        const int32_t both = __builtin_amdgcn_readlane(my_step, t);
        const int32_t a = both & (2 * kN - 1);
        if (a == 0) continue;
        const __amdgpu_buffer_rsrc_t bk_rsrc = bk_resource(bkf + (size_t)(both >> 11) * ((size_t)step_bytes / sizeof(double2)), 1, step_bytes);
        double2 s[4][8];
        uint32_t v0[8], v1[8];
        const uint32_t jb4 = ((uint32_t)(lane - a) & (2 * kN - 1)) << 2;
        auto decompose = [&](const uint32_t pb, const uint32_t jb) {
            const int32_t* accp = reinterpret_cast<const int32_t*>(accb + pb);
            decompose_rotated(v0, v1, accb, accp, pb, jb, lane, dec_offset);
        };
        decompose(pb0, jb4);
        digit_row_two_limb_rt<true>(s, v0, v1, 32 - bgbit, bgbit, bk_rsrc, lane16, 0, sT, lane, R);
#pragma unroll 1
        for (int row = 1; row < l; row++) digit_row_two_limb_rt<false>(s, v0, v1, 32 - (row + 1) * bgbit, bgbit, bk_rsrc, lane16, row * kRowBytes, sT, lane, R);
        uint32_t jb4b = jb4;
        asm volatile("" : "+v"(jb4b));
        decompose(pb0 + 4096u, jb4b);
#pragma unroll 1
        for (int row = l; row < rows2l; row++)
            digit_row_two_limb_rt<false>(s, v0, v1, 32 - (row - l + 1) * bgbit, bgbit, bk_rsrc, lane16, row * kRowBytes, sT, lane, R);
#pragma unroll
        for (int c = 0; c < 2; c++) {
            fft512_inverse_pair<true>(s[2 * c], s[2 * c + 1], sT, lane, R);
            uint32_t* accc = reinterpret_cast<uint32_t*>(acc) + c * kN;
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const uint32_t d0 = join_limbs(s[2 * c][q].x, s[2 * c + 1][q].x, q), d1 = join_limbs(s[2 * c][q].y, s[2 * c + 1][q].y, q);
                const int32_t j = 64 * q + lane;
                __hip_atomic_fetch_add(&accc[j], d0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                __hip_atomic_fetch_add(&accc[j + kM], d1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            }
        }
        wave_sync();
    }
    int elane = lane;
    asm volatile("" : "+v"(elane));
    {
        const int4* src = reinterpret_cast<const int4*>(acc);
        int4* dst = reinterpret_cast<int4*>(A.dst + (size_t)r * 2 * kN);
#pragma unroll
        for (int q = 0; q < 8; q++) dst[64 * q + elane] = src[64 * q + elane];
    }
}

// ---- what a lookup's tree and extraction read: selectors steps .. steps + depth - 1 of each item as a [items][depth] array of
// explicit indices (an implied one taken mod n_set, an explicit one clamped: the rule of the call, applied once), and the
// public coefficient once per item ----
__global__ __launch_bounds__(256) void k_read_indices(const int32_t* __restrict__ sel_of, int64_t item0, int64_t items, int32_t depth, int32_t steps,
                                                      int32_t n_set, int32_t coef, int32_t* __restrict__ tree_sel, int32_t* __restrict__ coef_of) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q < items) coef_of[q] = coef;
    if (q >= items * depth) return;
    const int64_t item = q / depth, k = q - item * depth;
    tree_sel[q] = (int32_t)selector_at(sel_of, (item0 + item) * (depth + steps) + steps + k, n_set);
}

// selectors steps .. steps + depth - 1 of items item0 .. of the call, explicit, as the piece's own array tree_sel [items][depth],
// and `coef` once per item in the `items` words after it (with_coef: written at depth 0 as well; otherwise not read).  Not
// counted as a launch of the call's.
void launch_read_indices(hipStream_t stream, const int32_t* sel_of, int64_t item0, int64_t items, int32_t depth, int32_t steps, int32_t n_set,
                         bool with_coef, int32_t coef, int32_t* tree_sel) {
    const int64_t words = items * (with_coef && depth < 1 ? 1 : depth);
    if (words <= 0) return;
    hipLaunchKernelGGL(k_read_indices, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, sel_of, item0, items, depth, steps, n_set, coef,
                       tree_sel, tree_sel + (size_t)items * depth);
}

constexpr size_t kRotateLds = (size_t)kCmuxWaveRows * 2 * kN * 4 + ((size_t)kCmuxWaveRows * kTile + kTwElems) * sizeof(double2);
LdsGrant g_rotate_grant[3];  // one per build: cmux_step.h's with_gadget

}  // namespace

void Cmux::launch_rotate(const TgswSet& set, hipStream_t stream, RotateRows rows) {
    check_owner(set);  // ahead of the steps, as the shared launcher's own check would not be
    if (rows.rows > 0 && (rows.steps < 0 || rows.steps > kRotateMaxSteps || rows.sel_stride < rows.steps))
        throw std::invalid_argument("tlwe_rotate: steps out of range");
    launch_rows(
        set, stream, rows,
        [](auto ps) {
            if constexpr (decltype(ps)::L == 0)
                return k_rotate_rt<>;
            else
                return k_rotate_x1<ps.L, ps.BGBIT>;
        },
        kRotateLds, g_rotate_grant, "k_rotate_x1", "k_rotate_rt");
}

void Cmux::reserve_read(CmuxScratch& scratch, const CmuxPlan& pl, int32_t depth) {
    reserve(scratch, pl);
    scratch.rows.reserve_exact((size_t)pl.items_per_piece * 2 * kN);
    scratch.idx.reserve_exact((size_t)pl.items_per_piece * (size_t)(depth + 1));
}

int Cmux::launch_read(const TgswSet& set, CmuxScratch& scratch, hipStream_t stream, int64_t item0, int64_t items, int32_t depth, int32_t steps,
                      const int32_t* sel_of, const int32_t* amount_of, const int32_t* tables, int32_t n_tables, const int32_t* table_of, int32_t coef,
                      int32_t* u, int32_t stride) {
    check_owner(set);
    if (items <= 0) return 0;
    if (steps < 0 || steps > kRotateMaxSteps) throw std::invalid_argument("lut_read: steps out of range");
    if (scratch.rows.items() < (size_t)items * 2 * kN || scratch.idx.items() < (size_t)items * (size_t)(depth + 1))
        throw std::invalid_argument("lut_read: piece larger than the reserved scratch");
    int32_t* tree_sel = scratch.idx;
    launch_read_indices(stream, sel_of, item0, items, depth, steps, (int32_t)set.n, true, coef < 0 ? 0 : (coef >= p_.N ? p_.N - 1 : coef), tree_sel);
    // the tree sees a piece of its own: items 0 .. items - 1 with their explicit selectors, but the call's table_of
    int launches = 1 + launch_tree(set, scratch, stream, 0, items, depth, tree_sel, tables, n_tables, table_of ? table_of + item0 : nullptr, scratch.rows);
    launches += launch_rotate_selected(set, scratch, stream, item0, items, depth, steps, sel_of, amount_of);
    launch_extract(stream, items, scratch.rows, tree_sel + (size_t)items * depth, u, stride);
    return launches + 1;
}

int Cmux::launch_rotate_selected(const TgswSet& set, CmuxScratch& scratch, hipStream_t stream, int64_t item0, int64_t items, int32_t depth, int32_t steps,
                                 const int32_t* sel_of, const int32_t* amount_of) {
    if (steps <= 0) return 0;
    RotateRows R;
    R.src = R.dst = scratch.rows;
    R.rows = items;
    R.item0 = item0;
    R.sel_of = sel_of;
    R.amount_of = amount_of;
    R.steps = steps;
    R.sel_stride = depth + steps;
    launch_rotate(set, stream, R);
    return 1;
}

int Cmux::launch_read_own(const TgswSet& set, CmuxScratch& scratch, hipStream_t stream, int64_t item0, int64_t items, int32_t depth, int32_t steps,
                          const int32_t* sel_of, const int32_t* amount_of, const int32_t* mem) {
    check_owner(set);
    if (items <= 0) return 0;
    if (depth < 0 || depth > kCmuxMaxDepth || steps < 0 || steps > kRotateMaxSteps) throw std::invalid_argument("lut_write_coef: depth or steps out of range");
    if (scratch.rows.items() < (size_t)items * 2 * kN || scratch.idx.items() < (size_t)items * (size_t)(depth + 1))
        throw std::invalid_argument("lut_write_coef: piece larger than the reserved scratch");
    int32_t* tree_sel = scratch.idx;
    launch_read_indices(stream, sel_of, item0, items, depth, steps, (int32_t)set.n, false, 0, tree_sel);
    // the tree sees a piece of its own, as launch_read's does
    const int tree = launch_own_tree(set, scratch, stream, 0, items, depth, tree_sel, mem, scratch.rows, "lut_write_coef: piece larger than the reserved scratch");
    return tree + launch_rotate_selected(set, scratch, stream, item0, items, depth, steps, sel_of, amount_of);
}

int Cmux::launch_read_rows(const TgswSet& set, CmuxScratch& scratch, hipStream_t stream, int64_t item0, int64_t items, int32_t depth, int32_t steps,
                           const int32_t* sel_of, const int32_t* amount_of, const int32_t* tables, int32_t n_tables, const int32_t* table_of) {
    check_owner(set);
    if (items <= 0) return 0;
    if (depth < 0 || depth > kCmuxMaxDepth || steps < 0 || steps > kRotateMaxSteps) throw std::invalid_argument("word_read: depth or steps out of range");
    if (scratch.rows.items() < (size_t)items * 2 * kN || scratch.idx.items() < (size_t)items * (size_t)(depth + 1))
        throw std::invalid_argument("word_read: piece larger than the reserved scratch");
    int32_t* tree_sel = scratch.idx;
    launch_read_indices(stream, sel_of, item0, items, depth, steps, (int32_t)set.n, false, 0, tree_sel);
    // the tree sees a piece of its own, as launch_read's does
    const int tree = launch_tree(set, scratch, stream, 0, items, depth, tree_sel, tables, n_tables, table_of ? table_of + item0 : nullptr, scratch.rows);
    return tree + launch_rotate_selected(set, scratch, stream, item0, items, depth, steps, sel_of, amount_of);
}

int Cmux::launch_add(const TgswSet& set, CmuxScratch& scratch, hipStream_t stream, int64_t item0, int64_t items, int32_t depth, int32_t steps,
                     const int32_t* sel_of, const int32_t* amount_of, const int32_t* values, int32_t n_mems, const int32_t* mem_of, int32_t* out) {
    check_owner(set);
    if (items <= 0) return 0;
    if (steps < 0 || steps > kRotateMaxSteps) throw std::invalid_argument("lut_add: steps out of range");
    if (scratch.rows.items() < (size_t)items * 2 * kN || scratch.idx.items() < (size_t)items * (size_t)(depth + 1))
        throw std::invalid_argument("lut_add: piece larger than the reserved scratch");
    int launches = 0;
    const int32_t* parents = values;
    if (steps > 0) {
        if (!amount_of) {
            // the write's direction, +2^t mod 2N (0 from t = 11 on): k_rotate_x1's own default is the read's
            if (!add_amounts_) {
                int32_t host[kRotateMaxSteps];
                for (int32_t t = 0; t < kRotateMaxSteps; t++) host[t] = t < 11 ? 1 << t : 0;
                add_amounts_.allocate(kRotateMaxSteps);
                HIP_CHECK(hipMemcpy(add_amounts_, host, sizeof host, hipMemcpyHostToDevice));
            }
            amount_of = add_amounts_;
        }
        RotateRows R;
        R.src = values;
        R.dst = scratch.rows;
        R.rows = items;
        R.item0 = item0;
        R.sel_of = sel_of;
        R.amount_of = amount_of;
        R.steps = steps;
        R.sel_stride = depth + steps;
        launch_rotate(set, stream, R);
        launches++;
        parents = scratch.rows;
    }
    int32_t* tree_sel = scratch.idx;
    launch_read_indices(stream, sel_of, item0, items, depth, steps, (int32_t)set.n, false, 0, tree_sel);
    return launches + launch_scatter_acc(set, scratch, stream, items, depth, tree_sel, parents, mem_of ? mem_of + item0 : nullptr, n_mems, out);
}

}  // namespace ieache
