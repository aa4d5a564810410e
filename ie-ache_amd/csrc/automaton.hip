// Deterministic (weighted) finite automata over words whose letters are TGSW-encrypted bits (include/ieache.h section 3k; the
// TFHE paper's det-WFA evaluation): for t = steps-1 .. 0
//   V_t[q] = CMux(C_sel(i,t), d1 = V_{t+1}[next1[t][q]], d0 = V_{t+1}[next0[t][q]]),   V_steps = the final rows,  out = V_0[0 .. n_out)
// with the transition tables a public program (automaton_plan.h) and CMux word for word k_cmux_x1's: d0 + C [.] (d1 - d0) on the
// provably exact two-limb spectrum, with the SET's gadget.  Where the other calls of the family have a fixed shape -- a tree, a
// demux tree, a rotation -- this is the general sequential one, and its levels are narrow (2 to 16 states): run as one launch of
// k_cmux_x1 per step it would be all launch latency.  So k_automaton_x1 runs ALL steps of an item
// inside one launch, as k_rotate_x1 does for a row, and hands the state vector from wave to wave inside one workgroup.
// Built from the pieces of br_step.h, fft512.h and cmux_step.h; N = 1024, k = 1; three builds as the family's (with_gadget).
#include "cmux.h"

#include <cstddef>
#include <memory>
#include <stdexcept>
#include <type_traits>
#include <vector>

#include "blind_rotate_w64.h"
#include "cmux_step.h"

namespace ieache {

using namespace dev;
using namespace w64;

namespace {

// ---- one CMux of a step: k_cmux_x1's body on rows the caller names ----
// d1 = p1, d0 = p0, result po: rows through 8 KB buffer resources, d0 read AGAIN for the epilogue through an opaque copy, both
// decompositions in ONE row loop -- what k_cmux_x1 says about each holds here and is not repeated.  There is no "d0 = zeros"
// form.  Stated once for the three builds: L > 0 takes the compile-time digit row, L == 0 the run-time one (k_cmux_rt's
// differences), as k_demux_acc does.
template <int L, int BGBIT>
__device__ __forceinline__ void automaton_cmux(const int32_t* p1, const int32_t* p0, int32_t* po, const __amdgpu_buffer_rsrc_t bk_rsrc, const int l,
                                               const int bgbit, double2* sT, const int lane, const LaneRoots& R) {
    const __amdgpu_buffer_rsrc_t r1 = row_resource(p1), r0 = row_resource(p0), ro = row_resource(po);
    const int lane4 = lane * 4;
    constexpr int kBlockBytes = kM * (int)sizeof(double2), kRowBytes = 4 * kBlockBytes;
    const int rows2l = L > 0 ? 2 * L : 2 * l, half = L > 0 ? L : l, width = L > 0 ? BGBIT : bgbit;
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
            const int j = c * kN + 64 * q;
            const uint32_t a0 = row_word(r0, lane4, j), a1 = row_word(r0, lane4, j + kM);
            v0[q] = ((row_word(r1, lane4, j) - a0) + dec_offset) ^ dec_offset;
            v1[q] = ((row_word(r1, lane4, j + kM) - a1) + dec_offset) ^ dec_offset;
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
#pragma unroll 1
    for (int row = 1; row < rows2l; row++) {
        const int c = row >= half ? 1 : 0, q = row - c * half;
        if (q == 0) decompose(1);
        digit_row(32 - (q + 1) * width, row * kRowBytes, std::false_type{});
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
            const uint32_t a0 = row_word(r0e, lane4, j), a1 = row_word(r0e, lane4, j + kM);
            __builtin_amdgcn_raw_buffer_store_b32(a0 + e0, ro, lane4, j * 4, 0);
            __builtin_amdgcn_raw_buffer_store_b32(a1 + e1, ro, lane4, (j + kM) * 4, 0);
        }
    }
}

// next0 == next1: the difference is zero, every digit of 0 is 0, the product is zero and the CMux is exactly d0 -- a copy of
// the row, word for word what the product would have stored
__device__ __forceinline__ void automaton_copy_row(const int32_t* p0, int32_t* po, const int lane) {
    const __amdgpu_buffer_rsrc_t r0 = row_resource(p0), ro = row_resource(po);
    const int lane4 = lane * 4;
#pragma unroll
    for (int c = 0; c < 2; c++) {
        uint32_t w[16];
#pragma unroll
        for (int q = 0; q < 16; q++) w[q] = row_word(r0, lane4, c * kN + 64 * q);
#pragma unroll
        for (int q = 0; q < 16; q++) __builtin_amdgcn_raw_buffer_store_b32(w[q], ro, lane4, (c * kN + 64 * q) * 4, 0);
    }
}

// ---- one item per workgroup, every step of the launch inside it ----
// WORK.  Workgroup b (the grid is the piece's items exactly, so none is partly filled) owns item b; in step t wave w takes
// states w, w + G, .. (`rounds` = ceil(states / G) of them).  A state that is not live at t (bit q of live[t] clear: no output
// depends on it) is skipped, one whose two tables agree is copied; both leave every word of `out` what the full evaluation
// would give.  Everything that selects memory -- item, step, state, table entries (clamped into [0, states) although the
// object validated them), selector (clamped or taken mod n_set), final_of (clamped) -- is wave-uniform scalar arithmetic, and
// every row is an 8 KB buffer resource: nothing outside the rows AutomatonRows names can be touched whatever the arrays hold.
//
// MEMORY.  V_t for 0 < t < steps lives in global scratch, buffer t & 1 of the item's two of `states` rows; step t reads buffer
// (t + 1) & 1 (t = steps - 1: the caller's finals) and writes buffer t & 1 (t = 0: the caller's out, states below n_out only).
// The parity is t's, so a run cut into several launches (hi, lo) continues in the same buffers.
//
// HAND-OFF.  Rows stored by one wave in step t are loaded by the other waves of the SAME workgroup in step t - 1: the same CU,
// so workgroup scope is the right scope and nothing here is agent-scope -- no cache write-back, no invalidate, no flag.
//   * Every wave ends a step with s_waitcnt vmcnt(0) -- as inline assembly with a memory clobber, which the compiler can
//     neither drop nor move memory operations across -- and then joins the workgroup barrier.  vmcnt counts a store until the
//     memory system has acknowledged it, so when the barrier releases, every store of step t by every wave has completed and
//     every load of step t has returned (its value was consumed before the wave's own stores).  The loads of step t - 1 are
//     issued after the barrier.
//   * All waves of a workgroup run on one CU and go through that CU's one vector L1, which is write-through: a completed store
//     has updated (or dropped) the CU's own copy of the line and stands in L2, and a later load from the same CU cannot return
//     older bytes than that.  This is the same-CU coherence the AMDGPU memory model rests workgroup scope on (code objects
//     built without threadgroup-split mode, as these are: a workgroup-scope acquire needs no invalidate).  Hence the REUSE of a
//     scratch row two steps later is sound as well: row q of buffer t & 1 was read in step t + 1 (as V_{t+2}), perhaps by other
//     waves, and its old lines may still sit in L1 when step t stores V_t over it -- but those loads had returned before the
//     barrier that ended step t + 1, the stores come after it, and a load of step t - 1, after the next barrier, sees the
//     completed stores through the same L1.  No other CU ever reads an item's scratch rows; `out` is read by nobody in the launch.
//   * Between launches of a cut run the hand-off is the kernel boundary.
//
// BARRIERS.  One per step, after the drain: hi - lo of them for every wave of every workgroup, from launch arguments only.  A
// wave with no state in a round, a dead state or a copy skips the work inside the round loop, never the barrier; no wave
// returns before the step loop ends.
//
// hipcc: the register, LDS and scratch figures per build are in DESIGN.md section 4.12; __launch_bounds__(256, 2) and the
// static LDS sT [4][kTile] | tw [kTwElems] double2 = 46 080 B are k_cmux_x1's.
// The kernel's arguments as they stand in the kernarg segment (the first explicit argument at offset 0, each at its natural
// alignment): the round loop reads what it needs from there through an opaque pointer, per round, so that nothing of it is
// held in scalar registers across a CMux -- held, the loop state was spilled.
struct AutomatonKernargs {
    AutomatonRows A;
    const double2* bkf;
    const double2* gtw;
};
static_assert(std::is_standard_layout<AutomatonKernargs>::value && offsetof(AutomatonKernargs, bkf) == sizeof(AutomatonRows) && sizeof(AutomatonRows) % 8 == 0,
              "the kernels' first three arguments in kernarg order");
typedef const __attribute__((address_space(4))) AutomatonKernargs* AutomatonKernargPtr;

template <int L, int BGBIT, int G>
__device__ __forceinline__ void automaton_body(const int32_t hi, const int32_t lo, const int32_t rounds, const double2* __restrict__ gtw, const int l,
                                               const int bgbit, double2* sT_all, double2* sTw) {
    const WaveRow W = wave_prologue<G>(sT_all, sTw, gtw);
    const int lane = W.lane, wave = W.wave;
    double2* sT = W.sT;
    const LaneRoots R = make_roots(sTw, lane);
    constexpr size_t kRowWords = (size_t)2 * kN;
    constexpr int kBlockBytes = kM * (int)sizeof(double2), kRowBytes = 4 * kBlockBytes;

#pragma unroll 1
    for (int32_t t = hi - 1; t >= lo; t--) {
#pragma unroll 1
        for (int32_t round = 0; round < rounds; round++) {
            AutomatonKernargPtr K = (AutomatonKernargPtr)__builtin_amdgcn_kernarg_segment_ptr();
            asm volatile("" : "+s"(K));
            const int32_t states = K->A.states;
            const int32_t q = round * G + wave;
            if (q < (t == 0 ? K->A.n_out : states) && ((K->A.live[t] >> q) & 1)) {
                const int64_t b = blockIdx.x, item = K->A.item0 + b;
                const int32_t steps = K->A.steps;
                int32_t* const scratch = K->A.scratch + (size_t)b * 2 * (size_t)states * kRowWords;
                const int32_t* const final_of = K->A.final_of;
                const int32_t* src;
                if (t == steps - 1)
                    src = K->A.finals + (size_t)clamp_index(final_of ? (int64_t)final_of[item] : (int64_t)0, K->A.n_finals) * (size_t)states * kRowWords;
                else
                    src = scratch + (size_t)((t + 1) & 1) * (size_t)states * kRowWords;
                int32_t* const dst = t == 0 ? K->A.out + (size_t)b * (size_t)K->A.n_out * kRowWords : scratch + (size_t)(t & 1) * (size_t)states * kRowWords;
                const int32_t a = clamp_index(__builtin_amdgcn_readfirstlane(K->A.next0[(size_t)t * states + q]), states);
                const int32_t c = clamp_index(__builtin_amdgcn_readfirstlane(K->A.next1[(size_t)t * states + q]), states);
                const int32_t* p0 = src + (size_t)a * kRowWords;
                int32_t* po = dst + (size_t)q * kRowWords;
                if (a == c) {
                    automaton_copy_row(p0, po, lane);
                } else {
                    const int64_t sel = selector_at(K->A.sel_of, item * steps + t, K->A.n_set);
                    // the resource covers the selected sample only, as in k_cmux_x1
                    const int step_bytes = (L > 0 ? 2 * L : 2 * l) * kRowBytes;
                    const __amdgpu_buffer_rsrc_t bk_rsrc = bk_resource(K->bkf + (size_t)sel * ((size_t)step_bytes / sizeof(double2)), 1, step_bytes);
                    automaton_cmux<L, BGBIT>(src + (size_t)c * kRowWords, p0, po, bk_rsrc, l, bgbit, sT, lane, R);
                }
            }
        }
        // the hand-off: drain this wave's stores (and loads), then the workgroup barrier; see HAND-OFF above
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
}

template <int L, int BGBIT, int G = kCmuxWaveRows>
__global__ __launch_bounds__(64 * G, 2) void k_automaton_x1(AutomatonRows A, const double2* __restrict__ bkf, const double2* __restrict__ gtw) {
    __shared__ __align__(16) double2 sT_all[G * kTile];
    __shared__ __align__(16) double2 sTw[kTwElems];
    automaton_body<L, BGBIT, G>(A.hi, A.lo, (A.states + G - 1) / G, gtw, L, BGBIT, sT_all, sTw);
}
template <int G = kCmuxWaveRows>
__global__ __launch_bounds__(64 * G, 2) void k_automaton_rt(AutomatonRows A, const double2* __restrict__ bkf, const double2* __restrict__ gtw, int l,
                                                            int bgbit) {
    __shared__ __align__(16) double2 sT_all[G * kTile];
    __shared__ __align__(16) double2 sTw[kTwElems];
    automaton_body<0, 0, G>(A.hi, A.lo, (A.states + G - 1) / G, gtw, l, bgbit, sT_all, sTw);
}

// ---- steps == 0: out[i][q] = finals[final_of[i]][q], q < n_out ----
__global__ __launch_bounds__(256) void k_automaton_copy(const int32_t* __restrict__ finals, int32_t n_finals, const int32_t* __restrict__ final_of,
                                                        int64_t item0, int32_t states, int32_t n_out, int32_t* __restrict__ out) {
    const int64_t i = blockIdx.x;
    const int64_t f0 = final_of ? (int64_t)final_of[item0 + i] : 0;
    const int64_t f = f0 < 0 ? 0 : (f0 >= n_finals ? n_finals - 1 : f0);
    const int4* src = reinterpret_cast<const int4*>(finals + (size_t)f * (size_t)states * 2 * kN);
    int4* dst = reinterpret_cast<int4*>(out + (size_t)i * (size_t)n_out * 2 * kN);
    for (int q = threadIdx.x; q < n_out * (2 * kN / 4); q += 256) dst[q] = src[q];
}

}  // namespace

Automaton* Cmux::automaton_create(int32_t states, int32_t steps, int32_t n_out, const int32_t* next0, const int32_t* next1) {
    if (p_.N != 1024 || p_.k != 1) throw std::invalid_argument("automaton: the CMux kernels cover N = 1024, k = 1 only");
    const std::string refusal = automaton_refusal(states, steps, n_out, next0, next1);
    if (!refusal.empty()) throw std::invalid_argument(refusal);
    std::unique_ptr<Automaton> a(new Automaton);
    std::vector<uint64_t> live((size_t)steps + 1);
    a->cmuxes = automaton_live(states, steps, n_out, next0, next1, live.data());
    const size_t table = (size_t)steps * (size_t)states;
    a->next.allocate(2 * table + 1);
    a->live.allocate(live.size());
    if (table) {
        HIP_CHECK(hipMemcpy(a->next, next0, table * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy((int32_t*)a->next + table, next1, table * 4, hipMemcpyHostToDevice));
    }
    HIP_CHECK(hipMemcpy(a->live, live.data(), live.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    a->states = states;
    a->steps = steps;
    a->n_out = n_out;
    a->owner = id_;
    a->device = device_;
    return a.release();
}

void Cmux::check_owner(const Automaton& a) const {
    if (a.owner != id_ || !a.next || a.states < 1) throw std::invalid_argument("the automaton was compiled on another context");
}

void Cmux::reserve_automaton(CmuxScratch& scratch, const AutomatonPlan& pl) { scratch.a.reserve_exact((size_t)pl.scratch_rows * 2 * kN); }

int Cmux::launch_automaton(const TgswSet& set, const Automaton& a, CmuxScratch& scratch, hipStream_t stream, const AutomatonPlan& pl, int64_t item0,
                           int64_t items, const int32_t* sel_of, const int32_t* finals, int32_t n_finals, const int32_t* final_of, int32_t* out) {
    check_owner(set);
    check_owner(a);
    if (items <= 0) return 0;
    if (n_finals < 1) throw std::invalid_argument("automaton_run: n_finals must be at least 1");
    if (a.steps == 0) {
        hipLaunchKernelGGL(k_automaton_copy, dim3((unsigned)items), dim3(256), 0, stream, finals, n_finals, final_of, item0, a.states, a.n_out, out);
        return 1;
    }
    if (a.steps >= 2 && scratch.a.items() < (size_t)items * 2 * (size_t)a.states * 2 * kN)
        throw std::invalid_argument("automaton_run: piece larger than the reserved scratch");
    AutomatonRows R;
    R.finals = finals;
    R.out = out;
    R.scratch = scratch.a;
    R.sel_of = sel_of;
    R.final_of = final_of;
    R.next0 = a.next;
    R.next1 = (const int32_t*)a.next + (size_t)a.steps * (size_t)a.states;
    R.live = a.live;
    R.rows = items * kCmuxWaveRows;  // waves: one workgroup per item
    R.item0 = item0;
    R.n_finals = n_finals;
    R.states = a.states;
    R.steps = a.steps;
    R.n_out = a.n_out;
    for (int32_t j = 0; j < pl.launches; j++) {
        automaton_launch_steps(pl, a.steps, j, &R.hi, &R.lo);
        launch_rows(set, stream, R, [](auto ps) {
            if constexpr (decltype(ps)::L == 0)
                return k_automaton_rt<>;
            else
                return k_automaton_x1<ps.L, ps.BGBIT>;
        });
    }
    return pl.launches;
}

}  // namespace ieache
