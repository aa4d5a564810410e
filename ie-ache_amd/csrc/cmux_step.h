// Internal to the CMux family (cmux.hip, rotate.hip): what its kernels share beyond the CMux step of br_step.h, each stated
// once -- the rule that turns an index of the caller's into a member of a set, and a row [2][1024] through the buffer path.
// Forced inlines over the caller's registers, under br_step.h's rule: a kernel whose code a piece would change keeps its
// open-coded copy (the table there).
#pragma once
#include "blind_rotate_w64.h"
#include "br_step.h"
#include "cmux.h"

namespace ieache {
namespace w64 {
namespace {

// ---- indices of the caller's: a bad one reads another member of the set, never memory outside it ----
// a table or coefficient index: clamped into [0, n)
template <class T>
__device__ __forceinline__ T clamp_index(T i, int32_t n) {
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}
// the selector at position `at` of a call: explicit, sel_of[at] clamped into the set; with no array it is implied, the
// position itself taken mod n_set.  (The clamp is written out: through clamp_index the compiler narrows it to 32 bits in
// k_demux_x1.  k_cmux_x1 keeps its own copy of the rule: its flat form reads a piece's array at r but implies the call's
// item0 + r, and every shared form of that moved its code.)
__device__ __forceinline__ int64_t selector_at(const int32_t* sel_of, int64_t at, int32_t n_set) {
    int64_t sel;
    if (sel_of == nullptr) {
        sel = at % n_set;
    } else {
        sel = (int64_t)sel_of[at];
        sel = sel < 0 ? 0 : (sel >= n_set ? n_set - 1 : sel);
    }
    return sel;
}

// ---- the wave prologue of the one-wave kernels ----
// who the wave is, the twiddle table into LDS behind the kernel's one workgroup barrier, its tile and its row
struct WaveRow {
    int lane, wave;
    double2* sT;
    int64_t r;
};
template <int G>
__device__ __forceinline__ WaveRow wave_prologue(double2* sT_all, double2* sTw, const double2* __restrict__ gtw) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double2* sT = sT_all + wave * kTile;
    load_twiddles(sTw, gtw, tid, 64 * G);
    __syncthreads();  // the only workgroup barrier
    return WaveRow{lane, wave, sT, (int64_t)blockIdx.x * G + wave};
}

// ---- rows through the buffer path ----
// one row [2][1024] int32 as a buffer resource (its 8 KB, so nothing past it can be touched), and word j + lane of it (j a
// multiple of 64 known at compile time): resource and word offset in SGPRs, the lane's 4 bytes the only vector operand
__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_resource(const int32_t* row) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t*>(row), (short)0, 2 * kN * 4, 0x00020000);
}
__device__ __forceinline__ uint32_t row_word(__amdgpu_buffer_rsrc_t rsrc, int lane4, int j) {
    return (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rsrc, lane4, j * 4, 0);
}

}  // namespace
}  // namespace w64

// ---- which build of a one-wave kernel serves a set's gadget ----
// libtfhe's two gadgets keep the builds they had (w64::ParamSet, as the blind rotation's with_param_set names them; that
// dispatch is keyed by l alone and is not touched); every other gadget, and the two as well under the debug option
// "cmux_gadget_runtime", takes the build whose (l, Bgbit) are launch arguments.
struct RuntimeGadget {
    static constexpr int L = 0, BGBIT = 0, index = 2;
};
template <class F>
void with_gadget(int32_t l, int32_t Bgbit, bool runtime, F&& f) {
    if (!runtime && l == 3 && Bgbit == 7)
        f(w64::ParamSet<3, 7>{});
    else if (!runtime && l == 2 && Bgbit == 10)
        f(w64::ParamSet<2, 10>{});
    else
        f(RuntimeGadget{});
}

// ---- the launcher cmux.h declares ----
template <class Rows, class KernelOf>
void Cmux::launch_rows(const TgswSet& set, hipStream_t stream, Rows rows, KernelOf kernel_of, size_t lds, dev::LdsGrant* grant, const char* name,
                       const char* name_rt) {
    check_owner(set);
    if (rows.rows <= 0) return;
    rows.n_set = (int32_t)set.n;
    const unsigned grid = (unsigned)((rows.rows + kCmuxWaveRows - 1) / kCmuxWaveRows);
    with_gadget(set.l, set.Bgbit, runtime_always_ && *runtime_always_ != 0, [&](auto ps) {
        auto kernel = kernel_of(ps);
        if (grant) dev::allow_dynamic_lds_once(grant[ps.index], (const void*)kernel, lds, decltype(ps)::L == 0 ? name_rt : name);
        if constexpr (decltype(ps)::L == 0)
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * kCmuxWaveRows), lds, stream, rows, (const double2*)set.spectrum, (const double2*)tw_,
                               (int)set.l, (int)set.Bgbit);
        else
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * kCmuxWaveRows), lds, stream, rows, (const double2*)set.spectrum, (const double2*)tw_);
    });
}

}  // namespace ieache
