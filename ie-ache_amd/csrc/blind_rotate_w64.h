// Internal to the blind-rotation unit (blind_rotate.hip, blind_rotate_w64.hip): the key forms and the launcher of the
// kernels specialised for N=1024, k=1 and libtfhe's two default gate-bootstrapping sets (br_supported(), br_plan.h).  The
// launcher decides nothing: variant, slice length, gates per workgroup and the rotation of roles come from the plan.
#pragma once
#include "blind_rotate.h"

namespace ieache {
namespace w64 {

// number of double2 elements of the two-limb BK spectrum in these kernels' layout, of the one-limb form (k_blind_rotate_w1b
// and the other guarded kernels), and of the kernels' twiddle table
size_t spectrum_elems(const Params& p);
size_t spectrum1_elems(const Params& p);
size_t twiddle_table_elems();
// raw BK [n][2l][2][N] int32 (device) -> two-limb spectrum [n][2l][4][8][64] double2 / one-limb [n][2l][2][8][64] double2
void prepare_spectrum(const Params& p, const Torus32* d_bk_raw, double2* d_bkf, hipStream_t stream);
void prepare_spectrum1(const Params& p, const Torus32* d_bk_raw, double2* d_bkf1, hipStream_t stream);
void build_twiddle_table(double2* d_tw, hipStream_t stream);

// the one place that turns the runtime parameter set into template arguments (br_supported(): these two only).  The CMux
// family (cmux.hip, rotate.hip) names its two fixed builds by ParamSet too but dispatches by the SET's gadget: with_gadget, cmux_step.h
template <int L_, int BGBIT_>
struct ParamSet {
    static constexpr int L = L_, BGBIT = BGBIT_, index = L_ == 3 ? 0 : 1;
};
template <class F>
void with_param_set(int32_t l, F&& f) {
    if (l == 3)
        f(ParamSet<3, 7>{});
    else
        f(ParamSet<2, 10>{});
}

// what the kernels read besides the work: both spectra, the twiddle table, the three-word guard record of the one-limb
// kernels, and the stamp buffer of the diagnostic builds (16 words; null unless the plan names one of them)
struct Tables {
    const double2 *bkf = nullptr, *bkf1 = nullptr, *twiddles = nullptr;
    unsigned* guard = nullptr;
    unsigned long long* diag = nullptr;
};

// K0..K4 for `items` gate instances as `plan` says: prologue, then the CMux steps in slices of plan.slice steps per launch.
// Rotation of roles for mid-size launches (launch_mixed_phases): plan.mix.k <= 4 subsets of the items on as many streams,
// (mix.streams[0] = the launch's own; events without timing), mix.tw of them at a time on the two-waves-per-gate kernel for s2 steps while the others take s1 (<= 64 x any) steps on the
// one-wave-per-gate kernel; `cycles` rounds of k phases, the rest of the rotation by the ordinary slice loop.
// state: items * br_state_bytes_per_item() bytes of scratch.
// ext rows of N+4 int32 (may be null), dbg_acc [items][2][N] (may be null; when set, pass ext = null).
// Returns the number of blind-rotation kernel launches issued (the prologue not counted).
// parts: the items' descriptors -- one prologue per part into consecutive rows of the state block (the TV build chosen per
// part), then everything else over all `items` = sum of the parts' counts.
int launch(const Params& p, const dev::DevKeys& K, const Tables& t, const BrPlan& plan, const BrLanes& mix, hipStream_t stream,
           const BrPart* parts, size_t n_parts, void* state, Torus32* ext, int32_t steps, Torus32* dbg_acc);

}  // namespace w64
}  // namespace ieache
