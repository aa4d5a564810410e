// Internal to the blind-rotation unit: the door of blind_rotate_h2.hip, the two-limb blind rotation on the ring of degree 2048
// (br_h2_supported(), br_plan.h) as two products on the ring of degree 1024 per CMux step.
//
// Exact by construction like every two-limb kernel: each rounded sum is 4l x 1024 = 2l x N products of a digit and a balanced
// 16-bit limb, what Params::br_exact() counts, so there is NO one-limb form, NO rounding guard and NO audit on such a context:
// a call at N = 2048 reports zero audited launches and a guard record that was never written.
#pragma once
#include "blind_rotate.h"

namespace ieache {
namespace h2 {

// double2 elements of the key form [n][2l rows][half: even, odd][q = 2 c + limb][8][64]: per BK_i, row and component c the
// two-limb spectra of the even and of the odd half of the polynomial, each in fft512's (register, lane) order.  The size of a
// direct 1024-point form: 248 MB at n = 630, l = 3.
size_t spectrum_elems(const Params& p);
// raw BK [n][2l][2][2048] int32 (device) -> that form
void prepare_spectrum(const Params& p, const Torus32* d_bk_raw, double2* d_bkf, hipStream_t stream);

// K0..K4 for the items of the parts: one prologue per part (mod switch to 2N = 4096; the constant polynomial, the item's test
// polynomial or its TLWE sample rotated by 2N - barb) into consecutive rows of the state block, then the CMux steps in slices
// of plan.slice <= 64 steps per launch, the last of which extracts into ext (rows of N + 4 words; may be null).
// state: items x br_state_bytes_per_item() bytes: [items][2][2048] int32 accumulators in coefficient order, then
// [items][br_bara_stride()] u16 rotation amounts.  dbg_acc [items][2][2048] (may be null; then pass ext = null).
// twiddles: the table of w64::build_twiddle_table.  Returns the kernel launches issued (the prologues not counted).
int launch(const Params& p, const dev::DevKeys& K, const double2* bkf, const double2* twiddles, const BrPlan& plan, hipStream_t stream,
           const BrPart* parts, size_t n_parts, void* state, Torus32* ext, int32_t steps, Torus32* dbg_acc);

}  // namespace h2
}  // namespace ieache
