// Internal to the key-switch unit (keyswitch.hip, keyswitch_sliced.hip, keyswitch_mfma.hip): the device lines its kernels
// share, and the launchers of the two families that live in files of their own.  The launchers decide nothing: the cut of a
// launch comes from ks_plan.h.
// A helper is used only where the kernel's instruction stream stays what it was spelled out: k_keyswitch_generic and _vec keep
// the output-row expression open-coded, k_keyswitch_batch both (through the helpers the compiler schedules them differently).
#pragma once
#include "device_common.h"
#include "ks_plan.h"

namespace ieache {
namespace dev {

// output row of gate instance `item` of a launch: row `item` of flat_out, or where the work descriptor puts it
__device__ __forceinline__ Torus32* ks_out_row(const WorkDesc& W, Torus32* flat_out, int64_t item, int32_t stride) {
    return flat_out ? flat_out + (size_t)item * stride : resolve(W, W.item0 + item, stride).out;
}
// digit j of a coefficient a' = a + prec_offset (lweKeySwitchTranslate_fromArray): its j-th group of basebit bits from the top
__device__ __forceinline__ uint32_t ks_digit(uint32_t a_off, int32_t j, int32_t basebit, uint32_t mask) {
    return (a_off >> (32 - (j + 1) * basebit)) & mask;
}

}  // namespace dev

namespace kss {
// The walk over the N coefficients in launches of `slice` coefficients each (partial sums are kept in the output rows in
// between), gates_per_wg = 4, 8, 16 or 32 gate instances per workgroup.  The key buffer must be readable 16 rows past its
// end (prefetch).  Returns the number of launches.
int launch(const Params& p, const dev::DevKeys& K, const dev::WorkDesc& W, int64_t items, const Torus32* ext, Torus32* flat_out,
           int32_t slice, int32_t gates_per_wg, hipStream_t stream);
}  // namespace kss

namespace ksm {
// padded KSK [N][t][base][stride] int32 (device) -> limb matrix in MFMA operand order, ks_limb_matrix_bytes(p) bytes
void prepare(const Params& p, const int32_t* d_ksk_padded, int8_t* d_limbs, hipStream_t stream);
// d_digits: ks_digit_scratch_bytes(p, items) bytes of scratch.  ksplit: the walk over the N coefficients cut into this many
// workgroups per (gate block, coefficient block), partial sums meeting through atomic adds; it must pass ks_mfma_split_ok.
// Returns the number of kernel launches.
int launch(const Params& p, const dev::DevKeys& K, const dev::WorkDesc& W, int64_t items, const Torus32* ext, Torus32* flat_out,
           const int8_t* d_limbs, void* d_digits, int32_t ksplit, int32_t xcd_map, hipStream_t stream);
// The same product on rows given as a window of samples (KsWindowRows, ks_plan.h): k_ksm_window_digits and k_ksm_window_init
// make the digits and the initial rows from the samples, k_ksm_gemm is launch()'s.  Run row g -> row g of out_rows (rows of
// K.stride words).  The same scratch, split rule and return value.
int launch_window(const Params& p, const dev::DevKeys& K, int64_t items, const KsWindowRows& rows, Torus32* out_rows, const int8_t* d_limbs,
                  void* d_digits, int32_t ksplit, int32_t xcd_map, hipStream_t stream);
// the extracted rows of such a window, stored: run row g -> N + 1 words of row g of u (rows of `stride` words).  Any parameter set.
void extract_window(const Params& p, int64_t items, const KsWindowRows& rows, Torus32* u, int32_t stride, hipStream_t stream);
}  // namespace ksm

}  // namespace ieache
