// LWE key switch (K5), the one door: every kernel family, the byte-limb form of the key, the LDS grants and the choice among
// them (ks_plan.h) are behind this object.  A caller hands it extracted samples -- or a window of TLWE samples whose extracted
// rows it means (launch_window) -- and gets key-switched rows; it never learns which kernel ran.  Kernels: keyswitch.hip (the per-gate and gate-batched walks), keyswitch_sliced.hip, keyswitch_mfma.hip.
#pragma once
#include "device_buffer.h"
#include "device_common.h"
#include "ks_plan.h"

namespace ieache {

// Per-stream scratch of the key switch (counted in bytes): the MFMA product's transposed digits and output row addresses.
struct KsScratch {
    dev::DeviceBuffer<char> digits;
};

// One per evaluator.  All methods expect the evaluator's device to be current.
struct KeySwitch {
    // Grants the kernels their dynamic LDS on the current device.  Of K the key switch reads n, N, ks_t, ks_basebit and stride.
    // Throws std::invalid_argument for a parameter set whose generic key switch needs more than the LDS of a CU.
    void init(const Params& p, const dev::DevKeys& K);
    // The padded key [N][t][base][stride] (readable 16 rows past its end: the sliced walk prefetches), kept by the caller;
    // builds the byte-limb form of it where the MFMA product is usable (allocated once).
    void load_key(const int32_t* d_ksk_padded, hipStream_t stream);
    // Scratch for a launch of `cnt` gate instances ahead of time, so that launch() finds it in place (an allocation is a
    // device-wide synchronisation).
    void reserve(KsScratch& scratch, int64_t cnt, const EvalOptions& opt, bool force_generic);
    // out rows = key switch of `cnt` extracted samples (ext rows of N + 4 words): rows of flat_out, or where W puts gate
    // instance W.item0 + i.  Every family gives the same bits.
    void launch(KsScratch& scratch, hipStream_t stream, const dev::WorkDesc& W, int64_t cnt, const Torus32* ext, Torus32* flat_out,
                const EvalOptions& opt, bool force_generic);
    // The same for rows given as a window of samples (KsWindowRows, ks_plan.h): run row g -> row g of out_rows.  Where the plan
    // for `cnt` rows is the MFMA product the extracted rows are never stored and `ext` is not touched; otherwise they are
    // stored in ext (cnt rows of N + 4 words at least) and go through launch() as they are.  Every family gives the same bits.
    void launch_window(KsScratch& scratch, hipStream_t stream, int64_t cnt, const KsWindowRows& rows, Torus32* ext, Torus32* out_rows,
                       const EvalOptions& opt, bool force_generic);
    // whether launch_window of `cnt` rows needs `ext`
    bool window_needs_rows(int64_t cnt, const EvalOptions& opt, bool force_generic) const;
    // the extracted rows of such a window themselves: run row g -> N + 1 words of row g of u (rows of `stride` words)
    void extract_window(hipStream_t stream, int64_t cnt, const KsWindowRows& rows, Torus32* u, int32_t stride);

private:
    Params p_;
    dev::DevKeys K_{};
    KsSupport sup_;
    dev::DeviceBuffer<int8_t> limbs_;  // byte-limb form of the key for the MFMA product
};

}  // namespace ieache
