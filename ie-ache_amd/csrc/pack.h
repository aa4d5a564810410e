// Packing key switch (LWE rows -> TLWE samples; the public functional key switch with f = placement of the phases into
// coefficients, include/ieache.h section 3e), the one door: the kernels, the byte-limb form of the packing key, the scratch
// and the cut of a call (pack_plan.h) are behind this object.  Kernels: pack_keyswitch.hip.
#pragma once
#include <memory>

#include "device_buffer.h"
#include "pack_plan.h"
#include "project_plan.h"

namespace ieache {

// Scratch of a call on one stream: the pieces' R rows [rows][2][N] and their digits.
struct PackScratch {
    dev::DeviceBuffer<char> r, digits;
};

// One per evaluator and key: the packing key's, and a second one on project_params() for the projection key (section 3l).
// All methods expect the evaluator's device to be current.
struct Pack {
    void init(const Params& p) { p_ = p; }
    // pk [n][t][2][N] int32 on the HOST -> the byte-limb form on the device, the only form kept (the int32 key is scratch of
    // this call); a second call replaces the first key, pk == null drops it.  Synchronises the stream.  Throws
    // std::invalid_argument for a decomposition pack_set_error refuses.
    void set_key(int32_t t, int32_t basebit, const int32_t* pk, hipStream_t stream);
    bool has_key() const { return limbs_ != nullptr; }
    int32_t t() const { return t_; }
    // the cut of a call of `groups` groups of m rows with this object's key (pack_plan on its parameter set, which for the
    // projection is project_plan): piece_rows_opt "pack_piece_rows", split_opt the object's forced split, cus the device's
    PackPlan plan(int64_t groups, int32_t m, int64_t piece_rows_opt, int32_t split_opt, int64_t cus) const {
        return pack_plan(p_, t_, groups, m, piece_rows_opt, split_opt, cus);
    }
    // scratch for every piece of the plan ahead of the loop, so that no piece allocates
    void reserve(PackScratch& scratch, const PackPlan& pl);
    // one piece: `groups` groups of m rows of `stride` words (n + 1 read) -> out [groups][2][N]
    void launch(PackScratch& scratch, hipStream_t stream, const PackPlan& pl, int64_t groups, int32_t m, int32_t spread, int32_t shift,
                const Torus32* rows, int32_t stride, Torus32* out);
    // one piece of a projection (section 3l; project_plan.h), on an object initialised with project_params(): `items` TLWE
    // samples tlwe [items][2][N] and the window (first, width, dest) instead of rows -> out [items][2][N]; the extracted rows
    // are never stored (k_window_digits), the product and the placement are launch()'s.  out must not overlap tlwe.
    void launch_window(PackScratch& scratch, hipStream_t stream, const PackPlan& pl, int64_t items, int32_t first, int32_t width, int32_t dest,
                       const Torus32* tlwe, Torus32* out);

private:
    Params p_;
    int32_t t_ = 0, basebit_ = 0;
    std::unique_ptr<dev::DeviceBuffer<int8_t>> limbs_;  // byte-limb form of the key for the product; null: no key
};

}  // namespace ieache
