// Which key-switch kernel (K5) takes a launch, and cut how: THE statement of it (keyswitch.hip dispatches on the answer and
// sizes its scratch by it; nothing else decides).  Free of HIP so that the CPU tests can check it (tests/native/ks_plan_test.cpp).
//
//   Generic  k_keyswitch_generic     any parameter set, one workgroup per gate instance
//   PerGate  k_keyswitch_vec<nld>    one 512-thread workgroup per gate instance, or `splits` of them (+ k_keyswitch_init)
//   Batched  k_keyswitch_batch<16>   compiler-scheduled gate-batched walk (the cross-check)
//   Sliced   k_keyswitch_sliced<G>   hand-scheduled gate-batched walk, G gate instances per workgroup, `slice` coefficients per launch
//   Mfma     k_ksm_digits / _init / _gemm   the int8 product on the MFMA pipe, the walk over K cut into `ksplit`
//
// Rows given as a window of samples (KsWindowRows; unpack_plan.h): the same plan for the run's row count.  Mfma takes them
// through k_ksm_window_digits / k_ksm_window_init / k_ksm_gemm with no extracted row stored; every other family reads the rows
// k_ksm_window_rows stores.
#pragma once
#include <cstdint>

#include "evaluator_options.h"
#include "params.h"
#include "unpack_plan.h"

namespace ieache {

// `cnt` rows of a launch given as a window of TLWE samples: run row g is row row0 + g of samples [..][2][N] seen as
// [..][win.width] rows, the extracted row of coefficient win.first + q win.spread of sample (row0 + g) / win.width.
struct KsWindowRows {
    const Torus32* samples = nullptr;
    int64_t row0 = 0;
    UnpackWindow win;
};

// coefficients of B fragments in flight per wave of k_ksm_gemm: 8 (round 4; 4 until then: 0.658 -> 0.610 ms per 8 192 gates, profiles/r4_keyswitch_ahead.txt).
// 4 or 8: the walk of a K split is a multiple of 8 coefficients for every supported N (N % 64 == 0, splits <= 8).
#ifndef IEACHE_KS_AHEAD
#define IEACHE_KS_AHEAD 8
#endif

constexpr int32_t kKsMaxSlice = 1024;  // largest slice (coefficients i per launch) of the sliced walk: its digits in LDS, slice * G * 2 bytes <= 64 KiB
constexpr int32_t kKsMfmaWgGates = 512;  // gate instances per workgroup of k_ksm_gemm: four waves x four 32-row tiles
constexpr size_t kKsLdsMax = 160 * 1024;  // LDS of a CU

// What a parameter set allows, and the dynamic LDS its kernels ask for.
struct KsSupport {
    int nld = 0;          // dwordx4 loads per KSK row per wave of k_keyswitch_vec; 0 = only the generic kernel
    bool batch = false;   // gate-batched key switch usable (base == 4, digits fit 16 bits, columns fit 4 waves)
    bool sliced = false;  // hand-scheduled sliced variant of it usable (t = 8, basebit = 2, one int4 column per lane of at most 4 waves)
    bool mfma = false;    // libtfhe's decomposition t = 8, basebit = 2: one coefficient = 8 positions x 4 digit values = one K-step of 32
    size_t generic_lds = 0;  // u [N+4] | list [N*t]
    size_t vec_lds = 0;      // ... | part [8][stride]
    size_t batch_lds = 0;    // dw [16][N] u16 | bprime [16]
};

inline KsSupport ks_support(const Params& p) {
    KsSupport s;
    const int32_t stride = p.lwe_stride();
    const int nvec = stride / 4, nld = (nvec + 63) / 64;
    s.generic_lds = (size_t)(p.N + 4) * 4 + (size_t)p.N * p.ks_t * 4;
    s.vec_lds = s.generic_lds + (size_t)8 * stride * 4;
    s.batch_lds = (size_t)16 * p.N * 2 + 64;
    s.batch = p.ks_base() == 4 && p.ks_t * p.ks_basebit <= 16 && p.ks_t % 4 == 0 && nld <= 4;
    s.sliced = p.ks_t == 8 && p.ks_basebit == 2 && nvec <= 256 && p.N % 8 == 0 && nld <= 4;
    s.mfma = p.ks_t == 8 && p.ks_basebit == 2 && p.k == 1 && p.N % 64 == 0 && p.N >= 64;
    if (nld <= 4 && s.vec_lds <= kKsLdsMax) s.nld = nld;
    return s;
}

// A K split of the product is usable when it divides the N / 4 digit groups and leaves every split a whole number (>= 1) of
// the loop's trips of IEACHE_KS_AHEAD / 4 groups: the B fragments are preloaded a whole trip ahead, so a split shorter than a
// trip would multiply the NEXT split's fragments by stale digits and preload past the end of the limb table.
// (Two groups per trip with B fragments eight coefficients ahead: N = 1024 -> 1 .. 128, N = 64 -> 1 .. 8.)
inline bool ks_mfma_split_ok(const Params& p, int32_t ksplit) {
    constexpr int32_t groups_per_trip = IEACHE_KS_AHEAD / 4;
    if (ksplit < 1 || (p.N / 4) % ksplit != 0) return false;
    const int32_t per_split = p.N / 4 / ksplit;
    return per_split >= groups_per_trip && per_split % groups_per_trip == 0;
}

inline int32_t ks_coef_blocks(const Params& p) { return (p.lwe_stride() + 31) / 32; }  // 32 output coefficients per MFMA tile
inline int64_t ks_mfma_padded_items(int64_t items) { return (items + kKsMfmaWgGates - 1) / kKsMfmaWgGates * kKsMfmaWgGates; }
// bytes of the byte-limb form of the key-switch key (built once per key load): N * ceil(stride / 32) * 4096
inline size_t ks_limb_matrix_bytes(const Params& p) { return (size_t)p.N * ks_coef_blocks(p) * 4096; }
// bytes of digit scratch of the product for launches of up to `items` gate instances: the transposed digits and one output
// row address per (padded) gate instance
inline size_t ks_digit_scratch_bytes(const Params& p, int64_t items) {
    const int64_t gpad = ks_mfma_padded_items(items);
    return (size_t)(p.N / 4) * gpad * 8 + (size_t)gpad * sizeof(Torus32*);
}

enum class KsFamily { Generic, PerGate, Batched, Sliced, Mfma };

struct KsPlan {
    KsFamily family = KsFamily::Generic;
    int32_t splits = 1;        // PerGate: workgroups one gate's walk is cut into
    int32_t gates_per_wg = 0;  // Sliced: 4, 8, 16 or 32
    int32_t slice = 0;         // Sliced: coefficients per launch
    int32_t ksplit = 0;        // Mfma: workgroups the walk over K is cut into per (gate block, coefficient block)
    int32_t xcd_map = 0;       // Mfma: "ks_xcd", see k_ksm_gemm
};

// have_limbs: the byte-limb form of the key is loaded; cnt: gate instances of the launch.
inline KsPlan ks_plan(const KsSupport& s, const Params& p, const EvalOptions& o, bool have_limbs, bool force_generic, int64_t cnt) {
    KsPlan pl;
    const int nld = force_generic ? 0 : s.nld;
    if (!force_generic && s.mfma && have_limbs && cnt >= o.ks_mfma_min) {
        pl.family = KsFamily::Mfma;
        pl.xcd_map = (int32_t)o.ks_xcd;
        pl.ksplit = (int32_t)o.ks_mfma_split;
        if (pl.ksplit <= 0) {
            // One workgroup (4 waves, all 512 registers each) per CU at a time: W = gblocks * ncb workgroups take ceil(W k / CUs)
            // rounds of 1 / k of the walk each, plus a fixed cost per split (table build, one more pass of atomic adds).
            // Measured at n = 630 (profiles/r3_keyswitch_mfma.txt): 512 gates k = 8, 1 024 k = 4, 2 304 k = 2, 8 192 k = 4, 16 384 k = 2.
            const int64_t cus = o.cus <= 0 ? 256 : o.cus;
            const int64_t W0 = ks_mfma_padded_items(cnt) / kKsMfmaWgGates * ks_coef_blocks(p);
            double best = 0;
            for (int32_t k = 1; k <= 8; k *= 2) {
                if (!ks_mfma_split_ok(p, k)) break;
                const double cost = (double)((W0 * k + cus - 1) / cus) / k + 0.02 * k;
                if (pl.ksplit <= 0 || cost < best) {
                    best = cost;
                    pl.ksplit = k;
                }
            }
        }
        return pl;
    }
    if (nld > 0 && s.sliced && cnt >= o.ks_sliced_min) {
        pl.family = KsFamily::Sliced;
        const int32_t nco = p.N * p.k;
        pl.slice = (int32_t)o.ks_slice;
        if (pl.slice < 1 || pl.slice > kKsMaxSlice) pl.slice = kKsMaxSlice;
        if (pl.slice > nco) pl.slice = nco;
        // gates per workgroup: fewer row fetches per gate with 32, more workgroups in flight with 16 / 8
        pl.gates_per_wg = (int32_t)o.ks_gates;
        if (pl.gates_per_wg != 4 && pl.gates_per_wg != 8 && pl.gates_per_wg != 16 && pl.gates_per_wg != 32)  // measured (profiles/r1_v8_kernel_microbench.txt): 1024 -> 4, 2048-4096 -> 8, 8192 -> 16
            pl.gates_per_wg = cnt >= 14336 ? 32 : (cnt >= 5120 ? 16 : (cnt >= 1536 ? 8 : 4));
        return pl;
    }
    if (nld > 0 && s.batch && cnt >= o.ks_batch_min) {
        pl.family = KsFamily::Batched;
        return pl;
    }
    if (nld == 0) return pl;  // Generic
    pl.family = KsFamily::PerGate;
    // a handful of gates: cut each gate's walk into `splits` workgroups
    // measured: pays while gates x splits stays within ~1.5 workgroups per CU (1-8 gates: 0.18 -> 0.03 ms, 44: 0.09, 256: no gain)
    if (o.ks_split_max > 1)
        while (pl.splits < o.ks_split_max && cnt * pl.splits * 2 <= (3 * o.cus) / 2 && p.N % (pl.splits * 2) == 0) pl.splits *= 2;
    return pl;
}

// Digit scratch a launch of `cnt` gate instances needs ahead of time: that of the product when the plan is Mfma, none otherwise.
inline size_t ks_scratch_bytes(const KsSupport& s, const Params& p, const EvalOptions& o, bool have_limbs, bool force_generic, int64_t cnt) {
    return ks_plan(s, p, o, have_limbs, force_generic, cnt).family == KsFamily::Mfma ? ks_digit_scratch_bytes(p, cnt) : 0;
}

}  // namespace ieache
