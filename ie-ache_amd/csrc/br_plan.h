// Which blind-rotation kernel (K0-K4) takes a launch of `cnt` gate instances, with how many CMux steps per launch, how many
// gates per workgroup, and whether as a rotation of roles: THE statement of it (blind_rotate.hip executes the answer, sizes
// its scratch by it and names it; nothing else decides).  Free of HIP so that the CPU tests can check it
// (tests/native/br_plan_test.cpp).
#pragma once
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>

#include "evaluator_options.h"
#include "mix_plan.h"
#include "params.h"

namespace ieache {

// Kernel variants ("br_variant" / IEACHE_BR_VARIANT; all produce identical bits).  kBrVariants below is the table
// everything is derived from, one row per number; the launch half of each row (threads, LDS, launcher) is kLaunchRows in
// blind_rotate_w64.hip, which does not compile unless both hold the same numbers.  0 lets br_plan() choose by launch size
// (<= one gate per CU -> 38, <= 2 per CU -> 43, <= 5 per CU -> 36, above -> 31; "exact_fft": 7 / 0 / 9); where a number is
// forced, 0 is the two-limb two-wave kernel.
//   two limbs (exact by construction):
//     9  k_blind_rotate_x1: one wave per gate (round 4; wide launches)
//     0  k_blind_rotate_w2: two waves per gate, split by output polynomial  12  every transpose through LDS (round 1)
//     7  k_blind_rotate_wide: 2L waves per gate (latency; any slice length up to n)   8  with s_memtime phase stamps on stderr
//   one limb with the rounding guard (on one rounded coefficient in four unless noted):
//     31 k_blind_rotate_w1b: one wave per gate (wide launches)   32 guard on every coefficient   35 no guard (measurement)   49 phase stamps
//     36 k_blind_rotate_w2r: two waves per gate, rows split (2 .. 5 gates per CU)      37 guard on every coefficient
//     43 k_blind_rotate_w4r: four waves per gate, rows 2:1:2:1 (1 .. 2 gates per CU)  44 guard on every coefficient
//     38 k_blind_rotate_wide4: 2L waves per gate, four output waves (<= 1 gate per CU) 39 guard on every coefficient
//     24 k_blind_rotate_wide on the one-limb spectrum (round 2's latency kernel, the A/B partner of 38)
// Every other number of rounds 1-3 (k_blind_rotate_w1, _w2s, _wide1, _wide4b and the template flags that lost their A/B) is
// refused; attic/README.md maps them to the profile that records each measurement.
constexpr int32_t kVariantWide = 7;
constexpr int32_t kVariantWideStamps = 8;
constexpr int32_t kVariantExactOneWave = 9;         // k_blind_rotate_x1 (round 4): two limbs, one wave per gate
constexpr int32_t kVariantTwoWavesLds = 12;
constexpr int32_t kVariantWideOneLimb = 24;
constexpr int32_t kVariantOneLimbDefault = 31;      // k_blind_rotate_w1b, guard on one coefficient in four (round 3)
constexpr int32_t kVariantOneLimbStamps = 49;
constexpr int32_t kVariantOneLimbTwoWaves = 36;     // k_blind_rotate_w2r (round 3)
constexpr int32_t kVariantOneLimbFourWaves = 43;    // k_blind_rotate_w4r (round 3): launches of one to two gates per CU
constexpr int32_t kVariantWideHandoverOneLimb = 38;  // k_blind_rotate_wide4 (round 3)

struct BrVariant {
    int32_t number;     // "br_variant"
    const char* name;   // the kernel
    bool chosen;        // what the choice by launch size reports under the kernel's name; false: a measurement or
                        // diagnostic build of it, reported by number
    int limbs;          // 1: the one-limb spectrum and the guard record (the sampled audit applies); 2: exact by construction
    bool long_slices;   // keeps a slice's rotation amounts in LDS or reloads them every 64 steps: a slice may be the whole rotation
    int gates;          // gate instances per workgroup of its default build
    bool wg_builds;     // builds for 1 .. gates - 1 per workgroup exist too: what a launch that does not fill the chip takes
                        // (the two kernels wide launches use)
};
inline constexpr BrVariant kBrVariants[] = {
    // number                        kernel                  chosen limbs long  gates builds
    // ---- two limbs: exact by construction ----
    {0,                               "k_blind_rotate_w2",    true,  2, false, 1, false},
    {kVariantTwoWavesLds,             "k_blind_rotate_w2",    false, 2, false, 1, false},  // every transpose through LDS (round 1)
    {kVariantExactOneWave,            "k_blind_rotate_x1",    true,  2, false, 4, true},
    {kVariantWide,                    "k_blind_rotate_wide",  true,  2, true,  1, false},
    {kVariantWideStamps,              "k_blind_rotate_wide",  false, 2, true,  1, false},  // phase stamps
    // ---- one limb, guarded (on one rounded coefficient in four unless noted) ----
    {kVariantWideOneLimb,             "k_blind_rotate_wide",  false, 1, true,  1, false},  // A/B partner of k_blind_rotate_wide4
    {kVariantOneLimbDefault,          "k_blind_rotate_w1b",   true,  1, false, 4, true},
    {kVariantOneLimbDefault + 1,      "k_blind_rotate_w1b",   false, 1, false, 4, false},  // guard on every coefficient
    {kVariantOneLimbDefault + 4,      "k_blind_rotate_w1b",   false, 1, false, 4, false},  // no guard arithmetic (measurement)
    {kVariantOneLimbStamps,           "k_blind_rotate_w1b",   false, 1, false, 4, false},  // phase stamps
    {kVariantOneLimbTwoWaves,         "k_blind_rotate_w2r",   true,  1, true,  1, false},
    {kVariantOneLimbTwoWaves + 1,     "k_blind_rotate_w2r",   false, 1, true,  1, false},  // guard on every coefficient
    {kVariantOneLimbFourWaves,        "k_blind_rotate_w4r",   true,  1, true,  1, false},
    {kVariantOneLimbFourWaves + 1,    "k_blind_rotate_w4r",   false, 1, true,  1, false},
    {kVariantWideHandoverOneLimb,     "k_blind_rotate_wide4", true,  1, true,  1, false},
    {kVariantWideHandoverOneLimb + 1, "k_blind_rotate_wide4", false, 1, true,  1, false},
};
// the row of `number`; null: no such variant
constexpr const BrVariant* br_variant(int32_t number) {
    for (const BrVariant& v : kBrVariants)
        if (v.number == number) return &v;
    return nullptr;
}
// whether `number` has a build for `gates` gate instances per workgroup
constexpr bool br_variant_build(int32_t number, int gates) {
    const BrVariant* v = br_variant(number);
    return v && (gates == v->gates || (v->wg_builds && gates >= 1 && gates < v->gates));
}
inline bool variant_known(int32_t v) { return br_variant(v) != nullptr; }
// takes the one-limb spectrum and the guard record (the sampled audit applies)
inline bool variant_one_limb(int32_t v) {
    const BrVariant* r = br_variant(v);
    return r && r->limbs == 1;
}
// the kernel's name for the numbers the choice by launch size uses (0, 7, 9, 31, 36, 38, 43); null for the measurement and
// diagnostic builds, which are reported by number, and for unknown numbers
inline const char* variant_kernel_name(int32_t v) {
    const BrVariant* r = br_variant(v);
    return r && r->chosen ? r->name : nullptr;
}

// The 64-lane kernels: N=1024, k=1 with either libtfhe parameter set: l=3/Bgbit=7 (>= v1.1, "128-bit") or l=2/Bgbit=10
// (v1.0 and the paper's 78 MiB keys).  Exactness margin for the latter: 4 rows x 1024 x 512 x 2^15 < 2^37.
inline bool br_supported(const Params& p) {
    return p.N == 1024 && p.k == 1 && ((p.l == 3 && p.Bgbit == 7) || (p.l == 2 && p.Bgbit == 10)) && p.n <= 4096;
}
// The one-limb kernels round sums of up to 2l x N x 2^(Bgbit-1) x 2^31: 2^49.6 for l=3 / Bgbit=7, where the measured
// rounding error is 35x below the guard's limit.  For l=2 / Bgbit=10 the worst case is 2^52 and the typical error 6.5x
// larger -- inside 0.5 but no longer clear of the limit -- so that set stays on the two-limb kernels.
inline bool br_one_limb_supported(const Params& p) { return br_supported(p) && p.l == 3 && p.Bgbit == 7; }
// The ring of degree 2048 (blind_rotate_h2.hip): one two-limb kernel, two waves per gate, (l, Bgbit) as launch arguments for
// every gadget of at most 16 digit rows; longer gadgets stay on the any-parameter kernel.  No one-limb form.
inline bool br_h2_supported(const Params& p) { return p.N == 2048 && p.k == 1 && 2 * p.l <= 16 && p.supported(); }
// rotation amounts per gate instance as the kernels keep them (u16, padded to 16 bytes)
inline int32_t br_bara_stride(const Params& p) { return (p.n + 7) & ~7; }
// bytes of blind-rotation state (accumulator + rotation amounts) one gate instance keeps in HBM between slices
inline size_t br_state_bytes_per_item(const Params& p) { return (size_t)br_bara_stride(p) * 2 + (size_t)2 * (p.N == 2048 ? 2048 : 1024) * 4; }

// dynamic LDS of k_blind_rotate_generic: F [max(kpl, 4)][N / 2] double2 | acc [2][N] int32 | bara [n] u16 (padded to 16 bytes).
// BlindRotate::init refuses a set that needs more than kBrLdsMax.  At N = 2048: 2l = 8 rows of 16 KiB + 16 KiB + bara fit, l >= 5 does not.
constexpr size_t kBrLdsMax = 160 * 1024;  // LDS of a CU
inline size_t br_generic_lds_bytes(const Params& p) {
    const size_t frows = p.kpl() > 4 ? p.kpl() : 4;
    return frows * (size_t)(p.N / 2) * 16 + (size_t)2 * p.N * 4 + (((size_t)p.n * 2 + 15) & ~(size_t)15);
}

// What the choice reads of the call in progress, besides its options.
struct BrCall {
    bool exact = false;               // the call is a repeat after a guard trip ("exact_fft" stays in the options)
    int32_t concurrency = 1;          // streams issuing launches side by side right now (the choice is by cnt x concurrency)
    bool level_on_two_lanes = false;  // a level's halves are being queued on two streams
    bool whole_rotation = true;       // all n CMux steps (false: the first `steps` of a debug call)
    bool lane0 = true;                // the launch is on the context's own stream
};

struct BrPlan {
    bool generic = true;    // k_blind_rotate_generic, one workgroup per gate instance; nothing below applies
    bool h2 = false;        // k_blind_rotate_h2 (N = 2048): of the fields below only `slice` applies, 1 .. 64
    int32_t variant = 0;    // a number of kBrVariants
    int32_t slice = 0;      // CMux steps per launch, final: 1 .. 64, or up to br_bara_stride() where the kernel has long_slices
    int32_t wg_gates = 0;   // gate instances per workgroup, where the kernel has a build for it (else its default build)
    MixGeometry mix;        // the rotation of roles (mix_plan.h); k == 0: none
    MixSteps mix_steps;
    MixGeometry mix_named;  // the geometry the launch size names, which the label reports: mix, except where no round of turns
                            // fits the rotation (a short LWE dimension, long "mix_s1") and the launch therefore runs without
    bool mix_sync = false;  // a barrier across its streams at every phase boundary
    int32_t mix_wg = 4;     // gate instances per workgroup of its one-wave turns (LDS: with two two-wave gates per CU, 4 or 2 x 2 fit)
    int32_t w4r_flip = 0;   // k_blind_rotate_w4r: workgroups i and i + this are taken to share a CU
    int32_t concurrency = 1;  // as chosen for (a label may say so)
};

// the two-limb latency kernel over the whole rotation in one launch: what the sampled audit runs its sample on
inline BrPlan br_exact_plan(const Params& p) {
    BrPlan pl;
    pl.generic = false;
    pl.variant = kVariantWide;
    pl.slice = br_bara_stride(p);
    return pl;
}

// use_w64: the 64-lane kernels serve this call (br_supported() and not "force_generic"); cnt: gate instances of the launch.
// br_variant 0 = by launch size: the 2L-waves-per-gate kernel for a handful of gates, two waves per gate on the one-limb
// spectrum while every gate is resident at once, one wave per gate above; "exact_fft" / a repeat after a guard trip: the
// two-limb kernels.
inline BrPlan br_plan(const Params& p, const EvalOptions& o, const BrCall& c, bool use_w64, int64_t cnt) {
    BrPlan pl;
    pl.generic = !use_w64;
    pl.concurrency = c.concurrency;
    if (pl.generic) {
        // N = 2048: the one kernel of that ring unless "force_generic"; slices as the one-wave kernels of N = 1024 take them
        if (br_h2_supported(p) && !o.force_generic) {
            pl.generic = false;
            pl.h2 = true;
            pl.slice = (o.br_slice >= 1 && o.br_slice <= 64) ? (int32_t)o.br_slice : (int32_t)o.br_slice_default;
        }
        return pl;
    }
    const bool exact = o.exact_fft || c.exact;
    const int32_t nb = br_bara_stride(p);
    int32_t variant = (int32_t)o.br_variant, slice = (int32_t)o.br_slice;
    const int64_t flight = cnt * c.concurrency;  // the other stream's launch of the same level shares the chip: choose by the gates in flight
    if (variant == 0) {
        if (flight <= o.br_wide_max) {
            // the latency kernel, on the one-limb spectrum unless exactness by construction is asked for
            variant = exact ? kVariantWide : kVariantWideHandoverOneLimb;
            slice = nb;
        } else if (!exact && flight >= o.one_limb_min) {
            // one to two gates per CU: four waves per gate (two waves per SIMD); while every gate fits a two-wave slot, two
            // waves per gate finish a step sooner than one
            variant = flight <= o.four_wave_max ? kVariantOneLimbFourWaves
                      : flight <= o.two_wave_max ? kVariantOneLimbTwoWaves : kVariantOneLimbDefault;
            // every gate of such a launch is resident at once, so nothing is gained from short slices (they keep the rounds
            // of a WIDE launch on the same BK blocks) and each launch boundary costs a tail and a reload of the accumulators:
            // the whole rotation in one launch for four waves per gate, 64 steps for two (interleaved A/B, profiles/r3_slice_ab.txt)
            // (likewise one wave per gate while the launch is a single round of 8 gates per CU)
            if (slice <= 0)
                slice = variant == kVariantOneLimbFourWaves ? nb
                        : (variant == kVariantOneLimbTwoWaves || flight <= 8 * o.cus) ? 64 : slice;
        } else if (flight >= o.exact_one_wave_min) {
            variant = kVariantExactOneWave;  // "exact_fft" / a repeat: the two-limb product, one wave per gate
            if (slice <= 0 && flight <= 8 * o.cus) slice = 64;  // a single round of resident gates: as above
        }
    } else if (c.exact && variant_one_limb(variant)) {
        variant = flight >= o.exact_one_wave_min ? kVariantExactOneWave : 0;
    }
    const BrVariant* row = br_variant(variant);
    if (!row) throw std::invalid_argument("unknown blind-rotation variant");
    pl.variant = variant;
    // 1 .. 64 for the kernels that keep one rotation amount per lane, up to the whole rotation for those with long_slices;
    // anything else -- "br_slice" 0 with several rounds of resident gates, or a value the kernel cannot take -- is
    // "br_slice_default" (16: the rounds of a wide launch stay on the same BK blocks while they are hot in L2)
    pl.slice = (slice >= 1 && slice <= (row->long_slices ? nb : 64)) ? slice : (int32_t)o.br_slice_default;
    // Gate instances per workgroup of the one-wave-per-gate kernels.  Four share a workgroup (for the twiddle table only) and
    // two such workgroups fill a CU; a launch of at most six gates per CU in fours leaves half the CUs with two workgroups and
    // half with one, in threes every CU gets the same six waves.
    pl.wg_gates = o.wg_gates ? (int32_t)o.wg_gates : (flight <= o.wg3_max ? 3 : 4);
    // workgroups i and i + period are taken to share a CU: the device's CU count ("w4r_flip" overrides; a huge value = never flip)
    pl.w4r_flip = (int32_t)(o.w4r_flip > 0 ? o.w4r_flip : o.cus > 0 ? o.cus : 256);
    // A rotation of roles only where it can pay: the kernels chosen by launch size (br_variant 0) on the one-limb spectrum,
    // the launch alone on the chip (no other stream of this context at work), a whole rotation on the context's own stream,
    // and a size mix_plan.h names: 4 .. 7 gates per CU, or a full round of the one-wave kernel plus a small remainder
    // (8 .. 10.5 per CU).  "mix_k" / "mix_tw" force a geometry (measurement aid), 0 = by launch size.
    if (!o.overlap || !o.br_mix || o.br_variant != 0 || c.concurrency != 1 || c.level_on_two_lanes || exact) return pl;
    if (!c.whole_rotation || !c.lane0 || row->limbs != 1) return pl;
    MixGeometry g;
    MixSteps m;
    if (!mix_geometry_for(o.cus, cnt, (int)o.mix_k, (int)o.mix_tw, &g) || g.k > kMaxLanes) return pl;
    pl.mix_named = g;
    if (!mix_steps_for(p.n, g, (int32_t)o.mix_s1, (int32_t)o.mix_ratio, &m) || m.covered >= p.n) return pl;  // the slice loop keeps a step: it extracts
    pl.mix = g;
    pl.mix_steps = m;
    pl.mix_sync = o.mix_sync != 0;
    pl.mix_wg = (int32_t)o.mix_wg;
    return pl;
}

// The name of what a plan launches (Evaluator::kernel_for_launch): the kernel with its parameter set; a rotation of roles
// between the two kernels with its geometry; a measurement or diagnostic build by number.
inline std::string br_kernel_label(const Params& p, const BrPlan& pl) {
    if (pl.generic) return "k_blind_rotate_generic";
    char tag[96];
    if (pl.h2) {
        snprintf(tag, sizeof tag, "<%d,%d>", (int)p.l, (int)p.Bgbit);
        return std::string("k_blind_rotate_h2") + tag;
    }
    if (pl.mix_named.k) {  // tw of k subsets on two waves at a time
        snprintf(tag, sizeof tag, "<%d,%d> %d of %d subsets on two waves", (int)p.l, (int)p.Bgbit, pl.mix_named.tw, pl.mix_named.k);
        return std::string("k_blind_rotate_w2r+w1b") + tag;
    }
    if (const char* kernel = variant_kernel_name(pl.variant)) {
        snprintf(tag, sizeof tag, "<%d,%d>", (int)p.l, (int)p.Bgbit);
        return std::string(kernel) + tag;
    }
    snprintf(tag, sizeof tag, "<%d,%d> br_variant %d", (int)p.l, (int)p.Bgbit, (int)pl.variant);
    return std::string("k_blind_rotate") + tag;
}

}  // namespace ieache
