// The evaluator's named options and read-only figures (Evaluator::set_option / get_option, ieache_ctx_set_option /
// _get_option): ONE table.  A row gives the name, the environment variable read once when a context is created (or none),
// the accepted range, and where the value lives in EvalOptions.  Free of HIP so that a host test can walk it.
// What the stream modes ("overlap", "pipe_*", "br_mix") do is explained at Evaluator::set_option in evaluator.h.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace ieache {

constexpr int kMaxLanes = 4;  // streams of one context (evaluator.hip: Lane)

// Every value is an int64_t so that one kind of member pointer reaches them all.  "per CU" defaults are set in
// Evaluator::init(), next to the measurements they come from.
struct EvalOptions {
    int64_t chunk = 65536;  // (scratch grows on demand up to this, see dev::grown())
    int64_t force_generic = 0;
    // key switch: which kernel takes a launch of how many gate instances
    int64_t ks_batch_min = 4096;  // one workgroup walk takes ~5 ms
    int64_t ks_sliced_min = 576;  // measured crossover with the per-gate kernel: ~560
    int64_t ks_slice = 0, ks_gates = 0;
    int64_t ks_mfma_min = 64;     // measured crossover with the per-gate walk: ~40 gates (0.08 ms either way)
    int64_t ks_mfma_split = 0, ks_split_max = 16;
    int64_t ks_xcd = 0;
    // packing key switch: how a call is cut (pack_plan.h)
    int64_t pack_split = 0, pack_piece_rows = 4096;
    int64_t project_split = 0;  // the projection (project_plan.h): pack_split's sibling for the projection key's walk
    // CMux on caller TGSW samples and its tree: rows of a piece (cmux_plan.h)
    int64_t cmux_piece_rows = 8192;
    int64_t cmux_gadget_runtime = 0;  // debug: every TGSW set on the run-time-gadget builds (cmux_step.h)
    int64_t automaton_steps_per_launch = 0;  // automata: steps of one launch at most (automaton_plan.h); 0 = by the plan
    int64_t linear_kernel = 0;  // linear layers (linear_plan.h): 0 = by n_out, 1 = the simple kernel, 2 = the MFMA product
    // blind rotation: which kernel takes a launch of how many gate instances (br_plan.h)
    int64_t br_slice = 0, br_slice_default = 16, br_variant = 0;
    int64_t br_wide_max = 0, one_limb_min = 0, four_wave_max = 0, two_wave_max = 0;  // per CU
    int64_t exact_one_wave_min = 1025;                                                // per CU
    int64_t wg_gates = 0, wg3_max = 0;                                                // wg3_max per CU
    int64_t w4r_flip = 0;
    int64_t exact_fft = 0;
    int64_t fft_audit = 64, fft_audit_inject = 0, fft_guard_inject = 0;
    // stream modes
    int64_t overlap = 1, overlap_min = 0;               // overlap_min per CU
    int64_t pipe_min = 0, pipe_lanes = 2, pipe_auto = 1;  // pipe_min per CU
    int64_t br_mix = 1, mix_s1 = 16, mix_ratio = 200, mix_sync = 0, mix_wg = 2, mix_k = 0, mix_tw = 0;
    // read-only figures
    int64_t cus = 0, resident_gates = 1024;
    int64_t overlapped_levels = 0, pipelined_evals = 0, tuned_evals = 0, mixed_launches = 0, staging_allocations = 0;
};

struct OptionRow {
    const char* name;
    const char* env;  // or nullptr
    int64_t EvalOptions::*at;
    int64_t lo, hi;         // accepted values; lo > hi: a read-only figure
    bool (*ok)(int64_t);    // a further condition on a value in range, or nullptr
    const char* doc;
};

constexpr int64_t kNoLimit = INT64_MAX;
inline bool pow2_or_0(int64_t v) { return (v & (v - 1)) == 0; }
inline bool ks_gates_ok(int64_t v) { return v == 0 || v == 4 || v == 8 || v == 16 || v == 32; }
inline bool not_1(int64_t v) { return v != 1; }
#define IEACHE_OPT(name, env) #name, env, &EvalOptions::name
#define IEACHE_FIGURE(name) #name, nullptr, &EvalOptions::name, 1, 0, nullptr

// Which key-switch kernel these select for a launch is stated in ks_plan.h, which blind-rotation kernel in br_plan.h.
// Conditions that need the device or the parameter set, and effects beyond storing the value, are in Evaluator::option_hook
// (evaluator.hip); the rows they apply to say "hook".
inline constexpr OptionRow kOptionTable[] = {
    {IEACHE_OPT(chunk, nullptr), 1, kNoLimit, nullptr, "gate instances per launch at most"},
    {IEACHE_OPT(force_generic, nullptr), INT64_MIN, kNoLimit, nullptr, "hook (stored as 0 / 1): the any-parameter kernels even where a specialised one exists"},
    {IEACHE_OPT(ks_batch_min, "IEACHE_KS_BATCH_MIN"), 0, kNoLimit, nullptr, "launches from this size: the compiler-scheduled gate-batched key switch (the cross-check)"},
    {IEACHE_OPT(ks_sliced_min, "IEACHE_KS_SLICED_MIN"), 0, kNoLimit, nullptr, "launches from this size: the hand-scheduled sliced key switch"},
    {IEACHE_OPT(ks_slice, nullptr), 0, 1024, nullptr, "coefficients per launch of the sliced key switch (up to kKsMaxSlice, ks_plan.h); 0 = the whole walk"},
    {IEACHE_OPT(ks_gates, nullptr), 0, 32, ks_gates_ok, "its gate instances per workgroup: 4, 8, 16, 32; 0 = by launch size"},
    {IEACHE_OPT(ks_mfma_min, "IEACHE_KS_MFMA_MIN"), 0, kNoLimit, nullptr, "launches from this size: the key switch as an int8 product on the MFMA pipe (keyswitch_mfma.hip)"},
    {IEACHE_OPT(ks_mfma_split, nullptr), 0, 64, pow2_or_0, "hook (ks_mfma_split_ok, ks_plan.h): workgroups its walk is cut into per tile, a power of two; 0 = by launch size"},
    {IEACHE_OPT(ks_xcd, "IEACHE_KS_XCD"), 0, 1, nullptr, "measurement aid: 1 = each XCD walks its own eighth of the MFMA key switch's streams (measured slower, see k_ksm_gemm)"},
    {IEACHE_OPT(ks_split_max, nullptr), 1, 64, nullptr, "workgroups the per-gate key switch may cut one gate's walk into when a launch holds a handful of gates; 1 = never"},
    {IEACHE_OPT(pack_split, nullptr), 0, 8, pow2_or_0, "hook (pack_split_ok, pack_plan.h, for the packing key that is set): waves the packing key switch's walk over K is cut into per tile; 0 = by size"},
    {IEACHE_OPT(pack_piece_rows, nullptr), 1, 4096, nullptr, "rows of a piece of a packing call, and of a projection (whole items of `width` rows), at most (whole groups; up to kPackPieceRows, pack_plan.h)"},
    {IEACHE_OPT(project_split, nullptr), 0, 8, pow2_or_0, "hook (pack_split_ok for the projection key that is set, project_plan.h): waves the projection's walk over K = N t is cut into per tile; 0 = by size"},
    {IEACHE_OPT(cmux_piece_rows, nullptr), 1, 1 << 20, nullptr, "rows of a launch of a CMux call, and of the first level of a piece of a CMux tree, at most (whole items; default kCmuxPieceRows = 8192: 96 MB of tree scratch; cmux_plan.h)"},
    {IEACHE_OPT(cmux_gadget_runtime, nullptr), 0, 1, nullptr, "unstable, measurement aid: 1 = every TGSW set runs on the builds of the CMux kernels that take (l, Bgbit) as launch arguments, the key's two gadgets included"},
    {IEACHE_OPT(automaton_steps_per_launch, nullptr), 0, 4096, nullptr, "steps of an automaton per launch at most (1 = a launch per step, the hand-off a kernel boundary); 0 = every step in one launch while steps x rounds stays within kAutomatonLaunchRounds, equal chunks above (automaton_plan.h)"},
    {IEACHE_OPT(linear_kernel, nullptr), 0, 2, nullptr, "the kernel of lwe_linear: 1 = a thread per output word (k_linear_simple), 2 = the int8 MFMA product (k_linear_mfma); 0 = by n_out (kLinearMfmaMinOut, linear_plan.h)"},
    {IEACHE_OPT(br_slice, nullptr), 0, 4096, nullptr, "CMux steps per blind-rotation launch; 0 = by kernel and launch size (16 over several rounds of resident gates, 64 while all are resident, the whole rotation for the four-wave and latency kernels)"},
    {IEACHE_OPT(br_slice_default, "IEACHE_BR_SLICE"), 1, 64, nullptr, "... where neither br_slice nor the launch size says otherwise, and where the kernel cannot take what br_slice says"},
    {IEACHE_OPT(br_variant, "IEACHE_BR_VARIANT"), 0, 1000, nullptr, "hook (variant_known; a retired number is reported on stderr): a number of br_plan.h's table; 0 = by launch size"},
    {IEACHE_OPT(br_wide_max, "IEACHE_BR_WIDE_MAX"), 0, kNoLimit, nullptr, "launches up to this size: the latency-oriented 2L-waves-per-gate kernel (default 1 per CU; 0 = never)"},
    {IEACHE_OPT(one_limb_min, "IEACHE_ONE_LIMB_MIN"), 0, kNoLimit, nullptr, "launches from this size: the one-limb kernels (default 1 per CU + 1)"},
    {IEACHE_OPT(four_wave_max, nullptr), 0, kNoLimit, nullptr, "of those, launches up to this size: four waves per gate, k_blind_rotate_w4r (default 2 per CU)"},
    {IEACHE_OPT(two_wave_max, "IEACHE_TWO_WAVE_MAX"), 0, kNoLimit, nullptr, "... up to this size: two waves per gate, k_blind_rotate_w2r (default 5 per CU); one wave per gate above"},
    {IEACHE_OPT(exact_one_wave_min, "IEACHE_EXACT_ONE_WAVE_MIN"), 0, kNoLimit, nullptr, "two-limb launches from this size: one wave per gate, k_blind_rotate_x1 (default 4 per CU + 1)"},
    {IEACHE_OPT(wg_gates, "IEACHE_WG_GATES"), 0, 4, nullptr, "gate instances per workgroup of the one-wave-per-gate kernels; 0 = by launch size"},
    {IEACHE_OPT(wg3_max, "IEACHE_WG3_MAX"), 0, kNoLimit, nullptr, "... by launch size: three up to this many gate instances (default 6 per CU), four above"},
    {IEACHE_OPT(w4r_flip, "IEACHE_W4R_FLIP"), 0, 1 << 30, nullptr, "k_blind_rotate_w4r: workgroups i and i + this are taken to share a CU; 0 = the device's CU count, a huge value = never flip"},
    {IEACHE_OPT(exact_fft, "IEACHE_EXACT_FFT"), 0, 1, nullptr, "hook (0 needs br_one_limb_supported): 1 = the two-limb blind rotation always"},
    {IEACHE_OPT(fft_audit, "IEACHE_FFT_AUDIT"), 0, 1 << 30, nullptr, "every K-th one-limb launch has a sample run again on the two-limb kernel (Evaluator::fft_audit_counts); 0 = off"},
    {IEACHE_OPT(fft_audit_inject, nullptr), 1, 1, nullptr, "test hook: the next audit reports a differing row (reads 1 until it has)"},
    {IEACHE_OPT(fft_guard_inject, nullptr), 1, 1, nullptr, "hook (device write), test hook: the next call finds the rounding guard tripped (reads 1 until it has)"},
    {IEACHE_OPT(overlap, "IEACHE_OVERLAP"), 0, 1, nullptr, "1 = launches go to several streams of the context; 0 = one stream"},
    {IEACHE_OPT(overlap_min, "IEACHE_OVERLAP_MIN"), 2, kNoLimit, nullptr, "levels from this size are issued as two halves on two streams (default 16 per CU)"},
    {IEACHE_OPT(pipe_min, "IEACHE_PIPE_MIN"), 0, kNoLimit, nullptr, "circuits whose mean level holds this many gate instances run as expression pipelines (default 8 per CU)"},
    {IEACHE_OPT(pipe_lanes, "IEACHE_PIPE_LANES"), 2, kMaxLanes, nullptr, "pipelines such an evaluation is cut into"},
    {IEACHE_OPT(pipe_auto, nullptr), 0, 1, nullptr, "1 = between pipe_min / 8 and 2 x pipe_min the mode is chosen by timing the first four evaluations"},
    {IEACHE_OPT(br_mix, "IEACHE_BR_MIX"), 0, 1, nullptr, "1 = launches of 4 .. 7 and 8 .. 10.5 gates per CU run as a rotation of roles (mix_plan.h)"},
    {IEACHE_OPT(mix_s1, nullptr), 1, 630, nullptr, "its steps of a one-wave turn"},
    {IEACHE_OPT(mix_ratio, nullptr), 100, 400, nullptr, "100 x (two-wave steps per one-wave step)"},
    {IEACHE_OPT(mix_sync, nullptr), 0, 1, nullptr, "1 = barriers between its phases"},
    {IEACHE_OPT(mix_wg, nullptr), 1, 4, nullptr, "gate instances per workgroup of its one-wave turns"},
    {IEACHE_OPT(mix_k, nullptr), 0, kMaxLanes, not_1, "a forced number of subsets (measurement aid); 0 = by launch size"},
    {IEACHE_OPT(mix_tw, nullptr), 0, kMaxLanes - 1, nullptr, "... of which this many on two waves at a time"},
    {IEACHE_FIGURE(cus), "compute units of the context's device"},
    {IEACHE_FIGURE(resident_gates), "gate instances the one-wave-per-gate kernels keep resident at once (8 per CU)"},
    {IEACHE_FIGURE(overlapped_levels), "levels issued as halves on two streams so far"},
    {IEACHE_FIGURE(pipelined_evals), "circuit evaluations run as expression pipelines so far"},
    {IEACHE_FIGURE(tuned_evals), "evaluations that were a timed trial of their (circuit, batch) so far (pipe_auto)"},
    {IEACHE_FIGURE(mixed_launches), "(level, piece) launches run as a rotation of roles so far"},
    {IEACHE_FIGURE(staging_allocations), "(re)allocations of the host entry points' staging rows so far"},
};
#undef IEACHE_OPT
#undef IEACHE_FIGURE

inline const OptionRow* find_option(const char* name) {
    for (const OptionRow& r : kOptionTable)
        if (!strcmp(r.name, name)) return &r;
    return nullptr;
}
inline bool option_accepts(const OptionRow& r, int64_t v) { return r.lo <= v && v <= r.hi && (!r.ok || r.ok(v)); }

// Stores `v` if the row accepts it and `hook(row, v)` -- which may normalise v and has the option's other effects -- agrees.
template <class Hook>
bool option_set(EvalOptions& o, const OptionRow& r, int64_t v, Hook&& hook) {
    if (!option_accepts(r, v) || !hook(r, v)) return false;
    o.*r.at = v;
    return true;
}
// The environment pass: a variable that is set is treated as a set_option of its value; one out of range is ignored.
template <class Hook>
void options_from_environment(EvalOptions& o, Hook&& hook) {
    for (const OptionRow& r : kOptionTable)
        if (const char* e = r.env ? getenv(r.env) : nullptr) (void)option_set(o, r, atoll(e), hook);
}

}  // namespace ieache
