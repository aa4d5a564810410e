// Blind rotation (K0-K4), the one door: every kernel, the forms of the bootstrapping key, the twiddle tables, the rounding
// guard's record, the sampled audit and the LDS grants are behind this object; which kernel takes a launch and cut how is
// br_plan.h.  A caller plans a launch (br_plan), hands the plan over with the work and gets extracted samples.
// Kernels: blind_rotate.hip (any parameter set), blind_rotate_w64.hip (N = 1024, the nine 64-lane kernels), blind_rotate_h2.hip
// (N = 2048, one two-limb kernel).
#pragma once
#include "br_plan.h"
#include "device_buffer.h"
#include "device_common.h"

namespace ieache {

// Per-stream scratch of the blind rotation.
struct BrScratch {
    dev::DeviceBuffer<char> state;  // sliced blind rotation: accumulators + rotation amounts, br_state_bytes_per_item() per item
    dev::DeviceBuffer<Torus32> audit_ext;
    dev::DeviceBuffer<Torus32> audit_acc;  // the audit of a multi-output launch: whole accumulators, [kAuditGates][2][N]
    dev::DeviceBuffer<char> audit_state;
};

// What a rotation of roles runs on: plan.mix.k streams of the context (the first: the launch's own) and an event each.  The
// caller owns them; the unit creates no stream.
struct BrLanes {
    hipStream_t streams[kMaxLanes] = {};
    hipEvent_t ev[kMaxLanes] = {};
};

// One share of a launch: `cnt` consecutive rotation items of one descriptor, from W.item0 on.  A launch is a list of parts;
// their items are the launch's items one after another (rows of the state block and of `ext` in that order).  Every call
// but a joint evaluation (joint_plan.h) passes a list of one.
struct BrPart {
    dev::WorkDesc W;
    int64_t cnt;
};

// One per evaluator.  All methods expect the evaluator's device to be current.
struct BlindRotate {
    // The twist and twiddle tables of the any-parameter kernel (K.twist / K.wtab are set to them) and its dynamic LDS on the
    // current device.  Of K the blind rotation reads everything but the key-switch fields.
    // Throws std::invalid_argument for a parameter set whose generic kernel needs more than the LDS of a CU, unless
    // br_h2_supported(): there a launch of the generic kernel ("force_generic") throws it instead.
    void init(const Params& p, dev::DevKeys& K);
    // raw BK [n][2l][2][N] (device) -> every form the kernels read (allocated once): the generic two-limb spectrum and,
    // where br_supported(), the 64-lane kernels' two-limb and one-limb spectra, their twiddle table and the guard record.
    void load_key(const Torus32* d_bk_raw, hipStream_t stream);
    // State for a launch of `need` gate instances ahead of time, so that launch() finds it in place (an allocation is a
    // device-wide synchronisation).
    void reserve(BrScratch& scratch, size_t need, const EvalOptions& opt, bool use_w64);
    // K0..K4 of the gate instances the parts describe -- sum of cnt of them, `plan` made for that sum -- on `stream`.  ext: rows
    // of N + 4 words (may be null); steps < 0: the whole rotation; dbg_acc [sum][2][N] (may be null; then pass ext = null).
    // lanes: plan.mix.k streams and events when the plan is a rotation of roles.  Returns the kernel launches issued (the
    // prologues not counted).
    // 64-lane kernels: only the prologue reads a descriptor, so there is ONE prologue per part, at the part's row offset of
    // the state block, and one sequence of CMux slices over all rows -- the parts SHARE every rotation launch.
    // Any-parameter kernel: its prologue is inside it, so the parts are launched one after another on `stream`, each over its
    // rows of ext.  Same results, nothing shared.
    int launch(BrScratch& scratch, const BrPlan& plan, const EvalOptions& opt, const BrLanes& lanes, hipStream_t stream, const BrPart* parts,
               size_t n_parts, Torus32* ext, int32_t steps, Torus32* dbg_acc);
    // The sampled audit behind the rounding guard: after a (level, chunk) launch that took a one-limb kernel, every
    // fft_audit-th time, kAuditGates consecutive gate instances of it (at an offset that moves from audit to audit) are run
    // again on the two-limb kernel -- exact by construction -- and their extracted samples compared word for word with what the
    // one-limb kernel wrote to `ext`.  A differing row is counted on the device; the call then repeats itself on the
    // two-limb kernels like a call whose guard tripped (Evaluator::fft_guard_tripped).  The guard watches the error LEVEL of
    // every launch; this compares BITS, of a sample.  Clears "fft_audit_inject" when it has used it.
    // One decision per launch, whatever the number of parts.  The window lies inside ONE part (the exact kernel's prologue
    // reads one descriptor); a part shorter than the window is audited whole; which part moves from audit to audit.
    // acc (may be null): the launch's whole accumulators [sum][2][N] where it left them instead of `ext` -- a multi-output
    // call, whose factor products read EVERY word of an accumulator, while an extracted sample holds only polynomial a and
    // coefficient 0 of polynomial b: there the accumulators are what is compared (a wrong word of b elsewhere would be a wrong
    // output the extraction never shows: tests/test_safety_nets_gpu.py).
    void audit(BrScratch& scratch, const BrPlan& plan, EvalOptions& opt, hipStream_t stream, const BrPart* parts, size_t n_parts, const Torus32* ext,
               const Torus32* acc = nullptr);
    static constexpr int64_t kAuditGates = 64;
    struct AuditCounts {
        int64_t seq = 0;  // one-limb (level, chunk) launches so far
        int64_t audits = 0, gates = 0, mismatches = 0;
    } audit_counts;

    // The guard record of the one-limb kernels: [0] launches whose rounding deviation exceeded the limit, [1] max deviation
    // (float bits), [2] audit rows that differed.  Absent (false / nothing happens) until a key for the 64-lane kernels is loaded.
    bool guard_read(unsigned h[3]) const;
    void guard_rearm();   // the two counts only; the maximum stays
    bool guard_inject();  // test hook: the next read finds a launch over the limit

    // What a launch reads of the key, for the transform probe's read-back (Evaluator::debug_spectrum, debug_twiddles): null
    // where load_key has not made it.  generic: [n 2l 2][2 limbs][M] in the radix-2 transform's bit-reversed order;
    // w64: [n 2l 2][2 limbs][8][64]; w64_1: [n 2l 2][8][64]; twiddles: w64::twiddle_table_elems() entries.
    struct KeyForms {
        const double2 *generic, *w64, *w64_1, *twiddles;
    };
    KeyForms key_forms() const { return KeyForms{bkf_, bkf_w64_, bkf1_w64_, tw_w64_}; }

private:
    Params p_;
    dev::DevKeys K_{};
    size_t generic_lds_ = 0;
    dev::DeviceBuffer<double2> twist_, wtab_;
    dev::DeviceBuffer<double2> bkf_;       // generic two-limb spectrum
    dev::DeviceBuffer<double2> bkf_w64_;   // spectrum in the wave-per-gate kernels' layout
    dev::DeviceBuffer<double2> tw_w64_;    // their twiddle table
    dev::DeviceBuffer<double2> bkf1_w64_;  // one-limb spectrum
    dev::DeviceBuffer<double2> bkf_h2_;    // N = 2048: two-limb spectra of the even and odd halves (blind_rotate_h2.h)
    dev::DeviceBuffer<unsigned> guard_;
    dev::DeviceBuffer<unsigned long long> diag_;  // diagnostic builds (br_variant 8 / 49): phase stamps, allocated on first use
};

}  // namespace ieache
