// Device evaluator: level-batched gate bootstrapping on MI355X (gfx950).
//
// Per gate instance (one bootsAND/bootsXOR of the reference, cloud.c:30-43,159):
//   K0 gate pre-combination   t = cst + sa*ca + sb*cb          (boot-gates.cpp)
//   K1 mod-switch             bara_i, barb in [0,2N)            (numeric-functions.cpp)
//   K2 test-vector init       acc = (0, X^{2N-barb} * mu)       (lwe-bootstrapping-functions-fft.cpp)
//   K3 blind rotation         n x  acc += BK_i (x) ((X^bara_i - 1) acc)
//   K4 sample extract
//   K5 key switch                                                 (lwe-keyswitch-functions.cpp)
// K0-K4 are one kernel (k_blind_rotate_*) of the blind-rotation unit (blind_rotate.h), K5 is the key-switch unit (keyswitch.h).
//
// The external product is EXACT.  libtfhe multiplies polynomials with an
// approximate FP64 FFT; here every BK polynomial is split into two balanced
// 16-bit limbs before the transform, so every inverse-transform output is an
// integer of magnitude < 2^37 carried with > 15 spare mantissa bits and
// rounding recovers it exactly.  Results therefore equal the integer
// definition (and the CPU oracle) bit for bit, whatever the FFT schedule.
#include "evaluator.h"

#include <cstring>
#include <initializer_list>

#include "blind_rotate.h"
#include "device_buffer.h"
#include "device_common.h"
#include "evaluator_options.h"
#include "cmux.h"
#include "fft_probe.h"
#include "joint_plan.h"
#include "keyswitch.h"
#include "lwe_linear.h"
#include "multi_extract.h"
#include "pack.h"
#include "scoped_set.h"
#include "set_calls.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <map>
#include <memory>
#include <stdexcept>
#include <tuple>
#include <vector>

namespace ieache {

void hip_check(hipError_t e, const char* what, const char* file, int line) {
    if (e == hipSuccess) return;
    (void)hipGetLastError();  // the runtime keeps a failure as "last error": clear it, or a later, healthy call's
                              // hipGetLastError() check would report this one again
    char buf[512];
    snprintf(buf, sizeof buf, "HIP error %d (%s) at %s:%d: %s", (int)e, hipGetErrorString(e), file, line, what);
    throw std::runtime_error(buf);
}

namespace {

using namespace dev;

// raw KSK rows (n+1) -> padded rows (stride)
__global__ void k_pad_rows(const Torus32* src, Torus32* dst, int64_t rows, int32_t width, int32_t stride) {
    const int64_t total = rows * stride;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / stride;
        const int32_t c = (int32_t)(i - r * stride);
        dst[i] = c < width ? src[r * width + c] : 0;
    }
}

// A circuit level with MUX gates (level_items.h): the rows of extracted samples of one piece, one per ROTATION item, become
// one row per GATE for the key switch -- a two-input gate's row as it is, a MUX gate's as bootsMUX forms it,
// (0, 1/8) + u1 + u2 over its two rotations (boot-gates.cpp), uint32 adds.  A flat MUX call is the level ng = nm = 1.  One workgroup per gate of the piece; pure streaming, rows
// of N + 4 words moved as 16-byte words (N is a multiple of 4, so word N -- the b term -- is lane x of 16-byte word N / 4).
// gate0 / item0: the piece's first gate instance / rotation item; the caller cuts pieces at gate boundaries, so both rows of
// a MUX are inside ext's `cnt` rows.
__global__ __launch_bounds__(256) void k_level_combine(const Torus32* ext, Torus32* dst, int32_t N, int64_t gate0, int64_t item0,
                                                       int32_t ng, int32_t nm) {
    const int64_t q = gate0 + (int64_t)blockIdx.x;
    const int64_t row = level_first_item(q, ng, nm) - item0;
    const bool mux = (int32_t)(q % ng) >= ng - nm;
    const int32_t R = (N + 4) >> 2;
    const int4* u1 = reinterpret_cast<const int4*>(ext) + (size_t)row * R;
    const int4* u2 = u1 + R;
    int4* d = reinterpret_cast<int4*>(dst) + (size_t)blockIdx.x * R;
    for (int32_t v = threadIdx.x; v < R; v += 256) {
        int4 x = u1[v];
        if (mux) {
            const int4 y = u2[v];
            x.x = (int32_t)((uint32_t)x.x + (uint32_t)y.x + (v == (N >> 2) ? (uint32_t)kMU : 0u));
            x.y = (int32_t)((uint32_t)x.y + (uint32_t)y.y);
            x.z = (int32_t)((uint32_t)x.z + (uint32_t)y.z);
            x.w = (int32_t)((uint32_t)x.w + (uint32_t)y.w);
        }
        d[v] = x;
    }
}

// outputs of a circuit: out[b][o] = +-store[b][slot] or the constant
__global__ void k_gather_outputs(const OutRef* outs, int32_t n_out, const Torus32* store, int32_t n_slots,
                                 Torus32* out, int64_t batch, int32_t stride, int32_t n) {
    const int64_t row = blockIdx.x;  // b * n_out + o
    const int64_t b = row / n_out;
    const OutRef r = outs[row % n_out];
    Torus32* dst = out + (size_t)row * stride;
    for (int32_t q = threadIdx.x; q < stride; q += blockDim.x) {
        uint32_t v;
        if (r.slot >= 0)
            v = (uint32_t)store[((size_t)b * n_slots + r.slot) * stride + q];
        else
            v = q == n ? 0xE0000000u : 0u;
        if (r.neg) v = 0u - v;
        dst[q] = q <= n ? (int32_t)v : 0;
    }
}

// The public tables of a replace write of a window (lut_write_coef; project_plan.h: write_coef_amount), once per call: the
// amounts of its two rotations, toward [steps] = 2N - unit 2^t (the read) and back [steps] = unit 2^t (the write), and
// own [count] = 0, 1, .. -- item i writes memory i.
__global__ __launch_bounds__(256) void k_write_coef_tables(int32_t unit, int32_t steps, int32_t two_n, int64_t count, int32_t* __restrict__ toward,
                                                           int32_t* __restrict__ back, int32_t* __restrict__ own) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q < steps) {
        const int32_t w = (int32_t)(((int64_t)unit << q) & (two_n - 1));  // steps <= 30 (write_coef_error)
        back[q] = w;
        toward[q] = (two_n - w) & (two_n - 1);
    }
    if (q < count) own[q] = (int32_t)q;
}

}  // namespace

// ------------------------------------------------------------------------
// One stream's worth of per-launch scratch.  Lane 0 runs on the evaluator's own stream and is all a call uses with
// "overlap" = 0.  Otherwise further lanes -- more streams of the SAME context (one copy of the key), each with its own
// extracted-sample rows, blind-rotation and key-switch scratch -- take either a contiguous share of a
// batch's expressions through every level of a circuit (pipelines: one fork, one join per evaluation) or every other piece
// of a wide level (lane 0 then waits for lane 1 before the next level starts).  See Evaluator::set_option in evaluator.h.
struct Lane {
    Stream stream;                  // lane 0: the evaluator's own
    DeviceBuffer<Torus32> ext;      // extracted samples, rows of N + 4 words
    DeviceBuffer<Torus32> comb;     // levels with MUX gates: one combined row per gate of a piece (k_level_combine).  Per lane, not
                                    // per context: two lanes run their combines and key switches side by side
    BrScratch br;                   // blind rotation: state between slices, the audit's sample
    KsScratch ks;                   // key switch
    MvScratch mv;                   // multi-output programmable bootstrap: a piece's accumulators and its extracted rows
    std::unique_ptr<PackScratch> pack;  // packing key switch: a piece's R rows and digits; there while a packing key is set
    CmuxScratch cmux;               // CMux tree: the two buffers whose roles swap from level to level (empty until a tree runs)
    std::unique_ptr<PackScratch> project;  // projection: a piece's R rows and digits; there while a projection key is set
    DeviceBuffer<Torus32> coef_old;  // replace write of a window: a piece's projected old words, then the differences [items][2][N]
    DeviceBuffer<int32_t> coef_idx;  // ... the two amount arrays [kRotateMaxSteps] each, then own [count] = 0, 1, ..
    Event ev_join;                  // the lane's share of a level / of an evaluation is queued
    Event ev_mix;
};

// Members are released in reverse order; Evaluator::destroy() has every stream idle before that starts.
struct Evaluator::Impl {
    Lane lane[kMaxLanes];
    Event ev_fork;
    EvalOptions opt;  // evaluator_options.h: everything set_option / get_option name
    // per-call state (begin_call, ScopedSet)
    bool use_w64 = false;
    bool force_generic_ks = false;
    bool exact_once = false;          // set while a call is repeated after a guard trip
    int32_t concurrency = 1;          // streams issuing launches side by side right now (kernel choice is by cnt x concurrency)
    bool level_on_two_lanes = false;  // set while a level's halves are being queued on two streams (no rotation of roles then)
    // "pipe_auto": the first four evaluations of a (circuit, batch) in the band where neither stream mode wins everywhere
    // alternate -- without pipelines, with, without, with -- and later ones take whichever mode had the faster evaluation
    struct Tuned {
        double ms[2] = {-1.0, -1.0};  // best wall time of an evaluation without / with pipelines
        int n[2] = {0, 0};            // trials so far (two each, alternating: a first call also pays for allocations)
    };
    std::map<std::tuple<size_t, int32_t, size_t, size_t, bool>, Tuned> tuned;  // (gates, levels, outputs, batch, exact_fft)
    DeviceBuffer<Torus32> stage[kStageSlots];  // rows the host-buffer entry points stage operands and results in (counted in bytes)
    DevKeys K{};
    BlindRotate br;  // K0-K4: kernels, key forms, guard record, audit and LDS grants; the choice among the kernels is br_plan.h
    double guard_max = 0;        // largest rounding deviation seen by the one-limb kernel (of 0.5)
    int64_t guard_reruns = 0;    // calls repeated on the two-limb kernel
    DeviceBuffer<int32_t> ksk;
    KeySwitch ks;  // K5: kernels, key form, LDS grants and the choice among them
    Pack pack;  // the packing key switch (LWE rows -> TLWE samples): kernels, key form and the cut of a call (pack_plan.h)
    Pack project;  // the same unit on project_params(): the projection key (TLWE sample -> the window of its coefficients, section 3l)
    Cmux cmux;  // CMux on caller TGSW samples, its tree and the extraction of a coefficient: kernels, twiddles, the cut (cmux_plan.h)
    LweLinear linear;  // linear layers on encrypted rows: kernels and the prepared weights (linear_plan.h states the calls)
    MultiExtract mv;  // between K3 and K5 of a multi-output programmable bootstrap: the factors' lists and the extraction by factor
    DeviceBuffer<Torus32> store;    // circuits: the wire store, the gate and the output table
    DeviceBuffer<DevGate> d_gates;
    DeviceBuffer<OutRef> d_outs;
    // a joint evaluation (eval_jobs_device): the same three per job, slot i for the call's i-th job with a batch -- jobs have
    // disjoint stores
    struct JobStore {
        DeviceBuffer<Torus32> store;
        DeviceBuffer<DevGate> d_gates;
        DeviceBuffer<OutRef> d_outs;
    };
    std::vector<std::unique_ptr<JobStore>> job_store;
    size_t ext_row_bytes() const { return (size_t)(K.N + 4) * 4; }
};

Evaluator::Evaluator(const Params& p, int device) : p_(p), device_(device), d_(new Impl) {
    try {
        init();
    } catch (...) {
        destroy();  // the destructor does not run for a half-built object
        throw;
    }
}

void Evaluator::init() {
    const Params& p = p_;
    const int device = device_;
    if (!p.supported()) throw std::invalid_argument("unsupported TFHE parameter set");
    int count = 0;
    HIP_CHECK(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) throw std::runtime_error("no such HIP device");
    HIP_CHECK(hipSetDevice(device));
    d_->lane[0].stream.ensure();
    stream_ = d_->lane[0].stream;
    {
        int cus = 0;
        HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
        EvalOptions& o = d_->opt;
        o.cus = cus;
        o.br_wide_max = cus;  // one workgroup of the wide kernel fills a CU
        o.overlap_min = 16 * (int64_t)cus;  // each half of a level is then a full round of resident gates
        o.pipe_min = 8 * (int64_t)cus;      // measured: 11 per CU +2.9 %, 4 per CU -10 %, profiles/r5_overlap_ab.txt
        o.wg3_max = 6 * (int64_t)cus;
        // k_blind_rotate_w1: one wave per gate, 256 VGPRs -> 2 per SIMD = 8 gates per CU
        // ("exact_fft": k_blind_rotate_x1 holds 8 gates per CU too; k_blind_rotate_w2, 2 waves per gate and 35.8 KB of LDS, 4 per CU)
        o.resident_gates = 8 * cus;
        o.one_limb_min = cus + 1;  // everything the latency kernel does not take
        o.four_wave_max = 2 * cus;
        o.two_wave_max = 5 * cus;  // measured crossover with one wave per gate: 1 216 gates 8.6 against 10.0 ms, 1 400 gates 10.8 against 10.1
        o.exact_one_wave_min = 4 * cus + 1;  // two-limb launches that do not fit the two-waves-per-gate kernel's 4 gates per CU
        if (!br_one_limb_supported(p)) o.exact_fft = 1;
        options_from_environment(o, [this](const OptionRow& r, int64_t& v) { return option_hook(r, v); });
    }
    DevKeys& K = d_->K;
    K.n = p.n;
    K.N = p.N;
    K.M = p.N / 2;
    K.logM = 0;
    while ((1 << K.logM) < K.M) K.logM++;
    K.l = p.l;
    K.Bgbit = p.Bgbit;
    K.kpl = p.kpl();
    K.ks_t = p.ks_t;
    K.ks_basebit = p.ks_basebit;
    K.ks_base = p.ks_base();
    K.stride = p.lwe_stride();
    K.dec_offset = 0;
    for (int32_t i = 1; i <= p.l; i++) K.dec_offset += (1u << (p.Bgbit - 1)) << (32 - i * p.Bgbit);
    d_->br.init(p, K);
    d_->ks.init(p, K);
    d_->mv.init(p);
    d_->pack.init(p);
    d_->project.init(project_params(p));
    d_->linear.init(p);
    d_->cmux.init(p, device_, &d_->opt.cmux_gadget_runtime);
}

Evaluator::~Evaluator() { destroy(); }

// Every stream idle, then Impl's members release what they own.
void Evaluator::destroy() {
    if (!d_) return;
    (void)hipSetDevice(device_);
    for (int k = kMaxLanes - 1; k >= 0; k--)
        if (d_->lane[k].stream) (void)hipStreamSynchronize(d_->lane[k].stream);
    delete d_;
    d_ = nullptr;
    stream_ = nullptr;
}

void Evaluator::wait_for_stream(hipStream_t producer) {
    HIP_CHECK(hipSetDevice(device_));
    hipEvent_t ev;
    HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, producer);
    if (e == hipSuccess) e = hipStreamWaitEvent(stream_, ev, 0);
    (void)hipEventDestroy(ev);
    HIP_CHECK(e);
}

// Staging rows for the host-buffer entry points (StageSlot in evaluator.h).  A slot grows to at least `bytes`
// (doubling, so a run of growing batches does not reallocate every call) and is zeroed when it is (re)allocated: callers
// upload n + 1 words per row of lwe_stride() and rely on the padding words of OPERAND rows being zero, which holds because
// nothing but such uploads ever writes the operand slots.  Every hipMalloc / hipFree is a device-wide synchronisation, which
// is why a warm daemon request must not make one.
Torus32* Evaluator::staging(StageSlot slot, size_t bytes) {
    if (slot < 0 || slot >= kStageSlots) throw std::invalid_argument("staging slot");
    HIP_CHECK(hipSetDevice(device_));
    bytes = (bytes + 255) & ~(size_t)255;
    DeviceBuffer<Torus32>& st = d_->stage[slot];
    if (st.items() < bytes || !st) {
        st.allocate(std::max(bytes, std::min<size_t>(2 * st.items(), (size_t)1 << 30)), 1, /*slack=*/16, /*zero=*/true);
        d_->opt.staging_allocations++;
    }
    return st;
}

int Evaluator::resident_gates() const { return (int)d_->opt.resident_gates; }
int Evaluator::resident_gates_two_wave() const { return d_->opt.exact_fft ? 0 : 4 * (int)d_->opt.cus; }
void Evaluator::set_force_generic(bool v) { d_->opt.force_generic = v; }
void Evaluator::set_chunk(size_t items) { d_->opt.chunk = items < 1 ? 1 : (int64_t)items; }

// What a row of the option table cannot say: conditions that need the parameter set or the device, and effects beyond
// storing the value.
bool Evaluator::option_hook(const OptionRow& r, int64_t& v) {
    if (r.at == &EvalOptions::force_generic) v = v != 0;
    if (r.at == &EvalOptions::ks_mfma_split) return v == 0 || ks_mfma_split_ok(p_, (int32_t)v);  // every split holds whole loop trips
    if (r.at == &EvalOptions::pack_split) return v == 0 || (d_->pack.has_key() && pack_split_ok(pack_k_steps(p_, d_->pack.t()), (int32_t)v));
    if (r.at == &EvalOptions::project_split)
        return v == 0 || (d_->project.has_key() && pack_split_ok(pack_k_steps(project_params(p_), d_->project.t()), (int32_t)v));
    if (r.at == &EvalOptions::br_variant && !variant_known((int32_t)v)) {
        // a retired number (an old A/B script): say so rather than measure another kernel under the wrong label
        fprintf(stderr, "ieache: br_variant %d names no kernel of this build (csrc/br_plan.h); the choice of kernels stays as it is\n", (int)v);
        return false;
    }
    if (r.at == &EvalOptions::exact_fft) return v == 1 || br_one_limb_supported(p_);
    if (r.at == &EvalOptions::fft_guard_inject) {
        HIP_CHECK(hipSetDevice(device_));
        return d_->br.guard_inject();
    }
    return true;
}

bool Evaluator::set_option(const std::string& name, int64_t value) {
    const OptionRow* r = find_option(name.c_str());
    if (!r || !option_set(d_->opt, *r, value, [this](const OptionRow& row, int64_t& v) { return option_hook(row, v); })) return false;
    d_->tuned.clear();  // whatever was timed was timed under the old options
    return true;
}

bool Evaluator::get_option(const std::string& name, int64_t* value) const {
    const OptionRow* r = find_option(name.c_str());
    if (!r) return false;
    if (value) *value = d_->opt.*r->at;
    return true;
}

std::string Evaluator::kernel_variant() const {
    if (br_h2_supported(p_) && !d_->opt.force_generic) return "h2x64-radix8-twolimb";  // N = 2048: two products on the half ring per step
    if (!br_supported(p_) || d_->opt.force_generic) return "generic-radix2";
    // the kernel wide launches take: one wave per gate, on the one-limb spectrum or ("exact_fft") on the two-limb one
    return d_->opt.exact_fft ? "x1x64-radix8-twolimb" : "w1x64-radix8-onelimb";
}

void Evaluator::load_keys_host(const Torus32* bk, const Torus32* ksk) {
    HIP_CHECK(hipSetDevice(device_));
    DeviceBuffer<Torus32> d_bk, d_ksk;
    d_bk.allocate(p_.bk_count());
    d_ksk.allocate(p_.ksk_count());
    HIP_CHECK(hipMemcpy(d_bk, bk, p_.bk_count() * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_ksk, ksk, p_.ksk_count() * 4, hipMemcpyHostToDevice));
    load_keys_device(d_bk, d_ksk);
}

void Evaluator::load_keys_device(const Torus32* d_bk, const Torus32* d_ksk) {
    HIP_CHECK(hipSetDevice(device_));
    DevKeys& K = d_->K;
    const size_t ks_rows = (size_t)p_.k * p_.N * p_.ks_t * K.ks_base;
    if (!d_->ksk) {
        // 16 rows of slack: the sliced key switch prefetches four positions past the end of its walk
        d_->ksk.allocate((ks_rows + 16) * K.stride);
        HIP_CHECK(hipMemsetAsync(d_->ksk + ks_rows * K.stride, 0, (size_t)16 * K.stride * 4, stream_));
    }
    K.ksk = d_->ksk;
    d_->br.load_key(d_bk, stream_);
    hipLaunchKernelGGL(k_pad_rows, dim3(2048), dim3(256), 0, stream_, d_ksk, d_->ksk, (int64_t)ks_rows, p_.n + 1,
                       K.stride);
    HIP_CHECK(hipGetLastError());
    d_->ks.load_key(d_->ksk, stream_);
    HIP_CHECK(hipStreamSynchronize(stream_));
    keys_loaded_ = true;
}

namespace {
struct Timer {
    std::vector<hipEvent_t> ev;  // pairs
    bool on;
    hipStream_t s;
    Timer(bool enabled, hipStream_t st) : on(enabled), s(st) {}
    ~Timer() {
        for (auto e : ev) (void)hipEventDestroy(e);
    }
    void mark() { mark(s); }
    // a pair of marks brackets launches on ONE stream; pairs may come from different streams (overlapped levels)
    void mark(hipStream_t on_stream) {
        if (!on) return;
        hipEvent_t e;
        HIP_CHECK(hipEventCreate(&e));
        HIP_CHECK(hipEventRecord(e, on_stream));
        ev.push_back(e);
    }
    // Time during which at least one bracketed interval was open.  On one stream the intervals follow each other and this
    // is their sum; intervals of two streams (overlapped levels) run side by side and are merged on the common device
    // timeline (offsets from the first event), so the figure stays "time the chip spent in these launches".
    double sum_ms() {
        std::vector<std::pair<double, double>> iv;
        for (size_t i = 0; i + 1 < ev.size(); i += 2) {
            float t0 = 0, dt = 0;
            if (i) HIP_CHECK(hipEventElapsedTime(&t0, ev[0], ev[i]));
            HIP_CHECK(hipEventElapsedTime(&dt, ev[i], ev[i + 1]));
            iv.emplace_back((double)t0, (double)t0 + (double)dt);
        }
        std::sort(iv.begin(), iv.end());
        double tot = 0, lo = 0, hi = -1;
        for (const auto& x : iv) {
            if (hi < lo || x.first > hi) {
                if (hi >= lo) tot += hi - lo;
                lo = x.first;
                hi = x.second;
            } else if (x.second > hi) {
                hi = x.second;
            }
        }
        if (hi >= lo) tot += hi - lo;
        return tot;
    }
};
// the three timers of a call, folded into its statistics once the stream is idle
void add_times(EvalStats* stats, Timer& tall, Timer& tbr, Timer& tks) {
    if (!stats) return;
    stats->total_ms += tall.sum_ms();
    stats->blind_rotate_ms += tbr.sum_ms();
    stats->keyswitch_ms += tks.sum_ms();
}

// One piece of a levelled call as its body sees it (Evaluator::run_pieces): items [first, first + count) of the call, and
// the two kinds of phase a body runs on the evaluator's stream, in any order and any number of times.  A phase that never
// runs records no event, so its time and its launches stay 0.
struct Piece {
    int64_t first, count;
    // a rotation-side phase: fn() launches and returns how many kernels it did ("blind_rotate_launches", timed as blind_rotate_ms)
    template <class F>
    void rotate(F&& fn) {
        tbr.mark();
        const int launches = fn();
        tbr.mark();
        HIP_CHECK(hipGetLastError());
        if (stats) stats->blind_rotate_launches += launches;
    }
    // a key-switch-side phase over `rows` rows in runs of at most run_rows: fn(rows done, rows of the run), one
    // "keyswitch_launches" each, timed as keyswitch_ms
    template <class F>
    void keyswitch(int64_t rows, int64_t run_rows, F&& fn) {
        const Cut runs = cut_in_runs(rows, run_rows);
        for (int64_t r = 0; r < runs.pieces; r++) {
            tks.mark();
            fn(piece_first(runs, r), piece_count(runs, rows, r));
            tks.mark();
            HIP_CHECK(hipGetLastError());
            if (stats) stats->keyswitch_launches++;
        }
    }
    Timer &tbr, &tks;
    EvalStats* stats;
};
}  // namespace

// streams and join events of lanes 1 .. lanes-1, and the fork event
static void ensure_lanes(Evaluator::Impl* d, int lanes) {
    d->ev_fork.ensure();
    for (int k = 1; k < lanes; k++) {
        d->lane[k].stream.ensure();
        d->lane[k].ev_join.ensure();
    }
}
// Fork: lanes 1 .. lanes-1 start when everything queued so far on lane 0 is done (lanes < 2: nothing happens, here or
// later); join(): lane 0 waits for all of them.  A Fork that goes without having been joined -- an exception is on its way
// out -- waits on the host for the lanes it forked, so that nothing of the failed call is still queued on them, writing the
// wire store or their scratch, when the caller goes on using the context.
struct Fork {
    Evaluator::Impl* d;
    int lanes;
    bool joined = false;
    Fork(Evaluator::Impl* d_, int lanes_) : d(d_), lanes(lanes_) {
        if (lanes < 2) return;
        HIP_CHECK(hipEventRecord(d->ev_fork, d->lane[0].stream));
        for (int k = 1; k < lanes; k++) HIP_CHECK(hipStreamWaitEvent(d->lane[k].stream, d->ev_fork, 0));
    }
    Fork(const Fork&) = delete;
    Fork& operator=(const Fork&) = delete;
    void join() {
        for (int k = 1; k < lanes; k++) {
            HIP_CHECK(hipEventRecord(d->lane[k].ev_join, d->lane[k].stream));
            HIP_CHECK(hipStreamWaitEvent(d->lane[0].stream, d->lane[k].ev_join, 0));
        }
        joined = true;
    }
    ~Fork() {
        for (int k = 1; k < lanes && !joined; k++) (void)hipStreamSynchronize(d->lane[k].stream);
    }
};

// The plan of a launch of `cnt` gate instances on lane `ln` under the call's state as it is now (br_plan.h).
static BrPlan plan_blind_rotate(const Params& p, const Evaluator::Impl* d, const Lane& ln, int64_t cnt, int32_t steps = -1) {
    return br_plan(p, d->opt, BrCall{d->exact_once, d->concurrency, d->level_on_two_lanes, steps < 0, &ln == &d->lane[0]}, d->use_w64, cnt);
}

// By the options as they are now, like begin_call(): a context that has made no call yet names the kernels its first call takes.
std::string Evaluator::kernel_for_launch(int64_t gates) const {
    const bool use_w64 = br_supported(p_) && !d_->opt.force_generic;
    return br_kernel_label(p_, br_plan(p_, d_->opt, BrCall{d_->exact_once, d_->concurrency, d_->level_on_two_lanes, true, true}, use_w64, gates < 1 ? 1 : gates));
}

// Runs the gate instances the parts describe as `plan` says.  A rotation of roles gets the context's first plan.mix.k
// lanes: their streams and an event each.
static int launch_blind_rotate(Evaluator::Impl* d, Lane& ln, const BrPlan& plan, const BrPart* parts, size_t n_parts, Torus32* ext, int32_t steps,
                               Torus32* dbg_acc) {
    BrLanes lanes;
    if (plan.mix.k) {
        ensure_lanes(d, plan.mix.k);
        for (int j = 0; j < plan.mix.k; j++) {
            d->lane[j].ev_mix.ensure();
            lanes.streams[j] = d->lane[j].stream;
            lanes.ev[j] = d->lane[j].ev_mix;
        }
        d->opt.mixed_launches++;
    }
    return d->br.launch(ln.br, plan, d->opt, lanes, ln.stream, parts, n_parts, ext, steps, dbg_acc);
}

// the key switch of `cnt` extracted samples on a lane's stream, with the lane's scratch
static void launch_keyswitch(Evaluator::Impl* d, Lane& ln, const WorkDesc& w, int64_t cnt, const Torus32* ext, Torus32* flat_out) {
    d->ks.launch(ln.ks, ln.stream, w, cnt, ext, flat_out, d->opt, d->force_generic_ks);
}

// How a level of `items` gate instances is issued: on lane 0 in pieces of at most a chunk, or (overlap) in pieces of at most
// half the level that alternate between the two lanes.
struct LevelPlan {
    bool two_lanes;
    int64_t piece;  // gate instances per (blind rotation, key switch) pair of launches at most
};
static LevelPlan plan_level(const Evaluator::Impl* d, int64_t items) {
    // joint_plan.h states the rule (halves of whole workgroups of the one-wave-per-gate kernels; two lanes only when there
    // are two pieces to give them: up to 4 items the rounded half is the whole level, and a fork would then use a second
    // stream nobody has created -- reserve_scratch sees nothing to reserve for it)
    const JointLevelPlan jp = joint_level_plan(items, (int64_t)d->opt.chunk, d->opt.overlap && d->use_w64 && d->concurrency == 1, d->opt.overlap_min);
    return LevelPlan{jp.two_lanes, jp.piece};
}

// need: rotation items of the lane's widest piece; need_comb: gates of its widest piece of a level with MUX gates (0 = none)
static void reserve_lane(const Params& p, Evaluator::Impl* d, Lane& ln, size_t need, size_t need_comb = 0) {
    ln.comb.reserve(need_comb, (size_t)d->opt.chunk, d->ext_row_bytes());
    ln.ext.reserve(need, (size_t)d->opt.chunk, d->ext_row_bytes());
    d->br.reserve(ln.br, need, d->opt, d->use_w64);
    d->ks.reserve(ln.ks, (int64_t)need, d->opt, d->force_generic_ks);  // for the widest launch
}

// Before an evaluation starts: scratch for its widest launch in one go (the per-launch checks below then find it in place),
// so that a circuit whose levels widen does not reallocate -- and synchronise -- between them.  level_items: gate instances
// of each level the evaluation will issue.
// level_gates (may be null: no level has MUX gates): gate instances of each level -- fewer than its rotation items where it
// has MUX gates.  A piece of such a level may end one item past the planned size (level_items.h: level_piece_items) and needs
// combined rows, one per gate: at most as many as it has items, and never more than the level has gates.
static void reserve_scratch(const Params& p, Evaluator::Impl* d, const int64_t* level_items, size_t n_levels,
                            const int64_t* level_gates = nullptr) {
    size_t need0 = 1, need1 = 0, comb0 = 0, comb1 = 0;
    for (size_t i = 0; i < n_levels; i++) {
        const int64_t items = std::max<int64_t>(level_items[i], 1);
        const bool mux = level_gates && level_gates[i] < level_items[i];
        const LevelPlan pl = plan_level(d, items);
        const size_t piece = (size_t)std::min<int64_t>(pl.piece + (mux ? 1 : 0), items);
        need0 = std::max(need0, piece);
        if (mux) comb0 = std::max(comb0, std::min<size_t>(piece, (size_t)level_gates[i]));
        if (pl.two_lanes) {
            const size_t rest = std::min<size_t>(piece, (size_t)(items - pl.piece));
            need1 = std::max(need1, rest);
            if (mux) comb1 = std::max(comb1, std::min<size_t>(rest, (size_t)level_gates[i]));
        }
    }
    reserve_lane(p, d, d->lane[0], need0, comb0);
    if (need1) {
        ensure_lanes(d, 2);
        reserve_lane(p, d, d->lane[1], need1, comb1);
    }
}

// What follows a piece's blind rotation, and on which lanes the pieces of a level run: the one statement of run_items' mode.
struct After {
    // -1: as plan_level says -- lane 0 in pieces of a chunk, or the level's halves alternating between two lanes; k >= 0: the
    // whole level on lane k in pieces of at most a chunk, no fork / join (a pipeline of its own, see eval_circuit_device_once,
    // or a flat MUX on lane 0)
    int lane = -1;
    // The stage between a piece's rotation and its output rows:
    //   kMuxCombine: k_level_combine turns the piece's rows, one per ROTATION item, into one per GATE in the lane's `comb`; the
    //     level's (ng, nm) come from the descriptor, a flat MUX call (flat_type == kFlatMux) is the level ng = nm = 1;
    //   kMultiExtract (flat calls, planned lanes): a multi-output programmable bootstrap -- the rotation leaves its whole
    //     accumulators in the lane's scratch (what the audit compares: the factors read every word of them), k_mv_extract turns
    //     them into the lane's ordinary `ext` rows and n_factors rows per item: output row = item x n_factors + factor.  Pieces are max(1, chunk / n_factors) items at
    //     most, so the key switch and the rows stay within what `chunk` bounds (n_factors > chunk: one item, n_factors rows).
    //   kAccumulator (flat calls, planned lanes, rows_out set): the rotation's whole accumulators ARE the result -- each piece
    //     hands its accumulators, [2][N] per item, to rows_out at the piece's first row (rows of 2N words) once its last
    //     slice -- after a rotation of roles has joined its subsets -- is behind it; no extraction, no key switch, and the
    //     audit compares whole accumulators there.
    enum Stage { kNone, kMuxCombine, kMultiExtract, kAccumulator } stage = kNone;
    int32_t n_factors = 1;          // kMultiExtract
    const Torus32* bias = nullptr;  // kMultiExtract: device, [n_factors], or null
    // Where the rows go: null -- through the key switch to where the descriptor puts them; else (flat calls, not after
    // kMuxCombine) the extracted samples are the result -- rows of N + 4 words written there, at the piece's first row, and no
    // key switch follows.  kAccumulator: rows of 2N words instead.
    Torus32* rows_out = nullptr;
};

// Scratch of a multi-output call before its loop starts: per lane the piece's extracted samples and blind-rotation state, its
// accumulators, its n_factors rows per item (not when they go straight to the caller) and a key switch over those rows.
static void reserve_multi(const Params& p, Evaluator::Impl* d, const LevelPlan& pl, int64_t items, int32_t n_factors, bool rows_to_caller) {
    const size_t piece = (size_t)std::min<int64_t>(pl.piece, std::max<int64_t>(items, 1));
    const size_t rows = piece * (size_t)n_factors, cap = (size_t)d->opt.chunk;
    if (pl.two_lanes) ensure_lanes(d, 2);
    for (int k = 0; k < (pl.two_lanes ? 2 : 1); k++) {
        Lane& ln = d->lane[k];
        reserve_lane(p, d, ln, piece);
        d->mv.reserve(ln.mv, piece, rows_to_caller ? 0 : rows, cap, std::max(cap, (size_t)n_factors));
        if (!rows_to_caller) d->ks.reserve(ln.ks, (int64_t)rows, d->opt, d->force_generic_ks);
    }
}

// The key switch's descriptor over ROWS of a flat call: row item0 + i -> row item0 + i of w.flat_out (only GateInst::out is
// used by the key switch).  What the multi-output call and the flat MUX hand it: a flat-MUX descriptor must not reach the
// key switch, resolve() gives it no output row.
static WorkDesc rows_desc(const WorkDesc& w, int64_t item0) {
    WorkDesc wk{};
    wk.flat_a = w.flat_a;
    wk.flat_out = w.flat_out;
    wk.flat_type = -1;
    wk.item0 = item0;
    return wk;
}

// One level: `items` independent rotation items described by W (item0 is advanced per piece), followed by what `after` says.
// Everything queued so far on lane 0 (the previous level) is complete before any piece starts; lane 0 has every piece behind
// it when this returns.  The scratch of a level on a fixed lane may have been reserved by the caller; it is checked here.
static void run_items(const Params& p, Evaluator::Impl* d, WorkDesc W, int64_t items, Timer& tbr, Timer& tks, EvalStats* stats,
                      const After& after = After{}) {
    // A level with MUX gates: `items` are rotation items, two per MUX.  PIECES ARE CUT AT GATE BOUNDARIES (level_piece_items),
    // so both rotations of a MUX are in the same piece, on the same lane, in the same `ext`, before its combine runs.  That
    // one rule covers every way a level is cut:
    //   * "chunk", odd values included: a piece that would end between a MUX's two items takes the second one as well;
    //   * level halves on two lanes (plan_level): the halves are pieces like any other, each lane combines its own;
    //   * expression-half pipelines (a fixed lane): a pipeline's share starts and ends at an expression, which is a gate boundary;
    //   * a flat MUX call: every gate is a MUX, so its pieces are planned in whole gates -- max(chunk & ~1, 2) items -- and the
    //     rule has nothing to add;
    //   * the rotation of roles cuts a launch into subsets INSIDE launch_blind_rotate, and its last act is to make the lane's
    //     stream wait for every subset's stream (launch_mixed_phases' join) before the final slices write `ext` there: what is
    //     queued on the lane's stream afterwards -- audit, combine, key switch -- sees the whole piece.
    // The mode, decided here once for every piece:
    const bool mux = after.stage == After::kMuxCombine, mv = after.stage == After::kMultiExtract, accs = after.stage == After::kAccumulator;
    if (accs && !after.rows_out) throw std::logic_error("accumulator output without rows to put it in");
    const bool flat_mux = mux && !W.gates, to_caller = after.rows_out != nullptr;
    const int32_t ng = flat_mux ? 1 : W.ng, nm = flat_mux ? 1 : W.nm;  // read only where mux
    const int64_t nf = mv ? after.n_factors : 1;                       // output rows per item
    const int64_t gates = mux ? items / (ng + nm) * ng : items;        // gate instances of the level
    const size_t row_words = (size_t)(d->K.N + 4);
    const int64_t chunk = (int64_t)d->opt.chunk;
    LevelPlan pl = plan_level(d, items);
    if (after.lane >= 0) pl = LevelPlan{false, flat_mux ? std::max<int64_t>(chunk & ~(int64_t)1, 2) : chunk};
    if (mv) {
        pl.piece = std::min<int64_t>(pl.piece, std::max<int64_t>(1, chunk / nf));
        reserve_multi(p, d, pl, items, after.n_factors, to_caller);
    } else if (after.lane >= 0) {
        const size_t need = (size_t)std::min<int64_t>(pl.piece + (mux ? 1 : 0), std::max<int64_t>(items, 1));
        reserve_lane(p, d, d->lane[after.lane], need, mux ? std::min<size_t>(need, (size_t)gates) : 0);
    } else {
        reserve_scratch(p, d, &items, 1, mux ? &gates : nullptr);
    }
    Fork fork(d, pl.two_lanes ? 2 : 1);
    if (pl.two_lanes) d->opt.overlapped_levels++;
    ScopedSet<bool> halves(d->level_on_two_lanes, pl.two_lanes);
    int k = 0;
    for (int64_t done = 0, cnt = 0; done < items; done += cnt, k++) {
        cnt = mux ? level_piece_items(W.item0 + done, pl.piece, items - done, ng, nm) : std::min<int64_t>(pl.piece, items - done);
        Lane& ln = d->lane[after.lane >= 0 ? after.lane : (pl.two_lanes ? (k & 1) : 0)];
        WorkDesc w = W;
        w.item0 = W.item0 + done;
        if ((size_t)cnt > ln.ext.items()) throw std::logic_error("piece larger than the lane's extracted-sample rows");
        if (mv && ((size_t)cnt > ln.mv.acc.items() || (!to_caller && (size_t)(cnt * nf) > ln.mv.rows.items())))
            throw std::logic_error("piece larger than the lane's multi-output scratch");
        const BrPlan plan = plan_blind_rotate(p, d, ln, cnt);  // once: the launch and the audit see the same choice
        // ext: the rotation's extracted samples, one row per item; rows: what the stage after it leaves for the output
        Torus32* ext = accs ? nullptr : to_caller && !mv ? after.rows_out + (size_t)done * row_words : (Torus32*)ln.ext;
        // whole accumulators the rotation leaves: a multi-output piece's in the lane's scratch, or the caller's rows
        Torus32* acc = mv ? (Torus32*)ln.mv.acc : accs ? after.rows_out + (size_t)done * 2 * (size_t)d->K.N : nullptr;
        Torus32* rows = mux ? (Torus32*)ln.comb : !mv ? ext : to_caller ? after.rows_out + (size_t)(done * nf) * row_words : (Torus32*)ln.mv.rows;
        tbr.mark(ln.stream);
        const BrPart part{w, cnt};
        const int nbr = launch_blind_rotate(d, ln, plan, &part, 1, acc ? nullptr : ext, -1, acc);
        tbr.mark(ln.stream);
        HIP_CHECK(hipGetLastError());
        if (mv) d->mv.extract(ln.stream, ln.mv.acc, cnt, after.n_factors, after.bias, ext, rows);
        d->br.audit(ln.br, plan, d->opt, ln.stream, &part, 1, ext, acc);
        if (!to_caller) {
            tks.mark(ln.stream);
            WorkDesc wk = w;
            int64_t n_rows = cnt;
            if (mux) {
                // one row per gate, then the key switch over GATES: a level's own descriptor read with nm = 0 and item0 in gate
                // instances, for which resolve() is the identity the key-switch kernels have always used to find out_slot
                if (!level_gate_boundary(w.item0, ng, nm) || !level_gate_boundary(w.item0 + cnt, ng, nm))
                    throw std::logic_error("piece of a level cut inside a MUX gate");
                const int64_t gate0 = level_gates_before(w.item0, ng, nm);
                n_rows = level_gates_before(w.item0 + cnt, ng, nm) - gate0;
                if ((size_t)n_rows > ln.comb.items() || (d->K.N & 3)) throw std::logic_error("combined rows of a MUX level not reserved");
                hipLaunchKernelGGL(k_level_combine, dim3((unsigned)n_rows), dim3(256), 0, ln.stream, ext, rows, d->K.N, gate0, w.item0, ng, nm);
                if (flat_mux) {
                    wk = rows_desc(w, gate0);
                } else {
                    wk.nm = 0;
                    wk.item0 = gate0;
                }
            } else if (mv) {
                n_rows = cnt * nf;
                wk = rows_desc(w, w.item0 * nf);
            }
            launch_keyswitch(d, ln, wk, n_rows, rows, nullptr);
            tks.mark(ln.stream);
            HIP_CHECK(hipGetLastError());
        }
        if (stats) {
            stats->blind_rotate_launches += nbr;
            stats->keyswitch_launches += to_caller ? 0 : 1;
            stats->chunks++;
        }
    }
    fork.join();
    if (stats) stats->bootstraps += items;
}

// After a synchronous call: fold the one-limb kernel's guard record into the context and tell whether the call has to be
// repeated on the two-limb kernel (some launch saw a coefficient further than kGuardLimit from an integer).
bool Evaluator::fft_guard_tripped() {
    unsigned h[3] = {0, 0, 0};
    if (!d_->br.guard_read(h)) return false;
    float m;
    memcpy(&m, &h[1], sizeof m);
    if ((double)m > d_->guard_max) d_->guard_max = (double)m;
    if (h[0] == 0 && h[2] == 0) return false;
    d_->br.audit_counts.mismatches += h[2];
    d_->opt.fft_guard_inject = 0;
    d_->br.guard_rearm();
    return true;
}

void Evaluator::fft_audit_counts(int64_t* audits, int64_t* gates, int64_t* mismatches) const {
    if (audits) *audits = d_->br.audit_counts.audits;
    if (gates) *gates = d_->br.audit_counts.gates;
    if (mismatches) *mismatches = d_->br.audit_counts.mismatches;
}

double Evaluator::fft_guard_max() const { return d_->guard_max; }
int64_t Evaluator::fft_guard_reruns() const { return d_->guard_reruns; }

namespace {
// a device range of an entry point's argument, in words
struct Range {
    const void* p;
    size_t words;
};
// whether the output range shares a word with any of the input ranges (a null pointer is no range)
bool overlaps(const Torus32* out, size_t n_out, std::initializer_list<Range> inputs) {
    for (const Range& r : inputs) {
        const Torus32* in = static_cast<const Torus32*>(r.p);
        if (out && in && out < in + r.words && in < out + n_out) return true;
    }
    return false;
}
}  // namespace

// Repeats `once` on the two-limb kernels when the guard tripped or an audited row differed; the first attempt's time stays
// in the stats, its counts do not.  A call whose output overlaps its inputs cannot be repeated (the first attempt has
// overwritten them), so it runs on the two-limb kernels -- exact by construction -- from the start.
template <class F>
void Evaluator::run_guarded(bool inputs_intact, EvalStats* stats, F&& once) {
    if (!inputs_intact && !d_->exact_once) {
        {
            ScopedSet<bool> exact(d_->exact_once, true);
            once();
        }
        (void)fft_guard_tripped();  // folds the record of earlier calls; nothing this call did can trip it
        return;
    }
    const EvalStats before = stats ? *stats : EvalStats{};
    once();
    if (!fft_guard_tripped()) return;
    d_->guard_reruns++;
    EvalStats first{};
    if (stats) {
        first = *stats;
        *stats = before;
    }
    ScopedSet<bool> exact(d_->exact_once, true);
    once();
    if (stats) stats->total_ms += first.total_ms - before.total_ms;
}

// What every entry point that launches starts with: the key is there, the device is current, and the kernels this call
// takes follow the options as they are now.
void Evaluator::begin_call() {
    if (!keys_loaded_) throw std::runtime_error("cloud key not loaded");
    HIP_CHECK(hipSetDevice(device_));
    d_->use_w64 = br_supported(p_) && !d_->opt.force_generic;
    d_->force_generic_ks = d_->opt.force_generic;
}

// A flat call: `items` rotation items of one level, no circuit.
struct Evaluator::FlatCall {
    WorkDesc W{};                      // flat mode (gates null), item0 = 0
    int64_t items = 0;                 // rotation items: rows in, except that a MUX is two
    After after;                       // what follows the rotation
    const int32_t* factors = nullptr;  // multi-output call: the factor table [after.n_factors][N] to compact first
};

// One flat call, once: its pieces through run_items on the evaluator's stream, timed, and the stream idle at the end.
void Evaluator::flat_device_once(const FlatCall& call, EvalStats* stats) {
    begin_call();
    if (call.items == 0) return;
    Timer tall(stats != nullptr, stream_), tbr(stats != nullptr, stream_), tks(stats != nullptr, stream_);
    tall.mark();
    // on lane 0, ahead of the fork: every lane's extraction finds the lists
    if (call.factors) d_->mv.compact(stream_, call.factors, call.after.n_factors);
    run_items(p_, d_, call.W, call.items, tbr, tks, stats, call.after);
    tall.mark();
    HIP_CHECK(hipStreamSynchronize(stream_));
    add_times(stats, tall, tbr, tks);
    if (stats) stats->levels += 1;
}

// out[i] = gate(a[i], b[i] [, c[i]]): one rotation item and one key-switched row per gate
static Evaluator::FlatCall gate_call(int32_t type, size_t count, const Torus32* d_a, const Torus32* d_b, const Torus32* d_c, Torus32* d_out) {
    Evaluator::FlatCall call;
    call.W.flat_a = d_a;
    call.W.flat_b = d_b;
    call.W.flat_c = d_c;
    call.W.flat_out = d_out;
    call.W.flat_type = type;
    call.items = (int64_t)count;
    return call;
}

void Evaluator::gates_device(int32_t type, size_t count, const Torus32* d_a, const Torus32* d_b, Torus32* d_out,
                             EvalStats* stats) {
    const size_t len = count * (size_t)d_->K.stride;
    const FlatCall call = gate_call(type, count, d_a, d_b, nullptr, d_out);
    run_guarded(!overlaps(d_out, len, {{d_a, len}, {d_b, len}}), stats, [&] { flat_device_once(call, stats); });
}

void Evaluator::gates3_device(int32_t type, size_t count, const Torus32* d_a, const Torus32* d_b, const Torus32* d_c, Torus32* d_out,
                              EvalStats* stats) {
    if (!is_gate3(type)) throw std::invalid_argument("not a one-rotation three-input gate type");
    const size_t len = count * (size_t)d_->K.stride;
    const FlatCall call = gate_call(type, count, d_a, d_b, d_c, d_out);
    run_guarded(!overlaps(d_out, len, {{d_a, len}, {d_b, len}, {d_c, len}}), stats, [&] { flat_device_once(call, stats); });
}

// bootsMUX (boot-gates.cpp): two blind rotations per gate, their extracted samples added, one key switch -- a one-gate MUX
// level on lane 0: rotation items 2g and 2g + 1 are gate g's (device_common.h: kFlatMux), k_level_combine sums them, and the
// key switch runs over gates.  libtfhe counts a MUX as two bootstraps and one key switch; so do the statistics.
void Evaluator::mux_device(size_t count, const Torus32* d_a, const Torus32* d_b, const Torus32* d_c, Torus32* d_out,
                           EvalStats* stats) {
    const size_t len = count * (size_t)d_->K.stride;
    FlatCall call = gate_call(kFlatMux, count, d_a, d_b, d_c, d_out);
    call.items = 2 * (int64_t)count;
    call.after.lane = 0;
    call.after.stage = After::kMuxCombine;
    run_guarded(!overlaps(d_out, len, {{d_a, len}, {d_b, len}, {d_c, len}}), stats, [&] { flat_device_once(call, stats); });
}

// tfhe_blindRotateAndExtract_FFT from a caller's test polynomial (+ lweKeySwitch): a gate call with the raw row of flat_a as
// the combination (flat_type < 0 -- resolve(): the row as it stands, no second operand, no constant) and the descriptor
// carrying the table, so every cut of the launch finds its polynomial.  Without key switch the extracted samples are the result.
// tlwe: the table holds TLWE samples, rows of 2N words (kFlatRawTlwe: the prologue's third build).
static Evaluator::FlatCall pbs_call(size_t count, const Torus32* d_x, const Torus32* d_tv, int32_t n_tv, const int32_t* d_tv_of, Torus32* d_out,
                                    bool woks, bool tlwe) {
    Evaluator::FlatCall call = gate_call(tlwe ? kFlatRawTlwe : kFlatRaw, count, d_x, nullptr, nullptr, woks ? nullptr : d_out);
    call.W.tv = d_tv;
    call.W.n_tv = n_tv;
    call.W.tv_of = d_tv_of;
    call.after.rows_out = woks ? d_out : nullptr;
    return call;
}

void Evaluator::pbs_device(size_t count, const Torus32* d_x, const Torus32* d_tv, int32_t n_tv, const int32_t* d_tv_of, Torus32* d_out,
                           int32_t flags, EvalStats* stats) {
    if (flags & ~(kPbsNoKeyswitch | kPbsTlwePolys | kPbsAccumulator)) throw std::invalid_argument("programmable bootstrap: unknown flag");
    if (n_tv < 1 || !d_tv) throw std::invalid_argument("programmable bootstrap: no test polynomial");
    const bool tlwe = (flags & kPbsTlwePolys) != 0, accs = (flags & kPbsAccumulator) != 0;
    const bool woks = accs || (flags & kPbsNoKeyswitch) != 0;  // the accumulators are the result: nothing to key-switch
    const size_t len = count * (size_t)d_->K.stride;
    const size_t out_len = count * (accs ? (size_t)2 * (size_t)p_.N : (size_t)(woks ? extract_stride() : d_->K.stride));
    const bool over_x = overlaps(d_out, out_len, {{d_x, len}});
    // a repeat reads the table and the indices again: an output over either of them is over an input as much as one over x
    const bool over_table = overlaps(d_out, out_len, {{d_tv, (size_t)n_tv * (size_t)p_.N * (tlwe ? 2 : 1)}, {d_tv_of, count}});
    if (over_table || (woks && over_x))
        throw std::invalid_argument(over_table ? "programmable bootstrap: the output overlaps the test polynomials or their indices"
                                    : accs     ? "programmable bootstrap with accumulator output: the output overlaps the input rows"
                                               : "programmable bootstrap without key switch: the output overlaps the input rows");
    FlatCall call = pbs_call(count, d_x, d_tv, n_tv, d_tv_of, d_out, woks, tlwe);
    if (accs) call.after.stage = After::kAccumulator;
    run_guarded(!over_x, stats, [&] { flat_device_once(call, stats); });
}

// pbs_device with the stage of multi_extract.h between every piece's rotation and its key switch
void Evaluator::pbs_multi_device(size_t count, const Torus32* d_x, const Torus32* d_tv, int32_t n_tv, const int32_t* d_tv_of,
                                 const int32_t* d_factors, int32_t n_factors, const Torus32* d_bias, Torus32* d_out, int32_t flags,
                                 EvalStats* stats) {
    if (flags & kPbsAccumulator) throw std::invalid_argument("multi-output programmable bootstrap: no accumulator output (IEACHE_PBS_ACCUMULATOR is for pbs)");
    if (flags & ~(kPbsNoKeyswitch | kPbsTlwePolys)) throw std::invalid_argument("multi-output programmable bootstrap: unknown flag");
    if (n_tv < 1 || !d_tv) throw std::invalid_argument("multi-output programmable bootstrap: no test polynomial");
    if (n_factors < 1 || n_factors > kMultiMaxFactors || !d_factors)
        throw std::invalid_argument("multi-output programmable bootstrap: n_factors must be 1 .. 64 and the factor table non-null");
    const bool woks = (flags & kPbsNoKeyswitch) != 0, tlwe = (flags & kPbsTlwePolys) != 0;
    const size_t out_len = count * (size_t)n_factors * (size_t)(woks ? extract_stride() : d_->K.stride);
    // no in-place form: the output is n_factors times the input, and a repeat reads every input again
    if (overlaps(d_out, out_len,
                 {{d_x, count * (size_t)d_->K.stride}, {d_tv, (size_t)n_tv * (size_t)p_.N * (tlwe ? 2 : 1)}, {d_tv_of, count},
                  {d_factors, (size_t)n_factors * (size_t)p_.N}, {d_bias, (size_t)n_factors}}))
        throw std::invalid_argument("multi-output programmable bootstrap: the output overlaps an input (rows, test polynomials, indices, factors or bias)");
    FlatCall call = pbs_call(count, d_x, d_tv, n_tv, d_tv_of, d_out, woks, tlwe);
    call.after.stage = After::kMultiExtract;
    call.after.n_factors = n_factors;
    call.after.bias = d_bias;
    call.factors = d_factors;
    run_guarded(true, stats, [&] { flat_device_once(call, stats); });
}

// THE piece loop of the levelled calls -- everything that is cut into pieces and is no gate bootstrapping -- on the evaluator's
// stream: per piece of the cut body(piece), which runs the piece's phases (Piece above); one chunk per piece; the stream idle and
// the three times folded in at the end.  The call counts as `levels` levels.  Every scratch is reserved before this is called.
// No run_guarded: the two-limb product and the integer key switches are exact, nothing can trip.
template <class Body>
void Evaluator::run_pieces(const Cut& cut, int64_t total, int32_t levels, EvalStats* stats, Body&& body) {
    Timer tall(stats != nullptr, stream_), tbr(stats != nullptr, stream_), tks(stats != nullptr, stream_);
    tall.mark();
    for (int64_t i = 0; i < cut.pieces; i++) {
        Piece piece{piece_first(cut, i), piece_count(cut, total, i), tbr, tks, stats};
        body(piece);
        if (stats) stats->chunks++;
    }
    tall.mark();
    HIP_CHECK(hipStreamSynchronize(stream_));
    add_times(stats, tall, tbr, tks);
    if (stats) stats->levels += levels;
}

// lweKeySwitch alone: a flat call without a rotation.  Pieces of at most a chunk, each one launch of the key-switch unit with a
// flat descriptor whose flat_out is the caller's rows (what the multi-output call hands it).
void Evaluator::keyswitch_device(size_t count, const Torus32* d_u, Torus32* d_out, EvalStats* stats) {
    if (overlaps(d_out, count * (size_t)d_->K.stride, {{d_u, count * (size_t)extract_stride()}}))
        throw std::invalid_argument("key switch: the output overlaps the input rows");
    begin_call();
    if (count == 0) return;
    if (!d_u || !d_out) throw std::invalid_argument("key switch: null rows");
    Lane& ln = d_->lane[0];
    const Cut cut = cut_in_runs((int64_t)count, std::min<int64_t>((int64_t)count, (int64_t)d_->opt.chunk));
    d_->ks.reserve(ln.ks, cut.per_piece, d_->opt, d_->force_generic_ks);
    WorkDesc W{};
    W.flat_out = d_out;
    W.flat_type = kFlatRaw;
    run_pieces(cut, (int64_t)count, 1, stats, [&](Piece& pc) {
        pc.keyswitch(pc.count, pc.count, [&](int64_t, int64_t rows) {
            launch_keyswitch(d_, ln, rows_desc(W, pc.first), rows, d_u + (size_t)pc.first * (size_t)extract_stride(), nullptr);
        });
    });
}

// The packing unit twice in a context (pack.h): the packing key switch and the projection, and what differs between their
// evaluator paths -- the object, lane 0's scratch, the forced-split option, and the words of the messages.
struct Evaluator::PackSide {
    Pack& unit;
    std::unique_ptr<PackScratch>& scratch;
    int64_t& split;
    const char *name, *key, *input;  // "<name>: no <key> key set", "<name>: the output overlaps the input <input>"
    void require_key() const {
        if (!unit.has_key()) throw std::invalid_argument(std::string(name) + ": no " + key + " key set");
    }
    // the cut of a call under the options as they are
    PackPlan plan(const Impl* d, int64_t groups, int32_t m) const { return unit.plan(groups, m, d->opt.pack_piece_rows, (int32_t)split, d->opt.cus); }
};
Evaluator::PackSide Evaluator::packing() const { return {d_->pack, d_->lane[0].pack, d_->opt.pack_split, "pack", "packing", "rows"}; }
Evaluator::PackSide Evaluator::projection() const {
    return {d_->project, d_->lane[0].project, d_->opt.project_split, "tlwe_project", "projection", "samples"};
}

void Evaluator::set_pack_key(const PackSide& s, int32_t t, int32_t basebit, const Torus32* pk) {
    HIP_CHECK(hipSetDevice(device_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    s.unit.set_key(t, basebit, pk, stream_);
    if (!pk) s.scratch.reset();  // the key is gone (the stream is idle): so is the scratch of its calls
    s.split = 0;  // a forced split was accepted for the walk of the key that is gone
}
void Evaluator::set_packing_key(int32_t t, int32_t basebit, const Torus32* pk) { set_pack_key(packing(), t, basebit, pk); }
void Evaluator::set_projection_key(int32_t t, int32_t basebit, const Torus32* pk) { set_pack_key(projection(), t, basebit, pk); }
bool Evaluator::has_packing_key() const { return d_->pack.has_key(); }
bool Evaluator::has_projection_key() const { return d_->project.has_key(); }

void Evaluator::pack_side_figures(const PackSide& s, size_t groups, int32_t m, int64_t out[4]) const {
    s.require_key();
    const PackPlan pl = s.plan(d_, (int64_t)groups, m);
    out[0] = pl.pieces;
    out[1] = pl.groups_per_piece;
    out[2] = pl.ksplit;
    out[3] = pl.k_steps;
}
void Evaluator::pack_plan_figures(size_t groups, int32_t m, int64_t out[4]) const { pack_side_figures(packing(), groups, m, out); }
void Evaluator::project_plan_figures(size_t count, int32_t width, int64_t out[4]) const { pack_side_figures(projection(), count, width, out); }

// A call of the packing unit: `groups` groups (items) of m rows, in_words words of d_in and 2N of d_out each; pieces of whole
// groups, each one launch(plan, first group, groups) of the unit -- several kernels, counted as one key-switch launch.
// shape_error: what the call's own rule says of its scalars, judged after the key.
template <class Launch>
void Evaluator::pack_side_device(const PackSide& s, const char* shape_error, size_t groups, int32_t m, const Torus32* d_in, size_t in_words,
                                 Torus32* d_out, EvalStats* stats, Launch&& launch) {
    const std::string who = std::string(s.name) + ": ";
    s.require_key();
    if (shape_error) throw std::invalid_argument(shape_error);
    if (overlaps(d_out, groups * (size_t)2 * (size_t)p_.N, {{d_in, groups * in_words}})) throw std::invalid_argument(who + "the output overlaps the input " + s.input);
    begin_call();
    if (groups == 0) return;
    if (!d_in || !d_out) throw std::invalid_argument(who + "null rows");
    const PackPlan pl = s.plan(d_, (int64_t)groups, m);
    if (!s.scratch) s.scratch.reset(new PackScratch);
    s.unit.reserve(*s.scratch, pl);
    run_pieces(pl.cut(), (int64_t)groups, 1, stats, [&](Piece& pc) {
        pc.keyswitch(pc.count, pc.count, [&](int64_t, int64_t cnt) { launch(pl, pc.first, cnt); });
    });
}

// The packing key switch: per piece four launches of the unit (digits, init, product, placement).
void Evaluator::pack_device(size_t groups, int32_t m, int32_t spread, int32_t shift, const Torus32* d_rows, Torus32* d_out, EvalStats* stats) {
    const PackSide s = packing();
    const size_t row_words = (size_t)m * (size_t)d_->K.stride, out_words = (size_t)2 * (size_t)p_.N;
    pack_side_device(s, pack_call_error(p_, m, spread, shift), groups, m, d_rows, row_words, d_out, stats, [&](const PackPlan& pl, int64_t g0, int64_t cnt) {
        s.unit.launch(*s.scratch, stream_, pl, cnt, m, spread, shift, d_rows + (size_t)g0 * row_words, d_->K.stride, d_out + (size_t)g0 * out_words);
    });
}

// The projection: per piece three launches of the unit (window digits, product, placement).
void Evaluator::tlwe_project_device(size_t count, int32_t first, int32_t width, int32_t dest, const Torus32* d_in, Torus32* d_out, EvalStats* stats) {
    const PackSide s = projection();
    const size_t row = (size_t)2 * (size_t)p_.N;
    pack_side_device(s, project_call_error(p_, first, width, dest), count, width, d_in, row, d_out, stats, [&](const PackPlan& pl, int64_t i0, int64_t cnt) {
        s.unit.launch_window(*s.scratch, stream_, pl, cnt, first, width, dest, d_in + (size_t)i0 * row, d_out + (size_t)i0 * row);
    });
}

// The replace write of a window: the tree's pieces; per piece the unit's read (the tree over the items' own memories, the rotation
// toward position 0), the projection in runs of its own plan, and the unit's subtraction and lut_add's piece with memory i for item
// i.  A piece reads and adds into its own items' memories only and has read them before it adds (one stream), so d_out == d_mem
// is sound.
void Evaluator::lut_write_coef_device(const TgswSet& set, size_t count, int32_t depth, int32_t steps, int32_t width, int32_t unit,
                                      const int32_t* d_sel_of, const Torus32* d_new, const Torus32* d_mem, Torus32* d_out, EvalStats* stats) {
    const size_t row = (size_t)2 * (size_t)p_.N;
    const SetCall c{kCallLutWriteCoef, count, depth, steps, 1, 0, 0, width, unit};
    if (!begin_set_call(set, c, {d_sel_of, d_new, d_mem, d_out}, row)) return;
    Lane& ln = d_->lane[0];
    const PackSide proj = projection();
    const CmuxPlan pl = cmux_plan((int64_t)count, depth, d_->opt.cmux_piece_rows);
    const PackPlan pp = proj.plan(d_, pl.items_per_piece, width);
    d_->cmux.reserve_read(ln.cmux, pl, depth);
    if (!proj.scratch) proj.scratch.reset(new PackScratch);
    proj.unit.reserve(*proj.scratch, pp);
    ln.coef_old.reserve_exact((size_t)pl.items_per_piece * row);
    ln.coef_idx.reserve_exact((size_t)2 * kRotateMaxSteps + count);
    int32_t *toward = ln.coef_idx, *back = toward + kRotateMaxSteps, *own = back + kRotateMaxSteps;
    // not launches of the call's: the copy the sums start from, and the public amounts and memory indices
    if (d_out != d_mem) HIP_CHECK(hipMemcpyAsync(d_out, d_mem, set_arg_words(c, set_call_output(c), p_.N, row) * 4, hipMemcpyDeviceToDevice, stream_));
    const int64_t tables = std::max<int64_t>((int64_t)count, steps);
    hipLaunchKernelGGL(k_write_coef_tables, dim3((unsigned)((tables + 255) / 256)), dim3(256), 0, stream_, unit, steps, 2 * p_.N, (int64_t)count, toward,
                       back, own);
    run_pieces(pl.cut(), (int64_t)count, 2 * (depth + steps) + 1, stats, [&](Piece& pc) {
        Torus32 *rows = ln.cmux.rows, *old = ln.coef_old;
        // old row: the addressed word of each item's own memory at position 0
        pc.rotate([&] {
            return d_->cmux.launch_read_own(set, ln.cmux, stream_, pc.first, pc.count, depth, steps, d_sel_of, toward, d_mem + ((size_t)pc.first << depth) * row);
        });
        // old = the window alone
        pc.keyswitch(pc.count, pp.groups_per_piece, [&](int64_t g0, int64_t g) {
            proj.unit.launch_window(*proj.scratch, stream_, pp, g, 0, width, 0, rows + (size_t)g0 * row, old + (size_t)g0 * row);
        });
        // delta = new - old, added at the address into the items' own memories
        pc.rotate([&] {
            d_->cmux.launch_delta(stream_, pc.count, d_new + (size_t)pc.first * row, old);
            return 1 + d_->cmux.launch_add(set, ln.cmux, stream_, pc.first, pc.count, depth, steps, d_sel_of, back, old, (int32_t)count, own, d_out);
        });
    });
}

TgswSet* Evaluator::tgsw_prepare_device(const Torus32* d_samples, size_t n) {
    HIP_CHECK(hipSetDevice(device_));
    return d_->cmux.prepare(d_samples, n, stream_);
}

TgswSet* Evaluator::tgsw_prepare_device(const Torus32* d_samples, size_t n, int32_t l, int32_t Bgbit) {
    HIP_CHECK(hipSetDevice(device_));
    return d_->cmux.prepare(d_samples, n, l, Bgbit, stream_);
}

uint64_t Evaluator::cmux_id() const { return d_->cmux.id(); }

void Evaluator::cmux_plan_figures(size_t count, int32_t depth, int64_t out[4]) const {
    // a negative depth asks for the flat plan: only the upper bound is refused, as lut_tree refuses it
    if (depth > kCmuxMaxDepth) throw std::invalid_argument(set_call_refusal(SetCall{kCallLutTree, count, depth}, p_.N));
    const CmuxPlan pl = cmux_plan((int64_t)count, depth, d_->opt.cmux_piece_rows);
    out[0] = pl.pieces;
    out[1] = pl.items_per_piece;
    out[2] = pl.a_rows;
    out[3] = pl.b_rows;
}

// What every call on a set opens with, from the table of set_calls.h (`a`: the call's pointer arguments in its order): the
// set is this context's, the projection key is there where the call needs it, the scalars are in range, the output shares no word with an input -- but for the one input that may
// be the output exactly -- then begin_call() and the rows a call needs are there.  -> whether there are items to run
bool Evaluator::begin_set_call(const TgswSet& set, const SetCall& c, std::initializer_list<const void*> args, size_t out_row_words) {
    const void* const* a = args.begin();
    d_->cmux.check_owner(set);
    const SetCallShape& s = set_call_shape(c);
    if (s.window && !d_->project.has_key()) throw std::invalid_argument(std::string(s.name) + ": no projection key set");
    const std::string refusal = set_call_refusal(c, p_.N);
    if (!refusal.empty()) throw std::invalid_argument(refusal);
    const int out = s.n_args - 1;
    const SetArg* alias = nullptr;
    bool shared = false;
    for (int i = 0; i < out; i++) {
        if (s.args[i].role == kMayBeOutput) alias = &s.args[i];
        if (s.args[i].role == kMayBeOutput && a[i] == a[out]) continue;
        shared |= overlaps(static_cast<const Torus32*>(a[out]), set_arg_words(c, s.args[out], p_.N, out_row_words),
                           {{a[i], set_arg_words(c, s.args[i], p_.N, out_row_words)}});
    }
    if (shared)
        throw std::invalid_argument(std::string(s.name) + ": the output overlaps an input" +
                                    (alias ? std::string(" (only d_out == ") + alias->name + ", the " + s.in_place + " in place, is accepted)" : ""));
    begin_call();
    for (int i = 0; i <= out; i++)
        if (!a[i] && s.args[i].need != kOptional && (c.count > 0 || s.args[i].empty_too)) throw std::invalid_argument(std::string(s.name) + ": null rows");
    return c.count > 0;
}

// The flat CMux: pieces of at most "cmux_piece_rows" rows, one launch each.
void Evaluator::cmux_device(const TgswSet& set, size_t count, const int32_t* d_sel_of, const Torus32* d_d1, const Torus32* d_d0, Torus32* d_out,
                            EvalStats* stats) {
    const size_t row = (size_t)2 * (size_t)p_.N;
    if (!begin_set_call(set, SetCall{kCallCmux, count}, {d_sel_of, d_d1, d_d0, d_out}, row)) return;
    run_pieces(cmux_plan((int64_t)count, -1, d_->opt.cmux_piece_rows).cut(), (int64_t)count, 1, stats, [&](Piece& pc) {
        const int64_t r0 = pc.first;
        CmuxRows R;
        R.rows = pc.count;
        R.src = d_d1 + (size_t)r0 * row;
        R.src0 = d_d0 ? d_d0 + (size_t)r0 * row : nullptr;
        R.dst = d_out + (size_t)r0 * row;
        R.sel_of = d_sel_of ? d_sel_of + r0 : nullptr;
        R.item0 = r0;
        pc.rotate([&] {
            d_->cmux.launch(set, stream_, R);
            return 1;
        });
    });
}

// The CMux tree: pieces of whole items, each `depth` launches through the two scratch buffers, which are reserved for the
// largest piece before the first.
void Evaluator::lut_tree_device(const TgswSet& set, size_t count, int32_t depth, const int32_t* d_sel_of, const Torus32* d_tables, int32_t n_tables,
                                const int32_t* d_table_of, Torus32* d_out, EvalStats* stats) {
    const size_t row = (size_t)2 * (size_t)p_.N;
    if (!begin_set_call(set, SetCall{kCallLutTree, count, depth, 0, n_tables}, {d_sel_of, d_tables, d_table_of, d_out}, row)) return;
    Lane& ln = d_->lane[0];
    const CmuxPlan pl = cmux_plan((int64_t)count, depth, d_->opt.cmux_piece_rows);
    d_->cmux.reserve(ln.cmux, pl);
    run_pieces(pl.cut(), (int64_t)count, depth, stats, [&](Piece& pc) {
        pc.rotate([&] {
            return d_->cmux.launch_tree(set, ln.cmux, stream_, pc.first, pc.count, depth, d_sel_of, d_tables, n_tables, d_table_of,
                                        d_out + (size_t)pc.first * row);
        });
    });
}

// The scatter: the tree's pieces and scratch with the steps run the other way (Cmux::launch_scatter); the last step of a piece
// adds the memory rows and may write over them.
void Evaluator::lut_scatter_device(const TgswSet& set, size_t count, int32_t depth, const int32_t* d_sel_of, const Torus32* d_values,
                                   const Torus32* d_mem, Torus32* d_out, EvalStats* stats) {
    const size_t row = (size_t)2 * (size_t)p_.N;
    if (!begin_set_call(set, SetCall{kCallLutScatter, count, depth}, {d_sel_of, d_values, d_mem, d_out}, row)) return;
    Lane& ln = d_->lane[0];
    const CmuxPlan pl = cmux_plan((int64_t)count, depth, d_->opt.cmux_piece_rows);
    d_->cmux.reserve(ln.cmux, pl);
    run_pieces(pl.cut(), (int64_t)count, depth, stats, [&](Piece& pc) {
        const size_t i0 = (size_t)pc.first;
        pc.rotate([&] {
            return d_->cmux.launch_scatter(set, ln.cmux, stream_, pc.first, pc.count, depth, d_sel_of, d_values + i0 * row,
                                           d_mem ? d_mem + (i0 << depth) * row : nullptr, d_out + (i0 << depth) * row);
        });
    });
}

// The replace write mem[addr] := new: the tree's pieces; per piece the tree over the items' own memories, the subtraction and the
// scatter (Cmux::launch_write).  A piece touches its own items' rows only, so the pieces are independent and d_out == d_mem is sound.
void Evaluator::lut_write_device(const TgswSet& set, size_t count, int32_t depth, const int32_t* d_sel_of, const Torus32* d_new, const Torus32* d_mem,
                                 Torus32* d_out, EvalStats* stats) {
    const size_t row = (size_t)2 * (size_t)p_.N;
    if (!begin_set_call(set, SetCall{kCallLutWrite, count, depth}, {d_sel_of, d_new, d_mem, d_out}, row)) return;
    Lane& ln = d_->lane[0];
    const CmuxPlan pl = cmux_plan((int64_t)count, depth, d_->opt.cmux_piece_rows);
    d_->cmux.reserve_read(ln.cmux, pl, depth);
    run_pieces(pl.cut(), (int64_t)count, 2 * depth, stats, [&](Piece& pc) {
        const size_t i0 = (size_t)pc.first;
        pc.rotate([&] {
            return d_->cmux.launch_write(set, ln.cmux, stream_, pc.first, pc.count, depth, d_sel_of, d_new + i0 * row, d_mem + (i0 << depth) * row,
                                         d_out + (i0 << depth) * row);
        });
    });
}

// The shared write mem[m_i][hi_i].coef[lo_i] += v_i: the tree's pieces for (count, depth); out starts as the memories (or zeros,
// or is the memories themselves) and every piece ADDS into it (Cmux::launch_add), so which piece an item falls into does not
// matter: the adds are order-free mod 2^32 and all on one stream behind the initialising copy.
void Evaluator::lut_add_device(const TgswSet& set, size_t count, int32_t depth, int32_t steps, const int32_t* d_sel_of, const int32_t* d_amount_of,
                               const Torus32* d_values, const Torus32* d_mems, int32_t n_mems, const int32_t* d_mem_of, Torus32* d_out, EvalStats* stats) {
    const size_t row = (size_t)2 * (size_t)p_.N;
    const SetCall c{kCallLutAdd, count, depth, steps, n_mems};
    const bool items = begin_set_call(set, c, {d_sel_of, d_amount_of, d_values, d_mems, d_mem_of, d_out}, row);
    // not a launch of the call's: the copy or fill the sums start from
    const size_t words = set_arg_words(c, set_call_output(c), p_.N, row);
    if (d_mems && d_mems != d_out)
        HIP_CHECK(hipMemcpyAsync(d_out, d_mems, words * 4, hipMemcpyDeviceToDevice, stream_));
    else if (!d_mems)
        HIP_CHECK(hipMemsetAsync(d_out, 0, words * 4, stream_));
    if (!items) {
        HIP_CHECK(hipStreamSynchronize(stream_));
        return;
    }
    Lane& ln = d_->lane[0];
    const CmuxPlan pl = cmux_plan((int64_t)count, depth, d_->opt.cmux_piece_rows);
    d_->cmux.reserve_read(ln.cmux, pl, depth);
    run_pieces(pl.cut(), (int64_t)count, depth + steps, stats, [&](Piece& pc) {
        pc.rotate([&] {
            return d_->cmux.launch_add(set, ln.cmux, stream_, pc.first, pc.count, depth, steps, d_sel_of, d_amount_of, d_values + (size_t)pc.first * row,
                                       n_mems, d_mem_of, d_out);
        });
    });
}

// Automata (section 3k).  The call stands beside the table of set_calls.h (automaton_plan.h says why), so its prelude is written
// out here: owners, n_finals, the overlap of the output with any input, begin_call(), null rows -- begin_set_call's order.  Its
// pieces go through the piece loop like every other call's.
Automaton* Evaluator::automaton_create(int32_t states, int32_t steps, int32_t n_out, const int32_t* next0, const int32_t* next1) {
    HIP_CHECK(hipSetDevice(device_));
    return d_->cmux.automaton_create(states, steps, n_out, next0, next1);
}

void Evaluator::automaton_plan_figures(const Automaton& a, size_t count, int64_t out[5]) const {
    d_->cmux.check_owner(a);
    const AutomatonPlan pl = automaton_plan((int64_t)count, a.states, a.steps, d_->opt.cmux_piece_rows, d_->opt.automaton_steps_per_launch);
    out[0] = pl.pieces;
    out[1] = pl.items_per_piece;
    out[2] = pl.scratch_rows;
    out[3] = pl.steps_per_launch;
    out[4] = pl.launches;
}

void Evaluator::automaton_run_device(const TgswSet& set, const Automaton& a, size_t count, const int32_t* d_sel_of, const Torus32* d_finals,
                                     int32_t n_finals, const int32_t* d_final_of, Torus32* d_out, EvalStats* stats) {
    d_->cmux.check_owner(set);
    d_->cmux.check_owner(a);
    if (n_finals < 1) throw std::invalid_argument("automaton_run: n_finals must be at least 1");
    const size_t row = (size_t)2 * (size_t)p_.N;
    if (overlaps(d_out, count * (size_t)a.n_out * row,
                 {{d_finals, (size_t)n_finals * (size_t)a.states * row}, {d_sel_of, count * (size_t)a.steps}, {d_final_of, count}}))
        throw std::invalid_argument("automaton_run: the output overlaps an input");
    begin_call();
    if (count == 0) return;
    if (!d_finals || !d_out) throw std::invalid_argument("automaton_run: null rows");
    Lane& ln = d_->lane[0];
    const AutomatonPlan pl = automaton_plan((int64_t)count, a.states, a.steps, d_->opt.cmux_piece_rows, d_->opt.automaton_steps_per_launch);
    d_->cmux.reserve_automaton(ln.cmux, pl);
    run_pieces(pl.cut(), (int64_t)count, a.steps, stats, [&](Piece& pc) {
        pc.rotate([&] {
            return d_->cmux.launch_automaton(set, a, ln.cmux, stream_, pl, pc.first, pc.count, d_sel_of, d_finals, n_finals, d_final_of,
                                             d_out + (size_t)pc.first * (size_t)a.n_out * row);
        });
    });
}

// The rotation by caller selectors: the flat CMux's pieces, one launch each whatever the number of steps; no scratch.
void Evaluator::tlwe_rotate_device(const TgswSet& set, size_t count, int32_t steps, const int32_t* d_sel_of, const int32_t* d_amount_of,
                                   const Torus32* d_in, Torus32* d_out, EvalStats* stats) {
    const size_t row = (size_t)2 * (size_t)p_.N;
    if (!begin_set_call(set, SetCall{kCallTlweRotate, count, 0, steps}, {d_sel_of, d_amount_of, d_in, d_out}, row)) return;
    run_pieces(cmux_plan((int64_t)count, -1, d_->opt.cmux_piece_rows).cut(), (int64_t)count, steps, stats, [&](Piece& pc) {
        const int64_t r0 = pc.first;
        RotateRows R;
        R.rows = pc.count;
        R.src = d_in + (size_t)r0 * row;
        R.dst = d_out + (size_t)r0 * row;
        R.sel_of = d_sel_of;
        R.amount_of = d_amount_of;
        R.item0 = r0;
        R.steps = R.sel_stride = steps;
        pc.rotate([&] {
            d_->cmux.launch_rotate(set, stream_, R);
            return 1;
        });
    });
}

// The coefficient-level lookup: the tree's pieces; per piece the tree into the rows the lane keeps, their rotation in place, the
// extraction (into the caller's rows, or the lane's for the key switch) and the key switch in runs of at most a chunk.
// Everything is reserved before the first piece.
void Evaluator::lut_read_device(const TgswSet& set, size_t count, int32_t depth, int32_t steps, const int32_t* d_sel_of, const int32_t* d_amount_of,
                                const Torus32* d_tables, int32_t n_tables, const int32_t* d_table_of, int32_t coef, int32_t flags, Torus32* d_out,
                                EvalStats* stats) {
    const bool woks = (flags & kLutReadNoKeyswitch) != 0;
    const size_t out_stride = (size_t)(woks ? extract_stride() : d_->K.stride);
    const SetCall c{kCallLutRead, count, depth, steps, n_tables, flags, coef};
    if (!begin_set_call(set, c, {d_sel_of, d_amount_of, d_tables, d_table_of, d_out}, out_stride)) return;
    Lane& ln = d_->lane[0];
    const CmuxPlan pl = cmux_plan((int64_t)count, depth, d_->opt.cmux_piece_rows);
    d_->cmux.reserve_read(ln.cmux, pl, depth);
    const int64_t ks_piece = std::min<int64_t>(pl.items_per_piece, (int64_t)d_->opt.chunk);
    if (!woks) {
        ln.ext.reserve_exact((size_t)pl.items_per_piece, d_->ext_row_bytes());
        d_->ks.reserve(ln.ks, ks_piece, d_->opt, d_->force_generic_ks);
    }
    WorkDesc W{};
    W.flat_out = d_out;
    W.flat_type = kFlatRaw;
    // the extracted rows of a piece: the caller's, or the lane's for the key switch
    auto rows_of = [&](int64_t i0) { return woks ? d_out + (size_t)i0 * out_stride : (Torus32*)ln.ext; };
    run_pieces(pl.cut(), (int64_t)count, depth + steps, stats, [&](Piece& pc) {
        pc.rotate([&] {
            return d_->cmux.launch_read(set, ln.cmux, stream_, pc.first, pc.count, depth, steps, d_sel_of, d_amount_of, d_tables, n_tables, d_table_of,
                                        coef, rows_of(pc.first), extract_stride());
        });
        if (woks) return;
        pc.keyswitch(pc.count, ks_piece, [&](int64_t done, int64_t run) {
            launch_keyswitch(d_, ln, rows_desc(W, pc.first + done), run, rows_of(pc.first) + (size_t)done * (size_t)extract_stride(), nullptr);
        });
    });
}

// ---- the way back to the gates (section 3m; unpack_plan.h) ----
namespace {
// What both calls do with `rows` rows of a window of samples: runs of at most `chunk` rows through the key switch's door for such
// rows, or (woks) the extracted rows themselves into the caller's.  Row r of `out` takes run row r.
struct UnpackRows {
    Evaluator::Impl* d;
    Lane& ln;
    UnpackWindow win;
    bool woks;
    size_t out_stride;
    // the rows of a call whose runs have these sizes at most: the key switch's scratch, and the lane's extracted rows for the
    // runs whose family walks stored rows (the product stores none)
    void reserve(std::initializer_list<int64_t> run_sizes) const {
        if (woks) return;
        int64_t widest = 0, stored = 0;
        for (const int64_t s : run_sizes) {
            widest = std::max(widest, s);
            if (d->ks.window_needs_rows(s, d->opt, d->force_generic_ks)) stored = std::max(stored, s);
        }
        d->ks.reserve(ln.ks, widest, d->opt, d->force_generic_ks);
        if (stored) ln.ext.reserve_exact((size_t)stored, d->ext_row_bytes());
    }
    // rows row0 .. row0 + rows of `samples` seen as [..][width] rows, inside piece pc
    void run(Piece& pc, const Torus32* samples, int64_t row0, int64_t rows, Torus32* out) const {
        if (woks) {  // belongs to neither kind of phase, as tlwe_extract's launch: timed in total_ms alone and counted nowhere
            d->ks.extract_window(ln.stream, rows, KsWindowRows{samples, row0, win}, out, (int32_t)out_stride);
            HIP_CHECK(hipGetLastError());
            return;
        }
        pc.keyswitch(rows, std::min<int64_t>(rows, (int64_t)d->opt.chunk), [&](int64_t done, int64_t run_rows) {
            d->ks.launch_window(ln.ks, ln.stream, run_rows, KsWindowRows{samples, row0 + done, win}, ln.ext, out + (size_t)done * out_stride, d->opt,
                                d->force_generic_ks);
        });
    }
};
// the sizes the runs of `rows` rows in runs of at most `chunk` take: the full run and the last
std::pair<int64_t, int64_t> run_sizes(int64_t rows, int64_t chunk) {
    const int64_t full = std::min(rows, std::max<int64_t>(chunk, 1));
    return {full, rows > 0 && rows % full ? rows % full : full};
}
}  // namespace

// The unpacking key switch: the call's rows in runs of at most a chunk, one piece per run.
void Evaluator::unpack_device(size_t count, int32_t first, int32_t width, int32_t spread, int32_t flags, const Torus32* d_in, Torus32* d_out,
                              EvalStats* stats) {
    if (const char* e = unpack_call_error(p_.N, first, width, spread, flags)) throw std::invalid_argument(e);
    const bool woks = (flags & kUnpackNoKeyswitch) != 0;
    const size_t out_stride = (size_t)(woks ? extract_stride() : d_->K.stride);
    const int64_t rows = unpack_rows((int64_t)count, width);
    if (overlaps(d_out, (size_t)rows * out_stride, {{d_in, count * (size_t)2 * (size_t)p_.N}})) throw std::invalid_argument("unpack: the output overlaps the input samples");
    begin_call();
    if (count == 0) return;
    if (!d_in || !d_out) throw std::invalid_argument("unpack: null rows");
    const UnpackRows U{d_, d_->lane[0], UnpackWindow{first, width, spread}, woks, out_stride};
    const Cut cut = unpack_runs((int64_t)count, width, (int64_t)d_->opt.chunk);
    const auto sizes = run_sizes(rows, cut.per_piece);
    U.reserve({sizes.first, sizes.second});
    run_pieces(cut, rows, 1, stats, [&](Piece& pc) { U.run(pc, d_in, pc.first, pc.count, d_out + (size_t)pc.first * out_stride); });
}

// The read of an addressed word: the tree's pieces; per piece the tree into the rows the lane keeps and their rotation in place
// toward position 0 (Cmux::launch_read_rows), then the window (0, width, 1) of those rows unpacked in runs of at most a chunk.
// Everything is reserved before the first piece.
void Evaluator::word_read_device(const TgswSet& set, size_t count, int32_t depth, int32_t steps, int32_t width, int32_t unit, const int32_t* d_sel_of,
                                 const Torus32* d_tables, int32_t n_tables, const int32_t* d_table_of, int32_t flags, Torus32* d_out, EvalStats* stats) {
    const bool woks = (flags & kUnpackNoKeyswitch) != 0;
    const size_t out_stride = (size_t)(woks ? extract_stride() : d_->K.stride);
    SetCall c{kCallLutRead, count, depth, steps, n_tables, flags, 0, width, unit};
    c.word = true;
    if (!begin_set_call(set, c, {d_sel_of, nullptr, d_tables, d_table_of, d_out}, out_stride)) return;
    Lane& ln = d_->lane[0];
    const CmuxPlan pl = cmux_plan((int64_t)count, depth, d_->opt.cmux_piece_rows);
    d_->cmux.reserve_read(ln.cmux, pl, depth);
    const UnpackRows U{d_, ln, UnpackWindow{0, width, 1}, woks, out_stride};
    const int64_t last_items = (int64_t)count - (pl.pieces - 1) * pl.items_per_piece;
    const auto widest = run_sizes(unpack_rows(pl.items_per_piece, width), (int64_t)d_->opt.chunk);
    const auto last = run_sizes(unpack_rows(last_items, width), (int64_t)d_->opt.chunk);
    U.reserve({widest.first, widest.second, last.first, last.second});
    // not a launch of the call's: the public amounts 2N - unit 2^t of the rotation toward position 0 (lut_write_coef's table)
    ln.coef_idx.reserve_exact((size_t)2 * kRotateMaxSteps);
    int32_t *toward = ln.coef_idx, *back = toward + kRotateMaxSteps;
    if (steps > 0)
        hipLaunchKernelGGL(k_write_coef_tables, dim3((unsigned)((steps + 255) / 256)), dim3(256), 0, stream_, unit, steps, 2 * p_.N, (int64_t)0, toward, back, back);
    run_pieces(pl.cut(), (int64_t)count, depth + steps, stats, [&](Piece& pc) {
        pc.rotate([&] {
            return d_->cmux.launch_read_rows(set, ln.cmux, stream_, pc.first, pc.count, depth, steps, d_sel_of, toward, d_tables, n_tables, d_table_of);
        });
        U.run(pc, ln.cmux.rows, 0, unpack_rows(pc.count, width), d_out + (size_t)unpack_rows(pc.first, width) * out_stride);
    });
}

void Evaluator::tlwe_extract_device(size_t count, const Torus32* d_tlwe, const int32_t* d_coef_of, Torus32* d_u, EvalStats* stats) {
    if (overlaps(d_u, count * (size_t)extract_stride(), {{d_tlwe, count * (size_t)2 * (size_t)p_.N}, {d_coef_of, count}}))
        throw std::invalid_argument("tlwe_extract: the output overlaps an input");
    begin_call();
    if (count == 0) return;
    if (!d_tlwe || !d_u) throw std::invalid_argument("tlwe_extract: null rows");
    // one piece whose one launch belongs to neither kind of phase: it is timed in total_ms alone and counted nowhere
    run_pieces(Cut{1, (int64_t)count}, (int64_t)count, 1, stats, [&](Piece&) {
        d_->cmux.launch_extract(stream_, (int64_t)count, d_tlwe, d_coef_of, d_u, extract_stride());
        HIP_CHECK(hipGetLastError());
    });
}

// A linear layer: one piece whose one launch of the unit belongs to neither kind of phase, as tlwe_extract_device's.  No key is
// read, so begin_call() is not asked for one.
void Evaluator::lwe_linear_device(int32_t rows, size_t batch, int32_t n_out, int32_t n_in, const int8_t* d_w, const int32_t* d_bias, const Torus32* d_x,
                                  Torus32* d_out, EvalStats* stats) {
    LinearCall c;
    c.rows = rows, c.batch = batch, c.n_out = n_out, c.n_in = n_in, c.w = d_w, c.bias = d_bias, c.x = d_x, c.out = d_out, c.device = true;
    if (const char* e = linear_call_error(p_, c)) throw std::invalid_argument(e);
    if (linear_rows(p_, kLinearRowsExtracted).stride != extract_stride()) throw std::logic_error("lwe_linear: linear_plan.h and extract_stride() disagree");
    HIP_CHECK(hipSetDevice(device_));
    if (batch == 0) return;
    const LinearPlan pl = d_->linear.plan(rows, n_out, n_in, (int32_t)d_->opt.linear_kernel);
    run_pieces(Cut{1, (int64_t)batch}, (int64_t)batch, 1, stats, [&](Piece&) {
        d_->linear.launch(stream_, pl, rows, batch, n_out, n_in, d_w, d_bias, d_x, d_out);
        HIP_CHECK(hipGetLastError());
    });
}

void Evaluator::linear_plan_figures(int32_t rows, int32_t n_out, int32_t n_in, int64_t out[4]) const {
    if (const char* e = linear_scalar_error(rows, n_out, n_in, false)) throw std::invalid_argument(e);
    const LinearPlan pl = d_->linear.plan(rows, n_out, n_in, (int32_t)d_->opt.linear_kernel);
    out[0] = pl.kernel;
    out[1] = pl.col_blocks;
    out[2] = pl.wave_tiles;
    out[3] = pl.k_steps;
}

void Evaluator::eval_circuit_device(const Circuit& c, size_t batch, const Torus32* d_in, Torus32* d_out, EvalStats* stats) {
    const size_t stride = (size_t)d_->K.stride;
    run_guarded(!overlaps(d_out, batch * c.outputs.size() * stride, {{d_in, batch * (size_t)c.n_inputs * stride}}), stats,
                [&] { eval_circuit_device_once(c, batch, d_in, d_out, stats); });
}

void Evaluator::debug_blind_rotate(size_t count, const Torus32* d_x, Torus32* d_acc, int32_t steps) {
    run_guarded(true, nullptr, [&] { debug_blind_rotate_once(count, d_x, d_acc, steps); });
}

using TuneKey = std::tuple<size_t, int32_t, size_t, size_t, bool>;
static TuneKey tune_key(const Evaluator::Impl* d, const Circuit& c, size_t batch) {
    return std::make_tuple(c.gates.size(), (int32_t)c.n_levels(), c.outputs.size(), batch, d->opt.exact_fft || d->exact_once);
}
// Whether an evaluation of `c` over `batch` expressions runs as expression pipelines ("pipe_min").
// -> 0 (no) or the number of pipelines (each gets at least one expression)
// trial (may be null): set to 0 / 1 when this evaluation is one of the two timed trials of its (circuit, batch) -- without /
// with pipelines -- and to -1 otherwise; the caller then reports the evaluation's wall time to tune_report().
static int pipelined(Evaluator::Impl* d, const Circuit& c, size_t batch, int* trial = nullptr, bool either = false) {
    if (trial) *trial = -1;
    if (!d->opt.overlap || !d->use_w64 || batch < 2 || c.n_levels() < 1) return 0;
    const int lanes = (int)std::min<size_t>((size_t)d->opt.pipe_lanes, batch);
    int64_t gates = (int64_t)c.level_offset[c.n_levels()] - (int64_t)c.level_offset[0];
    for (int32_t m : c.level_mux) gates += m;  // in blind rotations: a MUX is two
    const int64_t work = gates * (int64_t)batch, bar = d->opt.pipe_min * (int64_t)c.n_levels();  // mean level against pipe_min
    // From 2 x pipe_min on pipelines won every measurement.  Below, it depends on where the levels fall among the kernels'
    // regimes (a level of 2 200 gate instances as two pipelines' launches of 1 100 costs a second, nearly empty round; on one
    // stream it runs as a rotation of roles): tried both ways from pipe_min / 8 up.
    if (work >= 2 * bar || (!d->opt.pipe_auto && work >= bar)) return lanes;
    if (d->opt.pipe_auto && d->opt.pipe_min > 0 && work * 8 >= bar) {
        if (either) return lanes;  // scratch for both modes
        const auto it = d->tuned.find(tune_key(d, c, batch));
        const Evaluator::Impl::Tuned t = it == d->tuned.end() ? Evaluator::Impl::Tuned{} : it->second;
        const bool trying = t.n[0] < 2 || t.n[1] < 2;
        const int mode = trying ? (t.n[0] <= t.n[1] ? 0 : 1) : (t.ms[1] < t.ms[0] ? 1 : 0);
        if (trial && trying) *trial = mode;
        return mode ? lanes : 0;
    }
    return 0;
}
static void tune_report(Evaluator::Impl* d, const Circuit& c, size_t batch, int trial, double ms) {
    if (trial < 0 || trial > 1) return;
    if (d->tuned.size() > 256) d->tuned.clear();  // a daemon sees many batch sizes; the table is a cache, not a record
    Evaluator::Impl::Tuned& t = d->tuned[tune_key(d, c, batch)];
    t.ms[trial] = t.n[trial] == 0 ? ms : std::min(t.ms[trial], ms);
    t.n[trial]++;
    d->opt.tuned_evals++;
}
// expressions [first, first + count) of pipeline k of `lanes`: contiguous, sizes differing by at most one, the first ones longer
static void pipe_slice(size_t batch, int lanes, int k, size_t* first, size_t* count) {
    const size_t base = batch / (size_t)lanes, extra = batch % (size_t)lanes;
    *first = (size_t)k * base + std::min<size_t>((size_t)k, extra);
    *count = base + ((size_t)k < extra ? 1 : 0);
}

// Everything an evaluation of `c` over `batch` expressions allocates -- the wire store, the gate / output tables, the scratch
// of its widest level (extracted samples, blind-rotation state, key-switch digits) -- so that the evaluation itself makes no
// allocation (each one is a device-wide synchronisation).  eval_circuit_device calls it; a caller that times its first
// evaluation calls it beforehand (ieache_prepare_batch).
void Evaluator::prepare_circuit(const Circuit& c, size_t batch) {
    begin_call();
    if (batch == 0) return;
    d_->store.reserve_exact(batch * (size_t)c.n_slots, (size_t)d_->K.stride * 4);
    d_->d_gates.reserve_exact(c.gates.size());
    d_->d_outs.reserve_exact(c.outputs.size());
    // rotation items (a MUX gate is two) and gate instances of each level
    std::vector<int64_t> level_items, level_gates;
    int64_t widest = 1, widest_mux_gates = 0;  // per expression: the widest level in items; the most gates of a level that has MUX gates
    bool mux = false;
    for (int32_t L = 1; L <= c.n_levels(); L++) {
        const int64_t ng = c.level_offset[L] - c.level_offset[L - 1], nm = c.n_mux(L);
        level_items.push_back((ng + nm) * (int64_t)batch);
        level_gates.push_back(ng * (int64_t)batch);
        widest = std::max(widest, ng + nm);
        if (nm) widest_mux_gates = std::max(widest_mux_gates, ng);
        mux = mux || nm > 0;
    }
    const int64_t* lg = mux ? level_gates.data() : nullptr;
    if (const int lanes = pipelined(d_, c, batch, nullptr, /*either=*/true)) {
        // pipelines of batch / lanes expressions each (the first ones take the odd ones); where the mode is still being
        // tried out (pipe_auto) the one-stream scratch is reserved as well
        if (!pipelined(d_, c, batch)) reserve_scratch(p_, d_, level_items.data(), level_items.size(), lg);
        ensure_lanes(d_, lanes);
        for (int k = 0; k < lanes; k++) {
            size_t first = 0, count = 0;
            pipe_slice(batch, lanes, k, &first, &count);
            const size_t need = std::min<size_t>(d_->opt.chunk + (mux ? 1 : 0), (size_t)widest * count);
            reserve_lane(p_, d_, d_->lane[k], need, mux ? std::min<size_t>(need, (size_t)widest_mux_gates * count) : 0);
        }
    } else {
        reserve_scratch(p_, d_, level_items.data(), level_items.size(), lg);
    }
}

void Evaluator::eval_circuit_device_once(const Circuit& c, size_t batch, const Torus32* d_in, Torus32* d_out,
                                         EvalStats* stats) {
    begin_call();
    if (batch == 0) return;
    const int32_t stride = d_->K.stride;
    const size_t row_bytes = (size_t)stride * 4;
    prepare_circuit(c, batch);
    if (!c.gates.empty())
        HIP_CHECK(hipMemcpyAsync(d_->d_gates, c.gates.data(), c.gates.size() * sizeof(DevGate), hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipMemcpyAsync(d_->d_outs, c.outputs.data(), c.outputs.size() * sizeof(OutRef), hipMemcpyHostToDevice, stream_));
    Timer tall(stats != nullptr, stream_), tbr(stats != nullptr, stream_), tks(stats != nullptr, stream_);
    tall.mark();
    // inputs -> slots 0..n_inputs-1 of every expression
    HIP_CHECK(hipMemcpy2DAsync(d_->store, (size_t)c.n_slots * row_bytes, d_in, (size_t)c.n_inputs * row_bytes,
                               (size_t)c.n_inputs * row_bytes, batch, hipMemcpyDeviceToDevice, stream_));
    int trial = -1;
    const int pipes = pipelined(d_, c, batch, &trial);
    const auto wall0 = std::chrono::steady_clock::now();
    {
        Fork fork(d_, pipes);  // the other pipelines start when the inputs are in the wire store
        ScopedSet<int32_t> side_by_side(d_->concurrency, std::max(pipes, 1));
        if (pipes) d_->opt.pipelined_evals++;
        for (int32_t L = 1; L <= c.n_levels(); L++) {
            WorkDesc W{};
            W.gates = d_->d_gates;
            W.g0 = c.level_offset[L - 1];
            W.ng = c.level_offset[L] - c.level_offset[L - 1];
            W.nm = c.n_mux(L);
            W.store = d_->store;
            W.n_slots = c.n_slots;
            W.item0 = 0;
            const int64_t ni = (int64_t)W.ng + (int64_t)W.nm;  // rotation items per expression (level_items.h)
            After after;
            after.stage = W.nm > 0 ? After::kMuxCombine : After::kNone;
            if (!pipes) {
                run_items(p_, d_, W, ni * (int64_t)batch, tbr, tks, stats, after);
            } else {
                // items are expression-major (item = expression x ni + position): a contiguous range of expressions is a
                // contiguous range of items that starts and ends at a gate boundary
                for (int k = 0; k < pipes; k++) {
                    size_t first = 0, count = 0;
                    pipe_slice(batch, pipes, k, &first, &count);
                    W.item0 = ni * (int64_t)first;
                    after.lane = k;
                    run_items(p_, d_, W, ni * (int64_t)count, tbr, tks, stats, after);
                }
            }
            if (stats) stats->levels++;
        }
        fork.join();
    }
    const int32_t n_out = (int32_t)c.outputs.size();
    hipLaunchKernelGGL(k_gather_outputs, dim3((unsigned)(batch * n_out)), dim3(128), 0, stream_, d_->d_outs, n_out,
                       d_->store, c.n_slots, d_out, (int64_t)batch, stride, p_.n);
    HIP_CHECK(hipGetLastError());
    tall.mark();
    HIP_CHECK(hipStreamSynchronize(stream_));
    tune_report(d_, c, batch, trial, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count());
    add_times(stats, tall, tbr, tks);
}


// ------------------------------------------------------------------------
// Joint evaluation: several circuits' batches together, level by level (joint_plan.h).

// One step of a joint evaluation: run_items' sibling over the concatenation of the parts' rotation items.  parts[i] is job
// parts[i].job's level, descs[i] its descriptor (item0 = 0: items are numbered within the part).  plan_level, the chunk,
// the level halves on two lanes, plan_blind_rotate, the rotation of roles and the guard all act on the JOINT item count;
// every piece is ONE blind-rotation launch over the shares of the parts it touches (a prologue per share, one sequence of CMux
// slices), one audit decision, and then per share the tail run_items has: k_level_combine where the part's level has MUX gates,
// and a key switch with the part's own descriptor over its rows of `ext`.  Pieces are cut at gate boundaries of the part the
// cut falls in (joint_piece_items), so both rotations of a MUX are in the same piece, lane and `ext`.
static void run_joint_items(const Params& p, Evaluator::Impl* d, const JointPart* parts, const WorkDesc* descs, size_t n_parts, Timer& tbr,
                            Timer& tks, EvalStats* stats) {
    const int64_t items = joint_items(parts, n_parts);
    if (items == 0) return;
    const size_t row_words = (size_t)(d->K.N + 4);
    const LevelPlan pl = plan_level(d, items);
    {
        JointNeeds needs;
        joint_step_needs(parts, n_parts, JointLevelPlan{pl.two_lanes, pl.piece}, &needs);
        reserve_lane(p, d, d->lane[0], needs.items[0], needs.comb[0]);  // in place already: prepare_jobs
        if (needs.items[1]) {
            ensure_lanes(d, 2);
            reserve_lane(p, d, d->lane[1], needs.items[1], needs.comb[1]);
        }
    }
    Fork fork(d, pl.two_lanes ? 2 : 1);
    if (pl.two_lanes) d->opt.overlapped_levels++;
    ScopedSet<bool> halves(d->level_on_two_lanes, pl.two_lanes);
    std::vector<BrPart> sub;
    std::vector<size_t> of;  // sub[q] is a share of parts[of[q]]
    int k = 0;
    for (int64_t done = 0, cnt = 0; done < items; done += cnt, k++) {
        cnt = joint_piece_items(parts, n_parts, done, pl.piece);
        Lane& ln = d->lane[pl.two_lanes ? (k & 1) : 0];
        if (cnt < 1 || (size_t)cnt > ln.ext.items()) throw std::logic_error("joint piece larger than the lane's extracted-sample rows");
        sub.clear();
        of.clear();
        for (size_t i = 0; i < n_parts; i++) {
            const JointShare sh = joint_share(parts, i, done, cnt);
            if (!sh.cnt) continue;
            WorkDesc w = descs[i];
            w.item0 = sh.local0;
            sub.push_back(BrPart{w, sh.cnt});
            of.push_back(i);
        }
        const BrPlan plan = plan_blind_rotate(p, d, ln, cnt);  // by the joint size; once: the launch and the audit see the same choice
        Torus32* ext = ln.ext;
        tbr.mark(ln.stream);
        const int nbr = launch_blind_rotate(d, ln, plan, sub.data(), sub.size(), ext, -1, nullptr);
        tbr.mark(ln.stream);
        HIP_CHECK(hipGetLastError());
        d->br.audit(ln.br, plan, d->opt, ln.stream, sub.data(), sub.size(), ext);
        tks.mark(ln.stream);
        int64_t row = 0, comb_row = 0;  // the share's first row of ext; combined rows handed out so far
        for (size_t q = 0; q < sub.size(); q++) {
            const JointPart& part = parts[of[q]];
            const WorkDesc& w = sub[q].W;
            const Torus32* rows = ext + (size_t)row * row_words;
            WorkDesc wk = w;
            int64_t n_rows = sub[q].cnt;
            if (part.nm > 0) {
                if (!level_gate_boundary(w.item0, part.ng, part.nm) || !level_gate_boundary(w.item0 + sub[q].cnt, part.ng, part.nm))
                    throw std::logic_error("joint piece cut inside a MUX gate");
                const int64_t gate0 = level_gates_before(w.item0, part.ng, part.nm);
                n_rows = level_gates_before(w.item0 + sub[q].cnt, part.ng, part.nm) - gate0;
                if ((size_t)(comb_row + n_rows) > ln.comb.items() || (d->K.N & 3)) throw std::logic_error("combined rows of a joint MUX level not reserved");
                Torus32* dst = ln.comb + (size_t)comb_row * row_words;
                hipLaunchKernelGGL(k_level_combine, dim3((unsigned)n_rows), dim3(256), 0, ln.stream, rows, dst, d->K.N, gate0, w.item0, part.ng, part.nm);
                rows = dst;
                comb_row += n_rows;
                wk.nm = 0;  // the key switch over GATES, as in run_items
                wk.item0 = gate0;
            }
            launch_keyswitch(d, ln, wk, n_rows, rows, nullptr);
            HIP_CHECK(hipGetLastError());
            row += sub[q].cnt;
        }
        tks.mark(ln.stream);
        if (stats) {
            stats->blind_rotate_launches += nbr;
            stats->keyswitch_launches += (int64_t)sub.size();
            stats->chunks++;
        }
    }
    fork.join();
    if (stats) stats->bootstraps += items;
}

namespace {
// the jobs of a call that have a batch, and what joint_plan.h reads of them
struct LiveJobs {
    std::vector<const EvalJob*> jobs;
    std::vector<std::vector<int32_t>> ng, nm;
    std::vector<JointJob> plan;
    LiveJobs(const EvalJob* all, size_t n) {
        for (size_t j = 0; j < n; j++) {
            if (all[j].batch == 0) continue;
            if (!all[j].circuit) throw std::invalid_argument("joint evaluation: a job without a circuit");
            jobs.push_back(&all[j]);
        }
        ng.resize(jobs.size());
        nm.resize(jobs.size());
        for (size_t j = 0; j < jobs.size(); j++) {
            const Circuit& c = *jobs[j]->circuit;
            for (int32_t L = 1; L <= c.n_levels(); L++) {
                ng[j].push_back(c.level_offset[L] - c.level_offset[L - 1]);
                nm[j].push_back(c.n_mux(L));
            }
            plan.push_back(JointJob{c.n_levels(), ng[j].data(), nm[j].data(), (int64_t)jobs[j]->batch});
        }
    }
};
}  // namespace

// Everything a joint evaluation allocates: per job the wire store and the gate / output tables, and the scratch of the
// widest joint step, so that the evaluation itself -- and a warm call -- allocates nothing.
void Evaluator::prepare_jobs(const EvalJob* jobs, size_t n_jobs) {
    begin_call();
    const LiveJobs live(jobs, n_jobs);
    if (live.jobs.empty()) return;
    while (d_->job_store.size() < live.jobs.size()) d_->job_store.emplace_back(new Impl::JobStore);
    for (size_t j = 0; j < live.jobs.size(); j++) {
        const Circuit& c = *live.jobs[j]->circuit;
        Impl::JobStore& js = *d_->job_store[j];
        js.store.reserve_exact(live.jobs[j]->batch * (size_t)c.n_slots, (size_t)d_->K.stride * 4);
        js.d_gates.reserve_exact(std::max<size_t>(c.gates.size(), 1));
        js.d_outs.reserve_exact(std::max<size_t>(c.outputs.size(), 1));
    }
    ScopedSet<int32_t> alone(d_->concurrency, 1);  // no pipelines in a joint evaluation: plan_level sees one stream
    JointNeeds needs;
    std::vector<JointPart> parts(live.jobs.size());
    const int32_t steps = joint_steps(live.plan.data(), live.plan.size());
    for (int32_t s = 1; s <= steps; s++) {
        const size_t n = joint_step_parts(live.plan.data(), live.plan.size(), s, parts.data());
        const LevelPlan pl = plan_level(d_, std::max<int64_t>(joint_items(parts.data(), n), 1));
        joint_step_needs(parts.data(), n, JointLevelPlan{pl.two_lanes, pl.piece}, &needs);
    }
    reserve_lane(p_, d_, d_->lane[0], needs.items[0], needs.comb[0]);
    if (needs.items[1]) {
        ensure_lanes(d_, 2);
        reserve_lane(p_, d_, d_->lane[1], needs.items[1], needs.comb[1]);
    }
}

// A joint call repeats as a WHOLE (run_guarded), and runs on the two-limb kernels from the start when any job's output range
// shares a word with any job's input range: the rule of the single calls, over all pairs.
void Evaluator::eval_jobs_device(const EvalJob* jobs, size_t n_jobs, EvalStats* stats) {
    const size_t stride = (size_t)d_->K.stride;
    bool intact = true;
    for (size_t a = 0; a < n_jobs && intact; a++) {
        if (!jobs[a].batch || !jobs[a].circuit) continue;
        for (size_t b = 0; b < n_jobs && intact; b++) {
            if (!jobs[b].batch || !jobs[b].circuit) continue;
            intact = !overlaps(jobs[a].d_out, jobs[a].batch * jobs[a].circuit->outputs.size() * stride,
                               {{jobs[b].d_in, jobs[b].batch * (size_t)jobs[b].circuit->n_inputs * stride}});
        }
    }
    run_guarded(intact, stats, [&] { eval_jobs_device_once(jobs, n_jobs, stats); });
}

void Evaluator::eval_jobs_device_once(const EvalJob* jobs, size_t n_jobs, EvalStats* stats) {
    begin_call();
    const LiveJobs live(jobs, n_jobs);
    if (live.jobs.empty()) return;
    const int32_t stride = d_->K.stride;
    const size_t row_bytes = (size_t)stride * 4;
    prepare_jobs(jobs, n_jobs);
    for (size_t j = 0; j < live.jobs.size(); j++) {
        const Circuit& c = *live.jobs[j]->circuit;
        Impl::JobStore& js = *d_->job_store[j];
        if (!c.gates.empty())
            HIP_CHECK(hipMemcpyAsync(js.d_gates, c.gates.data(), c.gates.size() * sizeof(DevGate), hipMemcpyHostToDevice, stream_));
        if (!c.outputs.empty())
            HIP_CHECK(hipMemcpyAsync(js.d_outs, c.outputs.data(), c.outputs.size() * sizeof(OutRef), hipMemcpyHostToDevice, stream_));
    }
    Timer tall(stats != nullptr, stream_), tbr(stats != nullptr, stream_), tks(stats != nullptr, stream_);
    tall.mark();
    // every job's inputs -> slots 0..n_inputs-1 of every expression of ITS store, before any output row is written
    for (size_t j = 0; j < live.jobs.size(); j++) {
        const Circuit& c = *live.jobs[j]->circuit;
        if (c.n_inputs > 0)
            HIP_CHECK(hipMemcpy2DAsync(d_->job_store[j]->store, (size_t)c.n_slots * row_bytes, live.jobs[j]->d_in, (size_t)c.n_inputs * row_bytes,
                                       (size_t)c.n_inputs * row_bytes, live.jobs[j]->batch, hipMemcpyDeviceToDevice, stream_));
    }
    {
        ScopedSet<int32_t> alone(d_->concurrency, 1);
        std::vector<JointPart> parts(live.jobs.size());
        std::vector<WorkDesc> descs(live.jobs.size());
        const int32_t steps = joint_steps(live.plan.data(), live.plan.size());
        for (int32_t s = 1; s <= steps; s++) {
            const size_t n = joint_step_parts(live.plan.data(), live.plan.size(), s, parts.data());
            for (size_t i = 0; i < n; i++) {
                const Circuit& c = *live.jobs[parts[i].job]->circuit;
                const Impl::JobStore& js = *d_->job_store[parts[i].job];
                WorkDesc W{};
                W.gates = js.d_gates;
                W.g0 = c.level_offset[s - 1];
                W.ng = parts[i].ng;
                W.nm = parts[i].nm;
                W.store = js.store;
                W.n_slots = c.n_slots;
                W.item0 = 0;
                descs[i] = W;
            }
            run_joint_items(p_, d_, parts.data(), descs.data(), n, tbr, tks, stats);
            if (stats) stats->levels++;
        }
    }
    for (size_t j = 0; j < live.jobs.size(); j++) {
        const Circuit& c = *live.jobs[j]->circuit;
        const int32_t n_out = (int32_t)c.outputs.size();
        if (n_out == 0) continue;
        hipLaunchKernelGGL(k_gather_outputs, dim3((unsigned)(live.jobs[j]->batch * n_out)), dim3(128), 0, stream_, d_->job_store[j]->d_outs, n_out,
                           d_->job_store[j]->store, c.n_slots, live.jobs[j]->d_out, (int64_t)live.jobs[j]->batch, stride, p_.n);
        HIP_CHECK(hipGetLastError());
    }
    tall.mark();
    HIP_CHECK(hipStreamSynchronize(stream_));
    add_times(stats, tall, tbr, tks);
}

void Evaluator::debug_blind_rotate_once(size_t count, const Torus32* d_x, Torus32* d_acc, int32_t steps) {
    begin_call();
    WorkDesc W{};
    W.flat_a = d_x;
    W.flat_b = nullptr;
    W.flat_out = nullptr;
    W.flat_type = -1;
    Lane& ln = d_->lane[0];
    const BrPart part{W, (int64_t)count};
    launch_blind_rotate(d_, ln, plan_blind_rotate(p_, d_, ln, (int64_t)count, steps), &part, 1, nullptr, steps, d_acc);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(stream_));
}

void Evaluator::debug_keyswitch(size_t count, const Torus32* d_u, Torus32* d_out) {
    begin_call();
    // the kernel reads rows of N+4 ints; repack the caller's N+1 rows
    DeviceBuffer<Torus32> tmp;
    tmp.allocate(count, d_->ext_row_bytes());
    HIP_CHECK(hipMemcpy2DAsync(tmp, (size_t)(p_.N + 4) * 4, d_u, (size_t)(p_.N + 1) * 4, (size_t)(p_.N + 1) * 4, count,
                               hipMemcpyDeviceToDevice, stream_));
    WorkDesc W{};
    launch_keyswitch(d_, d_->lane[0], W, (int64_t)count, tmp, d_out);
    hipError_t e = hipGetLastError();
    (void)hipStreamSynchronize(stream_);  // before tmp goes
    HIP_CHECK(e);
}

// ---- the transform probe (fft_probe.h): every refusal is thrown before anything is written to the caller's array ----
static const char* const kProbeRing = "the transform probe covers the 512-point transform of N = 1024, k = 1 contexts only";
static const char* const kProbeNoKey = "this context holds no key form of the 64-lane kernels (br_supported(), br_plan.h)";

void Evaluator::debug_twiddles(int which, double* out) {
    if (!out) throw std::invalid_argument("null argument");
    if (p_.N != 1024 || p_.k != 1) throw std::invalid_argument(kProbeRing);
    if (which < 0 || which > 2) throw std::invalid_argument("debug_twiddles: which must be 0 (blind rotation), 1 (CMux family) or 2 (built in a wave)");
    begin_call();
    const size_t bytes = probe::kTwiddleElems * sizeof(double2);
    DeviceBuffer<double2> built;
    const double2* src = nullptr;
    if (which == 0) {
        src = d_->br.key_forms().twiddles;
        if (!src) throw std::invalid_argument(kProbeNoKey);
    } else if (which == 1) {
        src = d_->cmux.twiddles(stream_);
    } else {
        built.allocate(probe::kTwiddleElems);
        probe::build_twiddles_in_wave(built, stream_);
        src = built;
    }
    HIP_CHECK(hipStreamSynchronize(stream_));
    HIP_CHECK(hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
}

void Evaluator::debug_fft512(int form, size_t count, const double* in, double* out) {
    if (!in || !out) throw std::invalid_argument("null argument");
    if (p_.N != 1024 || p_.k != 1) throw std::invalid_argument(kProbeRing);
    if (const char* why = probe::form_refusal(form, count)) throw std::invalid_argument(why);
    begin_call();
    const double2* tw = d_->br.key_forms().twiddles;
    if (!tw) throw std::invalid_argument(kProbeNoKey);
    const size_t elems = count * probe::kTransformElems;
    DeviceBuffer<double2> d_in, d_out;
    d_in.allocate(elems);
    d_out.allocate(elems);
    HIP_CHECK(hipMemcpy(d_in, in, elems * sizeof(double2), hipMemcpyHostToDevice));
    probe::run_fft512(form, count, d_in, d_out, tw, stream_);  // synchronises the stream
    HIP_CHECK(hipMemcpy(out, d_out, elems * sizeof(double2), hipMemcpyDeviceToHost));
}

void Evaluator::debug_spectrum(int which, size_t first, size_t count, double* out) {
    if (!out) throw std::invalid_argument("null argument");
    if (which < 0 || which > 2) throw std::invalid_argument("debug_spectrum: which must be 0 (two-limb w64), 1 (one-limb w64) or 2 (generic two-limb)");
    if (which != 2 && (p_.N != 1024 || p_.k != 1)) throw std::invalid_argument(kProbeRing);
    const size_t npoly = (size_t)p_.n * p_.kpl() * 2;
    if (count < 1 || first >= npoly || count > npoly - first) throw std::invalid_argument("debug_spectrum: polynomials outside the key's n x 2l x 2");
    begin_call();
    const BlindRotate::KeyForms f = d_->br.key_forms();
    const double2* src = which == 0 ? f.w64 : which == 1 ? f.w64_1 : f.generic;
    if (!src) throw std::invalid_argument(kProbeNoKey);
    const size_t per_poly = which == 1 ? (size_t)512 : which == 0 ? (size_t)1024 : (size_t)p_.N;  // double2: one limb, or two
    HIP_CHECK(hipStreamSynchronize(stream_));
    HIP_CHECK(hipMemcpy(out, src + first * per_poly, count * per_poly * sizeof(double2), hipMemcpyDeviceToHost));
}

}  // namespace ieache
