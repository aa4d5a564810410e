// C ABI (include/ieache.h) over the C++ evaluator.  No exception leaves this file.
#include "../../include/ieache.h"

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "br_plan.h"
#include "circuit.h"
#include "circuit_cache.h"
#include "cloud_run.h"
#include "cmux.h"
#include "codec.h"
#include "daemon.h"
#include "evaluator.h"
#include "fft_probe.h"
#include "group.h"
#include "group_run.h"
#include "linear_plan.h"
#include "mix_plan.h"
#include "pack_plan.h"
#include "project_plan.h"
#include "program.h"
#include "set_calls.h"
#include "tfhe_host.h"

using namespace ieache;

// struct ieache_ctx: group.h (a member of a device group is one)

namespace {
thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
template <class F>
int guarded(F&& f) {
    try {
        g_err.clear();
        return f();
    } catch (const CodecError& e) {
        return fail(IEACHE_EIO, e.what());
    } catch (const std::bad_alloc&) {
        return fail(IEACHE_ENOMEM, "out of host memory");
    } catch (const std::invalid_argument& e) {
        return fail(IEACHE_EINVAL, e.what());
    } catch (const std::exception& e) {
        return fail(IEACHE_ENODEV, e.what());
    } catch (...) {
        return fail(IEACHE_ENODEV, "unknown failure");
    }
}
Params to_params(const ieache_params& a) {
    Params p;
    p.n = a.n;
    p.N = a.N;
    p.k = a.k;
    p.l = a.l;
    p.Bgbit = a.Bgbit;
    p.ks_t = a.ks_t;
    p.ks_basebit = a.ks_basebit;
    p.lwe_alpha_min = a.lwe_alpha_min;
    p.lwe_alpha_max = a.lwe_alpha_max;
    p.tlwe_alpha_min = a.tlwe_alpha_min;
    p.tlwe_alpha_max = a.tlwe_alpha_max;
    return p;
}
void from_params(const Params& p, ieache_params* a) {
    a->n = p.n;
    a->N = p.N;
    a->k = p.k;
    a->l = p.l;
    a->Bgbit = p.Bgbit;
    a->ks_t = p.ks_t;
    a->ks_basebit = p.ks_basebit;
    a->lwe_alpha_min = p.lwe_alpha_min;
    a->lwe_alpha_max = p.lwe_alpha_max;
    a->tlwe_alpha_min = p.tlwe_alpha_min;
    a->tlwe_alpha_max = p.tlwe_alpha_max;
}
void to_stats(const EvalStats& s, ieache_stats* o) {
    if (!o) return;
    o->total_ms = s.total_ms;
    o->blind_rotate_ms = s.blind_rotate_ms;
    o->keyswitch_ms = s.keyswitch_ms;
    o->blind_rotate_launches = s.blind_rotate_launches;
    o->keyswitch_launches = s.keyswitch_launches;
    o->bootstraps = s.bootstraps;
    o->levels = s.levels;
    o->chunks = s.chunks;
}
// A kernel dereferencing a host or stray address faults the GPU (and can take the node's other GPUs with it), so
// the device-pointer entry points refuse anything the runtime does not know as device-accessible memory.
void require_device_pointer(const void* ptr, const char* name) {
    hipPointerAttribute_t attr;
    const hipError_t e = hipPointerGetAttributes(&attr, ptr);
    if (e != hipSuccess) (void)hipGetLastError();
    if (e != hipSuccess || (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged && attr.type != hipMemoryTypeUnified))
        throw std::invalid_argument(std::string(name) + " is not a device pointer");
}
// ... for every pointer argument of an entry point; an empty call launches nothing and names no memory
struct DevArg {
    const void* ptr;
    const char* name;
    bool optional = false;  // null is allowed
};
void require_device_pointers(size_t count, std::initializer_list<DevArg> args) {
    if (!count) return;
    for (const DevArg& a : args)
        if (a.ptr || !a.optional) require_device_pointer(a.ptr, a.name);
}
// Runs `body` with the evaluator's statistics record -- null when the caller wants none -- and hands the caller its copy.
template <class F>
int with_stats(ieache_stats* stats, F&& body) {
    EvalStats st;
    body(stats ? &st : nullptr);
    to_stats(st, stats);
    return 0;
}
// What can be judged of a programmable bootstrap's arguments without the context, in the order the entry points report it:
// the message of the first failing check, or null.  The host and the device form share them.
const char* pbs_args_error(int flags, int32_t n_polys, const int32_t* test_polys) {
    if (flags & ~(IEACHE_PBS_NO_KEYSWITCH | IEACHE_PBS_TLWE_POLYS | IEACHE_PBS_ACCUMULATOR)) return "pbs: unknown flag";
    if (n_polys < 1) return "pbs: n_polys must be at least 1";
    if (!test_polys) return "pbs: null test polynomial table";
    return nullptr;
}
const char* pbs_multi_args_error(int flags, int32_t n_polys, const int32_t* test_polys, int32_t n_factors, const int32_t* factors) {
    if (flags & IEACHE_PBS_ACCUMULATOR) return "pbs_multi: IEACHE_PBS_ACCUMULATOR is a flag of ieache_pbs: a multi-output call has no accumulator output";
    if (flags & ~(IEACHE_PBS_NO_KEYSWITCH | IEACHE_PBS_TLWE_POLYS)) return "pbs_multi: unknown flag";
    if (n_polys < 1) return "pbs_multi: n_polys must be at least 1";
    if (!test_polys) return "pbs_multi: null test polynomial table";
    if (n_factors < 1 || n_factors > IEACHE_PBS_MULTI_MAX_FACTORS) return "pbs_multi: n_factors must be 1 .. 64";
    if (!factors) return "pbs_multi: null factor table";
    return nullptr;
}
// Host forms only: the device form cannot read the indices, and the kernel clamps.  -> the message, or empty
std::string poly_of_error(const char* call, const int32_t* poly_of, size_t count, int32_t n_polys) {
    for (size_t i = 0; poly_of && i < count; i++)
        if (poly_of[i] < 0 || poly_of[i] >= n_polys)
            return std::string(call) + ": poly_of[" + std::to_string(i) + "] = " + std::to_string(poly_of[i]) + " is outside [0, n_polys)";
    return std::string();
}

const char* const kUnsupported = "unsupported circuit kind/bits";
// The cached circuit a context evaluates `batch` expressions with.  Callers hold the pointer for the call: the evaluator keeps
// no Circuit beyond it.  IEACHE_LEVEL_CAP is a measurement aid: it forces a level width (and with it the balanced schedule).
CircuitCache::Ptr get_circuit(ieache_ctx* ctx, int kind, int bits, size_t batch) {
    const char* forced = getenv("IEACHE_LEVEL_CAP");
    return ctx->circuits.select(kind, bits, ctx->fold, (int64_t)batch, ctx->eval->resident_gates(), ctx->eval->resident_gates_two_wave(),
                                ctx->level_quantum, forced ? atoi(forced) : 0);
}
// ---- The argument checks of the host-buffer entry points: 0, or the code after fail().  Each context form opens with its
// check; the group form of the same call (section 2b) makes it once, on member 0 and the caller's whole arrays, before any
// thread starts. ----
int check_rows(std::initializer_list<const void*> pointers) {  // the context (or group member) and every row array
    for (const void* p : pointers)
        if (!p) return fail(IEACHE_EINVAL, "null argument");
    return 0;
}
// ... -> *c: the circuit the context evaluates `batch` expressions with
int check_prepare(ieache_ctx* ctx, int kind, int bits, size_t batch, CircuitCache::Ptr* c) {
    if (!ctx) return fail(IEACHE_EINVAL, "null argument");
    *c = get_circuit(ctx, kind, bits, batch);
    return *c ? 0 : fail(IEACHE_EINVAL, kUnsupported);
}
int check_batch(ieache_ctx* ctx, int kind, int bits, size_t batch, const int32_t* in_lwe, const int32_t* out_lwe, CircuitCache::Ptr* c) {
    if (const int rc = check_rows({ctx, in_lwe, out_lwe})) return rc;
    return check_prepare(ctx, kind, bits, batch, c);
}
bool bad_gate2(int gate_type) { return gate_type < 0 || gate_type >= GATE_TYPES || gate_type == GATE_MUX; }
const char* const kNotGate3 = "not a three-input gate type (IEACHE_GATE_MAJ3 / IEACHE_GATE_XOR3)";
int check_gates(const ieache_ctx* ctx, int gate_type, const int32_t* a, const int32_t* b, const int32_t* out) {
    if (const int rc = check_rows({ctx, a, b, out})) return rc;
    return bad_gate2(gate_type) ? fail(IEACHE_EINVAL, "unknown gate type") : 0;
}
int check_gates3(const ieache_ctx* ctx, int gate_type, const int32_t* a, const int32_t* b, const int32_t* c, const int32_t* out) {
    if (!is_gate3(gate_type)) return fail(IEACHE_EINVAL, kNotGate3);
    return check_rows({ctx, a, b, c, out});
}
// what can be judged without the context comes first
int check_pbs(const ieache_ctx* ctx, size_t count, const int32_t* x, const int32_t* test_polys, int32_t n_polys, const int32_t* poly_of,
              const int32_t* out, int flags) {
    if (const char* e = pbs_args_error(flags, n_polys, test_polys)) return fail(IEACHE_EINVAL, e);
    const std::string bad_index = poly_of_error("pbs", poly_of, count, n_polys);
    if (!bad_index.empty()) return fail(IEACHE_EINVAL, bad_index);
    return check_rows({ctx, x, out});
}
int check_pbs_multi(const ieache_ctx* ctx, size_t count, const int32_t* x, const int32_t* test_polys, int32_t n_polys, const int32_t* poly_of,
                    const int32_t* factors, int32_t n_factors, const int32_t* out, int flags) {
    if (const char* e = pbs_multi_args_error(flags, n_polys, test_polys, n_factors, factors)) return fail(IEACHE_EINVAL, e);
    const std::string bad_index = poly_of_error("pbs_multi", poly_of, count, n_polys);
    if (!bad_index.empty()) return fail(IEACHE_EINVAL, bad_index);
    return check_rows({ctx, x, out});
}
// f(circuit) on a throw-away build of the circuit, or the refusal
template <class F>
int with_circuit(int kind, int bits, int fold_constants, int level_cap, F&& f) {
    Circuit c;
    if (!build_circuit(kind, bits, &c, true, fold_constants != 0, level_cap)) return fail(IEACHE_EINVAL, kUnsupported);
    return f(c);
}
// the context is owned by a unique_ptr until it is handed to the caller, so a throwing key load
// (or Evaluator constructor) releases it
template <class Load>
ieache_ctx* make_ctx(const Params& p, int device, Load&& load) {
    std::unique_ptr<ieache_ctx> ctx(new ieache_ctx);
    ctx->eval.reset(new Evaluator(p, device));
    load(*ctx->eval);
    return ctx.release();
}
void fill_info(const Circuit& c, bool fold, ieache_circuit_info* out) {
    out->n_inputs = c.n_inputs;
    out->n_outputs = (int32_t)c.outputs.size();
    out->n_slots = c.n_slots;
    out->depth = c.depth;
    out->max_width = c.max_width;
    out->bootstraps = c.n_bootstraps;
    out->n_and = c.n_and;
    out->n_xor = c.n_xor;
    out->sched_max_width = c.sched_max_width;
    out->folded = fold ? 1 : 0;
    out->reference_bootstraps = c.n_reference_bootstraps;
    out->sched_levels = c.n_levels();
    out->level_cap = 0;
}
}  // namespace

extern "C" {

const char* ieache_version(void) { return "ieache-amd 0.2 (gfx950)"; }
const char* ieache_last_error(void) { return g_err.c_str(); }
const char* ieache_last_key_layout(void) { return last_key_layout().c_str(); }

int ieache_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void ieache_default_params(ieache_params* out) {
    if (out) from_params(Params{}, out);
}

int ieache_cloud_run(const char* workdir) {
    // the reference binary takes no arguments, so the GPU is chosen through the environment
    const char* dev = getenv("IEACHE_DEVICE");
    return guarded([&] { return cloud_run(workdir ? workdir : ".", nullptr, nullptr, dev ? atoi(dev) : 0); });
}

ieache_ctx* ieache_ctx_create(const char* cloud_key_path, int device) {
    ieache_ctx* ctx = nullptr;
    const int rc = guarded([&] {
        if (!cloud_key_path) return fail(IEACHE_EINVAL, "null path");
        CloudKeyData ck;
        load_cloud_key(cloud_key_path, &ck);
        ctx = make_ctx(ck.p, device, [&](Evaluator& e) { e.load_keys_host(ck.bk.data(), ck.ksk.data()); });
        return 0;
    });
    return rc == 0 ? ctx : nullptr;
}

ieache_ctx* ieache_ctx_create_raw(const ieache_params* p, const int32_t* bk, const int32_t* ksk, int device) {
    ieache_ctx* ctx = nullptr;
    const int rc = guarded([&] {
        if (!p || !bk || !ksk) return fail(IEACHE_EINVAL, "null argument");
        ctx = make_ctx(to_params(*p), device, [&](Evaluator& e) { e.load_keys_host(bk, ksk); });
        return 0;
    });
    return rc == 0 ? ctx : nullptr;
}

ieache_ctx* ieache_ctx_create_device(const ieache_params* p, const int32_t* d_bk, const int32_t* d_ksk, int device) {
    ieache_ctx* ctx = nullptr;
    const int rc = guarded([&] {
        if (!p || !d_bk || !d_ksk) return fail(IEACHE_EINVAL, "null argument");
        ctx = make_ctx(to_params(*p), device, [&](Evaluator& e) {
            require_device_pointer(d_bk, "d_bk");
            require_device_pointer(d_ksk, "d_ksk");
            e.load_keys_device(d_bk, d_ksk);
        });
        return 0;
    });
    return rc == 0 ? ctx : nullptr;
}

void ieache_ctx_destroy(ieache_ctx* ctx) {
    try {
        delete ctx;
    } catch (...) {
    }
}

int ieache_ctx_params(const ieache_ctx* ctx, ieache_params* out) {
    if (!ctx || !out) return fail(IEACHE_EINVAL, "null argument");
    from_params(ctx->eval->params(), out);
    return 0;
}

int ieache_lwe_stride(const ieache_ctx* ctx) { return ctx ? ctx->eval->params().lwe_stride() : IEACHE_EINVAL; }

void* ieache_ctx_stream(const ieache_ctx* ctx) { return ctx ? (void*)ctx->eval->stream() : nullptr; }

int ieache_ctx_cloud_run(ieache_ctx* ctx, const char* workdir) {
    if (!ctx) return fail(IEACHE_EINVAL, "null context");
    return guarded([&] { return cloud_run(workdir ? workdir : ".", ctx->eval.get(), nullptr, ctx->eval->device()); });
}

int ieache_ctx_set_chunk(ieache_ctx* ctx, int64_t items) {
    if (!ctx || items < 1) return fail(IEACHE_EINVAL, "bad chunk");
    ctx->eval->set_chunk((size_t)items);
    return 0;
}

int ieache_ctx_force_generic(ieache_ctx* ctx, int on) {
    if (!ctx) return fail(IEACHE_EINVAL, "null context");
    ctx->eval->set_force_generic(on != 0);
    return 0;
}

int ieache_ctx_wait_stream(ieache_ctx* ctx, void* hip_stream) {
    if (!ctx) return fail(IEACHE_EINVAL, "null context");
    return guarded([&] {
        ctx->eval->wait_for_stream((hipStream_t)hip_stream);
        return 0;
    });
}

int ieache_ctx_set_option(ieache_ctx* ctx, const char* name, int64_t value) {
    if (!ctx || !name) return fail(IEACHE_EINVAL, "null argument");
    if (std::string(name) == "level_quantum") {
        if (value != 0 && value != 1) return fail(IEACHE_EINVAL, "level_quantum takes 0 or 1");
        ctx->level_quantum = value != 0;
        return 0;
    }
    if (std::string(name) == "fold_constants") {
        if (value != 0 && value != 1) return fail(IEACHE_EINVAL, "fold_constants takes 0 or 1");
        ctx->fold = value != 0;
        return 0;
    }
    if (!ctx->eval->set_option(name, value)) return fail(IEACHE_EINVAL, std::string("unknown option or bad value: ") + name);
    return 0;
}

int ieache_ctx_fft_guard(const ieache_ctx* ctx, double* max_deviation, int64_t* reruns) {
    if (!ctx) return fail(IEACHE_EINVAL, "null context");
    if (max_deviation) *max_deviation = ctx->eval->fft_guard_max();
    if (reruns) *reruns = ctx->eval->fft_guard_reruns();
    return 0;
}

int ieache_ctx_get_option(const ieache_ctx* ctx, const char* name, int64_t* value) {
    if (!ctx || !name) return fail(IEACHE_EINVAL, "null argument");
    if (std::string(name) == "level_quantum") {
        if (value) *value = ctx->level_quantum ? 1 : 0;
        return 0;
    }
    if (std::string(name) == "fold_constants") {
        if (value) *value = ctx->fold ? 1 : 0;
        return 0;
    }
    if (!ctx->eval->get_option(name, value)) return fail(IEACHE_EINVAL, std::string("unknown option: ") + name);
    return 0;
}

int ieache_ctx_fft_audit(const ieache_ctx* ctx, int64_t* audits, int64_t* gates_compared, int64_t* mismatches) {
    if (!ctx) return fail(IEACHE_EINVAL, "null context");
    ctx->eval->fft_audit_counts(audits, gates_compared, mismatches);
    return 0;
}

const char* ieache_ctx_kernel_variant(const ieache_ctx* ctx) {
    if (!ctx) return "";
    const_cast<ieache_ctx*>(ctx)->variant = ctx->eval->kernel_variant();
    return ctx->variant.c_str();
}

const char* ieache_ctx_kernel_for_launch(const ieache_ctx* ctx, int64_t gates) {
    if (!ctx) return "";
    const_cast<ieache_ctx*>(ctx)->variant = ctx->eval->kernel_for_launch(gates);
    return ctx->variant.c_str();
}

int ieache_circuit_info_get_ex(int kind, int bits, int fold_constants, ieache_circuit_info* out) {
    return guarded([&] {
        if (!out) return fail(IEACHE_EINVAL, "null argument");
        return with_circuit(kind, bits, fold_constants, 0, [&](const Circuit& c) {
            fill_info(c, fold_constants != 0, out);
            return 0;
        });
    });
}
// The 0.1 entry point: its callers were compiled against the 56-byte struct (through `folded`), so it writes exactly that
// prefix.  The fields added since are reached through the _ex / _cap entry points, which take the current struct.
int ieache_circuit_info_get(int kind, int bits, ieache_circuit_info* out) {
    if (!out) return fail(IEACHE_EINVAL, "null argument");
    ieache_circuit_info full;
    memset(&full, 0, sizeof full);  // padding included: the prefix is copied bytewise
    const int rc = ieache_circuit_info_get_ex(kind, bits, 0, &full);
    if (rc == 0) memcpy(out, &full, IEACHE_CIRCUIT_INFO_V01_BYTES);
    return rc;
}

int ieache_ctx_circuit_level_cap(const ieache_ctx* ctx, int kind, int bits, int64_t batch) {
    return guarded([&] {
        if (!ctx) return fail(IEACHE_EINVAL, "null context");
        return with_circuit(kind, bits, ctx->fold, 0, [&](const Circuit& c) {
            return (int)circuit_level_cap(c, batch, ctx->eval->resident_gates(), ctx->eval->resident_gates_two_wave());
        });
    });
}

int ieache_circuit_level_cap(int kind, int bits, int fold_constants, int64_t batch, int resident_workgroups) {
    return guarded([&] {
        return with_circuit(kind, bits, fold_constants, 0, [&](const Circuit& c) { return (int)circuit_level_cap(c, batch, resident_workgroups); });
    });
}

int ieache_circuit_info_get_cap(int kind, int bits, int fold_constants, int level_cap, ieache_circuit_info* out) {
    return guarded([&] {
        if (!out || level_cap < 0) return fail(IEACHE_EINVAL, "bad argument");
        return with_circuit(kind, bits, fold_constants, level_cap, [&](const Circuit& c) {
            fill_info(c, fold_constants != 0, out);
            out->level_cap = c.balanced_schedule ? level_cap : 0;
            return 0;
        });
    });
}

int ieache_circuit_simulate_cap(int kind, int bits, int fold_constants, int level_cap, const uint8_t* in_bits, uint8_t* out_bits) {
    return guarded([&] {
        if (!in_bits || !out_bits || level_cap < 0) return fail(IEACHE_EINVAL, "bad argument");
        return with_circuit(kind, bits, fold_constants, level_cap, [&](const Circuit& c) {
            simulate_circuit(c, in_bits, out_bits);
            return 0;
        });
    });
}

int ieache_circuit_simulate_ex(int kind, int bits, int fold_constants, const uint8_t* in_bits, uint8_t* out_bits) {
    return guarded([&] {
        if (!in_bits || !out_bits) return fail(IEACHE_EINVAL, "null argument");
        return with_circuit(kind, bits, fold_constants, 0, [&](const Circuit& c) {
            simulate_circuit(c, in_bits, out_bits);
            return 0;
        });
    });
}
int ieache_circuit_simulate(int kind, int bits, const uint8_t* in_bits, uint8_t* out_bits) {
    return ieache_circuit_simulate_ex(kind, bits, 0, in_bits, out_bits);
}

int ieache_eval_batch(ieache_ctx* ctx, int kind, int bits, size_t batch, const int32_t* in_lwe, int32_t* out_lwe,
                      ieache_stats* stats) {
    return guarded([&] {
        CircuitCache::Ptr c;
        if (const int rc = check_batch(ctx, kind, bits, batch, in_lwe, out_lwe, &c)) return rc;
        return with_stats(stats, [&](EvalStats* st) { eval_circuit_host(*ctx->eval, *c, batch, in_lwe, out_lwe, st); });
    });
}

int ieache_eval_batch_device(ieache_ctx* ctx, int kind, int bits, size_t batch, const int32_t* d_in, int32_t* d_out,
                             ieache_stats* stats) {
    return guarded([&] {
        if (!ctx || !d_in || !d_out) return fail(IEACHE_EINVAL, "null argument");
        const CircuitCache::Ptr c = get_circuit(ctx, kind, bits, batch);
        if (!c) return fail(IEACHE_EINVAL, kUnsupported);
        require_device_pointers(batch, {{d_in, "d_in"}, {d_out, "d_out"}});
        return with_stats(stats, [&](EvalStats* st) { ctx->eval->eval_circuit_device(*c, batch, d_in, d_out, st); });
    });
}

int ieache_prepare_batch(ieache_ctx* ctx, int kind, int bits, size_t batch) {
    return guarded([&] {
        CircuitCache::Ptr c;
        if (const int rc = check_prepare(ctx, kind, bits, batch, &c)) return rc;
        ctx->eval->prepare_circuit(*c, batch);
        return 0;
    });
}

// ---- caller-defined netlists: a compiled Circuit behind an opaque handle (host only) ----
struct ieache_netlist {
    Circuit circuit;
    RecordedNetlist recorded;  // the gate list as recorded: what ieache_netlist_export gives
};

ieache_netlist* ieache_netlist_create(int32_t n_inputs, const ieache_net_gate* gates, size_t n_gates, const int32_t* outputs,
                                      size_t n_outputs, int flags) {
    static_assert(sizeof(ieache_net_gate) == sizeof(NetGate), "ieache_net_gate is circuit.h's NetGate");
    ieache_netlist* nl = nullptr;
    guarded([&] {
        if (flags & ~IEACHE_NETLIST_BALANCED) return fail(IEACHE_EINVAL, "netlist: unknown flag");
        std::unique_ptr<ieache_netlist> made(new ieache_netlist);
        made->circuit = build_netlist(n_inputs, reinterpret_cast<const NetGate*>(gates), n_gates, outputs, n_outputs,
                                      (flags & IEACHE_NETLIST_BALANCED) != 0, &made->recorded);
        nl = made.release();
        return 0;
    });
    return nl;
}

void ieache_netlist_destroy(ieache_netlist* nl) { delete nl; }

// ---- 3d. word programs: compiled to the same handle (program.h) ----
ieache_netlist* ieache_program_compile(const ieache_word_instr* instrs, size_t n_instrs, const ieache_word_arg* args, size_t n_args,
                                       const uint32_t* const_words, size_t n_const_words, const int32_t* outputs, size_t n_outputs,
                                       int flags) {
    static_assert(sizeof(ieache_word_instr) == sizeof(WordInstr) && sizeof(ieache_word_arg) == sizeof(WordArg),
                  "ieache_word_instr / ieache_word_arg are program.h's WordInstr / WordArg");
    static_assert(IEACHE_WOP_INPUT == WOP_INPUT && IEACHE_WOP_CONST == WOP_CONST && IEACHE_WOP_ZEXT == WOP_ZEXT && IEACHE_WOP_SLICE == WOP_SLICE &&
                      IEACHE_WOP_SHL == WOP_SHL && IEACHE_WOP_NOT == WOP_NOT && IEACHE_WOP_CONCAT == WOP_CONCAT && IEACHE_WOP_AND == WOP_AND &&
                      IEACHE_WOP_OR == WOP_OR && IEACHE_WOP_XOR == WOP_XOR && IEACHE_WOP_ANDBIT == WOP_ANDBIT && IEACHE_WOP_ADD == WOP_ADD &&
                      IEACHE_WOP_SUB == WOP_SUB && IEACHE_WOP_RSUB == WOP_RSUB && IEACHE_WOP_MUL == WOP_MUL && IEACHE_WOP_SUM == WOP_SUM &&
                      IEACHE_WOP_LT == WOP_LT && IEACHE_WOP_EQ == WOP_EQ && IEACHE_WOP_SELECT == WOP_SELECT && WOP_COUNT == IEACHE_WOP_SELECT + 1,
                  "program.h's opcodes and include/ieache.h's IEACHE_WOP_* disagree");
    static_assert(IEACHE_FAMILY_REFERENCE == FAMILY_REFERENCE && IEACHE_FAMILY_FULL_ADDER == FAMILY_FULL_ADDER && IEACHE_FAMILY_KOGGE_STONE == FAMILY_KOGGE_STONE &&
                      IEACHE_FAMILY_CARRY_SAVE == FAMILY_CARRY_SAVE && IEACHE_PROGRAM_FOLD == kProgramFold &&
                      IEACHE_NETLIST_BALANCED == kProgramBalanced && IEACHE_WORD_MAX_WIDTH == kMaxWordWidth,
                  "program.h and include/ieache.h's section 3d disagree");
    ieache_netlist* nl = nullptr;
    guarded([&] {
        std::unique_ptr<ieache_netlist> made(new ieache_netlist);
        CompiledProgram p = compile_program(reinterpret_cast<const WordInstr*>(instrs), n_instrs, reinterpret_cast<const WordArg*>(args), n_args,
                                            const_words, n_const_words, outputs, n_outputs, flags);
        made->circuit = std::move(p.circuit);
        made->recorded = std::move(p.recorded);
        nl = made.release();
        return 0;
    });
    return nl;
}

int64_t ieache_netlist_export(const ieache_netlist* nl, ieache_net_gate* gates, size_t cap, int32_t* outputs, size_t out_cap) {
    if (!nl) return fail(IEACHE_EINVAL, "null argument");
    const RecordedNetlist& r = nl->recorded;
    if (gates && cap >= r.gates.size() && !r.gates.empty()) memcpy(gates, r.gates.data(), r.gates.size() * sizeof(NetGate));
    if (outputs && out_cap >= r.outputs.size() && !r.outputs.empty()) memcpy(outputs, r.outputs.data(), r.outputs.size() * sizeof(int32_t));
    return (int64_t)r.gates.size();
}

int ieache_netlist_info(const ieache_netlist* nl, ieache_circuit_info* out, int64_t gates_by_type[IEACHE_GATE_TYPES]) {
    return guarded([&] {
        if (!nl || !out) return fail(IEACHE_EINVAL, "null argument");
        fill_info(nl->circuit, false, out);
        if (gates_by_type)
            for (int t = 0; t < GATE_TYPES; t++) gates_by_type[t] = nl->circuit.n_by_type[t];
        return 0;
    });
}

int64_t ieache_netlist_gate_count(const ieache_netlist* nl, int gate_type) {
    if (!nl) return fail(IEACHE_EINVAL, "null argument");
    const int64_t n = nl->circuit.count_of(gate_type);
    return n < 0 ? fail(IEACHE_EINVAL, "unknown gate type") : n;
}

int64_t ieache_circuit_gate_count(int kind, int bits, int fold_constants, int gate_type) {
    int64_t n = 0;
    const int rc = guarded([&] {
        return with_circuit(kind, bits, fold_constants, 0, [&](const Circuit& c) {
            n = c.count_of(gate_type);
            return n < 0 ? fail(IEACHE_EINVAL, "unknown gate type") : 0;
        });
    });
    return rc != 0 ? rc : n;
}

int ieache_netlist_simulate(const ieache_netlist* nl, const uint8_t* in_bits, uint8_t* out_bits) {
    return guarded([&] {
        if (!nl || !in_bits || !out_bits) return fail(IEACHE_EINVAL, "null argument");
        simulate_circuit(nl->circuit, in_bits, out_bits);
        return 0;
    });
}

int ieache_prepare_netlist(ieache_ctx* ctx, const ieache_netlist* nl, size_t batch) {
    return guarded([&] {
        if (const int rc = check_rows({ctx, nl})) return rc;
        ctx->eval->prepare_circuit(nl->circuit, batch);
        return 0;
    });
}

int ieache_eval_netlist(ieache_ctx* ctx, const ieache_netlist* nl, size_t batch, const int32_t* in_lwe, int32_t* out_lwe,
                        ieache_stats* stats) {
    return guarded([&] {
        if (const int rc = check_rows({ctx, nl, in_lwe, out_lwe})) return rc;
        return with_stats(stats, [&](EvalStats* st) { eval_circuit_host(*ctx->eval, nl->circuit, batch, in_lwe, out_lwe, st); });
    });
}

int ieache_eval_netlist_device(ieache_ctx* ctx, const ieache_netlist* nl, size_t batch, const int32_t* d_in, int32_t* d_out,
                               ieache_stats* stats) {
    return guarded([&] {
        if (!ctx || !nl || !d_in || !d_out) return fail(IEACHE_EINVAL, "null argument");
        require_device_pointers(batch, {{d_in, "d_in"}, {d_out, "d_out"}});
        return with_stats(stats, [&](EvalStats* st) { ctx->eval->eval_circuit_device(nl->circuit, batch, d_in, d_out, st); });
    });
}

// ---- 3c. several circuits' batches in one call (Evaluator::eval_jobs_device, joint_plan.h) ----
extern "C++" {
namespace {
// The jobs of a call resolved to circuits, or the refusal: everything that can fail is judged here, before anything is
// launched, staged or written.  What needs no context comes first.  held: the cached circuits, kept for the call.
struct ResolvedJobs {
    std::vector<EvalJob> jobs;  // one per caller's job, circuit null and batch 0 where the job is skipped
    std::vector<CircuitCache::Ptr> held;
};
int resolve_jobs(ieache_ctx* ctx, const ieache_job* jobs, size_t n_jobs, bool need_rows, ResolvedJobs* r) {
    if (n_jobs && !jobs) return fail(IEACHE_EINVAL, "null argument");
    for (size_t j = 0; need_rows && j < n_jobs; j++)
        if (jobs[j].batch && (!jobs[j].in_lwe || !jobs[j].out_lwe)) return fail(IEACHE_EINVAL, "job " + std::to_string(j) + ": null argument");
    if (!ctx) return fail(IEACHE_EINVAL, "null argument");
    r->jobs.assign(n_jobs, EvalJob{});
    for (size_t j = 0; j < n_jobs; j++) {
        if (!jobs[j].batch) continue;
        const Circuit* c = nullptr;
        if (jobs[j].netlist) {
            c = &jobs[j].netlist->circuit;
        } else {
            // the base circuit: a level cap is chosen for ONE batch filling rounds alone
            const CircuitCache::Ptr held = ctx->circuits.fetch(jobs[j].kind, jobs[j].bits, ctx->fold, 0);
            if (!held) return fail(IEACHE_EINVAL, "job " + std::to_string(j) + ": " + kUnsupported);
            r->held.push_back(held);
            c = held.get();
        }
        r->jobs[j].circuit = c;
        r->jobs[j].batch = jobs[j].batch;
    }
    return 0;
}
}  // namespace
}  // extern "C++"

int ieache_prepare_jobs(ieache_ctx* ctx, const ieache_job* jobs, size_t n_jobs) {
    return guarded([&] {
        ResolvedJobs r;
        if (const int rc = resolve_jobs(ctx, jobs, n_jobs, false, &r)) return rc;
        ctx->eval->prepare_jobs(r.jobs.data(), r.jobs.size());
        return 0;
    });
}

int ieache_eval_jobs_device(ieache_ctx* ctx, const ieache_job* jobs, size_t n_jobs, ieache_eval_stats* stats) {
    return guarded([&] {
        ResolvedJobs r;
        if (const int rc = resolve_jobs(ctx, jobs, n_jobs, true, &r)) return rc;
        for (size_t j = 0; j < n_jobs; j++) {
            require_device_pointers(jobs[j].batch, {{jobs[j].in_lwe, "in_lwe"}, {jobs[j].out_lwe, "out_lwe"}});
            r.jobs[j].d_in = jobs[j].in_lwe;
            r.jobs[j].d_out = jobs[j].out_lwe;
        }
        return with_stats(stats, [&](EvalStats* st) { ctx->eval->eval_jobs_device(r.jobs.data(), r.jobs.size(), st); });
    });
}

int ieache_eval_jobs(ieache_ctx* ctx, const ieache_job* jobs, size_t n_jobs, ieache_eval_stats* stats) {
    return guarded([&] {
        ResolvedJobs r;
        if (const int rc = resolve_jobs(ctx, jobs, n_jobs, true, &r)) return rc;
        std::vector<HostJob> host(n_jobs);
        for (size_t j = 0; j < n_jobs; j++)
            if (r.jobs[j].batch) host[j] = HostJob{r.jobs[j].circuit, r.jobs[j].batch, jobs[j].in_lwe, jobs[j].out_lwe};
        return with_stats(stats, [&](EvalStats* st) { eval_jobs_host(*ctx->eval, host.data(), host.size(), st); });
    });
}

namespace {
// host rows (n+1) <-> device rows (stride)
struct DevRows {
    Torus32* p = nullptr;
    size_t rows, stride;
    DevRows(size_t r, size_t s) : rows(r), stride(s) {
        HIP_CHECK(hipMalloc(&p, rows * stride * 4 + 16));
        HIP_CHECK(hipMemset(p, 0, rows * stride * 4 + 16));
    }
    ~DevRows() { (void)hipFree(p); }
    void upload(const int32_t* h, size_t width) {
        HIP_CHECK(hipMemcpy2D(p, stride * 4, h, width * 4, width * 4, rows, hipMemcpyHostToDevice));
    }
    void download(int32_t* h, size_t width) {
        HIP_CHECK(hipMemcpy2D(h, width * 4, p, stride * 4, width * 4, rows, hipMemcpyDeviceToHost));
    }
};
// the same on the evaluator's kept staging rows (Evaluator::staging): what the host forms of the flat calls use, so that a
// warm call allocates nothing
struct StagedRows {
    Torus32* p;
    size_t rows, stride;
    // rows for results
    StagedRows(Evaluator& ev, StageSlot slot, size_t r, size_t s) : p(ev.staging(slot, r * s * 4)), rows(r), stride(s) {}
    // an input: `width` words of every host row uploaded.  A null `h` (an optional argument) stages no rows; p is then null.
    StagedRows(Evaluator& ev, StageSlot slot, size_t r, size_t s, const int32_t* h, size_t width) : StagedRows(ev, slot, h ? r : 0, s) {
        if (!h) p = nullptr;
        if (rows) HIP_CHECK(hipMemcpy2D(p, stride * 4, h, width * 4, width * 4, rows, hipMemcpyHostToDevice));
    }
    void download(int32_t* h, size_t width) {
        if (rows) HIP_CHECK(hipMemcpy2D(h, width * 4, p, stride * 4, width * 4, rows, hipMemcpyDeviceToHost));
    }
};
// What the host form of a flat call stages with: the context's device current, and operand / result rows of lwe_stride() words.
struct HostCall {
    Evaluator& ev;
    const Params& p;
    size_t count;
    HostCall(ieache_ctx* ctx, size_t n) : ev(*ctx->eval), p(ev.params()), count(n) { HIP_CHECK(hipSetDevice(ev.device())); }
    StagedRows operand(StageSlot slot, const int32_t* h) { return StagedRows(ev, slot, count, (size_t)p.lwe_stride(), h, (size_t)p.n + 1); }
    // test polynomials / factors: `rows` whole polynomials; indices / bias: `rows` single words, optional
    StagedRows polys(StageSlot slot, const int32_t* h, size_t rows) { return StagedRows(ev, slot, rows, (size_t)p.N, h, (size_t)p.N); }
    StagedRows words(StageSlot slot, const int32_t* h, size_t rows) { return StagedRows(ev, slot, rows, 1, h, 1); }
    StagedRows results(size_t rows, bool extracted = false) {
        return StagedRows(ev, kStageOut, rows, extracted ? (size_t)ev.extract_stride() : (size_t)p.lwe_stride());
    }
    // key-switched rows carry n + 1 words, extracted samples N + 1
    void download(StagedRows& out, int32_t* h, bool extracted = false) { out.download(h, extracted ? (size_t)p.N + 1 : (size_t)p.n + 1); }
    // a table of a programmable bootstrap: n_polys polynomials, or (IEACHE_PBS_TLWE_POLYS) n_polys samples of two each, packed
    StagedRows table(const int32_t* h, int32_t n_polys, int flags) {
        return polys(kStageTestPolys, h, (size_t)n_polys * ((flags & IEACHE_PBS_TLWE_POLYS) ? 2 : 1));
    }
};
// words per host row of a programmable bootstrap's output
size_t pbs_out_words(const Params& p, int flags) {
    if (flags & IEACHE_PBS_ACCUMULATOR) return (size_t)2 * (size_t)p.N;
    return (flags & IEACHE_PBS_NO_KEYSWITCH) ? (size_t)p.N + 1 : (size_t)p.n + 1;
}
}  // namespace

// ---- flat calls.  Device form: validate, check the pointers, run.  Host form: validate, stage the inputs, run the same
// evaluator call on the staged rows, download. ----
int ieache_gates_device(ieache_ctx* ctx, int gate_type, size_t count, const int32_t* d_a, const int32_t* d_b,
                        int32_t* d_out, ieache_stats* stats) {
    return guarded([&] {
        if (!ctx || !d_a || !d_b || !d_out) return fail(IEACHE_EINVAL, "null argument");
        if (bad_gate2(gate_type)) return fail(IEACHE_EINVAL, "unknown gate type");
        require_device_pointers(count, {{d_a, "d_a"}, {d_b, "d_b"}, {d_out, "d_out"}});
        return with_stats(stats, [&](EvalStats* st) { ctx->eval->gates_device(gate_type, count, d_a, d_b, d_out, st); });
    });
}

int ieache_gates(ieache_ctx* ctx, int gate_type, size_t count, const int32_t* a, const int32_t* b, int32_t* out,
                 ieache_stats* stats) {
    return guarded([&] {
        if (const int rc = check_gates(ctx, gate_type, a, b, out)) return rc;
        HostCall h(ctx, count);
        StagedRows da = h.operand(kStageA, a), db = h.operand(kStageB, b), dout = h.results(count);
        with_stats(stats, [&](EvalStats* st) { h.ev.gates_device(gate_type, count, da.p, db.p, dout.p, st); });
        h.download(dout, out);
        return 0;
    });
}

int ieache_gates3_device(ieache_ctx* ctx, int gate_type, size_t count, const int32_t* d_a, const int32_t* d_b, const int32_t* d_c,
                         int32_t* d_out, ieache_stats* stats) {
    return guarded([&] {
        if (!is_gate3(gate_type)) return fail(IEACHE_EINVAL, kNotGate3);
        if (!ctx || !d_a || !d_b || !d_c || !d_out) return fail(IEACHE_EINVAL, "null argument");
        require_device_pointers(count, {{d_a, "d_a"}, {d_b, "d_b"}, {d_c, "d_c"}, {d_out, "d_out"}});
        return with_stats(stats, [&](EvalStats* st) { ctx->eval->gates3_device(gate_type, count, d_a, d_b, d_c, d_out, st); });
    });
}

int ieache_gates3(ieache_ctx* ctx, int gate_type, size_t count, const int32_t* a, const int32_t* b, const int32_t* c, int32_t* out,
                  ieache_stats* stats) {
    return guarded([&] {
        if (const int rc = check_gates3(ctx, gate_type, a, b, c, out)) return rc;
        HostCall h(ctx, count);
        StagedRows da = h.operand(kStageA, a), db = h.operand(kStageB, b), dc = h.operand(kStageC, c), dout = h.results(count);
        with_stats(stats, [&](EvalStats* st) { h.ev.gates3_device(gate_type, count, da.p, db.p, dc.p, dout.p, st); });
        h.download(dout, out);
        return 0;
    });
}

int ieache_mux_device(ieache_ctx* ctx, size_t count, const int32_t* d_a, const int32_t* d_b, const int32_t* d_c,
                      int32_t* d_out, ieache_stats* stats) {
    return guarded([&] {
        if (!ctx || !d_a || !d_b || !d_c || !d_out) return fail(IEACHE_EINVAL, "null argument");
        require_device_pointers(count, {{d_a, "d_a"}, {d_b, "d_b"}, {d_c, "d_c"}, {d_out, "d_out"}});
        return with_stats(stats, [&](EvalStats* st) { ctx->eval->mux_device(count, d_a, d_b, d_c, d_out, st); });
    });
}

int ieache_mux(ieache_ctx* ctx, size_t count, const int32_t* a, const int32_t* b, const int32_t* c, int32_t* out,
               ieache_stats* stats) {
    return guarded([&] {
        if (const int rc = check_rows({ctx, a, b, c, out})) return rc;
        HostCall h(ctx, count);
        StagedRows da = h.operand(kStageA, a), db = h.operand(kStageB, b), dc = h.operand(kStageC, c), dout = h.results(count);
        with_stats(stats, [&](EvalStats* st) { h.ev.mux_device(count, da.p, db.p, dc.p, dout.p, st); });
        h.download(dout, out);
        return 0;
    });
}

int ieache_extract_stride(const ieache_ctx* ctx) { return ctx ? ctx->eval->extract_stride() : IEACHE_EINVAL; }

int ieache_pbs_device(ieache_ctx* ctx, size_t count, const int32_t* d_x, const int32_t* d_test_polys, int32_t n_polys,
                      const int32_t* d_poly_of, int32_t* d_out, int flags, ieache_stats* stats) {
    return guarded([&] {
        if (const char* e = pbs_args_error(flags, n_polys, d_test_polys)) return fail(IEACHE_EINVAL, e);
        if (!ctx || !d_x || !d_out) return fail(IEACHE_EINVAL, "null argument");
        require_device_pointers(count, {{d_x, "d_x"}, {d_test_polys, "d_test_polys"}, {d_poly_of, "d_poly_of", true}, {d_out, "d_out"}});
        return with_stats(stats, [&](EvalStats* st) { ctx->eval->pbs_device(count, d_x, d_test_polys, n_polys, d_poly_of, d_out, flags, st); });
    });
}

int ieache_pbs(ieache_ctx* ctx, size_t count, const int32_t* x, const int32_t* test_polys, int32_t n_polys, const int32_t* poly_of,
               int32_t* out, int flags, ieache_stats* stats) {
    return guarded([&] {
        if (const int rc = check_pbs(ctx, count, x, test_polys, n_polys, poly_of, out, flags)) return rc;
        const bool woks = (flags & IEACHE_PBS_NO_KEYSWITCH) != 0, accs = (flags & IEACHE_PBS_ACCUMULATOR) != 0;
        HostCall h(ctx, count);
        // whole accumulators: packed rows of 2N words, on the device as on the host
        StagedRows dx = h.operand(kStageA, x), dout = accs ? StagedRows(h.ev, kStageOut, count, (size_t)2 * (size_t)h.p.N) : h.results(count, woks);
        StagedRows dtv = h.table(test_polys, n_polys, flags), dof = h.words(kStagePolyOf, poly_of, count);
        with_stats(stats, [&](EvalStats* st) { h.ev.pbs_device(count, dx.p, dtv.p, n_polys, dof.p, dout.p, flags, st); });
        if (accs)
            dout.download(out, (size_t)2 * (size_t)h.p.N);
        else
            h.download(dout, out, woks);
        return 0;
    });
}

int ieache_pbs_multi_device(ieache_ctx* ctx, size_t count, const int32_t* d_x, const int32_t* d_test_polys, int32_t n_polys,
                            const int32_t* d_poly_of, const int32_t* d_factors, int32_t n_factors, const int32_t* d_bias, int32_t* d_out,
                            int flags, ieache_stats* stats) {
    return guarded([&] {
        if (const char* e = pbs_multi_args_error(flags, n_polys, d_test_polys, n_factors, d_factors)) return fail(IEACHE_EINVAL, e);
        if (!ctx || !d_x || !d_out) return fail(IEACHE_EINVAL, "null argument");
        require_device_pointers(count, {{d_x, "d_x"}, {d_test_polys, "d_test_polys"}, {d_poly_of, "d_poly_of", true}, {d_factors, "d_factors"},
                                        {d_bias, "d_bias", true}, {d_out, "d_out"}});
        return with_stats(stats, [&](EvalStats* st) {
            ctx->eval->pbs_multi_device(count, d_x, d_test_polys, n_polys, d_poly_of, d_factors, n_factors, d_bias, d_out, flags, st);
        });
    });
}

int ieache_pbs_multi(ieache_ctx* ctx, size_t count, const int32_t* x, const int32_t* test_polys, int32_t n_polys, const int32_t* poly_of,
                     const int32_t* factors, int32_t n_factors, const int32_t* bias, int32_t* out, int flags, ieache_stats* stats) {
    return guarded([&] {
        if (const int rc = check_pbs_multi(ctx, count, x, test_polys, n_polys, poly_of, factors, n_factors, out, flags)) return rc;
        const bool woks = (flags & IEACHE_PBS_NO_KEYSWITCH) != 0;
        HostCall h(ctx, count);
        StagedRows dx = h.operand(kStageA, x), dout = h.results(count * (size_t)n_factors, woks);
        StagedRows dtv = h.table(test_polys, n_polys, flags), dof = h.words(kStagePolyOf, poly_of, count);
        StagedRows dfa = h.polys(kStageFactors, factors, (size_t)n_factors), dbi = h.words(kStageBias, bias, (size_t)n_factors);
        with_stats(stats, [&](EvalStats* st) {
            h.ev.pbs_multi_device(count, dx.p, dtv.p, n_polys, dof.p, dfa.p, n_factors, dbi.p, dout.p, flags, st);
        });
        h.download(dout, out, woks);
        return 0;
    });
}

int ieache_keyswitch_device(ieache_ctx* ctx, size_t count, const int32_t* d_u, int32_t* d_out, ieache_stats* stats) {
    return guarded([&] {
        if (!ctx || !d_u || !d_out) return fail(IEACHE_EINVAL, "null argument");
        require_device_pointers(count, {{d_u, "d_u"}, {d_out, "d_out"}});
        return with_stats(stats, [&](EvalStats* st) { ctx->eval->keyswitch_device(count, d_u, d_out, st); });
    });
}

int ieache_keyswitch(ieache_ctx* ctx, size_t count, const int32_t* u, int32_t* out, ieache_stats* stats) {
    return guarded([&] {
        if (const int rc = check_rows({ctx, u, out})) return rc;
        HostCall h(ctx, count);
        StagedRows du(h.ev, kStageExtracted, count, (size_t)h.ev.extract_stride(), u, (size_t)h.p.N + 1), dout = h.results(count);
        with_stats(stats, [&](EvalStats* st) { h.ev.keyswitch_device(count, du.p, dout.p, st); });
        h.download(dout, out);
        return 0;
    });
}

// ---- linear layers on encrypted rows (section 3n).  linear_plan.h states the kinds and the rules; what needs no context is
// judged before the context is looked at. ----
static_assert(kLinearRowsLwe == IEACHE_ROWS_LWE && kLinearRowsExtracted == IEACHE_ROWS_EXTRACTED && kLinearRowsTlwe == IEACHE_ROWS_TLWE &&
                  kLinearMaxDim == IEACHE_LINEAR_MAX_DIM,
              "linear_plan.h knows the constants of include/ieache.h");
namespace {
// 0 with *c filled, or the code after fail()
int check_linear(const ieache_ctx* ctx, bool device, int rows, size_t batch, int32_t n_out, int32_t n_in, const int8_t* w, const int32_t* bias,
                 const int32_t* x, const int32_t* out, LinearCall* c) {
    if (const char* e = linear_scalar_error(rows, n_out, n_in, bias != nullptr)) return fail(IEACHE_EINVAL, e);
    if (!ctx) return fail(IEACHE_EINVAL, kLinearNull);
    c->rows = rows, c->batch = batch, c->n_out = n_out, c->n_in = n_in, c->w = w, c->bias = bias, c->x = x, c->out = out, c->device = device;
    if (const char* e = linear_call_error(ctx->eval->params(), *c)) return fail(IEACHE_EINVAL, e);
    return 0;
}
}  // namespace

int ieache_lwe_linear_device(ieache_ctx* ctx, int rows, size_t batch, int32_t n_out, int32_t n_in, const int8_t* d_w, const int32_t* d_bias,
                             const int32_t* d_x, int32_t* d_out, ieache_stats* stats) {
    return guarded([&] {
        LinearCall c;
        if (const int rc = check_linear(ctx, true, rows, batch, n_out, n_in, d_w, d_bias, d_x, d_out, &c)) return rc;
        require_device_pointers(batch, {{d_w, "d_w"}, {d_bias, "d_bias", true}, {d_x, "d_x"}, {d_out, "d_out"}});
        return with_stats(stats, [&](EvalStats* st) { ctx->eval->lwe_linear_device(rows, batch, n_out, n_in, d_w, d_bias, d_x, d_out, st); });
    });
}

int ieache_lwe_linear(ieache_ctx* ctx, int rows, size_t batch, int32_t n_out, int32_t n_in, const int8_t* w, const int32_t* bias, const int32_t* x,
                      int32_t* out, ieache_stats* stats) {
    return guarded([&] {
        LinearCall c;
        if (const int rc = check_linear(ctx, false, rows, batch, n_out, n_in, w, bias, x, out, &c)) return rc;
        if (batch == 0) return 0;
        HostCall h(ctx, batch);
        const LinearRows r = linear_rows(h.p, rows);
        // each kind's rows in the slot that holds rows of its shape (LWE rows: an operand slot, n + 1 words of lwe_stride() as ever)
        const StageSlot slot = rows == kLinearRowsLwe ? kStageA : rows == kLinearRowsExtracted ? kStageExtracted : kStageTlweA;
        StagedRows dx(h.ev, slot, batch * (size_t)n_in, (size_t)r.stride, x, (size_t)r.words);
        StagedRows dout(h.ev, kStageOut, batch * (size_t)n_out, (size_t)r.stride), dbi = h.words(kStageBias, bias, (size_t)n_out);
        const size_t w_bytes = (size_t)n_out * (size_t)n_in;
        int8_t* dw = reinterpret_cast<int8_t*>(h.ev.staging(kStageFactors, w_bytes));
        HIP_CHECK(hipMemcpy(dw, w, w_bytes, hipMemcpyHostToDevice));
        with_stats(stats, [&](EvalStats* st) { h.ev.lwe_linear_device(rows, batch, n_out, n_in, dw, dbi.p, dx.p, dout.p, st); });
        dout.download(out, (size_t)r.words);
        return 0;
    });
}

int ieache_debug_linear_plan(const ieache_ctx* ctx, int rows, size_t batch, int32_t n_out, int32_t n_in, int64_t out[4]) {
    return guarded([&] {
        (void)batch;  // the tiling of a call does not depend on it: gridDim.x is batch x column blocks
        if (const char* e = linear_scalar_error(rows, n_out, n_in, false)) return fail(IEACHE_EINVAL, e);
        if (!ctx || !out) return fail(IEACHE_EINVAL, kLinearNull);
        ctx->eval->linear_plan_figures(rows, n_out, n_in, out);
        return 0;
    });
}

// ---- packing key switch: LWE rows -> TLWE samples ----
namespace {
// what both forms of the call refuse before anything is staged or launched: 0, or the code after fail()
int check_pack(const ieache_ctx* ctx, int32_t m, int32_t spread, int32_t shift, const int32_t* rows, const int32_t* out) {
    if (!ctx || !rows || !out) return fail(IEACHE_EINVAL, "null argument");
    if (!ctx->eval->has_packing_key()) return fail(IEACHE_EINVAL, "pack: no packing key set");
    if (const char* e = pack_call_error(ctx->eval->params(), m, spread, shift)) return fail(IEACHE_EINVAL, e);
    return 0;
}
}  // namespace

int ieache_ctx_set_packing_key(ieache_ctx* ctx, int32_t pk_t, int32_t pk_basebit, const int32_t* pk) {
    return guarded([&] {
        if (!ctx) return fail(IEACHE_EINVAL, "null context");
        if (pk)
            if (const char* e = pack_set_error(ctx->eval->params(), pk_t, pk_basebit)) return fail(IEACHE_EINVAL, e);
        ctx->eval->set_packing_key(pk_t, pk_basebit, pk);
        return 0;
    });
}

int ieache_debug_pack_plan(const ieache_ctx* ctx, size_t groups, int32_t m, int64_t out[4]) {
    return guarded([&] {
        if (!ctx || !out) return fail(IEACHE_EINVAL, "null argument");
        if (m < 1) return fail(IEACHE_EINVAL, "pack: m must be at least 1");
        ctx->eval->pack_plan_figures(groups, m, out);
        return 0;
    });
}

int ieache_pack_device(ieache_ctx* ctx, size_t groups, int32_t m, int32_t spread, int32_t shift, const int32_t* d_rows, int32_t* d_out,
                       ieache_stats* stats) {
    return guarded([&] {
        if (const int rc = check_pack(ctx, m, spread, shift, d_rows, d_out)) return rc;
        require_device_pointers(groups, {{d_rows, "d_rows"}, {d_out, "d_out"}});
        return with_stats(stats, [&](EvalStats* st) { ctx->eval->pack_device(groups, m, spread, shift, d_rows, d_out, st); });
    });
}

int ieache_pack(ieache_ctx* ctx, size_t groups, int32_t m, int32_t spread, int32_t shift, const int32_t* rows, int32_t* out, ieache_stats* stats) {
    return guarded([&] {
        if (const int rc = check_pack(ctx, m, spread, shift, rows, out)) return rc;
        HostCall h(ctx, groups * (size_t)m);
        const size_t sample = (size_t)2 * (size_t)h.p.N;
        StagedRows drows = h.operand(kStageA, rows), dout(h.ev, kStageOut, groups, sample);
        with_stats(stats, [&](EvalStats* st) { h.ev.pack_device(groups, m, spread, shift, drows.p, dout.p, st); });
        dout.download(out, sample);
        return 0;
    });
}

// ---- CMux on caller TGSW samples, the CMux-tree lookup, extraction of a coefficient ----
struct ieache_tgsw {
    std::unique_ptr<TgswSet> set;
};

namespace {
// what both forms of the two calls refuse before anything is staged or launched: 0, or the code after fail()
int check_tgsw(const ieache_ctx* ctx, const ieache_tgsw* set) {
    if (!ctx || !set || !set->set) return fail(IEACHE_EINVAL, "null argument");
    if (set->set->owner != ctx->eval->cmux_id()) return fail(IEACHE_EINVAL, "the TGSW set was prepared on another context");
    return 0;
}
// host indices: every one of idx[0 .. count) inside [0, bound), or the code after fail(); the message names "<call>: <name>"
int check_indices(const int32_t* idx, size_t count, int64_t bound, const char* call, const char* name) {
    if (idx)
        for (size_t i = 0; i < count; i++)
            if (idx[i] < 0 || idx[i] >= bound)
                return fail(IEACHE_EINVAL, std::string(call) + ": " + name + "[" + std::to_string(i) + "] = " + std::to_string(idx[i]) +
                                               " is outside [0, " + std::to_string(bound) + ")");
    return 0;
}

// ---- The calls on a set (sections 3f to 3j, and the replace write of a window of 3l).  set_calls.h states what each is; these read it.  `a`: the call's pointer
// arguments in the order of its signature (kSetCalls[..].args). ----
static_assert(kSetCalls[kCallLutRead].known_flags == IEACHE_LUT_READ_NO_KEYSWITCH && Evaluator::kLutReadNoKeyswitch == IEACHE_LUT_READ_NO_KEYSWITCH,
              "set_calls.h knows, and the evaluator reads, the flags of include/ieache.h");
int check_set_scalars(const SetCall& c, int32_t N) {
    const std::string refusal = set_call_refusal(c, N);
    return refusal.empty() ? 0 : fail(IEACHE_EINVAL, refusal);
}
// what the device and the host form refuse first: the context and the set, a null required argument, a missing projection key;
// the scalars come next
int check_set_call(const ieache_ctx* ctx, const ieache_tgsw* set, const SetCall& c, SetPtrs a) {
    if (const int rc = check_tgsw(ctx, set)) return rc;
    const SetCallShape& s = set_call_shape(c);
    for (int i = 0; i < s.n_args; i++)
        if (!a.begin()[i] && set_arg_required(c, s.args[i])) return fail(IEACHE_EINVAL, "null argument");
    if (s.window && !ctx->eval->has_projection_key()) return fail(IEACHE_EINVAL, std::string(s.name) + ": no projection key set");
    return 0;
}
// the host and the reference forms: the scalars, then the first bad entry of the index arrays in argument order, then lut_read's coef
int check_set_indices(const SetCall& c, SetPtrs a, int32_t N, size_t n_set) {
    if (const int rc = check_set_scalars(c, N)) return rc;
    const SetCallShape& s = set_call_shape(c);
    for (int i = 0; i < s.n_args; i++) {
        const SetArg& arg = s.args[i];
        if (arg.kind != kArgIndices) continue;
        if (const int rc = check_indices(static_cast<const int32_t*>(a.begin()[i]), set_arg_units(c, arg), set_arg_bound(c, arg, N, n_set), s.name, arg.name + 2))
            return rc;
    }
    return c.kind == kCallLutRead ? check_indices(&c.coef, 1, N, s.name, "coef") : 0;
}
// the device forms: the scalars, then every pointer the call will read or write; a null optional one is none
int check_set_pointers(const SetCall& c, SetPtrs args, int32_t N) {
    if (const int rc = check_set_scalars(c, N)) return rc;
    const SetCallShape& s = set_call_shape(c);
    const void* const* a = args.begin();
    for (int i = 0; i < s.n_args; i++)  // first, and always, what a call without items touches as well (lut_add's memories and output)
        if (s.args[i].empty_too && (a[i] || s.args[i].need != kOptional)) require_device_pointer(a[i], s.args[i].name);
    for (int i = 0; i < s.n_args && c.count; i++)  // then the rest, which only a call with items reads
        if (!s.args[i].empty_too && (a[i] || s.args[i].need != kOptional)) require_device_pointer(a[i], s.args[i].name);
    return 0;
}
extern "C++" {  // templates
// The device form: refuse, check the pointers, run(stats).
template <class Run>
int set_call_device(ieache_ctx* ctx, const ieache_tgsw* set, const SetCall& c, const SetPtrs& a, ieache_stats* stats, Run&& run) {
    return guarded([&] {
        if (const int rc = check_set_call(ctx, set, c, a)) return rc;
        if (const int rc = check_set_pointers(c, a, ctx->eval->params().N)) return rc;
        return with_stats(stats, run);
    });
}
// The host form: refuse, stage every input where the table says (a null one stages nothing and stays null), run(evaluator, d,
// stats) with d[i] argument i on the device, download `out` (a's last entry, as the pointer to write through).  An input staged
// at the result rows is uploaded into them: the call then runs in place.  lut_read's rows are LWE rows, key-switched or extracted.
template <class Run>
int set_call_host(ieache_ctx* ctx, const ieache_tgsw* set, const SetCall& c, const SetPtrs& a, int32_t* out, ieache_stats* stats, Run&& run) {
    return guarded([&] {
        if (const int rc = check_set_call(ctx, set, c, a)) return rc;
        if (const int rc = check_set_indices(c, a, ctx->eval->params().N, set->set->n)) return rc;
        static constexpr StageSlot kSlot[] = {kStageOut, kStagePolyOf, kStageBias, kStageFactors, kStageTlweA, kStageTlweB, kStageTestPolys, kStageOut};
        const SetCallShape& s = set_call_shape(c);
        HostCall h(ctx, c.count);
        const size_t sample = (size_t)2 * (size_t)h.p.N, out_rows = set_arg_units(c, set_call_output(c));
        const bool lwe = c.kind == kCallLutRead, extracted = lwe && (c.flags & IEACHE_LUT_READ_NO_KEYSWITCH);
        StagedRows dout = lwe ? h.results(out_rows, extracted) : StagedRows(h.ev, kStageOut, out_rows, sample);
        Torus32* d[kSetCallMaxArgs] = {};
        d[s.n_args - 1] = dout.p;
        for (int i = 0; i + 1 < s.n_args; i++) {
            const SetArg& arg = s.args[i];
            const int32_t* src = static_cast<const int32_t*>(a.begin()[i]);
            const size_t units = set_arg_units(c, arg);
            if (arg.kind == kArgIndices) {
                d[i] = h.words(kSlot[arg.stage], src, units).p;
            } else if (arg.stage == kAtResult) {
                if (src && units) HIP_CHECK(hipMemcpy(dout.p, src, units * sample * 4, hipMemcpyHostToDevice));
                d[i] = src ? dout.p : nullptr;
            } else {
                d[i] = StagedRows(h.ev, kSlot[arg.stage], units, sample, src, sample).p;
            }
        }
        with_stats(stats, [&](EvalStats* st) { run(h.ev, d, st); });
        if (lwe)
            h.download(dout, out, extracted);
        else
            dout.download(out, sample);
        return 0;
    });
}
}  // extern "C++"

// The one preparation behind the four exported forms: samples on the host or the device, made with the context's gadget
// (gadget false) or with (l, Bgbit).
ieache_tgsw* tgsw_prepare(ieache_ctx* ctx, const int32_t* samples, size_t n, bool on_device, bool gadget, int32_t l, int32_t Bgbit) {
    ieache_tgsw* out = nullptr;
    guarded([&] {
        if (!ctx || !samples) return fail(IEACHE_EINVAL, "null argument");
        const Params& p = ctx->eval->params();
        if (const char* why = gadget ? gadget_refusal(p, l, Bgbit) : nullptr) return fail(IEACHE_EINVAL, why);
        if (n < 1) return fail(IEACHE_EINVAL, "tgsw_prepare: no samples");
        auto prepare = [&](const Torus32* d_samples) {
            std::unique_ptr<ieache_tgsw> h(new ieache_tgsw);
            h->set.reset(gadget ? ctx->eval->tgsw_prepare_device(d_samples, n, l, Bgbit) : ctx->eval->tgsw_prepare_device(d_samples, n));
            out = h.release();
            return 0;
        };
        if (on_device) {
            require_device_pointer(samples, "d_samples");
            return prepare(samples);
        }
        if (!gadget && !br_supported(p))
            return fail(IEACHE_EINVAL, "tgsw_prepare: the CMux kernels cover N = 1024, k = 1 with (l, Bgbit) = (3, 7) or (2, 10) only");
        HIP_CHECK(hipSetDevice(ctx->eval->device()));
        DevRows words(n, (gadget ? (size_t)2 * (size_t)l : (size_t)p.kpl()) * 2 * (size_t)p.N);  // the int32 samples: scratch of this call
        HIP_CHECK(hipMemcpy(words.p, samples, words.rows * words.stride * 4, hipMemcpyHostToDevice));
        return prepare(words.p);
    });
    return out;
}
}  // namespace

ieache_tgsw* ieache_tgsw_prepare_device(ieache_ctx* ctx, const int32_t* d_samples, size_t n) { return tgsw_prepare(ctx, d_samples, n, true, false, 0, 0); }
ieache_tgsw* ieache_tgsw_prepare(ieache_ctx* ctx, const int32_t* samples, size_t n) { return tgsw_prepare(ctx, samples, n, false, false, 0, 0); }

void ieache_tgsw_free(ieache_tgsw* set) {
    if (!set) return;
    try {
        if (set->set) (void)hipSetDevice(set->set->device);  // the set owns its memory: the context may be gone already
        delete set;
    } catch (...) {
    }
}

int ieache_debug_cmux_plan(const ieache_ctx* ctx, size_t count, int32_t depth, int64_t out[4]) {
    return guarded([&] {
        if (!ctx || !out) return fail(IEACHE_EINVAL, "null argument");
        // a negative depth asks for the flat plan, so only the upper bound is a refusal here: lut_tree's, in its words
        if (depth > IEACHE_LUT_TREE_MAX_DEPTH) return check_set_scalars(SetCall{kCallLutTree, count, depth}, ctx->eval->params().N);
        ctx->eval->cmux_plan_figures(count, depth, out);
        return 0;
    });
}

int ieache_cmux_device(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, const int32_t* d_sel_of, const int32_t* d_d1, const int32_t* d_d0,
                       int32_t* d_out, ieache_stats* stats) {
    return set_call_device(ctx, set, {kCallCmux, count}, {d_sel_of, d_d1, d_d0, d_out}, stats,
                           [&](EvalStats* st) { ctx->eval->cmux_device(*set->set, count, d_sel_of, d_d1, d_d0, d_out, st); });
}

int ieache_cmux(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, const int32_t* sel_of, const int32_t* d1, const int32_t* d0, int32_t* out,
                ieache_stats* stats) {
    return set_call_host(ctx, set, {kCallCmux, count}, {sel_of, d1, d0, out}, out, stats, [&](Evaluator& ev, Torus32* const* d, EvalStats* st) {
        ev.cmux_device(*set->set, count, d[0], d[1], d[2], d[3], st);
    });
}

int ieache_lut_tree_device(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, const int32_t* d_sel_of, const int32_t* d_tables,
                           int32_t n_tables, const int32_t* d_table_of, int32_t* d_out, ieache_stats* stats) {
    return set_call_device(ctx, set, {kCallLutTree, count, depth, 0, n_tables}, {d_sel_of, d_tables, d_table_of, d_out}, stats, [&](EvalStats* st) {
        ctx->eval->lut_tree_device(*set->set, count, depth, d_sel_of, d_tables, n_tables, d_table_of, d_out, st);
    });
}

int ieache_lut_tree(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, const int32_t* sel_of, const int32_t* tables,
                    int32_t n_tables, const int32_t* table_of, int32_t* out, ieache_stats* stats) {
    return set_call_host(ctx, set, {kCallLutTree, count, depth, 0, n_tables}, {sel_of, tables, table_of, out}, out, stats,
                         [&](Evaluator& ev, Torus32* const* d, EvalStats* st) { ev.lut_tree_device(*set->set, count, depth, d[0], d[1], n_tables, d[2], d[3], st); });
}

// ---- the scatter (section 3g): the tree's partner ----
int ieache_lut_scatter_device(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, const int32_t* d_sel_of, const int32_t* d_values,
                              const int32_t* d_mem, int32_t* d_out, ieache_stats* stats) {
    return set_call_device(ctx, set, {kCallLutScatter, count, depth}, {d_sel_of, d_values, d_mem, d_out}, stats, [&](EvalStats* st) {
        ctx->eval->lut_scatter_device(*set->set, count, depth, d_sel_of, d_values, d_mem, d_out, st);
    });
}

int ieache_lut_scatter(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, const int32_t* sel_of, const int32_t* values,
                       const int32_t* mem, int32_t* out, ieache_stats* stats) {
    return set_call_host(ctx, set, {kCallLutScatter, count, depth}, {sel_of, values, mem, out}, out, stats,
                         [&](Evaluator& ev, Torus32* const* d, EvalStats* st) { ev.lut_scatter_device(*set->set, count, depth, d[0], d[1], d[2], d[3], st); });
}

// ---- the rotation by caller selectors and the coefficient-level lookup (section 3h) ----
int ieache_tlwe_rotate_device(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t steps, const int32_t* d_sel_of,
                              const int32_t* d_amount_of, const int32_t* d_in, int32_t* d_out, ieache_stats* stats) {
    return set_call_device(ctx, set, {kCallTlweRotate, count, 0, steps}, {d_sel_of, d_amount_of, d_in, d_out}, stats, [&](EvalStats* st) {
        ctx->eval->tlwe_rotate_device(*set->set, count, steps, d_sel_of, d_amount_of, d_in, d_out, st);
    });
}

int ieache_tlwe_rotate(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t steps, const int32_t* sel_of, const int32_t* amount_of,
                       const int32_t* in, int32_t* out, ieache_stats* stats) {
    return set_call_host(ctx, set, {kCallTlweRotate, count, 0, steps}, {sel_of, amount_of, in, out}, out, stats,
                         [&](Evaluator& ev, Torus32* const* d, EvalStats* st) { ev.tlwe_rotate_device(*set->set, count, steps, d[0], d[1], d[2], d[3], st); });
}

int ieache_lut_read_device(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, int32_t steps, const int32_t* d_sel_of,
                           const int32_t* d_amount_of, const int32_t* d_tables, int32_t n_tables, const int32_t* d_table_of, int32_t coef, int flags,
                           int32_t* d_out, ieache_stats* stats) {
    return set_call_device(ctx, set, {kCallLutRead, count, depth, steps, n_tables, flags, coef}, {d_sel_of, d_amount_of, d_tables, d_table_of, d_out}, stats,
                           [&](EvalStats* st) {
                               ctx->eval->lut_read_device(*set->set, count, depth, steps, d_sel_of, d_amount_of, d_tables, n_tables, d_table_of, coef, flags,
                                                          d_out, st);
                           });
}

int ieache_lut_read(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, int32_t steps, const int32_t* sel_of,
                    const int32_t* amount_of, const int32_t* tables, int32_t n_tables, const int32_t* table_of, int32_t coef, int flags, int32_t* out,
                    ieache_stats* stats) {
    return set_call_host(ctx, set, {kCallLutRead, count, depth, steps, n_tables, flags, coef}, {sel_of, amount_of, tables, table_of, out}, out, stats,
                         [&](Evaluator& ev, Torus32* const* d, EvalStats* st) {
                             Torus32 *dsel = d[0], *damount = d[1], *dtables = d[2], *dof = d[3], *dout = d[4];
                             ev.lut_read_device(*set->set, count, depth, steps, dsel, damount, dtables, n_tables, dof, coef, flags, dout, st);
                         });
}

// ---- sets with a gadget of their own, and the replace write (section 3i) ----
ieache_tgsw* ieache_tgsw_prepare_gadget_device(ieache_ctx* ctx, const int32_t* d_samples, size_t n, int32_t l, int32_t Bgbit) {
    return tgsw_prepare(ctx, d_samples, n, true, true, l, Bgbit);
}
ieache_tgsw* ieache_tgsw_prepare_gadget(ieache_ctx* ctx, const int32_t* samples, size_t n, int32_t l, int32_t Bgbit) {
    return tgsw_prepare(ctx, samples, n, false, true, l, Bgbit);
}

int ieache_tgsw_gadget(const ieache_tgsw* set, int32_t* l, int32_t* Bgbit) {
    return guarded([&] {
        if (!set || !set->set) return fail(IEACHE_EINVAL, "null argument");
        if (l) *l = set->set->l;
        if (Bgbit) *Bgbit = set->set->Bgbit;
        return 0;
    });
}

int ieache_lut_write_device(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, const int32_t* d_sel_of, const int32_t* d_new,
                            const int32_t* d_mem, int32_t* d_out, ieache_stats* stats) {
    return set_call_device(ctx, set, {kCallLutWrite, count, depth}, {d_sel_of, d_new, d_mem, d_out}, stats, [&](EvalStats* st) {
        ctx->eval->lut_write_device(*set->set, count, depth, d_sel_of, d_new, d_mem, d_out, st);
    });
}

int ieache_lut_write(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, const int32_t* sel_of, const int32_t* fresh,
                     const int32_t* mem, int32_t* out, ieache_stats* stats) {
    return set_call_host(ctx, set, {kCallLutWrite, count, depth}, {sel_of, fresh, mem, out}, out, stats,
                         [&](Evaluator& ev, Torus32* const* d, EvalStats* st) { ev.lut_write_device(*set->set, count, depth, d[0], d[1], d[2], d[3], st); });
}

// ---- many values into shared memories (section 3j) ----
int ieache_lut_add_device(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, int32_t steps, const int32_t* d_sel_of,
                          const int32_t* d_amount_of, const int32_t* d_values, const int32_t* d_mems, int32_t n_mems, const int32_t* d_mem_of,
                          int32_t* d_out, ieache_stats* stats) {
    return set_call_device(ctx, set, {kCallLutAdd, count, depth, steps, n_mems}, {d_sel_of, d_amount_of, d_values, d_mems, d_mem_of, d_out}, stats,
                           [&](EvalStats* st) {
                               ctx->eval->lut_add_device(*set->set, count, depth, steps, d_sel_of, d_amount_of, d_values, d_mems, n_mems, d_mem_of, d_out, st);
                           });
}

int ieache_lut_add(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, int32_t steps, const int32_t* sel_of,
                   const int32_t* amount_of, const int32_t* values, const int32_t* mems, int32_t n_mems, const int32_t* mem_of, int32_t* out,
                   ieache_stats* stats) {
    return set_call_host(ctx, set, {kCallLutAdd, count, depth, steps, n_mems}, {sel_of, amount_of, values, mems, mem_of, out}, out, stats,
                         [&](Evaluator& ev, Torus32* const* d, EvalStats* st) {
                             Torus32 *dsel = d[0], *damount = d[1], *dvalues = d[2], *dmems = d[3], *dof = d[4], *dout = d[5];
                             ev.lut_add_device(*set->set, count, depth, steps, dsel, damount, dvalues, dmems, n_mems, dof, dout, st);
                         });
}

// ---- the TLWE projection and the replace write of a window (section 3l).  project_plan.h states what the calls accept; the
// write is a row of set_calls.h. ----
namespace {
int check_project(const ieache_ctx* ctx, int32_t first, int32_t width, int32_t dest, size_t count, const int32_t* in, const int32_t* out) {
    if (!ctx || (count && (!in || !out))) return fail(IEACHE_EINVAL, "null argument");
    if (!ctx->eval->has_projection_key()) return fail(IEACHE_EINVAL, "tlwe_project: no projection key set");
    if (const char* e = project_call_error(ctx->eval->params(), first, width, dest)) return fail(IEACHE_EINVAL, e);
    return 0;
}
}  // namespace

int ieache_ctx_set_projection_key(ieache_ctx* ctx, int32_t pk_t, int32_t pk_basebit, const int32_t* pk) {
    return guarded([&] {
        if (!ctx) return fail(IEACHE_EINVAL, "null context");
        if (pk)
            if (const char* e = project_set_error(ctx->eval->params(), pk_t, pk_basebit)) return fail(IEACHE_EINVAL, e);
        ctx->eval->set_projection_key(pk_t, pk_basebit, pk);
        return 0;
    });
}

int ieache_debug_project_plan(const ieache_ctx* ctx, size_t count, int32_t width, int64_t out[4]) {
    return guarded([&] {
        if (!ctx || !out) return fail(IEACHE_EINVAL, "null argument");
        if (!ctx->eval->has_projection_key()) return fail(IEACHE_EINVAL, "tlwe_project: no projection key set");
        if (const char* e = project_call_error(ctx->eval->params(), 0, width, 0)) return fail(IEACHE_EINVAL, e);
        ctx->eval->project_plan_figures(count, width, out);
        return 0;
    });
}

int ieache_tlwe_project_device(ieache_ctx* ctx, size_t count, int32_t first, int32_t width, int32_t dest, const int32_t* d_in, int32_t* d_out,
                               ieache_stats* stats) {
    return guarded([&] {
        if (const int rc = check_project(ctx, first, width, dest, count, d_in, d_out)) return rc;
        require_device_pointers(count, {{d_in, "d_in"}, {d_out, "d_out"}});
        return with_stats(stats, [&](EvalStats* st) { ctx->eval->tlwe_project_device(count, first, width, dest, d_in, d_out, st); });
    });
}

int ieache_tlwe_project(ieache_ctx* ctx, size_t count, int32_t first, int32_t width, int32_t dest, const int32_t* in, int32_t* out, ieache_stats* stats) {
    return guarded([&] {
        if (const int rc = check_project(ctx, first, width, dest, count, in, out)) return rc;
        HostCall h(ctx, count);
        const size_t sample = (size_t)2 * (size_t)h.p.N;
        StagedRows din(h.ev, kStageTlweA, count, sample, in, sample), dout(h.ev, kStageOut, count, sample);
        with_stats(stats, [&](EvalStats* st) { h.ev.tlwe_project_device(count, first, width, dest, din.p, dout.p, st); });
        dout.download(out, sample);
        return 0;
    });
}

int ieache_lut_write_coef_device(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, int32_t steps, int32_t width, int32_t unit,
                                 const int32_t* d_sel_of, const int32_t* d_new, const int32_t* d_mem, int32_t* d_out, ieache_stats* stats) {
    return set_call_device(ctx, set, {kCallLutWriteCoef, count, depth, steps, 1, 0, 0, width, unit}, {d_sel_of, d_new, d_mem, d_out}, stats,
                           [&](EvalStats* st) { ctx->eval->lut_write_coef_device(*set->set, count, depth, steps, width, unit, d_sel_of, d_new, d_mem, d_out, st); });
}

int ieache_lut_write_coef(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, int32_t steps, int32_t width, int32_t unit,
                          const int32_t* sel_of, const int32_t* fresh, const int32_t* mem, int32_t* out, ieache_stats* stats) {
    return set_call_host(ctx, set, {kCallLutWriteCoef, count, depth, steps, 1, 0, 0, width, unit}, {sel_of, fresh, mem, out}, out, stats,
                         [&](Evaluator& ev, Torus32* const* d, EvalStats* st) {
                             ev.lut_write_coef_device(*set->set, count, depth, steps, width, unit, d[0], d[1], d[2], d[3], st);
                         });
}

// ---- automata over words of TGSW-encrypted bits (section 3k).  The call stands beside the table of set_calls.h
// (automaton_plan.h says why); the device and host forms below follow set_call_device's and set_call_host's steps. ----
struct ieache_automaton {
    std::unique_ptr<Automaton> a;
};

namespace {
// what both forms refuse before anything is staged or launched: 0, or the code after fail()
int check_automaton_call(const ieache_ctx* ctx, const ieache_tgsw* set, const ieache_automaton* a, size_t count, const int32_t* finals, const int32_t* out,
                         int32_t n_finals) {
    if (const int rc = check_tgsw(ctx, set)) return rc;
    if (!a || !a->a) return fail(IEACHE_EINVAL, "null argument");
    if (a->a->owner != ctx->eval->cmux_id()) return fail(IEACHE_EINVAL, "the automaton was compiled on another context");
    if (count && (!finals || !out)) return fail(IEACHE_EINVAL, "null argument");
    if (n_finals < 1) return fail(IEACHE_EINVAL, "automaton_run: n_finals must be at least 1");
    return 0;
}
}  // namespace

ieache_automaton* ieache_automaton_create(ieache_ctx* ctx, int32_t states, int32_t steps, int32_t n_out, const int32_t* next0, const int32_t* next1) {
    ieache_automaton* out = nullptr;
    guarded([&] {
        if (!ctx) return fail(IEACHE_EINVAL, "null argument");
        const std::string refusal = automaton_refusal(states, steps, n_out, next0, next1);
        if (!refusal.empty()) return fail(IEACHE_EINVAL, refusal);
        std::unique_ptr<ieache_automaton> h(new ieache_automaton);
        h->a.reset(ctx->eval->automaton_create(states, steps, n_out, next0, next1));
        out = h.release();
        return 0;
    });
    return out;
}

void ieache_automaton_free(ieache_automaton* a) {
    if (!a) return;
    try {
        if (a->a) (void)hipSetDevice(a->a->device);  // the automaton owns its memory: the context may be gone already
        delete a;
    } catch (...) {
    }
}

int ieache_automaton_info(const ieache_automaton* a, int32_t* states, int32_t* steps, int32_t* n_out, int64_t* cmuxes) {
    return guarded([&] {
        if (!a || !a->a) return fail(IEACHE_EINVAL, "null argument");
        if (states) *states = a->a->states;
        if (steps) *steps = a->a->steps;
        if (n_out) *n_out = a->a->n_out;
        if (cmuxes) *cmuxes = a->a->cmuxes;
        return 0;
    });
}

int ieache_automaton_check(int32_t states, int32_t steps, int32_t n_out, const int32_t* next0, const int32_t* next1) {
    return guarded([&] {
        const std::string refusal = automaton_refusal(states, steps, n_out, next0, next1);
        return refusal.empty() ? 0 : fail(IEACHE_EINVAL, refusal);
    });
}

int ieache_debug_automaton_plan(const ieache_ctx* ctx, const ieache_automaton* a, size_t count, int64_t out[5]) {
    return guarded([&] {
        if (!ctx || !a || !a->a || !out) return fail(IEACHE_EINVAL, "null argument");
        ctx->eval->automaton_plan_figures(*a->a, count, out);
        return 0;
    });
}

int ieache_automaton_run_device(ieache_ctx* ctx, const ieache_tgsw* set, const ieache_automaton* a, size_t count, const int32_t* d_sel_of,
                                const int32_t* d_finals, int32_t n_finals, const int32_t* d_final_of, int32_t* d_out, ieache_stats* stats) {
    return guarded([&] {
        if (const int rc = check_automaton_call(ctx, set, a, count, d_finals, d_out, n_finals)) return rc;
        if (count) {
            require_device_pointer(d_finals, "d_finals");
            require_device_pointer(d_out, "d_out");
            if (d_sel_of && a->a->steps > 0) require_device_pointer(d_sel_of, "d_sel_of");
            if (d_final_of) require_device_pointer(d_final_of, "d_final_of");
        }
        return with_stats(stats, [&](EvalStats* st) { ctx->eval->automaton_run_device(*set->set, *a->a, count, d_sel_of, d_finals, n_finals, d_final_of, d_out, st); });
    });
}

int ieache_automaton_run(ieache_ctx* ctx, const ieache_tgsw* set, const ieache_automaton* a, size_t count, const int32_t* sel_of, const int32_t* finals,
                         int32_t n_finals, const int32_t* final_of, int32_t* out, ieache_stats* stats) {
    return guarded([&] {
        if (const int rc = check_automaton_call(ctx, set, a, count, finals, out, n_finals)) return rc;
        const Automaton& au = *a->a;
        if (const int rc = check_indices(sel_of, count * (size_t)au.steps, (int64_t)set->set->n, "automaton_run", "sel_of")) return rc;
        if (const int rc = check_indices(final_of, count, n_finals, "automaton_run", "final_of")) return rc;
        if (count == 0) return with_stats(stats, [&](EvalStats*) {});
        HostCall h(ctx, count);
        const size_t sample = (size_t)2 * (size_t)h.p.N;
        StagedRows dout(h.ev, kStageOut, count * (size_t)au.n_out, sample);
        StagedRows dfinals(h.ev, kStageTestPolys, (size_t)n_finals * (size_t)au.states, sample, finals, sample);
        StagedRows dsel = h.words(kStagePolyOf, au.steps > 0 ? sel_of : nullptr, count * (size_t)au.steps);
        StagedRows dof = h.words(kStageBias, final_of, count);
        with_stats(stats, [&](EvalStats* st) { h.ev.automaton_run_device(*set->set, au, count, dsel.p, dfinals.p, n_finals, dof.p, dout.p, st); });
        dout.download(out, sample);
        return 0;
    });
}

int ieache_tlwe_extract_device(ieache_ctx* ctx, size_t count, const int32_t* d_tlwe, const int32_t* d_coef_of, int32_t* d_u, ieache_stats* stats) {
    return guarded([&] {
        if (!ctx || !d_tlwe || !d_u) return fail(IEACHE_EINVAL, "null argument");
        require_device_pointers(count, {{d_tlwe, "d_tlwe"}, {d_coef_of, "d_coef_of", true}, {d_u, "d_u"}});
        return with_stats(stats, [&](EvalStats* st) { ctx->eval->tlwe_extract_device(count, d_tlwe, d_coef_of, d_u, st); });
    });
}

int ieache_tlwe_extract(ieache_ctx* ctx, size_t count, const int32_t* tlwe, const int32_t* coef_of, int32_t* u, ieache_stats* stats) {
    return guarded([&] {
        if (const int rc = check_rows({ctx, tlwe, u})) return rc;
        if (const int rc = check_indices(coef_of, count, ctx->eval->params().N, "tlwe_extract", "coef_of")) return rc;
        HostCall h(ctx, count);
        const size_t sample = (size_t)2 * (size_t)h.p.N;
        StagedRows dt(h.ev, kStageTlweA, count, sample, tlwe, sample), dof = h.words(kStagePolyOf, coef_of, count), du = h.results(count, true);
        with_stats(stats, [&](EvalStats* st) { h.ev.tlwe_extract_device(count, dt.p, dof.p, du.p, st); });
        h.download(du, u, true);
        return 0;
    });
}

// ---- the way back to the gates (section 3m).  unpack_plan.h states what the calls accept; word_read is kWordRead of
// set_calls.h, lut_read's row under its own name. ----
static_assert(kUnpackNoKeyswitch == IEACHE_UNPACK_NO_KEYSWITCH && IEACHE_UNPACK_NO_KEYSWITCH == IEACHE_LUT_READ_NO_KEYSWITCH,
              "unpack_plan.h knows the flag of include/ieache.h, and set_call_host reads it as lut_read's");
namespace {
int check_unpack(const ieache_ctx* ctx, size_t count, int32_t first, int32_t width, int32_t spread, int flags, const int32_t* in, const int32_t* out) {
    if (!ctx || (count && (!in || !out))) return fail(IEACHE_EINVAL, "null argument");
    if (const char* e = unpack_call_error(ctx->eval->params().N, first, width, spread, flags)) return fail(IEACHE_EINVAL, e);
    return 0;
}
extern "C++" SetCall word_read_call(size_t count, int32_t depth, int32_t steps, int32_t width, int32_t unit, int32_t n_tables, int flags) {
    return SetCall{kCallLutRead, count, depth, steps, n_tables, flags, 0, width, unit, true};
}
}  // namespace

int ieache_unpack_device(ieache_ctx* ctx, size_t count, int32_t first, int32_t width, int32_t spread, const int32_t* d_in, int flags, int32_t* d_out,
                         ieache_stats* stats) {
    return guarded([&] {
        if (const int rc = check_unpack(ctx, count, first, width, spread, flags, d_in, d_out)) return rc;
        require_device_pointers(count, {{d_in, "d_in"}, {d_out, "d_out"}});
        return with_stats(stats, [&](EvalStats* st) { ctx->eval->unpack_device(count, first, width, spread, flags, d_in, d_out, st); });
    });
}

int ieache_unpack(ieache_ctx* ctx, size_t count, int32_t first, int32_t width, int32_t spread, const int32_t* in, int flags, int32_t* out,
                  ieache_stats* stats) {
    return guarded([&] {
        if (const int rc = check_unpack(ctx, count, first, width, spread, flags, in, out)) return rc;
        const bool woks = (flags & IEACHE_UNPACK_NO_KEYSWITCH) != 0;
        HostCall h(ctx, count);
        const size_t sample = (size_t)2 * (size_t)h.p.N;
        StagedRows din(h.ev, kStageTlweA, count, sample, in, sample), dout = h.results(count * (size_t)width, woks);
        with_stats(stats, [&](EvalStats* st) { h.ev.unpack_device(count, first, width, spread, flags, din.p, dout.p, st); });
        h.download(dout, out, woks);
        return 0;
    });
}

int ieache_word_read_device(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, int32_t steps, int32_t width, int32_t unit,
                            const int32_t* d_sel_of, const int32_t* d_tables, int32_t n_tables, const int32_t* d_table_of, int flags, int32_t* d_out,
                            ieache_stats* stats) {
    return set_call_device(ctx, set, word_read_call(count, depth, steps, width, unit, n_tables, flags), {d_sel_of, nullptr, d_tables, d_table_of, d_out}, stats,
                           [&](EvalStats* st) {
                               ctx->eval->word_read_device(*set->set, count, depth, steps, width, unit, d_sel_of, d_tables, n_tables, d_table_of, flags, d_out, st);
                           });
}

int ieache_word_read(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, int32_t steps, int32_t width, int32_t unit, const int32_t* sel_of,
                     const int32_t* tables, int32_t n_tables, const int32_t* table_of, int flags, int32_t* out, ieache_stats* stats) {
    return set_call_host(ctx, set, word_read_call(count, depth, steps, width, unit, n_tables, flags), {sel_of, nullptr, tables, table_of, out}, out, stats,
                         [&](Evaluator& ev, Torus32* const* d, EvalStats* st) {
                             ev.word_read_device(*set->set, count, depth, steps, width, unit, d[0], d[2], n_tables, d[3], flags, d[4], st);
                         });
}

int ieache_lut_factor_poly(const ieache_params* p, int32_t entries, const int32_t* w, int32_t* P) {
    if (!p || !w || !P) return fail(IEACHE_EINVAL, "null argument");
    const int64_t N = p->N;
    if (N < 2 || entries < 1 || N % (2 * (int64_t)entries) != 0) return fail(IEACHE_EINVAL, "lut_factor_poly: 2 x entries must divide N");
    // v as ieache_lut_test_poly lays the table out, then P = v (1 - X): P[0] = v[0] + v[N-1], P[j] = v[j] - v[j-1]
    const int64_t half_slot = N / (2 * (int64_t)entries);
    auto v = [&](int64_t j) -> uint32_t {
        const int64_t e = (j + half_slot) * entries / N;
        return e < entries ? (uint32_t)w[e] : 0u - (uint32_t)w[0];
    };
    P[0] = (int32_t)(v(0) + v(N - 1));
    for (int64_t j = 1; j < N; j++) P[j] = (int32_t)(v(j) - v(j - 1));
    g_err.clear();
    return 0;
}

int ieache_lut_test_poly(const ieache_params* p, int32_t entries, const int32_t* f, int32_t* v) {
    if (!p || !f || !v) return fail(IEACHE_EINVAL, "null argument");
    const int64_t N = p->N;
    if (N < 2 || entries < 1 || N % (2 * (int64_t)entries) != 0) return fail(IEACHE_EINVAL, "lut_test_poly: 2 x entries must divide N");
    const int64_t half_slot = N / (2 * (int64_t)entries);
    for (int64_t j = 0; j < N; j++) {
        const int64_t e = (j + half_slot) * entries / N;  // the slot centred on message e covers phases (e -+ 1/2) / (2 entries)
        v[j] = e < entries ? f[e] : (int32_t)(0u - (uint32_t)f[0]);  // past the last slot: f[0] through the negacyclic wrap
    }
    g_err.clear();
    return 0;
}

int ieache_debug_blind_rotate(ieache_ctx* ctx, size_t count, const int32_t* x, int32_t* acc, int32_t steps) {
    return guarded([&] {
        if (!ctx || !x || !acc) return fail(IEACHE_EINVAL, "null argument");
        const Params& p = ctx->eval->params();
        HIP_CHECK(hipSetDevice(ctx->eval->device()));
        DevRows dx(count, p.lwe_stride()), dacc(count, (size_t)2 * p.N);
        dx.upload(x, p.n + 1);
        ctx->eval->debug_blind_rotate(count, dx.p, dacc.p, steps);
        dacc.download(acc, (size_t)2 * p.N);
        return 0;
    });
}

int ieache_debug_keyswitch(ieache_ctx* ctx, size_t count, const int32_t* u, int32_t* out) {
    return guarded([&] {
        if (!ctx || !u || !out) return fail(IEACHE_EINVAL, "null argument");
        const Params& p = ctx->eval->params();
        HIP_CHECK(hipSetDevice(ctx->eval->device()));
        DevRows du(count, (size_t)p.N + 1), dout(count, p.lwe_stride());
        du.upload(u, (size_t)p.N + 1);
        ctx->eval->debug_keyswitch(count, du.p, dout.p);
        dout.download(out, p.n + 1);
        return 0;
    });
}

// the transform probe: the evaluator checks every argument before it writes (its refusals: std::invalid_argument -> EINVAL)
int ieache_debug_twiddles(ieache_ctx* ctx, int which, double* out) {
    return guarded([&] {
        if (!ctx || !out) return fail(IEACHE_EINVAL, "null argument");
        ctx->eval->debug_twiddles(which, out);
        return 0;
    });
}

int ieache_debug_fft512(ieache_ctx* ctx, int form, size_t count, const double* in, double* out) {
    return guarded([&] {
        if (!ctx || !in || !out) return fail(IEACHE_EINVAL, "null argument");
        ctx->eval->debug_fft512(form, count, in, out);
        return 0;
    });
}

int ieache_debug_spectrum(ieache_ctx* ctx, int which, size_t first, size_t count, double* out) {
    return guarded([&] {
        if (!ctx || !out) return fail(IEACHE_EINVAL, "null argument");
        ctx->eval->debug_spectrum(which, first, count, out);
        return 0;
    });
}

int ieache_debug_forward_path(int xlane) {
    return guarded([&] {
        probe::set_w1b_forward_path(xlane);  // its refusal: std::invalid_argument -> EINVAL
        return 0;
    });
}

// ---- 2b. device group: one key on several GPUs, one call ----
struct ieache_group {
    std::unique_ptr<DeviceGroup> g;
    bool precheck = true;  // "precheck" (ieache_group_set_option)
    ieache_ctx* member(size_t m) const { return g->member(m); }
    size_t size() const { return g->size(); }
};

extern "C++" {
namespace {
// what a member's entry point returned on its thread, carried to the caller's: g_err is thread_local
struct MemberFailure {
    size_t member;
    int rc;
    std::string message;
};
// One group call over `count` independent rows: call(member context, first row, rows, the member's statistics or null) -- an
// existing host entry point on the member's slice of the caller's arrays -- for every member with rows, side by side
// (run_sliced: member 0 on this thread, no thread outlives the call).  count == 0: member 0 alone makes the call.  -> 0, or
// the code of the lowest-numbered member that failed, its message behind "member M (device D): ".
template <class Call>
int group_call(ieache_group* grp, size_t count, ieache_stats* stats, Call&& call) {
    for (size_t m = 0; stats && m < grp->size(); m++) memset(&stats[m], 0, sizeof stats[m]);  // a member without rows reports zeros
    if (count == 0) return call(grp->member(0), (size_t)0, (size_t)0, stats);
    try {
        run_sliced(grp->size(), count, [&](size_t m, size_t first, size_t rows) {
            const int rc = call(grp->member(m), first, rows, stats ? stats + m : nullptr);
            if (rc < 0) throw MemberFailure{m, rc, ieache_last_error()};
        });
    } catch (const MemberFailure& f) {
        return fail(f.rc, grp->g->member_label(f.member) + f.message);
    }
    g_err.clear();
    return 0;
}
template <class Make>
ieache_group* make_group(Make&& make) {
    ieache_group* grp = nullptr;
    guarded([&] {
        std::unique_ptr<ieache_group> made(new ieache_group);
        made->g = make();
        grp = made.release();
        return 0;
    });
    return grp;
}
const char* const kNullGroup = "null group";
// rows member 0 takes of `count`: the batch its circuit is chosen for
size_t first_slice(const ieache_group* grp, size_t count) {
    size_t first = 0, rows = 0;
    shard_slice(count, grp->size(), 0, &first, &rows);
    return rows;
}
// a member's share of a caller's array: `words` further on; a null array stays null for the member's own check to find
template <class T>
T* at(T* rows, size_t words) {
    return rows ? rows + words : nullptr;
}
}  // namespace
}  // extern "C++"

ieache_group* ieache_group_create(const char* cloud_key_path, const int* devices, int n_devices) {
    return make_group([&] {
        DeviceGroup::validate_devices(devices, n_devices);
        if (!cloud_key_path) throw std::invalid_argument("null cloud_key_path");
        return DeviceGroup::from_file(cloud_key_path, devices, n_devices);
    });
}

ieache_group* ieache_group_create_raw(const ieache_params* p, const int32_t* bk, const int32_t* ksk, const int* devices, int n_devices) {
    return make_group([&] {
        DeviceGroup::validate_devices(devices, n_devices);
        if (!p) throw std::invalid_argument("null params");
        return std::unique_ptr<DeviceGroup>(new DeviceGroup(to_params(*p), bk, ksk, devices, n_devices));
    });
}

void ieache_group_destroy(ieache_group* g) {
    try {
        delete g;
    } catch (...) {
    }
}

int ieache_group_size(const ieache_group* g) { return g ? (int)g->size() : fail(IEACHE_EINVAL, kNullGroup); }

int ieache_group_device(const ieache_group* g, int member) {
    if (!g || member < 0 || (size_t)member >= g->size()) return fail(IEACHE_EINVAL, g ? "no such member" : kNullGroup);
    return g->g->device((size_t)member);
}

ieache_ctx* ieache_group_ctx(ieache_group* g, int member) {
    if (!g || member < 0 || (size_t)member >= g->size()) {
        fail(IEACHE_EINVAL, g ? "no such member" : kNullGroup);
        return nullptr;
    }
    return g->member((size_t)member);
}

int ieache_group_set_option(ieache_group* g, const char* name, int64_t value) {
    if (!g || !name) return fail(IEACHE_EINVAL, g ? "null argument" : kNullGroup);
    if (std::string(name) == "precheck") {
        if (value != 0 && value != 1) return fail(IEACHE_EINVAL, "precheck takes 0 or 1");
        g->precheck = value != 0;
        return 0;
    }
    return guarded([&] {
        std::vector<int64_t> before(g->size());
        for (size_t m = 0; m < g->size(); m++)
            if (const int rc = ieache_ctx_get_option(g->member(m), name, &before[m])) return rc;  // no such option
        // member 0's row judges the value first; a later refusal (a hook that asks the device) puts the earlier members back
        for (size_t m = 0; m < g->size(); m++) {
            const int rc = ieache_ctx_set_option(g->member(m), name, value);
            if (rc == 0) continue;
            const std::string why = g->g->member_label(m) + ieache_last_error();
            for (size_t j = 0; j < m; j++) (void)ieache_ctx_set_option(g->member(j), name, before[j]);
            return fail(rc, why);
        }
        return 0;
    });
}

int ieache_group_prepare_batch(ieache_group* g, int kind, int bits, size_t batch) {
    if (!g) return fail(IEACHE_EINVAL, kNullGroup);
    return guarded([&] {
        CircuitCache::Ptr c;
        if (g->precheck)
            if (const int rc = check_prepare(g->member(0), kind, bits, first_slice(g, batch), &c)) return rc;
        return group_call(g, batch, nullptr, [&](ieache_ctx* ctx, size_t, size_t n, ieache_stats*) { return ieache_prepare_batch(ctx, kind, bits, n); });
    });
}

int ieache_group_eval_batch(ieache_group* g, int kind, int bits, size_t batch, const int32_t* in_lwe, int32_t* out_lwe, ieache_stats* stats) {
    if (!g) return fail(IEACHE_EINVAL, kNullGroup);
    return guarded([&] {
        // rows per expression come from the circuit, so this check is made whatever "precheck" says
        CircuitCache::Ptr c;
        if (const int rc = check_batch(g->member(0), kind, bits, first_slice(g, batch), in_lwe, out_lwe, &c)) return rc;
        const size_t S = (size_t)c->n_inputs * (size_t)(g->member(0)->eval->params().n + 1), T = c->outputs.size() * (size_t)(g->member(0)->eval->params().n + 1);
        return group_call(g, batch, stats, [&](ieache_ctx* ctx, size_t first, size_t n, ieache_stats* st) {
            return ieache_eval_batch(ctx, kind, bits, n, at(in_lwe, first * S), at(out_lwe, first * T), st);
        });
    });
}

int ieache_group_prepare_netlist(ieache_group* g, const ieache_netlist* nl, size_t batch) {
    if (!g) return fail(IEACHE_EINVAL, kNullGroup);
    return guarded([&] {
        if (g->precheck)
            if (const int rc = check_rows({g->member(0), nl})) return rc;
        return group_call(g, batch, nullptr, [&](ieache_ctx* ctx, size_t, size_t n, ieache_stats*) { return ieache_prepare_netlist(ctx, nl, n); });
    });
}

int ieache_group_eval_netlist(ieache_group* g, const ieache_netlist* nl, size_t batch, const int32_t* in_lwe, int32_t* out_lwe, ieache_stats* stats) {
    if (!g) return fail(IEACHE_EINVAL, kNullGroup);
    return guarded([&] {
        if (const int rc = check_rows({g->member(0), nl, in_lwe, out_lwe})) return rc;  // the netlist gives the rows per expression
        const size_t W = (size_t)g->member(0)->eval->params().n + 1, S = (size_t)nl->circuit.n_inputs * W, T = nl->circuit.outputs.size() * W;
        return group_call(g, batch, stats, [&](ieache_ctx* ctx, size_t first, size_t n, ieache_stats* st) {
            return ieache_eval_netlist(ctx, nl, n, at(in_lwe, first * S), at(out_lwe, first * T), st);
        });
    });
}

// Every job's batch cut over the members (shard_jobs): a member is one "row" of run_sliced, so each runs on its own thread
// whatever the batches are; one whose slices are all empty does nothing and reports zeros.
int ieache_group_eval_jobs(ieache_group* g, const ieache_job* jobs, size_t n_jobs, ieache_stats* stats) {
    if (!g) return fail(IEACHE_EINVAL, kNullGroup);
    return guarded([&] {
        // rows per expression come from the circuits, so this check is made whatever "precheck" says
        ResolvedJobs r;
        if (const int rc = resolve_jobs(g->member(0), jobs, n_jobs, true, &r)) return rc;
        const size_t W = (size_t)g->member(0)->eval->params().n + 1;
        std::vector<size_t> in_words(n_jobs, 0), out_words(n_jobs, 0);
        for (size_t j = 0; j < n_jobs; j++) {
            if (!r.jobs[j].batch) continue;
            in_words[j] = (size_t)r.jobs[j].circuit->n_inputs * W;
            out_words[j] = r.jobs[j].circuit->outputs.size() * W;
        }
        return group_call(g, g->size(), stats, [&](ieache_ctx* ctx, size_t m, size_t, ieache_stats* st) {
            std::vector<ieache_job> mine;
            shard_jobs(jobs, n_jobs, in_words.data(), out_words.data(), g->size(), m, &mine);
            if (mine.empty()) return 0;
            return ieache_eval_jobs(ctx, mine.data(), mine.size(), st);
        });
    });
}

int ieache_group_gates(ieache_group* g, int gate_type, size_t count, const int32_t* a, const int32_t* b, int32_t* out, ieache_stats* stats) {
    if (!g) return fail(IEACHE_EINVAL, kNullGroup);
    return guarded([&] {
        if (g->precheck)
            if (const int rc = check_gates(g->member(0), gate_type, a, b, out)) return rc;
        const size_t W = (size_t)g->member(0)->eval->params().n + 1;
        return group_call(g, count, stats, [&](ieache_ctx* ctx, size_t first, size_t n, ieache_stats* st) {
            return ieache_gates(ctx, gate_type, n, at(a, first * W), at(b, first * W), at(out, first * W), st);
        });
    });
}

int ieache_group_gates3(ieache_group* g, int gate_type, size_t count, const int32_t* a, const int32_t* b, const int32_t* c, int32_t* out,
                        ieache_stats* stats) {
    if (!g) return fail(IEACHE_EINVAL, kNullGroup);
    return guarded([&] {
        if (g->precheck)
            if (const int rc = check_gates3(g->member(0), gate_type, a, b, c, out)) return rc;
        const size_t W = (size_t)g->member(0)->eval->params().n + 1;
        return group_call(g, count, stats, [&](ieache_ctx* ctx, size_t first, size_t n, ieache_stats* st) {
            return ieache_gates3(ctx, gate_type, n, at(a, first * W), at(b, first * W), at(c, first * W), at(out, first * W), st);
        });
    });
}

int ieache_group_mux(ieache_group* g, size_t count, const int32_t* a, const int32_t* b, const int32_t* c, int32_t* out, ieache_stats* stats) {
    if (!g) return fail(IEACHE_EINVAL, kNullGroup);
    return guarded([&] {
        if (g->precheck)
            if (const int rc = check_rows({g->member(0), a, b, c, out})) return rc;
        const size_t W = (size_t)g->member(0)->eval->params().n + 1;
        return group_call(g, count, stats, [&](ieache_ctx* ctx, size_t first, size_t n, ieache_stats* st) {
            return ieache_mux(ctx, n, at(a, first * W), at(b, first * W), at(c, first * W), at(out, first * W), st);
        });
    });
}

int ieache_group_pbs(ieache_group* g, size_t count, const int32_t* x, const int32_t* test_polys, int32_t n_polys, const int32_t* poly_of,
                     int32_t* out, int flags, ieache_stats* stats) {
    if (!g) return fail(IEACHE_EINVAL, kNullGroup);
    return guarded([&] {
        if (g->precheck)
            if (const int rc = check_pbs(g->member(0), count, x, test_polys, n_polys, poly_of, out, flags)) return rc;
        // rows in: n + 1 words; rows out: N + 1 without the key switch.  The table goes to every member whole, the indices with the rows.
        const Params& p = g->member(0)->eval->params();
        const size_t W = (size_t)p.n + 1, V = pbs_out_words(p, flags);  // 2N for whole accumulators
        return group_call(g, count, stats, [&](ieache_ctx* ctx, size_t first, size_t n, ieache_stats* st) {
            return ieache_pbs(ctx, n, at(x, first * W), test_polys, n_polys, at(poly_of, first), at(out, first * V), flags, st);
        });
    });
}

int ieache_group_pbs_multi(ieache_group* g, size_t count, const int32_t* x, const int32_t* test_polys, int32_t n_polys, const int32_t* poly_of,
                           const int32_t* factors, int32_t n_factors, const int32_t* bias, int32_t* out, int flags, ieache_stats* stats) {
    if (!g) return fail(IEACHE_EINVAL, kNullGroup);
    return guarded([&] {
        if (g->precheck)
            if (const int rc = check_pbs_multi(g->member(0), count, x, test_polys, n_polys, poly_of, factors, n_factors, out, flags)) return rc;
        // as ieache_group_pbs; factors and bias go to every member whole, and a member's output starts at row first x n_factors
        const Params& p = g->member(0)->eval->params();
        const size_t W = (size_t)p.n + 1, V = (flags & IEACHE_PBS_NO_KEYSWITCH) ? (size_t)p.N + 1 : W;
        const size_t F = n_factors > 0 ? (size_t)n_factors : 0;  // a refused n_factors (precheck off) moves no pointer
        return group_call(g, count, stats, [&](ieache_ctx* ctx, size_t first, size_t n, ieache_stats* st) {
            return ieache_pbs_multi(ctx, n, at(x, first * W), test_polys, n_polys, at(poly_of, first), factors, n_factors, bias,
                                    at(out, first * F * V), flags, st);
        });
    });
}

// ---------------- CPU tools ----------------
int ieache_keygen_raw(const ieache_params* p, const uint32_t* seed_words, int n_seed_words, int32_t* lwe_key,
                      int32_t* tlwe_key, int32_t* bk, int32_t* ksk) {
    return guarded([&] {
        if (!p) return fail(IEACHE_EINVAL, "null params");
        const Params pp = to_params(*p);
        if (!pp.supported()) return fail(IEACHE_EINVAL, "unsupported parameter set");
        SecretKeyData sk;
        keygen(pp, seed_words, n_seed_words, &sk, bk != nullptr || ksk != nullptr);
        if (lwe_key) memcpy(lwe_key, sk.lwe_key.data(), sk.lwe_key.size() * 4);
        if (tlwe_key) memcpy(tlwe_key, sk.tlwe_key.data(), sk.tlwe_key.size() * 4);
        if (bk) memcpy(bk, sk.cloud.bk.data(), sk.cloud.bk.size() * 4);
        if (ksk) memcpy(ksk, sk.cloud.ksk.data(), sk.cloud.ksk.size() * 4);
        return 0;
    });
}

int ieache_keygen_files(const char* dir, const ieache_params* p, const uint32_t* seed, int n_seed,
                        const uint32_t* nbit_seed, int n_nbit_seed) {
    return guarded([&] {
        const std::string d = dir ? dir : ".";
        Params pp;
        if (p) pp = to_params(*p);
        if (!pp.supported()) return fail(IEACHE_EINVAL, "unsupported parameter set");
        static const uint32_t kSeed[3] = {314, 1592, 657}, kBitSeed[3] = {314, 1592, 888};  // keygen.c:30,34
        if (!seed && n_seed >= 0) {
            seed = kSeed;
            n_seed = 3;
        }
        if (!nbit_seed && n_nbit_seed >= 0) {
            nbit_seed = kBitSeed;
            n_nbit_seed = 3;
        }
        SecretKeyData key, nbit;
        keygen(pp, seed, n_seed, &key, true);
        save_secret_key(d + "/secret.key", key);   // keygen.c:38-40
        save_cloud_key(d + "/cloud.key", key.cloud);  // :43-45
        keygen(pp, nbit_seed, n_nbit_seed, &nbit, true);
        save_secret_key(d + "/nbit.key", nbit);  // :48-50
        return 0;
    });
}

int ieache_encrypt_bits(const ieache_params* p, const int32_t* lwe_key, const uint8_t* bits, size_t count,
                        uint64_t seed, int32_t* out) {
    return guarded([&] {
        if (!p || !lwe_key || !bits || !out) return fail(IEACHE_EINVAL, "null argument");
        const Params pp = to_params(*p);
        Rng rng = seed ? Rng(seed) : Rng::secure();
        for (size_t i = 0; i < count; i++) lwe_encrypt_bit(pp, lwe_key, bits[i] & 1, rng, out + i * (size_t)(pp.n + 1));
        return 0;
    });
}

int ieache_tlwe_encrypt(const ieache_params* p, const int32_t* tlwe_key, const int32_t* polys, size_t count, double alpha, uint64_t seed,
                        int32_t* out) {
    return guarded([&] {
        if (!p || !tlwe_key || (count && (!polys || !out))) return fail(IEACHE_EINVAL, "null argument");
        const Params pp = to_params(*p);
        if (pp.k != 1 || pp.N < 1) return fail(IEACHE_EINVAL, "tlwe_encrypt: k must be 1 and N positive");
        Rng rng = seed ? Rng(seed) : Rng::secure();
        tlwe_encrypt(pp, tlwe_key, polys, count, alpha > 0 ? alpha : pp.tlwe_alpha_min, rng, out);
        return 0;
    });
}

int ieache_packing_keygen(const ieache_params* p, const int32_t* lwe_key, const int32_t* tlwe_key, int32_t pk_t, int32_t pk_basebit, double alpha,
                          uint64_t seed, int32_t* out) {
    return guarded([&] {
        if (!p || !lwe_key || !tlwe_key || !out) return fail(IEACHE_EINVAL, "null argument");
        const Params pp = to_params(*p);
        if (const char* e = pack_set_error(pp, pk_t, pk_basebit)) return fail(IEACHE_EINVAL, e);
        Rng rng = seed ? Rng(seed) : Rng::secure();
        packing_keygen(pp, lwe_key, tlwe_key, pk_t, pk_basebit, alpha > 0 ? alpha : pp.tlwe_alpha_min, rng, out);
        return 0;
    });
}

int ieache_pack_reference(const ieache_params* p, int32_t pk_t, int32_t pk_basebit, const int32_t* pk, size_t groups, int32_t m, int32_t spread,
                          int32_t shift, const int32_t* rows, int32_t* out) {
    return guarded([&] {
        if (!p || !pk || (groups && (!rows || !out))) return fail(IEACHE_EINVAL, "null argument");
        const Params pp = to_params(*p);
        if (const char* e = pack_set_error(pp, pk_t, pk_basebit)) return fail(IEACHE_EINVAL, e);
        if (const char* e = pack_call_error(pp, m, spread, shift)) return fail(IEACHE_EINVAL, e);
        pack_reference(pp, pk_t, pk_basebit, pk, groups, m, spread, shift, rows, out);
        return 0;
    });
}

int ieache_tgsw_encrypt(const ieache_params* p, const int32_t* tlwe_key, const int32_t* mu, size_t count, double alpha, uint64_t seed, int32_t* out) {
    return guarded([&] {
        if (!p || !tlwe_key || (count && (!mu || !out))) return fail(IEACHE_EINVAL, "null argument");
        const Params pp = to_params(*p);
        if (!pp.supported()) return fail(IEACHE_EINVAL, "tgsw_encrypt: unsupported TFHE parameter set");
        Rng rng = seed ? Rng(seed) : Rng::secure();
        const size_t sample = (size_t)pp.kpl() * 2 * (size_t)pp.N;
        for (size_t i = 0; i < count; i++) tgsw_encrypt_sample(pp, tlwe_key, mu[i], alpha > 0 ? alpha : pp.tlwe_alpha_min, rng, out + i * sample);
        return 0;
    });
}

int ieache_cmux_reference(const ieache_params* p, const int32_t* set, size_t n, size_t count, const int32_t* sel_of, const int32_t* d1,
                          const int32_t* d0, int32_t* out) {
    return guarded([&] {
        if (!p || !set || (count && (!d1 || !out))) return fail(IEACHE_EINVAL, "null argument");
        const Params pp = to_params(*p);
        if (!pp.supported()) return fail(IEACHE_EINVAL, "cmux_reference: unsupported TFHE parameter set");
        if (n < 1) return fail(IEACHE_EINVAL, "cmux_reference: no samples");
        if (const int rc = check_set_indices({kCallCmux, count}, {sel_of, d1, d0, out}, pp.N, n)) return rc;
        cmux_reference(pp, set, n, count, sel_of, d1, d0, out);
        return 0;
    });
}

int ieache_lut_tree_reference(const ieache_params* p, const int32_t* set, size_t n, size_t count, int32_t depth, const int32_t* sel_of,
                              const int32_t* tables, int32_t n_tables, const int32_t* table_of, int32_t* out) {
    return guarded([&] {
        if (!p || !set || (count && (!tables || !out))) return fail(IEACHE_EINVAL, "null argument");
        const Params pp = to_params(*p);
        if (!pp.supported()) return fail(IEACHE_EINVAL, "lut_tree_reference: unsupported TFHE parameter set");
        if (n < 1) return fail(IEACHE_EINVAL, "lut_tree_reference: no samples");
        if (const int rc = check_set_indices({kCallLutTree, count, depth, 0, n_tables}, {sel_of, tables, table_of, out}, pp.N, n)) return rc;
        lut_tree_reference(pp, set, n, count, depth, sel_of, tables, table_of, out);
        return 0;
    });
}

int ieache_lut_scatter_reference(const ieache_params* p, const int32_t* set, size_t n, size_t count, int32_t depth, const int32_t* sel_of,
                                 const int32_t* values, const int32_t* mem, int32_t* out) {
    return guarded([&] {
        if (!p || !set || (count && (!values || !out))) return fail(IEACHE_EINVAL, "null argument");
        const Params pp = to_params(*p);
        if (!pp.supported()) return fail(IEACHE_EINVAL, "lut_scatter_reference: unsupported TFHE parameter set");
        if (n < 1) return fail(IEACHE_EINVAL, "lut_scatter_reference: no samples");
        if (const int rc = check_set_indices({kCallLutScatter, count, depth}, {sel_of, values, mem, out}, pp.N, n)) return rc;
        lut_scatter_reference(pp, set, n, count, depth, sel_of, values, mem, out);
        return 0;
    });
}

int ieache_tlwe_rotate_reference(const ieache_params* p, const int32_t* set, size_t n, size_t count, int32_t steps, const int32_t* sel_of,
                                 const int32_t* amount_of, const int32_t* in, int32_t* out) {
    return guarded([&] {
        if (!p || !set || (count && (!in || !out))) return fail(IEACHE_EINVAL, "null argument");
        const Params pp = to_params(*p);
        if (!pp.supported()) return fail(IEACHE_EINVAL, "tlwe_rotate_reference: unsupported TFHE parameter set");
        if (n < 1) return fail(IEACHE_EINVAL, "tlwe_rotate_reference: no samples");
        if (const int rc = check_set_indices({kCallTlweRotate, count, 0, steps}, {sel_of, amount_of, in, out}, pp.N, n)) return rc;
        tlwe_rotate_reference(pp, set, n, count, steps, sel_of, amount_of, in, out);
        return 0;
    });
}

int ieache_lut_read_reference(const ieache_params* p, const int32_t* set, size_t n, const int32_t* ksk, size_t count, int32_t depth, int32_t steps,
                              const int32_t* sel_of, const int32_t* amount_of, const int32_t* tables, int32_t n_tables, const int32_t* table_of,
                              int32_t coef, int flags, int32_t* out) {
    return guarded([&] {
        if (!p || !set || (count && (!tables || !out))) return fail(IEACHE_EINVAL, "null argument");
        const Params pp = to_params(*p);
        if (!pp.supported()) return fail(IEACHE_EINVAL, "lut_read_reference: unsupported TFHE parameter set");
        if (n < 1) return fail(IEACHE_EINVAL, "lut_read_reference: no samples");
        const SetCall c{kCallLutRead, count, depth, steps, n_tables, flags, coef};
        if (const int rc = check_set_scalars(c, pp.N)) return rc;
        const bool woks = (flags & IEACHE_LUT_READ_NO_KEYSWITCH) != 0;
        if (!woks && !ksk) return fail(IEACHE_EINVAL, "lut_read_reference: the key switch needs ksk");
        if (const int rc = check_set_indices(c, {sel_of, amount_of, tables, table_of, out}, pp.N, n)) return rc;
        lut_read_reference(pp, set, n, woks ? nullptr : ksk, count, depth, steps, sel_of, amount_of, tables, table_of, coef, out);
        return 0;
    });
}

int ieache_lut_add_reference(const ieache_params* p, const int32_t* set, size_t n, size_t count, int32_t depth, int32_t steps, const int32_t* sel_of,
                             const int32_t* amount_of, const int32_t* values, const int32_t* mems, int32_t n_mems, const int32_t* mem_of, int32_t* out) {
    return guarded([&] {
        if (!p || !set || (count && !values) || !out) return fail(IEACHE_EINVAL, "null argument");
        const Params pp = to_params(*p);
        if (!pp.supported()) return fail(IEACHE_EINVAL, "lut_add_reference: unsupported TFHE parameter set");
        if (n < 1) return fail(IEACHE_EINVAL, "lut_add_reference: no samples");
        if (const int rc = check_set_indices({kCallLutAdd, count, depth, steps, n_mems}, {sel_of, amount_of, values, mems, mem_of, out}, pp.N, n)) return rc;
        lut_add_reference(pp, set, n, count, depth, steps, sel_of, amount_of, values, mems, (size_t)n_mems, mem_of, out);
        return 0;
    });
}

int ieache_automaton_reference(const ieache_params* p, const int32_t* set, size_t n, int32_t states, int32_t steps, int32_t n_out, const int32_t* next0,
                               const int32_t* next1, size_t count, const int32_t* sel_of, const int32_t* finals, int32_t n_finals, const int32_t* final_of,
                               int32_t* out) {
    return guarded([&] {
        if (!p || !set || (count && (!finals || !out))) return fail(IEACHE_EINVAL, "null argument");
        const Params pp = to_params(*p);
        if (!pp.supported()) return fail(IEACHE_EINVAL, "automaton_reference: unsupported TFHE parameter set");
        if (n < 1) return fail(IEACHE_EINVAL, "automaton_reference: no samples");
        const std::string refusal = automaton_refusal(states, steps, n_out, next0, next1);
        if (!refusal.empty()) return fail(IEACHE_EINVAL, refusal);
        if (n_finals < 1) return fail(IEACHE_EINVAL, "automaton_run: n_finals must be at least 1");
        if (const int rc = check_indices(sel_of, count * (size_t)steps, (int64_t)n, "automaton_run", "sel_of")) return rc;
        if (const int rc = check_indices(final_of, count, n_finals, "automaton_run", "final_of")) return rc;
        automaton_reference(pp, set, n, states, steps, n_out, next0, next1, count, sel_of, finals, final_of, out);
        return 0;
    });
}

int ieache_lwe_linear_reference(const ieache_params* p, int rows, size_t batch, int32_t n_out, int32_t n_in, const int8_t* w, const int32_t* bias,
                                const int32_t* x, int32_t* out) {
    return guarded([&] {
        if (const char* e = linear_scalar_error(rows, n_out, n_in, bias != nullptr)) return fail(IEACHE_EINVAL, e);
        if (!p) return fail(IEACHE_EINVAL, kLinearNull);
        const Params pp = to_params(*p);
        if (!pp.supported()) return fail(IEACHE_EINVAL, "lwe_linear_reference: unsupported TFHE parameter set");
        LinearCall c;
        c.rows = rows, c.batch = batch, c.n_out = n_out, c.n_in = n_in, c.w = w, c.bias = bias, c.x = x, c.out = out;
        if (const char* e = linear_call_error(pp, c)) return fail(IEACHE_EINVAL, e);
        lwe_linear_reference(linear_rows(pp, rows), batch, n_out, n_in, w, bias, x, out);
        return 0;
    });
}

int ieache_tlwe_extract_reference(const ieache_params* p, size_t count, const int32_t* tlwe, const int32_t* coef_of, int32_t* u) {
    return guarded([&] {
        if (!p || (count && (!tlwe || !u))) return fail(IEACHE_EINVAL, "null argument");
        const Params pp = to_params(*p);
        if (!pp.supported()) return fail(IEACHE_EINVAL, "tlwe_extract_reference: unsupported TFHE parameter set");
        if (const int rc = check_indices(coef_of, count, pp.N, "tlwe_extract", "coef_of")) return rc;
        tlwe_extract_reference(pp, count, tlwe, coef_of, u);
        return 0;
    });
}

int ieache_tlwe_project_reference(const ieache_params* p, int32_t pk_t, int32_t pk_basebit, const int32_t* pk, size_t count, int32_t first, int32_t width,
                                  int32_t dest, const int32_t* in, int32_t* out) {
    return guarded([&] {
        if (!p || !pk || (count && (!in || !out))) return fail(IEACHE_EINVAL, "null argument");
        const Params pp = to_params(*p);
        if (const char* e = project_set_error(pp, pk_t, pk_basebit)) return fail(IEACHE_EINVAL, e);
        if (const char* e = project_call_error(pp, first, width, dest)) return fail(IEACHE_EINVAL, e);
        tlwe_project_reference(pp, pk_t, pk_basebit, pk, count, first, width, dest, in, out);
        return 0;
    });
}

int ieache_lut_write_coef_reference(const ieache_params* p, const int32_t* set, size_t n, int32_t pk_t, int32_t pk_basebit, const int32_t* pk, size_t count,
                                    int32_t depth, int32_t steps, int32_t width, int32_t unit, const int32_t* sel_of, const int32_t* fresh,
                                    const int32_t* mem, int32_t* out) {
    return guarded([&] {
        if (!p || !set || (count && (!fresh || !mem || !out))) return fail(IEACHE_EINVAL, "null argument");
        if (!pk) return fail(IEACHE_EINVAL, "lut_write_coef: no projection key set");
        const Params pp = to_params(*p);
        if (!pp.supported()) return fail(IEACHE_EINVAL, "lut_write_coef_reference: unsupported TFHE parameter set");
        if (n < 1) return fail(IEACHE_EINVAL, "lut_write_coef_reference: no samples");
        if (const char* e = project_set_error(pp, pk_t, pk_basebit)) return fail(IEACHE_EINVAL, e);
        if (const int rc = check_set_indices({kCallLutWriteCoef, count, depth, steps, 1, 0, 0, width, unit}, {sel_of, fresh, mem, out}, pp.N, n)) return rc;
        lut_write_coef_reference(pp, set, n, pk_t, pk_basebit, pk, count, depth, steps, width, unit, sel_of, fresh, mem, out);
        return 0;
    });
}

int ieache_unpack_reference(const ieache_params* p, const int32_t* ksk, size_t count, int32_t first, int32_t width, int32_t spread, const int32_t* in,
                            int flags, int32_t* out) {
    return guarded([&] {
        if (!p || (count && (!in || !out))) return fail(IEACHE_EINVAL, "null argument");
        const Params pp = to_params(*p);
        if (!pp.supported()) return fail(IEACHE_EINVAL, "unpack_reference: unsupported TFHE parameter set");
        if (const char* e = unpack_call_error(pp.N, first, width, spread, flags)) return fail(IEACHE_EINVAL, e);
        const bool woks = (flags & IEACHE_UNPACK_NO_KEYSWITCH) != 0;
        if (!woks && !ksk) return fail(IEACHE_EINVAL, "unpack_reference: the key switch needs ksk");
        unpack_reference(pp, woks ? nullptr : ksk, count, first, width, spread, in, out);
        return 0;
    });
}

int ieache_word_read_reference(const ieache_params* p, const int32_t* set, size_t n, const int32_t* ksk, size_t count, int32_t depth, int32_t steps,
                               int32_t width, int32_t unit, const int32_t* sel_of, const int32_t* tables, int32_t n_tables, const int32_t* table_of,
                               int flags, int32_t* out) {
    return guarded([&] {
        if (!p || !set || (count && (!tables || !out))) return fail(IEACHE_EINVAL, "null argument");
        const Params pp = to_params(*p);
        if (!pp.supported()) return fail(IEACHE_EINVAL, "word_read_reference: unsupported TFHE parameter set");
        if (n < 1) return fail(IEACHE_EINVAL, "word_read_reference: no samples");
        const SetCall c = word_read_call(count, depth, steps, width, unit, n_tables, flags);
        if (const int rc = check_set_scalars(c, pp.N)) return rc;
        const bool woks = (flags & IEACHE_UNPACK_NO_KEYSWITCH) != 0;
        if (!woks && !ksk) return fail(IEACHE_EINVAL, "word_read_reference: the key switch needs ksk");
        if (const int rc = check_set_indices(c, {sel_of, nullptr, tables, table_of, out}, pp.N, n)) return rc;
        word_read_reference(pp, set, n, woks ? nullptr : ksk, count, depth, steps, width, unit, sel_of, tables, table_of, out);
        return 0;
    });
}

int ieache_tlwe_phase(const ieache_params* p, const int32_t* tlwe_key, const int32_t* samples, size_t count, int32_t* phase) {
    return guarded([&] {
        if (!p || !tlwe_key || (count && (!samples || !phase))) return fail(IEACHE_EINVAL, "null argument");
        const Params pp = to_params(*p);
        if (pp.k != 1 || pp.N < 1) return fail(IEACHE_EINVAL, "tlwe_phase: k must be 1 and N positive");
        tlwe_phase(pp, tlwe_key, samples, count, phase);
        return 0;
    });
}

int ieache_decrypt_bits(const ieache_params* p, const int32_t* lwe_key, const int32_t* samples, size_t count,
                        uint8_t* bits) {
    return guarded([&] {
        if (!p || !lwe_key || !samples || !bits) return fail(IEACHE_EINVAL, "null argument");
        const Params pp = to_params(*p);
        for (size_t i = 0; i < count; i++) bits[i] = (uint8_t)lwe_decrypt_bit(pp, lwe_key, samples + i * (size_t)(pp.n + 1));
        return 0;
    });
}

int ieache_read_secret_key(const char* path, ieache_params* p, int32_t* lwe_key, int32_t* tlwe_key) {
    return guarded([&] {
        if (!path) return fail(IEACHE_EINVAL, "null path");
        SecretKeyData sk;
        load_secret_key(path, &sk, false);
        if (p) from_params(sk.p, p);
        if (lwe_key) memcpy(lwe_key, sk.lwe_key.data(), sk.lwe_key.size() * 4);
        if (tlwe_key) memcpy(tlwe_key, sk.tlwe_key.data(), sk.tlwe_key.size() * 4);
        return 0;
    });
}

int ieache_read_cloud_key(const char* path, ieache_params* p, int32_t* bk, int32_t* ksk) {
    return guarded([&] {
        if (!path) return fail(IEACHE_EINVAL, "null path");
        if (!bk && !ksk) {
            const Params pp = load_params(path);
            if (p) from_params(pp, p);
            return 0;
        }
        CloudKeyData ck;
        load_cloud_key(path, &ck);
        if (p) from_params(ck.p, p);
        if (bk) memcpy(bk, ck.bk.data(), ck.bk.size() * 4);
        if (ksk) memcpy(ksk, ck.ksk.data(), ck.ksk.size() * 4);
        return 0;
    });
}

int ieache_write_cloud_key(const char* path, const ieache_params* p, const int32_t* bk, const int32_t* ksk) {
    return guarded([&] {
        if (!path || !p || !bk || !ksk) return fail(IEACHE_EINVAL, "null argument");
        CloudKeyData ck;
        ck.p = to_params(*p);
        ck.bk.assign(bk, bk + ck.p.bk_count());
        ck.ksk.assign(ksk, ksk + ck.p.ksk_count());
        save_cloud_key(path, ck);
        return 0;
    });
}

int ieache_write_secret_key(const char* path, const ieache_params* p, const int32_t* lwe_key, const int32_t* tlwe_key,
                            const int32_t* bk, const int32_t* ksk) {
    return guarded([&] {
        if (!path || !p || !lwe_key || !tlwe_key || !bk || !ksk) return fail(IEACHE_EINVAL, "null argument");
        SecretKeyData sk;
        sk.p = to_params(*p);
        sk.lwe_key.assign(lwe_key, lwe_key + sk.p.n);
        sk.tlwe_key.assign(tlwe_key, tlwe_key + (size_t)sk.p.k * sk.p.N);
        sk.cloud.p = sk.p;
        sk.cloud.bk.assign(bk, bk + sk.p.bk_count());
        sk.cloud.ksk.assign(ksk, ksk + sk.p.ksk_count());
        save_secret_key(path, sk);
        return 0;
    });
}

int ieache_read_samples(const char* path, int32_t n, size_t first, size_t count, int32_t* out) {
    return guarded([&] {
        if (!path || !out || n < 1) return fail(IEACHE_EINVAL, "bad argument");
        FILE* f = fopen(path, "rb");
        if (!f) throw CodecError(std::string("cannot open ") + path);
        try {
            if (fseek(f, (long)(first * lwe_sample_bytes(n)), SEEK_SET) != 0) throw CodecError("seek failed");
            read_lwe_samples(f, n, count, out);
        } catch (...) {
            fclose(f);
            throw;
        }
        fclose(f);
        return 0;
    });
}

int ieache_write_samples(const char* path, int32_t n, size_t count, const int32_t* rows, int append) {
    return guarded([&] {
        if (!path || !rows || n < 1) return fail(IEACHE_EINVAL, "bad argument");
        FILE* f = fopen(path, append ? "ab" : "wb");
        if (!f) throw CodecError(std::string("cannot open ") + path);
        try {
            write_lwe_samples(f, n, count, rows, (size_t)n + 1);
        } catch (...) {
            fclose(f);
            throw;
        }
        fclose(f);
        return 0;
    });
}

int ieache_alice(const char* secret_key_path, const char* nbit_key_path, const char* cloud_data_path, int append,
                 uint32_t sign_code, uint32_t bit_size, const uint32_t* words, uint64_t seed) {
    return guarded([&] {
        if (!secret_key_path || !nbit_key_path || !cloud_data_path || !words) return fail(IEACHE_EINVAL, "null argument");
        SecretKeyData key, nbit;
        load_secret_key(secret_key_path, &key, false);
        load_secret_key(nbit_key_path, &nbit, false);
        if (key.p.n != nbit.p.n) throw CodecError("secret.key and nbit.key disagree on n");
        const size_t S = (size_t)key.p.n + 1;
        std::vector<Torus32> rows(352 * S);
        Rng rng = seed ? Rng(seed) : Rng::secure();
        auto enc_word = [&](const SecretKeyData& k, uint32_t v, size_t word_index) {
            for (int i = 0; i < 32; i++)  // alice.c:123-125: bit i of the word is sample i
                lwe_encrypt_bit(k.p, k.lwe_key.data(), (v >> i) & 1, rng, rows.data() + (word_index * 32 + i) * S);
        };
        enc_word(nbit, sign_code, 0);                            // alice.c:116-118
        enc_word(nbit, bit_size, 1);                             // :120-122
        for (int w = 0; w < 8; w++) enc_word(key, words[w], 2 + w);  // :123-146
        enc_word(key, 0, 10);                                    // :147-149 carry = 0
        FILE* f = fopen(cloud_data_path, append ? "ab" : "wb");
        if (!f) throw CodecError(std::string("cannot open ") + cloud_data_path);
        try {
            write_lwe_samples(f, key.p.n, 352, rows.data(), S);  // alice.c:167-191
        } catch (...) {
            fclose(f);
            throw;
        }
        fclose(f);
        return 0;
    });
}

int ieache_verif(const char* secret_key_path, const char* nbit_key_path, const char* answer_data_path,
                 uint32_t* sign_code, uint32_t* bit_size, uint32_t* words9) {
    return guarded([&] {
        if (!secret_key_path || !nbit_key_path || !answer_data_path) return fail(IEACHE_EINVAL, "null argument");
        SecretKeyData key, nbit;
        load_secret_key(secret_key_path, &key, false);
        load_secret_key(nbit_key_path, &nbit, false);
        const size_t S = (size_t)key.p.n + 1;
        std::vector<Torus32> rows(352 * S);
        FILE* f = fopen(answer_data_path, "rb");
        if (!f) throw CodecError(std::string("cannot open ") + answer_data_path);
        try {
            read_lwe_samples(f, key.p.n, 352, rows.data());
        } catch (...) {
            fclose(f);
            throw;
        }
        fclose(f);
        auto dec_word = [&](const SecretKeyData& k, size_t word_index) {
            uint32_t v = 0;
            for (int i = 0; i < 32; i++)  // verif.c:57-60, 92-95
                v |= (uint32_t)lwe_decrypt_bit(k.p, k.lwe_key.data(), rows.data() + (word_index * 32 + i) * S) << i;
            return v;
        };
        if (sign_code) *sign_code = dec_word(nbit, 0);
        if (bit_size) *bit_size = dec_word(nbit, 1);
        if (words9)
            for (int w = 0; w < 9; w++) words9[w] = dec_word(key, 2 + w);
        return 0;
    });
}

// ---- 5. resident-key daemon ----
int64_t ieache_serve(const char* socket_path, const char* cloud_key_path, const char* nbit_key_path, int device,
                     int64_t max_requests) {
    return ieache_serve_devices(socket_path, cloud_key_path, nbit_key_path, &device, 1, max_requests);
}

int ieache_debug_mix_plan(int cus, int n, int64_t gates, int s1, int ratio_x100, int out[9]) {
    if (!out) return fail(IEACHE_EINVAL, "null argument");
    MixGeometry g;
    MixSteps m;
    for (int i = 0; i < 9; i++) out[i] = 0;
    if (!mix_geometry_for(cus, gates, 0, 0, &g) || !mix_steps_for(n, g, s1, ratio_x100, &m)) return 0;  // no rotation at this size
    const int v[9] = {g.k, g.tw, m.s1, m.s2, m.cycles, m.tail_s1, m.tail_s2, m.covered, (int)mix_subset_size(gates, g.k)};
    for (int i = 0; i < 9; i++) out[i] = v[i];
    return 1;
}

int ieache_shard_slice(size_t total, size_t parts, size_t part, size_t* first, size_t* count) {
    if (!first || !count || parts == 0 || part >= parts) return fail(IEACHE_EINVAL, "bad shard arguments");
    shard_slice(total, parts, part, first, count);
    return 0;
}

int64_t ieache_serve_devices(const char* socket_path, const char* cloud_key_path, const char* nbit_key_path, const int* devices,
                             int n_devices, int64_t max_requests) {
    int64_t served = 0;
    const int rc = guarded([&] {
        if (!socket_path || !cloud_key_path || !devices) return fail(IEACHE_EINVAL, "null argument");
        DeviceGroup::validate_devices(devices, n_devices);  // the daemon's evaluators are a device group
        DaemonConfig cfg;
        cfg.socket_path = socket_path;
        cfg.cloud_key_path = cloud_key_path;
        if (nbit_key_path) cfg.nbit_key_path = nbit_key_path;
        cfg.device = devices[0];
        cfg.devices.assign(devices, devices + n_devices);
        cfg.max_requests = max_requests;
        if (const char* w = getenv("IEACHE_DAEMON_BATCH_WINDOW_MS")) cfg.batch_window_ms = atoi(w) > 0 ? atoi(w) : 0;
        if (const char* m = getenv("IEACHE_DAEMON_MAX_BATCH")) cfg.max_batch = atoi(m) > 0 ? atoi(m) : 1;
        if (const char* j = getenv("IEACHE_DAEMON_JOINT")) cfg.joint = atoi(j) != 0;
        served = daemon_serve(cfg);
        return 0;
    });
    return rc != 0 ? rc : served;
}

static int client_call(const char* socket_path, uint32_t op, const void* payload, size_t len, DaemonReply* reply) {
    return guarded([&] {
        if (!socket_path) return fail(IEACHE_EINVAL, "null socket path");
        *reply = daemon_request(socket_path, op, payload, len);
        if (reply->rc < 0) g_err = reply->log;  // the daemon's message for IEACHE_E*
        return (int)reply->rc;
    });
}

int ieache_client_ping(const char* socket_path) {
    DaemonReply r;
    return client_call(socket_path, DAEMON_PING, nullptr, 0, &r);
}

int ieache_client_run_dir(const char* socket_path, const char* workdir) {
    if (!workdir) return fail(IEACHE_EINVAL, "null workdir");
    DaemonReply r;
    const int rc = client_call(socket_path, DAEMON_RUN_DIR, workdir, strlen(workdir), &r);
    if (rc >= 0) fputs(r.log.c_str(), stdout);  // the chatter main() of cloud.c prints
    return rc;
}

int ieache_client_run_data(const char* socket_path, int operator_code, const void* cloud_data, size_t cloud_data_len,
                           void* answer, size_t answer_cap, size_t* answer_len) {
    if (!cloud_data && cloud_data_len) return fail(IEACHE_EINVAL, "null cloud.data");
    DaemonReply r;
    std::vector<unsigned char> payload;
    const int prc = guarded([&] {
        payload.resize(4 + cloud_data_len);
        const int32_t op = operator_code;
        memcpy(payload.data(), &op, 4);
        if (cloud_data_len) memcpy(payload.data() + 4, cloud_data, cloud_data_len);
        return 0;
    });
    if (prc != 0) return prc;
    const int rc = client_call(socket_path, DAEMON_RUN_DATA, payload.data(), payload.size(), &r);
    if (rc < 0) return rc;
    if (answer_len) *answer_len = r.data.size();
    if (r.data.size() > answer_cap || (!answer && !r.data.empty())) return fail(IEACHE_EINVAL, "answer buffer too small");
    if (!r.data.empty()) memcpy(answer, r.data.data(), r.data.size());
    return rc;
}

int ieache_client_shutdown(const char* socket_path) {
    DaemonReply r;
    return client_call(socket_path, DAEMON_SHUTDOWN, nullptr, 0, &r);
}

}  // extern "C"
