/*
 * ieache.h -- C ABI of the MI355X-native evaluator for the IE-ACHE Cloud path.
 *
 * Drop-in boundary for the hot path of kennethsoh/IE-ACHE: the homomorphic ALU
 * in Cloud/cloud.c and the libtfhe gate bootstrapping beneath it.  Plain C
 * types only, caller-allocated buffers, no exceptions cross this boundary:
 * every function returns 0 on success or a negative IEACHE_E* code (the
 * process-contract function returns the reference's exit codes 0 / 126), and
 * ieache_last_error() holds the message.  A context is not thread-safe; use one
 * per process per GPU, or a device group (section 2b) for several GPUs behind one handle.
 *
 * Streams: a context launches on its own non-blocking HIP stream
 * (ieache_ctx_stream).  Every entry point that takes DEVICE pointers
 * (ieache_ctx_create_device, ieache_eval_batch_device, ieache_gates_device,
 * ieache_gates3_device, ieache_pbs_device, ieache_pbs_multi_device, ieache_keyswitch_device, ieache_mux_device) reads them on that stream
 * without ordering against the
 * stream that produced them: the caller must either have synchronised the
 * producing stream (torch.cuda.synchronize(), hipStreamSynchronize) or call
 * ieache_ctx_wait_stream(ctx, producer) first.  Outputs are complete when the
 * call returns (each call synchronises the context's stream before returning).
 * Device-pointer arguments are checked with hipPointerGetAttributes: a host or
 * stray address is refused with IEACHE_EINVAL instead of reaching a kernel.
 *
 * Sample layout: one LWE sample = int32[n+1] = a[0..n-1], b (Torus32).  Host
 * buffers are packed rows of n+1; DEVICE buffers are rows of
 * ieache_lwe_stride() int32 (n+1 rounded up to a multiple of 4).
 *
 * Each entry point names the reference interface it replaces.
 */
#ifndef IEACHE_H
#define IEACHE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IEACHE_EINVAL (-22)   /* bad argument / unsupported parameter set */
#define IEACHE_EIO (-5)       /* file missing, short or malformed */
#define IEACHE_ENODEV (-19)   /* no usable GPU / HIP failure */
#define IEACHE_ENOMEM (-12)

/* TFHE parameter set; replaces TFheGateBootstrappingParameterSet as read from
 * the key header (Cloud/cloud.c:666-669, Keygen/keygen.c:22-23). */
typedef struct ieache_params {
    int32_t n, N, k, l, Bgbit, ks_t, ks_basebit;
    double lwe_alpha_min, lwe_alpha_max, tlwe_alpha_min, tlwe_alpha_max;
} ieache_params;

/* libtfhe >= 1.1 new_default_gate_bootstrapping_parameters(110) (keygen.c:22-23):
 * n=630 N=1024 k=1 l=3 Bgbit=7 ks_t=8 ks_basebit=2, sigma 2^-15 / 2^-25.
 *
 * Accepted sets (anything else is IEACHE_EINVAL when a key header is read, a key generated or a context created): k = 1; N a
 * power of two in 16 .. 2048; n >= 1; l Bgbit <= 32 with 2 l N 2^Bgbit <= 2^32; ks_t ks_basebit < 32 with ks_basebit <= 4.
 * N = 2048: gates, gates3, mux, eval_batch, netlists, programs, pbs / pbs_multi with every flag,
 * keyswitch, tlwe_extract, lut_test_poly / lut_factor_poly and the group forms work as at N = 1024, on a two-limb kernel that is
 * exact for any words: there is no one-limb form, no rounding guard and no audit, so ieache_ctx_fft_audit reports zero audited
 * launches.  Refused on such a context, each with its message: ieache_tgsw_prepare* and with them every call on a TGSW set
 * (N = 1024 only), the packing and the projection key and with them pack, tlwe_project, unpack and lut_write_coef, a gadget of
 * more than 16 rows (l > 8), and ks_t >= 19 (the key switch's digit list of N ks_t words exceeds a CU's LDS); the "force_generic"
 * option on a set with l >= 5 makes a call fail with the LDS message instead of running. */
void ieache_default_params(ieache_params* out);

typedef struct ieache_stats {
    double total_ms;          /* GPU timeline of the call (HIP events on the evaluator's stream) */
    double blind_rotate_ms;   /* sum over blind-rotation launches */
    double keyswitch_ms;      /* sum over key-switch launches */
    int64_t blind_rotate_launches; /* blind-rotation kernel launches (one per slice of CMux steps per chunk) */
    int64_t keyswitch_launches;
    int64_t bootstraps;       /* bootsAND/bootsXOR-equivalent gate instances evaluated */
    int64_t levels;
    int64_t chunks;           /* (level, chunk) work units */
} ieache_stats;

/* circuit kinds = the branches of main() in Cloud/cloud.c */
#define IEACHE_CIRC_ADD 1     /* A+B                cloud.c:870-1190  */
#define IEACHE_CIRC_SUB 2     /* A+(~B+1)           cloud.c:1196-1807 */
#define IEACHE_CIRC_RSUB 3    /* B+(~A+1)           cloud.c:1809-2365 */
#define IEACHE_CIRC_MUL 4     /* A*B, double width  cloud.c:2366-2718 */
#define IEACHE_CIRC_ADD_KS 6   /* Kogge-Stone variants of ADD/SUB/RSUB: same decrypted */
#define IEACHE_CIRC_SUB_KS 7   /* result, depth 2*log2(bits)+2 instead of 3*bits, not the same       */
#define IEACHE_CIRC_RSUB_KS 8  /* ciphertext bits as the reference's ripple adders                   */
#define IEACHE_CIRC_MUL_WALLACE 9 /* A*B by carry-save (Wallace) reduction + one Kogge-Stone add: same decrypted
                                     product as MUL, ~8x fewer levels (32 instead of 255 at 32 bits) and fewer
                                     bootstraps; not the reference's ciphertext; IEACHE_MULTIPLIER=wallace selects
                                     it for the process contract */
/* The same four operators on the two-bootstrap full adder, sum = XOR3(x,y,c), carry = MAJ3(x,y,c) (opt-in: same inputs,
 * outputs and decrypted result, not the reference's gate sequence; IEACHE_ADDER=full-adder / IEACHE_MULTIPLIER=full-adder
 * select them for the process contract).  ADD_FA: 2 bootstraps per bit instead of 5, one level per bit instead of 3; its
 * carry-in is bit 0 of the carry word, as the reference's.  SUB_FA / RSUB_FA add the complement with a constant-true carry-in
 * and so need a carry word that encrypts 0 (alice.c:147-149), like the _KS kinds.  MUL_FA (32/64/128 bits): bits*bits ANDs, a
 * carry-save array of full adders, one full-adder ripple: 3*bits*bits - 2*bits bootstraps, 2*bits - 1 levels. */
#define IEACHE_CIRC_ADD_FA 16
#define IEACHE_CIRC_SUB_FA 17
#define IEACHE_CIRC_RSUB_FA 18
#define IEACHE_CIRC_MUL_FA 19
#define IEACHE_CIRC_MULADD 5  /* (A*B)+C, the compute_final() chaining of
                                 Cloud/dragonfly_cipher_cloud.py:1300-1327 fused; 32-, 64- or 128-bit A,B
                                 (= IEACHE_CIRC_CHAIN(MUL, ADD, 1)) */
/* Any two operators chained as compute() + compute_final() do
 * (dragonfly_cipher_cloud.py:1219-1327), fused into one DAG without the answer.data
 * round trip: stage 1 = k1(A, B); stage 2 = k2(answer, C) when flip (cloud.data =
 * answer | C, :1306-1314) or k2(C, answer) otherwise (:1318-1326).  k1, k2 in
 * {ADD, SUB, RSUB, MUL}.  Inputs per expression: A bits, B bits, A's 32-sample carry
 * word, C at stage 2's width (bits, or 2*bits after a MUL) [, C's carry word when
 * !flip].  E.g. the paper's A+B-C = IEACHE_CIRC_CHAIN(ADD, SUB, 1), A*B*C =
 * IEACHE_CIRC_CHAIN(MUL, MUL, 1) (AC058.pdf Fig. 7). */
#define IEACHE_CIRC_CHAIN(k1, k2, flip) (32 + ((k1)-1) + 4 * ((k2)-1) + ((flip) ? 0 : 16))

/* gate types = libtfhe boot-gates.cpp entry points used by cloud.c:30-43,159 */
#define IEACHE_GATE_AND 0
#define IEACHE_GATE_XOR 1
#define IEACHE_GATE_OR 2
#define IEACHE_GATE_NAND 3
/* three-input gate, own entry points (ieache_mux*): bootsMUX(a,b,c) = a ? b : c.
 * Not called by Cloud/cloud.c; BASELINE.json's north_star names it. */
#define IEACHE_GATE_MUX 4
/* the other two-input gates of libtfhe's boot-gates.cpp, with its linear combinations word for word:
 * bootsNOR (0,-1/8)-ca-cb, bootsXNOR (0,-1/4)-2(ca+cb), bootsANDNY (0,-1/8)-ca+cb, bootsANDYN (0,-1/8)+ca-cb,
 * bootsORNY (0,1/8)-ca+cb, bootsORYN (0,1/8)+ca-cb.  Accepted by ieache_gates* and as netlist gates (section 3b). */
#define IEACHE_GATE_NOR 5
#define IEACHE_GATE_XNOR 6
#define IEACHE_GATE_ANDNY 7
#define IEACHE_GATE_ANDYN 8
#define IEACHE_GATE_ORNY 9
#define IEACHE_GATE_ORYN 10
#define IEACHE_GATE_TYPES 11
/* Three-input gates of ONE bootstrap each (not libtfhe's): a gate bootstrap takes the sign of a linear combination of its
 * inputs, and with the +-1/8 encoding MAJ3(a,b,c) = bootstrap(ca + cb + cc) (phases +-1/8, +-3/8) and XOR3(a,b,c) =
 * bootstrap((0,1/2) + 2(ca + cb + cc)) (phases +-1/4).  Noise budget: DESIGN.md section 7.  Own entry points
 * (ieache_gates3*), netlist gates, and the gates of the IEACHE_CIRC_*_FA kinds.  Their codes lie outside
 * 0 .. IEACHE_GATE_TYPES-1: arrays sized by IEACHE_GATE_TYPES do not count them (ieache_netlist_gate_count does). */
#define IEACHE_GATE_MAJ3 32
#define IEACHE_GATE_XOR3 33

typedef struct ieache_circuit_info {
    int32_t n_inputs;    /* samples per expression: A bits, B bits, 32-sample carry word [, C bits] */
    int32_t n_outputs;   /* samples per expression, LSB first */
    int32_t n_slots;     /* wire-store rows per expression on the device */
    int32_t depth;       /* ASAP levels */
    int32_t max_width;   /* widest ASAP level */
    int64_t bootstraps, n_and, n_xor;
    int32_t sched_max_width; /* widest level of the slack-balanced schedule the executor runs */
    int32_t folded;          /* 1 when this is the constant-folded variant (see "fold_constants") */
    int64_t reference_bootstraps; /* gates Cloud/cloud.c performs for this circuit; == bootstraps unless folded */
    int32_t sched_levels;    /* levels the executor runs (== depth unless a level cap stretched the schedule) */
    int32_t level_cap;       /* the cap this schedule was built with (0 = mean ASAP width) */
} ieache_circuit_info;
/* the struct of header version 0.1 ended with `folded`: ieache_circuit_info_get() -- the entry point that existed then --
 * writes these bytes and no more, so a caller built against that header is not written past its struct; the later
 * fields come from ieache_circuit_info_get_ex / _get_cap */
#define IEACHE_CIRCUIT_INFO_V01_BYTES 56

const char* ieache_version(void);
const char* ieache_last_error(void);
/* Key files are libtfhe's tfhe_io.cpp serialisations; libtfhe is not in the reference tree, so the
 * reader locates text sections by title and picks the binary layout among enumerated hypotheses
 * by the exact byte count (csrc/codec.h).  This names the hypothesis the calling thread's last
 * key load matched. */
const char* ieache_last_key_layout(void);
int ieache_device_count(void);

/* ------------------------------------------------------------------ *
 * 1. Process contract.  Replaces subprocess.call("./cloud")           *
 *    (Cloud/dragonfly_cipher_cloud.py:1233,1248,1263,1278) = main()   *
 *    of Cloud/cloud.c:650-2720.  Reads cloud.key, nbit.key,           *
 *    cloud.data, operator.txt in `workdir`; writes answer.data        *
 *    (352 samples, or exactly 64 = failure marker checked at          *
 *    dragonfly_cipher_cloud.py:1295); appends averagestandard.txt on  *
 *    MUL.  Returns 0 or 126 like the reference, or IEACHE_E*.         *
 * ------------------------------------------------------------------ */
int ieache_cloud_run(const char* workdir);

/* ------------------------------------------------------------------ *
 * 2. Context: cloud key resident on one GPU.  Replaces                *
 *    new_tfheGateBootstrappingCloudKeySet_fromFile (cloud.c:656-658), *
 *    without the per-call reload.                                     *
 * ------------------------------------------------------------------ */
typedef struct ieache_ctx ieache_ctx;

/* from a cloud.key file.  The second argument is a device INDEX: one GPU per context -- not the `ngpus` of SURVEY.md 8(b)'s
 * ieache_ctx_create(cloud_key_path, int ngpus).  A device COUNT lives in a device group (section 2b). */
ieache_ctx* ieache_ctx_create(const char* cloud_key_path, int device);
/* from raw arrays on the host: bk [n][(k+1)l][k+1][N], ksk [kN][t][base][n+1] */
ieache_ctx* ieache_ctx_create_raw(const ieache_params* p, const int32_t* bk, const int32_t* ksk, int device);
/* from raw arrays already in this GPU's memory (e.g. an RCCL broadcast buffer) */
ieache_ctx* ieache_ctx_create_device(const ieache_params* p, const int32_t* d_bk, const int32_t* d_ksk, int device);
void ieache_ctx_destroy(ieache_ctx* ctx);
int ieache_ctx_params(const ieache_ctx* ctx, ieache_params* out);
int ieache_lwe_stride(const ieache_ctx* ctx);
/* the HIP stream the evaluator launches on (hipStream_t as void*) */
void* ieache_ctx_stream(const ieache_ctx* ctx);
/* make the context's stream wait for the work queued so far on `hip_stream`
 * (hipStream_t as void*; NULL = the default stream) -- see "Streams" above */
int ieache_ctx_wait_stream(ieache_ctx* ctx, void* hip_stream);
/* The wide-launch blind rotation multiplies with ONE FP64 transform of the 32-bit key coefficients, as libtfhe does
 * (lwe-bootstrapping-functions-fft.cpp -> tGswFFTExternMulToTLwe), instead of the provably exact two-limb transform:
 * its rounded sums carry ~2^-9 of error, and the kernel records how far from an integer they came.
 * max_deviation: the largest distance seen by this context (0.5 would flip a bit; a launch above 1/16 makes the call
 * repeat itself on the two-limb kernel, counted in reruns).  Option "exact_fft" = 1 (or IEACHE_EXACT_FFT=1) uses the
 * two-limb kernel always.  Either pointer may be NULL. */
int ieache_ctx_fft_guard(const ieache_ctx* ctx, double* max_deviation, int64_t* reruns);
/* The guard watches the error LEVEL of every launch; the audit compares BITS of a sample: every K-th launch that took the
 * one-FFT kernel (option "fft_audit" = K, default 64, 0 = off; IEACHE_FFT_AUDIT=K) has 64 of its gate instances run again on
 * the two-limb kernel, and the extracted samples are compared word for word on the device.  A differing row makes the call
 * repeat itself on the two-limb kernels (counted in `reruns` above).  audits: audits run by this context; gates_compared:
 * gate instances they covered; mismatches: rows that differed (0 in every run so far).  Any pointer may be NULL.
 * A call whose output buffer overlaps an input cannot be repeated, so it runs on the two-limb kernels from the start. */
int ieache_ctx_fft_audit(const ieache_ctx* ctx, int64_t* audits, int64_t* gates_compared, int64_t* mismatches);
/* same contract as ieache_cloud_run but with this context's resident key */
int ieache_ctx_cloud_run(ieache_ctx* ctx, const char* workdir);
/* tuning / test knobs */
int ieache_ctx_set_chunk(ieache_ctx* ctx, int64_t gate_instances_per_launch);
int ieache_ctx_force_generic(ieache_ctx* ctx, int on);
/* Named knobs.  The evaluator's are the rows of ONE table, csrc/evaluator_options.h: name, environment variable (read once,
 * when the context is created), accepted range, default, and a line on what the option does.  A value a row refuses --
 * through this call or in the environment -- changes nothing; here it returns IEACHE_EINVAL.  Two more belong to this layer:
 * "level_quantum" (0/1, default 1: the slack-balanced circuits -- 64/128-bit multipliers -- get a level
 * width that makes level x batch a whole number of resident-workgroup rounds; same DAG and output bits, more
 * levels of exactly-full launches when the batch is small), and
 * "fold_constants" (0/1, default 0, also IEACHE_FOLD=1 for the process contract): build circuits
 * with constant operands folded and repeated gates shared.  cloud.c bootstraps every gate, even
 * `x AND 0` on the zero rows of its shift-add multipliers (SURVEY App. C note); the folded circuit
 * decrypts to the same bits with fewer bootstraps but is NOT the reference's ciphertext. */
int ieache_ctx_set_option(ieache_ctx* ctx, const char* name, int64_t value);
/* "overlap" (0/1, default 1; IEACHE_OVERLAP): the context issues its launches on two streams.  A circuit over a batch whose
 * mean level holds at least "pipe_min" gate instances (default 8 per CU) runs as two pipelines, each taking half of the
 * EXPRESSIONS through every level with no join in between; otherwise a level of at least "overlap_min" gate instances
 * (default 16 per CU) is issued as two halves with a join before the next level.  Same output bits either way; 0 = one
 * stream, the mode per-kernel timings are taken in (csrc/evaluator.h).  "pipe_auto" (0/1, default 1): between pipe_min / 8
 * and 2 x pipe_min the mode is chosen per (circuit, batch) by timing its first four evaluations, two in each mode.
 * "br_mix" (0/1, default 1; IEACHE_BR_MIX): launches of 4 .. 7 and of 8 .. 10.5 gates per CU run as a rotation of roles
 * between the two-waves- and the one-wave-per-gate kernel on three streams ("mix_s1", "mix_ratio", "mix_wg": turn length,
 * step ratio x 100, gates per workgroup).  "wg_gates" (0 = by launch size, 1 .. 4): gate instances per workgroup of the
 * one-wave-per-gate kernels.
 * ieache_ctx_get_option: the current value of any row of that table -- every option that can be set, and the read-only
 * figures ("cus", "resident_gates", "overlapped_levels", "pipelined_evals", "tuned_evals", "mixed_launches",
 * "staging_allocations") -- and of "level_quantum" / "fold_constants". */
int ieache_ctx_get_option(const ieache_ctx* ctx, const char* name, int64_t* value);
const char* ieache_ctx_kernel_variant(const ieache_ctx* ctx);
/* Name of the blind-rotation kernel a launch of `gates` gate instances takes under the context's
 * current options (launch sizes select different kernels: docs in csrc/br_plan.h).  Like
 * ieache_ctx_kernel_variant the string lives in the context until the next such call. */
const char* ieache_ctx_kernel_for_launch(const ieache_ctx* ctx, int64_t gates);

/* ------------------------------------------------------------------ *
 * 2b. Device group: the cloud key resident on SEVERAL GPUs of the     *
 *    node behind one handle, and every host-buffer call of sections   *
 *    3 and 3b on all of them at once.  What SURVEY.md 8(b) specified  *
 *    as ieache_ctx_create(cloud_key_path, ngpus) + ieache_eval_batch: *
 *    one handle, N GPUs, one call -- for a caller at                  *
 *    dragonfly_cipher_cloud.py:1233 that holds a batch and wants the  *
 *    whole node without a torchrun job or the socket daemon.          *
 * ------------------------------------------------------------------ */
/* A group owns one member per entry of its device list.  A member IS an ieache_ctx (own evaluator, streams, scratch, key
 * copy, circuit cache and options).  A call is `count` independent rows or expressions: member m evaluates the contiguous
 * slice ieache_shard_slice(count, members, m) gives it, on a host thread of its own (member 0 on the caller's), through the
 * context form of the same call.  Nothing crosses GPUs, and outputs equal the context form's word for word: every row goes
 * through the same circuit and kernels wherever it runs.
 * One call at a time: a group, like a context, is NOT thread-safe.  Its member contexts (ieache_group_ctx) may be used
 * directly between group calls, never during one.  No thread outlives a call.
 * Members that share a card: a device may be listed more than once (two or three contexts on one GPU, as cloudd --devices 0,0).
 * A member whose device index occurs more than once in the list is created with option "br_mix" = 0: the rotation of roles
 * assumes that its context has the chip to itself, and each of two contexts on a card would open three streams for it.
 * Output bits do not depend on the option; ieache_group_set_option(g, "br_mix", 1) overrides the rule.
 * Rates: profiles/group_rates.txt (scripts/group_rates.py) is the only record; several distinct devices are unmeasured. */
typedef struct ieache_group ieache_group;
#define IEACHE_GROUP_MAX_DEVICES 16
/* Replaces N calls of new_tfheGateBootstrappingCloudKeySet_fromFile (cloud.c:656-658), one per ./cloud process per GPU: the key
 * file is read and parsed ONCE, then uploaded to every listed device.  -> NULL with ieache_last_error() naming the argument
 * for n_devices outside 1 .. IEACHE_GROUP_MAX_DEVICES, a NULL device list, a negative index or an unsupported parameter set
 * -- all judged before the first HIP call, so a machine without a GPU refuses them the same way -- and naming member and
 * device when a member cannot be made (the members already made are destroyed). */
ieache_group* ieache_group_create(const char* cloud_key_path, const int* devices, int n_devices);
/* from raw arrays on the host, as ieache_ctx_create_raw */
ieache_group* ieache_group_create_raw(const ieache_params* p, const int32_t* bk, const int32_t* ksk, const int* devices, int n_devices);
void ieache_group_destroy(ieache_group* g);
int ieache_group_size(const ieache_group* g);                 /* members */
int ieache_group_device(const ieache_group* g, int member);   /* the device index of one */
/* the member as a context, for everything section 2 offers per context (options read back, statistics, kernel names).
 * Borrowed: it dies with the group and must not be given to ieache_ctx_destroy. */
ieache_ctx* ieache_group_ctx(ieache_group* g, int member);
/* ieache_ctx_set_option on every member, all or none: member 0's table row judges the value first, and a refusal -- there or,
 * for an option whose hook asks the device, at a later member, after which the earlier members get their old value back --
 * returns IEACHE_EINVAL with no member changed.  One name belongs to this layer, a test hook: "precheck" (0/1, default 1);
 * 0 = the evaluating forms below leave value checks to each member's own call, on its thread. */
int ieache_group_set_option(ieache_group* g, const char* name, int64_t value);
/* The group forms of the host-buffer entry points of sections 3 and 3b: the context form's arguments behind the group, same
 * buffer shapes, same error conventions.  (The *_device forms have no group form: device buffers would need cross-device
 * stream ordering and peer copies.)
 * Slicing: per-row arrays (operands, outputs, poly_of) are cut with the rows; shared tables (test polynomials, factors, bias,
 * a compiled netlist) go to every member whole; ieache_group_pbs_multi's output slice starts at row first x n_factors; rows
 * are N + 1 words under IEACHE_PBS_NO_KEYSWITCH.  ieache_group_prepare_* prepares each member for its slice size.
 * stats: NULL, or an array of ieache_group_size() records: stats[m] is member m's own, all zero when its slice was empty.
 * count == 0: member 0 alone makes the call and its return value is the group's.
 * Errors: arguments are checked once, before any thread starts, by the checks of the context forms.  If members fail, the
 * return code is that of the lowest-numbered one and ieache_last_error() -- on the CALLING thread -- carries its message
 * behind "member M (device D): ".  The output buffer's contents are then unspecified; the group stays usable.
 * A NULL group: IEACHE_EINVAL. */
/* replaces ieache_prepare_batch per GPU */
int ieache_group_prepare_batch(ieache_group* g, int kind, int bits, size_t batch);
/* replaces ieache_eval_batch per GPU = the add()/mul32()/... call trees of cloud.c:18-647 over a batch, on the whole node */
int ieache_group_eval_batch(ieache_group* g, int kind, int bits, size_t batch, const int32_t* in_lwe, int32_t* out_lwe,
                            ieache_stats* stats /* [n members] or NULL */);
/* replace ieache_prepare_netlist / ieache_eval_netlist per GPU (section 3b; the netlist is declared there).  ONE compiled
 * netlist is read by all members at once: it is immutable after ieache_netlist_create. */
struct ieache_netlist;
int ieache_group_prepare_netlist(ieache_group* g, const struct ieache_netlist* nl, size_t batch);
int ieache_group_eval_netlist(ieache_group* g, const struct ieache_netlist* nl, size_t batch, const int32_t* in_lwe, int32_t* out_lwe,
                              ieache_stats* stats /* [n members] or NULL */);
/* replaces ieache_gates per GPU = bootsAND / bootsXOR / ... (cloud.c:30-43,159) over `count` gates */
int ieache_group_gates(ieache_group* g, int gate_type, size_t count, const int32_t* a, const int32_t* b, int32_t* out,
                       ieache_stats* stats /* [n members] or NULL */);
/* replaces ieache_gates3 per GPU (MAJ3 / XOR3; no libtfhe counterpart) */
int ieache_group_gates3(ieache_group* g, int gate_type, size_t count, const int32_t* a, const int32_t* b, const int32_t* c, int32_t* out,
                        ieache_stats* stats /* [n members] or NULL */);
/* replaces ieache_mux per GPU = bootsMUX */
int ieache_group_mux(ieache_group* g, size_t count, const int32_t* a, const int32_t* b, const int32_t* c, int32_t* out,
                     ieache_stats* stats /* [n members] or NULL */);
/* replaces ieache_pbs per GPU = tfhe_blindRotateAndExtract_FFT / tfhe_bootstrap_woKS_FFT / tfhe_bootstrap_FFT over `count` rows */
int ieache_group_pbs(ieache_group* g, size_t count, const int32_t* x, const int32_t* test_polys, int32_t n_polys, const int32_t* poly_of,
                     int32_t* out, int flags, ieache_stats* stats /* [n members] or NULL */);
/* replaces ieache_pbs_multi per GPU (the multi-value bootstrap; no libtfhe counterpart) */
int ieache_group_pbs_multi(ieache_group* g, size_t count, const int32_t* x, const int32_t* test_polys, int32_t n_polys,
                           const int32_t* poly_of, const int32_t* factors, int32_t n_factors, const int32_t* bias, int32_t* out, int flags,
                           ieache_stats* stats /* [n members] or NULL */);

/* ------------------------------------------------------------------ *
 * 3. Batch evaluation: `batch` independent expressions through one    *
 *    circuit, level by level.  Replaces the add()/mul32()/mul64()/    *
 *    mul128()/split() call trees of cloud.c:18-647 and their use in   *
 *    main().  bits: 16 (generalised add(...,16,...)), 32, 64, 128,    *
 *    256 for ADD/SUB/RSUB; 32/64/128 for MUL and MULADD; chains: see  *
 *    IEACHE_CIRC_CHAIN.                                               *
 * ------------------------------------------------------------------ */
int ieache_circuit_info_get(int kind, int bits, ieache_circuit_info* out);
int ieache_circuit_info_get_ex(int kind, int bits, int fold_constants, ieache_circuit_info* out);
/* the schedule a context would pick for `batch` expressions on a GPU holding `resident_workgroups` blind rotations
 * at once (4 per CU; "level_quantum"): level_cap = 0 reproduces ieache_circuit_info_get_ex */
int ieache_circuit_level_cap(int kind, int bits, int fold_constants, int64_t batch, int resident_workgroups);
/* ... the same for the GPU and the kernels THIS context runs (one-wave and two-wave residency of its device, its
 * fold_constants setting): the level width ieache_eval_batch* will use for `batch` expressions; 0 = the default schedule */
int ieache_ctx_circuit_level_cap(const ieache_ctx* ctx, int kind, int bits, int64_t batch);
int ieache_circuit_info_get_cap(int kind, int bits, int fold_constants, int level_cap, ieache_circuit_info* out);
int ieache_circuit_simulate_cap(int kind, int bits, int fold_constants, int level_cap, const uint8_t* in_bits, uint8_t* out_bits);
/* gates of one IEACHE_GATE_* type (MAJ3 / XOR3 included) in a built-in circuit, counted as ieache_netlist_info counts them;
 * IEACHE_EINVAL for a code that names no gate type */
int64_t ieache_circuit_gate_count(int kind, int bits, int fold_constants, int gate_type);
/* host buffers: in [batch][n_inputs][n+1], out [batch][n_outputs][n+1] */
int ieache_eval_batch(ieache_ctx* ctx, int kind, int bits, size_t batch, const int32_t* in_lwe, int32_t* out_lwe,
                      ieache_stats* stats);
/* device buffers: rows of ieache_lwe_stride() int32 */
int ieache_eval_batch_device(ieache_ctx* ctx, int kind, int bits, size_t batch, const int32_t* d_in, int32_t* d_out,
                             ieache_stats* stats);
/* Builds (and caches) the circuit and allocates everything ieache_eval_batch*(ctx, kind, bits, batch, ...) needs on the
 * device -- wire store, gate tables, scratch of the widest level -- so that the evaluation itself allocates nothing.
 * Optional: the evaluation does the same on first use (the reference has no counterpart: ./cloud allocates per run,
 * cloud.c:651-700). */
int ieache_prepare_batch(ieache_ctx* ctx, int kind, int bits, size_t batch);
/* `count` independent gates: out[i] = gate(a[i], b[i]); replaces bootsAND /
 * bootsXOR / bootsOR / bootsNAND (cloud.c:30-43,159) and, with gate types 5 .. 10, bootsNOR / bootsXNOR /
 * bootsANDNY / bootsANDYN / bootsORNY / bootsORYN.  Device rows. */
int ieache_gates_device(ieache_ctx* ctx, int gate_type, size_t count, const int32_t* d_a, const int32_t* d_b,
                        int32_t* d_out, ieache_stats* stats);
/* host rows of n+1 */
int ieache_gates(ieache_ctx* ctx, int gate_type, size_t count, const int32_t* a, const int32_t* b, int32_t* out,
                 ieache_stats* stats);
/* out[i] = gate(a[i], b[i], c[i]) for gate_type IEACHE_GATE_MAJ3 or IEACHE_GATE_XOR3 (any other type: IEACHE_EINVAL): one
 * blind rotation and one key switch per gate, like a two-input gate.  No libtfhe counterpart; a full adder is these two. */
int ieache_gates3_device(ieache_ctx* ctx, int gate_type, size_t count, const int32_t* d_a, const int32_t* d_b, const int32_t* d_c,
                         int32_t* d_out, ieache_stats* stats);
int ieache_gates3(ieache_ctx* ctx, int gate_type, size_t count, const int32_t* a, const int32_t* b, const int32_t* c, int32_t* out,
                  ieache_stats* stats);
/* Programmable (functional) bootstrap: one blind rotation from a CALLER'S test polynomial instead of the constant
 * (1/8, ..., 1/8) every gate starts from.  Replaces libtfhe's tfhe_blindRotateAndExtract_FFT(result, v, bk, barb, bara, ...)
 * (arbitrary test polynomial v), tfhe_bootstrap_woKS_FFT (IEACHE_PBS_NO_KEYSWITCH) and tfhe_bootstrap_FFT with an arbitrary
 * mu (the constant polynomial v = (mu, ..., mu)); like MAJ3 / XOR3 none of it is called by Cloud/cloud.c, which only reaches
 * bootsAND / bootsXOR.
 * Convention: row x[i] is bootstrapped as it stands (no gate combination).  With its mod-switched phase
 * phi = barb - sum_j bara_j s_j (mod 2N) and v = test_polys[poly_of[i]] (row 0 when poly_of is NULL), out[i] encrypts
 *     v[phi]        when phi < N,
 *     -v[phi - N]   otherwise
 * -- libtfhe's testvectbis = X^(2N-barb) * v, the n CMux steps, extraction of coefficient 0 -- and is key-switched back to
 * the LWE key unless IEACHE_PBS_NO_KEYSWITCH is set.  ieache_lut_test_poly builds v from a table of values.
 * test_polys: [n_polys][N] Torus32, rows packed on the host and on the device alike.  poly_of: [count] row indices or NULL.
 * Host form: IEACHE_EINVAL for n_polys < 1, a NULL table, or an index outside [0, n_polys).  Device form: the indices are
 * not read on the host; the kernel clamps each into [0, n_polys), so a bad one gives a wrong answer, never a stray read.
 * IEACHE_PBS_NO_KEYSWITCH: the extracted samples (a'[0..N-1], b) under the ring key are the result and no key switch is
 * launched (stats->keyswitch_launches == 0); host rows of N+1, device rows of ieache_extract_stride() int32 (N+1 rounded
 * up to a multiple of 4), and d_out must not overlap d_x.  ieache_keyswitch* is its partner.  Otherwise rows as for
 * ieache_gates*, and d_out may be d_x (the call then runs on the two-limb kernels from the start).
 * One blind rotation and (unless skipped) one key switch per row; stats->bootstraps == count.  Noise budget of tables:
 * DESIGN.md section 7 (at libtfhe's gate parameters four entries is the recommended ceiling).
 *
 * IEACHE_PBS_TLWE_POLYS (ieache_pbs*, ieache_pbs_multi*, and their group forms): the table is ENCRYPTED.  test_polys is
 * [n_polys][2][N]: TLWE samples under the ring key, A then B, phase B - A s -- the samples key generation makes for the rows
 * of the bootstrapping key, and what ieache_tlwe_encrypt makes of a table (section 4).  The accumulator starts from
 * X^(2N-barb) * (A, B), both polynomials rotated by the same amount with the same negacyclic rule: libtfhe's
 * tfhe_blindRotate_FFT on a caller's accumulator.  Everything after that is the call without the flag: poly_of and its
 * clamping, IEACHE_PBS_NO_KEYSWITCH, the in-place rule, guard, audit and repeat; the overlap checks use the 2N-word rows.
 * Convention: with A = 0 the call is the plain call on B, bit for bit.  With an encryption of v the output encrypts what
 * the plain call on v encrypts, plus the table's own encryption noise, which a monomial rotation does not amplify
 * (DESIGN.md section 7).
 * IEACHE_PBS_ACCUMULATOR (ieache_pbs, ieache_pbs_device and ieache_group_pbs; IEACHE_EINVAL on ieache_pbs_multi*): output
 * row i is the WHOLE rotated accumulator [2][N], A then B -- 2N packed int32 on the host and on the device alike (2N is a
 * multiple of 4 for every supported N): libtfhe's tfhe_blindRotate_FFT applied to X^(2N-barb) * test_poly.  There is no
 * extraction and no key switch whether or not IEACHE_PBS_NO_KEYSWITCH is set (stats->keyswitch_launches == 0), and no
 * in-place form: an output overlapping rows, polynomials or indices is IEACHE_EINVAL.  It combines with
 * IEACHE_PBS_TLWE_POLYS.  ieache_tlwe_phase (section 4) decrypts such rows; the sample ieache_pbs extracts is
 * (A[0], -A[N-1], ..., -A[1]; B[0]).
 * The value 2 names no flag and is refused as every unknown bit is. */
#define IEACHE_PBS_NO_KEYSWITCH 1
#define IEACHE_PBS_TLWE_POLYS 4
#define IEACHE_PBS_ACCUMULATOR 8
int ieache_pbs_device(ieache_ctx* ctx, size_t count, const int32_t* d_x, const int32_t* d_test_polys, int32_t n_polys,
                      const int32_t* d_poly_of, int32_t* d_out, int flags, ieache_stats* stats);
int ieache_pbs(ieache_ctx* ctx, size_t count, const int32_t* x, const int32_t* test_polys, int32_t n_polys, const int32_t* poly_of,
               int32_t* out, int flags, ieache_stats* stats);
/* int32 per device row of extracted samples (ieache_pbs_device with IEACHE_PBS_NO_KEYSWITCH) */
int ieache_extract_stride(const ieache_ctx* ctx);
/* The key switch alone: libtfhe's lweKeySwitch over `count` extracted samples under the ring key -> rows under the LWE key.
 * Rows are shaped exactly as IEACHE_PBS_NO_KEYSWITCH shapes its outputs, so one call's output is the other's input -- after
 * whatever additions the caller makes in between (bootsMUX adds two extracted samples before ONE key switch): host rows
 * u [count][N+1] -> out [count][n+1]; device rows d_u [count][ieache_extract_stride()] -> d_out [count][lwe_stride].
 * The call is cut by "chunk" like every flat call; stats->bootstraps == 0, stats->keyswitch_launches >= 1 (one per piece),
 * stats->levels == 1.  count == 0 is a no-op.  IEACHE_EINVAL when the output overlaps the input.  The host form goes through
 * the context's staging rows: a warm call allocates nothing.  ieache_debug_keyswitch gives the same rows.  There is no
 * group form: a key switch is a small fraction of a bootstrap, and cutting it over devices is out of scope. */
int ieache_keyswitch_device(ieache_ctx* ctx, size_t count, const int32_t* d_u, int32_t* d_out, ieache_stats* stats);
int ieache_keyswitch(ieache_ctx* ctx, size_t count, const int32_t* u, int32_t* out, ieache_stats* stats);
/* Host only: the test polynomial of a lookup table f[0 .. entries-1] of Torus32 values for messages m encoded at phase
 * m / (2 entries) (padding bit clear: phases below 1/2): v[j] = f[((j + N/(2 entries)) * entries) div N] for
 * j < N - N/(2 entries), -f[0] on the last N/(2 entries) coefficients -- every slot centred on its message, and the negacyclic
 * wrap returning f[0] just below phase 0.  Only p->N is read.  IEACHE_EINVAL unless 2 x entries divides N. */
int ieache_lut_test_poly(const ieache_params* p, int32_t entries, const int32_t* f, int32_t* v /*[N]*/);
/* Multi-output programmable bootstrap: ONE blind rotation per row, several outputs (the multi-value bootstrap of Carpov,
 * Izabachene and Mollimard, CT-RSA 2019).  Each further output costs one exact integer polynomial product and one key
 * switch, not a rotation.  Ring: Torus32[X]/(X^N+1); everything below is mod 2^32 with wraparound.
 * Convention:
 *   1. Row x[i] is blind-rotated exactly as ieache_pbs does it -- test polynomial test_polys[poly_of[i]], the row as it
 *      stands, no gate combination -- and the WHOLE accumulator ACC_i = (A, B), two polynomials of N words, is kept.
 *   2. For every factor polynomial P_t = factors[t] (N int32, any values), t = 0 .. n_factors-1:
 *        A' = P_t A and B' = P_t B, negacyclic;
 *        coefficient 0 of (A', B') is extracted the way every bootstrap here extracts:
 *            u[0] = A'[0],  u[j] = -A'[N-j] (0 < j < N),  u[N] = B'[0] + bias[t]      (bias NULL: 0);
 *        u is key-switched back to the LWE key unless IEACHE_PBS_NO_KEYSWITCH is set.
 *   3. Output row i * n_factors + t (item-major), shaped as ieache_pbs shapes its rows: host rows of n+1 (N+1 without the
 *      key switch), device rows of lwe_stride (ieache_extract_stride(); all its words are written, the padding as zero).
 * P = 1 is ieache_pbs itself, bit for bit.  P = -X^(N-j) (that is X^(-j)) extracts coefficient j of the accumulator: the
 * multi-coefficient extraction of "PBS-many-LUT".
 * Tables -> factors: ieache_lut_factor_poly.  With v = ieache_lut_test_poly(entries, w) for a table w of small INTEGERS (not
 * torus values), P = v (1 - X): P[0] = v[0] + v[N-1], P[j] = v[j] - v[j-1]; it has at most entries + 1 nonzero
 * coefficients.  Because (1 + X + ... + X^(N-1)) (1 - X) = 2, rotating the CONSTANT polynomial c and multiplying by P gives
 * the message a rotation from 2c v gives: a message m comes out as 2c w[m] + bias.  With c = 1/8, w in {0, 1} and
 * bias = -1/8 the outputs are ordinary gate bits at +-1/8.
 * Noise: the rotation's share of the output variance is multiplied by |P|_2^2 (sum of squared coefficients); the key switch
 * adds its share once per output.  DESIGN.md section 7 has the budget.
 * Flags and argument rules are ieache_pbs's.  In addition IEACHE_EINVAL when n_factors is outside
 * 1 .. IEACHE_PBS_MULTI_MAX_FACTORS or the factor table is NULL, and when the output overlaps ANY input -- rows, test
 * polynomials, indices, factors or bias: there is no in-place form, the output is n_factors times the input.  The device
 * form reads neither the indices nor the factors on the host.
 * stats->bootstraps == count (rotations, not outputs); stats->keyswitch_launches == 0 with IEACHE_PBS_NO_KEYSWITCH. */
#define IEACHE_PBS_MULTI_MAX_FACTORS 64
int ieache_pbs_multi_device(ieache_ctx* ctx, size_t count, const int32_t* d_x, const int32_t* d_test_polys, int32_t n_polys,
                            const int32_t* d_poly_of, const int32_t* d_factors /*[n_factors][N]*/, int32_t n_factors,
                            const int32_t* d_bias /*[n_factors] or NULL*/, int32_t* d_out /*[count * n_factors] rows*/, int flags,
                            ieache_stats* stats);
int ieache_pbs_multi(ieache_ctx* ctx, size_t count, const int32_t* x, const int32_t* test_polys, int32_t n_polys, const int32_t* poly_of,
                     const int32_t* factors, int32_t n_factors, const int32_t* bias, int32_t* out, int flags, ieache_stats* stats);
/* Host only: the factor polynomial P = v (1 - X) of a table w[0 .. entries-1] of small integers, v laid out as
 * ieache_lut_test_poly lays it out.  Only p->N is read.  IEACHE_EINVAL unless 2 x entries divides N. */
int ieache_lut_factor_poly(const ieache_params* p, int32_t entries, const int32_t* w, int32_t* P /*[N]*/);
/* out[i] = a[i] ? b[i] : c[i]; replaces bootsMUX (libtfhe boot-gates.cpp): per gate two blind
 * rotations without key switch, their extracted samples added to (0, 1/8), one key switch.
 * stats->bootstraps counts the blind rotations (2 per gate). */
int ieache_mux_device(ieache_ctx* ctx, size_t count, const int32_t* d_a, const int32_t* d_b, const int32_t* d_c,
                      int32_t* d_out, ieache_stats* stats);
int ieache_mux(ieache_ctx* ctx, size_t count, const int32_t* a, const int32_t* b, const int32_t* c, int32_t* out,
               ieache_stats* stats);

/* ------------------------------------------------------------------ *
 * 3b. Your own circuit: a netlist of gates, evaluated like the        *
 *     built-in kinds -- levelised, slot-allocated, a whole level x    *
 *     batch per launch, on two streams.  Replaces a program that      *
 *     calls libtfhe's bootsAND / bootsXNOR / bootsMUX ... gate by     *
 *     gate, as Cloud/cloud.c:30-43 calls bootsAND / bootsXOR.         *
 * ------------------------------------------------------------------ */
/* Reference to a sample inside a netlist: wire w (inputs are wires 0 .. n_inputs-1, gate g's output is wire
 * n_inputs + g), optionally negated (bootsNOT: free), or a constant (bootsCONSTANT: free). */
#define IEACHE_NET_WIRE(w) ((int32_t)(w) << 1)
#define IEACHE_NET_NOT(ref) ((ref) ^ 1)
#define IEACHE_NET_FALSE (-2)
#define IEACHE_NET_TRUE (-1)
/* one gate: type is an IEACHE_GATE_* value; c is the third operand of IEACHE_GATE_MUX (a ? b : c), IEACHE_GATE_MAJ3 and
 * IEACHE_GATE_XOR3, and must be 0 otherwise.  MAJ3 / XOR3 must name three different wires (constants may repeat): the same
 * wire twice adds its noise coherently and eats the margin. */
typedef struct ieache_net_gate {
    int32_t type, a, b, c;
} ieache_net_gate;
#define IEACHE_NETLIST_BALANCED 1 /* slack-balanced schedule at the mean level width instead of ASAP levels */
typedef struct ieache_netlist ieache_netlist;
/* Validates and compiles a gate list (the place of the C source that calls libtfhe's bootsXXX one after the other).  A host
 * object: it belongs to no context and holds no device memory; several contexts may evaluate it, and it must outlive
 * every call that uses it.  A gate may only refer to inputs and to gates before it.  Every recorded gate is bootstrapped:
 * the context options "fold_constants" and "level_quantum" do not apply to netlists (fold what you want folded before
 * recording).  -> NULL with ieache_last_error() naming the offending gate: an operand or output that refers to a wire not
 * defined at that point, an unknown type, a third operand on a two-input gate, a MAJ3 / XOR3 that names a wire twice, no
 * inputs / no outputs, more than 2^30 wires. */
ieache_netlist* ieache_netlist_create(int32_t n_inputs, const ieache_net_gate* gates, size_t n_gates, const int32_t* outputs,
                                      size_t n_outputs, int flags);
void ieache_netlist_destroy(ieache_netlist* nl);
/* statistics of the compiled netlist, as ieache_circuit_info_get gives for a built-in kind.  bootstraps and the widths count
 * BLIND ROTATIONS -- a MUX gate is two, as in libtfhe's bootsMUX -- so that an evaluation reports batch x bootstraps;
 * n_and / n_xor count the AND / XOR gates the executor runs (NOR, ANDNY, ANDYN run as AND with negated operands).
 * gates_by_type (may be NULL): gates recorded, by the IEACHE_GATE_* type they were given as (a MUX counts 1 here). */
int ieache_netlist_info(const ieache_netlist* nl, ieache_circuit_info* out, int64_t gates_by_type[IEACHE_GATE_TYPES]);
/* gates recorded with one IEACHE_GATE_* type, for any valid type code -- IEACHE_GATE_MAJ3 / _XOR3 too, which gates_by_type
 * above has no room for; IEACHE_EINVAL for a code that names no gate type */
int64_t ieache_netlist_gate_count(const ieache_netlist* nl, int gate_type);
/* plaintext simulation (host only, no GPU): in_bits [n_inputs] -> out_bits [n_outputs], each 0/1 */
int ieache_netlist_simulate(const ieache_netlist* nl, const uint8_t* in_bits, uint8_t* out_bits);
/* the netlist counterparts of ieache_prepare_batch / ieache_eval_batch / ieache_eval_batch_device: same buffer shapes
 * (in [batch][n_inputs] rows, out [batch][n_outputs] rows; host rows of n+1, device rows of ieache_lwe_stride()), same
 * stream ordering, device-pointer checks and error conventions.  Replaces the gate-by-gate bootsXNOR / bootsMUX / ...
 * program of the netlist run once per expression. */
int ieache_prepare_netlist(ieache_ctx* ctx, const ieache_netlist* nl, size_t batch);
int ieache_eval_netlist(ieache_ctx* ctx, const ieache_netlist* nl, size_t batch, const int32_t* in_lwe, int32_t* out_lwe,
                        ieache_stats* stats);
int ieache_eval_netlist_device(ieache_ctx* ctx, const ieache_netlist* nl, size_t batch, const int32_t* d_in, int32_t* d_out,
                               ieache_stats* stats);

/* ------------------------------------------------------------------ *
 * 3c. Several circuits' batches in ONE call, evaluated together level *
 *    by level.  What a caller holds who has, in the same moment, a    *
 *    few additions, a few subtractions and a few multiplications      *
 *    (dragonfly_cipher_cloud.py:1233 runs one ./cloud per operator):  *
 *    evaluated one after another each is a run of narrow launches,    *
 *    and a level costs one rotation's latency however few gates it    *
 *    holds.  Their gates are independent, so they share every launch. *
 * ------------------------------------------------------------------ */
/* A job is what ieache_eval_batch or ieache_eval_netlist takes: a circuit, a batch, input and output rows of the shapes
 * those calls document.  Step s = 1, 2, ... of the call runs level s of every job that still has one as one launch
 * sequence over all their gates (one prologue and one key switch per job, one sequence of blind-rotation launches over all,
 * the kernel chosen by the joint size); a shallow job finishes early.  Every job's output words are what the same job gives
 * alone -- word for word, whatever it ran with.  Level mode only: no expression pipelines ("overlap" still splits wide joint
 * levels over two streams), so a job that is wide on its own gains nothing here; the call always joins, the decision is the
 * caller's (cloudd's rule: csrc/joint_plan.h).
 * Circuits are the context's base circuits of (kind, bits) under its "fold_constants"; "level_quantum" does not apply (a
 * level cap is chosen for one batch filling rounds alone).  A compiled netlist carries no parameter set and runs under
 * any context.
 * A job with batch 0 is skipped (its pointers are not read); n_jobs == 0 succeeds.  A NULL row pointer with a batch, or an
 * unknown kind / width, fails the WHOLE call with IEACHE_EINVAL before anything is launched or written;
 * ieache_last_error() starts with "job I: ", I the failing job's index.
 * stats: bootstraps summed over the jobs; levels = the deepest job's depth; chunks = launch sequences issued (one per joint
 * level unless "chunk" or level halves cut it); times as for any call.
 * The rounding guard and the audit act on the joint launches: a trip repeats the whole call on the two-limb kernels, and a
 * device-form call in which any job's output range shares a word with any job's input range runs on them from the start. */
typedef ieache_stats ieache_eval_stats;
typedef struct ieache_job {
    int kind, bits;                        /* a CIRC_* kind and its width, or */
    const struct ieache_netlist* netlist;  /* non-NULL: the netlist instead (kind, bits ignored) */
    size_t batch;
    const int32_t* in_lwe;                 /* as ieache_eval_batch / ieache_eval_netlist take them (device rows in the _device form) */
    int32_t* out_lwe;
} ieache_job;
/* allocates what the joint evaluation of these jobs needs (pointers are not read), so that a timed first call allocates nothing */
int ieache_prepare_jobs(ieache_ctx* ctx, const ieache_job* jobs, size_t n_jobs);
/* host rows, staged through the context's kept staging rows: a warm call allocates nothing */
int ieache_eval_jobs(ieache_ctx* ctx, const ieache_job* jobs, size_t n_jobs, ieache_eval_stats* stats);
/* device rows of ieache_lwe_stride() words; stream ordering and pointer checks as ieache_eval_batch_device */
int ieache_eval_jobs_device(ieache_ctx* ctx, const ieache_job* jobs, size_t n_jobs, ieache_eval_stats* stats);
/* The form for a device group (section 2b) is exported as well and declared in csrc/group.h, next to the group it cuts the
 * jobs over: every job's batch goes over the members by ieache_shard_slice's rule, and each member runs ieache_eval_jobs on
 * its slices. */

/* ------------------------------------------------------------------ *
 * 3d. Word programs: a multi-operator integer expression -- a*b + c*d, *
 *    (a+b)*c - d, the sum of eight words, max(a+b, c) -- compiled into *
 *    ONE circuit.  Issued as one call per operator (one ./cloud run    *
 *    each at dragonfly_cipher_cloud.py:1233), a*b and c*d run one      *
 *    after the other although their gates are independent, every call  *
 *    pays its own depth and the intermediates travel through the       *
 *    caller.  As one program their gates share levels.                 *
 * ------------------------------------------------------------------ */
/* A program is a list of instructions; the result of instruction i is REGISTER i, a word of 1 .. 512 samples, LSB first.
 * Operands a, b, c name earlier registers.  The expression's input samples are the INPUT registers in declaration order; its
 * output samples are the listed output registers in order.
 *   wiring only (no gate):
 *     INPUT   width                        CONST   width, value words const_words[first .. first+count), LSW first
 *     ZEXT    a to width (>= a's)          SLICE   samples imm0 .. imm0+imm1-1 of a
 *     SHL     a << imm0, same width        NOT     ~a                       CONCAT  a (low), b (high)
 *   one gate per bit:
 *     AND, OR, XOR  a, b of equal widths   ANDBIT  every bit of a ANDed with the 1-sample register b
 *   word operators ADD (a+b), SUB (a-b), RSUB (b-a), MUL (a*b, double width): the circuit kind of (operator, family) itself --
 *     family 0 the reference's (IEACHE_CIRC_ADD ...), IEACHE_FAMILY_KOGGE_STONE (_KS), _CARRY_SAVE (MUL_WALLACE), _FULL_ADDER
 *     (_FA) -- with its width rules (adders 1 .. 256, multipliers 32 / 64 / 128) and refusals (no Kogge-Stone multiplier).
 *     c = the 32-sample carry word of that kind, or -1 for 32 constant zeros.  A one-instruction program given the caller's carry
 *     word records the built-in kind's circuit gate for gate (MUL_WALLACE: under IEACHE_PROGRAM_FOLD, which that kind builds with).
 *   SUM     the sum mod 2^width of count >= 2 operands args[first .. first+count), each a register shifted left by `shift`, zero-
 *           extended or truncated to width: a carry-save reduction on XOR3 / MAJ3 compressors (one level per stage; stages: the
 *           least s with w_s >= count, w_0 = 2, w_{s+1} = floor(3 w_s / 2)) down to two rows, then ONE addition in `family`
 *           (IEACHE_FAMILY_FULL_ADDER or _KOGGE_STONE) -- not count - 1 additions.
 *   LT, EQ  a < b / a == b, unsigned, equal widths -> 1 sample.   SELECT  a (1 sample) ? b : c, one MUX per bit.
 * Every recorded gate is bootstrapped, as for netlists and the reference, unless IEACHE_PROGRAM_FOLD asks for the constant-
 * folded, gate-shared build ("fold_constants" of the built-in kinds); IEACHE_NETLIST_BALANCED keeps its meaning. */
#define IEACHE_WOP_INPUT 0
#define IEACHE_WOP_CONST 1
#define IEACHE_WOP_ZEXT 2
#define IEACHE_WOP_SLICE 3
#define IEACHE_WOP_SHL 4
#define IEACHE_WOP_NOT 5
#define IEACHE_WOP_CONCAT 6
#define IEACHE_WOP_AND 7
#define IEACHE_WOP_OR 8
#define IEACHE_WOP_XOR 9
#define IEACHE_WOP_ANDBIT 10
#define IEACHE_WOP_ADD 11
#define IEACHE_WOP_SUB 12
#define IEACHE_WOP_RSUB 13
#define IEACHE_WOP_MUL 14
#define IEACHE_WOP_SUM 15
#define IEACHE_WOP_LT 16
#define IEACHE_WOP_EQ 17
#define IEACHE_WOP_SELECT 18
#define IEACHE_FAMILY_REFERENCE 0
#define IEACHE_FAMILY_KOGGE_STONE 1
#define IEACHE_FAMILY_CARRY_SAVE 2
#define IEACHE_FAMILY_FULL_ADDER 3
#define IEACHE_PROGRAM_FOLD 2 /* flag, next to IEACHE_NETLIST_BALANCED */
#define IEACHE_WORD_MAX_WIDTH 512
typedef struct ieache_word_instr {
    int32_t op;            /* IEACHE_WOP_* */
    int32_t family;        /* IEACHE_FAMILY_* of ADD / SUB / RSUB / MUL / SUM, 0 otherwise */
    int32_t width;         /* INPUT, CONST, ZEXT: the result's width; SUM: the sum's width; 0 otherwise */
    int32_t a, b, c;       /* register operands; the ones an opcode does not take are ignored */
    int32_t imm0, imm1;    /* SLICE: first, count; SHL: the shift */
    int32_t first, count;  /* SUM: into args; CONST: into const_words */
} ieache_word_instr;
typedef struct ieache_word_arg {
    int32_t reg, shift;
} ieache_word_arg;
/* -> an ordinary ieache_netlist: every ieache_*netlist* call, ieache_job.netlist and the group forms take it unchanged, and
 * ieache_netlist_destroy frees it.  NULL with ieache_last_error() on refusal; where an instruction is at fault the message is
 * "program: instruction I: ...": an operand that names a register not defined there, a width mismatch, a width the kind
 * table refuses, a word or sum width outside 1 .. IEACHE_WORD_MAX_WIDTH, more than 2^30 wires, side-array ranges that do not lie
 * in the arrays given and -- without IEACHE_PROGRAM_FOLD -- an instruction that would put one wire twice into a MAJ3 / XOR3
 * (a SUM of a register with itself at overlapping positions): the noise rule of DESIGN.md section 7 stands.  No outputs,
 * no inputs and unknown flags are refused too.  Nothing is returned half-built. */
ieache_netlist* ieache_program_compile(const ieache_word_instr* instrs, size_t n_instrs, const ieache_word_arg* args, size_t n_args,
                                       const uint32_t* const_words, size_t n_const_words, const int32_t* outputs, size_t n_outputs,
                                       int flags);
/* The recorded gate list of ANY compiled netlist -- from ieache_netlist_create too -- in ieache_net_gate form, wire numbering and
 * reference encoding those of ieache_netlist_create; `outputs` gets the output references.  -> the gate count; gates are
 * written when cap holds them all and outputs when out_cap holds them all (cap = 0, out_cap = 0: only counts; the output count
 * is ieache_netlist_info's n_outputs).  For a program built with IEACHE_PROGRAM_FOLD these are the gates AFTER folding.  Fed
 * back to ieache_netlist_create (same IEACHE_NETLIST_BALANCED) the list gives a netlist with the same ieache_netlist_info:
 * what lets a caller -- or a test, on another implementation -- walk a program gate by gate. */
int64_t ieache_netlist_export(const ieache_netlist* nl, ieache_net_gate* gates, size_t cap, int32_t* outputs, size_t out_cap);

/* plaintext simulation of the levelised circuit (host only, no GPU): bits in/out 0/1 */
int ieache_circuit_simulate(int kind, int bits, const uint8_t* in_bits, uint8_t* out_bits);
int ieache_circuit_simulate_ex(int kind, int bits, int fold_constants, const uint8_t* in_bits, uint8_t* out_bits);

/* stage hooks for parity tests (host rows): blind rotation from the
 * test-vector after `steps` CMux steps (<0: all n) -> acc [count][2][N];
 * key switch u [count][N+1] -> out [count][n+1] */
int ieache_debug_blind_rotate(ieache_ctx* ctx, size_t count, const int32_t* x, int32_t* acc, int32_t steps);
int ieache_debug_keyswitch(ieache_ctx* ctx, size_t count, const int32_t* u, int32_t* out);
/* The transform probe (csrc/fft_probe.h), for tests: the 512-point transform every N = 1024 kernel multiplies polynomials
 * with, its twiddle table and the prepared key spectra, as doubles before any rounding.  Host arrays in and out; complex values
 * are (re, im) pairs of doubles.  Each returns IEACHE_EINVAL with the reason in ieache_last_error() -- and has written nothing --
 * for a null pointer, for a context whose ring is not N = 1024, k = 1 (all but ieache_debug_spectrum's which = 2), for an
 * unknown `which` or form, an odd count on a paired form, and polynomials outside the key.
 *
 * ieache_debug_twiddles: out [576][2], the table of csrc/tw_roots.h -- entry 64 k + lane = exp(i pi lane (1 - 4 k) / 1024),
 * entry 512 + 8 k + p0 = exp(-2 pi i p0 k / 64).  which = 0: the table the blind-rotation kernels load; 1: the CMux
 * family's, built now if no TGSW set has been prepared yet, as the first ieache_tgsw_prepare would; 2: a table built
 * inside a 64-thread kernel, as the key-preparation kernels build theirs.
 *
 * ieache_debug_fft512: `count` transforms in form `form`, four per workgroup as the kernels sit.
 *   form 0 .. 4, forward: in [count][512][2], y_j = p[j] + i p[j + 512] in natural order; out [count][8][64][2] raw,
 *     out[t][k2][lane] = X[k0 + 8 k1 + 64 k2] with lane = 8 k0 + k1, X_k = sum_j y_j exp(i pi j (1 - 4 k) / 1024).
 *     0: <true, 0>; 1: <true, 1>; 2: <true, 1, hook, late>; 3: <true, 1, hook, early, resident roots>; 4: <true, 0, hook>.
 *   form 5 .. 7, inverse: in [count][8][64][2] in that layout; out [count][8][64][2], out[t][r][lane] = y_{64 r + lane}, the
 *     double a kernel is about to round (normalised: the 1/512 and the untwist applied).  5: fft512_inverse; 6: the paired
 *     inverse, transforms 2 i and 2 i + 1 through one call (count even); 7: the paired inverse on resident roots.
 *   csrc/fft_probe.h lists which kernels use which form.
 *
 * ieache_debug_spectrum: `count` prepared polynomials of the bootstrapping key from polynomial `first` on, polynomial
 * (i 2l + row) 2 + c being bk[i][row][c], as a launch reads them.
 *   which = 0: two-limb, 64-lane order: out [count][2 limbs: low, high][8][64][2], each limb laid out as a forward form's output
 *   which = 1: one-limb, 64-lane order: out [count][8][64][2], the transform of the 32-bit words themselves
 *   which = 2: the any-parameter kernel's, any ring: out [count][2 limbs][N/2][2], entry m of a limb = X_{bitrev(m)} (bit reversal
 *     over log2(N/2) bits), X_k = sum_j y_j exp(i pi j / N) exp(-2 pi i j k / (N/2))
 * The limbs of a word w: low = (int16_t)w, high = (w - low) >> 16, so that w = low + 2^16 high with high in [-2^15, 2^15]. */
int ieache_debug_twiddles(ieache_ctx* ctx, int which, double* out);
int ieache_debug_fft512(ieache_ctx* ctx, int form, size_t count, const double* in, double* out);
int ieache_debug_spectrum(ieache_ctx* ctx, int which, size_t first, size_t count, double* out);
/* Which form of the forward transforms' lane-high transpose the launches of k_blind_rotate_w1b's default-guard builds take from
 * here on, in every context of the process: 2, the exchange form (one DPP move per dword for lane bit 3; the default), or 1, the
 * v_cndmask form built beside it.  Both give the same words: the partner of an A/B and of a test.  A process starts with
 * the value of IEACHE_W1B_FORWARD (1 or 2) if that is set.  IEACHE_EINVAL for another value.  No device needed. */
int ieache_debug_forward_path(int xlane);
/* The plan of a rotation of roles (option "br_mix") for a launch of `gates` gate instances on a device of `cus` compute units,
 * rotations of n steps, one-wave turns of s1 steps, two-wave turns of s1 x ratio_x100 / 100: returns 1 and out = {subsets k,
 * subsets on two waves at a time, s1, s2, whole rounds, shortened round's s1, s2, steps covered by the rounds (< n), gate
 * instances per subset}, or 0 (out zeroed) when that launch size takes a single kernel.  No device needed (csrc/mix_plan.h). */
int ieache_debug_mix_plan(int cus, int n, int64_t gates, int s1, int ratio_x100, int out[9]);

/* ------------------------------------------------------------------ *
 * 3e. Packing key switch: LWE rows into one TLWE sample.  The public   *
 *    functional key switch of Chillotti, Gama, Georgieva, Izabachene   *
 *    (Algorithm 2) with f = placement of the phases into coefficients. *
 * ------------------------------------------------------------------ */
/* The contract.  The parameter set p comes from the context; the packing decomposition (pk_t, pk_basebit) is written t, b.
 * The LWE key s is n binary words, the ring key N binary words.
 *
 * Packing key PK [n][t][2][N] int32: PK[i][j] is a TLWE sample under the ring key (A then B, phase B - A s_ring, as
 * everywhere here) of the constant polynomial whose coefficient 0 is s_i 2^(32 - (j+1) b) and whose other coefficients are 0.
 * There is no `base` dimension, unlike the LWE key-switch key: the digit multiplies the row.
 *
 * Digits are lweKeySwitch's: abar = a_i + 2^(31 - t b) (uint32), d_{i,j} = (abar >> (32 - (j+1) b)) & (2^b - 1), j = 0 .. t-1.
 *
 * A call takes groups x m LWE rows (m >= 1), an integer spread w >= 1 with m w <= N, and a shift in [0, 2N).  Per row r
 * with words (a, b_r):
 *
 *   R_r   = (0, b_r X^0) - sum_{i<n} sum_{j<t} d_{r,i,j} PK[i][j]              (scalar x [2][N], mod 2^32)
 *   out_g = sum_{p<m} sum_{q<w} X^((p w + q + shift) mod 2N) R_{g m + p}       (negacyclic: X^N = -1, mod 2^32)
 *
 * out is [groups][2][N], A then B.  The phase of out_g is sum_p phi_p X^shift (X^(p w) + ... + X^(p w + w - 1)) plus noise,
 * phi_p the phase of row p.  spread = 1, shift = 0 puts bit p at coefficient p: output compaction, read back with
 * ieache_tlwe_phase.  m = entries, spread = N / entries, shift = 2N - N / (2 entries) gives an encryption of exactly
 * ieache_lut_test_poly(f) from encrypted entries f[e]: a table for ieache_pbs with IEACHE_PBS_TLWE_POLYS built by the cloud.
 * This is an integer definition: every implementation gives the same words whatever its order of summation (the device
 * computes the first line as an int8 matrix product, csrc/pack_keyswitch.hip; nothing is rounded, guarded or audited).
 *
 * Accepted: b in 1 .. 4, t >= 1, t b < 32, n t (2^b - 1) 128 < 2^31, on any supported parameter set with N <= 1024; anything else is
 * IEACHE_EINVAL with a message, when the key is generated and when it is set.
 *
 * ieache_ctx_set_packing_key takes the key from HOST memory and keeps only its device form; a second call replaces the first
 * key, pk == NULL drops it and the device scratch of its calls (pk_t / pk_basebit are then ignored).  ieache_pack_device: d_rows [groups m][lwe_stride] ->
 * d_out [groups][2][N], on the context's stream like every device form; ieache_pack: rows [groups m][n+1] through the
 * context's staging rows (a warm call allocates nothing).  A call is cut into pieces of whole groups of at most
 * "pack_piece_rows" rows (default and most 4096); "pack_split" forces the product's K split (1, 2, 4 or 8, no more than the
 * K steps ceil(n t / 32); 0 = by size; a new key resets it).  stats: bootstraps == 0, levels == 1, keyswitch_launches == chunks
 * == pieces, keyswitch_ms and total_ms filled.  groups == 0 is a no-op.  IEACHE_EINVAL with ieache_last_error text: no
 * packing key set; m < 1, spread < 1, m spread > N; shift outside [0, 2N); device form: output overlapping input.
 * ieache_packing_keygen and ieache_pack_reference are in section 4.  There is no group form. */
int ieache_ctx_set_packing_key(ieache_ctx* ctx, int32_t pk_t, int32_t pk_basebit, const int32_t* pk /*host [n][t][2][N]*/);
/* How a call of `groups` groups of m rows would be cut under the options as they are (csrc/pack_plan.h decides, nothing else):
 * out = {pieces, groups per piece, K split of the product, K steps}.  IEACHE_EINVAL without a packing key or for m < 1. */
int ieache_debug_pack_plan(const ieache_ctx* ctx, size_t groups, int32_t m, int64_t out[4]);
int ieache_pack_device(ieache_ctx* ctx, size_t groups, int32_t m, int32_t spread, int32_t shift,
                       const int32_t* d_rows /*[groups*m][lwe_stride]*/, int32_t* d_out /*[groups][2][N]*/, ieache_stats* stats);
int ieache_pack(ieache_ctx* ctx, size_t groups, int32_t m, int32_t spread, int32_t shift,
                const int32_t* rows /*[groups*m][n+1]*/, int32_t* out /*[groups][2][N]*/, ieache_stats* stats);

/* ------------------------------------------------------------------ *
 * 3f. External product and CMux on TGSW samples the caller supplies,  *
 *    the CMux-tree lookup, and the extraction of a coefficient:       *
 *    levelled evaluation (Chillotti, Gama, Georgieva, Izabachene,     *
 *    tGswExternMulToTLwe / CMux) as public calls.                     *
 * ------------------------------------------------------------------ */
/* The contract.  Integer definitions, mod 2^32, polynomial products negacyclic (X^N = -1).  l, Bgbit come from the context.
 *
 * TGSW sample C [2l][2][N] int32: every row a TLWE sample under the ring key (A then B, phase B - A s_ring); row bloc l + q
 * (bloc 0 = A, 1 = B; q = 0 .. l-1) encrypts zero plus mu 2^(32 - (q+1) Bgbit) added to coefficient 0 of polynomial `bloc`.
 * That is how the bootstrapping key's BK_i is built (mu = the key bit): bk[i] of any key IS a valid sample, and
 * ieache_tgsw_encrypt (section 4) makes fresh ones with the same routine.
 *
 * External product C [.] d of a TLWE sample d = (dA, dB), with the blind rotation's decomposition (truncating, with offset):
 *   offset = sum_{q=1..l} 2^(Bgbit-1) << (32 - q Bgbit),  w = u32(x) + offset,
 *   dig_q(x) = ((w >> (32 - q Bgbit)) & (2^Bgbit - 1)) - 2^(Bgbit-1)             per coefficient x,
 *   rows 0 .. l-1 take the digits q = 1 .. l of dA, rows l .. 2l-1 those of dB,
 *   C [.] d = sum_r dig_r (A_r, B_r),  every product negacyclic and exact.
 * CMux: out = d0 + C [.] (d1 - d0): d1's message when mu = 1, d0's when mu = 0; d0 == NULL stands for zeros and gives the
 * external product alone.
 * Tree: an item has `depth` selectors C_0 .. C_{depth-1} (bit k of the index, least significant first) and a table
 * T [2^depth][2][N]; level k maps rows (2j, 2j+1) of the level before to CMux(C_k, row 2j+1, row 2j); the row left after `depth`
 * levels is T[index] plus noise.  depth = 0 copies row 0 of the table.
 * Every implementation returns the same words: the device computes the products on the two-limb spectrum, whose sums stay
 * below 2l N 2^(Bgbit-1) 2^15 <= 2^37 of the 2^53 an FP64 mantissa holds, so the result is exact for ANY caller words, key-like
 * or not.  Nothing is rounded, guarded or audited.
 *
 * A prepared set of n samples is an object: its spectrum (192 KB per sample at l = 3) is made once and used by many rows.
 * ieache_tgsw_prepare takes samples [n][2l][2][N] from host memory, ieache_tgsw_prepare_device from device memory; NULL with
 * ieache_last_error text for n < 1 and on a context whose parameter set the CMux kernels do not cover (they cover N = 1024,
 * k = 1 with (l, Bgbit) = (3, 7) or (2, 10); the CPU references of section 4 take every supported set).  The set owns its
 * device memory and nothing of the context's: ieache_tgsw_free may come BEFORE OR AFTER ieache_ctx_destroy of the context that
 * prepared it.  Only that context accepts it.
 *
 * Row i of ieache_cmux uses sample sel_of[i]; sel_of == NULL: sample i mod n.  Item i of ieache_lut_tree uses samples
 * sel_of[i depth + k], k = 0 .. depth-1; sel_of == NULL: (i depth + k) mod n; and table table_of[i] of
 * tables [n_tables][2^depth][2][N]; table_of == NULL: table 0.  A call is cut into pieces of whole rows / items so that no
 * launch, and no first level of a tree, holds more than "cmux_piece_rows" rows (default 8192, which bounds the tree's scratch --
 * two buffers the context keeps -- at 96 MB; a single item wider than that still runs, alone).  ieache_tlwe_extract is the
 * partner of ieache_keyswitch: coefficient j = coef_of[i] (NULL: 0) of TLWE sample i becomes the extracted row u[i'] = A[j - i']
 * for i' <= j, -A[N + j - i'] otherwise, u[N] = B[j], rows shaped as IEACHE_PBS_NO_KEYSWITCH shapes them (host: N + 1 words;
 * device: ieache_extract_stride words, N + 1 written), on any supported parameter set; so lut_tree -> tlwe_extract -> keyswitch
 * brings a tree's result back among the gates.
 *
 * Host forms check every index and return IEACHE_EINVAL naming the first bad one; they stage through rows the context keeps
 * (a warm call allocates nothing).  Device forms never read an index on the host: the kernel clamps an explicit index into its
 * range, so a bad one gives a wrong answer, never a stray read.  IEACHE_EINVAL with ieache_last_error text: the output
 * overlapping any input (device forms), depth outside 0 .. IEACHE_LUT_TREE_MAX_DEPTH, n_tables < 1, a set prepared on another
 * context.  count == 0 is a no-op.  stats: bootstraps == 0, keyswitch_launches == 0, levels = 1 (cmux, tlwe_extract) or depth
 * (tree), chunks = pieces, total_ms filled.  ieache_stats has no version field, so none was added: the CMux kernel launches
 * (pieces for ieache_cmux, pieces x max(depth, 1) for a tree) and their time are reported in blind_rotate_launches and
 * blind_rotate_ms.  There is no group form and no cloudd verb. */
#define IEACHE_LUT_TREE_MAX_DEPTH 12
typedef struct ieache_tgsw ieache_tgsw;
ieache_tgsw* ieache_tgsw_prepare(ieache_ctx* ctx, const int32_t* samples /*host [n][2l][2][N]*/, size_t n);
ieache_tgsw* ieache_tgsw_prepare_device(ieache_ctx* ctx, const int32_t* d_samples /*[n][2l][2][N]*/, size_t n);
void ieache_tgsw_free(ieache_tgsw* set);
int ieache_cmux(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, const int32_t* sel_of /*[count] or NULL*/,
                const int32_t* d1 /*[count][2][N]*/, const int32_t* d0 /*[count][2][N] or NULL*/, int32_t* out /*[count][2][N]*/, ieache_stats* stats);
int ieache_cmux_device(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, const int32_t* d_sel_of, const int32_t* d_d1, const int32_t* d_d0,
                       int32_t* d_out, ieache_stats* stats);
int ieache_lut_tree(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, const int32_t* sel_of /*[count][depth] or NULL*/,
                    const int32_t* tables /*[n_tables][2^depth][2][N]*/, int32_t n_tables, const int32_t* table_of /*[count] or NULL*/,
                    int32_t* out /*[count][2][N]*/, ieache_stats* stats);
int ieache_lut_tree_device(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, const int32_t* d_sel_of, const int32_t* d_tables,
                           int32_t n_tables, const int32_t* d_table_of, int32_t* d_out, ieache_stats* stats);
int ieache_tlwe_extract(ieache_ctx* ctx, size_t count, const int32_t* tlwe /*[count][2][N]*/, const int32_t* coef_of /*[count] or NULL*/,
                        int32_t* u /*[count][N+1]*/, ieache_stats* stats);
int ieache_tlwe_extract_device(ieache_ctx* ctx, size_t count, const int32_t* d_tlwe, const int32_t* d_coef_of,
                               int32_t* d_u /*[count][extract_stride]*/, ieache_stats* stats);
/* How a call would be cut under the options as they are (csrc/cmux_plan.h decides, nothing else): depth < 0 names a flat call
 * of `count` rows, 0 .. IEACHE_LUT_TREE_MAX_DEPTH a tree over `count` items; out = {pieces, items per piece, rows of scratch A,
 * rows of scratch B}. */
int ieache_debug_cmux_plan(const ieache_ctx* ctx, size_t count, int32_t depth, int64_t out[4]);

/* 3g. The write at an encrypted index: the CMux demux tree, partner of ieache_lut_tree.  Conventions, sets, decomposition and
 * exactness are those of 3f (integers mod 2^32; N = 1024, k = 1, (l, Bgbit) = (3, 7) or (2, 10) on the device).
 *
 * Item i has `depth` selectors C_0 .. C_{depth-1} (bit k of the index, least significant first, exactly as for the tree:
 * sample sel_of[i depth + k]; sel_of == NULL: (i depth + k) mod n), a value v [2][N] and optionally a memory block
 * mem [2^depth][2][N] of its own.  The demux runs from the most significant bit down: step t = 0 .. depth-1 uses selector
 * k = depth-1-t, and every row p at position j of the step's 2^t rows becomes two:
 *   hi = C_k [.] p  at position 2j + 1,     lo = p - hi  at position 2j.
 * After `depth` steps the 2^depth leaves are v at the encrypted index and encryptions of zero elsewhere, each plus noise, and
 *   out[j] = mem[j] + leaf[j];
 * mem == NULL stands for zeros and returns the leaves themselves: the encrypted one-hot vector times v.  depth = 0 gives
 * out[0] = mem[0] + v.  The leaves of an item always sum to v word for word.  One item costs 2^depth - 1 external products, as
 * a lookup does.  A replace write mem[addr] := new is a read, a subtraction and a scatter: delta = new - lut_tree(mem), then
 * scatter delta (the Python binding's Context.lut_write does that on host arrays).
 *
 * The device form accepts d_out == d_mem EXACTLY: the write is then in place (every word of the memory is read by the one
 * lane that later stores it).  Any other overlap of the output with an input is refused.  Pieces and scratch are the tree's:
 * whole items so that items 2^(depth-1) stays within "cmux_piece_rows", the two scratch buffers the context keeps, and
 * ieache_debug_cmux_plan(count, depth) describes a scatter as it describes a tree.  Host forms check every index and name the
 * first bad one and stage through rows the context keeps; device forms clamp.  IEACHE_EINVAL: depth outside
 * 0 .. IEACHE_LUT_TREE_MAX_DEPTH, overlap, a set prepared on another context.  count == 0 is a no-op.  stats: bootstraps == 0,
 * keyswitch_launches == 0, levels = depth, chunks = pieces, the kernel launches (pieces x max(depth, 1)) and their time in
 * blind_rotate_launches and blind_rotate_ms.  Several items writing into ONE memory in a single call are ieache_lut_add
 * (section 3j), which sums the leaves on the device; there is no group form and no cloudd verb. */
int ieache_lut_scatter(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, const int32_t* sel_of /*[count][depth] or NULL*/,
                       const int32_t* values /*[count][2][N]*/, const int32_t* mem /*[count][2^depth][2][N] or NULL*/,
                       int32_t* out /*[count][2^depth][2][N]*/, ieache_stats* stats);
int ieache_lut_scatter_device(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, const int32_t* d_sel_of,
                              const int32_t* d_values, const int32_t* d_mem, int32_t* d_out /* == d_mem: in place */, ieache_stats* stats);

/* 3h. Rotation of a TLWE sample by an encrypted amount, and the coefficient-level lookup: the last stage of vertical packing.
 * Conventions, sets, decomposition and exactness are those of 3f.
 *
 * Item i has a sample in[i] [2][N], `steps` selectors C_0 .. C_{steps-1} (sample sel_of[i steps + t]; sel_of == NULL:
 * (i steps + t) mod n) and the call has public amounts a_t in [0, 2N), shared by all items.  For t = 0 .. steps-1 in order
 *   acc <- acc + C_t [.] (X^(a_t) acc - acc),        integers mod 2^32,
 * where X^a is the negacyclic monomial product (coefficient j takes +/- coefficient j - a mod 2N: libtfhe's
 * tfhe_MuxRotate_FFT).  It is the blind rotation's step on a caller's selector: with C_t = BK_i one step is the rotation's step i
 * word for word.  A step with a_t = 0 is an exact no-op.  If C_t encrypts the bit b_t, the result encrypts
 * X^(sum b_t a_t) in[i] plus the noise of `steps` external products.  amount_of == NULL stands for a_t = 2N - 2^t (0 from
 * t = log2(2N) on): it brings coefficient sum b_t 2^t of in[i] to position 0.  With a_t = +2^t the same call moves
 * coefficient 0 to position sum b_t 2^t: followed by ieache_lut_scatter it places a value at an encrypted (slot, coefficient).
 * steps ranges over 0 .. IEACHE_ROTATE_MAX_STEPS; steps = 0 copies.
 *
 * The device form accepts d_out == d_in EXACTLY (a row is read whole before any of it is stored, and rows are disjoint); any
 * other overlap is refused.  Pieces: the flat rule of 3f, rows = items, under "cmux_piece_rows"; one launch per piece, all the
 * steps of a row inside it; no scratch, a warm call allocates nothing.  Host forms check every index and amount and name the
 * first bad one; on the device an explicit index is clamped into the set, an implied one is taken mod n and an amount is
 * masked to 2N - 1.  IEACHE_EINVAL: steps outside 0 .. IEACHE_ROTATE_MAX_STEPS, overlap, a set prepared on another context.
 * count == 0 is a no-op.  stats: bootstraps == 0, keyswitch_launches == 0, levels = steps, chunks = pieces, one launch per piece
 * (steps == 0: the same launch, which then only copies), the launches and their time in blind_rotate_launches and
 * blind_rotate_ms.
 *
 * ieache_lut_read is the vertical-packing lookup over depth + steps address bits, run on the context's stream with no host
 * round trip.  Item i has selectors sel_of[i (steps + depth) + t] (NULL: that index mod n): t = 0 .. steps-1 are the LOW address
 * bits, least significant first, t = steps .. steps+depth-1 the HIGH ones.  (1) ieache_lut_tree by the high bits over
 * tables[table_of[i]] selects one sample; (2) that ONE row per item is rotated by the low bits; (3) the public coefficient
 * `coef` (0 with the default amounts) is extracted as ieache_tlwe_extract does; (4) the key switch.  out is [count][n+1] LWE rows
 * under the LWE key, what the gates take; with IEACHE_LUT_READ_NO_KEYSWITCH the extracted rows (host: N + 1 words; device:
 * ieache_extract_stride() words).  A table of 2^(depth + log2 N) bits is 2^depth samples and costs 2^depth - 1 CMuxes plus
 * `steps` products per item.  The cut is the tree's plan for (count, depth); the selected rows and the indices of a piece are
 * reserved with the tree's scratch ahead of the loop.  stats: levels = depth + steps, chunks = pieces, the tree's, the
 * rotation's and the extraction's launches in blind_rotate_launches, the key switch's in keyswitch_launches.  Refusals as for
 * ieache_lut_tree and ieache_tlwe_rotate, coef outside [0, N) (host form; the device form clamps), an unknown flag.
 * No group form, no cloudd verb, no other rings, no one-limb form; the replace write of single coefficients is section 3l. */
#define IEACHE_ROTATE_MAX_STEPS 64
#define IEACHE_LUT_READ_NO_KEYSWITCH 1
int ieache_tlwe_rotate(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t steps, const int32_t* sel_of /*[count][steps] or NULL*/,
                       const int32_t* amount_of /*[steps] or NULL*/, const int32_t* in /*[count][2][N]*/, int32_t* out /*[count][2][N]*/,
                       ieache_stats* stats);
int ieache_tlwe_rotate_device(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t steps, const int32_t* d_sel_of,
                              const int32_t* d_amount_of, const int32_t* d_in, int32_t* d_out /* == d_in: in place */, ieache_stats* stats);
int ieache_lut_read(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, int32_t steps,
                    const int32_t* sel_of /*[count][steps+depth] or NULL*/, const int32_t* amount_of /*[steps] or NULL*/,
                    const int32_t* tables /*[n_tables][2^depth][2][N]*/, int32_t n_tables, const int32_t* table_of /*[count] or NULL*/, int32_t coef,
                    int flags, int32_t* out, ieache_stats* stats);
int ieache_lut_read_device(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, int32_t steps, const int32_t* d_sel_of,
                           const int32_t* d_amount_of, const int32_t* d_tables, int32_t n_tables, const int32_t* d_table_of, int32_t coef, int flags,
                           int32_t* d_out, ieache_stats* stats);

/* 3i. TGSW sets with a gadget of their own, and the replace write.
 * A set prepared by ieache_tgsw_prepare uses the context's (l, Bgbit), the bootstrapping key's gadget.  Nothing ties a
 * caller's selector samples to the key's decomposition: ieache_tgsw_prepare_gadget takes samples [n][2l][2][N] made with ANY
 * admissible gadget (tools: ieache_tgsw_encrypt with l and Bgbit of the ieache_params changed), on any context with N = 1024
 * and k = 1 whatever the key's own gadget -- a (2, 10) key may use (6, 5) selectors.  A finer gadget trades digit rows (the
 * work of a product grows with 2l) for noise: the truncation ramp of a product falls with 2^-(l Bgbit), its key-noise term
 * with 2^Bgbit.  Admissible: l >= 1, 1 <= Bgbit < 32, l Bgbit <= 32, 2 l N 2^Bgbit <= 2^32 (the bound
 * under which the two-limb product is exact for any words); anything else is NULL with IEACHE_EINVAL and a message naming
 * the rule that failed.  ieache_tgsw_gadget reads a set's gadget back.  Every call of sections 3f to 3h accepts such a set
 * unchanged: rows stay [2][N], pieces and scratch do not depend on the gadget, the host forms validate as before.  Sets at
 * (3, 7) and (2, 10) run on the kernels they always had; every other gadget on one further build of each kernel that takes
 * (l, Bgbit) as launch arguments.  ieache_tgsw_prepare and ieache_tgsw_prepare_device are unchanged.
 *
 * ieache_lut_write is the replace write mem[i][addr_i] := new[i], addr_i the index item i's `depth` selectors encrypt
 * (sel_of as for ieache_lut_tree and ieache_lut_scatter: [count][depth], bit k of the index first; NULL: i depth + k mod n):
 *   old_i = ieache_lut_tree over item i's own memory (table_of[i] = i),  delta_i = new[i] - old_i mod 2^32,
 *   out[i] = ieache_lut_scatter of delta_i onto mem[i],
 * word for word what the three calls composed give, on the context's stream with no host round trip; the subtraction is a
 * small pass of its own over the piece's [items][2][N] words.  It is cut into the tree's pieces for (count, depth); a piece
 * reads and writes only its own items' memories, so the device form accepts d_out == d_mem EXACTLY (the write in place);
 * any other overlap is refused.  depth 0 .. IEACHE_LUT_TREE_MAX_DEPTH.  Refusals as for ieache_lut_scatter (host form: every
 * index checked; device form: clamped / mod n), a set prepared on another context, a host pointer to a device form.
 * stats: levels = 2 depth, chunks = pieces, the launches in blind_rotate_launches.  A warm call allocates nothing. */
ieache_tgsw* ieache_tgsw_prepare_gadget(ieache_ctx* ctx, const int32_t* samples /*host [n][2l][2][N], l the set's*/, size_t n, int32_t l,
                                        int32_t Bgbit);
ieache_tgsw* ieache_tgsw_prepare_gadget_device(ieache_ctx* ctx, const int32_t* d_samples /*[n][2l][2][N]*/, size_t n, int32_t l, int32_t Bgbit);
int ieache_tgsw_gadget(const ieache_tgsw* set, int32_t* l, int32_t* Bgbit);
int ieache_lut_write(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, const int32_t* sel_of /*[count][depth] or NULL*/,
                     const int32_t* fresh /*new: [count][2][N]*/, const int32_t* mem /*[count][2^depth][2][N]*/,
                     int32_t* out /*[count][2^depth][2][N]*/, ieache_stats* stats);
int ieache_lut_write_device(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, const int32_t* d_sel_of, const int32_t* d_new,
                            const int32_t* d_mem, int32_t* d_out /* == d_mem: in place */, ieache_stats* stats);

/* 3j. Many values into shared memories in one call: mem[m_i][hi_i].coef[lo_i] += v_i.  Conventions, sets, gadgets and
 * exactness are those of 3f to 3i (integers mod 2^32; any set section 3i admits).
 *
 * The call has n_mems memories mems [n_mems][2^depth][2][N]; item i has a value values[i] [2][N], a memory mem_of[i] in
 * [0, n_mems) (mem_of == NULL: every item writes memory 0) and depth + steps selectors sel_of[i (steps + depth) + t] (NULL:
 * that index mod n), laid out as for ieache_lut_read: t = 0 .. steps-1 are the LOW address bits, least significant first,
 * t = steps .. steps+depth-1 the HIGH ones.  Three steps, each an existing definition:
 *   (1) w_i = ieache_tlwe_rotate of values[i] by selectors 0 .. steps-1 with the public amounts a_t; amount_of == NULL stands
 *       for a_t = +2^t mod 2N -- the OPPOSITE of ieache_lut_read's default: it moves coefficient 0 to the encrypted position;
 *       steps == 0 gives w_i = values[i];
 *   (2) leaves_i = ieache_lut_scatter of w_i by selectors steps .. steps+depth-1 with mem == NULL: [2^depth][2][N];
 *   (3) out[m][j] = mems[m][j] + the sum of leaves_i[j] over the items with mem_of[i] = m;  mems == NULL stands for zeros.
 * Word for word the three references composed and summed: depth == 0, steps == 0 is out[m][0] = mems[m][0] + sum v_i, and one
 * item with n_mems = 1 and steps = 0 is ieache_lut_scatter bit for bit.  The sum is formed on the device by the last demux
 * step of each piece itself, with integer atomic adds: they are order-free mod 2^32, so the words do not depend on the order
 * the adds arrive in, and a call repeated gives identical words.  Nothing of the size of the leaves (count x 2^depth rows) is
 * ever stored.  Each addition brings a scatter's noise (and a rotation's) to EVERY slot of its memory: DESIGN.md section 7
 * gives the number of additions a memory takes.
 *
 * The device form accepts d_out == d_mems EXACTLY: the write in place -- nothing of the memory is read, it is only added to.
 * Any other overlap of d_out with an input is refused; with distinct buffers d_out is initialised from d_mems (NULL: zero-filled)
 * on the context's stream before the first piece.  The cut is the tree's plan for (count, depth), ieache_debug_cmux_plan; the
 * items of one memory may fall into different pieces, which changes nothing.  Scratch is ieache_lut_read's; a warm call
 * allocates nothing.  depth 0 .. IEACHE_LUT_TREE_MAX_DEPTH, steps 0 .. IEACHE_ROTATE_MAX_STEPS, n_mems >= 1.  Host forms check
 * every index and amount and name the first bad one; device forms clamp an explicit selector (an implied one is taken mod n),
 * clamp mem_of into [0, n_mems) and mask amounts to 2N - 1.  count == 0 returns mems unchanged (zeros for NULL).
 * IEACHE_EINVAL: depth, steps or n_mems out of range, overlap, a set prepared on another context, a host pointer to a device
 * form.  stats: bootstraps == 0, keyswitch_launches == 0, levels = depth + steps, chunks = pieces, blind_rotate_launches =
 * pieces x ((steps > 0 ? 1 : 0) + max(depth, 1)); the initialising copy or fill and the small index pass are not counted.
 * No group form, no cloudd verb, no other rings, no one-limb form; the replace write of single coefficients is section 3l. */
int ieache_lut_add(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, int32_t steps,
                   const int32_t* sel_of /*[count][steps+depth] or NULL*/, const int32_t* amount_of /*[steps] or NULL*/,
                   const int32_t* values /*[count][2][N]*/, const int32_t* mems /*[n_mems][2^depth][2][N] or NULL*/, int32_t n_mems,
                   const int32_t* mem_of /*[count] or NULL*/, int32_t* out /*[n_mems][2^depth][2][N]*/, ieache_stats* stats);
int ieache_lut_add_device(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, int32_t steps, const int32_t* d_sel_of,
                          const int32_t* d_amount_of, const int32_t* d_values, const int32_t* d_mems, int32_t n_mems, const int32_t* d_mem_of,
                          int32_t* d_out /* == d_mems: in place */, ieache_stats* stats);

/* 3k. Deterministic (weighted) finite automata over words whose letters are TGSW-encrypted bits: the sequential shape among
 * the calls on a set, where 3f to 3j are a tree, a demux tree and a rotation.  Conventions, sets, gadgets and exactness are
 * those of 3f to 3i (integers mod 2^32; any set section 3i admits; N = 1024, k = 1).
 *
 * An automaton has `states` Q in 1 .. IEACHE_AUTOMATON_MAX_STATES, `steps` p in 0 .. IEACHE_AUTOMATON_MAX_STEPS, n_out in
 * 1 .. Q and public transition tables next0, next1 [steps][states] with entries in [0, Q), which may differ from step to step.
 * For item i, with the set's samples C, the selectors sel_of[i steps + t] (NULL: that index mod n) and the final rows
 * finals[final_of[i]] [states][2][N] (final_of == NULL: 0):
 *     V_p[q] = finals[final_of[i]][q]
 *     V_t[q] = CMux(C_sel(i,t), d1 = V_{t+1}[next1[t][q]], d0 = V_{t+1}[next0[t][q]])      t = p-1 .. 0
 *     out[i][q] = V_0[q]                                                                   q < n_out
 * CMux is word for word ieache_cmux_reference, d0 + C [.] (d1 - d0) with the SET's gadget.  Letter t of the word is the one the
 * automaton reads t-th when it runs forward from state q; the evaluation runs backward, as in the TFHE paper, so out[i][q] is an
 * encryption of the final row the forward run from q ends in.  With finals of +-1/8 in coefficient 0, ieache_tlwe_extract and
 * ieache_keyswitch turn out[i][0] into a gate input.  p CMuxes bring p times a CMux's noise: DESIGN.md section 7 gives the steps
 * each gadget allows.
 *
 * The automaton is an object compiled once and run many times, like a netlist or a set.  ieache_automaton_create takes the
 * tables from host memory, refuses a bad scalar or the first out-of-range entry by name ("next1[t][q] = v is outside [0, Q)":
 * scalars first, then entries in the order step, state, next0 before next1), computes per step the 64-bit mask of LIVE states
 * (live_0 = [0, n_out), live_{t+1} = the image of live_t under both tables of step t) and uploads tables and masks.  It returns
 * NULL on failure (ieache_last_error).  ieache_automaton_free may come before or after the context is destroyed; only the
 * context that compiled an automaton accepts it.  ieache_automaton_info: states, steps, n_out and the live CMuxes per item --
 * the live (t, q) whose two tables differ; where they agree the CMux is exactly d0 and the device copies the row.
 * ieache_automaton_check is the same validation with no context and no GPU: 0, or IEACHE_EINVAL with the message.
 *
 * ieache_automaton_run is the host form, ieache_automaton_run_device the same on device pointers on the context's stream:
 * finals [n_finals][states][2][N], out [count][n_out][2][N] packed.  ANY overlap of out with finals (or an index array) is
 * refused: there is no in-place form.  One workgroup runs every step of an item inside one launch and hands the state vector
 * from wave to wave through two scratch buffers of `states` rows per item; dead states are skipped and
 * states whose tables agree copied, which leaves every word of out unchanged.  The cut (ieache_debug_automaton_plan: pieces,
 * items per piece, scratch rows, steps per launch, launches per piece): pieces of whole items with 2 x states scratch rows each
 * within the option "cmux_piece_rows" (an item wider than the cap runs alone); the steps of a piece in one launch, or with the
 * option "automaton_steps_per_launch" = k > 0 in consecutive launches of at most k steps (1: a launch per step); the default 0
 * cuts only where steps x ceil(states / 4) exceeds 8 192.  Scratch is reserved before the first piece; a warm call allocates
 * nothing.  steps == 0 copies the final rows.  Host form: every index is checked first and the first bad one named; device
 * form: an explicit selector is clamped into the set (an implied one taken mod n) and final_of into [0, n_finals).
 * IEACHE_EINVAL: a set or an automaton of another context, N != 1024, null pointers, n_finals < 1, overlap, a host pointer to the
 * device form.  stats: bootstraps == 0, keyswitch_launches == 0, levels = steps, chunks = pieces, blind_rotate_launches =
 * pieces x launches per piece, their time in blind_rotate_ms.
 * No per-item automata in one call, no group form, no cloudd verb, no weights other than TLWE rows, no other rings, no one-limb form. */
#define IEACHE_AUTOMATON_MAX_STATES 64
#define IEACHE_AUTOMATON_MAX_STEPS 4096
typedef struct ieache_automaton ieache_automaton;
ieache_automaton* ieache_automaton_create(ieache_ctx* ctx, int32_t states, int32_t steps, int32_t n_out, const int32_t* next0 /*[steps][states]*/,
                                          const int32_t* next1 /*[steps][states]*/);
void ieache_automaton_free(ieache_automaton* a);
int ieache_automaton_info(const ieache_automaton* a, int32_t* states, int32_t* steps, int32_t* n_out, int64_t* cmuxes);
int ieache_automaton_check(int32_t states, int32_t steps, int32_t n_out, const int32_t* next0, const int32_t* next1);
int ieache_automaton_run(ieache_ctx* ctx, const ieache_tgsw* set, const ieache_automaton* a, size_t count, const int32_t* sel_of /*[count][steps] or NULL*/,
                         const int32_t* finals /*[n_finals][states][2][N]*/, int32_t n_finals, const int32_t* final_of /*[count] or NULL*/,
                         int32_t* out /*[count][n_out][2][N]*/, ieache_stats* stats);
int ieache_automaton_run_device(ieache_ctx* ctx, const ieache_tgsw* set, const ieache_automaton* a, size_t count, const int32_t* d_sel_of,
                                const int32_t* d_finals, int32_t n_finals, const int32_t* d_final_of, int32_t* d_out, ieache_stats* stats);
int ieache_debug_automaton_plan(const ieache_ctx* ctx, const ieache_automaton* a, size_t count, int64_t out[5]);

/* 3l. The TLWE projection, and the replace write of single coefficients of an encrypted memory.
 *
 * The projection is a public functional key switch with f = projection onto a window of coefficients: out carries the phase of
 * coefficients first .. first + width - 1 of a TLWE sample at dest .. dest + width - 1 (negacyclic) and ZERO everywhere else,
 * plus the key switch's noise.  It is section 3e's packing key switch on the parameter set with n := N and the ring key as its
 * source key -- the extracted key of a TLWE sample is the ring key itself -- so every definition is one that exists:
 *
 * Projection key PK' [N][t][2][N] int32: ieache_packing_keygen for the parameter set with n := N, given the ring key's N words
 * as its "LWE key" (ieache_amd.tools.projection_keygen).  ieache_ctx_set_projection_key takes it from HOST memory and keeps only
 * the byte-limb device form (67 MB at t = 8); it replaces and drops exactly as ieache_ctx_set_packing_key does, refuses the
 * decompositions section 3e refuses on that parameter set, and is independent of the packing key: a context may hold both.
 *
 * ieache_tlwe_project: the window (first in [0, N), width >= 1 with first + width <= N, dest in [0, 2N)) is public and shared by
 * the call.  Word for word, for item i:
 *   u_q    = ieache_tlwe_extract(in[i], coef = first + q),  q < width                       (N + 1 words each)
 *   out[i] = ieache_pack_reference(p', PK', groups = 1, m = width, spread = 1, shift = dest, rows = u_0 .. u_{width-1})
 * An integer definition, the same words in any order of summation; nothing is rounded, guarded or audited.  On the device the
 * extracted rows (count x width x 4 KB) are never stored: one kernel writes their digits and R = (0, B[first + q] X^0) from the
 * samples, then section 3e's product (K = N t) and placement run unchanged.  The digit of an entry -A[.] is the digit of the
 * negated word, not the negated digit.  Pieces are whole items with items x width rows within "pack_piece_rows";
 * "project_split" forces the product's K split as "pack_split" does (a new key resets it); ieache_debug_project_plan reports
 * {pieces, items per piece, K split, K steps}.  Scratch is reserved before the loop: a warm call allocates nothing.  Device
 * form: d_in, d_out [count][2][N] packed, ANY overlap of d_out with d_in refused.  stats as ieache_pack: bootstraps == 0,
 * levels == 1, keyswitch_launches == chunks == pieces.  count == 0 is a no-op.  IEACHE_EINVAL with text: no projection key set; a
 * window out of range; a host pointer to the device form.
 *
 * ieache_lut_write_coef is the replace write  mem[i][hi_i].coef[lo_i unit .. lo_i unit + width) := new[i].coef[0 .. width).
 * Memories are per item as in ieache_lut_write, [count][2^depth][2][N]; sel_of is [count][steps + depth] laid out as for
 * ieache_lut_read and ieache_lut_add (the `steps` LOW address bits first; NULL: that index mod n); width <= unit and
 * unit 2^steps <= N (the Python forms default unit to width).  Each step is an existing definition:
 *   (1) r_i     = ieache_lut_tree over mem[i] by the high selectors;
 *   (2) r_i    <- ieache_tlwe_rotate by the low selectors with the amounts (2N - unit 2^t) mod 2N;
 *   (3) old_i   = ieache_tlwe_project(r_i, first 0, width, dest 0);
 *   (4) delta_i = new[i] - old_i mod 2^32, on all 2N words;
 *   (5) out     = ieache_lut_add(values = delta, depth, steps, amounts +unit 2^t, mems = mem, n_mems = count, mem_of[i] = i).
 * `new` must carry NOTHING outside its first `width` coefficients -- an ieache_pack result, a client's encryption, an
 * ieache_tlwe_project result; the call does not project it.  The written window ends as new's phase plus the noise of one read
 * path, one projection and one write path (the old content's own noise cancels); every other coefficient and slot takes one
 * ieache_lut_add's noise.  depth = steps = 0 gives mem + new - project(mem).
 * The device form runs on the context's stream with no host round trip; step (4) is a small pass of its own.  It is cut into the
 * tree's pieces for (count, depth), the projection in runs of its own plan inside a piece; a piece reads and adds into its own
 * items' memories only, so d_out == d_mem EXACTLY is the write in place, and any other overlap is refused; with distinct buffers
 * d_out starts as a copy of d_mem.  A warm call allocates nothing.  Any set section 3i admits.  Host form: every selector
 * checked and the first bad one named; device form: clamped / mod n.  stats: bootstraps == 0, levels = 2 (depth + steps) + 1,
 * chunks = pieces, keyswitch_launches = the projection's runs (pieces while a piece's items x width fit "pack_piece_rows"),
 * blind_rotate_launches = pieces x (2 max(depth, 1) + 2 (steps > 0 ? 1 : 0) + 1): the tree (a copy at depth 0), the two
 * rotations, the subtraction and the scatter; the small index passes and the initialising copy are not counted.
 * IEACHE_EINVAL: no projection key set; depth, steps outside their ranges; width < 1; unit < width; unit 2^steps > N; overlap; a set
 * of another context; a host pointer to the device form.
 * The way back to the gates -- the written word read as LWE rows -- is section 3m.
 * Not here: projecting `new`, several items replacing into ONE memory (two at one address would both
 * subtract the old value), a group form, a cloudd verb, a key-file format; the tree, rotation and scatter cover N = 1024 only,
 * the projection alone any supported set. */
int ieache_ctx_set_projection_key(ieache_ctx* ctx, int32_t pk_t, int32_t pk_basebit, const int32_t* pk /*host [N][t][2][N]*/);
int ieache_debug_project_plan(const ieache_ctx* ctx, size_t count, int32_t width, int64_t out[4]);
int ieache_tlwe_project(ieache_ctx* ctx, size_t count, int32_t first, int32_t width, int32_t dest, const int32_t* in /*[count][2][N]*/,
                        int32_t* out /*[count][2][N]*/, ieache_stats* stats);
int ieache_tlwe_project_device(ieache_ctx* ctx, size_t count, int32_t first, int32_t width, int32_t dest, const int32_t* d_in, int32_t* d_out,
                               ieache_stats* stats);
/* (The ieache_lut_write_coef declarations are spelled with `extern`, which changes nothing for a C or C++ caller: it sets them
 * apart from section 3i's ieache_lut_write family, whose declarations tests/test_gadget_cpu.py enumerates by that prefix.) */
extern int ieache_lut_write_coef(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, int32_t steps, int32_t width, int32_t unit,
                                 const int32_t* sel_of /*[count][steps+depth] or NULL*/, const int32_t* fresh /*new: [count][2][N]*/,
                                 const int32_t* mem /*[count][2^depth][2][N]*/, int32_t* out /*[count][2^depth][2][N]*/, ieache_stats* stats);
extern int ieache_lut_write_coef_device(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, int32_t steps, int32_t width, int32_t unit,
                                 const int32_t* d_sel_of, const int32_t* d_new, const int32_t* d_mem, int32_t* d_out /* == d_mem: in place */,
                                 ieache_stats* stats);

/* 3m. The way back to the gates: the unpacking key switch, and the read of an addressed word.
 *
 * Sections 3e to 3l carry gate outputs into TLWE samples and work on them there; these two calls carry coefficients of TLWE
 * samples back to LWE rows under the gate key, many per call.  All arithmetic is integer mod 2^32 and every definition is a
 * composition of definitions that exist: nothing is rounded, guarded or audited.
 *
 * ieache_unpack, the partner of ieache_pack: the window (first, width, spread) is public and shared by the call.  For item i
 * and q < width:
 *   u_{i,q}   = ieache_tlwe_extract(in[i], coef = first + q spread)                        (N + 1 words)
 *   out[i][q] = lweKeySwitch(u_{i,q})                     (what ieache_keyswitch gives for that row)
 * Rule: first in [0, N), width >= 1, spread >= 1, first + (width - 1) spread < N; anything else is IEACHE_EINVAL naming the
 * rule.  ieache_unpack(first = shift, spread) reads back what ieache_pack(spread, shift) placed.  in [count][2][N] packed; the
 * host out [count][width][n+1]; the device d_out [count][width] rows of ieache_lwe_stride words.  IEACHE_UNPACK_NO_KEYSWITCH
 * returns the extracted rows u instead: N + 1 words per row on the host, rows of ieache_extract_stride() words on the device.
 * Any parameter set the key switch supports (no CMux kernel is involved).  The count x width rows are cut into runs of at most
 * `chunk` rows as every flat call's are; a run may begin and end inside an item.  Where the key switch's plan for a run is the
 * MFMA product, the extracted rows (rows x 4 KB) are never stored: k_ksm_window_digits and k_ksm_window_init write the product's
 * transposed digits and initial rows from the samples (the digit of an entry -A[.] is the digit of the negated word, not the
 * negated digit).  Below "ks_mfma_min", under force_generic and on a set without the product the run's rows are stored and walked
 * as ieache_keyswitch walks them.  Every family gives the same words.  ANY overlap of the output with the input is refused;
 * count == 0 is a no-op; a warm call allocates nothing.
 * stats: bootstraps == 0, levels == 1, chunks == runs == ceil(count width / min(count width, chunk)); keyswitch_launches == runs
 * and the runs' time in keyswitch_ms -- what ieache_keyswitch reports for the same rows; with IEACHE_UNPACK_NO_KEYSWITCH
 * keyswitch_launches == 0 and the extraction is in total_ms alone; blind_rotate_launches == 0.
 *
 * ieache_word_read, the partner of ieache_lut_write_coef with its address convention:
 *   out[i][q] = LWE row of  tables[table_of[i]][hi_i].coef[lo_i unit + q],   q < width
 *   (1) r_i  = ieache_lut_tree over tables[table_of[i]] by item i's HIGH `depth` selectors;
 *   (2) r_i <- ieache_tlwe_rotate by its LOW `steps` selectors with the amounts (2N - unit 2^t) mod 2N  (ieache_lut_write_coef's step 2);
 *   (3) out[i] = ieache_unpack(r_i, first 0, width, spread 1), with the same flag.
 * The arguments are ieache_lut_read's with coef and amount_of replaced by width and unit: sel_of [count][steps + depth] laid
 * out as in 3h / 3l (NULL: that index mod n), tables [n_tables][2^depth][2][N], table_of [count] or NULL.  Any set section 3i
 * admits; N = 1024 only, as the tree and the rotation are.  width 1 is ieache_lut_read with coef 0 and those amounts, word for
 * word.  The device form runs on the context's stream with no host round trip: the tree's pieces for (count, depth), the
 * selected rows rotated in place in the context's scratch, then a piece's items x width rows unpacked in runs of at most
 * `chunk`; everything is reserved before the first piece.  Host form: every selector and table index checked and the first bad
 * one named; device form: clamped / mod n.
 * stats: bootstraps == 0, levels == depth + steps, chunks == pieces, blind_rotate_launches == pieces x (max(depth, 1) +
 * (steps > 0 ? 1 : 0)) -- the tree (a copy at depth 0) and the rotation; the small index passes are not counted --
 * keyswitch_launches == the sum over pieces of ceil(items width / min(items width, chunk)), 0 with the flag.
 * IEACHE_EINVAL, in ieache_lut_read's order: depth, steps outside their ranges; n_tables < 1; an unknown flag; then the window's
 * rules, which are ieache_lut_write_coef's: width < 1; unit < width; unit 2^steps > N; overlap of the output with any input; a set
 * of another context; null pointers; a host pointer to the device form.  A refused call writes nothing.
 * Not here: group forms, cloudd verbs, other rings for the tree and the rotation, a one-limb form. */
#define IEACHE_UNPACK_NO_KEYSWITCH 1
int ieache_unpack(ieache_ctx* ctx, size_t count, int32_t first, int32_t width, int32_t spread, const int32_t* in /*[count][2][N]*/, int flags,
                  int32_t* out /*[count][width][n+1]*/, ieache_stats* stats);
int ieache_unpack_device(ieache_ctx* ctx, size_t count, int32_t first, int32_t width, int32_t spread, const int32_t* d_in, int flags, int32_t* d_out,
                         ieache_stats* stats);
int ieache_word_read(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, int32_t steps, int32_t width, int32_t unit,
                     const int32_t* sel_of /*[count][steps+depth] or NULL*/, const int32_t* tables /*[n_tables][2^depth][2][N]*/, int32_t n_tables,
                     const int32_t* table_of /*[count] or NULL*/, int flags, int32_t* out /*[count][width][n+1]*/, ieache_stats* stats);
int ieache_word_read_device(ieache_ctx* ctx, const ieache_tgsw* set, size_t count, int32_t depth, int32_t steps, int32_t width, int32_t unit,
                            const int32_t* d_sel_of, const int32_t* d_tables, int32_t n_tables, const int32_t* d_table_of, int flags, int32_t* d_out,
                            ieache_stats* stats);

/* 3n. Linear layers on encrypted rows: a public int8 matrix times LWE rows.
 *
 * A computation on small encrypted integers alternates two steps: a linear combination of rows with public integer weights,
 * then a table lookup (ieache_pbs).  This is the first step, on rows that stay on the device: scalar multiples and sums of
 * ciphertexts, x p + y ahead of one bivariate table, sums ahead of a single key switch, slot-wise arithmetic on packed samples,
 * a dense layer with a table activation.  Three kinds of rows:
 *
 *     kind                       words    device stride              bias word
 *     IEACHE_ROWS_LWE       0    n + 1    ieache_lwe_stride()        n
 *     IEACHE_ROWS_EXTRACTED 1    N + 1    ieache_extract_stride()    N
 *     IEACHE_ROWS_TLWE      2    2N       2N                         none (bias must be NULL)
 *
 *     out[b][i][w] = ( sum_{j < n_in} W[i][j] x[b][j][w]  +  [w == bias word] bias[i] )  mod 2^32
 *                    for b < batch, i < n_out, w < words
 *
 * x is [batch][n_in] rows and out [batch][n_out] rows; W is int8_t [n_out][n_in], row-major, the full range -128 .. 127; bias
 * is int32 [n_out] (Torus32) or NULL.  Host arrays are packed rows of `words`; device rows use the stride above, and every
 * padding word of an output row is written as zero, as ieache_pbs_multi writes it.  The call reads no key and works on every
 * parameter set a context accepts, N = 2048 included.  All arithmetic is integer mod 2^32: nothing is rounded, guarded or
 * audited, and the two kernels give the same words.  Noise: the output's variance is sum_j W[i][j]^2 times a row's, and an
 * offset common to the rows enters with sum_j W[i][j] (DESIGN.md section 7 gives the margin of a layer).
 * Kernels (context option "linear_kernel": 0 = by n_out, the default; 1; 2 -- any other value is refused):
 *   1  k_linear_simple: a thread per output word, n_in 32-bit multiply-adds; any shape;
 *   2  k_linear_mfma: the same sum as an exact product on the int8 MFMA pipe.  W is copied once per call into the context's
 *      scratch in operand order, zero-padded to tiles of 32; a word v of x is cut in registers into four balanced byte limbs
 *      -- u = (v + 0x80808080) ^ 0x80808080, whose bytes read as signed are b_k in [-128, 127] with v = sum_k b_k 2^(8k) mod 2^32
 *      -- and out = sum_k (W x limb k) << 8k.  A limb's int32 accumulator holds at most n_in x 2^14, which is where
 *      IEACHE_LINEAR_MAX_DIM = 65 536 comes from: 65 536 x 128 x 128 = 2^30 < 2^31.
 * ieache_debug_linear_plan reports what a call would take under the option as it is: out[0] the kernel (1 or 2), out[1] the
 * blocks of 32 words a device row is cut into, out[2] the output tiles of 32 a wave owns (1, 2 or 4), out[3] the K steps of 32
 * inputs (csrc/linear_plan.h; the tiling figures describe the product whichever kernel runs).
 * The device form runs on the context's stream, like every device form; the host form goes through the context's staging rows,
 * so a warm call allocates nothing.  batch == 0 is a no-op.  There is no in-place form.
 * stats: bootstraps == 0, blind_rotate_launches == 0, keyswitch_launches == 0, levels == 1, chunks == 1, total_ms > 0.
 * IEACHE_EINVAL, with the message in ieache_last_error, in this order: (1) an unknown rows kind; (2) n_out or n_in outside
 * 1 .. IEACHE_LINEAR_MAX_DIM; (3) a bias with the TLWE kind -- these three are judged before the context is looked at --;
 * (4) a NULL context, or a NULL W, x or out when batch > 0; (5) device form only: d_out overlapping d_x, d_w or d_bias; then
 * a host pointer to the device form.  A refused call writes nothing.
 * ieache_lwe_linear_reference is the definition on the CPU, on packed rows, without a context (the words come from p).
 * Weights wider than int8 are a second call with shifted weights and one more addition.  There is no group form and no cloudd
 * verb: the call is a small fraction of the bootstrap that follows it, and cutting it over devices is out of scope. */
#define IEACHE_ROWS_LWE 0
#define IEACHE_ROWS_EXTRACTED 1
#define IEACHE_ROWS_TLWE 2
#define IEACHE_LINEAR_MAX_DIM 65536
int ieache_lwe_linear_device(ieache_ctx* ctx, int rows, size_t batch, int32_t n_out, int32_t n_in, const int8_t* d_w /*[n_out][n_in]*/,
                             const int32_t* d_bias /*[n_out] or NULL*/, const int32_t* d_x, int32_t* d_out, ieache_stats* stats);
int ieache_lwe_linear(ieache_ctx* ctx, int rows, size_t batch, int32_t n_out, int32_t n_in, const int8_t* w /*[n_out][n_in]*/,
                      const int32_t* bias /*[n_out] or NULL*/, const int32_t* x /*[batch][n_in][words]*/, int32_t* out /*[batch][n_out][words]*/,
                      ieache_stats* stats);
int ieache_lwe_linear_reference(const ieache_params* p, int rows, size_t batch, int32_t n_out, int32_t n_in, const int8_t* w, const int32_t* bias,
                                const int32_t* x, int32_t* out);
int ieache_debug_linear_plan(const ieache_ctx* ctx, int rows, size_t batch, int32_t n_out, int32_t n_in, int64_t out[4]);

/* ------------------------------------------------------------------ *
 * 4. CPU tools around the path (no GPU): what Keygen/keygen.c:22-51,  *
 *    Client1/alice.c:116-191 and Output/verif.c:41-76 get from        *
 *    libtfhe.  Needed to produce and check ciphertexts without it.    *
 * ------------------------------------------------------------------ */
/* Randomness: a seed / seed-word list gives a REPRODUCIBLE xoshiro256** stream -- for test
 * vectors and for mirroring keygen.c's fixed seeds, not cryptographic (the generator's raw
 * outputs are published as the `a` coefficients).  seed == 0 (encrypt_bits, alice) or
 * n_seed_words < 0 (keygen) draws everything from a ChaCha20 stream keyed by getrandom(2).
 * The fresh metadata encryptions of the process contract always use the latter. */
/* raw key material; any output pointer may be NULL to skip it */
int ieache_keygen_raw(const ieache_params* p, const uint32_t* seed_words, int n_seed_words, int32_t* lwe_key /*[n]*/,
                      int32_t* tlwe_key /*[kN]*/, int32_t* bk, int32_t* ksk);
/* keygen.c equivalent: writes secret.key, cloud.key, nbit.key into `dir`
 * (seeds {314,1592,657} / {314,1592,888} as keygen.c:30,34 when seeds are NULL and the
 * counts are >= 0; a count < 0 = kernel entropy for that key set) */
int ieache_keygen_files(const char* dir, const ieache_params* p, const uint32_t* seed, int n_seed,
                        const uint32_t* nbit_seed, int n_nbit_seed);
/* bootsSymEncrypt / bootsSymDecrypt over arrays of bits; rows of n+1 */
int ieache_encrypt_bits(const ieache_params* p, const int32_t* lwe_key, const uint8_t* bits, size_t count,
                        uint64_t seed, int32_t* out);
int ieache_decrypt_bits(const ieache_params* p, const int32_t* lwe_key, const int32_t* samples, size_t count,
                        uint8_t* bits);
/* TLWE samples under the ring key (k = 1), [2][N] each, A then B, phase B - A s negacyclic mod 2^32: the form of a row of the
 * bootstrapping key, of an encrypted table of ieache_pbs (IEACHE_PBS_TLWE_POLYS) and of a returned accumulator
 * (IEACHE_PBS_ACCUMULATOR).  ieache_tlwe_encrypt draws A uniform and sets B = A s + polys + e, e Gaussian of standard
 * deviation alpha (alpha <= 0: p->tlwe_alpha_min), with the routine key generation uses for the rows of the bootstrapping
 * key; seed as for ieache_encrypt_bits (0: ChaCha20 from kernel entropy).  ieache_tlwe_phase is the exact B - A s.
 * count == 0 is a no-op. */
int ieache_tlwe_encrypt(const ieache_params* p, const int32_t* tlwe_key, const int32_t* polys /*[count][N]*/, size_t count,
                        double alpha, uint64_t seed, int32_t* out /*[count][2][N]*/);
int ieache_tlwe_phase(const ieache_params* p, const int32_t* tlwe_key, const int32_t* samples /*[count][2][N]*/, size_t count,
                      int32_t* phase /*[count][N]*/);
/* The packing key of section 3e, made by whoever holds both secret keys: out [n][pk_t][2][N], every row through the routine
 * ieache_tlwe_encrypt and key generation use, rows (i, j) one after another from one generator (existing keys and their
 * draw order are unchanged).  alpha <= 0: p->tlwe_alpha_min; seed as for ieache_tlwe_encrypt.  IEACHE_EINVAL for a
 * decomposition section 3e does not accept. */
int ieache_packing_keygen(const ieache_params* p, const int32_t* lwe_key, const int32_t* tlwe_key, int32_t pk_t, int32_t pk_basebit,
                          double alpha, uint64_t seed, int32_t* out);
/* CPU reference of the definition of section 3e on raw arrays, no GPU, no context: rows [groups*m][n+1] -> out [groups][2][N].
 * The refusals of the decomposition and of (m, spread, shift) are those of section 3e. */
int ieache_pack_reference(const ieache_params* p, int32_t pk_t, int32_t pk_basebit, const int32_t* pk, size_t groups, int32_t m,
                          int32_t spread, int32_t shift, const int32_t* rows /*[groups*m][n+1]*/, int32_t* out /*[groups][2][N]*/);
/* CPU references of section 3l on raw arrays, no GPU, no context, any supported set: the references of ieache_tlwe_extract and
 * ieache_pack composed, and those of ieache_lut_tree, ieache_tlwe_rotate, the projection and ieache_lut_add composed.
 * pk [N][pk_t][2][N] is the projection key; refusals as in section 3l (the write also names the first bad selector). */
int ieache_tlwe_project_reference(const ieache_params* p, int32_t pk_t, int32_t pk_basebit, const int32_t* pk, size_t count, int32_t first,
                                  int32_t width, int32_t dest, const int32_t* in /*[count][2][N]*/, int32_t* out /*[count][2][N]*/);
extern int ieache_lut_write_coef_reference(const ieache_params* p, const int32_t* set /*[n][2l][2][N]*/, size_t n, int32_t pk_t, int32_t pk_basebit,
                                    const int32_t* pk, size_t count, int32_t depth, int32_t steps, int32_t width, int32_t unit,
                                    const int32_t* sel_of /*[count][steps+depth] or NULL*/, const int32_t* fresh /*[count][2][N]*/,
                                    const int32_t* mem /*[count][2^depth][2][N]*/, int32_t* out /*[count][2^depth][2][N]*/);
/* TGSW samples of section 3f, made by whoever holds the ring key: out [count][2l][2][N], sample i of the int32 message mu[i]
 * (selector bits: 0 or 1), through the routine key generation makes BK_i with -- 2l rows of ieache_tlwe_encrypt's zero
 * encryption one after another from one generator, then the gadget (existing keys and their draw order are unchanged).
 * alpha <= 0: p->tlwe_alpha_min; seed as for ieache_tlwe_encrypt.  Any supported parameter set. */
int ieache_tgsw_encrypt(const ieache_params* p, const int32_t* tlwe_key, const int32_t* mu /*[count]*/, size_t count, double alpha, uint64_t seed,
                        int32_t* out /*[count][2l][2][N]*/);
/* CPU references of the definitions of section 3f on raw arrays, no GPU, no context, any supported parameter set:
 * set [n][2l][2][N]; arguments, defaults of the NULL index arrays and refusals (indices, depth, n_tables) as for the host forms
 * ieache_cmux and ieache_lut_tree. */
int ieache_cmux_reference(const ieache_params* p, const int32_t* set, size_t n, size_t count, const int32_t* sel_of, const int32_t* d1,
                          const int32_t* d0, int32_t* out);
int ieache_lut_tree_reference(const ieache_params* p, const int32_t* set, size_t n, size_t count, int32_t depth, const int32_t* sel_of,
                              const int32_t* tables, int32_t n_tables, const int32_t* table_of, int32_t* out);
/* ... of ieache_lut_scatter (section 3g), arguments and refusals as for its host form; out may be mem itself ... */
int ieache_lut_scatter_reference(const ieache_params* p, const int32_t* set, size_t n, size_t count, int32_t depth, const int32_t* sel_of,
                                 const int32_t* values, const int32_t* mem, int32_t* out);
/* ... of ieache_tlwe_rotate and ieache_lut_read (section 3h), arguments and refusals as for their host forms; out may be `in`
 * itself.  The lookup's key switch is lweKeySwitch with ksk [N][ks_t][2^ks_basebit][n+1] as ieache_keygen_raw gives it; ksk may
 * be NULL under IEACHE_LUT_READ_NO_KEYSWITCH, and out is then [count][N+1] ... */
int ieache_tlwe_rotate_reference(const ieache_params* p, const int32_t* set, size_t n, size_t count, int32_t steps, const int32_t* sel_of,
                                 const int32_t* amount_of, const int32_t* in, int32_t* out);
int ieache_lut_read_reference(const ieache_params* p, const int32_t* set, size_t n, const int32_t* ksk, size_t count, int32_t depth, int32_t steps,
                              const int32_t* sel_of, const int32_t* amount_of, const int32_t* tables, int32_t n_tables, const int32_t* table_of,
                              int32_t coef, int flags, int32_t* out);
/* ... of ieache_lut_add (section 3j): the references of ieache_tlwe_rotate and ieache_lut_scatter composed and the leaves summed
 * per memory; arguments, defaults and refusals as for its host form; out may be mems itself ... */
int ieache_lut_add_reference(const ieache_params* p, const int32_t* set, size_t n, size_t count, int32_t depth, int32_t steps,
                             const int32_t* sel_of, const int32_t* amount_of, const int32_t* values, const int32_t* mems, int32_t n_mems,
                             const int32_t* mem_of, int32_t* out);
/* ... of ieache_automaton_run (section 3k), composed from the CMux reference: set [n][2l][2][N] with p's gadget, tables
 * [steps][states], finals [n_finals][states][2][N] -> out [count][n_out][2][N]; arguments, defaults and refusals (the automaton's
 * and the indices') as for ieache_automaton_create and the host form ... */
int ieache_automaton_reference(const ieache_params* p, const int32_t* set, size_t n, int32_t states, int32_t steps, int32_t n_out,
                               const int32_t* next0, const int32_t* next1, size_t count, const int32_t* sel_of, const int32_t* finals,
                               int32_t n_finals, const int32_t* final_of, int32_t* out);
/* ... and of ieache_tlwe_extract: tlwe [count][2][N] -> u [count][N+1]. */
int ieache_tlwe_extract_reference(const ieache_params* p, size_t count, const int32_t* tlwe, const int32_t* coef_of, int32_t* u);
/* CPU references of section 3m on raw arrays, no GPU, no context: the references of ieache_tlwe_extract and the lookup's
 * lweKeySwitch composed (any supported set), and those of ieache_lut_tree, ieache_tlwe_rotate and the unpacking composed.
 * ksk [N][ks_t][2^ks_basebit][n+1] as ieache_keygen_raw gives it; it may be NULL under IEACHE_UNPACK_NO_KEYSWITCH, and out rows
 * are then N + 1 words.  Refusals as in section 3m (the read also names the first bad selector or table index). */
int ieache_unpack_reference(const ieache_params* p, const int32_t* ksk, size_t count, int32_t first, int32_t width, int32_t spread,
                            const int32_t* in /*[count][2][N]*/, int flags, int32_t* out /*[count][width][n+1]*/);
int ieache_word_read_reference(const ieache_params* p, const int32_t* set /*[n][2l][2][N]*/, size_t n, const int32_t* ksk, size_t count, int32_t depth,
                               int32_t steps, int32_t width, int32_t unit, const int32_t* sel_of, const int32_t* tables, int32_t n_tables,
                               const int32_t* table_of, int flags, int32_t* out /*[count][width][n+1]*/);
/* key files -> raw arrays (sizes from ieache_params; pass NULL to query params only) */
int ieache_read_secret_key(const char* path, ieache_params* p, int32_t* lwe_key, int32_t* tlwe_key);
int ieache_read_cloud_key(const char* path, ieache_params* p, int32_t* bk, int32_t* ksk);
int ieache_write_cloud_key(const char* path, const ieache_params* p, const int32_t* bk, const int32_t* ksk);
int ieache_write_secret_key(const char* path, const ieache_params* p, const int32_t* lwe_key, const int32_t* tlwe_key,
                            const int32_t* bk, const int32_t* ksk);
/* LweSample streams (cloud.data / answer.data): rows of n+1 */
int ieache_read_samples(const char* path, int32_t n, size_t first, size_t count, int32_t* out);
int ieache_write_samples(const char* path, int32_t n, size_t count, const int32_t* rows, int append);
/* alice.c equivalent: one operand -> 352 samples appended to `cloud_data_path`:
 * sign code + bit size under the nbit key, 8 value words + zero carry word
 * under the secret key (alice.c:116-191).  words: 8 x uint32, LSW first. */
int ieache_alice(const char* secret_key_path, const char* nbit_key_path, const char* cloud_data_path, int append,
                 uint32_t sign_code, uint32_t bit_size, const uint32_t* words, uint64_t seed);
/* verif.c decrypt step: answer.data -> sign code, bit size, 8 value words + carry word */
int ieache_verif(const char* secret_key_path, const char* nbit_key_path, const char* answer_data_path,
                 uint32_t* sign_code, uint32_t* bit_size, uint32_t* words9);

/* ------------------------------------------------------------------ *
 * 5. Resident-key daemon.  The reference reloads and     *
 *    re-transforms the cloud key in every ./cloud launch               *
 *    (cloud.c:656-663), i.e. once per operator; its caller             *
 *    (dragonfly_cipher_cloud.py:1233) only needs "run the files in     *
 *    this directory".  ieache_serve keeps the key on the GPU and       *
 *    serves that request over an AF_UNIX stream socket (wire format:   *
 *    csrc/daemon.h); the `cloud` shim forwards to it when              *
 *    IEACHE_DAEMON=<socket path> is set.                               *
 * ------------------------------------------------------------------ */
/* IEACHE_DAEMON_BATCH_WINDOW_MS=T (cloudd --batch-window-ms T; default 0 = one request at a time like the
 * reference): requests arriving within T ms are answered together, and those asking for the same circuit are
 * evaluated as ONE level-batched run -- a lone expression keeps a few of the GPU's 1 024 workgroup slots busy,
 * a hundred concurrent ones fill it.  IEACHE_DAEMON_MAX_BATCH caps a round (default 256). */
/* Blocks.  nbit_key_path may be NULL (= nbit.key next to cloud.key; only
 * RUN_DATA needs it).  max_requests < 0: until a shutdown request or
 * SIGINT/SIGTERM.  Returns the number of requests served or IEACHE_E*. */
int64_t ieache_serve(const char* socket_path, const char* cloud_key_path, const char* nbit_key_path, int device,
                     int64_t max_requests);
/* The same daemon on several GPUs of the node (cloudd --devices 0,1,... or IEACHE_DEVICES=0,1,...): one evaluator per listed
 * device, the cloud key read once and uploaded to each.  A round's same-circuit requests (batch window above) are cut into
 * contiguous slices, one per device -- ieache_shard_slice's rule, the one bench.py and ie-ache_amd/parallel.py apply across
 * ranks (independent expressions, no exchange between GPUs) --, evaluated concurrently and answered in request
 * order; a lone request runs on devices[0].  A device may be listed twice (two contexts on one card).  Answers do not
 * depend on the device list: every expression goes through the same circuit and kernels.  The evaluators are a device group
 * (section 2b): 1 .. IEACHE_GROUP_MAX_DEVICES entries, and contexts that share a card run with "br_mix" = 0.
 * Reference caller served: dragonfly_cipher_cloud.py:1233 (one ./cloud per operator; batches come from concurrent clients). */
int64_t ieache_serve_devices(const char* socket_path, const char* cloud_key_path, const char* nbit_key_path, const int* devices,
                             int n_devices, int64_t max_requests);
/* slice [*first, *first + *count) of `total` independent expressions that part `part` of `parts` takes: contiguous, sizes
 * differing by at most one, the first total % parts parts one longer */
int ieache_shard_slice(size_t total, size_t parts, size_t part, size_t* first, size_t* count);
/* clients: return what main() of cloud.c would (0 / 126) or IEACHE_E*;
 * IEACHE_ENODEV when no daemon listens on socket_path */
int ieache_client_ping(const char* socket_path);
int ieache_client_run_dir(const char* socket_path, const char* workdir);
/* cloud.data bytes + operator code in, answer.data bytes out (caller buffer;
 * *answer_len = bytes needed even when answer_cap is too small -> IEACHE_EINVAL) */
int ieache_client_run_data(const char* socket_path, int operator_code, const void* cloud_data, size_t cloud_data_len,
                           void* answer, size_t answer_cap, size_t* answer_len);
int ieache_client_shutdown(const char* socket_path);

#ifdef __cplusplus
}
#endif
#endif
