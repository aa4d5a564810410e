// Device-side gate-bootstrapping evaluator (HIP, gfx950).
//
// Replaces, for whole levels of independent gates at once, what the reference
// does one gate at a time through libtfhe's bootsAND / bootsXOR ->
// tfhe_bootstrap_FFT (Cloud/cloud.c:30-43,159).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "circuit.h"
#include "params.h"

namespace ieache {

struct OptionRow;  // evaluator_options.h
struct TgswSet;    // cmux.h
struct Automaton;  // cmux.h
struct Cut;        // cmux_plan.h
struct SetCall;    // set_calls.h

struct EvalStats {
    double total_ms = 0;         // wall time of the call on the GPU timeline (events on the stream)
    double blind_rotate_ms = 0;  // time with a blind-rotation launch in flight: the sum over launches on one stream; with
                                 // overlapped levels the union of the two streams' intervals on the device timeline
    double keyswitch_ms = 0;     // the same for key-switch launches (under overlap mostly hidden behind the other stream's rotation)
    int64_t blind_rotate_launches = 0;  // k_blind_rotate_* kernel launches (one per slice of CMux steps per chunk)
    int64_t keyswitch_launches = 0;
    int64_t chunks = 0;  // (level, chunk) work units = key-switch launches
    int64_t bootstraps = 0;  // gate instances bootstrapped
    int64_t levels = 0;
};

// what each staging buffer of an evaluator holds (Evaluator::staging)
enum StageSlot : int {
    kStageA,          // operands a, b, c: rows of lwe_stride() words
    kStageB,
    kStageC,
    kStageOut,        // results
    kStageTestPolys,  // programmable bootstrap: test polynomials [n][N], or TLWE samples [n][2][N]
    kStagePolyOf,     //   ... and the row of that table each item takes
    kStageFactors,    // multi-output programmable bootstrap: factor polynomials [n_factors][N]
    kStageBias,       //   ... and the bias of each factor
    kStageExtracted,  // key switch alone: extracted samples, rows of extract_stride() words (a slot of its own: the operand
                      // slots' padding words stay zero)
    kStageTlweA,      // CMux / extraction: TLWE rows [count][2][N] (d1, or the samples to extract from), and d0
    kStageTlweB,
    kStageSlots
};

// One job of a joint evaluation (Evaluator::eval_jobs_device): a circuit over a batch of its own, rows shaped as
// eval_circuit_device takes them.  The circuit is read during the call only.
struct EvalJob {
    const Circuit* circuit = nullptr;
    size_t batch = 0;
    const Torus32* d_in = nullptr;  // [batch][circuit.n_inputs][lwe_stride]
    Torus32* d_out = nullptr;       // [batch][circuit.outputs.size()][lwe_stride]
};

class Evaluator {
public:
    Evaluator(const Params& p, int device);
    ~Evaluator();
    Evaluator(const Evaluator&) = delete;
    Evaluator& operator=(const Evaluator&) = delete;

    const Params& params() const { return p_; }
    int device() const { return device_; }
    hipStream_t stream() const { return stream_; }
    // gate instances the blind-rotation kernel keeps resident at once (one workgroup each, 4 per CU): a launch
    // takes ceil(gate instances / this) rounds
    int resident_gates() const;
    // ... and by the two-waves-per-gate one-limb kernel that takes launches up to that size (0 when "exact_fft" leaves one size)
    int resident_gates_two_wave() const;
    // Orders everything launched later on the evaluator's stream after the work queued so far on
    // `producer` (the stream that wrote the key / input buffers handed over as device pointers).
    void wait_for_stream(hipStream_t producer);

    // Upload the cloud key.  Raw libtfhe order: bk [n][(k+1)l][k+1][N],
    // ksk [kN][t][base][n+1].  The *_device form takes pointers already in this
    // GPU's memory (e.g. the receive buffer of an RCCL broadcast).
    void load_keys_host(const Torus32* bk, const Torus32* ksk);
    void load_keys_device(const Torus32* d_bk, const Torus32* d_ksk);
    bool keys_loaded() const { return keys_loaded_; }

    // `count` independent gates of one type on device rows of lwe_stride()
    // int32: out[i] = gate(a[i], b[i]).
    void gates_device(int32_t type, size_t count, const Torus32* d_a, const Torus32* d_b,
                      Torus32* d_out, EvalStats* stats);

    // GATE_MAJ3 / GATE_XOR3: out[i] = gate(a[i], b[i], c[i]), one blind rotation and one key switch per gate like any
    // two-input gate
    void gates3_device(int32_t type, size_t count, const Torus32* d_a, const Torus32* d_b, const Torus32* d_c, Torus32* d_out,
                       EvalStats* stats);

    // Programmable bootstrap: out[i] = bootstrap of the row x[i] as it stands from the test polynomial tv[tv_of[i]] (row 0
    // when d_tv_of is null) of d_tv [n_tv][N]: libtfhe's tfhe_blindRotateAndExtract_FFT with testvectbis = X^(2N-barb) * v,
    // then the key switch.  The result encrypts v[phi] for a mod-switched phase phi < N, -v[phi - N] otherwise
    // (include/ieache.h states the convention).  One blind rotation and one key switch per row through the flat path of
    // gates_device: pieces, level halves, rotation of roles, guard and audit.  kPbsNoKeyswitch: the extracted samples are
    // the result (tfhe_bootstrap_woKS_FFT) -- rows of extract_stride() words, N + 1 of them written, no key-switch launch;
    // d_out must then not overlap an input (its rows are longer than x's).  An index outside [0, n_tv) is clamped on the device.
    // kPbsTlwePolys: d_tv is [n_tv][2][N], TLWE samples under the ring key (A then B, phase B - A s), and the accumulator starts
    // from X^(2N-barb) * (A, B): tfhe_blindRotate_FFT on a caller's accumulator.  With A = 0 it is the plain call on B bit for
    // bit.  Everything after the prologue is the same call; the overlap checks use the 2N-word rows.
    // kPbsAccumulator (pbs_device only): row i of d_out is the whole rotated accumulator [2][N], 2N packed words; no
    // extraction and no key switch whether or not kPbsNoKeyswitch is set; the audit compares whole accumulators.  No in-place
    // form: an output over the rows, the table or the indices throws std::invalid_argument.
    // The value 2 names no flag and stays refused.
    static constexpr int32_t kPbsNoKeyswitch = 1;
    static constexpr int32_t kPbsTlwePolys = 4;
    static constexpr int32_t kPbsAccumulator = 8;
    void pbs_device(size_t count, const Torus32* d_x, const Torus32* d_tv, int32_t n_tv, const int32_t* d_tv_of, Torus32* d_out,
                    int32_t flags, EvalStats* stats);
    // words per device row of extracted samples (N + 1 rounded up to a multiple of 4)
    int32_t extract_stride() const { return p_.N + 4; }

    // Multi-output programmable bootstrap: ONE blind rotation per row x[i], exactly pbs_device's, whose whole accumulator
    // (A, B) is kept; then for every factor polynomial P_t of d_factors [n_factors][N] (any int32 values) the extracted
    // sample of coefficient 0 of (P_t A, P_t B), negacyclic and mod 2^32, plus d_bias[t] (null: 0) on its b term, key-switched
    // unless kPbsNoKeyswitch -> row i x n_factors + t of d_out, shaped as pbs_device shapes its rows.  P = 1 is pbs_device
    // bit for bit (include/ieache.h states the convention).  The stage between rotation and key switch is multi_extract.h;
    // a piece of the call is max(1, chunk / n_factors) items, so that its key switch stays within `chunk` rows.  The
    // sampled audit compares the PLAIN extraction of the audited accumulators, which covers the rotation bit for bit; the
    // integer products have nothing to audit.  d_out must not overlap any input (it is n_factors times as long as x): such
    // a call, n_factors outside 1 .. kMultiMaxFactors or a null factor table throw std::invalid_argument.  kPbsTlwePolys as for
    // pbs_device; kPbsAccumulator is refused (the accumulators stay in lane scratch here).
    void pbs_multi_device(size_t count, const Torus32* d_x, const Torus32* d_tv, int32_t n_tv, const int32_t* d_tv_of,
                          const int32_t* d_factors, int32_t n_factors, const Torus32* d_bias, Torus32* d_out, int32_t flags, EvalStats* stats);

    // lweKeySwitch alone: rows d_u [count][extract_stride()] (N + 1 words read, shaped as kPbsNoKeyswitch shapes its output)
    // -> d_out [count][lwe_stride], in pieces of at most `chunk` rows through the key-switch unit's door with a flat
    // descriptor over the caller's rows.  No rotation, so nothing for the guard or the audit to see.  stats: bootstraps 0,
    // one key-switch launch and one chunk per piece, levels 1.  An output over the input throws std::invalid_argument.
    void keyswitch_device(size_t count, const Torus32* d_u, Torus32* d_out, EvalStats* stats);

    // Packing key switch (pack.h; include/ieache.h section 3e states the definition).  set_packing_key: pk [n][t][2][N] on the
    // host; a second key replaces the first, null drops it; std::invalid_argument for a decomposition pack_set_error refuses.
    // pack_device: rows d_rows [groups m][lwe_stride] -> d_out [groups][2][N], in pieces of whole groups (pack_plan.h) on the
    // evaluator's stream, every piece's scratch reserved before the first.  Exact integer arithmetic: no guard, no audit.  stats:
    // bootstraps 0, one key-switch launch and one chunk per piece, levels 1.  std::invalid_argument without a key, for a shape
    // pack_call_error refuses, and for an output over the input.
    void set_packing_key(int32_t t, int32_t basebit, const Torus32* pk);
    bool has_packing_key() const;
    // the plan pack_device would follow for such a call under the options as they are (pack_plan.h): pieces, groups per piece,
    // K split, K steps.  std::invalid_argument without a key.
    void pack_plan_figures(size_t groups, int32_t m, int64_t out[4]) const;
    void pack_device(size_t groups, int32_t m, int32_t spread, int32_t shift, const Torus32* d_rows, Torus32* d_out, EvalStats* stats);

    // The TLWE projection (include/ieache.h section 3l; project_plan.h): the packing unit a second time, on the parameter set
    // with n := N and the projection key pk [N][t][2][N] (host; a second key replaces the first, null drops it and its scratch),
    // independent of the packing key.  tlwe_project_device: d_in [count][2][N] -> d_out [count][2][N], sample i's coefficients
    // first .. first + width - 1 at dest .., nothing else, in pieces of whole items (project_plan) on the evaluator's stream,
    // every piece's scratch reserved before the first; the extracted rows are never stored.  stats as pack_device's.
    // std::invalid_argument without a key, for a window project_call_error refuses, and for ANY overlap of d_out with d_in.
    // project_plan_figures: pieces, items per piece, K split, K steps of such a call under the options as they are
    // ("pack_piece_rows", "project_split").
    void set_projection_key(int32_t t, int32_t basebit, const Torus32* pk);
    bool has_projection_key() const;
    void project_plan_figures(size_t count, int32_t width, int64_t out[4]) const;
    void tlwe_project_device(size_t count, int32_t first, int32_t width, int32_t dest, const Torus32* d_in, Torus32* d_out, EvalStats* stats);

    // CMux on caller TGSW samples, the CMux-tree lookup and the extraction of a coefficient (cmux.h; include/ieache.h section
    // 3f states the definitions).  tgsw_prepare_device: d_samples [n][2l][2][N] -> a set the caller owns (delete it before or
    // after this evaluator goes; only this evaluator accepts it); std::invalid_argument unless br_supported().
    // cmux_device: out[i] = d0[i] + set[sel] [.] (d1[i] - d0[i]), rows [2][N]; d_sel_of null: sample i mod n; d_d0 null: zeros.
    // lut_tree_device: item i folds d_tables[table_of[i]] ([2^depth][2][N]; table_of null: 0) by the selectors
    // sel_of[i depth + k] (null: (i depth + k) mod n), LSB first, level by level on two scratch buffers the evaluator keeps.
    // Both in pieces (cmux_plan.h, "cmux_piece_rows") on the evaluator's stream, a tree's scratch reserved before the first.
    // Indices are read on the device only and clamped there.  Exact on the two-limb spectrum: no guard, no audit.  stats:
    // bootstraps 0, no key-switch launch, one chunk per piece, levels 1 / depth, the CMux launches and their time in the
    // blind-rotation fields.  std::invalid_argument for an output over any input, depth outside 0 .. kCmuxMaxDepth,
    // n_tables < 1 and a set of another evaluator.
    // tlwe_extract_device: coefficient coef_of[i] (null: 0) of d_tlwe [count][2][N] -> d_u [count][extract_stride()], N + 1
    // words written: what keyswitch_device takes.  Any supported parameter set.
    TgswSet* tgsw_prepare_device(const Torus32* d_samples, size_t n);
    // ... with a gadget of the set's own (include/ieache.h section 3i): d_samples [n][2l][2][N] with that l; any context with
    // N = 1024 and k = 1, whatever the key's gadget.  std::invalid_argument naming the rule that failed (gadget_refusal, cmux.h).
    TgswSet* tgsw_prepare_device(const Torus32* d_samples, size_t n, int32_t l, int32_t Bgbit);
    uint64_t cmux_id() const;  // what TgswSet::owner holds for this evaluator's sets
    void cmux_device(const TgswSet& set, size_t count, const int32_t* d_sel_of, const Torus32* d_d1, const Torus32* d_d0, Torus32* d_out,
                     EvalStats* stats);
    void lut_tree_device(const TgswSet& set, size_t count, int32_t depth, const int32_t* d_sel_of, const Torus32* d_tables, int32_t n_tables,
                         const int32_t* d_table_of, Torus32* d_out, EvalStats* stats);
    void tlwe_extract_device(size_t count, const Torus32* d_tlwe, const int32_t* d_coef_of, Torus32* d_u, EvalStats* stats);
    // lut_scatter_device (include/ieache.h section 3g), the tree's partner: item i demultiplexes d_values[i] ([2][N]) by its
    // selectors sel_of[i depth + k] (null: (i depth + k) mod n), most significant first, into 2^depth leaves -- the value at the
    // encrypted index, encryptions of zero elsewhere -- and out[i][j] = mem[i][j] + leaf j (d_mem null: zeros), rows
    // [count][2^depth][2][N].  Pieces, scratch, clamping, stats and refusals as for lut_tree_device (the same plan: cmux_plan.h
    // for (count, depth)), except that d_out == d_mem exactly is accepted: the write is in place.
    void lut_scatter_device(const TgswSet& set, size_t count, int32_t depth, const int32_t* d_sel_of, const Torus32* d_values, const Torus32* d_mem,
                            Torus32* d_out, EvalStats* stats);
    // tlwe_rotate_device (include/ieache.h section 3h): row i goes through acc <- acc + C_t [.] (X^(a_t) acc - acc) for
    // t = 0 .. steps-1, C_t = sample sel_of[i steps + t] (null: (i steps + t) mod n), a_t = d_amount_of[t] masked to 2N - 1
    // (null: 2N - 2^t).  The flat call's pieces, ONE launch per piece with every step inside it, no scratch; d_out == d_in
    // exactly is accepted.  stats: levels = steps, otherwise as cmux_device.  std::invalid_argument for steps outside
    // 0 .. kRotateMaxSteps, any other overlap, a set of another evaluator.
    // lut_read_device: the vertical-packing lookup -- lut_tree_device by selectors steps .. steps+depth-1 of each item's
    // depth + steps, the rotation of the ONE selected row per item by selectors 0 .. steps-1, coefficient `coef` (clamped into
    // [0, N)) extracted and key-switched, all on the evaluator's stream: d_out [count][lwe_stride], or with kLutReadNoKeyswitch
    // the extracted rows [count][extract_stride()].  The tree's plan for (count, depth); the selected rows, the indices and the
    // key switch's scratch are reserved before the first piece.  stats: levels = depth + steps, chunks = pieces, a key-switch
    // launch per run of at most `chunk` rows.
    static constexpr int32_t kLutReadNoKeyswitch = 1;
    // lut_write_device (section 3i), the replace write mem[addr] := new: per item old = the tree over its own memory rows,
    // delta = new - old mod 2^32 on the device, the scatter of delta onto the memory.  d_new [count][2][N], d_mem and d_out
    // [count][2^depth][2][N]; d_out == d_mem writes in place, no other overlap.  Pieces, scratch and stream as the tree's.
    void lut_write_device(const TgswSet& set, size_t count, int32_t depth, const int32_t* d_sel_of, const Torus32* d_new, const Torus32* d_mem,
                          Torus32* d_out, EvalStats* stats = nullptr);
    // lut_add_device (section 3j), the shared write mem[m_i][hi_i].coef[lo_i] += v_i: per item the rotation of d_values[i] by
    // selectors 0 .. steps-1 of its depth + steps (d_amount_of null: +2^t mod 2N), the scatter by selectors steps ..
    // steps+depth-1, and the leaves ADDED into memory d_mem_of[i] (clamped into [0, n_mems); null: 0) by the last demux step
    // itself.  d_mems and d_out [n_mems][2^depth][2][N]; d_out is initialised from d_mems (null: zeros) on the stream unless
    // d_out == d_mems exactly, the write in place; no other overlap.  The tree's plan for (count, depth), reserve_read's scratch.
    // stats: levels = depth + steps, chunks = pieces, launches pieces x ((steps > 0) + max(depth, 1)).
    void lut_add_device(const TgswSet& set, size_t count, int32_t depth, int32_t steps, const int32_t* d_sel_of, const int32_t* d_amount_of,
                        const Torus32* d_values, const Torus32* d_mems, int32_t n_mems, const int32_t* d_mem_of, Torus32* d_out,
                        EvalStats* stats = nullptr);
    // lut_write_coef_device (section 3l), the replace write of a window mem[i][hi_i].coef[lo_i unit .. + width) := new[i].coef[0 ..
    // width): per piece of the tree's plan for (count, depth) the tree over the items' own memories, the rotation toward
    // position 0, the projection onto (0, width, 0) in runs of the projection's plan, delta = new - old, and lut_add_device's
    // piece with memory i for item i and the amounts +unit 2^t.  d_new [count][2][N], d_mem and d_out [count][2^depth][2][N];
    // d_out == d_mem writes in place (a piece reads and adds into its own items' memories only), no other overlap; with
    // distinct buffers d_out starts as a copy of d_mem on the stream.  Everything is reserved before the first piece.  stats:
    // levels = 2 (depth + steps) + 1, chunks = pieces, keyswitch_launches = the projection's runs, blind_rotate_launches =
    // pieces x (2 max(depth, 1) + 2 (steps > 0) + 1).  The eighth row of set_calls.h: std::invalid_argument without a projection
    // key, for scalars write_coef_error refuses, an overlap, a set of another evaluator.
    void lut_write_coef_device(const TgswSet& set, size_t count, int32_t depth, int32_t steps, int32_t width, int32_t unit, const int32_t* d_sel_of,
                               const Torus32* d_new, const Torus32* d_mem, Torus32* d_out, EvalStats* stats = nullptr);
    void tlwe_rotate_device(const TgswSet& set, size_t count, int32_t steps, const int32_t* d_sel_of, const int32_t* d_amount_of, const Torus32* d_in,
                            Torus32* d_out, EvalStats* stats);
    void lut_read_device(const TgswSet& set, size_t count, int32_t depth, int32_t steps, const int32_t* d_sel_of, const int32_t* d_amount_of,
                         const Torus32* d_tables, int32_t n_tables, const int32_t* d_table_of, int32_t coef, int32_t flags, Torus32* d_out,
                         EvalStats* stats);
    // The way back to the gates (include/ieache.h section 3m; unpack_plan.h states the windows and the cut).
    // unpack_device, the partner of pack_device: row (i, q) of d_out = the key switch of the extracted row of coefficient
    // first + q spread of d_in[i] ([count][2][N]), q < width: [count][width] rows of lwe_stride words, or with kUnpackNoKeyswitch
    // the extracted rows themselves, rows of extract_stride() words.  The count x width rows in runs of at most `chunk`, one piece
    // per run, through KeySwitch::launch_window: where a run's plan is the MFMA product no extracted row is stored.  Any
    // parameter set the key switch supports.  stats: bootstraps 0, levels 1, chunks = runs, one key-switch launch per run (none
    // with the flag).  std::invalid_argument for a window or a flag unpack_call_error refuses and for ANY overlap of d_out with d_in.
    // word_read_device, the partner of lut_write_coef_device: per piece of the tree's plan for (count, depth) the tree over
    // d_tables by selectors steps .. steps+depth-1 of each item, the rotation of the selected rows in place by selectors
    // 0 .. steps-1 with the amounts 2N - unit 2^t, and the window (0, width, 1) of those rows unpacked as above in runs of at most
    // `chunk`: d_out [count][width] rows.  Everything is reserved before the first piece.  stats: levels = depth + steps, chunks =
    // pieces, blind_rotate_launches = pieces x (max(depth, 1) + (steps > 0)), a key-switch launch per run.  kWordRead of
    // set_calls.h: std::invalid_argument for scalars word_read_error refuses, an overlap, a set of another evaluator.
    void unpack_device(size_t count, int32_t first, int32_t width, int32_t spread, int32_t flags, const Torus32* d_in, Torus32* d_out, EvalStats* stats);
    void word_read_device(const TgswSet& set, size_t count, int32_t depth, int32_t steps, int32_t width, int32_t unit, const int32_t* d_sel_of,
                          const Torus32* d_tables, int32_t n_tables, const int32_t* d_table_of, int32_t flags, Torus32* d_out, EvalStats* stats);
    // Linear layers on encrypted rows (include/ieache.h section 3n; linear_plan.h states the row kinds, the rules and the choice
    // of kernel).  lwe_linear_device: out[b][i] = sum_j W[i][j] x[b][j] (+ bias[i] on the kind's bias word) mod 2^32 over rows
    // of the kind `rows`: d_x [batch][n_in] and d_out [batch][n_out] rows of the kind's stride, d_w [n_out][n_in] int8, d_bias
    // [n_out] or null; every word of d_out up to the stride is written.  One launch of the unit (lwe_linear.h) on the
    // evaluator's stream ("linear_kernel": 0 by n_out, 1 simple, 2 the MFMA product); needs no key.  Exact integer arithmetic: no
    // guard, no audit.  stats: bootstraps 0, no rotation and no key-switch launch, levels 1, chunks 1, the time in total_ms alone.
    // std::invalid_argument with linear_call_error's words.  linear_plan_figures: kernel (1 simple, 2 MFMA), column blocks,
    // output tiles per wave, K steps of such a call under the option as it is.
    void lwe_linear_device(int32_t rows, size_t batch, int32_t n_out, int32_t n_in, const int8_t* d_w, const int32_t* d_bias, const Torus32* d_x,
                           Torus32* d_out, EvalStats* stats);
    void linear_plan_figures(int32_t rows, int32_t n_out, int32_t n_in, int64_t out[4]) const;
    // Automata over words of TGSW-encrypted bits (include/ieache.h section 3k; automaton_plan.h states what one is and how a
    // call is cut).  automaton_create: the tables [steps][states] from host memory -> an object the caller owns (delete it before
    // or after this evaluator goes; only this evaluator accepts it); std::invalid_argument with the first rule broken.
    // automaton_run_device: item i runs V_t[q] = CMux(C_sel(i,t), V_{t+1}[next1[t][q]], V_{t+1}[next0[t][q]]) for t = steps-1 .. 0
    // from V_steps = d_finals[final_of[i]] ([n_finals][states][2][N]; d_final_of null: 0, clamped) with the selectors
    // sel_of[i steps + t] (null: (i steps + t) mod n; explicit: clamped) -> d_out [count][n_out][2][N] = V_0[0 .. n_out).  Pieces of
    // whole items ("cmux_piece_rows" over 2 states rows each) on the evaluator's stream, every step of a piece in one launch or in
    // chunks ("automaton_steps_per_launch"), the two state buffers reserved before the first piece.  stats: bootstraps 0, no
    // key-switch launch, levels = steps, chunks = pieces, the launches and their time in the blind-rotation fields.
    // std::invalid_argument for an output over any input (there is no in-place form), n_finals < 1, null rows, a set or an
    // automaton of another evaluator.  automaton_plan_figures: pieces, items per piece, scratch rows, steps per launch, launches
    // per piece of such a call under the options as they are.
    Automaton* automaton_create(int32_t states, int32_t steps, int32_t n_out, const int32_t* next0, const int32_t* next1);
    void automaton_run_device(const TgswSet& set, const Automaton& a, size_t count, const int32_t* d_sel_of, const Torus32* d_finals, int32_t n_finals,
                              const int32_t* d_final_of, Torus32* d_out, EvalStats* stats = nullptr);
    void automaton_plan_figures(const Automaton& a, size_t count, int64_t out[5]) const;
    // the plan such a call would follow under the options as they are (cmux_plan.h; depth < 0: a flat call of `count` rows):
    // pieces, items per piece, rows of scratch A, rows of scratch B
    void cmux_plan_figures(size_t count, int32_t depth, int64_t out[4]) const;

    // bootsMUX: out[i] = a[i] ? b[i] : c[i] (two blind rotations + one key switch per gate)
    void mux_device(size_t count, const Torus32* d_a, const Torus32* d_b, const Torus32* d_c, Torus32* d_out,
                    EvalStats* stats);

    // allocates what an evaluation of `c` over `batch` expressions needs (idempotent; eval_circuit_device calls it itself)
    void prepare_circuit(const Circuit& c, size_t batch);
    // One circuit on `batch` independent expressions.
    //   d_in  [batch][circuit.n_inputs][lwe_stride]
    //   d_out [batch][circuit.outputs.size()][lwe_stride]
    void eval_circuit_device(const Circuit& c, size_t batch, const Torus32* d_in, Torus32* d_out,
                             EvalStats* stats);

    // Several circuits' batches TOGETHER, level by level (joint_plan.h): step s runs level s of every job that still has one
    // as ONE call of the level machinery over the concatenation of their rotation items, so that narrow levels of different
    // circuits share every blind-rotation launch -- one prologue and one key switch per job and piece, one sequence of CMux
    // slices over all of them, the kernel chosen by the joint size.  Each job has its own wire store and tables.  Level mode
    // only: no expression pipelines.  A job with batch 0 is skipped; every job's output words are what the job gives alone
    // through eval_circuit_device.  stats: bootstraps summed over jobs, levels = the deepest job's depth, chunks = pieces issued.
    void prepare_jobs(const EvalJob* jobs, size_t n_jobs);
    void eval_jobs_device(const EvalJob* jobs, size_t n_jobs, EvalStats* stats);

    // Device rows the host-buffer entry points stage operands and results in, one buffer per StageSlot: owned by the
    // evaluator, kept between calls and grown on demand, so that a warm call allocates nothing.  Operand slots are zero outside
    // what the caller uploads (rows of lwe_stride() words, n + 1 of them uploaded); of the tables of a programmable bootstrap
    // whole rows are uploaded, and no other call reads them.  get_option("staging_allocations") counts the (re)allocations
    // made so far.
    Torus32* staging(StageSlot slot, size_t bytes);

    // ---- single-stage hooks (parity tests compare each against its oracle stage) ----
    // x [count][lwe_stride] -> acc [count][2][N] after `steps` CMux steps (steps<0: all n),
    // starting from the test-vector initialisation.
    void debug_blind_rotate(size_t count, const Torus32* d_x, Torus32* d_acc, int32_t steps);
    // u [count][N+1] -> out [count][lwe_stride]
    void debug_keyswitch(size_t count, const Torus32* d_u, Torus32* d_out);
    // The transform probe (fft_probe.h; include/ieache.h states the shapes), on HOST arrays: the twiddle table of the blind
    // rotation (which = 0), of the CMux family (1, built now if no set has been) or as a 64-thread kernel builds it (2); `count`
    // transforms in one of the probe's forms; `count` polynomials of a prepared key form from polynomial `first` on (which =
    // 0: two-limb w64, 1: one-limb w64, 2: the any-parameter kernel's).  std::invalid_argument, with nothing written, for a
    // null array, a ring other than N = 1024 / k = 1 (all but the any-parameter form), an unknown `which` or form, an odd
    // count on a paired form, polynomials outside the key.
    void debug_twiddles(int which, double* out);
    void debug_fft512(int form, size_t count, const double* in, double* out);
    void debug_spectrum(int which, size_t first, size_t count, double* out);

    // Force the generic (any-parameter) kernels even where a specialised one exists.
    void set_force_generic(bool v);
    // Maximum gate instances per launch (bounds the scratch buffers).
    void set_chunk(size_t items);
    // Named options and read-only figures: evaluator_options.h holds THE table -- every name, its environment variable,
    // accepted range, default and a line on what it does.  set_option returns false for an unknown name, a read-only
    // figure or a value the row refuses; get_option reads every row, false for an unknown name.  An environment variable is
    // read once, when the context is created, and treated as a set_option: a value out of range is ignored.
    bool set_option(const std::string& name, int64_t value);
    bool get_option(const std::string& name, int64_t* value) const;
    // The stream modes those options steer:
    // "overlap" (default 1; IEACHE_OVERLAP): launches go to TWO streams of the context (own scratch each, the one key copy),
    // so that the ragged end of one stream's launch, its key switch and its prologue run under the other stream's rotation:
    //   * a circuit over a batch whose mean level holds at least "pipe_min" gate instances (default 8 per CU;
    //     IEACHE_PIPE_MIN): the batch is cut into two halves of EXPRESSIONS and each half runs through every level on its own
    //     stream -- expressions are independent, so there is one fork after the input copy and one join before the outputs
    //     are gathered, nothing in between (add16 x 4096: +3.5 %, mul32 x 1024: +1.1 %, profiles/r5_overlap_ab.txt);
    //     kernels are chosen by the gate instances in flight on both streams ("pipe_lanes" = 3 or 4 cuts the batch into
    //     that many pipelines instead: measured no better than two, profiles/r5_overlap_ab.txt);
    //   * otherwise (flat gate calls, narrower circuits) a level of at least "overlap_min" gate instances (default 16 per
    //     CU; IEACHE_OVERLAP_MIN) is cut into pieces of at most half the level that alternate between the two streams, and
    //     the next level starts when both have finished.
    //   * "pipe_auto" (default 1): with a mean level between pipe_min / 8 and 2 x pipe_min neither mode wins everywhere, so the
    //     first four evaluations of a (circuit, batch) alternate without / with pipelines and later ones take the faster
    //     (each is a complete evaluation; "tuned_evals" counts the trials);
    //   * "br_mix" (default 1; IEACHE_BR_MIX): a launch of 4 .. 7 gates per CU -- or of 8 .. 10.5: a full round of the
    //     one-wave kernel plus a small remainder -- that has the chip to itself runs as a ROTATION OF ROLES: the gates in
    //     three subsets on three streams, two subsets at a time on the two-waves-per-gate kernel for "mix_s1" x "mix_ratio"
    //     / 100 steps while the third takes "mix_s1" steps on the one-wave-per-gate kernel ("mix_wg" gates per workgroup),
    //     roles rotating, so that every wave slot of a CU works whatever the launch size: a size-independent 180-185 k
    //     gates/s where the single kernels give 130-180 k (profiles/r5_mix_sweep.txt; csrc/mix_plan.h).
    // The same gate instances go through the same kernels' arithmetic either way: output bits do not depend on it.
    // 0 = every launch on one stream -- the mode per-kernel timings (rocprofv3 averages, bench.py's roofline) are taken
    // in, since overlapped kernels share the chip.
    std::string kernel_variant() const;
    // name of the blind-rotation kernel a launch of `gates` gate instances takes under the current options
    std::string kernel_for_launch(int64_t gates) const;
    // The one-limb blind rotation (k_blind_rotate_w1) rounds sums an FP64 transform carries with ~2^-9 of error instead of
    // provably none; it records how far from an integer its coefficients came.  fft_guard_max(): the largest such distance
    // over the context's life (0.5 would be a wrong bit; the kernel's limit is 1/16); fft_guard_reruns(): calls that crossed
    // the limit and were therefore repeated on the two-limb kernel.  Option "exact_fft" = 1 uses the two-limb kernel always.
    double fft_guard_max() const;
    int64_t fft_guard_reruns() const;
    bool fft_guard_tripped();  // internal: reads and re-arms the device-side record
    // The sampled audit behind the guard (option "fft_audit" = K, default 64, 0 = off; IEACHE_FFT_AUDIT): every K-th launch
    // that took a one-limb kernel has 64 of its gate instances run again on the two-limb kernel and compared word for word;
    // a differing row makes the call repeat itself on the two-limb kernels (counted in fft_guard_reruns()).
    // -> audits run, gate instances compared, rows that differed, over the context's life.
    void fft_audit_counts(int64_t* audits, int64_t* gates, int64_t* mismatches) const;

    struct Impl;      // device buffers; defined in evaluator.hip
    struct FlatCall;  // what a flat call (gates, mux, programmable bootstraps) hands its one body; defined in evaluator.hip
    struct PackSide;  // the packing unit's object, scratch, option and names for one of its two uses; defined in evaluator.hip

private:
    void flat_device_once(const FlatCall& call, EvalStats* stats);  // gates, gates3, mux, pbs and pbs_multi, once
    void eval_circuit_device_once(const Circuit& c, size_t batch, const Torus32* d_in, Torus32* d_out, EvalStats* stats);
    void debug_blind_rotate_once(size_t count, const Torus32* d_x, Torus32* d_acc, int32_t steps);
    void eval_jobs_device_once(const EvalJob* jobs, size_t n_jobs, EvalStats* stats);
    // runs `once`, and again on the two-limb kernels if the rounding guard or the audit asks for it (evaluator.hip)
    template <class F>
    void run_guarded(bool inputs_intact, EvalStats* stats, F&& once);
    // what the calls on caller TGSW samples open with, from the table of set_calls.h -> whether there are items to run (evaluator.hip)
    bool begin_set_call(const TgswSet& set, const SetCall& c, std::initializer_list<const void*> args, size_t out_row_words);
    // the piece loop of every levelled call: body(piece) per piece of the cut (evaluator.hip)
    template <class Body>
    void run_pieces(const Cut& cut, int64_t total, int32_t levels, EvalStats* stats, Body&& body);
    // the packing key switch and the projection: one path over what differs between them (evaluator.hip)
    PackSide packing() const;
    PackSide projection() const;
    void set_pack_key(const PackSide& side, int32_t t, int32_t basebit, const Torus32* pk);
    void pack_side_figures(const PackSide& side, size_t groups, int32_t m, int64_t out[4]) const;
    template <class Launch>
    void pack_side_device(const PackSide& side, const char* shape_error, size_t groups, int32_t m, const Torus32* d_in, size_t in_words, Torus32* d_out,
                          EvalStats* stats, Launch&& launch);
    void init();
    void destroy();
    void begin_call();
    bool option_hook(const OptionRow& row, int64_t& value);
    Params p_;
    int device_;
    hipStream_t stream_ = nullptr;  // lane 0's, owned by Impl
    bool keys_loaded_ = false;
    Impl* d_ = nullptr;
};

// throws std::runtime_error carrying the HIP error string
void hip_check(hipError_t e, const char* what, const char* file, int line);
#define HIP_CHECK(x) ::ieache::hip_check((x), #x, __FILE__, __LINE__)

}  // namespace ieache
