// The one door to the operations on TGSW samples the caller supplies (include/ieache.h):
//   section 3f  the CMux, the CMux-tree lookup built from it, and the extraction of a coefficient of a TLWE sample;
//   section 3g  the scatter that writes at an encrypted index;
//   section 3h  the rotation by caller selectors and the coefficient-level lookup;
//   section 3i  sets with a gadget of their own, and the replace write;
//   section 3j  many values added into shared memories in one call;
//   section 3k  deterministic automata over words of encrypted bits, every step of an item in one launch;
//   section 3l  the two steps of the replace write of a window that are this family's: the read of each item's own memory toward
//               position 0 (launch_read_own) and the subtraction (launch_delta); the projection between them is pack.h's;
//   section 3m  the read of an addressed word up to its rotation toward position 0 (launch_read_rows); the rows' way to the gates
//               is keyswitch.h's.
// The kernels, the spectrum form of a prepared set, the twiddle table and the scratch of a tree are behind this object: a tree
// is ONE level loop (launch_levels) whether its level 0 reads shared tables or each item's own rows, whether its selectors are
// the call's or a piece's explicit ones, and nothing outside fills in a CmuxRows of a tree.  How
// a call is cut is cmux_plan.h; what a call is -- scalars, refusals, arguments -- is set_calls.h.  Kernels: cmux.hip (3f, 3g),
// rotate.hip (3h) and automaton.hip (3k, cut by automaton_plan.h); what they share is cmux_step.h.
#pragma once
#include <cstdint>

#include "automaton_plan.h"
#include "cmux_plan.h"
#include "device_buffer.h"
#include "params.h"

namespace ieache {
namespace dev {
struct LdsGrant;  // device_common.h
}

// A prepared set of n TGSW samples: their two-limb spectrum [n][2l][q = 2 c + limb][8][64] double2 -- the layout of the
// bootstrapping key's spectrum, one sample where that has one BK_i (192 KB at l = 3).  It owns its device memory and nothing of
// the context's, so it may be freed before or after the context that made it is closed; `owner` names that context among all
// the process has had, and only it accepts the set.  The set carries its gadget (l, Bgbit): the context's unless the caller
// prepared it with another (section 3i), and the one everything about the set is sized and dispatched by -- never the key's.
struct TgswSet {
    dev::DeviceBuffer<double2> spectrum;
    size_t n = 0;
    int32_t l = 0, Bgbit = 0;
    uint64_t owner = 0;
    int device = 0;
};

// Where the rows of one launch of k_cmux_x1 live: source and destination bases plus the rule that maps row r to (d1 row, d0 row,
// selector) -- no pointer tables.
//   flat (depth < 0):       d1 = src + r, d0 = src0 + r (src0 null: zeros), out = dst + r, selector sel_of[r] (null: item0 + r)
//   tree level k, width w:  item = r / w, pair = r % w; block = item, or at level 0 (shared) table_of[item0 + item] clamped (null: 0);
//                           d0 = src + block 2 w + 2 pair, d1 = d0 + 1, out = dst + r, selector sel_of[(item0 + item) depth + k]
//                           (null: (item0 + item) depth + k)
// An explicit selector is clamped into [0, n_set), an implied one taken mod n_set: a bad index reads another sample, never
// memory outside the set.  Rows are [2][1024] words.
struct CmuxRows {
    const int32_t* src = nullptr;
    const int32_t* src0 = nullptr;
    int32_t* dst = nullptr;
    const int32_t* sel_of = nullptr;
    const int32_t* table_of = nullptr;  // read only when `shared`; indexed by call item, like the tree's selectors
    int64_t rows = 0;
    int64_t item0 = 0;                  // first row / item of the piece within the call (a flat piece's src, dst and sel_of are already offset)
    int32_t n_set = 1, n_tables = 1;
    int32_t depth = -1, level = 0, width = 1;
    int32_t shared = 0;
};

// Where the rows of one launch of k_demux_x1 live (step t of a scatter, include/ieache.h section 3g): parent row r of the
// piece splits into two children -- again a rule, no pointer tables, everything wave-uniform.
//   width w = 2^t parents per item:  item = r / w, j = r % w;  parent = src + item w + j = src + r,
//   children = dst + item 2 w + 2 j = dst + 2 r (lo = parent - hi) and the row after it (hi = C [.] parent),
//   selector sel_of[(item0 + item) depth + depth - 1 - t] (null: that index mod n_set; explicit: clamped into the set).
//   On the last step (2 w = 2^depth) `base` is null (zeros) or the piece's memory rows: child c is stored as base[2 r + c] + child.
// base == dst is allowed (k_demux_x1 says why); no other overlap is.
struct DemuxRows {
    const int32_t* src = nullptr;
    int32_t* dst = nullptr;
    const int32_t* base = nullptr;
    const int32_t* sel_of = nullptr;
    int64_t rows = 0;                   // parents of this launch: items x w
    int64_t item0 = 0;                  // first item of the piece within the call (src, dst and base are already offset)
    int32_t n_set = 1;
    int32_t depth = 1, step = 0, width = 1;
};

// Where the rows of one launch of k_demux_acc live: the LAST step of a piece of lut_add (include/ieache.h section 3j), DemuxRows'
// sibling.  The parents are a piece's as above; the children are not stored per item but ADDED into the memory the item names:
//   width w = 2^(depth-1):  item = r / w, j = r % w;  parent = src + r;  m = mem_of[item] clamped into [0, n_mems) (null: 0);
//   child c of the parent is added into out + (m 2^depth + 2 j + c), 2 j + c < 2^depth: a row of memory m whatever mem_of holds;
//   selector sel_of[item depth + depth - 1 - step] with DemuxRows' rule.
// sel_of and mem_of are the PIECE's (already offset by its first item): the selectors are the explicit ones k_read_indices
// wrote, which the earlier steps of the piece read through DemuxRows with item0 = 0.  `out` is the call's, the same for every
// piece.  Nothing of out is read: any number of rows of any number of pieces may name one memory row.
struct DemuxAccRows {
    const int32_t* src = nullptr;
    int32_t* out = nullptr;
    const int32_t* sel_of = nullptr;
    const int32_t* mem_of = nullptr;
    int64_t rows = 0;                   // parents of this launch: items x w
    int32_t n_set = 1, n_mems = 1;
    int32_t depth = 1, step = 0, width = 1;
};

// Where the rows of one launch of k_rotate_x1 live (include/ieache.h section 3h): row r of the piece is rotated by its
// selectors in `steps` steps inside the launch -- a rule again, everything wave-uniform.
//   in = src + r, out = dst + r (dst == src is allowed: k_rotate_x1 says why);
//   selector of step t: sel_of[(item0 + r) sel_stride + t] (null: that index mod n_set; explicit: clamped into the set);
//   amount of step t: amount_of[t] masked to 2N - 1 (null: 2N - 2^t, which is 0 from t = 11 on).
// sel_stride is `steps` for a rotation of its own and depth + steps inside a coefficient-level lookup.
struct RotateRows {
    const int32_t* src = nullptr;
    int32_t* dst = nullptr;
    const int32_t* sel_of = nullptr;
    const int32_t* amount_of = nullptr;
    int64_t rows = 0;
    int64_t item0 = 0;                  // first row of the piece within the call (src and dst are already offset)
    int32_t n_set = 1;
    int32_t steps = 0, sel_stride = 0;  // steps in 0 .. kRotateMaxSteps
};

// A compiled automaton (include/ieache.h section 3k; automaton_plan.h states what one is): the public transition tables
// next [2][steps][states] (next0 first) and the live masks [steps] on the device.  Like a TgswSet it owns its device memory and
// nothing of the context's, may be freed before or after the context, and only the context named by `owner` accepts it.
struct Automaton {
    dev::DeviceBuffer<int32_t> next;
    dev::DeviceBuffer<uint64_t> live;
    int32_t states = 0, steps = 0, n_out = 0;
    int64_t cmuxes = 0;  // live CMuxes per item (automaton_live)
    uint64_t owner = 0;
    int device = 0;
};

// Where the rows of one launch of k_automaton_x1 live: workgroup b owns item b of the piece and runs steps t = hi-1 .. lo of it
// -- a rule again, no pointer tables, everything wave-uniform.
//   V_t, 0 < t < steps: scratch + (b 2 states + (t & 1) states) rows; V_steps: finals + fo states rows, fo = final_of[item0 + b]
//   clamped into [0, n_finals) (null: 0); V_0: out + b n_out rows, states 0 .. n_out-1 only.
//   State q of step t (bit q of live[t] set): d0 = V_{t+1}[next0[t][q]], d1 = V_{t+1}[next1[t][q]] -> V_t[q]; the two equal: a copy.
//   Selector of step t: sel_of[(item0 + b) steps + t] (null: that index mod n_set; explicit: clamped into the set).
// out and scratch are the PIECE's (already offset); sel_of and final_of are the call's.  `rows` counts WAVES, items x
// kCmuxWaveRows, so that the family's launcher makes one workgroup per item.
struct AutomatonRows {
    const int32_t* finals = nullptr;
    int32_t* out = nullptr;
    int32_t* scratch = nullptr;
    const int32_t* sel_of = nullptr;
    const int32_t* final_of = nullptr;
    const int32_t* next0 = nullptr;
    const int32_t* next1 = nullptr;
    const uint64_t* live = nullptr;
    int64_t rows = 0;
    int64_t item0 = 0;
    int32_t n_set = 1, n_finals = 1;
    int32_t states = 1, steps = 0, n_out = 1;
    int32_t hi = 0, lo = 0;
};

// Scratch of a tree on one stream: the two buffers whose roles swap from level to level.  A coefficient-level lookup
// (lut_read) adds the rows its trees select, which the rotation turns in place, and the indices its launches read: the tree's
// selectors [items][depth] taken out of the call's [count][depth + steps], then the public coefficient once per item.
struct CmuxScratch {
    dev::DeviceBuffer<int32_t> a, b;
    dev::DeviceBuffer<int32_t> rows, idx;
};

// One per evaluator.  All methods expect the evaluator's device to be current.
// What ieache_tgsw_prepare_gadget accepts on a context with parameters p: null, or the rule that failed.  HIP-free.
inline const char* gadget_refusal(const Params& p, int32_t l, int32_t Bgbit) {
    if (p.N != 1024 || p.k != 1) return "tgsw_prepare_gadget: the CMux kernels cover N = 1024, k = 1 only";
    if (l < 1) return "tgsw_prepare_gadget: l must be at least 1";
    if (Bgbit < 1 || Bgbit >= 32) return "tgsw_prepare_gadget: Bgbit must lie in 1 .. 31";
    if ((int64_t)l * Bgbit > 32) return "tgsw_prepare_gadget: l x Bgbit must not exceed 32";
    if (((int64_t)2 * l * p.N << Bgbit) > ((int64_t)1 << 32))
        return "tgsw_prepare_gadget: 2 l N 2^Bgbit must not exceed 2^32 (the exactness bound of the two-limb product, Params::br_exact)";
    return nullptr;
}

struct Cmux {
    // runtime_always: where the debug option "cmux_gadget_runtime" lives (null: never) -- non-zero sends every set to the
    // run-time-gadget builds of the kernels, libtfhe's two gadgets included
    void init(const Params& p, int device, const int64_t* runtime_always = nullptr);
    uint64_t id() const { return id_; }
    // d_samples [n][2l][2][N] int32 on the device -> a new set (the caller owns it).  Synchronises the stream.  Throws
    // std::invalid_argument where the parameter set is not one of the 64-lane kernels' (br_supported(), br_plan.h) or n < 1.
    TgswSet* prepare(const int32_t* d_samples, size_t n, hipStream_t stream);
    // the same with a gadget of the set's own, d_samples [n][2l][2][N] with that l, on any context with N = 1024 and k = 1
    // whatever the key's gadget.  std::invalid_argument naming the rule of gadget_refusal() that failed.
    TgswSet* prepare(const int32_t* d_samples, size_t n, int32_t l, int32_t Bgbit, hipStream_t stream);
    // std::invalid_argument unless `set` was prepared by this object
    void check_owner(const TgswSet& set) const;
    // scratch for every piece of a tree's plan ahead of the loop, so that no piece allocates
    void reserve(CmuxScratch& scratch, const CmuxPlan& pl);
    // one launch of `rows.rows` CMuxes
    void launch(const TgswSet& set, hipStream_t stream, CmuxRows rows);
    // one piece of a tree: `items` items from call item `item0` on, tables [n_tables][2^depth][2][N] -> out [items][2][N];
    // returns the kernel launches issued (depth, or 1 for the copy of depth 0)
    int launch_tree(const TgswSet& set, CmuxScratch& scratch, hipStream_t stream, int64_t item0, int64_t items, int32_t depth,
                    const int32_t* sel_of, const int32_t* tables, int32_t n_tables, const int32_t* table_of, int32_t* out);
    // one launch of `rows.rows` demux steps (2 x rows.rows rows written)
    void launch_demux(const TgswSet& set, hipStream_t stream, DemuxRows rows);
    // one piece of a scatter: `items` items from call item `item0` on, values [items][2][N] (+ mem [items][2^depth][2][N], or
    // null: zeros) -> out [items][2^depth][2][N]; out == mem is allowed.  Step t < depth - 1 writes the scratch buffer that
    // (depth - 2 - t) names: even A, odd B, so the widest intermediate (items x 2^(depth-1) rows) lands in A and the sizes are
    // the tree's (cmux_plan.h).  Returns the kernel launches issued (depth, or 1 for the add of depth 0).
    int launch_scatter(const TgswSet& set, CmuxScratch& scratch, hipStream_t stream, int64_t item0, int64_t items, int32_t depth,
                       const int32_t* sel_of, const int32_t* values, const int32_t* mem, int32_t* out);
    // one piece of a replace write (section 3i): old_i = the tree of item i's own memory rows by its selectors, delta_i = fresh_i
    // - old_i mod 2^32 (k_write_delta, over scratch.rows), the scatter of delta onto the memory -> out; out == mem is allowed: a
    // piece reads and writes its own items' rows only, the tree (launch_own_tree) has finished reading them when the scatter's last step -- the
    // only launch that writes them -- starts (one stream), and that step is in place by k_demux_x1's argument.  scratch as
    // reserve_read's.  Returns the kernel launches issued.
    int launch_write(const TgswSet& set, CmuxScratch& scratch, hipStream_t stream, int64_t item0, int64_t items, int32_t depth, const int32_t* sel_of,
                     const int32_t* fresh, const int32_t* mem, int32_t* out);
    // one launch of `rows.rows` rotations, all `rows.steps` steps of a row inside it (rotate.hip); no scratch
    void launch_rotate(const TgswSet& set, hipStream_t stream, RotateRows rows);
    // a coefficient-level lookup (lut_read): besides the tree's buffers, the selected rows and the indices of the largest piece
    void reserve_read(CmuxScratch& scratch, const CmuxPlan& pl, int32_t depth);
    // one piece of a lookup up to the extraction: the tree by selectors steps .. steps + depth - 1 of each item into
    // scratch.rows, the rotation of those rows in place by selectors 0 .. steps - 1, coefficient `coef` (clamped into [0, N))
    // of each as an extracted row u [items][stride].  Returns the kernel launches issued.
    int launch_read(const TgswSet& set, CmuxScratch& scratch, hipStream_t stream, int64_t item0, int64_t items, int32_t depth, int32_t steps,
                    const int32_t* sel_of, const int32_t* amount_of, const int32_t* tables, int32_t n_tables, const int32_t* table_of, int32_t coef,
                    int32_t* u, int32_t stride);
    // one piece of the read of a replace write of a window (section 3l), launch_read's sibling: selectors steps .. steps + depth - 1
    // of each item made explicit in scratch.idx (k_read_indices; not counted as a launch), the tree of each item's OWN memory rows
    // mem [items][2^depth][2][N] (the piece's, already offset) by them into scratch.rows, the rotation of those rows in place by
    // selectors 0 .. steps - 1 and amount_of.  sel_of is the call's.  scratch as reserve_read's.  Returns max(depth, 1) + (steps > 0).
    int launch_read_own(const TgswSet& set, CmuxScratch& scratch, hipStream_t stream, int64_t item0, int64_t items, int32_t depth, int32_t steps,
                        const int32_t* sel_of, const int32_t* amount_of, const int32_t* mem);
    // one piece of the read of an addressed word (section 3m), launch_read up to the rotation and with launch_read_own's count:
    // selectors steps .. steps + depth - 1 of each item made explicit in scratch.idx (not counted as a launch), the tree over the
    // shared tables [n_tables][2^depth][2][N] by them into scratch.rows, the rotation of those rows in place by selectors
    // 0 .. steps - 1 and amount_of.  sel_of and table_of are the call's.  scratch as reserve_read's.  Returns max(depth, 1) + (steps > 0).
    int launch_read_rows(const TgswSet& set, CmuxScratch& scratch, hipStream_t stream, int64_t item0, int64_t items, int32_t depth, int32_t steps,
                         const int32_t* sel_of, const int32_t* amount_of, const int32_t* tables, int32_t n_tables, const int32_t* table_of);
    // delta_i = fresh_i - old_i mod 2^32 in place over old [items][2][N] (k_write_delta): one launch
    void launch_delta(hipStream_t stream, int64_t items, const int32_t* fresh, int32_t* old_to_delta);
    // one launch of `rows.rows` accumulating demux steps (k_demux_acc: 2 x rows.rows rows added into rows.out)
    void launch_demux_acc(const TgswSet& set, hipStream_t stream, DemuxAccRows rows);
    // the scatter of one piece of lut_add (section 3j): `items` parents src [items][2][N] by the piece's explicit selectors
    // tree_sel [items][depth]; steps 0 .. depth - 2 are launch_scatter's (k_demux_x1, the same scratch buffers), the last is
    // k_demux_acc into out [n_mems][2^depth][2][N] by mem_of (the piece's, null: memory 0); depth 0 adds the parents themselves
    // (k_demux_acc0).  Returns the kernel launches issued (max(depth, 1)).
    int launch_scatter_acc(const TgswSet& set, CmuxScratch& scratch, hipStream_t stream, int64_t items, int32_t depth, const int32_t* tree_sel,
                           const int32_t* src, const int32_t* mem_of, int32_t n_mems, int32_t* out);
    // one piece of lut_add: the rotation of values [items][2][N] into scratch.rows by selectors 0 .. steps - 1 of each item's
    // depth + steps (amount_of null: +2^t mod 2N, the amounts that move coefficient 0 to the encrypted position; steps == 0: the
    // values are the parents), the selectors steps .. steps + depth - 1 made explicit in scratch.idx (k_read_indices; not
    // counted as a launch), launch_scatter_acc.  `values` is the PIECE's (already offset by item0); sel_of, mem_of and out are
    // the call's.  scratch as reserve_read's.  Returns (steps > 0) + max(depth, 1).
    int launch_add(const TgswSet& set, CmuxScratch& scratch, hipStream_t stream, int64_t item0, int64_t items, int32_t depth, int32_t steps,
                   const int32_t* sel_of, const int32_t* amount_of, const int32_t* values, int32_t n_mems, const int32_t* mem_of, int32_t* out);
    // ---- automata (section 3k; automaton.hip) ----
    // the tables [steps][states] from host memory -> a new automaton (the caller owns it).  std::invalid_argument with
    // automaton_refusal()'s message, or where the context's ring is not N = 1024, k = 1.
    Automaton* automaton_create(int32_t states, int32_t steps, int32_t n_out, const int32_t* next0, const int32_t* next1);
    void check_owner(const Automaton& a) const;
    // the two state buffers of the largest piece, in scratch.a
    void reserve_automaton(CmuxScratch& scratch, const AutomatonPlan& pl);
    // one piece: `items` items from call item `item0` on through every launch of the plan; out is the piece's
    // [items][n_out][2][N], sel_of, final_of and finals the call's.  Returns the kernel launches issued (pl.launches).
    int launch_automaton(const TgswSet& set, const Automaton& a, CmuxScratch& scratch, hipStream_t stream, const AutomatonPlan& pl, int64_t item0,
                         int64_t items, const int32_t* sel_of, const int32_t* finals, int32_t n_finals, const int32_t* final_of, int32_t* out);
    // coefficient coef_of[i] (null: 0; clamped into [0, N)) of tlwe [count][2][N] -> u [count][stride], N + 1 words written.
    // Any supported parameter set.
    void launch_extract(hipStream_t stream, int64_t count, const int32_t* tlwe, const int32_t* coef_of, int32_t* u, int32_t stride);
    // The family's twiddle table, built on `stream` if no set has been prepared yet -- the one step of prepare() that makes it.
    // For the transform probe's read-back (Evaluator::debug_twiddles).
    const double2* twiddles(hipStream_t stream);

private:
    // The one launcher of the one-wave kernels (k_cmux_x1, k_demux_x1, k_rotate_x1), defined in cmux_step.h: the owner check,
    // nothing for no rows, n_set filled in, kCmuxWaveRows rows per workgroup, kernel_of(parameter set) launched with `lds`
    // bytes of dynamic LDS -- which `grant`[build], where given, allows first, once per device, under the build's own name
    // (`name`: the two fixed builds, `name_rt`: the run-time-gadget build).
    template <class Rows, class KernelOf>
    void launch_rows(const TgswSet& set, hipStream_t stream, Rows rows, KernelOf kernel_of, size_t lds = 0, dev::LdsGrant* grant = nullptr,
                     const char* name = nullptr, const char* name_rt = nullptr);
    // THE level loop of a tree of depth >= 1 over one piece: level k is one launch of items x 2^(depth-1-k) CMuxes; level 0
    // reads `src` -- shared: tables [n_tables][2^depth] picked by table_of, otherwise each item's own 2^depth rows -- the last
    // level writes `out`, the levels between the scratch buffers (scratch_rows).  sel_of with item0: the call's array and the
    // piece's first item, or a piece's explicit array and 0.  `refusal`: what a scratch too small throws.  Returns depth.
    int launch_levels(const TgswSet& set, CmuxScratch& scratch, hipStream_t stream, int64_t item0, int64_t items, int32_t depth, const int32_t* sel_of,
                      const int32_t* src, bool shared, int32_t n_tables, const int32_t* table_of, int32_t* out, const char* refusal);
    // item i looks up its own memory: launch_levels unshared over mem [items][2^depth][2][N] -> out [items][2][N]; depth 0: the
    // rows copied (counted as one launch)
    int launch_own_tree(const TgswSet& set, CmuxScratch& scratch, hipStream_t stream, int64_t item0, int64_t items, int32_t depth, const int32_t* sel_of,
                        const int32_t* mem, int32_t* out, const char* refusal);
    // the rows a lookup selected (scratch.rows) rotated in place by selectors 0 .. steps - 1 of each item's depth + steps;
    // returns the launches (steps > 0)
    int launch_rotate_selected(const TgswSet& set, CmuxScratch& scratch, hipStream_t stream, int64_t item0, int64_t items, int32_t depth, int32_t steps,
                               const int32_t* sel_of, const int32_t* amount_of);
    Params p_;
    const int64_t* runtime_always_ = nullptr;
    int device_ = 0;
    uint64_t id_ = 0;
    dev::DeviceBuffer<double2> tw_;  // the 64-lane transforms' twiddle table, built with the first set
    dev::DeviceBuffer<int32_t> add_amounts_;  // lut_add's default amounts [kRotateMaxSteps]: +2^t mod 2N, made by the first call that needs them
};

}  // namespace ieache
