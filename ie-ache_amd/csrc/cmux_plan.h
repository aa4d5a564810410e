// The CMux on caller TGSW samples and the CMux-tree lookup (cmux.hip; include/ieache.h section 3f): how a call is cut into
// pieces: THE statement of it (the evaluator loops by the answer and cmux.hip sizes its scratch by it; nothing else decides).
// Free of HIP so that the CPU tests can check it (tests/native/cmux_plan_test.cpp).
//
//   k_cmux_x1        one CMux per wave: out = d0 + C_sel [.] (d1 - d0) on the two-limb spectrum
//   k_cmux_copy      a tree of depth 0: out_i = tables[table_of[i]][0]
//   k_tlwe_extract   coefficient j of a TLWE sample as an extracted LWE row
//   k_demux_x1       one demux step per wave (section 3g): parent p -> hi = C_sel [.] p and lo = p - hi, the memory added on the last step
//   k_demux_add      a scatter of depth 0: out_i = mem_i + v_i
//   k_demux_acc      (section 3j) the last demux step of a piece of lut_add: the children ADDED into the memory the item names
//   k_demux_acc0     lut_add at depth 0: out[mem_of[i]][0] += v_i
//   k_rotate_x1      (rotate.hip, section 3h) one row per wave, every step inside the launch: acc += C_t [.] (X^a_t acc - acc)
//   k_read_indices   (rotate.hip) a lookup's tree selectors and its public coefficient as the arrays the two kernels above read
//
// A tree call over `items` items of depth d runs level k = 0 .. d-1 as ONE launch of items x 2^(d-1-k) CMuxes.  Level 0 reads
// the caller's tables and the last level writes the caller's output; the levels between go through two scratch buffers that
// swap roles: A holds the output of levels 0, 2, 4 .., B of levels 1, 3, ...  A piece is a run of WHOLE items whose level-0
// output stays within the cap, so A is items x 2^(d-1) rows and B half of that; a single item wider than the cap (d = 12 at a
// cap below 2 048) is a piece of its own.  A flat call has no scratch; the same cap bounds the rows of one launch.
// A scatter (lut_scatter) over `items` items of depth d is the same plan run the other way: step t = 0 .. d-1 is one launch of
// items x 2^t parents writing items x 2^(t+1) rows; step d-1 writes the caller's output, step d-2 (items x 2^(d-1) rows) A,
// step d-3 B, and so on backwards -- the tree's sizes, so cmux_plan(items, d, ...) is its cut unchanged.
// A rotation (tlwe_rotate) is a flat call: rows = items, one launch per piece whatever the number of steps, no scratch.  A
// coefficient-level lookup (lut_read) is cut as its tree is, cmux_plan(items, d, ...), and keeps one selected row per item.
// The shared write (lut_add) is cut as a scatter of its depth is, cmux_plan(items, d, ...), with lut_read's scratch: the
// rotated row per item; its last step adds into the caller's memories, so which piece an item falls into does not matter.
#pragma once
#include <cstddef>
#include <cstdint>

namespace ieache {

constexpr int32_t kCmuxMaxDepth = 12;       // IEACHE_LUT_TREE_MAX_DEPTH: a table of 4 096 samples (32 MB at N = 1024) per item
constexpr int32_t kCmuxWaveRows = 4;        // rows (= waves) per workgroup of k_cmux_x1
constexpr int32_t kRotateMaxSteps = 64;     // IEACHE_ROTATE_MAX_STEPS: what one lane-held vector of amounts and selectors covers
// Rows of a piece at most: 8 192 rows of [2][1024] int32 are 64 MB of scratch A and 32 MB of B, which a depth-10 tree over 16
// items or a depth-12 tree over 4 fills; a launch of 8 192 waves is 4 rounds of the 2 048 resident on 256 CUs, so the ragged
// end of a piece costs little.
constexpr int64_t kCmuxPieceRows = 8192;
constexpr int64_t kCmuxPieceRowsMax = (int64_t)1 << 20;

// THE cut of a levelled call -- of a tree's items, a packing call's groups (pack_plan.h), an automaton's items
// (automaton_plan.h), the rows of a key switch: `pieces` runs of `per_piece`, the last perhaps shorter.  Piece i of a call over
// `total` holds [piece_first, piece_first + piece_count); the evaluator's piece loop walks a cut and knows no plan.
struct Cut {
    int64_t pieces = 0, per_piece = 0;
};
inline int64_t piece_first(const Cut& c, int64_t i) { return i * c.per_piece; }
inline int64_t piece_count(const Cut& c, int64_t total, int64_t i) {
    const int64_t left = total - piece_first(c, i);
    return left < c.per_piece ? left : c.per_piece;
}
// `total` in runs of at most `run` (nothing, or no run length: no pieces)
inline Cut cut_in_runs(int64_t total, int64_t run) { return total <= 0 || run <= 0 ? Cut{} : Cut{(total + run - 1) / run, run}; }

struct CmuxPlan {
    int64_t items_per_piece = 0, pieces = 0;
    int64_t level0_rows = 0;   // rows the first level of the largest piece (the first) writes: items_per_piece x 2^(depth-1); flat: its rows
    int64_t a_rows = 0, b_rows = 0;  // scratch rows of [2][N] words: A (depth >= 2), B (depth >= 3)
    Cut cut() const { return {pieces, items_per_piece}; }
};

// A call of `items` items: depth < 0 names a flat call (rows = items), 0 .. kCmuxMaxDepth a tree.  piece_rows_opt:
// "cmux_piece_rows" (anything outside 1 .. kCmuxPieceRowsMax: the default).
inline CmuxPlan cmux_plan(int64_t items, int32_t depth, int64_t piece_rows_opt) {
    CmuxPlan pl;
    if (items <= 0 || depth > kCmuxMaxDepth) return pl;
    if (piece_rows_opt < 1 || piece_rows_opt > kCmuxPieceRowsMax) piece_rows_opt = kCmuxPieceRows;
    const int64_t per_item = depth < 1 ? 1 : (int64_t)1 << (depth - 1);  // level-0 output rows of one item (a copy: one)
    pl.items_per_piece = piece_rows_opt / per_item < 1 ? 1 : piece_rows_opt / per_item;
    if (pl.items_per_piece > items) pl.items_per_piece = items;
    pl.pieces = (items + pl.items_per_piece - 1) / pl.items_per_piece;
    pl.level0_rows = pl.items_per_piece * per_item;
    pl.a_rows = depth >= 2 ? pl.level0_rows : 0;
    pl.b_rows = depth >= 3 ? pl.level0_rows / 2 : 0;
    return pl;
}

}  // namespace ieache
