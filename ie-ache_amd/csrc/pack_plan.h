// The packing key switch (LWE rows -> one TLWE sample, pack_keyswitch.hip): which decompositions it accepts, and how a call is
// cut -- pieces of whole groups, row blocks, K steps and their split: THE statement of it (pack_keyswitch.hip launches by the
// answer and sizes its scratch by it; nothing else decides).  Free of HIP so that the CPU tests can check it
// (tests/native/pack_plan_test.cpp).
//
//   k_pack_prepare   once per key: PK [n t][2N] int32 -> B fragments of balanced byte limbs in MFMA operand order
//   k_pack_digits    per piece: the rows' digits as int8 values 0 .. 2^b - 1, [K step][row][32]
//   k_pack_init      per piece: R rows start as (0, b X^0)
//   k_pack_gemm      per piece: R -= digits x key, a wave per (row block, 32 columns, K split) on the int8 MFMA
//   k_pack_place     per piece: out_g = rotate-and-sum of its group's R rows
#pragma once
#include <cstddef>
#include <cstdint>

#include "cmux_plan.h"
#include "params.h"

namespace ieache {

constexpr int32_t kPackKStep = 32;         // k values (i, j) per MFMA step
constexpr int32_t kPackTileRows = 32;      // rows per MFMA tile
constexpr int32_t kPackWaveTiles = 4;      // row tiles a wave of k_pack_gemm owns (16 accumulator tiles with the four limbs)
constexpr int32_t kPackBlockRows = kPackTileRows * kPackWaveTiles;  // a piece's rows are padded to whole blocks with zero digits
constexpr int32_t kPackMaxSplit = 8;       // K splits: 1, 2, 4, 8, none longer than the walk
constexpr int64_t kPackPieceRows = 4096;   // rows of a piece at most (a single group may hold N <= 1024): R = 8 KB x 4096 = 32 MB at N = 1024

// Why a decomposition (t, b) is refused for the parameter set, or null: b in 1 .. 4, t >= 1, t b < 32 (the bound of the LWE
// key switch), and n t (2^b - 1) 128 < 2^31, so that the int32 accumulator of one byte-limb column cannot overflow.
inline const char* pack_set_error(const Params& p, int32_t t, int32_t b) {
    if (!p.supported()) return "packing key: unsupported TFHE parameter set";
    // pieces, R rows and the placement are stated and measured for groups of up to 1 024 rows; an N = 2048 context blind-rotates
    // and key-switches, and refuses this key (and with it the projection key and unpack, which are this unit on n := N)
    if (p.N > 1024) return "packing key: the packing key switch covers rings up to N = 1024";
    if (b < 1 || b > 4) return "packing key: pk_basebit must be 1 .. 4";
    if (t < 1) return "packing key: pk_t must be at least 1";
    if (t * b >= 32) return "packing key: pk_t x pk_basebit must stay below 32";
    if ((int64_t)p.n * t * ((1 << b) - 1) * 128 >= ((int64_t)1 << 31)) return "packing key: n x pk_t x (2^pk_basebit - 1) x 128 must stay below 2^31";
    return nullptr;
}
// Why the shape of a call is refused, or null.
inline const char* pack_call_error(const Params& p, int32_t m, int32_t spread, int32_t shift) {
    if (m < 1) return "pack: m must be at least 1";
    if (spread < 1) return "pack: spread must be at least 1";
    if ((int64_t)m * spread > p.N) return "pack: m x spread must not exceed N";
    if (shift < 0 || shift >= 2 * p.N) return "pack: shift must lie in [0, 2N)";
    return nullptr;
}

inline int64_t pack_k(const Params& p, int32_t t) { return (int64_t)p.n * t; }                                   // k = (i, j) flattened
inline int32_t pack_k_steps(const Params& p, int32_t t) { return (int32_t)((pack_k(p, t) + kPackKStep - 1) / kPackKStep); }  // zero key rows pad the last
inline int32_t pack_col_blocks(const Params& p) { return 2 * p.N / 32; }   // columns: the 2N words of a TLWE row, 32 per tile (N >= 16)
// bytes of the byte-limb form of the key: [K step][column block][4 limbs][64 lanes][16 bytes]
inline size_t pack_limb_bytes(const Params& p, int32_t t) { return (size_t)pack_k_steps(p, t) * pack_col_blocks(p) * 4096; }
inline int64_t pack_padded_rows(int64_t rows) { return (rows + kPackBlockRows - 1) / kPackBlockRows * kPackBlockRows; }
inline bool pack_split_ok(int32_t k_steps, int32_t split) {
    return split >= 1 && split <= kPackMaxSplit && (split & (split - 1)) == 0 && split <= k_steps;
}
// K steps [first, last) of split `s` of `split`: consecutive, together 0 .. k_steps exactly once, none empty when pack_split_ok
inline int32_t pack_split_first(int32_t k_steps, int32_t split, int32_t s) { return (int32_t)((int64_t)k_steps * s / split); }

struct PackPlan {
    int64_t groups_per_piece = 0, pieces = 0;
    int64_t piece_rows = 0;   // rows of the largest piece (the first)
    int64_t padded_rows = 0;  // ... padded to whole blocks of kPackBlockRows
    int32_t k_steps = 0, ksplit = 0;
    size_t r_bytes = 0;       // scratch every piece fits: R [piece_rows][2][N] int32
    size_t digit_bytes = 0;   //   and the digits [k_steps][padded_rows][32] int8
    Cut cut() const { return {pieces, groups_per_piece}; }  // of the groups (cmux_plan.h)
};

// A call of `groups` groups of `m` rows.  piece_rows_opt: "pack_piece_rows" (1 .. kPackPieceRows); split_opt: "pack_split",
// 0 = by size; cus: compute units of the device (<= 0: 256).
inline PackPlan pack_plan(const Params& p, int32_t t, int64_t groups, int32_t m, int64_t piece_rows_opt, int32_t split_opt, int64_t cus) {
    PackPlan pl;
    if (groups <= 0 || m < 1) return pl;
    if (piece_rows_opt < 1 || piece_rows_opt > kPackPieceRows) piece_rows_opt = kPackPieceRows;
    pl.groups_per_piece = piece_rows_opt / m < 1 ? 1 : piece_rows_opt / m;   // whole groups; one group when a group alone is longer
    if (pl.groups_per_piece > groups) pl.groups_per_piece = groups;
    pl.pieces = (groups + pl.groups_per_piece - 1) / pl.groups_per_piece;
    pl.piece_rows = pl.groups_per_piece * m;
    pl.padded_rows = pack_padded_rows(pl.piece_rows);
    pl.k_steps = pack_k_steps(p, t);
    pl.ksplit = split_opt;
    if (!pack_split_ok(pl.k_steps, pl.ksplit)) {
        // One wave of k_pack_gemm (all 512 registers) per SIMD at a time: W0 = row blocks x column blocks waves take
        // ceil(W0 k / slots) rounds of 1 / k of the walk each, plus a fixed cost per split (one more pass of atomic adds) --
        // the cost model of the LWE key switch's product (ks_plan.h).  Measured at n = 630 beside every forced split
        // (profiles/pack_rates.txt): 32 and 256 rows k = 8, 1 024 rows k = 2, 4 096 and 8 192 rows k = 1, each the fastest or within
        // the spread of the fastest.
        const int64_t slots = 4 * (cus <= 0 ? 256 : cus), W0 = pl.padded_rows / kPackBlockRows * pack_col_blocks(p);
        double best = 0;
        pl.ksplit = 0;
        for (int32_t k = 1; k <= kPackMaxSplit && pack_split_ok(pl.k_steps, k); k *= 2) {
            const double cost = (double)((W0 * k + slots - 1) / slots) / k + 0.02 * k;
            if (pl.ksplit == 0 || cost < best) {
                best = cost;
                pl.ksplit = k;
            }
        }
    }
    pl.r_bytes = (size_t)pl.piece_rows * 2 * (size_t)p.N * 4;
    pl.digit_bytes = (size_t)pl.k_steps * (size_t)pl.padded_rows * kPackKStep;
    return pl;
}

}  // namespace ieache
