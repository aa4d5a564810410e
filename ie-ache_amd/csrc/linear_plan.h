// Linear layers on encrypted rows (include/ieache.h section 3n; lwe_linear.hip): a public int8 matrix times LWE rows, mod 2^32.
// The row kinds (words, device stride, bias word), which calls are accepted -- the rules, their order and their words -- and the
// choice of kernel with its tiling: THE statement of it (capi.cpp and the evaluator refuse by linear_call_error, lwe_linear.hip
// launches by linear_plan and sizes its scratch by it; nothing else states a bound).  Free of HIP so that the CPU tests can check
// it (tests/native/linear_plan_test.cpp).
//
//   out[b][i][w] = sum_{j < n_in} W[i][j] x[b][j][w]  +  [w == bias word] bias[i]      (mod 2^32; b < batch, i < n_out, w < words)
//
//   k_linear_simple    a thread per output word, n_in 32-bit multiply-adds: any shape, and the second witness
//   k_linear_prepare   per call of the product: W [n_out][n_in] int8 -> A fragments in MFMA operand order, zero-padded
//   k_linear_mfma      the product on the int8 MFMA pipe, the words of x cut in registers into four balanced byte limbs
#pragma once
#include <cstddef>
#include <cstdint>

#include "params.h"

namespace ieache {

constexpr int32_t kLinearRowsLwe = 0;        // IEACHE_ROWS_LWE: n + 1 words, rows of lwe_stride(), bias on word n
constexpr int32_t kLinearRowsExtracted = 1;  // IEACHE_ROWS_EXTRACTED: N + 1 words, rows of extract_stride(), bias on word N
constexpr int32_t kLinearRowsTlwe = 2;       // IEACHE_ROWS_TLWE: 2N words, packed, no bias word
// IEACHE_LINEAR_MAX_DIM: n_out and n_in at most.  A limb column of k_linear_mfma accumulates n_in products of magnitude
// <= 128 x 128, so 65 536 x 2^14 = 2^30 < 2^31 keeps its int32 accumulators exact.
constexpr int32_t kLinearMaxDim = 65536;
constexpr int32_t kLinearTile = 32;          // outputs of an MFMA tile, words of a column block, inputs of a K step
constexpr int32_t kLinearMaxWaveTiles = 4;   // output tiles a wave of k_linear_mfma owns at most (16 accumulator tiles with the four limbs)
// "linear_kernel" = 0: calls of at least this many outputs take the product.  The product streams x once per group of tiles
// while the simple kernel reads it once per output.  MEASURED (profiles/linear_rates.txt, LWE rows at n = 630, batch 1 024,
// n_in = 64): one output 0.045 ms simple against 0.048 ms product, two 0.069 against 0.049, eight 0.217 against 0.051 -- the
// product's time is flat up to a tile of 32 outputs, the simple kernel's grows with n_out; at 4 -> 1 over 4 096 elements the
// simple kernel takes 0.017 ms against 0.047.
constexpr int32_t kLinearMfmaMinOut = 2;
constexpr int32_t kLinearSimple = 1, kLinearMfma = 2;  // "linear_kernel" values other than 0, and LinearPlan::kernel

struct LinearRows {
    int32_t words = 0;      // words of a row that carry data
    int32_t stride = 0;     // words from a device row to the next (host rows are packed: `words`)
    int32_t bias_word = 0;  // the word a bias is added to, or -1: the kind takes none
};
inline bool linear_kind_known(int32_t rows) { return rows == kLinearRowsLwe || rows == kLinearRowsExtracted || rows == kLinearRowsTlwe; }
// THE kind table (an unknown kind: zeros)
inline LinearRows linear_rows(const Params& p, int32_t rows) {
    switch (rows) {
    case kLinearRowsLwe: return {p.n + 1, p.lwe_stride(), p.n};
    case kLinearRowsExtracted: return {p.N + 1, (p.N + 1 + 3) & ~3, p.N};  // Evaluator::extract_stride()
    case kLinearRowsTlwe: return {2 * p.N, 2 * p.N, -1};
    default: return {};
    }
}

// One call as the rules see it.  Pointers are compared and never read.
struct LinearCall {
    int32_t rows = 0;
    size_t batch = 0;
    int32_t n_out = 0, n_in = 0;
    const void *w = nullptr, *bias = nullptr, *x = nullptr, *out = nullptr;
    bool device = false;  // the device form: rows of `stride` words, and the overlap rule
};

constexpr const char* kLinearNull = "lwe_linear: null argument";
// Rules 1 to 3, which need neither a context nor a parameter set: the message of the first one broken, or null.
inline const char* linear_scalar_error(int32_t rows, int32_t n_out, int32_t n_in, bool has_bias) {
    static_assert(kLinearMaxDim == 65536, "the message below spells the limit out");
    if (!linear_kind_known(rows)) return "lwe_linear: unknown rows kind (IEACHE_ROWS_LWE, IEACHE_ROWS_EXTRACTED, IEACHE_ROWS_TLWE)";
    if (n_out < 1 || n_out > kLinearMaxDim || n_in < 1 || n_in > kLinearMaxDim) return "lwe_linear: n_out and n_in must lie in 1 .. 65536";
    if (rows == kLinearRowsTlwe && has_bias) return "lwe_linear: TLWE rows have no bias word: bias must be NULL";
    return nullptr;
}
inline bool linear_ranges_meet(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return a && b && pa < pb + b_bytes && pb < pa + a_bytes;
}
// Why a call is refused, or null, in the order of include/ieache.h: (1) the kind, (2) n_out and n_in, (3) a bias with TLWE
// rows, (4) a null W, x or out when batch > 0, (5) device form only: out over x, W or bias.
inline const char* linear_call_error(const Params& p, const LinearCall& c) {
    if (const char* e = linear_scalar_error(c.rows, c.n_out, c.n_in, c.bias != nullptr)) return e;
    if (c.batch > 0 && (!c.w || !c.x || !c.out)) return kLinearNull;
    if (c.device && c.batch > 0) {
        const size_t row_bytes = (size_t)linear_rows(p, c.rows).stride * 4;
        const size_t out_bytes = c.batch * (size_t)c.n_out * row_bytes;
        if (linear_ranges_meet(c.out, out_bytes, c.x, c.batch * (size_t)c.n_in * row_bytes) ||
            linear_ranges_meet(c.out, out_bytes, c.w, (size_t)c.n_out * (size_t)c.n_in) ||
            linear_ranges_meet(c.out, out_bytes, c.bias, (size_t)c.n_out * 4))
            return "lwe_linear: the output overlaps an input (rows, weights or bias); there is no in-place form";
    }
    return nullptr;
}

// How a call runs.  The product: gridDim.x = batch x col_blocks waves of 32 consecutive words of one batch element,
// gridDim.y = tile_groups groups of wave_tiles output tiles each; a wave walks all k_steps alone.
struct LinearPlan {
    int32_t kernel = 0;       // kLinearSimple or kLinearMfma
    int32_t col_blocks = 0;   // blocks of 32 words covering a device row up to its stride (the padding is written as zero)
    int32_t wave_tiles = 0;   // output tiles of 32 a wave owns: 1, 2 or 4
    int32_t k_steps = 0;      // steps of 32 inputs; zero weights pad the last
    int32_t tile_groups = 0;  // groups of wave_tiles tiles covering n_out; zero weights pad the last
    size_t frag_bytes = 0;    // the prepared weights [tile_groups x wave_tiles][k_steps][64 lanes][16 bytes]; 0: the simple kernel
    int32_t padded_tiles() const { return tile_groups * wave_tiles; }
};
inline int32_t linear_ceil_div(int32_t a, int32_t b) { return (a + b - 1) / b; }
// kernel_opt: "linear_kernel" (0 = by n_out).  The figures describe the product's tiling whichever kernel runs, except that the
// simple kernel prepares nothing.
inline LinearPlan linear_plan(const LinearRows& r, int32_t n_out, int32_t n_in, int32_t kernel_opt) {
    LinearPlan pl;
    pl.kernel = kernel_opt == kLinearSimple || kernel_opt == kLinearMfma ? kernel_opt : n_out >= kLinearMfmaMinOut ? kLinearMfma : kLinearSimple;
    pl.col_blocks = linear_ceil_div(r.stride, kLinearTile);
    const int32_t tiles = linear_ceil_div(n_out, kLinearTile);
    pl.wave_tiles = tiles >= 3 ? 4 : tiles;  // 1, 2 or 4: three tiles run as four, the last of them zero weights
    static_assert(kLinearMaxWaveTiles == 4, "the line above names the largest");
    pl.tile_groups = linear_ceil_div(tiles, pl.wave_tiles);
    pl.k_steps = linear_ceil_div(n_in, kLinearTile);
    pl.frag_bytes = pl.kernel == kLinearMfma ? (size_t)pl.padded_tiles() * (size_t)pl.k_steps * 1024 : 0;
    return pl;
}

}  // namespace ieache
