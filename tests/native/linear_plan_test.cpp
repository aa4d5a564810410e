// Which linear calls are accepted, the row kinds, the choice of kernel and the tiling (ie-ache_amd/csrc/linear_plan.h), as plain
// host C++ under AddressSanitizer / UBSan: every rule at its last accepted and first refused value and in its order, the kind
// table on several parameter sets, the automatic choice at the threshold, and for edge shapes a tiling that covers every
// output, every input and every word of a row up to its stride with nothing beyond the padded scratch.
// Built and run by tests/test_linear_cpu.py.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ie-ache_amd/csrc/linear_plan.h"

using namespace ieache;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                   \
        }                                                               \
    } while (0)

static bool says(const char* e, const char* what) { return e && strstr(e, what); }

static Params params(int32_t n, int32_t N) {
    Params p;
    p.n = n;
    p.N = N;
    return p;
}

static int check_kinds() {
    const int32_t sets[][2] = {{5, 16}, {37, 64}, {130, 1024}, {630, 1024}, {750, 2048}, {3, 16}, {4, 16}};
    for (const auto& s : sets) {
        const Params p = params(s[0], s[1]);
        const LinearRows lwe = linear_rows(p, kLinearRowsLwe), ext = linear_rows(p, kLinearRowsExtracted), tl = linear_rows(p, kLinearRowsTlwe);
        CHECK(lwe.words == p.n + 1 && lwe.stride == p.lwe_stride() && lwe.bias_word == p.n);
        CHECK(ext.words == p.N + 1 && ext.stride == p.N + 4 && ext.bias_word == p.N);
        CHECK(tl.words == 2 * p.N && tl.stride == 2 * p.N && tl.bias_word == -1);
        for (const LinearRows& r : {lwe, ext, tl}) CHECK(r.stride >= r.words && r.stride % 4 == 0 && r.stride - r.words < 4 && r.bias_word < r.words);
        CHECK(linear_rows(p, 3).words == 0 && linear_rows(p, -1).stride == 0);
    }
    CHECK(linear_kind_known(0) && linear_kind_known(1) && linear_kind_known(2) && !linear_kind_known(3) && !linear_kind_known(-1));
    return 0;
}

static int check_rules() {
    const Params p = params(37, 64);
    std::vector<int32_t> mem(64 * 1024);
    int8_t* w = reinterpret_cast<int8_t*>(mem.data());
    const int32_t *bias = mem.data() + 1024, *x = mem.data() + 2048;
    int32_t* out = mem.data() + 32768;
    auto call = [&](int32_t rows, size_t batch, int32_t n_out, int32_t n_in, const void* cw, const void* cb, const void* cx, const void* co, bool device) {
        LinearCall c;
        c.rows = rows, c.batch = batch, c.n_out = n_out, c.n_in = n_in, c.w = cw, c.bias = cb, c.x = cx, c.out = co, c.device = device;
        return linear_call_error(p, c);
    };
    // accepted: every kind, both forms, with and without a bias, the bounds of the dimensions
    for (int32_t rows : {0, 1, 2})
        for (bool device : {false, true}) {
            CHECK(!call(rows, 1, 1, 1, w, nullptr, x, out, device) && !call(rows, 2, 3, 5, w, rows == 2 ? nullptr : bias, x, out, device));
            CHECK(!call(rows, 0, kLinearMaxDim, kLinearMaxDim, nullptr, nullptr, nullptr, nullptr, device));  // batch 0: nothing is named
        }
    // 1: the kind, ahead of everything
    CHECK(says(call(3, 1, 0, 0, nullptr, bias, nullptr, nullptr, true), "unknown rows kind") && says(call(-1, 0, 1, 1, w, nullptr, x, out, false), "unknown rows kind"));
    // 2: the dimensions, ahead of the bias and the pointers
    CHECK(says(call(2, 1, 0, 1, nullptr, bias, nullptr, nullptr, true), "1 .. 65536") && says(call(0, 1, 1, 0, w, nullptr, x, out, false), "1 .. 65536"));
    CHECK(says(call(0, 1, kLinearMaxDim + 1, 1, w, nullptr, x, out, false), "1 .. 65536") && says(call(0, 1, 1, kLinearMaxDim + 1, w, nullptr, x, out, false), "1 .. 65536"));
    CHECK(says(call(0, 1, -1, 1, w, nullptr, x, out, false), "1 .. 65536") && says(call(0, 0, 1, INT32_MIN, w, nullptr, x, out, false), "1 .. 65536"));
    CHECK(says(linear_scalar_error(0, 65537, 65536, false), "1 .. 65536") && !linear_scalar_error(0, 65536, 65536, true));
    // 3: a bias with TLWE rows, ahead of the pointers, whatever the batch
    CHECK(says(call(2, 1, 1, 1, nullptr, bias, nullptr, nullptr, true), "bias must be NULL") && says(call(2, 0, 1, 1, w, bias, x, out, false), "bias must be NULL"));
    CHECK(!call(1, 1, 1, 1, w, bias, x, out, true));
    // 4: null required pointers when there are rows; a null bias is no bias
    CHECK(says(call(0, 1, 1, 1, nullptr, nullptr, x, out, false), "null argument") && says(call(0, 1, 1, 1, w, nullptr, nullptr, out, true), "null argument"));
    CHECK(says(call(0, 1, 1, 1, w, nullptr, x, nullptr, true), "null argument") && !call(0, 0, 1, 1, nullptr, nullptr, nullptr, nullptr, true));
    // 5: device form only -- the output over x, W or the bias, by a single byte at either end; the host form stages copies
    const size_t row = (size_t)p.lwe_stride();  // 40 words
    const int32_t* xs = mem.data() + 4096;      // x: 2 x 5 rows
    CHECK(!call(0, 2, 3, 5, w, bias, xs, xs + 2 * 5 * row, true) && says(call(0, 2, 3, 5, w, bias, xs, xs + 2 * 5 * row - 1, true), "overlaps"));
    CHECK(!call(0, 2, 3, 5, w, bias, xs, xs - 2 * 3 * row, true) && says(call(0, 2, 3, 5, w, bias, xs, xs - 2 * 3 * row + 1, true), "overlaps"));
    CHECK(says(call(0, 2, 3, 5, w, bias, xs, xs, true), "overlaps") && !call(0, 2, 3, 5, w, bias, xs, xs, false));
    int32_t* near_w = reinterpret_cast<int32_t*>(w + 16);  // W holds 15 bytes: the output may start at byte 16, not at byte 12
    CHECK(!call(0, 1, 3, 5, w, nullptr, xs, near_w, true) && says(call(0, 1, 3, 5, w, nullptr, xs, near_w - 1, true), "overlaps"));
    CHECK(says(call(0, 1, 3, 5, w, bias, xs, const_cast<int32_t*>(bias) + 2, true), "overlaps") && !call(0, 1, 3, 5, w, bias, xs, const_cast<int32_t*>(bias) + 3, true));
    CHECK(says(call(0, 1, 3, 5, w, bias, xs, const_cast<int32_t*>(bias) - 3 * row + 1, true), "overlaps"));
    // TLWE rows are 2N words long: the same pointers that are apart as LWE rows meet
    CHECK(!call(0, 1, 1, 1, w, nullptr, xs, xs + row, true) && says(call(2, 1, 1, 1, w, nullptr, xs, xs + row, true), "overlaps"));
    return 0;
}

static int check_plan(const LinearRows& r, int32_t n_out, int32_t n_in) {
    for (int32_t opt : {0, 1, 2}) {
        const LinearPlan pl = linear_plan(r, n_out, n_in, opt);
        CHECK(pl.kernel == (opt ? opt : n_out >= kLinearMfmaMinOut ? kLinearMfma : kLinearSimple));
        CHECK(pl.wave_tiles == 1 || pl.wave_tiles == 2 || pl.wave_tiles == 4);
        // every output in a tile, fewer than wave_tiles tiles of padding, and no wider a wave than the tiles need
        CHECK((int64_t)pl.padded_tiles() * kLinearTile >= n_out && (int64_t)(pl.padded_tiles() - pl.wave_tiles) * kLinearTile < n_out);
        CHECK(pl.wave_tiles == 1 || (int64_t)(pl.wave_tiles / 2) * kLinearTile < n_out);
        CHECK((int64_t)pl.k_steps * kLinearTile >= n_in && (int64_t)(pl.k_steps - 1) * kLinearTile < n_in);
        CHECK((int64_t)pl.col_blocks * kLinearTile >= r.stride && (int64_t)(pl.col_blocks - 1) * kLinearTile < r.stride);
        CHECK(pl.tile_groups >= 1 && pl.tile_groups <= 65535 && pl.k_steps <= 65535);  // gridDim.y of the product and of the preparation
        CHECK(pl.frag_bytes == (pl.kernel == kLinearMfma ? (size_t)pl.padded_tiles() * pl.k_steps * 64 * 16 : 0));
        // the largest fragment index the product reads is inside the scratch
        if (pl.kernel == kLinearMfma) {
            const size_t last = (((size_t)(pl.tile_groups - 1) * pl.wave_tiles + pl.wave_tiles - 1) * pl.k_steps + pl.k_steps - 1) * 64 + 63;
            CHECK((last + 1) * 16 == pl.frag_bytes);
        }
    }
    return 0;
}

int main() {
    if (check_kinds() || check_rules()) return 1;
    // the threshold of the automatic choice
    const LinearRows lwe = linear_rows(params(630, 1024), kLinearRowsLwe);
    CHECK(kLinearMfmaMinOut >= 1 && linear_plan(lwe, kLinearMfmaMinOut, 64, 0).kernel == kLinearMfma);
    CHECK(kLinearMfmaMinOut == 1 || linear_plan(lwe, kLinearMfmaMinOut - 1, 64, 0).kernel == kLinearSimple);
    CHECK(linear_plan(lwe, 1, 64, 2).kernel == kLinearMfma && linear_plan(lwe, 65536, 64, 1).kernel == kLinearSimple);
    CHECK(linear_plan(lwe, 8, 8, 7).kernel == linear_plan(lwe, 8, 8, 0).kernel);  // a value the option table refuses reads as 0
    // figures at the product parameters: 631 words in rows of 632, 20 column blocks
    const LinearPlan pl = linear_plan(lwe, 32, 784, 0);
    CHECK(pl.col_blocks == 20 && pl.wave_tiles == 1 && pl.tile_groups == 1 && pl.k_steps == 25 && pl.frag_bytes == 25 * 1024);
    CHECK(linear_plan(lwe, 33, 1, 2).wave_tiles == 2 && linear_plan(lwe, 65, 1, 2).wave_tiles == 4 && linear_plan(lwe, 65, 1, 2).tile_groups == 1);
    CHECK(linear_plan(lwe, 129, 1, 2).tile_groups == 2 && linear_plan(lwe, 65536, 65536, 2).tile_groups == 512);
    CHECK(linear_plan(lwe, 65536, 65536, 2).frag_bytes == (size_t)65536 * 65536);
    // edge shapes on every kind of several sets
    const int32_t sets[][2] = {{5, 16}, {37, 64}, {130, 1024}, {630, 1024}, {750, 2048}};
    for (const auto& s : sets)
        for (int32_t rows : {0, 1, 2})
            for (int32_t n_out : {1, 7, 8, 31, 32, 33, 64, 65, 96, 97, 128, 129, 1024, 65535, 65536})
                for (int32_t n_in : {1, 15, 16, 17, 31, 32, 33, 64, 65, 784, 65535, 65536})
                    if (check_plan(linear_rows(params(s[0], s[1]), rows), n_out, n_in)) return 1;
    printf("LINEAR_PLAN_OK\n");
    return 0;
}
