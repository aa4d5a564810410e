// How a packing call is cut (ie-ache_amd/csrc/pack_plan.h), as plain host C++ under AddressSanitizer / UBSan: every row lies in
// exactly one piece, pieces hold whole groups, the reserved sizes bound every piece, every K split covers K exactly once, and
// the accepted decompositions end where include/ieache.h section 3e says.
// Built and run by tests/test_pack_cpu.py.
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "../../ie-ache_amd/csrc/pack_plan.h"

using namespace ieache;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                   \
        }                                                               \
    } while (0)

static Params set(int32_t n, int32_t N) {
    Params p;
    p.n = n;
    p.N = N;
    return p;
}

static int check_pieces(const Params& p, int32_t t, int64_t groups, int32_t m, int64_t piece_opt, int32_t split_opt) {
    const PackPlan pl = pack_plan(p, t, groups, m, piece_opt, split_opt, 256);
    CHECK(pl.pieces >= 1 && pl.groups_per_piece >= 1 && pl.k_steps == pack_k_steps(p, t) && pack_split_ok(pl.k_steps, pl.ksplit));
    if (pack_split_ok(pl.k_steps, split_opt)) CHECK(pl.ksplit == split_opt);
    // whole groups, each row in exactly one piece
    std::vector<int> seen((size_t)(groups * m), 0);
    for (int64_t i = 0; i < pl.pieces; i++) {
        const int64_t g0 = piece_first(pl.cut(), i), cnt = piece_count(pl.cut(), groups, i);
        CHECK(cnt >= 1 && g0 + cnt <= groups);
        const int64_t rows = cnt * m, rpad = pack_padded_rows(rows);
        // the reserved sizes bound the piece, and the piece stays under the named constant unless one group alone is longer
        CHECK(rows <= pl.piece_rows && rpad <= pl.padded_rows && rpad % kPackBlockRows == 0 && rpad >= rows);
        CHECK((size_t)rows * 2 * (size_t)p.N * 4 <= pl.r_bytes && (size_t)pl.k_steps * (size_t)rpad * kPackKStep <= pl.digit_bytes);
        const int64_t cap = piece_opt >= 1 && piece_opt <= kPackPieceRows ? piece_opt : kPackPieceRows;
        CHECK(rows <= cap || cnt == 1);
        for (int64_t r = g0 * m; r < (g0 + cnt) * m; r++) seen[(size_t)r]++;
    }
    for (int v : seen) CHECK(v == 1);
    CHECK(pl.pieces == (groups + pl.groups_per_piece - 1) / pl.groups_per_piece);
    return 0;
}

static int check_splits() {
    for (int32_t k_steps : {1, 2, 3, 7, 8, 9, 33, 158, 630}) {
        int allowed = 0;
        for (int32_t split = -1; split <= 17; split++) {
            const bool ok = pack_split_ok(k_steps, split);
            CHECK(ok == ((split == 1 || split == 2 || split == 4 || split == 8) && split <= k_steps));
            if (!ok) continue;
            allowed++;
            // consecutive shares, none empty, together every K step exactly once
            std::vector<int> seen((size_t)k_steps, 0);
            CHECK(pack_split_first(k_steps, split, 0) == 0 && pack_split_first(k_steps, split, split) == k_steps);
            for (int32_t s = 0; s < split; s++) {
                const int32_t s0 = pack_split_first(k_steps, split, s), s1 = pack_split_first(k_steps, split, s + 1);
                CHECK(s0 < s1);
                for (int32_t q = s0; q < s1; q++) seen[(size_t)q]++;
            }
            for (int v : seen) CHECK(v == 1);
        }
        CHECK(allowed == (k_steps >= 8 ? 4 : k_steps >= 4 ? 3 : k_steps >= 2 ? 2 : 1));
    }
    return 0;
}

static int check_accepted() {
    const Params p;  // n = 630, N = 1024
    CHECK(!pack_set_error(p, 8, 2) && pack_k(p, 8) == 5040 && pack_k_steps(p, 8) == 158 && pack_col_blocks(p) == 64);
    CHECK(pack_limb_bytes(p, 8) == (size_t)158 * 64 * 4096);  // 41 MB
    CHECK(kPackPieceRows * 2 * 1024 * 4 == 32 << 20);           // R of a full piece: 32 MB
    // b in 1 .. 4, t >= 1, t b < 32
    CHECK(!pack_set_error(p, 31, 1) && pack_set_error(p, 32, 1) && !pack_set_error(p, 7, 4) && pack_set_error(p, 8, 4));
    CHECK(!pack_set_error(p, 1, 1) && pack_set_error(p, 0, 2) && pack_set_error(p, 8, 0) && pack_set_error(p, 4, 5) && !pack_set_error(p, 10, 3) &&
          pack_set_error(p, 11, 3));
    // n t (2^b - 1) 128 < 2^31: at b = 4, t = 7 the last n is floor((2^24 - 1) / 105) = 159 783
    CHECK(!pack_set_error(set(159783, 1024), 7, 4) && pack_set_error(set(159784, 1024), 7, 4));
    CHECK((int64_t)159783 * 7 * 15 * 128 < ((int64_t)1 << 31) && (int64_t)159784 * 7 * 15 * 128 >= ((int64_t)1 << 31));
    // ring sizes are Params::supported()'s
    CHECK(!pack_set_error(set(5, 16), 8, 2) && pack_set_error(set(5, 8), 8, 2) && pack_set_error(set(5, 2048), 8, 2) && pack_col_blocks(set(5, 16)) == 1);
    // the shape of a call, each bound at its last accepted and first refused value
    CHECK(!pack_call_error(p, 1, 1, 0) && pack_call_error(p, 0, 1, 0) && pack_call_error(p, 1, 0, 0));
    CHECK(!pack_call_error(p, 1024, 1, 0) && pack_call_error(p, 1025, 1, 0) && !pack_call_error(p, 4, 256, 0) && pack_call_error(p, 4, 257, 0));
    CHECK(!pack_call_error(p, 1, 1, 2047) && pack_call_error(p, 1, 1, 2048) && pack_call_error(p, 1, 1, -1));
    CHECK(pack_call_error(p, 65536, 65536, 0));  // the product does not wrap
    return 0;
}

static int check_auto_split() {
    const Params p;
    // 64 column blocks, 1 024 wave slots: one row block takes the longest split, many take none
    CHECK(pack_plan(p, 8, 1, 32, 0, 0, 256).ksplit == 8);
    CHECK(pack_plan(p, 8, 1, 1024, 0, 0, 256).ksplit == 2);
    CHECK(pack_plan(p, 8, 8, 1024, 0, 0, 256).ksplit == 1 && pack_plan(p, 8, 8, 1024, 0, 0, 256).pieces == 2);
    // a walk shorter than the split: n = 5, t = 8 is two K steps
    CHECK(pack_plan(set(5, 1024), 8, 1, 32, 0, 8, 256).ksplit <= 2 && pack_plan(set(5, 1024), 8, 1, 32, 0, 2, 256).ksplit == 2);
    CHECK(pack_plan(set(1, 16), 1, 1, 1, 0, 0, 256).ksplit == 1 && pack_plan(p, 8, 0, 4, 0, 0, 256).pieces == 0);
    return 0;
}

int main() {
    if (check_splits() || check_accepted() || check_auto_split()) return 1;
    for (const Params& p : {set(630, 1024), set(37, 64), set(5, 16)})
        for (int32_t t : {1, 8, 31})
            for (int64_t groups : {1, 2, 3, 5, 64, 1000})
                for (int32_t m : {1, 2, 4, 33, 256, 1024})
                    for (int64_t piece : {(int64_t)0, (int64_t)1, (int64_t)33, (int64_t)64, (int64_t)100, (int64_t)4096, (int64_t)5000})
                        for (int32_t split : {0, 1, 3, 8})
                            if (m <= p.N && check_pieces(p, t, groups, m, piece, split)) return 1;
    printf("PACK_PLAN_OK\n");
    return 0;
}
