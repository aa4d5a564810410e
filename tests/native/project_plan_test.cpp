// How a projection and a replace write of a window are accepted and cut (ie-ache_amd/csrc/project_plan.h), as plain host C++
// under AddressSanitizer / UBSan: the projection's plan is the packing plan on n := N with an item as the group, every item
// lies in exactly one piece, an item of N rows fits one piece, the runs inside a piece of a write cover its items once, and
// each bound of the window and of the write's scalars holds at its last accepted and first refused value.
// Built and run by tests/test_project_cpu.py.
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../../ie-ache_amd/csrc/project_plan.h"

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

static int check_cut(const Params& p, int32_t t, int64_t items, int32_t width, int64_t piece_opt, int32_t split_opt) {
    const PackPlan pl = project_plan(p, t, items, width, piece_opt, split_opt, 256);
    const Params q = project_params(p);
    CHECK(q.n == p.N && q.N == p.N && pl.k_steps == (p.N * t + kPackKStep - 1) / kPackKStep && pack_split_ok(pl.k_steps, pl.ksplit));
    CHECK(pl.pieces >= 1 && pl.groups_per_piece >= 1);
    const int64_t cap = piece_opt >= 1 && piece_opt <= kPackPieceRows ? piece_opt : kPackPieceRows;
    std::vector<int> seen((size_t)items, 0);
    for (int64_t i = 0; i < pl.pieces; i++) {
        const int64_t i0 = piece_first(pl.cut(), i), cnt = piece_count(pl.cut(), items, i);
        CHECK(cnt >= 1 && i0 + cnt <= items);
        const int64_t rows = cnt * width, rpad = pack_padded_rows(rows);
        CHECK(rows <= cap || cnt == 1);
        CHECK((size_t)rows * 2 * (size_t)p.N * 4 <= pl.r_bytes && (size_t)pl.k_steps * (size_t)rpad * kPackKStep <= pl.digit_bytes);
        for (int64_t r = i0; r < i0 + cnt; r++) seen[(size_t)r]++;
    }
    for (int v : seen) CHECK(v == 1);
    // the runs of the projection inside a piece of a write with fewer items than the plan's largest piece
    for (int64_t piece_items : {(int64_t)1, items / 2 + 1, items}) {
        const int64_t runs = project_runs(pl, piece_items);
        int64_t covered = 0;
        for (int64_t r = 0; r < runs; r++) {
            const int64_t g = piece_count(pl.cut(), piece_items, r);
            CHECK(g >= 1 && g <= pl.groups_per_piece && piece_first(pl.cut(), r) == covered);
            covered += g;
        }
        CHECK(covered == piece_items);
    }
    CHECK(project_runs(pl, 0) == 0);
    return 0;
}

static bool says(const char* e, const char* part) { return e && strstr(e, part); }

static int check_accepted() {
    const Params p;  // n = 630, N = 1024
    // the key: section 3e's rules on n := N
    CHECK(!project_set_error(p, 8, 2) && project_set_error(p, 16, 2) && project_set_error(p, 8, 5) && project_set_error(p, 0, 2));
    CHECK(!project_set_error(p, 7, 4) && !project_set_error(set(159784, 1024), 7, 4));  // the source key has N words whatever n
    CHECK(pack_k(project_params(p), 8) == 8192 && pack_k_steps(project_params(p), 8) == 256);
    CHECK(pack_limb_bytes(project_params(p), 8) == (size_t)256 * 64 * 4096);  // 67 MB
    CHECK(says(project_set_error(set(5, 8), 8, 2), "unsupported"));
    // the window
    CHECK(!project_call_error(p, 0, 1, 0) && !project_call_error(p, 1023, 1, 2047) && !project_call_error(p, 0, 1024, 0));
    CHECK(says(project_call_error(p, -1, 1, 0), "first") && says(project_call_error(p, 1024, 1, 0), "first"));
    CHECK(says(project_call_error(p, 0, 0, 0), "width") && says(project_call_error(p, 1, 1024, 0), "exceed N") &&
          says(project_call_error(p, 1023, 2, 0), "exceed N") && says(project_call_error(p, 5, 2147483647, 0), "exceed N"));
    CHECK(says(project_call_error(p, 0, 1, -1), "dest") && says(project_call_error(p, 0, 1, 2048), "dest"));
    CHECK(!project_call_error(set(5, 16), 15, 1, 31) && project_call_error(set(5, 16), 15, 2, 0) && project_call_error(set(5, 16), 0, 1, 32));
    // the write's scalars
    CHECK(!write_coef_error(p.N, 0, 0, 1, 1) && !write_coef_error(p.N, 12, 10, 1, 1) && !write_coef_error(p.N, 4, 5, 32, 32) && !write_coef_error(p.N, 0, 0, 1024, 1024));
    CHECK(says(write_coef_error(p.N, -1, 0, 1, 1), "depth") && says(write_coef_error(p.N, 13, 0, 1, 1), "depth"));
    CHECK(says(write_coef_error(p.N, 0, -1, 1, 1), "steps") && says(write_coef_error(p.N, 0, 65, 1, 1), "steps"));
    CHECK(says(write_coef_error(p.N, 0, 0, 0, 1), "width") && says(write_coef_error(p.N, 0, 0, 4, 3), "unit must"));
    CHECK(says(write_coef_error(p.N, 0, 11, 1, 1), "exceed N") && says(write_coef_error(p.N, 0, 5, 32, 33), "exceed N") &&
          says(write_coef_error(p.N, 0, 64, 1, 1), "exceed N") && says(write_coef_error(p.N, 0, 31, 1, 1), "exceed N") &&
          says(write_coef_error(p.N, 0, 1, 1, 2147483647), "exceed N"));
    // the amounts: the read's and the write's of a step cancel mod 2N
    for (int32_t unit : {1, 3, 32})
        for (int32_t s = 0; ((int64_t)unit << s) <= p.N; s++) {
            const int32_t a = write_coef_amount(p, unit, s, true), b = write_coef_amount(p, unit, s, false);
            CHECK(b == unit << s && a >= 0 && a < 2 * p.N && (a + b) % (2 * p.N) == 0);
        }
    return 0;
}

static int check_pieces() {
    const Params p;
    // an item of N rows fits one piece; four of them too; a fifth starts the second piece
    CHECK(project_plan(p, 8, 1, 1024, 0, 0, 256).pieces == 1 && project_plan(p, 8, 4, 1024, 0, 0, 256).pieces == 1 &&
          project_plan(p, 8, 5, 1024, 0, 0, 256).pieces == 2);
    CHECK(project_plan(p, 8, 4096, 1, 0, 0, 256).pieces == 1 && project_plan(p, 8, 4097, 1, 0, 0, 256).pieces == 2);
    // "pack_piece_rows" lowered: one item per piece once an item alone reaches the cap
    CHECK(project_plan(p, 8, 3, 32, 32, 0, 256).pieces == 3 && project_plan(p, 8, 3, 32, 16, 0, 256).pieces == 3 &&
          project_plan(p, 8, 3, 32, 64, 0, 256).pieces == 2);
    // a forced split is kept where the walk allows it
    CHECK(project_plan(p, 8, 1, 1, 0, 8, 256).ksplit == 8 && project_plan(set(5, 16), 2, 1, 1, 0, 8, 256).ksplit == 1);
    CHECK(project_plan(p, 8, 0, 4, 0, 0, 256).pieces == 0);
    return 0;
}

int main() {
    if (check_accepted() || check_pieces()) return 1;
    for (const Params& p : {set(630, 1024), set(37, 64), set(5, 16)})
        for (int32_t t : {1, 2, 8})
            for (int64_t items : {1, 2, 3, 5, 64, 1000})
                for (int32_t width : {1, 3, 4, 32, 1024})
                    for (int64_t piece : {(int64_t)0, (int64_t)1, (int64_t)33, (int64_t)160, (int64_t)4096, (int64_t)5000})
                        for (int32_t split : {0, 1, 3, 8})
                            if (width <= p.N && check_cut(p, t, items, width, piece, split)) return 1;
    printf("PROJECT_PLAN_OK\n");
    return 0;
}
