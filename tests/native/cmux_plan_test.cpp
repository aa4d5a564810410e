// csrc/cmux_plan.h on its own (no HIP): the pieces cover every item exactly once and are whole items, the cap holds wherever
// an item fits under it, a single item wider than the cap still runs (alone), the scratch of the first piece fits every piece.
// Built with AddressSanitizer + UBSan by tests/test_cmux_cpu.py.
#include <cstdio>
#include <cstdlib>

#include "../../ie-ache_amd/csrc/cmux_plan.h"

using namespace ieache;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);        \
            exit(1);                                                   \
        }                                                              \
    } while (0)

static void check(int64_t items, int32_t depth, int64_t cap_opt) {
    const CmuxPlan pl = cmux_plan(items, depth, cap_opt);
    const int64_t cap = cap_opt < 1 || cap_opt > kCmuxPieceRowsMax ? kCmuxPieceRows : cap_opt;
    const int64_t per_item = depth < 1 ? 1 : (int64_t)1 << (depth - 1);
    CHECK(pl.pieces >= 1 && pl.items_per_piece >= 1 && pl.items_per_piece <= items);
    int64_t next = 0;
    for (int64_t i = 0; i < pl.pieces; i++) {
        const int64_t first = piece_first(pl.cut(), i), cnt = piece_count(pl.cut(), items, i);
        CHECK(first == next && cnt >= 1);
        // the cap, unless one item alone is wider
        CHECK(cnt * per_item <= cap || cnt == 1);
        // what was reserved for the first piece holds every piece
        CHECK(cnt * per_item <= pl.level0_rows);
        if (depth >= 2) CHECK(cnt * per_item <= pl.a_rows);
        if (depth >= 3) CHECK(cnt * per_item / 2 <= pl.b_rows);
        next = first + cnt;
    }
    CHECK(next == items);
    // no smaller number of pieces would do
    if (per_item <= cap) CHECK((pl.pieces - 1) * (cap / per_item) < items);
    if (depth < 2) CHECK(pl.a_rows == 0);
    if (depth < 3) CHECK(pl.b_rows == 0);
}

int main() {
    const int64_t counts[] = {1, 2, 3, 7, 8, 9, 63, 64, 65, 1000, 8191, 8192, 8193, 100000};
    const int64_t caps[] = {0, 1, 2, 3, 5, 16, 100, 2047, 2048, 2049, 8192, kCmuxPieceRowsMax, kCmuxPieceRowsMax + 1, -4};
    for (int64_t items : counts)
        for (int32_t depth = -1; depth <= kCmuxMaxDepth; depth++)
            for (int64_t cap : caps) check(items, depth, cap);
    // the figures the header states
    CmuxPlan pl = cmux_plan(64, 10, 0);
    CHECK(pl.items_per_piece == 16 && pl.pieces == 4 && pl.a_rows == 8192 && pl.b_rows == 4096);
    pl = cmux_plan(3, 12, 1024);  // an item of 2 048 level-0 rows under a cap of 1 024: one item per piece
    CHECK(pl.items_per_piece == 1 && pl.pieces == 3 && pl.a_rows == 2048 && pl.b_rows == 1024);
    pl = cmux_plan(20000, -1, 0);
    CHECK(pl.items_per_piece == 8192 && pl.pieces == 3 && pl.a_rows == 0 && pl.b_rows == 0);
    pl = cmux_plan(0, 4, 0);
    CHECK(pl.pieces == 0);
    pl = cmux_plan(5, 13, 0);
    CHECK(pl.pieces == 0);
    printf("CMUX_PLAN_OK\n");
    return 0;
}
