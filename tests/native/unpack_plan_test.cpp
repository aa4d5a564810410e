// Which unpacking calls and word reads are accepted and how their rows are cut (ie-ache_amd/csrc/unpack_plan.h), as plain host
// C++ under AddressSanitizer / UBSan: the window rule at its last accepted and first refused value for every bound, every
// coefficient of an accepted window inside the sample, the runs covering every row once (a run may begin inside an item), and
// word_read's refusals in lut_read's order with the write's window rule under its own name.
// Built and run by tests/test_unpack_cpu.py.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ie-ache_amd/csrc/unpack_plan.h"

using namespace ieache;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                   \
        }                                                               \
    } while (0)

static bool says(const char* e, const char* what) { return e && strstr(e, what); }

static int check_window(int32_t N) {
    // the bounds: first
    CHECK(!unpack_window_error(N, 0, 1, 1) && !unpack_window_error(N, N - 1, 1, 1));
    CHECK(says(unpack_window_error(N, -1, 1, 1), "first must") && says(unpack_window_error(N, N, 1, 1), "first must"));
    // width, spread
    CHECK(says(unpack_window_error(N, 0, 0, 1), "width must") && says(unpack_window_error(N, 0, -3, 1), "width must"));
    CHECK(says(unpack_window_error(N, 0, 1, 0), "spread must") && says(unpack_window_error(N, 0, 2, -1), "spread must"));
    // the last coefficient
    CHECK(!unpack_window_error(N, 0, N, 1) && says(unpack_window_error(N, 0, N + 1, 1), "below N") && says(unpack_window_error(N, 1, N, 1), "below N"));
    CHECK(!unpack_window_error(N, N - 1, 1, 1 << 30) && says(unpack_window_error(N, N - 1, 2, 1), "below N"));
    CHECK(!unpack_window_error(N, N / 2 - 1, 2, N / 2) && says(unpack_window_error(N, N / 2, 2, N / 2), "below N"));
    // no overflow at the extremes of int32
    CHECK(says(unpack_window_error(N, N - 1, 0x7FFFFFFF, 0x7FFFFFFF), "below N") && says(unpack_window_error(N, 0, 0x7FFFFFFF, 1), "below N"));
    // the order: first, width, spread, the end, the flags
    CHECK(says(unpack_call_error(N, -1, 0, 0, 2), "first must") && says(unpack_call_error(N, 0, 0, 0, 2), "width must"));
    CHECK(says(unpack_call_error(N, 0, 1, 0, 2), "spread must") && says(unpack_call_error(N, 0, 1, 1, 2), "unknown flag"));
    CHECK(!unpack_call_error(N, 0, 1, 1, 0) && !unpack_call_error(N, 0, 1, 1, kUnpackNoKeyswitch) && says(unpack_call_error(N, 0, 1, 1, 3), "unknown flag"));
    // every accepted window of a small grid keeps its coefficients inside the sample, every refused one does not
    for (int32_t first = -1; first <= N; first++)
        for (int32_t width = 0; width <= N + 1; width += (width < 4 ? 1 : N / 4))
            for (int32_t spread : {0, 1, 2, 3, N / 2, N - 1, N}) {
                const bool inside = first >= 0 && first < N && width >= 1 && spread >= 1 && (int64_t)first + (int64_t)(width - 1) * spread < N;
                CHECK((unpack_window_error(N, first, width, spread) == nullptr) == inside);
                if (!inside) continue;
                const UnpackWindow w{first, width, spread};
                CHECK(unpack_coef(w, 0) == first && unpack_coef(w, width - 1) >= first && unpack_coef(w, width - 1) < N);
            }
    return 0;
}

static int check_runs(int64_t items, int32_t width, int64_t chunk) {
    const int64_t rows = unpack_rows(items, width);
    const Cut cut = unpack_runs(items, width, chunk);
    if (rows == 0) {
        CHECK(cut.pieces == 0);
        return 0;
    }
    const int64_t cap = chunk < 1 || chunk > rows ? rows : chunk;
    CHECK(cut.per_piece == cap && cut.pieces == (rows + cap - 1) / cap);
    std::vector<int> seen((size_t)rows, 0);
    bool inside_an_item = false;
    for (int64_t r = 0; r < cut.pieces; r++) {
        const int64_t r0 = piece_first(cut, r), cnt = piece_count(cut, rows, r);
        CHECK(cnt >= 1 && cnt <= cap && r0 + cnt <= rows);
        inside_an_item |= r0 % width != 0;
        for (int64_t g = r0; g < r0 + cnt; g++) seen[(size_t)g]++;
    }
    for (int v : seen) CHECK(v == 1);
    CHECK(inside_an_item == (cut.pieces > 1 && cap % width != 0));
    return 0;
}

static int check_word_read(int32_t N) {
    CHECK(!word_read_error(N, 0, 0, 1, 0, 1, 1) && !word_read_error(N, 12, 0, 1, 1, 1, 1) && !word_read_error(N, 0, 0, 1, 0, N, N));
    CHECK(says(word_read_error(N, -1, 0, 1, 0, 1, 1), "word_read: depth must") && says(word_read_error(N, 13, 0, 1, 0, 1, 1), "depth must"));
    CHECK(says(word_read_error(N, 0, -1, 1, 0, 1, 1), "word_read: steps must") && says(word_read_error(N, 0, 65, 1, 0, 1, 1), "steps must"));
    CHECK(says(word_read_error(N, 0, 0, 0, 0, 1, 1), "word_read: n_tables must") && says(word_read_error(N, 0, 0, 1, 2, 1, 1), "word_read: unknown flag"));
    CHECK(says(word_read_error(N, 0, 0, 1, 0, 0, 1), "word_read: width must") && says(word_read_error(N, 0, 0, 1, 0, 4, 3), "word_read: unit must"));
    // unit 2^steps == N is the bound
    int32_t steps = 0;
    while (((int64_t)32 << (steps + 1)) <= N) steps++;
    if (N >= 32) {
        CHECK(((int64_t)32 << steps) <= N && !word_read_error(N, 0, steps, 1, 0, 32, 32));
        CHECK(says(word_read_error(N, 0, steps + 1, 1, 0, 32, 32), "word_read: unit x 2^steps must not exceed N"));
    }
    CHECK(says(word_read_error(N, 0, 0, 1, 0, N + 1, N + 1), "must not exceed N") && says(word_read_error(N, 0, 31, 1, 0, 1, 1), "must not exceed N"));
    CHECK(says(word_read_error(N, 0, 64, 1, 0, 1, 1), "must not exceed N"));
    // lut_read's order, then the window's
    CHECK(says(word_read_error(N, -1, -1, 0, 2, 0, 0), "depth must") && says(word_read_error(N, 0, -1, 0, 2, 0, 0), "steps must"));
    CHECK(says(word_read_error(N, 0, 0, 0, 2, 0, 0), "n_tables must") && says(word_read_error(N, 0, 0, 1, 2, 0, 0), "unknown flag"));
    CHECK(says(word_read_error(N, 0, 0, 1, 0, 0, -1), "width must"));
    // the window's rule is the write's: one refuses exactly where the other does, under its own name
    for (int32_t st : {0, 1, 5, 6, 30, 31})
        for (int32_t width : {0, 1, 3, 32, N})
            for (int32_t unit : {0, 1, 3, 4, 32, 33, N, N + 1}) {
                const char *r = word_read_error(N, 2, st, 1, 0, width, unit), *w = write_coef_error(N, 2, st, width, unit);
                CHECK((r == nullptr) == (w == nullptr));
                if (r) CHECK(!strncmp(r, "word_read: ", 11) && !strncmp(w, "lut_write_coef: ", 16) && !strcmp(r + 11, w + 16));
            }
    return 0;
}

int main() {
    for (int32_t N : {16, 64, 1024}) {
        if (check_window(N)) return 1;
        if (check_word_read(N)) return 1;
    }
    for (int64_t items : {0, 1, 3, 7})
        for (int32_t width : {1, 3, 5, 171, 1024})
            for (int64_t chunk : {-1, 0, 1, 2, 3, 4, 512, 513, 4096, 1 << 20})
                if (check_runs(items, width, chunk)) return 1;
    printf("UNPACK_PLAN_OK\n");
    return 0;
}
