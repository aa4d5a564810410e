// Stand-alone host test of csrc/automaton_plan.h (built with -fsanitize=address,undefined by tests/test_automaton_cpu.py): the
// refusals and their order, the live masks against a brute-force walk, the CMux count, the cut of a call into pieces and of the
// steps into launches.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../ie-ache_amd/csrc/automaton_plan.h"

using namespace ieache;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                    \
        }                                                                \
    } while (0)

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)((g_state >> 11) % n);
}
static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

static int refusals() {
    std::vector<int32_t> a(3 * 4, 0), b(3 * 4, 1);
    CHECK(automaton_refusal(4, 3, 2, a.data(), b.data()).empty());
    CHECK(automaton_refusal(1, 0, 1, nullptr, nullptr).empty());
    CHECK(automaton_refusal(64, 0, 64, nullptr, nullptr).empty());
    CHECK(has(automaton_refusal(0, 3, 1, a.data(), b.data()), "states must lie in 1 .. 64"));
    CHECK(has(automaton_refusal(65, 3, 1, a.data(), b.data()), "states"));
    CHECK(has(automaton_refusal(4, -1, 1, a.data(), b.data()), "steps must lie in 0 .. 4096"));
    CHECK(has(automaton_refusal(4, 4097, 1, a.data(), b.data()), "steps"));
    CHECK(has(automaton_refusal(4, 3, 0, a.data(), b.data()), "n_out must lie in 1 .. states"));
    CHECK(has(automaton_refusal(4, 3, 5, a.data(), b.data()), "n_out"));
    CHECK(has(automaton_refusal(0, -1, 0, a.data(), b.data()), "states"));  // the scalars in their order
    CHECK(has(automaton_refusal(4, 3, 1, nullptr, b.data()), "null transition table"));
    // the first bad entry by (step, state, next0 before next1)
    b[1 * 4 + 2] = 4;
    CHECK(has(automaton_refusal(4, 3, 1, a.data(), b.data()), "next1[1][2] = 4 is outside [0, 4)"));
    a[2 * 4 + 0] = -1;
    CHECK(has(automaton_refusal(4, 3, 1, a.data(), b.data()), "next1[1][2] = 4"));
    a[1 * 4 + 2] = 7;
    CHECK(has(automaton_refusal(4, 3, 1, a.data(), b.data()), "next0[1][2] = 7"));
    a[0] = -3;
    CHECK(has(automaton_refusal(4, 3, 1, a.data(), b.data()), "next0[0][0] = -3"));
    return 0;
}

// live masks against a walk of every word of `steps` letters from every start state below n_out
static int live_masks() {
    for (int trial = 0; trial < 200; trial++) {
        const int32_t states = 1 + (int32_t)rnd(trial < 20 ? 64 : 7), steps = (int32_t)rnd(9), n_out = 1 + (int32_t)rnd((uint32_t)states);
        std::vector<int32_t> a((size_t)steps * states + 1), b((size_t)steps * states + 1);
        for (size_t i = 0; i < (size_t)steps * states; i++) {
            a[i] = (int32_t)rnd((uint32_t)states);
            b[i] = rnd(4) == 0 ? a[i] : (int32_t)rnd((uint32_t)states);
        }
        CHECK(automaton_refusal(states, steps, n_out, a.data(), b.data()).empty());
        std::vector<uint64_t> live((size_t)steps + 1, 0xDEADBEEFull);
        const int64_t cmuxes = automaton_live(states, steps, n_out, a.data(), b.data(), live.data());
        std::vector<uint64_t> want((size_t)steps + 1, 0);
        for (int32_t q0 = 0; q0 < n_out; q0++)
            for (uint32_t word = 0; word < (1u << steps); word++) {
                int32_t q = q0;
                want[0] |= (uint64_t)1 << q;
                for (int32_t t = 0; t < steps; t++) {
                    q = ((word >> t) & 1 ? b : a)[(size_t)t * states + q];
                    want[t + 1] |= (uint64_t)1 << q;
                }
            }
        int64_t count = 0;
        for (int32_t t = 0; t <= steps; t++) {
            CHECK(live[t] == want[t]);
            for (int32_t q = 0; t < steps && q < states; q++)
                count += ((want[t] >> q) & 1) && a[(size_t)t * states + q] != b[(size_t)t * states + q];
        }
        CHECK(cmuxes == count);
    }
    // 64 states, all live: the mask is all ones and no shift overflows
    std::vector<int32_t> id(64), sw(64);
    for (int q = 0; q < 64; q++) id[q] = q, sw[q] = 63 - q;
    uint64_t live[2];
    CHECK(automaton_live(64, 1, 64, id.data(), sw.data(), live) == 64 && live[0] == ~(uint64_t)0 && live[1] == ~(uint64_t)0);
    CHECK(automaton_live(64, 1, 1, id.data(), sw.data(), live) == 1 && live[0] == 1 && live[1] == (((uint64_t)1 << 63) | 1));
    return 0;
}

static int pieces_and_chunks() {
    const int64_t caps[] = {0, 1, 2, 7, 8, 9, 127, 128, 129, 1000, 8192, (int64_t)1 << 20, ((int64_t)1 << 20) + 1};
    const int32_t states_of[] = {1, 2, 3, 4, 5, 9, 16, 63, 64};
    const int32_t steps_of[] = {0, 1, 2, 3, 5, 16, 255, 256, 2048, 2049, 4095, 4096};
    const int64_t per_launch[] = {0, 1, 2, 3, 7, 4096, 5000, -1};
    for (int64_t cap : caps)
        for (int32_t states : states_of)
            for (int32_t steps : steps_of)
                for (int64_t k : per_launch)
                    for (int64_t items : {(int64_t)1, (int64_t)2, (int64_t)3, (int64_t)64, (int64_t)1100, (int64_t)100000}) {
                        const AutomatonPlan pl = automaton_plan(items, states, steps, cap, k);
                        const int64_t eff = cap < 1 || cap > kCmuxPieceRowsMax ? kCmuxPieceRows : cap;
                        // every item falls in exactly one piece, whole; the cap holds, or the item runs alone
                        CHECK(pl.pieces >= 1 && pl.items_per_piece >= 1);
                        int64_t seen = 0;
                        for (int64_t i = 0; i < pl.pieces; i++) {
                            const int64_t first = piece_first(pl.cut(), i), cnt = piece_count(pl.cut(), items, i);
                            CHECK(first == seen && cnt >= 1 && cnt <= pl.items_per_piece);
                            CHECK(cnt * 2 * states <= eff || cnt == 1);
                            seen += cnt;
                        }
                        CHECK(seen == items);
                        CHECK(piece_count(pl.cut(), items, pl.pieces) <= 0);
                        CHECK(pl.scratch_rows == (steps >= 2 ? pl.items_per_piece * 2 * states : 0));
                        // the chunks cover steps-1 .. 0 once, in that order
                        if (steps == 0) {
                            CHECK(pl.launches == 1);
                            continue;
                        }
                        CHECK(pl.launches >= 1 && pl.steps_per_launch >= 1);
                        int32_t next = steps;
                        for (int32_t j = 0; j < pl.launches; j++) {
                            int32_t hi, lo;
                            automaton_launch_steps(pl, steps, j, &hi, &lo);
                            CHECK(hi == next && lo < hi && lo >= 0 && hi - lo <= pl.steps_per_launch);
                            if (k >= 1) CHECK(hi - lo <= k);
                            if (k < 1) CHECK((int64_t)(hi - lo) * automaton_rounds(states) <= kAutomatonLaunchRounds);
                            next = lo;
                        }
                        CHECK(next == 0);
                        if (k == 1) CHECK(pl.launches == steps);
                        if (k < 1 && (int64_t)steps * automaton_rounds(states) <= kAutomatonLaunchRounds) CHECK(pl.launches == 1);
                    }
    // nothing to run, or outside the interface: an empty plan
    CHECK(automaton_plan(0, 4, 4, 0, 0).pieces == 0 && automaton_plan(5, 0, 4, 0, 0).pieces == 0 && automaton_plan(5, 65, 4, 0, 0).pieces == 0);
    CHECK(automaton_plan(5, 4, -1, 0, 0).pieces == 0 && automaton_plan(5, 4, 4097, 0, 0).pieces == 0);
    // the figures the documents quote
    const AutomatonPlan big = automaton_plan(10, 64, 4096, 0, 0);
    CHECK(big.launches == 8 && big.steps_per_launch == 512 && big.items_per_piece == 10 && big.scratch_rows == 1280);
    CHECK(automaton_plan(1100, 5, 6, 0, 0).pieces == 2 && automaton_plan(1100, 5, 6, 0, 0).items_per_piece == 819);
    return 0;
}

int main() {
    if (refusals() || live_masks() || pieces_and_chunks()) return 1;
    std::printf("AUTOMATON_PLAN_OK\n");
    return 0;
}
