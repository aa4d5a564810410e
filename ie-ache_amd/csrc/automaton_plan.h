// Deterministic automata over words of TGSW-encrypted bits (automaton.hip; include/ieache.h section 3k): THE statement of
// what an automaton is -- its scalars, its tables and their refusal, which states are live at which step -- and of how a call
// is cut: items into pieces, steps into launches.  The C ABI (capi.cpp), the object (Cmux::automaton_create) and the evaluator
// loop by the answers; nothing else decides.  Free of HIP so that the CPU tests can check it (tests/native/automaton_plan_test.cpp).
//
// This call stands BESIDE the table of set_calls.h and is not a row of it: that table's calls are sized by (count, depth, steps,
// n_sets) alone, while this one's arguments are sized by an object made earlier (states, steps, n_out), its scalar refusals are
// the object's own, and the table is pinned at eight kinds.  What fits is reused: check_indices' messages, the staging slots,
// the overlap rule, the piece loop.
//
//   k_automaton_x1   one workgroup of kCmuxWaveRows waves per item, every step of a launch inside it: per step t = hi-1 .. lo
//                    wave w takes states w, w + 4, ..: V_t[q] = CMux(C_sel(i,t), V_{t+1}[next1[t][q]], V_{t+1}[next0[t][q]])
//   k_automaton_copy steps == 0: out[i][q] = finals[final_of[i]][q]
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "cmux_plan.h"

namespace ieache {

constexpr int32_t kAutomatonMaxStates = 64;    // IEACHE_AUTOMATON_MAX_STATES: a step's live set is one 64-bit word; 2 x 64 rows of 8 KB = 1 MB of scratch per item
constexpr int32_t kAutomatonMaxSteps = 4096;   // IEACHE_AUTOMATON_MAX_STEPS: what stays decodable for +-1/8 finals
// steps x rounds (a round: kCmuxWaveRows states of one step, one CMux per wave) of one launch at most.  A CMux of k_cmux_x1 takes
// some tens of microseconds, so 8 192 of them in sequence stay well under a second; 4 096 steps of 64 states are 8 such launches.
constexpr int64_t kAutomatonLaunchRounds = 8192;

inline int32_t automaton_rounds(int32_t states) { return (states + kCmuxWaveRows - 1) / kCmuxWaveRows; }

// The first rule the scalars or the tables (next0, next1: [steps][states], entries in [0, states)) break, as the message of the
// refusal, or empty.  The scalars first, then the entries in the order (step, state, next0 before next1).
inline std::string automaton_refusal(int64_t states, int64_t steps, int64_t n_out, const int32_t* next0, const int32_t* next1) {
    const std::string who = "automaton: ";
    if (states < 1 || states > kAutomatonMaxStates) return who + "states must lie in 1 .. 64";
    if (steps < 0 || steps > kAutomatonMaxSteps) return who + "steps must lie in 0 .. 4096";
    if (n_out < 1 || n_out > states) return who + "n_out must lie in 1 .. states";
    if (steps > 0 && (!next0 || !next1)) return who + "null transition table";
    for (int64_t t = 0; t < steps; t++)
        for (int64_t q = 0; q < states; q++)
            for (int which = 0; which < 2; which++) {
                const int32_t v = (which ? next1 : next0)[t * states + q];
                if (v < 0 || v >= states)
                    return who + "next" + std::to_string(which) + "[" + std::to_string(t) + "][" + std::to_string(q) + "] = " + std::to_string(v) +
                           " is outside [0, " + std::to_string(states) + ")";
            }
    return std::string();
}

// live[t], t = 0 .. steps: the states of V_t that the outputs depend on.  live_0 = [0, n_out); live_{t+1} = the image of live_t
// under both tables of step t.  V_t[q] is computed for q in live_t only (t < steps; V_steps is the finals).  Tables already
// accepted by automaton_refusal.  Returns the CMuxes per item: the live (t, q) whose two tables differ -- where they agree the
// CMux is exactly d0 (every digit of 0 is 0) and the kernel copies the row.
inline int64_t automaton_live(int32_t states, int32_t steps, int32_t n_out, const int32_t* next0, const int32_t* next1, uint64_t* live) {
    live[0] = n_out >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << n_out) - 1);
    int64_t cmuxes = 0;
    for (int32_t t = 0; t < steps; t++) {
        uint64_t image = 0;
        for (int32_t q = 0; q < states; q++) {
            if (!((live[t] >> q) & 1)) continue;
            const int32_t a = next0[(size_t)t * states + q], b = next1[(size_t)t * states + q];
            image |= ((uint64_t)1 << a) | ((uint64_t)1 << b);
            cmuxes += a != b;
        }
        live[t + 1] = image;
    }
    return cmuxes;
}

// How a call over `items` items is cut.
//   Pieces are runs of WHOLE items.  An item keeps its state vector in two buffers of `states` rows that swap roles from step to
//   step (steps < 2: none -- the one step reads the finals and writes the output), so a piece holds piece_rows / (2 states)
//   items within the cap "cmux_piece_rows"; an item wider than the cap (states = 64 at a cap below 128) is a piece of its own.
//   The steps of a piece run t = steps-1 .. 0 in `launches` consecutive launches of at most steps_per_launch steps that continue
//   in the same two buffers: option "automaton_steps_per_launch" k > 0 gives at most k steps per launch (1: a launch per step,
//   the hand-off a kernel boundary); 0, the default, everything in ONE launch unless steps x rounds exceeds
//   kAutomatonLaunchRounds, then the fewest equal chunks that do not.  steps == 0 is one copy launch.
struct AutomatonPlan {
    int64_t items_per_piece = 0, pieces = 0;
    int64_t scratch_rows = 0;       // rows of [2][N] words of the largest piece (the first): items_per_piece x 2 states, or 0
    int32_t steps_per_launch = 0;   // of every launch but perhaps the last
    int32_t launches = 0;           // per piece
    Cut cut() const { return {pieces, items_per_piece}; }  // of the items (cmux_plan.h)
};
// launch j = 0 .. launches-1 of a piece processes t = hi-1 down to lo: the chunks cover steps-1 .. 0 once, in that order
inline void automaton_launch_steps(const AutomatonPlan& pl, int32_t steps, int32_t j, int32_t* hi, int32_t* lo) {
    *hi = steps - j * pl.steps_per_launch;
    *lo = *hi - pl.steps_per_launch < 0 ? 0 : *hi - pl.steps_per_launch;
}

inline AutomatonPlan automaton_plan(int64_t items, int32_t states, int32_t steps, int64_t piece_rows_opt, int64_t steps_per_launch_opt) {
    AutomatonPlan pl;
    if (items <= 0 || states < 1 || states > kAutomatonMaxStates || steps < 0 || steps > kAutomatonMaxSteps) return pl;
    if (piece_rows_opt < 1 || piece_rows_opt > kCmuxPieceRowsMax) piece_rows_opt = kCmuxPieceRows;
    const int64_t per_item = 2 * (int64_t)states;
    pl.items_per_piece = piece_rows_opt / per_item < 1 ? 1 : piece_rows_opt / per_item;
    if (pl.items_per_piece > items) pl.items_per_piece = items;
    pl.pieces = (items + pl.items_per_piece - 1) / pl.items_per_piece;
    pl.scratch_rows = steps >= 2 ? pl.items_per_piece * per_item : 0;
    if (steps == 0) {
        pl.steps_per_launch = 0;
        pl.launches = 1;
        return pl;
    }
    int64_t k = steps_per_launch_opt;
    if (k < 1) {
        const int64_t work = (int64_t)steps * automaton_rounds(states);
        const int64_t chunks = (work + kAutomatonLaunchRounds - 1) / kAutomatonLaunchRounds;
        k = (steps + chunks - 1) / chunks;
    }
    if (k > steps) k = steps;
    pl.steps_per_launch = (int32_t)k;
    pl.launches = (int32_t)((steps + k - 1) / k);
    return pl;
}

}  // namespace ieache
