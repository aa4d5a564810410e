// The arithmetic of a JOINT evaluation -- several circuits' batches evaluated together, level by level (evaluator.hip:
// eval_jobs_device, run_joint_items) -- free of any device state so that the CPU tests can check it over random job lists
// (tests/native/joint_plan_test.cpp).
//
// A job is a circuit over a batch of its own.  Step s = 1, 2, ... of a joint evaluation runs level s of every job that still
// has one; a job's share of a step is a PART: the rotation items of its level over its batch ((ng + nm) x batch of them,
// level_items.h), numbered from 0 within the part.  The step's JOINT ITEMS are the parts' items one after another, jobs in
// their order.  Pieces (one blind-rotation launch each) are runs of consecutive joint items; they may begin and end inside a
// part, but only at a gate boundary of that part, so that both rotations of a MUX are in the same piece.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "level_items.h"

namespace ieache {

// A job as the plan sees it: its levels' gate and MUX counts per expression, and its batch.
struct JointJob {
    int32_t n_levels;
    const int32_t* level_ng;  // [n_levels]: gates of level L = index + 1, per expression
    const int32_t* level_nm;  // [n_levels]: how many of them are MUX (null: none anywhere)
    int64_t batch;
};

// One job's share of a step.
struct JointPart {
    int32_t job;    // index into the job list
    int32_t ng, nm;
    int64_t items;  // rotation items: (ng + nm) x batch
    int64_t gates;  // gate instances: ng x batch -- rows after the combine, rows the key switch takes
};

// steps of a joint evaluation: the deepest job's depth (jobs with an empty batch do not count)
inline int32_t joint_steps(const JointJob* jobs, size_t n_jobs) {
    int32_t s = 0;
    for (size_t j = 0; j < n_jobs; j++)
        if (jobs[j].batch > 0) s = std::max(s, jobs[j].n_levels);
    return s;
}

// step (1-based) -> its parts, jobs in their order, into out[n_jobs]; returns how many.  A job that has finished, has an
// empty batch or an empty level contributes none.
inline size_t joint_step_parts(const JointJob* jobs, size_t n_jobs, int32_t step, JointPart* out) {
    size_t n = 0;
    for (size_t j = 0; j < n_jobs; j++) {
        const JointJob& job = jobs[j];
        if (job.batch <= 0 || step < 1 || step > job.n_levels) continue;
        const int32_t ng = job.level_ng[step - 1], nm = job.level_nm ? job.level_nm[step - 1] : 0;
        if (ng <= 0) continue;
        out[n++] = JointPart{(int32_t)j, ng, nm, ((int64_t)ng + nm) * job.batch, (int64_t)ng * job.batch};
    }
    return n;
}

inline int64_t joint_items(const JointPart* parts, size_t n_parts) {
    int64_t t = 0;
    for (size_t i = 0; i < n_parts; i++) t += parts[i].items;
    return t;
}
inline int64_t joint_gates(const JointPart* parts, size_t n_parts) {
    int64_t t = 0;
    for (size_t i = 0; i < n_parts; i++) t += parts[i].gates;
    return t;
}

// joint item -> (part, item within the part).  item == the joint item count: (n_parts, 0).
struct JointAt {
    size_t part;
    int64_t local;
};
inline JointAt joint_locate(const JointPart* parts, size_t n_parts, int64_t item) {
    size_t i = 0;
    while (i < n_parts && item >= parts[i].items) item -= parts[i++].items;
    return JointAt{i, i < n_parts ? item : 0};
}

// THE PIECE-CUT RULE of a joint step: level_piece_items' rule applied within the part the cut falls in.  A piece starts at
// joint item `first` (a gate boundary of its part) and may hold `want` (>= 1) of the items that remain; it ends at the next
// gate boundary at or after first + want.  A part's first item is a gate boundary, so a cut between two parts stands.  A
// piece therefore holds at most want + 1 items and never 0.
inline int64_t joint_piece_items(const JointPart* parts, size_t n_parts, int64_t first, int64_t want) {
    const int64_t left = joint_items(parts, n_parts) - first;
    if (want >= left) return left;
    const JointAt at = joint_locate(parts, n_parts, first + want);
    const JointPart& p = parts[at.part];
    return level_gate_boundary(at.local, p.ng, p.nm) ? want : want + 1;
}

// The share of part `i` inside the piece [first, first + cnt) of joint items: its first item within the part and how many
// (0: the piece does not touch the part).
struct JointShare {
    int64_t local0, cnt;
};
inline JointShare joint_share(const JointPart* parts, size_t i, int64_t first, int64_t cnt) {
    int64_t start = 0;
    for (size_t q = 0; q < i; q++) start += parts[q].items;
    const int64_t lo = std::max(first, start), hi = std::min(first + cnt, start + parts[i].items);
    return hi > lo ? JointShare{lo - start, hi - lo} : JointShare{0, 0};
}

// How a step of `items` joint items is issued (evaluator.hip: plan_level, which decides the same from the evaluator's
// options): on one lane in pieces of at most `piece`, or the halves of the step alternating between two lanes.
struct JointLevelPlan {
    bool two_lanes;
    int64_t piece;
};
// halves_allowed: "overlap" on, the 64-lane kernels in use and nothing else running side by side
inline JointLevelPlan joint_level_plan(int64_t items, int64_t chunk, bool halves_allowed, int64_t overlap_min) {
    JointLevelPlan pl{false, chunk};
    if (halves_allowed && items >= overlap_min && items >= 2) {
        const int64_t half = (((items + 1) / 2) + 3) & ~(int64_t)3;
        if (std::min(chunk, half) < items) {
            pl.two_lanes = true;
            pl.piece = std::min(chunk, half);
        }
    }
    return pl;
}

// Scratch of a joint evaluation, grown step by step: rows of extracted samples (rotation items) and combined rows (gates of a
// piece that holds MUX gates) per lane.  Pieces alternate between the lanes from lane 0, so lane 1 never holds more than
// lane 0's widest piece nor more than what is left after the first piece.
struct JointNeeds {
    size_t items[2] = {1, 0};
    size_t comb[2] = {0, 0};
};
inline void joint_step_needs(const JointPart* parts, size_t n_parts, const JointLevelPlan& pl, JointNeeds* needs) {
    const int64_t items = std::max<int64_t>(joint_items(parts, n_parts), 1), gates = joint_gates(parts, n_parts);
    bool mux = false;
    for (size_t i = 0; i < n_parts; i++) mux = mux || parts[i].nm > 0;
    const size_t piece = (size_t)std::min<int64_t>(pl.piece + (mux ? 1 : 0), items);
    needs->items[0] = std::max(needs->items[0], piece);
    // a combined row per gate of every part of the piece that has MUX gates: never more than the piece has items
    if (mux) needs->comb[0] = std::max(needs->comb[0], std::min<size_t>(piece, (size_t)gates));
    if (pl.two_lanes) {
        const size_t rest = std::min<size_t>(piece, (size_t)(items - pl.piece));
        needs->items[1] = std::max(needs->items[1], rest);
        if (mux) needs->comb[1] = std::max(needs->comb[1], std::min<size_t>(rest, (size_t)gates));
    }
}

// WHEN THE DAEMON JOINS (csrc/daemon.cpp; ieache_eval_jobs itself always joins -- there it is the caller's decision).
// A round's requests fall into circuit groups, one per (kind, width, folding).  A group whose own mean level holds at least
// `pipe_min` rotation items (the evaluator's "pipe_min", 8 per CU by default) runs as expression pipelines when evaluated
// alone and fills its launches by itself: joining it gains nothing and costs it the pipelines.  So: a group takes part in the
// joint call when its mean level -- rotations x batch / levels -- is UNDER pipe_min, and the round is joint when at least two
// groups take part; the others are evaluated alone, as before.
// Measurement behind the rule (profiles/jobs_rates.txt, scripts/jobs_rates.py; n = 630, 256 CUs, pipe_min = 2 048): groups
// with mean levels of 353 rotation items and less -- mul32 x 8, mul64 x 4, muladd64 x 4, add32 / sub32 x 8, add32 x 64 --
// joined in 0.58 .. 0.85 of their sequential time; mul32 x 64 (mean level 2 827) joined with add32 x 64 took 1.066 of it,
// fifteen times the spread, and the rule keeps it out.  Nothing between 353 and 2 827 has been measured: the threshold is the one
// the single-circuit path already uses to call a batch wide (profiles/r5_overlap_ab.txt), not a fitted value.
inline bool joint_group_joins(int64_t rotations_per_expression, int32_t n_levels, int64_t batch, int64_t pipe_min) {
    if (n_levels < 1 || batch < 1) return false;
    return rotations_per_expression * batch < pipe_min * (int64_t)n_levels;
}
inline bool joint_round_joins(size_t joining_groups) { return joining_groups >= 2; }

}  // namespace ieache
