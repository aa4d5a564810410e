// The arithmetic of a joint evaluation (ie-ache_amd/csrc/joint_plan.h) over thousands of random job lists -- with and
// without MUX levels, odd chunk values, parts of one item, level halves on two lanes -- as plain host C++ under
// AddressSanitizer / UBSan, and the slicing of a job list over a device group (group_run.h: shard_jobs) for the Python test
// to compare with ieache_shard_slice.  The executor's piece loop (evaluator.hip: run_joint_items) uses exactly these
// functions; a mistake here would be a stray store on the GPU.  Built and run by tests/test_joint_plan_cpu.py.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../ie-ache_amd/csrc/group_run.h"
#include "../../ie-ache_amd/csrc/joint_plan.h"

using namespace ieache;

#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) {                                                              \
            fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                            \
        }                                                                        \
    } while (0)

struct Jobs {
    std::vector<std::vector<int32_t>> ng, nm;
    std::vector<JointJob> plan;
};

static Jobs random_jobs(std::mt19937_64& rng, bool with_mux) {
    Jobs J;
    const size_t n = 1 + rng() % 5;
    J.ng.resize(n);
    J.nm.resize(n);
    for (size_t j = 0; j < n; j++) {
        const int32_t levels = (int32_t)(rng() % 6);  // 0: a circuit without gates
        for (int32_t L = 0; L < levels; L++) {
            const int32_t ng = 1 + (int32_t)(rng() % 6);
            J.ng[j].push_back(ng);
            J.nm[j].push_back(with_mux && rng() % 2 ? (int32_t)(rng() % (uint64_t)(ng + 1)) : 0);
        }
        const int64_t batch = rng() % 7 == 0 ? 0 : 1 + (int64_t)(rng() % 5);  // empty batches among the others
        J.plan.push_back(JointJob{levels, J.ng[j].data(), with_mux || rng() % 2 ? J.nm[j].data() : nullptr, batch});
    }
    return J;
}

// one step under one plan: the pieces tile the joint items, respect every part's gate boundaries, cover the parts in order,
// and stay within what joint_step_needs reserved
static int check_step(const std::vector<JointPart>& parts, const JointLevelPlan& pl, const JointNeeds& needs) {
    const size_t n = parts.size();
    const int64_t items = joint_items(parts.data(), n);
    std::vector<int> hits((size_t)items, 0);
    size_t next_part = 0;       // parts before it are wholly covered
    int64_t next_local = 0;     // items of parts[next_part] covered so far
    int k = 0;
    for (int64_t done = 0, cnt = 0; done < items; done += cnt, k++) {
        cnt = joint_piece_items(parts.data(), n, done, pl.piece);
        CHECK(cnt >= 1 && cnt <= pl.piece + 1 && cnt <= items - done);
        const int lane = pl.two_lanes ? (k & 1) : 0;
        CHECK((size_t)cnt <= needs.items[lane]);
        int64_t row = 0, comb_rows = 0;
        for (size_t i = 0; i < n; i++) {
            const JointShare sh = joint_share(parts.data(), i, done, cnt);
            if (!sh.cnt) continue;
            const JointPart& p = parts[i];
            // in order, nothing skipped: the share continues where the part was left
            CHECK(i == next_part && sh.local0 == next_local);
            CHECK(sh.local0 + sh.cnt <= p.items);
            // no piece begins or ends inside a MUX
            CHECK(level_gate_boundary(sh.local0, p.ng, p.nm) && level_gate_boundary(sh.local0 + sh.cnt, p.ng, p.nm));
            const int64_t g0 = level_gates_before(sh.local0, p.ng, p.nm), g1 = level_gates_before(sh.local0 + sh.cnt, p.ng, p.nm);
            CHECK(g1 > g0 && g1 - g0 <= sh.cnt && g1 <= p.gates);
            // every gate's rows lie inside the share's rows of ext
            for (int64_t q = g0; q < g1; q++) {
                const int64_t r = level_first_item(q, p.ng, p.nm) - sh.local0;
                CHECK(r >= 0 && r + ((q % p.ng) >= p.ng - p.nm ? 1 : 0) < sh.cnt);
            }
            if (p.nm > 0) comb_rows += g1 - g0;
            // joint item -> (part, local) agrees with the share
            for (int64_t t = 0; t < sh.cnt; t++) {
                const JointAt at = joint_locate(parts.data(), n, done + row + t);
                CHECK(at.part == i && at.local == sh.local0 + t);
                hits[(size_t)(done + row + t)]++;
            }
            row += sh.cnt;
            next_local += sh.cnt;
            if (next_local == p.items) {
                next_part++;
                next_local = 0;
            }
        }
        CHECK(row == cnt);
        CHECK((size_t)comb_rows <= needs.comb[lane]);
    }
    CHECK(next_part == n && next_local == 0);
    for (int64_t t = 0; t < items; t++) CHECK(hits[(size_t)t] == 1);  // every item in exactly one piece
    const JointAt end = joint_locate(parts.data(), n, items);
    CHECK(end.part == n && end.local == 0);
    return 0;
}

static int check_jobs(const Jobs& J, int64_t chunk, bool halves, int64_t overlap_min) {
    const size_t n_jobs = J.plan.size();
    const int32_t steps = joint_steps(J.plan.data(), n_jobs);
    int32_t deepest = 0;
    for (const JointJob& j : J.plan)
        if (j.batch > 0 && j.n_levels > deepest) deepest = j.n_levels;
    CHECK(steps == deepest);
    // the needs of the whole evaluation first, as prepare_jobs takes them; then every step against them
    JointNeeds needs;
    std::vector<std::vector<JointPart>> step_parts((size_t)steps);
    std::vector<JointLevelPlan> plans;
    for (int32_t s = 1; s <= steps; s++) {
        std::vector<JointPart> parts(n_jobs);
        parts.resize(joint_step_parts(J.plan.data(), n_jobs, s, parts.data()));
        // step -> parts: every job that still has a level, in order, with its own counts
        size_t at = 0;
        for (size_t j = 0; j < n_jobs; j++) {
            const JointJob& job = J.plan[j];
            if (job.batch <= 0 || s > job.n_levels) continue;
            CHECK(at < parts.size() && parts[at].job == (int32_t)j);
            const int32_t nm = job.level_nm ? job.level_nm[s - 1] : 0;
            CHECK(parts[at].ng == job.level_ng[s - 1] && parts[at].nm == nm);
            CHECK(parts[at].items == (int64_t)(parts[at].ng + nm) * job.batch && parts[at].gates == (int64_t)parts[at].ng * job.batch);
            at++;
        }
        CHECK(at == parts.size());
        const JointLevelPlan pl = joint_level_plan(std::max<int64_t>(joint_items(parts.data(), parts.size()), 1), chunk, halves, overlap_min);
        CHECK(pl.piece >= 1 && pl.piece <= chunk);
        joint_step_needs(parts.data(), parts.size(), pl, &needs);
        step_parts[(size_t)s - 1] = parts;
        plans.push_back(pl);
    }
    for (int32_t s = 1; s <= steps; s++)
        if (check_step(step_parts[(size_t)s - 1], plans[(size_t)s - 1], needs)) return 1;
    // scratch is sized for one item more than the chunk at most
    CHECK(needs.items[0] <= (size_t)chunk + 1 && needs.items[1] <= needs.items[0] && needs.comb[0] <= needs.items[0] && needs.comb[1] <= needs.items[0]);
    return 0;
}

// the daemon's rule: a group joins exactly when its mean level is under pipe_min; a round joins from two such groups on
static int check_rule() {
    CHECK(joint_group_joins(/*rotations=*/100, /*levels=*/10, /*batch=*/8, /*pipe_min=*/81));   // mean level 80
    CHECK(!joint_group_joins(100, 10, 8, 80));
    CHECK(!joint_group_joins(100, 10, 8, 79));
    CHECK(!joint_group_joins(100, 0, 8, 1000) && !joint_group_joins(100, 10, 0, 1000));
    CHECK(!joint_round_joins(0) && !joint_round_joins(1) && joint_round_joins(2) && joint_round_joins(5));
    return 0;
}

struct Job {  // the fields shard_jobs reads of an ieache_job
    size_t batch;
    const int32_t* in_lwe;
    int32_t* out_lwe;
};

// --slices: "job_batch parts part first count" per job a member keeps, for the comparison with ieache_shard_slice
static int print_slices() {
    static int32_t in[1], out[1];
    for (size_t parts = 1; parts <= 5; parts++) {
        const std::vector<size_t> batches = {5, 1, 0, 7, parts, 2 * parts + 1};
        std::vector<Job> jobs;
        std::vector<size_t> in_words, out_words;
        for (size_t j = 0; j < batches.size(); j++) {
            jobs.push_back(Job{batches[j], in, out});
            in_words.push_back(3 + j);
            out_words.push_back(2 + 2 * j);
        }
        for (size_t part = 0; part < parts; part++) {
            std::vector<Job> mine;
            shard_jobs(jobs.data(), jobs.size(), in_words.data(), out_words.data(), parts, part, &mine);
            size_t at = 0;
            for (size_t j = 0; j < jobs.size(); j++) {
                size_t first = 0, count = 0;
                shard_slice(batches[j], parts, part, &first, &count);
                if (!count) continue;  // dropped
                CHECK(at < mine.size() && mine[at].batch == count);
                // the rows start `first` expressions in, in the job's own row widths
                CHECK(mine[at].in_lwe == in + first * in_words[j] && mine[at].out_lwe == out + first * out_words[j]);
                printf("%zu %zu %zu %zu %zu\n", batches[j], parts, part, (size_t)(mine[at].in_lwe - in) / in_words[j], mine[at].batch);
                at++;
            }
            CHECK(at == mine.size());
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "--slices")) return print_slices();
    if (check_rule()) return 1;
    std::mt19937_64 rng(20260419);
    int lists = 0;
    for (int round = 0; round < 1500; round++) {
        const bool with_mux = round % 2 == 1;
        const Jobs J = random_jobs(rng, with_mux);
        // odd and even chunks, 1 among them; with and without level halves, from a low threshold so that small steps fork
        const int64_t chunks[] = {1, 2, 3, 7, 8, 1 + (int64_t)(rng() % 40), 1 << 20};
        for (const int64_t chunk : chunks)
            for (int halves = 0; halves < 2; halves++) {
                if (check_jobs(J, chunk, halves != 0, halves ? 2 + (int64_t)(rng() % 12) : 0)) {
                    fprintf(stderr, "round %d chunk %lld halves %d\n", round, (long long)chunk, halves);
                    return 1;
                }
                lists++;
            }
    }
    // parts of one item next to a MUX part, by hand: chunk 2 must not split the MUX
    {
        const int32_t ng_a[1] = {1}, ng_b[1] = {1}, nm_b[1] = {1};
        const JointJob jobs[2] = {{1, ng_a, nullptr, 1}, {1, ng_b, nm_b, 1}};
        JointPart parts[2];
        CHECK(joint_step_parts(jobs, 2, 1, parts) == 2 && joint_items(parts, 2) == 3);
        CHECK(joint_piece_items(parts, 2, 0, 1) == 1);  // ends between the parts
        CHECK(joint_piece_items(parts, 2, 0, 2) == 3);  // would end inside the MUX: takes its second rotation as well
        CHECK(joint_piece_items(parts, 2, 1, 1) == 2);
    }
    printf("JOINT_PLAN_OK %d job lists\n", lists);
    return 0;
}
