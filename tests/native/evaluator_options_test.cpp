// The evaluator's option table (ie-ache_amd/csrc/evaluator_options.h) and the scoped-assignment guard
// (scoped_set.h), as plain host C++ under AddressSanitizer / UBSan: what Evaluator::set_option, get_option and the
// environment pass of a new context do is these loops with a hook that knows the device.
// Built and run by tests/test_evaluator_options_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <stdexcept>
#include <string>

#include "../../ie-ache_amd/csrc/evaluator_options.h"
#include "../../ie-ache_amd/csrc/scoped_set.h"

using namespace ieache;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                   \
        }                                                               \
    } while (0)

static bool any(const OptionRow&, int64_t&) { return true; }

static int check_table() {
    std::set<std::string> names, envs;
    int writable = 0, figures = 0;
    for (const OptionRow& r : kOptionTable) {
        CHECK(r.name && *r.name && r.at && r.doc && *r.doc);
        CHECK(names.insert(r.name).second);
        CHECK(find_option(r.name) == &r);
        if (r.env) CHECK(std::string(r.env).rfind("IEACHE_", 0) == 0 && envs.insert(r.env).second);
        EvalOptions o;
        const int64_t before = o.*r.at;  // every row reads
        if (r.lo > r.hi) {               // a read-only figure: refuses any set, has no environment variable
            figures++;
            CHECK(!r.env && !option_set(o, r, 0, any) && !option_set(o, r, 1, any) && !option_set(o, r, before, any));
            CHECK(o.*r.at == before);
            continue;
        }
        writable++;
        // its bounds are accepted and stored, one past them refused and the value kept
        CHECK(option_set(o, r, r.lo, any) && o.*r.at == r.lo);
        CHECK(option_set(o, r, r.hi, any) && o.*r.at == r.hi);
        if (r.lo > INT64_MIN) CHECK(!option_set(o, r, r.lo - 1, any) && o.*r.at == r.hi);
        if (r.hi < INT64_MAX) CHECK(!option_set(o, r, r.hi + 1, any) && o.*r.at == r.hi);
        // a hook that refuses keeps the value too
        CHECK(!option_set(o, r, r.lo, [](const OptionRow&, int64_t&) { return false; }) && o.*r.at == r.hi);
    }
    CHECK(writable >= 30 && figures == 7 && !find_option("no_such_option"));
    // validators inside a range
    EvalOptions o;
    CHECK(option_set(o, *find_option("ks_gates"), 16, any) && !option_set(o, *find_option("ks_gates"), 12, any) && o.ks_gates == 16);
    CHECK(option_set(o, *find_option("ks_mfma_split"), 8, any) && !option_set(o, *find_option("ks_mfma_split"), 6, any));
    CHECK(option_set(o, *find_option("mix_k"), 3, any) && !option_set(o, *find_option("mix_k"), 1, any) && o.mix_k == 3);
    // rejections the GPU suite pins through ieache_ctx_set_option
    CHECK(!option_set(o, *find_option("pipe_lanes"), 1, any) && !option_set(o, *find_option("pipe_lanes"), 5, any));
    CHECK(!option_set(o, *find_option("overlap"), 2, any) && !option_set(o, *find_option("overlap_min"), 1, any));
    // a hook may normalise what is stored
    CHECK(option_set(o, *find_option("force_generic"), 7, [](const OptionRow&, int64_t& v) { v = v != 0; return true; }) && o.force_generic == 1);
    return 0;
}

static int check_environment() {
    for (const OptionRow& r : kOptionTable)
        if (r.env) unsetenv(r.env);
    EvalOptions o;
    o.pipe_min = 2048;  // as Evaluator::init() does before the pass: defaults by CU count
    const EvalOptions defaults = o;
    options_from_environment(o, any);
    for (const OptionRow& r : kOptionTable) CHECK(o.*r.at == defaults.*r.at);
    for (const OptionRow& r : kOptionTable) {
        if (!r.env) continue;
        char buf[32];
        snprintf(buf, sizeof buf, "%lld", (long long)r.lo);
        setenv(r.env, buf, 1);  // in range: applied
        options_from_environment(o, any);
        CHECK(o.*r.at == r.lo);
        o.*r.at = defaults.*r.at;
        snprintf(buf, sizeof buf, "%lld", (long long)r.lo - 1);
        setenv(r.env, buf, 1);  // out of range: ignored, the default stays
        options_from_environment(o, any);
        CHECK(o.*r.at == defaults.*r.at);
        unsetenv(r.env);
    }
    setenv("IEACHE_PIPE_MIN", "-5", 1);
    setenv("IEACHE_FFT_AUDIT", "-1", 1);
    setenv("IEACHE_PIPE_LANES", "3", 1);
    options_from_environment(o, any);
    CHECK(o.pipe_min == 2048 && o.fft_audit == 64 && o.pipe_lanes == 3);
    return 0;
}

static int check_scoped_set() {
    int concurrency = 1;
    bool exact = false;
    {
        ScopedSet<int> a(concurrency, 3);
        CHECK(concurrency == 3);
        {
            ScopedSet<int> b(concurrency, 2);
            CHECK(concurrency == 2);
        }
        CHECK(concurrency == 3);
    }
    CHECK(concurrency == 1);
    try {
        ScopedSet<bool> e(exact, true);
        ScopedSet<int> c(concurrency, 4);
        if (exact && concurrency == 4) throw std::runtime_error("a launch failed");
        CHECK(false);
    } catch (const std::runtime_error&) {
        CHECK(!exact && concurrency == 1);
    }
    return 0;
}

int main() {
    if (check_table() || check_environment() || check_scoped_set()) return 1;
    printf("EVALUATOR_OPTIONS_OK\n");
    return 0;
}
