// CircuitCache (ie-ache_amd/csrc/circuit_cache.h) as plain host C++ under AddressSanitizer / UBSan: what it keeps, what it evicts
// and when, that an evicted circuit a caller still holds stays valid, and the selection rule -- base circuit, level cap for
// the batch, capped variant only where it differs from the base and came out balanced.  32- and 64-bit circuits only.
// `circuit_cache_test asap` runs the one case that needs IEACHE_SCHEDULE=asap (read once per process): a capped build that
// does not come out balanced.  Built and run by tests/test_circuit_cache_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../ie-ache_amd/csrc/circuit_cache.h"

using namespace ieache;

namespace {

#define REQUIRE(c)                                                              \
    do {                                                                        \
        if (!(c)) {                                                             \
            fprintf(stderr, "violated: %s (%s:%d)\n", #c, __FILE__, __LINE__); \
            return false;                                                       \
        }                                                                       \
    } while (0)

int32_t mean_width(const Circuit& c) { return (int32_t)((c.n_bootstraps + c.depth - 1) / c.depth); }

bool keeps_and_evicts() {
    CircuitCache cache(3);
    const CircuitCache::Ptr base = cache.fetch(CIRC_MUL, 32, false, 0);
    REQUIRE(base && base->name == "mul32" && !base->balanced_schedule);
    REQUIRE(cache.fetch(CIRC_MUL, 32, false, 0) == base);
    const CircuitCache::Ptr c32 = cache.fetch(CIRC_MUL, 32, false, 32), c35 = cache.fetch(CIRC_MUL, 32, false, 35), c40 = cache.fetch(CIRC_MUL, 32, false, 40);
    REQUIRE(c32 && c35 && c40 && c32 != c35 && c35 != c40 && c32 != base && c32->balanced_schedule);
    // three variants are kept, in whatever order they are asked for again
    REQUIRE(cache.fetch(CIRC_MUL, 32, false, 40) == c40 && cache.fetch(CIRC_MUL, 32, false, 35) == c35 && cache.fetch(CIRC_MUL, 32, false, 32) == c32);
    // ... so 40 is now the least recently USED, though 32 is the oldest built: a fourth variant evicts 40
    const Circuit* const c40_was = c40.get();
    const int32_t c40_levels = c40->n_levels();
    const CircuitCache::Ptr c48 = cache.fetch(CIRC_MUL, 32, false, 48);
    REQUIRE(c48 && cache.fetch(CIRC_MUL, 32, false, 32) == c32 && cache.fetch(CIRC_MUL, 32, false, 35) == c35 && cache.fetch(CIRC_MUL, 32, false, 48) == c48);
    // the evicted circuit, still held here, is untouched (under ASan: still allocated)
    REQUIRE(c40.use_count() == 1 && c40.get() == c40_was && c40->n_levels() == c40_levels && c40->gates.size() == base->gates.size());
    const CircuitCache::Ptr c40_again = cache.fetch(CIRC_MUL, 32, false, 40);  // rebuilt: another object, the same circuit; evicts 32
    REQUIRE(c40_again && c40_again != c40 && c40_again->n_levels() == c40_levels);
    REQUIRE(c32.use_count() == 1 && c35.use_count() == 2 && c48.use_count() == 2);
    // the base is never evicted, and the variants of another (kind, bits, fold) are counted apart
    REQUIRE(cache.fetch(CIRC_MUL, 32, false, 0) == base);
    const CircuitCache::Ptr folded = cache.fetch(CIRC_MUL, 32, true, 35), wide = cache.fetch(CIRC_MUL, 64, false, 64);
    REQUIRE(folded && wide && folded->name == "mul32_folded" && wide->name == "mul64");
    REQUIRE(c35.use_count() == 2 && c48.use_count() == 2 && c40_again.use_count() == 2);
    return true;
}

bool capacity_one_replaces() {
    CircuitCache cache(1);
    const CircuitCache::Ptr base = cache.fetch(CIRC_MUL, 32, false, 0), c35 = cache.fetch(CIRC_MUL, 32, false, 35);
    REQUIRE(base && c35 && cache.fetch(CIRC_MUL, 32, false, 35) == c35);
    REQUIRE(c35.use_count() == 2);
    const CircuitCache::Ptr c32 = cache.fetch(CIRC_MUL, 32, false, 32);
    REQUIRE(c32 && c35.use_count() == 1 && c32.use_count() == 2 && cache.fetch(CIRC_MUL, 32, false, 32) == c32);
    REQUIRE(c35->name == "mul32" && cache.fetch(CIRC_MUL, 32, false, 0) == base);
    return true;
}

bool unsupported_is_null() {
    CircuitCache cache(3);
    REQUIRE(!cache.fetch(CIRC_MUL, 16, false, 0) && !cache.fetch(CIRC_MUL, 16, false, 35) && !cache.fetch(10, 32, false, 0) && !cache.fetch(CIRC_ADD, 257, true, 0));
    REQUIRE(!cache.select(CIRC_MUL, 16, false, 32, 2048, 1024, true) && !cache.select(0, 32, false, 32, 2048, 1024, true, 35));
    // nothing was cached for them: a supported circuit asked for next is the first entry and is built once
    const CircuitCache::Ptr add = cache.fetch(CIRC_ADD, 16, false, 0);
    REQUIRE(add && add.use_count() == 2 && cache.fetch(CIRC_ADD, 16, false, 0) == add);
    return true;
}

bool selects() {
    CircuitCache cache(3);
    const CircuitCache::Ptr mul32 = cache.fetch(CIRC_MUL, 32, false, 0), mul64 = cache.fetch(CIRC_MUL, 64, false, 0);
    REQUIRE(mul32 && mul64 && !mul32->balanced_schedule && mul64->balanced_schedule);
    // level_quantum off: the base, whatever the batch
    REQUIRE(cache.select(CIRC_MUL, 64, false, 32, 2048, 1024, false) == mul64 && cache.select(CIRC_MUL, 32, false, 58, 2048, 1024, false) == mul32);
    // cap 0: a batch that fills whole rounds (balanced rule), an adder (round rule)
    REQUIRE(circuit_level_cap(*mul64, 2048, 2048, 1024) == 0 && cache.select(CIRC_MUL, 64, false, 2048, 2048, 1024, true) == mul64);
    const CircuitCache::Ptr add = cache.select(CIRC_ADD, 32, false, 58, 2048, 1024, true);
    REQUIRE(add && add == cache.fetch(CIRC_ADD, 32, false, 0) && circuit_level_cap(*add, 58, 2048, 1024) == 0);
    // cap == the mean width of a balanced base: the base, and no variant is built (it would be the same circuit)
    // (4 expressions on 4 x mean resident gates: one level of mean gates is exactly one round)
    const int32_t mean = mean_width(*mul64);
    REQUIRE(circuit_level_cap(*mul64, 4, 4 * mean, 0) == mean);
    REQUIRE(cache.select(CIRC_MUL, 64, false, 4, 4 * mean, 0, true) == mul64);
    const CircuitCache::Ptr at_mean = cache.fetch(CIRC_MUL, 64, false, mean);  // built now, for the first time
    REQUIRE(at_mean && at_mean.use_count() == 2 && at_mean != mul64);
    REQUIRE(at_mean->n_levels() == mul64->n_levels() && at_mean->n_slots == mul64->n_slots && at_mean->level_offset == mul64->level_offset);
    // the capped variants tests/test_gpu_parity.py::test_batch_aware_level_width_same_bits evaluates
    const CircuitCache::Ptr m64 = cache.select(CIRC_MUL, 64, false, 32, 2048, 1024, true);
    REQUIRE(m64 && m64 != mul64 && m64 == cache.fetch(CIRC_MUL, 64, false, 64) && m64->balanced_schedule && m64->n_levels() > 449);
    REQUIRE(cache.select(CIRC_MUL, 64, false, 32, 2048, 1024, true) == m64);
    const CircuitCache::Ptr m32 = cache.select(CIRC_MUL, 32, false, 58, 2048, 1024, true);
    REQUIRE(m32 && m32 != mul32 && m32 == cache.fetch(CIRC_MUL, 32, false, 35) && m32->balanced_schedule && m32->n_levels() == 334);
    // a forced cap wins over everything, level_quantum off included
    REQUIRE(cache.select(CIRC_MUL, 32, false, 4096, 2048, 1024, false, 35) == m32);
    return true;
}

// IEACHE_SCHEDULE=asap: no circuit is balanced, so a capped build of mul32 comes out ASAP and is not used
bool unbalanced_capped_build_is_not_used() {
    CircuitCache cache(3);
    const CircuitCache::Ptr mul32 = cache.fetch(CIRC_MUL, 32, false, 0);
    REQUIRE(mul32 && !mul32->balanced_schedule && circuit_level_cap(*mul32, 58, 2048, 1024) == 35);
    const CircuitCache::Ptr capped = cache.fetch(CIRC_MUL, 32, false, 35);
    REQUIRE(capped && capped != mul32 && !capped->balanced_schedule);
    REQUIRE(cache.select(CIRC_MUL, 32, false, 58, 2048, 1024, true) == mul32);
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "asap")) {
        setenv("IEACHE_SCHEDULE", "asap", 1);
        if (!unbalanced_capped_build_is_not_used()) return 1;
        printf("CIRCUIT_CACHE_ASAP_OK\n");
        return 0;
    }
    unsetenv("IEACHE_SCHEDULE");
    if (!keeps_and_evicts() || !capacity_one_replaces() || !unsupported_is_null() || !selects()) return 1;
    printf("CIRCUIT_CACHE_OK\n");
    return 0;
}
