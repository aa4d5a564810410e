// The runner behind a device group's calls and the daemon's sharding (ie-ache_amd/csrc/group_run.h), as plain host C++
// under AddressSanitizer + UBSan and, in a second build, ThreadSanitizer: slices, one call per non-empty part, the calling
// thread for part 0, the lowest-numbered exception after every part has finished, and the inline path of a part whose
// thread cannot be had.  `--slices` prints "total parts part first count" for every slice (the Python side compares them
// with ieache_shard_slice).  Built and run by tests/test_group_run_cpu.py.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../ie-ache_amd/csrc/group_run.h"

using namespace ieache;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                   \
        }                                                               \
    } while (0)

constexpr size_t kMaxTotal = 40, kMaxParts = 9;

struct Seen {
    int calls = 0;
    size_t first = 0, count = 0;
    std::thread::id thread;
};

// a spawn that has no thread for the parts named in `refuse`
struct Refusing {
    std::vector<size_t> refuse;
    std::atomic<int>* refused;
    template <class Body>
    std::thread operator()(size_t part, Body&& body) const {
        for (size_t r : refuse)
            if (r == part) {
                ++*refused;
                throw std::system_error(std::make_error_code(std::errc::resource_unavailable_try_again), "no thread to be had");
            }
        return std::thread(std::forward<Body>(body));
    }
};

// every (total, parts): the slices tile [0, total) in order, each non-empty part is called once with its slice, empty
// parts never, part 0 on the calling thread.  `spawn` decides which parts get a thread.
template <class Spawn>
static int sweep(Spawn spawn, bool others_on_threads) {
    for (size_t total = 0; total <= kMaxTotal; total++)
        for (size_t parts = 1; parts <= kMaxParts; parts++) {
            std::vector<Seen> seen(parts);
            std::vector<int> rows(total, 0);  // rows[i]: parts that were given row i
            run_sliced(parts, total, [&](size_t m, size_t first, size_t count) {
                seen[m].calls++;
                seen[m].first = first;
                seen[m].count = count;
                seen[m].thread = std::this_thread::get_id();
                for (size_t i = first; i < first + count; i++) rows[i]++;  // slices are disjoint: no two parts write one row
            }, spawn);
            size_t next = 0;
            for (size_t m = 0; m < parts; m++) {
                const size_t base = total / parts, extra = total % parts;  // the rule, written out a second time
                const size_t want_first = m * base + (m < extra ? m : extra), want_count = base + (m < extra ? 1 : 0);
                size_t first = 0, count = 0;
                shard_slice(total, parts, m, &first, &count);
                CHECK(first == want_first && count == want_count && first == next);
                next += count;
                CHECK(seen[m].calls == (count ? 1 : 0));
                if (!count) continue;
                CHECK(seen[m].first == first && seen[m].count == count);
                if (m == 0) CHECK(seen[m].thread == std::this_thread::get_id());
                if (m > 0 && others_on_threads) CHECK(seen[m].thread != std::this_thread::get_id());
            }
            CHECK(next == total);
            for (size_t i = 0; i < total; i++) CHECK(rows[i] == 1);
        }
    return 0;
}

// parts 2 and 5 throw: part 2's exception arrives, and only once every part has bumped the counter -- which each does last
template <class Spawn>
static int failing(Spawn spawn) {
    const size_t parts = 7, total = 23;
    std::atomic<int> finished{0};
    int at_catch = -1;
    std::string what;
    try {
        run_sliced(parts, total, [&](size_t m, size_t, size_t) {
            if (m != 2 && m != 5) std::this_thread::yield();  // the throwing parts tend to be done first
            struct Last {
                std::atomic<int>& n;
                ~Last() { ++n; }
            } last{finished};
            if (m == 5) throw std::runtime_error("part 5");
            if (m == 2) throw std::invalid_argument("part 2");
        }, spawn);
        CHECK(!"run_sliced returned although two parts threw");
    } catch (const std::invalid_argument& e) {
        at_catch = finished.load();
        what = e.what();
    } catch (...) {
        CHECK(!"the exception of a part other than the lowest-numbered one arrived");
    }
    CHECK(what == "part 2" && at_catch == (int)parts);
    // the runner is reusable after a failure, and a failure of part 0 -- the calling thread's -- waits for the others too
    finished = 0;
    try {
        run_sliced(parts, total, [&](size_t m, size_t, size_t) {
            struct Last {
                std::atomic<int>& n;
                ~Last() { ++n; }
            } last{finished};
            if (m == 0) throw std::runtime_error("part 0");
        }, spawn);
        CHECK(!"run_sliced returned although part 0 threw");
    } catch (const std::runtime_error& e) {
        CHECK(std::string(e.what()) == "part 0" && finished.load() == (int)parts);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "--slices")) {
        for (size_t total = 0; total <= kMaxTotal; total++)
            for (size_t parts = 1; parts <= kMaxParts; parts++)
                for (size_t m = 0; m < parts; m++) {
                    size_t first = 0, count = 0;
                    shard_slice(total, parts, m, &first, &count);
                    printf("%zu %zu %zu %zu %zu\n", total, parts, m, first, count);
                }
        return 0;
    }
    // a part that does not exist takes nothing
    size_t first = 1, count = 1;
    shard_slice(10, 0, 0, &first, &count);
    CHECK(first == 10 && count == 0);
    shard_slice(10, 3, 3, &first, &count);
    CHECK(first == 10 && count == 0);
    // no parts: nothing is called
    int calls = 0;
    run_sliced(0, 5, [&](size_t, size_t, size_t) { calls++; });
    CHECK(calls == 0);

    if (sweep(SpawnThread(), true)) return 1;
    if (failing(SpawnThread())) return 1;
    // part 3 finds no thread and runs inline: same slices, same calls, same exception rules
    std::atomic<int> refused{0};
    if (sweep(Refusing{{3}, &refused}, false)) return 1;
    CHECK(refused.load() > 0);
    if (failing(Refusing{{3}, &refused})) return 1;
    // ... and on the caller's thread
    std::thread::id where;
    run_sliced(6, 12, [&](size_t m, size_t, size_t) {
        if (m == 3) where = std::this_thread::get_id();
    }, Refusing{{3}, &refused});
    CHECK(where == std::this_thread::get_id());
    // no thread at all: everything inline, in part order after the refusals, part 0 last
    std::vector<size_t> order;
    run_sliced(4, 4, [&](size_t m, size_t, size_t) { order.push_back(m); }, Refusing{{1, 2, 3}, &refused});
    CHECK((order == std::vector<size_t>{1, 2, 3, 0}));
    // an exception from spawn that is not a std::system_error leaves after the threads already started were joined
    std::atomic<int> done{0};
    try {
        run_sliced(5, 5, [&](size_t, size_t, size_t) { ++done; }, [&](size_t part, auto&& body) -> std::thread {
            if (part == 3) throw std::logic_error("spawn");
            return std::thread(body);
        });
        CHECK(!"spawn's exception was swallowed");
    } catch (const std::logic_error&) {
        CHECK(done.load() == 2);  // parts 1 and 2 ran to their end; 0, 3 and 4 never started
    }
    puts("GROUP_RUN_OK");
    return 0;
}
