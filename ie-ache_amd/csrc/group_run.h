// `total` independent rows over `parts` workers: the slicing rule and the host threads that run the slices side by side.
// What a device group (group.h), its C ABI forms (capi.cpp) and the daemon (daemon.cpp) cut a call with.  Free of HIP, like
// br_plan.h, so that a host test drives it under the sanitizers (tests/native/group_run_test.cpp).
#pragma once
#include <cstddef>
#include <exception>
#include <system_error>
#include <thread>
#include <utility>
#include <vector>

namespace ieache {

// Contiguous slice [first, first + count) of `total` rows that part `part` of `parts` takes: sizes differ by at most one, the
// first total % parts parts take the extra row (= ieache_shard_slice, ie-ache_amd/parallel.py's shard_slice).  A part that
// does not exist takes nothing.
inline void shard_slice(size_t total, size_t parts, size_t part, size_t* first, size_t* count) {
    if (parts == 0 || part >= parts) {
        *first = total;
        *count = 0;
        return;
    }
    const size_t base = total / parts, extra = total % parts;
    *first = part * base + (part < extra ? part : extra);
    *count = base + (part < extra ? 1 : 0);
}

// A job list (ieache_job, include/ieache.h: anything with batch, in_lwe, out_lwe) as member `part` of `parts` takes it: every
// job's batch cut with shard_slice, its rows `in_words[j]` / `out_words[j]` words per expression further on, empty slices
// dropped.  Appends to *out; order is kept.
template <class Job>
void shard_jobs(const Job* jobs, size_t n_jobs, const size_t* in_words, const size_t* out_words, size_t parts, size_t part, std::vector<Job>* out) {
    for (size_t j = 0; j < n_jobs; j++) {
        size_t first = 0, count = 0;
        shard_slice(jobs[j].batch, parts, part, &first, &count);
        if (!count) continue;
        Job s = jobs[j];
        s.batch = count;
        s.in_lwe = jobs[j].in_lwe + first * in_words[j];
        s.out_lwe = jobs[j].out_lwe + first * out_words[j];
        out->push_back(s);
    }
}

// run_sliced's default `spawn`: a host thread per part
struct SpawnThread {
    template <class Body>
    std::thread operator()(size_t /*part*/, Body&& body) const {
        return std::thread(std::forward<Body>(body));
    }
};

// fn(m, first, count) for every part m of `parts` whose slice of `total` (shard_slice) is not empty: part 0 on the calling
// thread, every other part on a thread of its own -- spawn(m, body) -> std::thread.  A part whose thread cannot be had (spawn
// throws std::system_error) runs on the calling thread instead, there and then, beside the threads already started.  Every
// thread is joined before this returns or throws, whatever happened.  If parts threw, the exception of the lowest-numbered
// one is rethrown after the join; the others are dropped.  fn runs concurrently with itself: what it touches must belong to
// its part.
template <class Fn, class Spawn = SpawnThread>
void run_sliced(size_t parts, size_t total, Fn&& fn, Spawn&& spawn = Spawn()) {
    std::vector<std::exception_ptr> errors(parts);
    auto run_part = [&](size_t m, size_t first, size_t count) noexcept {
        try {
            fn(m, first, count);
        } catch (...) {
            errors[m] = std::current_exception();
        }
    };
    struct Joined {  // joins on every way out, an exception from spawn that is not a std::system_error included
        std::vector<std::thread> threads;
        ~Joined() {
            for (std::thread& t : threads)
                if (t.joinable()) t.join();
        }
    } joined;
    joined.threads.reserve(parts);  // so that keeping a started thread cannot fail
    size_t first0 = 0, count0 = 0;
    shard_slice(total, parts, 0, &first0, &count0);
    for (size_t m = 1; m < parts; m++) {
        size_t first = 0, count = 0;
        shard_slice(total, parts, m, &first, &count);
        if (!count) continue;
        try {
            joined.threads.push_back(spawn(m, [&run_part, m, first, count] { run_part(m, first, count); }));
        } catch (const std::system_error&) {
            run_part(m, first, count);
        }
    }
    if (count0) run_part(0, first0, count0);
    for (std::thread& t : joined.threads) t.join();
    for (const std::exception_ptr& e : errors)
        if (e) std::rethrow_exception(e);
}

}  // namespace ieache
