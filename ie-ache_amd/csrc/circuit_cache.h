// Built circuits, kept: the default-schedule circuit of every (kind, width, folding) asked for, plus a bounded number of
// level-capped variants of each.  Host only.  A context keeps 3 variants, the daemon's process-wide cache 1.
//
// Building the 128-bit multiplier's DAG and levelising it takes longer than evaluating a small batch of it, so a circuit is
// built once.  The cap follows the batch size (and the kernel family: "exact_fft" changes the resident-gate count), and a
// variant of the wide multipliers is several MB, so variants are bounded: the least recently used one goes, and only once the
// new circuit exists -- a caller that alternates between a few batch sizes or toggles exact_fft per call rebuilds nothing.
// Circuits are handed out as shared_ptr: an evaluation in flight keeps its circuit when another call evicts it.
#pragma once
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>

#include "circuit.h"

namespace ieache {

class CircuitCache {
public:
    using Ptr = std::shared_ptr<const Circuit>;
    explicit CircuitCache(size_t capped_variants) : capped_variants_(capped_variants) {}

    // The circuit of (kind, bits, fold) under its default schedule (cap 0) or with levels of `cap` gates; null, and nothing
    // cached, for an unsupported kind / width.
    Ptr fetch(int32_t kind, int32_t bits, bool fold, int32_t cap) {
        std::lock_guard<std::mutex> lock(mutex_);
        const Key key(kind, bits, fold, cap);
        const auto it = entries_.find(key);
        if (it != entries_.end()) {
            it->second.used = ++clock_;
            return it->second.circuit;
        }
        std::shared_ptr<Circuit> c(new Circuit);
        if (!build_circuit(kind, bits, c.get(), true, fold, cap)) return nullptr;
        if (cap != 0) {  // at most capped_variants_ variants of this (kind, bits, fold): the least recently used one makes room
            size_t n = 0;
            auto oldest = entries_.end();
            for (auto e = entries_.begin(); e != entries_.end(); ++e) {
                if (!same_circuit(e->first, key) || std::get<3>(e->first) == 0) continue;
                n++;
                if (oldest == entries_.end() || e->second.used < oldest->second.used) oldest = e;
            }
            if (n >= capped_variants_ && oldest != entries_.end()) entries_.erase(oldest);
        }
        entries_[key] = Entry{c, ++clock_};
        return c;
    }

    // The circuit to evaluate `batch` expressions with: the base circuit, or -- when level_quantum is on -- the same DAG
    // re-levelled to the width that makes a level x batch a whole number of the rounds of gates the GPU holds at once
    // (circuit_level_cap; same output bits): the slack-balanced 64/128-bit multipliers at any batch below a round, the
    // ASAP-scheduled 32-bit multiplier family at small batches.  forced_cap > 0 (a measurement aid) overrides all that.
    Ptr select(int32_t kind, int32_t bits, bool fold, int64_t batch, int32_t resident, int32_t resident_alt, bool level_quantum,
               int32_t forced_cap = 0) {
        const Ptr base = fetch(kind, bits, fold, 0);
        if (base && forced_cap > 0) return fetch(kind, bits, fold, forced_cap);
        if (!base || !level_quantum) return base;
        const int32_t cap = circuit_level_cap(*base, batch, resident, resident_alt);
        // the mean width is what the balanced schedule takes by default: that variant would be the base itself
        const int32_t mean = (int32_t)((base->n_bootstraps + base->depth - 1) / base->depth);
        if (cap <= 0 || (base->balanced_schedule && cap == mean)) return base;
        const Ptr capped = fetch(kind, bits, fold, cap);
        return capped && capped->balanced_schedule ? capped : base;
    }

private:
    using Key = std::tuple<int32_t, int32_t, bool, int32_t>;  // (kind, bits, folded, level cap)
    static bool same_circuit(const Key& a, const Key& b) {
        return std::get<0>(a) == std::get<0>(b) && std::get<1>(a) == std::get<1>(b) && std::get<2>(a) == std::get<2>(b);
    }
    struct Entry {
        Ptr circuit;
        uint64_t used;  // LRU order
    };
    const size_t capped_variants_;
    std::mutex mutex_;
    std::map<Key, Entry> entries_;
    uint64_t clock_ = 0;
};

}  // namespace ieache
