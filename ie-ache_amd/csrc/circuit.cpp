// See circuit.h.  Every builder function cites the cloud.c lines it mirrors.
#include "circuit.h"

#include "../../include/ieache.h"

#include <algorithm>
#include <cassert>
#include <cstdlib>
#include <queue>
#include <stdexcept>
#include <utility>

namespace ieache {

// f(wire) for every operand of a gate that is a wire (not a constant); an unused third operand is the constant 0
template <class F>
static void for_each_wire(const Gate& g, F&& f) {
    for (const Ref* r : {&g.a, &g.b, &g.c})
        if (r->id >= 0) f(r->id);
}

CircuitBuilder::CircuitBuilder(int32_t n_inputs, bool fold)
    : n_inputs_(n_inputs), next_wire_(n_inputs), fold_(fold), wire_level_(n_inputs, 0) {}

Ref CircuitBuilder::input(int32_t i) const {
    if (i < 0 || i >= n_inputs_) throw std::out_of_range("circuit input index");
    return Ref{i, false};
}

Word CircuitBuilder::input_word(int32_t first, int32_t count) const {
    Word w(count);
    for (int32_t i = 0; i < count; i++) w[i] = input(first + i);
    return w;
}

Ref CircuitBuilder::gate(int32_t type, Ref a, Ref b) {
    if (a.id == kUndefId || b.id == kUndefId)
        throw std::logic_error("gate consumes a never-written sample");
    if (type < 0 || type >= GATE_TYPES || type == GATE_MUX) throw std::invalid_argument("not a two-input gate type");
    n_requested_++;
    return gate2(type, a, b);
}

Ref CircuitBuilder::gate2(int32_t type, Ref a, Ref b) {
    const int32_t requested = type;
    // boot-gates.cpp: NOR / ANDNY / ANDYN / ORNY / ORYN are AND / OR of +-ca, +-cb -- recorded as such (the sign flags
    // of the operands), which is the same linear combination word for word
    switch (type) {
        case GATE_NOR: type = GATE_AND; a.neg = !a.neg; b.neg = !b.neg; break;
        case GATE_ANDNY: type = GATE_AND; a.neg = !a.neg; break;
        case GATE_ANDYN: type = GATE_AND; b.neg = !b.neg; break;
        case GATE_ORNY: type = GATE_OR; a.neg = !a.neg; break;
        case GATE_ORYN: type = GATE_OR; b.neg = !b.neg; break;
        default: break;
    }
    bool out_neg = false;
    if (fold_ && (type == GATE_AND || type == GATE_XOR)) {
        const bool ca = a.id == kConstId, cb = b.id == kConstId;
        if (type == GATE_AND) {
            if (ca) return a.neg ? b : constant(0);  // 1 AND b = b ; 0 AND b = 0
            if (cb) return b.neg ? a : constant(0);
            if (a.id == b.id) return a.neg == b.neg ? a : constant(0);  // x AND x ; x AND NOT x
        } else {
            if (ca) return Ref{b.id, b.neg != a.neg};  // 0 XOR b = b ; 1 XOR b = NOT b
            if (cb) return Ref{a.id, a.neg != b.neg};
            if (a.id == b.id) return constant(a.neg != b.neg);
            out_neg = a.neg != b.neg;  // XOR(NOT a, b) = NOT XOR(a, b): negations move to the output
            a.neg = b.neg = false;
        }
        if (a.id > b.id) std::swap(a, b);  // both gates commute
    }
    return Ref{record(type, requested, a, b, constant(0)), out_neg};
}

// bootsMUX(a, b, c) = a ? b : c.  Recorded as given: no folding, no sharing.
// GATE_MAJ3 / GATE_XOR3: one blind rotation of ca + cb + cc resp. (0,1/2) + 2(ca + cb + cc).
Ref CircuitBuilder::gate3(int32_t type, Ref a, Ref b, Ref c) {
    if (type != GATE_MUX && !is_gate3(type)) throw std::invalid_argument("not a three-input gate type");
    if (a.id == kUndefId || b.id == kUndefId || c.id == kUndefId)
        throw std::logic_error("gate consumes a never-written sample");
    bool out_neg = false;
    if (is_gate3(type)) {
        Ref r[3] = {a, b, c};
        int same = -1;  // r[same] and r[same2] name one wire
        int same2 = -1;
        for (int i = 0; i < 3 && same < 0; i++)
            for (int j = i + 1; j < 3; j++)
                if (r[i].id >= 0 && r[i].id == r[j].id) {
                    same = i;
                    same2 = j;
                    break;
                }
        if (same >= 0 && !fold_) throw std::invalid_argument("a three-input gate names the same wire twice");
        n_requested_++;
        if (fold_) {
            if (same >= 0) {  // MAJ3(x,x,z) = x ; MAJ3(x,~x,z) = z ; XOR3(x,x,z) = z ; XOR3(x,~x,z) = ~z
                const Ref z = r[3 - same - same2];
                const bool equal = r[same].neg == r[same2].neg;
                if (type == GATE_MAJ3) return equal ? r[same] : z;
                return Ref{z.id, z.neg != !equal};
            }
            for (int i = 0; i < 3; i++)
                if (r[i].id == kConstId) {  // a constant operand: the two-input gate of the other two (which folds further)
                    const Ref x = r[(i + 1) % 3], y = r[(i + 2) % 3];
                    const bool k = r[i].neg;
                    if (type == GATE_XOR3) {
                        const Ref t = gate2(GATE_XOR, x, y);  // XOR3(x,y,1) = XNOR(x,y) = NOT XOR(x,y): the negation is free
                        return Ref{t.id, t.neg != k};
                    }
                    if (x.id == kConstId || y.id == kConstId) {  // MAJ3(x, k', k) = k when k' == k, else x
                        const Ref w = x.id == kConstId ? y : x, k2 = x.id == kConstId ? x : y;
                        return k2.neg == k ? constant(k) : w;
                    }
                    return gate2(k ? GATE_OR : GATE_AND, x, y);
                }
            // share: both gates are symmetric; XOR3's operand negations move to the output
            std::sort(r, r + 3, [](const Ref& p, const Ref& q) { return p.id < q.id; });
            if (type == GATE_XOR3)
                for (Ref& q : r) {
                    out_neg = out_neg != q.neg;
                    q.neg = false;
                }
            a = r[0], b = r[1], c = r[2];
        }
    } else {
        n_requested_++;
    }
    return Ref{record(type, type, a, b, c), out_neg};
}

int32_t CircuitBuilder::record(int32_t type, int32_t requested, Ref a, Ref b, Ref c) {
    if (fold_ && (type == GATE_AND || type == GATE_XOR || is_gate3(type))) {  // the gates that share (a MUX is recorded as given)
        const auto key = std::make_tuple(type, a.id, (int32_t)a.neg, b.id, (int32_t)b.neg, c.id, (int32_t)c.neg);
        const auto it = known_.emplace(key, next_wire_);
        if (!it.second) return it.first->second;
    }
    Gate g;
    g.type = type;
    g.a = a;
    g.b = b;
    g.c = c;
    g.out = next_wire_++;
    g.level = 1;
    for_each_wire(g, [&](int32_t w) { g.level = std::max(g.level, wire_level_[w] + 1); });
    wire_level_.push_back(g.level);
    gates_.push_back(g);
    requested_type_.push_back(requested);
    return g.out;
}

// cloud.c:18-51.  carry-in is c[0] (bootsCOPY :24); carry-out lands in
// carryover[0] only (:46).  sum may alias x (cloud.c:194): x[i] is read before
// sum[i] is written, which SSA wires preserve by construction.
void CircuitBuilder::add(Word& sum, Word& carryover, const Word& x, const Word& y, const Word& c,
                         int32_t nb_bits) {
    Ref carry = c[0];
    for (int32_t i = 0; i < nb_bits; i++) {
        const Ref xi = x[i], yi = y[i];
        Ref axc = XOR(xi, carry);        // :30
        const Ref bxc = XOR(yi, carry);  // :32
        sum[i] = XOR(xi, bxc);           // :38
        axc = AND(axc, bxc);             // :40
        carry = XOR(carry, axc);         // :43
    }
    carryover[0] = carry;
}

void CircuitBuilder::zero(Word& result, size_t size) {  // cloud.c:53-57
    for (size_t i = 0; i < size; i++) result[i] = constant(0);
}

void CircuitBuilder::NOT(Word& result, const Word& x, size_t size) {  // cloud.c:59-63
    for (size_t i = 0; i < size; i++) result[i] = NOT(x[i]);
}

// cloud.c:65-113
void CircuitBuilder::split(Word& f1, Word& f2, Word& f3, const Word& a, const Word& b, const Word& c,
                           const Word& d, const Word& e, const Word& carry, int32_t nb_bits) {
    Word sum = fresh(), sum2 = fresh(), sum3 = fresh();
    Word co = fresh(), co2 = fresh(), co3 = fresh();
    for (Word* w : {&sum, &sum2, &sum3, &co, &co2, &co3}) zero(*w, nb_bits);  // :77-87
    add(sum, co, e, b, carry, nb_bits);                                          // :90
    add(sum2, co2, d, a, co, nb_bits);                                           // :91
    add(sum3, co3, c, co2, carry, nb_bits);  // :92  y = [carry-out, 0, 0, ...]
    for (int32_t i = 0; i < nb_bits; i++) {  // :94-105
        f1[i] = sum3[i];
        f2[i] = sum2[i];
        f3[i] = sum[i];
    }
}

// Shift-add multiply of a `words`-word operand by one 32-bit word
// (cloud.c:115-218, 220-385, 387-647).  Round r ANDs every operand bit with
// multiplier bit r, places that row at bit offset r across words+1 words
// (bits outside the row are bootsCONSTANT 0: cloud.c:164-192 and the
// initial zeroing :132-145), then adds word by word with the carry chained
// (:194-195, :355-357, :604-608).
void CircuitBuilder::mul_words(std::vector<Word*> results, const std::vector<const Word*>& in,
                               const Word& m, const Word& carry, int32_t nb_bits) {
    const int words = (int)in.size(), W1 = words + 1;
    assert((int)results.size() == W1 && nb_bits == 32);
    std::vector<Word> sum(W1, Word(32, constant(0)));
    std::vector<Word> cy(W1, Word(32, constant(0)));
    for (int32_t r = 0; r < nb_bits; r++) {
        // T[32w+k] = in[w][k] AND m[r]   (:150-162, :268-283, :452-473)
        std::vector<Ref> T((size_t)32 * words);
        for (int32_t kbit = 0; kbit < nb_bits; kbit++)
            for (int w = 0; w < words; w++) T[32 * w + kbit] = AND((*in[w])[kbit], m[r]);
        for (int w = 0; w < W1; w++) {
            Word row(32);
            for (int32_t q = 0; q < 32; q++) {
                const int32_t pos = 32 * w + q - r;
                row[q] = (pos >= 0 && pos < 32 * words) ? T[pos] : constant(0);
            }
            add(sum[w], cy[w], sum[w], row, w == 0 ? carry : cy[w - 1], 32);
        }
    }
    for (int w = 0; w < W1; w++) *results[w] = sum[W1 - 1 - w];  // :200-204 high word first
}

void CircuitBuilder::mul32(Word& result, Word& result2, const Word& a, const Word& b,
                           const Word& carry, int32_t nb_bits) {
    mul_words({&result, &result2}, {&a}, b, carry, nb_bits);
}

// widths and counts are in blind rotations: a MUX is two (level_items.h)
static int32_t cost(const Gate& g) { return g.type == GATE_MUX ? 2 : 1; }

// (a) ASAP statistics: depth, the widest ASAP level, blind rotations in all
struct AsapStats {
    int32_t depth = 0, max_width = 0;
    int64_t n_rot = 0;
};
static AsapStats asap_stats(const std::vector<Gate>& gates) {
    AsapStats s;
    for (const Gate& g : gates) {
        s.depth = std::max(s.depth, g.level);
        s.n_rot += cost(g);
    }
    std::vector<int32_t> w(s.depth + 1, 0);
    for (const Gate& g : gates) w[g.level] += cost(g);
    for (int32_t L = 1; L <= s.depth; L++) s.max_width = std::max(s.max_width, w[L]);
    return s;
}

// (b) The execution schedule.  ASAP piles every gate with slack into the earliest level (all 1024
// ANDs of mul32 land in level 1) and leaves the carry chains as levels of 2-3 gates.  The
// executor instead runs a slack-aware list schedule over the same number of levels: a gate
// on the critical path runs at its ASAP = ALAP level, the others are spread, least slack
// first, to keep every level near the mean width.  Narrow levels fill up (what matters when
// the batch is small) and the wire store shrinks (mul128: 16 800 -> 2 921 rows per
// expression).  The DAG, and therefore every output bit, is unchanged.
// depth > 0: the ASAP depth.  -> (level of every gate, levels the executor runs)
static std::pair<std::vector<int32_t>, int32_t> list_schedule(const std::vector<Gate>& gates, int32_t n_wires, int32_t depth, int64_t n_rot,
                                                              int32_t level_cap) {
    // Forward list scheduling: a gate is ready one level after its last operand; a gate
    // whose ALAP level is the current level must run now, the others fill the level up to
    // the mean width, least slack first.  (A backward, as-late-as-possible pass was tried:
    // with no spare capacity it starves low-ASAP gates and piles them into the first levels.)
    const int32_t n_gates = (int32_t)gates.size();
    std::vector<int32_t> sched(n_gates, 0);
    std::vector<int32_t> producer(n_wires, -1);  // wire -> gate index
    for (int32_t i = 0; i < n_gates; i++) producer[gates[i].out] = i;
    // f(producing gate) for every operand of gate i that a gate produces
    auto for_each_producer = [&](int32_t i, auto&& f) {
        for_each_wire(gates[i], [&](int32_t w) {
            if (producer[w] >= 0) f(producer[w]);
        });
    };
    std::vector<std::vector<int32_t>> users(n_gates);
    std::vector<int32_t> n_operands(n_gates, 0);
    for (int32_t i = 0; i < n_gates; i++)
        for_each_producer(i, [&](int32_t p) {
            users[p].push_back(i);
            n_operands[i]++;
        });
    // level_cap > 0 (the caller knows the batch): levels of exactly that many gates, so that a level times
    // the batch is a whole number of the workgroup rounds the GPU holds at once.  A cap under the mean width
    // cannot fit the ASAP depth: the schedule is then stretched (more levels, each of them full), which is the
    // better trade whenever a level is a few rounds wide -- 1.2 rounds cost 2.
    const int32_t mean = (int32_t)std::max<int64_t>((n_rot + depth - 1) / depth, 1);
    const int32_t cap = level_cap > 0 ? level_cap : mean;
    int32_t sched_depth = depth;
    if (cap < mean) sched_depth = std::max<int32_t>(depth, (int32_t)((n_rot + cap - 1) / cap));
    for (;; sched_depth += std::max(1, sched_depth / 50)) {
        std::vector<int32_t> alap(n_gates, sched_depth);
        for (int32_t i = n_gates - 1; i >= 0; i--)  // builder order is topological
            for_each_producer(i, [&](int32_t p) { alap[p] = std::min(alap[p], alap[i] - 1); });
        std::vector<int32_t> pending = n_operands;
        auto cmp = [&](int32_t x, int32_t y) { return alap[x] != alap[y] ? alap[x] > alap[y] : x > y; };  // min-heap on ALAP
        std::priority_queue<int32_t, std::vector<int32_t>, decltype(cmp)> ready(cmp);
        std::vector<int32_t> next_ready;
        for (int32_t i = 0; i < n_gates; i++)
            if (pending[i] == 0) ready.push(i);
        int32_t done = 0, overflowing = 0;  // levels in which critical gates had to exceed the cap
        for (int32_t L = 1; L <= sched_depth; L++) {
            int32_t taken = 0;
            bool over = false;
            next_ready.clear();
            while (!ready.empty()) {
                const int32_t g = ready.top();
                // only critical gates may exceed the cap (a MUX that starts under it may end one rotation over)
                if (alap[g] > L && taken >= cap) break;
                if (taken >= cap && !over) {
                    overflowing++;
                    over = true;
                }
                ready.pop();
                sched[g] = L;
                taken += cost(gates[g]);
                done++;
                for (int32_t u : users[g])
                    if (--pending[u] == 0) next_ready.push_back(u);  // usable from the next level on
            }
            for (int32_t u : next_ready) ready.push(u);
        }
        // a stretched schedule is accepted once (almost) every level respects the cap: a level over it costs a
        // whole extra round for a few gates
        if (done == n_gates && !(level_cap > 0 && cap < mean && overflowing * 50 > sched_depth)) break;
        if (sched_depth > 4 * depth + n_gates) throw std::logic_error("list scheduling left gates unscheduled");
    }
    return {std::move(sched), sched_depth};
}

// (c) Gates ordered by scheduled level (stable: keeps the reference's program order inside a level), the MUX gates of a level
// after its other gates: the executor's item arithmetic relies on it (level_items.h).  Fills level_offset, level_mux and
// sched_max_width.  -> the order
static std::vector<int32_t> order_levels(const std::vector<Gate>& gates, const std::vector<int32_t>& sched, int32_t depth, Circuit* c) {
    std::vector<int32_t> order(gates.size());
    for (size_t i = 0; i < order.size(); i++) order[i] = (int32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
        return sched[x] != sched[y] ? sched[x] < sched[y] : (gates[x].type == GATE_MUX) < (gates[y].type == GATE_MUX);
    });
    c->level_offset.assign(depth + 1, 0);
    c->level_mux.assign(depth, 0);
    for (size_t i = 0; i < gates.size(); i++) {
        c->level_offset[sched[i]]++;
        if (gates[i].type == GATE_MUX) c->level_mux[sched[i] - 1]++;
    }
    for (int32_t L = 1; L <= depth; L++) {
        c->sched_max_width = std::max(c->sched_max_width, c->level_offset[L] + c->level_mux[L - 1]);  // in blind rotations
        c->level_offset[L] += c->level_offset[L - 1];
    }
    return order;
}

// (d) Liveness and slot allocation: fills n_slots, gates (in `order`) and outputs.
static void allocate_slots(const std::vector<Gate>& gates, const std::vector<int32_t>& sched, const std::vector<int32_t>& order, int32_t n_wires,
                           const Word& outputs, Circuit* c) {
    // liveness: last level at which each wire is read; outputs live forever
    const int32_t depth = c->n_levels(), kForever = depth + 1;
    std::vector<int32_t> last_use(n_wires, 0);
    for (size_t i = 0; i < gates.size(); i++)
        for_each_wire(gates[i], [&](int32_t w) { last_use[w] = std::max(last_use[w], sched[i]); });
    for (const Ref& r : outputs) {
        if (r.id == kUndefId) throw std::logic_error("circuit output was never written");
        if (r.id >= 0) last_use[r.id] = kForever;
    }
    // slot allocation: inputs start in slots 0..n_inputs-1; a slot is recycled
    // from the level AFTER its wire's last read, so no gate of a level ever
    // overwrites a row another gate of the same level still reads.
    std::vector<int32_t> slot_of(n_wires, -1);
    std::vector<int32_t> free_slots;
    std::vector<std::vector<int32_t>> dying(depth + 2);
    int32_t n_slots = c->n_inputs;
    for (int32_t w = 0; w < c->n_inputs; w++) {
        slot_of[w] = w;
        dying[last_use[w]].push_back(w);
    }
    for (int32_t w : dying[0]) free_slots.push_back(slot_of[w]);
    auto slot = [&](const Ref& r) { return r.id >= 0 ? slot_of[r.id] : -1; };
    c->gates.resize(gates.size());
    size_t pos = 0;
    for (int32_t L = 1; L <= depth; L++) {
        const size_t end = (size_t)c->level_offset[L];
        for (; pos < end; pos++) {
            const Gate& g = gates[order[pos]];
            int32_t s;
            if (!free_slots.empty()) {
                s = free_slots.back();
                free_slots.pop_back();
            } else {
                s = n_slots++;
            }
            slot_of[g.out] = s;
            dying[last_use[g.out] == 0 ? L : last_use[g.out]].push_back(g.out);  // unread wires die at once
            DevGate& d = c->gates[pos];
            d.type = g.type;
            d.a_slot = slot(g.a);
            d.a_neg = g.a.neg;
            d.b_slot = slot(g.b);
            d.b_neg = g.b.neg;
            d.out_slot = s;
            d.c_slot = slot(g.c);
            d.c_neg = g.type == GATE_MUX || is_gate3(g.type) ? (int32_t)g.c.neg : 0;
        }
        for (int32_t w : dying[L]) free_slots.push_back(slot_of[w]);
    }
    c->n_slots = n_slots;
    c->outputs.resize(outputs.size());
    for (size_t i = 0; i < outputs.size(); i++) {
        c->outputs[i].slot = slot(outputs[i]);
        c->outputs[i].neg = outputs[i].neg;
    }
}

// (e) gates by the type they were requested as, and the recorded ANDs and XORs
static void count_types(const CircuitBuilder& b, Circuit* c) {
    for (int32_t requested : b.requested_types()) {
        if (requested < GATE_TYPES) c->n_by_type[requested]++;
        if (requested == GATE_MAJ3) c->n_maj3++;
        if (requested == GATE_XOR3) c->n_xor3++;
    }
    for (const Gate& g : b.gates()) {
        if (g.type == GATE_AND) c->n_and++;
        if (g.type == GATE_XOR) c->n_xor++;
    }
}

Circuit finalize_circuit(const std::string& name, const CircuitBuilder& b, const Word& outputs, bool balanced, int32_t level_cap) {
    Circuit c;
    c.name = name;
    c.n_inputs = b.n_inputs();
    const std::vector<Gate>& gates = b.gates();
    const AsapStats asap = asap_stats(gates);
    c.depth = asap.depth;  // stays the ASAP depth when a level cap stretches the schedule
    c.max_width = asap.max_width;
    c.n_bootstraps = asap.n_rot;
    std::vector<int32_t> sched(gates.size());
    int32_t levels = asap.depth;
    if (balanced && asap.depth > 0)
        std::tie(sched, levels) = list_schedule(gates, b.n_wires(), asap.depth, asap.n_rot, level_cap);
    else
        for (size_t i = 0; i < gates.size(); i++) sched[i] = gates[i].level;
    const std::vector<int32_t> order = order_levels(gates, sched, levels, &c);
    allocate_slots(gates, sched, order, b.n_wires(), outputs, &c);
    count_types(b, &c);
    return c;
}

// ---- what each plain kind is: one row per code.  Adding a kind: a row here, its builder function (and build_stage's call of it
// if it is not one of the adder families), one line in include/ieache.h and one in evaluator.py. ----
namespace {
enum Operator : int32_t { OP_ADD, OP_SUB, OP_RSUB, OP_MUL };
enum Widths : int32_t {
    ANY_WIDTH,   // 1 .. 256 (the reference uses 32/64/128/256; 16 is BASELINE.json's generalisation add(...,16,...))
    MUL_WIDTHS,  // 32, 64, 128 (cloud.c:860-864 refuses 256)
};
struct KindRow {
    int32_t code;
    const char* name;
    Operator op;
    CircuitFamily family;
    Widths widths;
    int32_t out_factor;  // output samples = out_factor x bits
    int32_t ref_kind;    // n_reference_bootstraps is this kind's bootstrap count: what cloud.c performs for the same result
    bool force_fold;     // built with folding on whatever the caller asks
};
constexpr KindRow kKinds[] = {
    {CIRC_ADD, "add", OP_ADD, FAMILY_REFERENCE, ANY_WIDTH, 1, CIRC_ADD, false},
    {CIRC_SUB, "sub", OP_SUB, FAMILY_REFERENCE, ANY_WIDTH, 1, CIRC_SUB, false},
    {CIRC_RSUB, "rsub", OP_RSUB, FAMILY_REFERENCE, ANY_WIDTH, 1, CIRC_RSUB, false},
    {CIRC_MUL, "mul", OP_MUL, FAMILY_REFERENCE, MUL_WIDTHS, 2, CIRC_MUL, false},
    // the Kogge-Stone adders report the gates they were asked for
    {CIRC_ADD_KS, "add_ks", OP_ADD, FAMILY_KOGGE_STONE, ANY_WIDTH, 1, CIRC_ADD_KS, false},
    {CIRC_SUB_KS, "sub_ks", OP_SUB, FAMILY_KOGGE_STONE, ANY_WIDTH, 1, CIRC_SUB_KS, false},
    {CIRC_RSUB_KS, "rsub_ks", OP_RSUB, FAMILY_KOGGE_STONE, ANY_WIDTH, 1, CIRC_RSUB_KS, false},
    // the carry-save multiplier is built with folding on: it is opt-in and not the reference's gate list
    // anyway, and its final adder sees constant-zero operands in the outer columns
    {CIRC_MUL_WALLACE, "mul_wallace", OP_MUL, FAMILY_CARRY_SAVE, MUL_WIDTHS, 2, CIRC_MUL, true},
    {CIRC_ADD_FA, "add_fa", OP_ADD, FAMILY_FULL_ADDER, ANY_WIDTH, 1, CIRC_ADD, false},
    {CIRC_SUB_FA, "sub_fa", OP_SUB, FAMILY_FULL_ADDER, ANY_WIDTH, 1, CIRC_SUB, false},
    {CIRC_RSUB_FA, "rsub_fa", OP_RSUB, FAMILY_FULL_ADDER, ANY_WIDTH, 1, CIRC_RSUB, false},
    {CIRC_MUL_FA, "mul_fa", OP_MUL, FAMILY_FULL_ADDER, MUL_WIDTHS, 2, CIRC_MUL, false},
};
constexpr const KindRow* find_kind(int32_t code) {
    for (const KindRow& r : kKinds)
        if (r.code == code) return &r;
    return nullptr;
}
constexpr bool accepts(const KindRow& r, int32_t bits) {
    return r.widths == ANY_WIDTH ? bits >= 1 && bits <= 256 : bits == 32 || bits == 64 || bits == 128;
}
// the table's codes, row by row, are the C ABI's
constexpr int32_t kAbiCodes[] = {IEACHE_CIRC_ADD,     IEACHE_CIRC_SUB,         IEACHE_CIRC_RSUB,   IEACHE_CIRC_MUL,
                                 IEACHE_CIRC_ADD_KS,  IEACHE_CIRC_SUB_KS,      IEACHE_CIRC_RSUB_KS, IEACHE_CIRC_MUL_WALLACE,
                                 IEACHE_CIRC_ADD_FA,  IEACHE_CIRC_SUB_FA,      IEACHE_CIRC_RSUB_FA, IEACHE_CIRC_MUL_FA};
constexpr bool table_matches_abi() {
    if (sizeof kAbiCodes / sizeof kAbiCodes[0] != sizeof kKinds / sizeof kKinds[0]) return false;
    for (size_t i = 0; i < sizeof kKinds / sizeof kKinds[0]; i++)
        if (kKinds[i].code != kAbiCodes[i] || find_kind(kKinds[i].ref_kind) == nullptr) return false;
    return true;
}
static_assert(table_matches_abi(), "the kind table and include/ieache.h's IEACHE_CIRC_* disagree");
static_assert(CIRC_MULADD == IEACHE_CIRC_MULADD && chain_kind(CIRC_MUL, CIRC_ADD, true) == IEACHE_CIRC_CHAIN(IEACHE_CIRC_MUL, IEACHE_CIRC_ADD, 1) &&
                  chain_kind(CIRC_RSUB, CIRC_SUB, false) == IEACHE_CIRC_CHAIN(IEACHE_CIRC_RSUB, IEACHE_CIRC_SUB, 0),
              "the chain encoding and include/ieache.h's IEACHE_CIRC_CHAIN disagree");

// A kind as its stages: one row for a plain kind, two for a chain (decode_chain's k1, k2 are reference kinds).
struct Stages {
    const KindRow* s1 = nullptr;  // null: the code names no kind
    const KindRow* s2 = nullptr;  // null: not a chain
    bool flip = true;
    int32_t w2(int32_t bits) const { return s1->out_factor * bits; }  // stage 1's output width = stage 2's operand width
};
Stages stages_of(int32_t kind) {
    Stages s;
    int32_t k1, k2;
    if (decode_chain(kind, &k1, &k2, &s.flip)) {
        s.s1 = find_kind(k1);
        s.s2 = find_kind(k2);
    } else {
        s.s1 = find_kind(kind);
    }
    return s;
}
}  // namespace

bool decode_chain(int32_t kind, int32_t* k1, int32_t* k2, bool* flip) {
    if (kind == CIRC_MULADD) kind = chain_kind(CIRC_MUL, CIRC_ADD, true);
    if (kind < CIRC_CHAIN_BASE || kind >= CIRC_CHAIN_END) return false;
    const int32_t c = kind - CIRC_CHAIN_BASE;
    *k1 = (c & 3) + 1;
    *k2 = ((c >> 2) & 3) + 1;
    *flip = (c & 16) == 0;
    return true;
}

bool circuit_multiplies(int32_t kind) {
    const Stages s = stages_of(kind);
    return s.s1 && (s.s1->op == OP_MUL || (s.s2 && s.s2->op == OP_MUL));
}

int32_t circuit_kind_in_family(int32_t kind, CircuitFamily family) {
    const Stages s = stages_of(kind);
    if (s.s1 && !s.s2)
        for (const KindRow& r : kKinds)
            if (r.op == s.s1->op && r.family == family) return r.code;
    return kind;
}

bool circuit_accepts_width(int32_t kind, int32_t bits) {
    const Stages s = stages_of(kind);
    return s.s1 && bits >= 1 && bits <= 256 && accepts(*s.s1, bits) && (!s.s2 || accepts(*s.s2, s.w2(bits)));
}

int32_t circuit_n_inputs(int32_t kind, int32_t bits) {
    const Stages s = stages_of(kind);
    if (!s.s1) return -1;
    // A, B, the carry word [, C at stage 2's width [, C's carry word when the answer is operand 2]]
    return 2 * bits + 32 + (s.s2 ? s.w2(bits) + (s.flip ? 0 : 32) : 0);
}

int32_t circuit_n_outputs(int32_t kind, int32_t bits) {
    const Stages s = stages_of(kind);
    if (!s.s1) return -1;
    return (s.s2 ? s.s2->out_factor : 1) * s.w2(bits);
}

// Split a flat bit vector into 32-bit words (the last may be shorter).
static std::vector<Word> to_words(const Word& bits) {
    std::vector<Word> w;
    for (size_t i = 0; i < bits.size(); i += 32)
        w.emplace_back(bits.begin() + i, bits.begin() + std::min(bits.size(), i + 32));
    return w;
}

// W chained adds over word pairs (e.g. cloud.c:951-952, 1020-1023, 1109-1116)
static Word chained_add(CircuitBuilder& b, const std::vector<Word>& x, const std::vector<Word>& y,
                        const Word& carry_in) {
    Word out;
    Word prev = carry_in;
    for (size_t w = 0; w < x.size(); w++) {
        const int32_t nb = (int32_t)x[w].size();
        Word res = CircuitBuilder::fresh(nb), cy = CircuitBuilder::fresh();
        b.add(res, cy, x[w], y[w], prev, nb);
        out.insert(out.end(), res.begin(), res.end());
        prev = cy;
    }
    return out;
}

// two's complement of an operand, word by word (cloud.c:1225-1236, 1325-1341)
static std::vector<Word> twos_complement(CircuitBuilder& b, const std::vector<Word>& v) {
    std::vector<Word> twos;
    Word temp = CircuitBuilder::fresh();
    CircuitBuilder::zero(temp, 32);          // :1228
    temp[0] = CircuitBuilder::constant(1);   // :1233
    Word prev_carry;
    for (size_t w = 0; w < v.size(); w++) {
        const int32_t nb = (int32_t)v[w].size();
        Word inverse = CircuitBuilder::fresh(nb), tempcarry = CircuitBuilder::fresh();
        CircuitBuilder::NOT(inverse, v[w], nb);  // :1225
        CircuitBuilder::zero(tempcarry, 32);     // :1229
        Word res = CircuitBuilder::fresh(nb), cy = CircuitBuilder::fresh();
        if (w == 0)
            b.add(res, cy, inverse, temp, tempcarry, nb);  // :1236  +1
        else
            b.add(res, cy, inverse, tempcarry, prev_carry, nb);  // :1341 propagate
        twos.push_back(res);
        prev_carry = cy;
    }
    return twos;
}

// Kogge-Stone addition x + y + cin with XOR/AND only.  (g, p) o (g', p') = (g | p&g', p&p');
// g and p&g' are never both 1 (g = 1 forces p = 0), so the OR is an XOR.
static Word kogge_stone_add(CircuitBuilder& b, const Word& x, const Word& y, Ref cin) {
    const int n = (int)x.size();
    std::vector<Ref> g(n), p(n), p0(n);
    for (int i = 0; i < n; i++) {
        g[i] = b.AND(x[i], y[i]);
        p[i] = b.XOR(x[i], y[i]);
        p0[i] = p[i];
    }
    // fold the carry-in into bit 0's generate: carry out of bit 0 = g0 ^ (p0 & cin)
    g[0] = b.XOR(g[0], b.AND(p[0], cin));
    for (int d = 1; d < n; d <<= 1) {
        std::vector<Ref> ng = g, np = p;
        for (int i = d; i < n; i++) {
            ng[i] = b.XOR(g[i], b.AND(p[i], g[i - d]));
            if (i >= 2 * d) np[i] = b.AND(p[i], p[i - d]);  // prefixes reaching bit 0 need no more propagate
        }
        g.swap(ng);
        p.swap(np);
    }
    Word sum(n);
    sum[0] = b.XOR(p0[0], cin);
    for (int i = 1; i < n; i++) sum[i] = b.XOR(p0[i], g[i - 1]);  // g[i-1] = carry into bit i
    return sum;
}

// A * B by carry-save reduction (see CIRC_MUL_WALLACE).  Full adder on XOR/AND only:
//   t = x ^ y ; sum = t ^ z ; carry = (x & y) ^ (z & t)      ((x & y) and (z & t) are never both 1)
static Word wallace_mul(CircuitBuilder& b, const Word& A, const Word& B) {
    const int n = (int)A.size(), W = 2 * n;
    std::vector<std::vector<Ref>> col(W);
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) col[i + j].push_back(b.AND(A[j], B[i]));
    // Dadda's schedule: heights 2, 3, 4, 6, 9, 13, 19, 28, ... (d_{j+1} = floor(1.5 d_j)); each stage reduces every
    // column just enough to meet the next smaller height, counting the carries that arrive from the column
    // below in the same stage -- so no carry ripples from stage to stage and 32 rows take 8 stages
    std::vector<size_t> heights{2};
    size_t tallest = 0;
    for (const auto& cc : col) tallest = std::max(tallest, cc.size());
    while (heights.back() < tallest) heights.push_back(heights.back() * 3 / 2);
    for (int stage = (int)heights.size() - 2; stage >= 0; stage--) {
        const size_t d = heights[stage];
        std::vector<std::vector<Ref>> next(W);
        for (int c = 0; c < W; c++) {
            const std::vector<Ref>& cur = col[c];
            size_t q = 0, total = cur.size() + next[c].size();  // next[c] already holds this stage's carries from column c-1
            while (total > d) {
                if (total == d + 1) {  // half adder
                    const Ref x = cur[q], y = cur[q + 1];
                    q += 2;
                    next[c].push_back(b.XOR(x, y));
                    if (c + 1 < W) next[c + 1].push_back(b.AND(x, y));
                    total -= 1;
                } else {               // full adder
                    const Ref x = cur[q], y = cur[q + 1], z = cur[q + 2];
                    q += 3;
                    const Ref t = b.XOR(x, y);
                    next[c].push_back(b.XOR(t, z));
                    if (c + 1 < W) next[c + 1].push_back(b.XOR(b.AND(x, y), b.AND(z, t)));  // the top column's carry is 2^(2n): dropped
                    total -= 2;
                }
            }
            for (; q < cur.size(); q++) next[c].push_back(cur[q]);
        }
        col.swap(next);
    }
    Word x(W), y(W);
    for (int c = 0; c < W; c++) {
        x[c] = col[c].size() > 0 ? col[c][0] : CircuitBuilder::constant(0);
        y[c] = col[c].size() > 1 ? col[c][1] : CircuitBuilder::constant(0);
    }
    return kogge_stone_add(b, x, y, CircuitBuilder::constant(0));
}

// x + y + cin as a ripple of two-bootstrap full adders: sum = XOR3, carry = MAJ3, one level per bit.  The carry out of the
// top bit is computed as the reference's add() computes it (cloud.c:43-46), though no caller here reads it.
static Word full_adder_ripple(CircuitBuilder& b, const Word& x, const Word& y, Ref cin) {
    const int n = (int)x.size();
    Word sum(n);
    Ref carry = cin;
    for (int i = 0; i < n; i++) {
        sum[i] = b.XOR3(x[i], y[i], carry);
        carry = b.MAJ3(x[i], y[i], carry);
    }
    return sum;
}

// A * B on full adders (see CIRC_MUL_FA).  Row i holds A[j] & B[i] at weight i + j.  The array keeps a sum row S and a
// carry row C; adding row i takes one full adder per column, FA(row[j], S[j+1], C[j]), and gives the next S and C and the
// product bit S[0] -- one level per row, since no carry travels inside a row.  A cell with two constant-zero operands is a
// wire (the top cell of every row: its carry is always zero); a cell with one is still a MAJ3 / XOR3 with that constant
// (row 1, whose C is all zero), which `fold` lowers to AND / XOR.  The last S and C are added by a ripple.
// Bootstraps: n*n ANDs + 2 (n-1)(n-1) in the array + 2 (n-1) in the ripple = 3 n*n - 2 n; depth 2 n - 1.
static Word full_adder_mul(CircuitBuilder& b, const Word& A, const Word& B) {
    const int n = (int)A.size();
    const Ref zero = CircuitBuilder::constant(0);
    auto is_zero = [](Ref r) { return r.id == kConstId && !r.neg; };
    // -> (sum, carry)
    auto cell = [&](Ref x, Ref y, Ref z) -> std::pair<Ref, Ref> {
        if (is_zero(y) && is_zero(z)) return {x, zero};
        if (is_zero(x) && is_zero(z)) return {y, zero};
        if (is_zero(x) && is_zero(y)) return {z, zero};
        return {b.XOR3(x, y, z), b.MAJ3(x, y, z)};
    };
    std::vector<Word> row(n, Word(n));
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) row[i][j] = b.AND(A[j], B[i]);
    Word S = row[0], C(n, zero), P(2 * n);
    P[0] = S[0];
    for (int i = 1; i < n; i++) {
        Word S2(n), C2(n);
        for (int j = 0; j < n; j++) std::tie(S2[j], C2[j]) = cell(row[i][j], j + 1 < n ? S[j + 1] : zero, C[j]);
        S.swap(S2);
        C.swap(C2);
        P[i] = S[0];
    }
    Ref carry = zero;  // weights n .. 2n-1: S[1 .. n-1] + C[0 .. n-1]; the carry out of the top bit is 2^(2n): dropped
    for (int k = 0; k < n; k++) {
        const auto sc = cell(k + 1 < n ? S[k + 1] : zero, C[k], carry);
        P[n + k] = sc.first;
        carry = sc.second;
    }
    return P;
}

// The reference's multiplier on words (cloud.c:2366-2718): 32, 64 or 128 bits, value samples LSB first.
static Word reference_mul(CircuitBuilder& b, const std::vector<Word>& Aw, const std::vector<Word>& Bw, const Word& carry1) {
    Word result;
    if (Aw.size() == 1) {  // cloud.c:2655-2718
        Word r1 = b.fresh(), r2 = b.fresh();
        b.mul_words({&r1, &r2}, {&Aw[0]}, Bw[0], carry1, 32);  // mul32, cloud.c:115-218
        result = r2;  // low word first (:2683-2686)
        result.insert(result.end(), r1.begin(), r1.end());
    } else if (Aw.size() == 2) {  // cloud.c:2568-2654
        Word r[6], f[3];
        for (auto& w : r) w = b.fresh();
        for (auto& w : f) w = b.fresh();
        b.mul_words({&r[0], &r[1], &r[2]}, {&Aw[0], &Aw[1]}, Bw[0], carry1, 32);  // :2589  mul64, cloud.c:220-385
        b.mul_words({&r[3], &r[4], &r[5]}, {&Aw[0], &Aw[1]}, Bw[1], carry1, 32);  // :2592
        b.split(f[0], f[1], f[2], r[0], r[1], r[3], r[4], r[5], carry1, 32);      // :2594
        for (const Word* w : {&r[2], &f[2], &f[1], &f[0]})                        // :2609-2616
            result.insert(result.end(), w->begin(), w->end());
    } else if (Aw.size() == 4) {  // cloud.c:2371-2567
        Word r[21], sm[16], co[16];
        for (auto& w : r) w = b.fresh();
        for (auto& w : sm) w = b.fresh();
        for (auto& w : co) w = b.fresh();
        for (int q = 0; q < 4; q++)  // :2434-2443  mul128, cloud.c:387-647
            b.mul_words({&r[5 * q + 1], &r[5 * q + 2], &r[5 * q + 3], &r[5 * q + 4], &r[5 * q + 5]}, {&Aw[0], &Aw[1], &Aw[2], &Aw[3]}, Bw[q],
                        carry1, 32);
        b.add(sm[1], co[1], r[10], r[4], carry1, 32);  // :2445-2449
        b.add(sm[2], co[2], r[9], r[3], co[1], 32);
        b.add(sm[3], co[3], r[8], r[2], co[2], 32);
        b.add(sm[4], co[4], r[7], r[1], co[3], 32);
        b.add(sm[5], co[5], r[6], carry1, co[4], 32);
        b.add(sm[6], co[6], sm[2], r[15], co[5], 32);  // :2451-2455 (carry-in = previous chain's top carry)
        b.add(sm[7], co[7], sm[3], r[14], co[6], 32);
        b.add(sm[8], co[8], sm[4], r[13], co[7], 32);
        b.add(sm[9], co[9], sm[5], r[12], co[8], 32);
        b.add(sm[10], co[10], r[11], carry1, co[9], 32);
        b.add(sm[11], co[11], sm[7], r[20], co[10], 32);  // :2457-2461
        b.add(sm[12], co[12], sm[8], r[19], co[11], 32);
        b.add(sm[13], co[13], sm[9], r[18], co[12], 32);
        b.add(sm[14], co[14], sm[10], r[17], co[13], 32);
        b.add(sm[15], co[15], r[16], carry1, co[14], 32);
        for (const Word* w : {&r[5], &sm[1], &sm[6], &sm[11], &sm[12], &sm[13], &sm[14], &sm[15]})  // :2476-2491
            result.insert(result.end(), w->begin(), w->end());
    }
    return result;
}

// One branch of main() (cloud.c:870-2718) on symbolic operands: A and B of a width the row accepts, carry = ciphertextcarry1.
// Returns the value samples LSB first.
static Word build_stage(CircuitBuilder& b, const KindRow& row, const Word& A, const Word& B, const Word& carry1) {
    if (row.family == FAMILY_REFERENCE) {
        const std::vector<Word> Aw = to_words(A), Bw = to_words(B);
        switch (row.op) {
            case OP_ADD: return chained_add(b, Aw, Bw, carry1);
            case OP_SUB: return chained_add(b, Aw, twos_complement(b, Bw), carry1);   // cloud.c:1196-1807: complement operand 2, add to operand 1
            case OP_RSUB: return chained_add(b, Bw, twos_complement(b, Aw), carry1);  // cloud.c:1809-2365: complement operand 1, add to operand 2
            case OP_MUL: return reference_mul(b, Aw, Bw, carry1);
        }
    }
    if (row.op == OP_MUL) return row.family == FAMILY_CARRY_SAVE ? wallace_mul(b, A, B) : full_adder_mul(b, A, B);
    // The opt-in adders, one rule for both families: ADD is x + y with the carry word's bit 0 as carry-in; SUB / RSUB are
    // minuend + ~subtrahend + 1, the 1 a constant carry-in (the reference's carry word encrypts 0: alice.c:147-149).
    const auto adder = row.family == FAMILY_KOGGE_STONE ? kogge_stone_add : full_adder_ripple;
    if (row.op == OP_ADD) return adder(b, A, B, carry1[0]);
    const Word& minuend = row.op == OP_SUB ? A : B;
    const Word& subtrahend = row.op == OP_SUB ? B : A;
    Word complement(subtrahend.size());
    CircuitBuilder::NOT(complement, subtrahend, subtrahend.size());
    return adder(b, minuend, complement, CircuitBuilder::constant(1));
}

Word build_word_operator(CircuitBuilder& b, int32_t kind, const Word& A, const Word& B, const Word& carry) {
    const Stages s = stages_of(kind);
    if (!s.s1 || s.s2) throw std::invalid_argument("not a plain circuit kind");
    if (A.size() != B.size()) throw std::invalid_argument("operands of different widths");
    if (A.size() > 256 || !accepts(*s.s1, (int32_t)A.size()))
        throw std::invalid_argument(std::string("kind ") + s.s1->name + " does not take operands of " + std::to_string(A.size()) + " samples");
    if (carry.size() != 32) throw std::invalid_argument("the carry word must be 32 samples");
    return build_stage(b, *s.s1, A, B, carry);
}

Word build_family_adder(CircuitBuilder& b, CircuitFamily family, const Word& x, const Word& y, Ref cin) {
    if (family != FAMILY_KOGGE_STONE && family != FAMILY_FULL_ADDER) throw std::invalid_argument("no adder of that family");
    if (x.empty() || x.size() != y.size()) throw std::invalid_argument("operands of different widths");
    return family == FAMILY_KOGGE_STONE ? kogge_stone_add(b, x, y, cin) : full_adder_ripple(b, x, y, cin);
}

bool build_circuit(int32_t kind, int32_t bits, Circuit* out, bool balanced, bool fold, int32_t level_cap) {
    if (!circuit_accepts_width(kind, bits)) return false;
    const Stages s = stages_of(kind);
    CircuitBuilder b(circuit_n_inputs(kind, bits), fold || s.s1->force_fold);
    const Word A = b.input_word(0, bits), B = b.input_word(bits, bits);
    const Word carry1 = b.input_word(2 * bits, 32);  // ciphertextcarry1
    Word result = build_stage(b, *s.s1, A, B, carry1);
    std::string name = s.s1->name;
    int32_t sched_bits = bits;
    if (s.s2) {
        // Two ./cloud runs of compute() / compute_final() (dragonfly_cipher_cloud.py:1219-1327) as
        // one DAG.  Stage 1's answer advertises bits (ADD/SUB) or 2*bits (MUL: cloud.c:833-844), the
        // third operand C is given at that width, so stage 2 runs at int_bit = w2 (cloud.c:841-855).
        // Its carry-in is operand 1's carry word (e.g. cloud.c:891): when the answer is operand 1
        // (flip) that is the answer's 11th word, which main() fills with stage 1's
        // ciphertextcarry1 (cloud.c:901-916, 2617-2626); otherwise it is C's own carry word.
        const int32_t w2 = s.w2(bits);
        const Word stage1 = result;
        const Word C = b.input_word(2 * bits + 32, w2);
        const Word carry2 = s.flip ? carry1 : b.input_word(2 * bits + 32 + w2, 32);
        result = s.flip ? build_stage(b, *s.s2, stage1, C, carry2) : build_stage(b, *s.s2, C, stage1, carry2);
        name = kind == CIRC_MULADD ? "muladd" : name + "_" + s.s2->name + (s.flip ? "" : "_r");
        if (s.s2->op == OP_MUL) sched_bits = w2;  // the wider multiplier decides the schedule below
    }
    // Schedule choice.  Measured (mul32, batches 32..1024) plain ASAP is 1-3 % faster than the
    // slack-balanced schedule -- its big early levels run at full machine width -- so the balanced
    // schedule is used where it pays in memory: the 64/128-bit multipliers, whose ASAP wire store
    // is 2.7-5.8x larger (mul128: 16 800 vs 2 921 rows of 2.5 KB per expression).
    static const char* force = getenv("IEACHE_SCHEDULE");  // "asap" | "balanced": A/B switch for measurements
    // ... and wherever the caller asks for a level width (level_cap > 0: small batches of the 32-bit multiplier, whose ASAP
    // levels swing between a fraction of a round of resident workgroups and several)
    bool use_balanced = balanced && circuit_multiplies(kind) && (sched_bits >= 64 || level_cap > 0);
    if (force && std::string(force) == "asap") use_balanced = false;
    if (force && std::string(force) == "balanced") use_balanced = balanced;
    *out = finalize_circuit(name + std::to_string(bits) + (fold ? "_folded" : ""), b, result, use_balanced, use_balanced ? level_cap : 0);
    out->n_reference_bootstraps = b.n_requested();
    out->balanced_schedule = use_balanced;
    if (!s.s2 && s.s1->ref_kind != kind) {  // an opt-in kind that is not the reference's gate list
        Circuit ref;
        if (build_circuit(s.s1->ref_kind, bits, &ref, false, false)) out->n_reference_bootstraps = ref.n_bootstraps;
    }
    return true;
}

// ASAP-scheduled wide circuits (the 32-bit multiplier and what is built on it) at small batches: their levels swing
// between a fraction of a round of resident gates and several (mul32: 1 ... 70 gates per expression around a mean of 44), so a
// level x batch is rarely a whole number of rounds.  Re-levelled with the slack-balanced scheduler to floor(m x resident /
// batch) gates per expression, m = the whole number of rounds nearest the mean level, every launch is m (almost) full rounds:
// measured +12.6 % at a batch of 58 (level width 35), +10 % at 64 (32), +8 % at 100 (40 = two rounds), +3 % at 128 (48 = three),
// nothing from 200 on.
static int32_t round_level_cap(const Circuit& base, int64_t batch, int32_t resident) {
    if (batch <= 0 || resident <= 0 || base.depth <= 0) return 0;
    const int64_t mean = (base.n_bootstraps + base.depth - 1) / base.depth;
    if (mean < 8 || base.depth < 128) return 0;  // adders have nothing to balance; the shallow carry-save trees are all critical path
    const int64_t m = (2 * mean * batch + resident) / (2 * (int64_t)resident);  // rounds per mean level, to nearest
    if (m < 1 || m > 3) return 0;
    const int64_t cap = m * resident / batch;
    if (cap * 10 < mean * 6) return 0;  // far below the mean: too many levels
    return (int32_t)cap;
}

// Balanced circuits: the multiple of resident / gcd(resident, batch) nearest to the mean width (see circuit.h).
static int32_t quantum_level_cap(const Circuit& base, int64_t batch, int32_t resident) {
    if (batch <= 0 || resident <= 0 || base.depth <= 0 || batch >= resident) return 0;
    const int64_t mean = (base.n_bootstraps + base.depth - 1) / base.depth;
    // a circuit whose default schedule already needs levels far above the mean has no slack to flatten
    // (the carry-save multipliers: their trees are all critical path); stretching it only adds levels
    if (base.sched_max_width > 2 * mean) return 0;
    if (mean * batch < resident) return 0;  // under one round per level: narrow levels are the cheap ones
    int64_t a = resident, b = batch;
    while (b) {
        const int64_t t = a % b;
        a = b;
        b = t;
    }
    const int64_t q = resident / a;  // gates per expression that make one level a whole number of rounds
    if (q <= 1 || 2 * q > 3 * mean) return 0;  // a quantum far above what the circuit offers per level cannot be filled
    const int64_t k = std::max<int64_t>(1, (mean + q / 2) / q);
    return (int32_t)(k * q);
}

int32_t circuit_level_cap(const Circuit& base, int64_t batch, int32_t resident, int32_t resident_alt) {
    if (!base.balanced_schedule) return round_level_cap(base, batch, resident);
    // resident_alt: a second, smaller residency the evaluator also runs efficiently (the two-waves-per-gate kernel's 4 per
    // CU below the one-wave kernel's 8 per CU): tried when the batch is too small to fill levels of the first
    const int32_t cap = quantum_level_cap(base, batch, resident);
    return cap > 0 || resident_alt <= 0 ? cap : quantum_level_cap(base, batch, resident_alt);
}

RecordedNetlist export_recorded(const CircuitBuilder& b, const Word& outputs) {
    auto ref = [](Ref r) -> int32_t { return r.id < 0 ? (r.neg ? -1 : -2) : (int32_t)((uint32_t)r.id << 1 | (r.neg ? 1u : 0u)); };
    RecordedNetlist out;
    const std::vector<Gate>& gates = b.gates();
    out.gates.resize(gates.size());
    for (size_t i = 0; i < gates.size(); i++) {
        const Gate& g = gates[i];
        const int32_t requested = b.requested_types()[i];
        Ref x = g.a, y = g.b;
        if (requested != g.type) {  // undo gate2's lowering: the operand signs it flipped
            if (requested == GATE_NOR || requested == GATE_ANDNY || requested == GATE_ORNY) x.neg = !x.neg;
            if (requested == GATE_NOR || requested == GATE_ANDYN || requested == GATE_ORYN) y.neg = !y.neg;
        }
        const bool three = g.type == GATE_MUX || is_gate3(g.type);
        out.gates[i] = NetGate{requested, ref(x), ref(y), three ? ref(g.c) : 0};
    }
    out.outputs.resize(outputs.size());
    for (size_t i = 0; i < outputs.size(); i++) out.outputs[i] = ref(outputs[i]);
    return out;
}

Circuit build_netlist(int32_t n_inputs, const NetGate* gates, size_t n_gates, const int32_t* outputs, size_t n_outputs,
                      bool balanced, RecordedNetlist* recorded) {
    auto bad = [](const std::string& msg) { throw std::invalid_argument("netlist: " + msg); };
    if (n_inputs < 1) bad("needs at least one input");
    if (n_outputs < 1 || !outputs) bad("needs at least one output");
    if (n_gates && !gates) bad("null gate list");
    // a reference is wire << 1 | negated in an int32_t; slots, level offsets and widths (a MUX counts 2) are int32_t
    constexpr int64_t kMaxWires = (int64_t)1 << 30;
    if ((int64_t)n_inputs + (int64_t)n_gates >= kMaxWires || n_gates >= (size_t)kMaxWires)
        bad("too large: inputs + gates must stay under 2^30 (gate " + std::to_string(kMaxWires - n_inputs) + " has no wire number)");
    if (n_outputs >= (size_t)kMaxWires) bad("too many outputs");
    CircuitBuilder b(n_inputs, /*fold=*/false);
    // -> the sample a reference names; `limit`: wires defined so far
    auto ref = [&](int32_t r, int64_t limit, const std::string& where) -> Ref {
        if (r == -1) return CircuitBuilder::constant(1);
        if (r == -2) return CircuitBuilder::constant(0);
        if (r < 0) bad(where + " is not a reference (" + std::to_string(r) + ")");
        const int32_t w = r >> 1;
        if (w >= limit)
            bad(where + " refers to wire " + std::to_string(w) + ", which is not defined there (" + std::to_string(limit) + " wires so far)");
        return Ref{w, (r & 1) != 0};
    };
    for (size_t g = 0; g < n_gates; g++) {
        const NetGate& ng = gates[g];
        const std::string at = "gate " + std::to_string(g);
        if ((ng.type < 0 || ng.type >= GATE_TYPES) && !is_gate3(ng.type)) bad(at + ": unknown gate type " + std::to_string(ng.type));
        const int64_t limit = (int64_t)n_inputs + (int64_t)g;
        const Ref a = ref(ng.a, limit, at + ": operand a"), bb = ref(ng.b, limit, at + ": operand b");
        if (ng.type == GATE_MUX) {
            b.gate3(GATE_MUX, a, bb, ref(ng.c, limit, at + ": operand c"));
        } else if (is_gate3(ng.type)) {
            const Ref cc = ref(ng.c, limit, at + ": operand c");
            // the same wire twice adds its noise coherently (XOR3(a,a,a): 13 sigma instead of 19): refused, constants may repeat
            if ((a.id >= 0 && (a.id == bb.id || a.id == cc.id)) || (bb.id >= 0 && bb.id == cc.id))
                bad(at + ": a three-input gate must name three different wires (constants may repeat)");
            b.gate3(ng.type, a, bb, cc);
        } else {
            if (ng.c != 0) bad(at + ": a two-input gate takes no third operand (c must be 0)");
            b.gate(ng.type, a, bb);
        }
    }
    Word outs(n_outputs);
    for (size_t i = 0; i < n_outputs; i++)
        outs[i] = ref(outputs[i], (int64_t)n_inputs + (int64_t)n_gates, "output " + std::to_string(i) + " (after gate " + std::to_string(n_gates) + ")");
    Circuit c = finalize_circuit("netlist", b, outs, balanced, 0);
    c.n_reference_bootstraps = c.n_bootstraps;
    if (recorded) *recorded = export_recorded(b, outs);
    return c;
}

void simulate_circuit(const Circuit& c, const uint8_t* in, uint8_t* out) {
    std::vector<uint8_t> store(c.n_slots, 0);
    for (int32_t i = 0; i < c.n_inputs; i++) store[i] = in[i] & 1;
    auto val = [&](int32_t slot, int32_t neg) -> uint8_t {
        const uint8_t v = slot >= 0 ? store[slot] : 0;
        return v ^ (uint8_t)(neg & 1);
    };
    for (int32_t L = 1; L <= c.n_levels(); L++) {
        // A model of the levelised DAG, not of the executor: every operand of the level is read before any output is written.
        // The GPU runs a level in pieces (chunks, two lanes, pipelines), one piece's outputs written before the next piece's
        // operands are read; that this gives the same result -- no gate of a level writes a slot the level reads -- is what
        // tests/native/circuit_store_test.cpp checks, by executing the slot table with every output written at once.
        const int32_t lo = c.level_offset[L - 1], hi = c.level_offset[L];
        std::vector<uint8_t> res(hi - lo);
        for (int32_t g = lo; g < hi; g++) {
            const DevGate& d = c.gates[g];
            const uint8_t a = val(d.a_slot, d.a_neg), b = val(d.b_slot, d.b_neg);
            uint8_t r = 0;
            switch (d.type) {
                case GATE_AND: r = a & b; break;
                case GATE_XOR: r = a ^ b; break;
                case GATE_OR: r = a | b; break;
                case GATE_NAND: r = !(a & b); break;
                case GATE_XNOR: r = !(a ^ b); break;
                case GATE_MUX: r = a ? b : val(d.c_slot, d.c_neg); break;
                case GATE_MAJ3: r = (uint8_t)((a + b + val(d.c_slot, d.c_neg)) >= 2); break;
                case GATE_XOR3: r = a ^ b ^ val(d.c_slot, d.c_neg); break;
            }
            res[g - lo] = r;
        }
        for (int32_t g = lo; g < hi; g++) store[c.gates[g].out_slot] = res[g - lo];
    }
    for (size_t i = 0; i < c.outputs.size(); i++) out[i] = val(c.outputs[i].slot, c.outputs[i].neg);
}

}  // namespace ieache
