// The wire store as the GPU uses it (ie-ache_amd/csrc/circuit.cpp: finalize_circuit), as plain host C++ under
// AddressSanitizer / UBSan.  The executor cuts a level into pieces ("chunk"), level halves on two lanes and expression
// pipelines: a piece's key switch writes its output slots before -- or while -- the next piece reads its operands.  That is
// only right if no gate of a level writes a slot any gate of the same level reads, which simulate_circuit(), reading a whole
// level before it writes, cannot see.  Here every Circuit is executed on symbolic values with each output written the
// moment its gate runs, the gates of a level taken forwards and again backwards, and compared with the builder's own gate
// list; the hazards, the level layout and the bounds are checked directly as well.
// Built and run by tests/test_circuit_store_cpu.py.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "../../ie-ache_amd/csrc/circuit.h"

using namespace ieache;

namespace {

struct Rng {  // xorshift64*
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x1234567ull) {}
    uint64_t next() {
        s ^= s >> 12;
        s ^= s << 25;
        s ^= s >> 27;
        return s * 0x2545F4914F6CDD1Dull;
    }
    int below(int n) { return (int)(next() % (uint64_t)n); }
    bool chance(int percent) { return below(100) < percent; }
};

// Hash-consed expressions over input ids and the constant.  A value is expression << 1 | negated.
constexpr int32_t kEmpty = -1;
struct Exprs {
    std::map<std::array<int32_t, 4>, int32_t> known;
    int32_t n = 0;
    int32_t constant;  // bootsCONSTANT(0)
    explicit Exprs(int32_t n_inputs) : n(n_inputs), constant(n_inputs) { n++; }
    int32_t gate(int32_t type, int32_t a, int32_t b, int32_t c) {
        const auto it = known.emplace(std::array<int32_t, 4>{type, a, b, c}, n);
        if (it.second) n++;
        return it.first->second;
    }
};

std::string g_case;
int g_failures = 0;
#define FAIL(...)                                        \
    do {                                                 \
        fprintf(stderr, "%s: ", g_case.c_str());         \
        fprintf(stderr, __VA_ARGS__);                    \
        fprintf(stderr, " (%s:%d)\n", __FILE__, __LINE__); \
        g_failures++;                                    \
        return false;                                    \
    } while (0)
#define REQUIRE(c)                       \
    do {                                 \
        if (!(c)) FAIL("violated: %s", #c); \
    } while (0)

// the builder's gates as expressions: per wire, and how often each expression is computed
struct Wanted {
    std::vector<int32_t> of_wire;
    std::map<int32_t, int> count;
    int32_t depth = 0, asap_width = 0;
    int64_t rotations = 0, n_mux = 0;
};

Wanted wanted_of(const CircuitBuilder& b, Exprs& ex) {
    Wanted w;
    w.of_wire.assign((size_t)b.n_wires(), kEmpty);
    std::vector<int32_t> level((size_t)b.n_wires(), 0), width;
    for (int32_t i = 0; i < b.n_inputs(); i++) w.of_wire[(size_t)i] = i;
    auto val = [&](const Ref& r) { return ((r.id >= 0 ? w.of_wire[(size_t)r.id] : ex.constant) << 1) | (int32_t)r.neg; };
    for (const Gate& g : b.gates()) {
        const bool mux = g.type == GATE_MUX;
        int32_t lv = 0;  // the longest path, from the operands alone
        for (const Ref& r : {g.a, g.b, g.c})  // (c is the constant on a two-input gate)
            if (r.id >= 0) lv = std::max(lv, level[(size_t)r.id]);
        level[(size_t)g.out] = ++lv;
        if ((size_t)lv >= width.size()) width.resize((size_t)lv + 1, 0);
        width[(size_t)lv] += mux ? 2 : 1;
        w.depth = std::max(w.depth, lv);
        const int32_t e = ex.gate(g.type, val(g.a), val(g.b), mux ? val(g.c) : 0);
        w.of_wire[(size_t)g.out] = e;
        w.count[e]++;
        w.rotations += mux ? 2 : 1;
        w.n_mux += mux;
    }
    for (int32_t x : width) w.asap_width = std::max(w.asap_width, x);
    return w;
}

bool check_circuit(const CircuitBuilder& b, const Word& outputs, const Circuit& c, bool balanced, int32_t cap) {
    const int32_t n_gates = (int32_t)b.gates().size(), L_n = c.n_levels();
    Exprs ex(b.n_inputs());
    const Wanted w = wanted_of(b, ex);

    // ---- bounds and statistics ----
    REQUIRE(c.n_inputs == b.n_inputs());
    REQUIRE((int32_t)c.gates.size() == n_gates);
    REQUIRE(c.n_slots >= c.n_inputs && c.n_slots <= c.n_inputs + n_gates);
    REQUIRE(c.depth == w.depth && c.max_width == w.asap_width);
    REQUIRE(c.n_bootstraps == w.rotations);
    REQUIRE(L_n >= w.depth && (L_n == w.depth || (balanced && cap > 0)));
    REQUIRE((int32_t)c.level_offset.size() == L_n + 1 && c.level_offset[0] == 0 && c.level_offset[(size_t)L_n] == n_gates);
    REQUIRE((int32_t)c.level_mux.size() == L_n);
    int64_t by_type[GATE_TYPES] = {}, total = 0;
    for (int32_t t : b.requested_types()) by_type[t]++;
    for (int t = 0; t < GATE_TYPES; t++) {
        REQUIRE(c.n_by_type[t] == by_type[t]);
        total += c.n_by_type[t];
    }
    REQUIRE(total == n_gates && c.n_by_type[GATE_MUX] == w.n_mux);
    auto slot_ok = [&](int32_t s) { return s >= -1 && s < c.n_slots; };
    for (const DevGate& d : c.gates) {
        REQUIRE(d.type == GATE_AND || d.type == GATE_XOR || d.type == GATE_OR || d.type == GATE_NAND || d.type == GATE_XNOR || d.type == GATE_MUX);
        REQUIRE(slot_ok(d.a_slot) && slot_ok(d.b_slot) && slot_ok(d.c_slot) && d.out_slot >= 0 && d.out_slot < c.n_slots);
        REQUIRE((d.a_neg | 1) == 1 && (d.b_neg | 1) == 1 && (d.c_neg | 1) == 1);
        if (d.type != GATE_MUX) REQUIRE(d.c_neg == 0 && d.c_slot == -1);
    }

    // ---- level layout and level hazards ----
    int32_t widest = 0;
    int64_t mux_total = 0;
    for (int32_t L = 1; L <= L_n; L++) {
        const int32_t lo = c.level_offset[(size_t)L - 1], hi = c.level_offset[(size_t)L], nm = c.level_mux[(size_t)L - 1];
        REQUIRE(lo <= hi && nm >= 0 && nm <= hi - lo && c.n_mux(L) == nm);
        for (int32_t g = lo; g < hi; g++) REQUIRE((c.gates[(size_t)g].type == GATE_MUX) == (g >= hi - nm));  // counted exactly, and last
        widest = std::max(widest, hi - lo + nm);
        mux_total += nm;
        std::vector<char> written((size_t)c.n_slots, 0), read((size_t)c.n_slots, 0);
        for (int32_t g = lo; g < hi; g++) {
            const DevGate& d = c.gates[(size_t)g];
            if (written[(size_t)d.out_slot]) FAIL("level %d: two gates write slot %d", L, d.out_slot);
            written[(size_t)d.out_slot] = 1;
            for (int32_t s : {d.a_slot, d.b_slot, d.type == GATE_MUX ? d.c_slot : -1})
                if (s >= 0) read[(size_t)s] = 1;
        }
        for (int32_t s = 0; s < c.n_slots; s++)
            if (written[(size_t)s] && read[(size_t)s]) FAIL("level %d writes slot %d, which a gate of the same level reads", L, s);
    }
    REQUIRE(c.sched_max_width == widest && mux_total == w.n_mux);

    // ---- piecewise execution: each output slot written the moment its gate runs ----
    for (int reverse = 0; reverse < 2; reverse++) {
        std::vector<int32_t> store((size_t)c.n_slots, kEmpty), born((size_t)c.n_slots, -1);
        for (int32_t i = 0; i < c.n_inputs; i++) {
            store[(size_t)i] = i;
            born[(size_t)i] = 0;
        }
        std::map<int32_t, int> count;
        for (int32_t L = 1; L <= L_n; L++) {
            const int32_t lo = c.level_offset[(size_t)L - 1], hi = c.level_offset[(size_t)L];
            for (int32_t k = 0; k < hi - lo; k++) {
                const int32_t g = reverse ? hi - 1 - k : lo + k;
                const DevGate& d = c.gates[(size_t)g];
                int32_t v[3] = {0, 0, 0};
                const int32_t slots[3] = {d.a_slot, d.b_slot, d.c_slot}, negs[3] = {d.a_neg, d.b_neg, d.c_neg};
                for (int o = 0; o < (d.type == GATE_MUX ? 3 : 2); o++) {
                    int32_t e = ex.constant;
                    if (slots[o] >= 0) {
                        e = store[(size_t)slots[o]];
                        if (e == kEmpty) FAIL("%s: level %d gate %d reads slot %d, which holds nothing", reverse ? "backwards" : "forwards", L, g, slots[o]);
                        if (born[(size_t)slots[o]] >= L)
                            FAIL("%s: level %d gate %d reads slot %d, written in level %d", reverse ? "backwards" : "forwards", L, g, slots[o], born[(size_t)slots[o]]);
                    }
                    v[o] = (e << 1) | negs[o];
                }
                const int32_t e = ex.gate(d.type, v[0], v[1], v[2]);
                store[(size_t)d.out_slot] = e;
                born[(size_t)d.out_slot] = L;
                count[e]++;
            }
        }
        if (count != w.count) FAIL("%s: the gates executed on the store are not the builder's gates", reverse ? "backwards" : "forwards");
        REQUIRE(c.outputs.size() == outputs.size());
        for (size_t i = 0; i < outputs.size(); i++) {
            const OutRef& o = c.outputs[i];
            REQUIRE(o.slot >= -1 && o.slot < c.n_slots && o.neg == (int32_t)outputs[i].neg);
            if (outputs[i].id < 0) {
                REQUIRE(outputs[i].id == kConstId && o.slot == -1);
            } else {
                REQUIRE(o.slot >= 0);
                if (store[(size_t)o.slot] != w.of_wire[(size_t)outputs[i].id])
                    FAIL("%s: output %zu (wire %d) is not in slot %d after the last level", reverse ? "backwards" : "forwards", i, outputs[i].id, o.slot);
            }
        }
    }
    return true;
}

// the plain walk of the builder's gates on bits, against simulate_circuit
bool check_simulation(const CircuitBuilder& b, const Word& outputs, const Circuit& c, Rng& rng) {
    std::vector<uint8_t> in((size_t)b.n_inputs()), wire((size_t)b.n_wires(), 0), got(outputs.size(), 2);
    for (size_t i = 0; i < in.size(); i++) wire[i] = in[i] = (uint8_t)rng.below(2);
    auto val = [&](const Ref& r) { return (uint8_t)((r.id >= 0 ? wire[(size_t)r.id] : 0) ^ (uint8_t)r.neg); };
    for (const Gate& g : b.gates()) {
        const uint8_t x = val(g.a), y = val(g.b);
        uint8_t r = 0;
        switch (g.type) {
            case GATE_AND: r = x & y; break;
            case GATE_XOR: r = x ^ y; break;
            case GATE_OR: r = x | y; break;
            case GATE_NAND: r = !(x & y); break;
            case GATE_XNOR: r = !(x ^ y); break;
            case GATE_MUX: r = x ? y : val(g.c); break;
            default: FAIL("builder recorded type %d", g.type);
        }
        wire[(size_t)g.out] = r;
    }
    simulate_circuit(c, in.data(), got.data());
    for (size_t i = 0; i < outputs.size(); i++)
        if (got[i] != val(outputs[i])) FAIL("simulate_circuit: output %zu", i);
    return true;
}

int g_circuits = 0;

// every schedule of one recorded DAG
bool check_all_schedules(const std::string& name, const CircuitBuilder& b, const Word& outputs, const std::vector<int32_t>& caps, Rng& rng) {
    for (int balanced = 0; balanced < 2; balanced++)
        for (int32_t cap : balanced ? caps : std::vector<int32_t>{0}) {
            g_case = name + (balanced ? " balanced cap " + std::to_string(cap) : " asap");
            const Circuit c = finalize_circuit("t", b, outputs, balanced != 0, cap);
            if (!check_circuit(b, outputs, c, balanced != 0, cap) || !check_simulation(b, outputs, c, rng)) return false;
            g_circuits++;
        }
    return true;
}

// A random DAG through the builder.  The knobs are drawn per DAG so that the corpus holds deep narrow chains (small window),
// long-lived wires (no window), MUX-only and MUX-free levels, constants in every position, the same wire on several
// operands, and wires and inputs nobody reads.
bool random_dag(uint64_t seed) {
    Rng rng(seed);
    const int32_t n_inputs = 1 + rng.below(6);
    const bool fold = rng.chance(30);
    const int n_gates = rng.chance(4) ? 0 : 1 + rng.below(48);
    const int window = rng.chance(40) ? 1 + rng.below(4) : (rng.chance(50) ? 8 : 1 << 20);
    const int p_mux = rng.chance(15) ? 100 : (rng.chance(20) ? 0 : 10 + rng.below(40));
    const int p_const = rng.chance(50) ? 0 : 5 + rng.below(25);
    const int p_same = rng.chance(60) ? 0 : 10 + rng.below(30);
    const int p_neg = rng.below(60);
    const int p_dead = rng.chance(50) ? 0 : 10 + rng.below(40);
    static const int32_t kTwoInput[] = {GATE_AND, GATE_XOR, GATE_OR, GATE_NAND, GATE_NOR, GATE_XNOR, GATE_ANDNY, GATE_ANDYN, GATE_ORNY, GATE_ORYN};
    CircuitBuilder b(n_inputs, fold);
    std::vector<Ref> pool;  // what later gates may read
    std::vector<Ref> all;   // everything recorded, for the outputs
    const int hidden_inputs = n_inputs > 1 && rng.chance(30) ? 1 : 0;  // an input no gate reads
    for (int32_t i = 0; i < n_inputs; i++) {
        all.push_back(b.input(i));
        if (i < n_inputs - hidden_inputs) pool.push_back(b.input(i));
    }
    auto pick = [&]() -> Ref {
        if (rng.chance(p_const)) return CircuitBuilder::constant(rng.below(2));
        const int span = std::min<int>(window, (int)pool.size());
        Ref r = pool[pool.size() - 1 - (size_t)rng.below(span)];
        if (rng.chance(p_neg)) r = CircuitBuilder::NOT(r);
        return r;
    };
    for (int i = 0; i < n_gates; i++) {
        Ref a = pick(), x = pick(), y = pick();
        if (rng.chance(p_same)) {
            x = rng.chance(50) ? a : CircuitBuilder::NOT(a);
            if (rng.chance(50)) y = rng.chance(50) ? x : a;
        }
        const Ref out = rng.chance(p_mux) ? b.gate3(GATE_MUX, a, x, y) : b.gate(kTwoInput[rng.below(10)], a, x);
        all.push_back(out);
        if (!rng.chance(p_dead)) pool.push_back(out);
    }
    Word outputs;
    const int n_out = 1 + rng.below(7);
    for (int i = 0; i < n_out; i++) {
        Ref r = rng.chance(10) ? CircuitBuilder::constant(rng.below(2)) : all[(size_t)rng.below((int)all.size())];
        if (rng.chance(20)) r = all[all.size() - 1 - (size_t)rng.below(std::min<int>(3, (int)all.size()))];
        if (rng.chance(30)) r = CircuitBuilder::NOT(r);
        outputs.push_back(r);
        if (rng.chance(15)) outputs.push_back(r);  // the same sample twice
    }
    return check_all_schedules("dag " + std::to_string(seed) + (fold ? " folded" : ""), b, outputs, {0, 1, 2, 3, 7}, rng);
}

// cloud.c's own DAGs, under the level widths round_level_cap() really produces; 8 and 35 are below the multiplier's mean
// width (44), so those schedules are stretched
bool reference_dags() {
    Rng rng(99);
    const std::vector<int32_t> caps = {0, 8, 35, 44, 70};
    for (int fold = 0; fold < 2; fold++) {
        CircuitBuilder a(64, fold != 0);
        Word sum = CircuitBuilder::fresh(16), co = CircuitBuilder::fresh();
        a.add(sum, co, a.input_word(0, 16), a.input_word(16, 16), a.input_word(32, 32), 16);
        if (!check_all_schedules(fold ? "add16 folded" : "add16", a, sum, caps, rng)) return false;
        CircuitBuilder m(96, fold != 0);
        Word r1 = CircuitBuilder::fresh(), r2 = CircuitBuilder::fresh();
        m.mul32(r1, r2, m.input_word(0, 32), m.input_word(32, 32), m.input_word(64, 32), 32);
        Word product = r2;
        product.insert(product.end(), r1.begin(), r1.end());
        if (!check_all_schedules(fold ? "mul32 folded" : "mul32", m, product, caps, rng)) return false;
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const int n_dags = argc > 1 ? atoi(argv[1]) : 4000;
    for (int s = 1; s <= n_dags; s++)
        if (!random_dag((uint64_t)s)) return 1;
    if (!reference_dags()) return 1;
    printf("CIRCUIT_STORE_OK circuits=%d\n", g_circuits);
    return 0;
}
