// The wire store under circuits that hold the three-input gates GATE_MAJ3 / GATE_XOR3 (ie-ache_amd/csrc/circuit.cpp), as plain
// host C++ under AddressSanitizer / UBSan -- the companion of circuit_store_test.cpp, whose DAGs hold none.  A three-input gate
// reads a third slot; if liveness did not count that read, the slot could be handed to another gate of the same or an
// earlier level, which simulate_circuit(), reading a whole level before it writes, cannot see.  Every Circuit is therefore
// executed with each output written the moment its gate runs, the gates of a level taken forwards and again backwards:
// random DAGs on symbolic values against the builder's own gate list, add16_fa and mul32_fa on bits against integer
// arithmetic; level hazards are checked directly, the third operand counted as a read.
// Built and run by tests/test_three_input_store_cpu.py.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../ie-ache_amd/csrc/circuit.h"

using namespace ieache;

namespace {

struct Rng {  // xorshift64*
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x7654321ull) {}
    uint64_t next() {
        s ^= s >> 12;
        s ^= s << 25;
        s ^= s >> 27;
        return s * 0x2545F4914F6CDD1Dull;
    }
    int below(int n) { return (int)(next() % (uint64_t)n); }
    bool chance(int percent) { return below(100) < percent; }
};

std::string g_case;
#define FAIL(...)                                          \
    do {                                                   \
        fprintf(stderr, "%s: ", g_case.c_str());           \
        fprintf(stderr, __VA_ARGS__);                      \
        fprintf(stderr, " (%s:%d)\n", __FILE__, __LINE__); \
        return false;                                      \
    } while (0)
#define REQUIRE(c)                          \
    do {                                    \
        if (!(c)) FAIL("violated: %s", #c); \
    } while (0)

bool reads_c(int32_t type) { return type == GATE_MUX || is_gate3(type); }

// bounds, level layout and level hazards of a finished circuit; -> gates of the two new types
bool check_layout(const Circuit& c, int64_t* n_gate3) {
    const int32_t L_n = c.n_levels();
    REQUIRE((int32_t)c.level_offset.size() == L_n + 1 && c.level_offset[0] == 0 && c.level_offset[(size_t)L_n] == (int32_t)c.gates.size());
    auto slot_ok = [&](int32_t s) { return s >= -1 && s < c.n_slots; };
    int64_t maj3 = 0, xor3 = 0, rotations = 0;
    for (const DevGate& d : c.gates) {
        REQUIRE(d.type == GATE_AND || d.type == GATE_XOR || d.type == GATE_OR || d.type == GATE_NAND || d.type == GATE_XNOR || d.type == GATE_MUX ||
                d.type == GATE_MAJ3 || d.type == GATE_XOR3);
        REQUIRE(slot_ok(d.a_slot) && slot_ok(d.b_slot) && slot_ok(d.c_slot) && d.out_slot >= 0 && d.out_slot < c.n_slots);
        REQUIRE((d.a_neg | 1) == 1 && (d.b_neg | 1) == 1 && (d.c_neg | 1) == 1);
        if (!reads_c(d.type)) REQUIRE(d.c_neg == 0 && d.c_slot == -1);
        maj3 += d.type == GATE_MAJ3;
        xor3 += d.type == GATE_XOR3;
        rotations += d.type == GATE_MUX ? 2 : 1;  // a three-input gate is ONE rotation
    }
    REQUIRE(c.n_maj3 == maj3 && c.n_xor3 == xor3 && c.n_bootstraps == rotations);
    REQUIRE(c.count_of(GATE_MAJ3) == maj3 && c.count_of(GATE_XOR3) == xor3 && c.count_of(11) == -1 && c.count_of(34) == -1);
    int64_t typed = 0;
    for (int t = 0; t < GATE_TYPES; t++) typed += c.n_by_type[t];
    REQUIRE(typed + maj3 + xor3 == (int64_t)c.gates.size());
    for (int32_t L = 1; L <= L_n; L++) {
        const int32_t lo = c.level_offset[(size_t)L - 1], hi = c.level_offset[(size_t)L], nm = c.n_mux(L);
        // three-input gates are ordinary items: only the MUX gates are moved to the end of a level
        for (int32_t g = lo; g < hi; g++) REQUIRE((c.gates[(size_t)g].type == GATE_MUX) == (g >= hi - nm));
        std::vector<char> written((size_t)c.n_slots, 0), read((size_t)c.n_slots, 0);
        for (int32_t g = lo; g < hi; g++) {
            const DevGate& d = c.gates[(size_t)g];
            if (written[(size_t)d.out_slot]) FAIL("level %d: two gates write slot %d", L, d.out_slot);
            written[(size_t)d.out_slot] = 1;
            for (int32_t s : {d.a_slot, d.b_slot, reads_c(d.type) ? d.c_slot : -1})
                if (s >= 0) read[(size_t)s] = 1;
        }
        for (int32_t s = 0; s < c.n_slots; s++)
            if (written[(size_t)s] && read[(size_t)s]) FAIL("level %d writes slot %d, which a gate of the same level reads", L, s);
    }
    *n_gate3 = maj3 + xor3;
    return true;
}

// Piecewise execution on values of type V: eval(type, a, b, c) with operands already negated by `neg`.  A slot must hold
// something, written in an EARLIER level, when a gate reads it.
template <class V, class Neg, class Eval>
bool run_piecewise(const Circuit& c, bool reverse, std::vector<V>& store, V empty, V constant, Neg neg, Eval eval) {
    std::vector<int32_t> born((size_t)c.n_slots, -1);
    for (int32_t i = 0; i < c.n_inputs; i++) born[(size_t)i] = 0;
    const char* dir = reverse ? "backwards" : "forwards";
    for (int32_t L = 1; L <= c.n_levels(); L++) {
        const int32_t lo = c.level_offset[(size_t)L - 1], hi = c.level_offset[(size_t)L];
        for (int32_t k = 0; k < hi - lo; k++) {
            const int32_t g = reverse ? hi - 1 - k : lo + k;
            const DevGate& d = c.gates[(size_t)g];
            const int32_t slots[3] = {d.a_slot, d.b_slot, d.c_slot}, negs[3] = {d.a_neg, d.b_neg, d.c_neg};
            V v[3] = {constant, constant, constant};
            for (int o = 0; o < (reads_c(d.type) ? 3 : 2); o++) {
                V e = constant;
                if (slots[o] >= 0) {
                    e = store[(size_t)slots[o]];
                    if (e == empty) FAIL("%s: level %d gate %d reads slot %d, which holds nothing", dir, L, g, slots[o]);
                    if (born[(size_t)slots[o]] >= L) FAIL("%s: level %d gate %d reads slot %d, written in level %d", dir, L, g, slots[o], born[(size_t)slots[o]]);
                }
                v[o] = neg(e, negs[o]);
            }
            store[(size_t)d.out_slot] = eval(d.type, v[0], v[1], reads_c(d.type) ? v[2] : neg(constant, 0));
            born[(size_t)d.out_slot] = L;
        }
    }
    return true;
}

uint8_t gate_bit(int32_t type, uint8_t x, uint8_t y, uint8_t z) {
    switch (type) {
        case GATE_AND: return x & y;
        case GATE_XOR: return x ^ y;
        case GATE_OR: return x | y;
        case GATE_NAND: return !(x & y);
        case GATE_XNOR: return !(x ^ y);
        case GATE_MUX: return x ? y : z;
        case GATE_MAJ3: return (uint8_t)(x + y + z >= 2);
        case GATE_XOR3: return x ^ y ^ z;
    }
    return 2;
}

// the circuit on bits, piecewise in both directions and through simulate_circuit: all three must give `want`
bool check_bits(const Circuit& c, const std::vector<uint8_t>& in, const std::vector<uint8_t>& want) {
    REQUIRE(c.outputs.size() == want.size() && (size_t)c.n_inputs == in.size());
    std::vector<uint8_t> got(want.size(), 2);
    simulate_circuit(c, in.data(), got.data());
    if (got != want) FAIL("simulate_circuit gives another result");
    for (int reverse = 0; reverse < 2; reverse++) {
        std::vector<uint8_t> store((size_t)c.n_slots, 9);
        std::copy(in.begin(), in.end(), store.begin());
        if (!run_piecewise<uint8_t>(c, reverse != 0, store, 9, 0, [](uint8_t v, int32_t n) { return (uint8_t)(v ^ (uint8_t)n); }, gate_bit)) return false;
        for (size_t i = 0; i < want.size(); i++) {
            const OutRef& o = c.outputs[i];
            const uint8_t v = (uint8_t)((o.slot >= 0 ? store[(size_t)o.slot] : 0) ^ (uint8_t)o.neg);
            if (v != want[i]) FAIL("%s: output %zu is %d, not %d", reverse ? "backwards" : "forwards", i, v, want[i]);
        }
    }
    return true;
}

int g_circuits = 0;
int64_t g_gate3 = 0;

// Hash-consed expressions over input ids and the constant.  A value is expression << 1 | negated.
struct Exprs {
    std::map<std::array<int32_t, 4>, int32_t> known;
    int32_t n, constant;
    explicit Exprs(int32_t n_inputs) : n(n_inputs + 1), constant(n_inputs) {}
    int32_t gate(int32_t type, int32_t a, int32_t b, int32_t c) {
        const auto it = known.emplace(std::array<int32_t, 4>{type, a, b, c}, n);
        if (it.second) n++;
        return it.first->second;
    }
};

// every schedule of one recorded DAG, on symbolic values against the builder's gate list and on bits against its plain walk
bool check_all_schedules(const std::string& name, const CircuitBuilder& b, const Word& outputs, const std::vector<int32_t>& caps, Rng& rng) {
    for (int balanced = 0; balanced < 2; balanced++)
        for (int32_t cap : balanced ? caps : std::vector<int32_t>{0}) {
            g_case = name + (balanced ? " balanced cap " + std::to_string(cap) : " asap");
            const Circuit c = finalize_circuit("t", b, outputs, balanced != 0, cap);
            int64_t n3 = 0;
            if (!check_layout(c, &n3)) return false;
            REQUIRE(c.n_inputs == b.n_inputs() && c.gates.size() == b.gates().size());
            // the builder's gates as expressions, per wire, and how often each is computed
            Exprs ex(b.n_inputs());
            std::vector<int32_t> of_wire((size_t)b.n_wires(), -1);
            std::map<int32_t, int> wanted;
            for (int32_t i = 0; i < b.n_inputs(); i++) of_wire[(size_t)i] = i;
            auto val = [&](const Ref& r) { return ((r.id >= 0 ? of_wire[(size_t)r.id] : ex.constant) << 1) | (int32_t)r.neg; };
            for (const Gate& g : b.gates()) {
                const int32_t e = ex.gate(g.type, val(g.a), val(g.b), reads_c(g.type) ? val(g.c) : ex.constant << 1);
                of_wire[(size_t)g.out] = e;
                wanted[e]++;
            }
            for (int reverse = 0; reverse < 2; reverse++) {
                std::vector<int32_t> store((size_t)c.n_slots, -1);
                for (int32_t i = 0; i < c.n_inputs; i++) store[(size_t)i] = i << 1;
                std::map<int32_t, int> count;
                const bool ok = run_piecewise<int32_t>(
                    c, reverse != 0, store, -1, ex.constant << 1, [](int32_t v, int32_t n) { return v ^ n; },
                    [&](int32_t type, int32_t x, int32_t y, int32_t z) {
                        const int32_t e = ex.gate(type, x, y, z);
                        count[e]++;
                        return e << 1;
                    });
                if (!ok) return false;
                if (count != wanted) FAIL("%s: the gates executed on the store are not the builder's gates", reverse ? "backwards" : "forwards");
                for (size_t i = 0; i < outputs.size(); i++) {
                    const OutRef& o = c.outputs[i];
                    REQUIRE(o.neg == (int32_t)outputs[i].neg);
                    if (outputs[i].id < 0) {
                        REQUIRE(o.slot == -1);
                    } else if (o.slot < 0 || store[(size_t)o.slot] != of_wire[(size_t)outputs[i].id] << 1) {
                        FAIL("%s: output %zu (wire %d) is not in its slot after the last level", reverse ? "backwards" : "forwards", i, outputs[i].id);
                    }
                }
            }
            // on bits: the plain walk of the builder's gates
            std::vector<uint8_t> in((size_t)b.n_inputs()), wire((size_t)b.n_wires(), 0), want(outputs.size());
            for (size_t i = 0; i < in.size(); i++) wire[i] = in[i] = (uint8_t)rng.below(2);
            auto bit = [&](const Ref& r) { return (uint8_t)((r.id >= 0 ? wire[(size_t)r.id] : 0) ^ (uint8_t)r.neg); };
            for (const Gate& g : b.gates()) wire[(size_t)g.out] = gate_bit(g.type, bit(g.a), bit(g.b), bit(g.c));
            for (size_t i = 0; i < outputs.size(); i++) want[i] = bit(outputs[i]);
            if (!check_bits(c, in, want)) return false;
            g_circuits++;
            g_gate3 += n3;
        }
    return true;
}

// A random DAG in which about half of the gates are MAJ3 / XOR3, with constants in every position and -- under folding, which
// lowers them -- the same wire on several operands.  Small windows make deep narrow chains whose slots are recycled at once:
// where an uncounted third read would show.
bool random_dag(uint64_t seed) {
    Rng rng(seed);
    const int32_t n_inputs = 3 + rng.below(4);
    const bool fold = rng.chance(30);
    const int n_gates = 1 + rng.below(48);
    const int window = rng.chance(50) ? 3 + rng.below(3) : (rng.chance(50) ? 8 : 1 << 20);
    const int p_gate3 = rng.chance(20) ? 100 : 30 + rng.below(50);
    const int p_mux = rng.chance(50) ? 0 : 10 + rng.below(30);
    const int p_const = rng.chance(50) ? 0 : 5 + rng.below(25);
    const int p_neg = rng.below(60);
    const int p_dead = rng.chance(50) ? 0 : 10 + rng.below(40);
    static const int32_t kTwoInput[] = {GATE_AND, GATE_XOR, GATE_OR, GATE_NAND, GATE_NOR, GATE_XNOR, GATE_ANDNY, GATE_ANDYN, GATE_ORNY, GATE_ORYN};
    CircuitBuilder b(n_inputs, fold);
    std::vector<Ref> pool, all;
    for (int32_t i = 0; i < n_inputs; i++) {
        all.push_back(b.input(i));
        pool.push_back(b.input(i));
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
        Ref out;
        if (rng.chance(p_gate3)) {
            // without folding a three-input gate must name three different wires (the builder throws otherwise)
            for (int tries = 0; !fold && tries < 64 && ((a.id >= 0 && (a.id == x.id || a.id == y.id)) || (x.id >= 0 && x.id == y.id)); tries++) {
                x = pick();
                y = pick();
            }
            if (!fold && ((a.id >= 0 && (a.id == x.id || a.id == y.id)) || (x.id >= 0 && x.id == y.id))) y = x = CircuitBuilder::constant(rng.below(2));
            out = b.gate3(rng.chance(50) ? GATE_MAJ3 : GATE_XOR3, a, x, y);
        } else if (rng.chance(p_mux)) {
            out = b.gate3(GATE_MUX, a, x, y);
        } else {
            out = b.gate(kTwoInput[rng.below(10)], a, x);
        }
        all.push_back(out);
        if (out.id >= 0 && !rng.chance(p_dead)) pool.push_back(out);
    }
    Word outputs;
    const int n_out = 1 + rng.below(7);
    for (int i = 0; i < n_out; i++) {
        Ref r = rng.chance(10) ? CircuitBuilder::constant(rng.below(2)) : all[(size_t)rng.below((int)all.size())];
        if (rng.chance(30)) r = all[all.size() - 1 - (size_t)rng.below(std::min<int>(3, (int)all.size()))];
        if (rng.chance(30)) r = CircuitBuilder::NOT(r);
        outputs.push_back(r);
    }
    return check_all_schedules("dag " + std::to_string(seed) + (fold ? " folded" : ""), b, outputs, {0, 1, 2, 3, 7}, rng);
}

void put_bits(std::vector<uint8_t>& v, size_t at, uint64_t x, int n) {
    for (int i = 0; i < n; i++) v[at + (size_t)i] = (uint8_t)((x >> i) & 1);
}

// the built-in kinds as build_circuit gives them: add16_fa (recorded here as well, to reach every schedule) and mul32_fa
// under ASAP levels and under the level widths round_level_cap() produces for the 32-bit multipliers
bool full_adder_circuits() {
    Rng rng(7);
    for (int fold = 0; fold < 2; fold++) {
        CircuitBuilder a(64, fold != 0);
        Word sum(16);
        Ref carry = a.input(32);
        for (int i = 0; i < 16; i++) {
            sum[(size_t)i] = a.XOR3(a.input(i), a.input(16 + i), carry);
            carry = a.MAJ3(a.input(i), a.input(16 + i), carry);
        }
        if (!check_all_schedules(fold ? "add16_fa recorded, folded" : "add16_fa recorded", a, sum, {0, 1, 2, 3, 7}, rng)) return false;
        for (int32_t kind : {CIRC_ADD_FA, CIRC_SUB_FA, CIRC_RSUB_FA}) {
            g_case = "kind " + std::to_string(kind) + " at 16 bits" + (fold ? " folded" : "");
            Circuit c;
            REQUIRE(build_circuit(kind, 16, &c, true, fold != 0));
            int64_t n3 = 0;
            if (!check_layout(c, &n3)) return false;
            REQUIRE(n3 == (fold && kind != CIRC_ADD_FA ? 30 : 32));
            for (int t = 0; t < 50; t++) {
                const uint64_t x = rng.next() & 0xFFFF, y = rng.next() & 0xFFFF, cin = kind == CIRC_ADD_FA ? rng.next() & 1 : 0;
                std::vector<uint8_t> in(64, 0), want(16);
                put_bits(in, 0, x, 16);
                put_bits(in, 16, y, 16);
                in[32] = (uint8_t)cin;
                put_bits(want, 0, kind == CIRC_ADD_FA ? x + y + cin : kind == CIRC_SUB_FA ? x - y : y - x, 16);
                if (!check_bits(c, in, want)) return false;
            }
            g_circuits++;
            g_gate3 += n3;
        }
        for (int32_t cap : {0, 8, 35, 47, 70}) {
            g_case = "mul32_fa cap " + std::to_string(cap) + (fold ? " folded" : "");
            Circuit c;
            REQUIRE(build_circuit(CIRC_MUL_FA, 32, &c, true, fold != 0, cap));
            REQUIRE(c.balanced_schedule == (cap > 0) && c.n_bootstraps == 3008);
            int64_t n3 = 0;
            if (!check_layout(c, &n3)) return false;
            REQUIRE(n3 == (fold ? 2 * (32 * 31 - 32) : 2 * 32 * 31));
            for (int t = 0; t < 6; t++) {
                const uint64_t x = t == 0 ? 0xFFFFFFFFull : rng.next() & 0xFFFFFFFFull, y = t == 0 ? 0xFFFFFFFFull : rng.next() & 0xFFFFFFFFull;
                std::vector<uint8_t> in(96, 0), want(64);
                put_bits(in, 0, x, 32);
                put_bits(in, 32, y, 32);
                put_bits(want, 0, x * y, 64);
                if (!check_bits(c, in, want)) return false;
            }
            g_circuits++;
            g_gate3 += n3;
        }
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const int n_dags = argc > 1 ? atoi(argv[1]) : 3000;
    for (int s = 1; s <= n_dags; s++)
        if (!random_dag((uint64_t)s)) return 1;
    if (!full_adder_circuits()) return 1;
    // a repeated wire is refused where nothing would lower it
    try {
        CircuitBuilder b(3, false);
        b.gate3(GATE_XOR3, b.input(0), b.input(1), CircuitBuilder::NOT(b.input(0)));
        fprintf(stderr, "a repeated wire was recorded\n");
        return 1;
    } catch (const std::invalid_argument&) {
    }
    printf("GATE3_STORE_OK circuits=%d gate3=%lld\n", g_circuits, (long long)g_gate3);
    return 0;
}
