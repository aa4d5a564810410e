// What "the circuits did not change" means, as text: 64-bit FNV-1a digests of the whole Circuit that ie-ache_amd/csrc/circuit.cpp
// builds -- every built-in kind over its widths and refusals, with and without folding, balancing and a level cap, and
// circuit_level_cap() of every base circuit over a table of batches and residencies, one line per (kind, width); a dozen
// fixed netlists and build_netlist's refusals, one line each.  tests/golden/circuit_digests.txt is this program's output at the commit
// before the circuit code was restructured, and tests/test_circuit_digest_cpu.py compares the two line for line.
// Uses only build_circuit, build_netlist, finalize_circuit, circuit_level_cap, circuit_n_inputs and circuit_n_outputs.
// Exit status 1 if a balanced base circuit rebuilt with level_cap = its mean width is not the base itself.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <string>
#include <vector>

#include "../../ie-ache_amd/csrc/circuit.h"

using namespace ieache;

namespace {

struct Fnv {
    uint64_t h = 0xcbf29ce484222325ull;
    void byte(uint8_t b) {
        h ^= b;
        h *= 0x100000001b3ull;
    }
    void i32(int32_t v) {
        for (int i = 0; i < 4; i++) byte((uint8_t)((uint32_t)v >> (8 * i)));
    }
    void i64(int64_t v) {
        for (int i = 0; i < 8; i++) byte((uint8_t)((uint64_t)v >> (8 * i)));
    }
    void ints(const std::vector<int32_t>& v) {
        i64((int64_t)v.size());
        for (int32_t x : v) i32(x);
    }
};

uint64_t digest(const Circuit& c) {
    Fnv f;
    f.i64((int64_t)c.name.size());
    for (char ch : c.name) f.byte((uint8_t)ch);
    f.i32(c.n_inputs);
    f.i32(c.n_slots);
    f.i64((int64_t)c.gates.size());
    for (const DevGate& d : c.gates)
        for (int32_t v : {d.type, d.a_slot, d.a_neg, d.b_slot, d.b_neg, d.out_slot, d.c_slot, d.c_neg}) f.i32(v);
    f.ints(c.level_offset);
    f.ints(c.level_mux);
    f.i64((int64_t)c.outputs.size());
    for (const OutRef& o : c.outputs) {
        f.i32(o.slot);
        f.i32(o.neg);
    }
    f.i64(c.n_bootstraps);
    f.i64(c.n_and);
    f.i64(c.n_xor);
    for (int64_t n : c.n_by_type) f.i64(n);
    f.i64(c.n_maj3);
    f.i64(c.n_xor3);
    f.i32(c.depth);
    f.i32(c.max_width);
    f.i32(c.sched_max_width);
    f.i64(c.n_reference_bootstraps);
    f.byte(c.balanced_schedule ? 1 : 0);
    return f.h;
}

const int kCaps[] = {0, 32, 35, 40, 64, 80};
const int64_t kBatches[] = {1, 2, 16, 32, 58, 64, 100, 128, 200, 256, 1000, 1024, 2048, 4096};
const int32_t kResident[][2] = {{2048, 1024}, {2048, 0}, {1024, 0}, {16, 0}};
bool g_ok = true;

bool g_verbose = false;  // -v: a line per configuration as well, to find which one of a (kind, bits) line changed

// One line per (kind, bits): its 24 configurations (fold x balanced x level cap, in that order), each as r = refused,
// b = built with the balanced schedule, a = built with ASAP levels, and ONE digest over the 24 circuits' digests and the
// level-cap tables of the two base circuits (fold 0 / 1, balanced, cap 0).
void kind_lines(int32_t kind, int32_t bits) {
    Fnv all;
    std::string what;
    for (int fold = 0; fold < 2; fold++)
        for (int balanced = 1; balanced >= 0; balanced--)
            for (int cap : kCaps) {
                Circuit c;
                if (!build_circuit(kind, bits, &c, balanced != 0, fold != 0, cap)) {
                    what += 'r';
                    all.byte(0);
                    continue;
                }
                if ((int32_t)c.outputs.size() != circuit_n_outputs(kind, bits) || c.n_inputs != circuit_n_inputs(kind, bits)) {
                    printf("BAD: circuit_n_inputs / circuit_n_outputs disagree with %s\n", c.name.c_str());
                    g_ok = false;
                }
                const uint64_t h = digest(c);
                what += c.balanced_schedule ? 'b' : 'a';
                all.byte(1);
                all.i64((int64_t)h);
                if (g_verbose) printf("  f%d b%d c%d %016" PRIx64 " %s %d/%d\n", fold, balanced, cap, h, c.name.c_str(), c.n_levels(), c.n_slots);
                if (!balanced || cap != 0) continue;
                // the base circuit of (kind, bits, fold): its level caps, and the identity the circuit cache's shortcut rests on
                for (const auto& r : kResident)
                    for (int64_t batch : kBatches) {
                        const int32_t level_cap = circuit_level_cap(c, batch, r[0], r[1]);
                        all.i32(level_cap);
                        if (g_verbose && level_cap) printf("  f%d cap(batch %d, resident %d, %d) = %d\n", fold, (int)batch, r[0], r[1], level_cap);
                    }
                if (c.balanced_schedule) {
                    const int32_t mean = (int32_t)((c.n_bootstraps + c.depth - 1) / c.depth);
                    Circuit again;
                    if (!build_circuit(kind, bits, &again, true, fold != 0, mean) || digest(again) != h) {
                        printf("BAD: %s rebuilt with level_cap = its mean width %d is not the base circuit\n", c.name.c_str(), mean);
                        g_ok = false;
                    }
                }
            }
    printf("c %d %d %s %016" PRIx64 "\n", kind, bits, what.c_str(), all.h);
}

constexpr int32_t W(int32_t wire, bool neg = false) { return wire << 1 | (neg ? 1 : 0); }
constexpr int32_t kTrue = -1, kFalse = -2;

void netlist_line(const char* what, int32_t n_inputs, const std::vector<NetGate>& gates, const std::vector<int32_t>& outs, bool balanced) {
    printf("n %s b%d ", what, balanced ? 1 : 0);
    try {
        const Circuit c = build_netlist(n_inputs, gates.data(), gates.size(), outs.data(), outs.size(), balanced);
        printf("%016" PRIx64 " %d/%d\n", digest(c), c.n_levels(), c.n_slots);
    } catch (const std::exception& e) {
        printf("refused %s\n", e.what());
    }
}

// A fixed pseudo-random netlist of every gate type: wide early levels, then a tail of dependent gates.
std::vector<NetGate> mixed_netlist(int32_t n_inputs, int32_t n_gates, uint64_t seed) {
    static const int32_t types[] = {GATE_AND, GATE_XOR, GATE_OR, GATE_NAND, GATE_MUX, GATE_NOR, GATE_XNOR, GATE_ANDNY,
                                    GATE_ANDYN, GATE_ORNY, GATE_ORYN, GATE_MAJ3, GATE_XOR3};
    uint64_t s = seed;
    auto next = [&](int n) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (int)((s >> 33) % (uint64_t)n);
    };
    std::vector<NetGate> g;
    for (int32_t i = 0; i < n_gates; i++) {
        const int32_t wires = n_inputs + i;
        const int32_t recent = i < n_gates / 2 ? wires : 6;  // the second half chains on the last few wires: a deep tail
        auto pick = [&] { return wires - 1 - next(recent < wires ? recent : wires); };
        NetGate ng{types[next(13)], 0, 0, 0};
        const int32_t a = pick();
        int32_t b = pick(), c = pick();
        if (is_gate3(ng.type)) {  // three different wires
            while (b == a) b = pick();
            while (c == a || c == b) c = pick();
        }
        ng.a = W(a, next(4) == 0);
        ng.b = next(16) == 0 ? (next(2) ? kTrue : kFalse) : W(b, next(4) == 0);
        if (ng.type == GATE_MUX || is_gate3(ng.type)) ng.c = next(16) == 0 ? kTrue : W(c, next(4) == 0);
        g.push_back(ng);
    }
    return g;
}

void netlist_lines() {
    for (int balanced = 0; balanced < 2; balanced++) {
        const bool bal = balanced != 0;
        netlist_line("one_and", 2, {{GATE_AND, W(0), W(1), 0}}, {W(2)}, bal);
        std::vector<NetGate> two;  // every two-input type, each on the previous gate and an input
        for (int32_t t = 0; t < GATE_TYPES; t++)
            if (t != GATE_MUX) two.push_back({t, W(3 + (int32_t)two.size() - 1, t % 2 == 1), W(t % 3), 0});
        netlist_line("two_input_types", 3, two, {W(3 + (int32_t)two.size() - 1), W(5, true), W(0)}, bal);
        // MUX gates sharing levels with two-input gates
        netlist_line("mux_levels", 4,
                     {{GATE_XOR, W(0), W(1), 0}, {GATE_MUX, W(0), W(1), W(2)}, {GATE_AND, W(2), W(3), 0}, {GATE_MUX, W(3, true), W(2), W(1, true)},
                      {GATE_MUX, W(4), W(5), W(6)}, {GATE_OR, W(5), W(7), 0}, {GATE_MUX, W(8), W(9), W(4)}, {GATE_NAND, W(8), W(6), 0},
                      {GATE_MUX, W(10), W(11), W(0)}},
                     {W(12), W(10, true), W(11)}, bal);
        std::vector<NetGate> fa;  // a 4-bit ripple of XOR3 / MAJ3 full adders, carry-in = input 8
        int32_t carry = W(8);
        std::vector<int32_t> sums;
        for (int32_t i = 0; i < 4; i++) {
            fa.push_back({GATE_XOR3, W(i), W(4 + i), carry});
            sums.push_back(W(9 + 2 * i));
            fa.push_back({GATE_MAJ3, W(i), W(4 + i), carry});
            carry = W(9 + 2 * i + 1);
        }
        sums.push_back(carry);
        netlist_line("full_adder4", 9, fa, sums, bal);
        netlist_line("constants", 3,
                     {{GATE_AND, W(0), kTrue, 0}, {GATE_XOR, kFalse, W(1), 0}, {GATE_MUX, kTrue, W(0), W(1)}, {GATE_MUX, W(2), kFalse, kTrue},
                      {GATE_MAJ3, W(0), W(1), kTrue}, {GATE_XOR3, W(2), kFalse, kFalse}, {GATE_ORYN, kTrue, kFalse, 0}, {GATE_XNOR, W(3), W(7, true), 0}},
                     {kTrue, kFalse, W(3), W(4, true), W(5), W(6), W(8), W(9), W(10), W(5)}, bal);
        netlist_line("mixed200", 8, mixed_netlist(8, 200, 1), {W(207), W(206, true), W(100), W(3)}, bal);
        netlist_line("mixed1500", 24, mixed_netlist(24, 1500, 7), {W(1523), W(1522), W(1400), W(700, true)}, bal);
        netlist_line("no_gates", 2, {}, {W(1), W(0, true), kTrue}, bal);
        // gates nobody reads, the same output twice
        netlist_line("unread", 2, {{GATE_AND, W(0), W(1), 0}, {GATE_OR, W(0), W(1), 0}, {GATE_XOR, W(2), W(0), 0}}, {W(4), W(4)}, bal);
    }
    netlist_line("bad_reference", 2, {{GATE_AND, W(0), -3, 0}}, {W(2)}, false);
    netlist_line("forward_reference", 2, {{GATE_AND, W(0), W(2), 0}}, {W(2)}, false);
    netlist_line("forward_output", 2, {{GATE_AND, W(0), W(1), 0}}, {W(3)}, false);
    netlist_line("gate3_same_wire", 3, {{GATE_MAJ3, W(0), W(1), W(0, true)}}, {W(3)}, false);
    netlist_line("gate2_with_c", 2, {{GATE_XOR, W(0), W(1), W(1)}}, {W(2)}, false);
    netlist_line("no_outputs", 2, {{GATE_AND, W(0), W(1), 0}}, {}, false);
    netlist_line("unknown_type", 2, {{GATE_TYPES, W(0), W(1), 0}}, {W(2)}, false);
    netlist_line("no_inputs", 0, {}, {kTrue}, false);
}

}  // namespace

int main(int argc, char** argv) {
    g_verbose = argc > 1 && std::string(argv[1]) == "-v";
    unsetenv("IEACHE_SCHEDULE");
    for (int32_t kind : {1, 2, 3, 6, 7, 8, 16, 17, 18})
        for (int32_t bits : {0, 1, 2, 4, 16, 31, 32, 33, 64, 256, 257}) kind_lines(kind, bits);
    for (int32_t kind : {4, 9, 19, (int32_t)CIRC_MULADD})
        for (int32_t bits : {16, 32, 64, 128, 256}) kind_lines(kind, bits);
    for (int32_t kind = CIRC_CHAIN_BASE; kind < CIRC_CHAIN_END; kind++)
        for (int32_t bits : {16, 32, 64, 128}) kind_lines(kind, bits);
    for (int32_t kind : {0, 10, 15, 20, 31, 64}) kind_lines(kind, 32);
    netlist_lines();
    return g_ok ? 0 : 1;
}
