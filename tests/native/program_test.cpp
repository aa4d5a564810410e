// Word programs (ie-ache_amd/csrc/program.cpp) as plain host C++ under AddressSanitizer + UBSan:
//   anchor     a one-instruction program with the caller's carry word IS the built-in kind's circuit -- every row of the kind
//              table, every statistic, every device gate, 64 random simulations; two instructions are the chain kinds
//   export     the recorded gate list, compiled again by build_netlist, is the same circuit
//   refusals   each names its instruction
//   garbage    truncated and random instruction arrays and side arrays, each in a heap block of exactly its size, so that a
//              read outside one is an ASan report
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../ie-ache_amd/csrc/program.h"

using namespace ieache;

static int g_checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        g_checks++;                                                        \
        if (!(cond)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

static WordInstr instr(int32_t op, int32_t family = 0, int32_t width = 0, int32_t a = 0, int32_t b = 0, int32_t c = 0, int32_t imm0 = 0,
                       int32_t imm1 = 0, int32_t first = 0, int32_t count = 0) {
    return WordInstr{op, family, width, a, b, c, imm0, imm1, first, count};
}
static WordInstr input(int32_t width) { return instr(WOP_INPUT, 0, width); }

// arrays copied into heap blocks of exactly their size (an empty one is a null pointer)
template <class T>
struct Exact {
    T* p = nullptr;
    size_t n = 0;
    explicit Exact(const std::vector<T>& v) : n(v.size()) {
        if (n) {
            p = (T*)malloc(n * sizeof(T));
            memcpy(p, v.data(), n * sizeof(T));
        }
    }
    ~Exact() { free(p); }
    Exact(const Exact&) = delete;
};

static CompiledProgram compile(const std::vector<WordInstr>& is, const std::vector<int32_t>& outs, int flags = 0, const std::vector<WordArg>& args = {},
                               const std::vector<uint32_t>& words = {}) {
    Exact<WordInstr> i(is);
    Exact<WordArg> a(args);
    Exact<uint32_t> w(words);
    Exact<int32_t> o(outs);
    return compile_program(i.p, i.n, a.p, a.n, w.p, w.n, o.p, o.n, flags);
}

static void same_circuit(const Circuit& p, const Circuit& k, bool with_reference_count) {
    CHECK(p.n_inputs == k.n_inputs && p.outputs.size() == k.outputs.size() && p.n_slots == k.n_slots);
    CHECK(p.depth == k.depth && p.max_width == k.max_width && p.sched_max_width == k.sched_max_width && p.n_levels() == k.n_levels());
    CHECK(p.n_bootstraps == k.n_bootstraps && p.n_and == k.n_and && p.n_xor == k.n_xor && p.n_maj3 == k.n_maj3 && p.n_xor3 == k.n_xor3);
    if (with_reference_count) CHECK(p.n_reference_bootstraps == k.n_reference_bootstraps);
    for (int t = 0; t < GATE_TYPES; t++) CHECK(p.n_by_type[t] == k.n_by_type[t]);
    CHECK(p.level_offset == k.level_offset && p.level_mux == k.level_mux);
    CHECK(p.gates.size() == k.gates.size());
    CHECK(p.gates.empty() || memcmp(p.gates.data(), k.gates.data(), p.gates.size() * sizeof(DevGate)) == 0);
    CHECK(memcmp(p.outputs.data(), k.outputs.data(), p.outputs.size() * sizeof(OutRef)) == 0);
    std::mt19937 rng(p.n_inputs * 31 + (uint32_t)p.gates.size());
    std::vector<uint8_t> in(p.n_inputs), o1(p.outputs.size()), o2(p.outputs.size());
    for (int v = 0; v < 64; v++) {
        for (auto& x : in) x = rng() & 1;
        simulate_circuit(p, in.data(), o1.data());
        simulate_circuit(k, in.data(), o2.data());
        CHECK(o1 == o2);
    }
}

static void recompiled_is_the_same(const CompiledProgram& p, bool balanced) {
    const RecordedNetlist& r = p.recorded;
    const Circuit again = build_netlist(p.circuit.n_inputs, r.gates.data(), r.gates.size(), r.outputs.data(), r.outputs.size(), balanced);
    same_circuit(again, p.circuit, true);
}

struct KindCase {
    int32_t kind, op, family;
    bool mul;
};
static const KindCase kCases[] = {
    {CIRC_ADD, WOP_ADD, FAMILY_REFERENCE, false},          {CIRC_SUB, WOP_SUB, FAMILY_REFERENCE, false},
    {CIRC_RSUB, WOP_RSUB, FAMILY_REFERENCE, false},        {CIRC_MUL, WOP_MUL, FAMILY_REFERENCE, true},
    {CIRC_ADD_KS, WOP_ADD, FAMILY_KOGGE_STONE, false},     {CIRC_SUB_KS, WOP_SUB, FAMILY_KOGGE_STONE, false},
    {CIRC_RSUB_KS, WOP_RSUB, FAMILY_KOGGE_STONE, false},   {CIRC_MUL_WALLACE, WOP_MUL, FAMILY_CARRY_SAVE, true},
    {CIRC_ADD_FA, WOP_ADD, FAMILY_FULL_ADDER, false},      {CIRC_SUB_FA, WOP_SUB, FAMILY_FULL_ADDER, false},
    {CIRC_RSUB_FA, WOP_RSUB, FAMILY_FULL_ADDER, false},    {CIRC_MUL_FA, WOP_MUL, FAMILY_FULL_ADDER, true},
};

static void anchor() {
    for (const KindCase& kc : kCases)
        for (int32_t bits : kc.mul ? std::vector<int32_t>{32, 64} : std::vector<int32_t>{1, 7, 16, 32}) {
            Circuit k;
            CHECK(build_circuit(kc.kind, bits, &k, true, false));  // what ieache_circuit_info_get builds
            // the schedule and the folding build_circuit picks for that kind
            const int flags = (k.balanced_schedule ? kProgramBalanced : 0) | (kc.kind == CIRC_MUL_WALLACE ? kProgramFold : 0);
            const CompiledProgram p = compile({input(bits), input(bits), input(32), instr(kc.op, kc.family, 0, 0, 1, 2)}, {3}, flags);
            same_circuit(p.circuit, k, false);
            if (bits <= 32) recompiled_is_the_same(p, k.balanced_schedule);
        }
    // two instructions = the chain kinds: (A+B)-C, A*B+C, and one with the answer as operand 2 (flip = 0)
    for (int32_t bits : {8, 32}) {
        Circuit k;
        CHECK(build_circuit(chain_kind(CIRC_ADD, CIRC_SUB, true), bits, &k, true, false));
        const CompiledProgram p = compile({input(bits), input(bits), input(32), input(bits), instr(WOP_ADD, 0, 0, 0, 1, 2), instr(WOP_SUB, 0, 0, 4, 3, 2)}, {5});
        same_circuit(p.circuit, k, false);
    }
    {
        Circuit k;
        CHECK(build_circuit(CIRC_MULADD, 32, &k, true, false));
        const CompiledProgram p = compile({input(32), input(32), input(32), input(64), instr(WOP_MUL, 0, 0, 0, 1, 2), instr(WOP_ADD, 0, 0, 4, 3, 2)}, {5});
        same_circuit(p.circuit, k, false);
    }
    {
        Circuit k;
        CHECK(build_circuit(chain_kind(CIRC_RSUB, CIRC_SUB, false), 16, &k, true, false));
        const CompiledProgram p =
            compile({input(16), input(16), input(32), input(16), input(32), instr(WOP_RSUB, 0, 0, 0, 1, 2), instr(WOP_SUB, 0, 0, 3, 5, 4)}, {6});
        same_circuit(p.circuit, k, false);
    }
}

// the program is refused with a message that starts with `prefix` and contains `part`
static void refused(const std::vector<WordInstr>& is, const std::vector<int32_t>& outs, const std::string& prefix, const std::string& part, int flags = 0,
                    const std::vector<WordArg>& args = {}, const std::vector<uint32_t>& words = {}) {
    try {
        compile(is, outs, flags, args, words);
    } catch (const std::invalid_argument& e) {
        const std::string msg = e.what();
        if (msg.rfind(prefix, 0) != 0 || msg.find(part) == std::string::npos) {
            printf("FAILED: refusal reads '%s', expected '%s ... %s'\n", msg.c_str(), prefix.c_str(), part.c_str());
            exit(1);
        }
        g_checks++;
        return;
    }
    printf("FAILED: accepted what should be refused (%s ... %s)\n", prefix.c_str(), part.c_str());
    exit(1);
}

static void refusals() {
    const std::string at1 = "program: instruction 1:", at2 = "program: instruction 2:", at3 = "program: instruction 3:";
    // a register referred to before it exists: itself, a later one, a negative one
    refused({input(4), instr(WOP_NOT, 0, 0, 1)}, {1}, at1, "does not exist");
    refused({input(4), instr(WOP_AND, 0, 0, 0, 2), input(4)}, {1}, at1, "does not exist");
    refused({input(4), instr(WOP_NOT, 0, 0, -3)}, {1}, at1, "does not exist");
    refused({input(4), input(4), instr(WOP_ADD, 0, 0, 0, 1, 7)}, {2}, at2, "does not exist");  // the carry word
    // width mismatches
    refused({input(4), input(5), instr(WOP_XOR, 0, 0, 0, 1)}, {2}, at2, "width mismatch");
    refused({input(4), input(5), instr(WOP_ADD, 0, 0, 0, 1, -1)}, {2}, at2, "width mismatch");
    refused({input(4), input(4), instr(WOP_ADD, 0, 0, 0, 1, 0)}, {2}, at2, "carry word");  // a 4-sample carry word
    refused({input(4), input(2), instr(WOP_ANDBIT, 0, 0, 0, 1)}, {2}, at2, "width mismatch");
    refused({input(2), input(4), input(4), instr(WOP_SELECT, 0, 0, 0, 1, 2)}, {3}, at3, "width mismatch");
    refused({input(1), input(4), input(3), instr(WOP_SELECT, 0, 0, 0, 1, 2)}, {3}, at3, "width mismatch");
    refused({input(4), input(3), instr(WOP_LT, 0, 0, 0, 1)}, {2}, at2, "width mismatch");
    refused({input(4), input(3), instr(WOP_EQ, 0, 0, 0, 1)}, {2}, at2, "width mismatch");
    refused({input(4), instr(WOP_ZEXT, 0, 3, 0)}, {1}, at1, "width mismatch");
    refused({input(4), instr(WOP_SLICE, 0, 0, 0, 0, 0, 2, 3)}, {1}, at1, "width mismatch");
    refused({input(4), instr(WOP_SLICE, 0, 0, 0, 0, 0, INT_MAX, INT_MAX)}, {1}, at1, "width mismatch");
    // widths the kind table refuses
    refused({input(16), input(16), instr(WOP_MUL, 0, 0, 0, 1, -1)}, {2}, at2, "width 16");
    refused({input(32), input(32), instr(WOP_MUL, FAMILY_KOGGE_STONE, 0, 0, 1, -1)}, {2}, at2, "no such operator");
    refused({input(32), input(32), instr(WOP_ADD, FAMILY_CARRY_SAVE, 0, 0, 1, -1)}, {2}, at2, "no such operator");
    refused({input(32), input(32), instr(WOP_ADD, 9, 0, 0, 1, -1)}, {2}, at2, "unknown family");
    refused({input(200), input(200), instr(WOP_CONCAT, 0, 0, 0, 1), instr(WOP_ADD, 0, 0, 2, 2, -1)}, {3}, at3, "width 400");
    // register widths and out_width outside 1 .. 512
    refused({input(4), input(0)}, {0}, at1, "outside 1 .. 512");
    refused({input(4), input(513)}, {0}, at1, "outside 1 .. 512");
    refused({input(4), instr(WOP_ZEXT, 0, 513, 0)}, {1}, at1, "outside 1 .. 512");
    refused({input(300), input(300), instr(WOP_CONCAT, 0, 0, 0, 1)}, {2}, at2, "outside 1 .. 512");
    refused({input(4), instr(WOP_CONST, 0, 0, 0, 0, 0, 0, 0, 0, 1)}, {1}, at1, "outside 1 .. 512", 0, {}, {5});
    refused({input(4), input(4), instr(WOP_SUM, FAMILY_FULL_ADDER, 513, 0, 0, 0, 0, 0, 0, 2)}, {2}, at2, "outside 1 .. 512", 0, {{0, 0}, {1, 0}});
    refused({input(4), input(4), instr(WOP_SUM, FAMILY_FULL_ADDER, 0, 0, 0, 0, 0, 0, 0, 2)}, {2}, at2, "outside 1 .. 512", 0, {{0, 0}, {1, 0}});
    // sums: family, operand ranges, fewer than two
    refused({input(4), input(4), instr(WOP_SUM, FAMILY_REFERENCE, 4, 0, 0, 0, 0, 0, 0, 2)}, {2}, at2, "no addition", 0, {{0, 0}, {1, 0}});
    refused({input(4), input(4), instr(WOP_SUM, FAMILY_FULL_ADDER, 4, 0, 0, 0, 0, 0, 0, 1)}, {2}, at2, "fewer than two", 0, {{0, 0}, {1, 0}});
    refused({input(4), input(4), instr(WOP_SUM, FAMILY_FULL_ADDER, 4, 0, 0, 0, 0, 0, 1, 2)}, {2}, at2, "do not lie", 0, {{0, 0}, {1, 0}});
    refused({input(4), input(4), instr(WOP_SUM, FAMILY_FULL_ADDER, 4, 0, 0, 0, 0, 0, INT_MAX, INT_MAX)}, {2}, at2, "do not lie", 0, {{0, 0}, {1, 0}});
    refused({input(4), input(4), instr(WOP_SUM, FAMILY_FULL_ADDER, 4, 0, 0, 0, 0, 0, 0, 2)}, {2}, at2, "does not exist", 0, {{0, 0}, {2, 0}});
    refused({input(4), input(4), instr(WOP_SUM, FAMILY_FULL_ADDER, 4, 0, 0, 0, 0, 0, 0, 2)}, {2}, at2, "negative shift", 0, {{0, 0}, {1, -1}});
    // constants: value words past the end, too few for the width
    refused({input(4), instr(WOP_CONST, 0, 40, 0, 0, 0, 0, 0, 0, 1)}, {1}, at1, "value words", 0, {}, {5});
    refused({input(4), instr(WOP_CONST, 0, 8, 0, 0, 0, 0, 0, 1, 1)}, {1}, at1, "value words", 0, {}, {5});
    refused({input(4), instr(WOP_CONST, 0, 8, 0, 0, 0, 0, 0, -1, 2)}, {1}, at1, "value words", 0, {}, {5});
    // more than 2^30 wires: a sum whose compressors alone would need them (judged before anything is built)
    {
        const int32_t count = (1 << 20) + 8;
        std::vector<WordArg> args(count, WordArg{0, 0});
        refused({input(512), instr(WOP_SUM, FAMILY_FULL_ADDER, 512, 0, 0, 0, 0, 0, 0, count)}, {1}, at1, "2^30", 0, args);
    }
    // one wire twice in a MAJ3 / XOR3: refused without FOLD, built with it
    refused({input(4), instr(WOP_SUM, FAMILY_FULL_ADDER, 4, 0, 0, 0, 0, 0, 0, 3)}, {1}, at1, "same wire twice", 0, {{0, 0}, {0, 0}, {0, 0}});
    refused({input(4), input(4), instr(WOP_SUM, FAMILY_FULL_ADDER, 6, 0, 0, 0, 0, 0, 0, 2)}, {2}, at2, "same wire twice", 0, {{0, 0}, {0, 0}});
    {
        const CompiledProgram p = compile({input(4), instr(WOP_SUM, FAMILY_FULL_ADDER, 6, 0, 0, 0, 0, 0, 0, 3)}, {1}, kProgramFold, {{0, 0}, {0, 0}, {0, 0}});
        for (int v = 0; v < 16; v++) {
            uint8_t in[4], out[6];
            for (int j = 0; j < 4; j++) in[j] = (v >> j) & 1;
            simulate_circuit(p.circuit, in, out);
            int got = 0;
            for (int j = 0; j < 6; j++) got |= out[j] << j;
            CHECK(got == 3 * v);
        }
        // a register with itself at positions that do not overlap is three different wires per column at most: accepted as it is
        compile({input(2), input(2), instr(WOP_SUM, FAMILY_FULL_ADDER, 6, 0, 0, 0, 0, 0, 0, 3)}, {2}, 0, {{0, 0}, {0, 2}, {1, 1}});
    }
    // unknown opcode, no outputs, an output that names no register, unknown flag, no input
    refused({input(4), instr(WOP_COUNT)}, {1}, at1, "unknown opcode");
    refused({input(4), instr(-1)}, {1}, at1, "unknown opcode");
    refused({input(4)}, {}, "program:", "no outputs");
    refused({input(4)}, {1}, "program: output 0", "does not exist");
    refused({input(4)}, {-1}, "program: output 0", "does not exist");
    refused({input(4)}, {0}, "program:", "unknown flag", 4);
    refused({instr(WOP_CONST, 0, 4, 0, 0, 0, 0, 0, 0, 1)}, {0}, "program:", "at least one input", 0, {}, {5});
    refused({}, {0}, "program:", "at least one instruction");
}

// Truncated side arrays of a valid program, and random instruction arrays: refused or compiled, never read outside the blocks.
static void garbage() {
    const std::vector<WordInstr> good = {input(6), input(6), input(6), instr(WOP_CONST, 0, 40, 0, 0, 0, 0, 0, 0, 2),
                                         instr(WOP_SLICE, 0, 0, 3, 0, 0, 0, 8), instr(WOP_SUM, FAMILY_FULL_ADDER, 8, 0, 0, 0, 0, 0, 0, 4),
                                         instr(WOP_SUM, FAMILY_KOGGE_STONE, 9, 0, 0, 0, 0, 0, 2, 3)};
    const std::vector<WordArg> args = {{0, 0}, {1, 1}, {2, 0}, {4, 0}, {5, 2}};
    const std::vector<uint32_t> words = {0xFFFFFFFFu, 0xA5u};
    compile(good, {6, 4}, 0, args, words);
    int refusedCount = 0;
    for (size_t na = 0; na < args.size(); na++)
        for (size_t nw = 0; nw <= words.size(); nw++) {
            try {
                compile(good, {6, 4}, 0, std::vector<WordArg>(args.begin(), args.begin() + na), std::vector<uint32_t>(words.begin(), words.begin() + nw));
                CHECK(false);
            } catch (const std::invalid_argument&) {
                refusedCount++;
            }
        }
    for (size_t nw = 0; nw < words.size(); nw++) {  // all operands, too few value words
        try {
            compile(good, {6, 4}, 0, args, std::vector<uint32_t>(words.begin(), words.begin() + nw));
            CHECK(false);
        } catch (const std::invalid_argument&) {
            refusedCount++;
        }
    }
    for (size_t ni = 1; ni < good.size(); ni++) {  // truncated instruction array: the outputs name registers that are gone
        try {
            compile(std::vector<WordInstr>(good.begin(), good.begin() + ni), {6, 4}, 0, args, words);
            CHECK(false);
        } catch (const std::invalid_argument&) {
            refusedCount++;
        }
    }
    CHECK(refusedCount == (int)(args.size() * (words.size() + 1) + words.size() + good.size() - 1));

    std::mt19937 rng(20240611);
    const int32_t pool[] = {INT_MIN, -2, -1, 0, 0, 1, 1, 2, 3, 4, 5, 7, 8, 31, 32, 33, 64, 511, 512, 513, 1 << 20, INT_MAX};
    auto pick = [&]() -> int32_t { return pool[rng() % (sizeof pool / sizeof pool[0])]; };
    int compiled = 0, refusedRandom = 0;
    for (int trial = 0; trial < 3000; trial++) {
        const size_t n = 1 + rng() % 8;
        std::vector<WordInstr> is(n);
        for (size_t i = 0; i < n; i++) {
            is[i] = instr((int32_t)(rng() % 24) - 2, (int32_t)(rng() % 6) - 1, pick(), pick(), pick(), pick(), pick(), pick(), pick(), pick());
            if (i == 0 || rng() % 3 == 0) is[i] = input(1 + (int32_t)(rng() % 8));  // something to build on
            if (rng() % 2) {  // operands that exist, so that later checks are reached too
                is[i].a = i ? (int32_t)(rng() % i) : 0;
                is[i].b = i ? (int32_t)(rng() % i) : 0;
                if (rng() % 2) is[i].c = i ? (int32_t)(rng() % i) : -1;
                if (rng() % 2) is[i].first = (int32_t)(rng() % 4), is[i].count = (int32_t)(rng() % 5);
                if (rng() % 2) is[i].width = 1 + (int32_t)(rng() % 12);
            }
        }
        std::vector<WordArg> as(rng() % 6);
        for (WordArg& a : as) a = WordArg{rng() % 2 ? (int32_t)(rng() % n) : pick(), rng() % 2 ? (int32_t)(rng() % 4) : pick()};
        std::vector<uint32_t> ws(rng() % 3);
        for (uint32_t& w : ws) w = rng();
        std::vector<int32_t> outs(rng() % 3);
        for (int32_t& o : outs) o = rng() % 4 ? (int32_t)(rng() % n) : pick();
        try {
            const CompiledProgram p = compile(is, outs, (int)(rng() % 4), as, ws);
            std::vector<uint8_t> in(p.circuit.n_inputs, 1), out(p.circuit.outputs.size());
            simulate_circuit(p.circuit, in.data(), out.data());
            compiled++;
        } catch (const std::invalid_argument&) {
            refusedRandom++;
        }
    }
    CHECK(compiled > 50 && refusedRandom > 50);  // the generator reaches both sides
    printf("garbage: %d compiled, %d refused\n", compiled, refusedRandom);
}

int main() {
    CHECK(sum_reduction_stages(2) == 0 && sum_reduction_stages(3) == 1 && sum_reduction_stages(4) == 2 && sum_reduction_stages(5) == 3 &&
          sum_reduction_stages(6) == 3 && sum_reduction_stages(8) == 4 && sum_reduction_stages(9) == 4 && sum_reduction_stages(13) == 5 &&
          sum_reduction_stages(14) == 6);
    anchor();
    refusals();
    garbage();
    printf("PROGRAM_OK %d checks\n", g_checks);
    return 0;
}
