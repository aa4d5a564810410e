// Word programs: multi-operator integer expressions compiled into ONE circuit.
//
// A circuit kind is one word operator; a caller who wants a*b + c*d, the sum of eight words or max(a+b, c) would issue one
// call per operator -- each paying its own depth, independent operators one after the other -- or transcribe the adders gate
// by gate into a netlist.  A program is a list of word-level instructions instead.  The result of instruction i is register
// i: a Word of 1 .. 512 samples, LSB first.  compile_program records the instructions in order into one CircuitBuilder, with
// the builders the circuit kinds are made of (build_word_operator), and finalises it: independent instructions share levels,
// intermediates never leave the wire store, and what comes out is an ordinary Circuit for everything that evaluates one.
//
// Host only and free of HIP, like circuit.h.  WordInstr / WordArg are include/ieache.h's ieache_word_instr / ieache_word_arg.
#pragma once
#include <cstddef>
#include <cstdint>

#include "circuit.h"

namespace ieache {

enum WordOp : int32_t {
    // wiring only: no gate
    WOP_INPUT = 0,   // width samples of the expression's input, in declaration order
    WOP_CONST = 1,   // width constant samples; bit j = bit j % 32 of const_words[first + j / 32]  (count >= ceil(width / 32))
    WOP_ZEXT = 2,    // a, zero-extended to width (>= a's)
    WOP_SLICE = 3,   // samples imm0 .. imm0 + imm1 - 1 of a
    WOP_SHL = 4,     // a shifted left by imm0, same width, zeros shifted in
    WOP_NOT = 5,     // ~a
    WOP_CONCAT = 6,  // a (low) then b (high)
    // bitwise: one gate per bit
    WOP_AND = 7,     // a, b of equal widths
    WOP_OR = 8,
    WOP_XOR = 9,
    WOP_ANDBIT = 10,  // every bit of a ANDed with the 1-sample register b
    // word operators: build_word_operator on the kind of (operator, family); c = the 32-sample carry word, -1 = 32 constant zeros
    WOP_ADD = 11,   // a + b
    WOP_SUB = 12,   // a - b
    WOP_RSUB = 13,  // b - a
    WOP_MUL = 14,   // a * b, 2 x width samples
    // the sum mod 2^width of count >= 2 operands args[first .. first + count), each a register shifted left, zero-extended or
    // truncated to width: carry-save reduction on XOR3 / MAJ3 to two rows, one addition in family (full adder or Kogge-Stone)
    WOP_SUM = 15,
    WOP_LT = 16,      // a < b, unsigned, equal widths -> 1 sample (one XNOR and one MUX per bit)
    WOP_EQ = 17,      // a == b -> 1 sample (XNORs and a balanced AND tree)
    WOP_SELECT = 18,  // a (1 sample) ? b : c, one MUX per bit
    WOP_COUNT = 19,
};

struct WordInstr {
    int32_t op;      // WordOp
    int32_t family;  // CircuitFamily of ADD / SUB / RSUB / MUL / SUM; 0 otherwise
    int32_t width;   // INPUT, CONST, ZEXT: the result's width; SUM: out_width; 0 otherwise
    int32_t a, b, c;  // register operands (indices of earlier instructions); unused ones are ignored
    int32_t imm0, imm1;
    int32_t first, count;  // SUM: into the (register, shift) pairs; CONST: into the value words
};
struct WordArg {
    int32_t reg, shift;
};

constexpr int32_t kMaxWordWidth = 512;
constexpr int kProgramBalanced = 1;  // IEACHE_NETLIST_BALANCED
constexpr int kProgramFold = 2;      // IEACHE_PROGRAM_FOLD: CircuitBuilder(fold = true)

struct CompiledProgram {
    Circuit circuit;
    RecordedNetlist recorded;  // what was recorded (after folding, if asked for), in build_netlist's form
};

// Every refusal throws std::invalid_argument, "program: instruction I: ..." wherever an instruction is at fault; nothing is
// returned half-built.  No array is read outside [0, its count).
CompiledProgram compile_program(const WordInstr* instrs, size_t n_instrs, const WordArg* args, size_t n_args, const uint32_t* const_words,
                                size_t n_const_words, const int32_t* outputs, size_t n_outputs, int flags);

// stages of the carry-save reduction of k rows to two: the least s with w_s >= k, w_0 = 2, w_{s+1} = floor(3 w_s / 2)
int32_t sum_reduction_stages(int64_t k);

}  // namespace ieache
