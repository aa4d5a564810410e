// See program.h.
#include "program.h"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace ieache {

namespace {
constexpr int64_t kMaxWires = (int64_t)1 << 30;  // build_netlist's bound: a reference is wire << 1 | negated in an int32_t

struct Refusal : std::invalid_argument {
    using std::invalid_argument::invalid_argument;
};
[[noreturn]] void refuse(const std::string& msg) { throw Refusal(msg); }

bool is_zero(Ref r) { return r.id == kConstId && !r.neg; }

// The sum of `rows` (each W samples) mod 2^W.  Columns hold the samples that are not the constant 0; Dadda's schedule -- heights
// 2, 3, 4, 6, 9, 13, ... -- reduces every column just enough per stage, counting the carries that arrive from the column below
// in the same stage, with full adders XOR3 / MAJ3 (three samples of a column -> one there, one in the next) and, where one
// sample too many is left, half adders XOR / AND.  A stage reads only what earlier stages made: one level.  The top column's
// carries are 2^W: never recorded.  Then one addition of the two rows left.
Word sum_rows(CircuitBuilder& b, CircuitFamily family, int32_t W, const std::vector<Word>& rows) {
    std::vector<std::vector<Ref>> col(W);
    for (const Word& r : rows)
        for (int32_t c = 0; c < W; c++)
            if (!is_zero(r[c])) col[c].push_back(r[c]);
    std::vector<size_t> heights{2};
    size_t tallest = 0;
    for (const auto& cc : col) tallest = std::max(tallest, cc.size());
    while (heights.back() < tallest) heights.push_back(heights.back() * 3 / 2);
    for (int stage = (int)heights.size() - 2; stage >= 0; stage--) {
        const size_t d = heights[stage];
        std::vector<std::vector<Ref>> next(W);
        for (int32_t c = 0; c < W; c++) {
            const std::vector<Ref>& cur = col[c];
            size_t q = 0, total = cur.size() + next[c].size();  // next[c] already holds this stage's carries from column c-1
            while (total > d) {
                if (total == d + 1) {  // half adder
                    const Ref x = cur[q], y = cur[q + 1];
                    q += 2;
                    next[c].push_back(b.XOR(x, y));
                    if (c + 1 < W) next[c + 1].push_back(b.AND(x, y));
                    total -= 1;
                } else {  // full adder
                    const Ref x = cur[q], y = cur[q + 1], z = cur[q + 2];
                    q += 3;
                    next[c].push_back(b.XOR3(x, y, z));
                    if (c + 1 < W) next[c + 1].push_back(b.MAJ3(x, y, z));
                    total -= 2;
                }
            }
            for (; q < cur.size(); q++) next[c].push_back(cur[q]);
        }
        col.swap(next);
    }
    Word x(W), y(W);
    for (int32_t c = 0; c < W; c++) {
        x[c] = col[c].size() > 0 ? col[c][0] : CircuitBuilder::constant(0);
        y[c] = col[c].size() > 1 ? col[c][1] : CircuitBuilder::constant(0);
    }
    return build_family_adder(b, family, x, y, CircuitBuilder::constant(0));
}

Ref and_tree(CircuitBuilder& b, std::vector<Ref> v) {
    while (v.size() > 1) {
        std::vector<Ref> up;
        for (size_t i = 0; i + 1 < v.size(); i += 2) up.push_back(b.AND(v[i], v[i + 1]));
        if (v.size() & 1) up.push_back(v.back());
        v.swap(up);
    }
    return v[0];
}
}  // namespace

int32_t sum_reduction_stages(int64_t k) {
    int32_t s = 0;
    for (int64_t w = 2; w < k; w = w * 3 / 2) s++;
    return s;
}

CompiledProgram compile_program(const WordInstr* instrs, size_t n_instrs, const WordArg* args, size_t n_args, const uint32_t* const_words,
                                size_t n_const_words, const int32_t* outputs, size_t n_outputs, int flags) {
    if (flags & ~(kProgramBalanced | kProgramFold)) refuse("program: unknown flag");
    if (n_instrs < 1 || !instrs) refuse("program: needs at least one instruction");
    if (n_outputs < 1 || !outputs) refuse("program: no outputs");
    if ((n_args && !args) || (n_const_words && !const_words)) refuse("program: null side array");
    if (n_instrs >= (size_t)kMaxWires || n_outputs >= (size_t)kMaxWires) refuse("program: too many instructions or outputs");

    auto at = [](size_t i) { return "program: instruction " + std::to_string(i) + ": "; };
    auto width_ok = [](int64_t w) { return w >= 1 && w <= kMaxWordWidth; };
    // the expression's input samples: the INPUT instructions in order
    int64_t n_inputs = 0;
    for (size_t i = 0; i < n_instrs; i++)
        if (instrs[i].op == WOP_INPUT) {
            if (!width_ok(instrs[i].width)) refuse(at(i) + "width " + std::to_string(instrs[i].width) + " is outside 1 .. 512");
            n_inputs += instrs[i].width;
            if (n_inputs >= kMaxWires) refuse(at(i) + "too large: wires must stay under 2^30");
        }
    if (n_inputs < 1) refuse("program: needs at least one input");

    CircuitBuilder b((int32_t)n_inputs, (flags & kProgramFold) != 0);
    std::vector<Word> regs(n_instrs);
    int32_t next_input = 0;
    const Ref zero = CircuitBuilder::constant(0);
    for (size_t i = 0; i < n_instrs; i++) {
        const WordInstr& in = instrs[i];
        // -> the register an operand names; it must exist already
        auto reg = [&](int32_t r, const char* name) -> const Word& {
            if (r < 0 || (size_t)r >= i)
                refuse(at(i) + "operand " + name + " refers to register " + std::to_string(r) + ", which does not exist there (" + std::to_string(i) +
                       " registers so far)");
            return regs[r];
        };
        auto same_width = [&](const Word& x, const Word& y) {
            if (x.size() != y.size()) refuse(at(i) + "width mismatch: " + std::to_string(x.size()) + " and " + std::to_string(y.size()) + " samples");
        };
        auto one_sample = [&](const Word& x, const char* name) {
            if (x.size() != 1) refuse(at(i) + "width mismatch: operand " + name + " must be 1 sample, not " + std::to_string(x.size()));
        };
        auto result_width = [&](int64_t w) {
            if (!width_ok(w)) refuse(at(i) + "width " + std::to_string(w) + " is outside 1 .. 512");
        };
        Word& out = regs[i];
        try {
            switch (in.op) {
                case WOP_INPUT:
                    out = b.input_word(next_input, in.width);
                    next_input += in.width;
                    break;
                case WOP_CONST: {
                    result_width(in.width);
                    const int64_t need = (in.width + 31) / 32;
                    if (in.first < 0 || in.count < need || (int64_t)in.first + in.count > (int64_t)n_const_words)
                        refuse(at(i) + "value words [" + std::to_string(in.first) + ", +" + std::to_string(in.count) + ") do not lie in the " +
                               std::to_string(n_const_words) + " given or are fewer than the width needs");
                    out.resize(in.width);
                    for (int32_t j = 0; j < in.width; j++) out[j] = CircuitBuilder::constant((const_words[in.first + j / 32] >> (j % 32)) & 1);
                    break;
                }
                case WOP_ZEXT: {
                    const Word& x = reg(in.a, "a");
                    result_width(in.width);
                    if ((size_t)in.width < x.size()) refuse(at(i) + "width mismatch: cannot extend " + std::to_string(x.size()) + " samples to " + std::to_string(in.width));
                    out = x;
                    out.resize(in.width, zero);
                    break;
                }
                case WOP_SLICE: {
                    const Word& x = reg(in.a, "a");
                    if (in.imm0 < 0 || in.imm1 < 1 || (int64_t)in.imm0 + in.imm1 > (int64_t)x.size())
                        refuse(at(i) + "width mismatch: slice [" + std::to_string(in.imm0) + ", +" + std::to_string(in.imm1) + ") of " +
                               std::to_string(x.size()) + " samples");
                    out.assign(x.begin() + in.imm0, x.begin() + in.imm0 + in.imm1);
                    break;
                }
                case WOP_SHL: {
                    const Word& x = reg(in.a, "a");
                    if (in.imm0 < 0) refuse(at(i) + "negative shift");
                    out.assign(x.size(), zero);
                    for (size_t j = (size_t)in.imm0; j < x.size(); j++) out[j] = x[j - in.imm0];
                    break;
                }
                case WOP_NOT: {
                    const Word& x = reg(in.a, "a");
                    out.resize(x.size());
                    CircuitBuilder::NOT(out, x, x.size());
                    break;
                }
                case WOP_CONCAT: {
                    const Word& lo = reg(in.a, "a");
                    const Word& hi = reg(in.b, "b");
                    result_width((int64_t)lo.size() + (int64_t)hi.size());
                    out = lo;
                    out.insert(out.end(), hi.begin(), hi.end());
                    break;
                }
                case WOP_AND:
                case WOP_OR:
                case WOP_XOR: {
                    const Word& x = reg(in.a, "a");
                    const Word& y = reg(in.b, "b");
                    same_width(x, y);
                    const int32_t type = in.op == WOP_AND ? GATE_AND : in.op == WOP_OR ? GATE_OR : GATE_XOR;
                    out.resize(x.size());
                    for (size_t j = 0; j < x.size(); j++) out[j] = b.gate(type, x[j], y[j]);
                    break;
                }
                case WOP_ANDBIT: {
                    const Word& x = reg(in.a, "a");
                    const Word& bit = reg(in.b, "b");
                    one_sample(bit, "b");
                    out.resize(x.size());
                    for (size_t j = 0; j < x.size(); j++) out[j] = b.AND(x[j], bit[0]);
                    break;
                }
                case WOP_ADD:
                case WOP_SUB:
                case WOP_RSUB:
                case WOP_MUL: {
                    const Word& x = reg(in.a, "a");
                    const Word& y = reg(in.b, "b");
                    same_width(x, y);
                    const int32_t base = in.op == WOP_ADD ? CIRC_ADD : in.op == WOP_SUB ? CIRC_SUB : in.op == WOP_RSUB ? CIRC_RSUB : CIRC_MUL;
                    if (in.family < FAMILY_REFERENCE || in.family > FAMILY_FULL_ADDER) refuse(at(i) + "unknown family " + std::to_string(in.family));
                    const int32_t kind = circuit_kind_in_family(base, (CircuitFamily)in.family);
                    if (kind == base && in.family != FAMILY_REFERENCE) refuse(at(i) + "family " + std::to_string(in.family) + " has no such operator");
                    if (!circuit_accepts_width(kind, (int32_t)x.size()))
                        refuse(at(i) + "width " + std::to_string(x.size()) + " is not one this operator takes in that family");
                    Word carry(32, zero);
                    if (in.c != -1) {
                        carry = reg(in.c, "c");
                        if (carry.size() != 32) refuse(at(i) + "width mismatch: the carry word must be 32 samples, not " + std::to_string(carry.size()));
                    }
                    out = build_word_operator(b, kind, x, y, carry);
                    break;
                }
                case WOP_SUM: {
                    result_width(in.width);
                    if (in.family != FAMILY_FULL_ADDER && in.family != FAMILY_KOGGE_STONE)
                        refuse(at(i) + "family " + std::to_string(in.family) + " has no addition for a sum (full adder or Kogge-Stone)");
                    if (in.first < 0 || in.count < 2 || (int64_t)in.first + in.count > (int64_t)n_args)
                        refuse(at(i) + "operands [" + std::to_string(in.first) + ", +" + std::to_string(in.count) + ") do not lie in the " +
                               std::to_string(n_args) + " given, or are fewer than two");
                    // two gates per compressor cell, at most width x (count - 2) cells, and the addition (Kogge-Stone: under 4 log2 per bit)
                    if (b.n_wires() + 2 * (int64_t)in.width * in.count + 64 * (int64_t)in.width >= kMaxWires)
                        refuse(at(i) + "too large: wires must stay under 2^30");
                    std::vector<Word> rows((size_t)in.count, Word(in.width, zero));
                    for (int32_t t = 0; t < in.count; t++) {
                        const WordArg& arg = args[in.first + t];
                        const Word& x = reg(arg.reg, "of the sum");
                        if (arg.shift < 0) refuse(at(i) + "negative shift");
                        for (int64_t j = arg.shift; j < in.width && j - arg.shift < (int64_t)x.size(); j++) rows[t][j] = x[j - arg.shift];
                    }
                    out = sum_rows(b, (CircuitFamily)in.family, in.width, rows);
                    break;
                }
                case WOP_LT: {
                    const Word& x = reg(in.a, "a");
                    const Word& y = reg(in.b, "b");
                    same_width(x, y);
                    // from the least significant bit up: where the bits agree the verdict so far stands, where they differ y's decides
                    Ref lt = zero;
                    for (size_t j = 0; j < x.size(); j++) lt = b.gate3(GATE_MUX, b.gate(GATE_XNOR, x[j], y[j]), lt, y[j]);
                    out = Word{lt};
                    break;
                }
                case WOP_EQ: {
                    const Word& x = reg(in.a, "a");
                    const Word& y = reg(in.b, "b");
                    same_width(x, y);
                    std::vector<Ref> same(x.size());
                    for (size_t j = 0; j < x.size(); j++) same[j] = b.gate(GATE_XNOR, x[j], y[j]);
                    out = Word{and_tree(b, same)};
                    break;
                }
                case WOP_SELECT: {
                    const Word& cond = reg(in.a, "a");
                    const Word& x = reg(in.b, "b");
                    const Word& y = reg(in.c, "c");
                    one_sample(cond, "a");
                    same_width(x, y);
                    out.resize(x.size());
                    for (size_t j = 0; j < x.size(); j++) out[j] = b.gate3(GATE_MUX, cond[0], x[j], y[j]);
                    break;
                }
                default: refuse(at(i) + "unknown opcode " + std::to_string(in.op));
            }
        } catch (const Refusal&) {
            throw;
        } catch (const std::bad_alloc&) {
            throw;
        } catch (const std::exception& e) {  // the builders' own refusals: a MAJ3 / XOR3 that names one wire twice, ...
            refuse(at(i) + e.what());
        }
        if (b.n_wires() >= kMaxWires) refuse(at(i) + "too large: wires must stay under 2^30");
    }

    Word outs;
    for (size_t o = 0; o < n_outputs; o++) {
        if (outputs[o] < 0 || (size_t)outputs[o] >= n_instrs)
            refuse("program: output " + std::to_string(o) + " refers to register " + std::to_string(outputs[o]) + ", which does not exist");
        const Word& r = regs[outputs[o]];
        outs.insert(outs.end(), r.begin(), r.end());
        if (outs.size() >= (size_t)kMaxWires) refuse("program: too many output samples");
    }
    CompiledProgram p;
    p.circuit = finalize_circuit("program", b, outs, (flags & kProgramBalanced) != 0, 0);
    p.circuit.n_reference_bootstraps = p.circuit.n_bootstraps;  // as a netlist: the export, compiled again, is the same object
    p.recorded = export_recorded(b, outs);
    return p;
}

}  // namespace ieache
