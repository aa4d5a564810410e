// Gate-DAG form of the arithmetic circuits of the reference's Cloud/cloud.c.
//
// The reference evaluates its circuits one libtfhe gate at a time
// (cloud.c:18-647).  Here the same gates are recorded as a DAG, levelised
// (every gate of a level is independent: ASAP levels, or a slack-balanced list
// schedule of the same DAG where build_circuit or the caller asks for one, with
// an optional cap on the gates per level) and given storage slots by liveness
// so that a whole level -- times the batch of expressions -- is one GPU launch.
// bootsNOT / bootsCOPY / bootsCONSTANT cost no bootstrap in libtfhe and none
// here: they are folded into wire references (sign flag, alias, constant).
//
// The parts: CircuitBuilder records gates; finalize_circuit
// schedules them and allocates slots; a table of kinds in circuit.cpp says what
// each CIRC_* code is; circuit_level_cap picks a level width for a batch;
// circuit_cache.h keeps built circuits.
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <tuple>
#include <vector>

namespace ieache {

// Reference to an LWE sample inside a circuit.
//   id >= 0 : wire (inputs are wires 0..n_inputs-1, gate outputs follow)
//   id == kConstId : bootsCONSTANT(0) = (0, -1/8); neg flips it to CONSTANT(1)
//   id == kUndefId : never-written storage (new_gate_bootstrapping_ciphertext_array)
struct Ref {
    int32_t id;
    bool neg;
};
constexpr int32_t kConstId = -1;
constexpr int32_t kUndefId = -2;

// libtfhe's boot-gates.cpp.  AND / XOR / OR / NAND / XNOR / MUX are what the device executes.  NOR, ANDNY, ANDYN, ORNY, ORYN
// are AND / OR with operand signs flipped -- the same linear combination as libtfhe's, word for word -- and are recorded
// that way (CircuitBuilder::gate lowers them), so a DevGate's type is never one of them.
enum GateType : int32_t {
    GATE_AND = 0, GATE_XOR = 1, GATE_OR = 2, GATE_NAND = 3,
    GATE_MUX = 4,    // a ? b : c -- two blind rotations, one key switch
    GATE_NOR = 5,    // (0,-1/8) - ca - cb   = AND(NOT a, NOT b)
    GATE_XNOR = 6,   // (0,-1/4) - 2(ca+cb)  -- the negated INPUT of XOR's bootstrap, not NOT(XOR): a type of its own
    GATE_ANDNY = 7,  // (0,-1/8) - ca + cb   = AND(NOT a, b)
    GATE_ANDYN = 8,  // (0,-1/8) + ca - cb   = AND(a, NOT b)
    GATE_ORNY = 9,   // (0, 1/8) - ca + cb   = OR(NOT a, b)
    GATE_ORYN = 10,  // (0, 1/8) + ca - cb   = OR(a, NOT b)
    GATE_TYPES = 11,  // the libtfhe types above; Circuit::n_by_type and the ABI's count array have this length
    // Three-input gates of ONE blind rotation each (not libtfhe's; DESIGN.md section 7 has the noise budget).  Their codes lie
    // outside 0 .. GATE_TYPES-1 so that everything sized or bounded by GATE_TYPES stays as it is.
    GATE_MAJ3 = 32,  // ca + cb + cc              majority of three: phases +-1/8, +-3/8
    GATE_XOR3 = 33,  // (0,1/2) + 2(ca+cb+cc)     parity of three: phases +-1/4
};
constexpr bool is_gate3(int32_t type) { return type == GATE_MAJ3 || type == GATE_XOR3; }

struct Gate {
    int32_t type;
    Ref a, b;
    int32_t out;    // wire id
    int32_t level;  // 1-based ASAP level
    Ref c{kConstId, false};  // third operand (GATE_MUX, GATE_MAJ3, GATE_XOR3)
};

using Word = std::vector<Ref>;

// Mirrors the helper functions of cloud.c on symbolic samples.
class CircuitBuilder {
public:
    // fold: constant-fold and share gates while recording (opt-in, SURVEY App. C note): a gate with
    // a bootsCONSTANT operand, or with the same sample on both inputs, collapses to a wire / its
    // NOT / a constant, and a gate already recorded on the same operands is reused.  The circuit
    // then decrypts to the same bits with fewer bootstraps; its ciphertext bits differ from the
    // reference's (which bootstraps even `x AND 0`), so this is never the default.
    explicit CircuitBuilder(int32_t n_inputs, bool fold = false);
    Ref input(int32_t i) const;
    Word input_word(int32_t first, int32_t count = 32) const;
    static Ref constant(int v) { return Ref{kConstId, v != 0}; }            // bootsCONSTANT
    static Ref NOT(Ref a) { return Ref{a.id, !a.neg}; }                     // bootsNOT
    static Word fresh(int32_t count = 32) { return Word(count, Ref{kUndefId, false}); }
    Ref gate(int32_t type, Ref a, Ref b);                                    // bootsAND / bootsXOR ...
    // bootsMUX: a ? b : c (recorded as given), or GATE_MAJ3 / GATE_XOR3.  The latter two must name three different wires
    // (constants may repeat): the same wire twice adds its noise coherently.  With fold on, a repeated wire or a constant
    // operand lowers the gate instead (MAJ3(a,b,0) = AND, MAJ3(a,b,1) = OR, XOR3(a,b,k) = XOR / XNOR) and gates are shared.
    Ref gate3(int32_t type, Ref a, Ref b, Ref c);
    Ref MAJ3(Ref a, Ref b, Ref c) { return gate3(GATE_MAJ3, a, b, c); }
    Ref XOR3(Ref a, Ref b, Ref c) { return gate3(GATE_XOR3, a, b, c); }
    Ref AND(Ref a, Ref b) { return gate(GATE_AND, a, b); }
    Ref XOR(Ref a, Ref b) { return gate(GATE_XOR, a, b); }

    // cloud.c:18-51
    void add(Word& sum, Word& carryover, const Word& x, const Word& y, const Word& c, int32_t nb_bits);
    // cloud.c:53-57 / 59-63
    static void zero(Word& result, size_t size);
    static void NOT(Word& result, const Word& x, size_t size);
    // cloud.c:65-113
    void split(Word& f1, Word& f2, Word& f3, const Word& a, const Word& b, const Word& c,
               const Word& d, const Word& e, const Word& carry, int32_t nb_bits);
    // cloud.c:115-218 / 220-385 / 387-647.  `in` low word first; `results` high word first.
    void mul_words(std::vector<Word*> results, const std::vector<const Word*>& in, const Word& m,
                   const Word& carry, int32_t nb_bits);
    void mul32(Word& result, Word& result2, const Word& a, const Word& b, const Word& carry, int32_t nb_bits);  // :115-218

    int32_t n_inputs() const { return n_inputs_; }
    const std::vector<Gate>& gates() const { return gates_; }
    int32_t n_wires() const { return next_wire_; }
    const std::vector<int32_t>& requested_types() const { return requested_type_; }
    int64_t n_requested() const { return n_requested_; }  // gates the reference performs (before folding)

private:
    // gate() after its checks and its count: lowers NOR .. ORYN, folds and shares when fold is on, records the rest
    Ref gate2(int32_t type, Ref a, Ref b);
    // The one place a gate is recorded: its ASAP level from its operands, a new wire.  With fold on, a gate already recorded
    // with this type on these operands is returned instead.  -> the gate's wire
    int32_t record(int32_t type, int32_t requested, Ref a, Ref b, Ref c);
    int32_t n_inputs_;
    int32_t next_wire_;
    bool fold_;
    int64_t n_requested_ = 0;
    std::vector<Gate> gates_;
    std::vector<int32_t> requested_type_;  // per recorded gate: the type asked for (before NOR .. ORYN were lowered)
    std::vector<int32_t> wire_level_;
    // (type,a,na,b,nb,c,nc) -> wire; c = the constant 0 for a two-input gate
    std::map<std::tuple<int32_t, int32_t, int32_t, int32_t, int32_t, int32_t, int32_t>, int32_t> known_;
};

// One gate as the device executor consumes it.  Slots index the wire store;
// slot -1 means the constant (0,-1/8).  flags bit0 = negate the operand.
// c_*: third operand of a GATE_MUX, GATE_MAJ3 or GATE_XOR3 (unused, slot -1, otherwise).
struct DevGate {
    int32_t type;
    int32_t a_slot, a_neg;
    int32_t b_slot, b_neg;
    int32_t out_slot;
    int32_t c_slot, c_neg;
};

struct OutRef {
    int32_t slot;  // -1 = constant
    int32_t neg;
};

// A levelised, slot-allocated circuit, ready for the executor.
struct Circuit {
    std::string name;
    int32_t n_inputs = 0;               // input samples per expression (slots 0..n_inputs-1 on entry)
    int32_t n_slots = 0;                // wire-store rows per expression
    std::vector<DevGate> gates;         // sorted by level
    std::vector<int32_t> level_offset;  // gates of level L are [level_offset[L-1], level_offset[L])
    std::vector<int32_t> level_mux;     // [L-1]: how many of level L's gates are MUX -- the LAST ones of the level (level_items.h)
    std::vector<OutRef> outputs;        // output samples per expression
    // statistics.  Counts and widths are in BLIND ROTATIONS: a MUX gate counts 2 (as libtfhe's bootsMUX
    // bootstraps twice), so that batch x n_bootstraps is what an evaluation reports and a width is what a launch holds.
    int64_t n_bootstraps = 0, n_and = 0, n_xor = 0;
    int64_t n_by_type[GATE_TYPES] = {};  // gates by the type they were requested as (a MUX counts 1 here)
    int64_t n_maj3 = 0, n_xor3 = 0;      // the three-input gates, whose codes lie outside n_by_type
    int64_t count_of(int32_t type) const {  // gates of any valid type code; -1 for a code that names no gate
        if (type >= 0 && type < GATE_TYPES) return n_by_type[type];
        return type == GATE_MAJ3 ? n_maj3 : type == GATE_XOR3 ? n_xor3 : -1;
    }
    int32_t depth = 0, max_width = 0;  // ASAP depth / widest ASAP level
    int32_t sched_max_width = 0;       // widest level of the schedule actually executed
    int64_t n_reference_bootstraps = 0;  // what cloud.c performs for this circuit (== n_bootstraps unless folded)
    bool balanced_schedule = false;      // slack-balanced list schedule (64/128-bit multipliers) rather than ASAP levels
    int32_t n_levels() const { return (int32_t)level_offset.size() - 1; }
    int32_t n_mux(int32_t L) const { return level_mux.empty() ? 0 : level_mux[L - 1]; }  // MUX gates of level L (1-based)
};

// Levelise + allocate slots.  `outputs` are the samples to return per expression.
// balanced: slack-aware list schedule (default) instead of plain ASAP levels.
// level_cap > 0: gates per level of the balanced schedule (0 = the mean ASAP width); see circuit_level_cap().
Circuit finalize_circuit(const std::string& name, const CircuitBuilder& b, const Word& outputs, bool balanced = true,
                         int32_t level_cap = 0);

// A caller-defined netlist (include/ieache.h: ieache_netlist_create).  Gate g's output is wire n_inputs + g; a reference is
// wire << 1 | negated, or -2 / -1 for the constants false / true.  Every recorded gate is bootstrapped (no folding).
// Throws std::invalid_argument naming the offending gate; nothing is returned half-built.
struct NetGate {
    int32_t type, a, b, c;
};
// The gate list a builder recorded, in the form build_netlist takes: gate g's output is wire n_inputs + g, the references of
// `outputs` likewise.  A gate lowered while recording (NOR .. ORYN) is given back as the type it was requested as, so feeding
// the list to build_netlist records the same gates again; with folding on it is the list AFTER folding and sharing.
struct RecordedNetlist {
    std::vector<NetGate> gates;
    std::vector<int32_t> outputs;
};
RecordedNetlist export_recorded(const CircuitBuilder& b, const Word& outputs);
// recorded (may be null): filled with export_recorded of what was built
Circuit build_netlist(int32_t n_inputs, const NetGate* gates, size_t n_gates, const int32_t* outputs, size_t n_outputs,
                      bool balanced, RecordedNetlist* recorded = nullptr);

// ---- the circuits main() dispatches to (cloud.c:870-2718) ----
// Input sample order for all of them: operand 1 words (32 samples each, LSB
// first, least-significant word first), operand 2 words, then operand 1's
// carry word (ciphertextcarry1, 32 samples).  See `circuit_inputs()`.
enum CircuitKind : int32_t {
    CIRC_ADD = 1,     // A+B                  cloud.c:870-1190
    CIRC_SUB = 2,     // A + (~B+1)           cloud.c:1196-1807
    CIRC_RSUB = 3,    // B + (~A+1)           cloud.c:1809-2365
    CIRC_MUL = 4,     // A*B, double width    cloud.c:2366-2718
    CIRC_MULADD = 5,  // (A*B)+C fused two-stage (compute_final chaining), 32/64/128-bit A,B
    // parallel-prefix (Kogge-Stone) adders, still XOR/AND only.  Same inputs and
    // outputs as ADD/SUB/RSUB and the same decrypted result (the carry word must encrypt 0, as
    // alice.c:147-149 guarantees), but NOT the same ciphertext bits: depth 2*log2(bits)+2 instead
    // of 3*bits, ~3.4x the bootstraps.  For small batches, where depth is what costs.
    CIRC_ADD_KS = 6,
    CIRC_SUB_KS = 7,
    CIRC_RSUB_KS = 8,
    // The multiplier counterpart of the Kogge-Stone adders (opt-in, same decrypted product, NOT the
    // reference's ciphertext): all bits*bits partial products at once, column-wise carry-save (Wallace)
    // reduction with XOR/AND-only full adders, one Kogge-Stone addition of the last two rows.  32 bits:
    // 32 levels instead of mul32's 255 and fewer bootstraps -- for single expressions, where depth is
    // what a level-batched evaluator pays for (cloud.c:115-218 is a 32-round ripple accumulate).
    CIRC_MUL_WALLACE = 9,
    // The same operators on the two-bootstrap full adder: sum = XOR3(x, y, c), carry = MAJ3(x, y, c) (opt-in; same inputs,
    // outputs and decrypted result as ADD / SUB / RSUB / MUL, NOT the reference's gate sequence).  ADD_FA is a ripple whose
    // carry-in is bit 0 of the carry word, as the reference's; SUB_FA / RSUB_FA add the complement with a constant-true
    // carry-in, so like the _KS kinds they need a carry word that encrypts 0 (alice.c:147-149).  MUL_FA: bits*bits ANDs, a
    // row-by-row carry-save array of full adders, one full-adder ripple over the last two rows.
    CIRC_ADD_FA = 16,
    CIRC_SUB_FA = 17,
    CIRC_RSUB_FA = 18,
    CIRC_MUL_FA = 19,
    // any two operators chained as compute_final() does
    // (Cloud/dragonfly_cipher_cloud.py:1300-1327), fused into one DAG: stage 1 = k1(A, B),
    // stage 2 = k2(op1, op2) with (op1, op2) = (answer, C) when flip (cloud.data = answer | C,
    // :1306-1314) or (C, answer) otherwise (:1318-1326).  kind = chain_kind(k1, k2, flip),
    // k1, k2 in {ADD, SUB, RSUB, MUL}.  Inputs: A, B, carry word, C at stage 2's width
    // (bits, or 2*bits after a MUL) [, C's carry word when !flip].
    CIRC_CHAIN_BASE = 32,
    CIRC_CHAIN_END = 64,
};
// What a plain (non-chain) kind is built from, besides its operator: the reference's gate list or one of the opt-in circuits.
enum CircuitFamily : int32_t {
    FAMILY_REFERENCE = 0,    // ADD / SUB / RSUB / MUL
    FAMILY_KOGGE_STONE = 1,  // the _KS adders
    FAMILY_CARRY_SAVE = 2,   // MUL_WALLACE
    FAMILY_FULL_ADDER = 3,   // the _FA kinds
};
// whether a kind multiplies (a chain: in either stage); false for a code that names no kind
bool circuit_multiplies(int32_t kind);
// the kind of the same operator in another family (CIRC_SUB, FAMILY_FULL_ADDER -> CIRC_SUB_FA); `kind` itself where that
// family has no such operator (there is no Kogge-Stone multiplier) and for chains and unknown codes
int32_t circuit_kind_in_family(int32_t kind, CircuitFamily family);
// whether build_circuit accepts this operand width for the kind: the adders 1 .. 256, the multipliers 32 / 64 / 128, a chain
// what its two stages accept (stage 2 at stage 1's output width)
bool circuit_accepts_width(int32_t kind, int32_t bits);
constexpr int32_t chain_kind(int32_t k1, int32_t k2, bool flip) { return CIRC_CHAIN_BASE + (k1 - 1) + 4 * (k2 - 1) + (flip ? 0 : 16); }
// decodes a CHAIN kind (CIRC_MULADD counts as chain(MUL, ADD, flip)); false for plain kinds
bool decode_chain(int32_t kind, int32_t* k1, int32_t* k2, bool* flip);

// bits: operand width.  ADD/SUB/RSUB accept any bits >= 1 (the reference uses
// 32/64/128/256; 16 is BASELINE.json's generalisation add(...,16,...));
// MUL accepts 32/64/128.  Returns false for unsupported combinations.
// balanced=true lets the builder pick the slack-balanced schedule where it saves memory
// (64/128-bit multipliers); false forces plain ASAP levels.
// fold=true: constant-folded / gate-shared variant (decrypt-identical, fewer bootstraps; opt-in).
bool build_circuit(int32_t kind, int32_t bits, Circuit* out, bool balanced = true, bool fold = false, int32_t level_cap = 0);
// One plain kind's operator on symbolic operands, recorded into `b` exactly as build_circuit records it for that kind (the
// word programs of program.h are made of these): A and B of one width the kind accepts, carry = the 32-sample carry word.
// -> the value samples, LSB first (2 x width for a multiplier).  Throws std::invalid_argument for a chain or unknown kind, operands of
// different widths, a width the kind table refuses or a carry word that is not 32 samples.
Word build_word_operator(CircuitBuilder& b, int32_t kind, const Word& A, const Word& B, const Word& carry);
// x + y + cin (equal widths, any width >= 1) as the opt-in adders build it: FAMILY_KOGGE_STONE or FAMILY_FULL_ADDER
Word build_family_adder(CircuitBuilder& b, CircuitFamily family, const Word& x, const Word& y, Ref cin);
// Level width (gates per expression) that makes `batch` expressions fill whole rounds of `resident` workgroups:
// the multiple of resident / gcd(resident, batch) nearest to the circuit's mean width, or 0 (= keep the mean) when
// a level is under one round anyway or the batch already is a multiple of a round.
// `base`: the circuit under its default schedule.
int32_t circuit_level_cap(const Circuit& base, int64_t batch, int32_t resident, int32_t resident_alt = 0);
// number of input / output samples per expression of a circuit kind
int32_t circuit_n_inputs(int32_t kind, int32_t bits);
int32_t circuit_n_outputs(int32_t kind, int32_t bits);

// Pure-integer simulation of a circuit on plaintext bits (for host tests):
// in[n_inputs] -> out[outputs.size()], each 0/1.
void simulate_circuit(const Circuit& c, const uint8_t* in, uint8_t* out);

}  // namespace ieache
