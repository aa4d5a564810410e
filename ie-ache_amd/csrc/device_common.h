// Device-side structures and helpers shared by the evaluator's kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "circuit.h"
#include "level_items.h"
#include "params.h"

namespace ieache {
namespace dev {

struct DevKeys {
    int32_t n, N, M, logM, l, Bgbit, kpl, ks_t, ks_basebit, ks_base, stride;
    uint32_t dec_offset;
    const double2* bkf;   // [n][kpl][2][2 limbs][M], bit-reversed spectrum order
    const int32_t* ksk;   // [N][t][base][stride]
    const double2* twist; // exp(i*pi*j/N), j < M
    const double2* wtab;  // exp(-2*pi*i*j/M), j < M/2
};

// Where the gate instances of one launch live.
// Circuit mode: a level is `ng` gates per expression of which the last `nm` are MUX, i.e. ni = ng + nm ROTATION items per
// expression (level_items.h); item0 and the item index of a blind-rotation launch count rotation items.  The key switch of
// such a level runs on one row per GATE: it gets the same descriptor with nm = 0 and item0 in gate instances, for which
// the arithmetic below is the identity it has always been (only GateInst::out is used there).
// Programmable bootstrap (flat mode only, tv non-null): the row in flat_a is bootstrapped as it stands (flat_type < 0) and the
// accumulator starts from X^(2N-barb) * tv[row] instead of the constant polynomial, row = tv_of[item] (null: row 0) clamped
// into [0, n_tv).  flat_type == kFlatRawTlwe: the same call on a table of TLWE samples under the ring key -- rows of tv are 2N
// words, A then B, and the accumulator starts from X^(2N-barb) * (A, B) (kFlatRaw: rows of N words, the B half; A = 0).  To
// resolve() both are the raw row.  Only the prologues read these fields.  The descriptor is an argument of every key-switch kernel as
// well, and a larger one would move their other arguments -- and with them their code -- so the three fields take the bytes
// of circuit-mode fields, which a flat launch leaves at zero, and of a padding word: sizeof(WorkDesc) is what it was.
struct WorkDesc {
    const DevGate* gates;  // circuit mode when non-null
    union {
        struct {
            int32_t g0, ng;
        };
        const Torus32* tv;  // flat mode: test polynomials, [n_tv][N] (kFlatRawTlwe: [n_tv][2][N])
    };
    int32_t nm;            // circuit mode: MUX gates among the ng (the last ones)
    int32_t n_tv;          // flat mode: rows of tv
    union {
        Torus32* store;
        const int32_t* tv_of;  // flat mode: row of tv per item (indexed like flat_a: item0 + item), or null
    };
    int32_t n_slots;
    const Torus32* flat_a;  // flat mode: rows [item]
    const Torus32* flat_b;
    const Torus32* flat_c;  // third operand: of bootsMUX (flat_type == kFlatMux), of GATE_MAJ3 / GATE_XOR3
    Torus32* flat_out;
    int32_t flat_type;
    int64_t item0;
};
static_assert(sizeof(WorkDesc) == 88, "WorkDesc is a kernel argument: its size and field offsets are part of every kernel that takes it");

// flat_type of a programmable bootstrap: the row in flat_a as it stands; the table holds plain polynomials / TLWE samples
constexpr int32_t kFlatRaw = -1;
constexpr int32_t kFlatRawTlwe = -2;

// the test polynomial of a programmable-bootstrap item -- the start of its row of `row_words` words: N for a table of plain
// polynomials, 2N (A then B) for one of TLWE samples -- or null for a gate item (whose test polynomial is the constant kMU)
__device__ __forceinline__ const Torus32* test_poly_row(const WorkDesc& W, int64_t item, int32_t row_words) {
    if (W.gates || !W.tv) return nullptr;
    int32_t r = W.tv_of ? W.tv_of[item] : 0;
    r = r < 0 ? 0 : (r >= W.n_tv ? W.n_tv - 1 : r);  // a bad index gives a wrong answer, never a read outside the table
    return W.tv + (size_t)r * row_words;
}

// flat_type of the two blind rotations of bootsMUX(a,b,c) (boot-gates.cpp): item 2g is
// (0,-1/8) + a + b, item 2g+1 is (0,-1/8) - a + c; neither is key-switched on its own
constexpr int32_t kFlatMux = 16;

struct GateInst {
    const Torus32* a;
    const Torus32* b;
    const Torus32* c;  // third operand (GATE_MAJ3 / GATE_XOR3; null otherwise)
    Torus32* out;
    int32_t sa, sb, sc;  // signed multipliers (0 = operand is the constant, handled via cst)
    uint32_t cst;
};

// multipliers of the operands and the constant term of a one-rotation gate (kc = 0: a two-input gate)
__device__ __forceinline__ void gate_coeffs(int32_t type, int32_t& ka, int32_t& kb, int32_t& kc, uint32_t& cst) {
    // boot-gates.cpp: AND (0,-1/8)+ca+cb ; XOR (0,1/4)+2(ca+cb) ; OR (0,1/8)+ca+cb ; NAND (0,1/8)-ca-cb ;
    // XNOR (0,-1/4)-2(ca+cb) ; NOR (0,-1/8)-ca-cb ; ANDNY (0,-1/8)-ca+cb ; ANDYN (0,-1/8)+ca-cb ; ORNY (0,1/8)-ca+cb ;
    // ORYN (0,1/8)+ca-cb.  (In a circuit the last five arrive as AND / OR with operand sign flags; flat calls name them.)
    // Not in libtfhe: MAJ3 ca+cb+cc (phases +-1/8, +-3/8) ; XOR3 (0,1/2)+2(ca+cb+cc) (phases +-1/4) -- DESIGN.md section 7.
    kc = 0;
    switch (type) {
        case GATE_MAJ3: ka = kb = kc = 1; cst = 0u; break;
        case GATE_XOR3: ka = kb = kc = 2; cst = 0x80000000u; break;
        case GATE_AND: ka = kb = 1; cst = 0xE0000000u; break;
        case GATE_XOR: ka = kb = 2; cst = 0x40000000u; break;
        case GATE_OR: ka = kb = 1; cst = 0x20000000u; break;
        case GATE_XNOR: ka = kb = -2; cst = 0xC0000000u; break;
        case GATE_NOR: ka = kb = -1; cst = 0xE0000000u; break;
        case GATE_ANDNY: ka = -1; kb = 1; cst = 0xE0000000u; break;
        case GATE_ANDYN: ka = 1; kb = -1; cst = 0xE0000000u; break;
        case GATE_ORNY: ka = -1; kb = 1; cst = 0x20000000u; break;
        case GATE_ORYN: ka = 1; kb = -1; cst = 0x20000000u; break;
        default: ka = kb = -1; cst = 0x20000000u; break;  // NAND
    }
}

__device__ __forceinline__ GateInst resolve(const WorkDesc& W, int64_t item, int32_t stride) {
    GateInst g;
    int32_t type, ka, kb, kc;
    g.c = nullptr;
    g.sc = 0;
    if (W.gates) {
        const LevelItem it = level_item(item, W.ng, W.nm);  // nm == 0: (item / ng, item % ng, 0)
        const DevGate d = W.gates[W.g0 + it.gate];
        Torus32* base = W.store + (size_t)it.expr * W.n_slots * stride;
        type = d.type;
        int32_t y_slot = d.b_slot, y_neg = d.b_neg;  // second operand of this rotation
        if (type == GATE_MUX) {
            // bootsMUX(a, b, c): half 0 is (0,-1/8) + a + b, half 1 is (0,-1/8) - a + c
            g.cst = 0xE0000000u;
            ka = it.half ? -1 : 1;
            kb = 1;
            if (it.half) {
                y_slot = d.c_slot;
                y_neg = d.c_neg;
            }
        } else {
            gate_coeffs(type, ka, kb, kc, g.cst);
            if (kc) {  // a constant third operand has sc != 0 and no row: its b term goes into cst below
                g.c = d.c_slot >= 0 ? base + (size_t)d.c_slot * stride : nullptr;
                g.sc = d.c_neg ? -kc : kc;
            }
        }
        g.a = d.a_slot >= 0 ? base + (size_t)d.a_slot * stride : nullptr;
        g.b = y_slot >= 0 ? base + (size_t)y_slot * stride : nullptr;
        g.out = base + (size_t)d.out_slot * stride;
        g.sa = d.a_neg ? -ka : ka;
        g.sb = y_neg ? -kb : kb;
        // a constant operand is (0, -1/8): only its b term contributes
        if (!g.a) g.cst += (uint32_t)g.sa * 0xE0000000u;
        if (!g.b) g.cst += (uint32_t)g.sb * 0xE0000000u;
        if (!g.c) g.cst += (uint32_t)g.sc * 0xE0000000u;
    } else if (W.flat_type == kFlatMux) {
        const int64_t gi = item >> 1;
        const bool second = item & 1;
        g.cst = 0xE0000000u;
        g.a = W.flat_a + (size_t)gi * stride;
        g.b = (second ? W.flat_c : W.flat_b) + (size_t)gi * stride;
        g.out = nullptr;
        g.sa = second ? -1 : 1;
        g.sb = 1;
    } else {
        type = W.flat_type;
        gate_coeffs(type, ka, kb, kc, g.cst);
        g.a = W.flat_a + (size_t)item * stride;
        g.b = W.flat_b ? W.flat_b + (size_t)item * stride : nullptr;
        g.out = W.flat_out + (size_t)item * stride;
        g.sa = ka;
        g.sb = kb;
        if (kc) {
            g.c = W.flat_c + (size_t)item * stride;
            g.sc = kc;
        }
        if (type < 0) {  // raw bootstrap of the row in flat_a (debug hook)
            g.sa = 1;
            g.sb = 0;
            g.cst = 0;
            g.b = nullptr;
        }
    }
    return g;
}

__device__ __forceinline__ uint32_t combined_coef(const GateInst& g, int32_t i, int32_t n) {
    uint32_t v = 0;
    if (g.a) v += (uint32_t)g.sa * (uint32_t)g.a[i];
    if (g.b) v += (uint32_t)g.sb * (uint32_t)g.b[i];
    if (g.c) v += (uint32_t)g.sc * (uint32_t)g.c[i];
    if (i == n) v += g.cst;
    return v;
}

// libtfhe modSwitchFromTorus32(phase, 2N) for power-of-two N: (phase + 2^(31-log2(2N))) >> (32-log2(2N))
__device__ __forceinline__ int32_t modswitch2N(uint32_t phase, int32_t log2N2) {
    return (int32_t)((phase + (1u << (31 - log2N2))) >> (32 - log2N2));
}

// coefficient i of X^a * p  (mod X^N+1), a in [0,2N)
__device__ __forceinline__ int32_t rot_coef(const int32_t* p, int32_t i, int32_t a, int32_t N) {
    // branch-free: one load plus a conditional negate (a ?: on two loads compiles to
    // divergent branches with a full LDS wait inside each)
    const int32_t idx = (i - a) & (2 * N - 1);
    const uint32_t v = (uint32_t)p[idx & (N - 1)];
    return (int32_t)((idx & N) ? 0u - v : v);
}

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 cmul_conj(double2 a, double2 b) {  // a * conj(b)
    return make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
}
__device__ __forceinline__ double2 cfma(double2 a, double2 b, double2 c) {  // a*b + c
    return make_double2(fma(a.x, b.x, fma(-a.y, b.y, c.x)), fma(a.x, b.y, fma(a.y, b.x, c.y)));
}

// ---- host: dynamic LDS beyond the default 64 KiB ----
// A kernel has to be allowed its dynamic LDS size explicitly (hipFuncAttributeMaxDynamicSharedMemorySize), and the
// permission belongs to the (kernel, device) pair: a process that drives two devices needs it on each.  This is the only
// place that asks for it.
inline void allow_dynamic_lds(const void* kernel, size_t bytes, const char* name) {
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
        throw std::runtime_error(std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed for ") + name);
}
// ... remembered for launch paths that would otherwise ask before every launch: one word per kernel, bit d = granted on
// device d, so later launches on a device cost one hipGetDevice (a thread-local read) and no attribute call.  `bytes` must
// not depend on the call (devices past 63 are asked every time).
struct LdsGrant {
    std::atomic<uint64_t> devices{0};
};
inline void allow_dynamic_lds_once(LdsGrant& grant, const void* kernel, size_t bytes, const char* name) {
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) throw std::runtime_error(std::string("hipGetDevice failed before launching ") + name);
    const uint64_t bit = device < 64 ? 1ull << device : 0;
    if (grant.devices.load(std::memory_order_acquire) & bit) return;
    allow_dynamic_lds(kernel, bytes, name);
    grant.devices.fetch_or(bit, std::memory_order_release);
}

}  // namespace dev
}  // namespace ieache
