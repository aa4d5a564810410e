// The item arithmetic of a circuit level that contains bootsMUX gates (device_common.h: resolve; evaluator.hip: run_items,
// k_level_combine), free of any device state so that the CPU tests can check it exhaustively (tests/native/level_items_test.cpp).
//
// A level of one expression is `ng` gates of which the LAST `nm` are MUX (finalize_circuit orders them so).  A two-input gate
// is one blind rotation, a MUX is two (boot-gates.cpp: (0,-1/8) + a + b and (0,-1/8) - a + c), so the level is
//     ni = ng + nm          rotation items per expression,
// laid out gate by gate: the ng - nm two-input gates first, then the two halves of each MUX side by side.  Over a batch the
// items are expression-major (item = expression x ni + position), the gates likewise (gate instance = expression x ng + gate).
// With nm == 0 both numberings coincide and everything below is the identity.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define IEACHE_HD __host__ __device__ __forceinline__
#else
#define IEACHE_HD inline
#endif

namespace ieache {

struct LevelItem {
    int64_t expr;  // expression of the batch
    int32_t gate;  // gate of the level, 0 .. ng - 1
    int32_t half;  // 0, or 1 for the second rotation of a MUX
};

// rotation item -> (expression, gate, half)
IEACHE_HD LevelItem level_item(int64_t item, int32_t ng, int32_t nm) {
    const int32_t ni = ng + nm, n2 = ng - nm;
    LevelItem r;
    r.expr = item / ni;
    const int32_t pos = (int32_t)(item - r.expr * ni);
    const int32_t over = pos - n2;  // >= 0: inside the MUX part of the level
    r.gate = over >= 0 ? n2 + (over >> 1) : pos;
    r.half = over >= 0 ? (over & 1) : 0;
    return r;
}

// gate instance (expression x ng + gate) -> its first rotation item
IEACHE_HD int64_t level_first_item(int64_t gate_instance, int32_t ng, int32_t nm) {
    const int64_t expr = gate_instance / ng;
    const int32_t gate = (int32_t)(gate_instance - expr * ng), n2 = ng - nm;
    return expr * (ng + nm) + (gate >= n2 ? n2 + 2 * (gate - n2) : gate);
}

// whether rotation item `item` is the first item of a gate (or the end of the level's items): a piece may be cut there
IEACHE_HD bool level_gate_boundary(int64_t item, int32_t ng, int32_t nm) {
    const int32_t ni = ng + nm;
    const int32_t over = (int32_t)(item % ni) - (ng - nm);
    return over <= 0 || (over & 1) == 0;
}

// gate instances whose first rotation item lies before `item` (item a gate boundary): the gate numbering of a cut
IEACHE_HD int64_t level_gates_before(int64_t item, int32_t ng, int32_t nm) {
    const int32_t ni = ng + nm, n2 = ng - nm;
    const int64_t expr = item / ni;
    const int32_t pos = (int32_t)(item - expr * ni);
    return expr * ng + (pos > n2 ? n2 + (pos - n2 + 1) / 2 : pos);
}

// THE PIECE-CUT RULE.  A piece of a level starts at a gate boundary `first` and may hold `want` (>= 1) of the `left`
// rotation items that remain; it ends at the next gate boundary at or after first + want, so that both rotations of a MUX
// land in the same piece (their extracted rows are summed before the key switch).  A piece therefore holds at most
// want + 1 items -- scratch is sized for that -- and never 0.
IEACHE_HD int64_t level_piece_items(int64_t first, int64_t want, int64_t left, int32_t ng, int32_t nm) {
    if (want >= left) return left;
    return level_gate_boundary(first + want, ng, nm) ? want : want + 1;
}

}  // namespace ieache
