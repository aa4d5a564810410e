// The item arithmetic of circuit levels that contain MUX gates (ie-ache_amd/csrc/level_items.h), exhaustively for small
// sizes, and the netlist constructor's validation, as plain host C++ under AddressSanitizer / UBSan.  The device's resolve()
// and the executor's piece cutting use exactly these functions; a mistake here would be a stray store on the GPU.
// Built and run by tests/test_netlist_sanitizers_cpu.py.
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../ie-ache_amd/csrc/circuit.h"
#include "../../ie-ache_amd/csrc/level_items.h"

using namespace ieache;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                   \
        }                                                               \
    } while (0)

static int check_level(int32_t ng, int32_t nm, int64_t batch) {
    const int32_t ni = ng + nm, n2 = ng - nm;
    const int64_t items = (int64_t)ni * batch;
    // item -> (expression, gate, half): in range, every gate hit once (two-input) or twice in order (MUX), MUX gates last
    std::vector<int> hits((size_t)(ng * batch), 0);
    for (int64_t it = 0; it < items; it++) {
        const LevelItem r = level_item(it, ng, nm);
        CHECK(r.expr >= 0 && r.expr < batch && r.gate >= 0 && r.gate < ng && (r.half == 0 || r.half == 1));
        CHECK(r.half == 0 || r.gate >= n2);
        CHECK(hits[(size_t)(r.expr * ng + r.gate)] == r.half);
        hits[(size_t)(r.expr * ng + r.gate)]++;
        const int64_t first = level_first_item(r.expr * ng + r.gate, ng, nm);
        CHECK(first + r.half == it);
        CHECK(level_gate_boundary(it, ng, nm) == (r.half == 0));
        if (r.half == 0) CHECK(level_gates_before(it, ng, nm) == r.expr * ng + r.gate);
    }
    for (int64_t q = 0; q < (int64_t)ng * batch; q++) CHECK(hits[(size_t)q] == ((q % ng) >= n2 ? 2 : 1));
    CHECK(level_gate_boundary(items, ng, nm) && level_gates_before(items, ng, nm) == (int64_t)ng * batch);
    // pieces: for every planned piece size and every expression-aligned share of the batch (a pipeline's), the pieces tile the
    // share, start and end at gate boundaries, hold 1 .. want + 1 items, and each gate's rows lie inside its piece
    for (int64_t want = 1; want <= items + 1; want++)
        for (int64_t e0 = 0; e0 < batch; e0++) {
            const int64_t item0 = e0 * ni, share = items - item0;
            int64_t gates_seen = e0 * ng;
            for (int64_t done = 0; done < share;) {
                const int64_t cnt = level_piece_items(item0 + done, want, share - done, ng, nm);
                CHECK(cnt >= 1 && cnt <= want + 1 && cnt <= share - done);
                CHECK(level_gate_boundary(item0 + done, ng, nm) && level_gate_boundary(item0 + done + cnt, ng, nm));
                const int64_t g0 = level_gates_before(item0 + done, ng, nm), g1 = level_gates_before(item0 + done + cnt, ng, nm);
                CHECK(g0 == gates_seen && g1 > g0 && g1 - g0 <= cnt);
                for (int64_t q = g0; q < g1; q++) {
                    const int64_t row = level_first_item(q, ng, nm) - (item0 + done);
                    CHECK(row >= 0 && row + ((q % ng) >= n2 ? 1 : 0) < cnt);
                }
                gates_seen = g1;
                done += cnt;
            }
            CHECK(gates_seen == (int64_t)ng * batch);
        }
    return 0;
}

static bool refused(int32_t n_in, const std::vector<NetGate>& g, const std::vector<int32_t>& outs, const char* needle) {
    try {
        build_netlist(n_in, g.data(), g.size(), outs.data(), outs.size(), false);
    } catch (const std::invalid_argument& e) {
        return std::string(e.what()).find(needle) != std::string::npos;
    }
    return false;
}

int main() {
    for (int32_t ng = 1; ng <= 7; ng++)
        for (int32_t nm = 0; nm <= ng; nm++)
            for (int64_t batch = 1; batch <= 4; batch++)
                if (check_level(ng, nm, batch)) return 1;

    // a netlist through build -> simulate, and every refusal
    const int32_t w = 2;  // wire << 1
    std::vector<NetGate> g = {{GATE_XNOR, 0 * w, 1 * w, 0}, {GATE_MUX, 3 * w, 2 * w, 1 * w ^ 1}, {GATE_NOR, 4 * w, -1, 0}};
    for (int balanced = 0; balanced < 2; balanced++) {
        const std::vector<int32_t> outs = {5 * w, 4 * w ^ 1, -2, 0};
        const Circuit c = build_netlist(3, g.data(), g.size(), outs.data(), outs.size(), balanced != 0);
        CHECK(c.n_bootstraps == 4 && c.depth == 3 && c.max_width == 2 && c.n_by_type[GATE_MUX] == 1 && c.n_by_type[GATE_NOR] == 1);
        for (int v = 0; v < 8; v++) {
            const uint8_t in[3] = {(uint8_t)(v & 1), (uint8_t)((v >> 1) & 1), (uint8_t)((v >> 2) & 1)};
            uint8_t out[4];
            simulate_circuit(c, in, out);
            const int x = !(in[0] ^ in[1]), m = x ? in[2] : !in[1];
            CHECK(out[0] == 0 && out[1] == !m && out[2] == 0 && out[3] == in[0]);  // NOR(m, TRUE) = 0
        }
    }
    CHECK(refused(3, {{GATE_AND, 0, 3 * w, 0}}, {0}, "gate 0"));             // its own output
    CHECK(refused(3, {{GATE_AND, 0, 2, 0}, {GATE_MUX, 0, 2, 5 * w}}, {0}, "gate 1"));
    CHECK(refused(3, {{11, 0, 2, 0}}, {0}, "gate 0"));
    CHECK(refused(3, {{-1, 0, 2, 0}}, {0}, "gate 0"));
    CHECK(refused(3, {{GATE_AND, 0, 2, 4}}, {0}, "gate 0"));                  // third operand on a two-input gate
    CHECK(refused(3, {{GATE_AND, 0, -3, 0}}, {0}, "gate 0"));
    CHECK(refused(3, {{GATE_AND, 0, 2, 0}}, {4 * w}, "output 0"));
    CHECK(refused(0, {}, {-1}, "input"));
    CHECK(refused(3, {{GATE_AND, 0, 2, 0}}, {}, "output"));
    printf("LEVEL_ITEMS_OK\n");
    return 0;
}
