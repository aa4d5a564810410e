// packing_keygen and pack_reference (csrc/tfhe_host.h -- what ieache_packing_keygen / ieache_pack_reference call) as a stand-alone
// program for AddressSanitizer + UBSan: buffers of exactly the documented size (heap-allocated, so a word past either end is
// seen), every boundary of the rotate-and-sum, and a second opinion that gathers every output word by the definition instead of
// scattering rows.
// Built by tests/test_pack_cpu.py together with csrc/tfhe_host.cpp.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "tfhe_host.h"

using namespace ieache;

static int failures = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            failures++;                                              \
        }                                                            \
    } while (0)

// word (c, x) of out_g gathered: sum_p sum_q of coefficient x of X^a R_{g m + p}[c], a = p w + q + shift mod 2N
static void run(int32_t n, int32_t N, int32_t t, int32_t b, size_t groups, int32_t m, int32_t spread, int32_t shift) {
    Params p;
    p.n = n;
    p.N = N;
    Rng rng((uint64_t)(77 + n + N + t + m + shift));
    const size_t cols = 2 * (size_t)N, nrows = groups * (size_t)m;
    std::unique_ptr<Torus32[]> pk(new Torus32[(size_t)n * t * cols]), rows(new Torus32[nrows * (n + 1)]), out(new Torus32[groups * cols]);
    for (size_t i = 0; i < (size_t)n * t * cols; i++) pk[i] = rng.uniform_torus32();
    for (size_t i = 0; i < nrows * (n + 1); i++) rows[i] = rng.uniform_torus32();
    pk[0] = INT32_MIN;
    pk[1] = INT32_MAX;
    pack_reference(p, t, b, pk.get(), groups, m, spread, shift, rows.get(), out.get());
    std::vector<uint32_t> R(nrows * cols, 0u);
    for (size_t r = 0; r < nrows; r++) {
        R[r * cols + N] = (uint32_t)rows[r * (n + 1) + n];
        for (int32_t i = 0; i < n; i++) {
            const uint32_t abar = (uint32_t)rows[r * (n + 1) + i] + (1u << (31 - t * b));
            for (int32_t j = 0; j < t; j++) {
                const uint32_t d = (abar >> (32 - (j + 1) * b)) & ((1u << b) - 1u);
                for (size_t c = 0; c < cols; c++) R[r * cols + c] -= d * (uint32_t)pk[((size_t)i * t + j) * cols + c];
            }
        }
    }
    bool same = true;
    for (size_t g = 0; g < groups; g++)
        for (int32_t c = 0; c < 2; c++)
            for (int32_t x = 0; x < N; x++) {
                uint32_t acc = 0;
                for (int32_t pp = 0; pp < m; pp++)
                    for (int32_t q = 0; q < spread; q++) {
                        const int32_t a = (pp * spread + q + shift) % (2 * N);
                        const int32_t j = ((x - a) % (2 * N) + 2 * N) % (2 * N);
                        const uint32_t v = R[(g * m + pp) * cols + (size_t)c * N + (size_t)(j % N)];
                        acc += j < N ? v : 0u - v;
                    }
                same = same && acc == (uint32_t)out[g * cols + (size_t)c * N + x];
            }
    CHECK(same);
}

static void keygen_rows(int32_t n, int32_t N, int32_t t, int32_t b) {
    Params p;
    p.n = n;
    p.N = N;
    Rng rng((uint64_t)(5 + N));
    std::unique_ptr<int32_t[]> lwe(new int32_t[n]), ring(new int32_t[N]);
    for (int32_t i = 0; i < n; i++) lwe[i] = i == 0 ? 1 : rng.bit();
    for (int32_t i = 0; i < N; i++) ring[i] = rng.bit();
    const size_t count = (size_t)n * t;
    std::unique_ptr<Torus32[]> pk(new Torus32[count * 2 * N]), phase(new Torus32[count * N]);
    const double alpha = std::ldexp(1.0, -25);
    packing_keygen(p, lwe.get(), ring.get(), t, b, alpha, rng, pk.get());
    tlwe_phase(p, ring.get(), pk.get(), count, phase.get());
    for (size_t r = 0; r < count; r++)
        for (int32_t x = 0; x < N; x++) {
            const uint32_t want = x == 0 ? (uint32_t)lwe[r / t] << (32 - ((int32_t)(r % t) + 1) * b) : 0u;
            const double d = (double)(int32_t)((uint32_t)phase[r * N + x] - want) / 4294967296.0;
            CHECK(std::fabs(d) < 8 * alpha);
        }
}

int main() {
    for (int32_t shift : {0, 1, 15, 16, 17, 31}) {
        run(5, 16, 8, 2, 1, 1, 1, shift);
        run(5, 16, 5, 3, 3, 2, 8, shift);
        run(3, 16, 31, 1, 2, 16, 1, shift);
        run(3, 16, 7, 4, 1, 1, 16, shift);
    }
    for (int32_t shift : {0, 1023, 1024, 2047}) run(3, 1024, 8, 2, 1, 33, 31, shift);
    run(2, 1024, 8, 2, 1, 1024, 1, 1);
    run(5, 16, 8, 2, 0, 4, 1, 0);  // no groups: null-sized buffers untouched
    keygen_rows(3, 16, 5, 3);
    keygen_rows(2, 1024, 8, 2);
    if (failures) return 1;
    printf("PACK_REFERENCE_OK\n");
    return 0;
}
