// tgsw_encrypt_sample, cmux_reference, lut_tree_reference and tlwe_extract_reference (csrc/tfhe_host.h -- what the section-4 tools
// of include/ieache.h call) as a stand-alone program for AddressSanitizer + UBSan: buffers of exactly the documented size
// (heap-allocated, so a word past either end is seen), the extreme decompositions (l x Bgbit = 32, the largest Bgbit of a ring,
// Bgbit = 1), every index default, and a tree checked against flat calls chained by hand.
// Built by tests/test_cmux_cpu.py together with csrc/tfhe_host.cpp.
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

static void run(int32_t N, int32_t l, int32_t Bgbit, size_t n_set, int32_t depth, size_t count) {
    Params p;
    p.n = 4;
    p.N = N;
    p.l = l;
    p.Bgbit = Bgbit;
    CHECK(p.supported());
    Rng rng((uint64_t)(99 + N + 10 * l + Bgbit + depth));
    const size_t W = 2 * (size_t)N, S = (size_t)p.kpl() * W, T = (size_t)1 << depth;
    std::unique_ptr<int32_t[]> key(new int32_t[N]);
    for (int32_t i = 0; i < N; i++) key[i] = rng.bit();
    std::unique_ptr<Torus32[]> set(new Torus32[n_set * S]);
    for (size_t i = 0; i < n_set; i++) tgsw_encrypt_sample(p, key.get(), (int32_t)(i & 1), 1e-9, rng, set.get() + i * S);
    set[0] = INT32_MIN;
    set[n_set * S - 1] = INT32_MAX;
    const size_t n_tables = 2;
    std::unique_ptr<Torus32[]> tables(new Torus32[n_tables * T * W]), out(new Torus32[count * W]), chained(new Torus32[count * W]);
    for (size_t i = 0; i < n_tables * T * W; i++) tables[i] = rng.uniform_torus32();
    const size_t F = count < 3 ? 3 : count;  // rows for the flat calls and the extraction
    std::unique_ptr<Torus32[]> flat(new Torus32[F * W]);
    for (size_t i = 0; i < F * W; i++) flat[i] = rng.uniform_torus32();
    std::unique_ptr<int32_t[]> sel(new int32_t[count * (size_t)(depth ? depth : 1)]), tof(new int32_t[count]);
    for (size_t i = 0; i < count * (size_t)(depth ? depth : 1); i++) sel[i] = (int32_t)(rng.next() % n_set);
    for (size_t i = 0; i < count; i++) tof[i] = (int32_t)(i % n_tables);
    sel[count * (size_t)(depth ? depth : 1) - 1] = (int32_t)n_set - 1;
    tof[count - 1] = (int32_t)n_tables - 1;

    lut_tree_reference(p, set.get(), n_set, count, depth, sel.get(), tables.get(), tof.get(), out.get());
    // the same tree as flat calls, level by level
    for (size_t i = 0; i < count; i++) {
        std::vector<Torus32> rows(tables.get() + (size_t)tof[i] * T * W, tables.get() + ((size_t)tof[i] + 1) * T * W);
        for (int32_t k = 0; k < depth; k++) {
            const size_t w = rows.size() / W / 2;
            std::vector<Torus32> d1(w * W), d0(w * W), next(w * W);
            std::vector<int32_t> of(w, sel[i * (size_t)depth + k]);
            for (size_t j = 0; j < w; j++)
                for (size_t x = 0; x < W; x++) {
                    d0[j * W + x] = rows[2 * j * W + x];
                    d1[j * W + x] = rows[(2 * j + 1) * W + x];
                }
            cmux_reference(p, set.get(), n_set, w, of.data(), d1.data(), d0.data(), next.data());
            rows.swap(next);
        }
        for (size_t x = 0; x < W; x++) chained[i * W + x] = rows[x];
    }
    bool same = true;
    for (size_t x = 0; x < count * W; x++) same = same && out[x] == chained[x];
    CHECK(same);
    // the defaults of the index arrays, and d0 = null
    lut_tree_reference(p, set.get(), n_set, count, depth, nullptr, tables.get(), nullptr, out.get());
    cmux_reference(p, set.get(), n_set, count, nullptr, flat.get(), nullptr, out.get());
    // d0 = null is d0 = zeros
    std::vector<Torus32> zeros(count * W, 0), with0(count * W);
    cmux_reference(p, set.get(), n_set, count, nullptr, flat.get(), zeros.data(), with0.data());
    same = true;
    for (size_t x = 0; x < count * W; x++) same = same && out[x] == with0[x];
    CHECK(same);
    // extraction at the ends of the ring
    std::unique_ptr<Torus32[]> u(new Torus32[3 * ((size_t)N + 1)]);
    const int32_t js[3] = {0, 1, N - 1};
    tlwe_extract_reference(p, 3, flat.get(), js, u.get());
    for (int r = 0; r < 3; r++) {
        const Torus32* A = flat.get() + (size_t)r * W;
        CHECK(u[(size_t)r * (N + 1) + N] == A[N + js[r]] && u[(size_t)r * (N + 1)] == A[js[r]]);
        CHECK(u[(size_t)r * (N + 1) + N - 1] == (js[r] == N - 1 ? A[0] : (Torus32)(0u - (uint32_t)A[js[r] + 1])));
    }
    tlwe_extract_reference(p, 3, flat.get(), nullptr, u.get());
}

int main() {
    run(16, 3, 7, 3, 3, 2);
    run(16, 2, 16, 1, 2, 3);   // l x Bgbit = 32: the last digit's shift is 0
    run(16, 1, 27, 2, 1, 1);   // the largest Bgbit of N = 16
    run(32, 32, 1, 2, 2, 2);   // Bgbit = 1
    run(64, 2, 10, 5, 4, 2);
    run(64, 3, 7, 2, 0, 3);    // depth 0: a copy
    run(1024, 3, 7, 2, 1, 1);
    if (failures) return 1;
    printf("CMUX_REFERENCE_OK\n");
    return 0;
}
