// lut_scatter_reference (csrc/tfhe_host.h -- what ieache_lut_scatter_reference of include/ieache.h section 4 calls) as a
// stand-alone program for AddressSanitizer + UBSan: buffers of exactly the documented size (heap-allocated, so a word past
// either end is seen), the extreme decompositions, both index defaults, mem given / null / the output itself, and the steps
// checked against flat external products (cmux_reference with d0 = null) chained by hand.
// Built by tests/test_scatter_cpu.py together with csrc/tfhe_host.cpp.
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
    Rng rng((uint64_t)(199 + N + 10 * l + Bgbit + depth));
    const size_t W = 2 * (size_t)N, S = (size_t)p.kpl() * W, T = (size_t)1 << depth, D = (size_t)(depth ? depth : 1);
    std::unique_ptr<Torus32[]> set(new Torus32[n_set * S]), values(new Torus32[count * W]), mem(new Torus32[count * T * W]);
    std::unique_ptr<Torus32[]> out(new Torus32[count * T * W]), leaves(new Torus32[count * T * W]);
    for (size_t i = 0; i < n_set * S; i++) set[i] = rng.uniform_torus32();
    set[0] = INT32_MIN;
    set[n_set * S - 1] = INT32_MAX;
    for (size_t i = 0; i < count * W; i++) values[i] = rng.uniform_torus32();
    for (size_t i = 0; i < count * T * W; i++) mem[i] = rng.uniform_torus32();
    std::unique_ptr<int32_t[]> sel(new int32_t[count * D]);
    for (size_t i = 0; i < count * D; i++) sel[i] = (int32_t)(rng.next() % n_set);
    sel[count * D - 1] = (int32_t)n_set - 1;

    lut_scatter_reference(p, set.get(), n_set, count, depth, sel.get(), values.get(), nullptr, leaves.get());
    lut_scatter_reference(p, set.get(), n_set, count, depth, sel.get(), values.get(), mem.get(), out.get());
    bool same = true;
    for (size_t x = 0; x < count * T * W; x++) same = same && (uint32_t)out[x] == (uint32_t)mem[x] + (uint32_t)leaves[x];
    CHECK(same);
    // the same steps as flat external products, most significant selector first
    for (size_t i = 0; i < count; i++) {
        std::vector<Torus32> rows(values.get() + i * W, values.get() + (i + 1) * W);
        for (int32_t t = 0; t < depth; t++) {
            const size_t w = rows.size() / W;
            std::vector<Torus32> hi(w * W), next(2 * w * W);
            std::vector<int32_t> of(w, sel[i * D + (size_t)(depth - 1 - t)]);
            cmux_reference(p, set.get(), n_set, w, of.data(), rows.data(), nullptr, hi.data());
            for (size_t j = 0; j < w; j++)
                for (size_t x = 0; x < W; x++) {
                    next[(2 * j + 1) * W + x] = hi[j * W + x];
                    next[2 * j * W + x] = (Torus32)((uint32_t)rows[j * W + x] - (uint32_t)hi[j * W + x]);
                }
            rows.swap(next);
        }
        same = true;
        for (size_t x = 0; x < T * W; x++) same = same && rows[x] == leaves[i * T * W + x];
        CHECK(same);
        // the leaves of an item sum to its value, word for word
        for (size_t x = 0; x < W; x++) {
            uint32_t sum = 0;
            for (size_t j = 0; j < T; j++) sum += (uint32_t)leaves[(i * T + j) * W + x];
            same = same && sum == (uint32_t)values[i * W + x];
        }
        CHECK(same);
    }
    // in place: the output is the memory itself
    std::unique_ptr<Torus32[]> inplace(new Torus32[count * T * W]);
    for (size_t x = 0; x < count * T * W; x++) inplace[x] = mem[x];
    lut_scatter_reference(p, set.get(), n_set, count, depth, sel.get(), values.get(), inplace.get(), inplace.get());
    same = true;
    for (size_t x = 0; x < count * T * W; x++) same = same && inplace[x] == out[x];
    CHECK(same);
    // the default of the index array
    lut_scatter_reference(p, set.get(), n_set, count, depth, nullptr, values.get(), nullptr, out.get());
}

int main() {
    run(16, 3, 7, 3, 3, 2);
    run(16, 2, 16, 1, 2, 3);   // l x Bgbit = 32: the last digit's shift is 0
    run(16, 1, 27, 2, 1, 1);   // the largest Bgbit of N = 16
    run(32, 32, 1, 2, 2, 2);   // Bgbit = 1
    run(64, 2, 10, 5, 4, 2);
    run(64, 3, 7, 2, 0, 3);    // depth 0: mem + v
    run(1024, 3, 7, 2, 1, 1);
    if (failures) return 1;
    printf("SCATTER_REFERENCE_OK\n");
    return 0;
}
