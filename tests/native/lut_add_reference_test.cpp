// lut_add_reference (csrc/tfhe_host.h -- what ieache_lut_add_reference of include/ieache.h section 4 calls) as a stand-alone
// program for AddressSanitizer + UBSan: buffers of exactly the documented size (heap-allocated, so a word past either end is
// seen), every optional array given and null, mems given / null / the output itself, depth 0 and steps 0, and the result
// checked against tlwe_rotate_reference, lut_scatter_reference and a sum written out by hand.
// Built by tests/test_lut_add_cpu.py together with csrc/tfhe_host.cpp.
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

static void run(int32_t N, int32_t l, int32_t Bgbit, size_t n_set, int32_t depth, int32_t steps, size_t count, size_t n_mems) {
    Params p;
    p.n = 4;
    p.N = N;
    p.l = l;
    p.Bgbit = Bgbit;
    CHECK(p.supported());
    Rng rng((uint64_t)(299 + N + 10 * l + Bgbit + depth + 7 * steps));
    const size_t W = 2 * (size_t)N, S = (size_t)p.kpl() * W, T = (size_t)1 << depth, D = (size_t)(depth + steps);
    std::unique_ptr<Torus32[]> set(new Torus32[n_set * S]), values(new Torus32[count * W]), mems(new Torus32[n_mems * T * W]);
    std::unique_ptr<Torus32[]> out(new Torus32[n_mems * T * W]), zeros(new Torus32[n_mems * T * W]);
    for (size_t i = 0; i < n_set * S; i++) set[i] = rng.uniform_torus32();
    set[0] = INT32_MIN;
    set[n_set * S - 1] = INT32_MAX;
    for (size_t i = 0; i < count * W; i++) values[i] = rng.uniform_torus32();
    for (size_t i = 0; i < n_mems * T * W; i++) mems[i] = rng.uniform_torus32();
    std::unique_ptr<int32_t[]> sel(new int32_t[count * D + 1]), mem_of(new int32_t[count]), amounts(new int32_t[steps + 1]);
    for (size_t i = 0; i < count * D; i++) sel[i] = (int32_t)(rng.next() % n_set);
    for (size_t i = 0; i < count; i++) mem_of[i] = (int32_t)(rng.next() % n_mems);
    mem_of[count - 1] = (int32_t)n_mems - 1;
    for (int32_t t = 0; t < steps; t++) amounts[t] = (int32_t)(rng.next() % (2 * (size_t)N));

    lut_add_reference(p, set.get(), n_set, count, depth, steps, sel.get(), amounts.get(), values.get(), mems.get(), n_mems, mem_of.get(), out.get());
    // by hand: rotate (selectors 0 .. steps - 1 of each item), scatter (the rest) with no memory, sum per memory
    std::vector<int32_t> low(count * (size_t)steps + 1), high(count * (size_t)depth + 1);
    for (size_t i = 0; i < count; i++) {
        for (size_t t = 0; t < (size_t)steps; t++) low[i * steps + t] = sel[i * D + t];
        for (size_t k = 0; k < (size_t)depth; k++) high[i * depth + k] = sel[i * D + steps + k];
    }
    std::vector<Torus32> turned(count * W), leaves(count * T * W), want(mems.get(), mems.get() + n_mems * T * W);
    tlwe_rotate_reference(p, set.get(), n_set, count, steps, low.data(), amounts.get(), values.get(), turned.data());
    lut_scatter_reference(p, set.get(), n_set, count, depth, high.data(), turned.data(), nullptr, leaves.data());
    for (size_t i = 0; i < count; i++)
        for (size_t x = 0; x < T * W; x++) want[(size_t)mem_of[i] * T * W + x] = (Torus32)((uint32_t)want[(size_t)mem_of[i] * T * W + x] + (uint32_t)leaves[i * T * W + x]);
    bool same = true;
    for (size_t x = 0; x < n_mems * T * W; x++) same = same && out[x] == want[x];
    CHECK(same);
    // no memories: what was gained; in place: the output is the memories themselves
    lut_add_reference(p, set.get(), n_set, count, depth, steps, sel.get(), amounts.get(), values.get(), nullptr, n_mems, mem_of.get(), zeros.get());
    same = true;
    for (size_t x = 0; x < n_mems * T * W; x++) same = same && (uint32_t)out[x] == (uint32_t)mems[x] + (uint32_t)zeros[x];
    CHECK(same);
    std::unique_ptr<Torus32[]> inplace(new Torus32[n_mems * T * W]);
    for (size_t x = 0; x < n_mems * T * W; x++) inplace[x] = mems[x];
    lut_add_reference(p, set.get(), n_set, count, depth, steps, sel.get(), amounts.get(), values.get(), inplace.get(), n_mems, mem_of.get(), inplace.get());
    same = true;
    for (size_t x = 0; x < n_mems * T * W; x++) same = same && inplace[x] == out[x];
    CHECK(same);
    // the defaults of the three optional arrays, and no items at all
    lut_add_reference(p, set.get(), n_set, count, depth, steps, nullptr, nullptr, values.get(), nullptr, n_mems, nullptr, zeros.get());
    lut_add_reference(p, set.get(), n_set, 0, depth, steps, nullptr, nullptr, nullptr, mems.get(), n_mems, nullptr, zeros.get());
    same = true;
    for (size_t x = 0; x < n_mems * T * W; x++) same = same && zeros[x] == mems[x];
    CHECK(same);
}

int main() {
    run(16, 3, 7, 3, 3, 2, 3, 2);
    run(16, 2, 16, 1, 2, 5, 3, 1);   // l x Bgbit = 32; steps beyond log2(2N): default amounts 0 from t = 5 on
    run(16, 1, 27, 2, 1, 0, 1, 1);   // steps 0: the values are the parents
    run(32, 32, 1, 2, 0, 2, 2, 3);   // depth 0: the rotated values summed into row 0 of their memories
    run(64, 6, 5, 5, 4, 3, 2, 2);
    run(64, 3, 7, 2, 0, 0, 3, 1);    // depth 0, steps 0: a plain sum
    run(16, 3, 7, 2, 1, 64, 1, 1);   // the most steps
    run(1024, 3, 7, 2, 1, 1, 2, 1);
    if (failures) return 1;
    printf("LUT_ADD_REFERENCE_OK\n");
    return 0;
}
