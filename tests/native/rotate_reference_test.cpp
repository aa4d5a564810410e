// tlwe_rotate_reference and lut_read_reference (csrc/tfhe_host.h -- what ieache_tlwe_rotate_reference / ieache_lut_read_reference
// of include/ieache.h section 4 call) as a stand-alone program for AddressSanitizer + UBSan: buffers of exactly the documented
// size (heap-allocated, so a word past either end is seen), a 2-step rotation against a schoolbook product written out here,
// both defaults, the boundary amounts, in place, and the lookup with and without its key switch against its stages.
// Built by tests/test_rotate_cpu.py together with csrc/tfhe_host.cpp.
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

// acc + C [.] (X^a acc - acc), schoolbook: the monomial shift, the digits and the negacyclic products spelt out
static std::vector<uint32_t> step(const Params& p, const Torus32* C, const std::vector<uint32_t>& acc, int32_t a) {
    const int32_t N = p.N, l = p.l, Bgbit = p.Bgbit;
    std::vector<uint32_t> d(2 * (size_t)N), out(acc);
    for (int32_t c = 0; c < 2; c++)
        for (int32_t j = 0; j < N; j++) {
            int32_t from = j - a;
            while (from < 0) from += 2 * N;
            const uint32_t v = acc[(size_t)c * N + from % N];
            d[(size_t)c * N + j] = (from >= N ? 0u - v : v) - acc[(size_t)c * N + j];
        }
    uint32_t offset = 0;
    for (int32_t q = 1; q <= l; q++) offset += (1u << (Bgbit - 1)) << (32 - q * Bgbit);
    const uint32_t mask = Bgbit >= 32 ? 0xFFFFFFFFu : (1u << Bgbit) - 1u;
    for (int32_t c = 0; c < 2; c++)
        for (int32_t q = 1; q <= l; q++)
            for (int32_t o = 0; o < 2; o++) {
                const uint32_t* key = (const uint32_t*)C + (((size_t)c * l + (q - 1)) * 2 + o) * N;
                for (int32_t i = 0; i < N; i++) {
                    const uint32_t e = (((d[(size_t)c * N + i] + offset) >> (32 - q * Bgbit)) & mask) - (1u << (Bgbit - 1));
                    for (int32_t j = 0; j < N; j++) {
                        const int32_t at = i + j;
                        if (at < N)
                            out[(size_t)o * N + at] += e * key[j];
                        else
                            out[(size_t)o * N + at - N] -= e * key[j];
                    }
                }
            }
    return out;
}

static void run(int32_t N, int32_t l, int32_t Bgbit, size_t n_set, int32_t steps, size_t count, const std::vector<int32_t>& amounts) {
    Params p;
    p.n = 4;
    p.N = N;
    p.l = l;
    p.Bgbit = Bgbit;
    CHECK(p.supported());
    CHECK(amounts.empty() || amounts.size() == (size_t)steps);
    Rng rng((uint64_t)(299 + N + 10 * l + Bgbit + steps));
    const size_t W = 2 * (size_t)N, S = (size_t)p.kpl() * W, D = (size_t)(steps ? steps : 1);
    std::unique_ptr<Torus32[]> set(new Torus32[n_set * S]), in(new Torus32[count * W]), out(new Torus32[count * W]);
    for (size_t i = 0; i < n_set * S; i++) set[i] = rng.uniform_torus32();
    set[0] = INT32_MIN;
    set[n_set * S - 1] = INT32_MAX;
    for (size_t i = 0; i < count * W; i++) in[i] = rng.uniform_torus32();
    std::unique_ptr<int32_t[]> sel(new int32_t[count * D]);
    for (size_t i = 0; i < count * D; i++) sel[i] = (int32_t)(rng.next() % n_set);
    sel[count * D - 1] = (int32_t)n_set - 1;
    std::unique_ptr<int32_t[]> am(new int32_t[D]);
    for (size_t t = 0; t < (size_t)steps; t++) am[t] = amounts.empty() ? (((size_t)1 << t) < W ? (int32_t)(W - ((size_t)1 << t)) : 0) : amounts[t];

    tlwe_rotate_reference(p, set.get(), n_set, count, steps, sel.get(), amounts.empty() ? nullptr : am.get(), in.get(), out.get());
    for (size_t r = 0; r < count; r++) {
        std::vector<uint32_t> acc(in.get() + r * W, in.get() + (r + 1) * W);
        for (int32_t t = 0; t < steps; t++) acc = step(p, set.get() + (size_t)sel[r * D + (size_t)t] * S, acc, am[t]);
        bool same = true;
        for (size_t x = 0; x < W; x++) same = same && acc[x] == (uint32_t)out[r * W + x];
        CHECK(same);
    }
    // in place, and the default of the index array (sample (r steps + t) mod n_set)
    std::unique_ptr<Torus32[]> inplace(new Torus32[count * W]);
    for (size_t x = 0; x < count * W; x++) inplace[x] = in[x];
    tlwe_rotate_reference(p, set.get(), n_set, count, steps, sel.get(), amounts.empty() ? nullptr : am.get(), inplace.get(), inplace.get());
    bool same = true;
    for (size_t x = 0; x < count * W; x++) same = same && inplace[x] == out[x];
    CHECK(same);
    tlwe_rotate_reference(p, set.get(), n_set, count, steps, nullptr, nullptr, in.get(), out.get());
    if (steps > 0) {
        std::vector<uint32_t> acc(in.get() + (count - 1) * W, in.get() + count * W);
        for (int32_t t = 0; t < steps; t++)
            acc = step(p, set.get() + (((count - 1) * (size_t)steps + (size_t)t) % n_set) * S, acc, ((size_t)1 << t) < W ? (int32_t)(W - ((size_t)1 << t)) : 0);
        same = true;
        for (size_t x = 0; x < W; x++) same = same && acc[x] == (uint32_t)out[(count - 1) * W + x];
        CHECK(same);
    }
}

// the lookup equals its stages: tree by the high selectors, rotation by the low ones, extraction, key switch
static void read(int32_t N, int32_t depth, int32_t steps, size_t count, int32_t coef) {
    Params p;
    p.n = 5;
    p.N = N;
    CHECK(p.supported());
    Rng rng((uint64_t)(399 + N + depth + 7 * steps));
    const size_t W = 2 * (size_t)N, n_set = 3, S = (size_t)p.kpl() * W, T = (size_t)1 << depth, A = (size_t)(depth + steps), n_tables = 2;
    std::unique_ptr<Torus32[]> set(new Torus32[n_set * S]), tables(new Torus32[n_tables * T * W]), ksk(new Torus32[p.ksk_count()]);
    for (size_t i = 0; i < n_set * S; i++) set[i] = rng.uniform_torus32();
    for (size_t i = 0; i < n_tables * T * W; i++) tables[i] = rng.uniform_torus32();
    for (size_t i = 0; i < p.ksk_count(); i++) ksk[i] = rng.uniform_torus32();
    std::unique_ptr<int32_t[]> sel(new int32_t[count * (A ? A : 1)]), tof(new int32_t[count]);
    for (size_t i = 0; i < count * A; i++) sel[i] = (int32_t)(rng.next() % n_set);
    for (size_t i = 0; i < count; i++) tof[i] = (int32_t)(i % n_tables);
    std::unique_ptr<Torus32[]> u(new Torus32[count * ((size_t)N + 1)]), out(new Torus32[count * ((size_t)p.n + 1)]);
    lut_read_reference(p, set.get(), n_set, nullptr, count, depth, steps, sel.get(), nullptr, tables.get(), tof.get(), coef, u.get());
    lut_read_reference(p, set.get(), n_set, ksk.get(), count, depth, steps, sel.get(), nullptr, tables.get(), tof.get(), coef, out.get());
    // by hand
    std::vector<int32_t> tree_sel(count * (size_t)(depth ? depth : 1)), rot_sel(count * (size_t)(steps ? steps : 1)), coefs(count, coef);
    for (size_t i = 0; i < count; i++) {
        for (int32_t t = 0; t < steps; t++) rot_sel[i * (size_t)steps + (size_t)t] = sel[i * A + (size_t)t];
        for (int32_t k = 0; k < depth; k++) tree_sel[i * (size_t)depth + (size_t)k] = sel[i * A + (size_t)steps + (size_t)k];
    }
    std::unique_ptr<Torus32[]> rows(new Torus32[count * W]), u2(new Torus32[count * ((size_t)N + 1)]), out2(new Torus32[count * ((size_t)p.n + 1)]);
    lut_tree_reference(p, set.get(), n_set, count, depth, tree_sel.data(), tables.get(), tof.get(), rows.get());
    tlwe_rotate_reference(p, set.get(), n_set, count, steps, rot_sel.data(), nullptr, rows.get(), rows.get());
    tlwe_extract_reference(p, count, rows.get(), coefs.data(), u2.get());
    keyswitch_reference(p, ksk.get(), count, u2.get(), out2.get());
    bool same = true;
    for (size_t x = 0; x < count * ((size_t)N + 1); x++) same = same && u[x] == u2[x];
    CHECK(same);
    same = true;
    for (size_t x = 0; x < count * ((size_t)p.n + 1); x++) same = same && out[x] == out2[x];
    CHECK(same);
    // implied selectors run too
    lut_read_reference(p, set.get(), n_set, ksk.get(), count, depth, steps, nullptr, nullptr, tables.get(), nullptr, coef, out.get());
}

int main() {
    run(64, 3, 7, 3, 2, 2, {5, 127});           // the 2-step rotation against the schoolbook product
    run(64, 2, 10, 1, 2, 3, {});                // default amounts 2N - 1, 2N - 2
    run(64, 3, 7, 2, 6, 1, {0, 1, 63, 64, 65, 127});  // every boundary of the 2N-ring, and a no-op step
    run(64, 3, 7, 4, 9, 2, {});                 // more steps than log2(2N): the default amounts end in zeros
    run(16, 2, 16, 2, 3, 2, {});                // l x Bgbit = 32: the last digit's shift is 0
    run(32, 32, 1, 2, 1, 2, {33});              // Bgbit = 1
    run(64, 3, 7, 2, 0, 3, {});                 // steps 0: a copy
    run(1024, 3, 7, 2, 1, 1, {1025});
    read(64, 2, 3, 3, 0);
    read(64, 0, 2, 2, 5);
    read(64, 1, 0, 2, 63);
    if (failures) return 1;
    printf("ROTATE_REFERENCE_OK\n");
    return 0;
}
