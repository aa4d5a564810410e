// The two TLWE host tools (csrc/tfhe_host.h: tlwe_encrypt, tlwe_phase -- what ieache_tlwe_encrypt / ieache_tlwe_phase call) as a
// stand-alone program for AddressSanitizer + UBSan: count = 0 on null buffers, N = 16 and N = 1024, output buffers of exactly
// the documented size (heap-allocated, so a word past either end is seen), a schoolbook phase as the second opinion, and the
// key generation's own rows (the routine is shared) decrypting to the gadget.
// Built by tests/test_pbs_tlwe_cpu.py together with csrc/tfhe_host.cpp.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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

// B - A s by the definition: coefficient j of A s is sum_i s_i A_{j-i}, negated where the index wraps
static std::vector<uint32_t> schoolbook_phase(int32_t N, const int32_t* key, const Torus32* sample) {
    std::vector<uint32_t> ph(N);
    for (int32_t j = 0; j < N; j++) {
        uint32_t as = 0;
        for (int32_t i = 0; i < N; i++) {
            if (!key[i]) continue;
            const int32_t q = j - i;
            as += q >= 0 ? (uint32_t)sample[q] : 0u - (uint32_t)sample[q + N];
        }
        ph[j] = (uint32_t)sample[N + j] - as;
    }
    return ph;
}

static void run(int32_t N, size_t count, double alpha, bool exact) {
    Params p;
    p.N = N;
    Rng rng((uint64_t)(1000 + N));
    std::unique_ptr<int32_t[]> key(new int32_t[N]);
    for (int32_t i = 0; i < N; i++) key[i] = rng.bit();
    std::unique_ptr<Torus32[]> polys(new Torus32[count * N]), out(new Torus32[count * 2 * N]), phase(new Torus32[count * N]);
    for (size_t i = 0; i < count * N; i++) polys[i] = rng.uniform_torus32();
    polys[0] = INT32_MIN;
    polys[1] = INT32_MAX;
    tlwe_encrypt(p, key.get(), polys.get(), count, alpha, rng, out.get());
    tlwe_phase(p, key.get(), out.get(), count, phase.get());
    const double bound = 6.0 * alpha * 4294967296.0;
    bool mask_nonzero = false;
    for (size_t c = 0; c < count; c++) {
        const std::vector<uint32_t> want = schoolbook_phase(N, key.get(), out.get() + c * 2 * N);
        for (int32_t j = 0; j < N; j++) {
            CHECK(want[j] == (uint32_t)phase[c * N + j]);
            const int32_t err = (int32_t)((uint32_t)phase[c * N + j] - (uint32_t)polys[c * N + j]);
            CHECK(exact ? err == 0 : std::fabs((double)err) < bound);
            mask_nonzero = mask_nonzero || out[c * 2 * N + j] != 0;
        }
    }
    CHECK(mask_nonzero);
}

int main() {
    // count = 0: nothing is read or written, null buffers included
    {
        Params p;
        p.N = 16;
        Rng rng((uint64_t)1);
        int32_t key[16] = {0};
        tlwe_encrypt(p, key, nullptr, 0, p.tlwe_alpha_min, rng, nullptr);
        tlwe_phase(p, key, nullptr, 0, nullptr);
    }
    run(16, 5, 0x1p-25, false);
    run(16, 3, 1e-30, true);  // a noise that rounds to 0 on the torus: the round trip is exact
    run(1024, 2, 0x1p-25, false);
    run(1024, 1, 1e-30, true);
    // a row of the bootstrapping key comes from the same routine: rows bloc * l + q of BK_i decrypt to s_i 2^(32-(q+1)Bgbit)
    // on the constant coefficient of polynomial bloc and to noise everywhere else
    {
        Params p;
        p.n = 3;
        p.N = 16;
        const uint32_t seed[2] = {7, 8};
        SecretKeyData sk;
        keygen(p, seed, 2, &sk, true);
        const int32_t N = p.N, kpl = p.kpl();
        std::vector<Torus32> ph((size_t)p.n * kpl * N);
        tlwe_phase(p, sk.tlwe_key.data(), sk.cloud.bk.data(), (size_t)p.n * kpl, ph.data());
        const double bound = 6.0 * p.tlwe_alpha_min * 4294967296.0;
        for (int32_t i = 0; i < p.n; i++)
            for (int32_t row = 0; row < kpl; row++) {
                const int32_t bloc = row / p.l, q = row % p.l;
                const uint32_t h = (uint32_t)sk.lwe_key[i] << (32 - (q + 1) * p.Bgbit);
                for (int32_t j = 0; j < N; j++) {
                    // the gadget sits on polynomial `bloc` of the row: on B (bloc = 1) it is the message itself, on A (bloc = 0)
                    // it enters the phase as -h s, coefficient j carrying -h s_j
                    const uint32_t msg = bloc == 1 ? (j == 0 ? h : 0u) : 0u - h * (uint32_t)sk.tlwe_key[j];
                    const int32_t err = (int32_t)((uint32_t)ph[((size_t)i * kpl + row) * N + j] - msg);
                    CHECK(std::fabs((double)err) < bound);
                }
            }
    }
    if (failures) {
        printf("TLWE_TOOLS_FAILED %d\n", failures);
        return 1;
    }
    printf("TLWE_TOOLS_OK\n");
    return 0;
}
