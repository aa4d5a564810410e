// Stand-alone host test (built with -fsanitize=address,undefined by tests/test_ring2048_cpu.py) of what csrc/params.h,
// csrc/br_plan.h and csrc/ks_plan.h say about rings of degree 2048: the gate, the LDS the any-parameter kernels ask for there,
// and which of those needs a context refuses at creation.
#include <cstdio>

#include "br_plan.h"
#include "ks_plan.h"
#include "pack_plan.h"

using namespace ieache;

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);     \
            return 1;                                                 \
        }                                                             \
    } while (0)

static Params at(int32_t n, int32_t N, int32_t l, int32_t Bgbit, int32_t t = 8, int32_t bb = 2) {
    Params p;
    p.n = n, p.N = N, p.l = l, p.Bgbit = Bgbit, p.ks_t = t, p.ks_basebit = bb;
    return p;
}

int main() {
    // the gate: 2048 in, nothing above, no other ring size, br_exact() as it was (2l x 2048 x 2^Bgbit <= 2^32: Bgbit <= 20 at l = 1)
    CHECK(at(630, 2048, 3, 7).supported() && at(4, 2048, 2, 10).supported() && at(4, 2048, 4, 6).supported() && at(4, 2048, 8, 4).supported());
    CHECK(!at(4, 4096, 2, 10).supported() && !at(4, 4096, 3, 7).supported() && !at(4, 1000, 3, 7).supported() && !at(4, 3072, 3, 7).supported());
    CHECK(at(5, 2048, 1, 20).supported() && at(5, 2048, 1, 20).br_exact() && !at(5, 2048, 1, 21).supported() && !at(5, 2048, 1, 21).br_exact());
    CHECK(at(5, 2048, 2, 16).supported() && !at(5, 2048, 3, 11).supported() && !at(5, 2048, 1, 32).supported());
    // none of them is a set of the N = 1024 kernels
    CHECK(!br_supported(at(630, 2048, 3, 7)) && !br_one_limb_supported(at(630, 2048, 3, 7)));
    // k_blind_rotate_generic: 2l rows of 16 KiB, the accumulator's 16 KiB, the rotation amounts: l <= 4 fits a CU, l = 5 does not
    CHECK(br_generic_lds_bytes(at(630, 2048, 3, 7)) == (size_t)6 * 16384 + 16384 + 1264);
    CHECK(br_generic_lds_bytes(at(630, 2048, 4, 6)) == (size_t)144 * 1024 + 1264 && br_generic_lds_bytes(at(630, 2048, 4, 6)) <= kBrLdsMax);
    CHECK(br_generic_lds_bytes(at(4, 2048, 1, 20)) == (size_t)4 * 16384 + 16384 + 16);  // l = 1: four rows, the outputs
    CHECK(at(3, 2048, 5, 6).supported() && br_generic_lds_bytes(at(3, 2048, 5, 6)) > kBrLdsMax);
    CHECK(at(3, 2048, 8, 4).supported() && br_generic_lds_bytes(at(3, 2048, 8, 4)) > kBrLdsMax);
    CHECK(br_generic_lds_bytes(at(630, 1024, 3, 7)) == (size_t)6 * 8192 + 8192 + 1264);  // N = 1024: as it was
    // the key switch's digit list, N x t words: t = 8 and t = 16 fit, t = 31 (supported: 31 x 1 < 32) does not -- reachable now
    CHECK(ks_support(at(4, 2048, 3, 7, 8, 2)).generic_lds == 8208 + 65536 && ks_support(at(4, 2048, 3, 7, 16, 1)).generic_lds == 8208 + 131072);
    CHECK(ks_support(at(4, 2048, 3, 7, 18, 1)).generic_lds <= kKsLdsMax && ks_support(at(4, 2048, 3, 7, 19, 1)).generic_lds > kKsLdsMax);
    CHECK(at(4, 2048, 3, 7, 31, 1).supported() && ks_support(at(4, 2048, 3, 7, 31, 1)).generic_lds == 8208 + 253952);
    // libtfhe's decomposition on the larger ring: every family, the per-gate walk with its 8 partial rows
    {
        const KsSupport s = ks_support(at(630, 2048, 3, 7));
        CHECK(s.nld == 3 && s.batch && s.sliced && s.mfma && s.vec_lds <= kKsLdsMax && s.batch_lds == 65536 + 64);
        for (int32_t k : {1, 2, 4, 8}) CHECK(ks_mfma_split_ok(at(630, 2048, 3, 7), k));
    }
    // br_plan names k_blind_rotate_h2 for every N = 2048 set of at most 16 digit rows, whatever the launch size, in slices of
    // 1 .. 64 steps; "force_generic" and longer gadgets take the any-parameter kernel; no variant number, no rotation of roles
    {
        EvalOptions o;
        o.cus = 256;
        const Params p = at(630, 2048, 3, 7);
        CHECK(br_h2_supported(p) && br_h2_supported(at(4, 2048, 8, 4)) && !br_h2_supported(at(4, 2048, 16, 2)) && !br_h2_supported(at(4, 1024, 3, 7)));
        for (int64_t cnt : {1, 64, 1024, 100000}) {
            const BrPlan pl = br_plan(p, o, BrCall{}, false, cnt);
            CHECK(!pl.generic && pl.h2 && pl.slice == (int32_t)o.br_slice_default && pl.mix.k == 0);
            CHECK(br_kernel_label(p, pl) == "k_blind_rotate_h2<3,7>");
        }
        o.br_slice = 5;
        CHECK(br_plan(p, o, BrCall{}, false, 9).slice == 5);
        o.br_slice = 64;
        CHECK(br_plan(p, o, BrCall{}, false, 9).slice == 64);
        o.br_slice = 65;  // one amount per lane: longer slices fall back to the default
        CHECK(br_plan(p, o, BrCall{}, false, 9).slice == (int32_t)o.br_slice_default);
        o.force_generic = 1;
        CHECK(br_plan(p, o, BrCall{}, false, 9).generic && !br_plan(p, o, BrCall{}, false, 9).h2);
        CHECK(br_kernel_label(p, br_plan(p, o, BrCall{}, false, 9)) == "k_blind_rotate_generic");
        o.force_generic = 0;
        CHECK(br_plan(at(4, 2048, 16, 2), o, BrCall{}, false, 9).generic);
        CHECK(br_plan(at(4, 1024, 4, 8), o, BrCall{}, false, 9).generic && !br_plan(at(4, 1024, 4, 8), o, BrCall{}, false, 9).h2);
        // the state a gate instance parks between slices: 16 KiB of accumulator on this ring, 8 KiB at N = 1024 as before
        CHECK(br_state_bytes_per_item(p) == 1264 + 16384 && br_state_bytes_per_item(at(630, 1024, 3, 7)) == 1264 + 8192);
    }
    // the packing key switch stays on rings up to 1024 (and with it the projection and unpack)
    CHECK(pack_set_error(at(5, 2048, 3, 7), 8, 2) && !pack_set_error(at(5, 1024, 3, 7), 8, 2));
    printf("RING2048_PLAN_OK\n");
    return 0;
}
