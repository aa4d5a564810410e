// Which key-switch kernel takes a launch, and cut how (ie-ache_amd/csrc/ks_plan.h), as plain host C++ under
// AddressSanitizer / UBSan.  The expected plans were derived by hand from the ladder, the sliced walk's choice of gates per
// workgroup and the product's K-split cost model as they stood before the header existed; the five K splits at the default
// options are the measured ones (profiles/r3_keyswitch_mfma.txt).
// Built and run by tests/test_ks_plan_cpu.py.
#include <cstdio>
#include <initializer_list>

#include "../../ie-ache_amd/csrc/ks_plan.h"

using namespace ieache;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                   \
        }                                                               \
    } while (0)

constexpr int64_t H = (int64_t)1 << 40;  // "never", as the GPU tests set it

static EvalOptions defaults() {
    EvalOptions o;
    o.cus = 256;
    return o;
}

struct Row {
    EvalOptions o;
    bool limbs, force_generic;
};

// every option row of the table below (the sweep runs under each)
static int option_rows(Row* rows) {
    int n = 0;
    rows[n++] = {defaults(), true, false};
    rows[n] = {defaults(), true, false};
    rows[n++].o.ks_mfma_split = 16;
    rows[n] = {defaults(), true, false};
    rows[n++].o.ks_split_max = 1;
    rows[n] = {defaults(), true, false};
    rows[n++].o.ks_mfma_min = H;
    rows[n] = {defaults(), true, false};
    rows[n].o.ks_mfma_min = H, rows[n].o.ks_sliced_min = 1, rows[n].o.ks_gates = 16, rows[n].o.ks_slice = 3;
    n++;
    rows[n] = {defaults(), true, false};
    rows[n].o.ks_mfma_min = H, rows[n].o.ks_sliced_min = H;
    n++;
    rows[n++] = {defaults(), false, false};
    rows[n++] = {defaults(), true, true};
    return n;
}

static int check_product_parameters() {
    const Params p;  // n = 630, N = 1024, t = 8, basebit = 2
    const KsSupport s = ks_support(p);
    CHECK(p.lwe_stride() == 632 && s.nld == 3 && s.batch && s.sliced && s.mfma && ks_coef_blocks(p) == 20);
    CHECK(s.generic_lds == (size_t)(1024 + 4) * 4 + (size_t)1024 * 8 * 4 && s.vec_lds == s.generic_lds + (size_t)8 * 632 * 4);
    CHECK(s.batch_lds == (size_t)16 * 1024 * 2 + 64);
    Row rows[8];
    CHECK(option_rows(rows) == 8);
    auto plan = [&](const Row& r, int64_t cnt) { return ks_plan(s, p, r.o, r.limbs, r.force_generic, cnt); };
    auto per_gate = [&](const Row& r, int64_t cnt, int32_t splits) {
        const KsPlan pl = plan(r, cnt);
        return pl.family == KsFamily::PerGate && pl.splits == splits;
    };
    auto mfma = [&](const Row& r, int64_t cnt, int32_t ksplit) {
        const KsPlan pl = plan(r, cnt);
        return pl.family == KsFamily::Mfma && pl.ksplit == ksplit && pl.xcd_map == 0;
    };
    auto sliced = [&](const Row& r, int64_t cnt, int32_t g, int32_t slice) {
        const KsPlan pl = plan(r, cnt);
        return pl.family == KsFamily::Sliced && pl.gates_per_wg == g && pl.slice == slice;
    };
    // no option set
    const Row& none = rows[0];
    CHECK(per_gate(none, 1, 16) && per_gate(none, 24, 16));
    CHECK(per_gate(none, 25, 8) && per_gate(none, 48, 8));
    CHECK(per_gate(none, 49, 4) && per_gate(none, 63, 4));
    CHECK(mfma(none, 64, 8) && mfma(none, 512, 8));
    CHECK(mfma(none, 1024, 4));
    CHECK(mfma(none, 2304, 2));
    CHECK(mfma(none, 8192, 4));
    CHECK(mfma(none, 16384, 2));
    // ks_mfma_split = 16
    CHECK(mfma(rows[1], 8192, 16));
    // ks_split_max = 1
    CHECK(per_gate(rows[2], 5, 1));
    // ks_mfma_min = H
    const Row& no_mfma = rows[3];
    CHECK(per_gate(no_mfma, 96, 4) && per_gate(no_mfma, 97, 2) && per_gate(no_mfma, 192, 2) && per_gate(no_mfma, 193, 1) && per_gate(no_mfma, 575, 1));
    CHECK(sliced(no_mfma, 576, 4, 1024) && sliced(no_mfma, 1535, 4, 1024));  // the whole walk, one launch
    CHECK(sliced(no_mfma, 1536, 8, 1024) && sliced(no_mfma, 5120, 16, 1024) && sliced(no_mfma, 14336, 32, 1024));
    // ... ks_sliced_min = 1, ks_gates = 16, ks_slice = 3
    CHECK(sliced(rows[4], 5, 16, 3));
    // ks_mfma_min = ks_sliced_min = H
    CHECK(per_gate(rows[5], 4095, 1) && plan(rows[5], 4096).family == KsFamily::Batched);
    // limbs absent
    CHECK(sliced(rows[6], 8192, 16, 1024));
    // force_generic
    for (int64_t cnt : {1, 64, 8192}) {
        const KsPlan pl = plan(rows[7], cnt);
        CHECK(pl.family == KsFamily::Generic && pl.splits == 1);
    }
    // "ks_xcd" reaches the product through the plan
    Row xcd = none;
    xcd.o.ks_xcd = 1;
    CHECK(plan(xcd, 8192).family == KsFamily::Mfma && plan(xcd, 8192).xcd_map == 1 && plan(xcd, 8192).ksplit == 4);
    // the reserve path asks for digit scratch exactly when the plan is Mfma, and then for the product's
    for (const Row& r : rows)
        for (int64_t cnt = 1; cnt <= 20000; cnt++) {
            const size_t bytes = ks_scratch_bytes(s, p, r.o, r.limbs, r.force_generic, cnt);
            const bool is_mfma = plan(r, cnt).family == KsFamily::Mfma;
            CHECK((bytes != 0) == is_mfma);
            if (is_mfma) CHECK(bytes == ks_digit_scratch_bytes(p, cnt));
        }
    // 512 gate instances per workgroup of the product: the digits of N / 4 groups and one row address per padded gate instance
    CHECK(ks_digit_scratch_bytes(p, 1) == (size_t)256 * 512 * 8 + (size_t)512 * sizeof(Torus32*));
    CHECK(ks_digit_scratch_bytes(p, 512) == ks_digit_scratch_bytes(p, 1) && ks_digit_scratch_bytes(p, 513) == 2 * ks_digit_scratch_bytes(p, 1));
    CHECK(ks_limb_matrix_bytes(p) == (size_t)1024 * 20 * 4096);
    return 0;
}

static int check_support_and_splits() {
    Params p;
    p.n = 5, p.N = 64;
    KsSupport s = ks_support(p);
    CHECK(s.nld == 1 && s.batch && s.sliced && s.mfma);
    for (int32_t k : {1, 2, 4, 8}) CHECK(ks_mfma_split_ok(p, k));
    CHECK(!ks_mfma_split_ok(p, 16) && !ks_mfma_split_ok(p, 3) && !ks_mfma_split_ok(p, 0));
    p.N = 1024;
    CHECK(ks_mfma_split_ok(p, 64) && ks_mfma_split_ok(p, 128) && !ks_mfma_split_ok(p, 256));
    // base 2: only the per-gate walk
    Params b;
    b.ks_basebit = 1;
    s = ks_support(b);
    CHECK(s.nld == 3 && !s.batch && !s.sliced && !s.mfma);
    for (int64_t cnt : {1, 64, 576, 4096, 8192}) CHECK(ks_plan(s, b, defaults(), true, false, cnt).family == KsFamily::PerGate);
    Params q;
    q.N = 32;
    CHECK(!ks_support(q).mfma);
    return 0;
}

// The boundaries of ks_support / ks_plan over the sets a key header may carry (tests/test_param_lattice_gpu.py runs the
// kernels at them and relies on these answers for which family ran), and of Params::supported() itself.
static int check_parameter_lattice() {
    auto at = [](int32_t n, int32_t N, int32_t t, int32_t basebit) {
        Params p;
        p.n = n, p.N = N, p.ks_t = t, p.ks_basebit = basebit;
        return p;
    };
    EvalOptions never = defaults();  // neither the product nor a gate-batched walk
    never.ks_mfma_min = never.ks_sliced_min = never.ks_batch_min = H;
    auto family = [](const Params& p, const EvalOptions& o, bool force_generic, int64_t cnt) {
        return ks_plan(ks_support(p), p, o, true, force_generic, cnt).family;
    };
    // dwordx4 loads per key row: n = 255 -> 1, 256 -> 2, 508 .. 511 -> 2, 512 -> 3, 1023 -> 4, 1024 -> none
    struct { int32_t n, stride, nld; } rows[] = {{3, 4, 1},     {7, 8, 1},     {31, 32, 1},    {63, 64, 1},   {255, 256, 1}, {256, 260, 2},
                                                 {508, 512, 2}, {511, 512, 2}, {512, 516, 3},  {767, 768, 3}, {768, 772, 4},
                                                 {1023, 1024, 4}, {1024, 1028, 0}, {1100, 1104, 0}};
    for (const auto& r : rows) {
        const Params p = at(r.n, 64, 8, 2);
        const KsSupport s = ks_support(p);
        CHECK(p.supported() && p.lwe_stride() == r.stride && s.nld == r.nld);
        CHECK(s.mfma && s.batch == (r.nld > 0) && s.sliced == (r.nld > 0));
        CHECK(ks_coef_blocks(p) == (r.stride + 31) / 32);
        for (int64_t cnt : {1, 5, 70}) {
            CHECK(family(p, never, true, cnt) == KsFamily::Generic);
            CHECK(family(p, never, false, cnt) == (r.nld ? KsFamily::PerGate : KsFamily::Generic));
            EvalOptions o = never;
            o.ks_mfma_min = 1;
            CHECK(family(p, o, false, cnt) == KsFamily::Mfma);  // also past n = 1023: the product has no column limit
            o = never, o.ks_sliced_min = 1;
            CHECK(family(p, o, false, cnt) == (r.nld ? KsFamily::Sliced : KsFamily::Generic));
            o = never, o.ks_batch_min = 1;
            CHECK(family(p, o, false, cnt) == (r.nld ? KsFamily::Batched : KsFamily::Generic));
            // no option set: the product from 64 gate instances, below it the per-gate walk or, past n = 1023, the generic kernel
            CHECK(family(p, defaults(), false, cnt) == (cnt >= 64 ? KsFamily::Mfma : r.nld ? KsFamily::PerGate : KsFamily::Generic));
        }
    }
    // the per-gate walk cut into workgroups: 1 and 16 at five gates of a 64-coefficient ring
    {
        const Params p = at(255, 64, 8, 2);
        EvalOptions o = never;
        o.ks_split_max = 1;
        CHECK(ks_plan(ks_support(p), p, o, true, false, 5).splits == 1);
        o.ks_split_max = 16;
        CHECK(ks_plan(ks_support(p), p, o, true, false, 5).splits == 16 && ks_plan(ks_support(p), p, o, true, false, 70).splits == 4);
    }
    // the decomposition: t = 4 at basebit 2 is gate-batched only; basebit 1, 3, 4 and t x basebit > 16 are per-gate / generic only
    struct { int32_t t, basebit; bool batch, sliced, mfma; } dec[] = {{8, 2, true, true, true},     {4, 2, true, false, false},
                                                                      {16, 1, false, false, false}, {31, 1, false, false, false},
                                                                      {5, 3, false, false, false},  {10, 3, false, false, false},
                                                                      {7, 4, false, false, false},  {1, 4, false, false, false}};
    for (const auto& d : dec)
        for (int32_t n : {7, 256}) {
            const Params p = at(n, 64, d.t, d.basebit);
            const KsSupport s = ks_support(p);
            CHECK(p.supported() && s.nld == (n == 7 ? 1 : 2) && s.batch == d.batch && s.sliced == d.sliced && s.mfma == d.mfma);
            EvalOptions o = defaults();
            o.ks_batch_min = 1;
            for (int64_t cnt : {1, 5, 70}) {
                CHECK(family(p, o, true, cnt) == KsFamily::Generic);
                CHECK(family(p, never, false, cnt) == KsFamily::PerGate);
                if (!d.mfma) CHECK(family(p, o, false, cnt) == (d.batch ? KsFamily::Batched : KsFamily::PerGate));
            }
        }
    // t = 31 on the largest ring: 131 088 bytes of list for the generic kernel, 256 more for the per-gate walk -- both inside a CU's
    // LDS, as is every other set supported() admits (t <= 31, N <= 1024), so KeySwitch::init's refusal is never reached from a key header
    {
        const Params p = at(4, 1024, 31, 1);
        const KsSupport s = ks_support(p);
        CHECK(p.supported() && s.generic_lds == 131088 && s.vec_lds == 131088 + 256 && s.nld == 1 && s.vec_lds <= kKsLdsMax);
        CHECK(!at(4, 1024, 32, 1).supported() && !at(4, 1024, 16, 2).supported() && !at(4, 64, 2, 5).supported());
        Params wide = at(4, 1024, 40, 1);  // what the refusal is there for, should supported() ever widen
        CHECK(!wide.supported() && ks_support(wide).generic_lds > kKsLdsMax);
    }
    // Params::br_exact(): kpl x N x 2^Bgbit <= 2^32 (tests/test_rounding_model_cpu.py), which only l = 1 reaches
    auto br = [](int32_t l, int32_t Bgbit, int32_t N) {
        Params p;
        p.n = 5, p.N = N, p.l = l, p.Bgbit = Bgbit;
        return p.supported();
    };
    for (int32_t logN = 4; logN <= 10; logN++) CHECK(br(1, 31 - logN, 1 << logN) && !br(1, 32 - logN, 1 << logN));
    CHECK(!br(1, 32, 16) && !br(1, 32, 1024) && !br(3, 11, 64) && !br(1, 0, 64));
    CHECK(br(3, 7, 1024) && br(2, 10, 1024) && br(2, 16, 1024) && br(4, 8, 1024) && br(32, 1, 1024) && br(16, 2, 512) && br(10, 3, 1024));
    return 0;
}

int main() {
    if (check_product_parameters() || check_support_and_splits() || check_parameter_lattice()) return 1;
    printf("KS_PLAN_OK\n");
    return 0;
}
