// Which blind-rotation kernel takes a launch, with how many CMux steps per launch, how many gates per workgroup, and whether
// as a rotation of roles (ie-ache_amd/csrc/br_plan.h), as plain host C++ under AddressSanitizer / UBSan.  The expected plans
// are the table of what the evaluator and the launcher decided between them before the header existed: every boundary on
// both sides, at the defaults Evaluator::init() sets per CU.
// Built and run by tests/test_br_plan_cpu.py; `br_plan_test --builds` prints the (number, gates per workgroup) builds the
// variant table names, for the comparison with the launch rows of blind_rotate_w64.hip.
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../ie-ache_amd/csrc/br_plan.h"

using namespace ieache;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                   \
        }                                                               \
    } while (0)

// what Evaluator::init() sets for a device of `cus` compute units
static EvalOptions defaults(int64_t cus, bool exact_fft = false) {
    EvalOptions o;
    o.cus = cus;
    o.br_wide_max = cus;
    o.overlap_min = 16 * cus;
    o.pipe_min = 8 * cus;
    o.wg3_max = 6 * cus;
    o.resident_gates = 8 * cus;
    o.one_limb_min = cus + 1;
    o.four_wave_max = 2 * cus;
    o.two_wave_max = 5 * cus;
    o.exact_one_wave_min = 4 * cus + 1;
    o.exact_fft = exact_fft;
    return o;
}

static const Params P;  // n = 630, N = 1024, l = 3, Bgbit = 7

static BrPlan plan(const EvalOptions& o, int64_t cnt, const BrCall& c = BrCall{}) { return br_plan(P, o, c, true, cnt); }
// variant, slice, gates per workgroup; no rotation of roles
static bool is(const BrPlan& pl, int32_t variant, int32_t slice, int32_t wg) {
    return !pl.generic && pl.variant == variant && pl.slice == slice && pl.wg_gates == wg && pl.mix.k == 0;
}
// ... as the rotation of roles the defaults give: k 3, tw 2, s1 16, s2 32, 7 cycles, tail 13 / 27, 627 steps covered
static bool is_mixed(const BrPlan& pl, int32_t variant, int32_t slice, int32_t wg) {
    const MixSteps& m = pl.mix_steps;
    return !pl.generic && pl.variant == variant && pl.slice == slice && pl.wg_gates == wg && pl.mix.k == 3 && pl.mix.tw == 2 && m.s1 == 16 &&
           m.s2 == 32 && m.cycles == 7 && m.tail_s1 == 13 && m.tail_s2 == 27 && m.covered == 627 && !pl.mix_sync && pl.mix_wg == 2;
}

static int check_table() {
    CHECK(br_supported(P) && br_one_limb_supported(P) && br_bara_stride(P) == 632 && br_state_bytes_per_item(P) == 632 * 2 + 2 * 1024 * 4);
    const EvalOptions d = defaults(256);
    // by launch size, whole rotation on lane 0, concurrency 1
    CHECK(is(plan(d, 1), 38, 632, 3) && is(plan(d, 256), 38, 632, 3));
    CHECK(is(plan(d, 257), 43, 632, 3) && is(plan(d, 512), 43, 632, 3));
    CHECK(is(plan(d, 513), 36, 64, 3) && is(plan(d, 1024), 36, 64, 3));
    CHECK(is_mixed(plan(d, 1025), 36, 64, 3) && is_mixed(plan(d, 1280), 36, 64, 3));
    CHECK(is_mixed(plan(d, 1281), 31, 64, 3) && is_mixed(plan(d, 1536), 31, 64, 3));
    CHECK(is_mixed(plan(d, 1537), 31, 64, 4) && is_mixed(plan(d, 1792), 31, 64, 4));
    CHECK(is(plan(d, 1793), 31, 64, 4) && is(plan(d, 2048), 31, 64, 4));
    CHECK(is_mixed(plan(d, 2049), 31, 16, 4) && is_mixed(plan(d, 2688), 31, 16, 4));
    CHECK(is(plan(d, 2689), 31, 16, 4) && is(plan(d, 65536), 31, 16, 4));
    CHECK(plan(d, 300).w4r_flip == 256 && plan(d, 300).concurrency == 1);
    // "exact_fft" = 1, and equally the repeat of a call after a guard trip: the two-limb kernels, never a rotation of roles
    BrCall repeat;
    repeat.exact = true;
    for (int how = 0; how < 2; how++) {
        const EvalOptions o = how ? d : defaults(256, true);
        const BrCall c = how ? repeat : BrCall{};
        CHECK(is(plan(o, 1, c), 7, 632, 3) && is(plan(o, 256, c), 7, 632, 3));
        CHECK(is(plan(o, 257, c), 0, 16, 3) && is(plan(o, 1024, c), 0, 16, 3));
        CHECK(is(plan(o, 1025, c), 9, 64, 3) && is(plan(o, 1536, c), 9, 64, 3) && is(plan(o, 1537, c), 9, 64, 4) && is(plan(o, 2048, c), 9, 64, 4));
        CHECK(is(plan(o, 2049, c), 9, 16, 4) && is(plan(o, 65536, c), 9, 16, 4));
    }
    // two streams side by side: the choice is by 2 x cnt, and never a rotation of roles
    BrCall two;
    two.concurrency = 2;
    CHECK(is(plan(d, 128, two), 38, 632, 3) && is(plan(d, 129, two), 43, 632, 3) && is(plan(d, 256, two), 43, 632, 3));
    CHECK(is(plan(d, 257, two), 36, 64, 3) && is(plan(d, 640, two), 36, 64, 3) && is(plan(d, 641, two), 31, 64, 3));
    CHECK(is(plan(d, 768, two), 31, 64, 3) && is(plan(d, 769, two), 31, 64, 4) && is(plan(d, 1024, two), 31, 64, 4) && is(plan(d, 1025, two), 31, 16, 4));
    CHECK(plan(d, 1025, two).concurrency == 2);
    // what else rules the rotation of roles out
    BrCall halves, part, lane1;
    halves.level_on_two_lanes = true;
    part.whole_rotation = false;
    lane1.lane0 = false;
    for (const BrCall& c : {halves, part, lane1}) CHECK(is(plan(d, 1100, c), 36, 64, 3) && is(plan(d, 1400, c), 31, 64, 3) && is(plan(d, 2300, c), 31, 16, 4));
    EvalOptions o = d;
    o.overlap = 0;
    CHECK(is(plan(o, 1100), 36, 64, 3) && is(plan(o, 2300), 31, 16, 4));
    o = d;
    o.br_mix = 0;
    CHECK(is(plan(o, 1100), 36, 64, 3) && is(plan(o, 2300), 31, 16, 4));
    // a forced variant: no rotation of roles; with a repeat, the two-limb kernel of the launch's size
    o = d;
    o.br_variant = 31;
    CHECK(is(plan(o, 1100), 31, 16, 3) && is(plan(o, 1400), 31, 16, 3) && is(plan(o, 200), 31, 16, 3));
    CHECK(is(plan(o, 1024, repeat), 0, 16, 3) && is(plan(o, 1025, repeat), 9, 16, 3));
    o.br_variant = 7;
    CHECK(is(plan(o, 1100, repeat), 7, 16, 3));  // exact already: stays
    // "br_slice": taken where the kernel can, "br_slice_default" where it cannot; never over the 632 of the latency kernels
    o = d;
    o.br_slice = 630;
    CHECK(is(plan(o, 200), 38, 632, 3) && is(plan(o, 400), 43, 630, 3) && is(plan(o, 900), 36, 630, 3));
    CHECK(is(plan(o, 1900), 31, 16, 4) && is(plan(o, 4096), 31, 16, 4));
    CHECK(is(plan(defaults(256, true), 1900), 9, 64, 4));
    o.exact_fft = 1;
    CHECK(is(plan(o, 1900), 9, 16, 4) && is(plan(o, 900), 0, 16, 3));
    o = d;
    o.br_slice = 8;
    CHECK(is(plan(o, 200), 38, 632, 3) && is(plan(o, 400), 43, 8, 3) && is(plan(o, 900), 36, 8, 3) && is(plan(o, 4096), 31, 8, 4));
    o.br_slice = 64;
    CHECK(is(plan(o, 4096), 31, 64, 4));
    o.br_slice = 65;
    CHECK(is(plan(o, 4096), 31, 16, 4) && is(plan(o, 900), 36, 65, 3));
    o.br_slice = 633;
    CHECK(is(plan(o, 900), 36, 16, 3) && is(plan(o, 400), 43, 16, 3));
    // "br_slice_default" replaces the 16 only
    o = d;
    o.br_slice_default = 24;
    CHECK(is(plan(o, 200), 38, 632, 3) && is(plan(o, 900), 36, 64, 3) && is(plan(o, 1900), 31, 64, 4) && is(plan(o, 4096), 31, 24, 4));
    // "wg_gates" forces the workgroup size, for every variant; "w4r_flip" reaches the launcher through the plan
    o = d;
    o.wg_gates = 2;
    o.w4r_flip = 1 << 30;
    CHECK(is(plan(o, 200), 38, 632, 2) && is(plan(o, 4096), 31, 16, 2) && plan(o, 300).w4r_flip == 1 << 30);
    // every boundary moves with the CU count
    const EvalOptions e = defaults(304);
    CHECK(is(plan(e, 304), 38, 632, 3) && is(plan(e, 305), 43, 632, 3) && is(plan(e, 608), 43, 632, 3) && is(plan(e, 609), 36, 64, 3));
    CHECK(is(plan(e, 1216), 36, 64, 3) && is_mixed(plan(e, 1217), 36, 64, 3) && is_mixed(plan(e, 1520), 36, 64, 3) && is_mixed(plan(e, 1521), 31, 64, 3));
    CHECK(is_mixed(plan(e, 1824), 31, 64, 3) && is_mixed(plan(e, 1825), 31, 64, 4));
    CHECK(is_mixed(plan(e, 2128), 31, 64, 4) && is(plan(e, 2129), 31, 64, 4) && is(plan(e, 2432), 31, 64, 4) && is_mixed(plan(e, 2433), 31, 16, 4));
    CHECK(is_mixed(plan(e, 3192), 31, 16, 4) && is(plan(e, 3193), 31, 16, 4) && plan(e, 700).w4r_flip == 304);
    // a forced geometry; one that is none; turns too long for a round to fit
    o = d;
    o.mix_k = 2, o.mix_tw = 1;
    CHECK(plan(o, 1301).mix.k == 2 && plan(o, 1301).mix.tw == 1 && plan(o, 5000).mix.k == 2 && plan(o, 1024).mix.k == 0);
    o.mix_tw = 2;
    CHECK(plan(o, 1301).mix.k == 0);
    o = d;
    o.mix_s1 = 126;  // a round of 2 x 252 + 126 = 630 steps leaves the slice loop none
    CHECK(is(plan(o, 1100), 36, 64, 3) && br_kernel_label(P, plan(o, 1100)) == "k_blind_rotate_w2r+w1b<3,7> 2 of 3 subsets on two waves");  // the label names the geometry all the same
    o.mix_s1 = 125, o.mix_sync = 1, o.mix_wg = 4;
    CHECK(plan(o, 1100).mix.k == 3 && plan(o, 1100).mix_steps.cycles == 1 && plan(o, 1100).mix_steps.covered == 625 && plan(o, 1100).mix_sync && plan(o, 1100).mix_wg == 4);
    // a short LWE dimension (the test suites' keys): 64 exceeds the 8 amounts a rotation has, so "br_slice_default" it is, and
    // the launcher ends the one slice at the rotation's end
    Params small;
    small.n = 8;
    CHECK(br_bara_stride(small) == 8 && br_plan(small, d, BrCall{}, true, 900).slice == 16 && br_plan(small, d, BrCall{}, true, 200).slice == 8);
    CHECK(br_plan(small, d, BrCall{}, true, 1100).mix.k == 0 && br_plan(small, d, BrCall{}, true, 4096).slice == 16);
    CHECK(br_kernel_label(small, br_plan(small, d, BrCall{}, true, 2304)) == "k_blind_rotate_w2r+w1b<3,7> 2 of 3 subsets on two waves");
    // the any-parameter kernel
    CHECK(br_plan(P, d, BrCall{}, false, 1100).generic && br_kernel_label(P, br_plan(P, d, BrCall{}, false, 1100)) == "k_blind_rotate_generic");
    // the sample the audit runs again
    CHECK(is(br_exact_plan(P), 7, 632, 0));
    return 0;
}

static int check_labels() {
    const EvalOptions d = defaults(256);
    CHECK(br_kernel_label(P, plan(d, 200)) == "k_blind_rotate_wide4<3,7>" && br_kernel_label(P, plan(d, 400)) == "k_blind_rotate_w4r<3,7>");
    CHECK(br_kernel_label(P, plan(d, 900)) == "k_blind_rotate_w2r<3,7>" && br_kernel_label(P, plan(d, 4096)) == "k_blind_rotate_w1b<3,7>");
    CHECK(br_kernel_label(P, plan(d, 1100)) == "k_blind_rotate_w2r+w1b<3,7> 2 of 3 subsets on two waves");
    CHECK(br_kernel_label(P, plan(d, 2304)) == "k_blind_rotate_w2r+w1b<3,7> 2 of 3 subsets on two waves");
    const EvalOptions x = defaults(256, true);
    CHECK(br_kernel_label(P, plan(x, 200)) == "k_blind_rotate_wide<3,7>" && br_kernel_label(P, plan(x, 900)) == "k_blind_rotate_w2<3,7>");
    CHECK(br_kernel_label(P, plan(x, 1100)) == "k_blind_rotate_x1<3,7>");
    // libtfhe 1.0's set: two limbs only ("exact_fft" is forced to 1 for it)
    Params q;
    q.l = 2, q.Bgbit = 10;
    CHECK(br_supported(q) && !br_one_limb_supported(q));
    CHECK(br_kernel_label(q, br_plan(q, x, BrCall{}, true, 1101)) == "k_blind_rotate_x1<2,10>");
    EvalOptions o = x;
    o.exact_one_wave_min = (int64_t)1 << 40;
    CHECK(br_kernel_label(q, br_plan(q, o, BrCall{}, true, 1101)) == "k_blind_rotate_w2<2,10>");
    // measurement and diagnostic builds: by number
    for (int v : {12, 35, 49}) {
        o = d;
        o.br_variant = v;
        char want[64];
        snprintf(want, sizeof want, "k_blind_rotate<3,7> br_variant %d", v);
        CHECK(br_kernel_label(P, plan(o, 1100)) == want && plan(o, 1100).mix.k == 0);
    }
    // parameter sets the 64-lane kernels do not serve
    Params r;
    r.N = 512;
    CHECK(!br_supported(r));
    r = Params{};
    r.l = 2;
    CHECK(!br_supported(r));
    r = Params{};
    r.n = 4097;
    CHECK(!br_supported(r));
    return 0;
}

static int check_variant_table() {
    const int32_t numbers[] = {0, 7, 8, 9, 12, 24, 31, 32, 35, 36, 37, 38, 39, 43, 44, 49};
    size_t rows = 0;
    for (const BrVariant& v : kBrVariants) {
        rows++;
        CHECK(br_variant(v.number) == &v);  // one row per number
        CHECK(v.name && (v.limbs == 1 || v.limbs == 2) && (v.gates == 1 || v.gates == 4) && (!v.wg_builds || v.gates == 4));
        CHECK(v.wg_builds == (v.number == 9 || v.number == 31));
    }
    CHECK(rows == sizeof numbers / sizeof numbers[0]);
    for (int32_t n : numbers) CHECK(variant_known(n));
    for (int32_t n = -5; n <= 1000; n++) {
        bool listed = false;
        for (int32_t m : numbers) listed = listed || m == n;
        CHECK(variant_known(n) == listed);
    }
    for (int32_t n : {24, 31, 32, 35, 49, 36, 37, 43, 44, 38, 39}) CHECK(variant_one_limb(n));
    for (int32_t n : {0, 7, 8, 9, 12, 1}) CHECK(!variant_one_limb(n));
    for (int32_t n : {0, 7, 9, 31, 36, 38, 43}) CHECK(variant_kernel_name(n) != nullptr);
    for (int32_t n : {8, 12, 24, 32, 35, 37, 39, 44, 49, 5}) CHECK(variant_kernel_name(n) == nullptr);
    for (int32_t n : {7, 8, 24, 36, 37, 43, 44, 38, 39}) CHECK(br_variant(n)->long_slices);
    for (int32_t n : {0, 9, 12, 31, 32, 35, 49}) CHECK(!br_variant(n)->long_slices);
    for (int g = 1; g <= 4; g++) CHECK(br_variant_build(31, g) && br_variant_build(9, g) && br_variant_build(32, g) == (g == 4) && br_variant_build(36, g) == (g == 1));
    CHECK(!br_variant_build(31, 0) && !br_variant_build(31, 5) && !br_variant_build(1, 1));
    bool threw = false;
    EvalOptions o = defaults(256);
    o.br_variant = 5;  // the option hook refuses it; a plan for it is an error, not a default
    try {
        (void)plan(o, 100);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    CHECK(threw);
    return 0;
}

// what the launcher relies on, over every launch size under each option row
static int check_invariants() {
    std::vector<EvalOptions> rows;
    for (int64_t cus : {256, 304, 64})
        for (int exact = 0; exact < 2; exact++) {
            const EvalOptions d = defaults(cus, exact != 0);
            rows.push_back(d);
            for (int v : {7, 9, 12, 31, 35, 36, 43, 38, 49}) {
                rows.push_back(d);
                rows.back().br_variant = v;
            }
            for (int s : {1, 64, 65, 630, 632, 633, 4096}) {
                rows.push_back(d);
                rows.back().br_slice = s;
            }
            for (int w : {1, 2, 3, 4}) {
                rows.push_back(d);
                rows.back().wg_gates = w;
            }
            for (int k : {2, 3, 4})
                for (int tw = 1; tw <= 3; tw++) {
                    rows.push_back(d);
                    rows.back().mix_k = k, rows.back().mix_tw = tw;
                }
            for (int s1 : {1, 16, 125, 126, 630})
                for (int ratio : {100, 200, 400}) {
                    rows.push_back(d);
                    rows.back().mix_s1 = s1, rows.back().mix_ratio = ratio;
                }
            rows.push_back(d);
            rows.back().br_slice_default = 1;
            rows.push_back(d);
            rows.back().br_slice_default = 64;
        }
    std::vector<BrCall> calls(5);
    calls[1].exact = true;
    calls[2].concurrency = 2;
    calls[3].level_on_two_lanes = true;
    calls[4].whole_rotation = false, calls[4].lane0 = false;
    for (const EvalOptions& o : rows)
        for (const BrCall& c : calls)
            for (int64_t cnt = 1; cnt <= 20000; cnt++) {
                const BrPlan pl = plan(o, cnt, c);
                const BrVariant* v = br_variant(pl.variant);
                CHECK(!pl.generic && v);
                CHECK(pl.slice >= 1 && pl.slice <= (v->long_slices ? 632 : 64));
                CHECK(pl.wg_gates >= 1 && pl.wg_gates <= 4);  // a build of that size, or the variant's default one
                CHECK(br_variant_build(pl.variant, pl.wg_gates) || br_variant_build(pl.variant, v->gates));
                CHECK(pl.w4r_flip >= 1);
                if ((o.exact_fft || c.exact)) CHECK(v->limbs == 2 || (o.br_variant != 0 && !c.exact));
                if (pl.mix.k) {
                    const MixSteps& m = pl.mix_steps;
                    CHECK(v->limbs == 1 && o.br_variant == 0 && !o.exact_fft && !c.exact && c.concurrency == 1 && !c.level_on_two_lanes && c.whole_rotation && c.lane0);
                    CHECK(pl.mix.k >= 2 && pl.mix.k <= kMaxLanes && pl.mix.tw >= 1 && pl.mix.tw < pl.mix.k && cnt > 4 * o.cus);
                    CHECK(m.s1 >= 1 && m.s2 >= m.s1 && m.cycles >= 1 && m.covered < P.n && pl.mix_wg >= 1 && pl.mix_wg <= 4);
                    CHECK(m.covered == m.cycles * (pl.mix.tw * m.s2 + (pl.mix.k - pl.mix.tw) * m.s1) + (m.tail_s1 > 0 && m.tail_s2 > 0 ? pl.mix.tw * m.tail_s2 + (pl.mix.k - pl.mix.tw) * m.tail_s1 : 0));
                    CHECK(pl.mix_named.k == pl.mix.k && pl.mix_named.tw == pl.mix.tw);
                }
                CHECK((br_kernel_label(P, pl).find("k_blind_rotate_w2r+w1b") == 0) == (pl.mix_named.k != 0));
            }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "--builds")) {
        for (const BrVariant& v : kBrVariants)
            for (int g = 1; g <= 4; g++)
                if (br_variant_build(v.number, g)) printf("%d:%d\n", (int)v.number, g);
        return 0;
    }
    if (check_table() || check_labels() || check_variant_table() || check_invariants()) return 1;
    printf("BR_PLAN_OK\n");
    return 0;
}
