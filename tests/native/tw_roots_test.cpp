// Host check of the two ways a lane reads the 512-point transform's twiddle table (ie-ache_amd/csrc/tw_roots.h): for every
// lane the second-set entries a ResidentRoots holds in registers, and the ones it still reads, are bit for bit the table's
// entries TableRoots::b(k) names, and the first set is the same through both.  The table is filled with the values
// build_twiddles (fft512.h) defines, each distinct, so a wrong index cannot pass by coincidence.  Exit 0 = all equal.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <set>
#include <utility>

#include "tw_roots.h"

struct D2 {
    double x, y;
};

static bool same(const D2& a, const D2& b) { return std::memcmp(&a, &b, sizeof(D2)) == 0; }

template <int NRES>
static long check(const D2* tw) {
    using namespace ieache::w64;
    long bad = 0;
    for (int lane = 0; lane < 64; lane++) {
        TableRoots<D2> T;
        ResidentRoots<D2, NRES> R;
        T.init(tw, lane);
        R.init(tw, lane);
        for (int k = 0; k < 8; k++) {
            if (!same(R.a(k), T.a(k)) || !same(T.a(k), tw[k * 64 + lane])) bad++;
            if (k == 0) continue;  // never read: the second pass leaves x[0] alone
            const D2 want = tw[512 + k * 8 + (lane & 7)];
            if (!same(T.b(k), want) || !same(R.b(k), want)) bad++;
            if (k <= NRES && !same(R.tb[k], want)) bad++;
        }
    }
    return bad;
}

int main() {
    using namespace ieache::w64;
    const double PI = 3.14159265358979323846;
    static D2 tw[kTwElems];
    for (int idx = 0; idx < 512; idx++) {
        const int k = idx >> 6, lane = idx & 63;
        const double a = PI * (double)(lane * (1 - 4 * k)) / 1024.0;
        tw[idx] = {std::cos(a), std::sin(a)};
    }
    for (int idx = 0; idx < 64; idx++) {
        const int k = idx >> 3, p0 = idx & 7;
        const double a = -PI * (double)(p0 * k) / 32.0;
        tw[512 + idx] = {std::cos(a), std::sin(a)};
    }
    // the second set's 49 entries with k, p0 >= 1 are pairwise distinct unless p0 k agrees mod 64: the index, not the value,
    // is what the comparison above pins, so count the distinct values to show the table is not degenerate
    std::set<std::pair<double, double>> distinct;
    for (int idx = 0; idx < 64; idx++) distinct.insert({tw[512 + idx].x, tw[512 + idx].y});
    const long bad = check<7>(tw) + check<6>(tw) + check<4>(tw) + check<0>(tw);
    printf("twiddle roots: %ld mismatches over 64 lanes x 4 resident counts; %zu distinct second-set values\n", bad, distinct.size());
    return (bad == 0 && distinct.size() >= 24) ? 0 : 1;
}
