// Host check of the exchange form of the forward transform's lane-high transpose (fft512_forward, XLANE = 2: ie-ache_amd/csrc/
// fft512.h), on the pieces that are plain code -- dft8_twist.h and tw_roots.h.  Every comparison is exact (== on doubles), on
// random 7-bit integer inputs, the gadget digits:
//   1. dft8_twist_fwd_signed with the negated cosines equals the plain pass with registers q and q ^ 4 exchanged;
//   2. dft8_plain<false> on inputs indexed q ^ 4 equals the plain result with the odd outputs negated;
//   3. xl_pi and the un-rotation of k0 are inverse bit permutations over all 64 lanes;
//   4. the whole forward transform of 64 lanes in the exchange form -- relabelled gather, signed first pass, swapped first-set
//      twiddles through ExchangeRoots' two bases, one move per dword for lane bit 3 and the two swaps, signed second-set
//      twiddles, the second transpose written with the un-rotated k0 -- leaves every lane the words the v_cndmask form leaves.
// Exit 0 = all equal.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dft8_twist.h"
#include "tw_roots.h"

struct D2 {
    double x, y;
};
using namespace ieache::w64;

static bool same(const D2& a, const D2& b) { return memcmp(&a, &b, sizeof a) == 0 || (a.x == b.x && a.y == b.y); }
static D2 cmul(D2 a, D2 b) { return D2{fma(a.x, b.x, -a.y * b.y), fma(a.x, b.y, a.y * b.x)}; }  // cmulx<false> of fft512.h
static int digit() { return rand() % 128 - 64; }

static int check_signed_pass() {
    for (int trial = 0; trial < 4000; trial++) {
        D2 x[8], y[8];
        for (int r = 0; r < 8; r++) x[r] = y[r] = D2{(double)digit(), (double)digit()};
        dft8_twist_fwd(x);
        dft8_twist_fwd_signed(y, -kCos16, -kCos316);
        for (int q = 0; q < 8; q++)
            if (!same(y[q], x[q ^ 4])) return printf("signed first pass: register %d differs from output %d\n", q, q ^ 4), 1;
        for (int r = 0; r < 8; r++) y[r] = D2{(double)digit(), (double)digit()}, x[r] = y[r];
        dft8_twist_fwd(x);
        dft8_twist_fwd_signed(y, kCos16, kCos316);
        for (int q = 0; q < 8; q++)
            if (!same(y[q], x[q])) return printf("signed first pass with the sign +1 is not the plain pass\n"), 1;
    }
    return 0;
}

static int check_shifted_inputs() {
    for (int trial = 0; trial < 4000; trial++) {
        D2 x[8], y[8];
        // what the second pass sees: first-pass outputs times twiddles; integers first, then values with full mantissas
        for (int r = 0; r < 8; r++) {
            x[r] = trial & 1 ? D2{digit() * 0.7310585786300049, digit() * 1.1920928955078125e-3 + digit()} : D2{(double)digit(), (double)digit()};
        }
        for (int q = 0; q < 8; q++) y[q] = x[q ^ 4];
        dft8_plain<false>(x);
        dft8_plain<false>(y);
        for (int k = 0; k < 8; k++) {
            const D2 want = (k & 1) ? D2{-x[k].x, -x[k].y} : x[k];
            if (!same(y[k], want)) return printf("DFT-8 of inputs indexed q ^ 4: output %d is not %sthe plain one\n", k, k & 1 ? "minus " : ""), 1;
        }
    }
    return 0;
}

static int check_bit_permutations() {
    bool seen[64] = {};
    for (int lane = 0; lane < 64; lane++) {
        const int p = xl_pi(lane);
        if (p < 0 || p >= 64 || seen[p]) return printf("xl_pi is not a permutation at lane %d\n", lane), 1;
        seen[p] = true;
        if ((p & 7) != (lane & 7)) return printf("xl_pi moves the low lane bits at lane %d\n", lane), 1;
        // lane bits (3, 4, 5) carry bits (2, 0, 1) of the digit
        const int d = p >> 3;
        if (((d >> 2) & 1) != ((lane >> 3) & 1) || (d & 1) != ((lane >> 4) & 1) || ((d >> 1) & 1) != ((lane >> 5) & 1)) return printf("xl_pi: wrong bit at lane %d\n", lane), 1;
        if (xl_k0(lane) != d) return printf("xl_k0 and xl_pi carry different digits at lane %d\n", lane), 1;
        if (xl_lane_hi(xl_k0(lane)) != (lane >> 3) || xl_digit(xl_lane_hi(lane >> 3)) != (lane >> 3)) return printf("the un-rotation is not the inverse at lane %d\n", lane), 1;
        if (xl_flipped(lane) != (d >= 4)) return printf("flipped lanes are not those of positions 32 .. 63 at lane %d\n", lane), 1;
    }
    return 0;
}

// ---- 4: the two forms on 64 lanes ----
static D2 g_table[256 + kTwElems];  // room in front: a flipped lane's second first-set base lies 256 entries below its position
static D2* const tw = g_table + 256;

static void second_half(D2 (&x)[64][8], const int (&k0_of)[64], D2 (&out)[64][8]) {
    // second transpose through the tile -- element (k0, k1, p0) written by lane (k0, p0), read by lane 8 k0 + k1 -- and the third pass
    static D2 tile[8][8][8];
    for (int lane = 0; lane < 64; lane++)
        for (int k1 = 0; k1 < 8; k1++) tile[k0_of[lane]][k1][lane & 7] = x[lane][k1];
    for (int lane = 0; lane < 64; lane++) {
        for (int q = 0; q < 8; q++) out[lane][q] = tile[lane >> 3][lane & 7][q];
        dft8_plain<false>(out[lane]);
    }
}

static int check_whole_transform() {
    const double PI = 3.14159265358979323846;
    for (int idx = 0; idx < 512; idx++) {
        const int k = idx >> 6, lane = idx & 63;
        const double a = PI * (double)(lane * (1 - 4 * k)) / 1024.0;
        tw[idx] = D2{cos(a), sin(a)};
    }
    for (int idx = 0; idx < 64; idx++) {
        const int k = idx >> 3, p0 = idx & 7;
        const double a = -PI * (double)(p0 * k) / 32.0;
        tw[512 + idx] = D2{cos(a), sin(a)};
    }
    for (int neven = 0; neven <= 3; neven++)
        for (int trial = 0; trial < 50; trial++) {
            D2 y[512];
            for (int j = 0; j < 512; j++) y[j] = D2{(double)digit(), (double)digit()};
            static D2 xa[64][8], xb[64][8], t[64][8], outa[64][8], outb[64][8];
            int k0a[64], k0b[64];
            // the v_cndmask form: lane = (p1, p0) -> lane = (k0, p0), register = p1
            for (int lane = 0; lane < 64; lane++) {
                TableRoots<D2> R;
                R.init(tw, lane);
                for (int r = 0; r < 8; r++) t[lane][r] = y[64 * r + lane];
                dft8_twist_fwd(t[lane]);
                for (int k = 0; k < 8; k++) t[lane][k] = cmul(t[lane][k], R.a(k));
            }
            for (int lane = 0; lane < 64; lane++) {
                TableRoots<D2> R;
                R.init(tw, lane);
                for (int p1 = 0; p1 < 8; p1++) xa[lane][p1] = t[8 * p1 + (lane & 7)][lane >> 3];
                dft8_plain<false>(xa[lane]);
                for (int k = 1; k < 8; k++) xa[lane][k] = cmul(xa[lane][k], R.b(k));
                k0a[lane] = lane >> 3;
            }
            second_half(xa, k0a, outa);
            // the exchange form
            auto run = [&](auto roots) {
                decltype(roots) R[64];
                for (int lane = 0; lane < 64; lane++) {
                    R[lane].init(tw, lane);
                    for (int r = 0; r < 8; r++) t[lane][r] = y[64 * r + xl_pi(lane)];
                    dft8_twist_fwd_signed(t[lane], R[lane].c16, R[lane].c316);
                    for (int k = 0; k < 8; k++) t[lane][k] = cmul(t[lane][k], R[lane].fa(k));
                }
                // lane bit 3: every lane gives registers 4 .. 7 and receives into them (row_ror:8 = lane ^ 8)
                for (int lane = 0; lane < 64; lane++)
                    for (int r = 0; r < 8; r++) xb[lane][r] = r < 4 ? t[lane][r] : t[lane ^ 8][r];
                // the swaps: register bit 0 <-> lane bit 4, register bit 1 <-> lane bit 5.  Lanes with the bit clear get in `hi` what
                // the partner had in `lo`, lanes with it set get in `lo` what the partner had in `hi` (swap_dwords, fft512.h)
                for (int step = 0; step < 2; step++) {
                    const int B = step ? 32 : 16, M = step ? 2 : 1;
                    memcpy(t, xb, sizeof t);
                    for (int lane = 0; lane < 64; lane++)
                        for (int r = 0; r < 8; r++) {
                            if (r & M) continue;
                            if (lane & B)
                                xb[lane][r] = t[lane ^ B][r | M];
                            else
                                xb[lane][r | M] = t[lane ^ B][r];
                        }
                }
                for (int lane = 0; lane < 64; lane++) {
                    dft8_plain<false>(xb[lane]);
                    for (int k = 1; k < 8; k++) xb[lane][k] = cmul(xb[lane][k], R[lane].fb(k));
                    k0b[lane] = xl_k0(lane);
                    // what the kernel's inverse transforms read through the same roots: the table's entries, unsigned
                    for (int k = 1; k < 8; k++)
                        if (!same(R[lane].b(k), tw[512 + 8 * k + (lane & 7)])) return printf("the inverse's entry %d is not the table's at lane %d\n", k, lane), 1;
                    for (int k = 0; k < 8; k++)
                        if (!same(R[lane].a(k), tw[64 * k + lane])) return printf("the inverse's first-set entry %d is not the table's at lane %d\n", k, lane), 1;
                }
                second_half(xb, k0b, outb);
                for (int lane = 0; lane < 64; lane++)
                    for (int k2 = 0; k2 < 8; k2++)
                        if (!same(outa[lane][k2], outb[lane][k2])) return printf("exchange form: register %d of lane %d differs from the v_cndmask form's\n", k2, lane), 1;
                return 0;
            };
            const int bad = neven == 0 ? run(ExchangeRoots<D2, 0>()) : neven == 1 ? run(ExchangeRoots<D2, 1>()) : neven == 2 ? run(ExchangeRoots<D2, 2>()) : run(ExchangeRoots<D2, 3>());
            if (bad) return 1;
        }
    return 0;
}

int main() {
    srand(20251);
    if (check_signed_pass() || check_shifted_inputs() || check_bit_permutations() || check_whole_transform()) return 1;
    printf("XLANE_EXCHANGE_OK\n");
    return 0;
}
