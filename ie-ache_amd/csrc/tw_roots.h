// Layout of the 512-point transform's twiddle table and the two ways a lane gets at its entries (fft512.h), as plain code on a
// two-component value type: compiled into the kernels (V = double2) and, on the host, into tests/native/tw_roots_test.cpp.
//   tw[k*64 + lane]       = exp(i*pi*lane/1024) * exp(-2*pi*i*lane*k/512)   twist (lane part) x first inter-pass twiddle
//   tw[512 + k*8 + p0]    = exp(-2*pi*i*p0*k/64)                            second inter-pass twiddle, p0 = lane & 7
// The second set depends on lane & 7 alone and is the same for every transform of a kernel: seven values per lane.
//   TableRoots      both sets read from the table (in LDS) by every transform: no registers held between transforms.
//   ResidentRoots   the second set copied into 28 VGPRs once per kernel, the first (32 VGPRs per transform) still from the table.
// The resident form fills its registers through the table form's own accessor, so the two cannot name different entries.
#pragma once

#include "dft8_twist.h"

#ifndef IEACHE_HD
#ifdef __HIPCC__
#define IEACHE_HD __device__ __forceinline__
#else
#define IEACHE_HD inline
#endif
#endif

namespace ieache {
namespace w64 {

constexpr int kTwElems = 8 * 64 + 8 * 8;
// first set: entry k of a lane at a(tw)[64 k];  second set: entry k at b(tw)[8 k]
template <class V>
IEACHE_HD const V* tw_a_base(const V* tw, int lane) { return tw + lane; }
template <class V>
IEACHE_HD const V* tw_b_base(const V* tw, int lane) { return tw + 512 + (lane & 7); }

template <class V>
struct TableRoots {
    const V* t1;  // &tw[lane], stride 64
    const V* t2;  // &tw[512 + (lane & 7)], stride 8
    IEACHE_HD V a(int k) const { return t1[k * 64]; }
    IEACHE_HD V b(int k) const { return t2[k * 8]; }
    IEACHE_HD void init(const V* tw, int lane) {
        t1 = tw_a_base(tw, lane);
        t2 = tw_b_base(tw, lane);
    }
};

// NRES: how many of the seven second-set entries (k = 1 .. NRES) are held; the others are read from the table like TableRoots'
template <class V, int NRES = 7>
struct ResidentRoots {
    TableRoots<V> table;
    V tb[8];  // tb[1 .. NRES]; tb[0] (= 1) is never multiplied with and never loaded
    IEACHE_HD V a(int k) const { return table.a(k); }
    IEACHE_HD V b(int k) const { return k <= NRES ? tb[k] : table.b(k); }
    IEACHE_HD void init(const V* tw, int lane) {
        table.init(tw, lane);
#pragma unroll
        for (int k = 1; k <= NRES; k++) tb[k] = table.b(k);
    }
};

// ---- the exchange form of the forward transform (fft512_forward, XLANE = 2) ----
// Its lane-high transpose exchanges register bit 2 with lane bit 3 (one DPP move per dword: every lane gives registers 4 .. 7),
// register bit 0 with lane bit 4 and register bit 1 with lane bit 5 (the two swap instructions).  So lane bits (3, 4, 5) carry
// bits (2, 0, 1) of a three-bit digit: of p1 before the exchange -- lane `lane` gathers the inputs of position xl_pi(lane) --
// and of k0 after it -- the second transpose writes the rows of xl_k0(lane).  xl_lane_hi is the way back.
IEACHE_HD constexpr int xl_digit(int hi) { return ((hi >> 1) & 3) | ((hi & 1) << 2); }     // lane >> 3 -> the digit it carries
IEACHE_HD constexpr int xl_lane_hi(int digit) { return ((digit & 3) << 1) | (digit >> 2); }  // the digit -> lane >> 3
IEACHE_HD constexpr int xl_pi(int lane) { return (xl_digit(lane >> 3) << 3) | (lane & 7); }
IEACHE_HD constexpr int xl_k0(int lane) { return xl_digit(lane >> 3); }
// lanes with bit 3 set run the first pass with the members of every output pair (q, q ^ 4) in each other's registers
// (dft8_twist_fwd_signed) and come out of the exchange with register s holding p1 = s ^ 4: a second pass on inputs shifted by 4,
// whose odd outputs are the true ones negated (dft8_plain).  Their second-set twiddles carry that sign.
IEACHE_HD constexpr bool xl_flipped(int lane) { return (lane >> 3) & 1; }

// Roots of a kernel whose forward transforms take the exchange form and whose inverse transforms stay in the table's order.
// The four odd entries of the second set are resident with the forward's sign (negated in flipped lanes), so the inverse reads
// those from the table; NEVEN of the three even ones (k = 2, 4, ..), which carry no sign, are resident for both directions.
//   a, b      the inverse's: a as TableRoots'; b resident for the held even entries, from the table otherwise
//   fa, fb    the forward's: first-set entry q ^ 4 for register q in flipped lanes, through two bases (q < 4: entry q + 4 at
//             + 256, q >= 4: entry q - 4 at - 256); second set resident but for the even entries not held
//   c16, c316 the cosines of the first pass's last stage times the lane's sign
template <class V, int NEVEN = 2>
struct ExchangeRoots {
    static_assert(NEVEN >= 0 && NEVEN <= 3, "the second set has three even entries: 2, 4, 6");
    static constexpr bool held(int k) { return (k & 1) || k <= 2 * NEVEN; }
    TableRoots<V> table;
    const V* f1lo;
    const V* f1hi;
    double c16, c316;
    V tb[8];
    IEACHE_HD V a(int k) const { return table.a(k); }
    IEACHE_HD V b(int k) const { return (held(k) && !(k & 1)) ? tb[k] : table.b(k); }
    IEACHE_HD V fa(int q) const { return q < 4 ? f1lo[q * 64] : f1hi[q * 64]; }
    IEACHE_HD V fb(int k) const { return held(k) ? tb[k] : table.b(k); }
    IEACHE_HD void init(const V* tw, int lane) {
        const bool flip = xl_flipped(lane);
        table.init(tw, lane);
        const V* base = tw_a_base(tw, xl_pi(lane));
        f1lo = base + (flip ? 256 : 0);
        f1hi = base - (flip ? 256 : 0);
        c16 = flip ? -kCos16 : kCos16;
        c316 = flip ? -kCos316 : kCos316;
#pragma unroll
        for (int k = 1; k < 8; k++) {
            if (!held(k)) continue;
            tb[k] = table.b(k);
            if ((k & 1) && flip) tb[k].x = -tb[k].x, tb[k].y = -tb[k].y;
        }
    }
};

}  // namespace w64
}  // namespace ieache
