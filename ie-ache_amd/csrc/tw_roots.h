// Layout of the 512-point transform's twiddle table and the two ways a lane gets at its entries (fft512.h), as plain code on a
// two-component value type: compiled into the kernels (V = double2) and, on the host, into tests/native/tw_roots_test.cpp.
//   tw[k*64 + lane]       = exp(i*pi*lane/1024) * exp(-2*pi*i*lane*k/512)   twist (lane part) x first inter-pass twiddle
//   tw[512 + k*8 + p0]    = exp(-2*pi*i*p0*k/64)                            second inter-pass twiddle, p0 = lane & 7
// The second set depends on lane & 7 alone and is the same for every transform of a kernel: seven values per lane.
//   TableRoots      both sets read from the table (in LDS) by every transform: no registers held between transforms.
//   ResidentRoots   the second set copied into 28 VGPRs once per kernel, the first (32 VGPRs per transform) still from the table.
// The resident form fills its registers through the table form's own accessor, so the two cannot name different entries.
#pragma once

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

}  // namespace w64
}  // namespace ieache
