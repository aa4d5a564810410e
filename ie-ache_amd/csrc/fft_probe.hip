// The transform probe (fft_probe.h): fft512.h's transforms and its twiddle builder on caller data, for tests only.
#include "fft_probe.h"

#include <atomic>
#include <cstdlib>
#include <stdexcept>

#include "evaluator.h"  // HIP_CHECK
#include "fft512.h"

namespace ieache {
namespace probe {

using namespace w64;

namespace {

constexpr int kWaves = 4;  // per workgroup, as the G = 4 kernels sit
static_assert(kTwiddleElems == (size_t)kTwElems && kTransformElems == (size_t)kM, "fft_probe.h restates tw_roots.h / fft512.h");

// What the hook of forms 2 .. 4 does: one global load into a register that outlives the transform.
struct HookLoad {
    const double2* src;
    double2* dst;
    __device__ __forceinline__ void operator()() const { *dst = *src; }
};

template <int FORM, class ROOTS>
__device__ __forceinline__ void forward_form(double2 (&x)[8], double2* sT, int lane, const ROOTS& R, const HookLoad& hook) {
    if constexpr (FORM == 0)
        fft512_forward<true, 0>(x, sT, lane, R);
    else if constexpr (FORM == 1)
        fft512_forward<true, 1>(x, sT, lane, R);
    else if constexpr (FORM == 2)
        fft512_forward<true, 1, HookLoad, true>(x, sT, lane, R, hook);
    else if constexpr (FORM == 3)
        fft512_forward<true, 1, HookLoad, false, LaneRootsResident>(x, sT, lane, R, hook);
    else
        fft512_forward<true, 0, HookLoad>(x, sT, lane, R, hook);
}

// units: transforms (forms 0 .. 5) or pairs of them (6, 7); wave w of workgroup b takes unit 4 b + w
// in, out: [transforms][8][64] double2 -- for a forward form `in` is natural order, which is the same addresses (64 r + lane)
// hook_out: [units][64] double2, the hook's register
template <int FORM>
__global__ __launch_bounds__(64 * kWaves) void k_probe_fft512(const double2* __restrict__ in, double2* __restrict__ out, int64_t units,
                                                                const double2* __restrict__ gtw, double2* __restrict__ hook_out) {
    __shared__ __align__(16) double2 sT_all[kWaves * kTile];
    __shared__ __align__(16) double2 sTw[kTwElems];
    using Roots = typename std::conditional<FORM == 3 || FORM == 7, LaneRootsResident, LaneRoots>::type;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double2* sT = sT_all + wave * kTile;
    const int64_t unit = (int64_t)blockIdx.x * kWaves + wave;
    load_twiddles(sTw, gtw, tid, 64 * kWaves);
    __syncthreads();  // the only workgroup barrier
    if (unit >= units) return;
    const Roots R = make_roots<Roots>(sTw, lane);
    if constexpr (FORM < kFirstInverseForm) {
        const double2* src = in + unit * kM;
        double2 x[8];
#pragma unroll
        for (int r = 0; r < 8; r++) x[r] = src[64 * r + lane];
        double2 held = make_double2(0.0, 0.0);
        forward_form<FORM>(x, sT, lane, R, HookLoad{gtw + lane, &held});
        double2* dst = out + unit * kM + lane;
#pragma unroll
        for (int k2 = 0; k2 < 8; k2++) dst[k2 * 64] = x[k2];
        if constexpr (FORM >= 2) hook_out[unit * 64 + lane] = held;
    } else if constexpr (FORM == 5) {
        const double2* src = in + unit * kM + lane;
        double2 x[8];
#pragma unroll
        for (int k2 = 0; k2 < 8; k2++) x[k2] = src[k2 * 64];
        fft512_inverse<true>(x, sT, lane, R);
        double2* dst = out + unit * kM + lane;
#pragma unroll
        for (int r = 0; r < 8; r++) dst[r * 64] = make_double2(x[r].x * untwist_gain(r), x[r].y * untwist_gain(r));
    } else {
        const double2* src = in + unit * 2 * kM + lane;
        double2 x[8], y[8];
#pragma unroll
        for (int k2 = 0; k2 < 8; k2++) x[k2] = src[k2 * 64], y[k2] = src[kM + k2 * 64];
        fft512_inverse_pair<true>(x, y, sT, lane, R);
        double2* dst = out + unit * 2 * kM + lane;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            dst[r * 64] = make_double2(x[r].x * untwist_gain(r), x[r].y * untwist_gain(r));
            dst[kM + r * 64] = make_double2(y[r].x * untwist_gain(r), y[r].y * untwist_gain(r));
        }
    }
}

__global__ __launch_bounds__(64) void k_probe_build_twiddles(double2* out) {
    __shared__ __align__(16) double2 sTw[kTwElems];
    const int lane = threadIdx.x;
    build_twiddles(sTw, lane, 64);
    __syncthreads();
    for (int idx = lane; idx < kTwElems; idx += 64) out[idx] = sTw[idx];
}

template <int FORM>
void launch_form(int64_t units, const double2* d_in, double2* d_out, const double2* d_tw, double2* d_hook, hipStream_t stream) {
    hipLaunchKernelGGL(k_probe_fft512<FORM>, dim3((unsigned)((units + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, stream, d_in, d_out, units, d_tw,
                       d_hook);
}

}  // namespace

const char* form_refusal(int form, size_t count) {
    if (form < 0 || form >= kForms) return "debug_fft512: unknown form (0 .. 7: csrc/fft_probe.h)";
    if (count < 1 || count > ((size_t)1 << 20)) return "debug_fft512: count must lie in 1 .. 2^20";
    if (form >= kFirstPairedForm && count % 2 != 0) return "debug_fft512: a paired form takes an even count";
    return nullptr;
}

void run_fft512(int form, size_t count, const double2* d_in, double2* d_out, const double2* d_tw, hipStream_t stream) {
    if (const char* why = form_refusal(form, count)) throw std::invalid_argument(why);
    const int64_t units = (int64_t)(form >= kFirstPairedForm ? count / 2 : count);
    double2* d_hook = nullptr;
    if (form >= 2 && form < kFirstInverseForm) HIP_CHECK(hipMalloc((void**)&d_hook, (size_t)units * 64 * sizeof(double2)));
    switch (form) {
        case 0: launch_form<0>(units, d_in, d_out, d_tw, d_hook, stream); break;
        case 1: launch_form<1>(units, d_in, d_out, d_tw, d_hook, stream); break;
        case 2: launch_form<2>(units, d_in, d_out, d_tw, d_hook, stream); break;
        case 3: launch_form<3>(units, d_in, d_out, d_tw, d_hook, stream); break;
        case 4: launch_form<4>(units, d_in, d_out, d_tw, d_hook, stream); break;
        case 5: launch_form<5>(units, d_in, d_out, d_tw, d_hook, stream); break;
        case 6: launch_form<6>(units, d_in, d_out, d_tw, d_hook, stream); break;
        default: launch_form<7>(units, d_in, d_out, d_tw, d_hook, stream); break;
    }
    const hipError_t launched = hipGetLastError();
    const hipError_t done = hipStreamSynchronize(stream);  // before the hook's buffer goes
    if (d_hook) (void)hipFree(d_hook);
    HIP_CHECK(launched);
    HIP_CHECK(done);
}

static int forward_path_at_start() {
    const char* e = getenv("IEACHE_W1B_FORWARD");
    return e && e[0] == '1' && !e[1] ? 1 : 2;
}
static std::atomic<int> g_w1b_forward_path{forward_path_at_start()};
void set_w1b_forward_path(int xlane) {
    if (xlane != 1 && xlane != 2) throw std::invalid_argument("debug_forward_path: 1 (v_cndmask pairs) or 2 (the exchange form, the default)");
    g_w1b_forward_path.store(xlane, std::memory_order_relaxed);
}
int w1b_forward_path() { return g_w1b_forward_path.load(std::memory_order_relaxed); }

void build_twiddles_in_wave(double2* d_out, hipStream_t stream) {
    hipLaunchKernelGGL(k_probe_build_twiddles, dim3(1), dim3(64), 0, stream, d_out);
    HIP_CHECK(hipGetLastError());
}

}  // namespace probe
}  // namespace ieache
