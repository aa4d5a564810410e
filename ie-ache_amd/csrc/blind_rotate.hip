// The blind-rotation unit's door (blind_rotate.h): the any-parameter kernel with its key preparation, the audit's compare
// kernel, and the host side -- key forms, scratch, guard record, audit -- that executes a BrPlan.  The 64-lane kernels and
// their launcher are in blind_rotate_w64.hip.
//
// The external product is EXACT on the two-limb spectrum: every BK polynomial is split into two balanced 16-bit limbs before
// the transform, so every inverse-transform output is an integer of magnitude <= kpl x N x 2^(Bgbit-1) x 2^15.  That is 2^37
// for libtfhe's two sets (l = 3 / Bgbit = 7, l = 2 / Bgbit = 10), carried with 15 spare mantissa bits, and at most 2^46 for
// any set Params::supported() admits (params.h: kpl x N x 2^Bgbit <= 2^32), where the modelled distance to an integer is 1/32
// at worst (tests/test_rounding_model_cpu.py, profiles/param_lattice.txt); rounding recovers the integer exactly.
#include "blind_rotate_h2.h"
#include "blind_rotate_w64.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <vector>

namespace ieache {

namespace {

constexpr int kThreads = 256;
const char* const kLdsRefusal = "parameter set exceeds the 160 KiB LDS of a CU";

using namespace dev;

// In-LDS radix-2 transforms over `npoly` polynomials of M complex points.
// Forward: DIF, natural in -> bit-reversed out.  Inverse: DIT, bit-reversed in
// -> natural out, unscaled.  Neither needs a permutation pass.
__device__ void fft_forward_lds(double2* F, int32_t npoly, int32_t M, int32_t logM, const double2* wtab) {
    const int32_t halfM = M >> 1, total = npoly * halfM;
    for (int32_t sh = 0; sh < logM; sh++) {
        const int32_t half = halfM >> sh;
        for (int32_t t = threadIdx.x; t < total; t += blockDim.x) {
            const int32_t poly = t / halfM, bf = t - poly * halfM;
            const int32_t j = bf & (half - 1), grp = bf >> (logM - 1 - sh);
            const int32_t a = poly * M + (grp * 2 * half) + j, b = a + half;
            const double2 w = wtab[j << sh];
            const double2 u = F[a], v = F[b];
            F[a] = make_double2(u.x + v.x, u.y + v.y);
            F[b] = cmul(make_double2(u.x - v.x, u.y - v.y), w);
        }
        __syncthreads();
    }
}
__device__ void fft_inverse_lds(double2* F, int32_t npoly, int32_t M, int32_t logM, const double2* wtab) {
    const int32_t halfM = M >> 1, total = npoly * halfM;
    for (int32_t st = 0; st < logM; st++) {
        const int32_t half = 1 << st, sh = logM - 1 - st;
        for (int32_t t = threadIdx.x; t < total; t += blockDim.x) {
            const int32_t poly = t / halfM, bf = t - poly * halfM;
            const int32_t j = bf & (half - 1), grp = bf >> st;
            const int32_t a = poly * M + (grp * 2 * half) + j, b = a + half;
            const double2 w = wtab[j << sh];
            const double2 u = F[a], v = cmul_conj(F[b], w);
            F[a] = make_double2(u.x + v.x, u.y + v.y);
            F[b] = make_double2(u.x - v.x, u.y - v.y);
        }
        __syncthreads();
    }
}

// ---- key preparation: BK polynomial -> two-limb spectrum ----
__global__ __launch_bounds__(kThreads) void k_bk_to_spectrum(DevKeys K, const Torus32* bk_raw, double2* bkf) {
    extern __shared__ __align__(16) unsigned char smem[];
    double2* F = reinterpret_cast<double2*>(smem);  // [2][M]
    const int32_t M = K.M;
    const Torus32* src = bk_raw + (size_t)blockIdx.x * K.N;
    for (int32_t j = threadIdx.x; j < M; j += blockDim.x) {
        const int32_t v0 = src[j], v1 = src[j + M];
        const int32_t lo0 = (int16_t)(v0 & 0xFFFF), lo1 = (int16_t)(v1 & 0xFFFF);
        const int32_t hi0 = (int32_t)(((int64_t)v0 - lo0) >> 16), hi1 = (int32_t)(((int64_t)v1 - lo1) >> 16);
        const double2 tw = K.twist[j];
        F[j] = cmul(make_double2((double)lo0, (double)lo1), tw);
        F[M + j] = cmul(make_double2((double)hi0, (double)hi1), tw);
    }
    __syncthreads();
    fft_forward_lds(F, 2, M, K.logM, K.wtab);
    double2* dst = bkf + (size_t)blockIdx.x * 2 * M;
    for (int32_t j = threadIdx.x; j < 2 * M; j += blockDim.x) dst[j] = F[j];
}

// ---- K0..K4, generic parameters: one workgroup per gate instance ----
// LDS: F [max(kpl,4)][M] double2 | acc [2][N] int32 | bara [n] u16
__global__ __launch_bounds__(kThreads) void k_blind_rotate_generic(DevKeys K, WorkDesc W, Torus32* ext,
                                                                   int32_t steps, Torus32* dbg_acc) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int32_t N = K.N, M = K.M, n = K.n, l = K.l, kpl = K.kpl;
    const int32_t frows = kpl > 4 ? kpl : 4;
    double2* F = reinterpret_cast<double2*>(smem);
    int32_t* acc = reinterpret_cast<int32_t*>(F + (size_t)frows * M);
    uint16_t* bara = reinterpret_cast<uint16_t*>(acc + 2 * N);
    __shared__ int32_t s_barb;

    const int64_t item = (int64_t)blockIdx.x;
    const GateInst g = resolve(W, W.item0 + item, K.stride);
    const int32_t log2N2 = K.logM + 2;

    // K0 + K1
    for (int32_t i = threadIdx.x; i <= n; i += blockDim.x) {
        const int32_t bar = modswitch2N(combined_coef(g, i, n), log2N2);
        if (i < n)
            bara[i] = (uint16_t)bar;
        else
            s_barb = bar;
    }
    __syncthreads();
    // K2: acc = (0, X^{2N-barb} * (mu,...,mu)); a programmable bootstrap starts from its item's test polynomial instead, or
    // (a table of TLWE samples) from both halves of its item's sample, rotated alike
    {
        const int32_t a0 = (2 * N - s_barb) & (2 * N - 1);
        const bool tlwe = W.flat_type == kFlatRawTlwe;
        const Torus32* v = test_poly_row(W, W.item0 + item, tlwe ? 2 * N : N);
        if (v && tlwe) {
            for (int32_t j = threadIdx.x; j < N; j += blockDim.x) {
                acc[j] = rot_coef(v, j, a0, N);
                acc[N + j] = rot_coef(v + N, j, a0, N);
            }
        } else {
            for (int32_t j = threadIdx.x; j < N; j += blockDim.x) {
                acc[j] = 0;
                const int32_t idx = (j - a0) & (2 * N - 1);
                acc[N + j] = v ? rot_coef(v, j, a0, N) : (idx < N ? kMU : -kMU);
            }
        }
    }
    __syncthreads();

    const uint32_t halfBg = 1u << (K.Bgbit - 1), maskBg = (1u << K.Bgbit) - 1;
    const double invM = 1.0 / (double)M;
    const int32_t nsteps = steps < 0 ? n : steps;
    // K3
    for (int32_t i = 0; i < nsteps; i++) {
        const int32_t a = bara[i];
        if (a == 0) continue;  // uniform across the workgroup; exact arithmetic makes the step a no-op
        // (X^a - 1) * acc, gadget decomposition, fold + twist
        for (int32_t j = threadIdx.x; j < M; j += blockDim.x) {
            const double2 tw = K.twist[j];
#pragma unroll 2
            for (int32_t c = 0; c < 2; c++) {
                const int32_t* p = acc + c * N;
                const uint32_t d0 = (uint32_t)rot_coef(p, j, a, N) - (uint32_t)p[j] + K.dec_offset;
                const uint32_t d1 = (uint32_t)rot_coef(p, j + M, a, N) - (uint32_t)p[j + M] + K.dec_offset;
                for (int32_t q = 0; q < l; q++) {
                    const int32_t sh = 32 - (q + 1) * K.Bgbit;
                    const int32_t e0 = (int32_t)((d0 >> sh) & maskBg) - (int32_t)halfBg;
                    const int32_t e1 = (int32_t)((d1 >> sh) & maskBg) - (int32_t)halfBg;
                    F[(size_t)(c * l + q) * M + j] = cmul(make_double2((double)e0, (double)e1), tw);
                }
            }
        }
        __syncthreads();
        fft_forward_lds(F, kpl, M, K.logM, K.wtab);
        // spectrum-domain accumulate: out(c,limb) = sum_row dec[row] * BK_i[row][c][limb]
        const double2* bki = K.bkf + (size_t)i * kpl * 4 * M;
        for (int32_t pt = threadIdx.x; pt < M; pt += blockDim.x) {
            double2 s[4];
#pragma unroll
            for (int32_t q = 0; q < 4; q++) s[q] = make_double2(0.0, 0.0);
            for (int32_t row = 0; row < kpl; row++) {
                const double2 d = F[(size_t)row * M + pt];
                const double2* b = bki + (size_t)row * 4 * M + pt;
#pragma unroll
                for (int32_t q = 0; q < 4; q++) s[q] = cfma(d, b[(size_t)q * M], s[q]);
            }
            // every thread has consumed its own column of F; rows 0..3 become the outputs
#pragma unroll
            for (int32_t q = 0; q < 4; q++) F[(size_t)q * M + pt] = s[q];
        }
        __syncthreads();
        fft_inverse_lds(F, 4, M, K.logM, K.wtab);
        // untwist, round, recombine limbs, accumulate
        for (int32_t j = threadIdx.x; j < M; j += blockDim.x) {
            const double2 tw = K.twist[j];
#pragma unroll 2
            for (int32_t c = 0; c < 2; c++) {
                const double2 lo = cmul_conj(F[(size_t)(2 * c) * M + j], tw);
                const double2 hi = cmul_conj(F[(size_t)(2 * c + 1) * M + j], tw);
                const int64_t r0 = __double2ll_rn(lo.x * invM) + (__double2ll_rn(hi.x * invM) << 16);
                const int64_t r1 = __double2ll_rn(lo.y * invM) + (__double2ll_rn(hi.y * invM) << 16);
                acc[c * N + j] = (int32_t)((uint32_t)acc[c * N + j] + (uint32_t)r0);
                acc[c * N + j + M] = (int32_t)((uint32_t)acc[c * N + j + M] + (uint32_t)r1);
            }
        }
        __syncthreads();
    }
    if (dbg_acc) {
        for (int32_t j = threadIdx.x; j < 2 * N; j += blockDim.x) dbg_acc[(size_t)item * 2 * N + j] = acc[j];
    }
    // K4: u = (a'_0 = acc.a_0, a'_j = -acc.a_{N-j}; b' = acc.b_0)
    if (ext) {
        Torus32* u = ext + (size_t)item * (N + 4);
        for (int32_t j = threadIdx.x; j <= N; j += blockDim.x)
            u[j] = j == 0 ? acc[0] : (j == N ? acc[N] : (int32_t)(0u - (uint32_t)acc[N - j]));
    }
}

// Audit of the one-limb blind rotation: rows it produced -- extracted samples (`words` = N + 1 of rows of N + 4) or whole
// accumulators (2N of 2N) -- against the same gate instances run on the two-limb (provably exact) kernel.  One workgroup per
// row; any differing word counts the row in *mismatches.
// inject: test hook -- row 0 is compared as if its first word differed.
__global__ void k_audit_compare(const Torus32* primary, const Torus32* exact, int32_t words, int32_t stride, unsigned* mismatches, int inject) {
    const size_t g = blockIdx.x;
    const Torus32* a = primary + g * (size_t)stride;
    const Torus32* b = exact + g * (size_t)stride;
    int bad = (inject && g == 0 && threadIdx.x == 0) ? 1 : 0;
    for (int32_t j = threadIdx.x; j < words; j += blockDim.x) bad |= a[j] != b[j];
    if (__syncthreads_or(bad) && threadIdx.x == 0) atomicAdd(mismatches, 1u);
}

}  // namespace

void BlindRotate::init(const Params& p, DevKeys& K) {
    p_ = p;
    const int32_t M = K.M;
    generic_lds_ = br_generic_lds_bytes(p);
    // (a set k_blind_rotate_h2 serves is accepted without it: there only a "force_generic" launch is refused, in launch())
    if (generic_lds_ > kBrLdsMax && !br_h2_supported(p)) throw std::invalid_argument(kLdsRefusal);
    // twiddles, computed once in double precision on the host
    std::vector<double2> tw(M), w(M / 2 > 0 ? M / 2 : 1);
    for (int32_t j = 0; j < M; j++) tw[j] = make_double2(std::cos(M_PI * j / p.N), std::sin(M_PI * j / p.N));
    for (int32_t j = 0; j < M / 2; j++)
        w[j] = make_double2(std::cos(-2.0 * M_PI * j / M), std::sin(-2.0 * M_PI * j / M));
    twist_.allocate(tw.size());
    wtab_.allocate(w.size());
    HIP_CHECK(hipMemcpy(twist_, tw.data(), sizeof(double2) * tw.size(), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(wtab_, w.data(), sizeof(double2) * w.size(), hipMemcpyHostToDevice));
    K.twist = twist_;
    K.wtab = wtab_;
    K_ = K;
    // (per context, on the context's device: the sizes depend on the parameter set)
    if (generic_lds_ <= kBrLdsMax) allow_dynamic_lds((const void*)k_blind_rotate_generic, generic_lds_, "k_blind_rotate_generic");
}

void BlindRotate::load_key(const Torus32* d_bk_raw, hipStream_t stream) {
    const size_t npoly = (size_t)p_.n * K_.kpl * 2;
    if (!bkf_) bkf_.allocate(npoly * 2 * K_.M);
    K_.bkf = bkf_;
    hipLaunchKernelGGL(k_bk_to_spectrum, dim3((unsigned)npoly), dim3(kThreads), 2 * K_.M * sizeof(double2), stream, K_, d_bk_raw, bkf_);
    HIP_CHECK(hipGetLastError());
    if (br_h2_supported(p_)) {
        if (!bkf_h2_) bkf_h2_.allocate(h2::spectrum_elems(p_));
        if (!tw_w64_) {
            tw_w64_.allocate(w64::twiddle_table_elems());
            w64::build_twiddle_table(tw_w64_, stream);
            HIP_CHECK(hipGetLastError());
        }
        h2::prepare_spectrum(p_, d_bk_raw, bkf_h2_, stream);
        HIP_CHECK(hipGetLastError());
    }
    if (!br_supported(p_)) return;
    if (!bkf_w64_) bkf_w64_.allocate(w64::spectrum_elems(p_));
    if (!tw_w64_) {
        tw_w64_.allocate(w64::twiddle_table_elems());
        w64::build_twiddle_table(tw_w64_, stream);
        HIP_CHECK(hipGetLastError());
    }
    w64::prepare_spectrum(p_, d_bk_raw, bkf_w64_, stream);
    HIP_CHECK(hipGetLastError());
    if (!bkf1_w64_) bkf1_w64_.allocate(w64::spectrum1_elems(p_));
    if (!guard_) {
        guard_.allocate(4);
        HIP_CHECK(hipMemsetAsync(guard_, 0, 4 * sizeof(unsigned), stream));
    }
    w64::prepare_spectrum1(p_, d_bk_raw, bkf1_w64_, stream);
    HIP_CHECK(hipGetLastError());
}

void BlindRotate::reserve(BrScratch& scratch, size_t need, const EvalOptions& opt, bool use_w64) {
    if (use_w64 || (br_h2_supported(p_) && !opt.force_generic)) scratch.state.reserve(need, (size_t)opt.chunk, br_state_bytes_per_item(p_));
}

int BlindRotate::launch(BrScratch& scratch, const BrPlan& plan, const EvalOptions& opt, const BrLanes& lanes, hipStream_t stream, const BrPart* parts,
                        size_t n_parts, Torus32* ext, int32_t steps, Torus32* dbg_acc) {
    int64_t cnt = 0;
    for (size_t q = 0; q < n_parts; q++) {
        const WorkDesc& w = parts[q].W;
        if (!w.gates && w.tv && w.n_tv < 1) throw std::invalid_argument("programmable bootstrap without test polynomials");
        if (parts[q].cnt < 1) throw std::logic_error("blind-rotation launch: an empty part");
        cnt += parts[q].cnt;
    }
    if (plan.h2) {
        reserve(scratch, (size_t)cnt, opt, false);  // in place already unless the caller did not reserve
        return h2::launch(p_, K_, bkf_h2_, tw_w64_, plan, stream, parts, n_parts, scratch.state, ext, steps, dbg_acc);
    }
    if (plan.generic) {
        if (generic_lds_ > kBrLdsMax) throw std::invalid_argument(kLdsRefusal);  // an N = 2048 set only k_blind_rotate_h2 can serve
        // the any-parameter kernel has its prologue inside it: the parts one after another, each over its own rows -- the
        // same results as a shared launch would give, without the sharing
        int64_t off = 0;
        for (size_t q = 0; q < n_parts; q++) {
            hipLaunchKernelGGL(k_blind_rotate_generic, dim3((unsigned)parts[q].cnt), dim3(kThreads), generic_lds_, stream, K_, parts[q].W,
                               ext ? ext + (size_t)off * (size_t)(K_.N + 4) : nullptr, steps, dbg_acc ? dbg_acc + (size_t)off * 2 * (size_t)K_.N : nullptr);
            off += parts[q].cnt;
        }
        return (int)n_parts;
    }
    reserve(scratch, (size_t)cnt, opt, true);  // in place already unless the caller did not reserve
    if ((plan.variant == kVariantWideStamps || plan.variant == kVariantOneLimbStamps) && !diag_) diag_.allocate(16, sizeof(unsigned long long), 0, /*zero=*/true);
    return w64::launch(p_, K_, w64::Tables{bkf_w64_, bkf1_w64_, tw_w64_, guard_, diag_}, plan, lanes, stream, parts, n_parts, scratch.state, ext, steps, dbg_acc);
}

void BlindRotate::audit(BrScratch& scratch, const BrPlan& plan, EvalOptions& opt, hipStream_t stream, const BrPart* parts, size_t n_parts, const Torus32* ext,
                        const Torus32* acc) {
    if (plan.generic || opt.fft_audit <= 0 || !guard_ || n_parts == 0) return;
    if (!variant_one_limb(plan.variant)) return;  // the launch was exact by construction
    if (++audit_counts.seq % opt.fft_audit != 0) return;
    // the part: by the count of audits made so far, so that consecutive audits of a joint evaluation visit its parts in turn
    const size_t part = (size_t)((uint64_t)audit_counts.audits % (uint64_t)n_parts);
    int64_t row0 = 0;  // the part's first row of ext
    for (size_t q = 0; q < part; q++) row0 += parts[q].cnt;
    const WorkDesc& w = parts[part].W;
    const int64_t cnt = parts[part].cnt;
    const int64_t m = std::min<int64_t>(kAuditGates, cnt);
    const int64_t off = cnt > m ? (int64_t)(((uint64_t)audit_counts.seq * 0x9E3779B97F4A7C15ull >> 33) % (uint64_t)(cnt - m + 1)) : 0;
    const size_t ext_row_bytes = (size_t)(K_.N + 4) * 4;
    const size_t acc_row_words = (size_t)2 * (size_t)K_.N;
    if (acc && !scratch.audit_acc) scratch.audit_acc.allocate((size_t)kAuditGates, acc_row_words * 4);
    if (!acc && !scratch.audit_ext) scratch.audit_ext.allocate((size_t)kAuditGates, ext_row_bytes);
    if (!scratch.audit_state) scratch.audit_state.allocate((size_t)kAuditGates, br_state_bytes_per_item(p_));
    WorkDesc wa = w;
    wa.item0 = w.item0 + off;
    const BrPart pa{wa, m};
    // the exact kernel leaves what the launch left: extracted samples, or (acc) its whole accumulators
    w64::launch(p_, K_, w64::Tables{bkf_w64_, bkf1_w64_, tw_w64_, guard_, nullptr}, br_exact_plan(p_), BrLanes{}, stream, &pa, 1, scratch.audit_state,
                acc ? nullptr : (Torus32*)scratch.audit_ext, -1, acc ? (Torus32*)scratch.audit_acc : nullptr);
    if (acc)
        hipLaunchKernelGGL(k_audit_compare, dim3((unsigned)m), dim3(256), 0, stream, acc + (size_t)(row0 + off) * acc_row_words, scratch.audit_acc,
                           (int32_t)acc_row_words, (int32_t)acc_row_words, guard_ + 2, opt.fft_audit_inject ? 1 : 0);
    else
        hipLaunchKernelGGL(k_audit_compare, dim3((unsigned)m), dim3(256), 0, stream, ext + (size_t)(row0 + off) * (size_t)(K_.N + 4), scratch.audit_ext,
                           K_.N + 1, K_.N + 4, guard_ + 2, opt.fft_audit_inject ? 1 : 0);
    HIP_CHECK(hipGetLastError());
    opt.fft_audit_inject = 0;
    audit_counts.audits++;
    audit_counts.gates += m;
}

bool BlindRotate::guard_read(unsigned h[3]) const {
    if (!guard_) return false;
    HIP_CHECK(hipMemcpy(h, guard_, 3 * sizeof(unsigned), hipMemcpyDeviceToHost));
    return true;
}

void BlindRotate::guard_rearm() {
    if (!guard_) return;
    HIP_CHECK(hipMemset(guard_, 0, sizeof(unsigned)));
    HIP_CHECK(hipMemset(guard_ + 2, 0, sizeof(unsigned)));
}

bool BlindRotate::guard_inject() {
    if (!guard_) return false;
    const unsigned one = 1;
    HIP_CHECK(hipMemcpy(guard_, &one, sizeof one, hipMemcpyHostToDevice));
    return true;
}

}  // namespace ieache
