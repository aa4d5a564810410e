// See tfhe_host.h.  CPU-side key generation and bit encryption for the
// evaluator's tools and the metadata handling of the `cloud` shim.
#include "tfhe_host.h"

#include <sys/random.h>

#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <stdexcept>
#include <vector>
#ifdef _OPENMP
#include <omp.h>
#endif

namespace ieache {

static inline uint64_t rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
static inline uint64_t splitmix64(uint64_t& x) {
    uint64_t z = (x += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

Rng::Rng(const uint32_t* seed_words, int count, uint64_t stream) {
    uint64_t x = 0x243F6A8885A308D3ULL ^ (stream * 0xD1342543DE82EF95ULL);
    for (int i = 0; i < count; i++) {
        x ^= seed_words[i];
        (void)splitmix64(x);
    }
    for (int i = 0; i < 4; i++) s_[i] = splitmix64(x);
}

// ChaCha20 block function (RFC 8439 section 2.3), 64-bit block counter in words 12-13
void Rng::chacha_refill() {
    auto rotl32 = [](uint32_t v, int c) { return (v << c) | (v >> (32 - c)); };
    uint32_t st[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u};
    for (int i = 0; i < 8; i++) st[4 + i] = key_[i];
    st[12] = (uint32_t)counter_;
    st[13] = (uint32_t)(counter_ >> 32);
    st[14] = nonce_[0];
    st[15] = nonce_[1];
    uint32_t x[16];
    memcpy(x, st, sizeof x);
    auto qr = [&](int a, int b, int c2, int d) {
        x[a] += x[b]; x[d] = rotl32(x[d] ^ x[a], 16);
        x[c2] += x[d]; x[b] = rotl32(x[b] ^ x[c2], 12);
        x[a] += x[b]; x[d] = rotl32(x[d] ^ x[a], 8);
        x[c2] += x[d]; x[b] = rotl32(x[b] ^ x[c2], 7);
    };
    for (int r = 0; r < 10; r++) {
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15);
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14);
    }
    for (int i = 0; i < 16; i++) x[i] += st[i];
    memcpy(buf_, x, sizeof buf_);
    buf_pos_ = 0;
    counter_++;
}

Rng Rng::secure() {
    Rng r((uint64_t)0);
    unsigned char seed[44];
    size_t got = 0;
    while (got < sizeof seed) {
        const ssize_t k = getrandom(seed + got, sizeof seed - got, 0);
        if (k < 0) {
            if (errno == EINTR) continue;
            throw std::runtime_error("getrandom() failed: no kernel entropy for fresh encryptions");
        }
        got += (size_t)k;
    }
    memcpy(r.key_, seed, 32);
    memcpy(r.nonce_, seed + 32, 12);
    r.chacha_ = true;
    r.counter_ = 0;
    r.buf_pos_ = 8;
    return r;
}

uint64_t Rng::next() {
    if (chacha_) {
        if (buf_pos_ >= 8) chacha_refill();
        return buf_[buf_pos_++];
    }
    const uint64_t result = rotl(s_[1] * 5, 7) * 9;
    const uint64_t t = s_[1] << 17;
    s_[2] ^= s_[0];
    s_[3] ^= s_[1];
    s_[1] ^= s_[2];
    s_[0] ^= s_[3];
    s_[2] ^= t;
    s_[3] = rotl(s_[3], 45);
    return result;
}

double Rng::uniform01() { return ((next() >> 11) + 1) * (1.0 / 9007199254740992.0); }

double Rng::gaussian(double sigma) {
    if (have_spare_) {
        have_spare_ = false;
        return spare_ * sigma;
    }
    const double u = uniform01(), v = uniform01();
    const double r = std::sqrt(-2.0 * std::log(u)), th = 6.283185307179586476925 * v;
    spare_ = r * std::sin(th);
    have_spare_ = true;
    return r * std::cos(th) * sigma;
}

Torus32 Rng::gaussian_torus32(double sigma) {
    // libtfhe dtot32: fractional part scaled to 2^32
    const double d = gaussian(sigma);
    const double frac = d - std::nearbyint(d);
    return (Torus32)(uint32_t)(int64_t)std::llrint(frac * 4294967296.0);
}

int32_t modswitch_from_torus32(Torus32 phase, int32_t Msize) {
    const uint64_t interv = ((UINT64_C(1) << 63) / (uint64_t)Msize) * 2;
    const uint64_t half = interv / 2;
    const uint64_t phase64 = ((uint64_t)(uint32_t)phase << 32) + half;
    return (int32_t)(phase64 / interv);
}

Torus32 modswitch_to_torus32(int32_t mu, int32_t Msize) {
    const uint64_t interv = ((UINT64_C(1) << 63) / (uint64_t)Msize) * 2;
    const uint64_t phase64 = (uint64_t)(int64_t)mu * interv;
    return (Torus32)(phase64 >> 32);
}

void lwe_encrypt_bit(const Params& p, const int32_t* lwe_key, int bit, Rng& rng, Torus32* out) {
    uint32_t b = (uint32_t)rng.gaussian_torus32(p.lwe_alpha_min) + (uint32_t)(bit ? kMU : -kMU);
    for (int32_t i = 0; i < p.n; i++) {
        const Torus32 a = rng.uniform_torus32();
        out[i] = a;
        if (lwe_key[i]) b += (uint32_t)a;
    }
    out[p.n] = (Torus32)b;
}

Torus32 lwe_phase(const Params& p, const int32_t* lwe_key, const Torus32* sample) {
    uint32_t acc = (uint32_t)sample[p.n];
    for (int32_t i = 0; i < p.n; i++)
        if (lwe_key[i]) acc -= (uint32_t)sample[i];
    return (Torus32)acc;
}

// b += a * s mod (X^N+1) for a binary key polynomial s
static void add_mul_binary_key(int32_t N, uint32_t* b, const Torus32* a, const int32_t* s) {
    for (int32_t i = 0; i < N; i++) {
        if (!s[i]) continue;
        // X^i * a : coefficient j of a lands on j+i, negated past N
        for (int32_t j = 0; j < N - i; j++) b[j + i] += (uint32_t)a[j];
        for (int32_t j = N - i; j < N; j++) b[j + i - N] -= (uint32_t)a[j];
    }
}

void tlwe_encrypt_zero(const Params& p, const int32_t* tlwe_key, double alpha, Rng& rng, Torus32* sample) {
    const int32_t N = p.N, k = p.k;
    Torus32* a = sample;  // polys a_0..a_{k-1}, then b
    uint32_t* b = (uint32_t*)(a + (size_t)k * N);
    for (int32_t j = 0; j < N; j++) b[j] = (uint32_t)rng.gaussian_torus32(alpha);
    for (int32_t c = 0; c < k; c++) {
        for (int32_t j = 0; j < N; j++) a[(size_t)c * N + j] = rng.uniform_torus32();
        add_mul_binary_key(N, b, a + (size_t)c * N, tlwe_key + (size_t)c * N);
    }
}

void tlwe_encrypt(const Params& p, const int32_t* tlwe_key, const Torus32* polys, size_t count, double alpha, Rng& rng, Torus32* out) {
    const size_t N = (size_t)p.N, row = (size_t)(p.k + 1) * N;
    for (size_t i = 0; i < count; i++) {
        tlwe_encrypt_zero(p, tlwe_key, alpha, rng, out + i * row);
        uint32_t* b = (uint32_t*)(out + i * row + (size_t)p.k * N);
        for (size_t j = 0; j < N; j++) b[j] += (uint32_t)polys[i * N + j];
    }
}

void tlwe_phase(const Params& p, const int32_t* tlwe_key, const Torus32* samples, size_t count, Torus32* phase) {
    const size_t N = (size_t)p.N, row = (size_t)(p.k + 1) * N;
    std::vector<uint32_t> as(N);
    for (size_t i = 0; i < count; i++) {
        std::fill(as.begin(), as.end(), 0u);
        for (int32_t c = 0; c < p.k; c++) add_mul_binary_key(p.N, as.data(), samples + i * row + (size_t)c * N, tlwe_key + (size_t)c * N);
        const Torus32* b = samples + i * row + (size_t)p.k * N;
        for (size_t j = 0; j < N; j++) phase[i * N + j] = (Torus32)((uint32_t)b[j] - as[j]);
    }
}

// Threads for the two key-generation loops: OpenMP's default is every hardware thread of the host, but a
// container is often allowed far less CPU time than that (cgroup cpu.max), and hundreds of threads on a
// 16-CPU share only contend.
static int host_threads() {
    int n = 1;
#ifdef _OPENMP
    n = omp_get_num_procs();
#endif
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char quota[64];
        long period = 0;
        if (fscanf(f, "%63s %ld", quota, &period) == 2 && strcmp(quota, "max") != 0 && period > 0) {
            const long q = (atol(quota) + period - 1) / period;
            if (q >= 1 && q < n) n = (int)q;
        }
        fclose(f);
    }
    return n < 1 ? 1 : (n > 64 ? 64 : n);
}

void packing_keygen(const Params& p, const int32_t* lwe_key, const int32_t* tlwe_key, int32_t t, int32_t basebit, double alpha, Rng& rng,
                    Torus32* out) {
    const size_t N = (size_t)p.N, row = 2 * N;
    for (int32_t i = 0; i < p.n; i++)
        for (int32_t j = 0; j < t; j++) {
            Torus32* s = out + ((size_t)i * t + j) * row;
            tlwe_encrypt_zero(p, tlwe_key, alpha, rng, s);
            // the constant polynomial s_i 2^(32 - (j+1) b): coefficient 0 of B
            ((uint32_t*)s)[N] += (uint32_t)(lwe_key[i] & 1) << (32 - (j + 1) * basebit);
        }
}

void pack_reference(const Params& p, int32_t t, int32_t basebit, const Torus32* pk, size_t groups, int32_t m, int32_t spread, int32_t shift,
                    const Torus32* rows, Torus32* out) {
    const size_t N = (size_t)p.N, cols = 2 * N, n = (size_t)p.n, nrows = groups * (size_t)m;
    const uint32_t prec = 1u << (31 - t * basebit), mask = (1u << basebit) - 1u;
    std::vector<uint32_t> R(nrows * cols, 0u);
    const int n_threads = host_threads();
    (void)n_threads;
#pragma omp parallel for schedule(dynamic, 1) num_threads(n_threads)
    for (int64_t r = 0; r < (int64_t)nrows; r++) {
        const Torus32* x = rows + (size_t)r * (n + 1);
        uint32_t* Rr = R.data() + (size_t)r * cols;
        Rr[N] = (uint32_t)x[n];  // (0, b X^0)
        for (size_t i = 0; i < n; i++) {
            const uint32_t abar = (uint32_t)x[i] + prec;
            for (int32_t j = 0; j < t; j++) {
                const uint32_t d = (abar >> (32 - (j + 1) * basebit)) & mask;
                if (!d) continue;
                const uint32_t* key = (const uint32_t*)pk + (i * (size_t)t + (size_t)j) * cols;
                for (size_t c = 0; c < cols; c++) Rr[c] -= d * key[c];
            }
        }
    }
    uint32_t* o = (uint32_t*)out;
    std::fill(o, o + groups * cols, 0u);
    for (size_t g = 0; g < groups; g++)
        for (int32_t pp = 0; pp < m; pp++)
            for (int32_t q = 0; q < spread; q++) {
                const size_t a = ((size_t)pp * (size_t)spread + (size_t)q + (size_t)shift) % cols;  // X^a with a in [0, 2N)
                for (size_t c = 0; c < 2; c++) {
                    const uint32_t* src = R.data() + (g * (size_t)m + (size_t)pp) * cols + c * N;
                    uint32_t* dst = o + g * cols + c * N;
                    // coefficient j of the row lands on j + a, negated for every wrap past N
                    if (a < N) {
                        for (size_t j = 0; j < N - a; j++) dst[j + a] += src[j];
                        for (size_t j = N - a; j < N; j++) dst[j + a - N] -= src[j];
                    } else {
                        const size_t aa = a - N;
                        for (size_t j = 0; j < N - aa; j++) dst[j + aa] -= src[j];
                        for (size_t j = N - aa; j < N; j++) dst[j + aa - N] += src[j];
                    }
                }
            }
}

void tgsw_encrypt_sample(const Params& p, const int32_t* tlwe_key, int32_t mu, double alpha, Rng& rng, Torus32* out) {
    const int32_t N = p.N, k = p.k, l = p.l, kpl = p.kpl();
    for (int32_t row = 0; row < kpl; row++) tlwe_encrypt_zero(p, tlwe_key, alpha, rng, out + (size_t)row * (k + 1) * N);
    // + mu * H : gadget on the constant coefficient of poly `bloc` in row bloc*l+q
    for (int32_t bloc = 0; bloc <= k; bloc++)
        for (int32_t q = 0; q < l; q++) {
            const uint32_t h = 1u << (32 - (q + 1) * p.Bgbit);
            uint32_t* coef = (uint32_t*)(out + ((size_t)(bloc * l + q) * (k + 1) + bloc) * N);
            coef[0] += (uint32_t)mu * h;
        }
}

// out (+)= C [.] d for one TGSW sample C [2l][2][N] and the TLWE difference d [2][N]: schoolbook, every word mod 2^32
static void external_product_add(const Params& p, const Torus32* C, const uint32_t* d, uint32_t* out) {
    const int32_t N = p.N, l = p.l, Bgbit = p.Bgbit;
    const uint32_t halfBg = 1u << (Bgbit - 1), mask = Bgbit >= 32 ? 0xFFFFFFFFu : (1u << Bgbit) - 1u;
    uint32_t offset = 0;
    for (int32_t q = 1; q <= l; q++) offset += halfBg << (32 - q * Bgbit);
    std::vector<uint32_t> dig(N);
    for (int32_t row = 0; row < 2 * l; row++) {
        const int32_t c = row / l, q = row % l + 1;
        for (int32_t j = 0; j < N; j++) dig[j] = (((d[(size_t)c * N + j] + offset) >> (32 - q * Bgbit)) & mask) - halfBg;
        for (int32_t o = 0; o < 2; o++) {
            const uint32_t* key = (const uint32_t*)C + ((size_t)row * 2 + o) * N;
            uint32_t* dst = out + (size_t)o * N;
            // X^i key scaled by digit i: coefficient j of key lands on j + i, negated past N
            for (int32_t i = 0; i < N; i++) {
                const uint32_t e = dig[i];
                if (!e) continue;
                for (int32_t j = 0; j < N - i; j++) dst[j + i] += e * key[j];
                for (int32_t j = N - i; j < N; j++) dst[j + i - N] -= e * key[j];
            }
        }
    }
}
static void cmux_one(const Params& p, const Torus32* C, const Torus32* d1, const Torus32* d0, Torus32* out) {
    const size_t W = (size_t)2 * p.N;
    std::vector<uint32_t> d(W), acc(W);
    for (size_t j = 0; j < W; j++) {
        acc[j] = d0 ? (uint32_t)d0[j] : 0u;
        d[j] = (uint32_t)d1[j] - acc[j];
    }
    external_product_add(p, C, d.data(), acc.data());
    for (size_t j = 0; j < W; j++) out[j] = (Torus32)acc[j];
}

void cmux_reference(const Params& p, const Torus32* set, size_t n_set, size_t count, const int32_t* sel_of, const Torus32* d1, const Torus32* d0,
                    Torus32* out) {
    const size_t W = (size_t)2 * p.N, S = (size_t)p.kpl() * W;
    const int n_threads = host_threads();
    (void)n_threads;
#pragma omp parallel for schedule(dynamic, 1) num_threads(n_threads)
    for (int64_t r = 0; r < (int64_t)count; r++) {
        const size_t sel = sel_of ? (size_t)sel_of[r] : (size_t)r % n_set;
        cmux_one(p, set + sel * S, d1 + (size_t)r * W, d0 ? d0 + (size_t)r * W : nullptr, out + (size_t)r * W);
    }
}

void lut_tree_reference(const Params& p, const Torus32* set, size_t n_set, size_t count, int32_t depth, const int32_t* sel_of,
                        const Torus32* tables, const int32_t* table_of, Torus32* out) {
    const size_t W = (size_t)2 * p.N, S = (size_t)p.kpl() * W, T = (size_t)1 << depth;
    const int n_threads = host_threads();
    (void)n_threads;
    for (size_t i = 0; i < count; i++) {
        const Torus32* table = tables + (table_of ? (size_t)table_of[i] : 0) * T * W;
        std::vector<Torus32> level(table, table + T * W), next;
        for (int32_t k = 0; k < depth; k++) {
            const size_t w = T >> (k + 1);
            const size_t sel = sel_of ? (size_t)sel_of[i * (size_t)depth + k] : (i * (size_t)depth + k) % n_set;
            next.assign(w * W, 0);
#pragma omp parallel for schedule(dynamic, 1) num_threads(n_threads)
            for (int64_t j = 0; j < (int64_t)w; j++)
                cmux_one(p, set + sel * S, level.data() + (2 * (size_t)j + 1) * W, level.data() + 2 * (size_t)j * W, next.data() + (size_t)j * W);
            level.swap(next);
        }
        std::copy(level.begin(), level.begin() + W, out + i * W);
    }
}

void lut_scatter_reference(const Params& p, const Torus32* set, size_t n_set, size_t count, int32_t depth, const int32_t* sel_of,
                           const Torus32* values, const Torus32* mem, Torus32* out) {
    const size_t W = (size_t)2 * p.N, S = (size_t)p.kpl() * W, T = (size_t)1 << depth;
    const int n_threads = host_threads();
    (void)n_threads;
    for (size_t i = 0; i < count; i++) {
        std::vector<uint32_t> level(values + i * W, values + (i + 1) * W), next;
        for (int32_t t = 0; t < depth; t++) {
            const size_t w = (size_t)1 << t, at = i * (size_t)depth + (size_t)(depth - 1 - t);
            const size_t sel = sel_of ? (size_t)sel_of[at] : at % n_set;
            next.assign(2 * w * W, 0u);
#pragma omp parallel for schedule(dynamic, 1) num_threads(n_threads)
            for (int64_t j = 0; j < (int64_t)w; j++) {
                const uint32_t* parent = level.data() + (size_t)j * W;
                uint32_t* lo = next.data() + 2 * (size_t)j * W;
                uint32_t* hi = lo + W;  // zeros: the product alone
                external_product_add(p, set + sel * S, parent, hi);
                for (size_t c = 0; c < W; c++) lo[c] = parent[c] - hi[c];
            }
            level.swap(next);
        }
        const Torus32* base = mem ? mem + i * T * W : nullptr;
        Torus32* dst = out + i * T * W;
        for (size_t c = 0; c < T * W; c++) dst[c] = (Torus32)((base ? (uint32_t)base[c] : 0u) + level[c]);
    }
}

// rows [count][2][N] rotated in `steps` steps each; the selector of (row r, step t) is index r stride + t of the call
static void rotate_rows(const Params& p, const Torus32* set, size_t n_set, size_t count, int32_t steps, size_t stride, const int32_t* sel_of,
                        const int32_t* amount_of, const Torus32* in, Torus32* out) {
    const size_t N = (size_t)p.N, W = 2 * N, S = (size_t)p.kpl() * W;
    const int n_threads = host_threads();
    (void)n_threads;
#pragma omp parallel for schedule(dynamic, 1) num_threads(n_threads)
    for (int64_t r = 0; r < (int64_t)count; r++) {
        std::vector<uint32_t> acc(in + (size_t)r * W, in + ((size_t)r + 1) * W), d(W);
        for (int32_t t = 0; t < steps; t++) {
            const size_t a = amount_of ? (size_t)amount_of[t] : (t < 31 && ((size_t)1 << t) < W ? W - ((size_t)1 << t) : 0);
            if (a == 0) continue;  // the operand is zero and so is its truncating decomposition
            const size_t at = (size_t)r * stride + (size_t)t, sel = sel_of ? (size_t)sel_of[at] : at % n_set;
            // X^a acc - acc: coefficient j takes +/- coefficient j - a mod 2N
            for (size_t c = 0; c < 2; c++)
                for (size_t j = 0; j < N; j++) {
                    const size_t from = (j + W - a) & (W - 1);
                    const uint32_t v = acc[c * N + (from & (N - 1))];
                    d[c * N + j] = ((from & N) ? 0u - v : v) - acc[c * N + j];
                }
            external_product_add(p, set + sel * S, d.data(), acc.data());
        }
        for (size_t j = 0; j < W; j++) out[(size_t)r * W + j] = (Torus32)acc[j];
    }
}

void tlwe_rotate_reference(const Params& p, const Torus32* set, size_t n_set, size_t count, int32_t steps, const int32_t* sel_of,
                           const int32_t* amount_of, const Torus32* in, Torus32* out) {
    rotate_rows(p, set, n_set, count, steps, (size_t)steps, sel_of, amount_of, in, out);
}

void keyswitch_reference(const Params& p, const Torus32* ksk, size_t count, const Torus32* u, Torus32* out) {
    const size_t N = (size_t)p.k * (size_t)p.N, n = (size_t)p.n, base = (size_t)p.ks_base();
    const int32_t t = p.ks_t, bb = p.ks_basebit;
    const uint32_t prec_offset = 1u << (32 - (1 + bb * t)), mask = (1u << bb) - 1u;
    for (size_t r = 0; r < count; r++) {
        const Torus32* x = u + r * (N + 1);
        uint32_t* o = (uint32_t*)out + r * (n + 1);
        std::fill(o, o + n, 0u);
        o[n] = (uint32_t)x[N];
        for (size_t i = 0; i < N; i++) {
            const uint32_t abar = (uint32_t)x[i] + prec_offset;
            for (int32_t j = 0; j < t; j++) {
                const uint32_t dig = (abar >> (32 - (j + 1) * bb)) & mask;
                if (!dig) continue;  // libtfhe subtracts nothing for digit 0
                const uint32_t* row = (const uint32_t*)ksk + ((i * (size_t)t + (size_t)j) * base + dig) * (n + 1);
                for (size_t q = 0; q <= n; q++) o[q] -= row[q];
            }
        }
    }
}

void lut_read_reference(const Params& p, const Torus32* set, size_t n_set, const Torus32* ksk, size_t count, int32_t depth, int32_t steps,
                        const int32_t* sel_of, const int32_t* amount_of, const Torus32* tables, const int32_t* table_of, int32_t coef,
                        Torus32* out) {
    const size_t W = (size_t)2 * p.N, stride = (size_t)depth + (size_t)steps;
    // the tree's selectors are indices steps .. steps + depth - 1 of each item
    std::vector<int32_t> tree_sel(count * (size_t)depth), coef_of(count, coef);
    for (size_t i = 0; i < count; i++)
        for (size_t k = 0; k < (size_t)depth; k++) {
            const size_t at = i * stride + (size_t)steps + k;
            tree_sel[i * (size_t)depth + k] = sel_of ? sel_of[at] : (int32_t)(at % n_set);
        }
    std::vector<Torus32> rows(count * W), u(ksk ? count * ((size_t)p.N + 1) : 0);
    lut_tree_reference(p, set, n_set, count, depth, tree_sel.data(), tables, table_of, rows.data());
    rotate_rows(p, set, n_set, count, steps, stride, sel_of, amount_of, rows.data(), rows.data());
    tlwe_extract_reference(p, count, rows.data(), coef_of.data(), ksk ? u.data() : out);
    if (ksk) keyswitch_reference(p, ksk, count, u.data(), out);
}

void lut_add_reference(const Params& p, const Torus32* set, size_t n_set, size_t count, int32_t depth, int32_t steps, const int32_t* sel_of,
                       const int32_t* amount_of, const Torus32* values, const Torus32* mems, size_t n_mems, const int32_t* mem_of, Torus32* out) {
    const size_t W = (size_t)2 * p.N, T = (size_t)1 << depth, stride = (size_t)depth + (size_t)steps;
    // the write's default amounts, +2^t mod 2N; the scatter's selectors are indices steps .. steps + depth - 1 of each item
    std::vector<int32_t> plus(steps);
    for (int32_t t = 0; t < steps; t++) plus[t] = t < 31 ? (int32_t)(((size_t)1 << t) & (W - 1)) : 0;
    std::vector<int32_t> tree_sel(count * (size_t)depth);
    for (size_t i = 0; i < count; i++)
        for (size_t k = 0; k < (size_t)depth; k++) {
            const size_t at = i * stride + (size_t)steps + k;
            tree_sel[i * (size_t)depth + k] = sel_of ? sel_of[at] : (int32_t)(at % n_set);
        }
    std::vector<Torus32> rows(count * W), leaves(count * T * W);
    rotate_rows(p, set, n_set, count, steps, stride, sel_of, amount_of ? amount_of : plus.data(), values, rows.data());
    lut_scatter_reference(p, set, n_set, count, depth, tree_sel.data(), rows.data(), nullptr, leaves.data());
    // out may be mems itself
    if (out != mems)
        for (size_t c = 0; c < n_mems * T * W; c++) out[c] = mems ? mems[c] : 0;
    for (size_t i = 0; i < count; i++) {
        Torus32* dst = out + (mem_of ? (size_t)mem_of[i] : 0) * T * W;
        const Torus32* leaf = leaves.data() + i * T * W;
        for (size_t c = 0; c < T * W; c++) dst[c] = (Torus32)((uint32_t)dst[c] + (uint32_t)leaf[c]);
    }
}

void automaton_reference(const Params& p, const Torus32* set, size_t n_set, int32_t states, int32_t steps, int32_t n_out, const int32_t* next0,
                         const int32_t* next1, size_t count, const int32_t* sel_of, const Torus32* finals, const int32_t* final_of, Torus32* out) {
    const size_t W = (size_t)2 * p.N, Q = (size_t)states;
    std::vector<Torus32> v(Q * W), d1(Q * W), d0(Q * W);
    std::vector<int32_t> sel(Q);
    for (size_t i = 0; i < count; i++) {
        const Torus32* fin = finals + (final_of ? (size_t)final_of[i] : 0) * Q * W;
        std::copy(fin, fin + Q * W, v.begin());
        for (int32_t t = steps - 1; t >= 0; t--) {
            const size_t at = i * (size_t)steps + (size_t)t;
            std::fill(sel.begin(), sel.end(), sel_of ? sel_of[at] : (int32_t)(at % n_set));
            for (size_t q = 0; q < Q; q++) {
                std::copy(v.begin() + (size_t)next1[(size_t)t * Q + q] * W, v.begin() + ((size_t)next1[(size_t)t * Q + q] + 1) * W, d1.begin() + q * W);
                std::copy(v.begin() + (size_t)next0[(size_t)t * Q + q] * W, v.begin() + ((size_t)next0[(size_t)t * Q + q] + 1) * W, d0.begin() + q * W);
            }
            cmux_reference(p, set, n_set, Q, sel.data(), d1.data(), d0.data(), v.data());
        }
        std::copy(v.begin(), v.begin() + (size_t)n_out * W, out + i * (size_t)n_out * W);
    }
}

void lwe_linear_reference(const LinearRows& r, size_t batch, int32_t n_out, int32_t n_in, const int8_t* w, const int32_t* bias, const Torus32* x,
                          Torus32* out) {
    const size_t words = (size_t)r.words;
#pragma omp parallel for collapse(2) schedule(static)
    for (int64_t b = 0; b < (int64_t)batch; b++)
        for (int32_t i = 0; i < n_out; i++) {
            Torus32* dst = out + ((size_t)b * n_out + i) * words;
            for (size_t q = 0; q < words; q++) dst[q] = 0;
            for (int32_t j = 0; j < n_in; j++) {
                const uint32_t f = (uint32_t)(int32_t)w[(size_t)i * n_in + j];
                const Torus32* src = x + ((size_t)b * n_in + j) * words;
                for (size_t q = 0; q < words; q++) dst[q] = (Torus32)((uint32_t)dst[q] + f * (uint32_t)src[q]);
            }
            if (bias && r.bias_word >= 0) dst[r.bias_word] = (Torus32)((uint32_t)dst[r.bias_word] + (uint32_t)bias[i]);
        }
}

void tlwe_extract_reference(const Params& p, size_t count, const Torus32* tlwe, const int32_t* coef_of, Torus32* u) {
    const int32_t N = p.N;
    for (size_t r = 0; r < count; r++) {
        const Torus32* A = tlwe + r * 2 * (size_t)N;
        Torus32* dst = u + r * ((size_t)N + 1);
        const int32_t j = coef_of ? coef_of[r] : 0;
        for (int32_t i = 0; i < N; i++) dst[i] = i <= j ? A[j - i] : (Torus32)(0u - (uint32_t)A[N + j - i]);
        dst[N] = A[N + j];
    }
}

void tlwe_project_reference(const Params& p, int32_t t, int32_t basebit, const Torus32* pk, size_t count, int32_t first, int32_t width, int32_t dest,
                            const Torus32* in, Torus32* out) {
    Params q = p;
    q.n = p.N;  // the packing key switch whose source key is the ring key
    const size_t N = (size_t)p.N, W = 2 * N;
    std::vector<Torus32> u((size_t)width * (N + 1));
    for (size_t i = 0; i < count; i++) {
        for (int32_t c = 0; c < width; c++) {
            const int32_t coef = first + c;
            tlwe_extract_reference(p, 1, in + i * W, &coef, u.data() + (size_t)c * (N + 1));
        }
        pack_reference(q, t, basebit, pk, 1, width, 1, dest, u.data(), out + i * W);
    }
}

void lut_write_coef_reference(const Params& p, const Torus32* set, size_t n_set, int32_t t, int32_t basebit, const Torus32* pk, size_t count,
                              int32_t depth, int32_t steps, int32_t width, int32_t unit, const int32_t* sel_of, const Torus32* fresh, const Torus32* mem,
                              Torus32* out) {
    const size_t W = (size_t)2 * p.N, stride = (size_t)depth + (size_t)steps;
    std::vector<int32_t> toward(steps), back(steps), tree_sel(count * (size_t)depth), own(count);
    for (int32_t s = 0; s < steps; s++) {
        back[s] = (int32_t)(((size_t)unit << s) & (W - 1));
        toward[s] = (int32_t)((W - (size_t)back[s]) & (W - 1));
    }
    for (size_t i = 0; i < count; i++) {
        own[i] = (int32_t)i;
        for (size_t k = 0; k < (size_t)depth; k++) {
            const size_t at = i * stride + (size_t)steps + k;
            tree_sel[i * (size_t)depth + k] = sel_of ? sel_of[at] : (int32_t)(at % n_set);
        }
    }
    std::vector<Torus32> rows(count * W), old(count * W);
    lut_tree_reference(p, set, n_set, count, depth, tree_sel.data(), mem, own.data(), rows.data());
    rotate_rows(p, set, n_set, count, steps, stride, sel_of, toward.data(), rows.data(), rows.data());
    tlwe_project_reference(p, t, basebit, pk, count, 0, width, 0, rows.data(), old.data());
    for (size_t c = 0; c < count * W; c++) old[c] = (Torus32)((uint32_t)fresh[c] - (uint32_t)old[c]);  // delta, in place over old
    lut_add_reference(p, set, n_set, count, depth, steps, sel_of, back.data(), old.data(), mem, count, own.data(), out);
}

void unpack_reference(const Params& p, const Torus32* ksk, size_t count, int32_t first, int32_t width, int32_t spread, const Torus32* in, Torus32* out) {
    const size_t N = (size_t)p.N, W = 2 * N, row = ksk ? (size_t)p.n + 1 : N + 1;
    std::vector<Torus32> u(ksk ? N + 1 : 0);
    for (size_t i = 0; i < count; i++)
        for (int32_t q = 0; q < width; q++) {
            const int32_t coef = first + q * spread;
            Torus32* dst = out + (i * (size_t)width + (size_t)q) * row;
            tlwe_extract_reference(p, 1, in + i * W, &coef, ksk ? u.data() : dst);
            if (ksk) keyswitch_reference(p, ksk, 1, u.data(), dst);
        }
}

void word_read_reference(const Params& p, const Torus32* set, size_t n_set, const Torus32* ksk, size_t count, int32_t depth, int32_t steps, int32_t width,
                         int32_t unit, const int32_t* sel_of, const Torus32* tables, const int32_t* table_of, Torus32* out) {
    const size_t W = (size_t)2 * p.N, stride = (size_t)depth + (size_t)steps;
    std::vector<int32_t> toward(steps), tree_sel(count * (size_t)depth);
    for (int32_t s = 0; s < steps; s++) toward[s] = (int32_t)((W - (((size_t)unit << s) & (W - 1))) & (W - 1));
    for (size_t i = 0; i < count; i++)
        for (size_t k = 0; k < (size_t)depth; k++) {
            const size_t at = i * stride + (size_t)steps + k;
            tree_sel[i * (size_t)depth + k] = sel_of ? sel_of[at] : (int32_t)(at % n_set);
        }
    std::vector<Torus32> rows(count * W);
    lut_tree_reference(p, set, n_set, count, depth, tree_sel.data(), tables, table_of, rows.data());
    rotate_rows(p, set, n_set, count, steps, stride, sel_of, toward.data(), rows.data(), rows.data());
    unpack_reference(p, ksk, count, 0, width, 1, rows.data(), out);
}

void keygen(const Params& p, const uint32_t* seed_words, int nseed, SecretKeyData* out,
            bool with_cloud) {
    out->p = p;
    // nseed < 0: every stream is its own kernel-keyed ChaCha20 generator (nothing reproducible)
    const bool secure = nseed < 0;
    auto make_rng = [&](uint64_t stream) { return secure ? Rng::secure() : Rng(seed_words, nseed, stream); };
    Rng krng = make_rng(0);
    out->lwe_key.resize(p.n);
    for (auto& b : out->lwe_key) b = krng.bit();
    out->tlwe_key.resize((size_t)p.k * p.N);
    for (auto& b : out->tlwe_key) b = krng.bit();
    out->cloud.p = p;
    out->cloud.bk.clear();
    out->cloud.ksk.clear();
    if (!with_cloud) return;

    const int n_threads = host_threads();
    (void)n_threads;
    const int32_t N = p.N, k = p.k, kpl = p.kpl();
    // Bootstrapping key: BK_i = TGSW_enc(lwe_key[i]) under the TLWE key.
    // One RNG stream per i so the loop can run in any order / in parallel.
    out->cloud.bk.assign(p.bk_count(), 0);
#pragma omp parallel for schedule(dynamic, 4) num_threads(n_threads)
    for (int32_t i = 0; i < p.n; i++) {
        Rng rng = make_rng(1 + (uint64_t)i);
        tgsw_encrypt_sample(p, out->tlwe_key.data(), out->lwe_key[i], p.tlwe_alpha_min, rng, out->cloud.bk.data() + (size_t)i * kpl * (k + 1) * N);
    }
    // Key-switch key: KSK[i][j][d] = LWE_enc(d * tlwe_key[i] / base^(j+1)) under the n-key
    const int32_t base = p.ks_base(), n = p.n;
    out->cloud.ksk.assign(p.ksk_count(), 0);
#pragma omp parallel for schedule(dynamic, 16) num_threads(n_threads)
    for (int32_t i = 0; i < k * N; i++) {
        Rng rng = make_rng((uint64_t)1 << 32 | (uint64_t)i);
        for (int32_t j = 0; j < p.ks_t; j++)
            for (int32_t d = 1; d < base; d++) {  // d = 0 stays all-zero: never read
                Torus32* s = out->cloud.ksk.data() + (((size_t)i * p.ks_t + j) * base + d) * (n + 1);
                uint32_t b = (uint32_t)rng.gaussian_torus32(p.lwe_alpha_min) +
                             (uint32_t)out->tlwe_key[i] * (uint32_t)d *
                                 (1u << (32 - (j + 1) * p.ks_basebit));
                for (int32_t q = 0; q < n; q++) {
                    const Torus32 a = rng.uniform_torus32();
                    s[q] = a;
                    if (out->lwe_key[q]) b += (uint32_t)a;
                }
                s[n] = (Torus32)b;
            }
    }
}

}  // namespace ieache
