// Stand-alone host test (built with -fsanitize=address,undefined by tests/test_ring2048_cpu.py) of the identity an N = 2048
// CMux step rests on: a polynomial of Z[X]/(X^2048 + 1) written as p = p_e(Y) + X p_o(Y), Y = X^2,
// with both halves in Z[Y]/(Y^1024 + 1).  Plain C++ restatements of
//   the product   (d k)_e = d_e k_e + (Y d_o) k_o,   (d k)_o = d_e k_o + d_o k_e
//   the rotation  X^a p:  a even: Y^(a/2) on each half;  a odd: new even = Y^((a+1)/2) p_o, new odd = Y^((a-1)/2) p_e
// against the direct negacyclic product and rotation mod 2^32, on random polynomials and on extreme ones, and composed into one
// whole CMux step (rotate, subtract, decompose, multiply, accumulate) for every amount where the halves may go wrong.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

namespace {

using Poly = std::vector<uint32_t>;  // coefficients mod 2^32

constexpr int N = 2048, H = N / 2;

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);         \
            return 1;                                                     \
        }                                                                 \
    } while (0)

// a b mod X^n + 1, mod 2^32
Poly mul(const Poly& a, const Poly& b) {
    const size_t n = a.size();
    Poly r(n, 0u);
    for (size_t i = 0; i < n; i++) {
        if (!a[i]) continue;
        for (size_t j = 0; j < n; j++) {
            const uint32_t t = a[i] * b[j];
            if (i + j < n)
                r[i + j] += t;
            else
                r[i + j - n] -= t;
        }
    }
    return r;
}

// X^a p mod X^n + 1, a in [0, 2n)
Poly rot(const Poly& p, int a) {
    const int n = (int)p.size();
    Poly r((size_t)n);
    for (int i = 0; i < n; i++) {
        const int idx = (i - a) & (2 * n - 1);
        const uint32_t v = p[(size_t)(idx & (n - 1))];
        r[(size_t)i] = (idx & n) ? 0u - v : v;
    }
    return r;
}

Poly add(const Poly& a, const Poly& b) {
    Poly r(a.size());
    for (size_t i = 0; i < a.size(); i++) r[i] = a[i] + b[i];
    return r;
}
Poly sub(const Poly& a, const Poly& b) {
    Poly r(a.size());
    for (size_t i = 0; i < a.size(); i++) r[i] = a[i] - b[i];
    return r;
}

struct Halves {
    Poly e, o;
};
Halves split(const Poly& p) {
    Halves h{Poly(H), Poly(H)};
    for (int j = 0; j < H; j++) h.e[(size_t)j] = p[(size_t)(2 * j)], h.o[(size_t)j] = p[(size_t)(2 * j + 1)];
    return h;
}
Poly join(const Halves& h) {
    Poly p(N);
    for (int j = 0; j < H; j++) p[(size_t)(2 * j)] = h.e[(size_t)j], p[(size_t)(2 * j + 1)] = h.o[(size_t)j];
    return p;
}

// the product on the halves: four products on the ring of degree 1024, the Y shift an index with the negacyclic sign
Halves mul_split(const Halves& d, const Halves& k) {
    const Poly yo = rot(d.o, 1);
    return Halves{add(mul(d.e, k.e), mul(yo, k.o)), add(mul(d.e, k.o), mul(d.o, k.e))};
}

// the rotation on the halves, a in [0, 2N)
Halves rot_split(const Halves& p, int a) {
    if ((a & 1) == 0) return Halves{rot(p.e, a / 2), rot(p.o, a / 2)};
    return Halves{rot(p.o, ((a + 1) / 2) & (N - 1)), rot(p.e, (a - 1) / 2)};  // Y^1024 = -1, Y^2048 = 1: (a + 1) / 2 = 2048 at a = 4095
}

// digit q (0-based) of every coefficient: tGswTorus32PolynomialDecompH
Poly digit(const Poly& p, int q, int l, int Bgbit) {
    uint32_t offset = 0;
    for (int i = 1; i <= l; i++) offset += (1u << (Bgbit - 1)) << (32 - i * Bgbit);
    Poly r(p.size());
    for (size_t i = 0; i < p.size(); i++)
        r[i] = (((p[i] + offset) >> (32 - (q + 1) * Bgbit)) & ((1u << Bgbit) - 1)) - (1u << (Bgbit - 1));
    return r;
}

Poly random_poly(std::mt19937& g, int n) {
    Poly p((size_t)n);
    for (auto& v : p) v = (uint32_t)g();
    return p;
}

const int kAmounts[] = {0, 1, 2, 2047, 2048, 2049, 4094, 4095};

int check_rotation(std::mt19937& g) {
    const Poly extremes[] = {Poly(N, 0x7FFFFFFFu), Poly(N, 0x80000000u), random_poly(g, N), random_poly(g, N)};
    for (const Poly& p : extremes)
        for (int a : kAmounts) CHECK(join(rot_split(split(p), a)) == rot(p, a));
    const Poly p = random_poly(g, N);  // every amount once
    for (int a = 0; a < 2 * N; a++) CHECK(join(rot_split(split(p), a)) == rot(p, a));
    return 0;
}

int check_product(std::mt19937& g) {
    const int Bgbit = 7;
    const Poly all_neg(N, 0u - (1u << (Bgbit - 1)));  // every digit at -Bg / 2
    Poly mixed(N);
    for (int i = 0; i < N; i++) mixed[(size_t)i] = (i & 1) ? 0x7FFFFFFFu : 0x80000000u;
    const Poly keys[] = {Poly(N, 0x7FFFFFFFu), Poly(N, 0x80000000u), mixed, random_poly(g, N)};
    Poly small = random_poly(g, N);
    for (auto& v : small) v = (v & 127u) - 64u;
    const Poly digits[] = {all_neg, small, random_poly(g, N)};
    for (const Poly& d : digits)
        for (const Poly& k : keys) CHECK(join(mul_split(split(d), split(k))) == mul(d, k));
    return 0;
}

// One CMux step acc += sum_rows digit_row((X^a - 1) acc) bk[row], directly and on the halves: the digits of the halves are the
// halves of the digits (the decomposition is coefficient-wise), the parity of a picks their roles.
int check_step(std::mt19937& g, int l, int Bgbit, const Poly* fixed_key) {
    const Poly acc[2] = {random_poly(g, N), random_poly(g, N)};
    std::vector<Poly> bk;  // [2l][2]
    for (int i = 0; i < 4 * l; i++) bk.push_back(fixed_key ? *fixed_key : random_poly(g, N));
    for (int a : kAmounts) {
        Poly want[2] = {acc[0], acc[1]};
        Halves got[2] = {split(acc[0]), split(acc[1])};
        const Halves in[2] = {split(acc[0]), split(acc[1])};
        for (int c = 0; c < 2; c++) {
            const Poly diff = sub(rot(acc[c], a), acc[c]);
            const Halves r = rot_split(in[c], a);
            const Halves diff_h{sub(r.e, in[c].e), sub(r.o, in[c].o)};
            for (int q = 0; q < l; q++) {
                const Poly d = digit(diff, q, l, Bgbit);
                const Halves dh{digit(diff_h.e, q, l, Bgbit), digit(diff_h.o, q, l, Bgbit)};
                CHECK(join(dh) == d);
                for (int out = 0; out < 2; out++) {
                    const Poly& key = bk[(size_t)((c * l + q) * 2 + out)];
                    want[out] = add(want[out], mul(d, key));
                    const Halves t = mul_split(dh, split(key));
                    got[out] = Halves{add(got[out].e, t.e), add(got[out].o, t.o)};
                }
            }
        }
        for (int out = 0; out < 2; out++) CHECK(join(got[out]) == want[out]);
    }
    return 0;
}

}  // namespace

int main() {
    std::mt19937 g(2048);
    if (check_rotation(g) || check_product(g)) return 1;
    const Poly top(N, 0x7FFFFFFFu), bottom(N, 0x80000000u);
    if (check_step(g, 2, 10, nullptr) || check_step(g, 1, 20, &top) || check_step(g, 1, 20, &bottom)) return 1;
    printf("RING_SPLIT_OK\n");
    return 0;
}
