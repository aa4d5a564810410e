// Host-side (CPU) TFHE primitives the Cloud path needs around the GPU
// evaluator: key generation, LWE encryption/decryption of single bits, and
// the trivial gates.  These are what the reference gets from libtfhe in
// Keygen/keygen.c:22-51 (new_random_gate_bootstrapping_secret_keyset),
// Client1/alice.c:116-149 (bootsSymEncrypt) and Cloud/cloud.c:709-713,
// 822-824 (bootsSymDecrypt / bootsSymEncrypt of the metadata words).
// None of this is on the bootstrapped-gate hot path.
#pragma once
#include "linear_plan.h"
#include "params.h"

namespace ieache {

// Two generators behind one interface:
//  * seeded: xoshiro256** seeded through splitmix64 from a list of 32-bit seed words (the
//    reference seeds libtfhe with {314,1592,657} / {314,1592,888}, Keygen/keygen.c:30,34; our
//    generator is documented, not libtfhe's).  Reproducible, NOT cryptographic: for test
//    vectors and for mirroring keygen.c's fixed seeds only.
//  * Rng::secure(): a ChaCha20 key stream keyed from the kernel (getrandom(2)).  Used wherever
//    fresh ciphertexts leave the process (the metadata words main() re-encrypts under the nbit
//    key, cloud.c:822-824, 837-839) and by the tools when no seed is given.
class Rng {
public:
    Rng(const uint32_t* seed_words, int count, uint64_t stream = 0);
    explicit Rng(uint64_t seed) : Rng(nullptr, 0, seed) {}
    static Rng secure();  // throws std::runtime_error when the kernel gives no entropy
    uint64_t next();
    Torus32 uniform_torus32() { return (Torus32)(uint32_t)(next() >> 32); }
    int32_t bit() { return (int32_t)(next() >> 63); }
    double uniform01();  // (0,1]
    double gaussian(double sigma);
    // libtfhe gaussian32(0, sigma): noise on the torus
    Torus32 gaussian_torus32(double sigma);

private:
    void chacha_refill();
    uint64_t s_[4];
    bool have_spare_ = false;
    double spare_ = 0;
    bool chacha_ = false;
    uint32_t key_[8] = {0}, nonce_[3] = {0};
    uint64_t counter_ = 0;
    uint64_t buf_[8];
    int buf_pos_ = 8;
};

// Full key generation (secret + cloud key).  with_cloud=false skips BK/KSK.
// nseed >= 0: reproducible from the seed words (keygen.c:30,34 uses fixed ones);
// nseed < 0: all randomness from Rng::secure().
void keygen(const Params& p, const uint32_t* seed_words, int nseed, SecretKeyData* out,
            bool with_cloud = true);

// TLWE samples under the ring key, [k+1][N]: polynomials a_0 .. a_{k-1}, then b; phase b - sum a_c s_c, negacyclic mod 2^32.
// tlwe_encrypt_zero: a uniform, b = a s + e with e Gaussian of standard deviation alpha -- what key generation makes a row of
// the bootstrapping key from, in its order of draws.  tlwe_encrypt: the same plus polys[i] on b, `count` samples one after
// another from one generator.  tlwe_phase: the exact phase of each sample -> [count][N].
void tlwe_encrypt_zero(const Params& p, const int32_t* tlwe_key, double alpha, Rng& rng, Torus32* sample);
void tlwe_encrypt(const Params& p, const int32_t* tlwe_key, const Torus32* polys, size_t count, double alpha, Rng& rng, Torus32* out);
void tlwe_phase(const Params& p, const int32_t* tlwe_key, const Torus32* samples, size_t count, Torus32* phase);

// Packing key switch (LWE rows -> TLWE samples; include/ieache.h section 3e states the definition).  packing_keygen:
// out [n][t][2][N], PK[i][j] = tlwe_encrypt_zero + the constant polynomial lwe_key[i] 2^(32 - (j+1) basebit), rows one after
// another from one generator.  pack_reference: the definition on raw arrays, rows [groups m][n+1] -> out [groups][2][N]; the
// caller has checked (t, basebit) and (m, spread, shift) (pack_plan.h).
void packing_keygen(const Params& p, const int32_t* lwe_key, const int32_t* tlwe_key, int32_t t, int32_t basebit, double alpha, Rng& rng,
                    Torus32* out);
void pack_reference(const Params& p, int32_t t, int32_t basebit, const Torus32* pk, size_t groups, int32_t m, int32_t spread, int32_t shift,
                    const Torus32* rows, Torus32* out);

// TGSW samples and the CMux (include/ieache.h section 3f states the definitions).  tgsw_encrypt_sample: out [2l][2][N], 2l rows
// of tlwe_encrypt_zero one after another, then mu 2^(32 - (q+1) Bgbit) on coefficient 0 of polynomial `bloc` of row bloc l + q:
// the routine keygen() makes BK_i with (mu = the key bit), so a seeded key is word for word what it was.
// cmux_reference: out[r] = d0[r] + set[sel] [.] (d1[r] - d0[r]), sel = sel_of[r] (null: r mod n_set), d0 null = zeros.
// lut_tree_reference: item i folds tables[table_of[i]] (null: 0) of 2^depth rows by the selectors sel_of[i depth + k]
// (null: (i depth + k) mod n_set), LSB first.  Raw arrays, indices already checked by the caller.
void tgsw_encrypt_sample(const Params& p, const int32_t* tlwe_key, int32_t mu, double alpha, Rng& rng, Torus32* out);
void cmux_reference(const Params& p, const Torus32* set, size_t n_set, size_t count, const int32_t* sel_of, const Torus32* d1, const Torus32* d0,
                    Torus32* out);
void lut_tree_reference(const Params& p, const Torus32* set, size_t n_set, size_t count, int32_t depth, const int32_t* sel_of,
                        const Torus32* tables, const int32_t* table_of, Torus32* out);
// lut_scatter_reference (section 3g): item i splits values[i] from the most significant selector down -- a row p at position j
// becomes hi = C_k [.] p at 2 j + 1 and p - hi at 2 j -- and out[i][j] = mem[i][j] + leaf j (mem null: zeros),
// [count][2^depth][2][N].  out may be mem itself.  Indices already checked by the caller.
void lut_scatter_reference(const Params& p, const Torus32* set, size_t n_set, size_t count, int32_t depth, const int32_t* sel_of,
                           const Torus32* values, const Torus32* mem, Torus32* out);

// tlwe_rotate_reference (section 3h): row r goes through acc <- acc + C_t [.] (X^(a_t) acc - acc) for t = 0 .. steps-1, C_t =
// set[sel_of[r steps + t]] (null: (r steps + t) mod n_set), a_t = amount_of[t] (null: 2N - 2^t, 0 once 2^t reaches 2N).  out may
// be `in`.  lut_read_reference: the tree by selectors steps .. steps+depth-1 of each item's depth + steps, the rotation of the
// selected row by selectors 0 .. steps-1, coefficient `coef` extracted, and keyswitch_reference (lweKeySwitch on raw arrays:
// u [count][N+1] -> out [count][n+1], ksk [N][t][base][n+1]) unless ksk is null: then out is the extracted rows [count][N+1].
// Indices and amounts already checked by the caller.
void tlwe_rotate_reference(const Params& p, const Torus32* set, size_t n_set, size_t count, int32_t steps, const int32_t* sel_of,
                           const int32_t* amount_of, const Torus32* in, Torus32* out);
void keyswitch_reference(const Params& p, const Torus32* ksk, size_t count, const Torus32* u, Torus32* out);
void lut_read_reference(const Params& p, const Torus32* set, size_t n_set, const Torus32* ksk, size_t count, int32_t depth, int32_t steps,
                        const int32_t* sel_of, const int32_t* amount_of, const Torus32* tables, const int32_t* table_of, int32_t coef,
                        Torus32* out);

// lut_add_reference (section 3j), the three references above composed and summed: w_i = the rotation of values[i] by selectors
// 0 .. steps-1 of item i's depth + steps with amounts a_t (null: +2^t mod 2N, the write's direction), leaves_i = the scatter of
// w_i by selectors steps .. steps+depth-1 with no memory, out[m][j] = mems[m][j] + the sum of leaves_i[j] over the items with
// mem_of[i] = m (mems null: zeros; mem_of null: memory 0).  mems and out [n_mems][2^depth][2][N]; out may be mems itself.
// Indices and amounts already checked by the caller.
void lut_add_reference(const Params& p, const Torus32* set, size_t n_set, size_t count, int32_t depth, int32_t steps, const int32_t* sel_of,
                       const int32_t* amount_of, const Torus32* values, const Torus32* mems, size_t n_mems, const int32_t* mem_of, Torus32* out);

// automaton_reference (section 3k), composed from cmux_reference: per item V_steps = finals[final_of[i]] (null: 0) and for
// t = steps-1 .. 0 one flat cmux_reference call over the `states` rows of the step -- d1 = V_{t+1}[next1[t][q]], d0 =
// V_{t+1}[next0[t][q]], every row with the sample sel_of[i steps + t] (null: (i steps + t) mod n_set) -> out[i] = V_0[0 .. n_out).
// Every state of every step is computed: no liveness, no copies.  Tables and indices already checked by the caller.
void automaton_reference(const Params& p, const Torus32* set, size_t n_set, int32_t states, int32_t steps, int32_t n_out, const int32_t* next0,
                         const int32_t* next1, size_t count, const int32_t* sel_of, const Torus32* finals, const int32_t* final_of, Torus32* out);

// A linear layer (include/ieache.h section 3n) on packed host rows of r.words words: out[b][i][w] = sum_j W[i][j] x[b][j][w]
// (+ bias[i] on r.bias_word; bias null: none) with 32-bit wrap-around, the definition as it reads.  Checked by the caller
// (linear_call_error).
void lwe_linear_reference(const LinearRows& r, size_t batch, int32_t n_out, int32_t n_in, const int8_t* w, const int32_t* bias, const Torus32* x,
                          Torus32* out);

// coefficient coef_of[r] (null: 0; checked by the caller) of tlwe [count][2][N] as extracted rows u [count][N+1]
void tlwe_extract_reference(const Params& p, size_t count, const Torus32* tlwe, const int32_t* coef_of, Torus32* u);

// The projection and the replace write of a window (include/ieache.h section 3l), the references above composed; the caller has
// checked the decomposition, the window and the scalars (project_plan.h) and the indices.  tlwe_project_reference: per sample
// tlwe_extract_reference of coefficients first .. first + width - 1, then pack_reference on the parameter set with n := N
// (pk [N][t][2][N], the projection key) as one group of `width` rows, spread 1, shift dest -> out [count][2][N], not `in`.
// lut_write_coef_reference: old_i = the tree over item i's own memory by selectors steps .. steps+depth-1, rotated by selectors
// 0 .. steps-1 with amounts 2N - unit 2^t and projected onto (0, width, 0); delta_i = fresh_i - old_i; out = lut_add_reference of
// delta with amounts +unit 2^t, memory i for item i.  mem and out [count][2^depth][2][N]; out may be mem itself.
void tlwe_project_reference(const Params& p, int32_t t, int32_t basebit, const Torus32* pk, size_t count, int32_t first, int32_t width, int32_t dest,
                            const Torus32* in, Torus32* out);
void lut_write_coef_reference(const Params& p, const Torus32* set, size_t n_set, int32_t t, int32_t basebit, const Torus32* pk, size_t count,
                              int32_t depth, int32_t steps, int32_t width, int32_t unit, const int32_t* sel_of, const Torus32* fresh, const Torus32* mem,
                              Torus32* out);

// The way back to the gates (include/ieache.h section 3m), the references above composed; the caller has checked the window,
// the scalars and the indices (unpack_plan.h).  unpack_reference: row (i, q) of out = tlwe_extract_reference of coefficient
// first + q spread of in[i], then keyswitch_reference -> out [count][width][n+1]; ksk null: the extracted rows [count][width][N+1].
// word_read_reference: lut_read_reference's tree and rotation with the amounts 2N - unit 2^t, then unpack_reference of the
// window (0, width, 1) of the rotated rows.
void unpack_reference(const Params& p, const Torus32* ksk, size_t count, int32_t first, int32_t width, int32_t spread, const Torus32* in, Torus32* out);
void word_read_reference(const Params& p, const Torus32* set, size_t n_set, const Torus32* ksk, size_t count, int32_t depth, int32_t steps, int32_t width,
                         int32_t unit, const int32_t* sel_of, const Torus32* tables, const int32_t* table_of, Torus32* out);

// bootsSymEncrypt / bootsSymDecrypt on raw samples (int32[n+1]).
void lwe_encrypt_bit(const Params& p, const int32_t* lwe_key, int bit, Rng& rng, Torus32* out);
Torus32 lwe_phase(const Params& p, const int32_t* lwe_key, const Torus32* sample);
inline int lwe_decrypt_bit(const Params& p, const int32_t* lwe_key, const Torus32* sample) {
    return lwe_phase(p, lwe_key, sample) > 0;
}

// libtfhe modSwitchFromTorus32 / modSwitchToTorus32
int32_t modswitch_from_torus32(Torus32 phase, int32_t Msize);
Torus32 modswitch_to_torus32(int32_t mu, int32_t Msize);

}  // namespace ieache
