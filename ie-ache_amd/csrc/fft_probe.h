// A probe of the 512-point transform (fft512.h) for tests: the twiddle table as a 64-thread kernel builds it, and the transform
// itself in every instantiation a shipped kernel uses, on caller data, with the doubles it produces returned unrounded.  No
// kernel of the library calls anything here and nothing here changes one, but for the switch at the end; tests/test_fft_probe_gpu.py compares the results with
// the defining sums in extended precision (tests/fft_reference.py).  Compiled with the flags of the kernels it stands in for
// (the Makefile's generic %.hip rule: -ffp-contract=on), so that contraction follows the same source expressions.
//
// The forms.  Forward forms take [count][512] complex points y_j = p[j] + i p[j + 512] in natural order; the kernel gathers
// x[r] = y_{64 r + lane} as k_bk_to_spectrum_w64_1 does and returns the registers raw, out[t][k2][lane] = x[k2], which
// fft512_forward documents as X[k0 + 8 k1 + 64 k2] at lane = 8 k0 + k1.  Inverse forms take a spectrum in that layout and return
// out[t][r][lane] = x[r] * untwist_gain(r) = y_{64 r + lane}: the product round_coef is about to round, not the rounded word.
//
//   form  instantiation                                              used by
//   0     fft512_forward<true, 0>                                    k_bk_to_spectrum_w64, k_bk_to_spectrum_w64_1 (key and TGSW
//                                                                    set preparation), k_blind_rotate_wide, the rows of
//                                                                    k_blind_rotate_wide4 without a request
//   1     fft512_forward<true, 1>                                    k_blind_rotate_w2, k_blind_rotate_w2r, k_blind_rotate_w4r
//   2     fft512_forward<true, 1, hook, true>                        the shared step of br_step.h (k_blind_rotate_x1 and the
//                                                                    CMux family: k_cmux / k_demux / k_rotate _x1 and _rt)
//   3     fft512_forward<true, 1, hook, false, LaneRootsResident>    k_blind_rotate_w1b's XLANE = 1 build (the switch at the end)
//   4     fft512_forward<true, 0, hook>                              k_blind_rotate_wide4
//   5     fft512_inverse<true>                                       k_blind_rotate_w2r, _w4r, _wide, _wide4
//   6     fft512_inverse_pair<true>                                  k_blind_rotate_w2, _x1, the CMux family (transforms 2i and
//                                                                    2i + 1 are x and y of one call: count must be even)
//   7     fft512_inverse_pair<true, LaneRootsResident>               k_blind_rotate_w1b's XLANE = 1 build (paired like form 6)
// k_blind_rotate_w1b's default build takes the exchange form, fft512_forward<true, 2, hook, false, LaneRootsExchange>, and the
// paired inverse on those roots (the same arithmetic on table entries): not forms here -- that form's inputs are gathered in
// another lane order -- but checked against form 3's data flow on the host (tests/native/xlane_exchange_test.cpp) and, through
// the kernel, word for word against its XLANE = 1 build (tests/test_xlane_exchange_gpu.py).
// WSYNC = false is instantiated by no kernel and not here.  The hook of forms 2 .. 4 is a global load into a register that is
// stored after the transform, as the kernels' hook requests a key block.
//
// A launch sits as the G = 4 kernels do: four waves per workgroup, one transform (or one pair) per wave, a kTile per wave and one
// twiddle table per workgroup in LDS, copied there with load_twiddles from the context's table.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace ieache {
namespace probe {

constexpr int kForms = 8;
constexpr int kFirstInverseForm = 5, kFirstPairedForm = 6;
constexpr size_t kTransformElems = 512;  // double2 per transform, in and out
constexpr size_t kTwiddleElems = 576;    // w64::kTwElems (tw_roots.h)

// null, or why (form, count) is refused
const char* form_refusal(int form, size_t count);
// d_in, d_out: [count][512] double2 on the device; d_tw: a twiddle table of kTwElems entries.  One launch on `stream`;
// std::invalid_argument where form_refusal() objects.
void run_fft512(int form, size_t count, const double2* d_in, double2* d_out, const double2* d_tw, hipStream_t stream);
// the table build_twiddles(.., lane, 64) leaves in the LDS of a 64-thread kernel (the key-preparation kernels' own) -> d_out
void build_twiddles_in_wave(double2* d_out, hipStream_t stream);

// The one switch of a shipped kernel this header holds: which form of the forward transforms' lane-high transpose the launches
// of k_blind_rotate_w1b's default-guard builds take from here on, in every context of the process -- 2, the exchange form
// (fft512_forward, XLANE = 2: the default), or 1, the v_cndmask form it replaced, built beside it.  Both give the same words;
// the partner of an A/B (the environment's IEACHE_W1B_FORWARD sets the value a process starts with) and of
// tests/test_xlane_exchange_gpu.py.  std::invalid_argument for another value.
void set_w1b_forward_path(int xlane);
int w1b_forward_path();

}  // namespace probe
}  // namespace ieache
