"""The parameter sets the lattice tests run: one list, shared by tests/test_param_lattice_cpu.py (which pins the oracle at
them against np_tfhe.np_bootstrap) and tests/test_param_lattice_gpu.py (which compares the kernels with the oracle).

Params::supported() (csrc/params.h) admits k = 1, N = 16 .. 1024, any l x Bgbit <= 32 with 2l x N x 2^Bgbit <= 2^32 (the
two-limb product's exactness bound, tests/test_rounding_model_cpu.py), and any ks_t x ks_basebit < 32 with ks_basebit <= 4."""
import numpy as np

KS_DECOMPS = [(8, 2), (4, 2), (16, 1), (31, 1), (5, 3), (10, 3), (7, 4), (1, 4)]  # (ks_t, ks_basebit)
BR_DECOMPS = [(1, 8), (1, 16), (2, 16), (4, 8), (6, 5), (3, 10), (16, 2)]           # (l, Bgbit)
BR_RINGS = (16, 32, 128, 512)
BR_DECOMPS_1024 = [(4, 8), (2, 8)]  # not br_supported(): the generic kernel without force_generic; (4, 8) needs > 64 KiB of LDS


def br_exact(l, Bgbit, N):
    """Params::br_exact(), restated."""
    return Bgbit < 32 and 2 * l * N * (1 << Bgbit) <= 1 << 32


def largest_bgbit(N):
    """The largest Bgbit supported() keeps on a ring of degree N (l = 1)."""
    return max(b for b in range(1, 33) if br_exact(1, b, N))


# whole gates: an unusual (l, Bgbit) with an unusual (ks_t, ks_basebit), n % 4 == 3 (no padding column in an output row)
GATE_SETS = [  # (n, N, l, Bgbit, ks_t, ks_basebit)
    (7, 32, 4, 8, 5, 3),
    (3, 16, 1, 16, 15, 2),
    (7, 64, 2, 16, 7, 4),
    (3, 32, 32, 1, 31, 1),
    (11, 128, 3, 10, 4, 2),
    (7, 64, 6, 5, 10, 3),
]

# sets outside supported(): every one must be refused before a kernel is launched
REFUSED_SETS = [  # (N, l, Bgbit, ks_t, ks_basebit)
    (32, 1, 32, 1, 1),              # Bgbit = 32: the digit mask is undefined, and the oracle and np_tfhe disagree there
    (16, 1, 28, 8, 2), (32, 1, 27, 8, 2), (128, 1, 25, 8, 2), (512, 1, 23, 8, 2), (1024, 1, 22, 8, 2),  # one Bgbit past the bound
    (64, 3, 11, 8, 2),              # l x Bgbit = 33
    (64, 3, 7, 16, 2), (64, 3, 7, 32, 1), (64, 3, 7, 2, 5),  # ks_t x ks_basebit = 32, ks_basebit = 5
]


def cpu_sets():
    """(n, N, l, Bgbit, ks_t, ks_basebit) on toy rings for every decomposition the GPU file uses."""
    sets = [(5, 64, 3, 7, t, bb) for t, bb in KS_DECOMPS]
    sets += [(5, 32, l, B, 8, 2) for l, B in BR_DECOMPS + BR_DECOMPS_1024 + [(2, 10)]]
    sets += [(3, N, 1, largest_bgbit(N), 8, 2) for N in (16, 32, 64, 128)]
    sets += [(3, 64, 1, largest_bgbit(512), 8, 2)]
    sets += GATE_SETS
    sets += [(5, 64, 2, 16, 7, 4), (4, 32, 32, 1, 31, 1), (9, 128, 3, 10, 4, 2)]
    return sets


def edge_rows(rng, N, t, bb, rows):
    """[rows + 4][N + 1] extracted samples for the key switch: `rows` random ones, then the two edge rows of
    test_keyswitch_stage_bit_exact (all zero: only the rounding offset, which reaches no digit; a_i = -prec_offset: a_i + offset
    wraps to 0), a row whose every digit is base - 1, and a row of 0xFFFFFFFF (the rounding offset carries out of the top)."""
    u = rng.integers(-2 ** 31, 2 ** 31, size=(rows + 4, N + 1), dtype=np.int64).astype(np.int32)
    u[rows, :N] = 0
    u[rows + 1, :N] = -(1 << (32 - (1 + bb * t)))
    u[rows + 2, :N] = (((1 << (bb * t)) - 1) << (32 - bb * t)) - (1 << 32)  # the top bb x t bits set, nothing below them
    u[rows + 3, :N] = -1
    return u
