"""Linear layers on encrypted rows (include/ieache.h section 3n) restated in numpy: an int64 product and a mask.  With weights
of magnitude <= 2^7, words below 2^32 and n_in <= 2^16 a sum stays below 2^55 < 2^63, so the int64 arithmetic is exact and
`& 0xFFFFFFFF` is the definition's mod 2^32.  Also here: the crafted words and weights that carry through every byte limb of
the MFMA kernel.  Test support only."""
import numpy as np

KINDS = ("lwe", "extracted", "tlwe")


def words_of(n, N, rows):
    return {"lwe": n + 1, "extracted": N + 1, "tlwe": 2 * N}[rows]


def stride_of(n, N, rows):
    """words from a device row to the next: lwe_stride, extract_stride, 2N"""
    return {"lwe": (n + 4) & ~3, "extracted": N + 4, "tlwe": 2 * N}[rows]


def bias_word(n, N, rows):
    return {"lwe": n, "extracted": N, "tlwe": None}[rows]


def wrap32(a):
    return (np.asarray(a, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def full_range(rng, shape):
    return rng.integers(-(1 << 31), 1 << 31, size=shape, dtype=np.int64).astype(np.int32)


def linear(x, W, bias=None, at=None):
    """x [batch][n_in][words] int32, W [n_out][n_in] integers, bias [n_out] words added to word `at` -> [batch][n_out][words]"""
    x = np.asarray(x, dtype=np.int32).astype(np.int64)
    W = np.asarray(W).astype(np.int64)
    out = np.matmul(W[None], x)  # [batch][n_out][words], exact in int64
    if bias is not None:
        out[:, :, at] += np.asarray(bias, dtype=np.int64)[None, :]
    return wrap32(out)


# every balanced limb at -128, every limb at +127, the offset itself (all limbs 0 but for the carry out of the top), all ones,
# a word whose bytes 7F, FF, 80, 00 mix an extreme, a borrow and a carry into the top limb, and the sign bit alone
CRAFTED_WORDS = (0x7F7F7F80, 0x7F7F7F7F, 0x80808080, 0xFFFFFFFF, 0x0080FF7F, 0x80000000)


def balanced_limbs(v):
    """the four limbs b_k in [-128, 127] with v = sum b_k 2^(8k) mod 2^32, by the kernel's identity"""
    u = ((int(v) + 0x80808080) & 0xFFFFFFFF) ^ 0x80808080
    return [((u >> (8 * k)) & 0xFF) - 256 * ((u >> (8 * k + 7)) & 1) for k in range(4)]


def crafted_rows(rng, shape):
    """rows [..][words] whose words are drawn from CRAFTED_WORDS, with a random word in between now and then"""
    pick = rng.integers(0, len(CRAFTED_WORDS) + 1, size=shape)
    table = np.array(CRAFTED_WORDS + (0,), dtype=np.uint32).view(np.int32)
    return np.where(pick == len(CRAFTED_WORDS), full_range(rng, shape), table[pick]).astype(np.int32)


def constant_rows(word, shape):
    return np.full(shape, np.array([word], dtype=np.uint32).view(np.int32)[0], dtype=np.int32)


def asymmetric_rows(batch, n_in, words):
    """x[b][j][w] = a word that names its place: no symmetry between j and w, every byte limb in use"""
    b, j, w = np.meshgrid(np.arange(batch), np.arange(n_in), np.arange(words), indexing="ij")
    return wrap32((b * 0x01000193 + j * 0x00010101 + w * 0x9E3779B1 + (j * j + 3 * w) * 0x811C9DC5))


def weight_cases(rng, n_out, n_in):
    """name -> int8 matrix: full range with the extremes planted, rows of zeros, the identity (padded with zero rows / columns
    when not square), single ones at the four corners, all -128, all +127"""
    full = rng.integers(-128, 128, size=(n_out, n_in)).astype(np.int8)
    full[0, 0], full[-1, -1] = -128, 127
    full[0, -1], full[-1, 0] = 127, -128
    zero_rows = full.copy()
    zero_rows[::2] = 0
    eye = np.eye(n_out, n_in, dtype=np.int8)
    corners = np.zeros((n_out, n_in), dtype=np.int8)
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = 1
    if n_out > 1 and n_in > 1:
        corners[0, -1], corners[-1, 0] = 2, 3  # a transposition moves them
    return {"full": full, "zero_rows": zero_rows, "identity": eye, "corners": corners,
            "min": np.full((n_out, n_in), -128, dtype=np.int8), "max": np.full((n_out, n_in), 127, dtype=np.int8)}
