#!/usr/bin/env python3
"""How many replace writes of a window a levelled memory takes, measured on the CPU reference alone
(tools.lut_write_coef_reference; no GPU): a depth-4 memory of 16 x 1 024 client-encrypted multiples of 1/64, successive writes
of client-encrypted words of `width` coefficients at random encrypted (slot, word) addresses with fresh selectors each time,
N = 1024, TGSW and TLWE noise 2^-25, the projection key at (8, 2); the selectors at the key's gadget (3, 7) and at (6, 5).
After every write the largest distance of any coefficient of any slot from the plaintext memory is taken; the record is the
series and the first write after which it exceeds the decoding condition 2^-8.

    python scripts/project_noise.py [--writes 64] [--steps 5] [--width 32]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--writes", type=int, default=64)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--width", type=int, default=32)
    a = ap.parse_args()

    import ieache_amd as ia
    from ieache_amd import tools
    base = ia.default_params()
    k = tools.keygen_raw(base, (1, 2, 3), with_cloud=False)
    key, N, bits = k["tlwe_key"], base.N, a.depth + a.steps
    pk = tools.projection_keygen(base, key, seed=71)
    print("depth %d, steps %d, width %d (unit = width): largest phase error over the whole memory after write w; bound 2^-8 = %.3e" % (a.depth, a.steps, a.width, 2.0 ** -8))
    for gadget in ((3, 7), (6, 5)):
        p = tools.with_gadget(base, *gadget)
        rng = np.random.default_rng(5)
        plain = rng.integers(-32, 32, size=(1 << a.depth, N)) << 26
        mem = tools.tlwe_encrypt(p, key, plain.astype(np.int32), 171)[None]
        series, crossed = [], None
        for w in range(a.writes):
            addr = int(rng.integers(0, 1 << bits))
            slot, word = addr >> a.steps, addr & ((1 << a.steps) - 1)
            msg = np.zeros((1, N), dtype=np.int64)
            msg[0, :a.width] = rng.integers(-32, 32, size=a.width) << 26
            new = tools.tlwe_encrypt(p, key, msg.astype(np.int32), 191 + w)
            samples = tools.tgsw_encrypt(p, key, [(addr >> t) & 1 for t in range(bits)], 181 + w)
            mem = tools.lut_write_coef_reference(p, samples, pk, mem, a.depth, a.steps, new, width=a.width)
            plain[slot, word * a.width:(word + 1) * a.width] = msg[0, :a.width]
            phase = tools.tlwe_phase(p, key, mem[0]).astype(np.int64)
            d = (phase - plain) & 0xFFFFFFFF
            err = float(np.minimum(d, (1 << 32) - d).max()) / 2.0 ** 32
            series.append(err)
            if crossed is None and err >= 2.0 ** -8:
                crossed = w + 1
        marks = [w for w in (1, 2, 4, 8, 12, 16, 24, 32, 48, 64, 96, 128) if w <= a.writes]
        print("(%d, %d): %s; first write after which the memory exceeds 2^-8: %s"
              % (gadget + (", ".join("w=%d %.2e" % (w, series[w - 1]) for w in marks), crossed if crossed else "none in %d" % a.writes)))


if __name__ == "__main__":
    main()
