"""Oracle: the Philox4x32-10 noise generator of the sampler (TEST INFRASTRUCTURE — see oracle/__init__.py).

Written from the definition of Philox (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)
and from the noise contract of include/prg.h, in numpy; pinned by the Random123 known-answer vectors
(tests/test_philox_oracle.py).  It shares no code with the device generator or its C++ twin.

Philox4x32 is a 10-round substitution-permutation network on a 4-word counter (c0, c1, c2, c3) with a 2-word key:

    round:   (hi0, lo0) = M0 * c0        (hi1, lo1) = M1 * c2              (32 x 32 -> 64 bit products)
             (c0, c1, c2, c3) <- (hi1 ^ c1 ^ k0,  lo1,  hi0 ^ c3 ^ k1,  lo0)
    between rounds the key is bumped by the Weyl constants: k0 += W0, k1 += W1 (mod 2^32)

Noise contract: image b of a batch is keyed by its 64-bit scene seed (k0 = low word, k1 = high word); the counter of pixels
4q .. 4q+3 of draw d (d = 0: the start image, d = k + 1: transition k) is {q, d, 0x70726721, 0}; the four output words become
two Box-Muller pairs.  The uniforms, and the angle 2*pi*u, are float32 values exactly as the contract states them; from there
on this oracle evaluates log, sqrt, cos and sin in float64, so that it is the exact value the float32 device functions approximate.
"""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # the two round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # Weyl key increments: golden ratio, sqrt(3) - 1
DOMAIN = 0x70726721                      # third counter word of every sampler draw
_MASK = np.uint64(0xFFFFFFFF)
_SH = np.uint64(32)


def philox4x32_10(counter_words, key, rounds: int = 10):
    """counter_words: four uint64 arrays (broadcastable) holding 32-bit words; key: (k0, k1) likewise.
    Returns the four output words as uint64 arrays masked to 32 bits."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _MASK for c in counter_words)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & _MASK for k in key)
    for _ in range(rounds):
        p0 = np.uint64(M0) * c0              # < 2^64: exact in uint64
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> _SH) ^ c1 ^ k0, p1 & _MASK, (p0 >> _SH) ^ c3 ^ k1, p0 & _MASK
        k0 = (k0 + np.uint64(W0)) & _MASK
        k1 = (k1 + np.uint64(W1)) & _MASK
    return c0, c1, c2, c3


def _uniform(c):
    """(float32(c) + 0.5f) * 2^-32, every step rounded to float32 (uint32 -> float32 rounds to nearest even)."""
    return (c.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -32)


def normals(key: int, draw: int, n_pixels: int):
    """Draw `draw` of the scene keyed `key`: (normals, radii), two float64 arrays of n_pixels values.
    radii[i] is the Box-Muller radius of pixel i's pair: |normals[i]| <= radii[i], the scale of its rounding error."""
    assert n_pixels % 4 == 0 and 0 <= draw < 2 ** 32
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    quad = np.arange(n_pixels // 4, dtype=np.uint64)
    zero = np.zeros_like(quad)
    words = philox4x32_10((quad, zero + np.uint64(draw), zero + np.uint64(DOMAIN), zero), (key & 0xFFFFFFFF, key >> 32))
    u0, u1, u2, u3 = (_uniform(w) for w in words)
    two_pi = np.float32(6.283185307179586)

    def radius(u):
        u = np.minimum(np.maximum(u, np.float32(1e-12)), np.float32(1.0))
        return np.sqrt(-2.0 * np.log(u.astype(np.float64)))

    r0, r1 = radius(u0), radius(u2)
    a0, a1 = (two_pi * u1).astype(np.float64), (two_pi * u3).astype(np.float64)     # float32 products, then exact
    n = np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=1).reshape(-1)
    r = np.stack([r0, r0, r1, r1], axis=1).reshape(-1)
    return n, r


def _f32_floor(v):
    """Largest float32 <= v (v float64)."""
    f = v.astype(np.float32)
    return np.where(f.astype(np.float64) > v, np.nextafter(f, np.float32(-np.inf)), f)


def _f32_ceil(v):
    f = v.astype(np.float32)
    return np.where(f.astype(np.float64) < v, np.nextafter(f, np.float32(np.inf)), f)


def start_image_interval(n, r, ulps: float):
    """The sampler returns (x + 1) * 0.5 in float32: one more rounding (of x + 1; the halving is exact), monotone in x.
    [lo, hi] = the images of the smallest and largest float32 x with |x - n| <= ulps * 2^-23 * r: an output outside it cannot
    come from a start image that is within that bound of the oracle's normals."""
    e = ulps * 2.0 ** -23 * np.abs(r)
    lo = (_f32_ceil(n - e) + np.float32(1.0)) * np.float32(0.5)
    hi = (_f32_floor(n + e) + np.float32(1.0)) * np.float32(0.5)
    return lo, hi
