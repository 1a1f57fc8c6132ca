"""Philox4x32-10 in numpy (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): the host
statement of csrc/philox.h, for the numpy specifications that draw from it (`postprocess.augment_cloud`).

A round maps the counter (c0, c1, c2, c3) under the key (k0, k1) to

    (hi(M1 * c2) ^ c1 ^ k0,  lo(M1 * c2),  hi(M0 * c0) ^ c3 ^ k1,  lo(M0 * c0))

with 32 x 32 -> 64 bit products; the key words grow by W0 / W1 (mod 2^32) after every round; ten rounds.
"""
from __future__ import annotations

import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LOW, _32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, key: int):
    """Counter words c0..c3 (arrays or scalars that broadcast, values < 2^32) and a 64-bit key (k0 = low word, k1 = high word)
    -> the four output words as uint32 arrays of the broadcast shape."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) & _LOW for c in (c0, c1, c2, c3)))
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = np.uint64(key & 0xFFFFFFFF), np.uint64(key >> 32)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                      # both factors < 2^32: the products are exact in uint64
        c0, c1, c2, c3 = (p1 >> _32) ^ c1 ^ k0, p1 & _LOW, (p0 >> _32) ^ c3 ^ k1, p0 & _LOW
        k0, k1 = (k0 + _W0) & _LOW, (k1 + _W1) & _LOW
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))
