"""The library's random function (gpmp2_amd/csrc/rng.h, include/gpmp2mi.h "seeding") restated in numpy: Philox4x32-10
with the Random123 constants, the packing of (stream, a, b, i, r) into the counter, the pairing of coordinates and
Box-Muller in float64.  Everything broadcasts over arrays of arguments.

    key     = (seed & 0xffffffff, seed >> 32)
    counter = (a, b, i, stream << 8 | pair),   pair = (r & 3) + 4 (r >> 3);  r is the cosine member when bit 2 of r
              is clear, the sine member (of the pair of r - 4) when it is set
    hi53 = o0 << 21 | o1 >> 11,  lo53 = o2 << 21 | o3 >> 11,  u1 = (hi53 + 1) 2^-53,  u2 = lo53 2^-53
    z = sqrt(-2 ln u1) (cos | sin)(2 pi u2)

A plain module like posterior_reference.py; tests/test_rng_cpu.py holds it to the known answers and to rng.h itself.
"""
from __future__ import annotations

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
RESTARTS, POSTERIOR = 1, 2
ZMAX = float(np.sqrt(106 * np.log(2.0)))


def _u64(x):
    return np.asarray(x).astype(np.uint64)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """ten rounds on uint32 words held in uint64 arrays -> (o0, o1, o2, o3) as uint64 arrays below 2^32"""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[_u64(x) & MASK for x in (c0, c1, c2, c3, k0, k1)])
    for rnd in range(10):
        p0, p1 = M0 * c0, M1 * c2
        n0, n2 = (p1 >> S32) ^ c1 ^ k0, (p0 >> S32) ^ c3 ^ k1
        c0, c1, c2, c3 = n0, p1 & MASK, n2, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return c0, c1, c2, c3


def pair_of(r):
    r = np.asarray(r)
    return (r & 3) + 4 * (r >> 3)


def is_sine(r):
    return (np.asarray(r) >> 2) & 1


def counter(stream, a, b, i, r):
    """the four counter words of the block that coordinate r of block i of problem (a, b) reads"""
    return _u64(a), _u64(b), _u64(i), (_u64(stream) << np.uint64(8)) | _u64(pair_of(r))


def block(seed, stream, a, b, i, r):
    """the 128-bit block output as four uint64 arrays"""
    seed = np.asarray(seed, dtype=np.uint64)
    return philox4x32_10(*counter(stream, a, b, i, r), seed & MASK, seed >> S32)


def uniforms(o):
    """block output -> (hi53, lo53) as uint64 and (u1, u2) as float64"""
    hi = (o[0] << np.uint64(21)) | (o[1] >> np.uint64(11))
    lo = (o[2] << np.uint64(21)) | (o[3] >> np.uint64(11))
    return hi, lo, (hi + np.uint64(1)).astype(np.float64) * 2.0 ** -53, lo.astype(np.float64) * 2.0 ** -53


def normal(seed, stream, a, b, i, r):
    _, _, u1, u2 = uniforms(block(seed, stream, a, b, i, r))
    rad, ang = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586476925286766559 * u2
    return np.where(is_sine(r) == 1, rad * np.sin(ang), rad * np.cos(ang))


def normal_fill(seed, stream, a_first, a_count, b_first, b_count, nblk, n):
    """out [a_count][b_count][nblk][n], as gpmp2mi_normal_fill"""
    a = (a_first + np.arange(a_count))[:, None, None, None]
    b = (b_first + np.arange(b_count))[None, :, None, None]
    i = np.arange(nblk)[None, None, :, None]
    r = np.arange(n)[None, None, None, :]
    return np.ascontiguousarray(normal(seed, stream, a, b, i, r))
