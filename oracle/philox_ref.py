"""ORACLE (test infrastructure only) -- the sampler's counter-based Gaussian noise on CPU.

Restates csrc/sampler.hip's generator in numpy: Philox4x32-10 (Salmon et al., "Parallel
random numbers: as easy as 1, 2, 3", SC'11; the Random123 known answers pin it in
tests/test_philox_host.py) and the Box-Muller mapping of one 4-word block onto 4 normals.

The integer part and the float32 uniforms / angle are exact restatements; log, sqrt, sin and
cos are evaluated in float64, so `normal` is the value the device's float32 logf / sqrtf /
sincosf approximate (tests/test_gpu_sampler.py measures by how much).
"""
from __future__ import annotations

import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """Philox4x32 with 10 rounds.  `ctr`: 4 words, `key`: 2 words, each a non-negative
    integer below 2**32 or an array of them (broadcast against each other).  Returns a
    uint32 array of shape [4, ...]."""
    c = [np.asarray(v, dtype=np.uint64) for v in ctr]
    k = [np.asarray(v, dtype=np.uint64) for v in key]
    assert len(c) == 4 and len(k) == 2
    assert all((v <= _MASK).all() for v in c + k), "counter / key words are 32 bits"
    for _ in range(10):
        p0 = _M0 * c[0]  # 32 x 32 -> 64 bit products (no overflow in uint64)
        p1 = _M1 * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ k[0], p1 & _MASK, (p0 >> _S32) ^ c[3] ^ k[1], p0 & _MASK]
        k = [(k[0] + _W0) & _MASK, (k[1] + _W1) & _MASK]
    return np.stack(np.broadcast_arrays(*c)).astype(np.uint32)


def _u01(r):
    """(0, 1] uniform of the top 24 bits, float32 (every step is exact in float32)."""
    return ((r >> np.uint32(8)).astype(np.float32) + np.float32(1.0)) * np.float32(2.0 ** -24)


def normal_at(ge, seed, step, draw):
    """Standard normals of the global element indices `ge` (any shape), float64."""
    ge = np.asarray(ge, dtype=np.uint64)
    seed = int(seed) & (2 ** 64 - 1)
    q = ge >> np.uint64(2)
    r = philox4x32_10((q & _MASK, q >> _S32, int(step) & 0xFFFFFFFF, int(draw) & 0xFFFFFFFF),
                      (seed & 0xFFFFFFFF, seed >> 32))
    two_pi = np.float32(6.283185307179586)
    lane = (ge & np.uint64(3)).astype(np.int64)
    hi = lane >= 2  # r.x, r.y -> elements 0, 1;  r.z, r.w -> elements 2, 3
    u_rad = np.where(hi, _u01(r[2]), _u01(r[0]))
    u_ang = np.where(hi, _u01(r[3]), _u01(r[1]))
    assert u_rad.dtype == np.float32 and u_ang.dtype == np.float32
    ang = (two_pi * u_ang).astype(np.float32).astype(np.float64)  # float32 product
    rad = np.sqrt(-2.0 * np.log(u_rad.astype(np.float64)))
    return np.where((lane & 1) == 0,rad * np.cos(ang), rad * np.sin(ang))


def normal(B, D, sample_offset, seed, step, draw):
    """[B, D] float64: element e of local sample b has the global index
    ge = (sample_offset + b) * D + e, counter (q_lo, q_hi, step, draw) with q = ge >> 2, key
    (seed_lo, seed_hi); the block's 4 normals are (r0 cos, r0 sin, r1 cos, r1 sin) and the
    element takes number ge & 3."""
    b = np.arange(B, dtype=np.uint64)[:, None]
    e = np.arange(D, dtype=np.uint64)[None, :]
    ge = (np.uint64(sample_offset) + b) * np.uint64(D) + e
    return normal_at(ge, seed, step, draw)
