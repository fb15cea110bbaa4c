"""CPU: the Philox4x32-10 restatement (oracle/philox_ref.py) that the device generator of
csrc/sampler.hip is compared with in tests/test_gpu_sampler.py."""
import numpy as np
import pytest

from oracle import philox_ref

# Random123 known-answer vectors for philox4x32 with 10 rounds (kat_vectors of the Random123
# distribution; the third uses the hexadecimal digits of pi)
KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_philox4x32_10_known_answers(ctr, key, out):
    got = philox_ref.philox4x32_10(ctr, key)
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert [int(v) for v in got] == list(out)


def test_philox4x32_10_is_elementwise_over_arrays():
    ctr = [np.array([c[0][i] for c in KAT]) for i in range(4)]
    key = [np.array([c[1][i] for c in KAT]) for i in range(2)]
    got = philox_ref.philox4x32_10(ctr, key)
    assert got.shape == (4, 3)
    np.testing.assert_array_equal(got.T, np.array([c[2] for c in KAT], dtype=np.uint32))


def test_normal_is_shard_invariant_across_a_block_boundary():
    """D = 7: sample boundaries fall inside a 4-element Philox block."""
    full = philox_ref.normal(4, 7, 0, 99, 3, 1)
    assert full.shape == (4, 7) and full.dtype == np.float64
    np.testing.assert_array_equal(philox_ref.normal(2, 7, 0, 99, 3, 1), full[:2])
    np.testing.assert_array_equal(philox_ref.normal(2, 7, 2, 99, 3, 1), full[2:])


def test_normal_block_layout_and_counter_words():
    """The 4 normals of a block are (r0 cos, r0 sin, r1 cos, r1 sin) of the uniforms of the
    block's 4 words; step, draw, both seed words and the high counter word all matter."""
    seed, step, draw = 2 ** 63 + 12345, 7, 2
    q = 2 ** 32 + 5  # q_hi = 1
    z = philox_ref.normal(1, 4, q, seed, step, draw)[0]  # D = 4: sample q is block q
    r = philox_ref.philox4x32_10((q & 0xffffffff, q >> 32, step, draw),
                                 (seed & 0xffffffff, seed >> 32)).astype(np.int64)
    u = [np.float64(np.float32(((int(w) >> 8) + 1) * 2.0 ** -24)) for w in r]
    for k, (ur, ua) in enumerate([(u[0], u[1]), (u[2], u[3])]):
        rad = np.sqrt(-2 * np.log(ur))
        ang = np.float64(np.float32(np.float32(6.283185307179586) * np.float32(ua)))
        assert z[2 * k] == rad * np.cos(ang) and z[2 * k + 1] == rad * np.sin(ang)
    for other in (philox_ref.normal(1, 4, q, seed, step + 1, draw),
                  philox_ref.normal(1, 4, q, seed, step, draw + 1),
                  philox_ref.normal(1, 4, q, seed - 2 ** 63, step, draw),
                  philox_ref.normal(1, 4, q, seed + 1, step, draw),
                  philox_ref.normal(1, 4, q - 2 ** 32, seed, step, draw)):
        assert not np.any(other[0] == z)


def test_normal_moments():
    v = philox_ref.normal(8, 4099, 0, 1, 0, 0).ravel()
    n = v.size
    assert np.abs(v).max() <= 5.77  # sqrt(-2 ln 2^-24) = 5.768
    assert abs(v.mean()) <= 5 / np.sqrt(n)
    assert abs(v.var() - 1) <= 5 * np.sqrt(2 / n)
