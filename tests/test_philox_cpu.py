"""The host restatement of the device random stream (tests/philox_ref.py) against the published Random123 known answers for
Philox-4x32-10, and the (seed, step) key derivation against plain Python integer arithmetic."""
import numpy as np
import pytest

from tests import philox_ref as P

KAT = [  # Random123 kat_vectors: philox4x32 10 rounds (ctr[4], key[2]) -> out[4]
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_philox_known_answers(ctr, key, out):
    got = P.philox4x32(*ctr, *key)
    assert [int(x) for x in got] == list(out)


def test_philox_is_vectorised_over_counters():
    """An array of counters gives, element by element, what the scalar calls give (the tests draw whole batches at once)."""
    ctr = np.array([0, 1, 0xFFFFFFFF, 0x243F6A88], dtype=np.uint64)
    vec = P.philox4x32(ctr, 7, ctr[::-1], 0x2545F491, 0xA4093822, 0x299F31D0)
    for i, c in enumerate(ctr):
        one = P.philox4x32(int(c), 7, int(ctr[::-1][i]), 0x2545F491, 0xA4093822, 0x299F31D0)
        assert [int(v[i]) for v in vec] == [int(x) for x in one]
    assert all(v.dtype == np.uint32 and v.shape == (4,) for v in vec)


def test_u01_takes_the_top_24_bits():
    x = np.array([0, 0xFF, 0x100, 0x80000000, 0xFFFFFFFF], dtype=np.uint32)
    got = P.u01(x)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got.astype(np.float64), [0.0, 0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24])


@pytest.mark.parametrize("seed,step", [(0, 0), (7, 1), (0x123456789ABCDEF0, 2 ** 32 + 5), (0xFFFFFFFFFFFFFFFF, 2 ** 64 - 1),
                                       (0x00000001FFFFFFFF, 2 ** 32 + 3), (11, 123456789)])
def test_key_derivation_with_high_bits(seed, step):
    mix = (step * 0x9E3779B97F4A7C15) % 2 ** 64
    k0 = (seed % 2 ** 32) ^ (mix // 2 ** 32)
    k1 = (seed // 2 ** 32) ^ (step % 2 ** 32)
    assert P.key(seed, step) == (k0, k1)
    assert 0 <= k0 < 2 ** 32 and 0 <= k1 < 2 ** 32


def test_key_of_a_step_above_2_32_differs_from_its_low_word():
    """A step counter past 2^32 reaches the key through the product's high word: it must not alias the step with the same low word."""
    seed = 0x123456789ABCDEF0
    assert P.key(seed, 2 ** 32 + 5) != P.key(seed, 5)
    assert P.key(seed, 2 ** 32 + 5)[1] == P.key(seed, 5)[1]
