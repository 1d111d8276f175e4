"""Host restatement of the device random stream (csrc/ultr_device.h: Philox, u01) and of the key both draws use
(csrc/ultr_feed.h click_draw, csrc/ultr_loss.hip regem_kernel), vectorised over counters with numpy uint64 arithmetic."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
GOLDEN_GAMMA = 0x9E3779B97F4A7C15


def philox4x32(c0, c1, c2, c3, k0, k1, rounds=10):
    """Philox-4x32-10 of the counters (c0, c1, c2, c3) (scalars or arrays, broadcast) under the key (k0, k1): four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in np.broadcast_arrays(c0, c1, c2, c3)]
    ka, kb = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    thirty_two = np.uint64(32)
    for _ in range(rounds):
        p0, p1 = M0 * c[0], M1 * c[2]  # < 2^64: exact in uint64
        n0 = (p1 >> thirty_two) ^ c[1] ^ np.uint64(ka)
        n2 = (p0 >> thirty_two) ^ c[3] ^ np.uint64(kb)
        c = [n0, p1 & MASK, n2, p0 & MASK]
        ka, kb = (ka + W0) & 0xFFFFFFFF, (kb + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def u01(x):
    """The kernels' uniform in [0, 1): the top 24 bits times 2^-24 (exact in float32)."""
    return ((np.asarray(x, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def key(seed, step):
    """(k0, k1) for (seed, step): k0 = lo32(seed) ^ hi32(step * golden gamma mod 2^64), k1 = hi32(seed) ^ lo32(step)."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    mix = (step * GOLDEN_GAMMA) & (2 ** 64 - 1)
    return (seed & 0xFFFFFFFF) ^ (mix >> 32), (seed >> 32) ^ (step & 0xFFFFFFFF)
