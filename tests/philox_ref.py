"""Philox4x32-10 (Salmon et al., SC'11; the Random123 constants) restated in NumPy with uint64 products, and the start-state stream of
include/hjbx.h built on it: the yardstick of the device sampler (tests/test_device_collection_host.py pins it to the published known
answers)."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter (..., 4), key (..., 2) of 32-bit words (broadcast against each other) -> (..., 4) uint32"""
    c = [np.asarray(counter, np.uint64)[..., i] & MASK for i in range(4)]
    k = [np.asarray(key, np.uint64)[..., i] & MASK for i in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def uniforms(seed, first_row, B, n, dtype):
    """(B, n) uniforms in [0, 1) of rows first_row .. first_row + B - 1 under `seed`, as include/hjbx.h defines them"""
    rows = (np.arange(B, dtype=np.uint64) + np.uint64(first_row))
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)
    per = 4 if np.dtype(dtype) == np.float32 else 2
    out = np.empty((B, n), dtype)
    for g in range((n + per - 1) // per):
        ctr = np.stack([rows & MASK, rows >> np.uint64(32), np.full(B, g, np.uint64), np.zeros(B, np.uint64)], axis=-1)
        w = philox4x32_10(ctr, key).astype(np.uint64)
        for j in range(per):
            if g * per + j < n:
                if per == 4:
                    out[:, g * per + j] = (w[:, j] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
                else:
                    out[:, g * per + j] = (((w[:, 2 * j] >> np.uint64(5)) << np.uint64(26)) + (w[:, 2 * j + 1] >> np.uint64(6))).astype(np.float64) * 2.0 ** -53
    return out
