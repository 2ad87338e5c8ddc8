"""The counter-based noise of the Social-GAN sampler (csrc/fot_noise.hpp) restated in NumPy, for the tests that hold the
CPU emulation and ``fot_sgan_noise`` against it: Philox4x32-10 on arrays of counters, the uniform and Box-Muller maps, and
the noise tensor [S, rows, noise_dim] of given row tables (slot, step, index within the slot)."""
import numpy as np

RAW, UNIFORM, GAUSSIAN, UNIFORM_SYM = 0, 1, 2, 3
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)

# counter / key -> output (Random123's known-answer tests of philox4x32_10)
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Arrays (any common shape) of uint32 counters and keys -> uint32 [..., 4]."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(np.asarray(v).astype(np.uint64) & MASK for v in (c0, c1, c2, c3, k0, k1)))
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def uniform(words):
    """[0, 1): (x >> 8) 2^-24, exact in float32."""
    return ((np.asarray(words, np.uint32) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def gaussian(words):
    """Box-Muller on the pairs (x0, x1), (x2, x3) of the last axis (length 4), in float64, rounded once to float32."""
    w = np.asarray(words, np.uint32)
    u1 = ((w[..., 0::2] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (w[..., 1::2] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    a = 6.283185307179586 * u2
    out = np.empty(w.shape, np.float64)
    out[..., 0::2], out[..., 1::2] = r * np.cos(a), r * np.sin(a)
    return out.astype(np.float32)


def noise(seed, kind, S, slot, step, index, noise_dim):
    """The tensor fot_sgan_noise writes: [S, rows, noise_dim], uint32 for RAW and float32 otherwise; row r belongs to index
    ``index[r]`` of slot ``slot[r]`` at that slot's step ``step[r]``."""
    slot, step, index = (np.asarray(v, np.int64) for v in (slot, step, index))
    rows, nb = len(slot), (noise_dim + 3) // 4
    s = np.arange(S, dtype=np.int64)[:, None, None]
    b = np.arange(nb, dtype=np.int64)[None, None, :]
    c1 = (index[None, :, None] | (s << 16)) & 0xFFFFFFFF
    words = philox4x32_10(b, c1, step[None, :, None] & 0xFFFFFFFF, slot[None, :, None] & 0xFFFFFFFF,
                          int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)        # [S, rows, nb, 4]
    if kind == RAW:
        vals = words
    elif kind == UNIFORM:
        vals = uniform(words)
    elif kind == UNIFORM_SYM:
        vals = (uniform(words) - np.float32(0.5)) * np.float32(2.0)
    elif kind == GAUSSIAN:
        vals = gaussian(words)
    else:
        raise ValueError(f"unknown kind {kind}")
    return np.ascontiguousarray(vals.reshape(S, rows, nb * 4)[:, :, :noise_dim])


def ulp_distance(a, b):
    """Distance of two float32 arrays in units in the last place (finite values), as int64."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def write_emu_noise_case(path, seed, kind, S, slot, step, index, noise_dim):
    with open(path, "wb") as f:
        f.write(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF).tobytes())
        f.write(np.array([kind, S, len(slot), noise_dim], np.int32).tobytes())
        for t in (slot, step, index):
            f.write(np.ascontiguousarray(t, np.int32).tobytes())
