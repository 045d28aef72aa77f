"""numpy restatement of the device noise generator (csrc/misc.hip: philox4, u01, rng_fill_kernel).

Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the known-answer vectors of the Random123
distribution pin `philox4x32_10` in tests/test_philox_cpu.py) with this project's counter layout: element i of a fill comes from
word i % 4 of the block whose counter is (i // 4 low, i // 4 high, stream id low, step low) and whose key is the seed mixed with
the high halves of the step and of the stream id. Checkpoints store the step; `--resume` continues the same sequence.
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32, MASK64 = (1 << 32) - 1, (1 << 64) - 1
U01_MAX = np.float32(1.0 - 2.0 ** -24)   # the largest float below 1


def philox4x32_10(ctr, key):
    """ctr: 4 uint32 arrays (or ints) of one shape, key: 2 ints. Returns the 4 output words as uint32 arrays."""
    c = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) for w in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    lo32 = np.uint64(MASK32)
    sh = np.uint64(32)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]   # 32 x 32 -> 64 bit products: no overflow in uint64
        c = [(p1 >> sh) ^ c[1] ^ np.uint64(k0), p1 & lo32, (p0 >> sh) ^ c[3] ^ np.uint64(k1), p0 & lo32]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return [w.astype(np.uint32) for w in c]


def raw_words(n, seed, offset, stream_id):
    """The n raw 32-bit draws of rng_fill(n elements, seed, step counter `offset`, call site `stream_id`), flat element order."""
    seed, offset, stream_id = int(seed) & MASK64, int(offset) & MASK64, int(stream_id) & MASK64
    blocks = np.arange((n + 3) // 4, dtype=np.uint64)
    key = seed ^ (offset >> 32 << 32) ^ (stream_id >> 32)
    out = philox4x32_10((blocks & np.uint64(MASK32), blocks >> np.uint64(32), stream_id & MASK32, offset & MASK32),
                        (key & MASK32, key >> 32))
    return np.stack(out, axis=1).reshape(-1)[:n]


def u01(r):
    """uint32 -> float32 in [2^-25, 1 - 2^-24]: ((r >> 8) + 0.5) * 2^-24 in fp32, clamped below 1. Without the clamp the one input
    r >> 8 = 0xFFFFFF gives exactly 1.0: 16777215.5 is a tie in fp32 and rounds to 16777216."""
    v = ((np.asarray(r, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    return np.minimum(v, U01_MAX)


def uniform(r, lo, hi):
    """float32 lo + (hi - lo) * u01, multiply and add rounded separately (the library is built without contraction)."""
    lo, hi = np.float32(lo), np.float32(hi)
    return (lo + (hi - lo) * u01(r)).astype(np.float32)


def keep_drop(r, keep_prob, value):
    """`value` where u01 < keep_prob, else 0 (Dropout2d keep masks)."""
    return np.where(u01(r) < np.float32(keep_prob), np.float32(value), np.float32(0)).astype(np.float32)


def normal(r):
    """Box-Muller over each block of four words, in float64 from the fp32 uniforms: (ra cos a, ra sin a, rb cos b, rb sin b) with
    ra = sqrt(-2 log u0), a = 2 pi u1, rb = sqrt(-2 log u2), b = 2 pi u3. A tail of fewer than four words is computed from the full
    block, as the kernel does, so `r` must hold whole blocks: pass raw_words(4 * ceil(n / 4), ...) and cut the result."""
    u = u01(r).astype(np.float64).reshape(-1, 4)
    ra, rb = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    a, b = 2.0 * np.pi * u[:, 1], 2.0 * np.pi * u[:, 3]
    return np.stack((ra * np.cos(a), ra * np.sin(a), rb * np.cos(b), rb * np.sin(b)), axis=1).reshape(-1)


def fill(n, kind, lo, hi, seed, offset, stream_id):
    """What kernels.rng_fill(out of n elements, kind, lo, hi, seed, offset, stream_id) writes ('normal': in float64)."""
    if kind == 'normal':
        return normal(raw_words(4 * ((n + 3) // 4), seed, offset, stream_id))[:n]
    r = raw_words(n, seed, offset, stream_id)
    return uniform(r, lo, hi) if kind == 'uniform' else keep_drop(r, lo, hi)
