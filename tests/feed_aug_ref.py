"""numpy restatement of the augmenting gather's noise rule (include/lvae_hip.h: lvae_batch_gather_aug_f32), built on the restated
generator of oracle/philox_ref.py. A helper of tests/test_feed_aug_cpu.py and tests/test_feed_aug_gpu.py, not a test.

A row's noise is a function of (seed, P, g): P the feed cursor (completed micro-batches, not taken modulo the epoch), g the row's place in
the global batch. The fixed rule (storage-order reads, binarize_fixed) has P = 0, g = the image number, its own tag and no flips."""
import numpy as np

from oracle.philox_ref import U01_MAX, raw_words, u01

TAG_PIXEL, TAG_FLIP, TAG_FIXED = 0xA1, 0xA2, 0xA3


def aug_seed(seed):
    return (int(seed) * 0x9E3779B97F4A7C15 + 0x5851F42D4C957F2D) & (2 ** 63 - 1)


def pixel_words(chw, seed, P, g, tag=TAG_PIXEL):
    """The raw word of every output element (CHW order) of one row."""
    return raw_words(4 * ((chw + 3) // 4), seed, P, (tag << 32) | int(g))[:chw]


def pixel_u(chw, seed, P, g, tag=TAG_PIXEL):
    return u01(pixel_words(chw, seed, P, g, tag))


def row_flips(seed, P, g):
    return bool(raw_words(1, seed, P, (TAG_FLIP << 32) | int(g))[0] >> np.uint32(31))


def binarize(v, u):
    """v: float32 values as the plain gather writes them."""
    return np.where(u < np.asarray(v, dtype=np.float32), np.float32(1), np.float32(0)).astype(np.float32)


def dequantize(b, u):
    """b: bytes. (b + u) / 256 with the sum and the product rounded separately in fp32, kept below 1."""
    s = (np.asarray(b).astype(np.float32) + np.asarray(u, dtype=np.float32)).astype(np.float32)
    return np.minimum((s * np.float32(0.00390625)).astype(np.float32), U01_MAX)


def plain(rows):
    """What the plain gather writes for uint8 (a byte means b / 255, an IEEE fp32 division) or float32 rows."""
    rows = np.asarray(rows)
    return (rows.astype(np.float32) / np.float32(255)).astype(np.float32) if rows.dtype == np.uint8 else rows.astype(np.float32)


def augment(rows, seed, P, gs, mode=None, hflip=False, fixed=False):
    """rows: (n, C, H, W) uint8 or float32, the table's images of the batch in CHW order; gs: each row's g (place in the global batch, or
    with fixed the image number). mode None | 'binarize' | 'dequantize'. -> float32 (n, C, H, W), and the list of rows that flipped."""
    rows = np.asarray(rows)
    n, chw = rows.shape[0], int(np.prod(rows.shape[1:]))
    if fixed:
        P = 0
    out = np.empty(rows.shape, dtype=np.float32)
    flipped = []
    for r in range(n):
        src = rows[r]
        if hflip and not fixed and row_flips(seed, P, gs[r]):
            src = src[:, :, ::-1]   # the draw belongs to the output element: only the source is mirrored
            flipped.append(r)
        if mode is None:
            out[r] = plain(src)
            continue
        u = pixel_u(chw, seed, P, gs[r], TAG_FIXED if fixed else TAG_PIXEL).reshape(rows.shape[1:])
        if mode == 'binarize':
            out[r] = binarize(plain(src), u)
        else:
            assert mode == 'dequantize' and rows.dtype == np.uint8
            out[r] = dequantize(src, u)
    return out, flipped


def binarize_fixed(images, seed):
    """uint8 0/1 (N, C, H, W): image i binarized by the fixed rule under aug_seed(seed)."""
    out, _ = augment(images, aug_seed(seed), 0, list(range(len(images))), 'binarize', fixed=True)
    return out.astype(np.uint8)
