"""Picture grids of samples and reconstructions, formed on the device and written as PNG.

`image_grid` restates torchvision's `make_grid` (padding 2) + `save_image` and boilr's `img_grid_pad_value` (white padding when the
pictures have dark edges); the arithmetic is two kernels of csrc/image_grid.hip. `write_png` copies the finished uint8 grid to the host once
and writes an 8-bit RGB PNG with zlib and struct alone: the package depends on no imaging library. Neither torchvision nor boilr is a
dependency; their behaviour is restated from what they publish (parity unpinned).
"""
import struct
import zlib

import numpy as np
import torch

from . import kernels as K

PAD_THRESHOLD = 0.2   # boilr's img_grid_pad_value: white padding when the median border value is below this


def grid_shape(n, nrow, H, W):
    """(Hg, Wg) of the grid of n images of H x W, nrow per row."""
    return K.image_grid_shape(n, nrow, H, W)


@torch.no_grad()
def image_grid(imgs, nrow, second=None, pad_value=None):
    """imgs: (N, C, H, W) float32 on the device, C = 1 or 3 -> uint8 device tensor (Hg, Wg, 3), nrow images per row.

    second: an image set of the same shape, interleaved with the first (imgs[0], second[0], imgs[1], second[1], ...): inputs beside their
    reconstructions. pad_value=None: 1.0 when the median border value of the images is below 0.2, else 0.0, counted and decided on the
    device (the host does not wait for it); a number: that padding value."""
    if pad_value is None:
        return K.image_grid(imgs, nrow, second, border_count=K.image_border_count(imgs, second, PAD_THRESHOLD))
    return K.image_grid(imgs, nrow, second, pad_value=float(pad_value))


def _chunk(tag, data):
    return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xFFFFFFFF)


def encode_png(rgb):
    """uint8 (H, W, 3) array -> the bytes of an 8-bit RGB PNG, filter type 0 on every row."""
    rgb = np.ascontiguousarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or 0 in rgb.shape:
        raise ValueError("encode_png needs a non-empty uint8 (H, W, 3) array, got %s %s" % (rgb.dtype, rgb.shape))
    H, W, _ = rgb.shape
    rows = np.zeros((H, 1 + 3 * W), dtype=np.uint8)   # column 0: the filter byte of each row
    rows[:, 1:] = rgb.reshape(H, 3 * W)
    ihdr = struct.pack('>IIBBBBB', W, H, 8, 2, 0, 0, 0)   # bit depth 8, colour type 2 (RGB), deflate, adaptive filtering, no interlace
    return b'\x89PNG\r\n\x1a\n' + _chunk(b'IHDR', ihdr) + _chunk(b'IDAT', zlib.compress(rows.tobytes(), 6)) + _chunk(b'IEND', b'')


def write_png(path, grid):
    """Write a (H, W, 3) uint8 grid (device tensor, CPU tensor or array) as PNG: one device-to-host copy."""
    if isinstance(grid, torch.Tensor):
        grid = grid.detach().cpu().numpy()
    data = encode_png(grid)
    with open(path, 'wb') as f:
        f.write(data)
