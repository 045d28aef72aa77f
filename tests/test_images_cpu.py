"""Host side of the picture grids: the PNG writer decoded with the standard library, the picture cadence of the schedule, and the flags.
No GPU needed."""
import struct
import zlib

import numpy as np
import pytest

import lvae_amd  # noqa: F401
from lvae_amd.schedule import TrainSchedule


def decode_png(data):
    """bytes of an 8-bit RGB PNG whose rows all use filter type 0 -> (H, W, 3) uint8 array. Standard library only; every chunk's CRC and
    every IHDR field is checked."""
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack('>I4s', data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert len(body) == n
        assert struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        chunks.append((tag, body))
        pos += 12 + n
    assert pos == len(data)
    assert chunks[0][0] == b'IHDR' and chunks[-1] == (b'IEND', b'')
    assert all(t in (b'IHDR', b'IDAT', b'IEND') for t, _ in chunks)
    W, H, depth, colour, compression, filt, interlace = struct.unpack('>IIBBBBB', chunks[0][1])
    assert (depth, colour, compression, filt, interlace) == (8, 2, 0, 0, 0)
    raw = zlib.decompress(b''.join(b for t, b in chunks if t == b'IDAT'))
    assert len(raw) == H * (1 + 3 * W)
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(H, 1 + 3 * W)
    assert not rows[:, 0].any()          # filter type 0 on every row
    return rows[:, 1:].reshape(H, W, 3).copy()


@pytest.mark.parametrize('shape', [(1, 1), (7, 13), (410, 410)])
@pytest.mark.parametrize('as_tensor', [False, True])
def test_write_png_round_trips(tmp_path, shape, as_tensor):
    import torch
    from lvae_amd.images import write_png
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    grid = rng.integers(0, 256, size=shape + (3,), dtype=np.uint8)
    grid[0, 0] = (0, 255, 10)            # 10 = a line feed: the file is written in binary mode
    path = str(tmp_path / 'g.png')
    write_png(path, torch.from_numpy(grid) if as_tensor else grid)
    data = open(path, 'rb').read()
    assert np.array_equal(decode_png(data), grid)
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(path) as im:
        assert im.mode == 'RGB' and im.size == (shape[1], shape[0])
        assert np.array_equal(np.asarray(im), grid)


def test_write_png_refuses_other_arrays(tmp_path):
    from lvae_amd.images import encode_png
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 1), np.uint8), np.zeros((4, 4, 3), np.float32), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            encode_png(bad)


def test_grid_shape_is_make_grid_with_padding_two():
    from lvae_amd.images import grid_shape
    assert grid_shape(64, 8, 32, 32) == (34 * 8 + 2, 34 * 8 + 2)
    assert grid_shape(144, 12, 64, 64) == (66 * 12 + 2, 66 * 12 + 2)
    assert grid_shape(5, 8, 28, 20) == (30 + 2, 22 * 5 + 2)          # fewer images than a row holds: the row is as wide as they are
    assert grid_shape(13, 12, 28, 28) == (30 * 2 + 2, 30 * 12 + 2)   # a second row with one image in it
    assert grid_shape(1, 8, 3, 4) == (7, 8)                          # a single image is padded like any other


def test_images_at():
    for every, due in ((-1, []), (0, []), (3, [3, 6, 9, 12])):
        s = TrainSchedule(2, 4, 8, 2, has_test=True, checkpoint_dir='ck', images_every=every)
        assert [k for k in range(1, 13) if s.images_at(k)] == due
        assert all(s.images_at(k) is (k in due) for k in range(1, 13))
    # no test split, no checkpoint directory: pictures are still due (the samples need neither)
    assert TrainSchedule(2, 4, 8, 2, has_test=False, images_every=5).images_at(10)
    # the default: never
    assert not any(TrainSchedule(2, 4, 8, 2, True, 'ck').images_at(k) for k in range(1, 13))


def test_at_is_what_it_was():
    want = {1: (0, False), 2: (1, True), 3: (0, False), 4: (8, True), 5: (0, False), 6: (1, True), 7: (0, False), 8: (8, True)}
    for kw in ({}, {'images_every': 3}, {'images_every': -1}):
        s = TrainSchedule(test_every=2, ll_every=4, ll_samples=8, checkpoint_every=2, has_test=True, checkpoint_dir='ck', **kw)
        assert {k: s.at(k) for k in range(1, 9)} == want
        s = TrainSchedule(2, 4, 8, 2, True, 'ck', **kw)   # the positional form of the existing callers
        assert {k: s.at(k) for k in range(1, 9)} == want
        assert all(TrainSchedule(2, 4, 8, 2, has_test=False, checkpoint_dir='', **kw).at(k) == (0, False) for k in range(1, 20))


def test_trainer_flags():
    from lvae_amd.experiment.experiment_manager import build_parser
    a = build_parser().parse_args([])
    assert a.img_dir == '' and a.test_imgs_every == -1
    s = TrainSchedule.from_args(a, has_test=True)
    assert s.images_every == -1 and not any(s.images_at(k) for k in range(1, 50))
    a = build_parser().parse_args(['--img-dir', 'pics', '--ts-img-every', '4'])
    assert a.img_dir == 'pics' and a.test_imgs_every == 4
    s = TrainSchedule.from_args(a, has_test=False)
    assert [k for k in range(1, 10) if s.images_at(k)] == [4, 8] and s.at(4) == (0, False)


def test_evaluate_flags(capsys):
    from lvae_amd.evaluate import parse_eval_args
    a = parse_eval_args(['--synthetic', '--ps'])
    assert a.img_dir == '' and not a.recons and a.ps
    a = parse_eval_args(['--synthetic', '--recons', '--img-dir', 'pics', '--layer-repr'])
    assert a.recons and a.img_dir == 'pics' and a.layer_repr
    with pytest.raises(SystemExit) as e:
        parse_eval_args(['--synthetic', '--recons'])
    assert e.value.code != 0
    assert '--recons needs --img-dir' in capsys.readouterr().err
