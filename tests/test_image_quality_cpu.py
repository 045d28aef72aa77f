"""Image quality without a GPU: the float64 statement of tests/image_quality_ref.py against an independent form of the window means and
against closed forms, how far the same centred formulas in float32 lie from it, the test line's suffix, the new flags, and the header."""
import os
import re

import numpy as np
import pytest

import image_quality_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pair(shape, seed, noise=0.1):
    rng = np.random.default_rng(seed)
    a = rng.random(shape)
    return a, np.clip(a + noise * rng.standard_normal(shape), 0.0, 1.0)


def test_window_is_the_normalised_gaussian():
    w = R.window()
    assert w.shape == (11, 11) and abs(w.sum() - 1.0) < 1e-15 and np.array_equal(w, w.T) and np.array_equal(w, w[::-1, ::-1])
    assert abs(w[5, 5] / w[5, 4] - np.exp(0.5 / 1.5 ** 2)) < 1e-14
    w32 = R.window(np.float32)
    assert w32.dtype == np.float32 and np.abs(w32.astype(np.float64) - w).max() <= 2.0 ** -24 * w.max()


def test_statement_means_match_an_independent_correlation():
    """mu = x_c + sum w (x - x_c) is the weighted mean: pinned to scipy's valid correlation with the same window, to 1e-12; the centred
    second moments to the raw-moment form in float64, where that form still holds (values of order 1, so 1e-12 is twelve digits)."""
    from scipy.signal import correlate2d
    w = R.window()
    for shape, seed in (((11, 11), 1), ((12, 17), 2), ((28, 28), 3), ((32, 32), 4)):
        a, b = _pair(shape, seed)
        mu_a, mu_b, var_a, var_b, cov = R.moments(a, b)
        ea, eb = correlate2d(a, w, mode='valid'), correlate2d(b, w, mode='valid')
        assert mu_a.shape == ea.shape == (shape[0] - 10, shape[1] - 10)
        assert np.abs(mu_a - ea).max() <= 1e-12 and np.abs(mu_b - eb).max() <= 1e-12
        assert np.abs(var_a - (correlate2d(a * a, w, mode='valid') - ea * ea)).max() <= 1e-12
        assert np.abs(cov - (correlate2d(a * b, w, mode='valid') - ea * eb)).max() <= 1e-12
        assert (var_a >= 0).all() and (var_b >= 0).all()


def test_closed_forms():
    rng = np.random.default_rng(5)
    a = rng.random((2, 3, 16, 19))
    # identical images: every window 1, mse 0, psnr +inf; in float32 as well, exactly
    for dtype in (np.float64, np.float32):
        x = a.astype(dtype)
        assert (R.ssim_map(x, x, 1.0, dtype) == 1).all()
        out = R.image_quality(x, x, dtype=dtype)
        assert out.dtype == dtype and (out[:, 0] == 0).all() and np.isposinf(out[:, 1]).all() and (out[:, 2] == 1).all()
    # two constant planes: the variances and the covariance vanish exactly, the luminance term is left
    for c1, c2, data_range in ((0.25, 0.75, 1.0), (0.1, 0.1001, 1.0), (40.0, 200.0, 255.0)):
        p, q = np.full((1, 1, 13, 14), c1), np.full((1, 1, 13, 14), c2)
        _, _, var_a, var_b, cov = R.moments(p, q)
        assert (var_a == 0).all() and (var_b == 0).all() and (cov == 0).all()
        C1 = (0.01 * data_range) ** 2
        out = R.image_quality(p, q, data_range=data_range)
        assert abs(out[0, 2] - (2 * c1 * c2 + C1) / (c1 * c1 + c2 * c2 + C1)) <= 1e-14
        assert abs(out[0, 0] - (c1 - c2) ** 2) <= 1e-15 * max(1.0, (c1 - c2) ** 2)
    # PSNR of a known mse
    assert abs(R.psnr_db(0.01) - 20.0) <= 1e-13 and abs(R.psnr_db(6.5025, 255.0) - 40.0) <= 1e-12
    assert np.isposinf(R.psnr_db(0.0)) and np.isnan(R.psnr_db(np.nan))
    b = np.clip(a + 0.1, 0, 2)
    out = R.image_quality(a, b, data_range=2.0)
    assert np.abs(out[:, 0] - 0.01).max() <= 1e-15 and np.abs(out[:, 1] - 10 * np.log10(4.0 / 0.01)).max() <= 1e-10


def test_clamp_and_mask_rules():
    rng = np.random.default_rng(6)
    a = rng.random((2, 1, 12, 13))
    b = a + 0.5 * rng.standard_normal(a.shape)
    assert np.array_equal(R.image_quality(a, b), R.image_quality(a, np.clip(b, 0, 1), clamp_images=False))
    assert not np.array_equal(R.image_quality(a, b), R.image_quality(a, b, clamp_images=False))
    c = R.clamp(np.array([-1.0, 0.5, 3.0, np.nan]), 1.0)
    assert c[:3].tolist() == [0.0, 0.5, 1.0] and np.isnan(c[3])
    # a single counted pixel at a window centre: mse is that pixel's squared error, ssim that one window
    mask = np.zeros((2, 12, 13), dtype=np.uint8)
    mask[:, 6, 7] = 1
    b = np.clip(b, 0, 1)
    out = R.image_quality(a, b, mask=mask)
    assert np.allclose(out[:, 0], (a[:, 0, 6, 7] - b[:, 0, 6, 7]) ** 2, rtol=1e-15, atol=0)
    assert np.array_equal(out[:, 2], R.ssim_map(a, b)[:, 0, 1, 2])
    # the other side of the same mask is everything else; a counted pixel off every centre leaves no position
    rest = R.image_quality(a, b, mask=mask, count_where=0)
    full = R.image_quality(a, b)
    assert np.allclose(rest[:, 0] * (12 * 13 - 1) + out[:, 0], full[:, 0] * 12 * 13, rtol=1e-13)
    edge = np.zeros((2, 12, 13), dtype=np.uint8)
    edge[:, 0, 0] = 1
    out = R.image_quality(a, b, mask=edge)
    assert np.isfinite(out[:, :2]).all() and np.isnan(out[:, 2]).all()
    none = R.image_quality(a, b, mask=np.zeros((2, 12, 13), dtype=np.uint8))
    assert np.isnan(none).all()


def test_float32_stays_close_to_the_statement():
    """The error scale the GPU parity rule doubles: the centred formulas in float32 against float64. Per window at most a few 1e-7 on
    reconstruction-like pairs (measured 3.4e-7 over these shapes), and 3.1e-8 on a flat plane with one pixel off by 1e-3: the bound
    asserted is 1e-6, four float32 roundings of a value near 1."""
    worst = 0.0
    for shape, seed in (((1, 11, 11), 1), ((3, 12, 17), 2), ((1, 28, 28), 3), ((3, 32, 32), 4)):
        a, b = _pair(shape, seed)
        a, b = a.astype(np.float32), b.astype(np.float32)
        worst = max(worst, float(np.abs(R.ssim_map(a, b, 1.0, np.float32).astype(np.float64) - R.ssim_map(a, b)).max()))
    flat = np.full((1, 16, 16), 0.5, dtype=np.float32)
    off = flat.copy()
    off[0, 8, 8] += 1e-3
    worst_flat = float(np.abs(R.ssim_map(flat, off, 1.0, np.float32).astype(np.float64) - R.ssim_map(flat, off)).max())
    print('float32 against float64, per window: %.3g (random pairs), %.3g (flat plane, one pixel off)' % (worst, worst_flat))
    assert worst <= 1e-6 and worst_flat <= 1e-6
    r32, r64 = R.image_quality(flat[None], off[None], dtype=np.float32), R.image_quality(flat[None], off[None])
    assert (np.abs(r32 - r64) <= R.parity_bound(r32, r64)).all()


def test_line_suffix():
    import lvae_amd  # noqa: F401
    from lvae_amd.quality import quality_line_suffix
    res = {'quality/psnr': 23.4567, 'quality/ssim': 0.87654321, 'quality/mse': 0.1}
    assert quality_line_suffix(res) == '   PSNR: 23.46 dB   SSIM: 0.8765'
    assert quality_line_suffix({'quality/psnr': float('inf'), 'quality/ssim': 1.0}) == '   PSNR: inf dB   SSIM: 1.0000'


def test_flags_parse():
    import lvae_amd  # noqa: F401
    from lvae_amd.evaluate import parse_eval_args
    from lvae_amd.experiment.experiment_manager import build_parser
    assert build_parser().parse_args([]).image_quality is False
    assert build_parser().parse_args(['--image-quality']).image_quality is True
    args = parse_eval_args(['--synthetic', '--quality-ladder'])
    assert args.quality_ladder and args.temperature is None and not args.image_quality
    args = parse_eval_args(['--synthetic', '--quality-ladder', '--temperature', '0.7'])
    assert args.temperature == [0.7]
    assert parse_eval_args(['--synthetic', '--ll', '--image-quality']).image_quality
    assert not parse_eval_args(['--synthetic', '--ll']).quality_ladder
    with pytest.raises(SystemExit):
        parse_eval_args(['--synthetic', '--image-quality'])               # measured during the log-likelihood pass
    with pytest.raises(SystemExit):
        parse_eval_args(['--synthetic', '--quality-ladder', '--temperature', '0.5', '0.6'])   # (never one value per layer here)


def test_python_argument_checks_need_no_device():
    import torch

    import lvae_amd  # noqa: F401
    from lvae_amd import _C
    from lvae_amd.quality import image_quality
    a = torch.zeros(2, 3, 16, 16)
    with pytest.raises(ValueError):
        image_quality(a, torch.zeros(2, 3, 16, 17))
    with pytest.raises(_C.LvaeHipError):
        image_quality(a, a)                                                # CPU tensors: there is no fallback
    with pytest.raises(ValueError):
        image_quality(a, a, count='hidden')
    with pytest.raises(ValueError):
        image_quality(a[:, :, :, :10], a[:, :, :, :10])                    # below the 11 x 11 window


def test_header_declares_the_entry_points():
    import lvae_amd  # noqa: F401
    from lvae_amd import _C
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'lvae_hip.h')).read(), flags=re.S)
    names = {'lvae_image_quality_workspace': 4, 'lvae_image_quality_f32': 18, 'lvae_image_quality_fold_f64': 4}
    for name, n_args in names.items():
        m = re.search(r'(?:size_t|int)\s+%s\s*\(([^;]*)\)\s*;' % name, hdr)
        assert m, 'include/lvae_hip.h does not declare %s' % name
        assert len(m.group(1).split(',')) == n_args == len(_C.SIGNATURES[name][1])
    m = re.search(r'int\s+lvae_image_quality_f32\s*\(([^;]*)\)\s*;', hdr)
    assert [' '.join(a.split()).split()[-1].lstrip('*') for a in m.group(1).split(',')] == [
        'a', 'a_nhwc', 'a_ld', 'b', 'b_nhwc', 'b_ld', 'mask', 'count_where', 'N', 'C', 'H', 'W', 'data_range', 'clamp', 'out', 'workspace',
        'workspace_bytes', 'stream']
    src = os.path.join(ROOT, 'ladder-vae-pytorch_amd', 'csrc')
    assert 'image_quality.hip' in open(os.path.join(src, 'Makefile')).read() and os.path.exists(os.path.join(src, 'image_quality.hip'))
