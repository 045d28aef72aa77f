"""Image quality on the GPU (csrc/image_quality.hip, lvae_amd.quality): the kernel against the float64 statement of
tests/image_quality_ref.py under the element-wise rule of docs/ELEMENTWISE_PARITY.md, the properties that hold exactly, independence of batch,
storage and alignment, the mask rules, the argument checks, the fold, and the test pass and the quality ladder on the tiny golden models."""
import functools
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import image_quality_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TILE = 32 + 10   # pixels of one LDS tile edge (csrc/image_quality.hip): 43 is one pixel more


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs, storage forms, references (computed once per case)
# ---------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(3, 1, 11, 11),              # a single window
          (2, 3, 12, 17),
          (5, 1, 28, 28),
          (4, 3, 32, 32),
          (2, 3, 64, 64),              # 2 x 2 tiles
          (2, 2, TILE + 1, TILE + 1)]  # one pixel past a tile in each direction: four tiles, three of them one position wide or high
KINDS = ['random', 'recon', 'flat']
STORAGES = ['nchw', 'nhwc', 'ld2c']


@functools.lru_cache(maxsize=None)
def _inputs(shape, kind):
    rng = np.random.default_rng(sum(shape) * 7 + KINDS.index(kind))
    if kind == 'random':
        a, b = rng.random(shape), rng.random(shape)
    elif kind == 'recon':
        a = rng.random(shape)
        b = np.clip(a + 0.1 * rng.standard_normal(shape), 0.0, 1.0)
    else:   # flat planes, one pixel of every plane of b off by 1e-3
        a = np.broadcast_to(rng.random(shape[:2])[:, :, None, None], shape).copy()
        b = a.copy()
        b[:, :, shape[2] // 2, shape[3] // 3] += 1e-3
    return a.astype(np.float32), b.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _refs(shape, kind):
    a, b = _inputs(shape, kind)
    r64, r32 = R.image_quality(a, b), R.image_quality(a, b, dtype=np.float32)
    assert np.isfinite(r64).all() and np.isfinite(r32).all()   # before anything goes to the device
    return r64, r32.astype(np.float64)


def _store(x, storage, offset=0):
    """The NCHW-shaped device tensor of the host array x (N, C, H, W) in one storage form; `offset` floats into its allocation.
    'ld2c' is the first C of 2C channels of a channel-last buffer whose other channels hold NaN."""
    t = torch.from_numpy(np.ascontiguousarray(x))
    N, C, H, W = t.shape
    if storage == 'nchw':
        buf = torch.full((t.numel() + offset,), float('nan'), device='cuda')
        v = buf[offset:].view(N, C, H, W)
    else:
        ld = C if storage == 'nhwc' else 2 * C
        buf = torch.full((N * H * W * ld + offset,), float('nan'), device='cuda')
        v = buf[offset:].view(N, H, W, ld)[..., :C].permute(0, 3, 1, 2)
    v.copy_(t)
    assert v.data_ptr() == buf.data_ptr() + 4 * offset
    return v


def _rows(a, b, **kw):
    from lvae_amd.quality import image_quality
    out = image_quality(a, b, **kw)
    return torch.stack([out['mse'], out['psnr'], out['ssim']], 1).cpu().numpy()


def _same_bits(x, y):
    return np.array_equal(np.asarray(x, dtype=np.float32).view(np.uint32), np.asarray(y, dtype=np.float32).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------------
# (1) parity with the float64 statement
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_parity_with_float64(shape, kind):
    """|kernel - r64| <= 2 max|r32 - r64| + 1e-5 |r64| + 1e-6 for mse, psnr and ssim, in every pair of storage forms. The largest use of
    the bound is printed (run with -s); docs/ELEMENTWISE_PARITY.md keeps the measured figures."""
    a, b = _inputs(shape, kind)
    r64, r32 = _refs(shape, kind)
    bound = R.parity_bound(r32, r64)
    first, worst = None, np.zeros(3)
    for sa in STORAGES:
        for sb in STORAGES:
            got = _rows(_store(a, sa), _store(b, sb))
            assert got.dtype == np.float32 and got.shape == (shape[0], 3)
            err = np.abs(got.astype(np.float64) - r64)
            worst = np.maximum(worst, (err / bound).max(0))
            assert (err <= bound).all(), (sa, sb, err.max(0), bound.min(0))
            first = got if first is None else first
            assert _same_bits(got, first), (sa, sb)           # and the storage form changes no bit
    print('%s %s: largest |kernel - r64| / bound (mse, psnr, ssim) = %s; bound %s; r32 - r64 %s'
          % ('x'.join(map(str, shape)), kind, worst.round(4), bound.max(0), np.abs(r32 - r64).max(0)))


def test_data_range_255():
    a, b = _inputs((4, 3, 32, 32), 'recon')
    a, b = np.round(a * 255), np.round(b * 255)
    r64, r32 = R.image_quality(a, b, data_range=255.0), R.image_quality(a, b, data_range=255.0, dtype=np.float32).astype(np.float64)
    got = _rows(_store(a, 'nchw'), _store(b, 'nhwc'), data_range=255.0).astype(np.float64)
    assert (np.abs(got - r64) <= R.parity_bound(r32, r64)).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# (2) what holds exactly
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(3, 1, 11, 11), (2, 3, TILE + 1, TILE + 1)], ids=['one-window', 'four-tiles'])
def test_identical_images_are_exact(shape):
    rng = np.random.default_rng(3)
    a = (1.5 * rng.random(shape) - 0.25).astype(np.float32)      # some values outside [0, 1]: clamped alike
    for clamp in (True, False):
        for sa, sb in (('nchw', 'nchw'), ('nchw', 'ld2c'), ('nhwc', 'nchw')):
            got = _rows(_store(a, sa), _store(a, sb), clamp=clamp)
            assert (got[:, 0] == 0).all() and np.isposinf(got[:, 1]).all() and (got[:, 2] == 1).all(), (clamp, sa, sb, got)


def test_constant_planes_have_no_variance():
    """Two constant planes: with mu == c and variance and covariance exactly 0 the SSIM is the luminance term alone, and equals its fp32
    evaluation, every product and sum rounded on its own, bit for bit."""
    f = np.float32
    for c1, c2, data_range in ((0.3, 0.7, 1.0), (0.1, 0.1001, 1.0), (0.0, 1.0, 1.0), (37.0, 201.0, 255.0)):
        a, b = np.full((2, 3, 13, TILE + 3), c1, dtype=f), np.full((2, 3, 13, TILE + 3), c2, dtype=f)
        got = _rows(_store(a, 'nchw'), _store(b, 'nhwc'), data_range=data_range)
        c1_, c2_, r = f(c1), f(c2), f(data_range)
        C1, C2 = (f(0.01) * r) * (f(0.01) * r), (f(0.03) * r) * (f(0.03) * r)
        num = (f(2) * (c1_ * c2_) + C1) * (f(2) * f(0) + C2)
        den = ((c1_ * c1_ + c2_ * c2_) + C1) * ((f(0) + f(0)) + C2)
        want = f(num) / f(den)
        assert want.dtype == f and _same_bits(got[:, 2], np.full(2, want)), (c1, c2, got[:, 2], want)
        d = c1_ - c2_
        assert np.abs(got[:, 0].astype(np.float64) - float(d) ** 2).max() <= 1e-6 * float(d) ** 2


def test_clamp_and_nan():
    rng = np.random.default_rng(4)
    shape = (3, 3, 16, 20)
    a = (2.0 * rng.random(shape) - 0.5).astype(np.float32)
    b = (2.0 * rng.random(shape) - 0.5).astype(np.float32)
    for data_range in (1.0, 0.75):
        clamped = _rows(_store(a, 'nchw'), _store(b, 'nhwc'), data_range=data_range)
        by_hand = _rows(_store(np.clip(a, 0, data_range), 'nchw'), _store(np.clip(b, 0, data_range), 'nhwc'), data_range=data_range, clamp=False)
        raw = _rows(_store(a, 'nchw'), _store(b, 'nhwc'), data_range=data_range, clamp=False)
        assert _same_bits(clamped, by_hand) and not np.array_equal(clamped, raw)
        r64 = R.image_quality(a, b, data_range=data_range)
        r32 = R.image_quality(a, b, data_range=data_range, dtype=np.float32).astype(np.float64)
        assert (np.abs(clamped.astype(np.float64) - r64) <= R.parity_bound(r32, r64)).all()
    # a NaN stays a NaN under the clamp: it reaches its own image's three numbers and no other image's
    clean = _rows(_store(a, 'nchw'), _store(b, 'nchw'))
    bn = b.copy()
    bn[1, 2, 7, 9] = np.nan
    got = _rows(_store(a, 'nchw'), _store(bn, 'nchw'))
    assert np.isnan(got[1]).all() and _same_bits(got[[0, 2]], clean[[0, 2]])


# ---------------------------------------------------------------------------------------------------------------------------------
# (3) independence of batch, position, storage and alignment
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(7, 3, 17, 23), (7, 2, TILE + 1, TILE + 1)], ids=['one-tile', 'four-tiles'])
def test_an_images_numbers_are_its_own(shape):
    a, b = _inputs(shape, 'recon')
    batch = _rows(_store(a, 'nchw'), _store(b, 'nchw'))
    for i in range(shape[0]):
        alone = _rows(_store(a[i:i + 1], 'nchw'), _store(b[i:i + 1], 'nchw'))
        assert _same_bits(alone[0], batch[i]), i
    perm = np.array([3, 0, 6, 1, 5, 2, 4])
    assert _same_bits(_rows(_store(a[perm], 'nhwc'), _store(b[perm], 'ld2c')), batch[perm])
    for sa in STORAGES:
        for off_a, off_b in ((1, 0), (0, 1), (1, 1), (3, 2)):
            assert _same_bits(_rows(_store(a, sa, off_a), _store(b, 'ld2c', off_b)), batch), (sa, off_a, off_b)
    # the channel-last calling convention reads the same storage
    an, bn = _store(a, 'nhwc').permute(0, 2, 3, 1), _store(b, 'ld2c').permute(0, 2, 3, 1)
    assert an.is_contiguous() and not bn.is_contiguous()
    assert _same_bits(_rows(an, bn, channel_last=True), batch)


# ---------------------------------------------------------------------------------------------------------------------------------
# (4) the mask
# ---------------------------------------------------------------------------------------------------------------------------------
def test_mask_rules():
    shape = (3, 3, TILE + 1, 20)
    N, C, H, W = shape
    a, b = _inputs(shape, 'recon')
    rng = np.random.default_rng(8)
    mask = (rng.random((N, H, W)) < 0.6)
    mask[2] = True                                   # image 2: everything observed, so nothing is 'missing'
    da, db = _store(a, 'nchw'), _store(b, 'nhwc')
    for count, where in (('observed', 1), ('missing', 0)):
        r64 = R.image_quality(a, b, mask=mask, count_where=where)
        r32 = R.image_quality(a, b, mask=mask, count_where=where, dtype=np.float32).astype(np.float64)
        keep = [0, 1] + ([2] if where else [])
        assert np.isfinite(r64[keep]).all()
        for m in (torch.from_numpy(mask).cuda(), torch.from_numpy(mask.astype(np.uint8)).cuda()[:, None]):
            got = _rows(da, db, mask=m, count=count)
            assert (np.abs(got[keep].astype(np.float64) - r64[keep]) <= R.parity_bound(r32[keep], r64[keep])).all(), count
            if not where:
                assert np.isnan(got[2]).all()        # nothing counted: NaN, NaN and NaN
    # a NaN under an uncounted pixel changes no bit of mse and psnr (the windows that cover it do see it)
    got = _rows(da, db, mask=torch.from_numpy(mask).cuda())
    bn = b.copy()
    y, x = np.argwhere(~mask[0])[5]
    bn[0, :, y, x] = np.nan
    poisoned = _rows(da, _store(bn, 'nhwc'), mask=torch.from_numpy(mask).cuda())
    assert _same_bits(poisoned[:, :2], got[:, :2]) and _same_bits(poisoned[1:], got[1:])
    # the centre rule: one counted pixel is one squared error per channel and one window per channel
    one = np.zeros((N, H, W), dtype=bool)
    one[:, TILE - 5, 9] = True                       # the centre of position (TILE - 10, 4): the one row of the second tile row
    got = _rows(da, db, mask=torch.from_numpy(one).cuda())
    r64 = R.image_quality(a, b, mask=one)
    r32 = R.image_quality(a, b, mask=one, dtype=np.float32).astype(np.float64)
    assert (np.abs(got.astype(np.float64) - r64) <= R.parity_bound(r32, r64)).all()
    assert np.abs(r64[:, 2] - R.ssim_map(a.astype(np.float64), b.astype(np.float64))[:, :, TILE - 10, 4].mean(1)).max() <= 1e-15
    corner = np.zeros((N, H, W), dtype=bool)
    corner[:, 0, W - 1] = True                       # a counted pixel that is no window's centre
    got = _rows(da, db, mask=torch.from_numpy(corner).cuda())
    assert np.isfinite(got[:, :2]).all() and np.isnan(got[:, 2]).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# (5) bad arguments
# ---------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch():
    import lvae_amd  # noqa: F401
    from lvae_amd import _C
    from lvae_amd.quality import image_quality
    EINVAL, EALIGN, EWORKSPACE = -1, -2, -3
    N, C, H, W = 2, 3, 16, 16
    a, b = torch.rand(N, C, H, W, device='cuda'), torch.rand(N, C, H, W, device='cuda')
    out = torch.full((N, 3), -7.0, device='cuda')
    lib = _C.load()
    need = lib.lvae_image_quality_workspace(N, C, H, W)
    assert need >= N * C * 16 and need % 8 == 0
    assert lib.lvae_image_quality_workspace(N, C, 10, W) == 0 == lib.lvae_image_quality_workspace(0, C, H, W) == lib.lvae_image_quality_workspace(N, 5, H, W)
    ws = torch.zeros(need + 8, dtype=torch.uint8, device='cuda')
    sp = _C.stream_ptr()
    good = dict(a=a.data_ptr(), a_nhwc=0, a_ld=0, b=b.data_ptr(), b_nhwc=0, b_ld=0, mask=None, cw=1, N=N, C=C, H=H, W=W, R=1.0, clamp=1,
                out=out.data_ptr(), ws=ws.data_ptr(), nbytes=need, stream=sp)
    cases = [(dict(a=None), EINVAL), (dict(b=None), EINVAL), (dict(out=None), EINVAL), (dict(N=0), EINVAL), (dict(C=0), EINVAL),
             (dict(C=5), EINVAL), (dict(H=10), EINVAL), (dict(W=10), EINVAL), (dict(a_nhwc=1, a_ld=2), EINVAL), (dict(b_nhwc=1, b_ld=1), EINVAL),
             (dict(R=0.0), EINVAL), (dict(R=-1.0), EINVAL), (dict(R=math.inf), EINVAL), (dict(R=math.nan), EINVAL),
             (dict(ws=None), EWORKSPACE), (dict(nbytes=need - 1), EWORKSPACE), (dict(nbytes=0), EWORKSPACE), (dict(ws=ws.data_ptr() + 4), EALIGN)]
    for change, code in cases:
        args = tuple(dict(good, **change).values())
        assert lib.lvae_image_quality_f32(*args) == code, (change, code)
        with pytest.raises(_C.LvaeHipError):
            _C.call('lvae_image_quality_f32', *args)
    sums = torch.full((5,), -7.0, dtype=torch.float64, device='cuda')
    rows = torch.rand(4, 3, device='cuda')
    assert lib.lvae_image_quality_fold_f64(None, 4, sums.data_ptr(), sp) == EINVAL
    assert lib.lvae_image_quality_fold_f64(rows.data_ptr(), 4, None, sp) == EINVAL
    assert lib.lvae_image_quality_fold_f64(rows.data_ptr(), 0, sums.data_ptr(), sp) == EINVAL
    assert lib.lvae_image_quality_fold_f64(rows.data_ptr(), 4, sums.data_ptr() + 4, sp) == EALIGN
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and not bool(ws.any()) and bool((sums == -7.0).all())   # nothing was launched or written
    _C.call('lvae_image_quality_f32', *good.values())                                        # and the good call goes through
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool((out != -7.0).all())
    # the Python layer
    with pytest.raises(ValueError):
        image_quality(a, b[:, :, :, :15])
    with pytest.raises(ValueError):
        image_quality(a[:, :, :10], b[:, :, :10])
    with pytest.raises(_C.LvaeHipError):
        image_quality(a.cpu(), b)
    with pytest.raises(_C.LvaeHipError):
        image_quality(a, b.transpose(2, 3).contiguous().transpose(2, 3))                      # a storage that is neither form: no silent copy
    with pytest.raises(ValueError):
        image_quality(a, b, mask=torch.ones(N, H, W + 1, dtype=torch.bool, device='cuda'))


# ---------------------------------------------------------------------------------------------------------------------------------
# (6) the fold
# ---------------------------------------------------------------------------------------------------------------------------------
def _sequential(sums, rows):
    """The fold restated: image by image, in double."""
    s = [np.float64(v) for v in sums]
    for mse, psnr, ssim in rows:
        s[0] += np.float64(1.0)
        s[1] += np.float64(mse)
        if not (psnr == np.inf):
            s[2] += np.float64(psnr)
        if mse == 0:
            s[3] += np.float64(1.0)
        s[4] += np.float64(ssim)
    return np.array(s, dtype=np.float64)


def test_fold_is_the_sequential_double_sum():
    from lvae_amd import kernels as K
    from lvae_amd.quality import ImageQuality
    a, b = _inputs((300, 1, 11, 11), 'recon')     # more images than one staging round of the fold holds
    b = b.copy()
    b[[4, 260]] = a[[4, 260]]                      # two exact images
    r1 = torch.from_numpy(_rows(_store(a, 'nchw'), _store(b, 'nchw'))).cuda()
    a2, b2 = _inputs((5, 3, 12, 17), 'random')
    r2 = torch.from_numpy(_rows(_store(a2, 'nchw'), _store(b2, 'nchw'))).cuda()
    sums = torch.zeros(5, dtype=torch.float64, device='cuda')
    K.image_quality_fold(r1, sums)
    want = _sequential(np.zeros(5), r1.cpu().numpy())
    assert np.array_equal(sums.cpu().numpy(), want) and want[0] == 300 and want[3] == 2
    K.image_quality_fold(r2, sums)
    want = _sequential(want, r2.cpu().numpy())
    assert np.array_equal(sums.cpu().numpy(), want) and want[0] == 305
    # the object: fold + take, the means, and the two PSNRs
    q = ImageQuality('cuda')
    q.fold(_store(a, 'nchw'), _store(b, 'nhwc'))
    q.fold(_store(a2, 'nchw'), _store(b2, 'ld2c'))
    assert np.array_equal(q.buf.cpu().numpy(), want)
    res = q.take()
    assert not bool(q.buf.any())
    assert res['n_images'] == 305 and res['quality/exact'] == 2
    assert res['quality/mse'] == want[1] / 305 and res['quality/ssim'] == want[4] / 305 and res['quality/psnr'] == want[2] / 303
    assert abs(res['quality/psnr_of_mean_mse'] - 10 * math.log10(305 / want[1])) <= 1e-12
    with pytest.raises(ValueError):
        q.take()
    # a NaN image is seen, not hidden; an image of a NaN only
    bad = torch.tensor([[0.5, 3.0, 0.9], [float('nan'), float('nan'), float('nan')], [0.0, float('inf'), 1.0]], device='cuda')
    sums.zero_()
    K.image_quality_fold(bad, sums)
    got = sums.cpu().numpy()
    assert got[0] == 3 and got[3] == 1 and np.isnan(got[[1, 2, 4]]).all()
    # all images exact: no finite PSNR
    q.fold(_store(a2, 'nchw'), _store(a2, 'nchw'))
    res = q.take()
    assert res['quality/exact'] == 5 and math.isnan(res['quality/psnr']) and res['quality/psnr_of_mean_mse'] == math.inf and res['quality/ssim'] == 1.0


# ---------------------------------------------------------------------------------------------------------------------------------
# (7) the test pass
# ---------------------------------------------------------------------------------------------------------------------------------
def _fresh_table():
    from lvae_amd import kernels as K
    K.prepared.entries.clear()
    K.prepared.table = None


def _model(cfg, sd, noise):
    import lvae_amd  # noqa: F401
    from lvae_amd.models.lvae import LadderVAE
    torch.manual_seed(0)
    m = LadderVAE(**cfg)
    m.load_state_dict(sd)
    m.cuda().train()
    m.noise = noise
    return m


def _images(n, seed, size=32):
    return torch.floor(256 * torch.rand(n, 3, size, size, generator=torch.Generator().manual_seed(seed))) / 255


QUALITY_KEYS = {'quality/mse', 'quality/psnr', 'quality/ssim', 'quality/psnr_of_mean_mse', 'quality/exact'}


def test_the_pass_is_bit_for_bit_the_pass_without_quality():
    from lvae_amd.evaluate import test_pass
    from lvae_amd.latent import LatentStats
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.quality import ImageQuality
    g = load_golden('tiny_cifar')
    _fresh_table()
    m = _model(g.cfg, g.state_dict(), PhiloxNoise(1))
    xs = [_images(5, 2).cuda(), _images(5, 3).cuda()]
    quality = ImageQuality('cuda')
    out = {}
    for use_graph in (False, True):
        plain_noise, noise = PhiloxNoise(seed=21), PhiloxNoise(seed=21)
        plain = test_pass(m, xs, 3, noise=plain_noise, use_graph=use_graph)
        with_q = test_pass(m, xs, 3, noise=noise, use_graph=use_graph, image_quality=quality)
        assert int(noise.step.item()) == int(plain_noise.step.item()) >= 2 * 3
        for k in plain:
            assert with_q[k] == plain[k], (use_graph, k, with_q[k], plain[k])
        assert set(with_q) - set(plain) == QUALITY_KEYS
        assert not bool(quality.buf.any())
        assert 0 < with_q['quality/mse'] < 1 and 0 < with_q['quality/psnr'] < 60 and -1 <= with_q['quality/ssim'] < 1
        out[use_graph] = with_q
        if use_graph:   # a second pass on the same object and the same captured plan starts from zero
            plans = dict(m._test_graphs)
            noise.step.zero_()
            again = test_pass(m, xs, 3, noise=noise, use_graph=True, image_quality=quality)
            assert all(m._test_graphs[k] is v for k, v in plans.items()) and len(m._test_graphs) == len(plans)
            assert again == with_q
    assert out[True] == out[False]                    # replayed = eager, bit for bit, quality/* included
    # only the first sample of a batch is judged
    first = test_pass(m, xs[:1], 1, noise=PhiloxNoise(seed=21), use_graph=False, image_quality=quality)
    three = test_pass(m, xs[:1], 3, noise=PhiloxNoise(seed=21), use_graph=False, image_quality=quality)
    assert first['n_images'] == three['n_images'] == 5
    assert all(first[k] == three[k] for k in QUALITY_KEYS)
    # the numbers are those of the pictures: the same first draw, judged through the public function
    from lvae_amd.evaluate import _EvalWeights, _test_bottom_up
    from lvae_amd.passes import eval_mode
    from lvae_amd.quality import image_quality
    with torch.no_grad(), eval_mode(m, PhiloxNoise(seed=21)), _EvalWeights([]):
        bu, x_nhwc = _test_bottom_up(m, xs[0])
        m.noise.begin(x_nhwc.device)
        o, _ = m._topdown(bu)
        _, head = m.likelihood(m._crop(o, x_nhwc.shape[1:3]), x_nhwc, m.noise)
        m.noise.end()
        assert head['mean'] is None                   # the logistic mixture: its sample is what is judged
        per = image_quality(x_nhwc, head['sample'], channel_last=True)
    want = _sequential(np.zeros(5), torch.stack([per['mse'], per['psnr'], per['ssim']], 1).cpu().numpy())
    assert first['quality/mse'] == want[1] / 5 and first['quality/ssim'] == want[4] / 5 and first['quality/psnr'] == want[2] / 5
    # one first-sample graph holds both hooks
    stats = LatentStats(m, 'cuda')
    both = test_pass(m, xs, 3, noise=PhiloxNoise(seed=21), use_graph=True, latent_stats=stats, image_quality=quality)
    only = test_pass(m, xs, 3, noise=PhiloxNoise(seed=21), use_graph=True, latent_stats=stats)
    assert all(both[k] == out[True][k] for k in out[True])
    assert all(np.array_equal(x[n], y[n]) for x, y in zip(both['latent_arrays'], only['latent_arrays']) for n in x)
    assert all(both[k] == only[k] for k in only if k != 'latent_arrays')


def test_two_shards_merged_give_the_whole_set():
    from lvae_amd.evaluate import reconstructions
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.quality import ImageQuality
    g = load_golden('tiny_cifar')
    _fresh_table()
    m = _model(g.cfg, g.state_dict(), PhiloxNoise(1))
    pairs = []
    for n, seed in ((5, 40), (3, 41)):
        m.noise = PhiloxNoise(seed)
        pairs.append(reconstructions(m, _images(n, seed)))
    whole, a, b = ImageQuality('cuda'), ImageQuality('cuda'), ImageQuality('cuda')
    whole.fold(*pairs[0])
    whole.fold(*pairs[1])
    a.fold(*pairs[0])
    b.fold(*pairs[1])
    assert float(a.buf[0]) == 5 and float(b.buf[0]) == 3
    a.merge(b)
    one, two = whole.take(), a.take()
    assert one['n_images'] == two['n_images'] == 8 and one['quality/exact'] == two['quality/exact']
    for k in QUALITY_KEYS:
        assert abs(one[k] - two[k]) <= 1e-12 * abs(one[k]), k


def test_quality_of_the_averaged_weights():
    from lvae_amd.checkpoint import ema_state_dict_reference_layout
    from lvae_amd.engine import TrainStep
    from lvae_amd.evaluate import test_pass
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax
    from lvae_amd.quality import ImageQuality
    g = load_golden('tiny_cifar')
    _fresh_table()
    m = _model(g.cfg, g.state_dict(), PhiloxNoise(seed=3))
    opt = Adamax(m, lr=1e-3, ema_decay=0.5)
    st = TrainStep(m, opt, use_graph=False)
    for k in range(2):
        st(_images(4, 10 + k).cuda())
    xt = [_images(5, 30).cuda(), _images(3, 31).cuda()]
    avg_sd = ema_state_dict_reference_layout(m, opt)
    before = m.arena.params.clone()
    got = test_pass(m, xt, 2, noise=PhiloxNoise(seed=21), optimizer=opt, use_graph=False, image_quality=ImageQuality('cuda'))
    torch.cuda.synchronize()
    assert torch.equal(m.arena.params, before)
    assert got.pop('weights') == 'ema' and QUALITY_KEYS <= set(got)
    m2 = _model(g.cfg, avg_sd, PhiloxNoise(1))
    assert got == test_pass(m2, xt, 2, noise=PhiloxNoise(seed=21), use_graph=False, image_quality=ImageQuality('cuda'))
    m3 = _model(g.cfg, g.state_dict(), PhiloxNoise(1))
    other = test_pass(m3, xt, 2, noise=PhiloxNoise(seed=21), use_graph=False, image_quality=ImageQuality('cuda'))
    assert other['quality/ssim'] != got['quality/ssim']


def test_gaussian_head_mean_is_folded_where_it_lies():
    """The Gaussian head's mean is the view params[..., :C] of a 2C-channel tensor: the kernel is handed that tensor's address, nothing is
    copied, and the numbers are those of the copied mean."""
    from lvae_amd.evaluate import test_pass
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.quality import ImageQuality, image_quality
    g = load_golden('tiny_gauss')
    _fresh_table()
    m = _model(g.cfg, g.state_dict(), PhiloxNoise(1))
    x = _images(6, 50, size=16).cuda()
    seen = []
    hook = m.likelihood.register_forward_hook(lambda mod, inp, out: seen.append((out[1]['mean'], out[1]['params']['logvar'], inp[1])))
    quality = ImageQuality('cuda')
    try:
        eager = test_pass(m, [x], 1, noise=PhiloxNoise(seed=5), use_graph=False, image_quality=quality)
    finally:
        hook.remove()
    mean, logvar, x_nhwc = seen[-1]
    assert tuple(mean.shape) == (6, 16, 16, 3) and mean.stride() == (16 * 16 * 6, 16 * 6, 6, 1) and not mean.is_contiguous()
    assert logvar.data_ptr() == mean.data_ptr() + 3 * 4          # one parameter tensor: (mean | logvar)
    assert quality.last_ptrs == (x_nhwc.data_ptr(), mean.data_ptr())
    per = image_quality(x, mean.permute(0, 3, 1, 2).contiguous())
    want = _sequential(np.zeros(5), torch.stack([per['mse'], per['psnr'], per['ssim']], 1).cpu().numpy())
    assert eager['quality/mse'] == want[1] / 6 and eager['quality/psnr'] == want[2] / 6 and eager['quality/ssim'] == want[4] / 6
    replayed = test_pass(m, [x], 1, noise=PhiloxNoise(seed=5), use_graph=True, image_quality=quality)
    assert replayed == eager


# ---------------------------------------------------------------------------------------------------------------------------------
# (8) the quality ladder
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,size', [('tiny_gauss', 16), ('tiny_cifar', 32)])
def test_quality_ladder(name, size):
    from lvae_amd.evaluate import quality_ladder
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.passes import eval_mode
    from lvae_amd.quality import image_quality
    g = load_golden(name)
    _fresh_table()
    m = _model(g.cfg, g.state_dict(), PhiloxNoise(7))
    xs = [_images(5, 60, size).cuda(), _images(3, 61, size).cuda()]
    L = m.n_layers
    rows = quality_ladder(m, xs, temperature=0.0)
    assert rows.shape == (L + 1, 3) and rows.dtype == np.float64 and np.isfinite(rows).all()
    assert m.training                                          # the mode is put back
    m.noise = PhiloxNoise(7)
    assert np.array_equal(quality_ladder(m, xs, temperature=0.0), rows)   # run to run, bit for bit
    if name == 'tiny_gauss':   # a head with a mean: row L is the use_mode reconstruction, whatever the noise source holds
        per = []
        with torch.no_grad(), eval_mode(m):
            for x in xs:
                out = m.sample_conditional(x, L, 1, temperature=0.0, use_mode=True)
                q = image_quality(x, out['mean'])
                per.append(torch.stack([q['mse'], q['psnr'], q['ssim']], 1).cpu().numpy())
        want = _sequential(np.zeros(5), np.concatenate(per))
        assert rows[L].tolist() == [want[1] / 8, want[2] / 8, want[4] / 8]
        assert not np.array_equal(rows[L], rows[0])            # (the golden weights are untrained: which row is better says nothing)


# ---------------------------------------------------------------------------------------------------------------------------------
# (9) the command lines
# ---------------------------------------------------------------------------------------------------------------------------------
_TINY_ARGV = ['-d', 'cifar10', '--zdims', '8', '8', '--downsample', '1', '1', '--nfilters', '16', '--skip', '--gated', '--freebits', '1.0',
              '--batch-size', '8', '--synthetic', '--seed', '3']
_SUFFIX = re.compile(r'   PSNR: (\S+) dB   SSIM: (\S+)$')


def test_evaluation_cli(tmp_path, monkeypatch, capsys):
    import lvae_amd  # noqa: F401
    from lvae_amd import evaluate as leval
    monkeypatch.chdir(tmp_path)
    img_dir = str(tmp_path / 'pics')
    leval.main(_TINY_ARGV + ['--n-test', '16', '--test-batch-size', '8', '--ll', '--ll-samples', '2', '--image-quality', '--recons',
                             '--img-dir', img_dir, '--quality-ladder', '--inpaint', '--inpaint-iters', '2'])
    out = capsys.readouterr().out.splitlines()
    test_line = [l for l in out if 'ELBO' in l]
    assert len(test_line) == 1 and _SUFFIX.search(test_line[0]), out
    psnr, ssim = (float(v) for v in _SUFFIX.search(test_line[0]).groups())
    assert 0 < psnr < 60 and -1 <= ssim <= 1
    rec = [l for l in out if l.startswith('reconstructions of 16 images: mse ')]
    assert len(rec) == 1 and re.search(r'PSNR \S+ dB \(of the mean mse: \S+ dB\)   SSIM \S+$', rec[0]), out
    assert os.path.exists(os.path.join(img_dir, 'reconstructions.png'))
    rows = np.load(str(tmp_path / 'quality_ladder.npy'))
    assert rows.shape == (3, 3) and rows.dtype == np.float64 and np.isfinite(rows).all()
    ladder = [l for l in out if l.startswith('quality ladder top ')]
    assert ladder == ['quality ladder top %d of 2 layers: mse %.5g   PSNR %.2f dB   SSIM %.4f' % ((k,) + tuple(rows[k])) for k in range(3)]
    inp = [l for l in out if l.startswith('inpaint left ')]
    m = re.search(r'mse on the missing pixels (\S+) \(initial fill\) -> (\S+) \(completion\); .*; PSNR on the missing pixels (\S+) dB -> (\S+) dB; '
                  r'SSIM at the missing centres (\S+) -> (\S+)$', inp[0])
    assert len(inp) == 1 and m, out
    mse0, mse1, p0, p1, s0, s1 = (float(v) for v in m.groups())
    assert all(math.isfinite(v) for v in (p0, p1, s0, s1))
    # 'left' hides the same number of pixels in every image, and Jensen: the mean of the per-image PSNRs is at least the PSNR of the mean mse
    assert p0 >= 10 * math.log10(1 / mse0) - 0.01 and p1 >= 10 * math.log10(1 / mse1) - 0.01


def test_trainer_flag(tmp_path):
    hist = str(tmp_path / 'h.jsonl')
    argv = _TINY_ARGV + ['--synthetic-test', '16', '--test-batch-size', '8', '--ts-log-every', '2', '--steps', '4', '--log-every', '2',
                         '--image-quality', '--history', hist]
    p = subprocess.run([sys.executable, '-m', 'lvae_amd.main'] + argv, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if re.search(r'\[step \d+, epoch', l)]
    assert len(lines) == 2 and all(_SUFFIX.search(l) for l in lines), p.stdout
    recs = [json.loads(l) for l in open(hist).read().splitlines()]
    tests = [r for r in recs if r['split'] == 'test']
    assert [r['step'] for r in tests] == [2, 4]
    for r, line in zip(tests, lines):
        assert QUALITY_KEYS <= set(r['metrics']) and r['metrics']['n_images'] == 16
        assert line.endswith('   PSNR: %.2f dB   SSIM: %.4f' % (r['metrics']['quality/psnr'], r['metrics']['quality/ssim']))
