"""Picture grids on the GPU: the grid kernel byte for byte against a numpy statement of make_grid + save_image, the padding rule against
torch.median, reconstructions against the CPU oracle, the trainer's picture pass leaving training untouched, and both command lines."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from test_images_cpu import decode_png

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the grid kernel
# ---------------------------------------------------------------------------------------------------------------------------------
def _special_values():
    """Every k/255 and (k + 0.5)/255 (the values whose byte changes with one rounding) with both fp32 neighbours, values outside [0, 1],
    infinities and NaN."""
    k = np.arange(255, dtype=np.float64)
    base = np.concatenate([k / 255.0, (k + 0.5) / 255.0]).astype(np.float32)
    vals = np.concatenate([base, np.nextafter(base, np.float32(-1)), np.nextafter(base, np.float32(2)),
                           np.array([-3.0, -1e-8, -0.0, 1.0, 1.0000001, 1.5, 1e30, -1e30, np.inf, -np.inf, np.nan], dtype=np.float32)])
    return vals.astype(np.float32)


def _test_images(n, c, h, w, seed):
    """(n, c, h, w) float32: uniform in [-0.2, 1.2] with the special values written over a stretch of it, at a place that moves with seed."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.2, 1.2, size=n * c * h * w).astype(np.float32)
    sp = _special_values()
    rng.shuffle(sp)
    m = min(sp.size, x.size)
    start = (seed * 977) % (x.size - m + 1)
    x[start:start + m] = sp[:m]
    return x.reshape(n, c, h, w), m == sp.size


def ref_bytes(v):
    """save_image's byte in numpy float32: the product and the sum are two operations, each rounded to fp32."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        t = v * np.float32(255.0)
        t = t + np.float32(0.5)
        t = np.where(np.isnan(t), np.float32(0.0), np.clip(t, np.float32(0.0), np.float32(255.0)))
    return t.astype(np.uint8)


def ref_grid(imgs, nrow, pad):
    """make_grid(imgs, nrow, padding=2, pad_value=pad) + save_image, restated: (Hg, Wg, 3) uint8. A single image is padded too."""
    n, c, h, w = imgs.shape
    xmaps = min(nrow, n)
    ymaps = -(-n // xmaps)
    canvas = np.full((3, (h + 2) * ymaps + 2, (w + 2) * xmaps + 2), np.float32(pad), dtype=np.float32)
    for k in range(n):
        y0, x0 = (k // xmaps) * (h + 2) + 2, (k % xmaps) * (w + 2) + 2
        canvas[:, y0:y0 + h, x0:x0 + w] = imgs[k]          # (one channel is broadcast to three)
    return np.ascontiguousarray(ref_bytes(canvas).transpose(1, 2, 0))


def ref_pad_value(imgs):
    """boilr's img_grid_pad_value with torch.median on the CPU: clamp, mean over channels in channel order with an fp32 division, border
    values of every image, 1.0 when their median is below 0.2."""
    t = torch.from_numpy(np.ascontiguousarray(imgs)).clamp(0.0, 1.0)
    s = t[:, 0]
    for ch in range(1, t.shape[1]):
        s = s + t[:, ch]
    m = s / float(t.shape[1])
    border = torch.cat([m[:, 0, :].reshape(-1), m[:, -1, :].reshape(-1), m[:, 1:-1, 0].reshape(-1), m[:, 1:-1, -1].reshape(-1)])
    return 1.0 if bool(torch.median(border) < 0.2) else 0.0


def _dev(x, layout):
    """x (n, c, h, w) numpy -> device tensor of that logical shape: NCHW contiguous, or the NCHW view of an NHWC buffer."""
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    if layout == 'nhwc':
        t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return t


GRID_CASES = [(c, n, nrow) for c in (1, 3) for n in (2, 5, 64, 144) for nrow in (8, 12)]


@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('c,n,nrow', GRID_CASES)
def test_grid_bytes_match_numpy(c, n, nrow, layout):
    from lvae_amd.images import grid_shape, image_grid
    h, w = (28, 20) if n < 144 else (16, 24)               # never square: a swapped H and W shows
    x, all_specials = _test_images(n, c, h, w, seed=7 * n + nrow + c)
    assert all_specials == (x.size >= _special_values().size)
    pad = ref_pad_value(x)
    want = ref_grid(x, nrow, pad)
    got = image_grid(_dev(x, layout), nrow)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == want.shape == grid_shape(n, nrow, h, w) + (3,)
    got = got.cpu().numpy()
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    if n % min(nrow, n):                                   # the last row has unfilled cells: they carry the padding colour
        assert (got[-(h + 2):, -(w + 2):] == ref_bytes(pad)).all()


def test_every_special_value_gets_the_numpy_byte():
    """One value per image of a single pixel, in all three channels: each special value's byte on its own."""
    from lvae_amd.images import image_grid
    sp = _special_values()
    n = sp.size
    x = np.repeat(sp.reshape(n, 1, 1, 1), 3, axis=1)        # n images of 1 x 1 x 3
    got = image_grid(torch.from_numpy(x).cuda(), n, pad_value=0.0).cpu().numpy()
    assert got.shape == (5, 3 * n + 2, 3)
    px = got[2, 2::3]                                      # row 2, columns 2, 5, 8, ...: the images
    assert np.array_equal(px, np.repeat(ref_bytes(sp).reshape(n, 1), 3, axis=1))
    # the two-rounding form is what is checked: some of these values round differently in exact arithmetic
    exact = np.clip(np.floor(sp.astype(np.float64)[np.isfinite(sp)] * 255.0 + 0.5), 0, 255).astype(np.uint8)
    assert (exact != ref_bytes(sp[np.isfinite(sp)])).any()


@pytest.mark.parametrize('nrow', [8, 12])
def test_interleaved_grid(nrow):
    from lvae_amd.images import image_grid
    a, _ = _test_images(36, 3, 20, 28, seed=1)
    b, _ = _test_images(36, 3, 20, 28, seed=2)
    both = np.stack([a, b], axis=1).reshape(72, 3, 20, 28)  # a[0], b[0], a[1], b[1], ...
    pad = ref_pad_value(both)
    got = image_grid(_dev(a, 'nchw'), nrow, second=_dev(b, 'nhwc')).cpu().numpy()
    assert np.array_equal(got, ref_grid(both, nrow, pad))
    got = image_grid(_dev(a, 'nhwc'), nrow, second=_dev(b, 'nchw'), pad_value=1.0).cpu().numpy()
    assert np.array_equal(got, ref_grid(both, nrow, 1.0))
    a1, b1 = a[:1, :1], b[:1, :1]                          # one pair of one-channel images
    got = image_grid(_dev(a1, 'nchw'), nrow, second=_dev(b1, 'nchw'), pad_value=0.0).cpu().numpy()
    assert np.array_equal(got, ref_grid(np.concatenate([a1, b1]), nrow, 0.0))


@pytest.mark.parametrize('pad', [0.0, 1.0, 0.5, 0.3, -2.0, 7.0])
def test_explicit_pad_value(pad):
    from lvae_amd.images import image_grid
    x, _ = _test_images(5, 3, 12, 10, seed=3)
    got = image_grid(_dev(x, 'nchw'), 3, pad_value=pad).cpu().numpy()
    assert np.array_equal(got, ref_grid(x, 3, pad))
    assert (got[0, 0] == ref_bytes(pad)).all() and (got[-1, -1] == ref_bytes(pad)).all()


def test_grid_refuses_what_it_cannot_draw():
    from lvae_amd import kernels as K
    from lvae_amd.images import image_grid
    with pytest.raises(K._C.LvaeHipError):
        image_grid(torch.zeros(4, 2, 8, 8).cuda(), 2)                           # two channels
    with pytest.raises(K._C.LvaeHipError):
        image_grid(torch.zeros(4, 3, 8, 8).cuda(), 2, second=torch.zeros(3, 3, 8, 8).cuda())
    with pytest.raises(K._C.LvaeHipError):
        image_grid(torch.zeros(4, 3, 8, 16).cuda()[..., ::2], 2)                # neither layout
    with pytest.raises(K._C.LvaeHipError):
        image_grid(torch.zeros(4, 3, 8, 8), 2)                                  # no CPU path
    with pytest.raises(K._C.LvaeHipError):
        image_grid(torch.zeros(4, 3, 8, 8).cuda(), 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the padding rule, decided on the device
# ---------------------------------------------------------------------------------------------------------------------------------
def _border_mask(h, w):
    m = np.zeros((h, w), dtype=bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return m


def _check_pad(x, layout='nchw', second=None):
    from lvae_amd.images import image_grid
    both = x if second is None else np.stack([x, second], axis=1).reshape((-1,) + x.shape[1:])
    pad = ref_pad_value(both)
    got = image_grid(_dev(x, layout), 8, second=None if second is None else _dev(second, layout)).cpu().numpy()
    assert (got[0, 0] == (255 if pad == 1.0 else 0)).all(), (pad, got[0, 0])
    assert np.array_equal(got, ref_grid(both, 8, pad))
    return pad


def test_pad_rule_random_batches():
    rng = np.random.default_rng(11)
    seen = set()
    for i in range(24):
        c = (1, 3)[i % 2]
        n, h, w = int(rng.integers(1, 20)), int(rng.integers(2, 14)), int(rng.integers(2, 14))
        # brightness levels around the threshold, so that both colours come up
        x = (rng.uniform(0.0, 1.0, size=(n, c, h, w)) * rng.uniform(0.2, 0.8)).astype(np.float32)
        seen.add(_check_pad(x, ('nchw', 'nhwc')[(i // 2) % 2]))
    assert seen == {0.0, 1.0}
    a = (rng.uniform(0.0, 0.3, size=(6, 3, 9, 7))).astype(np.float32)
    b = (rng.uniform(0.0, 1.0, size=(6, 3, 9, 7))).astype(np.float32)
    _check_pad(a, second=b)                                # the rule looks at both image sets
    _check_pad(np.full((3, 1, 1, 5), 0.1, np.float32))     # one row: rows 0 and H-1 are the same row, counted twice as torch does
    _check_pad(np.full((3, 3, 5, 1), 0.3, np.float32))


@pytest.mark.parametrize('c', [1, 3])
def test_pad_rule_with_values_exactly_at_the_threshold(c):
    """n_b = 112 border values, all exactly 0.2f except `below` of them at 0.1: the lower median is < 0.2 from below = 56 on."""
    n, h, w = 4, 8, 8
    mask = np.broadcast_to(_border_mask(h, w), (n, c, h, w))
    idx = np.argwhere(_border_mask(h, w))
    assert len(idx) * n == 112
    pads = {}
    for below in (0, 55, 56, 57, 112):
        x = np.full((n, c, h, w), 0.9, dtype=np.float32)
        x[mask] = np.float32(0.2)
        for j in range(below):
            img, (y, xx) = j % n, idx[j // n]
            x[img, :, y, xx] = np.float32(0.1)
        pads[below] = _check_pad(x, 'nhwc' if below % 2 else 'nchw')
    if c == 1:                                             # (with three channels the fp32 mean of three 0.2f decides where the step is)
        assert pads == {0: 0.0, 55: 0.0, 56: 1.0, 57: 1.0, 112: 1.0}
    else:
        assert pads[0] in (0.0, 1.0) and pads[112] == 1.0


def test_pad_rule_dark_bright_and_nan():
    dark = np.zeros((6, 3, 10, 12), dtype=np.float32)
    dark[:, :, 3:6, 3:6] = 1.0                             # bright inside, dark edges
    assert _check_pad(dark) == 1.0
    assert _check_pad(dark[:, :1], 'nhwc') == 1.0
    bright = np.ones((6, 3, 10, 12), dtype=np.float32)
    bright[:, :, 3:6, 3:6] = 0.0
    assert _check_pad(bright) == 0.0
    assert _check_pad(-5.0 * np.ones((2, 1, 4, 4), np.float32)) == 1.0   # clamped to 0 first
    assert _check_pad(5.0 * np.ones((2, 1, 4, 4), np.float32)) == 0.0
    nan = dark.copy()
    nan[2, 1, 0, 4] = np.nan                               # torch.median propagates a NaN, and NaN < 0.2 is false
    assert _check_pad(nan) == 0.0
    inside = dark.copy()
    inside[2, 1, 4, 4] = np.nan                            # not a border pixel: no influence
    assert _check_pad(inside) == 1.0


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. reconstructions against the oracle
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


@pytest.mark.parametrize('name', ['tiny_mnist', 'tiny_cifar'])
def test_reconstructions_match_oracle(name):
    """Tolerances: Bernoulli mean as test_model_gpu.test_forward_backward_matches_reference compares out_mean (rtol 1e-4, atol 1e-5); the
    logistic-mixture sample as test_kernels_gpu compares the sampler (in [-1, 1], rtol 1e-5, atol 1e-5)."""
    from oracle import lvae_ref as R
    from lvae_amd.evaluate import reconstructions
    from lvae_amd.noise import TapeNoise
    g = load_golden(name)
    x = g.t('x')
    tape = R.Tape(gen=torch.Generator().manual_seed(7))
    with torch.no_grad():
        mo = R.lvae_forward(g.state_dict(), g.cfg, x, tape, training=False)
    m = _model(g.cfg, g.state_dict(), TapeNoise(tape.entries))
    xin, rec = reconstructions(m, x)
    assert m.noise.exhausted() and m.training
    assert xin.is_cuda and rec.is_cuda and tuple(rec.shape) == tuple(x.shape) and torch.equal(xin.cpu(), x)
    if g.cfg['likelihood_form'] == 'bernoulli':
        print('%s: max |mean - oracle| = %.3e' % (name, float((rec.cpu() - mo['out_mean']).abs().max())))
        torch.testing.assert_close(rec.cpu(), mo['out_mean'], rtol=1e-4, atol=1e-5)
    else:
        assert mo['out_mean'] is None
        print('%s: max |sample - oracle| in [-1, 1] = %.3e' % (name, float((rec.cpu() * 2 - 1 - (mo['out_sample'] * 2 - 1)).abs().max())))
        torch.testing.assert_close(rec.cpu() * 2 - 1, mo['out_sample'] * 2 - 1, rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the picture pass leaves training untouched
# ---------------------------------------------------------------------------------------------------------------------------------
def _images(n, seed):
    return torch.floor(256 * torch.rand(n, 3, 32, 32, generator=torch.Generator().manual_seed(seed))) / 255


def _train_state(m, opt):
    sd = m.state_dict()   # (flushes the host-counted num_batches_tracked)
    bufs = {k: v.detach().clone() for k, v in sd.items() if not k.endswith(('weight', 'bias', 'top_prior_params'))}
    st = {'params': m.arena.params.detach().clone(), 'exp_avg': opt.exp_avg.clone(), 'exp_inf': opt.exp_inf.clone(),
          'adamax_step': opt.step_count.clone(), **bufs}
    if opt.ema is not None:
        st['ema'] = opt.ema.clone()
    return st


def _run_steps(m, opt, xs, between=None):
    from lvae_amd.engine import TrainStep
    st = TrainStep(m, opt, use_graph=True)
    outs = []
    for x in xs:
        outs.append({k: v.detach().clone() for k, v in st(x.cuda()).items()})
        if between is not None:
            between(m.global_step)
    torch.cuda.synchronize()
    return outs, st


def _same(a, b):
    return all((p is None and q is None) or torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize('decay', [0.0, 0.9])
def test_image_pass_does_not_perturb_training(decay):
    from lvae_amd import kernels as K
    from lvae_amd.evaluate import image_pass
    from lvae_amd.images import grid_shape
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax
    g = load_golden('tiny_cifar')
    xs = [_images(4, 10 + k) for k in range(6)]
    xt = _images(40, 30).cuda()
    res, grids = {}, {}
    for with_images in (False, True):
        _fresh_table()
        m = _model(g.cfg, g.state_dict(), PhiloxNoise(seed=3))
        opt = Adamax(m, lr=1e-3, ema_decay=decay)

        def between(step):
            if not with_images or step not in (2, 4):
                return
            before = m.arena.params.clone()
            ema_before = None if opt.ema is None else opt.ema.clone()
            P = K.prepared
            table_before = (dict(P.entries), P.table, P.enabled)
            noise_before = m.noise
            a = image_pass(m, 8, x=xt, step=step, optimizer=opt)
            b = image_pass(m, 8, x=xt, step=step, optimizer=opt)
            c = image_pass(m, 8, x=xt, step=step + 1, optimizer=opt)
            only_samples = image_pass(m, 8, step=step, optimizer=opt)
            torch.cuda.synchronize()
            assert tuple(a[0].shape) == grid_shape(64, 8, 32, 32) + (3,) == (274, 274, 3)
            assert tuple(a[1].shape) == grid_shape(64, 8, 32, 32) + (3,)        # 32 pairs
            assert _same(a, b)                                                    # the same step: the same pictures
            assert not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])    # another step: other noise
            assert only_samples[1] is None and torch.equal(only_samples[0], a[0])
            assert torch.equal(m.arena.params, before)                            # (with an average: exchanged back bit for bit)
            assert m.training and m.noise is noise_before and getattr(m, 'test_noise', None) is None
            assert P.table is table_before[1] and P.enabled == table_before[2]
            assert P.entries.keys() == table_before[0].keys() and all(P.entries[k] is v for k, v in table_before[0].items())
            if decay > 0.0:
                assert torch.equal(opt.ema, ema_before)
                raw = image_pass(m, 8, x=xt, step=step)                           # the weights as they are: not the average's pictures
                assert not torch.equal(raw[0], a[0]) and not torch.equal(raw[1], a[1])
            # the left half of a pair is the input itself
            assert np.array_equal(a[1].cpu().numpy()[2:34, 2:34], ref_bytes(xt[0].permute(1, 2, 0).cpu().numpy()))
            grids[step] = a

        outs, st = _run_steps(m, opt, xs, between=between)
        assert st.graph_a is not None
        res[with_images] = (outs, _train_state(m, opt), int(m.noise.step.item()))
    assert sorted(grids) == [2, 4]
    (o0, s0, n0), (o1, s1, n1) = res[False], res[True]
    assert n0 == n1 == 6
    for a, b in zip(o0, o1):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    assert s0.keys() == s1.keys()
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k


def test_image_pass_with_few_test_images_and_one_channel():
    """Fewer than nrows^2 // 2 test images: the grid shows what there is. Bernoulli: the reconstruction is the mean, one channel."""
    from lvae_amd.evaluate import image_pass
    from lvae_amd.images import grid_shape
    from lvae_amd.noise import PhiloxNoise
    g = load_golden('tiny_mnist')
    m = _model(g.cfg, g.state_dict(), PhiloxNoise(seed=5))
    x = (torch.rand(5, 1, 28, 28, generator=torch.Generator().manual_seed(1)) > 0.5).float()
    sample_grid, recon_grid = image_pass(m, 4, x=x, step=9)
    assert tuple(sample_grid.shape) == grid_shape(16, 4, 28, 28) + (3,)
    assert tuple(recon_grid.shape) == grid_shape(10, 4, 28, 28) + (3,)
    r = recon_grid.cpu().numpy()
    assert (r[..., 0] == r[..., 1]).all() and (r[..., 0] == r[..., 2]).all()
    assert np.array_equal(r[2:30, 2:30, 0], ref_bytes(x[0, 0].numpy()))
    assert m.training and int(m.noise.step.item() if m.noise.step is not None else 0) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the command lines
# ---------------------------------------------------------------------------------------------------------------------------------
def _run(module, argv, cwd):
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + (os.pathsep + env['PYTHONPATH'] if env.get('PYTHONPATH') else '')
    p = subprocess.run([sys.executable, '-m', module] + argv, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return p


def test_main_writes_pictures_and_trains_as_before(tmp_path):
    from lvae_amd.images import grid_shape
    saved = {}
    for tag, extra in (('plain', []), ('pictures', ['--img-dir', str(tmp_path / 'pics'), '--ts-img-every', '4'])):
        ck = tmp_path / ('ck_' + tag)
        argv = ['-d', 'cifar10', '--zdims', '8', '8', '--downsample', '1', '1', '--nfilters', '16', '--skip', '--gated', '--freebits', '1.0',
                '--batch-size', '8', '--synthetic', '--seed', '3', '--synthetic-test', '64', '--test-batch-size', '24',
                '--ts-log-every', '2', '--ll-every', '4', '--ll-samples', '8', '--checkpoint-every', '2', '--keep-checkpoint-max', '2',
                '--checkpoint-dir', str(ck), '--beta-anneal', '3', '--steps', '8', '--log-every', '4']
        _run('lvae_amd.main', argv + extra, ROOT)
        assert sorted(os.listdir(ck)) == ['model_6.pt', 'model_8.pt']
        saved[tag] = torch.load(str(ck / 'model_8.pt'))
    assert sorted(os.listdir(tmp_path / 'pics')) == ['reconstruction_4.png', 'reconstruction_8.png', 'sample_4.png', 'sample_8.png']
    assert not (tmp_path / 'ck_plain' / 'pics').exists()
    pics = {}
    for step in (4, 8):
        s = decode_png(open(str(tmp_path / 'pics' / ('sample_%d.png' % step)), 'rb').read())
        r = decode_png(open(str(tmp_path / 'pics' / ('reconstruction_%d.png' % step)), 'rb').read())
        assert s.shape == grid_shape(64, 8, 32, 32) + (3,) == (274, 274, 3)
        assert r.shape == grid_shape(48, 8, 32, 32) + (3,) == (206, 274, 3)     # the first test batch holds 24 images: 24 pairs
        assert len(np.unique(s)) > 16 and len(np.unique(r)) > 16                # pictures, not a flat canvas
        pics[step] = (s, r)
    assert not np.array_equal(pics[4][0], pics[8][0])
    a, b = saved['plain'], saved['pictures']
    assert a['model'].keys() == b['model'].keys()
    for k in a['model']:
        assert torch.equal(a['model'][k], b['model'][k]), k
    assert a['noise'] == b['noise'] and a['test_noise'] == b['test_noise'] and a['global_step'] == b['global_step'] == 8


def test_evaluate_writes_pictures_beside_the_arrays(tmp_path):
    pics = tmp_path / 'pics'
    argv = ['-d', 'cifar10', '--zdims', '8', '8', '--downsample', '1', '1', '--nfilters', '16', '--skip', '--gated', '--freebits', '1.0',
            '--batch-size', '8', '--synthetic', '--seed', '3', '--ll', '--ll-samples', '2', '--n-test', '80', '--test-batch-size', '40',
            '--ps', '--layer-repr', '--recons', '--img-dir', str(pics)]
    p = _run('lvae_amd.evaluate', argv, str(tmp_path))
    assert 'ELBO' in p.stdout, p.stdout
    assert sorted(os.listdir(pics)) == ['reconstructions.png', 'sample_mode_layer0.png', 'sample_mode_layer1.png', 'samples_0.png']
    for name in os.listdir(pics):
        img = decode_png(open(str(pics / name), 'rb').read())
        assert img.shape == (410, 410, 3), name                                 # 12 x 12 pictures of 32 x 32
        assert len(np.unique(img)) > 16, name
    assert np.load(str(tmp_path / 'prior_samples.npy')).shape == (64, 3, 32, 32)
    for i in range(2):
        assert np.load(str(tmp_path / ('layer_repr_%d.npy' % i))).shape == (64, 3, 32, 32)
    # --recons alone says what it needs
    q = subprocess.run([sys.executable, '-m', 'lvae_amd.evaluate', '--synthetic', '--recons'], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert q.returncode != 0 and '--img-dir' in q.stderr
