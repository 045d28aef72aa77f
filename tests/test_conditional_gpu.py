"""Conditional samples (the top k latents from an image's posterior, the layers below from the prior) and reduced-temperature prior samples:
the tempered-draw kernel against its formula, the mixed top-down pass against the CPU oracle on one noise tape, identities on the device,
and the evaluation CLI.

Kernel: r64 is the formula below in float64 on the CPU, r32 the same in float32, and the two rules of docs/ELEMENTWISE_PARITY.md hold
unchanged: element-wise for z, the per-sample-sum rule for logprob_p. Every comparison prints `yardstick | case | kernel error | r32 error |
bound` before it asserts (run with -s)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden

pytestmark = pytest.mark.gpu

INF = float('inf')


@pytest.fixture(scope='module')
def K():
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels
    return kernels


# ---------------------------------------------------------------------------------------------------------------------------------
# the two rules (tests/test_elementwise_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def _cmp(tag, got, r64, r32, floor):
    got, r64, r32 = got.detach().double().cpu(), r64.detach().double(), r32.detach().double()
    assert got.shape == r64.shape == r32.shape, (tag, got.shape, r64.shape, r32.shape)
    e32 = float((r32 - r64).abs().max())
    bound = (2.0 * e32 + floor).expand_as(r64).reshape(-1)
    err = (got - r64).abs().reshape(-1)
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, INF))
    k = int(torch.argmax(err / bound.clamp(min=1e-300)))
    print('yardstick | %-58s | kernel %.3e | r32 %.3e | bound %.3e | n %d' % (tag, float(err[k]), e32, float(bound[k]), err.numel()))
    assert bool((err <= bound).all()), '%s: |kernel - r64| = %.6e at flat element %d, bound %.6e (r32 error %.3e)' % (
        tag, float(err[k]), k, float(bound[k]), e32)


def close_elem(tag, got, r64, r32):
    _cmp(tag, got, r64, r32, 1e-5 * r64.detach().double().abs() + 1e-6)


def close_sum(tag, got, r64, r32, abs_terms):
    _cmp(tag, got, r64, r32, 4e-6 * abs_terms.detach().double())


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. lvae_normal_prior_sample_f32
# ---------------------------------------------------------------------------------------------------------------------------------
LV_RANGES = [(-12., 6.), (-3., 2.)]   # as docs/ELEMENTWISE_PARITY.md
LOG_SQRT_2PI = 0.91893853320467274178

# (N, HW, Z, p_bcast, misaligned). A pass is 2,048 four-channel groups (16-byte map) or 4,096 elements (scalar map) of a row:
# 16-byte map, exactly one full pass; 16-byte map, 4,800 groups = two full passes and a ragged third; scalar map, a row shorter than one
# pass; scalar map, 4,500 elements = a full pass and a ragged second; the 1x1 top level, one row; Z % 4 == 0 but no power of two; the
# broadcast prior; p, eps and z each one float off a 16-byte boundary (a result check: nothing here observes which map ran), short and
# with 4,800 elements (past one scalar pass)
PS_CASES = [(3, 256, 32, 0, False), (2, 600, 32, 0, False), (2, 5, 3, 0, False), (2, 1500, 3, 0, False), (1, 1, 4, 0, False),
            (2, 7, 20, 0, False), (5, 16, 8, 1, False), (3, 16, 8, 0, True), (2, 600, 8, 0, True)]
SCALAR_T = [0.0, 0.5, 1.0, 1.7]


def _ps_inputs(N, HW, Z, bcast, lv, seed):
    g = torch.Generator().manual_seed(seed)
    n = 1 if bcast else N
    p = torch.cat((torch.randn(n, HW, 1, Z, generator=g), torch.rand(n, HW, 1, Z, generator=g) * (lv[1] - lv[0]) + lv[0]), -1)
    eps = torch.randn(N, HW, 1, Z, generator=g)
    flat = eps.view(-1)
    for j, v in enumerate((0.0, 6.0, -6.0)):   # eps contains 0 and +-6: elements j, j + 7, ...
        flat[j::7] = v
    return p, eps


def _ps_ref(p, eps, t_rows, Z):
    """z = mu where t == 0, else mu + (t sigma) eps; log N(z; mu, sigma^2) under the untempered prior, summed per row. dtype of p."""
    N = eps.shape[0]
    mu, lv = p[..., :Z].expand(N, -1, -1, -1), p[..., Z:].expand(N, -1, -1, -1)
    sd = (lv / 2).exp()
    t = t_rows.to(p.dtype).view(N, 1, 1, 1)
    z = torch.where(t == 0, mu, mu + (t * sd) * eps.to(p.dtype))
    lp = -((z - mu) ** 2) / (2 * sd ** 2) - sd.log() - LOG_SQRT_2PI
    return z, lp.sum((1, 2, 3)), lp.abs().sum((1, 2, 3))


def _off_by_one_float(t):
    """a contiguous device copy of t that starts 4 bytes past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, device='cuda')
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def _ps_run(K, p, eps, Z, N, scalar, row_t, misaligned):
    if not misaligned:
        return K.normal_prior_sample(p.cuda(), None if eps is None else eps.cuda(), Z, N, scalar, None if row_t is None else row_t.cuda())
    pd, ed = _off_by_one_float(p), _off_by_one_float(eps)
    z = _off_by_one_float(torch.zeros(N, p.shape[1], 1, Z))
    lp = torch.empty(N, device='cuda')
    rt = None if row_t is None else row_t.cuda()
    K.call('lvae_normal_prior_sample_f32', K.ptr(pd), 0, K.ptr(ed), float(scalar), K.ptr(rt), N, p.shape[1], Z, K.ptr(z), K.ptr(lp),
           K.stream_ptr())
    return z, lp


@pytest.mark.parametrize('case', PS_CASES, ids=lambda c: '%dx%dx%d%s%s' % (c[0], c[1], c[2], '-bcast' if c[3] else '', '-misaligned' if c[4] else ''))
def test_prior_sample_kernel_cases(K, case):
    N, HW, Z, bcast, misaligned = case
    cyc = (0.0, 0.5, 1.0)
    temps = [('t%g' % t, torch.full((N,), t), t, False) for t in SCALAR_T]
    temps += [('rows+%d' % r, torch.tensor([cyc[(n + r) % 3] for n in range(N)]), 1.0, True) for r in (0, 1)]   # per row: 0, 0.5 and 1 mixed
    jobs = []
    for lv in LV_RANGES:
        p, eps = _ps_inputs(N, HW, Z, bcast, lv, 100 + HW + Z)
        for name, t_rows, scalar, per_row in temps:
            t_rows = t_rows.float()   # the kernel is handed float32 temperatures: 1.7 is the float32 nearest to it in both references
            r64 = _ps_ref(p.double(), eps, t_rows, Z)
            r32 = _ps_ref(p, eps, t_rows, Z)
            assert all(bool(torch.isfinite(v).all()) for v in r64 + r32), 'a reference value is not finite'
            jobs.append(('prior_sample %dx%dx%d%s lv%g..%g %s' % (N, HW, Z, ' misaligned' if misaligned else (' bcast' if bcast else ''),
                                                                    lv[0], lv[1], name), p, eps, scalar, t_rows if per_row else None, r64, r32))
    for tag, p, eps, scalar, row_t, r64, r32 in jobs:   # every reference exists before the first tensor goes to the device
        z, lp = _ps_run(K, p, eps, Z, N, scalar, row_t, misaligned)
        assert tuple(z.shape) == (N, HW, 1, Z) and tuple(lp.shape) == (N,)
        close_elem(tag + ' z', z, r64[0], r32[0])
        close_sum(tag + ' logprob_p', lp, r64[1], r32[1], r64[2])
        zero_rows = (torch.full((N,), scalar) if row_t is None else row_t) == 0
        mu = p[..., :Z].expand(N, -1, -1, -1)
        assert torch.equal(z.cpu()[zero_rows], mu[zero_rows]), tag + ': z is not bit-equal to mu where t == 0'


@pytest.mark.parametrize('Z', [8, 3], ids=['float4', 'scalar'])
def test_prior_sample_temperature_zero_is_a_branch(K, Z):
    """t = 0: z is mu bit for bit with logvar = 200 (sigma = inf), with eps absent, and with eps = inf / 1e38 present; nothing is NaN."""
    N, HW = 3, 9
    g = torch.Generator().manual_seed(7)
    p = torch.cat((torch.randn(N, HW, 1, Z, generator=g), torch.full((N, HW, 1, Z), 200.0)), -1)
    wild = torch.randn(N, HW, 1, Z, generator=g)
    wild.view(-1)[0::3] = INF
    wild.view(-1)[1::3] = -1e38
    mu = p[..., :Z]
    for tag, eps, scalar, row_t in (('eps absent', None, 0.0, None), ('eps wild', wild, 0.0, None), ('rows 0', wild, 1.0, torch.zeros(N))):
        z, lp = _ps_run(K, p, eps, Z, N, scalar, row_t, False)
        assert torch.equal(z.cpu(), mu), tag
        assert not bool(torch.isnan(lp).any()), tag
    # rows 0 and 2 at 0 beside a finite row: the zero rows stay exact whatever their eps holds
    p2 = torch.cat((mu, torch.full((N, HW, 1, Z), 1.0)), -1)
    z, lp = _ps_run(K, p2, wild, Z, N, 1.0, torch.tensor([0.0, 0.5, 0.0]), False)
    assert torch.equal(z.cpu()[[0, 2]], mu[[0, 2]]) and bool(torch.isfinite(lp.cpu()[[0, 2]]).all())


def test_prior_sample_refusals_leave_the_outputs_alone(K):
    from lvae_amd import _C
    N, HW, Z = 2, 4, 8
    p, eps, rt = torch.randn(N, HW, 1, 2 * Z).cuda(), torch.randn(N, HW, 1, Z).cuda(), torch.full((N,), 0.5).cuda()
    z, lp = torch.full((N, HW, 1, Z), 7.0).cuda(), torch.full((N,), 7.0).cuda()
    P = lambda t: None if t is None else t.data_ptr()
    ok = dict(p=p, eps=eps, t=0.5, rt=None, N=N, HW=HW, Z=Z, z=z, lp=lp)
    bad = [dict(p=None), dict(z=None), dict(lp=None),
           dict(eps=None), dict(eps=None, t=1.0), dict(eps=None, t=0.0, rt=rt),           # eps may be absent only with a scalar 0
           dict(N=0), dict(HW=0), dict(Z=0), dict(N=-1), dict(HW=-3), dict(Z=-8),
           dict(t=-0.5), dict(t=float('nan')), dict(t=INF), dict(t=-INF), dict(t=float('nan'), rt=rt)]
    lib = _C.load()
    for change in bad:
        a = dict(ok, **change)
        rc = lib.lvae_normal_prior_sample_f32(P(a['p']), 0, P(a['eps']), a['t'], P(a['rt']), a['N'], a['HW'], a['Z'], P(a['z']), P(a['lp']),
                                              K.stream_ptr())
        assert rc != 0, change
        assert lib.lvae_last_error(), change
    torch.cuda.synchronize()
    assert bool((z == 7.0).all()) and bool((lp == 7.0).all())
    with pytest.raises(_C.LvaeHipError):
        K.normal_prior_sample(p, None, Z, N, 0.5)
    z2, _ = K.normal_prior_sample(p, None, Z, N, 0.0)   # the legal absence
    assert torch.equal(z2, p[..., :Z])


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the mixed pass against the CPU oracle, on one noise tape
# ---------------------------------------------------------------------------------------------------------------------------------
class TemperedTape:
    """Round an oracle tape: the tape records (or replays) the unscaled draw; a `normal` draw is handed out multiplied by `t`, the
    temperature of the layer that is drawing (1 everywhere else)."""

    def __init__(self, tape):
        self.tape, self.t = tape, 1.0

    def draw(self, kind, shape, **kw):
        d = self.tape.draw(kind, shape, **kw)
        return d * self.t if kind == 'normal' else d


def ref_conditional(sd, cfg, x, k, n_samples, temps, tape, use_mode=False):
    """sample_conditional composed from the oracle's pieces (eval mode): bottom-up once, the top k layers in inference mode on the B rows,
    `repeat` to K * B rows, the layers below from the prior at temps[i] (at 0 through use_mode=True: no draw), final_top_down, crop,
    likelihood without a target. Returns (likelihood info, [z])."""
    from oracle import lvae_ref as R
    L, B = len(cfg['z_dims']), x.shape[0]
    tt = TemperedTape(tape)
    bu = R.bottomup_pass(sd, cfg, R.pad_img_tensor(x, R.get_padded_size(cfg, x.shape)), tt, False) if k > 0 else None
    out, z = None, [None] * L
    for i in reversed(range(L)):
        if i >= L - k:
            tt.t = 1.0
            out, _, aux = R.top_down_layer(sd, i, cfg, tt, False, out, out, True, bu[i], None, None, use_mode, False)
        else:
            if out is not None and i == L - k - 1:
                out = out.repeat(n_samples, 1, 1, 1)
            tt.t = 1.0 if temps[i] is None else float(temps[i])
            out, _, aux = R.top_down_layer(sd, i, cfg, tt, False, out, out, False, None, n_samples * B, None, tt.t == 0.0, False)
        z[i] = aux['z']
    tt.t = 1.0
    if k == L:
        out = out.repeat(n_samples, 1, 1, 1)
    j0 = 0
    if not cfg['no_initial_downscaling']:
        out = F.interpolate(out, scale_factor=2, mode='bilinear', align_corners=False)
        j0 = 1
    for j in range(cfg['blocks_per_layer']):
        out = R.resampling_block(sd, 'final_top_down.%d' % (j0 + j), out, cfg, 'top-down', False, cfg['gated'], tt, False)
    out = R.crop_img_tensor(out, x.shape[2:])
    _, info = R.likelihood(sd, cfg, out, None, tt)
    return info, z


def build(g, training=False):
    import lvae_amd  # noqa: F401
    from lvae_amd.models.lvae import LadderVAE
    torch.manual_seed(0)
    m = LadderVAE(**g.cfg)
    m.load_state_dict(g.state_dict(), strict=True)
    m.cuda()
    m.train(training)
    return m


ORACLE_TEMPS = {'tiny_cifar': [0.7, 1.0, 0.0], 'tiny_eval': [0.7, 0.0], 'tiny_gauss': [0.7, 0.0]}
ORACLE_CASES = [(name, k, False) for name, t in ORACLE_TEMPS.items() for k in range(len(t) + 1)] + [('tiny_cifar', 2, True)]
_REF = {}


def _oracle_reference(name, k, use_mode):
    """float64 oracle of one case, computed once: (info, z, tape entries)"""
    from oracle import lvae_ref as R
    key = (name, k, use_mode)
    if key not in _REF:
        g = load_golden(name)
        sd = {kk: (v.double() if v.is_floating_point() else v) for kk, v in g.state_dict().items()}
        tape = R.Tape(gen=torch.Generator().manual_seed(11 + k))
        with torch.no_grad():
            info, z = ref_conditional(sd, g.cfg, g.t('x').double(), k, 3, ORACLE_TEMPS[name], tape, use_mode)
        _REF[key] = (info, z, tape.entries)
    return _REF[key]


@pytest.mark.parametrize('name,k,use_mode', ORACLE_CASES, ids=lambda v: str(v))
def test_sample_conditional_matches_oracle(name, k, use_mode):
    from lvae_amd.noise import TapeNoise
    info, z_ref, entries = _oracle_reference(name, k, use_mode)
    g = load_golden(name)
    L, n_samples = len(g.cfg['z_dims']), 3
    x = g.t('x')
    B = x.shape[0]
    m = build(g)
    m.noise = TapeNoise(entries)
    with torch.no_grad():
        out = m.sample_conditional(x.cuda(), k, n_samples, temperature=ORACLE_TEMPS[name], use_mode=use_mode)
    assert m.noise.exhausted()
    assert not m.training
    for i in range(L):
        rows = B if i >= L - k else n_samples * B
        assert tuple(out['z'][i].shape) == tuple(z_ref[i].shape) and out['z'][i].shape[0] == rows
        torch.testing.assert_close(out['z'][i].cpu(), z_ref[i].float(), rtol=1e-4, atol=1e-4)
    tol = dict(rtol=1e-4, atol=2e-4)
    form = g.cfg['likelihood_form']
    assert out['sample'].shape[0] == n_samples * B and tuple(out['sample'].shape[1:]) == tuple(x.shape[1:])
    if form == 'bernoulli':
        mean_ref = info['mean']
        torch.testing.assert_close(out['mean'].cpu(), mean_ref.float(), **tol)
        torch.testing.assert_close(out['likelihood_params'].cpu(), mean_ref.float(), **tol)
        u = torch.as_tensor(entries[-1]).double()
        clear = (u - mean_ref).abs() > 2e-4
        inside = int((~clear).sum())
        print('bernoulli | %s k=%d | %d of %d pixels inside the 2e-4 margin' % (name, k, inside, clear.numel()))
        assert inside <= 1e-3 * clear.numel()
        assert torch.equal(out['sample'].cpu()[clear], (u < mean_ref).float()[clear])
    elif form == 'gaussian':
        for key in ('mean', 'mode', 'sample'):
            torch.testing.assert_close(out[key].cpu(), info[key].float(), **tol)
        torch.testing.assert_close(out['likelihood_params']['mean'].cpu(), info['params']['mean'].float(), **tol)
        torch.testing.assert_close(out['likelihood_params']['logvar'].cpu(), info['params']['logvar'].float(), **tol)
    else:
        assert out['mean'] is None and out['mode'] is None
        torch.testing.assert_close(out['likelihood_params']['all_params'].cpu(), info['params']['all_params'].float(), **tol)
        torch.testing.assert_close(out['sample'].cpu(), info['sample'].float(), **tol)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. identities on the device (PhiloxNoise: a fresh source of the same seed starts at the same step)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def cifar():
    g = load_golden('tiny_cifar')
    return build(g), g.t('x').cuda()


def _fresh(m, seed=5):
    from lvae_amd.noise import PhiloxNoise
    m.noise = PhiloxNoise(seed)
    return m


def test_sample_prior_temperature_one_and_none_are_the_plain_call(cifar):
    m, _ = cifar
    with torch.no_grad():
        a = _fresh(m).sample_prior(5).clone()
        b = _fresh(m).sample_prior(5, temperature=1.0).clone()
        c = _fresh(m).sample_prior(5, temperature=None).clone()
        d = _fresh(m).sample_prior(5, temperature=[1.0, 1.0, 1.0]).clone()
        e = _fresh(m).sample_prior(5, temperature=0.5).clone()
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)
    assert not torch.equal(a, e)


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_all_layers_from_the_posterior_is_the_forward_pass(cifar, dtype):
    m, x = cifar
    m.compute_dtype = dtype
    try:
        with torch.no_grad():
            fwd = [z.clone() for z in _fresh(m)(x)['z']]
            cond = _fresh(m).sample_conditional(x, m.n_layers, 1)['z']
        for a, b in zip(fwd, cond):
            assert torch.equal(a, b)
    finally:
        m.compute_dtype = 'f32'


@pytest.mark.parametrize('k', [1, 2])
def test_partial_conditioning_on_the_device(cifar, k):
    m, x = cifar
    L, B, n_samples = m.n_layers, x.shape[0], 3
    first = L - k - 1                      # the first layer that samples from the prior
    with torch.no_grad():
        fwd = [z.clone() for z in _fresh(m)(x)['z']]
        plain = [z.clone() for z in _fresh(m).sample_conditional(x, k, n_samples)['z']]
        at = {}
        for t in (0.0, 0.5, 1.0):
            temps = [1.0] * L
            temps[first] = t
            at[t] = _fresh(m).sample_conditional(x, k, n_samples, temperature=temps)['z'][first].clone()
        row_t = torch.tensor([(0.0, 0.5, 1.0)[r % 3] for r in range(n_samples * B)], device='cuda')
        per_row = _fresh(m).sample_conditional(x, k, n_samples, temperature=row_t)['z'][first].clone()
    for i in range(L):
        if i >= L - k:
            assert plain[i].shape[0] == B and torch.equal(plain[i], fwd[i])
        else:
            assert plain[i].shape[0] == n_samples * B
    v = plain[first].reshape(n_samples, B, -1)
    assert float((v[0] - v[1]).abs().max()) > 1e-3 and float((v[1] - v[2]).abs().max()) > 1e-3
    assert torch.equal(at[1.0], plain[first])
    # z_0.5 - z_0 = 0.5 (z_1 - z_0): the element-wise rule, with the float32 evaluation of the right-hand side on the CPU as the yardstick
    z0, zh, z1 = at[0.0].cpu(), at[0.5].cpu(), at[1.0].cpu()
    close_elem('tempering is linear in t, k=%d' % k, zh - z0, 0.5 * (z1.double() - z0.double()), 0.5 * (z1 - z0))
    # a per-row temperature gives, row by row, what the scalar calls give
    for r in range(n_samples * B):
        assert torch.equal(per_row[r], at[(0.0, 0.5, 1.0)[r % 3]][r]), r


def test_guards(cifar):
    m, x = cifar
    L = m.n_layers
    with torch.no_grad():
        for k in (-1, L + 1):
            with pytest.raises(ValueError):
                m.sample_conditional(x, k, 1)
        for n in (0, -2):
            with pytest.raises(ValueError):
                m.sample_conditional(x, 1, n)
        with pytest.raises(ValueError):
            m.sample_conditional(x, 1, 1, temperature=[0.5, 0.5])
        with pytest.raises(ValueError):
            m.sample_prior(2, temperature=-1.0)
        blk = m.top_down_layers[0].stochastic
        h = torch.zeros(2, 16, 16, m.n_filters, device='cuda')
        _fresh(m)._begin(x)   # packed parameters, fp32, a noise source that has begun
        for kw in (dict(q_params=h), dict(forced_latent=torch.zeros(2, 16, 16, blk.c_vars, device='cuda')), dict(use_mode=True)):
            with pytest.raises(ValueError):
                blk(h, noise=m.noise, temperature=0.5, **kw)
    hg = torch.zeros(2, 16, 16, m.n_filters, device='cuda', requires_grad=True)
    with pytest.raises(RuntimeError):   # no backward exists
        blk(hg, noise=m.noise, temperature=0.5)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the evaluation CLI
# ---------------------------------------------------------------------------------------------------------------------------------
def test_cond_samples_cli(tmp_path, monkeypatch):
    import lvae_amd  # noqa: F401
    from lvae_amd import evaluate as leval
    from lvae_amd.images import grid_shape
    from test_images_cpu import decode_png
    monkeypatch.chdir(tmp_path)
    img_dir = str(tmp_path / 'pics')
    argv = ['-d', 'cifar10', '--zdims', '8', '8', '--downsample', '1', '1', '--nfilters', '16', '--skip', '--gated',
            '--freebits', '1.0', '--batch-size', '8', '--synthetic', '--seed', '3', '--n-test', '16']
    leval.main(argv + ['--cond-samples', '--cond-variations', '2', '--cond-layers', '0', '1', '2', '--temperature', '0.8', '--img-dir', img_dir])
    n = leval.IMG_GRID_N
    data = torch.floor(256 * torch.rand((16, 3, 32, 32), generator=torch.Generator().manual_seed(3))) / 255   # main.synthetic_batch
    for k in (0, 1, 2):
        a = np.load(str(tmp_path / ('cond_samples_top%d.npy' % k)))
        assert a.shape == (n, 3, 3, 32, 32)
        assert np.array_equal(a[:, 0], data[:n].numpy())
        assert np.isfinite(a).all() and a.min() >= 0.0 and a.max() <= 1.0
        if k < 2:   # (with every layer from the posterior the variations differ only where the likelihood is sampled)
            assert np.abs(a[:, 1] - a[:, 2]).max() > 1e-3    # two variations, not one picture twice
        png = decode_png(open(os.path.join(img_dir, 'cond_samples_top%d.png' % k), 'rb').read())
        assert png.shape == tuple(grid_shape(n * 3, 3, 32, 32)) + (3,)
