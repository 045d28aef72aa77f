"""Training on the K-sample importance-weighted bound: the loss head and the broadcast over samples against the plain torch formula, the
whole model against the CPU oracle composed with one bottom-up pass for K samples, the captured step against eager launches, the
refusals, the untouched default and the bf16 step.

Rows are sample-major: row k * B + b is sample k of image b. The yardsticks are those of tests/test_elementwise_gpu.py
(docs/ELEMENTWISE_PARITY.md), none chosen here: r64 is the formula in float64 on the CPU (gradients by autograd), r32 the same in float32,

    element-wise (w, d_ll, d_kl_sep)              |kernel - r64| <= 2 max|r32 - r64| + 1e-5 |r64| + 1e-6
    per-sample sums (bound, the scalars, ess)     |kernel - r64| <= 2 max|r32 - r64| + 4e-6 sum_i |term_i|

The terms of bound[b] = max_k lw + log sum_k exp(lw - max) - log K are its three addends; the terms of a mean over images or rows are
the (absolute) per-image or per-row values divided by their number, with |ll| + |kl_sep| standing for a row's ll - kl_sep."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_elementwise_gpu import close_elem, close_sum, finite, leaf
from test_ema_gpu import _assert_same_state, _fresh_table, _images, _model, _train_state

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 5), (2, 1), (3, 7), (5, 64), (64, 3), (8, 257)]
ANNEAL = 10
G = 0.37   # upstream gradient of the loss


@pytest.fixture(scope='module')
def K():
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels
    return kernels


def _rows(K_, B, seed):
    """ll ~ -550 +- 5, kl_sep ~ 30 +- 5"""
    gen = torch.Generator().manual_seed(seed)
    return -550.0 + 5.0 * torch.randn(K_ * B, generator=gen), 30.0 + 5.0 * torch.randn(K_ * B, generator=gen)


def _betas():
    """(tag, beta as the kernel receives it, device counter or None): three float betas, then the annealed form below, inside and past the ramp"""
    from lvae_amd.engine import linear_anneal
    out = [('beta %g' % b, float(np.float32(b)), None) for b in (0.0, 0.3, 1.0)]
    out += [('anneal step %d' % s, float(np.float32(linear_anneal(s, 0.0, 1.0, ANNEAL))), s) for s in (-3, 4, 25)]
    assert [b for _, b, _ in out[3:]] == [0.0, float(np.float32(0.4)), 1.0]
    return out


def _ref(ll, kl, beta, K_, B, dt):
    ll, kl = leaf(ll, dt), leaf(kl, dt)
    lw = (ll - beta * kl).view(K_, B)
    mx = lw.max(0).values
    lse = torch.log(torch.exp(lw - mx).sum(0))
    bound = torch.logsumexp(lw, 0) - math.log(K_)
    w = torch.softmax(lw, 0)
    e = (ll - kl).view(K_, B)
    iw_b = torch.logsumexp(e, 0) - math.log(K_)
    ess_b = 1.0 / (w * w).sum(0)
    loss = -bound.mean()
    (G * loss).backward()
    d = lambda t: t.detach()
    emx = e.max(0).values
    return {'bound': d(bound), 'w': d(w).reshape(-1), 'loss': d(loss), 'elbo': d(e.mean()), 'recons': d((-ll).mean()), 'iw': d(iw_b.mean()),
            'ess': d(ess_b.mean()), 'd_ll': ll.grad, 'd_kl': kl.grad,
            'bound_abs': d(mx.abs() + lse.abs() + math.log(K_)),
            'iw_abs': d((emx.abs() + torch.log(torch.exp(e - emx).sum(0)).abs() + math.log(K_)).mean()),
            'loss_abs': d(bound.abs().mean()), 'elbo_abs': d((ll.abs() + kl.abs()).mean()), 'recons_abs': d(ll.abs().mean()),
            'ess_abs': d(ess_b.mean())}


def _run_head(K, ll, kl, beta, step, K_):
    dll, dkl = ll.cuda(), kl.cuda()
    g = torch.tensor([G], device='cuda')
    if step is None:
        elbo_sep, w, bound, scal = K.iw_loss_fwd(dll, dkl, beta, K_)
        d_ll, d_kl = K.iw_loss_bwd(g, w, beta, K_)
    else:
        ctr = torch.tensor([step], dtype=torch.int64, device='cuda')
        elbo_sep, w, bound, scal = K.iw_loss_fwd_anneal(dll, dkl, ctr, ANNEAL, K_)
        d_ll, d_kl = K.iw_loss_bwd_anneal(g, w, ctr, ANNEAL, K_)
    return elbo_sep, w, bound, scal, d_ll, d_kl


def _check_head(K, tag, ll, kl, beta, step, K_, B, elbo_finite=True):
    r64, r32 = _ref(ll, kl, beta, K_, B, torch.float64), _ref(ll, kl, beta, K_, B, torch.float32)
    skip = () if elbo_finite else ('elbo', 'recons', 'elbo_abs', 'recons_abs')
    finite({k: v for k, v in r64.items() if k not in skip}, {k: v for k, v in r32.items() if k not in skip})
    elbo_sep, w, bound, scal, d_ll, d_kl = _run_head(K, ll, kl, beta, step, K_)
    close_sum(tag + ' bound', bound, r64['bound'], r32['bound'], r64['bound_abs'])
    for i, name in enumerate(('loss', 'elbo', 'recons', 'iw', 'ess')):
        if name in skip:
            assert float(scal[i]) == float(r64[name]) and math.isinf(float(scal[i])), (tag, name, float(scal[i]), float(r64[name]))
            continue
        close_sum(tag + ' ' + name, scal[i], r64[name], r32[name], r64[name + '_abs'])
    close_elem(tag + ' w', w, r64['w'], r32['w'])
    close_elem(tag + ' d_ll', d_ll, r64['d_ll'], r32['d_ll'])
    close_elem(tag + ' d_kl_sep', d_kl, r64['d_kl'], r32['d_kl'])
    return elbo_sep, w, bound, scal, d_ll, d_kl


@pytest.mark.parametrize('K_,B', SHAPES)
def test_loss_head_against_the_float64_formula(K, K_, B):
    ll, kl = _rows(K_, B, 100 * K_ + B)
    zero = torch.zeros(1, device='cuda')
    for name, beta, step in _betas():
        tag = 'iw loss K%d B%d %s' % (K_, B, name)
        elbo_sep, w, bound, scal, d_ll, d_kl = _check_head(K, tag, ll, kl, beta, step, K_, B)
        # elbo_sep is produced as the ELBO loss produces it
        assert torch.equal(elbo_sep, K.elbo_loss_fwd(ll.cuda(), kl.cuda(), zero, 1.0)[0])
        if K_ == 1:   # one sample: the weight is exactly 1 and the gradients exactly those of a mean over the batch
            assert torch.equal(w, torch.ones(B, device='cuda'))
            assert torch.equal(d_ll.cpu(), torch.full((B,), -G) / B)
            assert torch.equal(d_kl.cpu(), torch.full((B,), G) * np.float32(beta) / B)


@pytest.mark.parametrize('K_,B', [(3, 7), (5, 64), (64, 3), (8, 257)])
def test_loss_head_at_a_wide_spread_at_ties_and_at_minus_infinity(K, K_, B):
    for name, beta, step in [b for b in _betas() if b[0] in ('beta 0.3', 'beta 1', 'anneal step 4')]:
        # image 0: log weights spread over +-1e4, so that all weights but one underflow to exactly 0
        ll, kl = _rows(K_, B, 7 * K_ + B)
        order = torch.randperm(K_, generator=torch.Generator().manual_seed(K_))
        ll.view(K_, B)[:, 0] = -550.0 + torch.linspace(-1e4, 1e4, K_)[order]
        _, w, _, _, d_ll, _ = _check_head(K, 'iw loss K%d B%d %s spread 1e4' % (K_, B, name), ll, kl, beta, step, K_, B)
        w0 = w.view(K_, B)[:, 0].cpu()
        top = int(torch.argmax(ll.view(K_, B)[:, 0] - beta * kl.view(K_, B)[:, 0]))
        assert float(w0[top]) == 1.0 and int((w0 == 0).sum()) == K_ - 1
        assert int((d_ll.view(K_, B)[:, 0] == 0).sum()) == K_ - 1
        # image 1: exact ties
        ll, kl = _rows(K_, B, 11 * K_ + B)
        ll.view(K_, B)[:, 1] = ll[1]
        kl.view(K_, B)[:, 1] = kl[1]
        _, w, _, _, _, _ = _check_head(K, 'iw loss K%d B%d %s ties' % (K_, B, name), ll, kl, beta, step, K_, B)
        w1 = w.view(K_, B)[:, 1]
        assert bool((w1 == w1[0]).all()) and float(w1[0]) == float(np.float32(1.0 / K_))
        # image 2: one row at -inf among finite ones weighs exactly nothing and makes nothing NaN (elbo and recons, means over all rows
        # that include the row, are -inf and +inf as the formula has them)
        ll, kl = _rows(K_, B, 13 * K_ + B)
        ll.view(K_, B)[K_ // 2, 2] = -math.inf
        out = _check_head(K, 'iw loss K%d B%d %s one -inf row' % (K_, B, name), ll, kl, beta, step, K_, B, elbo_finite=False)
        elbo_sep, w, bound, scal, d_ll, d_kl = out
        n = (K_ // 2) * B + 2
        assert float(w[n]) == 0.0 and float(d_ll[n]) == 0.0 and float(d_kl[n]) == 0.0 and float(elbo_sep[n]) == -math.inf
        for t in (w, bound, d_ll, d_kl, scal):
            assert not bool(torch.isnan(t).any())


def test_loss_head_refuses_rows_that_are_not_whole_images(K):
    from lvae_amd._C import LvaeHipError
    ll, kl = _rows(1, 7, 1)
    with pytest.raises(LvaeHipError):
        K.iw_loss_fwd(ll.cuda(), kl.cuda(), 1.0, 2)


# ---------------------------------------------------------------------------------------------------------------------------------
# broadcast over samples
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (3, 5, 7, 1), (4, 4, 8, 8), (4, 8, 8, 64)], ids=['n1', 'n105', 'n1024', 'n16384'])
@pytest.mark.parametrize('K_', [1, 2, 3, 8])
def test_broadcast_over_samples_is_exact_both_ways(K, shape, K_):
    from lvae_amd import ops
    gen = torch.Generator().manual_seed(K_ + shape[1])
    x = torch.randn(shape, generator=gen)
    dout = torch.randn((K_ * shape[0],) + shape[1:], generator=gen) * 10.0 ** torch.randint(-3, 4, (K_ * shape[0], 1, 1, 1), generator=gen).float()
    want = dout[:shape[0]].clone()
    for k in range(1, K_):   # the sequential float32 sum in ascending k
        want = want + dout[k * shape[0]:(k + 1) * shape[0]]
    out = K.repeat_samples(x.cuda(), K_)
    assert out.shape == dout.shape and torch.equal(out.cpu(), x.repeat(K_, 1, 1, 1))
    assert torch.equal(K.repeat_samples_bwd(dout.cuda(), K_).cpu(), want)
    xg = x.cuda().requires_grad_(True)   # and as the autograd node the model uses
    y = ops.RepeatSamplesFn.apply(xg, K_)
    y.backward(dout.cuda())
    assert torch.equal(y.detach().cpu(), x.repeat(K_, 1, 1, 1)) and torch.equal(xg.grad.cpu(), want)


# ---------------------------------------------------------------------------------------------------------------------------------
# whole model against the oracle: bottom-up on B images, each level and x repeated K times, top-down and likelihood on K * B rows
# ---------------------------------------------------------------------------------------------------------------------------------
def relerr(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-20))


@pytest.mark.parametrize('name', ['tiny_mnist', 'tiny_cifar'])
def test_whole_model_matches_the_oracle_composed_with_one_bottom_up_pass(name):
    import lvae_amd  # noqa: F401
    from lvae_amd import ops
    from lvae_amd.models.lvae import LadderVAE
    from lvae_amd.noise import TapeNoise
    from oracle import lvae_ref as R
    B, K_ = 4, 3
    g = load_golden(name)
    cfg = dict(g.cfg, free_bits=0.0)   # (the golden models were trained with free bits, which the bound does not have)
    x = g.t('x')[:B]
    assert x.shape[0] == B
    # oracle, recording the tape
    sd = g.state_dict()
    pkeys = [k for k in sd if R.is_parameter_key(k)]
    for k in pkeys:
        sd[k].requires_grad_(True)
    tape = R.Tape(gen=torch.Generator().manual_seed(5))
    x_pad = R.pad_img_tensor(x, R.get_padded_size(cfg, x.shape))
    bu = R.bottomup_pass(sd, cfg, x_pad, tape, True)
    n_bu_draws = len(tape.entries)
    bu = [t.repeat(K_, 1, 1, 1) for t in bu]
    xr = x.repeat(K_, 1, 1, 1)
    h, td = R.topdown_pass(sd, cfg, tape, True, bu_values=bu)
    h = R.crop_img_tensor(h, x.shape[2:])
    ll_ref, _ = R.likelihood(sd, cfg, h, xr, tape)
    kl_sep_ref = torch.stack(td['kl'], dim=1).sum(1)
    lw_ref = ll_ref - kl_sep_ref
    loss_ref = -(torch.logsumexp(lw_ref.view(K_, B), 0) - math.log(K_)).mean()
    # (d) the draw order: bottom-up masks at B images, then every top-down draw at K * B rows
    assert all(e.shape[0] == B for e in tape.entries[:n_bu_draws]) and all(e.shape[0] == K_ * B for e in tape.entries[n_bu_draws:])
    assert 0 < n_bu_draws < len(tape.entries)

    # engine on the same weights, images and tape
    torch.manual_seed(0)
    m = LadderVAE(**cfg)
    m.load_state_dict(g.state_dict())
    m.cuda().train()
    m.noise = TapeNoise(tape.entries)
    m.zero_grad()
    out = m(x.cuda(), n_samples=K_)
    assert m.noise.exhausted()                                                       # (d)
    assert len(out) == 12
    for key in ('ll', 'kl_sep'):
        assert out[key].shape == (K_ * B,)
    assert all(z.shape[0] == K_ * B for z in out['z']) and all(s.shape[0] == K_ * B for s in out['kl_spatial'])
    assert out['out_sample'].shape[0] == K_ * B and out['kl'].dim() == 0 and out['kl_avg_layerwise'].shape == (len(cfg['z_dims']),)
    elbo_sep, loss, elbo, recons, iw, ess, w = ops.IwLossFn.apply(out['ll'], out['kl_sep'], 1.0, K_)
    # (a) per-row terms and the loss at the tolerances of test_forward_backward_matches_reference
    tol = dict(rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(out['ll'].detach().cpu(), ll_ref.detach(), **tol)
    torch.testing.assert_close(out['kl_sep'].detach().cpu(), kl_sep_ref.detach(), **tol)
    torch.testing.assert_close(out['kl'].detach().cpu(), kl_sep_ref.detach().mean(), **tol)
    torch.testing.assert_close(out['logp'].cpu(), td['logprob_p'].detach(), **tol)
    print('iw whole model %s: loss %.6f oracle %.6f' % (name, float(loss.detach()), float(loss_ref.detach())))
    torch.testing.assert_close(loss.detach().cpu(), loss_ref.detach(), rtol=1e-5, atol=0)
    # (b) the engine's weights against the float64 softmax of the engine's own log weights
    ll_e, kl_e = out['ll'].detach().cpu(), out['kl_sep'].detach().cpu()
    w64 = torch.softmax((ll_e.double() - kl_e.double()).view(K_, B), 0).reshape(-1)
    w32 = torch.softmax((ll_e - kl_e).view(K_, B), 0).reshape(-1)
    close_elem('iw whole model %s w' % name, w, w64, w32)
    assert float(w.view(K_, B).sum(0).sub(1).abs().max()) < 1e-6
    # (c) parameter gradients: the IWAE estimator given the weights, -sum_n w_engine[n] lw_oracle[n] / B through the oracle
    loss.backward()
    (-(w.detach().cpu() * lw_ref).sum() / B).backward()
    gsq = rsq = 0.0
    worst = (0.0, None)
    for k, p in m.named_parameters():
        if not p.requires_grad:
            continue
        ref_g = sd[k].grad
        gsq += float(p.grad.double().pow(2).sum())
        rsq += float(ref_g.double().pow(2).sum())
        if float(ref_g.norm()) < 1e-5:   # biases in front of a BatchNorm: mathematically zero
            assert float(p.grad.norm()) < 1e-4, k
            continue
        e = relerr(p.grad.cpu(), ref_g)
        if e > worst[0]:
            worst = (e, k)
    print('iw whole model %s: worst gradient rel L2 %.3e (%s), norm %.6f oracle %.6f' % (name, worst[0], worst[1], gsq ** 0.5, rsq ** 0.5))
    assert worst[0] < 1e-4, worst
    assert abs(gsq ** 0.5 - rsq ** 0.5) <= 1e-5 * rsq ** 0.5


# ---------------------------------------------------------------------------------------------------------------------------------
# the training step
# ---------------------------------------------------------------------------------------------------------------------------------
def _iw_cfg(name='tiny_cifar', **over):
    g = load_golden(name)
    return dict(g.cfg, free_bits=0.0, **over), g.state_dict()


def _step_run(use_graph, n_steps=3, **kw):
    from lvae_amd.engine import TrainStep
    from lvae_amd.noise import FrozenNoise
    from lvae_amd.optim import Adamax
    cfg, sd = _iw_cfg()
    _fresh_table()
    m = _model(cfg, sd, FrozenNoise(seed=3))
    opt = Adamax(m, lr=1e-3)
    st = TrainStep(m, opt, use_graph=use_graph, **kw)
    x = _images(4, 80).cuda()
    outs = [{k: v.detach().clone() for k, v in st(x).items()} for _ in range(n_steps)]
    torch.cuda.synchronize()
    assert (st.graph_a is not None) == use_graph
    return outs, _train_state(m, opt), m.arena.grads.detach().clone()


def test_captured_iw_step_equals_eager_bit_for_bit():
    """Two eager steps, then the third captured and replayed, against three eager steps, on one frozen noise tape."""
    graph, eager = _step_run(True, iw_samples=2), _step_run(False, iw_samples=2)
    for a, b in zip(graph[0], eager[0]):
        assert set(a) >= {'loss', 'iw', 'ess', 'elbo', 'recons', 'kl'}
        for k in a:
            assert torch.equal(a[k], b[k]), k
    last = graph[0][-1]
    assert all(bool(torch.isfinite(last[k]).all()) for k in last)
    assert 1.0 <= float(last['ess']) <= 2.0
    assert float(last['iw']) >= float(last['elbo']) - 1e-3 * abs(float(last['elbo']))   # Jensen: the bound is no looser than the mean ELBO
    assert torch.equal(graph[2], eager[2]) and bool((graph[2] != 0).any())              # the gradient arena
    _assert_same_state(graph[1], eager[1])                                              # parameters, Adamax state, BatchNorm buffers


def test_annealed_iw_step_moves_beta_inside_the_graph():
    """beta_anneal: the loss head reads beta from the device counter the step advances, so the replayed step differs from the step
    captured (same noise tape, lr as above) in the way the eager steps do."""
    graph, eager = _step_run(True, n_steps=4, iw_samples=2, beta_anneal=3), _step_run(False, n_steps=4, iw_samples=2, beta_anneal=3)
    for a, b in zip(graph[0], eager[0]):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    _assert_same_state(graph[1], eager[1])


def test_one_sample_step_is_the_step_without_the_keyword():
    from lvae_amd import _C
    from lvae_amd import kernels as K
    from lvae_amd.engine import TrainStep
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax
    g = load_golden('tiny_cifar')
    res = []
    real = _C.call
    for kw in ({}, {'iw_samples': 1}):
        _fresh_table()
        m = _model(g.cfg, g.state_dict(), PhiloxNoise(seed=3))
        names = []

        def counted(name, *args):
            names.append(name)
            return real(name, *args)

        _C.call = K.call = counted
        try:
            st = TrainStep(m, Adamax(m, lr=1e-3), use_graph=False, **kw)
            outs = [{k: v.detach().clone() for k, v in st(_images(4, 80 + i).cuda()).items()} for i in range(2)]
            torch.cuda.synchronize()
        finally:
            _C.call = K.call = real
        res.append((outs, m.arena.grads.detach().clone(), names))
    (o0, g0, n0), (o1, g1, n1) = res
    assert n0 == n1 and not any('iw_loss' in n or 'repeat_samples' in n for n in n1)    # the launches it issued before, no other
    assert torch.equal(g0, g1)
    for a, b in zip(o0, o1):
        assert a.keys() == b.keys() and 'iw' not in a
        for k in a:
            assert torch.equal(a[k], b[k]), k


def test_model_with_one_sample_is_the_model_without_the_keyword():
    from lvae_amd.noise import PhiloxNoise
    g = load_golden('tiny_cifar')
    x = _images(4, 81).cuda()
    outs = []
    for kw in ({}, {'n_samples': 1}):
        m = _model(g.cfg, g.state_dict(), PhiloxNoise(seed=3))
        with torch.no_grad():
            o = m(x, **kw)
        outs.append(o)
    for k in ('ll', 'kl_sep', 'kl', 'kl_loss', 'kl_avg_layerwise', 'logp', 'out_sample'):
        assert torch.equal(outs[0][k], outs[1][k]), k


def test_two_mask_shapes_are_drawn_in_two_launches():
    """The Dropout2d masks of a K-sample forward: one launch for the bottom-up blocks' (B, C) masks, one for the top-down blocks' (K * B, C)."""
    from lvae_amd import kernels as K
    from lvae_amd.noise import PhiloxNoise
    cfg, sd = _iw_cfg()
    m = _model(cfg, sd, PhiloxNoise(seed=3))
    drawn = []
    real_fill = K.rng_fill

    def spy(out, kind, *a):
        drawn.append((kind, tuple(out.shape)))
        return real_fill(out, kind, *a)

    K.rng_fill = spy
    try:
        with torch.no_grad():
            m(_images(4, 82).cuda(), n_samples=3)
    finally:
        K.rng_fill = real_fill
    masks = [s for k, s in drawn if k == 'bernoulli']
    bu, td = m._mask_plan(4, 3)
    assert masks == [(bu[0], 4, 8), (td[0], 12, 8)], masks


def test_refusals():
    from lvae_amd.engine import TrainStep, forward_pass
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax
    g = load_golden('tiny_cifar')
    x = _images(4, 83).cuda()
    with_free_bits = _model(g.cfg, g.state_dict(), PhiloxNoise(seed=3))
    assert with_free_bits.free_bits >= 1e-6
    with pytest.raises(ValueError, match='free'):
        forward_pass(with_free_bits, x, iw_samples=2)
    with pytest.raises(ValueError, match='free'):
        TrainStep(with_free_bits, Adamax(with_free_bits), iw_samples=2)
    analytical = _model(dict(g.cfg, free_bits=0.0, analytical_kl=True), g.state_dict(), PhiloxNoise(seed=3))
    with pytest.raises(ValueError, match='analytical'):
        forward_pass(analytical, x, iw_samples=2)
    with pytest.raises(ValueError):
        forward_pass(analytical, x, iw_samples=0)
    forward_pass(with_free_bits, x, iw_samples=1)   # both stay legal with one sample
    forward_pass(analytical, x, iw_samples=1)
    ok = _model(dict(g.cfg, free_bits=0.0), g.state_dict(), PhiloxNoise(seed=3))
    out = forward_pass(ok, x, iw_samples=2)
    assert out['elbo_sep'].shape == (8,) and out['iw'].dim() == 0 and out['ess'].dim() == 0 and out['iw_weights'].shape == (8,)


def test_bf16_iw_step_is_within_the_stated_tolerance_of_the_fp32_engine():
    """elbo relative <= 1e-2 between compute_dtype 'bf16' and the fp32 engine on the same weights, images and frozen noise
    (K = 2 on 8 images of the 3-layer MNIST architecture at 64 filters, without free bits). A bottom-up level's output is a block output
    and stays fp32 under bf16, so the fp32 broadcast is the only one: a bf16 tensor there would be refused by the binding."""
    import lvae_amd  # noqa: F401
    from lvae_amd import configs
    from lvae_amd import kernels as K
    from lvae_amd.engine import TrainStep
    from lvae_amd.models.lvae import LadderVAE
    from lvae_amd.noise import FrozenNoise
    from lvae_amd.optim import Adamax
    cfg = dict(configs.MNIST3, free_bits=0.0)
    noise = FrozenNoise(seed=9)
    x = configs.synthetic_images(cfg, 8, torch.Generator().manual_seed(77)).cuda()
    torch.manual_seed(42)
    init = {k: v.clone() for k, v in LadderVAE(**cfg).state_dict().items()}
    res = {}
    for dtype in ('f32', 'bf16'):
        model = LadderVAE(**cfg)
        model.load_state_dict(init)
        model.cuda().train()
        model.compute_dtype = dtype
        model.noise = noise
        _fresh_table()
        out = TrainStep(model, Adamax(model, lr=0.0), use_graph=False, iw_samples=2)(x)
        res[dtype] = {k: float(out[k]) for k in ('loss', 'elbo', 'iw', 'ess')}
    _fresh_table()
    K.set_precision('f32')
    a, b = res['f32']['elbo'], res['bf16']['elbo']
    print('iw bf16 step: f32 %r bf16 %r elbo rel %.3e' % (res['f32'], res['bf16'], abs(a - b) / abs(a)))
    assert all(math.isfinite(v) for r in res.values() for v in r.values())
    assert abs(a - b) <= 1e-2 * abs(a), (a, b)


# ---------------------------------------------------------------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------------------------------------------------------------
TRAINER = ['-d', 'cifar10', '--zdims', '8', '8', '--downsample', '1', '1', '--nfilters', '16', '--skip', '--gated', '--batch-size', '8',
           '--synthetic', '--seed', '3', '--log-every', '2', '--lr', '1e-3']


@pytest.mark.parametrize('window', [False, True], ids=['last-step', 'window-summaries'])
def test_trainer_prints_records_and_notes_the_objective(window, tmp_path, capsys):
    """--iw-train-samples 2 together with the KL warm-up, a scheduled lr and the weight average; then a resume with another K."""
    import json
    import re
    from lvae_amd import main as lmain
    _fresh_table()
    hist, ck = str(tmp_path / 'history.jsonl'), str(tmp_path / 'end.pt')
    argv = TRAINER + ['--steps', '6', '--history', hist, '--save-checkpoint', ck, '--iw-train-samples', '2', '--beta-anneal', '4',
                      '--lr-warmup', '2', '--ema-decay', '0.9'] + (['--window-summaries'] if window else [])
    lmain.main(argv)
    out = capsys.readouterr().out
    assert ',iw2,' in out.splitlines()[0], out
    lines = [ln for ln in out.splitlines() if re.search(r'\[step \d+\]', ln)]
    assert len(lines) == 3, out
    recs = [json.loads(r) for r in open(hist)]
    assert [r['step'] for r in recs] == [2, 4, 6]
    for ln, r in zip(lines, recs):
        m = re.search(r'   IW\(2\): (\S+)   ESS: (\S+)$', ln)
        assert m and '   lr: ' in ln and 'img/s]' in ln, ln
        iw, ess, elbo = r['metrics']['elbo/iw_train'], r['metrics']['iw/ess'], r['metrics']['elbo/elbo']
        assert m.group(1) == '{:.5g}'.format(iw) and m.group(2) == '{:.3g}'.format(ess)
        assert math.isfinite(iw) and 1.0 <= ess <= 2.0
        if not window:   # (a window's ELBO is a mean over steps; the bound is the last step's)
            assert iw >= elbo - 1e-3 * abs(elbo)
    assert torch.load(ck)['iw_train_samples'] == 2
    # the command line's K runs on --resume; rank 0 says when the file's was another
    _fresh_table()
    resume = TRAINER + ['--steps', '8', '--resume', ck, '--beta-anneal', '4', '--lr-warmup', '2', '--ema-decay', '0.9']
    lmain.main(resume)
    out = capsys.readouterr().out
    assert len([ln for ln in out.splitlines() if 'warning' in ln and '--iw-train-samples 2' in ln and 'continuing with 1' in ln]) == 1, out
    lines = [ln for ln in out.splitlines() if re.search(r'\[step \d+\]', ln)]
    assert len(lines) == 1 and '[step 8]' in lines[0] and 'IW(' not in lines[0], out
    _fresh_table()
    lmain.main(resume + ['--iw-train-samples', '2'])
    assert 'warning' not in capsys.readouterr().out
    _fresh_table()
