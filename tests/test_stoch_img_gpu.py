"""Fused stochastic block of the low-resolution levels (csrc/stoch_img.hip, lvae_stoch_block_fwd_f32, ops.StochBlockFn) against a plain
torch float64 statement of lib/stochastic.py:45-99 and its autograd, against the one-kernel-per-op path on the same inputs, and inside
one training step of a small model."""
import contextlib
import math
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

C, Z = 64, 32
SHAPES = [(1, 8, 8), (3, 8, 8), (5, 4, 4), (9, 2, 2), (2, 4, 8), (3, 2, 4), (1, 1, 1)]   # (5, 4, 4): the last tile is partly empty
LOG_SQRT_2PI = 0.5 * math.log(2 * math.pi)


@pytest.fixture(scope='module')
def E():
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels, ops, resblock
    from lvae_amd.lib.stochastic import NormalStochasticBlock2d
    return types.SimpleNamespace(K=kernels, ops=ops, RB=resblock, Block=NormalStochasticBlock2d)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().float().cuda()


def nchw(t):
    return t.detach().permute(0, 3, 1, 2).cpu().double()


def rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


class Tape:
    """noise source that hands out one given eps tensor"""

    def __init__(self, eps):
        self.eps = eps

    def normal(self, shape, device):
        assert tuple(shape) == tuple(self.eps.shape)
        return self.eps


@contextlib.contextmanager
def nan_outputs():
    """every float tensor torch.empty / empty_like hands out inside is NaN: a kernel that leaves part of an output unwritten shows"""
    e, el = torch.empty, torch.empty_like

    def fill(t):
        return t.fill_(float('nan')) if t.is_floating_point() else t
    torch.empty, torch.empty_like = (lambda *a, **k: fill(e(*a, **k))), (lambda *a, **k: fill(el(*a, **k)))
    try:
        yield
    finally:
        torch.empty, torch.empty_like = e, el


@contextlib.contextmanager
def fused(E, on, bwd=None):
    """the fused forward on / off, and the fused backward with it unless told otherwise"""
    sw = E.RB.switches
    prev = sw.stoch_block, sw.stoch_block_bwd
    sw.stoch_block, sw.stoch_block_bwd = on, on if bwd is None else bwd
    try:
        yield
    finally:
        sw.stoch_block, sw.stoch_block_bwd = prev


@contextlib.contextmanager
def wgrad_log(E):
    """the (x, dy) pairs the backward hands to the weight-gradient queue, instead of launching them"""
    log, prev = [], E.ops.wgrad
    E.ops.wgrad = lambda x, dy, w, g, dw, db, **kw: log.append((w, x, dy))
    try:
        yield log
    finally:
        E.ops.wgrad = prev


_cases = {}


def case(E, N, H, W, top):
    """The block (default init), its inputs and upstream gradients in float64 on the CPU — made once per shape and never changed — and
    the module on the device."""
    key = (N, H, W, top)
    if key in _cases:
        return _cases[key]
    torch.manual_seed(100 + 7 * N + H * W + int(top))
    g = torch.Generator().manual_seed(11 * N + H + 3 * W + int(top))
    blk = E.Block(C, Z, C, transform_p_params=not top)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    c = types.SimpleNamespace(N=N, H=H, W=W, top=top, blk=blk)
    c.w = {n: p.detach().double().clone() for n, p in blk.named_parameters()}
    c.xp = (0.5 * r(1, 2 * Z, H, W)) if top else r(N, C, H, W)   # top layer: the broadcast parameter itself
    c.xq, c.eps, c.zf = r(N, C, H, W), r(N, Z, H, W), r(N, Z, H, W)
    c.d_out, c.g_lp, c.g_lq, c.g_kl, c.g_ks = r(N, C, H, W), r(N), r(N), r(N), r(N, H, W)
    blk.cuda()
    _cases[key] = c
    return c


_refs = {}


def reference(c, mode, analytical, absent=()):
    """float64: outputs, and gradients of sum(out d_out) + sum_n g_lp lp + g_lq lq + g_kl kl + sum g_ks ks without the `absent` terms"""
    key = (c.N, c.H, c.W, c.top, mode, analytical, tuple(absent))
    if key in _refs:
        return _refs[key]
    o = types.SimpleNamespace()
    xp, xq = c.xp.clone().requires_grad_(True), c.xq.clone().requires_grad_(True)
    o.p = xp if c.top else F.conv2d(xp, c.w['conv_in_p.weight'], c.w['conv_in_p.bias'], padding=1)
    o.q = F.conv2d(xq, c.w['conv_in_q.weight'], c.w['conv_in_q.bias'], padding=1)
    if not c.top:
        o.p.retain_grad()
    o.q.retain_grad()
    pmu, plv = o.p.chunk(2, 1)
    qmu, qlv = o.q.chunk(2, 1)
    o.z = qmu + (qlv / 2).exp() * c.eps if mode == 0 else qmu if mode == 1 else c.zf.clone()
    lognorm = lambda z, mu, lv: -(z - mu) ** 2 / (2 * lv.exp()) - lv / 2 - LOG_SQRT_2PI
    lp_e, lq_e = lognorm(o.z, pmu, plv), lognorm(o.z, qmu, qlv)
    kan = 0.5 * ((qlv - plv).exp() + (qmu - pmu) ** 2 / plv.exp() - 1 - (qlv - plv))
    o.lp, o.lq = lp_e.sum((1, 2, 3)), lq_e.sum((1, 2, 3))
    o.kl = kan.sum((1, 2, 3)) if analytical else (lq_e - lp_e).sum((1, 2, 3))
    o.ks = kan.sum(1)
    o.out = F.conv2d(o.z, c.w['conv_out.weight'], c.w['conv_out.bias'], padding=1)
    terms = {'out': (o.out * c.d_out).sum(), 'lp': (o.lp * c.g_lp).sum(), 'lq': (o.lq * c.g_lq).sum(), 'kl': (o.kl * c.g_kl).sum(),
             'ks': (o.ks * c.g_ks).sum()}
    sum(v for k, v in terms.items() if k not in absent).backward()
    o.dxp, o.dxq = xp.grad, xq.grad
    o.dp = o.dxp.expand(c.N, -1, -1, -1) if c.top else o.p.grad
    o.dq = o.q.grad
    _refs[key] = o
    return o


def run(E, c, mode, analytical, on, absent=(), backward=False, nan=False, bwd=None):
    """the module on the device; returns outputs (and, with backward, gradients and the weight-gradient log)"""
    xp = (nhwc(c.xp)).requires_grad_(True)
    xq = nhwc(c.xq).requires_grad_(True)
    kw = dict(analytical_kl=analytical, noise=Tape(nhwc(c.eps)), need_kl_elementwise=False)
    if mode == 1:
        kw['use_mode'] = True
    if mode == 2:
        kw['forced_latent'] = nhwc(c.zf)
    r = types.SimpleNamespace()
    with fused(E, on), (nan_outputs() if nan else contextlib.nullcontext()):
        calls, real = [], E.K.stoch_block_fwd
        E.K.stoch_block_fwd = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
        try:
            out, d = c.blk(xp, xq, **kw)
        finally:
            E.K.stoch_block_fwd = real
    r.fused_calls = len(calls)
    r.out, r.z, r.p, r.q, r.lp, r.lq, r.kl, r.ks = out, d['z'], d['p_params'], d['q_params'], d['logprob_p'], d['logprob_q'], d['kl_samplewise'], d['kl_spatial']
    if backward:
        dev = lambda t: t.float().cuda()
        terms = {'out': (out * nhwc(c.d_out)).sum(), 'lp': (r.lp * dev(c.g_lp)).sum(), 'lq': (r.lq * dev(c.g_lq)).sum(),
                 'kl': (r.kl * dev(c.g_kl)).sum(), 'ks': (r.ks * dev(c.g_ks)).sum()}
        calls, real = [], E.K.stoch_block_bwd
        E.K.stoch_block_bwd = lambda *a, **k: (lambda res: (calls.append(res is not None), res)[1])(real(*a, **k))
        try:
            with wgrad_log(E) as log, fused(E, on, bwd), (nan_outputs() if nan else contextlib.nullcontext()):
                sum(v for k, v in terms.items() if k not in absent).backward()
        finally:
            E.K.stoch_block_bwd = real
        r.fused_bwd_calls = sum(calls)
        r.dxp, r.dxq, r.log = xp.grad, xq.grad, log
        by_w = {w.data_ptr(): dy for w, x, dy in log}
        r.dq = by_w[c.blk.conv_in_q.weight.data_ptr()]
        r.dp = None if c.top else by_w[c.blk.conv_in_p.weight.data_ptr()]
    torch.cuda.synchronize()
    return r


def check_forward(r, o, top):
    if not top:
        assert rel(nchw(r.p), o.p.detach()) < 3e-6
    assert rel(nchw(r.q), o.q.detach()) < 3e-6
    assert rel(nchw(r.z), o.z.detach()) < 4e-6
    assert rel(nchw(r.out), o.out.detach()) < 5e-6
    for a, b in ((r.lp, o.lp), (r.lq, o.lq), (r.kl, o.kl)):   # the bounds tests/test_kernels_gpu.py holds lvae_normal_stochastic_fwd_f32 to
        torch.testing.assert_close(a.cpu().double(), b.detach(), rtol=1e-5, atol=1e-3)
    torch.testing.assert_close(r.ks.cpu().double(), o.ks.detach(), rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize('top', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_forward_against_float64(E, shape, top):
    c = case(E, *shape, top)
    for mode in (0, 1, 2):
        for analytical in (False, True):
            r = run(E, c, mode, analytical, True, nan=True)
            assert r.fused_calls == 1, 'the plan declined %r' % (shape,)
            for t in (r.out, r.z, r.p, r.q, r.lp, r.lq, r.kl, r.ks):
                assert bool(torch.isfinite(t).all())
            check_forward(r, reference(c, mode, analytical), top)


BTOL = 3   # backward bounds of tests/test_resblock_img_gpu.py: three times the forward ones


def check_backward(r, o, top):
    if not top:
        assert rel(nchw(r.dp), o.dp) < 4e-6 * BTOL
        assert rel(nchw(r.dxp), o.dxp) < 1e-5 * BTOL
    else:
        assert rel(nchw(r.dxp), o.dxp) < 4e-6 * BTOL   # the broadcast parameter's gradient is dp summed over the batch
    assert rel(nchw(r.dq), o.dq) < 4e-6 * BTOL
    assert rel(nchw(r.dxq), o.dxq) < 1e-5 * BTOL


@pytest.mark.parametrize('top', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_backward_against_float64_autograd(E, shape, top):
    c = case(E, *shape, top)
    for mode, analytical in ((0, False), (0, True), (1, False), (2, True)):
        r = run(E, c, mode, analytical, True, backward=True, nan=True)
        assert r.fused_calls == 1 and r.fused_bwd_calls == 1
        for t in (r.dq, r.dxp, r.dxq) + (() if top else (r.dp,)):
            assert bool(torch.isfinite(t).all())
        check_backward(r, reference(c, mode, analytical), top)
    for absent in ('lp', 'lq', 'kl', 'ks'):
        r = run(E, c, 0, False, True, absent=(absent,), backward=True)
        assert r.fused_bwd_calls == 1
        check_backward(r, reference(c, 0, False, (absent,)), top)
    # the fused forward with the one-kernel-per-op backward behind it
    r = run(E, c, 0, False, True, backward=True, bwd=False)
    assert r.fused_calls == 1 and r.fused_bwd_calls == 0
    check_backward(r, reference(c, 0, False), top)


@pytest.mark.parametrize('top', [False, True])
@pytest.mark.parametrize('shape', [(3, 8, 8), (5, 4, 4), (9, 2, 2)])
def test_fused_equals_composed(E, shape, top):
    c = case(E, *shape, top)
    for mode, analytical in ((0, False), (2, True)):
        a = run(E, c, mode, analytical, True, backward=True)
        b = run(E, c, mode, analytical, False, backward=True)
        assert a.fused_calls == 1 and a.fused_bwd_calls == 1 and b.fused_calls == 0 and b.fused_bwd_calls == 0
        o = types.SimpleNamespace(**{k: nchw(v) if v.dim() == 4 else v.cpu().double() for k, v in vars(b).items() if torch.is_tensor(v)})
        o.dp = None if top else o.dp
        check_forward(a, o, top)
        check_backward(a, o, top)
        # the weight-gradient queue receives the same list: conv_out, then the input convolutions
        assert len(a.log) == len(b.log) == (2 if top else 3)
        key = lambda log: sorted((w.data_ptr(), tuple(x.shape), tuple(dy.shape)) for w, x, dy in log)
        assert key(a.log) == key(b.log)
        assert a.log[0][0] is c.blk.conv_out.weight and b.log[0][0] is c.blk.conv_out.weight


@pytest.mark.parametrize('top', [False, True])
@pytest.mark.parametrize('shape', [(5, 4, 4), (3, 8, 8), (9, 2, 2)])   # both tile sizes, and a tile that ends inside the batch
def test_core_equals_the_stand_alone_kernel(E, shape, top):
    """The block's core and lvae_normal_stochastic_fwd_f32 call one element function (csrc/stoch_core.h). On the block's own p_params and
    q_params, z and kl_spatial are the same bits: at Z = 32 both kernels sum a pixel's KL as four channels per lane, then shuffles of 4,
    2, 1. The per-sample sums are added in another order and are held to check_forward's bounds."""
    c = case(E, *shape, top)
    for mode in (0, 1, 2):
        for analytical in (False, True):
            r = run(E, c, mode, analytical, True)
            assert r.fused_calls == 1
            noise = None if mode == 1 else nhwc(c.zf if mode == 2 else c.eps)
            z, lp, lq, kl, ks = E.K.normal_stochastic_fwd(r.p.detach(), r.q.detach(), noise, mode, analytical, Z, c.N)
            torch.cuda.synchronize()
            assert torch.equal(z, r.z.detach()), (mode, analytical)
            assert torch.equal(ks, r.ks.detach()), (mode, analytical)
            for a, b in ((lp, r.lp), (lq, r.lq), (kl, r.kl)):
                torch.testing.assert_close(a.cpu().double(), b.detach().cpu().double(), rtol=1e-5, atol=1e-3)


def test_large_level_and_other_widths_decline(E):
    c = case(E, 2, 8, 8, False)
    cv = lambda m: (m.weight, m.geom(), m.bias)
    b = c.blk
    x16 = torch.zeros(2, 16, 16, C, device='cuda')
    assert not E.K.stoch_block_ok(x16, cv(b.conv_in_p), None, x16, cv(b.conv_in_q), cv(b.conv_out), 0, 2)
    x8 = torch.zeros(2, 8, 8, C, device='cuda')
    assert E.K.stoch_block_ok(x8, cv(b.conv_in_p), None, x8, cv(b.conv_in_q), cv(b.conv_out), 0, 2)
    small = E.Block(32, 16, 32).cuda()
    x = torch.zeros(2, 8, 8, 32, device='cuda')
    assert not E.K.stoch_block_ok(x, cv(small.conv_in_p), None, x, cv(small.conv_in_q), cv(small.conv_out), 0, 2)


def test_training_step_of_a_small_model(E):
    """One training step of a two-level model (8x8 and 4x4, batch 3) with the fused block on and off: same loss, same gradients."""
    from lvae_amd.engine import forward_pass
    from lvae_amd.models.lvae import LadderVAE
    from lvae_amd.noise import FrozenNoise
    from lvae_amd.optim import Adamax
    cfg = dict(color_ch=3, z_dims=[32, 32], blocks_per_layer=1, downsample=[0, 1], nonlin='elu', merge_type='residual', batchnorm=True,
               stochastic_skip=True, n_filters=64, dropout=0.0, free_bits=0.0, learn_top_prior=True, img_shape=(16, 16),
               likelihood_form='discr_log_mix', res_block_type='bacdbacd', gated=True, no_initial_downscaling=False, analytical_kl=False)
    torch.manual_seed(5)
    model = LadderVAE(**cfg)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    x = (torch.floor(256 * torch.rand(3, 3, 16, 16)) / 255).cuda()
    res = {}
    for on in (True, False):
        m = LadderVAE(**cfg)
        m.load_state_dict(sd)
        m.cuda().train()
        m.noise = FrozenNoise(seed=9)
        opt = Adamax(m)
        opt.zero_grad()
        calls, real = [], E.K.stoch_block_fwd
        E.K.stoch_block_fwd = lambda *a, **k: (calls.append(tuple(a[3].shape[1:3])), real(*a, **k))[1]
        try:
            with fused(E, on):
                out = forward_pass(m, x)
                out['loss'].backward()
                E.ops.flush_wgrad_group()
        finally:
            E.K.stoch_block_fwd = real
        torch.cuda.synchronize()
        assert sorted(calls) == ([(4, 4), (8, 8)] if on else [])
        res[on] = (float(out['loss'].detach()), {k: p.grad.detach().cpu().double().clone() for k, p in m.named_parameters() if p.grad is not None})
    (la, ga), (lb, gb) = res[True], res[False]
    assert abs(la - lb) <= 1e-6 * abs(lb)
    worst = max(rel(ga[k], gb[k]) for k in gb if float(gb[k].norm()) >= 1e-5)
    assert set(ga) == set(gb) and worst < 5e-4, worst   # the bound smoke() holds the step's gradients to against the oracle
