"""Posteriors parameterised relative to the prior on the GPU (csrc/stochastic_residual.hip, ops.NormalStochResFn, the block, the model and
the trainer under --residual-posterior).

The core is held to the two rules of docs/ELEMENTWISE_PARITY.md with no tolerance of its own: r64 is tests/residual_ref.py in float64,
r32 the same in float32 on the CPU, gradients by autograd, and

    element-wise outputs      |kernel - r64| <= 2 max|r32 - r64| + 1e-5 |r64| + 1e-6
    per-sample sums           |kernel - r64| <= 2 max|r32 - r64| + 4e-6 sum_i |term_i|

Every comparison prints `yardstick | case | kernel error | r32 error | bound` before it asserts (run with -s). The block is held to the
project's stated fp32 tolerance: per-row sums 1e-5 |ref| + 1e-4, gradients 1e-4 relative L2 per tensor."""
import contextlib
import re
import subprocess
import sys
import types

import pytest
import torch
import torch.nn.functional as F

import residual_ref as RR
from conftest import ROOT

pytestmark = pytest.mark.gpu

INF = float('inf')
LV_RANGES = [(-12., 6.), (-3., 2.)]   # the log-variance ranges of tests/test_elementwise_gpu.py


@pytest.fixture(scope='module')
def K():
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels
    return kernels


def dev(t):
    return None if t is None else t.contiguous().cuda()


def off_by_one_float(t):
    """t on the device as a contiguous view that starts 4 bytes into its storage"""
    buf = torch.empty(t.numel() + 1, device='cuda')
    view = buf[1:].view(t.shape)
    view.copy_(t.cuda())
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def finite(*ts):
    for t in ts:
        for v in (t.values() if isinstance(t, dict) else [t]):
            if v is not None:
                assert bool(torch.isfinite(v).all()), 'a reference value is not finite'


def _cmp(tag, got, r64, r32, floor):
    got, r64, r32 = got.detach().double().cpu(), r64.detach().double(), r32.detach().double()
    assert got.shape == r64.shape == r32.shape, (tag, got.shape, r64.shape, r32.shape)
    e32 = float((r32 - r64).abs().max())
    bound = (2.0 * e32 + floor).expand_as(r64).reshape(-1)
    err = (got - r64).abs().reshape(-1)
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, INF))
    k = int(torch.argmax(err / bound.clamp(min=1e-300)))   # the element that uses most of its bound
    print('yardstick | %-62s | kernel %.3e | r32 %.3e | bound %.3e | n %d' % (tag, float(err[k]), e32, float(bound[k]), err.numel()))
    assert bool((err <= bound).all()), '%s: |kernel - r64| = %.6e at flat element %d, bound %.6e (r32 error %.3e)' % (
        tag, float(err[k]), k, float(bound[k]), e32)


def close_elem(tag, got, r64, r32):
    _cmp(tag, got, r64, r32, 1e-5 * r64.detach().double().abs() + 1e-6)


def close_sum(tag, got, r64, r32, abs_terms):
    _cmp(tag, got, r64, r32, 4e-6 * abs_terms.detach().double())


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the core against r64
# ---------------------------------------------------------------------------------------------------------------------------------
def _inputs(N, HW, Z, bcast, seed, lv):
    """p (N|1,HW,1,2Z) with log-variances uniform in `lv`; offsets d = (randn | U(-2, 2)), in one third of the elements 1e-4 noise, where
    the KL terms are tiny and only expm1 keeps them; eps; a forced latent."""
    g = torch.Generator().manual_seed(seed)
    n = 1 if bcast else N
    p = torch.cat((torch.randn(n, HW, 1, Z, generator=g), torch.rand(n, HW, 1, Z, generator=g) * (lv[1] - lv[0]) + lv[0]), -1)
    d = torch.cat((torch.randn(N, HW, 1, Z, generator=g), torch.rand(N, HW, 1, Z, generator=g) * 4 - 2), -1)
    near = (torch.rand(N, HW, 1, Z, generator=g) < 1 / 3).repeat(1, 1, 1, 2)
    d = torch.where(near, 1e-4 * torch.randn(N, HW, 1, 2 * Z, generator=g), d)
    return p, d, torch.randn(N, HW, 1, Z, generator=g), 1.5 * torch.randn(N, HW, 1, Z, generator=g)


def _raw_fwd(K, p, d, e, mode, analytical, Z, N, want_ks=True, want_q=True):
    """the entry point itself, so that kl_spatial and q_out can each be NULL"""
    HW = p.shape[1] * p.shape[2]
    z = torch.full((N, p.shape[1], p.shape[2], Z), float('nan'), device='cuda')
    lp, lq, kl = (torch.full((N,), float('nan'), device='cuda') for _ in range(3))
    ks = torch.full((N, p.shape[1], p.shape[2]), float('nan'), device='cuda') if want_ks else None
    q = torch.full((N, p.shape[1], p.shape[2], 2 * Z), float('nan'), device='cuda') if want_q else None
    K.call('lvae_normal_stochastic_res_fwd_f32', K.ptr(p), int(p.shape[0] == 1 and N > 1), K.ptr(d), K.ptr(e), N, HW, Z, mode, int(analytical),
           K.ptr(z), K.ptr(q), K.ptr(lp), K.ptr(lq), K.ptr(kl), K.ptr(ks), K.stream_ptr())
    return z, lp, lq, kl, ks, q


def _fwd_check(K, tag, p, d, e, mode, analytical, Z, N, d_dev=None, e_dev=None, want_ks=True, want_q=True):
    r64 = RR.residual_core(p.double(), d.double(), e.double(), mode, analytical, Z, N)
    r32 = RR.residual_core(p, d, e, mode, analytical, Z, N)
    finite(r64, r32)
    if e_dev is None:
        e_dev = None if mode == 1 else dev(e)   # mode 1 reads no eps: the pointer may be absent
    z, lp, lq, kl, ks, q = _raw_fwd(K, dev(p), dev(d) if d_dev is None else d_dev, e_dev, mode, analytical, Z, N, want_ks, want_q)
    close_elem(tag + ' z', z, r64['z'], r32['z'])
    close_sum(tag + ' logprob_p', lp, r64['lp'], r32['lp'], r64['lp_abs'])
    close_sum(tag + ' logprob_q', lq, r64['lq'], r32['lq'], r64['lq_abs'])
    close_sum(tag + ' kl_samplewise', kl, r64['kl'], r32['kl'], r64['kl_abs'])
    if want_ks:
        close_elem(tag + ' kl_spatial', ks, r64['ks'], r32['ks'])   # a sum of Z non-negative terms: the element-wise rule is the tighter one
    if want_q:
        assert torch.equal(q.cpu(), (p + d).expand(N, -1, -1, -1)), tag + ': q_out is not p + d in fp32'


FULL = ('dz', 'g_lp', 'g_lq', 'g_kl', 'g_ks')
GRAD_SUBSETS = [FULL, ('dz', 'g_kl'), ('g_lp', 'g_lq', 'g_ks')]


def _upstream(N, HW, Z, seed):
    g = torch.Generator().manual_seed(seed)
    return {'dz': torch.randn(N, HW, 1, Z, generator=g), 'g_lp': torch.randn(N, generator=g), 'g_lq': torch.randn(N, generator=g),
            'g_kl': torch.randn(N, generator=g), 'g_ks': torch.randn(N, HW, 1, generator=g)}


def _bwd_ref(p, d, e, grads, mode, analytical, Z, N, dt):
    p, d = p.detach().to(dt).clone().requires_grad_(True), d.detach().to(dt).clone().requires_grad_(True)
    o = RR.residual_core(p, d, e.to(dt), mode, analytical, Z, N)
    loss = None
    for key, name in (('z', 'dz'), ('lp', 'g_lp'), ('lq', 'g_lq'), ('kl', 'g_kl'), ('ks', 'g_ks')):
        if grads.get(name) is not None and o[key].requires_grad:
            term = (o[key] * grads[name].to(dt)).sum()
            loss = term if loss is None else loss + term
    loss.backward()
    return p.grad.detach(), d.grad.detach(), o['z'].detach()


def _bwd_check(K, tag, p, d, e, grads, mode, analytical, Z, N, d_dev=None, e_dev=None):
    dp64, dd64, _ = _bwd_ref(p, d, e, grads, mode, analytical, Z, N, torch.float64)
    dp32, dd32, z32 = _bwd_ref(p, d, e, grads, mode, analytical, Z, N, torch.float32)
    finite(dp64, dp32, dd64, dd32)
    gd = {k: dev(v) for k, v in grads.items()}
    dp, dd = K.normal_stochastic_res_bwd(dev(p), dev(d) if d_dev is None else d_dev, dev(e) if e_dev is None else e_dev, dev(z32), gd.get('dz'),
                                         gd.get('g_lp'), gd.get('g_lq'), gd.get('g_kl'), gd.get('g_ks'), mode, analytical, Z)
    dp = dp.double().cpu()
    close_elem(tag + ' dp', dp.sum(0, keepdim=True) if p.shape[0] == 1 and N > 1 else dp, dp64, dp32)   # a broadcast prior: after the column sum
    close_elem(tag + ' dd', dd, dd64, dd32)


# N, HW, Z, broadcast p, misaligned d and eps: what each exercises is in the id
CORE_CASES = [
    pytest.param(3, 80, 32, False, False, id='3x80x32-16B-map-second-slot-half-valid'),
    pytest.param(2, 1, 32, False, False, id='2x1x32-one-pixel-idle-lanes'),
    pytest.param(2, 7, 4, False, False, id='2x7x4-no-shuffle'),
    pytest.param(2, 5, 64, False, False, id='2x5x64-widest-group'),
    pytest.param(2, 300, 3, False, False, id='2x300x3-scalar-map-Z-no-power-of-two'),
    pytest.param(2, 5, 128, False, False, id='2x5x128-scalar-map-Z-above-64'),
    pytest.param(3, 80, 32, False, True, id='3x80x32-misaligned-scalar-map-32-lane-shuffles'),
    pytest.param(5, 16, 32, True, False, id='5x16x32-p-broadcast'),
]


@pytest.mark.parametrize('N,HW,Z,bcast,mis', CORE_CASES)
def test_core_forward_against_float64(K, N, HW, Z, bcast, mis):
    for lv in LV_RANGES:
        p, d, eps, zf = _inputs(N, HW, Z, bcast, 100 + Z + HW, lv)
        for analytical in (False, True):
            for mode in (0, 1, 2):
                e = zf if mode == 2 else eps
                # kl_spatial and q_out each absent in some of the combinations, both present in the others
                want_ks, want_q = not (mode == 1 and analytical), not (mode == 0 and not analytical)
                _fwd_check(K, 'res_fwd %dx%dx%d lv%g..%g an%d mode%d' % (N, HW, Z, lv[0], lv[1], analytical, mode), p, d, e, mode, analytical, Z, N,
                           d_dev=off_by_one_float(d) if mis else None, e_dev=off_by_one_float(e) if mis else None,
                           want_ks=want_ks, want_q=want_q)


@pytest.mark.parametrize('N,HW,Z,bcast,mis', CORE_CASES)
def test_core_backward_against_float64_autograd(K, N, HW, Z, bcast, mis):
    full = _upstream(N, HW, Z, 200 + Z + HW)
    for lv in LV_RANGES:
        p, d, eps, zf = _inputs(N, HW, Z, bcast, 300 + Z + HW, lv)
        for analytical in (False, True):
            for mode in (0, 1, 2):
                e = zf if mode == 2 else eps
                for ci, names in enumerate(GRAD_SUBSETS):
                    _bwd_check(K, 'res_bwd %dx%dx%d lv%g..%g an%d mode%d grads%d' % (N, HW, Z, lv[0], lv[1], analytical, mode, ci), p, d, e,
                               {k: full[k] for k in names}, mode, analytical, Z, N,
                               d_dev=off_by_one_float(d) if mis else None, e_dev=off_by_one_float(e) if mis else None)


def test_core_on_the_discriminating_inputs(K):
    """|mu_p| >> sigma_p (tests/test_residual_posterior_cpu.py shows that the absolute formula on fl32(p + d) is outside the rule at most
    elements there): the kernel meets the rule on kl_spatial, kl_samplewise and dp."""
    N, HW, Z = 3, 80, 32
    p, d, eps = RR.discriminating_inputs(N, HW, Z)
    full = _upstream(N, HW, Z, 7)
    for analytical in (True, False):
        r64 = RR.residual_core(p.double(), d.double(), eps.double(), 0, analytical, Z, N)
        r32 = RR.residual_core(p, d, eps, 0, analytical, Z, N)
        finite(r64, r32)
        z, lp, lq, kl, ks, q = K.normal_stochastic_res_fwd(dev(p), dev(d), dev(eps), 0, analytical, Z, N)
        close_elem('discriminating an%d kl_spatial' % analytical, ks, r64['ks'], r32['ks'])
        close_sum('discriminating an%d kl_samplewise' % analytical, kl, r64['kl'], r32['kl'], r64['kl_abs'])
        _bwd_check(K, 'discriminating an%d' % analytical, p, d, eps, full, 0, analytical, Z, N)
        _bwd_check(K, 'discriminating an%d kl only' % analytical, p, d, eps, {k: full[k] for k in ('g_kl', 'g_ks')}, 0, analytical, Z, N)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. q_out, determinism, the zero offset
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,HW,Z', [(3, 80, 32), (2, 300, 3)], ids=['16B-map', 'scalar-map'])
def test_two_launches_give_the_same_bits_and_q_out_is_the_fp32_sum(K, N, HW, Z):
    p, d, eps, _ = _inputs(N, HW, Z, False, 41, LV_RANGES[1])
    a = K.normal_stochastic_res_fwd(dev(p), dev(d), dev(eps), 0, True, Z, N)
    b = K.normal_stochastic_res_fwd(dev(p), dev(d), dev(eps), 0, True, Z, N)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.equal(a[5].cpu(), p + d)
    assert K.normal_stochastic_res_fwd(dev(p), dev(d), dev(eps), 0, True, Z, N, need_q=False)[5] is None
    g = _upstream(N, HW, Z, 5)
    ga = K.normal_stochastic_res_bwd(dev(p), dev(d), dev(eps), None, dev(g['dz']), None, None, dev(g['g_kl']), None, 0, True, Z)
    gb = K.normal_stochastic_res_bwd(dev(p), dev(d), dev(eps), None, dev(g['dz']), None, None, dev(g['g_kl']), None, 0, True, Z)
    assert torch.equal(ga[0], gb[0]) and torch.equal(ga[1], gb[1])


@pytest.mark.parametrize('N,HW,Z,bcast', [(3, 80, 32, False), (5, 16, 32, True), (2, 300, 3, False)], ids=['16B-map', 'p-broadcast', 'scalar-map'])
def test_zero_offset_sits_on_the_prior(K, N, HW, Z, bcast):
    """d = 0 with the analytical KL: kl_samplewise and kl_spatial are exactly 0.0 and z is the prior's own draw on the same eps."""
    p, _, eps, _ = _inputs(N, HW, Z, bcast, 43, LV_RANGES[0])
    zero = torch.zeros(N, HW, 1, 2 * Z)
    z, lp, lq, kl, ks, q = K.normal_stochastic_res_fwd(dev(p), dev(zero), dev(eps), 0, True, Z, N)
    zp, lpp = K.normal_stochastic_fwd(dev(p), None, dev(eps), 0, False, Z, N)[:2]
    assert torch.equal(kl, torch.zeros_like(kl)) and torch.equal(ks, torch.zeros_like(ks))
    assert torch.equal(z, zp)
    assert torch.equal(q.cpu(), p.expand(N, -1, -1, -1))


def test_entry_points_refuse_bad_arguments(K):
    from lvae_amd import _C
    N, HW, Z = 2, 5, 4
    p, d, eps, _ = _inputs(N, HW, Z, False, 3, LV_RANGES[1])
    with pytest.raises(_C.LvaeHipError):
        K.normal_stochastic_res_fwd(dev(p), dev(d), None, 0, True, Z, N)    # mode 0 without eps
    with pytest.raises(_C.LvaeHipError):
        K.normal_stochastic_res_fwd(dev(p), dev(d), dev(eps), 3, True, Z, N)   # no such mode
    with pytest.raises(_C.LvaeHipError):
        K.normal_stochastic_res_bwd(dev(p), dev(d), dev(eps), None, None, None, None, None, None, 2, True, Z)   # mode 2 without the latent


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the block
# ---------------------------------------------------------------------------------------------------------------------------------
C, ZB = 64, 32


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


@pytest.mark.parametrize('top', [False, True], ids=['non-top', 'top-broadcast-p'])
@pytest.mark.parametrize('N,H,W', [(4, 4, 4), (2, 16, 16)], ids=['4x4x4-fused-level', '2x16x16'])
def test_block_against_float64_composite(N, H, W, top):
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels as K, ops
    from lvae_amd.lib.stochastic import NormalStochasticBlock2d
    torch.manual_seed(300 + N + H + int(top))
    g = torch.Generator().manual_seed(17 * N + H + int(top))
    blk = NormalStochasticBlock2d(C, ZB, C, transform_p_params=not top)
    blk.residual_posterior = True
    w = {n: p.detach().double().clone() for n, p in blk.named_parameters()}
    assert len(w) == (4 if top else 6)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    xp0 = (0.5 * r(1, 2 * ZB, H, W)) if top else r(N, C, H, W)
    xq0, eps = r(N, C, H, W), r(N, ZB, H, W)
    d_out, g_lp, g_lq, g_kl, g_ks = r(N, C, H, W), r(N), r(N), r(N), r(N, H, W)
    # float64 composite: conv2d on the same weights plus the helper
    xp, xq = xp0.clone().requires_grad_(True), xq0.clone().requires_grad_(True)
    wr = {n: t.clone().requires_grad_(True) for n, t in w.items()}
    p64 = xp if top else F.conv2d(xp, wr['conv_in_p.weight'], wr['conv_in_p.bias'], padding=1)
    d64 = F.conv2d(xq, wr['conv_in_q.weight'], wr['conv_in_q.bias'], padding=1)
    o = RR.residual_core(p64.permute(0, 2, 3, 1), d64.permute(0, 2, 3, 1), eps.permute(0, 2, 3, 1), 0, False, ZB, N)
    out64 = F.conv2d(o['z'].permute(0, 3, 1, 2), wr['conv_out.weight'], wr['conv_out.bias'], padding=1)
    ((out64 * d_out).sum() + (o['lp'] * g_lp).sum() + (o['lq'] * g_lq).sum() + (o['kl'] * g_kl).sum() + (o['ks'] * g_ks).sum()).backward()
    # the module on the device
    blk.cuda()
    calls, real = [], K.stoch_block_fwd
    K.stoch_block_fwd = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        dxp, dxq = nhwc(xp0).requires_grad_(True), nhwc(xq0).requires_grad_(True)
        out, data = blk(dxp, dxq, noise=Tape(nhwc(eps)), need_kl_elementwise=False, n_img=N if top else None)
    finally:
        K.stoch_block_fwd = real
    assert not calls, 'the one-launch block is declined under residual_posterior'
    ((out * nhwc(d_out)).sum() + (data['logprob_p'] * g_lp.float().cuda()).sum() + (data['logprob_q'] * g_lq.float().cuda()).sum() +
     (data['kl_samplewise'] * g_kl.float().cuda()).sum() + (data['kl_spatial'] * g_ks.float().cuda()).sum()).backward()
    ops.flush_wgrad_group()
    torch.cuda.synchronize()
    for name, got, ref in (('logprob_p', data['logprob_p'], o['lp']), ('logprob_q', data['logprob_q'], o['lq']), ('kl', data['kl_samplewise'], o['kl'])):
        err = (got.cpu().double() - ref.detach()).abs()
        bound = 1e-5 * ref.detach().abs() + 1e-4
        print('yardstick | block %dx%dx%d top%d %-9s | error %.3e | bound %.3e' % (N, H, W, top, name, float(err.max()), float(bound.min())))
        assert bool((err <= bound).all()), name
    assert torch.equal(data['q_params'], (data['p_params'].detach() + _offset(blk, dxq)).expand(N, -1, -1, -1))
    pairs = [('x_p', nchw(dxp.grad), xp.grad), ('x_q', nchw(dxq.grad), xq.grad)]
    pairs += [(n, dict(blk.named_parameters())[n].grad.detach().cpu().double(), wr[n].grad) for n in w]
    for name, got, ref in pairs:
        print('yardstick | block %dx%dx%d top%d d%-18s | relative L2 %.3e | bound 1e-4' % (N, H, W, top, name, rel(got, ref)))
        assert rel(got, ref) <= 1e-4, name
    # without the keyword's consumers nothing is written for q_out, and kl_elementwise is the composed, detached value
    with torch.no_grad():
        _, lean = blk(dxp, dxq, noise=Tape(nhwc(eps)), need_kl_elementwise=False, need_q_params=False, n_img=N if top else None)
        _, rich = blk(dxp, dxq, noise=Tape(nhwc(eps)), need_kl_elementwise=True, need_q_params=False, n_img=N if top else None)
    assert lean['q_params'] is None and lean['kl_elementwise'] is None and torch.equal(lean['kl_samplewise'], data['kl_samplewise'].detach())
    want = K.kl_elementwise_fwd(rich['p_params'], rich['q_params'], rich['z'], False)
    assert torch.equal(rich['kl_elementwise'], want) and not rich['kl_elementwise'].requires_grad


def _offset(blk, x_q):
    from lvae_amd import ops
    with torch.no_grad():
        return ops.conv(x_q.detach(), blk.conv_in_q)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the model
# ---------------------------------------------------------------------------------------------------------------------------------
CFG = dict(color_ch=3, z_dims=[8, 8], blocks_per_layer=1, downsample=[1, 1], nonlin='elu', merge_type='residual', batchnorm=True,
           stochastic_skip=True, n_filters=16, dropout=0.1, free_bits=0.0, learn_top_prior=True, img_shape=(32, 32),
           likelihood_form='discr_log_mix', res_block_type='bacdbacd', gated=True, no_initial_downscaling=False, analytical_kl=False)
B = 4


def _images(n, seed):
    return torch.floor(256 * torch.rand(n, 3, 32, 32, generator=torch.Generator().manual_seed(seed))) / 255


_sd = {}


def _model(residual, seed=3, touch=True):
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels as K
    from lvae_amd.models.lvae import LadderVAE
    from lvae_amd.noise import PhiloxNoise
    K.prepared.entries.clear()
    K.prepared.table = None
    torch.manual_seed(0)
    m = LadderVAE(**CFG)
    if not _sd:
        _sd.update({k: v.clone() for k, v in m.state_dict().items()})
    m.load_state_dict(_sd)
    m.cuda().train()
    m.noise = PhiloxNoise(seed=seed)
    if touch:
        m.residual_posterior = residual
    return m


@contextlib.contextmanager
def _count(K, name):
    calls, real = [], getattr(K, name)
    setattr(K, name, lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    try:
        yield calls
    finally:
        setattr(K, name, real)


def test_model_forward_backward_and_the_public_entry_points(K):
    from lvae_amd.engine import forward_pass
    from lvae_amd.optim import Adamax
    m = _model(True)
    opt = Adamax(m)
    opt.zero_grad()
    x = _images(B, 1).cuda()
    with _count(K, 'normal_stochastic_res_fwd') as res, _count(K, 'normal_stochastic_fwd') as plain:
        out = forward_pass(m, x)
        out['loss'].backward()
    torch.cuda.synchronize()
    assert len(res) == 2 and not plain   # both layers, the top one included
    assert all(bool(torch.isfinite(out[k]).all()) for k in ('loss', 'elbo', 'recons', 'kl'))
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(t).all()) for t in grads)
    assert float(m.top_down_layers[-1].top_prior_params.grad.abs().max()) > 0 and float(m.top_down_layers[0].stochastic.conv_in_q.weight.grad.abs().max()) > 0
    m.eval()
    with torch.no_grad():
        zs = m.encode(x)
        pics = m.decode(zs)
        cond = m.sample_conditional(x, 1)
    assert len(zs) == 2
    for t in list(zs) + [v for res in (pics, cond) for v in res.values() if torch.is_tensor(v) and v.is_floating_point()]:
        assert bool(torch.isfinite(t).all())


def test_latent_stats_fold_the_absolute_parameters(K):
    """With a LatentStats attached the block writes q_out and folds from it: the folded per-unit KL is the absolute formula on the
    (p_params, q_params) the blocks returned, by the element-wise rule (r32: the formula in float32, as the fold evaluates it)."""
    from lvae_amd.latent import LatentStats
    m = _model(True).eval()
    stats = LatentStats(m, 'cuda')
    seen = {}
    hooks = [l.stochastic.register_forward_hook(lambda mod, a, res, i=i: seen.__setitem__(i, res[1])) for i, l in enumerate(m.top_down_layers)]
    x = _images(B, 2).cuda()
    from lvae_amd.evaluate import _test_bottom_up
    with torch.no_grad():
        bu, _ = _test_bottom_up(m, x)
        m.noise.begin(x.device)
        m._topdown(bu, latent_stats=stats)
        stats.count(B)
        res = stats.take()
        seen_with = dict(seen)
        m._topdown(bu)   # no statistics attached: the layer asks for no q_out
        m.noise.end()
    for h in hooks:
        h.remove()
    assert all(seen[i]['q_params'] is None for i in seen) and len(seen) == 2
    for i, data in seen_with.items():
        p, q = data['p_params'].cpu(), data['q_params'].cpu()
        Z = q.shape[3] // 2
        r64 = RR.absolute_kl(q.double(), p.double(), Z).mean(0).permute(2, 0, 1)
        r32 = RR.absolute_kl(q, p, Z).mean(0).permute(2, 0, 1)
        close_elem('latent statistics layer %d mean KL per unit' % i, torch.from_numpy(res['arrays'][i]['kl']), r64, r32)


def _state(m, opt):
    sd = m.state_dict()
    st = {k: v.detach().clone() for k, v in sd.items() if not k.endswith(('weight', 'bias', 'top_prior_params'))}
    st.update(params=m.arena.params.detach().clone(), exp_avg=opt.exp_avg.clone(), exp_inf=opt.exp_inf.clone(), opt_step=opt.step_count.clone(),
              noise=m.noise.step.clone())
    return st


def _three_steps(residual, use_graph, touch=True, **kw):
    from lvae_amd.engine import TrainStep
    from lvae_amd.optim import Adamax
    m = _model(residual, touch=touch)
    opt = Adamax(m, lr=1e-3)
    st = TrainStep(m, opt, use_graph=use_graph, **kw)
    rows = B * kw.get('accum_steps', 1)
    outs = [{k: v.detach().clone() for k, v in st(_images(rows, 60 + k).cuda()).items()} for k in range(3)]
    torch.cuda.synchronize()
    return outs, _state(m, opt)


@pytest.mark.parametrize('kw', [{}, {'iw_samples': 2}, {'accum_steps': 2}], ids=['elbo', 'iw2', 'accum2'])
def test_captured_step_equals_eager_bit_for_bit(kw):
    (eo, es), (go, gs) = _three_steps(True, False, **kw), _three_steps(True, True, eager_warmup=1, **kw)
    diff = [k for k in es if not torch.equal(es[k], gs[k])]
    print('yardstick | residual posterior, %r, three steps: captured against eager, %d of %d state tensors differ %r' % (kw, len(diff), len(es), diff[:4]))
    assert es.keys() == gs.keys() and not diff
    for a, b in zip(eo, go):
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    assert all(bool(torch.isfinite(v).all()) for o in go for v in o.values())


def test_property_off_is_the_model_that_never_had_it(K):
    with _count(K, 'normal_stochastic_res_fwd') as res:
        (ao, a), (bo, b) = _three_steps(False, False), _three_steps(False, False, touch=False)
    assert not res   # the absolute node
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    assert all(torch.equal(x[k], y[k]) for x, y in zip(ao, bo) for k in x)
    (co, c) = _three_steps(True, False)
    assert not torch.equal(c['params'], a['params'])   # and the property does change the model


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the trainer
# ---------------------------------------------------------------------------------------------------------------------------------
def _run(mod, argv, ok=True):
    p = subprocess.run([sys.executable, '-m', mod] + argv, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert (p.returncode == 0) == ok, p.stdout[-3000:] + p.stderr[-3000:]
    lines = [re.sub(r'\s*\[\d+ img/s\]', '', line) for line in p.stdout.splitlines() if re.search(r'\[step \d+\]', line)]
    return {int(re.search(r'\[step (\d+)\]', line).group(1)): line for line in lines}, p.stdout, p.stderr


def test_trainer_resumes_exactly_refuses_the_other_setting_and_evaluate_says_so(tmp_path):
    model = ['-d', 'cifar10', '--zdims', '8', '8', '--downsample', '1', '1', '--nfilters', '16', '--skip', '--gated', '--batch-size', '4', '--seed', '3']
    base = model + ['--log-every', '1', '--synthetic', '--residual-posterior']
    d_full, d_half = str(tmp_path / 'full'), str(tmp_path / 'half')
    full, half, rest = (str(tmp_path / n) for n in ('full.pt', 'half.pt', 'rest.pt'))
    tr_a, out_a, _ = _run('lvae_amd.main', base + ['--steps', '4', '--checkpoint-dir', d_full, '--save-checkpoint', full])
    tr_1, _, _ = _run('lvae_amd.main', base + ['--steps', '2', '--checkpoint-dir', d_half, '--save-checkpoint', half])
    tr_2, out_2, _ = _run('lvae_amd.main', base + ['--steps', '4', '--resume', half, '--save-checkpoint', rest])
    print('yardstick | train lines of the whole run %r, of the resumed one %r' % (sorted(tr_a), sorted(tr_2)))
    assert sorted(tr_a) == [1, 2, 3, 4] and sorted(tr_2) == [3, 4] and {**tr_1, **tr_2} == tr_a and len(set(tr_a.values())) == 4
    assert ',resq,' in out_a
    a, b = torch.load(full), torch.load(rest)
    assert a['residual_posterior'] is True and b['residual_posterior'] is True
    assert a['model'].keys() == b['model'].keys() and all(torch.equal(a['model'][k], b['model'][k]) for k in a['model'])
    # the same weights under the other setting are a different model: refused, with both settings named
    _, out_r, err_r = _run('lvae_amd.main', [x for x in base if x != '--residual-posterior'] + ['--steps', '4', '--resume', half], ok=False)
    assert 'ValueError' in err_r and 'residual' in err_r and 'absolute' in err_r, err_r[-2000:]
    _, out_e, _ = _run('lvae_amd.evaluate', model + ['--synthetic', '--checkpoint', full, '--ll', '--n-test', '8', '--ll-samples', '2'])
    print('yardstick | evaluate: %s' % [l for l in out_e.splitlines() if 'residual' in l])
    assert 'residual posteriors' in out_e
