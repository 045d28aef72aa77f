"""The kernels around the convolutions (likelihood heads, stochastic block, gate, glue, bookkeeping, Adamax, L2 norm, noise) at the
shapes, modes and values where they can go wrong, each against the plain torch formula of the same operation in float64.

The yardstick of every floating-point comparison is the one test_likelihood_golden_vectors uses for the DMoL gradient, so that no
tolerance is invented here: r64 is the formula in float64 on the CPU (gradients by autograd), r32 the same formula in float32, and

    element-wise outputs      |kernel - r64| <= 2 max|r32 - r64| + 1e-5 |r64| + 1e-6
    per-sample sums           |kernel - r64| <= 2 max|r32 - r64| + 4e-6 sum_i |term_i|        (terms in float64)

1e-5 / 1e-6 are the rtol / atol of the element-wise tests of test_kernels_gpu.py (they cover __expf and the hardware reciprocal of
sigmoidf_ for |x| <= 20); 4e-6 per term is ~2e-6 relative from the fast intrinsics plus the fixed-order fp32 summation. No bound is derived
from a kernel's output. Every comparison prints `yardstick | case | kernel error | r32 error | bound` before it asserts (run with -s): the
kernel's error and the bound at the element that uses most of its bound, and max|r32 - r64|.
Every reference of a test is computed, and checked to be finite, before the first tensor goes to the device.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

INF = float('inf')


@pytest.fixture(scope='module')
def K():
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels
    return kernels


def dev(t):
    return None if t is None else t.contiguous().cuda()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def nchw(t):
    return t.permute(0, 3, 1, 2).cpu()


def rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-20))


def leaf(t, dt):
    """a fresh leaf of dtype dt that requires grad (never the caller's tensor itself)"""
    return t.detach().to(dt).clone().requires_grad_(True)


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
    k = int(torch.argmax(err / bound.clamp(min=1e-300)))          # the element that uses most of its bound: its error and its bound are printed
    print('yardstick | %-58s | kernel %.3e | r32 %.3e | bound %.3e | n %d' % (tag, float(err[k]), e32, float(bound[k]), err.numel()))
    assert bool((err <= bound).all()), '%s: |kernel - r64| = %.6e at flat element %d, bound %.6e (r32 error %.3e)' % (
        tag, float(err[k]), k, float(bound[k]), e32)


def close_elem(tag, got, r64, r32):
    _cmp(tag, got, r64, r32, 1e-5 * r64.detach().double().abs() + 1e-6)


def close_sum(tag, got, r64, r32, abs_terms):
    _cmp(tag, got, r64, r32, 4e-6 * abs_terms.detach().double())


# ---------------------------------------------------------------------------------------------------------------------------------
# 1-2. Normal stochastic block
# ---------------------------------------------------------------------------------------------------------------------------------
# Log-variances uniform in [-12, 6]: standard deviations from 2.5e-3 to 20, so that single terms reach 1e8 and float32 itself is off by tens
# in the sums and by up to 5e7 in single gradient elements (measured: the r32 column of the printed table). The rule then allows twice that
# everywhere, which says little about the small elements; the same cases therefore also run on log-variances in [-3, 2], where the float32
# formula is good to ~1e-5 and the same rule is sharp.
LV_RANGES = [(-12., 6.), (-3., 2.)]


def _stoch_inputs(N, Z, H, W, top, seed, with_q=True, lv=LV_RANGES[0]):
    """(mu | logvar) tensors in the kernels' NHWC layout: log-variances uniform in `lv`; in one third of the elements q = p + 1e-4 noise,
    where the KL terms cancel and only absolute error means anything. Also eps and a forced latent."""
    g = torch.Generator().manual_seed(seed)

    def params(n):
        return torch.cat((torch.randn(n, H, W, Z, generator=g), torch.rand(n, H, W, Z, generator=g) * (lv[1] - lv[0]) + lv[0]), -1)

    p, q = params(1 if top else N), None
    if with_q:
        q = params(N)
        near = (torch.rand(N, H, W, Z, generator=g) < 1 / 3).repeat(1, 1, 1, 2)
        q = torch.where(near, p.expand(N, H, W, 2 * Z) + 1e-4 * torch.randn(N, H, W, 2 * Z, generator=g), q)
    return p, q, torch.randn(N, H, W, Z, generator=g), 1.5 * torch.randn(N, H, W, Z, generator=g)


def _stoch_ref(p, q, e, mode, analytical, Z, N):
    from oracle import lvae_ref as R
    pmu, plv = p[..., :Z], p[..., Z:]
    smu, slv = pmu, plv
    if q is not None:
        qmu, qlv = q[..., :Z], q[..., Z:]
        smu, slv = qmu, qlv
    z = smu + (slv / 2).exp() * e if mode == 0 else (smu if mode == 1 else e)
    z = z.expand(N, *z.shape[1:])
    lp = R.normal_log_prob(z, pmu, plv)
    o = {'z': z, 'lp': lp.sum((1, 2, 3)), 'lp_abs': lp.abs().sum((1, 2, 3))}
    if q is not None:
        lq, kan = R.normal_log_prob(z, qmu, qlv), R.normal_kl(qmu, qlv, pmu, plv)
        kl = kan if analytical else lq - lp
        o.update(lq=lq.sum((1, 2, 3)), lq_abs=lq.abs().sum((1, 2, 3)), kl=kl.sum((1, 2, 3)), kl_abs=kl.abs().sum((1, 2, 3)), ks=kan.sum(-1))
    return o


def _stoch_fwd_check(K, tag, p, q, e, mode, analytical, Z, N, e_dev=None):
    r64 = _stoch_ref(p.double(), None if q is None else q.double(), e.double(), mode, analytical, Z, N)
    r32 = _stoch_ref(p, q, e, mode, analytical, Z, N)
    finite(r64, r32)
    if e_dev is None:
        e_dev = None if mode == 1 else dev(e)          # mode 1 reads no eps: the pointer may be absent
    z, lp, lq, kl, ks = K.normal_stochastic_fwd(dev(p), dev(q), e_dev, mode, analytical, Z, N)
    close_elem(tag + ' z', z, r64['z'], r32['z'])
    close_sum(tag + ' logprob_p', lp, r64['lp'], r32['lp'], r64['lp_abs'])
    if q is None:
        assert lq is None and kl is None and ks is None
        return
    close_sum(tag + ' logprob_q', lq, r64['lq'], r32['lq'], r64['lq_abs'])
    close_sum(tag + ' kl_samplewise', kl, r64['kl'], r32['kl'], r64['kl_abs'])
    close_elem(tag + ' kl_spatial', ks, r64['ks'], r32['ks'])   # a sum over Z non-negative terms: the element-wise rule is the tighter one


# N, Z, H, W. Float4 kernel (Z / 4 a power of two <= 16): 4 iterations of 512 groups (the model's 16x16x32 level); less than one 256-lane pass;
# 286 groups = second unrolled slot partly live, 2-lane pixel groups; one lane per pixel, no shuffles; 16-lane groups.
STOCH_V4 = [(3, 32, 16, 16), (2, 32, 5, 5), (2, 8, 11, 13), (2, 4, 7, 9), (2, 64, 3, 3)]
# Scalar kernel: Z no power of two with 300 pixels (the per-pixel fallback loop strides); shuffle path; Z = 1; a multiple of 4 but 3 groups;
# Z = 128 (no shuffle path above 64)
STOCH_SCALAR = [(2, 3, 15, 20), (2, 2, 11, 13), (2, 1, 6, 6), (2, 12, 5, 5), (2, 128, 2, 2)]


@pytest.mark.parametrize('shape', STOCH_V4 + STOCH_SCALAR, ids=lambda s: 'x'.join(map(str, s)))
def test_normal_stochastic_fwd_shapes_and_modes(K, shape):
    N, Z, H, W = shape
    for lv in LV_RANGES:
        for top in (False, True):
            p, q, eps, zf = _stoch_inputs(N, Z, H, W, top, 20 + Z + H, lv=lv)
            for analytical in (False, True):
                for mode in (0, 1, 2):
                    _stoch_fwd_check(K, 'stoch_fwd %s lv%g..%g top%d an%d mode%d' % ('x'.join(map(str, shape)), lv[0], lv[1], top, analytical, mode),
                                     p, q, zf if mode == 2 else eps, mode, analytical, Z, N)


def test_normal_stochastic_fwd_misaligned_eps_takes_the_scalar_kernel(K):
    """Z = 32 with eps a contiguous view that starts 4 bytes into its storage: the entry point routes by alignment, so this is the scalar
    kernel's 32-lane shuffle (nothing else reaches it)."""
    N, Z, H, W = 2, 32, 5, 5
    p, q, eps, zf = _stoch_inputs(N, Z, H, W, False, 31)
    refs = [(_stoch_ref(p.double(), q.double(), (zf if m == 2 else eps).double(), m, an, Z, N),
             _stoch_ref(p, q, zf if m == 2 else eps, m, an, Z, N)) for an in (False, True) for m in (0, 2)]
    for a, b in refs:
        finite(a, b)
    for an in (False, True):
        for mode in (0, 2):
            src = zf if mode == 2 else eps
            buf = torch.empty(src.numel() + 1, device='cuda')
            view = buf[1:].view(src.shape)
            view.copy_(src.cuda())
            assert view.is_contiguous() and view.data_ptr() % 16 == 4
            _stoch_fwd_check(K, 'stoch_fwd misaligned eps an%d mode%d' % (an, mode), p, q, src, mode, an, Z, N, e_dev=view)


@pytest.mark.parametrize('shape', [(5, 32, 4, 4), (5, 3, 4, 4)], ids=lambda s: 'x'.join(map(str, s)))
def test_normal_stochastic_fwd_generative_path(K, shape):
    """q = None (sampling from the prior) with the top layer's prior of batch 1 broadcast over N = 5, modes 0 and 1."""
    N, Z, H, W = shape
    for lv in LV_RANGES:
        p, _, eps, _ = _stoch_inputs(N, Z, H, W, True, 40 + Z, with_q=False, lv=lv)
        for mode in (0, 1):
            _stoch_fwd_check(K, 'stoch_fwd q=None %s lv%g..%g mode%d' % ('x'.join(map(str, shape)), lv[0], lv[1], mode), p, None, eps, mode, False, Z, N)


def _stoch_bwd_ref(p, q, e, grads, mode, analytical, Z, N, dt):
    p = leaf(p, dt)
    q = None if q is None else leaf(q, dt)
    o = _stoch_ref(p, q, e.to(dt), mode, analytical, Z, N)
    loss = None
    for key, name in (('z', 'dz'), ('lp', 'g_lp'), ('lq', 'g_lq'), ('kl', 'g_kl'), ('ks', 'g_ks')):
        if grads.get(name) is not None and key in o and o[key].requires_grad:
            term = (o[key] * grads[name].to(dt)).sum()
            loss = term if loss is None else loss + term
    if loss is not None:
        loss.backward()
    gp = p.grad if p.grad is not None else torch.zeros_like(p)
    gq = None if q is None else (q.grad if q.grad is not None else torch.zeros_like(q))
    return gp.detach(), None if gq is None else gq.detach(), o['z'].detach()


def _stoch_bwd_check(K, tag, p, q, e, grads, mode, analytical, Z, N, top):
    dp64, dq64, _ = _stoch_bwd_ref(p, q, e, grads, mode, analytical, Z, N, torch.float64)
    dp32, dq32, z32 = _stoch_bwd_ref(p, q, e, grads, mode, analytical, Z, N, torch.float32)
    finite(dp64, dp32, dq64, dq32)
    gd = {k: dev(v) for k, v in grads.items()}
    dp, dq = K.normal_stochastic_bwd(dev(p), dev(q), dev(e), dev(z32), gd.get('dz'), gd.get('g_lp'), gd.get('g_lq'), gd.get('g_kl'),
                                     gd.get('g_ks'), mode, analytical, Z)
    dp = dp.double().cpu()
    close_elem(tag + ' dp', dp.sum(0, keepdim=True) if top else dp, dp64, dp32)   # a broadcast prior: the caller sums over the batch
    if q is None:
        assert dq is None
    else:
        close_elem(tag + ' dq', dq, dq64, dq32)


@pytest.mark.parametrize('shape', [(2, 8, 11, 13), (2, 3, 15, 20)], ids=lambda s: 'x'.join(map(str, s)))
def test_normal_stochastic_bwd_modes_and_optional_gradients(K, shape):
    N, Z, H, W = shape
    g = torch.Generator().manual_seed(50 + Z)
    full = {'dz': torch.randn(N, H, W, Z, generator=g), 'g_lp': torch.randn(N, generator=g), 'g_lq': torch.randn(N, generator=g),
            'g_kl': torch.randn(N, generator=g), 'g_ks': torch.randn(N, H, W, generator=g)}
    combos = [full, {k: full[k] for k in ('dz', 'g_kl')}, {k: full[k] for k in ('g_lp', 'g_lq', 'g_ks')}]
    for lv in LV_RANGES:
        for top in (False, True):
            p, q, eps, zf = _stoch_inputs(N, Z, H, W, top, 60 + Z, lv=lv)
            for analytical in (False, True):
                for mode in (0, 1, 2):
                    for ci, grads in enumerate(combos):
                        _stoch_bwd_check(K, 'stoch_bwd %s lv%g..%g top%d an%d mode%d grads%d' % ('x'.join(map(str, shape)), lv[0], lv[1], top, analytical,
                                                                                              mode, ci),
                                         p, q, zf if mode == 2 else eps, grads, mode, analytical, Z, N, top)


@pytest.mark.parametrize('shape', [(5, 8, 3, 5), (5, 3, 4, 4)], ids=lambda s: 'x'.join(map(str, s)))
def test_normal_stochastic_bwd_generative_path(K, shape):
    N, Z, H, W = shape
    g = torch.Generator().manual_seed(70 + Z)
    full = {'dz': torch.randn(N, H, W, Z, generator=g), 'g_lp': torch.randn(N, generator=g)}
    for lv in LV_RANGES:
        p, _, eps, zf = _stoch_inputs(N, Z, H, W, True, 80 + Z, with_q=False, lv=lv)
        for mode in (0, 1, 2):
            for ci, grads in enumerate([full, {'dz': full['dz']}, {'g_lp': full['g_lp']}]):
                _stoch_bwd_check(K, 'stoch_bwd q=None %s lv%g..%g mode%d grads%d' % ('x'.join(map(str, shape)), lv[0], lv[1], mode, ci), p, None,
                                 zf if mode == 2 else eps, grads, mode, False, Z, N, True)


def test_normal_stochastic_entry_points_refuse_a_sample_past_int32(K):
    """The kernels index the elements of one sample with int: HW * Z * 2 > INT32_MAX is refused, by the entry point's name, as the residual
    entry points refuse it. Nothing is launched: the two small tensors only stand for the operands."""
    from lvae_amd import _C
    a, b = torch.zeros(8, device='cuda'), torch.zeros(8, device='cuda')
    pa, pb, s = _C.ptr(a), _C.ptr(b), _C.stream_ptr()
    HW, Z = 1 << 25, 32   # HW * Z * 2 = 2^31, the first value past the bound
    with pytest.raises(_C.LvaeHipError, match=r'lvae_normal_stochastic_fwd_f32: HW \* Z too large'):
        _C.call('lvae_normal_stochastic_fwd_f32', pa, 0, pa, pa, 1, HW, Z, 0, 0, pb, pb, pb, pb, pb, s)
    with pytest.raises(_C.LvaeHipError, match=r'lvae_normal_stochastic_bwd_f32: HW \* Z too large'):
        _C.call('lvae_normal_stochastic_bwd_f32', pa, 0, pa, pa, pa, pa, None, None, None, None, 1, HW, Z, 0, 0, pb, pb, s)
    torch.cuda.synchronize()
    assert float(a.abs().max()) == 0.0 and float(b.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. kl_elementwise
# ---------------------------------------------------------------------------------------------------------------------------------
def _kl_elem_ref(p, q, z, g, analytical, Z, dt):
    from oracle import lvae_ref as R
    p, q, z = leaf(p, dt), leaf(q, dt), leaf(z, dt)
    pmu, plv, qmu, qlv = p[..., :Z], p[..., Z:], q[..., :Z], q[..., Z:]
    out = R.normal_kl(qmu, qlv, pmu, plv) if analytical else R.normal_log_prob(z, qmu, qlv) - R.normal_log_prob(z, pmu, plv)
    out = out.expand(z.shape)
    (out * g.to(dt)).sum().backward()
    return out.detach(), p.grad.detach(), q.grad.detach(), (z.grad if z.grad is not None else torch.zeros_like(z)).detach()


@pytest.mark.parametrize('lv', LV_RANGES, ids=['wide', 'mild'])
@pytest.mark.parametrize('bcast', ['p', 'q', 'none'])
@pytest.mark.parametrize('shape', [(3, 12, 5, 7), (300, 4, 2, 2)], ids=lambda s: 'x'.join(map(str, s)))
def test_kl_elementwise_fwd_bwd(K, shape, bcast, lv):
    N, Z, H, W = shape
    p, q, eps, _ = _stoch_inputs(N, Z, H, W, False, 90 + Z, lv=lv)
    if bcast == 'p':
        p = p[:1].clone()
    if bcast == 'q':
        q = q[:1].clone()
    z = (q[..., :Z] + (q[..., Z:] / 2).exp() * eps).expand(N, H, W, Z).contiguous()
    g = torch.randn(N, H, W, Z, generator=torch.Generator().manual_seed(91))
    for analytical in (False, True):
        r64, r32 = _kl_elem_ref(p, q, z, g, analytical, Z, torch.float64), _kl_elem_ref(p, q, z, g, analytical, Z, torch.float32)
        finite(*r64, *r32)
        tag = 'kl_elem %s lv%g..%g bcast=%s an%d' % ('x'.join(map(str, shape)), lv[0], lv[1], bcast, analytical)
        close_elem(tag + ' fwd', K.kl_elementwise_fwd(dev(p), dev(q), dev(z), analytical), r64[0], r32[0])
        for need_dz in (True, False):
            dp, dq, dz = K.kl_elementwise_bwd(dev(p), dev(q), dev(z), dev(g), analytical, need_dz=need_dz)
            dp, dq = dp.double().cpu(), dq.double().cpu()          # full batch shape: the caller reduces a broadcast operand
            close_elem(tag + ' dp', dp.sum(0, keepdim=True) if bcast == 'p' else dp, r64[1], r32[1])
            close_elem(tag + ' dq', dq.sum(0, keepdim=True) if bcast == 'q' else dq, r64[2], r32[2])
            if not need_dz:
                assert dz is None
            elif analytical:
                assert float(dz.abs().max()) == 0.0           # the analytical KL does not depend on z
            else:
                close_elem(tag + ' dz', dz, r64[3], r32[3])


# ---------------------------------------------------------------------------------------------------------------------------------
# 4-6. Bernoulli, Gaussian and discretized logistic heads
# ---------------------------------------------------------------------------------------------------------------------------------
BERN_FIXED = [0., 40., -40., 88., -88., 89., -89., 200., -200.]


def _bern_ref(logits, x, dt):
    from oracle import lvae_ref as R
    l = leaf(logits, dt)
    m = torch.sigmoid(l)
    terms = -F.binary_cross_entropy(m, x.to(dt), reduction='none')
    ll = R.log_bernoulli(x.to(dt), m)
    ll.sum().backward()
    return {'mean': m.detach(), 'll': ll.detach(), 'll_abs': terms.detach().abs().sum((1, 2, 3)), 'dll': l.grad.detach()}


@pytest.mark.parametrize('case', [(3, 784), (2, 5)], ids=['3x784', '2x5'])
def test_bernoulli_head_all_outputs(K, case):
    N, P = case
    g = torch.Generator().manual_seed(110 + P)
    logits = torch.rand(N, P, generator=g) * 24 - 12
    x = (torch.rand(N, P, generator=g) < 0.5).float()
    if P >= 2 * len(BERN_FIXED):      # every fixed value with x = 0 and with x = 1, in every image
        for i, v in enumerate(BERN_FIXED):
            logits[:, 40 * i + 3], logits[:, 40 * i + 4] = v, v
            x[:, 40 * i + 3], x[:, 40 * i + 4] = 0., 1.
    else:
        logits[1] = torch.tensor([0., 88., -88., 200., -200.])
        x[1] = torch.tensor([1., 0., 1., 0., 1.])
    x[N - 1] = torch.where(x[N - 1] > 0.5, 0.7, 0.3)     # one image of soft targets (x = 0.3 at every fixed value's first slot)
    u = torch.rand(N, P, generator=g)
    logits, x, u = (t.view(N, P, 1, 1) for t in (logits, x, u))
    r64, r32 = _bern_ref(logits, x, torch.float64), _bern_ref(logits, x, torch.float32)
    finite(r64, r32)
    sure = (u.double() - r64['mean']).abs() >= 1e-6
    assert float((~sure).float().mean()) <= 0.01          # expected number left out: 2e-6 * N * P < 1
    mean, mode, sample, ll, dll = K.bernoulli_fwd(dev(logits), dev(x), dev(u), True)
    tag = 'bernoulli %dx%d' % case
    close_elem(tag + ' mean', mean, r64['mean'], r32['mean'])
    close_sum(tag + ' ll', ll, r64['ll'], r32['ll'], r64['ll_abs'])
    close_elem(tag + ' dll', dll, r64['dll'], r32['dll'])
    off_half = (r64['mean'] - 0.5).abs() > 1e-6
    assert torch.equal(mode.cpu().double()[off_half], torch.round(r64['mean'])[off_half])
    assert float(mode.cpu()[logits == 0].abs().max()) == 0.0            # round half to even, as torch.round
    assert torch.equal(sample.cpu()[sure], (u.double() < r64['mean']).float()[sure])
    mean2, mode2, sample2, ll2, dll2 = K.bernoulli_fwd(dev(logits), None, dev(u), True)
    assert ll2 is None and dll2 is None
    assert torch.equal(mean2, mean) and torch.equal(mode2, mode) and torch.equal(sample2, sample)
    _, _, _, ll3, dll3 = K.bernoulli_fwd(dev(logits), dev(x), dev(u), False)
    assert dll3 is None and torch.equal(ll3, ll)


def _gauss_ref(params, x, eps, C, dt):
    pr = leaf(params, dt)
    mean, lv = pr[..., :C], pr[..., C:]
    terms = -0.5 * ((x.to(dt) - mean) ** 2 / lv.exp() + lv + math.log(2 * math.pi))
    ll = terms.sum((1, 2, 3))
    ll.sum().backward()
    return {'ll': ll.detach(), 'll_abs': terms.detach().abs().sum((1, 2, 3)), 'dll': pr.grad.detach(),
            'sample': (mean + (lv / 2).exp() * eps.to(dt)).detach()}


HEAD_SHAPES = [(3, 3, 6, 7), (2, 1, 20, 20)]      # N, C, H, W: 126 elements per image (less than one pass) and 400 (two passes)


@pytest.mark.parametrize('shape', HEAD_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_gaussian_head(K, shape):
    N, C, H, W = shape
    g = torch.Generator().manual_seed(120 + C)
    params = torch.cat((torch.rand(N, H, W, C, generator=g) * 4 - 2, torch.rand(N, H, W, C, generator=g) * 15 - 10), -1)
    x, eps = torch.rand(N, H, W, C, generator=g), torch.randn(N, H, W, C, generator=g)
    r64, r32 = _gauss_ref(params, x, eps, C, torch.float64), _gauss_ref(params, x, eps, C, torch.float32)
    finite(r64, r32)
    sample, ll, dll = K.gaussian_fwd(dev(params), dev(x), dev(eps), True)
    tag = 'gaussian %s' % 'x'.join(map(str, shape))
    close_sum(tag + ' ll', ll, r64['ll'], r32['ll'], r64['ll_abs'])
    close_elem(tag + ' dll/dmean', dll[..., :C], r64['dll'][..., :C], r32['dll'][..., :C])
    close_elem(tag + ' dll/dlogvar', dll[..., C:], r64['dll'][..., C:], r32['dll'][..., C:])
    close_elem(tag + ' sample', sample, r64['sample'], r32['sample'])
    s2, ll2, dll2 = K.gaussian_fwd(dev(params), None, dev(eps), True)
    assert ll2 is None and dll2 is None and torch.equal(s2, sample)
    s3, ll3, dll3 = K.gaussian_fwd(dev(params), dev(x), dev(eps), False)
    assert dll3 is None and torch.equal(ll3, ll) and torch.equal(s3, sample)


def _dlog_ref(raw, x, u, C, dt):
    from oracle import lvae_ref as R
    rw = leaf(raw, dt)
    mean, ls = rw[..., :C] + 0.5, (rw[..., C:] - 1.).clamp(min=-7.)
    xs = x.to(dt) * (255 / 256) + 1 / 512
    scale, xq = ls.exp(), torch.floor(xs * 256) / 256
    cp = torch.where(xq < 255 / 256, torch.sigmoid((xq + 1 / 256 - mean) / scale), torch.ones_like(xq))
    cm = torch.where(xq >= 1 / 256, torch.sigmoid((xq - mean) / scale), torch.zeros_like(xq))
    terms = torch.log(cp - cm + 1e-7)
    ll = terms.sum((1, 2, 3))
    assert torch.equal(ll, R.log_discretized_logistic(xs, mean, ls))      # the formula above is the oracle's, kept open for its terms
    ll.sum().backward()
    uu = u.to(dt)
    sample = (mean + scale * (torch.log(uu) - torch.log(1 - uu))).clamp(0., 1.)
    return {'mean': mean.detach(), 'ls': ls.detach(), 'll': ll.detach(), 'll_abs': terms.detach().abs().sum((1, 2, 3)),
            'dll': rw.grad.detach(), 'sample': sample.detach()}


@pytest.mark.parametrize('shape', HEAD_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_discretized_logistic_head(K, shape):
    N, C, H, W = shape
    g = torch.Generator().manual_seed(130 + C)
    raw_ls = torch.rand(N, H, W, C, generator=g) * 10 - 8          # below -6 the log-scale clamps to -7
    raw_ls[:, 0, 0, 0] = -6.0                                      # exactly on the clamp: the gradient still passes (>=)
    raw_ls[:, 0, 1, 0] = -7.5
    raw_mean = torch.rand(N, H, W, C, generator=g) * 2 - 1         # means in [-0.5, 1.5]
    raw_mean[:, 0, 0, 0], raw_mean[:, 0, 1, 0] = -0.498, 0.498     # two scales off their x (0 and 1 below): gradients that are not 0
    raw = torch.cat((raw_mean, raw_ls), -1)
    x = torch.floor(256 * torch.rand(N, H, W, C, generator=g)) / 255
    x[:, 1, 0, 0], x[:, 1, 1, 0], x[:, 1, 2, 0], x[:, 1, 3, 0] = 0., 1 / 255, 254 / 255, 1.   # the open-ended bins and their neighbours
    x[:, 0, 0, 0], x[:, 0, 1, 0] = 0., 1.
    u = torch.rand(N, H, W, C, generator=g).clamp(1e-7, 1 - 1e-7)
    u[:, 2, 0, 0], u[:, 2, 1, 0] = 1e-7, 1 - 1e-7
    r64, r32 = _dlog_ref(raw, x, u, C, torch.float64), _dlog_ref(raw, x, u, C, torch.float32)
    finite(r64, r32)
    clamped = raw_ls < -6
    assert bool(clamped.any()) and float(r64['dll'][..., C:][clamped].abs().max()) == 0.0
    assert float(r64['dll'][:, 0, 0, C].abs().min()) > 0.0
    mean, ls, sample, ll, dll = K.discr_logistic_fwd(dev(raw), dev(x), dev(u), True)
    tag = 'discr_logistic %s' % 'x'.join(map(str, shape))
    close_elem(tag + ' mean', mean, r64['mean'], r32['mean'])
    close_elem(tag + ' logscale', ls, r64['ls'], r32['ls'])
    close_sum(tag + ' ll', ll, r64['ll'], r32['ll'], r64['ll_abs'])
    close_elem(tag + ' dll/dmean', dll[..., :C], r64['dll'][..., :C], r32['dll'][..., :C])
    close_elem(tag + ' dll/dlogscale', dll[..., C:], r64['dll'][..., C:], r32['dll'][..., C:])
    close_elem(tag + ' sample', sample, r64['sample'], r32['sample'])
    assert float(dll.cpu()[..., C:][clamped].abs().max()) == 0.0             # exactly zero where the log-scale is clamped
    assert float(dll.cpu()[:, 0, 0, C].abs().min()) > 0.0
    assert 0.0 <= float(sample.min()) and float(sample.max()) <= 1.0
    m2, l2, s2, ll2, dll2 = K.discr_logistic_fwd(dev(raw), None, dev(u), True)
    assert ll2 is None and dll2 is None and torch.equal(m2, mean) and torch.equal(l2, ls) and torch.equal(s2, sample)
    _, _, _, ll3, dll3 = K.discr_logistic_fwd(dev(raw), dev(x), dev(u), False)
    assert dll3 is None and torch.equal(ll3, ll)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. DMoL ragged tiles
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 7, 7), (3, 7, 7)], ids=['49px', '147px'])
@pytest.mark.parametrize('nmix', [10, 20])
def test_dmol_ragged_tiles(K, nmix, shape):
    """49 pixels are less than one workgroup of either tile size (128 pixels for 10 components, 64 for 20); 147 pixels end in a partial tile of
    19. Compared as test_dmol_any_component_count_matches_oracle compares, with its tolerances."""
    from oracle import lvae_ref as R
    N, H, W = shape
    g = torch.Generator().manual_seed(140 + nmix + N)
    l = torch.randn(N, 10 * nmix, H, W, generator=g)
    x01 = torch.floor(256 * torch.rand(N, 3, H, W, generator=g)) / 255
    x01[0, :, 0, 0], x01[0, :, 0, 1], x01[N - 1, :, H - 1, W - 1] = 0.0, 1.0, 1.0
    l64 = l.double().requires_grad_(True)
    ll_ref = R.discretized_mix_logistic_ll((x01 * 2 - 1).double(), l64)
    ll_ref.sum().backward()
    tape = R.Tape(gen=torch.Generator().manual_seed(7))
    s_ref = R.sample_discretized_mix_logistic(l, tape)
    finite(ll_ref, l64.grad, s_ref)
    ll, dl = K.dmol_ll_fwd(nhwc(l), nhwc(x01), True)
    torch.testing.assert_close(ll.cpu().double(), ll_ref.detach(), rtol=1e-5, atol=1e-3)
    assert rel(nchw(dl).double(), l64.grad) < 2e-4
    ll_only, none = K.dmol_ll_fwd(nhwc(l), nhwc(x01), False)
    assert none is None and torch.equal(ll_only, ll)
    u_mix, u_log = [torch.as_tensor(e).float().cuda().contiguous() for e in tape.entries]
    s = K.dmol_sample(nhwc(l), u_mix, u_log)
    torch.testing.assert_close(nchw(s) * 2 - 1, s_ref, rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. Gate
# ---------------------------------------------------------------------------------------------------------------------------------
TORCH_ACT = {'elu': F.elu, 'relu': F.relu, 'leakyrelu': lambda t: F.leaky_relu(t, 0.01), 'selu': F.selu}


def _gate_ref(ab, res, dout, act, C, dt):
    ab = leaf(ab, dt)
    out = TORCH_ACT[act](ab[..., :C]) * torch.sigmoid(ab[..., C:])
    if res is not None:
        out = out + res.to(dt)
    (out * dout.to(dt)).sum().backward()
    return out.detach(), ab.grad.detach()


# (rows, C): float4 columns with all 256 threads busy; 25 columns and 10 rows per pass (six threads idle); the scalar instantiation (C = 3 and
# C = 255: one row per pass, one thread idle); one row per pass of 256 float4 columns
@pytest.mark.parametrize('shape', [(80, 64), (37, 100), (37, 3), (5, 255), (3, 1024)], ids=lambda s: 'x'.join(map(str, s)))
def test_gate_fwd_bwd_every_activation(K, shape):
    M, C = shape
    g = torch.Generator().manual_seed(150 + C)
    ab = torch.randn(M, 1, 1, 2 * C, generator=g) * 3
    edge = torch.tensor([0., 30., -30.])
    for i in range(min(3, C)):      # 0 and +-30 in both halves, against each other where C allows
        ab[0, 0, 0, i], ab[0, 0, 0, C + i] = edge[i], edge[(i + 1) % 3]
        ab[M - 1, 0, 0, C - 1 - i], ab[M - 1, 0, 0, 2 * C - 1 - i] = edge[(i + 2) % 3], edge[i]
    ab[1, 0, 0, 0], ab[1, 0, 0, C] = 0., 0.
    res_t, dout = torch.randn(M, 1, 1, C, generator=g), torch.randn(M, 1, 1, C, generator=g)
    for act in ('elu', 'relu', 'leakyrelu', 'selu'):
        for res in (res_t, None):
            r64, r32 = _gate_ref(ab, res, dout, act, C, torch.float64), _gate_ref(ab, res, dout, act, C, torch.float32)
            finite(*r64, *r32)
            tag = 'gate %dx%d %s res%d' % (M, C, act, res is not None)
            close_elem(tag + ' fwd', K.gate_fwd(dev(ab), dev(res), act), r64[0], r32[0])
            close_elem(tag + ' bwd', K.gate_bwd(dev(dout), dev(ab), act), r64[1], r32[1])


@pytest.mark.parametrize('act', ['elu', 'relu', 'leakyrelu', 'selu'])
def test_act_bwd_from_out(K, act):
    """The derivative taken from the activation's OUTPUT against the derivative from x, on the elements where the two are the same function
    (|x| > 1e-6: at 0 the output of relu no longer tells which side x was on)."""
    n = 70000            # 274 workgroups
    g = torch.Generator().manual_seed(160)
    x, dy = torch.randn(n, generator=g) * 3, torch.randn(n, generator=g)
    x[:3] = torch.tensor([0., 30., -30.])
    y = TORCH_ACT[act](x)

    def ref(dt):
        xx = leaf(x, dt)
        (TORCH_ACT[act](xx) * dy.to(dt)).sum().backward()
        return xx.grad.detach()

    r64, r32 = ref(torch.float64), ref(torch.float32)
    finite(r64, r32)
    keep = x.abs() > 1e-6
    dx = K.act_bwd_from_out(dev(dy), dev(y), act)
    close_elem('act_bwd_from_out %s' % act, dx.cpu()[keep], r64[keep], r32[keep])


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. Glue
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 1027, 2048 * 256 + 77])       # the last takes a second grid-stride sweep
def test_add_add3_exact(K, n):
    g = torch.Generator().manual_seed(170)
    a, b, c = (torch.randn(n, generator=g) * 10 ** float(i) for i in range(3))
    assert torch.equal(K.add(dev(a), dev(b)).cpu(), a + b)
    assert torch.equal(K.add3(dev(a), dev(b), dev(c)).cpu(), (a + b) + c)        # in that order


@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (3, 5, 7, 9), (5, 16, 16, 32)])
def test_scale_per_sample_and_scale_rows_add_exact(K, shape):
    g = torch.Generator().manual_seed(171)
    N, H, W, C = shape
    a, b = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    gs, rs = torch.randn(N, generator=g), torch.randn(N, C, generator=g)
    assert torch.equal(K.scale_per_sample(dev(a), dev(gs)).cpu(), a * gs.view(N, 1, 1, 1))
    scaled = a * rs.view(N, 1, 1, C)
    assert torch.equal(K.scale_rows_add(dev(a), dev(rs), dev(b)).cpu(), scaled + b)     # product and sum rounded separately
    assert torch.equal(K.scale_rows_add(dev(a), dev(rs), None).cpu(), scaled)
    assert torch.equal(K.scale_rows_add(dev(a), None, dev(b)).cpu(), a + b)
    out = torch.full(shape, float('nan'), device='cuda')
    assert K.scale_rows_add(dev(a), None, None, out=out) is out and torch.equal(out.cpu(), a)   # with neither: a copy


@pytest.mark.parametrize('n', [1, 3, 4, 1027])
def test_fill_and_fill_zero_stop_at_n(K, n):
    for fn, want in ((lambda t: K.fill(t, 2.5), 2.5), (lambda t: K.fill(t), 0.0), (K.fill_zero, 0.0)):
        buf = torch.full((n + 9,), float('nan'), device='cuda')
        fn(buf[:n])
        got = buf.cpu()
        assert bool((got[:n] == want).all()) and bool(torch.isnan(got[n:]).all())


@pytest.mark.parametrize('shape', [(15, 256), (3, 37), (1, 1)], ids=lambda s: 'x'.join(map(str, s)))
def test_sum_of_row_means(K, shape):
    L, N = shape
    x = torch.randn(L, N, generator=torch.Generator().manual_seed(172)) * 100 - 300
    r64, r32 = x.double().mean(1).sum().view(1), x.mean(1).sum().view(1)
    finite(r64, r32)
    close_sum('sum_of_row_means %dx%d' % shape, K.sum_of_row_means(dev(x)), r64, r32, (x.double().abs() / N).sum().view(1))


# N, C, H, W
@pytest.mark.parametrize('shape', [(2, 4, 1, 1), (2, 8, 1, 5), (1, 12, 7, 3), (3, 64, 16, 16)], ids=lambda s: 'x'.join(map(str, s)))
def test_upsample2x_shapes(K, shape):
    g = torch.Generator().manual_seed(173)
    x = torch.randn(shape, generator=g)
    dy = torch.randn(shape[0], shape[1], 2 * shape[2], 2 * shape[3], generator=g)

    def ref(dt):
        xx = leaf(x, dt)
        y = F.interpolate(xx, scale_factor=2, mode='bilinear', align_corners=False)
        (y * dy.to(dt)).sum().backward()
        return y.detach(), xx.grad.detach()

    r64, r32 = ref(torch.float64), ref(torch.float32)
    finite(*r64, *r32)
    tag = 'upsample2x %s' % 'x'.join(map(str, shape))
    close_elem(tag + ' fwd', nchw(K.upsample2x_fwd(nhwc(x))), r64[0], r32[0])
    close_elem(tag + ' bwd', nchw(K.upsample2x_bwd(nhwc(dy))), r64[1], r32[1])


def test_upsample2x_refuses_channels_that_are_no_multiple_of_four(K):
    with pytest.raises(K._C.LvaeHipError):
        K.upsample2x_fwd(torch.zeros(1, 2, 2, 6, device='cuda'))
    with pytest.raises(K._C.LvaeHipError):
        K.upsample2x_bwd(torch.zeros(1, 4, 4, 6, device='cuda'))


# ---------------------------------------------------------------------------------------------------------------------------------
# 10. Bookkeeping
# ---------------------------------------------------------------------------------------------------------------------------------
def _book_ref(kl_nl, ll, fb, beta, gr, dt):
    from oracle import lvae_ref as R
    kl, llv = leaf(kl_nl, dt), leaf(ll, dt)
    N = kl.shape[0]
    clamped = kl if fb < 1e-6 else kl.clamp(min=fb)
    kl_loss = R.free_bits_kl(kl, fb).sum()
    kl_sep, kl_avg = kl.sum(1), kl.mean(0)
    scal = torch.stack((kl_loss, kl_sep.mean()))
    ((kl_sep * gr['g_sep'].to(dt)).sum() + (kl_avg * gr['g_avg'].to(dt)).sum() + (scal * gr['g_scal'].to(dt)).sum()).backward()
    dkl = kl.grad.detach().clone()
    elbo_sep = llv - kl_sep.detach()
    recons = (-llv).mean()
    scal3 = torch.stack((recons + beta * kl_loss.detach(), elbo_sep.mean(), recons))
    llv.grad = None
    (scal3[0] * gr['g_loss'].to(dt)).backward()
    a = kl.detach().abs()
    return {'kl_sep': kl_sep.detach(), 'kl_sep_abs': a.sum(1), 'kl_avg': kl_avg.detach(), 'kl_avg_abs': a.sum(0) / N, 'scal': scal.detach(),
            'scal_abs': torch.stack((clamped.detach().abs().sum() / N, a.sum() / N)), 'dkl': dkl, 'elbo_sep': elbo_sep.detach(),
            'scal3': scal3.detach(), 'd_ll': llv.grad.detach(),
            'scal3_abs': torch.stack((llv.detach().abs().sum() / N + abs(beta) * kl_loss.detach().abs(),
                                      (llv.detach().abs() + kl_sep.detach().abs()).sum() / N, llv.detach().abs().sum() / N))}


@pytest.mark.parametrize('shape', [(15, 300), (1, 1)], ids=lambda s: 'x'.join(map(str, s)))
def test_kl_bookkeeping_and_elbo_loss(K, shape):
    L, N = shape
    g = torch.Generator().manual_seed(180 + L)
    kl = torch.rand(N, L, generator=g) * 2
    ll = -torch.rand(N, generator=g) * 100
    gr = {'g_sep': torch.randn(N, generator=g), 'g_avg': torch.randn(L, generator=g), 'g_scal': torch.tensor([1.7, -0.6]),
          'g_loss': torch.tensor(1.3)}
    beta = 0.3
    for fb in (0.0, 0.7, float(kl[N // 2, L // 2])):      # the last: free bits EQUAL to one entry (the kernel's >= is free_bits_kl's clamp)
        r64, r32 = _book_ref(kl, ll, fb, beta, gr, torch.float64), _book_ref(kl, ll, fb, beta, gr, torch.float32)
        finite(r64, r32)
        tag = 'bookkeeping %dx%d fb=%.3g' % (L, N, fb)
        kl_ln = dev(kl.t())
        ksep, kavg, scal = K.kl_bookkeeping_fwd(kl_ln, fb)
        close_sum(tag + ' kl_sep', ksep, r64['kl_sep'], r32['kl_sep'], r64['kl_sep_abs'])
        close_sum(tag + ' kl_avg', kavg, r64['kl_avg'], r32['kl_avg'], r64['kl_avg_abs'])
        close_sum(tag + ' kl_loss,kl', scal, r64['scal'], r32['scal'], r64['scal_abs'])
        dkl = K.kl_bookkeeping_bwd(kl_ln, fb, dev(gr['g_sep']), dev(gr['g_avg']), dev(gr['g_scal']))
        close_elem(tag + ' dkl', dkl.t(), r64['dkl'], r32['dkl'])
        # the ELBO assembly takes kl_sep and kl_loss as inputs: give it the fp32 reference's, so that only its own arithmetic is compared
        esep, s3 = K.elbo_loss_fwd(dev(ll), dev(r32['kl_sep']), dev(r32['scal'][0:1]), beta)
        e64 = ll.double() - r32['kl_sep'].double()
        close_elem(tag + ' elbo_sep', esep, e64, ll - r32['kl_sep'])
        recons64 = (-ll.double()).mean()
        s3_64 = torch.stack((recons64 + beta * r32['scal'][0].double(), e64.mean(), recons64))
        recons32 = (-ll).mean()
        s3_32 = torch.stack((recons32 + beta * r32['scal'][0], (ll - r32['kl_sep']).mean(), recons32))
        close_sum(tag + ' loss,elbo,recons', s3, s3_64, s3_32, r64['scal3_abs'])
        d_ll, d_kll = K.elbo_loss_bwd(dev(gr['g_loss'].view(1)), beta, N)
        close_elem(tag + ' d_ll', d_ll, r64['d_ll'], r32['d_ll'])
        close_elem(tag + ' d_kl_loss', d_kll, (gr['g_loss'].double() * beta).view(1), (gr['g_loss'] * beta).view(1))


@pytest.mark.parametrize('shape', [(1, 1), (7, 257), (1000, 300)], ids=lambda s: 'x'.join(map(str, s)))
def test_iw_logmeanexp_and_online(K, shape):
    """ELBOs near -3000 with spread 50: a sum of exponentials without the max shift underflows to log(0)."""
    S, N = shape
    elbo = torch.randn(S, N, generator=torch.Generator().manual_seed(190 + S)) * 50 - 3000
    e64 = elbo.double()
    iw64, iw32 = torch.logsumexp(e64, 0) - math.log(S), torch.logsumexp(elbo, 0) - math.log(S)
    m64, m32 = e64.mean(0), elbo.mean(0)
    finite(iw64, iw32, m64, m32)
    assert float(torch.exp(elbo).sum()) == 0.0
    tag = 'iw %dx%d' % shape
    ed = dev(elbo)
    a = K.iw_logmeanexp(ed)
    close_elem(tag + ' logmeanexp', a, iw64, iw32)
    state = torch.full((3, N), float('nan'), device='cuda')
    K.iw_online(state, 0)
    for s in range(S):
        K.iw_online(state, 1, elbo=ed[s])
    iw, mean = torch.empty(N, device='cuda'), torch.empty(N, device='cuda')
    K.iw_online(state, 2, S=S, iw=iw, mean=mean)
    close_elem(tag + ' online', iw, iw64, iw32)
    close_sum(tag + ' online mean', mean, m64, m32, e64.abs().sum(0) / S)
    e32 = float((iw32.double() - iw64).abs().max())
    assert bool(((iw.double() - a.double()).abs().cpu() <= 2 * e32 + 1e-5 * iw64.abs() + 1e-6).all())      # the two kernels agree


# ---------------------------------------------------------------------------------------------------------------------------------
# 11. Adamax and L2 norm
# ---------------------------------------------------------------------------------------------------------------------------------
def _adamax_ref(p0, m0, u0, grads, gscale, lr, wd, dt):
    p = leaf(p0, dt)
    opt = torch.optim.Adamax([p], lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    for gr in grads:
        p.grad = gr.to(dt) * gscale
        opt.step()
        if m0 is not None:        # the optimizer creates its state at the first step: redo that step from the given state
            st = opt.state[p]
            with torch.no_grad():
                p.copy_(p0.to(dt))
                st['exp_avg'].copy_(m0.to(dt))
                st['exp_inf'].copy_(u0.to(dt))
                st['step'].fill_(0)
            m0 = None
            opt.step()
    st = opt.state[p]
    return p.detach(), st['exp_avg'].detach(), st['exp_inf'].detach()


def test_adamax_mask_weight_decay_gscale_second_sweep(K):
    n = 2101252            # a multiple of 4 with more than 2048 * 256 float4: the grid-stride loop takes a second sweep
    assert n % 4 == 0 and n // 4 > 2048 * 256
    g = torch.Generator().manual_seed(200)
    p0, m0, u0 = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) + 0.05
    grads = [torch.randn(n, generator=g) for _ in range(3)]
    zero_at = 4 * 2048 * 256 + 2          # gradient and parameter 0 (in the second sweep): eps alone decides u
    p0[zero_at], m0[zero_at], u0[zero_at] = 0., 0., 0.
    for gr in grads:
        gr[zero_at] = 0.
    mask = (torch.rand(n, generator=g) < 0.9).float()
    mask[0], mask[n - 1], mask[5], mask[4], mask[6], mask[zero_at] = 0., 0., 0., 1., 1., 1.      # both ends; a 0 inside a float4
    lr, wd, gscale = 3e-4, 1e-2, 0.25
    r64, r32 = _adamax_ref(p0, m0, u0, grads, gscale, lr, wd, torch.float64), _adamax_ref(p0, m0, u0, grads, gscale, lr, wd, torch.float32)
    finite(*r64, *r32)
    assert float(r64[2][zero_at]) == 1e-8 and float(r64[0][zero_at]) == 0.0
    pd, md, ud = dev(p0), dev(m0), dev(u0)
    step = torch.zeros(1, dtype=torch.int64, device='cuda')
    gs = torch.tensor([gscale], device='cuda')
    maskd = dev(mask)
    for gr in grads:
        K.adamax_step(pd, dev(gr), md, ud, maskd, lr, 0.9, 0.999, 1e-8, wd, gs, step)
        K.counter_advance(step)
    on, off = mask > 0, mask == 0
    for name, got, init, a, b in (('p', pd, p0, r64[0], r32[0]), ('exp_avg', md, m0, r64[1], r32[1]), ('exp_inf', ud, u0, r64[2], r32[2])):
        got = got.cpu()
        assert torch.equal(got[off], init[off]), name       # masked elements keep p, m and u bit for bit
        close_elem('adamax n=%d %s' % (n, name), got[on], a[on], b[on])
    with pytest.raises(K._C.LvaeHipError):
        z = torch.zeros(1002, device='cuda')
        K.adamax_step(z, z.clone(), z.clone(), z.clone(), None, lr, 0.9, 0.999, 1e-8, 0.0, None, step)


@pytest.mark.parametrize('n', [1, 2047, 2049, 4195332])      # one element; around one workgroup's 2048; 2048 partials, each a second sweep
def test_l2norm_sizes(K, n):
    x = torch.randn(n, generator=torch.Generator().manual_seed(210))
    r64 = float(x.double().norm())
    assert math.isfinite(r64)
    got = float(K.l2norm(dev(x)).cpu()[0])
    print('yardstick | %-58s | kernel %.3e | r32 %.3e | bound %.3e | n 1' % ('l2norm n=%d' % n, abs(got - r64), abs(float(x.norm()) - r64), 2e-6 * r64))
    assert abs(got - r64) <= 2e-6 * r64          # the project's rtol = 1e-6 for this kernel, doubled for the deeper summation


# ---------------------------------------------------------------------------------------------------------------------------------
# 12. The generator
# ---------------------------------------------------------------------------------------------------------------------------------
def test_rng_fill_is_the_cpu_restatement_bit_for_bit(K):
    from oracle import philox_ref as P
    seed = (1 << 40) + 12345
    cases = [(n, sid, off) for n in (1, 5, 4099) for sid in (1, (1 << 32) + 3) for off in (0, 7, (1 << 32) + 5)]
    refs = {c: (P.fill(c[0], 'uniform', 0.0, 1.0, seed, c[2], c[1]), P.fill(c[0], 'bernoulli', 0.8, 1.25, seed, c[2], c[1]),
                P.fill(c[0], 'normal', 0.0, 0.0, seed, c[2], c[1])) for c in cases}
    worst = 0.0
    for (n, sid, off), (u_ref, b_ref, z_ref) in refs.items():
        offd = torch.tensor([off], dtype=torch.int64, device='cuda')
        buf = torch.full((n + 5,), float('nan'), device='cuda')
        u = K.rng_fill(buf[:n], 'uniform', 0.0, 1.0, seed, offd, sid)
        assert np.array_equal(u.cpu().numpy(), u_ref), (n, sid, off)
        assert bool(torch.isnan(buf[n:]).all())                       # a ragged last block writes nothing past n
        b = K.rng_fill(torch.empty(n, device='cuda'), 'bernoulli', 0.8, 1.25, seed, offd, sid)
        assert np.array_equal(b.cpu().numpy(), b_ref), (n, sid, off)
        z = K.rng_fill(torch.empty(n, device='cuda'), 'normal', 0.0, 0.0, seed, offd, sid)
        worst = max(worst, float(np.abs(z.cpu().numpy().astype(np.float64) - z_ref).max()))
    # 2 pi u and the constant 2 pi are rounded to fp32: at most 4.2e-7 rad, times a radius of at most 5.9 = 2.5e-6; the rest is a few ulp of
    # logf, sqrtf and sincosf
    print('yardstick | %-58s | kernel %.3e | r32 %.3e | bound %.3e | n %d' % ('rng_fill normal vs float64 Box-Muller', worst, 0.0, 5e-6, len(refs)))
    assert worst <= 5e-6
    # the offset-less form is step 0
    u0 = K.rng_fill(torch.empty(5, device='cuda'), 'uniform', 0.0, 1.0, seed, None, 1)
    assert np.array_equal(u0.cpu().numpy(), refs[(5, 1, 0)][0])


def test_uniform_draws_never_reach_one(K):
    """seed 4, stream id 1, step 0: the raw word of flat element 2170657 has its top 24 bits set (tests/test_philox_cpu.py), and
    (2^24 - 1 + 0.5) * 2^-24 rounds to exactly 1.0 in fp32. The draw is clamped to the largest float below 1."""
    n, k = 2170660, 2170657
    off = torch.zeros(1, dtype=torch.int64, device='cuda')
    u = K.rng_fill(torch.empty(n, device='cuda'), 'uniform', 0.0, 1.0, 4, off, 1)
    assert float(u.max()) < 1.0 and float(u.min()) > 0.0
    assert float(u[k]) == 1.0 - 2.0 ** -24
    b = K.rng_fill(torch.empty(n, device='cuda'), 'bernoulli', 1.0, 1.0, 4, off, 1)
    assert float(b[k]) == 1.0 and float(b.min()) == 1.0          # a keep-probability of 1 keeps every element
