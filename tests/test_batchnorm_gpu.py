"""The BatchNorm and affine-activation kernels of csrc/norm_act.hip (+ csrc/bn_stats.h) at their edges: bn_stats, bn_finalize_parts,
bn_eval_coeffs, affine_act, affine_act_bwd (training and eval, dropout mask and residual add folded in) and affine_act_bwd_parts (the apply
from the partial rows of a dgrad epilogue), each against the plain torch formula of the same operation in float64.

Rule (docs/ELEMENTWISE_PARITY.md; no tolerance per test). r64 is F.batch_norm(..., training=...) followed by the activation in float64 on
the CPU, gradients by autograd, the dropout mask and the residual add written out as dx = autograd_dx * drop[n, c] + add; r32 the same in
float32 on the CPU.

    element-wise outputs (y, dx, scale, shift, mean, rstd, running pair, eval coefficients)
                              |kernel - r64| <= 2 max|r32 - r64| + 1e-5 |r64| + 1e-6
    per-channel sums (dgamma, dbeta)
                              |kernel - r64| <= 2 max|r32 - r64| + 4e-6 sum |term|      (the M terms of that channel, in float64)

Every comparison is per element, prints `yardstick | case | kernel error | r32 error | bound` before it asserts (run with -s), and every
reference is checked to be finite before a tensor goes to the device. Tensors are NHWC on the device; (N, H, W, C) gives M = N H W rows.
Which path of the library a shape takes (thread map, scalar or float4 kernel, chunk cap, parts kernel or finalize launch) is said beside it.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS = 1e-5
INF = float('inf')
ACTS = ['elu', 'relu', 'leakyrelu', 'selu', None]
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope='module')
def K():
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels
    return kernels


def dev(t):
    return None if t is None else t.contiguous().cuda()


def misaligned(t):
    """a device copy of t that starts one float into a 16-byte aligned buffer: vec_ok() fails and the scalar kernels run"""
    buf = dev(torch.zeros(t.numel() + 4))
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def gen(seed):
    return torch.Generator().manual_seed(seed)


def leaf(t, dt):
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
    print('yardstick | %-72s | kernel %.3e | r32 %.3e | bound %.3e | n %d' % (tag, float(err[k]), e32, float(bound[k]), err.numel()))
    assert bool((err <= bound).all()), '%s: |kernel - r64| = %.6e at flat element %d, bound %.6e (r32 error %.3e)' % (
        tag, float(err[k]), k, float(bound[k]), e32)


def close_elem(tag, got, r64, r32):
    _cmp(tag, got, r64, r32, 1e-5 * r64.detach().double().abs() + 1e-6)


def close_sum(tag, got, r64, r32, abs_terms):
    _cmp(tag, got, r64, r32, 4e-6 * abs_terms.detach().double())


def same_bits(a, b):
    return a.shape == b.shape and bool((a.detach().cpu().view(torch.int32) == b.detach().cpu().view(torch.int32)).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------------
def act_ref(u, act):
    if act == 'elu':
        return F.elu(u)
    if act == 'relu':
        return F.relu(u)
    if act == 'leakyrelu':
        return F.leaky_relu(u, 0.01)
    if act == 'selu':
        return F.selu(u)
    return u * 1.0


def ref_bn(dt, x, gamma, beta, act=None, dh=None, rm=None, rv=None, momentum=0.1, eps=EPS):
    """Training-mode BatchNorm of x (N, H, W, C) + activation in dtype dt. The statistics by their plain formula, the running pair as
    F.batch_norm leaves it, y, and with dh the gradients by autograd (dx before mask and add) and the per-channel sums of |term|."""
    Cn = x.shape[-1]
    x2 = leaf(x.reshape(-1, Cn), dt)
    ga = None if gamma is None else leaf(gamma, dt)
    be = None if beta is None else leaf(beta, dt)
    o = {'running_mean': None if rm is None else rm.to(dt).clone(), 'running_var': None if rv is None else rv.to(dt).clone()}
    u = F.batch_norm(x2, o['running_mean'], o['running_var'], ga, be, True, momentum, eps)
    with torch.no_grad():
        mean, var = x2.mean(0), x2.var(0, unbiased=False)
        rstd = 1 / torch.sqrt(var + eps)
        scale = rstd if ga is None else ga * rstd
        o.update(mean=mean, rstd=rstd, scale=scale, shift=-mean * scale if be is None else be - mean * scale)
    y = act_ref(u, act)
    o['y'] = y.detach().reshape(x.shape)
    if dh is not None:
        u.retain_grad()
        y.backward(dh.reshape(-1, Cn).to(dt))
        g, xhat = u.grad, (x2.detach() - mean) * rstd
        o.update(dx=x2.grad.reshape(x.shape), dgamma=(g * xhat).sum(0) if ga is None else ga.grad, dbeta=g.sum(0) if be is None else be.grad,
                 tg=(g * xhat).abs().sum(0), tb=g.abs().sum(0))
    return o


def ref_affine(dt, x, scale, shift, act, row_scale=None, dh=None):
    """y = act(x * scale + shift) * row_scale[n, c] (scale None: the identity affine) and, with dh, dx by autograd"""
    N, Cn = x.shape[0], x.shape[-1]
    x_ = leaf(x, dt)
    u = x_ * 1.0 if scale is None else x_ * scale.to(dt) + shift.to(dt)
    y = act_ref(u, act)
    if row_scale is not None:
        y = y * row_scale.to(dt).view(N, 1, 1, Cn)
    o = {'y': y.detach(), 'u': u.detach()}
    if dh is not None:
        y.backward(dh.to(dt))
        o['dx'] = x_.grad
    return o


def fold(dx, drop, add):
    """dx = autograd_dx * drop[n, c] + add, in dx's dtype"""
    N, Cn = dx.shape[0], dx.shape[-1]
    if drop is not None:
        dx = dx * drop.to(dx.dtype).view(N, 1, 1, Cn)
    if add is not None:
        dx = dx + add.to(dx.dtype)
    return dx


def keep_mask(g, N, Cn, keep=0.8):
    """a dropout mask as the model draws it per (sample, channel): zeros and 1 / keep"""
    m = (torch.rand(N, Cn, generator=g) < keep).float() / keep
    m[0, 0], m[-1, -1] = 0.0, 1 / keep                                   # both values present whatever the draw
    return m


def chunk_sums(v, rows):
    """(M, 2, C) float64 -> (rows, 2, C) float32: one partial row per chunk of pixels, as a producer with `rows` workgroups writes them"""
    return torch.stack([c.sum(0) for c in v.tensor_split(rows)]).float().contiguous()


def coef32(r64):
    return [r64[k].float() for k in ('scale', 'shift', 'mean', 'rstd')]


def check_stats(tag, got, r64, r32):
    for name, t in zip(('scale', 'shift', 'mean', 'rstd'), got):
        close_elem('%s %s' % (tag, name), t, r64[name], r32[name])


def check_running(tag, rm, rv, r64, r32):
    close_elem(tag + ' running_mean', rm, r64['running_mean'], r32['running_mean'])
    close_elem(tag + ' running_var', rv, r64['running_var'], r32['running_var'])


# ---------------------------------------------------------------------------------------------------------------------------------
# A. bn_stats
# ---------------------------------------------------------------------------------------------------------------------------------
A_SHAPES = [(2, 3, 5, 12),          # cols 3, rpp 85: thread 255 owns no row group
            (3, 4, 4, 100),         # cols 25, rpp 10: six idle threads
            (2, 2, 2, 132),         # cols 33, rpp 7: 25 idle threads
            (2, 3, 3, 260),         # cols 65, rpp 3: 61 idle threads
            (1, 2, 3, 1024),        # cols 256, rpp 1
            (2, 4, 4, 512),         # cols 128, rpp 2
            (5, 3, 3, 6),           # C % 4 != 0: scalar kernel
            (7, 1, 1, 255),         # scalar kernel, cols 255
            (1, 1, 3, 64),          # M = 3 rows under rpp = 16
            (2, 2049, 1, 1024),     # M = 4098 > 1024 * 4 * rpp: 820 chunks of 5 rows, the last one of 3
            (3, 5463, 1, 256)]      # M = 16389 > 1024 * 4 * 4: rows_per_chunk 17 -> 20 (a multiple of rpp), 820 chunks, the last one of 9


def _bn_params(g, Cn):
    return (torch.rand(Cn, generator=g) + 0.5, torch.randn(Cn, generator=g), torch.randn(Cn, generator=g), torch.rand(Cn, generator=g) + 0.5)


@pytest.mark.parametrize('shape', A_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_bn_stats_shapes(K, shape):
    """all four coefficient rows and the running pair (M - 1 divisor), momentum 0.1 and 0.37; once without gamma / beta, once without the
    running pair"""
    N, H, W, Cn = shape
    g = gen(sum(shape))
    x = torch.randn(shape, generator=g) * 1.5 + 2 * torch.randn(Cn, generator=g)
    gamma, beta, rm0, rv0 = _bn_params(g, Cn)
    refs = {m: [ref_bn(dt, x, gamma, beta, rm=rm0, rv=rv0, momentum=m) for dt in (F64, F32)] for m in (0.1, 0.37)}
    plain = [ref_bn(dt, x, None, None, rm=rm0, rv=rv0) for dt in (F64, F32)]
    finite(plain[0], plain[1], *[r for p in refs.values() for r in p])
    xd, tag = dev(x), 'bn_stats %s' % 'x'.join(map(str, shape))
    for m, (r64, r32) in refs.items():
        rm, rv = dev(rm0), dev(rv0)
        got = K.bn_stats(xd, dev(gamma), dev(beta), rm, rv, EPS, m)
        check_stats('%s m=%g' % (tag, m), got, r64, r32)
        check_running('%s m=%g' % (tag, m), rm, rv, r64, r32)
    rm, rv = dev(rm0), dev(rv0)
    check_stats(tag + ' no gamma/beta', K.bn_stats(xd, None, None, rm, rv, EPS, 0.1), *plain)
    check_running(tag + ' no gamma/beta', rm, rv, *plain)
    check_stats(tag + ' no running pair', K.bn_stats(xd, dev(gamma), dev(beta), None, None, EPS, 0.1), *refs[0.1])


def test_bn_stats_misaligned_input_takes_the_scalar_kernel(K):
    shape = (2, 4, 4, 64)
    g = gen(64)
    x = torch.randn(shape, generator=g) * 1.5 + 2 * torch.randn(64, generator=g)
    gamma, beta, rm0, rv0 = _bn_params(g, 64)
    r64, r32 = [ref_bn(dt, x, gamma, beta, rm=rm0, rv=rv0, momentum=0.37) for dt in (F64, F32)]
    finite(r64, r32)
    rm, rv = dev(rm0), dev(rv0)
    got = K.bn_stats(misaligned(x), dev(gamma), dev(beta), rm, rv, EPS, 0.37)
    check_stats('bn_stats misaligned 2x4x4x64', got, r64, r32)
    check_running('bn_stats misaligned 2x4x4x64', rm, rv, r64, r32)


def test_bn_stats_refuses_a_misaligned_input_above_256_channels(K):
    """the scalar kernel has one thread per channel: C = 260 with a misaligned pointer (or C % 4 != 0) is EINVAL, and nothing is written"""
    g = gen(260)
    x = torch.randn(2, 3, 3, 260, generator=g)
    gamma, beta, rm0, rv0 = _bn_params(g, 260)
    rm, rv = dev(rm0), dev(rv0)
    with pytest.raises(K._C.LvaeHipError, match='above 256 channels'):
        K.bn_stats(misaligned(x), dev(gamma), dev(beta), rm, rv)
    with pytest.raises(K._C.LvaeHipError, match='above 256 channels'):
        K.bn_stats(dev(torch.randn(2, 3, 3, 258, generator=g)), None, None, None, None)
    torch.cuda.synchronize()
    assert same_bits(rm, rm0) and same_bits(rv, rv0)


# ---------------------------------------------------------------------------------------------------------------------------------
# B. conditioning
# ---------------------------------------------------------------------------------------------------------------------------------
COND_RATIO = 1000.0     # |mean| / std of the ordinary channels; r32 stays finite and inside the rule at it (checked below on the CPU)


def _cond_input(Cn, pivot_at_the_edge):
    g = gen(Cn + int(pivot_at_the_edge))
    std = 0.3
    x = std * COND_RATIO + std * torch.randn(4, 8, 8, Cn, generator=g)
    if pivot_at_the_edge:
        x[0, 0, 0, :] = std * COND_RATIO + 8 * std         # row 0 is the pivot of bn_partial_kernel: 8 std away from the rest
    x[..., 1] = 1.7                                        # constant: the m2 < 0 clamp, rstd = 1 / sqrt(eps)
    x[..., 2] = 0.0
    return x, torch.randn(4, 8, 8, Cn, generator=g), _bn_params(g, Cn)


@pytest.mark.parametrize('pivot_at_the_edge', [False, True])
@pytest.mark.parametrize('Cn', [8, 64])
def test_conditioning_mean_over_std_1000_and_constant_channels(K, Cn, pivot_at_the_edge):
    """statistics -> affine_act -> training backward as the model chains them (the kernels' own coefficients feed the next kernel).
    x * scale + shift is here the difference of two numbers near 1000 to 1500, so float32 is good to ~1e-4 in y however it is written:
    measured on an MI355X the kernel's y is off by 2.0e-4 against a bound of 2.1e-4 (C = 64, pivot at the edge; r32 1.0e-4, the floor of
    the affine form in float32 - a CPU that orders its sums worse only widens the bound). docs/ELEMENTWISE_PARITY.md has the table."""
    x, dh, (gamma, beta, rm0, rv0) = _cond_input(Cn, pivot_at_the_edge)
    r64, r32 = [ref_bn(dt, x, gamma, beta, 'elu', dh, rm0, rv0) for dt in (F64, F32)]
    finite(r64, r32)
    for k in ('mean', 'rstd', 'scale', 'shift', 'y', 'dx'):  # r32 itself: finite (above) and of use as a yardstick at this ratio, i.e. within 1 % of the values' size
        assert float((r32[k].double() - r64[k]).abs().max()) <= 1e-2 * float(r64[k].abs().max()), k
    assert float(r64['rstd'][1]) == pytest.approx(EPS ** -0.5, rel=1e-12) and float(r64['rstd'][2]) == pytest.approx(EPS ** -0.5, rel=1e-12)
    tag = 'conditioning C=%d ratio %g%s' % (Cn, COND_RATIO, ' pivot at +8 std' if pivot_at_the_edge else '')
    xd, rm, rv = dev(x), dev(rm0), dev(rv0)
    sc, sh, mean, rstd = K.bn_stats(xd, dev(gamma), dev(beta), rm, rv)
    check_stats(tag, (sc, sh, mean, rstd), r64, r32)
    check_running(tag, rm, rv, r64, r32)
    close_elem(tag + ' y', K.affine_act(xd, sc, sh, 'elu'), r64['y'], r32['y'])
    dg0, db0 = torch.randn(Cn, generator=gen(1)), torch.randn(Cn, generator=gen(2))
    dg, db = dev(dg0), dev(db0)
    dx = K.affine_act_bwd(dev(dh), xd, sc, sh, 'elu', True, mean, rstd, dg, db)
    close_elem(tag + ' dx', dx, r64['dx'], r32['dx'])
    close_sum(tag + ' dgamma', dg, dg0.double() + r64['dgamma'], dg0 + r32['dgamma'], r64['tg'])
    close_sum(tag + ' dbeta', db, db0.double() + r64['dbeta'], db0 + r32['dbeta'], r64['tb'])


def test_single_row_statistics(K):
    """M = 1, which torch refuses: the library's stated behaviour by hand. mean = x, variance 0 (rstd = 1 / sqrt(eps)), and the running
    variance moves toward the biased variance 0; nothing NaN"""
    g = gen(8)
    x = torch.randn(1, 1, 1, 8, generator=g) * 3
    gamma, beta, rm0, rv0 = _bn_params(g, 8)

    def hand(dt):
        xv, m = x.reshape(8).to(dt), 0.37
        rstd = torch.full((8,), EPS, dtype=dt).rsqrt()
        scale = gamma.to(dt) * rstd
        return dict(mean=xv, rstd=rstd, scale=scale, shift=beta.to(dt) - xv * scale, running_mean=(1 - m) * rm0.to(dt) + m * xv,
                    running_var=(1 - m) * rv0.to(dt))
    r64, r32 = hand(F64), hand(F32)
    finite(r64, r32)
    xd, rm, rv = dev(x), dev(rm0), dev(rv0)
    got = K.bn_stats(xd, dev(gamma), dev(beta), rm, rv, EPS, 0.37)
    check_stats('bn_stats M=1', got, r64, r32)
    check_running('bn_stats M=1', rm, rv, r64, r32)
    assert same_bits(got[2], x.reshape(8))
    y = K.affine_act(xd, got[0], got[1], 'elu')
    assert bool(torch.isfinite(y).all()) and all(bool(torch.isfinite(t).all()) for t in (*got, rm, rv))


# ---------------------------------------------------------------------------------------------------------------------------------
# C. bn_finalize_parts
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _finalize_case(Cn):
    g = gen(Cn)
    x = torch.randn(4, 103, 5, Cn, generator=g) * 1.5 + 2 * torch.randn(Cn, generator=g)           # M = 2060
    gamma, beta, _, rv0 = _bn_params(g, Cn)
    rm0 = x.reshape(-1, Cn)[:7].mean(0)                     # the pivot the producer used: the running mean, a value inside the data range
    refs = [ref_bn(dt, x, gamma, beta, rm=rm0, rv=rv0, momentum=0.37) for dt in (F64, F32)]
    finite(*refs)
    d = x.reshape(-1, Cn).double() - rm0.double()
    return torch.stack([d, d * d], 1), gamma, beta, rm0, rv0, refs


@pytest.mark.parametrize('Cn', [8, 100, 1024])
@pytest.mark.parametrize('rows', [1, 255, 256, 257, 1030])   # each side of one, and several, 256-row steps of the finalize loop
def test_bn_finalize_parts_rows_and_aliased_pivot(K, rows, Cn):
    v, gamma, beta, rm0, rv0, (r64, r32) = _finalize_case(Cn)
    parts = dev(chunk_sums(v, rows))
    tag = 'bn_finalize_parts rows=%d C=%d' % (rows, Cn)
    rm_a, rv_a = dev(rm0), dev(rv0)
    sep = K.bn_finalize_parts(parts, v.shape[0], dev(rm0), dev(gamma), dev(beta), rm_a, rv_a, EPS, 0.37)
    check_stats(tag, sep, r64, r32)
    check_running(tag, rm_a, rv_a, r64, r32)
    rm_b, rv_b = dev(rm0), dev(rv0)
    ali = K.bn_finalize_parts(parts, v.shape[0], rm_b, dev(gamma), dev(beta), rm_b, rv_b, EPS, 0.37)       # pivot IS running_mean
    for a, b in zip((*sep, rm_a, rv_a), (*ali, rm_b, rv_b)):
        assert same_bits(a, b), tag + ': the aliased pivot changed a result'
    check_running(tag + ' aliased', rm_b, rv_b, r64, r32)       # updated from the OLD running mean


# ---------------------------------------------------------------------------------------------------------------------------------
# D. bn_eval_coeffs
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('affine', [True, False])
@pytest.mark.parametrize('Cn', [1, 63, 64, 65, 1024])
def test_bn_eval_coeffs(K, Cn, affine):
    g = gen(Cn)
    gamma, beta, rm, rv = _bn_params(g, Cn)
    rv = rv * torch.rand(Cn, generator=g) ** 8               # down to ~0 ...
    rv[::3] = 0.0                                            # ... and exactly 0: rstd = 1 / sqrt(eps)
    if not affine:
        gamma = beta = None

    def ref(dt):
        rstd = 1 / torch.sqrt(rv.to(dt) + EPS)
        scale = rstd if gamma is None else gamma.to(dt) * rstd
        return scale, (0 if beta is None else beta.to(dt)) - rm.to(dt) * scale
    r64, r32 = ref(F64), ref(F32)
    finite(*r64, *r32)
    sc, sh = K.bn_eval_coeffs(dev(gamma), dev(beta), dev(rm), dev(rv), EPS)
    tag = 'bn_eval_coeffs C=%d%s' % (Cn, '' if affine else ' no gamma/beta')
    close_elem(tag + ' scale', sc, r64[0], r32[0])
    close_elem(tag + ' shift', sh, r64[1], r32[1])


# ---------------------------------------------------------------------------------------------------------------------------------
# E. affine_act
# ---------------------------------------------------------------------------------------------------------------------------------
E_SHAPES = [(3, 5, 7, 12),          # cols 3, rpp 85, an idle thread
            (5, 2, 2, 100),         # rpp 10 and 4 rows per sample: the rows of one block span three samples
            (2, 1, 1, 1024),        # rpp 1
            (3, 3, 3, 6)]           # scalar kernel
GRID_CAP_SHAPE = (3, 2731, 1, 1024)  # M = 8193 rows, rpp 1: past the 2048-block grid, a second sweep with one row left for block 0


def _affine_input(shape, with_scale, seed=0):
    """x with pre-activations x * scale + shift that include exact 0 and values within 1e-6 of 0 on both sides"""
    N, H, W, Cn = shape
    g = gen(sum(shape) + seed)
    x = torch.randn(shape, generator=g) * 1.5 + 0.3
    scale = shift = None
    if with_scale:
        scale = (torch.rand(Cn, generator=g) + 0.5) * (1 - 2 * (torch.rand(Cn, generator=g) < 0.25).float())
        shift = torch.randn(Cn, generator=g).clamp(-1.5, 1.5)
        shift[0] = 0.0
    xf = x.reshape(-1, Cn)
    xf[0, 0] = xf[-1, 0] = 0.0                                           # u = 0 exactly (shift[0] = 0)
    for r, c, u in ((0, 1, 5e-7), (0, 2, -5e-7), (xf.shape[0] - 1, Cn - 1, 5e-7), (xf.shape[0] - 1, Cn - 2, -5e-7)):
        xf[r, c] = u if scale is None else float((u - shift[c].double()) / scale[c].double())
    return x, scale, shift, g


def _affine_act_case(K, shape, act, with_scale, with_rs):
    N, Cn = shape[0], shape[-1]
    x, scale, shift, g = _affine_input(shape, with_scale)
    rs = keep_mask(g, N, Cn) if with_rs else None
    r64, r32 = [ref_affine(dt, x, scale, shift, act, rs) for dt in (F64, F32)]
    finite(r64, r32)
    u = r64['u']
    assert bool((u == 0).any()) and bool(((u > 0) & (u <= 1e-6)).any()) and bool(((u < 0) & (u >= -1e-6)).any())
    y = K.affine_act(dev(x), dev(scale), dev(shift), act, dev(rs))
    close_elem('affine_act %s %s%s%s y' % ('x'.join(map(str, shape)), act, ' scale+shift' if with_scale else ' identity',
                                           ' row_scale' if with_rs else ''), y, r64['y'], r32['y'])


@pytest.mark.parametrize('act', ACTS, ids=str)
@pytest.mark.parametrize('shape', E_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_affine_act(K, shape, act):
    for with_scale in (True, False):
        for with_rs in (False, True):
            _affine_act_case(K, shape, act, with_scale, with_rs)


def test_affine_act_past_the_grid_cap(K):
    _affine_act_case(K, GRID_CAP_SHAPE, 'elu', True, True)


# ---------------------------------------------------------------------------------------------------------------------------------
# F. affine_act_bwd
# ---------------------------------------------------------------------------------------------------------------------------------
DROP_ADD = [(False, False), (True, True), (True, False), (False, True)]


def _bwd_case(K, shape, act, combos, none_grads=True):
    N, Cn = shape[0], shape[-1]
    g = gen(sum(shape) + 7)
    x = torch.randn(shape, generator=g) * 1.5 + 0.3
    dh, add, drop = torch.randn(shape, generator=g), torch.randn(shape, generator=g), keep_mask(g, N, Cn)
    gamma, beta, _, _ = _bn_params(g, Cn)
    gamma = gamma * (1 - 2 * (torch.rand(Cn, generator=g) < 0.25).float())
    dg0, db0 = torch.randn(Cn, generator=g), torch.randn(Cn, generator=g)
    t64, t32 = [ref_bn(dt, x, gamma, beta, act, dh) for dt in (F64, F32)]
    sc, sh, mean, rstd = coef32(t64)                                # eval mode: the same pair as fixed coefficients; and the identity affine
    e64, e32 = [ref_affine(dt, x, sc, sh, act, None, dh) for dt in (F64, F32)]
    i64, i32 = [ref_affine(dt, x, None, None, act, None, dh) for dt in (F64, F32)]
    finite(t64, t32, e64, e32, i64, i32)
    xd, dhd, cd = dev(x), dev(dh), [dev(t) for t in (sc, sh, mean, rstd)]
    name = 'affine_act_bwd %s %s' % ('x'.join(map(str, shape)), act)
    for with_drop, with_add in combos:
        dr, ad = drop if with_drop else None, add if with_add else None
        tag = '%s%s%s' % (name, ' drop' if with_drop else '', ' add' if with_add else '')
        dg, db = dev(dg0), dev(db0)
        dx = K.affine_act_bwd(dhd, xd, cd[0], cd[1], act, True, cd[2], cd[3], dg, db, dev(dr), dev(ad))
        close_elem(tag + ' train dx', dx, fold(t64['dx'], dr, ad), fold(t32['dx'], dr, ad))
        close_sum(tag + ' train dgamma', dg, dg0.double() + t64['dgamma'], dg0 + t32['dgamma'], t64['tg'])    # start + gradient
        close_sum(tag + ' train dbeta', db, db0.double() + t64['dbeta'], db0 + t32['dbeta'], t64['tb'])
        for mode, r64, r32, co in (('eval', e64, e32, cd), ('eval identity', i64, i32, [None] * 4)):
            dg, db = dev(dg0), dev(db0)
            dx = K.affine_act_bwd(dhd, xd, co[0], co[1], act, False, None, None, dg, db, dev(dr), dev(ad))
            close_elem('%s %s dx' % (tag, mode), dx, fold(r64['dx'], dr, ad), fold(r32['dx'], dr, ad))
            assert same_bits(dg, dg0) and same_bits(db, db0), tag + ': eval mode touched dgamma / dbeta'
    if none_grads:
        dx = K.affine_act_bwd(dhd, xd, cd[0], cd[1], act, True, cd[2], cd[3], None, None, None, None)
        close_elem(name + ' train, dgamma = dbeta = None, dx', dx, t64['dx'], t32['dx'])


@pytest.mark.parametrize('act', ACTS, ids=str)
@pytest.mark.parametrize('shape', E_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_affine_act_bwd(K, shape, act):
    _bwd_case(K, shape, act, DROP_ADD)


@pytest.mark.parametrize('shape', [(4, 2, 1, 1024),      # M = 8 = 4 rows x 2 blocks (rpp 1): every row goes through the unrolled loop, stride 2
                                   (4, 8, 8, 64)],       # M = 256 = 4 x 4 blocks x rpp 16: stride 64 = the rows of one sample
                         ids=lambda s: 'x'.join(map(str, s)))
def test_affine_act_bwd_unrolled_rows_in_four_samples(K, shape):
    """the smallest shapes at which the four rows a thread takes per round trip of the apply loop lie in four different samples"""
    _bwd_case(K, shape, 'selu', [(True, True), (True, False)], none_grads=False)


def test_affine_act_bwd_past_the_grid_cap(K):
    """M = 8193, C = 1024: the reduce pass runs 911 chunks of 9 rows (past the chunk cap, ragged), the four rows of a thread of the unrolled
    apply loop lie 2048 rows apart, i.e. in different samples, and block 0 alone takes the last row"""
    _bwd_case(K, GRID_CAP_SHAPE, 'elu', [(True, True)], none_grads=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# G. affine_act_bwd_parts
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _parts_case(shape, act):
    N, Cn = shape[0], shape[-1]
    g = gen(sum(shape) + 11)
    x = torch.randn(shape, generator=g) * 1.5 + 0.3
    dh, add, drop = torch.randn(shape, generator=g), torch.randn(shape, generator=g), keep_mask(g, N, Cn)
    gamma, beta, _, _ = _bn_params(g, Cn)
    dg0, db0 = torch.randn(Cn, generator=g), torch.randn(Cn, generator=g)
    r64, r32 = [ref_bn(dt, x, gamma, beta, act, dh) for dt in (F64, F32)]
    finite(r64, r32)
    coef = coef32(r64)
    # (g, g * xhat) per pixel from the float32 coefficients the dgrad epilogue reads, in float64: what the partial rows are sums of
    u = leaf(x.reshape(-1, Cn).double() * coef[0].double() + coef[1].double(), F64)
    act_ref(u, act).backward(dh.reshape(-1, Cn).double())
    xh = (x.reshape(-1, Cn).double() - coef[2].double()) * coef[3].double()
    return dict(x=x, dh=dh, add=add, drop=drop, dg0=dg0, db0=db0, r64=r64, r32=r32, coef=coef, v=torch.stack([u.grad, u.grad * xh], 1))


def _parts_run(K, c, act, parts, drop=None, tag=None):
    dg, db = dev(c['dg0']), dev(c['db0'])
    cd = [dev(t) for t in c['coef']]
    dx = K.affine_act_bwd_parts(parts, dev(c['dh']), dev(c['x']), cd[0], cd[1], act, cd[2], cd[3], dg, db,
                                drop=dev(c['drop']) if drop is None else drop, add=dev(c['add']))
    if tag is not None:
        r64, r32 = c['r64'], c['r32']
        close_elem(tag + ' dx', dx, fold(r64['dx'], c['drop'], c['add']), fold(r32['dx'], c['drop'], c['add']))
        close_sum(tag + ' dgamma', dg, c['dg0'].double() + r64['dgamma'], c['dg0'] + r32['dgamma'], r64['tg'])
        close_sum(tag + ' dbeta', db, c['db0'].double() + r64['dbeta'], c['db0'] + r32['dbeta'], r64['tb'])
    return dx, dg, db


G_WIDTHS = [((3, 20, 20, 4), 'elu'),        # parts kernel, nsl = 256, two workgroups
            ((3, 20, 20, 8), 'selu'),       # parts kernel, nsl = 128
            ((5, 3, 3, 128), 'relu'),       # parts kernel, nsl = 8
            ((5, 3, 3, 256), 'elu'),        # parts kernel, nsl = 4: the widest it serves
            ((5, 3, 3, 12), 'selu'),        # 256 % 3 != 0: finalize launch + apply
            ((5, 3, 3, 100), 'relu'),       # 256 % 25 != 0: finalize launch + apply
            ((5, 3, 3, 6), 'elu'),          # finalize launch + scalar apply
            ((5, 3, 3, 512), 'selu'),       # 256 % 128 == 0 but C > 256: must NOT take the parts kernel
            ((3, 3, 3, 1024), 'relu')]      # 256 % 256 == 0 but C > 256


@pytest.mark.parametrize('rows', [3, 37])
@pytest.mark.parametrize('shape,act', G_WIDTHS, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_affine_act_bwd_parts_widths(K, shape, act, rows):
    c = _parts_case(shape, act)
    _parts_run(K, c, act, dev(chunk_sums(c['v'], rows)), tag='affine_act_bwd_parts %s %s rows=%d' % ('x'.join(map(str, shape)), act, rows))


@pytest.mark.parametrize('shape,rows', [((64, 16, 16, 64), 128),     # rows <= 128: parts kernel
                                        ((64, 16, 16, 64), 129),     # <= 256 rows and M <= 16384: parts kernel (few workgroups)
                                        ((64, 16, 16, 64), 256),
                                        ((64, 16, 16, 64), 257),     # finalize launch
                                        ((65, 16, 16, 64), 129)],    # M = 16640 > 16384: finalize launch
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_affine_act_bwd_parts_each_side_of_the_selection(K, shape, rows):
    c = _parts_case(shape, 'elu')
    _parts_run(K, c, 'elu', dev(chunk_sums(c['v'], rows)), tag='affine_act_bwd_parts %s elu rows=%d' % ('x'.join(map(str, shape)), rows))


@pytest.mark.parametrize('act', ['elu', 'selu', 'relu'])
def test_affine_act_bwd_parts_misaligned_fall_back_and_agree(K, act):
    """misaligned partial rows, or a misaligned mask, send the launch to finalize + apply: the same inputs through both paths"""
    shape = (7, 4, 4, 64)
    c = _parts_case(shape, act)
    parts = chunk_sums(c['v'], 40)
    tag = 'affine_act_bwd_parts 7x4x4x64 %s rows=40' % act
    _, dg_k, db_k = _parts_run(K, c, act, dev(parts), tag=tag + ' parts kernel')
    _, dg_f, db_f = _parts_run(K, c, act, misaligned(parts), tag=tag + ' misaligned parts')
    _parts_run(K, c, act, dev(parts), drop=misaligned(c['drop']), tag=tag + ' misaligned drop')
    # the two paths against each other, under the rule of the sums (the parts kernel's result in the place of r64)
    r64, r32 = c['r64'], c['r32']
    close_sum(tag + ' finalize vs parts kernel dgamma', dg_f, dg_k.double().cpu(), dg_k.double().cpu() + (r32['dgamma'].double() - r64['dgamma']), r64['tg'])
    close_sum(tag + ' finalize vs parts kernel dbeta', db_f, db_k.double().cpu(), db_k.double().cpu() + (r32['dbeta'].double() - r64['dbeta']), r64['tb'])
