"""The epilogue of the 256-pixel six-product Winograd kernel (conv3x3_wino2_kernel, csrc/conv3x3_wino.hip) at the smallest shapes that
reach it (64 -> 64 channels, at least 256 workgroups of 256 pixels), through lvae_conv2d_f32 and lvae_resblock_conv_f32 / LVAE_RB_EPI_GATE.
Everything the epilogue reads from memory is requested ahead of its first store, rows that are not wanted from a dummy address, and the
stores are predicated: so every output and every row of partial sums starts from NaNs and has NaN guard rows behind it that must still
be NaNs afterwards, and every optional operand is exercised present and absent.

Shapes: N = 256 and 257 at 16x16 (one image per workgroup; 257: a ragged batch), N = 64 and 65 at 32x32 (four workgroups per image).
The workgroup count comes from lvae_conv2d_stats_rows / lvae_resblock_conv_gate_rows and the variant from lvae_conv2d_variant.
N = 1021 at 8x8 (four images per workgroup, 256 workgroups, the second block of the last one without a valid row) is not among them:
the router answers 511 workgroups for it, the 128-pixel kernel's count, so an 8x8 shape does not reach this kernel.

Bounds, all against float64 and none of them new: 4e-6 norm-relative for the convolution, its dgrad and y2 / ab / out of the gate
(tests/test_kernels_gpu.py::test_conv3x3_winograd, tests/test_resblock_img_gpu.py::test_conv_gate_fusion_behind_the_winograd_kernel);
rtol 1e-4, atol 2e-2 for the BatchNorm partial sums of the stored values (the same gate test); 1e-5 norm-relative for the
BatchNorm-backward sums (sum g and sum g * xhat are dbeta and dgamma, which tests/test_kernels_gpu.py holds to 1e-5 when they are formed from
these rows)."""
import ctypes
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
C = 64
NAN = float('nan')
GUARD = 64   # rows behind every output
SHAPES = [(256, 16, 16), (257, 16, 16), (64, 32, 32), (65, 32, 32)]


@pytest.fixture(scope='module')
def K():
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels
    return kernels


def packed_weight(w):
    """the arena layout: physical [KH][KW][Cin][Cout], logical torch shape"""
    return w.float().permute(2, 3, 1, 0).contiguous().cuda().permute(3, 2, 0, 1)


def nhwc(t):
    return t.detach().float().permute(0, 2, 3, 1).contiguous().cuda()


def nchw(t):
    return t.permute(0, 3, 1, 2).cpu()


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def workgroups(N, H, W):
    per_img = H * W
    return N * (per_img // 256) if per_img >= 256 else -(-N // (256 // per_img))


class Guarded:
    """rows x width floats, NaN-filled, with GUARD rows of NaNs behind them"""

    def __init__(self, shape):
        width = shape[-1]
        rows = 1
        for s in shape[:-1]:
            rows *= s
        self.buf = torch.full(((rows + GUARD) * width,), NAN, device='cuda')
        self.t = self.buf[:rows * width].view(*shape)
        self.guard = self.buf[rows * width:]

    def check(self, what, rows=None):
        """rows: only the first `rows` rows have to be written (a pivot row behind the partial sums holds the pivot alone)"""
        assert bool(torch.isnan(self.guard).all()), what + ': guard rows written'
        assert bool(torch.isfinite(self.t if rows is None else self.t[:rows]).all()), what + ': not every element written'
        return self.t


_REF = {}


def operands(K, shape):
    """Operands and float64 references of one shape, made once: x through a training-mode BatchNorm + ELU into a 3x3 convolution (without
    bias; the cases add bias, mask and activation), the dgrad of dy, and what the gate and the statistics cases read."""
    if shape in _REF:
        return _REF[shape]
    N, H, W = shape
    g = torch.Generator().manual_seed(N + 3 * H)
    rn = lambda *s: torch.randn(*s, generator=g)
    p = types.SimpleNamespace(shape=shape)
    p.x = rn(N, C, H, W) * 1.5 + 0.3
    p.w = rn(C, C, 3, 3) / 24
    p.gamma, p.beta = torch.rand(C, generator=g) + 0.5, rn(C) * 0.3
    p.bias = rn(C)
    p.mask = (torch.rand(N, C, generator=g) < 0.8).float() / 0.8
    p.dy = rn(N, C, H, W)
    p.wg, p.bg = rn(2 * C, C, 1, 1) / 8, rn(2 * C) * 0.5
    p.res = rn(N, C, H, W)
    p.xb = rn(N, C, H, W) * 2 + 1   # the BatchNorm input of the dgrad's BatchNorm-backward sums
    p.gb, p.bb = torch.rand(C, generator=g) + 0.5, rn(C)
    p.pivot = rn(C) * 0.1
    xd = p.x.double()
    mean, var = xd.mean((0, 2, 3)), xd.var((0, 2, 3), unbiased=False)
    scale = p.gamma.double() / torch.sqrt(var + 1e-5)
    shift = p.beta.double() - mean * scale
    p.conv = F.conv2d(F.elu(xd * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)), p.w.double(), padding=1)
    p.dx = F.conv_transpose2d(p.dy.double(), p.w.double(), padding=1)
    # device side
    p.xd, p.dyd, p.resd, p.xbd = nhwc(p.x), nhwc(p.dy), nhwc(p.res), nhwc(p.xb)
    p.wp, p.wgp = packed_weight(p.w), packed_weight(p.wg)
    p.geom, p.geg = K.ConvGeom(p.wp, 1, 1), K.ConvGeom(p.wgp, 1, 0)
    p.coef = K.bn_stats(p.xd, p.gamma.cuda(), p.beta.cuda(), None, None)
    p.coefb = K.bn_stats(p.xbd, p.gb.cuda(), p.bb.cuda(), None, None)
    assert K.bn_coef_block(*p.coefb)
    # the partial sums a producer's epilogue would have left for x: 5 chunks of pixels around a pivot, the pivot in the row behind them
    piv_in = (mean + 0.05).float()
    flat = p.xd.double().reshape(-1, C).cpu() - piv_in.double()
    rows = [torch.stack([c.sum(0), (c * c).sum(0)]) for c in flat.tensor_split(5)]
    rows.append(torch.stack([piv_in.double(), torch.zeros(C, dtype=torch.float64)]))
    p.in_parts = torch.stack(rows).float().cuda().contiguous()
    p.piv_in = piv_in.cuda()
    _REF[shape] = p
    return p


def in_bn_of(K, p):
    bn = types.SimpleNamespace(weight=p.gamma.cuda(), bias=p.beta.cuda(), running_mean=torch.zeros(C, device='cuda'),
                               running_var=torch.ones(C, device='cuda'), eps=1e-5, momentum=0.1)
    return (K.StatParts(p.in_parts, 5, True), p.piv_in, bn)


def check_route(K, d, shape, rows):
    assert K._C.load().lvae_conv2d_variant(ctypes.byref(d)) == K._C.VARIANT_WINO_SIX, shape
    assert rows == workgroups(*shape) and rows >= 256, (shape, rows)


CONV_CASES = {
    # name: (dgrad, bias, mask, out_act, folded input BatchNorm, statistics)
    'fwd-bias-mask-elu-stats': (False, True, True, 'elu', False, 'fwd'),
    'fwd-plain': (False, False, False, None, False, None),
    'fwd-folded-bn-bias': (False, True, False, None, True, None),
    'fwd-folded-bn-mask-stats': (False, False, True, 'elu', True, 'fwd'),
    'dgrad-mask': (True, False, True, None, False, None),
    'dgrad-plain': (True, False, False, None, False, None),
    'dgrad-bn-bwd-sums': (True, False, False, None, False, 'bwd'),
}


@pytest.mark.parametrize('case', list(CONV_CASES))
@pytest.mark.parametrize('shape', SHAPES)
def test_conv2d_through_the_256_pixel_kernel(K, shape, case):
    """lvae_conv2d_f32, forward and dgrad view: bias, Dropout2d mask and activation on and off, given and folded input BatchNorm,
    no statistics, LVAE_STATS_BN_FWD, and LVAE_STATS_BN_BWD with stats_x."""
    dgrad, use_bias, use_mask, out_act, folded, stats = CONV_CASES[case]
    N, H, W = shape
    p = operands(K, shape)
    lib = K._C.load()
    y = Guarded((N, H, W, C))
    bias = p.bias.cuda() if use_bias else None
    mask = p.mask.cuda() if use_mask else None
    if dgrad:
        d = K._desc(p.geom, p.wp, p.dyd, None, N, H, W, H, W, C, p.geom.s_co, p.geom.s_ci, K.GATHER_TRANSPOSED, out_scale=mask, y=y.t)
    else:
        sc, sh = (None, None) if folded else (p.coef[0], p.coef[1])
        d = K._desc(p.geom, p.wp, p.xd, None, N, H, W, H, W, C, p.geom.s_ci, p.geom.s_co, K.GATHER_CONV, bias, sc, sh, 'elu', mask, out_act, y.t)
    K._conv_ws(d, p.wp, p.xd.device)
    rows = lib.lvae_conv2d_stats_rows(ctypes.byref(d))
    check_route(K, d, shape, rows)
    keep = None
    if folded:
        assert lib.lvae_conv2d_folds_bn_finalize(ctypes.byref(d))
        in_bn = in_bn_of(K, p)   # (holds gamma, beta and the running statistics: alive until the launch has run)
        coef, keep = K._in_bn(d, in_bn, p.xd, True)
        assert keep is not None, 'the finalize is meant to run inside the convolution'
    parts = None
    if stats == 'fwd':
        buf_rows = lib.lvae_conv2d_stats_buffer_rows(ctypes.byref(d))
        parts = Guarded((buf_rows, 2, C))
        pivot = p.pivot.cuda()
        d.stats_out, d.stats_pivot = K.ptr(parts.t), K.ptr(pivot)
    elif stats == 'bwd':
        parts = Guarded((rows, 2, C))
        d.stats_out, d.stats_pivot, d.stats_x = K.ptr(parts.t), K.ptr(p.coefb[0]), K.ptr_dt(p.xbd)
        d.stats_mode, d.stats_act, d.stats_x_dtype = 1, K.ACT['elu'], K._dt(p.xbd)
    K.call('lvae_conv2d_f32', ctypes.byref(d), K.stream_ptr())
    torch.cuda.synchronize()
    del keep
    got = nchw(y.check(case))
    if dgrad:
        ref = p.dx * p.mask.view(N, C, 1, 1).double() if use_mask else p.dx
    else:
        ref = p.conv
        if use_bias:
            ref = ref + p.bias.double().view(1, -1, 1, 1)
        if use_mask:
            ref = ref * p.mask.view(N, C, 1, 1).double()
        if out_act:
            ref = F.elu(ref)
    err = rel(got, ref)
    print('%s %s: %d workgroups, y %.3g' % (shape, case, rows, err))
    assert err < 4e-6
    if folded:
        xd = p.x.double()
        torch.testing.assert_close(coef[2].cpu().double(), xd.mean((0, 2, 3)), rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(coef[3].cpu().double(), 1 / torch.sqrt(xd.var((0, 2, 3), unbiased=False) + 1e-5), rtol=1e-5, atol=1e-5)
    if stats == 'fwd':
        pt = parts.check(case + ' partial sums', rows)
        s = pt[:rows].double().sum(0).cpu()
        dl = ref - p.pivot.double().view(1, -1, 1, 1)
        torch.testing.assert_close(s[0], dl.sum((0, 2, 3)), rtol=1e-4, atol=2e-2)
        torch.testing.assert_close(s[1], (dl * dl).sum((0, 2, 3)), rtol=1e-4, atol=2e-2)
        if pt.shape[0] > rows:
            assert torch.equal(pt[rows, 0], p.pivot.cuda())
    elif stats == 'bwd':
        s = parts.check(case + ' partial sums').double().sum(0).cpu()
        cf = [c.cpu().double().view(1, -1, 1, 1) for c in p.coefb]
        u = p.xb.double() * cf[0] + cf[1]
        gr = ref * torch.where(u > 0, torch.ones_like(u), torch.exp(u))
        xh = (p.xb.double() - cf[2]) * cf[3]
        e1, e2 = rel(s[0], gr.sum((0, 2, 3))), rel(s[1], (gr * xh).sum((0, 2, 3)))
        print('   sums %.3g %.3g' % (e1, e2))
        assert e1 < 1e-5 and e2 < 1e-5


GATE_CASES = {
    # name: (residual, ab stored, statistics of out, folded input BatchNorm)
    'res-ab-stats': (True, True, True, False),
    'res-stats': (True, False, True, True),
    'ab': (False, True, False, False),
    'bare-folded-bn': (False, False, False, True),
}


@pytest.mark.parametrize('case', list(GATE_CASES))
@pytest.mark.parametrize('shape', SHAPES)
def test_conv_gate_through_the_256_pixel_kernel(K, shape, case):
    """lvae_resblock_conv_f32 with LVAE_RB_EPI_GATE: y2 = (conv3x3(elu(BN(x))) + bias) * mask, ab = conv1x1(y2) + gate bias,
    out = elu(a) * sigmoid(b) [+ res], the BatchNorm partial sums of out; with and without the residual, the stored ab and the sums."""
    use_res, use_ab, use_stats, folded = GATE_CASES[case]
    N, H, W = shape
    p = operands(K, shape)
    lib = K._C.load()
    dev = p.xd.device
    y2, out = Guarded((N, H, W, C)), Guarded((N, H, W, C))
    ab = Guarded((N, H, W, 2 * C)) if use_ab else None
    bias, mask = p.bias.cuda(), p.mask.cuda()   # (the descriptor holds raw pointers: alive until the launch has run)
    d, need = K._rb_desc(p.xd, p.wp, p.geom, False, y2.t, bias, None, None, 'elu', mask)
    assert not need, 'not a whole-image shape'
    K._conv_ws(d, p.wp, dev)
    rows = lib.lvae_resblock_conv_gate_rows(ctypes.byref(d))
    check_route(K, d, shape, rows)
    if folded:
        assert lib.lvae_conv2d_folds_bn_finalize(ctypes.byref(d))
        in_bn = in_bn_of(K, p)   # (holds gamma, beta and the running statistics: alive until the launch has run)
        coef, keep = K._in_bn(d, in_bn, p.xd, True)
        assert keep is not None
    else:
        coef, keep = K._in_bn(d, None, p.xd, True, p.coef)
    e = K.RbExt()
    e.prologue, e.epilogue = K._C.RB_PRO_AFFINE, K._C.RB_EPI_GATE
    K._rb_gate_ws(e, p.wgp, p.geg, dev, False)
    bg = p.bg.cuda()
    e.gate_bias, e.act = K.ptr(bg), K.ACT['elu']
    e.res, e.ab, e.out = K.ptr(p.resd if use_res else None), K.ptr(ab.t if use_ab else None), K.ptr(out.t)
    parts = None
    if use_stats:
        parts = Guarded((rows + 1, 2, C))
        pivot = p.pivot.cuda()
        e.out_stats, e.out_stats_pivot = K.ptr(parts.t), K.ptr(pivot)
    K.call('lvae_resblock_conv_f32', ctypes.byref(d), ctypes.byref(e), K.stream_ptr())
    torch.cuda.synchronize()
    del keep
    r_y2 = (p.conv + p.bias.double().view(1, -1, 1, 1)) * p.mask.view(N, C, 1, 1).double()
    r_ab = F.conv2d(r_y2, p.wg.double(), p.bg.double())
    a_, b_ = r_ab.chunk(2, 1)
    r_out = F.elu(a_) * torch.sigmoid(b_) + (p.res.double() if use_res else 0)
    e_y2, e_out = rel(nchw(y2.check(case + ' y2')), r_y2), rel(nchw(out.check(case + ' out')), r_out)
    print('%s gate %s: %d workgroups, y2 %.3g out %.3g' % (shape, case, rows, e_y2, e_out))
    assert e_y2 < 4e-6
    assert e_out < 4e-6
    if use_ab:
        e_ab = rel(nchw(ab.check(case + ' ab')), r_ab)
        print('   ab %.3g' % e_ab)
        assert e_ab < 4e-6
    if use_stats:
        pt = parts.check(case + ' partial sums', rows)
        s = pt[:rows].double().sum(0).cpu()
        dl = r_out - p.pivot.double().view(1, -1, 1, 1)
        torch.testing.assert_close(s[0], dl.sum((0, 2, 3)), rtol=1e-4, atol=2e-2)
        torch.testing.assert_close(s[1], (dl * dl).sum((0, 2, 3)), rtol=1e-4, atol=2e-2)
        assert torch.equal(pt[rows, 0], p.pivot.cuda())
