"""The activation ids of the fused 64-channel kernels (in_act, out_act, stats_act, the gate's act, lvae_bn_apply.act) with relu, leakyrelu
and selu, against float64 (tests/act_ref.py). The rest of the suite runs these kernels almost only with ELU, where every slot holds the
same id, the `ELU = false` instantiations of the persistent gate backward are never launched and the generic loop of act_fwd4 / act_fwd16 /
act_grad4 is never reached.

Every case gives the slots of its entry point different ids, so that a swapped or ignored id shows. No bound is new: each comparison
uses the metric and bound of the ELU test of the same kernel and output, named in a comment next to it. Shapes are the smallest of those
tests that the router sends to the kernel, and the route is asserted through the host-only queries.

Backward cases follow the kink rule of tests/act_ref.py: a derivative at a pre-activation tensor the kernel is handed (the saved ab) is
differentiated by the reference at those same fp32 numbers; x * scale + shift with handed coefficients is moved off the kink beforehand
(rule 3); a pre-activation the kernel reduces itself has its upstream gradient zeroed within the margin (rule 4). The caps of every such
input are asserted on the CPU (tests/test_act_ref_cpu.py, the same builders with the same arguments).

Out of scope: the backward of the fused small-level block at precision bf16. Its pre-activations are internal to a chain of launches and
formed from bf16 products (about 1 % relative error each), so hundreds of elements per tensor land on the other side of the kink than in
any reference; that build is held on its forward values only."""
import ctypes
import functools
import math
import os
import types

import pytest
import torch
import torch.nn.functional as F

import act_ref as R

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, os.cpu_count() or 1))
C = 64
NAN = float('nan')


@pytest.fixture(scope='module')
def K():
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels
    return kernels


def nhwc(t):
    return t.detach().float().permute(0, 2, 3, 1).contiguous().cuda()


def nchw(t):
    return t.float().permute(0, 3, 1, 2).cpu().double()


def to_nchw(t):
    """channel-last CPU tensor -> float64 NCHW"""
    return t.double().permute(0, 3, 1, 2)


def packed_weight(w, transposed=False):
    """the arena layout: physical [KH][KW][Cin][Cout], logical torch shape"""
    if transposed:  # (Cin,Cout,KH,KW)
        return w.float().permute(2, 3, 0, 1).contiguous().cuda().permute(2, 3, 0, 1)
    return w.float().permute(2, 3, 1, 0).contiguous().cuda().permute(3, 2, 0, 1)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def chan(v):
    return v.double().view(1, -1, 1, 1)


def bf(t):
    return t.float().bfloat16().double()


class precision:
    def __init__(self, K, prec):
        self.K, self.prec = K, prec

    def __enter__(self):
        self.K.set_precision(self.prec)

    def __exit__(self, *exc):
        self.K.set_precision('f32')


def form_of(K, name):
    return {None: K._C.FORM_AUTO, 'mfma_f32': K._C.FORM_F32_MFMA, 'split': K._C.FORM_SIX_PRODUCT, 'six_direct': K._C.FORM_SIX_PRODUCT_DIRECT}[name]


def route(K, geom, wp, x, out_hw, cout, dgrad=False, x2=None):
    """(lvae_conv2d_variant, lvae_conv2d_position_major, lvae_conv2d_stats_rows) of the forward or dgrad launch of (wp, geom) on x"""
    N, H, W, _ = x.shape
    if dgrad:
        d = K._desc(geom, wp, x, None, N, H, W, out_hw[0], out_hw[1], cout, geom.s_co, geom.s_ci, K.GATHER_CONV if geom.transposed else K.GATHER_TRANSPOSED)
    else:
        d = K._desc(geom, wp, x, x2, N, H, W, out_hw[0], out_hw[1], cout, geom.s_ci, geom.s_co, K.GATHER_TRANSPOSED if geom.transposed else K.GATHER_CONV)
    K._conv_ws(d, wp, x.device)
    lib = K._C.load()
    return lib.lvae_conv2d_variant(ctypes.byref(d)), lib.lvae_conv2d_position_major(ctypes.byref(d)), lib.lvae_conv2d_stats_rows(ctypes.byref(d))


# =================================================================================================================================
# 1. Convolution forward, prologue and epilogue: y = out_act((conv(in_act(x * in_scale + in_shift)) + bias) * out_scale)

# name: ((N, Cin, Cout, H, W), k, mode, precision, form, weight layout, in_act, out_acts, (variant, position_major), bound)
# in_act None: in_scale / in_shift present without an activation. Bounds, norm-relative against float64:
#   2e-6  test_kernels_gpu.py::test_conv_fwd_dgrad_wgrad, ::test_conv_fused_prologue_epilogue_and_cat (generic, halo, 1x1, concat),
#         ::test_conv3x3_position_major_small_images, test_conv_resample_gpu.py::test_fused_prologue_and_epilogue
#   4e-6  test_kernels_gpu.py::test_conv3x3_winograd (all three forms), test_wino2_epilogue_gpu.py::test_conv2d_through_the_256_pixel_kernel
#   2e-4  test_kernels_gpu.py::test_conv3x3_bf16_operands, against float64 sums over operands rounded to bf16 beforehand
FWD_CASES = {
    'igemm':        ((2, 16, 6, 16, 16), 3, 'conv', 'f32', None, 'packed', 'relu', ('selu', 'leakyrelu'), ('DIRECT', 0), 2e-6),
    'igemm-contig': ((2, 16, 6, 16, 16), 3, 'conv', 'f32', None, 'contig', 'selu', ('leakyrelu', None), ('DIRECT', 0), 2e-6),
    'halo':         ((3, 64, 64, 8, 8), 3, 'conv', 'f32', None, 'packed', 'leakyrelu', (None, 'relu'), ('DIRECT', 0), 2e-6),
    'pos':          ((37, 64, 64, 4, 4), 3, 'conv', 'f32', None, 'packed', None, ('relu', 'selu'), ('POS', 1), 2e-6),
    '1x1':          ((3, 64, 128, 8, 8), 1, 'conv', 'f32', None, 'packed', 'relu', ('leakyrelu', 'selu'), ('DIRECT', 0), 2e-6),
    'stride2':      ((3, 64, 64, 4, 4), 3, 'stride2', 'f32', None, 'packed', 'selu', ('relu', 'leakyrelu'), ('DIRECT', 1), 2e-6),
    'transposed':   ((3, 64, 64, 4, 4), 3, 'transposed', 'f32', None, 'packed', 'leakyrelu', ('selu', 'relu'), ('DIRECT', 1), 2e-6),
    'wino-f32':     ((64, 64, 64, 16, 16), 3, 'conv', 'f32', None, 'packed', 'relu', ('selu', None), ('WINO_F32', 0), 4e-6),
    'wino-six':     ((200, 64, 64, 16, 16), 3, 'conv', 'f32', None, 'packed', 'selu', ('leakyrelu', 'relu'), ('WINO_SIX', 0), 4e-6),
    'wino-256':     ((256, 64, 64, 16, 16), 3, 'conv', 'f32', None, 'packed', 'leakyrelu', ('relu', 'selu'), ('WINO_SIX', 0), 4e-6),
    'six-direct':   ((64, 64, 64, 16, 16), 3, 'conv', 'f32', 'six_direct', 'packed', None, ('leakyrelu', 'selu'), ('SIX_DIRECT', 0), 4e-6),
    'bf16-direct':  ((200, 64, 64, 16, 16), 3, 'conv', 'bf16', None, 'packed', 'relu', ('selu', 'leakyrelu'), ('BF16_DIRECT', 0), 2e-4),
    'concat':       ((6, 128, 64, 8, 8), 3, 'conv', 'f32', None, 'packed', 'selu', ('relu', None), ('DIRECT', 0), 2e-6),
}


@functools.lru_cache(maxsize=None)
def fwd_problem(name):
    """operands of one case and its float64 pre-activation (conv + bias) * mask, computed once and shared by the case's out_acts"""
    (N, Ci, Co, H, W), k, mode, prec, _, _, in_act, _, _, _ = FWD_CASES[name]
    g = torch.Generator().manual_seed(sum((N, Ci, Co, H, W)) + len(name))
    x = torch.randn(N, Ci, H, W, generator=g)                                   # both signs, about half the mass negative
    sc, sh = torch.rand(Ci, generator=g) + 0.5, torch.randn(Ci, generator=g) * 0.3
    wshape = (Ci, Co, k, k) if mode == 'transposed' else (Co, Ci, k, k)
    w = torch.randn(*wshape, generator=g) / math.sqrt(Ci * k * k)
    b = torch.randn(Co, generator=g)
    drop = (torch.rand(N, Co, generator=g) < 0.8).float() / 0.8
    xin = R.act(x.double() * chan(sc) + chan(sh), in_act)
    rnd = bf if prec == 'bf16' else (lambda t: t.double())
    if mode == 'transposed':
        pre = F.conv_transpose2d(rnd(xin), rnd(w), b.double(), stride=2, padding=1, output_padding=1)
    else:
        pre = F.conv2d(rnd(xin), rnd(w), b.double(), stride=2 if mode == 'stride2' else 1, padding=k // 2)
    pre = pre * drop.double().view(N, Co, 1, 1)
    return types.SimpleNamespace(x=x, sc=sc, sh=sh, w=w, b=b, drop=drop, pre=pre)


@pytest.mark.parametrize('name', list(FWD_CASES))
def test_conv_forward_prologue_and_epilogue(K, name):
    (N, Ci, Co, H, W), k, mode, prec, form, layout, in_act, out_acts, (variant, pm), bound = FWD_CASES[name]
    p = fwd_problem(name)
    transposed = mode == 'transposed'
    wp = p.w.cuda().contiguous() if layout == 'contig' else packed_weight(p.w, transposed)
    geom = K.ConvGeom(wp, stride=1 if mode == 'conv' else 2, pad=k // 2, transposed=transposed, output_padding=1 if transposed else 0)
    xd = nhwc(p.x)
    x1, x2 = (xd[..., :C].contiguous(), xd[..., C:].contiguous()) if name == 'concat' else (xd, None)
    with precision(K, prec), K.use_form(form_of(K, form)):
        got_route = route(K, geom, wp, x1, tuple(p.pre.shape[2:]), Co, x2=x2)
        assert got_route[:2] == (getattr(K._C, 'VARIANT_' + variant), pm), (name, got_route)
        if name == 'wino-256':
            assert got_route[2] == N   # one workgroup of 256 pixels per image: the 256-pixel kernel (at least 256 of them)
        elif name == 'wino-six':
            assert got_route[2] == 2 * N   # two workgroups of 128 pixels per image: the 128-pixel kernel
        for out_act in out_acts:
            y = K.conv2d(x1, wp, geom, bias=p.b.cuda(), x2=x2, in_scale=p.sc.cuda(), in_shift=p.sh.cuda(), in_act=in_act, out_scale=p.drop.cuda(),
                         out_act=out_act)
            torch.cuda.synchronize()
            err = rel(nchw(y), R.act(p.pre, out_act))
            print('forward %s in_act %s out_act %s: %.3g (bound %.0e)' % (name, in_act, out_act, err, bound))
            assert err < bound, (name, in_act, out_act, err)


# =================================================================================================================================
# 2. Weight gradients with the fused prologue: dW of conv(in_act(x * in_scale + in_shift)), accumulated into non-zero buffers.
# The prologue is a forward value (continuous), so nothing is left out.

# name: ((N, Cin, Cout, H, W), precision, in_act, lvae_conv2d_wgrad_variant, bound of dW). Bounds, norm-relative against float64:
#   3e-6  test_kernels_gpu.py::test_conv_fwd_dgrad_wgrad (generic, tile), ::test_conv_wgrad_whole_image_tiles (fp32)
#   5e-6  test_kernels_gpu.py::test_conv3x3_winograd (Winograd-domain kernel)
#   3e-4  test_kernels_gpu.py::test_conv_wgrad_whole_image_tiles (bf16), ::test_conv3x3_wgrad_bf16_operands: operands rounded beforehand
# and the bias gradient to 3e-6 (5e-6 behind the Winograd kernel, 1e-5 behind the bf16 one), as the same tests hold it.
WGRAD_CASES = {
    'generic':    ((2, 16, 6, 16, 16), 'f32', 'relu', 'GENERIC', 3e-6, 3e-6),
    'tile':       ((4, 64, 64, 16, 16), 'f32', 'selu', 'TILE', 3e-6, 3e-6),
    'wino':       ((64, 64, 64, 16, 16), 'f32', 'leakyrelu', 'WINO', 5e-6, 5e-6),
    'wino-none':  ((64, 64, 64, 16, 16), 'f32', None, 'WINO', 5e-6, 5e-6),
    'img-f32':    ((37, 64, 64, 4, 4), 'f32', 'relu', 'IMG', 3e-6, 3e-6),
    'img-bf16':   ((37, 64, 64, 4, 4), 'bf16', 'selu', 'IMG', 3e-4, 3e-6),
    'bf16':       ((70, 32, 64, 16, 16), 'bf16', 'leakyrelu', 'BF16', 3e-4, 1e-5),
}


@pytest.mark.parametrize('name', list(WGRAD_CASES))
def test_weight_gradient_with_fused_prologue(K, name):
    (N, Ci, Co, H, W), prec, in_act, variant, bound, bound_b = WGRAD_CASES[name]
    g = torch.Generator().manual_seed(sum((N, Ci, Co, H, W)) + len(name))
    x = torch.randn(N, Ci, H, W, generator=g)
    dy = torch.randn(N, Co, H, W, generator=g)
    sc, sh = torch.rand(Ci, generator=g) + 0.5, torch.randn(Ci, generator=g) * 0.3
    w = torch.randn(Co, Ci, 3, 3, generator=g) / math.sqrt(9 * Ci)
    rnd = bf if prec == 'bf16' else (lambda t: t.double())
    xin = R.act(x.double() * chan(sc) + chan(sh), in_act)
    want = torch.nn.grad.conv2d_weight(rnd(xin), (Co, Ci, 3, 3), rnd(dy), padding=1)
    dw0, db0 = torch.randn(Co, Ci, 3, 3, generator=g) * 0.1, torch.randn(Co, generator=g)
    wp, dw, db = packed_weight(w), packed_weight(dw0), db0.cuda()
    geom = K.ConvGeom(wp, 1, 1)
    xd, dyd = nhwc(x), nhwc(dy)
    with precision(K, prec):
        d = K._desc(geom, wp, xd, None, N, H, W, H, W, Co, geom.s_ci, geom.s_co, K.GATHER_CONV, None, sc.cuda(), sh.cuda(), in_act)
        assert K._C.load().lvae_conv2d_wgrad_variant(ctypes.byref(d)) == getattr(K._C, 'WGRAD_VARIANT_' + variant)
        K.conv2d_wgrad(xd, dyd, wp, geom, dw, db, in_scale=sc.cuda(), in_shift=sh.cuda(), in_act=in_act)
        torch.cuda.synchronize()
    e_w, e_b = rel(dw.cpu() - dw0, want), rel(db.cpu() - db0, dy.double().sum((0, 2, 3)))
    print('wgrad %s in_act %s: dW %.3g (bound %.0e) db %.3g (bound %.0e)' % (name, in_act, e_w, bound, e_b, bound_b))
    assert e_w < bound and e_b < bound_b


def test_weight_gradient_of_a_channel_concat_with_fused_prologue(K):
    """the case of test_kernels_gpu.py::test_conv_fused_prologue_epilogue_and_cat (second source x2), dW to its 3e-6"""
    N, H, W = 6, 8, 8
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, 2 * C, H, W, generator=g)
    sc, sh = torch.rand(2 * C, generator=g) + 0.5, torch.randn(2 * C, generator=g)
    w = torch.randn(C, 2 * C, 3, 3, generator=g) / 30
    dy = torch.randn(N, C, H, W, generator=g)
    want = torch.nn.grad.conv2d_weight(R.act(x.double() * chan(sc) + chan(sh), 'leakyrelu'), (C, 2 * C, 3, 3), dy.double(), padding=1)
    dw0 = torch.randn(C, 2 * C, 3, 3, generator=g) * 0.1
    wp, dw = packed_weight(w), packed_weight(dw0)
    xd = nhwc(x)
    K.conv2d_wgrad(xd[..., :C].contiguous(), nhwc(dy), wp, K.ConvGeom(wp, 1, 1), dw, None, x2=xd[..., C:].contiguous(), in_scale=sc.cuda(),
                   in_shift=sh.cuda(), in_act='leakyrelu')
    torch.cuda.synchronize()
    err = rel(dw.cpu() - dw0, want)
    print('wgrad concat in_act leakyrelu: dW %.3g (bound 3e-06)' % err)
    assert err < 3e-6


def dev_apply(K, p, with_add=True, out=None, dh=None):
    """kernels.PendingApply of an act_ref.apply_input on the device, with zeroed dgamma / dbeta and a NaN-filled out"""
    coef = p['coef'].cuda()
    assert K.bn_coef_block(coef[0], coef[1], coef[2], coef[3])
    x = p['x'].cuda()
    out = torch.full_like(x, NAN) if out is None else out
    cls = type('Pending', (K.PendingApply,), {})   # (a subclass has a __dict__: the whole coefficient block travels along as .coef)
    pend = cls(p['parts'].cuda(), p['dh'].cuda() if dh is None else dh, x, coef[0], p['act'], torch.zeros(C, device='cuda'),
               torch.zeros(C, device='cuda'), p['add'].cuda() if with_add else None, out)
    pend.coef = coef
    return pend


def check_apply_sums(pend, p, who):
    """dbeta = sum g, dgamma = sum g * xhat against float64: rtol 1e-4 + atol 1e-3 of
    test_merge_bwd_gpu.py::test_deferred_apply_forms_dy_inside_the_launch (accumulated into zeros here)"""
    torch.testing.assert_close(pend.dbeta.double().cpu(), p['sg'], rtol=1e-4, atol=1e-3, msg=lambda m: who + ' dbeta: ' + m)
    torch.testing.assert_close(pend.dgamma.double().cpu(), p['sgx'], rtol=1e-4, atol=1e-3, msg=lambda m: who + ' dgamma: ' + m)


@pytest.mark.parametrize('in_act,ap_args', [('selu', (70, 70, 16, 16, 'relu', 256)), ('relu', (71, 70, 16, 16, 'selu', 256))])
def test_weight_gradient_that_absorbs_the_batchnorm_apply(K, in_act, ap_args):
    """lvae_conv2d_wgrad_apply_f32 with ap.act != in_act (kink rule 3 on the apply's x): against the two launches it replaces, to the bounds
    of test_kernels_gpu.py::test_weight_gradient_that_absorbs_the_batchnorm_apply_in_front_of_it (stored dy 1e-6, dgamma / dbeta rtol 1e-5 +
    atol 1e-4, dW / db 2e-6), and against float64: the stored dy to the 2e-6 of test_merge_bwd_gpu.py::test_deferred_apply_forms_dy_inside_
    the_launch, dW from the dy the launch stored to the 3e-6 of test_wgrad_pair_gpu.py::test_pair_launch_matches_the_two_launches_it_
    replaces_and_float64."""
    p = R.apply_input(*ap_args)
    N, H, W = ap_args[1:4]
    ap_act = ap_args[4]
    g = torch.Generator().manual_seed(N + 7 * H)
    x = torch.randn(N, H, W, C, generator=g)
    w = packed_weight(torch.randn(C, C, 3, 3, generator=g) / 24)
    drop = (torch.rand(N, C, generator=g) < 0.8).float() / 0.8
    geom = K.ConvGeom(w, 1, 1)
    xd = x.cuda()
    assert K.conv2d_wgrad_apply_ok(xd, w, geom)
    cin = R.bn_coef(x, torch.ones(C), torch.zeros(C)).cuda()
    a, b = dev_apply(K, p, with_add=False), dev_apply(K, p, with_add=False)
    dy_ref = K.affine_act_bwd_parts(a.parts, a.dh, a.x, a.coef[0], a.coef[1], ap_act, a.coef[2], a.coef[3], a.dgamma, a.dbeta, drop=drop.cuda())
    dw_a, dbias_a = torch.zeros_like(w), torch.zeros(C, device='cuda')
    K.conv2d_wgrad(xd, dy_ref, w, geom, dw_a, dbias_a, in_scale=cin[0], in_shift=cin[1], in_act=in_act)
    dw_b, dbias_b = torch.zeros_like(w), torch.zeros(C, device='cuda')
    dy = K.conv2d_wgrad_apply(xd, w, geom, dw_b, dbias_b, b.parts, b.dh, b.x, b.coef[0], ap_act, b.dgamma, b.dbeta, drop=drop.cuda(),
                              in_scale=cin[0], in_shift=cin[1], in_act=in_act)
    torch.cuda.synchronize()
    assert rel(dy, dy_ref) < 1e-6
    torch.testing.assert_close(b.dgamma, a.dgamma, rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(b.dbeta, a.dbeta, rtol=1e-5, atol=1e-4)
    assert rel(dw_b, dw_a) < 2e-6 and rel(dbias_b, dbias_a) < 2e-6
    dy64 = p['dy'] * drop.double().view(N, 1, 1, C)
    e_dy = rel(dy, dy64)
    xin = R.act(R.preact(x, cin.cpu()), in_act)
    e_w = rel(dw_b, torch.nn.grad.conv2d_weight(to_nchw(xin), (C, C, 3, 3), to_nchw(dy.cpu()), padding=1))
    print('wgrad_apply in_act %s ap.act %s: moved %d of %d, dy %.3g dW %.3g' % (in_act, ap_act, p['moved'], p['numel'], e_dy, e_w))
    assert e_dy < 2e-6 and e_w < 3e-6
    check_apply_sums(b, p, 'wgrad_apply')


def test_weight_gradient_pair_with_three_different_ids(K):
    """lvae_conv2d_wgrad_pair_f32: conv1's prologue relu, its apply leakyrelu (rule 3), conv2's prologue selu. Bounds of
    test_wgrad_pair_gpu.py::test_pair_launch_matches_the_two_launches_it_replaces_and_float64: stored dy 1e-6, dgamma / dbeta rtol 1e-5 +
    atol 1e-4 and gradients 2e-6 against the two launches, 3e-6 against float64."""
    ap_args = (72, 64, 16, 16, 'leakyrelu', 256)
    p = R.apply_input(*ap_args)
    N, H, W = 64, 16, 16
    g = torch.Generator().manual_seed(99)
    x, dy_b = torch.randn(N, H, W, C, generator=g), torch.randn(N, H, W, C, generator=g)
    w_a, w_b = packed_weight(torch.randn(C, C, 3, 3, generator=g) / 24), packed_weight(torch.randn(C, C, 3, 3, generator=g) / 24)
    g_a, g_b = K.ConvGeom(w_a, 1, 1), K.ConvGeom(w_b, 1, 1)
    drop = ((torch.rand(N, C, generator=g) < 0.8).float() / 0.8)
    pre = dict(dw_a=torch.randn(C, C, 3, 3, generator=g), db_a=torch.randn(C, generator=g), dw_b=torch.randn(C, C, 3, 3, generator=g),
               db_b=torch.randn(C, generator=g))
    xd, dybd, dropd = x.cuda(), dy_b.cuda(), drop.cuda()
    cin = R.bn_coef(x, torch.ones(C), torch.zeros(C)).cuda()
    assert K.conv2d_wgrad_pair_ok(xd, w_a, g_a, p['x'].cuda(), w_b, g_b)

    def buffers():
        return {k: (packed_weight(v) if v.dim() == 4 else v.cuda()) for k, v in pre.items()}
    ref, a = buffers(), dev_apply(K, p, with_add=False)
    dy_ref = K.conv2d_wgrad_apply(xd, w_a, g_a, ref['dw_a'], ref['db_a'], a.parts, a.dh, a.x, a.coef[0], 'leakyrelu', a.dgamma, a.dbeta, drop=dropd,
                                  in_scale=cin[0], in_shift=cin[1], in_act='relu')
    K.conv2d_wgrad(a.x, dybd, w_b, g_b, ref['dw_b'], ref['db_b'], in_scale=a.coef[0], in_shift=a.coef[1], in_act='selu')
    got, b = buffers(), dev_apply(K, p, with_add=False)
    dy = K.conv2d_wgrad_pair(xd, w_a, g_a, got['dw_a'], got['db_a'], b.parts, b.dh, b.x, b.coef[0], 'leakyrelu', b.dgamma, b.dbeta, dybd, w_b, g_b,
                             got['dw_b'], got['db_b'], drop=dropd, in_scale=cin[0], in_shift=cin[1], in_act='relu', in_scale_b=b.coef[0],
                             in_shift_b=b.coef[1], in_act_b='selu', out=b.out)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dy).all()) and rel(dy, dy_ref) < 1e-6
    torch.testing.assert_close(b.dgamma, a.dgamma, rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(b.dbeta, a.dbeta, rtol=1e-5, atol=1e-4)
    for k in pre:
        assert rel(got[k], ref[k]) < 2e-6, (k, rel(got[k], ref[k]))
    in_a = R.act(R.preact(x, cin.cpu()), 'relu')
    in_b = R.act(R.preact(p['x'], p['coef']), 'selu')
    for k, xin, dyk in (('a', in_a, dy.cpu()), ('b', in_b, dy_b)):
        want = torch.nn.grad.conv2d_weight(to_nchw(xin), (C, C, 3, 3), to_nchw(dyk), padding=1)
        err = rel(got['dw_' + k].cpu().double() - pre['dw_' + k].double(), want)
        # the bias gradient against the magnitudes summed (a BatchNorm backward sums to about zero per channel), as the pair test sets it
        have_b = got['db_' + k].cpu().double() - pre['db_' + k].double()
        err_b = float((have_b - dyk.double().sum((0, 1, 2))).norm() / dyk.double().abs().sum((0, 1, 2)).norm())
        print('pair %s: dW %.3g db %.3g' % (k, err, err_b))
        assert err < 3e-6 and err_b < 3e-6
    assert rel(dy, p['dy'] * drop.double().view(N, 1, 1, C)) < 2e-6   # (test_merge_bwd_gpu.py's bound of a stored apply)
    check_apply_sums(b, p, 'pair')


def test_shared_weight_gradient_launch_with_a_different_prologue_per_problem(K):
    """lvae_conv2d_wgrad_shared_f32 (a stochastic layer's three gradients, 64x16x16): in_act selu, relu and None with coefficients, one
    per problem. 3e-6 against float64 as test_wgrad_shared_gpu.py::test_shared_launch_matches_the_single_launches_and_float64."""
    N, H, W = 64, 16, 16
    g = torch.Generator().manual_seed(77)
    items, wants = [], []
    for cin, in_act in ((32, 'selu'), (64, 'relu'), (64, None)):
        x, dy = torch.randn(N, H, W, cin, generator=g), torch.randn(N, H, W, C, generator=g)
        w = packed_weight(torch.randn(C, cin, 3, 3, generator=g) / 24)
        coef = R.bn_coef(x, torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.3)
        dw0, db0 = torch.randn(C, cin, 3, 3, generator=g), torch.randn(C, generator=g)
        cd = coef.cuda()
        items.append((x.cuda(), dy.cuda(), w, K.ConvGeom(w, 1, 1), packed_weight(dw0), db0.cuda(), dict(in_scale=cd[0], in_shift=cd[1], in_act=in_act)))
        wants.append((torch.nn.grad.conv2d_weight(to_nchw(R.act(R.preact(x, coef), in_act)), (C, cin, 3, 3), to_nchw(dy), padding=1), dw0,
                      dy.double().sum((0, 1, 2)), db0))
    assert K.conv2d_wgrad_shared_ok([(it[0], it[2], it[3]) for it in items])
    K.conv2d_wgrad_shared(items)
    torch.cuda.synchronize()
    for it, (want_w, dw0, want_b, db0) in zip(items, wants):
        e_w, e_b = rel(it[4].cpu().double() - dw0.double(), want_w), rel(it[5].cpu().double() - db0.double(), want_b)
        print('shared in_act %s: dW %.3g db %.3g' % (it[6]['in_act'], e_w, e_b))
        assert e_w < 3e-6 and e_b < 3e-6


# =================================================================================================================================
# 3. BatchNorm-backward sums in the dgrad epilogues: sum g and sum g * xhat with g = dh * stats_act'(x * scale + shift) (kink rule 3)

# name: ((N, Cin, Cout, H, W), precision, stats_act, variant, workgroups per image or None, bound of dh). The sums are held to 1e-5 against
# the float64 formula (test_wino2_epilogue_gpu.py::test_conv2d_through_the_256_pixel_kernel, 'dgrad-bn-bwd-sums') and, through
# affine_act_bwd_parts, against affine_act_bwd to the bounds of test_kernels_gpu.py::test_bn_backward_sums_from_dgrad_epilogue (dx 2e-6,
# dgamma / dbeta 1e-5). dh itself: 2e-6 test_conv_fwd_dgrad_wgrad (halo) and test_conv3x3_position_major_small_images, 4e-6
# test_conv3x3_winograd, 1e-5 test_conv3x3_bf16_operands.
STATS_CASES = {
    'halo':     ((3, 64, 64, 8, 8), 'f32', 'leakyrelu', 'DIRECT', 2, 2e-6),   # (not in the list above: the halo kernel has the epilogue too)
    'pos':      ((37, 64, 64, 4, 4), 'f32', 'relu', 'POS', None, 2e-6),
    'wino-32':  ((66, 64, 64, 16, 16), 'f32', 'selu', 'WINO_F32', 2, 4e-6),
    'wino-32-leaky': ((66, 64, 64, 16, 16), 'f32', 'leakyrelu', 'WINO_F32', 2, 4e-6),
    'wino-six': ((200, 64, 64, 16, 16), 'f32', 'leakyrelu', 'WINO_SIX', 2, 4e-6),
    'wino-256': ((256, 64, 64, 16, 16), 'f32', 'relu', 'WINO_SIX', 1, 4e-6),
    'bf16':     ((200, 64, 64, 16, 16), 'bf16', 'selu', 'BF16_DIRECT', 2, 1e-5),
}


@pytest.mark.parametrize('name', list(STATS_CASES))
def test_batchnorm_backward_sums_from_the_dgrad_epilogue(K, name):
    (N, Ci, Co, H, W), prec, act, variant, per_image, bound = STATS_CASES[name]
    p = R.affine_input(46, N, H, W)
    g = torch.Generator().manual_seed(46 + N)
    dy = torch.randn(N, Co, H, W, generator=g)
    w = torch.randn(Co, Ci, 3, 3, generator=g) / math.sqrt(9 * Ci)
    drop = ((torch.rand(N, Ci, generator=g) < 0.8).float() / 0.8).cuda()
    add = torch.randn(N, H, W, Ci, generator=g).cuda()
    rnd = bf if prec == 'bf16' else (lambda t: t.double())
    dh64 = F.conv_transpose2d(rnd(dy), rnd(w), padding=1).permute(0, 2, 3, 1)
    wp = packed_weight(w)
    geom = K.ConvGeom(wp, 1, 1)
    xb, coef, dyd = p['x'].cuda(), p['coef'].cuda(), nhwc(dy)
    assert K.bn_coef_block(coef[0], coef[1], coef[2], coef[3])
    with precision(K, prec):
        got_route = route(K, geom, wp, dyd, (H, W), Ci, dgrad=True)
        assert got_route[0] == getattr(K._C, 'VARIANT_' + variant), (name, got_route)
        assert per_image is None or got_route[2] == per_image * N, (name, got_route)
        dh, parts = K.conv2d_dgrad(dyd, wp, geom, (H, W), bn_bwd=(xb, coef[0], act))
        assert parts is not None, "this shape is meant to take a kernel with the statistics epilogue"
        torch.cuda.synchronize()
    e_dh = rel(dh, dh64)
    gr, xh = R.bn_bwd_sums(dh64, p['x'], p['coef'], act)
    s = parts.double().sum(0).cpu()
    e1, e2 = rel(s[0], gr.reshape(-1, Ci).sum(0)), rel(s[1], (gr * xh).reshape(-1, Ci).sum(0))
    print('stats %s stats_act %s: moved %d of %d, dh %.3g sum g %.3g sum g xhat %.3g' % (name, act, p['moved'], p['numel'], e_dh, e1, e2))
    assert e_dh < bound
    assert e1 < 1e-5 and e2 < 1e-5
    dg, db = torch.zeros(Ci, device='cuda'), torch.zeros(Ci, device='cuda')
    dg2, db2 = torch.zeros(Ci, device='cuda'), torch.zeros(Ci, device='cuda')
    got = K.affine_act_bwd_parts(parts, dh, xb, coef[0], coef[1], act, coef[2], coef[3], dg, db, drop=drop, add=add)
    ref = K.affine_act_bwd(dh, xb, coef[0], coef[1], act, True, coef[2], coef[3], dg2, db2, drop=drop, add=add)
    torch.cuda.synchronize()
    assert rel(got, ref) < 2e-6
    assert rel(dg, dg2) < 1e-5 and rel(db, db2) < 1e-5


# =================================================================================================================================
# 4. Gate forward: ab = conv1x1(x) + bias, out = act(a) * sigmoid(b) + res. 2e-6 against float64 (operands rounded beforehand at
# precision bf16): test_kernels_gpu.py::test_conv1x1_gate_fused, ::test_conv1x1_gate_fused_bf16_operands.

@functools.lru_cache(maxsize=None)
def gate_fwd_problem(shape, prec):
    N, Cc, H, W = shape
    g = torch.Generator().manual_seed(11 + N)
    x, res = torch.randn(N, Cc, H, W, generator=g), torch.randn(N, Cc, H, W, generator=g)
    w, b = torch.randn(2 * Cc, Cc, 1, 1, generator=g) / math.sqrt(Cc), torch.randn(2 * Cc, generator=g)
    rnd = bf if prec == 'bf16' else (lambda t: t.double())
    return x, res, w, b, F.conv2d(rnd(x), rnd(w), b.double())


@pytest.mark.parametrize('shape,prec,form,act,variant', [
    ((40, 64, 16, 16), 'f32', 'split', 'relu', 'GATE_PERSISTENT'), ((40, 64, 16, 16), 'f32', 'mfma_f32', 'selu', 'GATE_PERSISTENT'),
    ((40, 64, 16, 16), 'f32', 'split', 'leakyrelu', 'GATE_PERSISTENT'), ((70, 32, 8, 8), 'f32', None, 'leakyrelu', 'GATE_SINGLE_SHOT'),
    ((70, 32, 8, 8), 'f32', None, 'relu', 'GATE_SINGLE_SHOT'), ((37, 64, 3, 3), 'bf16', None, 'selu', 'GATE_PERSISTENT'),
    ((37, 64, 3, 3), 'bf16', None, 'relu', 'GATE_PERSISTENT')])
def test_gate_forward(K, shape, prec, form, act, variant):
    N, Cc, H, W = shape
    x, res, w, b, ab = gate_fwd_problem(shape, prec)
    a_, b_ = ab.chunk(2, 1)
    out = R.act(a_, act) * torch.sigmoid(b_) + res.double()
    wp = packed_weight(w)
    geom = K.ConvGeom(wp, 1, 0)
    xd, bd = nhwc(x), b.cuda()
    with precision(K, prec), K.use_form(form_of(K, form)):
        d = K._desc(geom, wp, xd, None, N, H, W, H, W, 2 * Cc, geom.s_ci, geom.s_co, K.GATHER_CONV, bd, y=torch.empty(N, H, W, 2 * Cc, device='cuda'))
        assert K._C.load().lvae_conv1x1_gate_variant(ctypes.byref(d)) == getattr(K._C, variant)
        abd, outd = K.conv1x1_gate(xd, wp, geom, bd, nhwc(res), act)
        abn, outn = K.conv1x1_gate(xd, wp, geom, bd, None, act, need_ab=False)
        torch.cuda.synchronize()
    e_ab, e_out, e_bare = rel(nchw(abd), ab), rel(nchw(outd), out), rel(nchw(outn), out - res.double())
    print('gate forward %s %s %s act %s: ab %.3g out %.3g without residual %.3g' % (shape, prec, form, act, e_ab, e_out, e_bare))
    assert abn is None and e_ab < 2e-6 and e_out < 2e-6 and e_bare < 2e-6


@pytest.mark.parametrize('shape,in_act,g_act', [((64, 32, 32), 'relu', 'selu'), ((256, 16, 16), 'leakyrelu', 'relu'), ((256, 16, 16), None, 'leakyrelu')])
def test_conv_gate_behind_the_winograd_kernel(K, shape, in_act, g_act):
    """lvae_resblock_conv_f32 / LVAE_RB_EPI_GATE behind the 256-pixel Winograd kernel (g_act of its epilogue), forward only: y2, ab and out
    to the 4e-6 of test_resblock_img_gpu.py::test_conv_gate_fusion_behind_the_winograd_kernel and
    test_wino2_epilogue_gpu.py::test_conv_gate_through_the_256_pixel_kernel."""
    N, H, W = shape
    g = torch.Generator().manual_seed(N + 3 * H)
    rn = lambda *s: torch.randn(*s, generator=g)
    x, res = rn(N, H, W, C) * 1.5 + 0.3, rn(N, H, W, C)
    w2, b2 = rn(C, C, 3, 3) / 24, rn(C)
    wg, bg = rn(2 * C, C, 1, 1) / 8, rn(2 * C) * 0.5
    m2 = (torch.rand(N, C, generator=g) < 0.8).float() / 0.8
    coef = R.bn_coef(x, torch.rand(C, generator=g) + 0.5, rn(C) * 0.3)
    r_y2 = (F.conv2d(to_nchw(R.act(R.preact(x, coef), in_act)), w2.double(), b2.double(), padding=1) * m2.double().view(N, C, 1, 1))
    r_ab = F.conv2d(r_y2, wg.double(), bg.double())
    a_, b_ = r_ab.chunk(2, 1)
    r_out = R.act(a_, g_act) * torch.sigmoid(b_) + to_nchw(res)
    xd, w2p, wgp, cd = x.cuda(), packed_weight(w2), packed_weight(wg), coef.cuda()
    ge2, geg = K.ConvGeom(w2p, 1, 1), K.ConvGeom(wgp, 1, 0)
    assert K.rb_rows(xd, w2p, ge2) == 0 and K.rb_gate_rows(xd, w2p, ge2) == N * H * W // 256 >= 256
    y2, ab, out, _, _ = K.rb_conv_gate(xd, w2p, ge2, b2.cuda(), in_act, m2.cuda(), wgp, geg, bg.cuda(), res.cuda(), g_act,
                                       coef=(cd[0], cd[1], cd[2], cd[3]))
    torch.cuda.synchronize()
    e = rel(nchw(y2), r_y2), rel(nchw(ab), r_ab), rel(nchw(out), r_out)
    print('conv + gate %s in_act %s g_act %s: y2 %.3g ab %.3g out %.3g' % (shape, in_act, g_act, *e))
    assert max(e) < 4e-6


# =================================================================================================================================
# 5. Persistent gate backward (lvae_conv1x1_gate_bwd_wgrad_f32 / _recompute_f32): every `ELU = false` instantiation of
# conv1x1_gate_bwd_fused_bf16_kernel, the fp32-MFMA kernel's run-time id, and the two mixed cases that must take the `false` build.

def gate_bwd_ref(dout, ab, y, w, mask, act, rnd=None):
    """float64 (dx, dW [2C][C], db) of out = act(a) * sigmoid(b), (a, b) = ab = conv1x1(y) + bias (lib/nn.py:118-126), all channel-last;
    rnd: rounding of the three matrix operands (precision bf16)"""
    rnd = rnd or (lambda t: t)
    N, H, W, _ = dout.shape
    a_, b_ = ab.double()[..., :C], ab.double()[..., C:]
    sg = torch.sigmoid(b_)
    dab = torch.cat([dout.double() * sg * R.act_grad(a_, act), dout.double() * R.act(a_, act) * sg * (1 - sg)], -1).reshape(-1, 2 * C)
    w2 = w[:, :, 0, 0].double()
    dx = (rnd(dab) @ rnd(w2)).reshape(N, H, W, C) * mask.double().view(N, 1, 1, C)
    dw = rnd(dab).t() @ rnd(y.double().reshape(-1, C))
    return dx, dw, dab.sum(0)


@functools.lru_cache(maxsize=None)
def gate_bwd_operands(N, H, W):
    """saved-ab operands of one shape: y, the gate weights, ab = conv1x1(y) + bias in fp32 (what a forward would have stored), dout, the
    Dropout2d mask and what the gradient buffers start from"""
    g = torch.Generator().manual_seed(N + H)
    y = torch.randn(N, H, W, C, generator=g)
    w = torch.randn(2 * C, C, 1, 1, generator=g) / math.sqrt(C)
    b = torch.randn(2 * C, generator=g)
    ab = F.conv2d(y.permute(0, 3, 1, 2), w, b).permute(0, 2, 3, 1).contiguous()
    dout = torch.randn(N, H, W, C, generator=g)
    mask = (torch.rand(N, C, generator=g) < 0.8).float() / 0.8
    dw0, db0 = torch.randn(2 * C, C, 1, 1, generator=g) * 0.1, torch.randn(2 * C, generator=g)
    return types.SimpleNamespace(y=y, w=w, b=b, ab=ab, dout=dout, mask=mask, dw0=dw0, db0=db0)


# name: ((N, H, W), precision, form, saved ab | recompute, arguments of act_ref.apply_input or None, bf16 storage, the gate's act)
# the instantiation each launches: conv1x1_gate_bwd_fused_bf16_kernel<NP, S16, AP, ELU = false[, RC]>, csrc/conv1x1_gate_bwd_fused.hip
GATE_BWD_CASES = {
    'six-saved':           ((64, 16, 16), 'f32', None, 'saved', None, False, 'relu'),                                # <3, false, false, false>
    'six-apply':           ((70, 16, 16), 'f32', None, 'saved', (71, 70, 16, 16, 'selu', 256), False, 'leakyrelu'),   # <3, false, true, false>
    'six-recompute':       ((64, 16, 16), 'f32', None, 'recompute', None, False, 'selu'),                            # <3, false, false, false, true>
    'six-recompute-70':    ((70, 16, 16), 'f32', None, 'recompute', None, False, 'leakyrelu'),
    'six-recompute-apply': ((70, 16, 16), 'f32', None, 'recompute', (75, 70, 16, 16, 'selu', 7), False, 'relu'),      # <3, false, true, false, true>
    'bf16':                ((64, 16, 16), 'bf16', None, 'saved', None, False, 'leakyrelu'),                          # <1, false, false, false>
    'bf16-apply':          ((70, 16, 16), 'bf16', None, 'saved', (70, 70, 16, 16, 'relu', 256), False, 'selu'),       # <1, false, true, false>
    'bf16-stored':         ((64, 16, 16), 'bf16', None, 'saved', None, True, 'relu'),                                # <1, true, false, false>
    'bf16-stored-apply':   ((64, 16, 16), 'bf16', None, 'saved', (72, 64, 16, 16, 'leakyrelu', 256), True, 'selu'),   # <1, true, true, false>
    'mfma-f32':            ((70, 16, 16), 'f32', 'mfma_f32', 'saved', None, False, 'leakyrelu'),                      # conv1x1_gate_bwd_fused_kernel
    'mixed-relu-elu':      ((64, 16, 16), 'f32', None, 'saved', (74, 64, 16, 16, 'elu', 256), False, 'relu'),         # <3, false, true, false>
    'mixed-elu-relu':      ((64, 16, 16), 'f32', None, 'saved', (73, 64, 16, 16, 'relu', 3), False, 'elu'),           # <3, false, true, false>
}


@pytest.mark.parametrize('name', list(GATE_BWD_CASES))
def test_persistent_gate_backward(K, name):
    """dx, dW, db against float64: 3e-6, 5e-6, 5e-6 in fp32 (test_kernels_gpu.py::test_conv1x1_gate_bwd_with_fused_weight_gradient,
    test_gate_recompute_gpu.py::test_recompute_form_against_float64_autograd) and 3e-4, 3e-4, 5e-6 against operands rounded beforehand at
    precision bf16 (test_kernels_gpu.py::test_conv1x1_gate_bwd_fused_bf16_operands). With a deferred apply the kernel forms dout itself
    (ap.act != the gate's act, rule 3): the stored dout to 2e-6 and dgamma / dbeta to rtol 1e-4 + atol 1e-3
    (test_merge_bwd_gpu.py::test_deferred_apply_forms_dy_inside_the_launch), and against the two launches to 1e-6, rtol 1e-5 + atol 1e-4 and
    2e-6 / 2e-3 (test_resblock_img_gpu.py::test_deferred_batchnorm_apply_in_the_next_blocks_first_backward_launch). bf16 storage is exact
    against fp32 storage of the same values (test_bf16_storage_gpu.py::test_gate_kernels_bf16_storage_is_exact). The recompute form forms
    the pre-activations itself (rule 4)."""
    (N, H, W), prec, form, mode, ap_args, stored16, act = GATE_BWD_CASES[name]
    recompute = mode == 'recompute'
    touched = 0
    if recompute:
        q = R.gate_input(80 if N == 64 else 81, N, H, W)
        g = torch.Generator().manual_seed(N)
        o = types.SimpleNamespace(y=q['y'], w=q['w'], b=q['b'], ab=q['ab'], dout=q['dout'], mask=(torch.rand(N, C, generator=g) < 0.8).float() / 0.8,
                                  dw0=torch.randn(2 * C, C, 1, 1, generator=g) * 0.1, db0=torch.randn(2 * C, generator=g))
        touched = q['zeroed']
    else:
        o = gate_bwd_operands(N, H, W)
    ab_ref, y_ref = (bf(o.ab), bf(o.y)) if stored16 else (o.ab, o.y)   # the numbers the kernel is handed
    p = R.apply_input(*ap_args) if ap_args else None
    add = None
    if p is not None:
        add = p['add']
        if recompute:   # rule 4 with the upstream gradient formed inside the launch: add = -dy where the gate's pre-activation is near 0
            add = torch.where(q['near'], -p['dy'].float(), add)
        dout64 = p['dy'] + add.double()
    else:
        dout64 = o.dout.double()
    dx64, dw64, db64 = gate_bwd_ref(dout64, ab_ref, y_ref, o.w, o.mask, act, bf if prec == 'bf16' else None)
    wp = packed_weight(o.w)
    geom = K.ConvGeom(wp, 1, 0)
    yd, abd, maskd, bd = y_ref.float().cuda(), ab_ref.float().cuda(), o.mask.cuda(), o.b.cuda()

    def launch(stored, apply_now):
        dw, db = packed_weight(o.dw0), o.db0.cuda()
        pend = None
        if p is not None:
            pend = dev_apply(K, p)
            pend.add = add.cuda()
        if not apply_now and pend is not None:   # the two-launch form: the apply by its own kernel
            dout = K.affine_act_bwd_parts(pend.parts, pend.dh, pend.x, pend.coef[0], pend.coef[1], p['act'], pend.coef[2], pend.coef[3], pend.dgamma,
                                          pend.dbeta, add=pend.add)
            ap = None
        else:
            dout, ap = (pend.out, pend) if pend is not None else (o.dout.cuda(), None)
        if recompute:
            dx = K.conv1x1_gate_bwd_wgrad_recompute(dout, yd, wp, geom, bd, act, dw, db, out_scale=maskd, apply=ap)
        elif stored:
            dx = K.conv1x1_gate_bwd_wgrad(dout, abd.to(torch.bfloat16), yd.to(torch.bfloat16), wp, geom, act, dw, db, out_scale=maskd, out_bf16=True, apply=ap)
        else:
            dx = K.conv1x1_gate_bwd_wgrad(dout, abd, yd, wp, geom, act, dw, db, out_scale=maskd, apply=ap)
        assert dx is not None, "shape is meant to take the persistent kernel"
        torch.cuda.synchronize()
        return dx, dw, db, pend, dout

    with precision(K, prec), K.use_form(form_of(K, form)):
        assert K.gate_bwd_fused_ws(yd, wp, geom, packed_weight(o.dw0)) > 0
        assert p is None or K.gate_bwd_apply_ok(yd, wp, geom)
        assert not recompute or K.gate_bwd_recompute_ok(yd, wp, geom)
        dx, dw, db, pend, _ = launch(False, True)
        two = launch(False, False) if p is not None else None
        s16 = launch(True, True) if stored16 else None
    e_dx, e_dw, e_db = rel(dx, dx64), rel((dw.cpu() - o.dw0)[:, :, 0, 0], dw64), rel(db.cpu() - o.db0, db64)
    print('gate backward %s act %s ap.act %s: touched %d, dx %.3g dW %.3g db %.3g' % (name, act, p and p['act'], touched + (p['moved'] if p else 0),
                                                                                      e_dx, e_dw, e_db))
    b_dx, b_dw = (3e-4, 3e-4) if prec == 'bf16' else (3e-6, 5e-6)
    assert e_dx < b_dx and e_dw < b_dw and e_db < 5e-6
    if p is not None:
        e_out = rel(pend.out, dout64)
        print('   stored dout %.3g' % e_out)
        assert bool(torch.isfinite(pend.out).all()) and e_out < 2e-6
        check_apply_sums(pend, p, name)
        dx2, dw2, db2, pend2, dout2 = two
        assert rel(pend.out, dout2) < 1e-6
        torch.testing.assert_close(pend.dgamma, pend2.dgamma, rtol=1e-5, atol=1e-4)
        torch.testing.assert_close(pend.dbeta, pend2.dbeta, rtol=1e-5, atol=1e-4)
        for a_, b_ in ((dx, dx2), (dw, dw2), (db, db2)):
            assert rel(a_, b_) < (2e-6 if prec == 'f32' else 2e-3)
    if stored16:
        dx16, dw16, db16, pend16, _ = s16
        assert dx16.dtype == torch.bfloat16 and torch.equal(dx16, dx.to(torch.bfloat16)) and torch.equal(dw16, dw)
        torch.testing.assert_close(db16, db, rtol=1e-5, atol=1e-3)
        if p is not None:
            assert torch.equal(pend16.out, pend.out)


# =================================================================================================================================
# 6. Merge backward with a deferred apply (lvae_conv1x1_cat_bwd_f32, ap.act; kink rule 3)

@pytest.mark.parametrize('ap_args', [(76, 4, 8, 8, 'leakyrelu', 3), (78, 4, 8, 8, 'relu', 1), (79, 4, 8, 8, 'selu', 3), (82, 4, 8, 8, 'leakyrelu', 1),
                                     (83, 4, 8, 8, 'relu', 3), (84, 4, 8, 8, 'selu', 1)])
def test_merge_backward_with_a_deferred_apply(K, ap_args):
    """the case and the bounds of test_merge_bwd_gpu.py::test_deferred_apply_forms_dy_inside_the_launch: dx1 / dx2 3e-6, dW / db 5e-6, dgamma /
    dbeta rtol 1e-4 + atol 1e-3, the stored dy 2e-6, all against float64"""
    p = R.apply_input(*ap_args)
    N, H, W = ap_args[1:4]
    g = torch.Generator().manual_seed(70)
    x1, x2 = torch.randn(N, H, W, C, generator=g), torch.randn(N, H, W, C, generator=g)
    w = torch.randn(C, 2 * C, 1, 1, generator=g) / (2 * C) ** 0.5
    dy64 = p['dy'] + p['add'].double()
    xc = to_nchw(torch.cat([x1, x2], 3)).requires_grad_(True)
    wd, bd = w.double().requires_grad_(True), torch.zeros(C, dtype=torch.float64, requires_grad=True)
    F.conv2d(xc, wd, bd).backward(to_nchw(dy64))
    ref = xc.grad.permute(0, 2, 3, 1)
    wp = packed_weight(w)
    geom = K.ConvGeom(wp, 1, 0)
    dw0, db0 = torch.randn(C, 2 * C, 1, 1, generator=g) * 0.1, torch.randn(C, generator=g)
    dw, db = packed_weight(dw0), db0.cuda()
    pend = dev_apply(K, p)
    assert K.cat_bwd_apply_ok(pend.out, wp, geom, C)
    both = K.conv1x1_cat_bwd(pend.out, x1.cuda(), x2.cuda(), wp, geom, dw, db, apply=pend, store_dy=True, max_workgroups=3)
    assert both is not None
    torch.cuda.synchronize()
    figs = dict(dx1=rel(both[0], ref[..., :C]), dx2=rel(both[1], ref[..., C:]), dW=rel(dw.cpu().double() - dw0.double(), wd.grad),
                db=rel(db.cpu().double() - db0.double(), bd.grad), dy=rel(pend.out, dy64))
    print('merge backward ap.act %s: moved %d of %d' % (p['act'], p['moved'], p['numel']), ' '.join('%s %.2e' % kv for kv in figs.items()))
    assert figs['dx1'] < 3e-6 and figs['dx2'] < 3e-6 and figs['dW'] < 5e-6 and figs['db'] < 5e-6 and figs['dy'] < 2e-6
    check_apply_sums(pend, p, 'merge')


# =================================================================================================================================
# 7. Fused small-level block (csrc/resblock_img.hip)

@pytest.mark.parametrize('shape,acts', [((37, 2, 2), ('relu', 'selu', 'leakyrelu')), ((7, 8, 8), ('selu', 'leakyrelu', 'relu')),
                                        ((40, 4, 4), ('leakyrelu', None, 'selu'))])
def test_fused_block_forward_at_precision_bf16(K, shape, acts):
    """The run-time-activation build of the whole-image block kernels at precision bf16, forward only (its backward is out of scope, see
    the module docstring): conv1's prologue, conv2's prologue and the gate each with an id of their own. Bounds of
    test_resblock_img_gpu.py::test_fused_block_forward_and_backward at precision bf16 (tol = 4000): y1 2e-6 * tol, y2 / ab / out 3e-6 * tol."""
    from test_resblock_img_gpu import make_block
    N, H, W = shape
    a1, a2, a3 = acts
    p = make_block(N, H, W, 7 * N + H)
    with torch.no_grad():
        bn = lambda t, ga, be: F.batch_norm(t, None, None, ga, be, True, 0.1, 1e-5)
        y1 = F.conv2d(R.act(bn(p.x, p.g1, p.be1), a1), p.w1, p.b1, padding=1) * p.m1[:, :, None, None]
        y2 = F.conv2d(R.act(bn(y1, p.g2, p.be2), a2), p.w2, p.b2, padding=1) * p.m2[:, :, None, None]
        ab = F.conv2d(y2, p.wg, p.bg)
        a_, b_ = ab.chunk(2, 1)
        out = R.act(a_, a3) * torch.sigmoid(b_) + p.x
    tol = 4000.0
    f = lambda t: t.detach().float().cuda()
    x = nhwc(p.x)
    w1, w2, wg = packed_weight(p.w1.detach()), packed_weight(p.w2.detach()), packed_weight(p.wg.detach())
    ge1, ge2, geg = K.ConvGeom(w1, 1, 1), K.ConvGeom(w2, 1, 1), K.ConvGeom(wg, 1, 0)
    mk_bn = lambda ga, be: types.SimpleNamespace(weight=f(ga), bias=f(be), running_mean=torch.zeros(C, device='cuda'),
                                                 running_var=torch.ones(C, device='cuda'), eps=1e-5, momentum=0.1)
    bn1, bn2 = mk_bn(p.g1, p.be1), mk_bn(p.g2, p.be2)
    with precision(K, 'bf16'):
        assert K.rb_rows(x, w1, ge1) > 0
        coef1 = K.bn_stats(x, bn1.weight, bn1.bias, bn1.running_mean, bn1.running_var, bn1.eps, bn1.momentum)
        y1d, parts2, _ = K.rb_conv(x, w1, ge1, f(p.b1), a1, f(p.m1), coef=coef1, stats_pivot=bn2.running_mean)
        y2d, abd, outd, _, _ = K.rb_conv_gate(y1d, w2, ge2, f(p.b2), a2, f(p.m2), wg, geg, f(p.bg), x, a3, in_bn=(parts2, bn2.running_mean, bn2),
                                              stats_pivot=coef1[2])
        torch.cuda.synchronize()
    e = rel(nchw(y1d), y1), rel(nchw(y2d), y2), rel(nchw(abd), ab), rel(nchw(outd), out)
    print('block forward bf16 %s %s: y1 %.3g y2 %.3g ab %.3g out %.3g' % (shape, acts, *e))
    assert e[0] < 2e-6 * tol and max(e[1:]) < 3e-6 * tol


def test_deferred_apply_in_the_whole_image_gate_backward(K):
    """The deferred-apply chain of test_resblock_img_gpu.py::test_deferred_batchnorm_apply_in_the_next_blocks_first_backward_launch at fp32 and its
    smallest shape (37 x 2x2: the whole-image gate-backward + dgrad launch, lvae_rb_ext.ap_*), with ap.act = selu and ELU elsewhere: the
    deferred launch against the two-launch form to that test's bounds (dout 1e-6, dgamma / dbeta rtol 1e-5 + atol 1e-4, everything downstream
    2e-6), and the stored dout and the sums against float64 (2e-6, rtol 1e-4 + atol 1e-3: test_merge_bwd_gpu.py)."""
    ap_args = (77, 37, 2, 2, 'selu', 7)
    p = R.apply_input(*ap_args)
    N, H, W = ap_args[1:4]
    g = torch.Generator().manual_seed(11 * N + H)
    rn = lambda *s_: torch.randn(*s_, generator=g).cuda()
    wg = packed_weight(torch.randn(2 * C, C, 1, 1, generator=g) / 8)
    w2 = packed_weight(torch.randn(C, C, 3, 3, generator=g) / 24)
    geg, ge2 = K.ConvGeom(wg, 1, 0), K.ConvGeom(w2, 1, 1)
    ab, y1 = rn(N, H, W, 2 * C), rn(N, H, W, C)
    m2 = ((torch.rand(N, C, generator=g) < 0.8).float() / 0.8).cuda()
    coef2 = K.bn_stats(y1, None, None, None, None)
    a, b = dev_apply(K, p), dev_apply(K, p)
    assert K.rb_rows(a.x, w2, ge2) > 0
    dout = K.affine_act_bwd_parts(a.parts, a.dh, a.x, a.coef[0], a.coef[1], 'selu', a.coef[2], a.coef[3], a.dgamma, a.dbeta, add=a.add)
    ref = K.rb_gate_dgrad(dout, ab, wg, geg, 'elu', m2, w2, ge2, bn_bwd=(y1, coef2[0], 'elu'))
    got = K.rb_gate_dgrad(b.out, ab, wg, geg, 'elu', m2, w2, ge2, bn_bwd=(y1, coef2[0], 'elu'), apply=b)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(b.out).all())
    assert rel(b.out, dout) < 1e-6
    torch.testing.assert_close(b.dgamma, a.dgamma, rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(b.dbeta, a.dbeta, rtol=1e-5, atol=1e-4)
    for x_, y_ in zip(got, ref):
        assert rel(x_, y_) < 2e-6
    e_out = rel(b.out, p['dy'] + p['add'].double())
    print('deferred apply in the whole-image launch, ap.act selu: moved %d of %d, dout %.3g' % (p['moved'], p['numel'], e_out))
    assert e_out < 2e-6
    check_apply_sums(b, p, 'whole-image')
