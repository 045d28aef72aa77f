"""The position-major stride-2 / transposed 3x3 kernel (csrc/conv3x3_resample.hip) against F.conv2d / F.conv_transpose2d in float64.

Tolerance: the norm-relative 2e-6 the generic kernel is held to in tests/test_kernels_gpu.py (test_conv_fwd_dgrad_wgrad, test_conv_transpose).
Every launch goes through a descriptor built here, so that y can be pre-filled with NaN (every output pixel must be written) and carry a
guard tail (nothing behind it may be written), and lvae_conv2d_position_major can be asked on exactly the descriptor that is launched."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = 2e-6
GUARD = 1024      # floats behind y
GUARD_VALUE = -7.5


@pytest.fixture(scope='module')
def K():
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels
    return kernels


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().float().cuda()


def nchw(t):
    return t.permute(0, 3, 1, 2).cpu().double()


def rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-20))


def pack(w, cin_dim, cout_dim, order):
    """w in its logical torch shape -> fp32 device tensor of the same logical shape, physically [KH][KW][Cin][Cout] ('kn': the arena layout)
    or [KH][KW][Cout][Cin] ('nk'): a forward launch reads the first n-contiguous and the second k-contiguous, a dgrad launch the other way"""
    first, second = (cin_dim, cout_dim) if order == 'kn' else (cout_dim, cin_dim)
    perm = (2, 3, first, second)
    inv = [perm.index(i) for i in range(4)]
    return w.float().permute(*perm).contiguous().cuda().permute(*inv)


def run(K, g, w, x, out_hw, cout, dgrad, expect_pm, **kw):
    """one lvae_conv2d_f32 launch (forward of g, or its input gradient) into a NaN-filled y with a guard tail; returns y"""
    N, H, W, _ = x.shape
    OH, OW = out_hw
    numel = N * OH * OW * cout
    buf = torch.full((numel + GUARD,), float('nan'), device='cuda')
    buf[numel:] = GUARD_VALUE
    y = buf[:numel].view(N, OH, OW, cout)
    if dgrad:
        d = K._desc(g, w, x, kw.pop('x2', None), N, H, W, OH, OW, cout, g.s_co, g.s_ci, K.GATHER_CONV if g.transposed else K.GATHER_TRANSPOSED, y=y, **kw)
    else:
        d = K._desc(g, w, x, kw.pop('x2', None), N, H, W, OH, OW, cout, g.s_ci, g.s_co, K.GATHER_TRANSPOSED if g.transposed else K.GATHER_CONV, y=y, **kw)
    lib = K._C.load()
    assert lib.lvae_conv2d_position_major(ctypes.byref(d)) == expect_pm
    assert lib.lvae_conv2d_variant(ctypes.byref(d)) == K._C.VARIANT_DIRECT
    K.call('lvae_conv2d_f32', ctypes.byref(d), K.stream_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all()), 'an output pixel was not written'
    assert bool((buf[numel:] == GUARD_VALUE).all()), 'the guard tail behind y was written'
    return y


# (N, Cin, Cout, H, W) of the input
CONV_CASES = [
    (3, 64, 64, 4, 4),     # 2x2 output; top-left positions have 4 taps
    (33, 64, 64, 8, 8),    # ragged second image group
    (2, 16, 8, 8, 8),      # thin channels, ragged 32-column tile
    (5, 64, 64, 7, 7),     # odd size, 4x4 output
    (4, 64, 64, 8, 4),     # non-square
    (2, 32, 64, 16, 16),   # two output-channel tiles
]
# (N, Cin, Cout, H, W, output_padding)
TRANSPOSED_CASES = [
    (3, 64, 64, 4, 4, 1),    # 8x8 output
    (33, 64, 64, 2, 2, 1),   # 4x4 output, ragged group
    (2, 16, 8, 8, 8, 1),     # thin channels
    (3, 64, 64, 4, 4, 0),    # 7x7 output
    (4, 64, 64, 4, 8, 1),    # non-square
]


def conv_problem(case, seed=11):
    N, Ci, Co, H, W = case
    g = torch.Generator().manual_seed(seed + sum(case))
    x = torch.randn(N, Ci, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = (torch.randn(Co, Ci, 3, 3, generator=g, dtype=torch.float64) / math.sqrt(Ci * 9))
    b = torch.randn(Co, generator=g, dtype=torch.float64)
    y = F.conv2d(x, w, b, stride=2, padding=1)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    return x.detach(), w, b, y.detach(), dy, x.grad


def transposed_problem(case, seed=13):
    N, Ci, Co, H, W, op = case
    g = torch.Generator().manual_seed(seed + sum(case))
    x = torch.randn(N, Ci, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = (torch.randn(Ci, Co, 3, 3, generator=g, dtype=torch.float64) / math.sqrt(Ci * 9))
    b = torch.randn(Co, generator=g, dtype=torch.float64)
    y = F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=op)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    return x.detach(), w, b, y.detach(), dy, x.grad


@pytest.mark.parametrize('order', ['kn', 'nk'])
@pytest.mark.parametrize('case', CONV_CASES)
def test_strided_conv_forward_and_dgrad(K, case, order):
    N, Ci, Co, H, W = case
    x, w, b, y, dy, dx = conv_problem(case)
    wp = pack(w, 1, 0, order)
    geom = K.ConvGeom(wp, stride=2, pad=1)
    assert (geom.s_co == 1) == (order == 'kn') and (geom.s_ci == 1) == (order == 'nk')
    yd = run(K, geom, wp, nhwc(x), tuple(y.shape[2:]), Co, False, 1, bias=b.float().cuda())
    assert rel(nchw(yd), y) < TOL
    dxd = run(K, geom, wp, nhwc(dy), (H, W), Ci, True, 1)
    assert rel(nchw(dxd), dx) < TOL


@pytest.mark.parametrize('order', ['kn', 'nk'])
@pytest.mark.parametrize('case', TRANSPOSED_CASES)
def test_transposed_conv_forward_and_dgrad(K, case, order):
    N, Ci, Co, H, W, op = case
    x, w, b, y, dy, dx = transposed_problem(case)
    wp = pack(w, 0, 1, order)
    geom = K.ConvGeom(wp, stride=2, pad=1, transposed=True, output_padding=op)
    assert tuple(y.shape[2:]) == geom.out_size(H, W) == (2 * H - 1 + op, 2 * W - 1 + op)
    yd = run(K, geom, wp, nhwc(x), tuple(y.shape[2:]), Co, False, 1, bias=b.float().cuda())
    assert rel(nchw(yd), y) < TOL
    dxd = run(K, geom, wp, nhwc(dy), (H, W), Ci, True, 1)
    assert rel(nchw(dxd), dx) < TOL


@pytest.mark.parametrize('transposed', [False, True])
def test_fused_prologue_and_epilogue(K, transposed):
    N, C, H, W = 6, 64, 8, 8
    g = torch.Generator().manual_seed(5 + transposed)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    sc, sh = torch.rand(C, generator=g, dtype=torch.float64) + 0.5, torch.randn(C, generator=g, dtype=torch.float64)
    w = torch.randn(C, C, 3, 3, generator=g, dtype=torch.float64) / 24
    b = torch.randn(C, generator=g, dtype=torch.float64)
    drop = (torch.rand(N, C, generator=g) < 0.8).double() / 0.8
    xin = F.elu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    if transposed:
        pre = F.conv_transpose2d(xin, w, b, stride=2, padding=1, output_padding=1)
        wp = pack(w, 0, 1, 'kn')
    else:
        pre = F.conv2d(xin, w, b, stride=2, padding=1)
        wp = pack(w, 1, 0, 'kn')
    y = F.elu(pre * drop.view(N, C, 1, 1))
    geom = K.ConvGeom(wp, stride=2, pad=1, transposed=transposed, output_padding=1 if transposed else 0)
    yd = run(K, geom, wp, nhwc(x), tuple(y.shape[2:]), C, False, 1, bias=b.float().cuda(), in_scale=sc.float().cuda(), in_shift=sh.float().cuda(),
             in_act='elu', out_scale=drop.float().cuda(), out_act='elu')
    assert rel(nchw(yd), y) < TOL


def test_declines_run_on_the_generic_kernel(K):
    g = torch.Generator().manual_seed(21)

    def problem(N, Ci, Co, H, W, k=3, s=2, p=1):
        x = torch.randn(N, Ci, H, W, generator=g, dtype=torch.float64)
        w = torch.randn(Co, Ci, k, k, generator=g, dtype=torch.float64) / math.sqrt(Ci * k * k)
        return x, w, F.conv2d(x, w, None, stride=s, padding=p)

    # a second source (C2 = 64)
    x, w, y = problem(3, 128, 64, 8, 8)
    wp = pack(w, 1, 0, 'kn')
    xd = nhwc(x)
    yd = run(K, K.ConvGeom(wp, 2, 1), wp, xd[..., :64].contiguous(), (4, 4), 64, False, 0, x2=xd[..., 64:].contiguous())
    assert rel(nchw(yd), y) < TOL
    # C1 = 128
    yd = run(K, K.ConvGeom(wp, 2, 1), wp, xd, (4, 4), 64, False, 0)
    assert rel(nchw(yd), y) < TOL
    # x offset by 4 bytes
    x, w, y = problem(3, 64, 64, 8, 8)
    wp = pack(w, 1, 0, 'kn')
    xs = nhwc(x)
    xo = torch.empty(xs.numel() + 1, device='cuda')[1:].view(xs.shape)
    xo.copy_(xs)
    assert xo.data_ptr() % 16 == 4
    yd = run(K, K.ConvGeom(wp, 2, 1), wp, xo, (4, 4), 64, False, 0)
    assert rel(nchw(yd), y) < TOL
    # weights in (Cout, Cin, KH, KW) layout
    wc = w.float().cuda().contiguous()
    yd = run(K, K.ConvGeom(wc, 2, 1), wc, xs, (4, 4), 64, False, 0)
    assert rel(nchw(yd), y) < TOL
    # the 5x5 stem
    x, w, y = problem(3, 3, 64, 32, 32, k=5, s=2, p=2)
    wp = pack(w, 1, 0, 'kn')
    yd = run(K, K.ConvGeom(wp, 2, 2), wp, nhwc(x), (16, 16), 64, False, 0)
    assert rel(nchw(yd), y) < TOL
    # stride 3
    x, w, y = problem(3, 64, 64, 8, 8, s=3)
    wp = pack(w, 1, 0, 'kn')
    yd = run(K, K.ConvGeom(wp, 3, 1), wp, nhwc(x), (3, 3), 64, False, 0)
    assert rel(nchw(yd), y) < TOL
    # the conv gather above 1,024 workgroups (2 image groups x 17x17 positions x 2 channel tiles), where the generic kernel is faster
    x, w, y = problem(33, 64, 64, 34, 34)
    wp = pack(w, 1, 0, 'kn')
    yd = run(K, K.ConvGeom(wp, 2, 1), wp, nhwc(x), (17, 17), 64, False, 0)
    assert rel(nchw(yd), y) < TOL


@pytest.mark.parametrize('transposed', [False, True])
def test_agrees_with_the_generic_kernel(K, transposed):
    """the same convolution through the (Cout, Cin, KH, KW) / (Cin, Cout, KH, KW) weight layout runs on the generic kernel"""
    if transposed:
        case = (33, 64, 64, 4, 4, 1)
        x, w, b, y, dy, dx = transposed_problem(case)
        wp, out_hw = pack(w, 0, 1, 'kn'), tuple(y.shape[2:])
    else:
        case = (33, 64, 64, 8, 8)
        x, w, b, y, dy, dx = conv_problem(case)
        wp, out_hw = pack(w, 1, 0, 'kn'), tuple(y.shape[2:])
    wc = w.float().cuda().contiguous()
    kw = dict(stride=2, pad=1, transposed=transposed, output_padding=1 if transposed else 0)
    y_pm = run(K, K.ConvGeom(wp, **kw), wp, nhwc(x), out_hw, 64, False, 1, bias=b.float().cuda())
    y_gen = run(K, K.ConvGeom(wc, **kw), wc, nhwc(x), out_hw, 64, False, 0, bias=b.float().cuda())
    assert rel(y_pm.double().cpu(), y_gen.double().cpu()) < TOL
    dx_pm = run(K, K.ConvGeom(wp, **kw), wp, nhwc(dy), tuple(x.shape[2:]), 64, True, 1)
    dx_gen = run(K, K.ConvGeom(wc, **kw), wc, nhwc(dy), tuple(x.shape[2:]), 64, True, 0)
    assert rel(dx_pm.double().cpu(), dx_gen.double().cpu()) < TOL
