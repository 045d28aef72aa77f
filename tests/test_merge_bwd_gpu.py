"""The whole backward of a merge / skip-merge 1x1 convolution (128 -> 64 over the channel concat of two 64-channel tensors) as one
persistent launch (lvae_conv1x1_cat_bwd_f32, csrc/conv1x1_cat_bwd_fused.hip): both input gradients, the weight / bias gradient and, in the
deferred form, the BatchNorm-backward apply of the residual block behind the merge that forms dy.

Reference: float64 autograd of F.conv2d on the concatenated input, from the same inputs. Bounds: those
test_kernels_gpu.py::test_conv1x1_gate_bwd_with_fused_weight_gradient asserts for the same arithmetic (six bf16-piece products per product,
fp32 accumulate): norm-relative error of dx1 / dx2 below 3e-6, of dW / db below 5e-6. The two-launch path (lvae_conv2d_wgrad_f32 +
lvae_conv1x1_dgrad_cat_f32) is held to the same bounds on the same inputs, so that a bound too tight for the reference would show as such."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
C = 64
DX_BOUND, DW_BOUND = 3e-6, 5e-6


@pytest.fixture(scope='module')
def K():
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels
    return kernels


def packed_weight(w):
    return w.float().permute(2, 3, 1, 0).contiguous().cuda().permute(3, 2, 0, 1)


def rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / (b.double().cpu().norm() + 1e-30))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def case(N, H, W):
    """Inputs (channel-last, on the device) and the float64 reference of one shape, computed once."""
    g = torch.Generator().manual_seed(1000 * N + H)
    x1, x2, dy = (torch.randn(N, H, W, C, generator=g) for _ in range(3))
    w = torch.randn(C, 2 * C, 1, 1, generator=g) / (2 * C) ** 0.5
    dw0, db0 = torch.randn(C, 2 * C, 1, 1, generator=g) * 0.1, torch.randn(C, generator=g)
    xc = torch.cat([x1, x2], 3).permute(0, 3, 1, 2).double().requires_grad_(True)
    wd, bd = w.double().requires_grad_(True), torch.zeros(C, dtype=torch.float64, requires_grad=True)
    F.conv2d(xc, wd, bd).backward(dy.permute(0, 3, 1, 2).double())
    dx = nhwc(xc.grad)
    return dict(x1=x1.cuda(), x2=x2.cuda(), dy=dy.cuda(), w=w, dw0=dw0, db0=db0, dx1=dx[..., :C], dx2=dx[..., C:], dW=wd.grad, db=bd.grad)


def check(p, dx1, dx2, dw, db, who):
    torch.cuda.synchronize()
    figs = dict(dx1=rel(dx1, p['dx1']), dx2=rel(dx2, p['dx2']), dW=rel(dw.cpu().double() - p['dw0'].double(), p['dW']),
                db=rel(db.cpu().double() - p['db0'].double(), p['db']))
    print(who, ' '.join('%s %.2e' % kv for kv in figs.items()))
    assert figs['dx1'] < DX_BOUND and figs['dx2'] < DX_BOUND, (who, figs)
    assert figs['dW'] < DW_BOUND and figs['db'] < DW_BOUND, (who, figs)


@pytest.mark.parametrize('shape,cap', [((1, 2, 2), 0),      # one partial tile
                                       ((5, 4, 4), 2),      # a partial last tile; a workgroup loops over tiles
                                       ((3, 8, 8), 1),      # three tiles on one workgroup, one slab
                                       ((9, 8, 8), 4),      # nine tiles, uneven tiles per workgroup, several slabs
                                       ((2, 16, 16), 0)])   # default grid: as many workgroups as tiles, none without a tile
def test_fused_backward_against_float64(K, shape, cap):
    p = case(*shape)
    wp = packed_weight(p['w'])
    geom = K.ConvGeom(wp, 1, 0)
    dw, db = packed_weight(p['dw0']), p['db0'].cuda()
    both = K.conv1x1_cat_bwd(p['dy'], p['x1'], p['x2'], wp, geom, dw, db, max_workgroups=cap)
    assert both is not None, "shape is meant to take the fused kernel"
    check(p, both[0], both[1], dw, db, 'fused %s' % (shape,))
    # the two launches it replaces, on the same inputs, to the same bounds
    dw, db = packed_weight(p['dw0']), p['db0'].cuda()
    K.conv2d_wgrad(p['x1'], p['dy'], wp, geom, dw, db, x2=p['x2'])
    old = K.conv1x1_dgrad_cat(p['dy'], wp, geom, C)
    assert old is not None
    check(p, old[0], old[1], dw, db, 'two launches %s' % (shape,))


def bwd_parts(dh, x, coef, rows):
    """(sum g, sum g xhat) per chunk, g = dh * elu'(x * scale + shift), as a dgrad epilogue (stats_mode LVAE_STATS_BN_BWD) writes them
    (tests/test_partial_rows_gpu.py)."""
    u = x.double() * coef[0].double() + coef[1].double()
    g = dh.double() * torch.where(u > 0, torch.ones_like(u), torch.exp(u))
    xh = (x.double() - coef[2].double()) * coef[3].double()
    parts = torch.stack([torch.stack([a.sum(0), b.sum(0)]) for a, b in zip(g.reshape(-1, C).tensor_split(rows), (g * xh).reshape(-1, C).tensor_split(rows))])
    dx = (g - g.reshape(-1, C).mean(0) - xh * (g * xh).reshape(-1, C).mean(0)) * coef[0].double()
    return parts.float().contiguous(), dx, g.reshape(-1, C).sum(0), (g * xh).reshape(-1, C).sum(0)


@pytest.mark.parametrize('store', [False, True])
@pytest.mark.parametrize('rows', [1, 3])
def test_deferred_apply_forms_dy_inside_the_launch(K, rows, store):
    """dy = BN'(dh; xbn) + add from `rows` partial rows: the gradients against float64 from that dy; dgamma / dbeta; the pending tensor holds
    dy only where the caller asks for it and is left alone otherwise."""
    N, H, W = 4, 8, 8
    g = torch.Generator().manual_seed(70 + rows)
    rn = lambda *s: torch.randn(*s, generator=g).cuda()
    xbn, dh, add, x1, x2 = (rn(N, H, W, C) for _ in range(5))
    coef = K.bn_stats(xbn, (1 + 0.1 * torch.randn(C, generator=g)).cuda(), (0.1 * torch.randn(C, generator=g)).cuda(), None, None)
    parts, dx_ref, sg, sgx = bwd_parts(dh, xbn, coef, rows)
    dy64 = dx_ref + add.double()                                     # float64, [N,H,W,C]
    w = torch.randn(C, 2 * C, 1, 1, generator=g) / (2 * C) ** 0.5
    xc = torch.cat([x1, x2], 3).permute(0, 3, 1, 2).double().cpu().requires_grad_(True)
    wd, bd = w.double().requires_grad_(True), torch.zeros(C, dtype=torch.float64, requires_grad=True)
    F.conv2d(xc, wd, bd).backward(dy64.permute(0, 3, 1, 2).cpu())
    wp = packed_weight(w)
    geom = K.ConvGeom(wp, 1, 0)
    dw0, db0 = torch.randn(C, 2 * C, 1, 1, generator=g) * 0.1, torch.randn(C, generator=g)
    dw, db = packed_weight(dw0), db0.cuda()
    dgam, dbet = torch.zeros(C, device='cuda'), torch.zeros(C, device='cuda')
    out = torch.full_like(xbn, float('nan'))
    pend = K.PendingApply(parts, dh, xbn, coef[0], 'elu', dgam, dbet, add, out)
    both = K.conv1x1_cat_bwd(out, x1, x2, wp, geom, dw, db, apply=pend, store_dy=store, max_workgroups=3)
    assert both is not None
    torch.cuda.synchronize()
    ref = nhwc(xc.grad)
    figs = dict(dx1=rel(both[0], ref[..., :C]), dx2=rel(both[1], ref[..., C:]), dW=rel(dw.cpu().double() - dw0.double(), wd.grad),
                db=rel(db.cpu().double() - db0.double(), bd.grad))
    print('deferred rows %d' % rows, ' '.join('%s %.2e' % kv for kv in figs.items()))
    assert figs['dx1'] < DX_BOUND and figs['dx2'] < DX_BOUND, figs
    assert figs['dW'] < DW_BOUND and figs['db'] < DW_BOUND, figs
    torch.testing.assert_close(dbet.double(), sg, rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(dgam.double(), sgx, rtol=1e-4, atol=1e-3)
    if store:
        assert rel(out, dy64) < 2e-6
    else:
        assert bool(torch.isnan(out).all()), "nothing may be written to the pending tensor without an out pointer"


def test_calls_that_are_not_taken_return_none_and_write_nothing(K):
    p = case(3, 8, 8)
    lib = K._C.load()
    wp = packed_weight(p['w'])
    geom = K.ConvGeom(wp, 1, 0)
    dw, db = packed_weight(p['dw0']), p['db0'].cuda()
    dw_before, db_before = dw.clone(), db.clone()
    # C1 != 64: a 32 + 96 concat
    xa, xb = torch.cat([p['x1'], p['x2']], 3).split([32, 96], 3)
    assert K.conv1x1_cat_bwd(p['dy'], xa.contiguous(), xb.contiguous(), wp, geom, dw, db) is None
    # a weight view off 16 bytes (same strides)
    buf, gbuf = torch.zeros(C * 2 * C + 4, device='cuda'), torch.zeros(C * 2 * C + 4, device='cuda')
    wmis = buf[1:1 + C * 2 * C].view(1, 1, 2 * C, C).permute(3, 2, 0, 1)
    wmis.copy_(p['w'].cuda())
    dwmis = gbuf[1:1 + C * 2 * C].view(1, 1, 2 * C, C).permute(3, 2, 0, 1)
    assert wmis.stride() == wp.stride() and wmis.data_ptr() % 16 == 4
    assert K.conv1x1_cat_bwd(p['dy'], p['x1'], p['x2'], wmis, K.ConvGeom(wmis, 1, 0), dwmis, db) is None
    assert K.cat_bwd_ws(p['dy'], wmis, K.ConvGeom(wmis, 1, 0), C) == 0 and not K.cat_bwd_apply_ok(p['dy'], wmis, K.ConvGeom(wmis, 1, 0), C)
    # a workspace one byte short: the wrapper declines, and so does the entry point itself, without a launch
    need = K.cat_bwd_ws(p['dy'], wp, geom, C)
    assert need == 3 * (2 * C * C + C) * 4
    short = torch.empty(need - 1, dtype=torch.uint8, device='cuda')
    assert K.conv1x1_cat_bwd(p['dy'], p['x1'], p['x2'], wp, geom, dw, db, scratch=short) is None
    d = K._cat_bwd_desc(p['dy'], wp, geom, C, dw)
    dx1, dx2 = torch.full_like(p['x1'], float('nan')), torch.full_like(p['x2'], float('nan'))
    rc = lib.lvae_conv1x1_cat_bwd_f32(ctypes.byref(d), p['x1'].data_ptr(), p['x2'].data_ptr(), dx1.data_ptr(), dx2.data_ptr(), dw.data_ptr(),
                                      db.data_ptr(), None, short.data_ptr(), short.numel(), 0, K.stream_ptr())
    assert rc == -3   # LVAE_EWORKSPACE
    torch.cuda.synchronize()
    assert torch.equal(dw, dw_before) and torch.equal(db, db_before) and float(gbuf.abs().max()) == 0.0
    assert bool(torch.isnan(dx1).all()) and bool(torch.isnan(dx2).all())
    # control: the same call with the full workspace is taken
    assert K.conv1x1_cat_bwd(p['dy'], p['x1'], p['x2'], wp, geom, dw, db) is not None


def run_merge_layer(K, monkeypatch, fused, freeze):
    """One MergeLayer (residual type, 64 channels, batch 4, 8x8, training) forward + backward; returns the gradients and how the fused
    entry point was called."""
    from lvae_amd import ops
    from lvae_amd.arena import ParamArena
    from lvae_amd.models.lvae_layers import MergeLayer
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.resblock import switches
    monkeypatch.setattr(switches, 'merge_bwd_fused', fused)
    monkeypatch.setattr(switches, 'merge_bwd_min_rows', 1)
    calls = []
    real = getattr(K.conv1x1_cat_bwd, 'real', K.conv1x1_cat_bwd)   # (the second run of a test patches over the first run's spy)

    def spy(*a, **kw):
        r = real(*a, **kw)
        calls.append((kw.get('apply') is not None, r is not None))
        return r
    spy.real = real
    monkeypatch.setattr(K, 'conv1x1_cat_bwd', spy)
    N, H, W = 4, 8, 8
    torch.manual_seed(11)
    net = MergeLayer(C, 'residual', nonlin='elu', batchnorm=True, dropout=0.2, res_block_type='bacdbacd').cuda().train()
    arena = ParamArena(net, torch.device('cuda'))
    arena.zero_grad()
    g = torch.Generator().manual_seed(12)
    bu = torch.randn(N, H, W, C, generator=g).cuda().requires_grad_(not freeze)
    td = torch.randn(N, H, W, C, generator=g).cuda().requires_grad_(True)
    dout = torch.randn(N, H, W, C, generator=g).cuda()
    out = net(td, bu, PhiloxNoise(seed=5))
    out.backward(dout)
    ops.flush_wgrad_group()
    torch.cuda.synchronize()
    grads = {k: q.grad.clone() for k, q in net.named_parameters()}
    return td.grad.clone(), (None if freeze else bu.grad.clone()), grads, calls


@pytest.mark.parametrize('freeze', [False, True])
def test_merge_layer_with_the_switch_on_and_off(K, monkeypatch, freeze):
    """Input gradients and every parameter gradient to 1e-5 relative, BatchNorm dgamma / dbeta to the weight-gradient bound. With both inputs
    live the block behind the merge defers its last apply into the fused launch; with the bottom-up input frozen nothing is announced, the
    fused launch is not tried and the gradients are those of the switch-off run."""
    td0, bu0, g0, calls0 = run_merge_layer(K, monkeypatch, False, freeze)
    td1, bu1, g1, calls1 = run_merge_layer(K, monkeypatch, True, freeze)
    assert calls0 == []
    assert calls1 == ([] if freeze else [(True, True)])
    assert rel(td1, td0) < 1e-5
    if not freeze:
        assert rel(bu1, bu0) < 1e-5
    assert len(g0) >= 12
    for k in g0:
        bound = DW_BOUND if g0[k].dim() == 1 else 1e-5   # the vectors: dgamma / dbeta (and the bias gradients) to the tighter bound
        assert rel(g1[k], g0[k]) < bound, (k, rel(g1[k], g0[k]))
