"""The persistent gate backward WITHOUT saved pre-activations (lvae_conv1x1_gate_bwd_wgrad_recompute_f32): ab = conv1x1(y2) + bias is formed
again per tile from y2 and the forward's pre-split gate planes. Against float64 autograd at the tolerances of the stored form; bit for bit
against the stored form behind the Winograd kernel's gate epilogue (with and without a deferred apply, with non-finite values); and inside
a chain of two gated blocks."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
C = 64
NAN = float('nan')


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


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def poison(*shape):
    """leave a NaN-filled block of this size in the allocator's cache: the result tensor the next call allocates starts from NaNs"""
    t = torch.full(shape, NAN, device='cuda')
    del t


def planes(K, wp, geom, ready):
    """The forward-direction gate planes of (wp, geom) written and stamped (ready), or filled with bytes that are NaNs as bf16 and marked
    stale: the entry point then has to write them itself. Returns the ready flag a launch will see."""
    e = K.RbExt()
    K._rb_gate_ws(e, wp, geom, wp.device, False)
    if ready:
        K.prepared.prepare_all()
    else:
        K.prepared.invalidate()
        e._ws_tensor.fill_(0xff)
    e = K.RbExt()
    K._rb_gate_ws(e, wp, geom, wp.device, False)
    return int(e.gate_ws_ready)


@pytest.mark.parametrize('ready', [True, False])
@pytest.mark.parametrize('shape', [(64, 16, 16), (70, 16, 16), (17, 32, 32), (257, 8, 8)])
def test_recompute_form_against_float64_autograd(K, shape, ready):
    """16,384 pixels exactly (256 tiles), 280 tiles (some workgroups loop twice), a 32x32 level, and a pixel count ragged against the batch:
    Dropout2d row mask, non-zero gradient buffers, NaN-filled results; planes ready and not ready. Tolerances of
    test_conv1x1_gate_bwd_with_fused_weight_gradient."""
    N, H, W = shape
    g = torch.Generator().manual_seed(N + H)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64).float().double().requires_grad_(True)
    w = (torch.randn(2 * C, C, 1, 1, generator=g) / math.sqrt(C)).double().requires_grad_(True)
    b = torch.randn(2 * C, generator=g).double().requires_grad_(True)
    a_, b_ = F.conv2d(x, w, b).chunk(2, 1)
    out = F.elu(a_) * torch.sigmoid(b_)
    dout = torch.randn(out.shape, generator=g)
    mask = (torch.rand(N, C, generator=g) < 0.8).float() / 0.8
    out.backward(dout.double())
    wp = packed_weight(w.detach())
    geom = K.ConvGeom(wp, 1, 0)
    dw0, db0 = torch.randn(2 * C, C, 1, 1, generator=g) * 0.1, torch.randn(2 * C, generator=g)
    dw, db = packed_weight(dw0), db0.cuda()
    y, do = nhwc(x), nhwc(dout)
    assert K.gate_bwd_recompute_ok(y, wp, geom, dw)
    assert planes(K, wp, geom, ready) == int(ready)
    poison(N, H, W, C)
    dx = K.conv1x1_gate_bwd_wgrad_recompute(do, y, wp, geom, b.detach().float().cuda(), 'elu', dw, db, out_scale=mask.cuda())
    assert dx is not None, "shape is meant to take the recompute form"
    torch.cuda.synchronize()
    e_dx, e_dw, e_db = rel(nchw(dx), x.grad * mask.view(N, C, 1, 1)), rel(dw.cpu() - dw0, w.grad), rel(db.cpu() - db0, b.grad)
    print('recompute %s ready=%d: dx %.3g dW %.3g db %.3g' % (shape, ready, e_dx, e_dw, e_db))
    assert e_dx < 3e-6
    assert e_dw < 5e-6
    assert e_db < 5e-6


def bwd_parts(dh, x, coef, rows):
    """(sum g, sum g xhat) per chunk, g = dh * elu'(x * scale + shift), as a dgrad epilogue (stats_mode LVAE_STATS_BN_BWD) writes them"""
    u = x.double() * coef[0].double() + coef[1].double()
    g = dh.double() * torch.where(u > 0, torch.ones_like(u), torch.exp(u))
    xh = (x.double() - coef[2].double()) * coef[3].double()
    return torch.stack([torch.stack([a.sum(0), b.sum(0)]) for a, b in
                        zip(g.reshape(-1, C).tensor_split(rows), (g * xh).reshape(-1, C).tensor_split(rows))]).float().contiguous()


@pytest.fixture(scope='module', params=[(256, 16, 16), (64, 32, 32)])
def fwd_pair(K, request):
    """conv2 + gate of a block through the Winograd kernel's gate epilogue, once storing ab and once not; plus what the backward cases share"""
    N, H, W = request.param
    g = torch.Generator().manual_seed(7 * N + H)
    rn = lambda *s: torch.randn(*s, generator=g).cuda()
    p = dict(shape=(N, H, W), y1=rn(N, H, W, C), x=rn(N, H, W, C), dout=rn(N, H, W, C))
    p['w2'], p['wg'] = packed_weight(torch.randn(C, C, 3, 3, generator=g) / 24), packed_weight(torch.randn(2 * C, C, 1, 1, generator=g) / 8)
    p['ge2'], p['geg'] = K.ConvGeom(p['w2'], 1, 1), K.ConvGeom(p['wg'], 1, 0)
    p['b2'], p['bg'] = rn(C) * 0.1, rn(2 * C) * 0.5
    p['m2'] = ((torch.rand(N, C, generator=g) < 0.8).float() / 0.8).cuda()
    p['coef'] = K.bn_stats(p['y1'], torch.rand(C, generator=g).cuda() + 0.5, rn(C) * 0.1, None, None)
    p['dw0'], p['db0'] = rn(2 * C, C, 1, 1) * 0.1, rn(2 * C)
    assert K.rb_rows(p['y1'], p['w2'], p['ge2']) == 0 and K.rb_gate_rows(p['y1'], p['w2'], p['ge2']) > 0
    p['g'] = g
    return p


def forward_both(K, p, m2):
    f = lambda want: K.rb_conv_gate(p['y1'], p['w2'], p['ge2'], p['b2'], 'elu', m2, p['wg'], p['geg'], p['bg'], p['x'], 'elu', coef=p['coef'],
                                    want_ab=want)
    y2a, ab, outa, _, _ = f(True)
    y2b, none, outb, _, _ = f(False)
    assert ab is not None and none is None
    return y2a, ab, outa, y2b, outb


def backward_both(K, p, y2a, ab, y2b, dout, apply_of=None):
    """(dx, dW, db[, out, dgamma, dbeta]) of the stored and of the recompute form, from gradient buffers of equal, non-zero contents"""
    res = []
    for stored in (True, False):
        dw, db = torch.empty_like(p['wg']).copy_(p['dw0']), p['db0'].clone()
        pend = apply_of() if apply_of is not None else None
        do = pend.out if pend is not None else dout
        poison(*do.shape)
        if stored:
            dx = K.conv1x1_gate_bwd_wgrad(do, ab, y2a, p['wg'], p['geg'], 'elu', dw, db, out_scale=p['m2'], apply=pend)
        else:
            dx = K.conv1x1_gate_bwd_wgrad_recompute(do, y2b, p['wg'], p['geg'], p['bg'], 'elu', dw, db, out_scale=p['m2'], apply=pend)
        assert dx is not None
        torch.cuda.synchronize()
        res.append((dx, dw, db) + ((pend.out, pend.dgamma, pend.dbeta) if pend is not None else ()))
    return res


def test_recompute_form_is_the_stored_form_bit_for_bit(K, fwd_pair):
    p = fwd_pair
    y2a, ab, outa, y2b, outb = forward_both(K, p, p['m2'])
    torch.cuda.synchronize()
    assert same_bits(outa, outb) and same_bits(y2a, y2b)
    assert K.gate_bwd_recompute_ok(y2b, p['wg'], p['geg'])
    stored, rec = backward_both(K, p, y2a, ab, y2b, p['dout'])
    for name, a, b in zip(('dx', 'dW', 'db'), stored, rec):
        assert same_bits(a, b), name
    assert bool(torch.isfinite(rec[0]).all()) and float(rec[0].abs().max()) > 0


@pytest.mark.parametrize('rows', [1, 3, 256])
def test_recompute_form_with_a_deferred_apply_bit_for_bit(K, fwd_pair, rows):
    p = fwd_pair
    N, H, W = p['shape']
    y2a, ab, outa, y2b, outb = forward_both(K, p, p['m2'])
    g = torch.Generator().manual_seed(rows)
    rn = lambda *s: torch.randn(*s, generator=g).cuda()
    xb, dh, add = rn(N, H, W, C), rn(N, H, W, C), rn(N, H, W, C)
    coef = K.bn_stats(xb, None, None, None, None)
    parts = bwd_parts(dh, xb, coef, rows)
    mk = lambda: K.PendingApply(parts, dh, xb, coef[0], 'elu', torch.full((C,), 0.5, device='cuda'), torch.full((C,), -1.0, device='cuda'), add,
                                torch.full((N, H, W, C), NAN, device='cuda'))
    stored, rec = backward_both(K, p, y2a, ab, y2b, None, apply_of=mk)
    for name, a, b in zip(('dx', 'dW', 'db', 'ap.out', 'dgamma', 'dbeta'), stored, rec):
        assert same_bits(a, b), name
    assert bool(torch.isfinite(rec[3]).all())


def test_non_finite_values_give_the_same_bit_patterns(K, fwd_pair):
    """an inf and a NaN in y2 (through the Dropout2d mask the forward multiplies into it): both forms split, multiply and add them alike"""
    p = fwd_pair
    m2 = p['m2'].clone()
    m2[1, 5], m2[2, 40] = float('inf'), NAN
    y2a, ab, outa, y2b, outb = forward_both(K, p, m2)
    torch.cuda.synchronize()
    assert bool(torch.isinf(y2b[1, :, :, 5]).any()) and bool(torch.isnan(y2b[2, :, :, 40]).all())
    assert same_bits(outa, outb) and same_bits(y2a, y2b)
    stored, rec = backward_both(K, p, y2a, ab, y2b, p['dout'])
    for name, a, b in zip(('dx', 'dW', 'db'), stored, rec):
        assert same_bits(a, b), name
    assert bool(torch.isnan(rec[0][1]).any()) and bool(torch.isfinite(rec[0][3]).all())   # the planted images, and one beside them


def test_chain_of_two_gated_blocks_with_and_without_recompute(K, monkeypatch):
    """Two gated 'bacdbacd' blocks at 256x16x16 through ResBlockFn, eager: planned with recompute_ab, no ab saved, and dx and every
    parameter gradient equal to the run with the switch off, bit for bit."""
    from lvae_amd import ops
    from lvae_amd.arena import ParamArena
    from lvae_amd.lib.nn import ResidualGatedBlock
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.resblock import switches
    N, H, W = 256, 16, 16
    torch.manual_seed(4)
    net = torch.nn.ModuleList([ResidualGatedBlock(C, 'elu', batchnorm=True, block_type='bacdbacd', dropout=0.2) for _ in range(2)]).cuda().train()
    arena = ParamArena(net, torch.device('cuda'))   # packed weights ([KH][KW][Cin][Cout]) as in a model
    x0, dout = torch.randn(N, H, W, C, device='cuda'), torch.randn(N, H, W, C, device='cuda')
    state = {k: v.clone() for k, v in net.state_dict().items()}
    res = []
    for on in (False, True):
        monkeypatch.setattr(switches, 'gate_recompute', on)
        net.load_state_dict(state)   # the running means are the pivots of the forward's partial sums: both passes start from the same ones
        arena.zero_grad()
        x = x0.clone().requires_grad_(True)
        noise = PhiloxNoise(seed=3)
        h = net[0](x, noise)
        out = net[1](h, noise)
        nodes = [out.grad_fn, h.grad_fn]
        assert [n.plan.forward for n in nodes] == ['wino-gate'] * 2 and [n.plan.backward for n in nodes] == ['persistent-gate'] * 2
        assert [n.plan.recompute_ab for n in nodes] == [on] * 2
        assert [n.saved_tensors[3] is None for n in nodes] == [on] * 2
        out.backward(dout)
        ops.flush_wgrad_group()
        torch.cuda.synchronize()
        res.append((out.detach().clone(), x.grad.clone(), {k: q.grad.clone() for k, q in net.named_parameters()}))
    (o0, dx0, g0), (o1, dx1, g1) = res
    assert same_bits(o1, o0) and same_bits(dx1, dx0)
    assert len(g0) >= 20
    for k in g0:
        assert same_bits(g1[k], g0[k]), k
