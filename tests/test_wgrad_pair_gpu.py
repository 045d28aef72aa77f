"""The two Winograd-domain weight gradients of a residual block as one launch pair (lvae_conv2d_wgrad_pair_f32): against the two launches
it replaces (lvae_conv2d_wgrad_apply_f32 for conv1, lvae_conv2d_wgrad_f32 for conv2), against float64, run to run, at the entry point's
refusals, and inside a whole gated block."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

C = 64


@pytest.fixture(scope='module')
def K():
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels
    return kernels


def packed_weight(w):
    """the arena layout: physical [KH][KW][Cin][Cout], logical torch shape"""
    return w.permute(2, 3, 1, 0).contiguous().cuda().permute(3, 2, 0, 1)


def rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-20))


def elu(u):
    return torch.where(u > 0, u, torch.expm1(u))


def problem(K, N, H, W, rows, with_drop, seed):
    """Operands of one block's pair: conv1 on x (BatchNorm + ELU prologue) whose dy is BN2'(dh; xbn) * drop, conv2 on xbn with dy_b."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s_: torch.randn(*s_, generator=g).cuda()
    p = dict(x=rn(N, H, W, C), dh=rn(N, H, W, C), xbn=rn(N, H, W, C), dy_b=rn(N, H, W, C))
    p['w_a'], p['w_b'] = packed_weight(torch.randn(C, C, 3, 3, generator=g) / 24), packed_weight(torch.randn(C, C, 3, 3, generator=g) / 24)
    p['g_a'], p['g_b'] = K.ConvGeom(p['w_a'], 1, 1), K.ConvGeom(p['w_b'], 1, 1)
    p['coef_in'] = K.bn_stats(p['x'], None, None, None, None)
    coef = p['coef'] = K.bn_stats(p['xbn'], torch.rand(C, generator=g).cuda() + 0.5, rn(C) * 0.1, None, None)
    u = p['xbn'] * coef[0] + coef[1]
    gg = p['dh'] * torch.where(u > 0, torch.ones_like(u), torch.exp(u))
    xh = (p['xbn'] - coef[2]) * coef[3]
    p['parts'] = torch.stack([torch.stack([a.sum(0), b.sum(0)]) for a, b in
                              zip(gg.reshape(-1, C).tensor_split(rows), (gg * xh).reshape(-1, C).tensor_split(rows))]).contiguous()
    p['drop'] = ((torch.rand(N, C, generator=g) < 0.8).float() / 0.8).cuda() if with_drop else None
    # the kernels accumulate: every gradient buffer starts from values of its own
    p['pre'] = dict(dw_a=rn(C, C, 3, 3), db_a=rn(C), dw_b=rn(C, C, 3, 3), db_b=rn(C))
    return p


def buffers(p):
    b = {k: (torch.empty_like(p['w_a']).copy_(v) if v.dim() == 4 else v.clone()) for k, v in p['pre'].items()}
    b['dgamma'], b['dbeta'] = torch.full((C,), 0.5, device='cuda'), torch.full((C,), -1.0, device='cuda')
    return b


def run_pair(K, p, bn_b):
    b = buffers(p)
    out = torch.full_like(p['x'], float('nan'))
    pro_b = dict(in_scale_b=p['coef'][0], in_shift_b=p['coef'][1], in_act_b='elu') if bn_b else {}
    dy = K.conv2d_wgrad_pair(p['x'], p['w_a'], p['g_a'], b['dw_a'], b['db_a'], p['parts'], p['dh'], p['xbn'], p['coef'][0], 'elu', b['dgamma'],
                             b['dbeta'], p['dy_b'], p['w_b'], p['g_b'], b['dw_b'], b['db_b'], drop=p['drop'], in_scale=p['coef_in'][0],
                             in_shift=p['coef_in'][1], in_act='elu', out=out, **pro_b)
    assert dy is out
    torch.cuda.synchronize()
    return b, dy


def run_two(K, p, bn_b):
    b = buffers(p)
    dy = K.conv2d_wgrad_apply(p['x'], p['w_a'], p['g_a'], b['dw_a'], b['db_a'], p['parts'], p['dh'], p['xbn'], p['coef'][0], 'elu', b['dgamma'],
                              b['dbeta'], drop=p['drop'], in_scale=p['coef_in'][0], in_shift=p['coef_in'][1], in_act='elu')
    pro_b = dict(in_scale=p['coef'][0], in_shift=p['coef'][1], in_act='elu') if bn_b else {}
    K.conv2d_wgrad(p['xbn'], p['dy_b'], p['w_b'], p['g_b'], b['dw_b'], b['db_b'], **pro_b)
    torch.cuda.synchronize()
    return b, dy


# (N, H, W), Dropout2d mask, partial rows of the apply, BatchNorm + ELU prologue on conv2's input.
# 64x16x16 / 16x32x32: the family's minimum of 16,384 pixels, where the least chunks per range decide the range counts; 70, 130, 19: ragged last range
CASES = [((64, 16, 16), True, 1, True), ((70, 16, 16), False, 3, False), ((130, 16, 16), True, 256, True), ((256, 16, 16), True, 256, True),
         ((16, 32, 32), False, 3, True), ((19, 32, 32), True, 1, False)]


@pytest.mark.parametrize('shape,with_drop,rows,bn_b', CASES)
def test_pair_launch_matches_the_two_launches_it_replaces_and_float64(K, shape, with_drop, rows, bn_b):
    """Tolerances: those tests/test_kernels_gpu.py uses between two summation orders of these kernels (stored dy 1e-6, dgamma / dbeta
    rtol 1e-5 + atol 1e-4, weight and bias gradients 2e-6), and the suite's 3e-6 against float64."""
    N, H, W = shape
    p = problem(K, N, H, W, rows, with_drop, seed=N + 7 * H + rows)
    assert K.conv2d_wgrad_pair_ok(p['x'], p['w_a'], p['g_a'], p['xbn'], p['w_b'], p['g_b'])
    ref, dy_ref = run_two(K, p, bn_b)
    got, dy = run_pair(K, p, bn_b)
    assert not torch.isnan(dy).any()
    assert rel(dy.cpu(), dy_ref.cpu()) < 1e-6
    torch.testing.assert_close(got['dgamma'], ref['dgamma'], rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(got['dbeta'], ref['dbeta'], rtol=1e-5, atol=1e-4)
    for k in ('dw_a', 'db_a', 'dw_b', 'db_b'):
        assert rel(got[k].cpu(), ref[k].cpu()) < 2e-6, (k, rel(got[k].cpu(), ref[k].cpu()))
    # float64: conv2d_weight of the transformed inputs and the dy each gradient was given (A: the dy the launch stored)
    nchw = lambda t: t.permute(0, 3, 1, 2).double().cpu()
    in_a = elu(p['x'].double() * p['coef_in'][0].double() + p['coef_in'][1].double())
    in_b = elu(p['xbn'].double() * p['coef'][0].double() + p['coef'][1].double()) if bn_b else p['xbn'].double()
    for k, xin, dyk in (('a', in_a, dy), ('b', in_b, p['dy_b'])):
        want = torch.nn.grad.conv2d_weight(nchw(xin), (C, C, 3, 3), nchw(dyk), padding=1)
        have = got['dw_' + k].double().cpu() - p['pre']['dw_' + k].double().cpu()
        assert rel(have, want) < 3e-6, (k, rel(have, want))
        # the bias gradient: without a Dropout2d mask dy1 sums to zero per channel (it is a BatchNorm backward), so the error of the sum is
        # set against the magnitudes summed, not against the sum
        have_b = got['db_' + k].double().cpu() - p['pre']['db_' + k].double().cpu()
        err_b = float((have_b - dyk.double().sum((0, 1, 2)).cpu()).norm() / dyk.double().abs().sum((0, 1, 2)).cpu().norm())
        assert err_b < 3e-6, (k, err_b)
    # reproducible from run to run, bit for bit
    again, dy2 = run_pair(K, p, bn_b)
    assert torch.equal(dy2, dy)
    for k in got:
        assert torch.equal(again[k], got[k]), k


def _entry(K, p, d_a, d_b, b, out, dy_b=None, dh=None, ws=None):
    C_ = K._C
    ws = ws if ws is not None else torch.empty(64 << 20, dtype=torch.uint8, device='cuda')
    dh = p['dh'] if dh is None else dh
    ap = C_.BnApply(C_.ptr(p['parts']), p['parts'].shape[0], K.ACT['elu'], p['x'].numel() // C, C_.ptr(p['coef'][0]), C_.ptr(dh), C_.ptr(p['xbn']),
                    None, C_.ptr(b['dgamma']), C_.ptr(b['dbeta']), C_.ptr(out), 0, 0, None)
    C_.call('lvae_conv2d_wgrad_pair_f32', ctypes.byref(d_a), ctypes.byref(ap), ctypes.byref(d_b), C_.ptr(p['dy_b'] if dy_b is None else dy_b),
            C_.ptr(b['dw_a']), C_.ptr(b['db_a']), C_.ptr(b['dw_b']), C_.ptr(b['db_b']), ws.data_ptr(), ws.numel(), C_.stream_ptr())


def _untouched(p, b, out):
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    for k, v in p['pre'].items():
        assert torch.equal(b[k], v), k
    assert bool((b['dgamma'] == 0.5).all()) and bool((b['dbeta'] == -1.0).all())


def test_unaligned_operand_is_named(K):
    N, H, W = 64, 16, 16
    p = problem(K, N, H, W, 3, False, seed=5)
    d_a, d_b = K._wgrad_pair_descs(p['x'], p['w_a'], p['g_a'], p['xbn'], p['w_b'], p['g_b'])
    store = torch.zeros(p['x'].numel() + 4, device='cuda')
    off = store[1:1 + p['x'].numel()].view(N, H, W, C)
    for kw, name in ((dict(dy_b=off), 'dy_b'), (dict(dh=off), r'ap->dh')):
        b, out = buffers(p), torch.full_like(p['x'], float('nan'))
        with pytest.raises(K._C.LvaeHipError, match='%s must be 16-byte aligned' % name):
            _entry(K, p, d_a, d_b, b, out, **kw)
        _untouched(p, b, out)
    ws = torch.empty((64 << 20) + 16, dtype=torch.uint8, device='cuda')
    b, out = buffers(p), torch.full_like(p['x'], float('nan'))
    with pytest.raises(K._C.LvaeHipError, match='workspace must be 16-byte aligned'):
        _entry(K, p, d_a, d_b, b, out, ws=ws[8:])
    _untouched(p, b, out)


@pytest.mark.parametrize('why', ['bf16 storage', 'Cout != 64', 'different geometries', '8x8 image'])
def test_a_pair_the_query_declines_is_refused_without_a_launch(K, why):
    N, H, W = (256, 8, 8) if why == '8x8 image' else (64, 16, 16)
    p = problem(K, N, H, W, 3, False, seed=6)
    x_b, w_b = p['xbn'], p['w_b']
    if why == 'Cout != 64':
        w_b = packed_weight(torch.randn(128, C, 3, 3) / 24)
    if why == 'different geometries':
        x_b = torch.zeros(N + 1, H, W, C, device='cuda')
    g_b = K.ConvGeom(w_b, 1, 1)
    d_a, d_b = K._wgrad_pair_descs(p['x'], p['w_a'], p['g_a'], x_b, w_b, g_b)
    if why == 'bf16 storage':
        d_b.y_dtype = K._C.DT_BF16
    lib = K._C.load()
    assert not lib.lvae_conv2d_wgrad_pair_ok(ctypes.byref(d_a), ctypes.byref(d_b))
    assert lib.lvae_conv2d_wgrad_pair_workspace(ctypes.byref(d_a), ctypes.byref(d_b)) == 0
    if why != 'bf16 storage':
        assert not K.conv2d_wgrad_pair_ok(p['x'], p['w_a'], p['g_a'], x_b, w_b, g_b)
    b, out = buffers(p), torch.full_like(p['x'], float('nan'))
    if why == 'Cout != 64':
        b['dw_b'], b['db_b'] = torch.zeros_like(w_b), torch.zeros(128, device='cuda')
    with pytest.raises(K._C.LvaeHipError, match='not a pair'):
        _entry(K, p, d_a, d_b, b, out)
    if why == 'Cout != 64':
        assert not b['dw_b'].any() and not b['db_b'].any()
        b['dw_b'], b['db_b'] = p['pre']['dw_b'], p['pre']['db_b']
    _untouched(p, b, out)


def test_gated_block_with_and_without_the_pair(K, monkeypatch):
    """One gated 'bacdbacd' block at 64x16x16, forward and backward, with the pair switch on and off: dx and every parameter gradient."""
    from lvae_amd import ops
    from lvae_amd.arena import ParamArena
    from lvae_amd.lib.nn import ResidualGatedBlock
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.resblock import switches
    N, H, W = 64, 16, 16
    torch.manual_seed(4)
    blk = ResidualGatedBlock(C, 'elu', batchnorm=True, block_type='bacdbacd', dropout=0.2).cuda().train()
    arena = ParamArena(blk, torch.device('cuda'))   # packed weights ([KH][KW][Cin][Cout]) as in a model
    x0, dout = torch.randn(N, H, W, C, device='cuda'), torch.randn(N, H, W, C, device='cuda')
    calls = []
    real = K.conv2d_wgrad_pair
    monkeypatch.setattr(K, 'conv2d_wgrad_pair', lambda *a, **kw: calls.append(1) or real(*a, **kw))
    res = []
    state = {k: v.clone() for k, v in blk.state_dict().items()}
    for on in (False, True):
        monkeypatch.setattr(switches, 'wgrad_pair', on)
        blk.load_state_dict(state)   # the running means are the pivots of the forward's partial sums: both passes start from the same ones
        arena.zero_grad()
        x = x0.clone().requires_grad_(True)
        out = blk(x, PhiloxNoise(seed=3))
        out.backward(dout)
        ops.flush_wgrad_group()
        torch.cuda.synchronize()
        res.append((out.detach().clone(), x.grad.clone(), {k: p.grad.clone() for k, p in blk.named_parameters()}, len(calls)))
    (o0, dx0, g0, n0), (o1, dx1, g1, n1) = res
    assert (n0, n1) == (0, 1), 'the block is meant to take the pair launch exactly when the switch is on'
    assert torch.equal(o1, o0)
    assert rel(dx1, dx0) < 1e-6
    assert len(g0) >= 10
    bn = [q for m in (blk.bn1, blk.bn2) for q in (m.weight, m.bias)]
    for k, prm in blk.named_parameters():
        if any(prm is q for q in bn):   # dgamma / dbeta
            torch.testing.assert_close(g1[k], g0[k], rtol=1e-5, atol=1e-4)
        else:
            assert rel(g1[k], g0[k]) < 2e-6, (k, rel(g1[k], g0[k]))
