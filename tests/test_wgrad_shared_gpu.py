"""The Winograd-domain weight gradient with 32 input channels (conv_out of a stochastic layer, Z = 32 -> 64), and the shared launch of a
stochastic layer's two or three weight gradients (lvae_conv2d_wgrad_shared_f32): against float64, against the single launches it replaces,
run to run, and inside a whole stochastic layer. The family's floor is 16,384 pixels: 64x16x16, 256x8x8; 67x16x16 has 268 chunks, so the
shared launch's ranges are ragged and the last one is short.

Bounds: those tests/test_wgrad_pair_gpu.py holds for this kernel family over the same reduction length — 3e-6 norm-relative against
float64, 2e-6 between two summation orders (a launch that shares the chip sums each gradient over fewer partial slabs)."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

CO = 64


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


@functools.lru_cache(maxsize=None)
def problem(N, H, W, cin, prologue, seed):
    """One gradient's operands, its float64 answers (computed once, shared by the tests) and the values its buffers start from."""
    from lvae_amd import kernels as K
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s_: torch.randn(*s_, generator=g).cuda()
    p = dict(x=rn(N, H, W, cin), dy=rn(N, H, W, CO), w=packed_weight(torch.randn(CO, cin, 3, 3, generator=g) / 24), kw={})
    p['g'] = K.ConvGeom(p['w'], 1, 1)
    xin = p['x'].double()
    if prologue:   # BatchNorm + ELU on the input, applied while the kernel stages it
        coef = K.bn_stats(p['x'], torch.rand(cin, generator=g).cuda() + 0.5, rn(cin) * 0.1, None, None)
        p['kw'] = dict(in_scale=coef[0], in_shift=coef[1], in_act='elu')
        xin = elu(xin * coef[0].double() + coef[1].double())
    nchw = lambda t: t.permute(0, 3, 1, 2).double().cpu()
    p['want_w'] = torch.nn.grad.conv2d_weight(nchw(xin), (CO, cin, 3, 3), nchw(p['dy']), padding=1)
    p['want_b'] = p['dy'].double().sum((0, 1, 2)).cpu()
    p['pre_w'], p['pre_b'] = rn(CO, cin, 3, 3), rn(CO)   # the kernels accumulate: every buffer starts from values of its own
    return p


def buffers(p, bias=True):
    return torch.empty_like(p['w']).copy_(p['pre_w']), (p['pre_b'].clone() if bias else None)


def item(p, dw, db):
    return (p['x'], p['dy'], p['w'], p['g'], dw, db, p['kw'])


def check_f64(p, dw, db, tag):
    have = dw.double().cpu() - p['pre_w'].double().cpu()
    print('%s: dW against float64 %.2e' % (tag, rel(have, p['want_w'])))
    assert rel(have, p['want_w']) < 3e-6, (tag, rel(have, p['want_w']))
    if db is not None:
        have_b = db.double().cpu() - p['pre_b'].double().cpu()
        print('%s: db against float64 %.2e' % (tag, rel(have_b, p['want_b'])))
        assert rel(have_b, p['want_b']) < 3e-6, (tag, rel(have_b, p['want_b']))


def run_single(K, p, bias=True):
    dw, db = buffers(p, bias)
    K.conv2d_wgrad(p['x'], p['dy'], p['w'], p['g'], dw, db, **p['kw'])
    torch.cuda.synchronize()
    return dw, db


def run_shared(K, ps, bias=True):
    """the entry point itself, on a workspace of NaNs: every slab row the reduce reads has to have been written by the launch"""
    bufs = [buffers(p, bias) for p in ps]
    items = [item(p, dw, db) for p, (dw, db) in zip(ps, bufs)]
    descs, dys, dws, dbs = K._wgrad_item_arrays(items, 'test')
    need = K._C.load().lvae_conv2d_wgrad_shared_workspace(descs, len(ps))
    assert need > 0
    ws = torch.full((need // 4,), float('nan'), device='cuda')
    K._C.call('lvae_conv2d_wgrad_shared_f32', descs, ctypes.cast(dys, ctypes.c_void_p), ctypes.cast(dws, ctypes.c_void_p),
              ctypes.cast(dbs, ctypes.c_void_p), len(ps), ws.data_ptr(), ws.numel() * 4, K._C.stream_ptr())
    torch.cuda.synchronize()
    return bufs


def layer_problems(N, H, W, n):
    """conv_out (32 -> 64, plain input), conv_in_q (64 -> 64, here with the BatchNorm + ELU prologue) and, with n = 3, conv_in_p (plain)"""
    return [problem(N, H, W, 32, False, 11 + N), problem(N, H, W, 64, True, 12 + N), problem(N, H, W, 64, False, 13 + N)][:n]


@pytest.mark.parametrize('prologue,bias', [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize('N', [64, 67])
def test_32_input_channels_alone_against_float64(K, N, prologue, bias):
    """one problem through the entry point that takes 32 input channels (lvae_conv2d_wgrad_f32 keeps such a gradient on the tile kernel)"""
    p = problem(N, 16, 16, 32, prologue, 20 + N)
    assert K.conv2d_wgrad_shared_ok([(p['x'], p['w'], p['g'])])
    (dw, db), = run_shared(K, [p], bias)
    assert not torch.isnan(dw).any() and (db is None or not torch.isnan(db).any())
    check_f64(p, dw, db, '32 -> 64 at %dx16x16, prologue %s' % (N, prologue))
    (dw2, db2), = run_shared(K, [p], bias)
    assert torch.equal(dw2, dw) and (db is None or torch.equal(db2, db))


@pytest.mark.parametrize('n', [3, 2])
@pytest.mark.parametrize('N', [64, 67])
def test_shared_launch_matches_the_single_launches_and_float64(K, N, n):
    ps = layer_problems(N, 16, 16, n)
    assert K.conv2d_wgrad_shared_ok([(p['x'], p['w'], p['g']) for p in ps])
    got = run_shared(K, ps)
    for i, (p, (dw, db)) in enumerate(zip(ps, got)):
        tag = 'problem %d of %d at %dx16x16' % (i, n, N)
        assert not torch.isnan(dw).any() and not torch.isnan(db).any(), tag
        # its single launch: this kernel with the problem alone on the chip, and what lvae_conv2d_wgrad_f32 runs for it (the same for the
        # 64-channel problems, the tile kernel for conv_out's 32 channels)
        for what, (sw, sb) in (('alone', run_shared(K, [p])[0]), ('lvae_conv2d_wgrad_f32', run_single(K, p))):
            print('%s: against its single launch (%s) dW %.2e db %.2e' % (tag, what, rel(dw, sw), rel(db, sb)))
            assert rel(dw, sw) < 2e-6 and rel(db, sb) < 2e-6, (tag, what, rel(dw, sw), rel(db, sb))
        check_f64(p, dw, db, tag)


def test_shared_launch_is_reproducible_bit_for_bit(K):
    ps = layer_problems(67, 16, 16, 3)
    a, b = run_shared(K, ps), run_shared(K, ps)
    for (dw_a, db_a), (dw_b, db_b) in zip(a, b):
        assert torch.equal(dw_a, dw_b) and torch.equal(db_a, db_b)


def test_shared_launch_without_bias_gradients(K):
    ps = layer_problems(64, 16, 16, 3)
    for p, (dw, db) in zip(ps, run_shared(K, ps, bias=False)):
        assert db is None
        check_f64(p, dw, None, 'no bias gradient')


def test_64_channel_gradient_alone_and_in_a_group_agree_bitwise(K):
    """A 64 -> 64 gradient through the single kernel and its half-workgroup reduce (lvae_conv2d_wgrad_f32) and as a member of a grouped
    launch (the same body behind blockIdx.y, the whole-workgroup reduce): same ranges, same summation order, the same bits."""
    ps = [problem(64, 16, 16, 64, True, 31), problem(64, 16, 16, 64, False, 32)]
    bufs = [buffers(p) for p in ps]
    items = [item(p, dw, db) for p, (dw, db) in zip(ps, bufs)]
    descs = K._wgrad_item_arrays(items, 'test')[0]
    launch_of = (ctypes.c_int32 * 2)()
    assert K._C.load().lvae_conv2d_wgrad_grouped_schedule(descs, 2, launch_of) == 1   # one launch takes both
    K.conv2d_wgrad_grouped(items)
    torch.cuda.synchronize()
    for p, (dw, db) in zip(ps, bufs):
        sw, sb = run_single(K, p)
        assert torch.equal(dw, sw) and torch.equal(db, sb)
        check_f64(p, dw, db, '64 -> 64 alone')


def test_another_width_8x8(K):
    ps = layer_problems(256, 8, 8, 3)
    for i, (p, (dw, db)) in enumerate(zip(ps, run_shared(K, ps))):
        check_f64(p, dw, db, 'problem %d at 256x8x8' % i)


def test_entry_point_refuses_what_the_query_declines(K):
    ps = [problem(64, 16, 16, 32, False, 75), problem(64, 16, 16, 64, True, 76)]
    mixed = [ps[0], problem(16, 32, 32, 64, False, 41)]
    bufs = [buffers(p) for p in mixed]
    assert not K.conv2d_wgrad_shared_ok([(p['x'], p['w'], p['g']) for p in mixed])
    with pytest.raises(K._C.LvaeHipError, match='not a shared launch'):
        K.conv2d_wgrad_shared([item(p, dw, db) for p, (dw, db) in zip(mixed, bufs)])
    bufs = [buffers(p) for p in ps]
    with pytest.raises(K._C.LvaeHipError, match='accumulate into one dw'):
        K.conv2d_wgrad_shared([item(ps[1], *bufs[1]), item(ps[1], *bufs[1])])
    torch.cuda.synchronize()
    for p, (dw, db) in zip(ps, bufs):
        assert torch.equal(dw, torch.empty_like(p['w']).copy_(p['pre_w'])) and torch.equal(db, p['pre_b'])


@pytest.mark.parametrize('top', [False, True])
def test_stochastic_layer_with_and_without_the_shared_launch(K, monkeypatch, top):
    """One stochastic layer at 64x16x16, forward and backward, with the switch on and off: the layer issues its gradients as one shared
    launch of three problems (two in the top layer, which has no conv_in_p) exactly when it is on; input and parameter gradients agree."""
    from lvae_amd import ops
    from lvae_amd.arena import ParamArena
    from lvae_amd.lib.stochastic import NormalStochasticBlock2d
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.resblock import switches
    N, H, W, Z = 64, 16, 16, 32
    torch.manual_seed(8)
    blk = NormalStochasticBlock2d(64, Z, 64, transform_p_params=not top).cuda().train()
    arena = ParamArena(blk, torch.device('cuda'))   # packed weights ([KH][KW][Cin][Cout]) as in a model
    p0 = torch.randn(N, H, W, 64, device='cuda') * 0.3
    q0, dout = torch.randn(N, H, W, 64, device='cuda'), torch.randn(N, H, W, 64, device='cuda')
    calls = []
    real = K.conv2d_wgrad_shared
    monkeypatch.setattr(K, 'conv2d_wgrad_shared', lambda items: calls.append(len(items)) or real(items))
    res = []
    for on in (False, True):
        monkeypatch.setattr(switches, 'wgrad_shared', on)
        arena.zero_grad()
        p, q = p0.clone().requires_grad_(True), q0.clone().requires_grad_(True)
        out, data = blk(p, q, noise=PhiloxNoise(seed=3), need_kl_elementwise=False)
        ((out * dout).sum() + data['kl_samplewise'].sum()).backward()
        ops.flush_wgrad_group()
        torch.cuda.synchronize()
        res.append((out.detach().clone(), p.grad.clone(), q.grad.clone(), {k: v.grad.clone() for k, v in blk.named_parameters()}, list(calls)))
    (o0, dp0, dq0, g0, n0), (o1, dp1, dq1, g1, n1) = res
    assert n0 == [] and n1 == [2 if top else 3]
    assert torch.equal(o1, o0) and torch.equal(dp1, dp0) and torch.equal(dq1, dq0)
    assert len(g0) == (4 if top else 6)
    for k in g0:
        assert rel(g1[k], g0[k]) < 2e-6, (k, rel(g1[k], g0[k]))
