"""Host side of the persistent merge backward (ops.ConvFn, ops.merge_announces): who announces to the residual block behind a merge 1x1 that
its last BatchNorm apply may be left to the merge's backward, and what happens to such a pending apply when the kernel declines at backward
time. The kernels calls are stubbed (no GPU); the tensors are CPU tensors that only carry shapes and identities."""
import os
import re

import pytest
import torch

import lvae_amd  # noqa: F401
from lvae_amd import _C, kernels as K, ops, resblock as RB
from lvae_amd.lib.nn import Conv2dParams

C = 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_points_are_additions_to_abi_17():
    hdr = open(os.path.join(ROOT, 'include', 'lvae_hip.h')).read()
    assert int(re.search(r'#define LVAE_ABI_VERSION (\d+)', hdr).group(1)) == _C.ABI_VERSION == 17 == _C.load().lvae_abi_version()
    for name in ('lvae_conv1x1_cat_bwd_workspace', 'lvae_conv1x1_cat_bwd_apply_ok', 'lvae_conv1x1_cat_bwd_f32'):
        assert name in _C.SIGNATURES and re.search(r'\b%s\(' % name, hdr)
    assert RB.Switches({}).merge_bwd_fused and RB.Switches({}).merge_bwd_min_rows == 65536   # the 16x16 level at batch 256
    assert not RB.Switches({'LVAE_MERGE_BWD_FUSED': '0'}).merge_bwd_fused


def test_the_queries_decline_without_a_launch():
    """Host only: the 64 + 64 -> 64 view of any pixel count is taken, everything else is not (the pointers are never dereferenced)."""
    import ctypes
    lib = _C.load()

    def desc(**kw):
        d = _C.ConvDesc()
        d.x, d.w, d.C1, d.C2 = 1 << 32, 1 << 33, 64, 0
        d.w_sk, d.w_sn = 1, 64
        d.N, d.H, d.W, d.OH, d.OW, d.Cout = 3, 8, 8, 8, 8, 128
        d.KH = d.KW = d.stride = 1
        d.gather, d.precision = _C.GATHER_TRANSPOSED, _C.PREC_F32
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    ws = lambda d, split=64: lib.lvae_conv1x1_cat_bwd_workspace(ctypes.byref(d), split)
    assert ws(desc()) == 3 * (128 * 64 + 64) * 4 and lib.lvae_conv1x1_cat_bwd_apply_ok(ctypes.byref(desc()), 64) == 1
    assert ws(desc(N=256, H=16, W=16, OH=16, OW=16)) == 256 * (128 * 64 + 64) * 4      # one slab per workgroup, one workgroup per CU
    assert ws(desc(x=0)) == 3 * (128 * 64 + 64) * 4                                    # dy may be absent: the deferred form
    for bad in (dict(C1=32), dict(Cout=64), dict(C2=64), dict(w=(1 << 33) + 4), dict(x=(1 << 32) + 8), dict(w_sk=128, w_sn=1), dict(KH=3, KW=3),
                dict(stride=2), dict(precision=_C.PREC_BF16), dict(form=_C.FORM_F32_MFMA), dict(x_dtype=_C.DT_BF16), dict(out_scale=1 << 34),
                dict(N=0)):
        assert ws(desc(**bad)) == 0 and lib.lvae_conv1x1_cat_bwd_apply_ok(ctypes.byref(desc(**bad)), 64) == 0, bad
    assert ws(desc(), 32) == 0


@pytest.fixture
def merge(monkeypatch):
    """A 128 -> 64 1x1 convolution in training mode, its two inputs, and the stubs' call log."""
    torch.manual_seed(0)
    mod = Conv2dParams(2 * C, C, 1).train()
    x, x2 = torch.randn(2, 4, 4, C, requires_grad=True), torch.randn(2, 4, 4, C, requires_grad=True)
    log = []
    state = dict(ok=True, fused=None)
    monkeypatch.setattr(RB.switches, 'merge_bwd_fused', True)
    monkeypatch.setattr(RB.switches, 'merge_bwd_min_rows', 1)
    monkeypatch.setattr(K, 'conv2d', lambda x, w, g, **kw: torch.zeros(x.shape[:3] + (g.Cout,)))
    monkeypatch.setattr(K, 'cat_bwd_apply_ok', lambda *a, **kw: log.append('ask') or state['ok'])
    monkeypatch.setattr(K, 'conv1x1_cat_bwd', lambda *a, **kw: log.append(('fused', kw.get('apply'))) or state['fused'])
    monkeypatch.setattr(K, 'affine_act_bwd_parts', lambda *a, **kw: log.append(('apply', a, kw)))
    monkeypatch.setattr(K, 'conv1x1_dgrad_cat', lambda dy, w, g, C1: log.append('dgrad_cat') or (torch.ones(dy.shape[:3] + (C1,)), torch.ones(dy.shape[:3] + (g.Cin - C1,))))
    monkeypatch.setattr(ops, 'wgrad', lambda *a, **kw: log.append('wgrad'))
    return mod, x, x2, log, state


def test_a_merge_convolution_announces_itself_to_the_block_behind_it(merge):
    mod, x, x2, log, state = merge
    y = ops.conv(x, mod, x2=x2)
    h = y._lvae_handover
    assert h.producer is mod.sched and h.accepts == 'any-dh' and h.parts is None and h.pivot is None
    # the block that reads y takes the link exactly as it takes a producing block's (resblock.received), once
    assert RB.received(y, True)[2] == (mod.sched, 'any-dh')
    assert RB.received(y, True)[2] is None


@pytest.mark.parametrize('why', ['switch off', 'no second input', 'output activation', 'evaluation mode', 'no grad', 'frozen weight',
                                 'frozen first input', 'frozen second input', 'too few pixels', 'library declines'])
def test_who_does_not_announce(merge, monkeypatch, why):
    mod, x, x2, log, state = merge
    out_act = None
    if why == 'switch off':
        monkeypatch.setattr(RB.switches, 'merge_bwd_fused', False)
    elif why == 'no second input':
        mod, x2 = Conv2dParams(C, C, 1).train(), None
    elif why == 'output activation':
        out_act = 'elu'
    elif why == 'evaluation mode':
        mod.eval()
    elif why == 'frozen weight':
        mod.weight.requires_grad_(False)
    elif why == 'frozen first input':
        x = x.detach()
    elif why == 'frozen second input':
        x2 = x2.detach()
    elif why == 'too few pixels':
        monkeypatch.setattr(RB.switches, 'merge_bwd_min_rows', 2 * 4 * 4 + 1)
    elif why == 'library declines':
        state['ok'] = False
    monkeypatch.setattr(K, 'act_bwd_from_out', lambda dy, y, act: dy)
    with torch.set_grad_enabled(why != 'no grad'):
        y = ops.conv(x, mod, x2=x2, out_act=out_act)
    assert getattr(y, '_lvae_handover', None) is None
    assert ('ask' in log) == (why == 'library declines')   # the library is asked last, and only then


def pending_for(dy):
    block = torch.arange(4 * C, dtype=torch.float32).view(4, C)
    t = lambda: torch.zeros_like(dy)
    return K.PendingApply(torch.zeros(3, 2, C), t(), t(), block[0], 'elu', torch.zeros(C), torch.zeros(C), t(), dy), block


def test_a_stale_pending_apply_is_cleared_at_the_next_forward(merge):
    mod, x, x2, log, state = merge
    mod.sched.pending = object()
    ops.conv(x, mod, x2=x2)
    assert mod.sched.pending is None


def test_the_fused_launch_takes_the_pending_apply(merge):
    mod, x, x2, log, state = merge
    y = ops.conv(x, mod, x2=x2)
    dy = torch.empty_like(y)
    mod.sched.pending, _ = pending_for(dy)
    pend = mod.sched.pending
    state['fused'] = (torch.full_like(x, 2.0), torch.full_like(x2, 3.0))
    y.backward(dy)
    assert [e for e in log if e != 'ask'] == [('fused', pend)]          # no apply launch, no weight-gradient launch, no dgrad launch
    assert mod.sched.pending is None
    assert float(x.grad.mean()) == 2.0 and float(x2.grad.mean()) == 3.0


@pytest.mark.parametrize('why', ['kernel declines', 'side stream', 'switch off at backward'])
def test_a_pending_apply_the_kernel_does_not_take_runs_as_its_own_launch_first(merge, monkeypatch, why):
    mod, x, x2, log, state = merge
    y = ops.conv(x, mod, x2=x2)
    dy = torch.empty_like(y)
    pend, block = pending_for(dy)
    mod.sched.pending = pend
    if why == 'side stream':
        monkeypatch.setitem(ops._side, 'stream', [object()])
    elif why == 'switch off at backward':
        monkeypatch.setattr(RB.switches, 'merge_bwd_fused', False)
    y.backward(dy)
    seq = [e[0] if isinstance(e, tuple) else e for e in log if e != 'ask']
    assert seq == (['fused'] if why == 'kernel declines' else []) + ['apply', 'wgrad', 'dgrad_cat']
    a, kw = next(e for e in log if isinstance(e, tuple) and e[0] == 'apply')[1:]
    assert a[0] is pend.parts and a[1] is pend.dh and a[2] is pend.x and a[5] == 'elu'
    for got, row in zip((a[3], a[4], a[6], a[7]), block):               # scale, shift, mean, rstd: the rows of the coefficient block
        assert torch.equal(got, row)
    assert a[8] is pend.dgamma and a[9] is pend.dbeta
    assert kw['out'] is pend.out and kw['add'] is pend.add and pend.out.data_ptr() == dy.data_ptr()
    assert mod.sched.pending is None
    assert float(x.grad.mean()) == 1.0 and float(x2.grad.mean()) == 1.0   # the old path's results


def test_without_a_pending_apply_a_declining_kernel_leaves_the_old_path_unchanged(merge):
    mod, x, x2, log, state = merge
    y = ops.conv(x, mod, x2=x2)
    y.backward(torch.ones_like(y))
    assert [e[0] if isinstance(e, tuple) else e for e in log if e != 'ask'] == ['fused', 'wgrad', 'dgrad_cat']
    assert next(e for e in log if isinstance(e, tuple))[1] is None
