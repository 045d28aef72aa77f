"""The recompute form of the persistent gate backward, host side (no GPU): header, binding and library agree on its two symbols, the ABI
version stays, the query takes what it says it takes, and resblock.plan_block sets BlockPlan.recompute_ab exactly under its conditions."""
import ctypes
import os
import re
import types

import pytest
import torch

import lvae_amd  # noqa: F401
from lvae_amd import _C
from lvae_amd import kernels as K
from lvae_amd import resblock as RB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('lvae_conv1x1_gate_bwd_wgrad_recompute_ok', 'lvae_conv1x1_gate_bwd_wgrad_recompute_f32')


def test_header_binding_and_library_agree_and_the_abi_is_still_17():
    hdr = open(os.path.join(ROOT, 'include', 'lvae_hip.h')).read()
    assert int(re.search(r'#define LVAE_ABI_VERSION (\d+)', hdr).group(1)) == _C.ABI_VERSION == 17 == _C.load().lvae_abi_version()
    lib = _C.load()
    for name in NAMES:
        m = re.search(r'^(\w+) %s\(([^;]*)\);' % name, hdr, flags=re.M)
        assert m, name
        params = [q.strip() for q in m.group(2).split(',')]
        restype, argtypes = _C.SIGNATURES[name]
        assert len(params) == len(argtypes), (name, params)
        assert restype is {'int32_t': ctypes.c_int32, 'int': ctypes.c_int}[m.group(1)]
        for q, t in zip(params, argtypes):   # pointers are pointers, 64-bit integers 64-bit, on both sides
            want = ctypes.c_void_p if '*' in q else {'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'size_t': ctypes.c_size_t}[q.split()[0]]
            assert ctypes.sizeof(t) == ctypes.sizeof(want) and (('*' in q) == (t is ctypes.c_void_p or hasattr(t, 'contents'))), (name, q, t)
        assert getattr(lib, name) is not None
    assert open(os.path.join(ROOT, 'INTEGRATION.md')).read().count(NAMES[1]) >= 1


def desc(N, H, W, prec=_C.PREC_F32, form=0):
    """the 128 -> 64 dgrad view of a gate convolution, as kernels._gate_bwd_fused_desc builds it"""
    d = _C.ConvDesc()
    d.w, d.C1, d.C2, d.Cout = 1 << 33, 128, 0, 64   # aligned, never dereferenced
    d.w_stap, d.w_sk, d.w_sn = 64 * 128, 1, 128
    d.N, d.H, d.W, d.OH, d.OW = N, H, W, H, W
    d.KH = d.KW = 1
    d.stride, d.pad, d.gather, d.precision, d.form = 1, 0, _C.GATHER_TRANSPOSED, prec, form
    return d


def test_query_takes_the_fp32_six_product_form_only():
    ok = lambda d: _C.load().lvae_conv1x1_gate_bwd_wgrad_recompute_ok(ctypes.byref(d))
    for shape in [(64, 16, 16), (70, 16, 16), (17, 32, 32), (257, 8, 8), (256, 32, 32)]:
        assert ok(desc(*shape)) == 1, shape
    assert ok(desc(63, 16, 16)) == 0                              # below the persistent kernel's 16,384 pixels
    assert ok(desc(64, 16, 16, prec=_C.PREC_BF16)) == 0           # bf16 operands keep the stored form
    assert ok(desc(64, 16, 16, form=_C.FORM_F32_MFMA)) == 0       # so does the fp32-MFMA form
    for field in ('x_dtype', 'y_dtype'):
        d = desc(64, 16, 16)
        setattr(d, field, _C.DT_BF16)
        assert ok(d) == 0                                         # bf16 storage
    d = desc(64, 16, 16)
    d.Cout = 32
    assert ok(d) == 0
    # the stored form's own queries are what they were
    d = desc(64, 16, 16, prec=_C.PREC_BF16)
    assert _C.load().lvae_conv1x1_gate_bwd_wgrad_workspace(ctypes.byref(d)) == 256 * (64 * 128 + 128) * 4
    assert _C.load().lvae_conv1x1_gate_bwd_wgrad_apply_ok(ctypes.byref(d)) == 1


def test_the_switch_is_on_by_default_and_the_field_is_the_last():
    d = RB.Switches({})
    assert d.gate_recompute is True and d.gate_recompute_maxw >= 16
    s = RB.Switches({'LVAE_GATE_RECOMPUTE': '0', 'LVAE_GATE_RECOMPUTE_MAXW': '16'})
    assert (s.gate_recompute, s.gate_recompute_maxw) == (False, 16)
    assert RB.BlockPlan._fields[-1] == 'recompute_ab' and RB.BlockPlan._field_defaults == {'recompute_ab': False}


def fake_block():
    w = lambda *s: torch.zeros(*s, requires_grad=True)
    conv = lambda co, ci, k: types.SimpleNamespace(weight=w(co, ci, k, k), bias=w(co), geom=lambda: None)
    bn = lambda: types.SimpleNamespace(weight=w(64), bias=w(64), running_mean=torch.zeros(64), running_var=torch.ones(64))
    return types.SimpleNamespace(conv1=conv(64, 64, 3), conv2=conv(64, 64, 3), gate=conv(128, 64, 1), bn1=bn(), bn2=bn())


@pytest.fixture
def large_level(monkeypatch):
    """the library's answers for a 64-channel gated block of a >= 16x16 level in fp32 (no GPU: every query is patched)"""
    q = dict(rb_rows=0, resblock_bf16_storage=False, rb_gate_rows=128, gate_bwd_fused_ws=1 << 20, gate_bwd_apply_ok=True,
             conv2d_wgrad_apply_ok=False, conv2d_wgrad_pair_ok=False, gate_bwd_recompute_ok=True)
    for name in q:
        monkeypatch.setattr(K, name, lambda *a, _n=name, **kw: q[_n])
    monkeypatch.setattr(RB.switches, 'gate_recompute', True)
    monkeypatch.setattr(RB.switches, 'gate_recompute_maxw', 32)
    return q


def test_plan_block_sets_and_clears_the_flag(large_level, monkeypatch):
    q, blk = large_level, fake_block()
    x16, x32 = torch.zeros(2, 16, 16, 64), torch.zeros(2, 32, 32, 64)
    plan = RB.plan_block(blk, x16, True)
    assert (plan.forward, plan.backward, plan.bf16_internals, plan.recompute_ab) == ('wino-gate', 'persistent-gate', False, True)
    assert RB.plan_block(blk, x32, True).recompute_ab
    q['gate_bwd_recompute_ok'] = False                       # the library declines
    assert not RB.plan_block(blk, x16, True).recompute_ab
    q['gate_bwd_recompute_ok'] = True
    monkeypatch.setattr(RB.switches, 'gate_recompute', False)   # the switch
    assert not RB.plan_block(blk, x16, True).recompute_ab
    monkeypatch.setattr(RB.switches, 'gate_recompute', True)
    monkeypatch.setattr(RB.switches, 'gate_recompute_maxw', 16)  # the width cap
    assert RB.plan_block(blk, x16, True).recompute_ab and not RB.plan_block(blk, x32, True).recompute_ab
    monkeypatch.setattr(RB.switches, 'gate_recompute_maxw', 32)
    q['rb_gate_rows'] = 0                                     # per-op forward: its gate kernel stores ab
    plan = RB.plan_block(blk, x16, True)
    assert plan.forward == 'per-op' and not plan.recompute_ab
    q['rb_gate_rows'] = 128
    q['gate_bwd_fused_ws'] = 0                                # composed backward: reads ab
    plan = RB.plan_block(blk, x16, True)
    assert plan.backward == 'composed' and not plan.recompute_ab
    q['gate_bwd_fused_ws'] = 1 << 20
    with torch.no_grad():                                     # no graph: nothing is saved anyway
        plan = RB.plan_block(blk, x16, True)
    assert plan.backward is None and not plan.recompute_ab
    assert not RB.plan_block(blk, x16, False).recompute_ab    # evaluation: per-op forward
    q['rb_rows'] = 4                                          # whole-image levels keep the stored form
    assert not RB.plan_block(blk, torch.zeros(2, 8, 8, 64), True).recompute_ab
