"""Host-side schedule of the residual block (lvae_amd/resblock.py): the hand-over rules, the per-block state and the switches, without a GPU."""
import copy
import os
import re

import torch

import lvae_amd  # noqa: F401
from lvae_amd import resblock as RB
from lvae_amd.lib.nn import ResidualGatedBlock

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'ladder-vae-pytorch_amd')


def test_partials_follow_aliases_and_the_producer_link_is_consumed_once():
    x, a, b = torch.zeros(2), torch.zeros(2), torch.zeros(2)
    producer = RB.BlockState()
    x._lvae_handover = RB.Handover('parts', 'pivot', producer, 'any-dh')
    RB.passed_on(x, (a, b))
    for t in (a, b):
        assert t._lvae_handover == RB.Handover('parts', 'pivot', None, None)   # the link does not survive a fan-out
    assert RB.received(a, True) == ('parts', 'pivot', None)
    assert RB.received(a, False) == (None, None, None)                         # partials are used in training only
    assert RB.received(x, True) == ('parts', 'pivot', (producer, 'any-dh'))
    assert RB.received(x, True) == ('parts', 'pivot', None)                    # consumed by the first block that read it
    y = torch.zeros(2)
    y._lvae_handover = RB.Handover(None, None, producer, 'f32-dh')
    with torch.no_grad():
        assert RB.received(y, True) == (None, None, None)                      # consumed even where it cannot be used
    assert y._lvae_handover.producer is None
    assert RB.received(torch.zeros(2), True) == (None, None, None)


def test_block_state_is_no_part_of_the_module():
    blk = ResidualGatedBlock(8, 'elu', batchnorm=True, block_type='bacdbacd', dropout=0.2)
    assert isinstance(blk.sched, RB.BlockState)
    assert not any('sched' in k for k in blk.state_dict()) and not any('sched' in k for k, _ in blk.named_parameters())
    assert 'sched' not in repr(blk) and 'sched' not in dict(blk.named_modules())
    blk.sched.pending = object()
    other = copy.deepcopy(blk)
    assert other.sched is not blk.sched and other.sched.pending is None


def test_cross_block_links():
    a, b = RB.BlockState(), RB.BlockState()
    a.link('fwd', ['ra'])
    b.link('fwd', ['rb'])
    assert a.next_ranges('fwd') == ['rb'] and b.next_ranges('fwd') is None and a.next_ranges('bwd') is None
    del b
    assert a.next_ranges('fwd') is None   # a link never keeps a block alive


def test_switches_keep_their_environment_names_defaults_and_polarity():
    d = RB.Switches({})
    assert (d.wgrad_flush, d.dgrad_cat, d.wgrad_apply, d.wgrad_apply_maxw, d.gate_stats, d.defer_apply, d.defer_apply_large,
            d.rb_fwd_min_hw, d.rb_bwd_min_hw, d.rb_gate_large) == (1024, True, True, 16, True, True, True, 16, 1, True)
    s = RB.Switches({'LVAE_WGRAD_FLUSH': '32', 'LVAE_DGRAD_CAT': '0', 'LVAE_WGRAD_APPLY': '0', 'LVAE_WGRAD_APPLY_MAXW': '32',
                     'LVAE_NO_GATE_STATS': '', 'LVAE_DEFER_APPLY': '0', 'LVAE_DEFER_APPLY_LARGE': '0', 'LVAE_RB_FWD_MIN_HW': '0',
                     'LVAE_RB_BWD_MIN_HW': '4', 'LVAE_RB_GATE_LARGE': '0'})
    assert (s.wgrad_flush, s.dgrad_cat, s.wgrad_apply, s.wgrad_apply_maxw, s.gate_stats, s.defer_apply, s.defer_apply_large,
            s.rb_fwd_min_hw, s.rb_bwd_min_hw, s.rb_gate_large) == (32, False, False, 32, False, False, False, 0, 4, False)


def test_no_environment_reads_or_string_keyed_block_state_left():
    read = lambda *p: open(os.path.join(PKG, *p)).read()
    assert 'environ' not in read('ops.py') and 'environ' not in read('kernels.py')
    keys = '_in_parts|_in_src|_out_parts|_accepts_deferred|_pending_apply|_rb_first_|_rb_next_|_lvae_bn_parts|_lvae_rb_src'
    for p in (('ops.py',), ('resblock.py',), ('lib', 'nn.py')):
        assert not re.search(keys, read(*p)), p
