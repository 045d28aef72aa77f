"""Host-side schedule of the pre-activation residual block (ops.ResBlockFn): which launches one block call takes (BlockPlan, decided once
by plan_block), what travels with a block's output tensor to the next block (Handover), what a block keeps between calls (BlockState), and
the A/B switches of all of it (switches). No launch happens here; the queries go through kernels.py."""
import os
import weakref
from typing import NamedTuple, Optional

import torch

from . import kernels as K


class Switches:
    """A/B switches (profiling only; tools/*_ab.sh set them by their environment names), read once at import. Tests patch the fields."""

    def __init__(self, env):
        on = lambda name: env.get(name, '1') != '0'
        self.wgrad_flush = int(env.get('LVAE_WGRAD_FLUSH', '1024'))   # queued weight gradients per grouped launch (ops.set_wgrad_grouping)
        self.dgrad_cat = on('LVAE_DGRAD_CAT')                         # both halves of a channel concat's input gradient from one launch
        self.wgrad_apply = on('LVAE_WGRAD_APPLY')                     # conv1's weight gradient absorbs the BatchNorm-2 apply ...
        self.wgrad_apply_maxw = int(env.get('LVAE_WGRAD_APPLY_MAXW', '16'))   # ... up to this width: 32x32 measured +0.09 ms (profiles/r05_wgrad_apply_ab.txt)
        self.wgrad_pair = on('LVAE_WGRAD_PAIR')                       # ... and conv2's weight gradient rides in the same launch (kernels.conv2d_wgrad_pair) ...
        self.wgrad_pair_maxw = int(env.get('LVAE_WGRAD_PAIR_MAXW', '16'))     # ... up to this width (profiles/wgrad_pair_ab.txt)
        self.wgrad_shared = on('LVAE_WGRAD_SHARED')                   # a 16x16 stochastic layer's weight gradients go out as one launch (ops.WgradShare; profiles/wgrad_shared_ab.txt)
        self.merge_bwd_fused = on('LVAE_MERGE_BWD_FUSED')             # a merge / skip 1x1's dgrad, weight gradient and the deferred apply before them in one persistent launch ...
        self.merge_bwd_min_rows = int(env.get('LVAE_MERGE_BWD_MIN_ROWS', '65536'))   # ... from this many pixels (N*H*W) up: the 16x16 level at batch 256; below, the weight gradient rides the grouped launches (16384 measured -0.125 ms but not routed: profiles/merge_bwd_ab.txt, `routing`)
        self.gate_stats = env.get('LVAE_NO_GATE_STATS') is None      # the gate epilogue writes the next block's BatchNorm partials
        self.defer_apply = on('LVAE_DEFER_APPLY')                     # a block leaves its last BatchNorm apply to its producer (BlockPlan.accepts)
        self.defer_apply_large = on('LVAE_DEFER_APPLY_LARGE')         # ... also into the persistent gate-backward kernel of the >= 16x16 levels
        # Which blocks take the whole-image launches (measured per level at batch 256, tools/rb_bench.py: forward old -> fused 41 -> 31 us at
        # 8x8, 33 -> 26 at 4x4, 22 -> 27 at 2x2, where the position-major kernels skip the taps outside the image; backward 60 -> 43,
        # 46 -> 33, 37 -> 33): forward from 16 pixels per image up, backward everywhere the kernels exist. 0 pixels = never.
        self.rb_fwd_min_hw, self.rb_bwd_min_hw = int(env.get('LVAE_RB_FWD_MIN_HW', '16')), int(env.get('LVAE_RB_BWD_MIN_HW', '1'))
        self.rb_nsplit = int(env.get('LVAE_RB_NSPLIT', '0'))         # workgroups per tile of the whole-image plain launches (lvae_rb_ext.nsplit): 0 = the library decides (two at the 4x4 and 2x2 levels at batch 256: profiles/rb_nsplit_ab.txt), 1 = one, 2 = two wherever the kernel exists
        self.rb_gate_large = on('LVAE_RB_GATE_LARGE')                 # conv2 + gate in one launch at the >= 16x16 levels (Winograd kernel)
        self.stoch_block = on('LVAE_STOCH_BLOCK')                     # the stochastic block of the <= 8x8 levels in one forward launch (ops.StochBlockFn)
        self.stoch_block_bwd = on('LVAE_STOCH_BLOCK_BWD')             # ... and its backward in one launch
        self.gate_recompute = on('LVAE_GATE_RECOMPUTE')               # 'wino-gate' blocks do not store ab; the persistent gate backward forms it again ...
        self.gate_recompute_maxw = int(env.get('LVAE_GATE_RECOMPUTE_MAXW', '16'))   # ... up to this width: 32x32 measured -0.09 ms, inside the run-to-run range (profiles/gate_recompute_ab.txt)


switches = Switches(os.environ)


class BlockPlan(NamedTuple):
    """The launches of one block call. forward:
      'whole-image'  conv1, then conv2 + gate + residual: two launches of csrc/resblock_img.hip (low-resolution levels)
      'wino-gate'    conv1, then conv2 with the gate behind the Winograd kernel's epilogue (larger levels, fp32)
      'per-op'       one kernel per convolution, then the gate kernel;  'ungated': ... then the residual add
    backward (None: the call records no graph):
      'whole-image'      gate backward + dgrad conv2, BatchNorm-2 backward + dgrad conv1, BatchNorm-1 apply
      'persistent-gate'  gate derivative, its dgrad and weight gradient in one persistent kernel, then the two halves composed per op
      'composed'         one kernel per op throughout
    ResBlockFn.forward turns 'whole-image' into 'composed' when the BatchNorm coefficients did not come out as one block."""
    forward: str
    bf16_internals: bool        # conv outputs, gate pre-activations and their gradients stored as bf16 (block input / output stay fp32)
    gate_stats: bool            # the gate epilogue writes the BatchNorm partials of the block output (the next block's input)
    backward: Optional[str]
    wgrad_absorbs_apply: bool   # conv1's weight-gradient kernel may form the BatchNorm-2 apply itself (ResBlockFn.backward has the run-time rest)
    wgrad_pair: bool            # ... and the block's two weight gradients go out as a pair, in that launch (same run-time rest)
    accepts: Optional[str]      # deferred BatchNorm-1 apply of the NEXT block that this block's first backward launch can absorb:
                                # None | 'f32-dh' (only with an fp32 dh) | 'any-dh'. The one place that says so; tagged() publishes it.
    recompute_ab: bool = False  # the forward stores no gate pre-activations: the persistent gate backward forms them again from y2


def plan_block(blk, x, training):
    sw, grad = switches, torch.is_grad_enabled()
    cv1, cv2, gate, bn1, bn2 = blk.conv1, blk.conv2, blk.gate, blk.bn1, blk.bn2
    gated_bn = gate is not None and bn1 is not None and bn2 is not None and gate.bias is not None
    full = (training and gated_bn and cv1.bias is not None and cv2.bias is not None and bn1.running_mean is not None and
            bn2.running_mean is not None and x.dtype == torch.float32)
    hw = x.shape[1] * x.shape[2]
    whole = full and K.rb_rows(x, cv1.weight, cv1.geom()) > 0
    whole_fwd, whole_bwd = whole and 0 < sw.rb_fwd_min_hw <= hw, whole and 0 < sw.rb_bwd_min_hw <= hw
    s16 = bool(not whole_fwd and not whole_bwd and gated_bn and K.resblock_bf16_storage(x, cv1.weight, cv1.geom()))
    if whole_fwd:
        forward = 'whole-image'
    elif full and not s16 and sw.rb_gate_large and K.rb_gate_rows(x, cv2.weight, cv2.geom(), whole_image=False) > 0:
        forward = 'wino-gate'
    else:
        forward = 'per-op' if gate is not None else 'ungated'
    gate_stats = gate is not None and training and bn1 is not None and bn1.running_mean is not None and sw.gate_stats
    backward, accepts, absorbs, pair = None, None, False, False
    if grad and whole_bwd:
        backward, accepts = 'whole-image', 'f32-dh'
    elif grad:
        backward = 'composed'
        if gate is not None and gate.bias is not None and gate.weight.requires_grad and \
                K.gate_bwd_fused_ws(x, gate.weight, gate.geom(), gate.weight.grad) > 0:
            backward = 'persistent-gate'
            if training and not whole_fwd and sw.defer_apply_large and K.gate_bwd_apply_ok(x, gate.weight, gate.geom(), gate.weight.grad):   # (the whole-image forward never announced it)
                accepts = 'any-dh'
        absorbs = bool(training and bn2 is not None and sw.wgrad_apply and not s16 and cv1.weight.requires_grad and
                       x.shape[2] <= sw.wgrad_apply_maxw and K.conv2d_wgrad_apply_ok(x, cv1.weight, cv1.geom()))
        pair = bool(absorbs and sw.wgrad_pair and cv2.weight.requires_grad and x.shape[2] <= sw.wgrad_pair_maxw and
                    K.conv2d_wgrad_pair_ok(x, cv1.weight, cv1.geom(), x, cv2.weight, cv2.geom()))   # (conv2's input has conv1's output shape = x's: 64 -> 64)
    recompute = bool(forward == 'wino-gate' and backward == 'persistent-gate' and not s16 and sw.gate_recompute and
                     x.shape[2] <= sw.gate_recompute_maxw and K.gate_bwd_recompute_ok(x, gate.weight, gate.geom(), gate.weight.grad))
    return BlockPlan(forward, s16, gate_stats, backward, absorbs, pair, accepts, recompute)


class Handover(NamedTuple):
    """Travels with a block's output as the attribute `_lvae_handover` of exactly that tensor object (a view, a copy or any other tensor does
    not carry it): BatchNorm partial sums of the tensor written by the gate kernel's epilogue (kernels.StatParts) and their pivot; the
    BlockState of the producing block and what its first backward launch accepts. The partials follow aliases (passed_on); the producer
    link does not survive a fan-out and is consumed by the first block that reads it (received)."""
    parts: object
    pivot: object
    producer: object = None
    accepts: Optional[str] = None


def passed_on(src, aliases):
    h = getattr(src, '_lvae_handover', None)
    if h is not None and h.parts is not None:
        for a in aliases:
            a._lvae_handover = Handover(h.parts, h.pivot)


def received(x, training):
    """(parts, pivot, defer) for the block about to read x: the statistics partials of x (training only) and, where this block's last
    backward launch, the BatchNorm-1 apply, can be left to the block that produced x, (that block's BlockState, what it accepts)."""
    h = getattr(x, '_lvae_handover', None) or Handover(None, None)
    defer = None
    if h.producer is not None:
        x._lvae_handover = h._replace(producer=None)
        if training and torch.is_grad_enabled() and switches.defer_apply and x.dtype == torch.float32:
            defer = (h.producer, h.accepts)
    return (h.parts, h.pivot, defer) if training else (None, None, defer)


def tagged(out, blk, plan, parts, pivot):
    """Attach what the next block may use to the block output. The one function that publishes BlockPlan.accepts."""
    producer = blk.sched if (plan.accepts and blk.training and torch.is_grad_enabled()) else None
    if parts is not None or producer is not None:
        out._lvae_handover = Handover(parts, pivot, producer, plan.accepts)
    return out


class BlockState:
    """What outlives a call on the block itself (lib.nn.ResidualBlock.sched; not a parameter, a buffer or a submodule).
    pending: the kernels.BnBwdApply the consuming block's backward left for this block's first backward launch.
    first / next, per direction 'fwd' | 'bwd': the whole-image blocks of the low-resolution levels run as one dependent chain, and every launch
    streams weights of its own that are cold in the L2s. Inside a block the first launch warms the L2s for the second (kernels.rb_weight_ranges);
    ACROSS blocks the order is only known from the previous step: each block remembers which whole-image block ran right after it and what
    that block's first launch streams. Speed only: a stale link makes a launch touch bytes nobody needs; the link holds the scratch tensors
    themselves (third element of a range), so the addresses a launch — or a captured graph — touches stay allocated whatever the cache does."""
    __slots__ = ('pending', 'first', 'next', '__weakref__')

    def __init__(self):
        self.pending, self.first, self.next = None, {}, weakref.WeakValueDictionary()

    def __reduce__(self):
        return BlockState, ()   # a copied or unpickled block starts afresh

    def take_pending(self, dout):
        pend, self.pending = self.pending, None
        if pend is not None and pend.out.data_ptr() != dout.data_ptr():
            raise K._C.LvaeHipError("deferred BatchNorm-backward apply: the gradient that reached the consuming block is not the tensor the "
                                    "producer left unwritten (the block output has another consumer?)")
        return pend

    _last = weakref.WeakValueDictionary()   # direction -> the whole-image block that ran last

    def link(self, direction, first_ranges):
        """This block runs now, and its first launch streams first_ranges: tell the block that ran before it."""
        self.first[direction] = first_ranges
        prev = BlockState._last.get(direction)
        if prev is not None and prev is not self:
            prev.next[direction] = self
        BlockState._last[direction] = self

    def next_ranges(self, direction):
        nb = self.next.get(direction)
        return nb.first.get(direction) if nb is not None else None
