"""Autograd glue: torch.autograd.Function wrappers whose forward AND backward are hand-written HIP launches.

torch's autograd engine is used only to order the backward calls (plumbing). Parameter gradients are written by
the wgrad / reduction kernels straight into `param.grad` (a view of the flat gradient arena, see arena.py), so the
Functions return None for parameter inputs; activations flow through autograd normally.

All activations are NHWC (N,H,W,C) contiguous float32 CUDA tensors.
"""
from types import SimpleNamespace

import torch
from torch.autograd import Function

from . import kernels as K
from . import resblock as RB

_const_cache = {}


def _ones_zeros(C, device):
    key = (C, device)
    if key not in _const_cache:
        _const_cache[key] = (torch.ones(C, device=device), torch.zeros(C, device=device))
    return _const_cache[key]


def grad_buf(p):
    """The accumulation buffer of a parameter (a view of the gradient arena once the model is packed)."""
    if not p.requires_grad:
        return None
    if p.grad is None:
        p.grad = torch.zeros_like(p)  # preserve_format keeps the arena strides
    return p.grad


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


# ----------------------------------------------------------------------------------------------------------------
# Weight-gradient kernels feed nothing but the optimiser, so they do not have to sit on the critical path of the
# backward chain: with a side stream set (engine.TrainStep does it) every wgrad launch goes there, ordered after the
# producer of dy by a stream dependency, and the main stream joins once at the end of backward. Inside a captured
# hipGraph these become parallel branches. The scratch slabs are per stream (kernels.workspace).
_side = {'stream': None}


def set_wgrad_stream(streams):
    """None, one stream, or a list of streams the weight-gradient kernels are spread over (they depend on nothing but
    their inputs, and the small layers' launches fill only a fraction of the CUs each)."""
    if streams is None:
        _side['stream'] = None
    else:
        _side['stream'] = list(streams) if isinstance(streams, (list, tuple)) else [streams]


def join_wgrad_stream():
    sts = _side['stream']
    if sts is not None:
        for st in sts:
            torch.cuda.current_stream().wait_stream(st)


def set_wgrad_grouping(max_rows, flush_at=None):
    """Queue the weight gradients of layers with at most `max_rows` pixels (N*H*W) and issue them `flush_at` at a time through
    lvae_conv2d_wgrad_grouped_f32 (None switches grouping off and flushes). The default, 1024 (RB.switches.wgrad_flush), rests on the grouped
    entry point taking 32 problems per launch and kernel kind: fuller groups of each kind were faster as far as was measured (CIFAR-15
    step: 12 -> 43.6 ms, 72 -> 42.8, 288 -> 42.4); no sweep of 1024 itself is recorded. The queued (x, dy) pairs are at most 4 MB each.
    The caller must call flush_wgrad_group() before anything reads the gradients."""
    flush_wgrad_group()
    _side['group_rows'] = max_rows
    _side['group_at'] = RB.switches.wgrad_flush if flush_at is None else flush_at


def flush_wgrad_group():
    q, _side['group_q'] = _side.get('group_q') or [], []
    if len(q) == 1:
        x, dy, w, g, dw, db, kw = q[0]
        K.conv2d_wgrad(x, dy, w, g, dw, db, **kw)
    elif q:
        K.conv2d_wgrad_grouped(q)


def drop_wgrad_group():
    """Forget the queued weight gradients WITHOUT launching them: the pass they belong to was abandoned (an exception inside a step or
    inside its capture); their inputs may be tensors of a capture that no longer exists."""
    _side['group_q'] = []


def wgrad(x, dy, w, g, dw, db, **kw):
    rows = _side.get('group_rows')
    if rows is not None and x.shape[0] * x.shape[1] * x.shape[2] <= rows:
        q = _side.setdefault('group_q', [])
        if any(e[4].data_ptr() == dw.data_ptr() for e in q):
            flush_wgrad_group()  # two gradients of one weight must not share a launch
            q = _side['group_q']
        q.append((x, dy, w, g, dw, db, kw))
        if len(q) >= _side.get('group_at', 1024):
            flush_wgrad_group()
        return
    sts = _side['stream']
    if sts is None:
        return K.conv2d_wgrad(x, dy, w, g, dw, db, **kw)
    st = sts[(dw.data_ptr() >> 8) % len(sts)]  # one weight always on the same stream: its accumulations stay ordered
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        K.conv2d_wgrad(x, dy, w, g, dw, db, **kw)
    for t in (x, dy, kw.get('x2'), kw.get('in_scale'), kw.get('in_shift')):
        if t is not None:
            t.record_stream(st)  # the caching allocator must not recycle these blocks before the side kernel ran


class WgradShare:
    """The weight gradients of one stochastic layer call (lib/stochastic.py: conv_out, conv_in_q and, below the top layer, conv_in_p), which
    are independent of each other and of the backward chain: each convolution's backward node hands its (x, dy) in instead of launching,
    and the arrival of the last input convolution issues all of them as one shared launch (kernels.conv2d_wgrad_shared). conv_out's node
    runs first if it runs at all and the core's backward feeds both input convolutions, so waiting for those covers every order autograd
    takes; what has arrived when they have is issued, alone or through wgrad() where the launch declines (a side stream, bf16 operands)."""

    def __init__(self, n_in):
        self.items, self.wait = [], n_in

    @staticmethod
    def plan(convs):
        """A WgradShare for these (x, Conv2dParams) calls — the input convolutions first, conv_out last — where the library shares their
        gradients' launch (fp32, one N, H, W of the Winograd family: the 16x16 level at batch 256), else None."""
        if not (RB.switches.wgrad_shared and torch.is_grad_enabled() and all(m.weight.requires_grad for _, m in convs)):
            return None
        if not K.conv2d_wgrad_shared_ok([(x, m.weight, m.geom()) for x, m in convs], routed=True):
            return None
        return WgradShare(len(convs) - 1)

    def add(self, item, is_input):
        self.items.append(item)
        self.wait -= int(is_input)
        if self.wait > 0:
            return
        items, self.items = self.items, []
        if (len(items) >= 2 and _side['stream'] is None and all(it[1].dtype == torch.float32 for it in items) and
                K.conv2d_wgrad_shared_ok([(it[0], it[2], it[3]) for it in items])):
            K.conv2d_wgrad_shared(items)
        else:
            for x, dy, w, g, dw, db, kw in items:
                wgrad(x, dy, w, g, dw, db, **kw)


# ----------------------------------------------------------------------------------------------------------------
class ConvFn(Function):
    """y = out_act(conv(cat(x, x2)) + bias); call sites: stem, pre_conv (strided / transposed), merge 1x1,
    stochastic convs, likelihood head. `mod` is the parameter holder (lib.nn.Conv2dParams). share: None, or (WgradShare, is an input
    convolution of its layer): the weight gradient goes out with the layer's others."""

    @staticmethod
    def forward(ctx, x, x2, mod, out_act, weight, bias, share=None):
        g = mod.geom()
        y = K.conv2d(x, weight, g, bias=bias, x2=x2, out_act=out_act)
        ctx.mod, ctx.out_act, ctx.g, ctx.share = mod, out_act, g, share
        ctx.has_x2 = x2 is not None
        ctx.save_for_backward(x, x2, y if out_act else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, x2, y = ctx.saved_tensors
        mod, g = ctx.mod, ctx.g
        dy = _c(dy)
        w = mod.weight
        if x2 is not None:
            # merge / skip 1x1: dgrad of both halves and the weight gradient in one persistent launch, which also forms a dy that the
            # residual block behind the merge left as a BnBwdApply (merge_announces); anything it does not take goes the old way
            st = getattr(mod, 'sched', None)
            pend = st.take_pending(dy) if st is not None else None
            if (RB.switches.merge_bwd_fused and not ctx.out_act and w.requires_grad and ctx.needs_input_grad[0] and ctx.needs_input_grad[1] and
                    _side['stream'] is None and dy.dtype == torch.float32 and
                    dy.shape[0] * dy.shape[1] * dy.shape[2] >= RB.switches.merge_bwd_min_rows):
                both = K.conv1x1_cat_bwd(dy, x, x2, w, g, grad_buf(w), grad_buf(mod.bias) if mod.bias is not None else None, apply=pend)
                if both is not None:
                    return both + (None,) * 5
            if pend is not None:   # never dropped: the apply the block did not launch runs here, into the tensor the block returned
                pend.run()
        if ctx.out_act:
            dy = K.act_bwd_from_out(dy, y, ctx.out_act)
        if w.requires_grad:
            db = grad_buf(mod.bias) if mod.bias is not None else None
            if ctx.share is not None and x2 is None:
                ctx.share[0].add((x, dy, w, g, grad_buf(w), db, {}), ctx.share[1])
            else:
                wgrad(x, dy, w, g, grad_buf(w), db, x2=x2)
        dx = dx2 = None
        hw = (x.shape[1], x.shape[2])
        if x2 is None:
            if ctx.needs_input_grad[0]:
                dx = K.conv2d_dgrad(dy, w, g, hw)
        else:
            C1 = x.shape[3]
            both = K.conv1x1_dgrad_cat(dy, w, g, C1) if (RB.switches.dgrad_cat and ctx.needs_input_grad[0] and ctx.needs_input_grad[1]) else None
            if both is not None:
                dx, dx2 = both   # merge / skip 1x1: both halves of the channel concat from one launch
            else:
                if ctx.needs_input_grad[0]:
                    dx = K.conv2d_dgrad(dy, w, g, hw, ci_range=(0, C1))
                if ctx.needs_input_grad[1]:
                    dx2 = K.conv2d_dgrad(dy, w, g, hw, ci_range=(C1, g.Cin))
        return dx, dx2, None, None, None, None, None


def merge_announces(x, x2, mod, y, out_act):
    """True when the backward of this convolution over the concat (x, x2) with output y will be the persistent merge backward and can form
    its own dy: the residual block that reads y may then leave its last BatchNorm apply to it (RB.Handover, as between two blocks)."""
    sw = RB.switches
    if not (sw.merge_bwd_fused and x2 is not None and out_act is None and mod.training and torch.is_grad_enabled()):
        return False
    if not (mod.weight.requires_grad and x.requires_grad and x2.requires_grad and y.dtype == torch.float32):
        return False
    if y.shape[0] * y.shape[1] * y.shape[2] < sw.merge_bwd_min_rows:
        return False
    return K.cat_bwd_apply_ok(y, mod.weight, mod.geom(), x.shape[3], mod.weight.grad)


def conv(x, mod, x2=None, out_act=None, share=None):
    st = getattr(mod, 'sched', None)
    if st is not None:
        st.pending = None   # (left behind by a backward pass that was abandoned)
    y = ConvFn.apply(x, x2, mod, out_act, mod.weight, mod.bias, share)
    if st is not None and merge_announces(x, x2, mod, y, out_act):
        y._lvae_handover = RB.Handover(None, None, st, 'any-dh')
    return y


# ----------------------------------------------------------------------------------------------------------------
def _bn_of_half(h, bn, training, parts, pivot):
    """BatchNorm coefficients of one half of a block as (in_bn, coef), exactly one of them set: in_bn = (parts, pivot, bn) where the kernel
    that produced h left partial sums (the convolution that reads h finalizes them: kernels.conv2d), else coef = (scale, shift, mean | None,
    rstd | None) from a statistics pass, the running statistics, or the identity."""
    if bn is None:
        return None, _ones_zeros(h.shape[3], h.device) + (None, None)
    if not training:
        return None, K.bn_eval_coeffs(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps) + (None, None)
    if parts is not None:
        return (parts, pivot, bn), None
    return None, K.bn_stats(h, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, bn.momentum)


def _conv_half(h, bn, cv, act, m, training, parts, pivot, stats_pivot, s16):
    """One half as its own launch: y = (conv(act(bn(h))) + bias) * m, BatchNorm-apply + act fused in the A-operand load, with the partial sums
    of y around stats_pivot where asked for and the kernel has that epilogue. Returns (y, parts | None, coef)."""
    in_bn, coef = _bn_of_half(h, bn, training, parts, pivot)
    if in_bn is not None:
        return K.conv2d(h, cv.weight, cv.geom(), bias=cv.bias, in_act=act, out_scale=m, in_bn=in_bn, stats_pivot=stats_pivot, out_bf16=s16)
    r = K.conv2d(h, cv.weight, cv.geom(), bias=cv.bias, in_scale=coef[0], in_shift=coef[1], in_act=act, out_scale=m, stats_pivot=stats_pivot,
                 out_bf16=s16)
    return (r if stats_pivot is not None else (r, None)) + (coef,)


def _fwd_fused_gate(call, x, blk, m1, m2, training):
    """conv1 (+ BatchNorm-2 partial sums), then conv2 + gate + residual (+ the next block's BatchNorm partial sums) in ONE launch.
    'whole-image': both are launches of csrc/resblock_img.hip, each warming the L2s with the weights of the launch after it;
    'wino-gate': conv1 as its own convolution, the gate behind the Winograd kernel's epilogue (conv3x3_wino.hip)."""
    act, st, bn2, cv1, cv2, gate = blk.act, blk.sched, blk.bn2, blk.conv1, blk.conv2, blk.gate
    whole = call.plan.forward == 'whole-image'
    if whole:
        in_bn, coef1 = _bn_of_half(x, blk.bn1, True, call.parts, call.pivot)
        st.link('fwd', K.rb_weight_ranges(x, cv1.weight, cv1.geom(), False))
        y1, parts2, coef1 = K.rb_conv(x, cv1.weight, cv1.geom(), cv1.bias, act, m1, in_bn=in_bn, coef=coef1, stats_pivot=bn2.running_mean,
                                      prefetch=K.rb_weight_ranges(x, cv2.weight, cv2.geom(), False, gate=(gate.weight, gate.geom())),
                                      nsplit=RB.switches.rb_nsplit)
    else:
        y1, parts2, coef1 = _conv_half(x, blk.bn1, cv1, act, m1, True, call.parts, call.pivot, bn2.running_mean, False)
    in_bn, coef2 = _bn_of_half(y1, bn2, True, parts2, bn2.running_mean)
    call.out_pivot = coef1[2].detach() if call.plan.gate_stats else None   # this block's own batch mean: inside the data range of the residual stream
    y2, ab, out, call.out_parts, coef2 = K.rb_conv_gate(y1, cv2.weight, cv2.geom(), cv2.bias, act, m2, gate.weight, gate.geom(), gate.bias, x, act,
                                                        in_bn=in_bn, coef=coef2, stats_pivot=call.out_pivot,
                                                        prefetch=st.next_ranges('fwd') if whole else None,
                                                        want_ab=not call.plan.recompute_ab)
    return y1, y2, ab, out, coef1, coef2


def _fwd_per_op(call, x, blk, m1, m2, training):
    """One launch per convolution (conv1's epilogue writes BatchNorm 2's partial sums), then the gate kernel or the residual add."""
    act, bn2, gate, s16 = blk.act, blk.bn2, blk.gate, call.plan.bf16_internals
    want_stats = training and bn2 is not None and bn2.running_mean is not None
    y1, parts2, coef1 = _conv_half(x, blk.bn1, blk.conv1, act, m1, training, call.parts, call.pivot, bn2.running_mean if want_stats else None, s16)
    y2, _, coef2 = _conv_half(y1, bn2, blk.conv2, act, m2, training, parts2, bn2.running_mean if bn2 is not None else None, None, s16)
    if gate is None:
        return y1, y2, None, K.add(y2, x), coef1, coef2
    # the block output is (usually) the next block's BatchNorm input: statistics in the gate epilogue, around this block's own batch mean
    call.out_pivot = coef1[2].detach() if call.plan.gate_stats else None
    r = K.conv1x1_gate(y2, gate.weight, gate.geom(), gate.bias, x, act, stats_pivot=call.out_pivot)
    ab, out, call.out_parts = r if call.out_pivot is not None else r + (None,)
    return y1, y2, ab, out, coef1, coef2


# The last launch of a residual block's backward is the BatchNorm-1 apply, dx = BN1'(dh1; x) + dout. When the tensor x is exactly the output
# of the previous residual block of the chain (resblock.Handover) and that block's backward starts with a kernel that can form its `dout`
# itself (BlockPlan.accepts), the apply is not launched: the block returns an unwritten dx and leaves a kernels.BnBwdApply with the producer,
# whose first backward launch computes dx in its prologue and stores it there. This assumes what loss.backward() does: the backward pass goes on
# through the producing block (torch.autograd.grad w.r.t. a tensor BETWEEN two such blocks would get the unwritten dx). LVAE_DEFER_APPLY=0: never.
class ResBlockFn(Function):
    """Whole pre-activation residual block ('bacdbacd' / 'bacdbac' recipes of lib/nn.py:64-89, with or without
    BatchNorm, Dropout2d and the gate) as ONE autograd node, run as its resblock.BlockPlan says:

        y1 = drop1(conv1(act(bn1(x))))
        y2 = drop2(conv2(act(bn2(y1))))
        out = gate(conv1x1(y2)) + x      or  y2 + x
    Saved for backward: x, y1, y2, ab and the BN coefficients; act(bn(.)) is recomputed inside the wgrad loader. With plan.recompute_ab
    (fp32 'wino-gate' blocks with the persistent gate backward) ab is neither stored nor saved (None): that backward kernel forms it again
    from y2, bit for bit as the forward did."""

    @staticmethod
    def forward(ctx, x, blk, m1, m2, training, call, *params):
        plan, fwd = call.plan, _fwd_fused_gate if call.plan.forward in ('whole-image', 'wino-gate') else _fwd_per_op
        y1, y2, ab, out, coef1, coef2 = fwd(call, x, blk, m1, m2, training)
        if plan.backward == 'whole-image' and not (K.bn_coef_block(*coef1) and K.bn_coef_block(*coef2)):
            call.plan = plan = plan._replace(backward='composed', accepts=None)
        ctx.blk, ctx.plan, ctx.training, ctx.defer = blk, plan, training, call.defer
        ctx.save_for_backward(x, y1, y2, ab, *coef1, *coef2, m1, m2)
        return out

    @staticmethod
    def backward(ctx, dout):
        blk, plan, act = ctx.blk, ctx.plan, ctx.blk.act
        x, y1, y2, ab, sc1, sh1, mean1, rstd1, sc2, sh2, mean2, rstd2, m1, m2 = ctx.saved_tensors
        coef1, coef2 = (sc1, sh1, mean1, rstd1), (sc2, sh2, mean2, rstd2)
        dout = _c(dout)
        if plan.backward == 'whole-image':
            dh1, parts1 = _bwd_whole_image(blk, dout, x, y1, y2, ab, coef1, coef2, m1, m2)
        else:
            dy2 = _bwd_gate(blk, plan, dout, y2, ab, m2)
            cv1, bn2 = blk.conv1, blk.bn2
            cv2 = blk.conv2
            # the pair: conv2's weight gradient waits for conv1's launch (nothing reads it before the end of the block)
            paired = (plan.wgrad_pair and _side['stream'] is None and dy2.dtype == torch.float32 and bn2 is not None and ctx.training and
                      K.bn_coef_block(*coef2))
            dh2, parts2 = _bwd_half(ctx, cv2, bn2, y1, dy2, coef2, wgrad_done=paired)
            absorbed = (plan.wgrad_absorbs_apply and parts2 is not None and _side['stream'] is None and dh2.dtype == torch.float32)
            apply2 = K.BnBwdApply(parts2, dh2, y1, coef2, act, grad_buf(bn2.weight), grad_buf(bn2.bias), drop=m1) if absorbed else None
            if paired and absorbed:
                dy1 = K.conv2d_wgrad_pair(x, cv1.weight, cv1.geom(), grad_buf(cv1.weight), grad_buf(cv1.bias), apply2, dy2, cv2.weight, cv2.geom(),
                                          grad_buf(cv2.weight), grad_buf(cv2.bias), in_scale=sc1, in_shift=sh1, in_act=act, in_scale_b=sc2,
                                          in_shift_b=sh2, in_act_b=act)
            elif absorbed:
                # >= 16x16 levels (fp32): the BatchNorm-2 apply runs inside conv1's weight-gradient kernel, which needs its result as an operand
                # anyway (and stores it for the dgrad below): one launch, its finalize and one tensor pass less
                dy1 = K.conv2d_wgrad_apply(x, cv1.weight, cv1.geom(), grad_buf(cv1.weight), grad_buf(cv1.bias), apply2, in_scale=sc1, in_shift=sh1,
                                           in_act=act)
            else:
                if paired:   # the dgrad left no partial sums after all: conv2's gradient as a launch of its own, late
                    wgrad(y1, dy2, cv2.weight, cv2.geom(), grad_buf(cv2.weight), grad_buf(cv2.bias), in_scale=sc2, in_shift=sh2, in_act=act)
                dy1 = _bwd_apply(ctx, bn2, parts2, dh2, y1, coef2, drop=m1, out_bf16=plan.bf16_internals)
            dh1, parts1 = _bwd_half(ctx, cv1, blk.bn1, x, dy1, coef1, wgrad_done=absorbed)
        if parts1 is not None and ctx.defer is not None and (dh1.dtype == torch.float32 or ctx.defer[1] == 'any-dh') and K.bn_coef_block(*coef1):
            dx = torch.empty_like(x)   # left to the first backward launch of the block that produced x
            ctx.defer[0].pending = K.BnBwdApply(parts1, dh1, x, coef1, act, grad_buf(blk.bn1.weight), grad_buf(blk.bn1.bias), add=dout, out=dx)
        else:
            dx = _bwd_apply(ctx, blk.bn1, parts1, dh1, x, coef1, add=dout)
        return (dx, None, None, None, None, None) + (None,) * (len(ctx.needs_input_grad) - 6)


def _bwd_whole_image(blk, dout, x, y1, y2, ab, coef1, coef2, m1, m2):
    """Low-resolution levels: gate backward + dgrad conv2, then BatchNorm-2 backward + dgrad conv1. Returns (dh1, its partial sums)."""
    act, st, gate, cv2, cv1, bn2 = blk.act, blk.sched, blk.gate, blk.conv2, blk.conv1, blk.bn2
    gw, w2, w1 = gate.weight, cv2.weight, cv1.weight
    st.link('bwd', K.rb_weight_ranges(dout, w2, cv2.geom(), True, gate=(gw, gate.geom()), gate_bwd=True))
    dab, dy2, dh2, parts2 = K.rb_gate_dgrad(dout, ab, gw, gate.geom(), act, m2, w2, cv2.geom(), bn_bwd=(y1, coef2[0], act),
                                            prefetch=K.rb_weight_ranges(dout, w1, cv1.geom(), True), apply=st.take_pending(dout),
                                            nsplit=RB.switches.rb_nsplit)
    if gw.requires_grad:
        wgrad(y2, dab, gw, gate.geom(), grad_buf(gw), grad_buf(gate.bias))
    wgrad(y1, dy2, w2, cv2.geom(), grad_buf(w2), grad_buf(cv2.bias), in_scale=coef2[0], in_shift=coef2[1], in_act=act)
    dy1, dh1, parts1 = K.rb_apply_dgrad(K.BnBwdApply(parts2, dh2, y1, coef2, act, grad_buf(bn2.weight), grad_buf(bn2.bias), drop=m1), w1, cv1.geom(),
                                        bn_bwd=(x, coef1[0], act), prefetch=st.next_ranges('bwd'), nsplit=RB.switches.rb_nsplit)
    wgrad(x, dy1, w1, cv1.geom(), grad_buf(w1), grad_buf(cv1.bias), in_scale=coef1[0], in_shift=coef1[1], in_act=act)
    return dh1, parts1


def _bwd_gate(blk, plan, dout, y2, ab, m2):
    """dy2, the gradient w.r.t. conv2's output, from dout through the gate (or the residual add)."""
    gate, act, s16 = blk.gate, blk.act, plan.bf16_internals   # (bf16-stored internals: every launch has to take the bf16-storage kernel)
    if gate is None:
        return K.scale_rows_add(dout, m2, None) if m2 is not None else dout
    gw = gate.weight
    if plan.backward == 'persistent-gate':
        # large levels: gate derivative, dgrad and the gate convolution's weight gradient in one persistent kernel
        if plan.recompute_ab:
            dy2 = K.conv1x1_gate_bwd_wgrad_recompute(dout, y2, gw, gate.geom(), gate.bias, act, grad_buf(gw), grad_buf(gate.bias), out_scale=m2,
                                                     apply=blk.sched.take_pending(dout))
        else:
            dy2 = K.conv1x1_gate_bwd_wgrad(dout, ab, y2, gw, gate.geom(), act, grad_buf(gw), grad_buf(gate.bias), out_scale=m2, out_bf16=s16,
                                           apply=blk.sched.take_pending(dout))
        if dy2 is None:
            raise K._C.LvaeHipError("residual block: the persistent gate backward the block was planned with did not take this shape")
        return dy2
    if s16:
        raise K._C.LvaeHipError("bf16-stored residual block: the fused gate backward did not take this shape")
    dab, dy2 = K.conv1x1_gate_bwd(dout, ab, gw, gate.geom(), act, out_scale=m2)
    wgrad(y2, dab, gw, gate.geom(), grad_buf(gw), grad_buf(gate.bias))
    return dy2


def _bwd_half(ctx, cv, bn, h, dy, coef, wgrad_done=False):
    """Weight gradient and dgrad of one half's convolution y = conv(act(bn(h))): returns (dh, parts) with dh the gradient w.r.t. act(bn(h))
    and parts the BatchNorm-backward sums where the dgrad kernel's epilogue wrote them (None: a reduction pass has to)."""
    w, g, act = cv.weight, cv.geom(), ctx.blk.act
    if not wgrad_done:
        wgrad(h, dy, w, g, grad_buf(w), grad_buf(cv.bias), in_scale=coef[0], in_shift=coef[1], in_act=act)
    if bn is not None and ctx.training and K.bn_coef_block(*coef):
        return K.conv2d_dgrad(dy, w, g, h.shape[1:3], bn_bwd=(h, coef[0], act), out_bf16=ctx.plan.bf16_internals)
    return K.conv2d_dgrad(dy, w, g, h.shape[1:3]), None


def _bwd_apply(ctx, bn, parts, dh, h, coef, drop=None, add=None, out_bf16=False):
    """Gradient through act(bn(h)); drop: the producer's Dropout2d mask, add: the residual gradient; parts: the reduction is done already."""
    sc, sh, mean, rstd = coef
    train = bn is not None and ctx.training
    dgamma, dbeta = (grad_buf(bn.weight), grad_buf(bn.bias)) if train else (None, None)
    if parts is not None:
        return K.BnBwdApply(parts, dh, h, coef, ctx.blk.act, dgamma, dbeta, add=add, drop=drop).run(out_bf16=out_bf16)
    return K.affine_act_bwd(dh, h, sc, sh, ctx.blk.act, train, mean, rstd, dgamma, dbeta, drop=drop, add=add)


def residual_block(x, blk, m1, m2):
    """`call`: what the node is told beside its tensors (the plan; what came with x) and reports back (the plan as run; the output's partials)."""
    training = blk.training
    blk.sched.pending = None   # (left behind by a backward pass that was abandoned)
    parts, pivot, defer = RB.received(x, training)
    call = SimpleNamespace(plan=RB.plan_block(blk, x, training), parts=parts, pivot=pivot, defer=defer, out_parts=None, out_pivot=None)
    out = ResBlockFn.apply(x, blk, m1, m2, training, call, *blk.parameters())
    return RB.tagged(out, blk, call.plan, call.out_parts, call.out_pivot)


# ----------------------------------------------------------------------------------------------------------------
# small nodes used by the non-fused 'cabdcabd' recipe (lib/nn.py:50-62)
class BnDropFn(Function):
    """y = BN(x) * mask[n, c] materialised (BatchNorm after the activation, then Dropout2d)."""

    @staticmethod
    def forward(ctx, x, bn, mask, training, *params):
        _, (sc, sh, mean, rstd) = _bn_of_half(x, bn, training, None, None)
        y = K.affine_act(x, sc, sh, None, row_scale=mask)
        ctx.bn, ctx.training = bn, training
        ctx.save_for_backward(x, sc, sh, mean, rstd, mask)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, sc, sh, mean, rstd, mask = ctx.saved_tensors
        dy = _c(dy)
        if mask is not None:
            dy = K.scale_rows_add(dy, mask, None)
        bn = ctx.bn
        train = bn is not None and ctx.training
        dx = K.affine_act_bwd(dy, x, sc, sh, None, train, mean, rstd, grad_buf(bn.weight) if train else None,
                              grad_buf(bn.bias) if train else None)
        return (dx, None, None, None) + (None,) * (len(ctx.needs_input_grad) - 4)


class GateFn(Function):
    """out = act(a) * sigmoid(b) [+ res] from ab = conv1x1 output (lib/nn.py:121-126)."""

    @staticmethod
    def forward(ctx, ab, res, act):
        ctx.act = act
        ctx.has_res = res is not None
        ctx.save_for_backward(ab)
        return K.gate_fwd(ab, res, act)

    @staticmethod
    def backward(ctx, dout):
        (ab,) = ctx.saved_tensors
        dout = _c(dout)
        return K.gate_bwd(dout, ab, ctx.act), (dout if ctx.has_res else None), None


class AddFn(Function):
    @staticmethod
    def forward(ctx, a, b):
        return K.add(a, b)

    @staticmethod
    def backward(ctx, d):
        return d, d


# ----------------------------------------------------------------------------------------------------------------
def _batch_sum_like(t, d):
    """The gradient of an operand t (1, ...) that was broadcast over the batch: the per-sample gradient d (N, ...) summed over N."""
    red = torch.empty_like(t)
    K.colsum(d.view(d.shape[0], -1), red.view(-1), False)
    return red


class NormalStochFn(Function):
    """lib/stochastic.py:45-99 elementwise core. Returns z, logprob_p, logprob_q, kl_samplewise, kl_spatial."""

    @staticmethod
    def forward(ctx, p, q, noise, mode, analytical, Z, N, rows=None):
        z, lp, lq, kl, ks = K.normal_stochastic_fwd(p, q, noise, mode, analytical, Z, N, rows=rows)
        ctx.set_materialize_grads(False)  # unused outputs arrive as None (the kernel takes NULL) instead of zero-filled tensors
        ctx.mode, ctx.analytical, ctx.Z = mode, analytical, Z
        ctx.has_q = q is not None
        ctx.p_bcast = p.shape[0] == 1 and N > 1
        ctx.save_for_backward(p, q, noise if mode == 0 else None, z)
        if q is None:
            return z, lp
        return z, lp, lq, kl, ks

    @staticmethod
    def backward(ctx, dz, g_lp, g_lq=None, g_kl=None, g_ks=None):
        p, q, eps, z = ctx.saved_tensors
        cc = lambda t: None if t is None else _c(t)
        if dz is None and g_lp is None and g_lq is None and g_kl is None and g_ks is None:
            return None, None, None, None, None, None, None, None
        dp, dq = K.normal_stochastic_bwd(p, q, eps, z, cc(dz), cc(g_lp), cc(g_lq), cc(g_kl), cc(g_ks), ctx.mode,
                                         ctx.analytical, ctx.Z)
        return (_batch_sum_like(p, dp) if ctx.p_bcast else dp), dq, None, None, None, None, None, None


class NormalStochResFn(Function):
    """NormalStochFn with the posterior given as an offset from the prior, d = (dmu | dlv) in place of q (csrc/stochastic_residual.hip).
    Returns z, logprob_p, logprob_q, kl_samplewise, kl_spatial, q_out; q_out = p + d is None with need_q=False and carries no gradient
    (it serves the readers of absolute posterior parameters). The backward returns dp, the total gradient of the prior parameters, and dd."""

    @staticmethod
    def forward(ctx, p, d, noise, mode, analytical, Z, N, rows=None, need_q=True):
        z, lp, lq, kl, ks, q_out = K.normal_stochastic_res_fwd(p, d, noise, mode, analytical, Z, N, rows=rows, need_q=need_q)
        ctx.set_materialize_grads(False)  # unused outputs arrive as None (the kernel takes NULL) instead of zero-filled tensors
        ctx.mode, ctx.analytical, ctx.Z = mode, analytical, Z
        ctx.p_bcast = p.shape[0] == 1 and N > 1
        ctx.save_for_backward(p, d, noise if mode == 0 else None, z if mode == 2 else None)
        if q_out is not None:
            ctx.mark_non_differentiable(q_out)
        return z, lp, lq, kl, ks, q_out

    @staticmethod
    def backward(ctx, dz, g_lp, g_lq=None, g_kl=None, g_ks=None, g_q=None):
        p, d, eps, z = ctx.saved_tensors
        cc = lambda t: None if t is None else _c(t)
        if dz is None and g_lp is None and g_lq is None and g_kl is None and g_ks is None:
            return (None,) * 9
        dp, dd = K.normal_stochastic_res_bwd(p, d, eps, z, cc(dz), cc(g_lp), cc(g_lq), cc(g_kl), cc(g_ks), ctx.mode,
                                             ctx.analytical, ctx.Z)
        return (_batch_sum_like(p, dp) if ctx.p_bcast else dp, dd) + (None,) * 7


class StochBlockFn(Function):
    """The whole NormalStochasticBlock2d of a low-resolution level (lib/stochastic.py:45-99) as ONE autograd node whose forward is one launch
    (csrc/stoch_img.hip): p_params = conv_in_p(x_p) (top layer: p_given as it is), q_params = conv_in_q(x_q), the core of NormalStochFn,
    out = conv_out(z). Returns out, z, q_params, logprob_p, logprob_q, kl_samplewise, kl_spatial [, p_params]. The backward runs the chain
    from d_out in one launch too (lvae_stoch_block_bwd_f32) or — where that declines, or an upstream gradient of p_params / q_params exists —
    the launches the separate nodes ran (dgrad of conv_out, the core's backward, the two dgrads); either way it hands (x, dy) of the three
    convolutions to the weight-gradient queue as ConvFn does."""

    @staticmethod
    def forward(ctx, x_p, p_given, x_q, noise, blk, mode, analytical, N, rows, *params):
        cv = lambda m: (m.weight, m.geom(), m.bias)
        has_p = x_p is not None
        out, z, p, q, lp, lq, kl, ks = K.stoch_block_fwd(x_p, cv(blk.conv_in_p) if has_p else None, p_given, x_q, cv(blk.conv_in_q), cv(blk.conv_out),
                                                         noise, mode, analytical, N, rows=rows)
        ctx.set_materialize_grads(False)  # unused outputs arrive as None (the kernels take NULL) instead of zero-filled tensors
        ctx.blk, ctx.mode, ctx.analytical, ctx.has_p = blk, mode, analytical, has_p
        ctx.p_bcast = p.shape[0] == 1 and N > 1
        ctx.save_for_backward(x_p, p, x_q, q, noise if mode == 0 else None, z)
        return (out, z, q, lp, lq, kl, ks) + ((p,) if has_p else ())

    @staticmethod
    def backward(ctx, d_out, dz, dq_out, g_lp, g_lq, g_kl, g_ks, dp_out=None):
        x_p, p, x_q, q, eps, z = ctx.saved_tensors
        none = (None,) * len(ctx.needs_input_grad)
        if all(g is None for g in (d_out, dz, dq_out, g_lp, g_lq, g_kl, g_ks, dp_out)):
            return none
        cc = lambda t: None if t is None else _c(t)
        cv = lambda m: None if m is None else (m.weight, m.geom(), m.bias)
        co, cq, cp = ctx.blk.conv_out, ctx.blk.conv_in_q, ctx.blk.conv_in_p if ctx.has_p else None
        hw = (z.shape[1], z.shape[2])
        d_out, dz, g = cc(d_out), cc(dz), (cc(g_lp), cc(g_lq), cc(g_kl), cc(g_ks))
        one = None
        if d_out is not None and dq_out is None and dp_out is None and RB.switches.stoch_block_bwd:
            one = K.stoch_block_bwd(d_out, cv(cp), cv(cq), cv(co), p, q, z, eps, dz, *g, ctx.mode, ctx.analytical)
        if one is not None:
            dp, dq, dx_p, dx_q = one
        else:
            if d_out is not None:
                dzc = K.conv2d_dgrad(d_out, co.weight, co.geom(), hw)
                dz = dzc if dz is None else K.add(dzc, dz)
            dp, dq = K.normal_stochastic_bwd(p, q, eps, z, dz, *g, ctx.mode, ctx.analytical, z.shape[3])
            if dq_out is not None:
                dq = K.add(dq, _c(dq_out))
            if dp_out is not None:
                dp = K.add(dp, _c(dp_out))
            dx_q = K.conv2d_dgrad(dq, cq.weight, cq.geom(), hw) if ctx.needs_input_grad[2] else None
            dx_p = K.conv2d_dgrad(dp, cp.weight, cp.geom(), hw) if cp is not None and ctx.needs_input_grad[0] else None
        for m, x, dy in ((co, z, d_out), (cq, x_q, dq), (cp, x_p, dp)):
            if m is not None and dy is not None and m.weight.requires_grad:
                wgrad(x, dy, m.weight, m.geom(), grad_buf(m.weight), grad_buf(m.bias))
        dpg = None
        if cp is None and ctx.needs_input_grad[1]:   # the given p_params: a broadcast parameter's gradient is summed over the batch
            dpg = _batch_sum_like(p, dp) if ctx.p_bcast else dp
        return (dx_p, dpg, dx_q) + none[3:]


class KlElementwiseFn(Function):
    """`kl_elementwise` of lib/stochastic.py:88-91 / kl_normal_mc :209-226 as a differentiable node (off the training path)."""

    @staticmethod
    def forward(ctx, z, p, q, analytical):
        ctx.analytical = analytical
        ctx.save_for_backward(z, p, q)
        return K.kl_elementwise_fwd(p, q, z, analytical)

    @staticmethod
    def backward(ctx, g):
        z, p, q = ctx.saved_tensors
        dp, dq, dz = K.kl_elementwise_bwd(p, q, z, _c(g), ctx.analytical, need_dz=ctx.needs_input_grad[0])
        dp, dq = (_batch_sum_like(t, d) if t.shape[0] == 1 and d.shape[0] > 1 else d for t, d in ((p, dp), (q, dq)))
        return dz, dp, dq, None


# ----------------------------------------------------------------------------------------------------------------
class BernoulliFn(Function):
    """lib/likelihoods.py:60-78: returns ll (N,) [differentiable], mean, mode, sample (NHWC, no grad)."""

    @staticmethod
    def forward(ctx, logits, x, u):
        mean, mode, sample, ll, dll = K.bernoulli_fwd(logits, x, u, True)
        ctx.save_for_backward(dll)
        ctx.mark_non_differentiable(mode, sample)
        ctx.has_ll = ll is not None
        if ll is None:
            ll = torch.zeros((logits.shape[0],), device=logits.device)
        return ll, mean, mode, sample

    @staticmethod
    def backward(ctx, g_ll, g_mean, g_mode, g_sample):
        (dll,) = ctx.saved_tensors
        if dll is None:
            return None, None, None
        return K.scale_per_sample(dll, _c(g_ll)), None, None


class GaussianFn(Function):
    """lib/likelihoods.py:81-114: returns ll (N,) [differentiable w.r.t. params] and the reparameterised sample."""

    @staticmethod
    def forward(ctx, params, x, eps):
        sample, ll, dll = K.gaussian_fwd(params, x, eps, True)
        ctx.save_for_backward(dll)
        ctx.mark_non_differentiable(sample)
        if ll is None:
            ll = torch.zeros((params.shape[0],), device=params.device)
        return ll, sample

    @staticmethod
    def backward(ctx, g_ll, g_sample):
        (dll,) = ctx.saved_tensors
        return (K.scale_per_sample(dll, _c(g_ll)) if dll is not None else None), None, None


class DiscrLogisticFn(Function):
    """lib/likelihoods.py:117-180: returns ll (N,), mean, logscale, sample (the last three carry no gradient)."""

    @staticmethod
    def forward(ctx, raw, x, u):
        mean, ls, sample, ll, dll = K.discr_logistic_fwd(raw, x, u, True)
        ctx.save_for_backward(dll)
        ctx.mark_non_differentiable(mean, ls, sample)
        if ll is None:
            ll = torch.zeros((raw.shape[0],), device=raw.device)
        return ll, mean, ls, sample

    @staticmethod
    def backward(ctx, g_ll, g_mean, g_ls, g_sample):
        (dll,) = ctx.saved_tensors
        return (K.scale_per_sample(dll, _c(g_ll)) if dll is not None else None), None, None


class DmolFn(Function):
    """lib/likelihoods.py:227-230 + 291-382: ll (N,) from params (N,H,W,100) and x (N,H,W,3) in [0,1]."""

    @staticmethod
    def forward(ctx, l, x):
        ll, dl = K.dmol_ll_fwd(l, x, True)
        ctx.save_for_backward(dl)
        return ll

    @staticmethod
    def backward(ctx, g_ll):
        (dl,) = ctx.saved_tensors
        return K.scale_per_sample(dl, _c(g_ll)), None


# Masked counterparts of the four heads (a likelihood on the observed pixels; kernels.*_masked_fwd): mask (N,H,W) uint8, non-zero = observed.
# The saved dll is the masked one (+0.0 at every parameter of a missing pixel), so the backward is that of the unmasked head. `filled` (x
# where observed, the head's draw where missing) is the last output and carries no gradient; filled_out, when given, is the buffer it is
# written to: x itself completes x in place (LadderVAE.inpaint, under no_grad).
def _filled_out(ctx, filled_out):
    if filled_out is not None:
        ctx.mark_dirty(filled_out)


class BernoulliMaskedFn(Function):
    @staticmethod
    def forward(ctx, logits, x, u, mask, filled_out=None):
        _filled_out(ctx, filled_out)
        mean, mode, sample, ll, dll, filled = K.bernoulli_masked_fwd(logits, x, u, mask, True, filled_out)
        ctx.save_for_backward(dll)
        ctx.mark_non_differentiable(mode, sample, filled)
        return ll, mean, mode, sample, filled

    @staticmethod
    def backward(ctx, g_ll, g_mean, g_mode, g_sample, g_filled):
        (dll,) = ctx.saved_tensors
        return K.scale_per_sample(dll, _c(g_ll)), None, None, None, None


class GaussianMaskedFn(Function):
    @staticmethod
    def forward(ctx, params, x, eps, mask, filled_out=None):
        _filled_out(ctx, filled_out)
        sample, ll, dll, filled = K.gaussian_masked_fwd(params, x, eps, mask, True, filled_out)
        ctx.save_for_backward(dll)
        ctx.mark_non_differentiable(sample, filled)
        return ll, sample, filled

    @staticmethod
    def backward(ctx, g_ll, g_sample, g_filled):
        (dll,) = ctx.saved_tensors
        return K.scale_per_sample(dll, _c(g_ll)), None, None, None, None


class DiscrLogisticMaskedFn(Function):
    @staticmethod
    def forward(ctx, raw, x, u, mask, filled_out=None):
        _filled_out(ctx, filled_out)
        mean, ls, sample, ll, dll, filled = K.discr_logistic_masked_fwd(raw, x, u, mask, True, filled_out)
        ctx.save_for_backward(dll)
        ctx.mark_non_differentiable(mean, ls, sample, filled)
        return ll, mean, ls, sample, filled

    @staticmethod
    def backward(ctx, g_ll, g_mean, g_ls, g_sample, g_filled):
        (dll,) = ctx.saved_tensors
        return K.scale_per_sample(dll, _c(g_ll)), None, None, None, None


class DmolMaskedFn(Function):
    """sample: K.dmol_sample of the same parameters (the head's draw), from which the missing pixels of `filled` are taken."""

    @staticmethod
    def forward(ctx, l, x, mask, sample, filled_out=None):
        _filled_out(ctx, filled_out)
        ll, dl, filled = K.dmol_ll_masked_fwd(l, x, mask, sample, True, filled_out)
        ctx.save_for_backward(dl)
        ctx.mark_non_differentiable(filled)
        return ll, filled

    @staticmethod
    def backward(ctx, g_ll, g_filled):
        (dl,) = ctx.saved_tensors
        return K.scale_per_sample(dl, _c(g_ll)), None, None, None, None


class SegmentMarkFn(Function):
    """Identity in forward. Its backward runs after every backward node of the model segment that starts at this tensor has been
    issued: the deferred (grouped) weight gradients of that segment are flushed and the gradient exchange is told the segment's slice
    of the gradient arena is complete (dist.GradAllReduce.segment_done)."""

    @staticmethod
    def forward(ctx, x, tracker, seg):
        ctx.tracker, ctx.seg = tracker, seg
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        flush_wgrad_group()
        ctx.tracker.segment_done(ctx.seg)
        return g, None, None


def segment_mark(x, tracker, seg):
    y = SegmentMarkFn.apply(x, tracker, seg)
    RB.passed_on(x, (y,))
    return y


class FanoutFn(Function):
    """n aliases of an activation that has n consumers (a top-down layer's input feeds conv_in_p, the merge layer and the skip
    merger; a bottom-up value feeds the next bottom-up layer and its top-down layer): their gradients are summed by ONE launch of
    our own kernel instead of autograd's chain of n - 1 tensor adds."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.set_materialize_grads(False)
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *grads):
        gs = [_c(g) for g in grads if g is not None]
        if not gs:
            return None, None
        while len(gs) > 1:
            gs = ([K.add3(gs[0], gs[1], gs[2])] + gs[3:]) if len(gs) >= 3 else [K.add(gs[0], gs[1])]
        return gs[0], None


def fanout(x, n):
    if n <= 1 or not (torch.is_grad_enabled() and x.requires_grad):
        return (x,) * n
    outs = FanoutFn.apply(x, n)
    RB.passed_on(x, outs)
    return outs


# ----------------------------------------------------------------------------------------------------------------
class UpsampleFn(Function):
    @staticmethod
    def forward(ctx, x):
        return K.upsample2x_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        return K.upsample2x_bwd(_c(dy))


class CropFn(Function):
    """centre crop (or pad) of an NHWC tensor; backward is the inverse pad (or crop)."""

    @staticmethod
    def forward(ctx, x, out_hw):
        ctx.in_hw = (x.shape[1], x.shape[2])
        return K.pad_crop(x, False, out_hw, False)

    @staticmethod
    def backward(ctx, dy):
        return K.pad_crop(_c(dy), False, ctx.in_hw, False), None


# ----------------------------------------------------------------------------------------------------------------
class KLBookFn(Function):
    """models/lvae.py:192-198: kl (L,N) -> kl_sep (N,), kl_avg_layerwise (L,), scalars [kl_loss, kl]."""

    @staticmethod
    def forward(ctx, kl_ln, free_bits):
        ctx.fb = free_bits
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(kl_ln)
        kl_sep, kl_avg, scal = K.kl_bookkeeping_fwd(kl_ln, free_bits)
        kl_loss, kl = scal[0], scal[1]
        ctx.mark_non_differentiable(kl)   # `kl` (the batch mean of kl_sep) is a metric
        return kl_sep, kl_avg, kl_loss, kl

    @staticmethod
    def backward(ctx, g_sep, g_avg, g_kl_loss, g_kl):
        (kl_ln,) = ctx.saved_tensors
        cc = lambda t: None if t is None else _c(t)
        if g_sep is None and g_avg is None and g_kl_loss is None:
            return None, None
        g_scal = None
        if g_kl_loss is not None:   # [d/d kl_loss, d/d kl = 0] as the kernel expects them, written by our own copy kernel
            g_scal = torch.empty((2,), dtype=torch.float32, device=kl_ln.device)
            K.scale_rows_add(cc(g_kl_loss).view(1, 1), None, None, out=g_scal[0:1])
            K.fill_zero(g_scal[1:2])
        return K.kl_bookkeeping_bwd(kl_ln, ctx.fb, cc(g_sep), cc(g_avg), g_scal), None


class KlBalanceFn(Function):
    """KLBookFn with the terms of kl_loss balanced over the layers while beta < 1 (balance.KlBalance holds the fixed weights and the beta
    source; csrc/kl_balance.hip): kl (L,N) -> kl_sep, kl_avg_layerwise, kl_loss (balanced), kl, coeff (L,). kl_sep, kl_avg_layerwise and kl
    are KLBookFn's, bit for bit. coeff is a constant of the gradient: the backward reads what the forward wrote."""

    @staticmethod
    def forward(ctx, kl_ln, free_bits, balance):
        ctx.fb = free_bits
        ctx.set_materialize_grads(False)
        kl_sep, kl_avg, scal, coeff = K.kl_balance_fwd(kl_ln, free_bits, balance.alpha, **balance.beta_source())
        ctx.save_for_backward(kl_ln, coeff)
        kl_loss, kl = scal[0], scal[1]
        ctx.mark_non_differentiable(kl, coeff)
        return kl_sep, kl_avg, kl_loss, kl, coeff

    @staticmethod
    def backward(ctx, g_sep, g_avg, g_kl_loss, g_kl, g_coeff):
        kl_ln, coeff = ctx.saved_tensors
        cc = lambda t: None if t is None else _c(t)
        if g_sep is None and g_avg is None and g_kl_loss is None:
            return None, None, None
        g_scal = None
        if g_kl_loss is not None:   # as in KLBookFn.backward
            g_scal = torch.empty((2,), dtype=torch.float32, device=kl_ln.device)
            K.scale_rows_add(cc(g_kl_loss).view(1, 1), None, None, out=g_scal[0:1])
            K.fill_zero(g_scal[1:2])
        return K.kl_balance_bwd(kl_ln, ctx.fb, coeff, cc(g_sep), cc(g_avg), g_scal), None, None


class StackFn(Function):
    """stack L per-layer (N,) vectors into one (L,N) matrix; backward hands the rows back as views."""

    @staticmethod
    def forward(ctx, *rows):
        L, N = len(rows), rows[0].numel()
        base = rows[0].data_ptr()
        if all(r.is_contiguous() and r.data_ptr() == base + 4 * N * i for i, r in enumerate(rows)):
            # the stochastic kernels wrote their per-sample sums straight into the rows of one [L][N] matrix (models/lvae.py)
            return rows[0].new_empty(0).set_(rows[0].untyped_storage(), rows[0].storage_offset(), (L, N), (N, 1))
        out = torch.empty((L, N), dtype=torch.float32, device=rows[0].device)
        for i, r in enumerate(rows):
            K.scale_rows_add(_c(r).view(1, -1), None, None, out=out[i])
        return out

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        return tuple(g[i] for i in range(g.shape[0]))


class ElboLossFn(Function):
    """experiment/experiment_manager.py:329-344: returns elbo_sep (N,), scalars [loss, elbo, recons]."""

    @staticmethod
    def forward(ctx, ll, kl_sep, kl_loss, beta):
        ctx.beta, ctx.N = beta, ll.numel()
        ctx.kl_dim0 = kl_loss.dim() == 0
        elbo_sep, scal = K.elbo_loss_fwd(ll, kl_sep, kl_loss, beta)
        loss, elbo, recons = scal[0], scal[1], scal[2]
        ctx.mark_non_differentiable(elbo_sep, elbo, recons)   # only d(loss) is propagated; elbo / recons are metrics
        return elbo_sep, loss, elbo, recons

    @staticmethod
    def backward(ctx, g_sep, g_loss, g_elbo, g_recons):
        d_ll, d_kl = K.elbo_loss_bwd(_c(g_loss).view(1), ctx.beta, ctx.N)
        return d_ll, None, d_kl.view(()) if ctx.kl_dim0 else d_kl, None


class ElboLossAnnealFn(Function):
    """ElboLossFn with beta = linear_anneal(step[0], 0, 1, anneal_steps) read on the device: a captured step replays with the beta of
    the step it runs (step: device int64[1], the number of completed training steps)."""

    @staticmethod
    def forward(ctx, ll, kl_sep, kl_loss, step, anneal_steps):
        ctx.step, ctx.anneal_steps, ctx.N = step, int(anneal_steps), ll.numel()
        ctx.kl_dim0 = kl_loss.dim() == 0
        elbo_sep, scal = K.elbo_loss_fwd_anneal(ll, kl_sep, kl_loss, step, anneal_steps)
        loss, elbo, recons = scal[0], scal[1], scal[2]
        ctx.mark_non_differentiable(elbo_sep, elbo, recons)
        return elbo_sep, loss, elbo, recons

    @staticmethod
    def backward(ctx, g_sep, g_loss, g_elbo, g_recons):
        d_ll, d_kl = K.elbo_loss_bwd_anneal(_c(g_loss).view(1), ctx.step, ctx.anneal_steps, ctx.N)
        return d_ll, None, d_kl.view(()) if ctx.kl_dim0 else d_kl, None, None


# ----------------------------------------------------------------------------------------------------------------
# Training on the K-sample importance-weighted bound: rows are sample-major, row k*B + b is sample k of image b
class IwLossFn(Function):
    """ll, kl_sep (K*B,) -> elbo_sep (K*B,), scalars loss = -mean_b logmeanexp_k(ll - beta kl_sep), elbo, recons, iw (the bound at beta = 1),
    ess, and the self-normalised weights w (K*B,) the backward scales the rows' gradients with."""

    @staticmethod
    def forward(ctx, ll, kl_sep, beta, n_samples):
        ctx.beta, ctx.K = beta, n_samples
        elbo_sep, w, bound, scal = K.iw_loss_fwd(ll, kl_sep, beta, n_samples)
        ctx.save_for_backward(w)
        loss, elbo, recons, iw, ess = scal[0], scal[1], scal[2], scal[3], scal[4]
        ctx.mark_non_differentiable(elbo_sep, elbo, recons, iw, ess, w)   # only d(loss) is propagated
        return elbo_sep, loss, elbo, recons, iw, ess, w

    @staticmethod
    def backward(ctx, g_sep, g_loss, g_elbo, g_recons, g_iw, g_ess, g_w):
        (w,) = ctx.saved_tensors
        d_ll, d_kl = K.iw_loss_bwd(_c(g_loss).view(1), w, ctx.beta, ctx.K)
        return d_ll, d_kl, None, None


class IwLossAnnealFn(Function):
    """IwLossFn with beta = linear_anneal(step[0], 0, 1, anneal_steps) read on the device, as ElboLossAnnealFn reads it."""

    @staticmethod
    def forward(ctx, ll, kl_sep, step, anneal_steps, n_samples):
        ctx.step, ctx.anneal_steps, ctx.K = step, int(anneal_steps), n_samples
        elbo_sep, w, bound, scal = K.iw_loss_fwd_anneal(ll, kl_sep, step, anneal_steps, n_samples)
        ctx.save_for_backward(w)
        loss, elbo, recons, iw, ess = scal[0], scal[1], scal[2], scal[3], scal[4]
        ctx.mark_non_differentiable(elbo_sep, elbo, recons, iw, ess, w)
        return elbo_sep, loss, elbo, recons, iw, ess, w

    @staticmethod
    def backward(ctx, g_sep, g_loss, g_elbo, g_recons, g_iw, g_ess, g_w):
        (w,) = ctx.saved_tensors
        d_ll, d_kl = K.iw_loss_bwd_anneal(_c(g_loss).view(1), w, ctx.step, ctx.anneal_steps, ctx.K)
        return d_ll, d_kl, None, None, None


class RepeatSamplesFn(Function):
    """(B, ...) -> (K*B, ...): a bottom-up level's output handed to the K samples of the top-down pass; backward sums the K gradients of
    an image in ascending k with one launch. The output is a new tensor: a block's Handover does not travel with it."""

    @staticmethod
    def forward(ctx, x, n_samples):
        ctx.K = n_samples
        return K.repeat_samples(_c(x), n_samples)

    @staticmethod
    def backward(ctx, dout):
        return K.repeat_samples_bwd(_c(dout), ctx.K), None
