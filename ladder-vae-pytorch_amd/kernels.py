"""Tensor-level wrappers over the C ABI (one Python function per kernel entry point).

Activations are 4-D torch tensors stored NHWC: shape (N, H, W, C), contiguous, float32, on the GPU. No arithmetic
happens in Python or in torch ops here: every function launches hand-written HIP kernels on torch's current
stream. Buffers (outputs, workspaces) come from torch's caching allocator, which is graph-capture safe.
"""
import ctypes as C
import weakref

import torch

from . import _C
from ._C import ACT, BnFold, ConvDesc, RbExt, GATHER_CONV, GATHER_TRANSPOSED, PREC_BF16, PREC_F32, call, ptr, ptr_dt, stream_ptr

_ws_cache = {}

# Arithmetic of the matrix-core kernels for every convolution descriptor built from here on: PREC_F32 (results as an fp32
# multiply-add chain) or PREC_BF16 (operands rounded to bf16 at the MFMA input, fp32 accumulate). LadderVAE sets it from its
# `compute_dtype` at the start of every pass; backward launches of that pass follow before the next forward.
precision = PREC_F32


# Arithmetic-form request (lvae_conv_desc.form) of every descriptor built from here on: FORM_AUTO in the product; the parity tests
# walk the other forms (`with kernels.use_form(_C.FORM_F32_MFMA): ...`).
form = _C.FORM_AUTO


class use_form:
    def __init__(self, f):
        self.f = f

    def __enter__(self):
        global form
        self.prev, form = form, self.f

    def __exit__(self, *exc):
        global form
        form = self.prev


BF16_MODE_NOTE = ('forward, dgrad and weight gradient of the 3x3 convolutions of the 8x8..32x32 levels and the GateLayer2d 1x1 family on '
                  'v_mfma_f32_32x32x16_bf16 with bf16 operands; the tensors inside those residual blocks (conv outputs, gate pre-activations '
                  'and their gradients) stored as bf16 in HBM, as torch.autocast(bfloat16) stores conv outputs; residual stream, fp32 '
                  'accumulate / statistics / KL / likelihood / parameters / Adamax; merge 1x1 and <=4x4 convolutions fp32')


def set_precision(dtype):
    global precision
    precision = {'f32': PREC_F32, 'fp32': PREC_F32, 'float32': PREC_F32, 'bf16': PREC_BF16, 'bfloat16': PREC_BF16}[str(dtype).replace('torch.', '')]


def workspace(nbytes, device):
    """A per-device scratch buffer, grown on demand. Kernels run in stream order, so one buffer is enough."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)  # one scratch buffer per launch stream
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes or buf.device != device:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def _chk_nhwc(t, name):
    if t.dim() != 4 or not t.is_contiguous() or t.dtype not in (torch.float32, torch.bfloat16):
        raise _C.LvaeHipError("%s must be a contiguous float32 (or, inside a residual block under compute_dtype bf16, bfloat16) (N,H,W,C) "
                              "tensor, got shape %s strides %s %s" % (name, tuple(t.shape), tuple(t.stride()), t.dtype))


def _dt(t):
    """lvae_conv_desc.*_dtype of a tensor (LVAE_DT_F32 for None)."""
    return _C.DT_BF16 if (t is not None and t.dtype == torch.bfloat16) else _C.DT_F32


class ConvGeom:
    """Geometry of one convolution call site plus the strides of its weight tensor.

    `weight` is the nn.Parameter in the reference's logical shape — (Cout,Cin,KH,KW) for nn.Conv2d,
    (Cin,Cout,KH,KW) for nn.ConvTranspose2d — in ANY tap-linear memory layout; the arena packs it as
    [KH][KW][Cin][Cout] so that forward reads are n-contiguous and dgrad reads k-contiguous float4s.
    """

    def __init__(self, weight, stride=1, pad=0, transposed=False, output_padding=0):
        self.transposed = bool(transposed)
        if transposed:
            self.Cin, self.Cout, self.KH, self.KW = weight.shape
            s_ci, s_co, s_kh, s_kw = weight.stride()
        else:
            self.Cout, self.Cin, self.KH, self.KW = weight.shape
            s_co, s_ci, s_kh, s_kw = weight.stride()
        if self.KH * self.KW > 1 and s_kh != self.KW * s_kw:
            raise _C.LvaeHipError("weight layout is not tap-linear (strides %s)" % (tuple(weight.stride()),))
        self.s_tap, self.s_ci, self.s_co = (s_kw if self.KH * self.KW > 1 else 0), s_ci, s_co
        self.stride, self.pad, self.output_padding = int(stride), int(pad), int(output_padding)

    def out_size(self, H, W):
        if self.transposed:
            return ((H - 1) * self.stride - 2 * self.pad + self.KH + self.output_padding,
                    (W - 1) * self.stride - 2 * self.pad + self.KW + self.output_padding)
        return ((H + 2 * self.pad - self.KH) // self.stride + 1, (W + 2 * self.pad - self.KW) // self.stride + 1)


def _desc(g, weight, x, x2, N, H, W, OH, OW, Cout, k_stride, n_stride, gather, bias=None, in_scale=None, in_shift=None,
          in_act=None, out_scale=None, out_act=None, y=None):
    d = ConvDesc()
    d.x, d.x2 = ptr_dt(x), ptr_dt(x2)   # element types travel in d.x_dtype / d.y_dtype below
    d.C1, d.C2 = x.shape[3], (x2.shape[3] if x2 is not None else 0)
    d.w, d.w_stap, d.w_sk, d.w_sn = ptr(weight), g.s_tap, k_stride, n_stride
    d.bias, d.in_scale, d.in_shift = ptr(bias), ptr(in_scale), ptr(in_shift)
    d.in_act, d.out_scale, d.out_act = ACT[in_act], ptr(out_scale), ACT[out_act]
    d.y = ptr_dt(y)
    d.N, d.H, d.W, d.OH, d.OW, d.Cout = N, H, W, OH, OW, Cout
    d.KH, d.KW, d.stride, d.pad, d.gather = g.KH, g.KW, g.stride, g.pad, gather
    d.precision = precision
    d.form = form
    d.x_dtype, d.y_dtype = _dt(x), _dt(y)
    if x2 is not None and x2.dtype != x.dtype:
        raise _C.LvaeHipError("x and x2 must have the same element type")
    return d


class _PreparedWeights:
    """Transformed-weight cache of the Winograd convolutions (lvae_conv2d_prepare_weights).

    Every eligible (weight view, orientation) gets a private scratch buffer; `prepare_all()` refreshes all of them in ONE
    launch (the training step calls it right after the optimizer has written the weights) and a convolution whose entry is
    current runs with workspace_ready = 1. An entry is current while neither the tensor's autograd version counter (any
    torch in-place op: load_state_dict, copy_, ...) nor `epoch` (bumped by every kernel of this package that writes weights
    through raw pointers: Adamax, broadcast, graph replays) has moved since it was written; otherwise the convolution falls
    back to transforming its weights itself, so a stale buffer is never read.
    """

    def __init__(self):
        self.entries = {}   # key -> dict(weight, U, desc bytes, stamp)
        self.epoch = 0
        self.table = None   # device table of the entries, rebuilt when the set changes
        self.enabled = True

    def stamp(self, weight):
        return (weight._version, self.epoch)

    @staticmethod
    def _alive(ent):
        """The entry's weight tensor still exists and still lives where the entry's raw pointers say (a model that was dropped, or
        re-packed by .to(), leaves entries behind that must neither pin its arena nor be transformed again)."""
        w = ent['weight']()
        return w is not None and w.data_ptr() == ent['base']

    def evict_dead(self):
        dead = [k for k, e in self.entries.items() if not self._alive(e)]
        for k in dead:
            del self.entries[k]
        if dead:
            self.table = None
        return len(dead)

    def attach(self, d, weight, device, need, entry_fn='lvae_conv2d_prepare_entry'):
        key = (d.w, d.w_sk, d.w_sn, d.gather, d.Cout, int(need), device.index, entry_fn)   # `need` / entry_fn tell the transform kinds apart
        ent = self.entries.get(key)
        if ent is not None and not self._alive(ent):   # the address was recycled for another tensor
            del self.entries[key]
            self.table = None
            ent = None
        if ent is None:
            ent = {'weight': weakref.ref(weight), 'base': weight.data_ptr(), 'U': torch.empty(int(need), dtype=torch.uint8, device=device), 'stamp': None, 'entry': None}
            d.workspace, d.workspace_bytes = ent['U'].data_ptr(), ent['U'].numel()
            raw = (C.c_char * _C.load().lvae_conv2d_prepare_entry_bytes())()
            call(entry_fn, C.byref(d), C.cast(raw, C.c_void_p))
            ent['entry'] = bytes(raw)
            ent['cout'] = max(d.Cout, d.C1) if entry_fn == 'lvae_resblock_gate_prepare_entry' else d.Cout   # threads per entry of the batched launch
            self.entries[key] = ent
            self.table = None
        d.workspace, d.workspace_bytes = ent['U'].data_ptr(), ent['U'].numel()
        d._ws_tensor = ent['U']   # (a Python attribute of the ctypes object: lets a caller keep the scratch buffer alive, rb_weight_ranges)
        d.workspace_ready = 1 if (self.enabled and ent['stamp'] == self.stamp(weight)) else 0

    def prepare_all(self):
        """One launch that (re)writes every registered buffer from the current weights. Returns the number of entries."""
        if not torch.cuda.is_current_stream_capturing():
            self.evict_dead()   # (a captured step keeps its table: the replayed launch reads the pointers it was captured with)
        if not self.entries or not self.enabled:
            return 0
        by_dev = {}
        for k, e in self.entries.items():
            by_dev.setdefault(k[6], []).append(e)
        if self.table is None:
            if torch.cuda.is_current_stream_capturing():
                return 0  # the table upload is a host copy: convolutions transform their own weights until an eager step built it
            self.table = {}
            for dev, ents in by_dev.items():
                blob = b''.join(e['entry'] for e in ents)
                t = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(torch.device('cuda', dev))
                self.table[dev] = (t, len(ents), max(e['cout'] for e in ents))
        for dev, ents in by_dev.items():
            t, n, max_cout = self.table[dev]
            with torch.cuda.device(dev):
                call('lvae_conv2d_prepare_weights', t.data_ptr(), n, max_cout, stream_ptr())
            for e in ents:
                w = e['weight']()
                e['stamp'] = self.stamp(w) if w is not None else None
        return len(self.entries)

    def pin_current(self):
        """Called by a TrainStep right after it captured a graph containing prepare_all(): returns a handle that keeps the table the
        captured launch reads, and every scratch buffer its entries point to, alive. A later change of the entry set (another batch
        size, another model, evict_dead) builds a NEW table; the pinned one stays valid for the replays of that graph."""
        if self.table is None:
            return None
        return (self.table, [e for e in self.entries.values()])   # the caller (the graph's owner) holds it; nothing here does

    def invalidate(self):
        """Forget that any buffer is current (a step that stamped them was abandoned before its launches ran, e.g. a failed capture):
        every convolution transforms its own weights until the next prepare_all()."""
        for e in self.entries.values():
            e['stamp'] = None

    def weights_written(self):
        """Call after weights were modified through raw pointers (optimizer kernel, collective, graph replay)."""
        self.epoch += 1


prepared = _PreparedWeights()


def _conv_ws(d, weight, device):
    need = _C.load().lvae_conv2d_workspace(C.byref(d))
    if need:
        prepared.attach(d, weight, device, need)


def resblock_bf16_storage(x, weight, g):
    """True when a residual block whose 3x3 convolutions are (weight, g) on input x can keep its internal tensors (conv outputs, gate
    pre-activations and their gradients) in bf16: precision bf16 and every kernel of the block's forward and backward has the
    bf16-storage form for this shape (lvae_resblock_bf16_storage)."""
    if precision != PREC_BF16 or _ddi is not None or x.dtype != torch.float32:
        return False
    N, H, W, _ = x.shape
    d = _desc(g, weight, x, None, N, H, W, H, W, g.Cout, g.s_ci, g.s_co, GATHER_CONV)
    _conv_ws(d, weight, x.device)
    return bool(_C.load().lvae_resblock_bf16_storage(C.byref(d)))


_ddi = None  # set by init.data_dependent_init for the duration of its forward pass


def _ddi_conv(state, x, weight, g, bias, x2, in_scale, in_shift, in_act, out_scale, out_act):
    """One convolution of the data-dependent initialisation pass (init.py): plain output, per-channel statistics, parameter
    rescale in place, corrected output, then the caller's epilogue."""
    global _ddi
    _ddi = None
    try:
        y = conv2d(x, weight, g, bias=bias, x2=x2, in_scale=in_scale, in_shift=in_shift, in_act=in_act)
        _, _, mean, rstd = bn_stats(y, None, None, None, None, eps=1e-20)
    finally:
        _ddi = state
    scale = 1.0 / (1.0 / rstd + 1e-5)
    weight.mul_(scale.view(1, -1, 1, 1) if g.transposed else scale.view(-1, 1, 1, 1))
    if bias is not None:
        bias.sub_(mean).mul_(scale)
        y = affine_act(y, scale, -mean * scale, None)
    else:
        y = affine_act(y, scale, torch.zeros_like(scale), None)
    if out_scale is not None or out_act is not None:
        ones, zeros = torch.ones_like(scale), torch.zeros_like(scale)
        y = affine_act(y, ones, zeros, out_act, row_scale=out_scale)
    state['done'].add(weight.data_ptr())
    state['count'] += 1
    return y


class StatParts:
    """BatchNorm partial sums a kernel epilogue wrote for its OUTPUT: buf (rows [+1], 2, C) — (sum(y - pivot), sum((y - pivot)^2)) per
    workgroup row; has_pivot: the producer stored its pivot in row `rows` (such a buffer can be finalized inside the consuming
    convolution's prologue, see lvae_bn_fold)."""
    __slots__ = ('buf', 'rows', 'has_pivot')

    def __init__(self, buf, rows, has_pivot):
        self.buf, self.rows, self.has_pivot = buf, rows, has_pivot

    def rows_view(self):
        return self.buf[:self.rows]


def conv2d(x, weight, g, bias=None, x2=None, in_scale=None, in_shift=None, in_act=None, out_scale=None, out_act=None,
           stats_pivot=None, in_bn=None, out_bf16=False):
    """y = out_act((conv(in_act(x*in_scale+in_shift)) + bias) * out_scale). x (and x2) NHWC; returns NHWC.
    stats_pivot (Cout,): also ask the kernel's epilogue for BatchNorm partials of y around that pivot; returns (y, parts) with
    parts a StatParts, or (y, None) when the kernel variant chosen for this shape has no such epilogue.
    in_bn = (parts: StatParts, pivot, bn): training-mode BatchNorm of the INPUT whose statistics exist as partial sums (bn has
    weight, bias, running_mean, running_var, eps, momentum); the coefficients are finalized inside the convolution when the
    selected kernel can do that (lvae_conv2d_folds_bn_finalize) and by lvae_bn_finalize_parts_f32 otherwise. Returns
    (y, parts | None, (scale, shift, mean, rstd)).
    out_bf16: store y as bfloat16 (only inside a residual block whose shape passed resblock_bf16_storage)."""
    if _ddi is not None and weight.data_ptr() not in _ddi['done']:
        assert in_bn is None
        y = _ddi_conv(_ddi, x, weight, g, bias, x2, in_scale, in_shift, in_act, out_scale, out_act)
        return y if stats_pivot is None else (y, None)
    _chk_nhwc(x, 'x')
    N, H, W, C1 = x.shape
    if x2 is not None:
        _chk_nhwc(x2, 'x2')
        assert x2.shape[:3] == x.shape[:3]
    if C1 + (x2.shape[3] if x2 is not None else 0) != g.Cin:
        raise _C.LvaeHipError("conv2d: input has %d channels, weight expects %d" % (C1 + (x2.shape[3] if x2 is not None else 0), g.Cin))
    OH, OW = g.out_size(H, W)
    y = torch.empty((N, OH, OW, g.Cout), dtype=torch.bfloat16 if out_bf16 else torch.float32, device=x.device)
    d = _desc(g, weight, x, x2, N, H, W, OH, OW, g.Cout, g.s_ci, g.s_co,
              GATHER_TRANSPOSED if g.transposed else GATHER_CONV, bias, in_scale, in_shift, in_act, out_scale, out_act, y)
    _conv_ws(d, weight, x.device)
    lib = _C.load()
    coef = fold = None
    if in_bn is not None:
        coef, fold = _in_bn(d, in_bn, x, in_bn[0].has_pivot and x2 is None and bool(lib.lvae_conv2d_folds_bn_finalize(C.byref(d))))
    parts = None
    if stats_pivot is not None:
        rows = lib.lvae_conv2d_stats_rows(C.byref(d))
        if rows > 0:
            buf_rows = lib.lvae_conv2d_stats_buffer_rows(C.byref(d))   # + 1 where the kernel stores its pivot behind the partial rows
            buf = torch.empty((buf_rows, 2, g.Cout), dtype=torch.float32, device=x.device)
            parts = StatParts(buf, rows, buf_rows > rows)
            d.stats_out, d.stats_pivot = ptr(buf), ptr(stats_pivot)
    call('lvae_conv2d_f32', C.byref(d), stream_ptr())
    del fold
    if in_bn is not None:
        return y, parts, coef
    return y if stats_pivot is None else (y, parts)


def conv1x1_gate(x, weight, g, bias, res, act, need_ab=True, stats_pivot=None):
    """GateLayer2d forward: ab = conv1x1(x) + bias (returned when need_ab), out = act(a) * sigmoid(b) + res, one kernel.
    Falls back to conv2d + gate_fwd when the fused kernel does not support the shape (lvae_conv1x1_gate_variant == 0).
    stats_pivot (C,): also return BatchNorm partials of `out` (rows, 2, C) around that pivot, or None when unsupported:
    returns (ab, out, parts)."""
    _chk_nhwc(x, 'x')
    N, H, W, _ = x.shape
    Cn = g.Cout // 2
    lib = _C.load()
    fused = _ddi is None or weight.data_ptr() in _ddi['done']
    if fused:
        ab = torch.empty((N, H, W, g.Cout), dtype=x.dtype, device=x.device) if need_ab else None   # bf16-stored x: bf16-stored ab
        d = _desc(g, weight, x, None, N, H, W, H, W, g.Cout, g.s_ci, g.s_co, GATHER_CONV, bias, y=ab)
        fused = bool(lib.lvae_conv1x1_gate_variant(C.byref(d)))
    if not fused:
        ab = conv2d(x, weight, g, bias=bias)
        out = gate_fwd(ab, res, act)
        return (ab, out) if stats_pivot is None else (ab, out, None)
    out = torch.empty((N, H, W, Cn), dtype=torch.float32, device=x.device)
    parts = None
    if stats_pivot is not None:
        rows = lib.lvae_conv1x1_gate_stats_rows(C.byref(d))
        if rows > 0:
            buf = torch.empty((rows + 1, 2, Cn), dtype=torch.float32, device=x.device)   # last row: the pivot (written by the kernel)
            parts = StatParts(buf, rows, True)
            d.stats_out, d.stats_pivot = ptr(buf), ptr(stats_pivot)
    call('lvae_conv1x1_gate_f32', C.byref(d), ptr(res), ACT[act], ptr(out), stream_ptr())
    return (ab, out) if stats_pivot is None else (ab, out, parts)


def conv1x1_gate_bwd(dout, ab, weight, g, act, out_scale=None):
    """Backward of conv1x1_gate w.r.t. the convolution input and the pre-activations: returns (dab, dx). One kernel when the
    shape is supported (gate backward formed in the dgrad kernel's operand staging; lvae_conv1x1_gate_bwd_ok), else gate_bwd +
    conv2d_dgrad."""
    _chk_nhwc(dout, 'dout')
    N, H, W, Cn = dout.shape
    dx = torch.empty((N, H, W, g.Cin), dtype=torch.float32, device=dout.device)
    d = _desc(g, weight, ab, None, N, H, W, H, W, g.Cin, g.s_co, g.s_ci, GATHER_TRANSPOSED, out_scale=out_scale, y=dx)
    if g.Cout != 2 * Cn or not _C.load().lvae_conv1x1_gate_bwd_ok(C.byref(d)):
        dab = gate_bwd(dout, ab, act)
        return dab, conv2d_dgrad(dab, weight, g, (H, W), out_scale=out_scale)
    dab = torch.empty_like(ab)
    call('lvae_conv1x1_gate_bwd_f32', C.byref(d), ptr(dout), ptr(ab), ACT[act], ptr(dab), stream_ptr())
    return dab, dx


def _gate_bwd_fused_desc(x_like, weight, g, dweight):
    """The 128 -> 64 dgrad view the persistent gate backward is asked about, for the gate convolution (weight, g) on tensors shaped like
    x_like (N,H,W,C); None where Python alone can tell that it does not apply (what the library cannot see)."""
    N, H, W, Cn = x_like.shape
    if g.Cout != 2 * Cn or (dweight is not None and tuple(dweight.stride()) != tuple(weight.stride())):
        return None
    d = _desc(g, weight, x_like, None, N, H, W, H, W, g.Cin, g.s_co, g.s_ci, GATHER_TRANSPOSED)
    d.C1 = g.Cout
    return d


def gate_bwd_fused_ws(x_like, weight, g, dweight=None):
    """Scratch bytes conv1x1_gate_bwd_wgrad needs for the gate convolution (weight, g) on tensors shaped like x_like (N,H,W,C); 0: it does
    not take the shape. dweight: the gradient buffer, where it exists already."""
    d = _gate_bwd_fused_desc(x_like, weight, g, dweight)
    return int(_C.load().lvae_conv1x1_gate_bwd_wgrad_workspace(C.byref(d))) if d is not None else 0


def gate_bwd_apply_ok(x_like, weight, g, dweight=None):
    """True when conv1x1_gate_bwd_wgrad takes the gate convolution (weight, g) on tensors shaped like x_like (N,H,W,C) with a deferred
    BatchNorm-backward apply (BnBwdApply) forming its dout."""
    d = _gate_bwd_fused_desc(x_like, weight, g, dweight)
    return d is not None and bool(_C.load().lvae_conv1x1_gate_bwd_wgrad_apply_ok(C.byref(d)))


gate_bwd_fused_ok = gate_bwd_apply_ok   # (the name the residual-block tests ask by)


def conv1x1_gate_bwd_wgrad(dout, ab, y, weight, g, act, dweight, dbias, out_scale=None, out_bf16=False, apply=None):
    """conv1x1_gate_bwd and the weight / bias gradient of the gate convolution in one persistent kernel (dab never leaves LDS):
    returns dx, and accumulates into dweight / dbias. Returns None when the shape is not supported (caller composes the two).
    apply (BnBwdApply): dout does not exist yet; the kernel forms it from the deferred BatchNorm-backward apply and stores it to apply.out."""
    _chk_nhwc(dout, 'dout')
    N, H, W, Cn = dout.shape
    if g.Cout != 2 * Cn or tuple(dweight.stride()) != tuple(weight.stride()):
        return None
    if ab.dtype != y.dtype:
        raise _C.LvaeHipError("conv1x1_gate_bwd_wgrad: ab and y must have the same element type")
    dx = torch.empty((N, H, W, g.Cin), dtype=torch.bfloat16 if out_bf16 else torch.float32, device=dout.device)
    d = _desc(g, weight, ab, None, N, H, W, H, W, g.Cin, g.s_co, g.s_ci, GATHER_TRANSPOSED, out_scale=out_scale, y=dx)
    lib = _C.load()
    need = lib.lvae_conv1x1_gate_bwd_wgrad_workspace(C.byref(d))
    if not need or (apply is not None and not lib.lvae_conv1x1_gate_bwd_wgrad_apply_ok(C.byref(d))):
        return None
    ws = workspace(need, dout.device)
    ap = apply.struct(N * H * W) if apply is not None else None
    call('lvae_conv1x1_gate_bwd_wgrad_f32', C.byref(d), ptr(dout), ptr_dt(ab), ptr_dt(y), ACT[act], ptr(dweight), g.s_ci, g.s_co, ptr(dbias),
         ws.data_ptr(), ws.numel(), C.byref(ap) if ap is not None else None, stream_ptr())
    return dx


def gate_bwd_recompute_ok(x_like, weight, g, dweight=None):
    """True when conv1x1_gate_bwd_wgrad_recompute takes the gate convolution (weight, g) on tensors shaped like x_like (N,H,W,C), with or
    without a deferred apply: the fp32 six-product form of the persistent gate backward, fp32-stored tensors."""
    d = _gate_bwd_fused_desc(x_like, weight, g, dweight)
    return d is not None and x_like.dtype == torch.float32 and bool(_C.load().lvae_conv1x1_gate_bwd_wgrad_recompute_ok(C.byref(d)))


def conv1x1_gate_bwd_wgrad_recompute(dout, y, weight, g, bias, act, dweight, dbias, out_scale=None, apply=None):
    """conv1x1_gate_bwd_wgrad without the saved pre-activations: the kernel forms ab = conv1x1(y) + bias again per tile, from y and the gate
    weights as rb_conv_gate(..., want_ab=False) pre-split them, in the forward's accumulation order (the same bits). Returns dx, and
    accumulates into dweight / dbias; None when the shape is not supported. apply: as for conv1x1_gate_bwd_wgrad."""
    _chk_nhwc(dout, 'dout')
    N, H, W, Cn = dout.shape
    if g.Cout != 2 * Cn or tuple(dweight.stride()) != tuple(weight.stride()) or y.dtype != torch.float32:
        return None
    dx = torch.empty((N, H, W, g.Cin), dtype=torch.float32, device=dout.device)
    d = _desc(g, weight, y, None, N, H, W, H, W, g.Cin, g.s_co, g.s_ci, GATHER_TRANSPOSED, out_scale=out_scale, y=dx)
    d.C1 = g.Cout
    lib = _C.load()
    need = lib.lvae_conv1x1_gate_bwd_wgrad_workspace(C.byref(d))
    if not need or not lib.lvae_conv1x1_gate_bwd_wgrad_recompute_ok(C.byref(d)):
        return None
    e = RbExt()
    _rb_gate_ws(e, weight, g, dout.device, False)   # the forward's planes: the buffer (and its ready flag) the forward launch used
    ws = workspace(need, dout.device)
    ap = apply.struct(N * H * W) if apply is not None else None
    call('lvae_conv1x1_gate_bwd_wgrad_recompute_f32', C.byref(d), ptr(dout), ptr(y), ACT[act], e.gate_ws, e.gate_ws_bytes, e.gate_ws_ready,
         e.gate_w, e.gate_w_sk, e.gate_w_sn, ptr(bias), ptr(dweight), g.s_ci, g.s_co, ptr(dbias), ws.data_ptr(), ws.numel(),
         C.byref(ap) if ap is not None else None, stream_ptr())
    return dx


# ----------------------------------------------------------------------------------------------------------------
# Fused residual-block launches of the low-resolution levels (csrc/resblock_img.hip, lvae_resblock_conv_f32)
def _rb_desc(x_like, weight, g, dgrad, y=None, bias=None, in_scale=None, in_shift=None, in_act=None, out_scale=None):
    """Descriptor of the block's 3x3 convolution (forward) or of its dgrad, with the pre-split weights attached."""
    N, H, W, _ = x_like.shape
    if dgrad:
        d = _desc(g, weight, x_like, None, N, H, W, H, W, g.Cin, g.s_co, g.s_ci, GATHER_TRANSPOSED, out_scale=out_scale, y=y)
    else:
        d = _desc(g, weight, x_like, None, N, H, W, H, W, g.Cout, g.s_ci, g.s_co, GATHER_CONV, bias, in_scale, in_shift, in_act, out_scale, None, y)
    need = _C.load().lvae_resblock_conv_workspace(C.byref(d))
    if need:
        prepared.attach(d, weight, x_like.device, need, 'lvae_resblock_conv_prepare_entry')
    return d, need


def _rb_gate_ws(e, gate_w, gate_g, device, bwd):
    """Attach the pre-split copy of the gate weight (direction: forward 64 -> 128, or its dgrad 128 -> 64) to the extension block."""
    gd = ConvDesc()
    gd.w, gd.precision = ptr(gate_w), precision
    if bwd:
        gd.C1, gd.Cout, gd.w_sk, gd.w_sn, gd.gather = gate_g.Cout, gate_g.Cin, gate_g.s_co, gate_g.s_ci, GATHER_TRANSPOSED
    else:
        gd.C1, gd.Cout, gd.w_sk, gd.w_sn, gd.gather = gate_g.Cin, gate_g.Cout, gate_g.s_ci, gate_g.s_co, GATHER_CONV
    need = _C.load().lvae_resblock_gate_workspace(C.byref(gd))
    if not need:
        raise _C.LvaeHipError("fused residual block: the gate convolution must be 1x1, 64 -> 128 channels")
    prepared.attach(gd, gate_w, device, need, 'lvae_resblock_gate_prepare_entry')
    e.gate_w, e.gate_w_sk, e.gate_w_sn = gd.w, gd.w_sk, gd.w_sn
    e.gate_ws, e.gate_ws_bytes, e.gate_ws_ready = gd.workspace, gd.workspace_bytes, gd.workspace_ready
    e._ws_tensor = gd._ws_tensor


def rb_rows(x, weight, g):
    """Workgroups (= statistics rows) of the fused residual-block kernels for the 3x3 convolution (weight, g) on x, 0 when the shape is
    not theirs (needs 3x3 / stride 1 / pad 1, 64 -> 64 channels, H*W a divisor of 64, fp32 NHWC x)."""
    d = _rb_query_desc(x, weight, g)
    return int(_C.load().lvae_resblock_conv_rows(C.byref(d))) if d is not None else 0


def _rb_query_desc(x, weight, g):
    """Bare descriptor for the shape queries of the residual-block kernels, None where none of them applies. (No scratch is attached here:
    asking must not register weights the caller may never run through these kernels.)"""
    if _ddi is not None or x.dtype != torch.float32 or x.dim() != 4 or g.transposed or g.KH != 3 or g.stride != 1 or g.pad != 1:
        return None
    N, H, W, _ = x.shape
    return _desc(g, weight, x, None, N, H, W, H, W, g.Cout, g.s_ci, g.s_co, GATHER_CONV)


def _in_bn(d, in_bn, x, can_fold=True, coef=None):
    """Training-mode BatchNorm of the convolution input from partial sums: folded into the prologue when the producer stored its pivot
    (and the kernel that will run can fold), by lvae_bn_finalize_parts_f32 otherwise. in_bn None: the given coefficients. Returns (coef
    4-tuple, keep-alive)."""
    if in_bn is None:
        d.in_scale, d.in_shift = ptr(coef[0]), ptr(coef[1])
        return coef, None
    sp, pivot, bn = in_bn
    N, H, W, C1 = x.shape
    M = N * H * W
    if sp.has_pivot and can_fold:
        coef = torch.empty((4, C1), dtype=torch.float32, device=x.device)
        fold = BnFold(ptr(sp.buf), sp.rows, M, ptr(bn.weight), ptr(bn.bias), bn.eps, bn.momentum, ptr(bn.running_mean),
                      ptr(bn.running_var), ptr(coef))
        d.in_fold = C.addressof(fold)
        return (coef[0], coef[1], coef[2], coef[3]), fold
    coef = bn_finalize_parts(sp.rows_view(), M, pivot, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, bn.momentum)
    d.in_scale, d.in_shift = ptr(coef[0]), ptr(coef[1])
    return coef, None


def rb_weight_ranges(x_like, weight, g, dgrad, gate=None, gate_bwd=False):
    """[(device pointer, bytes, buffer)] of the pre-split weights a later fused launch will stream: the 3x3 convolution (weight, g) in the
    given direction and optionally the gate (gate = (gate_w, gate_g)). For the `prefetch` argument of the launch that runs just before it.
    The third element is the scratch tensor itself: whoever remembers a range (ops' cross-block links, baked into captured graphs as raw
    addresses) thereby keeps the memory allocated, whatever happens to the transformed-weight cache in between (evict_dead, a cleared
    cache, a precision switch) — a stale range is then touched uselessly, never a freed one."""
    d, need = _rb_desc(x_like, weight, g, dgrad)
    out = [(int(d.workspace), int(need), d._ws_tensor)] if need else []
    if gate is not None:
        e = RbExt()
        _rb_gate_ws(e, gate[0], gate[1], x_like.device, gate_bwd)
        out.append((int(e.gate_ws), int(e.gate_ws_bytes), e._ws_tensor))
    return out


def _rb_prefetch(e, prefetch):
    for i, rng in enumerate((prefetch or [])[:2]):
        e.pf_ptr[i], e.pf_bytes[i] = rng[0], rng[1]


def rb_conv(x, weight, g, bias, in_act, out_scale, in_bn=None, coef=None, stats_pivot=None, prefetch=None, nsplit=0):
    """y = (conv3x3(act(BN(x))) + bias) * out_scale with BatchNorm partials of y around stats_pivot (first half of a residual block).
    in_bn = (StatParts, pivot, bn) or coef = (scale, shift, ...) given. Returns (y, StatParts | None, coef).
    nsplit (here and in rb_gate_dgrad / rb_apply_dgrad): workgroups per tile, lvae_rb_ext.nsplit (0: the library decides; speed only)."""
    N, H, W, _ = x.shape
    y = torch.empty((N, H, W, g.Cout), dtype=torch.float32, device=x.device)
    d, _ = _rb_desc(x, weight, g, False, y, bias, None, None, in_act, out_scale)
    coef, keep = _in_bn(d, in_bn, x, coef=coef)
    parts = None
    if stats_pivot is not None:
        rows = _C.load().lvae_resblock_conv_rows(C.byref(d))
        buf = torch.empty((rows + 1, 2, g.Cout), dtype=torch.float32, device=x.device)
        parts = StatParts(buf, rows, True)
        d.stats_out, d.stats_pivot = ptr(buf), ptr(stats_pivot)
    e = RbExt()
    e.prologue, e.epilogue, e.nsplit = _C.RB_PRO_AFFINE, _C.RB_EPI_PLAIN, nsplit
    _rb_prefetch(e, prefetch)
    call('lvae_resblock_conv_f32', C.byref(d), C.byref(e), stream_ptr())
    del keep
    return y, parts, coef


def rb_gate_rows(x, weight, g, whole_image=True):
    """Workgroups (= statistics rows of `out`) of the forward conv + gate fusion for the 3x3 convolution (weight, g) on x: the whole-image
    kernels' shapes (counted as 0 with whole_image=False), or the 256-pixel six-product Winograd kernel's (fp32, 16x16 and 32x32 levels at
    batch 256). 0: not available."""
    d = _rb_query_desc(x, weight, g)
    if d is None:
        return 0
    rows = int(_C.load().lvae_resblock_conv_rows(C.byref(d)))
    if rows > 0:
        return rows if whole_image else 0
    _conv_ws(d, weight, x.device)   # the Winograd kernel's transformed weights: the buffer the plain convolution of this layer uses too
    return int(_C.load().lvae_resblock_conv_gate_rows(C.byref(d)))


def rb_conv_gate(x, weight, g, bias, in_act, out_scale, gate_w, gate_g, gate_bias, res, act, in_bn=None, coef=None, stats_pivot=None,
                 prefetch=None, want_ab=True):
    """Second half of a gated residual block in one launch: y2 = (conv3x3(act(BN(x))) + bias) * out_scale, ab = conv1x1(y2) + gate_bias,
    out = act(a) * sigmoid(b) + res, BatchNorm partials of out around stats_pivot. Returns (y2, ab, out, StatParts | None, coef).
    want_ab=False: ab is not stored and comes back as None (for a backward that forms it again, conv1x1_gate_bwd_wgrad_recompute; the
    Winograd kernel's gate epilogue only)."""
    N, H, W, _ = x.shape
    dev = x.device
    y = torch.empty((N, H, W, g.Cout), dtype=torch.float32, device=dev)
    out = torch.empty((N, H, W, gate_g.Cout // 2), dtype=torch.float32, device=dev)
    d, need = _rb_desc(x, weight, g, False, y, bias, None, None, in_act, out_scale)
    if need and not want_ab:
        raise _C.LvaeHipError("rb_conv_gate: the whole-image kernels always store ab")
    ab = torch.empty((N, H, W, gate_g.Cout), dtype=torch.float32, device=dev) if want_ab else None
    can_fold = True
    if not need:   # not a whole-image shape: the Winograd kernel with the gate behind it (its own transformed weights)
        _conv_ws(d, weight, dev)
        can_fold = bool(_C.load().lvae_conv2d_folds_bn_finalize(C.byref(d)))
    coef, keep = _in_bn(d, in_bn, x, can_fold, coef)
    e = RbExt()
    e.prologue, e.epilogue = _C.RB_PRO_AFFINE, _C.RB_EPI_GATE
    _rb_gate_ws(e, gate_w, gate_g, dev, False)
    e.gate_bias, e.act = ptr(gate_bias), ACT[act]
    e.res, e.ab, e.out = ptr(res), ptr(ab), ptr(out)
    parts = None
    if stats_pivot is not None:
        rows = _C.load().lvae_resblock_conv_gate_rows(C.byref(d))
        buf = torch.empty((rows + 1, 2, g.Cout), dtype=torch.float32, device=dev)
        parts = StatParts(buf, rows, True)
        e.out_stats, e.out_stats_pivot = ptr(buf), ptr(stats_pivot)
    _rb_prefetch(e, prefetch)
    call('lvae_resblock_conv_f32', C.byref(d), C.byref(e), stream_ptr())
    del keep
    return y, ab, out, parts, coef


def _rb_bn_bwd(d, bn_bwd, dx):
    """BatchNorm-backward sums of the dgrad result in the epilogue: bn_bwd = (x, coefficient block row 0, act). Returns the partial rows."""
    xb, coef0, act = bn_bwd
    rows = _C.load().lvae_resblock_conv_rows(C.byref(d))
    parts = torch.empty((rows, 2, dx.shape[3]), dtype=torch.float32, device=dx.device)
    d.stats_out, d.stats_pivot, d.stats_x = ptr(parts), ptr(coef0), ptr(xb)
    d.stats_mode, d.stats_act = 1, ACT[act]
    return parts


class BnBwdApply:
    """One BatchNorm-backward apply, dx = BN'(dh; x) [* drop] [+ add], from the partial rows `parts` the producer of dh left: what a fused
    launch that forms dx itself is handed (struct / fill_ext), what a block that does not launch its last apply leaves for the consumer
    of dx (ops.ResBlockFn), and the stand-alone launch (run). coef = (scale, shift, mean, rstd) as bn_stats / bn_finalize_parts return them;
    dgamma / dbeta are accumulated; drop: the Dropout2d mask (N, C); out: the fp32 tensor dx goes to (None: allocated when a launch stores it)."""
    __slots__ = ('parts', 'dh', 'x', 'coef', 'act', 'dgamma', 'dbeta', 'add', 'drop', 'out')

    def __init__(self, parts, dh, x, coef, act, dgamma, dbeta, add=None, drop=None, out=None):
        self.parts, self.dh, self.x, self.coef, self.act, self.dgamma, self.dbeta = parts, dh, x, tuple(coef), act, dgamma, dbeta
        self.add, self.drop, self.out = add, drop, out

    def _block(self):
        if not bn_coef_block(*self.coef):
            raise _C.LvaeHipError("BnBwdApply: a fused launch reads the four coefficient vectors as one (4, C) block")
        return self.coef[0]

    def _out(self):
        if self.out is None:
            self.out = torch.empty(self.x.shape, dtype=torch.float32, device=self.x.device)
        return ptr(self.out)

    def struct(self, M, store_out=True):
        """The lvae_bn_apply of a launch over M = N*H*W pixels (store_out=False: the launch forms dx without storing it)."""
        return _C.BnApply(ptr(self.parts), self.parts.shape[0], ACT[self.act], M, ptr(self._block()), ptr_dt(self.dh), ptr(self.x), ptr(self.add),
                          ptr(self.dgamma), ptr(self.dbeta), self._out() if store_out else None, int(self.dh.dtype == torch.bfloat16), 0,
                          ptr(self.drop))

    def fill_ext(self, e, which):
        """As a prologue of lvae_resblock_conv_f32: 'bwd' (RB_PRO_BN_APPLY: dh is the launch's x, out its xt_out) or 'ap' (deferred)."""
        head = ptr(self.parts), self.parts.shape[0], ACT[self.act], self.x.numel() // self.x.shape[-1], ptr(self._block()), ptr(self.x)
        if which == 'ap':
            e.ap_parts, e.ap_rows, e.ap_act, e.ap_M, e.ap_coef, e.ap_x = head
            e.ap_dh, e.ap_add, e.ap_dgamma, e.ap_dbeta, e.ap_out = ptr(self.dh), ptr(self.add), ptr(self.dgamma), ptr(self.dbeta), self._out()
        else:
            e.bwd_parts, e.bwd_rows, e.bwd_act, e.bwd_M, e.bwd_coef, e.bwd_x = head
            e.dgamma, e.dbeta, e.pro_drop, e.xt_out = ptr(self.dgamma), ptr(self.dbeta), ptr(self.drop), self._out()

    def run(self, out_bf16=False):
        """The apply as a launch of its own (any four coefficient vectors). Returns dx."""
        sc, sh, mean, rstd = self.coef
        return affine_act_bwd_parts(self.parts, self.dh, self.x, sc, sh, self.act, mean, rstd, self.dgamma, self.dbeta, drop=self.drop,
                                    add=self.add, out_bf16=out_bf16, out=self.out)


class PendingApply(BnBwdApply):
    """BnBwdApply as the existing tests construct it: coef0 = row 0 of the (4, C) coefficient block, add and out positional. The product
    code builds BnBwdApply; this form and _flat_apply stay so that those tests run unedited against the single description."""

    def __init__(self, parts, dh, x, coef0, act, dgamma, dbeta, add, out):
        Cn = coef0.numel()
        super().__init__(parts, dh, x, torch.as_strided(coef0, (4, Cn), (Cn, 1)).unbind(0), act, dgamma, dbeta, add=add, out=out)


def _flat_apply(args, drop=None, out=None):
    """(apply, the arguments behind it) of a wrapper's positional tail: a BnBwdApply, or in its place the seven values parts, dh, x, coef0,
    act, dgamma, dbeta (with drop / out as the wrapper got them) of the existing tests' calls."""
    if isinstance(args[0], BnBwdApply):
        return args[0], args[1:]
    apply = PendingApply(*args[:7], None, out)
    apply.drop = drop
    return apply, args[7:]


def rb_gate_dgrad(dout, ab, gate_w, gate_g, act, drop, weight, g, bn_bwd, prefetch=None, apply=None, nsplit=0):
    """Backward of rb_conv_gate up to the block's second BatchNorm in one launch: dab = gate'(dout, ab), dy2 = (dab . Wg^T) * drop,
    dh2 = dgrad3x3(dy2) with the BatchNorm-backward sums of bn_bwd = (y1, coef block row 0, act). Returns (dab, dy2, dh2, parts).
    apply (BnBwdApply): dout does not exist yet; the launch forms it in its prologue and stores it to apply.out (= dout's memory)."""
    N, H, W, Cn = dout.shape
    dev = dout.device
    dab = torch.empty_like(ab)
    dy2 = torch.empty((N, H, W, Cn), dtype=torch.float32, device=dev)
    dh = torch.empty((N, H, W, g.Cin), dtype=torch.float32, device=dev)
    d, _ = _rb_desc(dout, weight, g, True, dh)
    e = RbExt()
    e.prologue, e.epilogue, e.nsplit = _C.RB_PRO_GATE_BWD, _C.RB_EPI_PLAIN, nsplit
    _rb_gate_ws(e, gate_w, gate_g, dev, True)
    e.act = ACT[act]
    e.dout, e.ab_in, e.dab, e.pro_drop, e.xt_out = ptr(dout), ptr(ab), ptr(dab), ptr(drop), ptr(dy2)
    if apply is not None:
        apply.fill_ext(e, 'ap')
    parts = _rb_bn_bwd(d, bn_bwd, dh)
    _rb_prefetch(e, prefetch)
    call('lvae_resblock_conv_f32', C.byref(d), C.byref(e), stream_ptr())
    return dab, dy2, dh, parts


def rb_apply_dgrad(apply, *rest, bn_bwd, prefetch=None, nsplit=0):
    """BatchNorm backward (training mode) + Dropout2d mask + dgrad of the block's first convolution in one launch: dy1 = the apply
    (BnBwdApply, with the block's drop) stored to apply.out, dh1 = dgrad3x3(dy1) with the sums of bn_bwd = (x, coef block row 0, act).
    Called as rb_apply_dgrad(apply, weight, g, bn_bwd=...). Returns (dy1, dh1, parts)."""
    apply, rest = _flat_apply((apply,) + rest)
    if len(rest) == 3:   # (the flat form carries drop behind its seven values)
        apply.drop, rest = rest[0], rest[1:]
    weight, g = rest
    N, H, W, _ = apply.dh.shape
    dh = torch.empty((N, H, W, g.Cin), dtype=torch.float32, device=apply.dh.device)
    d, _ = _rb_desc(apply.dh, weight, g, True, dh)
    e = RbExt()
    e.prologue, e.epilogue, e.nsplit = _C.RB_PRO_BN_APPLY, _C.RB_EPI_PLAIN, nsplit
    apply.fill_ext(e, 'bwd')
    parts = _rb_bn_bwd(d, bn_bwd, dh)
    _rb_prefetch(e, prefetch)
    call('lvae_resblock_conv_f32', C.byref(d), C.byref(e), stream_ptr())
    return apply.out, dh, parts


def bn_coef_block(scale, shift, mean, rstd):
    """True when the four coefficient vectors are consecutive rows of one buffer (as bn_stats / bn_finalize_parts return them)."""
    if scale is None or shift is None or mean is None or rstd is None:
        return False
    n = 4 * scale.numel()
    p0 = scale.data_ptr()
    return shift.data_ptr() == p0 + n and mean.data_ptr() == p0 + 2 * n and rstd.data_ptr() == p0 + 3 * n


def affine_act_bwd_parts(parts, dh, x, scale, shift, act, mean, rstd, dgamma, dbeta, drop=None, add=None, out_bf16=False, out=None):
    """affine_act_bwd (training-mode BatchNorm) with the reduction already done by the epilogue of the convolution that produced dh
    (conv2d_dgrad(..., bn_bwd=...)). out: write into this tensor instead of a new one."""
    Cn = x.shape[-1]
    M = x.numel() // Cn
    dx = out if out is not None else torch.empty(x.shape, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=x.device)
    ws = workspace(8 * Cn, x.device)
    rows_per_n = M // x.shape[0]
    dtypes = _dt(dh) | (_dt(x) << 1) | (_dt(dx) << 2)
    call('lvae_affine_act_bwd_parts_f32', ptr(parts), parts.shape[0], ptr_dt(dh), ptr_dt(x), M, Cn, ptr(scale), ptr(shift), ACT[act],
         ptr(mean), ptr(rstd), ptr(dgamma), ptr(dbeta), ptr(drop), rows_per_n, ptr(add), ptr_dt(dx), ws.data_ptr(), ws.numel(),
         dtypes, stream_ptr())
    return dx


def conv2d_dgrad(dy, weight, g, in_hw, out_scale=None, ci_range=None, bn_bwd=None, out_bf16=False):
    """Gradient w.r.t. the conv input (before any fused input transform). dy NHWC (N,OH,OW,Cout) -> (N,H,W,Cin).
    out_scale (N,Cin) multiplies the result per (sample, channel) (Dropout2d mask of the producer).
    ci_range=(a,b) restricts the result to input channels [a,b) (the two halves of a fused channel concat)."""
    _chk_nhwc(dy, 'dy')
    N, OH, OW, Co = dy.shape
    H, W = in_hw
    a, b = ci_range if ci_range is not None else (0, g.Cin)
    dx = torch.empty((N, H, W, b - a), dtype=torch.bfloat16 if out_bf16 else torch.float32, device=dy.device)
    d = _desc(g, weight, dy, None, N, OH, OW, H, W, b - a, g.s_co, g.s_ci,
              GATHER_CONV if g.transposed else GATHER_TRANSPOSED, out_scale=out_scale, y=dx)
    d.w = ptr(weight) + 4 * a * g.s_ci
    _conv_ws(d, weight, dy.device)
    if bn_bwd is None:
        call('lvae_conv2d_f32', C.byref(d), stream_ptr())
        return dx
    # bn_bwd = (x, scale, act): dx is the gradient w.r.t. act(BN(x)); ask the epilogue for the BatchNorm-backward partials
    # (scale must be the first row of the (4, C) coefficient block, see bn_coef_block). Returns (dx, parts | None).
    xb, coef, act = bn_bwd
    parts = None
    rows = _C.load().lvae_conv2d_stats_rows(C.byref(d))
    if rows > 0 and out_scale is None and ci_range is None and tuple(xb.shape) == tuple(dx.shape):
        parts = torch.empty((rows, 2, b - a), dtype=torch.float32, device=dy.device)
        d.stats_out, d.stats_pivot, d.stats_x = ptr(parts), ptr(coef), ptr_dt(xb)
        d.stats_mode, d.stats_act, d.stats_x_dtype = 1, ACT[act], _dt(xb)
    call('lvae_conv2d_f32', C.byref(d), stream_ptr())
    return dx, parts


def conv2d_wgrad_apply_ok(x, weight, g):
    """True when conv2d_wgrad_apply takes the 3x3 convolution (weight, g) on input x (the Winograd-domain fp32 weight gradient of a
    64 -> 64 layer at the >= 16x16 levels)."""
    if precision != PREC_F32 or x.dtype != torch.float32 or x.dim() != 4 or g.transposed or _ddi is not None:
        return False
    N, H, W, _ = x.shape
    d = _desc(g, weight, x, None, N, H, W, H, W, g.Cout, g.s_ci, g.s_co, GATHER_CONV)
    return bool(_C.load().lvae_conv2d_wgrad_apply_ok(C.byref(d)))


def conv2d_wgrad_apply(x, weight, g, dweight, dbias, *apply, drop=None, in_scale=None, in_shift=None, in_act=None):
    """conv2d_wgrad whose dy operand is the BatchNorm-backward apply that has not run: dy = apply.run() (a BnBwdApply, with the block's drop)
    is formed inside the weight-gradient kernel, stored to apply.out and returned (the dgrad that follows reads it). Only where
    conv2d_wgrad_apply_ok(). Called as conv2d_wgrad_apply(x, weight, g, dweight, dbias, apply, ...)."""
    apply, _ = _flat_apply(apply, drop)
    _chk_nhwc(x, 'x')
    N, H, W, _ = x.shape
    if tuple(dweight.stride()) != tuple(weight.stride()):
        raise _C.LvaeHipError("conv2d_wgrad_apply: gradient strides differ from weight strides")
    d = _desc(g, weight, x, None, N, H, W, H, W, g.Cout, g.s_ci, g.s_co, GATHER_CONV, None, in_scale, in_shift, in_act)
    need = _C.load().lvae_conv2d_wgrad_workspace(C.byref(d))
    ws = workspace(need, x.device)
    ap = apply.struct(N * H * W)
    call('lvae_conv2d_wgrad_apply_f32', C.byref(d), C.byref(ap), ptr(dweight), ptr(dbias), ws.data_ptr(), ws.numel(), stream_ptr())
    return apply.out


def _wgrad_pair_descs(x_a, w_a, g_a, x_b, w_b, g_b, in_a=(None, None, None), in_b=(None, None, None)):
    """The descriptors of a residual block's two weight gradients (A: conv1 on x_a, B: conv2 on x_b), None where the shapes cannot be a pair."""
    if precision != PREC_F32 or _ddi is not None or g_a.transposed or g_b.transposed:
        return None
    if x_a.dim() != 4 or x_b.dim() != 4:
        return None
    N, H, W, _ = x_a.shape
    d_a = _desc(g_a, w_a, x_a, None, N, H, W, H, W, g_a.Cout, g_a.s_ci, g_a.s_co, GATHER_CONV, None, *in_a)
    N, H, W, _ = x_b.shape
    d_b = _desc(g_b, w_b, x_b, None, N, H, W, H, W, g_b.Cout, g_b.s_ci, g_b.s_co, GATHER_CONV, None, *in_b)
    return d_a, d_b


def conv2d_wgrad_pair_ok(x_a, w_a, g_a, x_b, w_b, g_b):
    """True when conv2d_wgrad_pair takes the two 3x3 convolutions of a residual block (conv1 = (w_a, g_a) on x_a, conv2 = (w_b, g_b) on x_b)."""
    ds = _wgrad_pair_descs(x_a, w_a, g_a, x_b, w_b, g_b)
    return ds is not None and bool(_C.load().lvae_conv2d_wgrad_pair_ok(C.byref(ds[0]), C.byref(ds[1])))


def conv2d_wgrad_pair_schedule(x_a, w_a, g_a, x_b, w_b, g_b):
    """((ranges, chunks per range, workgroups) of A, the same of B) as the pair launch splits the chip, or None where it declines. No launch."""
    ds = _wgrad_pair_descs(x_a, w_a, g_a, x_b, w_b, g_b)
    out = (C.c_int32 * 6)()
    if ds is None or not _C.load().lvae_conv2d_wgrad_pair_schedule(C.byref(ds[0]), C.byref(ds[1]), out):
        return None
    return tuple(out[:3]), tuple(out[3:])


def conv2d_wgrad_pair(x, weight, g, dweight, dbias, *rest, drop=None, out=None, in_scale=None, in_shift=None, in_act=None, in_scale_b=None,
                      in_shift_b=None, in_act_b=None):
    """conv2d_wgrad_apply(x, weight, g, dweight, dbias, apply, ...) and conv2d_wgrad(apply.x, dy_b, weight_b, g_b, dweight_b, dbias_b,
    in_scale_b ...) of one residual block as one launch and one slab reduce (conv2 reads the tensor whose BatchNorm conv1's apply
    differentiates). Returns the stored dy of A (apply.out). Only where conv2d_wgrad_pair_ok(). Called as conv2d_wgrad_pair(x, weight, g,
    dweight, dbias, apply, dy_b, weight_b, g_b, dweight_b, dbias_b, ...)."""
    apply, (dy_b, weight_b, g_b, dweight_b, dbias_b) = _flat_apply(rest, drop, out)
    xbn = apply.x
    _chk_nhwc(x, 'x')
    _chk_nhwc(xbn, 'xbn')
    _chk_nhwc(dy_b, 'dy_b')
    N, H, W, _ = x.shape
    if tuple(dweight.stride()) != tuple(weight.stride()) or tuple(dweight_b.stride()) != tuple(weight_b.stride()):
        raise _C.LvaeHipError("conv2d_wgrad_pair: gradient strides differ from weight strides")
    ds = _wgrad_pair_descs(x, weight, g, xbn, weight_b, g_b, (in_scale, in_shift, in_act), (in_scale_b, in_shift_b, in_act_b))
    if ds is None:
        raise _C.LvaeHipError("conv2d_wgrad_pair: not a pair (fp32 precision, plain convolutions)")
    d_a, d_b = ds
    d_b.y_dtype = _dt(dy_b)
    need = _C.load().lvae_conv2d_wgrad_pair_workspace(C.byref(d_a), C.byref(d_b))
    ws = workspace(need, x.device)
    ap = apply.struct(N * H * W)
    call('lvae_conv2d_wgrad_pair_f32', C.byref(d_a), C.byref(ap), C.byref(d_b), ptr_dt(dy_b), ptr(dweight), ptr(dbias), ptr(dweight_b), ptr(dbias_b),
         ws.data_ptr(), ws.numel(), stream_ptr())
    return apply.out


def conv1x1_dgrad_cat(dy, weight, g, C1):
    """Both halves of the input gradient of a 1x1 / stride-1 convolution whose input was the channel concat (x [.., C1], x2 [.., Cin - C1]),
    in one launch: returns (dx, dx2), or None when the shape is not the single-shot 1x1 kernel's (the caller launches one dgrad per half)."""
    _chk_nhwc(dy, 'dy')
    N, H, W, _ = dy.shape
    if not 0 < C1 < g.Cin:
        return None
    dx = torch.empty((N, H, W, C1), dtype=torch.float32, device=dy.device)
    dx2 = torch.empty((N, H, W, g.Cin - C1), dtype=torch.float32, device=dy.device)
    d = _desc(g, weight, dy, None, N, H, W, H, W, g.Cin, g.s_co, g.s_ci, GATHER_TRANSPOSED, y=dx)
    if not _C.load().lvae_conv1x1_dgrad_cat_ok(C.byref(d), C1):
        return None
    call('lvae_conv1x1_dgrad_cat_f32', C.byref(d), ptr(dx2), C1, stream_ptr())
    return dx, dx2


def _cat_bwd_desc(dy_like, weight, g, C1, dweight):
    """The dgrad view over the concat that the persistent merge backward is asked about, for the 1x1 convolution (weight, g) whose output
    (and output gradient) is shaped like dy_like (N,H,W,Cout); None where Python alone can tell that it does not apply."""
    if _ddi is not None or dy_like.dim() != 4 or g.transposed or dy_like.dtype != torch.float32 or not 0 < C1 < g.Cin:
        return None
    if dweight is not None and tuple(dweight.stride()) != tuple(weight.stride()):
        return None
    N, H, W, _ = dy_like.shape
    return _desc(g, weight, dy_like, None, N, H, W, H, W, g.Cin, g.s_co, g.s_ci, GATHER_TRANSPOSED)


def cat_bwd_ws(dy_like, weight, g, C1, dweight=None):
    """Scratch bytes conv1x1_cat_bwd needs for the merge convolution (weight, g) with an output shaped like dy_like; 0: not taken."""
    d = _cat_bwd_desc(dy_like, weight, g, C1, dweight)
    return int(_C.load().lvae_conv1x1_cat_bwd_workspace(C.byref(d), C1)) if d is not None else 0


def cat_bwd_apply_ok(dy_like, weight, g, C1, dweight=None):
    """True when conv1x1_cat_bwd takes the merge convolution (weight, g) with a deferred BatchNorm-backward apply (BnBwdApply) as its dy."""
    d = _cat_bwd_desc(dy_like, weight, g, C1, dweight)
    return d is not None and bool(_C.load().lvae_conv1x1_cat_bwd_apply_ok(C.byref(d), C1))


def conv1x1_cat_bwd(dy, x, x2, weight, g, dweight, dbias, apply=None, store_dy=False, max_workgroups=0, scratch=None):
    """The whole backward of a 1x1 convolution over the channel concat (x, x2) in one persistent kernel (+ its slab reduce): returns (dx, dx2)
    and accumulates into dweight / dbias; None, with nothing launched or written, when the library does not take it (the caller runs
    conv2d_wgrad + conv1x1_dgrad_cat). apply (BnBwdApply): dy does not exist yet (dy is apply.out, unwritten); the kernel forms it from
    the deferred BatchNorm-backward apply and stores it to apply.out only with store_dy. max_workgroups caps the grid (0: default);
    scratch: a uint8 buffer to use instead of the shared workspace (too small: None)."""
    _chk_nhwc(dy, 'dy')
    C1 = x.shape[3]
    d = _cat_bwd_desc(dy, weight, g, C1, dweight)
    if d is None or x.dtype != torch.float32 or x2 is None or x2.dtype != torch.float32 or tuple(x.shape[:3]) != tuple(dy.shape[:3]) or \
            tuple(x2.shape[:3]) != tuple(dy.shape[:3]) or x2.shape[3] != g.Cin - C1 or not (x.is_contiguous() and x2.is_contiguous()):
        return None
    lib = _C.load()
    need = lib.lvae_conv1x1_cat_bwd_workspace(C.byref(d), C1)
    if not need or (apply is not None and (not lib.lvae_conv1x1_cat_bwd_apply_ok(C.byref(d), C1) or apply.dh.dtype != torch.float32)):
        return None
    ws = scratch if scratch is not None else workspace(need, dy.device)
    if ws.numel() < need or ws.data_ptr() % 16 or any(t is not None and t.data_ptr() % 16 for t in (x, x2)):
        return None
    N, H, W, _ = dy.shape
    ap = None
    if apply is not None:
        d.x = None
        ap = apply.struct(N * H * W, store_out=store_dy)
    dx = torch.empty((N, H, W, C1), dtype=torch.float32, device=dy.device)
    dx2 = torch.empty((N, H, W, g.Cin - C1), dtype=torch.float32, device=dy.device)
    call('lvae_conv1x1_cat_bwd_f32', C.byref(d), ptr(x), ptr(x2), ptr(dx), ptr(dx2), ptr(dweight), ptr(dbias),
         C.byref(ap) if ap is not None else None, ws.data_ptr(), ws.numel(), int(max_workgroups), stream_ptr())
    return dx, dx2


def conv2d_wgrad(x, dy, weight, g, dweight, dbias=None, x2=None, in_scale=None, in_shift=None, in_act=None):
    """dweight += d/dw, dbias += d/db for the convolution of `conv2d` with the same fused input transform.
    dweight must have the same strides as weight (a view of the gradient arena)."""
    _chk_nhwc(x, 'x')
    _chk_nhwc(dy, 'dy')
    N, H, W, _ = x.shape
    OH, OW = dy.shape[1], dy.shape[2]
    if tuple(dweight.stride()) != tuple(weight.stride()):
        raise _C.LvaeHipError("conv2d_wgrad: gradient strides %s differ from weight strides %s" %
                              (tuple(dweight.stride()), tuple(weight.stride())))
    d = _desc(g, weight, x, x2, N, H, W, OH, OW, g.Cout, g.s_ci, g.s_co,
              GATHER_TRANSPOSED if g.transposed else GATHER_CONV, None, in_scale, in_shift, in_act)
    d.y_dtype = _dt(dy)
    need = _C.load().lvae_conv2d_wgrad_workspace(C.byref(d))
    ws = workspace(need, x.device)
    call('lvae_conv2d_wgrad_f32', C.byref(d), ptr_dt(dy), ptr(dweight), ptr(dbias), ws.data_ptr(), ws.numel(), stream_ptr())   # dy's type: d.y_dtype


def _wgrad_item_arrays(items, who):
    """The descriptor array and the dy / dw / db pointer arrays of (x, dy, weight, g, dweight, dbias, kw) entries."""
    n = len(items)
    descs = (ConvDesc * n)()
    dys, dws, dbs = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_void_p * n)()
    for i, (x, dy, weight, g, dweight, dbias, kw) in enumerate(items):
        _chk_nhwc(x, 'x')
        _chk_nhwc(dy, 'dy')
        if tuple(dweight.stride()) != tuple(weight.stride()):
            raise _C.LvaeHipError("%s: gradient strides %s differ from weight strides %s" %
                                  (who, tuple(dweight.stride()), tuple(weight.stride())))
        N, H, W, _ = x.shape
        d = _desc(g, weight, x, kw.get('x2'), N, H, W, dy.shape[1], dy.shape[2], g.Cout, g.s_ci, g.s_co,
                  GATHER_TRANSPOSED if g.transposed else GATHER_CONV, None, kw.get('in_scale'), kw.get('in_shift'), kw.get('in_act'))
        d.y_dtype = _dt(dy)
        C.memmove(C.byref(descs, i * C.sizeof(ConvDesc)), C.byref(d), C.sizeof(ConvDesc))
        dys[i], dws[i], dbs[i] = ptr_dt(dy), ptr(dweight), ptr(dbias)
    return descs, dys, dws, dbs


def _wgrad_shared_descs(convs):
    """The descriptors of (x, weight, g) stride-1 'same' convolutions with fp32 dy, None where they cannot share a launch anyway."""
    if precision != PREC_F32 or _ddi is not None or not 1 <= len(convs) <= 3:
        return None
    descs = (ConvDesc * len(convs))()
    for i, (x, weight, g) in enumerate(convs):
        if x.dim() != 4 or x.dtype != torch.float32 or g.transposed:
            return None
        N, H, W, _ = x.shape
        d = _desc(g, weight, x, None, N, H, W, H, W, g.Cout, g.s_ci, g.s_co, GATHER_CONV)
        C.memmove(C.byref(descs, i * C.sizeof(ConvDesc)), C.byref(d), C.sizeof(ConvDesc))
    return descs


def conv2d_wgrad_shared_ok(convs, routed=False):
    """True when conv2d_wgrad_shared takes the weight gradients of these 1 to 3 convolutions, each (x, weight, g), in one launch (the 3x3
    convolutions of a stochastic layer at the 16x16 level: the Winograd-domain fp32 weight gradient, one N, H, W). routed: only where
    the 64-channel gradients among them — there has to be one — run in that kernel family alone too (the 8x8 level's go to the
    whole-image kernel and stay there); a 32-channel gradient enters the family through this launch only."""
    descs = _wgrad_shared_descs(convs)
    if descs is None or not _C.load().lvae_conv2d_wgrad_shared_ok(descs, None, len(convs)):
        return False
    if not routed:
        return True
    wide = [i for i in range(len(convs)) if descs[i].C1 == 64]
    return bool(wide) and all(_C.load().lvae_conv2d_wgrad_variant(C.byref(descs[i])) == _C.WGRAD_VARIANT_WINO for i in wide)


def conv2d_wgrad_shared_schedule(convs):
    """((ranges, chunks per range, workgroups) of each problem) as the shared launch splits the chip, or None where it declines. No launch."""
    descs = _wgrad_shared_descs(convs)
    out = (C.c_int32 * (3 * len(convs)))()
    if descs is None or not _C.load().lvae_conv2d_wgrad_shared_schedule(descs, None, len(convs), out):
        return None
    return tuple(tuple(out[3 * i:3 * i + 3]) for i in range(len(convs)))


def conv2d_wgrad_shared(items):
    """conv2d_wgrad of 1 to 3 entries (x, dy, weight, g, dweight, dbias, kw), kw: in_scale / in_shift / in_act, as one launch and one slab
    reduce. Only where conv2d_wgrad_shared_ok()."""
    n = len(items)
    descs, dys, dws, dbs = _wgrad_item_arrays(items, 'conv2d_wgrad_shared')
    need = _C.load().lvae_conv2d_wgrad_shared_workspace(descs, n)
    ws = workspace(need, items[0][0].device)
    call('lvae_conv2d_wgrad_shared_f32', descs, C.cast(dys, C.c_void_p), C.cast(dws, C.c_void_p), C.cast(dbs, C.c_void_p), n,
         ws.data_ptr(), ws.numel(), stream_ptr())


def conv2d_wgrad_grouped(items):
    """items: list of (x, dy, weight, g, dweight, dbias, kw) exactly as for conv2d_wgrad (kw: x2 / in_scale / in_shift /
    in_act). One C call; gradients that share a kernel variant are launched together."""
    n = len(items)
    descs, dys, dws, dbs = _wgrad_item_arrays(items, 'conv2d_wgrad_grouped')
    need = _C.load().lvae_conv2d_wgrad_grouped_workspace(descs, n)
    ws = workspace(need, items[0][0].device)
    call('lvae_conv2d_wgrad_grouped_f32', descs, C.cast(dys, C.c_void_p), C.cast(dws, C.c_void_p), C.cast(dbs, C.c_void_p), n,
         ws.data_ptr(), ws.numel(), stream_ptr())


# ----------------------------------------------------------------------------------------------------------------
def bn_stats(x, gamma, beta, running_mean, running_var, eps=1e-5, momentum=0.1):
    """Training-mode BatchNorm statistics of NHWC x. Returns (scale, shift, mean, rstd), each (C,)."""
    Cn = x.shape[-1]
    M = x.numel() // Cn
    out = torch.empty((4, Cn), dtype=torch.float32, device=x.device)
    need = _C.load().lvae_bn_stats_workspace(M, Cn)
    ws = workspace(need, x.device)
    call('lvae_bn_stats_f32', ptr(x), M, Cn, ptr(gamma), ptr(beta), eps, momentum, ptr(running_mean), ptr(running_var),
         ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), ws.data_ptr(), ws.numel(), stream_ptr())
    return out[0], out[1], out[2], out[3]


def bn_finalize_parts(parts, M, pivot, gamma, beta, running_mean, running_var, eps=1e-5, momentum=0.1):
    """BatchNorm coefficients from the partials a convolution epilogue wrote (conv2d(..., stats_pivot=pivot)); same outputs and
    running-statistics update as bn_stats. pivot may be running_mean itself."""
    rows, _, Cn = parts.shape
    out = torch.empty((4, Cn), dtype=torch.float32, device=parts.device)
    call('lvae_bn_finalize_parts_f32', ptr(parts), rows, M, Cn, ptr(pivot), ptr(gamma), ptr(beta), eps, momentum,
         ptr(running_mean), ptr(running_var), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), stream_ptr())
    return out[0], out[1], out[2], out[3]


def bn_eval_coeffs(gamma, beta, running_mean, running_var, eps=1e-5):
    Cn = running_mean.numel()
    out = torch.empty((2, Cn), dtype=torch.float32, device=running_mean.device)
    call('lvae_bn_eval_coeffs_f32', Cn, ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), eps, ptr(out[0]),
         ptr(out[1]), stream_ptr())
    return out[0], out[1]


def affine_act(x, scale, shift, act, row_scale=None):
    Cn = x.shape[-1]
    M = x.numel() // Cn
    y = torch.empty_like(x)
    rows_per_n = M // x.shape[0]
    call('lvae_affine_act_f32', ptr(x), M, Cn, ptr(scale), ptr(shift), ACT[act], ptr(row_scale), rows_per_n, ptr(y),
         stream_ptr())
    return y


def affine_act_bwd(dh, x, scale, shift, act, bn_train, mean=None, rstd=None, dgamma=None, dbeta=None, drop=None, add=None):
    Cn = x.shape[-1]
    M = x.numel() // Cn
    dx = torch.empty_like(x)
    need = _C.load().lvae_bn_stats_workspace(M, Cn)
    ws = workspace(need, x.device)
    rows_per_n = M // x.shape[0]
    call('lvae_affine_act_bwd_f32', ptr(dh), ptr(x), M, Cn, ptr(scale), ptr(shift), ACT[act], int(bool(bn_train)),
         ptr(mean), ptr(rstd), ptr(dgamma), ptr(dbeta), ptr(drop), rows_per_n, ptr(add), ptr(dx), ws.data_ptr(),
         ws.numel(), stream_ptr())
    return dx


def gate_fwd(ab, res, act):
    Cn = ab.shape[-1] // 2
    M = ab.numel() // (2 * Cn)
    out = torch.empty(ab.shape[:-1] + (Cn,), dtype=torch.float32, device=ab.device)
    call('lvae_gate_fwd_f32', ptr(ab), ptr(res), M, Cn, ACT[act], ptr(out), stream_ptr())
    return out


def gate_bwd(dout, ab, act):
    Cn = ab.shape[-1] // 2
    M = ab.numel() // (2 * Cn)
    dab = torch.empty_like(ab)
    call('lvae_gate_bwd_f32', ptr(dout), ptr(ab), M, Cn, ACT[act], ptr(dab), stream_ptr())
    return dab


def act_bwd_from_out(dy, y, act):
    dx = torch.empty_like(y)
    call('lvae_act_bwd_from_out_f32', ptr(dy), ptr(y), y.numel(), ACT[act], ptr(dx), stream_ptr())
    return dx


def add(a, b):
    out = torch.empty_like(a)
    call('lvae_add_f32', ptr(a), ptr(b), a.numel(), ptr(out), stream_ptr())
    return out


def fill(t, value=0.0):
    """t[...] = value with our own kernel (t contiguous float32, 16-byte aligned): the gradient arena's zero_grad."""
    call('lvae_fill_f32', ptr(t), t.numel(), float(value), stream_ptr())
    return t


def fill_zero(t):
    """zero a (small) tensor with our own kernel: out = 0 * out is not safe for NaN garbage, so scale_rows_add of a cached zero"""
    z = _zeros_like_cached(t)
    call('lvae_scale_rows_add_f32', ptr(z), None, 1, 1, None, t.numel(), ptr(t), stream_ptr())
    return t


_zero_cache = {}


def _zeros_like_cached(t):
    key = (t.device, t.numel())
    if key not in _zero_cache:
        _zero_cache[key] = torch.zeros(t.numel(), dtype=torch.float32, device=t.device)
    return _zero_cache[key]


def add3(a, b, c):
    out = torch.empty_like(a)
    call('lvae_add3_f32', ptr(a), ptr(b), ptr(c), a.numel(), ptr(out), stream_ptr())
    return out


def sum_of_row_means(x_ln):
    L, N = x_ln.shape
    out = torch.empty((1,), dtype=torch.float32, device=x_ln.device)
    call('lvae_sum_of_row_means_f32', ptr(x_ln), L, N, ptr(out), stream_ptr())
    return out


def scale_rows_add(a, row_scale, b, out=None):
    """out = a * row_scale[n, c] + b  (either optional; with neither it is a device copy into `out`)."""
    Cn = a.shape[-1]
    M = a.numel() // Cn
    if out is None:
        out = torch.empty_like(a)
    call('lvae_scale_rows_add_f32', ptr(a), ptr(row_scale), M // a.shape[0], Cn, ptr(b), M, ptr(out), stream_ptr())
    return out


def colsum(x2d, out, accumulate):
    R, P = x2d.shape
    call('lvae_colsum_f32', ptr(x2d), R, P, ptr(out), int(bool(accumulate)), stream_ptr())


# ----------------------------------------------------------------------------------------------------------------
def _stoch_outputs(N, H, W, Z, dev, rows, with_ks=True):
    """What every form of the stochastic core writes: z (N,H,W,Z), small = the (N,) rows logprob_p, logprob_q, kl_samplewise (rows, where
    given, takes the places of the first and the last) and kl_spatial (N,H,W), or None without it."""
    z = torch.empty((N, H, W, Z), dtype=torch.float32, device=dev)
    small = torch.empty((3, N), dtype=torch.float32, device=dev)
    if rows is not None:
        small = [rows[0], small[1], rows[1]]
    ks = torch.empty((N, H, W), dtype=torch.float32, device=dev) if with_ks else None
    return z, small, ks


def normal_stochastic_fwd(p, q, eps_or_z, mode, analytical_kl, Z, N, rows=None):
    """p (N|1,H,W,2Z), q (N,H,W,2Z)|None. Returns z (N,H,W,Z), logprob_p, logprob_q, kl_samplewise (N,), kl_spatial (N,H,W).
    rows = (logprob_p row, kl row): (N,) views of the model's [L][N] matrices the kernel writes into directly (no stacking copies)."""
    p_bcast = int(p.shape[0] == 1 and N > 1)
    _, H, W, _ = p.shape
    z, small, ks = _stoch_outputs(N, H, W, Z, p.device, rows, with_ks=q is not None)
    call('lvae_normal_stochastic_fwd_f32', ptr(p), p_bcast, ptr(q), ptr(eps_or_z), N, H * W, Z, mode, int(bool(analytical_kl)),
         ptr(z), ptr(small[0]), ptr(small[1]) if q is not None else None, ptr(small[2]) if q is not None else None, ptr(ks),
         stream_ptr())
    if q is None:
        return z, small[0], None, None, None
    return z, small[0], small[1], small[2], ks


def normal_stochastic_res_fwd(p, d, eps_or_z, mode, analytical_kl, Z, N, rows=None, need_q=True):
    """The core with the posterior given as an offset from the prior (csrc/stochastic_residual.hip): p (N|1,H,W,2Z), d (N,H,W,2Z) =
    (dmu | dlv). Returns z, logprob_p, logprob_q, kl_samplewise, kl_spatial as normal_stochastic_fwd (rows alike) and q_out (N,H,W,2Z) =
    p + d, or None with need_q=False: the kernel then writes nothing for it."""
    p_bcast = int(p.shape[0] == 1 and N > 1)
    _, H, W, _ = p.shape
    z, small, ks = _stoch_outputs(N, H, W, Z, p.device, rows)
    q_out = torch.empty((N, H, W, 2 * Z), dtype=torch.float32, device=p.device) if need_q else None
    call('lvae_normal_stochastic_res_fwd_f32', ptr(p), p_bcast, ptr(d), ptr(eps_or_z), N, H * W, Z, mode, int(bool(analytical_kl)),
         ptr(z), ptr(q_out), ptr(small[0]), ptr(small[1]), ptr(small[2]), ptr(ks), stream_ptr())
    return z, small[0], small[1], small[2], ks, q_out


def normal_stochastic_res_bwd(p, d, eps, z, dz, g_lp, g_lq, g_kl, g_ks, mode, analytical_kl, Z):
    """Returns dp, the total gradient of the prior parameters (N,H,W,2Z: the caller sums a broadcast p over N), and dd, the offset's."""
    N, H, W, _ = d.shape
    p_bcast = int(p.shape[0] == 1 and N > 1)
    dp = torch.empty((N, H, W, 2 * Z), dtype=torch.float32, device=d.device)
    dd = torch.empty_like(dp)
    call('lvae_normal_stochastic_res_bwd_f32', ptr(p), p_bcast, ptr(d), ptr(eps), ptr(z), ptr(dz), ptr(g_lp), ptr(g_lq),
         ptr(g_kl), ptr(g_ks), N, H * W, Z, mode, int(bool(analytical_kl)), ptr(dp), ptr(dd), stream_ptr())
    return dp, dd


# Fused stochastic block of the low-resolution levels (csrc/stoch_img.hip, lvae_stoch_block_fwd_f32)
def _stoch_block_desc(x_p, cv_p, p_given, x_q, cv_q, cv_out, eps_or_z, mode, analytical_kl, N, attach=True):
    """The lvae_stoch_block of one call, without output tensors; None where Python alone can tell that the fused launch does not apply.
    cv_*: (weight, ConvGeom, bias) of conv_in_p (None: the block has none and p_given is p_params), conv_in_q, conv_out. attach: register the
    three weights' pre-split planes (a query must not register weights the caller may never run through this kernel)."""
    if _ddi is not None or x_q is None or x_q.dim() != 4 or x_q.dtype != torch.float32 or not x_q.is_contiguous():
        return None
    _, H, W, _ = x_q.shape
    b = _C.StochBlock()
    keep = []
    for name, cv, x, cin in (('conv_p', cv_p, x_p, None), ('conv_q', cv_q, x_q, None), ('conv_out', cv_out, None, cv_out[1].Cin)):
        if cv is None:
            continue
        w, g, bias = cv
        if g.transposed or (x is not None and (x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous() or tuple(x.shape[:3]) != (N, H, W))):
            return None
        d = ConvDesc()
        d.x = ptr(x)
        d.C1 = x.shape[3] if x is not None else cin
        d.w, d.w_stap, d.w_sk, d.w_sn, d.bias = ptr(w), g.s_tap, g.s_ci, g.s_co, ptr(bias)
        d.N, d.H, d.W, d.OH, d.OW, d.Cout = N, H, W, H, W, g.Cout
        d.KH, d.KW, d.stride, d.pad, d.gather, d.precision = g.KH, g.KW, g.stride, g.pad, GATHER_CONV, precision
        if d.C1 != g.Cin:
            return None
        if attach:
            need = _C.load().lvae_stoch_block_workspace(C.byref(d))
            if not need:
                return None
            prepared.attach(d, w, x_q.device, need, 'lvae_stoch_block_prepare_entry')
            keep.append(d._ws_tensor)
        setattr(b, name, d)
    if cv_p is None:
        if p_given is None or p_given.dim() != 4 or p_given.dtype != torch.float32 or not p_given.is_contiguous() or tuple(p_given.shape[1:3]) != (H, W):
            return None
        b.p_given, b.p_bcast = ptr(p_given), int(p_given.shape[0] == 1 and N > 1)
        if p_given.shape[0] not in (1, N) or p_given.shape[3] != cv_q[1].Cout:
            return None
    b.mode, b.analytical_kl, b.eps = mode, int(bool(analytical_kl)), ptr(eps_or_z)
    b._keep = keep
    return b


def stoch_block_ok(x_p, cv_p, p_given, x_q, cv_q, cv_out, mode, N):
    """True when stoch_block_fwd takes this call (lvae_stoch_block_ok): 3x3 / stride 1 / pad 1 convolutions, 64 input channels, Z = 32, H*W a
    divisor of 64, fp32 NHWC tensors, 16-byte aligned operands and weight views, q present, mode 0..2."""
    b = _stoch_block_desc(x_p, cv_p, p_given, x_q, cv_q, cv_out, None, mode, False, N, attach=False)
    return b is not None and bool(_C.load().lvae_stoch_block_ok(C.byref(b)))


def stoch_block_fwd(x_p, cv_p, p_given, x_q, cv_q, cv_out, eps_or_z, mode, analytical_kl, N, rows=None):
    """The stochastic block of a low-resolution level in one launch: p_params = conv_in_p(x_p) (or p_given), q_params = conv_in_q(x_q), the
    core of normal_stochastic_fwd, out = conv_out(z). Returns (out, z, p_params, q_params, logprob_p, logprob_q, kl_samplewise, kl_spatial);
    rows as in normal_stochastic_fwd. Only where stoch_block_ok()."""
    b = _stoch_block_desc(x_p, cv_p, p_given, x_q, cv_q, cv_out, eps_or_z, mode, analytical_kl, N)
    if b is None:
        raise _C.LvaeHipError("stoch_block_fwd: not a call of the fused stochastic block (ask stoch_block_ok first)")
    _, H, W, _ = x_q.shape
    dev, Z = x_q.device, cv_out[1].Cin
    q_params = torch.empty((N, H, W, cv_q[1].Cout), dtype=torch.float32, device=dev)
    p_params = torch.empty_like(q_params) if cv_p is not None else p_given
    z, small, ks = _stoch_outputs(N, H, W, Z, dev, rows)
    out = torch.empty((N, H, W, cv_out[1].Cout), dtype=torch.float32, device=dev)
    if cv_p is not None:
        b.conv_p.y = ptr(p_params)
    b.conv_q.y, b.conv_out.x, b.conv_out.y = ptr(q_params), ptr(z), ptr(out)
    b.logprob_p, b.logprob_q, b.kl_samplewise, b.kl_spatial = ptr(small[0]), ptr(small[1]), ptr(small[2]), ptr(ks)
    call('lvae_stoch_block_fwd_f32', C.byref(b), stream_ptr())
    return out, z, p_params, q_params, small[0], small[1], small[2], ks


def stoch_block_bwd(d_out, cv_p, cv_q, cv_out, p, q, z, eps, dz, g_lp, g_lq, g_kl, g_ks, mode, analytical_kl):
    """Backward of stoch_block_fwd from d_out in one launch (lvae_stoch_block_bwd_f32): dgrad of conv_out, the core's backward, the dgrads of
    conv_in_q and conv_in_p (cv_p None: the block has none). p, q, z, eps: what the forward used and wrote; dz, g_*: upstream gradients, each
    may be None. Returns (dp, dq, d x_p | None, d x_q), or None where the launch does not take the call (the caller composes it)."""
    if _ddi is not None or any(t is None or t.dtype != torch.float32 or not t.is_contiguous() for t in (d_out, p, q, z)):
        return None
    N, H, W, _ = z.shape
    dev = z.device
    b = _C.StochBlockBwd()
    keep = []
    dq = torch.empty_like(q)
    dp = torch.empty_like(q)
    dxq = torch.empty((N, H, W, cv_q[1].Cin), dtype=torch.float32, device=dev)
    dxp = torch.empty((N, H, W, cv_p[1].Cin), dtype=torch.float32, device=dev) if cv_p is not None else None
    for name, cv, x, y in (('dgrad_out', cv_out, d_out, None), ('dgrad_q', cv_q, dq, dxq), ('dgrad_p', cv_p, dp, dxp)):
        d = ConvDesc()
        d.x, d.y = ptr(x), ptr(y)
        if cv is not None:
            w, g, _ = cv
            if g.transposed or tuple(x.shape) != (N, H, W, g.Cout):
                return None
            d.C1, d.Cout = g.Cout, g.Cin
            d.w, d.w_stap, d.w_sk, d.w_sn = ptr(w), g.s_tap, g.s_co, g.s_ci
            d.N, d.H, d.W, d.OH, d.OW = N, H, W, H, W
            d.KH, d.KW, d.stride, d.pad, d.gather, d.precision = g.KH, g.KW, g.stride, g.pad, GATHER_TRANSPOSED, precision
            need = _C.load().lvae_stoch_block_workspace(C.byref(d))
            if not need:
                return None
            prepared.attach(d, w, dev, need, 'lvae_stoch_block_prepare_entry')
            keep.append(d._ws_tensor)
        setattr(b, name, d)
    b.p, b.p_bcast, b.q, b.z, b.eps, b.dz = ptr(p), int(p.shape[0] == 1 and N > 1), ptr(q), ptr(z), ptr(eps), ptr(dz)
    b.g_lp, b.g_lq, b.g_kl, b.g_ks = ptr(g_lp), ptr(g_lq), ptr(g_kl), ptr(g_ks)
    b.mode, b.analytical_kl = mode, int(bool(analytical_kl))
    if not _C.load().lvae_stoch_block_bwd_ok(C.byref(b)):
        return None
    call('lvae_stoch_block_bwd_f32', C.byref(b), stream_ptr())
    del keep
    return dp, dq, dxp, dxq


def normal_prior_sample(p, eps, Z, N, temperature, row_temperature=None, rows=None):
    """Tempered draw from the prior p (N|1,H,W,2Z): z = mu + (t * sigma) * eps, z = mu exactly where t == 0; log p(z) under the untempered
    prior. temperature: the scalar t; row_temperature: a device float tensor (N,) that replaces it row by row. eps (N,H,W,Z) may be None
    only with a scalar temperature of 0. rows: as in normal_stochastic_fwd (only the logprob_p row is written). Returns (z, logprob_p)."""
    p_bcast = int(p.shape[0] == 1 and N > 1)
    _, H, W, _ = p.shape
    if row_temperature is not None and (row_temperature.dtype != torch.float32 or tuple(row_temperature.shape) != (N,)):
        raise ValueError("row_temperature must be a float32 tensor of shape (%d,), got %s %s"
                         % (N, row_temperature.dtype, tuple(row_temperature.shape)))
    z = torch.empty((N, H, W, Z), dtype=torch.float32, device=p.device)
    lp = rows[0] if rows is not None else torch.empty((N,), dtype=torch.float32, device=p.device)
    call('lvae_normal_prior_sample_f32', ptr(p), p_bcast, ptr(eps), float(temperature),
         ptr(None if row_temperature is None else row_temperature.contiguous()), N, H * W, Z, ptr(z), ptr(lp), stream_ptr())
    return z, lp


INTERP_MODES = {'lerp': 0, 'slerp': 1}


def latent_interp(za, zb, t, mode='slerp'):
    """The path between the rows of za and zb (B, ...), both contiguous float32 and of one shape, at the steps t, a device float32 tensor
    (T,) that is NOT validated: -> (T * B, ...), step-major (row j * B + b). mode 'lerp': (1 - t) a + t c; 'slerp': spherical, with the
    angle between the two rows as lvae_latent_interp_f32 forms it (a zero, parallel or antipodal pair falls back to lerp). t == 0 and
    t == 1 give the rows of za / zb bit for bit. ValueError for a shape mismatch or an unknown mode."""
    if mode not in INTERP_MODES:
        raise ValueError("mode must be 'slerp' or 'lerp', got %r" % (mode,))
    if tuple(za.shape) != tuple(zb.shape) or za.dim() < 1:
        raise ValueError("za and zb must have one shape (B, ...), got %s and %s" % (tuple(za.shape), tuple(zb.shape)))
    if t.dim() != 1:
        raise ValueError("t must have shape (T,), got %s" % (tuple(t.shape),))
    pa, pb, pt = ptr(za, (torch.float32,)), ptr(zb, (torch.float32,)), ptr(t, (torch.float32,))   # (CPU tensors are refused here)
    if not (za.is_contiguous() and zb.is_contiguous() and t.is_contiguous()):
        raise _C.LvaeHipError("latent_interp: za, zb and t must be contiguous, got strides %s, %s, %s" % (za.stride(), zb.stride(), t.stride()))
    B, T = int(za.shape[0]), int(t.shape[0])
    n = za.numel() // B if B > 0 else 0
    out = torch.empty((T * B,) + tuple(za.shape[1:]), dtype=torch.float32, device=za.device)
    ws = workspace(_C.load().lvae_latent_interp_workspace(B, T), za.device)
    call('lvae_latent_interp_f32', pa, pb, pt, B, n, T, INTERP_MODES[mode], ptr(out), ws.data_ptr(), ws.numel(), stream_ptr())
    return out


def normal_stochastic_bwd(p, q, eps, z, dz, g_lp, g_lq, g_kl, g_ks, mode, analytical_kl, Z):
    N, H, W, _ = z.shape
    p_bcast = int(p.shape[0] == 1 and N > 1)
    dp = torch.empty((N, H, W, 2 * Z), dtype=torch.float32, device=z.device)
    dq = torch.empty_like(dp) if q is not None else None
    call('lvae_normal_stochastic_bwd_f32', ptr(p), p_bcast, ptr(q), ptr(eps), ptr(z), ptr(dz), ptr(g_lp), ptr(g_lq),
         ptr(g_kl), ptr(g_ks), N, H * W, Z, mode, int(bool(analytical_kl)), ptr(dp), ptr(dq), stream_ptr())
    return dp, dq


def kl_elementwise_fwd(p, q, z, analytical_kl):
    """p, q (N|1,H,W,2Z), z (N,H,W,Z) -> (N,H,W,Z): log q(z) - log p(z), or KL(q||p) when analytical_kl."""
    N, H, W, Z = z.shape
    out = torch.empty_like(z)
    call('lvae_kl_elementwise_fwd_f32', ptr(p), int(p.shape[0] == 1 and N > 1), ptr(q), int(q.shape[0] == 1 and N > 1), ptr(z),
         N, H * W, Z, int(bool(analytical_kl)), ptr(out), stream_ptr())
    return out


def kl_elementwise_bwd(p, q, z, g, analytical_kl, need_dz=True):
    N, H, W, Z = z.shape
    dp = torch.empty((N, H, W, 2 * Z), dtype=torch.float32, device=z.device)
    dq = torch.empty_like(dp)
    dz = torch.empty_like(z) if need_dz else None
    call('lvae_kl_elementwise_bwd_f32', ptr(p), int(p.shape[0] == 1 and N > 1), ptr(q), int(q.shape[0] == 1 and N > 1), ptr(z),
         ptr(g), N, H * W, Z, int(bool(analytical_kl)), ptr(dp), ptr(dq), ptr(dz), stream_ptr())
    return dp, dq, dz


# ----------------------------------------------------------------------------------------------------------------
def bernoulli_fwd(logits, x, u, need_grad):
    """logits, x, u: (N,H,W,C) NHWC. Returns mean, mode, sample, ll (N,) | None, dll_dlogits | None."""
    N = logits.shape[0]
    P = logits.numel() // N
    mean, mode, sample = torch.empty_like(logits), torch.empty_like(logits), torch.empty_like(logits)
    ll = torch.empty((N,), dtype=torch.float32, device=logits.device) if x is not None else None
    dll = torch.empty_like(logits) if (need_grad and x is not None) else None
    call('lvae_bernoulli_fwd_f32', ptr(logits), ptr(x), ptr(u), N, P, ptr(mean), ptr(mode), ptr(sample), ptr(ll), ptr(dll),
         stream_ptr())
    return mean, mode, sample, ll, dll


def dmol_ll_fwd(l, x, need_grad):
    """l (N,H,W,100), x (N,H,W,3) in [0,1]. Returns ll (N,), dll_dl | None."""
    N, H, W, Cp = l.shape
    ll = torch.empty((N,), dtype=torch.float32, device=l.device)
    dl = torch.empty_like(l) if need_grad else None
    need = _C.load().lvae_dmol_workspace(N, H * W)
    ws = workspace(need, l.device)
    call('lvae_dmol_ll_fwd_f32', ptr(l), ptr(x), N, H * W, Cp // 10, ptr(ll), ptr(dl), ws.data_ptr(), ws.numel(), stream_ptr())
    return ll, dl


def dmol_sample(l, u_mix, u_log):
    N, H, W, Cp = l.shape
    s = torch.empty((N, H, W, 3), dtype=torch.float32, device=l.device)
    call('lvae_dmol_sample_f32', ptr(l), ptr(u_mix), ptr(u_log), N, H * W, Cp // 10, ptr(s), stream_ptr())
    return s


def gaussian_fwd(params, x, eps, need_grad):
    """params (N,H,W,2C); x, eps (N,H,W,C). Returns sample, ll | None, dll_dparams | None."""
    N, H, W, C2 = params.shape
    Cn = C2 // 2
    sample = torch.empty((N, H, W, Cn), dtype=torch.float32, device=params.device)
    ll = torch.empty((N,), dtype=torch.float32, device=params.device) if x is not None else None
    dll = torch.empty_like(params) if (need_grad and x is not None) else None
    call('lvae_gaussian_fwd_f32', ptr(params), ptr(x), ptr(eps), N, H * W, Cn, ptr(sample), ptr(ll), ptr(dll), stream_ptr())
    return sample, ll, dll


def discr_logistic_fwd(raw, x, u, need_grad):
    """raw (N,H,W,2C); x, u (N,H,W,C). Returns mean, logscale, sample, ll | None, dll_draw | None."""
    N, H, W, C2 = raw.shape
    Cn = C2 // 2
    mk = lambda: torch.empty((N, H, W, Cn), dtype=torch.float32, device=raw.device)
    mean, ls, sample = mk(), mk(), mk()
    ll = torch.empty((N,), dtype=torch.float32, device=raw.device) if x is not None else None
    dll = torch.empty_like(raw) if (need_grad and x is not None) else None
    call('lvae_discr_logistic_fwd_f32', ptr(raw), ptr(x), ptr(u), N, H * W, Cn, ptr(mean), ptr(ls), ptr(sample), ptr(ll), ptr(dll),
         stream_ptr())
    return mean, ls, sample, ll, dll


def pixel_mask(mask, N, H, W, device):
    """The (N,H,W) uint8 tensor the masked kernels read (non-zero = observed) from a bool or uint8 mask of shape (N,H,W) or (N,1,H,W) on
    `device`; no copy for a contiguous one (bool is reinterpreted). ValueError for another shape, dtype or device."""
    if not torch.is_tensor(mask) or mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError("mask must be a bool or uint8 tensor, got %s" % (mask.dtype if torch.is_tensor(mask) else type(mask).__name__))
    if tuple(mask.shape) not in ((N, H, W), (N, 1, H, W)):
        raise ValueError("mask must be (%d, %d, %d) or (%d, 1, %d, %d), got %s" % (N, H, W, N, H, W, tuple(mask.shape)))
    if mask.device != torch.device(device):
        raise ValueError("mask is on %s, the images on %s" % (mask.device, device))
    mask = mask.reshape(N, H, W).contiguous()
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def _filled_buf(filled, like):
    """The `filled` output of a masked head: a new tensor shaped like x, or the caller's (x itself: in-place completion)."""
    if filled is None:
        return torch.empty_like(like)
    if tuple(filled.shape) != tuple(like.shape) or not filled.is_contiguous():
        raise _C.LvaeHipError("filled must be contiguous and shaped like x %s, got %s" % (tuple(like.shape), tuple(filled.shape)))
    return filled


def _chk_masked(x, mask, N, H, W):
    if x is None:
        raise ValueError("a mask needs the image x it belongs to")
    if mask.dtype != torch.uint8 or tuple(mask.shape) != (N, H, W) or not mask.is_contiguous():
        raise ValueError("mask must be a contiguous uint8 (%d, %d, %d) tensor (kernels.pixel_mask makes one), got %s %s"
                         % (N, H, W, mask.dtype, tuple(mask.shape)))


def bernoulli_masked_fwd(logits, x, u, mask, need_grad, filled=None):
    """bernoulli_fwd on the observed pixels: mask (N,H,W) uint8, non-zero = observed. Returns mean, mode, sample, ll, dll | None, filled
    (x where observed, the sample where missing; `filled` may be x)."""
    N, H, W, Cn = logits.shape
    _chk_masked(x, mask, N, H, W)
    mean, mode, sample = torch.empty_like(logits), torch.empty_like(logits), torch.empty_like(logits)
    ll = torch.empty((N,), dtype=torch.float32, device=logits.device)
    dll = torch.empty_like(logits) if need_grad else None
    filled = _filled_buf(filled, x)
    call('lvae_bernoulli_masked_fwd_f32', ptr(logits), ptr(x), ptr(u), N, H * W * Cn, Cn, ptr(mean), ptr(mode), ptr(sample), ptr(ll),
         ptr(dll), ptr(mask), ptr(filled), stream_ptr())
    return mean, mode, sample, ll, dll, filled


def dmol_ll_masked_fwd(l, x, mask, sample, need_grad, filled=None):
    """dmol_ll_fwd on the observed pixels; sample: dmol_sample(l, ...) of the same parameters. Returns ll (N,), dll_dl | None, filled."""
    N, H, W, Cp = l.shape
    _chk_masked(x, mask, N, H, W)
    ll = torch.empty((N,), dtype=torch.float32, device=l.device)
    dl = torch.empty_like(l) if need_grad else None
    filled = _filled_buf(filled, x)
    ws = workspace(_C.load().lvae_dmol_workspace(N, H * W), l.device)
    call('lvae_dmol_ll_masked_fwd_f32', ptr(l), ptr(x), N, H * W, Cp // 10, ptr(ll), ptr(dl), ws.data_ptr(), ws.numel(), ptr(mask),
         ptr(sample), ptr(filled), stream_ptr())
    return ll, dl, filled


def gaussian_masked_fwd(params, x, eps, mask, need_grad, filled=None):
    """gaussian_fwd on the observed pixels. Returns sample, ll, dll_dparams | None, filled."""
    N, H, W, C2 = params.shape
    Cn = C2 // 2
    _chk_masked(x, mask, N, H, W)
    sample = torch.empty((N, H, W, Cn), dtype=torch.float32, device=params.device)
    ll = torch.empty((N,), dtype=torch.float32, device=params.device)
    dll = torch.empty_like(params) if need_grad else None
    filled = _filled_buf(filled, x)
    call('lvae_gaussian_masked_fwd_f32', ptr(params), ptr(x), ptr(eps), N, H * W, Cn, ptr(sample), ptr(ll), ptr(dll), ptr(mask),
         ptr(filled), stream_ptr())
    return sample, ll, dll, filled


def discr_logistic_masked_fwd(raw, x, u, mask, need_grad, filled=None):
    """discr_logistic_fwd on the observed pixels. Returns mean, logscale, sample, ll, dll_draw | None, filled."""
    N, H, W, C2 = raw.shape
    Cn = C2 // 2
    _chk_masked(x, mask, N, H, W)
    mk = lambda: torch.empty((N, H, W, Cn), dtype=torch.float32, device=raw.device)
    mean, ls, sample = mk(), mk(), mk()
    ll = torch.empty((N,), dtype=torch.float32, device=raw.device)
    dll = torch.empty_like(raw) if need_grad else None
    filled = _filled_buf(filled, x)
    call('lvae_discr_logistic_masked_fwd_f32', ptr(raw), ptr(x), ptr(u), N, H * W, Cn, ptr(mean), ptr(ls), ptr(sample), ptr(ll), ptr(dll),
         ptr(mask), ptr(filled), stream_ptr())
    return mean, ls, sample, ll, dll, filled


def mask_select(a, b, mask, nchw, out=None):
    """out = mask ? a : b, exactly. a: contiguous float32 (N,C,H,W) when nchw else (N,H,W,C); b: a tensor of a's shape or a number (that
    value everywhere); mask (N,H,W) uint8, non-zero = take a. out: None (a new tensor), or a or b themselves (in place)."""
    if nchw:
        N, Cn, H, W = a.shape
    else:
        N, H, W, Cn = a.shape
    if mask.dtype != torch.uint8 or tuple(mask.shape) != (N, H, W) or not mask.is_contiguous():
        raise ValueError("mask must be a contiguous uint8 (%d, %d, %d) tensor, got %s %s" % (N, H, W, mask.dtype, tuple(mask.shape)))
    tensor_b = torch.is_tensor(b)
    if tensor_b and tuple(b.shape) != tuple(a.shape):
        raise ValueError("a and b must have one shape, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    if not a.is_contiguous() or (tensor_b and not b.is_contiguous()):
        raise _C.LvaeHipError("mask_select: a and b must be contiguous")
    if out is None:
        out = torch.empty_like(a)
    elif tuple(out.shape) != tuple(a.shape) or not out.is_contiguous():
        raise _C.LvaeHipError("mask_select: out must be contiguous and shaped like a")
    call('lvae_mask_select_f32', ptr(a, (torch.float32,)), ptr(b, (torch.float32,)) if tensor_b else None, 0.0 if tensor_b else float(b),
         ptr(mask, (torch.uint8,)), N, Cn, H * W, int(bool(nchw)), ptr(out, (torch.float32,)), stream_ptr())
    return out


def scale_per_sample(a, g):
    N = a.shape[0]
    out = torch.empty_like(a)
    call('lvae_scale_per_sample_f32', ptr(a), ptr(g), N, a.numel() // N, ptr(out), stream_ptr())
    return out


# ----------------------------------------------------------------------------------------------------------------
def upsample2x_fwd(x):
    N, H, W, Cn = x.shape
    y = torch.empty((N, 2 * H, 2 * W, Cn), dtype=torch.float32, device=x.device)
    call('lvae_upsample2x_fwd_f32', ptr(x), N, H, W, Cn, ptr(y), stream_ptr())
    return y


def upsample2x_bwd(dy):
    N, H2, W2, Cn = dy.shape
    dx = torch.empty((N, H2 // 2, W2 // 2, Cn), dtype=torch.float32, device=dy.device)
    call('lvae_upsample2x_bwd_f32', ptr(dy), N, H2 // 2, W2 // 2, Cn, ptr(dx), stream_ptr())
    return dx


def pad_crop(x, src_nchw, out_hw, dst_nchw):
    """Centred zero-pad or centre-crop + layout change. x is (N,C,H,W) contiguous when src_nchw else (N,H,W,C)."""
    if src_nchw:
        N, Cn, H, W = x.shape
    else:
        N, H, W, Cn = x.shape
    OH, OW = int(out_hw[0]), int(out_hw[1])
    shape = (N, Cn, OH, OW) if dst_nchw else (N, OH, OW, Cn)
    y = torch.empty(shape, dtype=torch.float32, device=x.device)
    call('lvae_pad_crop_f32', ptr(x), N, Cn, H, W, int(src_nchw), ptr(y), OH, OW, int(dst_nchw), stream_ptr())
    return y


# ----------------------------------------------------------------------------------------------------------------
def kl_bookkeeping_fwd(kl_ln, free_bits):
    L, N = kl_ln.shape
    dev = kl_ln.device
    kl_sep = torch.empty((N,), dtype=torch.float32, device=dev)
    kl_avg = torch.empty((L,), dtype=torch.float32, device=dev)
    scal = torch.empty((2,), dtype=torch.float32, device=dev)
    call('lvae_kl_bookkeeping_fwd_f32', ptr(kl_ln), L, N, float(free_bits), ptr(kl_sep), ptr(kl_avg), ptr(scal), stream_ptr())
    return kl_sep, kl_avg, scal


def kl_bookkeeping_bwd(kl_ln, free_bits, g_sep, g_avg, g_scal):
    L, N = kl_ln.shape
    dkl = torch.empty_like(kl_ln)
    call('lvae_kl_bookkeeping_bwd_f32', ptr(kl_ln), L, N, float(free_bits), ptr(g_sep), ptr(g_avg), ptr(g_scal), ptr(dkl),
         stream_ptr())
    return dkl


def kl_balance_fwd(kl_ln, free_bits, alpha, beta=1.0, step=None, anneal_steps=0, coeff=None):
    """kl_bookkeeping_fwd with the KL terms balanced over the layers while beta < 1 (csrc/kl_balance.hip). alpha: device float[L], positive
    and finite (balance.KlBalance validates it on the host). beta: a float, or with step (device int64[1]) linear_anneal(step[0], 0, 1,
    anneal_steps) read on the device. coeff: device float[L] to write the coefficients to (allocated when None).
    -> kl_sep, kl_avg_layerwise, scalars [kl_loss (balanced), kl], coeff."""
    L, N = kl_ln.shape
    dev = kl_ln.device
    if alpha.numel() != L:
        raise ValueError("kl_balance_fwd: %d weights for %d layers" % (alpha.numel(), L))
    if coeff is None:
        coeff = torch.empty((L,), dtype=torch.float32, device=dev)
    elif coeff.numel() != L or not coeff.is_contiguous():
        raise ValueError("kl_balance_fwd: coeff must be a contiguous float[%d]" % L)
    kl_sep = torch.empty((N,), dtype=torch.float32, device=dev)
    kl_avg = torch.empty((L,), dtype=torch.float32, device=dev)
    scal = torch.empty((2,), dtype=torch.float32, device=dev)
    call('lvae_kl_balance_fwd_f32', ptr(kl_ln), L, N, float(free_bits), ptr(alpha, (torch.float32,)), float(beta),
         None if step is None else ptr(step, (torch.int64,)), int(anneal_steps), ptr(kl_sep), ptr(kl_avg), ptr(scal),
         ptr(coeff, (torch.float32,)), stream_ptr())
    return kl_sep, kl_avg, scal, coeff


def kl_balance_bwd(kl_ln, free_bits, coeff, g_sep, g_avg, g_scal):
    """kl_bookkeeping_bwd with the forward's coefficients on the kl_loss term (read from coeff, never formed again)."""
    L, N = kl_ln.shape
    if coeff.numel() != L:
        raise ValueError("kl_balance_bwd: %d coefficients for %d layers" % (coeff.numel(), L))
    dkl = torch.empty_like(kl_ln)
    call('lvae_kl_balance_bwd_f32', ptr(kl_ln), L, N, float(free_bits), ptr(coeff, (torch.float32,)), ptr(g_sep), ptr(g_avg), ptr(g_scal),
         ptr(dkl), stream_ptr())
    return dkl


def elbo_loss_fwd(ll, kl_sep, kl_loss, beta):
    N = ll.numel()
    elbo_sep = torch.empty((N,), dtype=torch.float32, device=ll.device)
    scal = torch.empty((3,), dtype=torch.float32, device=ll.device)
    call('lvae_elbo_loss_fwd_f32', ptr(ll), ptr(kl_sep), ptr(kl_loss), float(beta), N, ptr(elbo_sep), ptr(scal), stream_ptr())
    return elbo_sep, scal


def elbo_loss_bwd(g_loss, beta, N):
    d_ll = torch.empty((N,), dtype=torch.float32, device=g_loss.device)
    d_kl = torch.empty((1,), dtype=torch.float32, device=g_loss.device)
    call('lvae_elbo_loss_bwd_f32', ptr(g_loss), float(beta), N, ptr(d_ll), ptr(d_kl), stream_ptr())
    return d_ll, d_kl


def elbo_loss_fwd_anneal(ll, kl_sep, kl_loss, step, anneal_steps):
    """elbo_loss_fwd with beta = linear_anneal(step[0], 0, 1, anneal_steps) read on the device (step: device int64[1])."""
    N = ll.numel()
    elbo_sep = torch.empty((N,), dtype=torch.float32, device=ll.device)
    scal = torch.empty((3,), dtype=torch.float32, device=ll.device)
    call('lvae_elbo_loss_fwd_anneal_f32', ptr(ll), ptr(kl_sep), ptr(kl_loss), ptr(step, (torch.int64,)), int(anneal_steps), N,
         ptr(elbo_sep), ptr(scal), stream_ptr())
    return elbo_sep, scal


def elbo_loss_bwd_anneal(g_loss, step, anneal_steps, N):
    d_ll = torch.empty((N,), dtype=torch.float32, device=g_loss.device)
    d_kl = torch.empty((1,), dtype=torch.float32, device=g_loss.device)
    call('lvae_elbo_loss_bwd_anneal_f32', ptr(g_loss), ptr(step, (torch.int64,)), int(anneal_steps), N, ptr(d_ll), ptr(d_kl),
         stream_ptr())
    return d_ll, d_kl


def _iw_out(ll, K_):
    N = ll.numel()
    if K_ < 1 or N % K_:
        raise _C.LvaeHipError("importance-weighted loss: %d rows are not %d samples of a whole number of images" % (N, K_))
    new = lambda n: torch.empty((n,), dtype=torch.float32, device=ll.device)
    return N // K_, new(N), new(N), new(N // K_), new(5)


def iw_loss_fwd(ll, kl_sep, beta, K_):
    """ll, kl_sep (K*B,) sample-major. Returns elbo_sep (K*B,), w (K*B,), bound (B,), scalars [loss, elbo, recons, iw, ess]."""
    B, elbo_sep, w, bound, scal = _iw_out(ll, K_)
    call('lvae_iw_loss_fwd_f32', ptr(ll), ptr(kl_sep), float(beta), K_, B, ptr(elbo_sep), ptr(w), ptr(bound), ptr(scal), stream_ptr())
    return elbo_sep, w, bound, scal


def iw_loss_bwd(g_loss, w, beta, K_):
    d_ll, d_kl = torch.empty_like(w), torch.empty_like(w)
    call('lvae_iw_loss_bwd_f32', ptr(g_loss), ptr(w), float(beta), K_, w.numel() // K_, ptr(d_ll), ptr(d_kl), stream_ptr())
    return d_ll, d_kl


def iw_loss_fwd_anneal(ll, kl_sep, step, anneal_steps, K_):
    """iw_loss_fwd with beta = linear_anneal(step[0], 0, 1, anneal_steps) read on the device (step: device int64[1])."""
    B, elbo_sep, w, bound, scal = _iw_out(ll, K_)
    call('lvae_iw_loss_fwd_anneal_f32', ptr(ll), ptr(kl_sep), ptr(step, (torch.int64,)), int(anneal_steps), K_, B, ptr(elbo_sep), ptr(w),
         ptr(bound), ptr(scal), stream_ptr())
    return elbo_sep, w, bound, scal


def iw_loss_bwd_anneal(g_loss, w, step, anneal_steps, K_):
    d_ll, d_kl = torch.empty_like(w), torch.empty_like(w)
    call('lvae_iw_loss_bwd_anneal_f32', ptr(g_loss), ptr(w), ptr(step, (torch.int64,)), int(anneal_steps), K_, w.numel() // K_, ptr(d_ll),
         ptr(d_kl), stream_ptr())
    return d_ll, d_kl


def repeat_samples(x, K_):
    """(B, ...) contiguous -> (K*B, ...): K copies of x, sample-major."""
    out = torch.empty((K_ * x.shape[0],) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    call('lvae_repeat_samples_fwd_f32', ptr(x, (torch.float32,)), x.numel(), K_, ptr(out), stream_ptr())
    return out


def repeat_samples_bwd(dout, K_):
    """(K*B, ...) contiguous -> (B, ...): the float32 sum over the K samples in ascending k."""
    din = torch.empty((dout.shape[0] // K_,) + tuple(dout.shape[1:]), dtype=torch.float32, device=dout.device)
    call('lvae_repeat_samples_bwd_f32', ptr(dout, (torch.float32,)), din.numel(), K_, ptr(din), stream_ptr())
    return din


# ----------------------------------------------------------------------------------------------------------------
def iw_logmeanexp(elbo_sn):
    S, N = elbo_sn.shape
    out = torch.empty((N,), dtype=torch.float32, device=elbo_sn.device)
    call('lvae_iw_logmeanexp_f32', ptr(elbo_sn), S, N, ptr(out), stream_ptr())
    return out


def iw_online(state, mode, elbo=None, S=0, iw=None, mean=None):
    """state (3, N). mode 0 init / 1 accumulate elbo (N,) / 2 finalize into iw, mean (N,)."""
    call('lvae_iw_online_f32', ptr(elbo), ptr(state), state.shape[1], int(mode), int(S), ptr(iw), ptr(mean), stream_ptr())


def eval_online(state, L, mode, elbo=None, ll=None, kl_sep=None, kl_avg=None):
    """state: float64 (5 * N + L). mode 0 initialise / 1 fold in one sample's elbo_sep, ll, kl_sep (N,) and kl_avg_layerwise (L,)."""
    N = (state.numel() - L) // 5
    call('lvae_eval_online_f32', ptr(elbo), ptr(ll), ptr(kl_sep), ptr(kl_avg), ptr(state, (torch.float64,)), N, int(L), int(mode),
         stream_ptr())


def eval_totals(state, L, S, totals):
    """totals: float64 (5 + L) += this batch's [sum IW, sum ELBO, sum recons, sum KL, images, per-layer KL sums]."""
    N = (state.numel() - L) // 5
    call('lvae_eval_totals_f64', ptr(state, (torch.float64,)), N, int(L), int(S), ptr(totals, (torch.float64,)), stream_ptr())


def latent_stats_fold(p, q, sums, N=None):
    """sums: float64 (3, U) view += this batch's [sum mu_q, sum mu_q^2, sum KL(q || p)] per latent unit, U = H * W * Z in NHWC order.
    p (N|1,H,W,2Z), q (N,H,W,2Z): the fp32 (mu | logvar) tensors normal_stochastic_fwd reads. Two launches, no allocation once the scratch
    buffer of the stream is large enough."""
    if N is None:
        N = q.shape[0]
    _, H, W, Z2 = q.shape
    if not (p.dtype == q.dtype == torch.float32 and q.is_contiguous() and tuple(p.shape[1:]) == (H, W, Z2) and Z2 % 2 == 0):
        raise _C.LvaeHipError("latent_stats_fold: p %s / q %s are not fp32 (mu | logvar) tensors of one layer" % (tuple(p.shape), tuple(q.shape)))
    if sums.numel() != 3 * H * W * (Z2 // 2) or not sums.is_contiguous():
        raise _C.LvaeHipError("latent_stats_fold: sums has %d entries, this layer 3 x %d units" % (sums.numel(), H * W * (Z2 // 2)))
    need = _C.load().lvae_latent_stats_workspace(int(N), H * W, Z2 // 2)
    ws = workspace(need, q.device)
    call('lvae_latent_stats_fold_f32', ptr(p), int(p.shape[0] == 1 and N > 1), ptr(q), int(N), H * W, Z2 // 2, ptr(sums, (torch.float64,)),
         ws.data_ptr(), ws.numel(), stream_ptr())


def latent_stats_finalize(sums, n_images, kl_threshold, var_threshold, unit_out, layer_out):
    """sums float64 (3, U) -> unit_out float64 (3, U) = per-unit mean KL, mean and population variance of mu_q; layer_out float64 (4,) =
    [units with KL > kl_threshold, units with variance > var_threshold, U, sum of the per-unit KLs]. One launch of one workgroup."""
    U = sums.numel() // 3
    if unit_out.numel() != 3 * U or layer_out.numel() != 4:
        raise _C.LvaeHipError("latent_stats_finalize: outputs of %d and %d entries for %d units" % (unit_out.numel(), layer_out.numel(), U))
    f64 = (torch.float64,)
    call('lvae_latent_stats_finalize_f64', ptr(sums, f64), U, int(n_images), float(kl_threshold), float(var_threshold), ptr(unit_out, f64),
         ptr(layer_out, f64), stream_ptr())


IQ_WINDOW = 11   # edge of the SSIM window: the smallest image lvae_image_quality_f32 takes


def _iq_src(t, name, channel_last):
    """(nhwc flag, pixel stride, (N, C, H, W)) of an image set for lvae_image_quality_f32: (N, C, H, W) by shape, or (N, H, W, C) with
    channel_last; stored NCHW contiguous, or channel-last with a pixel stride of ld >= C floats (an NHWC buffer, its NCHW view, or the
    first C channels of a wider NHWC buffer). No copy: another storage is an error."""
    if not torch.is_tensor(t) or t.dim() != 4:
        raise ValueError("%s: need a 4-d image tensor, got %s" % (name, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
    v = t.permute(0, 3, 1, 2) if channel_last else t
    N, Cn, H, W = (int(s) for s in v.shape)
    sn, sc, sh, sw = (int(s) for s in v.stride())
    if (Cn == 1 or sc == H * W) and sh == W and sw == 1 and (N == 1 or sn == Cn * H * W):
        return 0, 0, (N, Cn, H, W)
    if (Cn == 1 or sc == 1) and sw >= Cn and sh == W * sw and (N == 1 or sn == H * W * sw):
        return 1, sw, (N, Cn, H, W)
    raise _C.LvaeHipError("%s: neither NCHW contiguous nor channel-last with one pixel stride (shape %s, strides %s)"
                          % (name, tuple(t.shape), tuple(t.stride())))


def image_quality(a, b, mask=None, count_where=1, data_range=1.0, clamp=True, channel_last=False, out=None):
    """float32 (N, 3) on the device: per image the mse, the PSNR in dB and the SSIM of b judged against a (lvae_image_quality_f32 states
    the formulas). a, b: float32 image sets of one shape, each in a storage _iq_src takes (they may differ in it). mask: None, or the
    (N, H, W) uint8 tensor pixel_mask makes; a pixel is counted when (mask != 0) == (count_where != 0). Two launches, no allocation once
    `out` is given and the scratch buffer of the stream is large enough."""
    if not (torch.is_tensor(a) and torch.is_tensor(b)) or tuple(a.shape) != tuple(b.shape):
        raise ValueError("image_quality: the two image sets differ in shape: %s and %s" % (tuple(getattr(a, 'shape', ())), tuple(getattr(b, 'shape', ()))))
    a_nhwc, a_ld, (N, Cn, H, W) = _iq_src(a, 'a', channel_last)
    b_nhwc, b_ld, _ = _iq_src(b, 'b', channel_last)
    if H < IQ_WINDOW or W < IQ_WINDOW:
        raise ValueError("image_quality: images of %d x %d are smaller than the %d x %d window" % (H, W, IQ_WINDOW, IQ_WINDOW))
    f32 = (torch.float32,)
    pa, pb = ptr(a, f32), ptr(b, f32)
    if mask is not None:
        _chk_masked(a, mask, N, H, W)
    if out is None:
        out = torch.empty((N, 3), dtype=torch.float32, device=a.device)
    elif tuple(out.shape) != (N, 3) or not out.is_contiguous():
        raise _C.LvaeHipError("image_quality: out must be a contiguous (%d, 3) tensor, got %s" % (N, tuple(out.shape)))
    ws = workspace(_C.load().lvae_image_quality_workspace(N, Cn, H, W), a.device)
    call('lvae_image_quality_f32', pa, a_nhwc, a_ld, pb, b_nhwc, b_ld, ptr(mask, (torch.uint8,)), int(bool(count_where)), N, Cn, H, W,
         float(data_range), int(bool(clamp)), ptr(out, f32), ws.data_ptr(), ws.numel(), stream_ptr())
    return out


IQ_SUMS = 5   # lvae_image_quality_fold_f64's sums: images, sum mse, sum of the PSNRs that are not +inf, images with mse == 0, sum ssim


def image_quality_fold(per_image, sums):
    """sums: float64 (5,) += the (N, 3) rows of image_quality, in image order. One launch of one workgroup; captured passes replay it."""
    if per_image.dim() != 2 or per_image.shape[1] != 3 or not per_image.is_contiguous() or sums.numel() != IQ_SUMS or not sums.is_contiguous():
        raise _C.LvaeHipError("image_quality_fold: rows %s into sums of %d entries" % (tuple(per_image.shape), sums.numel()))
    call('lvae_image_quality_fold_f64', ptr(per_image, (torch.float32,)), int(per_image.shape[0]), ptr(sums, (torch.float64,)), stream_ptr())


SUMMARY_FIXED, SUMMARY_MAX_LAYERS = 8, 64   # slots of lvae_summary_fold_f64's accumulator before the per-layer KLs; the most layers it takes


def summary_fold(loss, elbo, recons, kl, l2, kl_layers, acc, grad_norm=None, gscale=None):
    """acc: float64 (8 + L) += one training step's fp32 scalars (device tensors of one element; kl_layers (L,)), laid out as
    [steps, non-finite steps, loss, elbo, recons, kl, l2, grad, kl_layer_0 ...]. grad = grad_norm * gscale (fp32), grad_norm alone, or 0.
    A step whose loss or grad is not finite only counts in slot 1. One launch of one wave; captured steps replay it."""
    L = acc.numel() - SUMMARY_FIXED
    n_kl = 0 if kl_layers is None else kl_layers.numel()
    if acc.dim() != 1 or n_kl != L or (n_kl and not kl_layers.is_contiguous()):
        raise _C.LvaeHipError("summary_fold: the accumulator has %d slots, which is not 8 + %d contiguous per-layer KLs" % (acc.numel(), n_kl))
    f32 = (torch.float32,)
    call('lvae_summary_fold_f64', ptr(loss, f32), ptr(elbo, f32), ptr(recons, f32), ptr(kl, f32), ptr(l2, f32), ptr(grad_norm, f32),
         ptr(gscale, f32), ptr(kl_layers, f32) if n_kl else None, L, ptr(acc, (torch.float64,)), stream_ptr())


def summary_take(acc, out):
    """out <- acc, acc <- 0 (two float64 vectors of one length): one launch, stream-ordered between two steps."""
    if acc.numel() != out.numel():
        raise _C.LvaeHipError("summary_take: %d slots into a buffer of %d" % (acc.numel(), out.numel()))
    call('lvae_summary_take_f64', ptr(acc, (torch.float64,)), acc.numel(), ptr(out, (torch.float64,)), stream_ptr())
    return out


MICRO_FIXED = 7   # slots of lvae_micro_fold_f64's accumulator before the per-layer KLs: loss, elbo, recons, kl, l2, iw, ess


def micro_fold(loss, elbo, recons, kl, l2, kl_layers, m, acc, count, out, iw=None, ess=None):
    """One micro-pass of a step accumulated over `m`: acc float64 (7 + L) += the pass's fp32 scalars (device tensors of one element;
    kl_layers (L,); iw / ess or None), count int64 (1,) += 1. The m-th call writes the means (float)(acc / m) into out float32 (7 + L) and
    clears acc and count; out is untouched before it. One launch of one wave; captured micro-passes replay it."""
    L = acc.numel() - MICRO_FIXED
    n_kl = 0 if kl_layers is None else kl_layers.numel()
    if acc.dim() != 1 or n_kl != L or (n_kl and not kl_layers.is_contiguous()):
        raise _C.LvaeHipError("micro_fold: the accumulator has %d slots, which is not 7 + %d contiguous per-layer KLs" % (acc.numel(), n_kl))
    if out.numel() != acc.numel() or not out.is_contiguous() or not acc.is_contiguous() or count.numel() != 1:
        raise _C.LvaeHipError("micro_fold: %d means into an output of %d, or a counter of %d elements" % (acc.numel(), out.numel(), count.numel()))
    f32 = (torch.float32,)
    call('lvae_micro_fold_f64', ptr(loss, f32), ptr(elbo, f32), ptr(recons, f32), ptr(kl, f32), ptr(l2, f32), ptr(iw, f32), ptr(ess, f32),
         ptr(kl_layers, f32) if n_kl else None, L, int(m), ptr(acc, (torch.float64,)), ptr(count, (torch.int64,)), ptr(out, f32),
         stream_ptr())
    return out


def _img_src(t, name):
    """(tensor, nhwc flag, (n, C, H, W)) of an image set given in the NCHW convention: NCHW contiguous, or the NCHW view of an NHWC
    contiguous buffer (what the model returns). No copy, no layout change."""
    if t.dim() != 4 or t.dtype != torch.float32:
        raise _C.LvaeHipError("%s: need a float32 (N, C, H, W) tensor, got %s %s" % (name, t.dtype, tuple(t.shape)))
    if t.is_contiguous():
        return t, 0, tuple(t.shape)
    if t.permute(0, 2, 3, 1).is_contiguous():
        return t, 1, tuple(t.shape)
    raise _C.LvaeHipError("%s: neither NCHW nor NHWC contiguous (strides %s)" % (name, t.stride()))


def _img_pair(a, b):
    a, a_nhwc, (n, Cn, H, W) = _img_src(a, 'images')
    b_nhwc = 0
    if b is not None:
        b, b_nhwc, shape_b = _img_src(b, 'second')
        if shape_b != (n, Cn, H, W):
            raise _C.LvaeHipError("the two image sets differ in shape: %s and %s" % ((n, Cn, H, W), shape_b))
        n *= 2
    return a, a_nhwc, b, b_nhwc, n, Cn, H, W


def image_border_count(a, b=None, threshold=0.2):
    """int32 [2] on the device: how many border values of the images (of both sets) are below `threshold`, and how many are NaN."""
    a, a_nhwc, b, b_nhwc, n, Cn, H, W = _img_pair(a, b)
    count = torch.empty((2,), dtype=torch.int32, device=a.device)
    call('lvae_image_border_count_f32', ptr(a), a_nhwc, ptr(b), b_nhwc, n, Cn, H, W, float(threshold), ptr(count, (torch.int32,)),
         stream_ptr())
    return count


def image_grid_shape(n, nrow, H, W):
    """(Hg, Wg) of make_grid(padding=2) for n images of H x W, nrow per row (a single image is padded like any other)."""
    xmaps = min(int(nrow), n)
    ymaps = -(-n // xmaps)
    return (H + 2) * ymaps + 2, (W + 2) * xmaps + 2


def image_grid(a, nrow, b=None, border_count=None, pad_value=0.0):
    """uint8 (Hg, Wg, 3) grid of the images a (with b: a[0], b[0], a[1], b[1], ...), nrow per row. The padding value is decided on the
    device from `border_count` (image_border_count) when given, else it is `pad_value`."""
    a, a_nhwc, b, b_nhwc, n, Cn, H, W = _img_pair(a, b)
    if n < 1 or int(nrow) < 1:
        raise _C.LvaeHipError("image_grid needs at least one image and nrow >= 1")
    Hg, Wg = image_grid_shape(n, nrow, H, W)
    grid = torch.empty((Hg, Wg, 3), dtype=torch.uint8, device=a.device)
    call('lvae_image_grid_u8', ptr(a), a_nhwc, ptr(b), b_nhwc, n, Cn, H, W, int(nrow), ptr(border_count, (torch.int32,)),
         float(pad_value), ptr(grid, (torch.uint8,)), grid.numel(), stream_ptr())
    return grid


def adamax_step(p, g, exp_avg, exp_inf, mask, lr, beta1, beta2, eps, weight_decay, gscale, step_count):
    call('lvae_adamax_step_f32', ptr(p), ptr(g), ptr(exp_avg), ptr(exp_inf), ptr(mask), p.numel(), lr, beta1, beta2, eps,
         weight_decay, ptr(gscale), step_count.data_ptr(), stream_ptr())
    prepared.weights_written()


def adamax_ema_step(p, g, exp_avg, exp_inf, mask, lr, beta1, beta2, eps, weight_decay, gscale, step_count, ema, decay):
    """adamax_step plus, in the same pass, ema += (p_new - ema) * (1 - min(decay, (1 + n) / (10 + n))), n = step_count[0] on the device."""
    if ema.numel() != p.numel():
        raise _C.LvaeHipError("ema has %d elements, the parameters %d" % (ema.numel(), p.numel()))
    call('lvae_adamax_ema_step_f32', ptr(p), ptr(g), ptr(exp_avg), ptr(exp_inf), ptr(mask), p.numel(), lr, beta1, beta2, eps,
         weight_decay, ptr(gscale), step_count.data_ptr(), ptr(ema), float(decay), stream_ptr())
    prepared.weights_written()


def lr_schedule_struct(base_lr, kind, warmup_steps, decay_steps, min_lr, gamma):
    """struct lvae_lr_schedule of the arguments (`kind` by name: _C.LR_KINDS)."""
    if kind not in _C.LR_KINDS:
        raise ValueError("unknown lr schedule %r (one of %s)" % (kind, ', '.join(_C.LR_KINDS)))
    return _C.LrScheduleStruct(float(base_lr), float(min_lr), float(gamma), _C.LR_KINDS[kind], int(warmup_steps), int(decay_steps))


def lr_schedule_at(schedule, n):
    """The lr a _C.LrScheduleStruct gives at n completed steps: the host twin of what the scheduled Adamax kernel computes. Needs no GPU."""
    lr = C.c_float()
    call('lvae_lr_schedule_at', C.byref(schedule), int(n), C.byref(lr))
    return lr.value


def adamax_sched_step(p, g, exp_avg, exp_inf, mask, schedule, beta1, beta2, eps, weight_decay, gscale, step_count, ema=None, decay=0.0,
                      lr_out=None):
    """adamax_step / adamax_ema_step (`ema` None or a buffer) with lr = schedule(step_count[0]) evaluated inside the kernel; `lr_out`
    (device float[1], optional) receives the lr applied."""
    if ema is not None and ema.numel() != p.numel():
        raise _C.LvaeHipError("ema has %d elements, the parameters %d" % (ema.numel(), p.numel()))
    call('lvae_adamax_sched_step_f32', ptr(p), ptr(g), ptr(exp_avg), ptr(exp_inf), ptr(mask), p.numel(), C.byref(schedule), beta1,
         beta2, eps, weight_decay, ptr(gscale), step_count.data_ptr(), ptr(ema), float(decay), ptr(lr_out, (torch.float32,)), stream_ptr())
    prepared.weights_written()


def grad_guard(g, gscale, max_norm, skip_threshold, state):
    """The gradient guard's decision for the arena `g` into `state` (device int64[4] laid out as struct lvae_grad_guard_state: norm, scale,
    skip flag, cumulative clipped / skipped counts). max_norm <= 0: no clipping; skip_threshold < 0: only non-finite steps are skipped.
    Two launches (the partial sums of l2norm, then the decision)."""
    if state.dtype != torch.int64 or state.numel() * 8 != C.sizeof(_C.GradGuardState) or not state.is_contiguous():
        raise _C.LvaeHipError("grad_guard: the state is a contiguous device int64[%d]" % (C.sizeof(_C.GradGuardState) // 8))
    ws = workspace(_C.load().lvae_sumsq_workspace(g.numel()), g.device)
    call('lvae_grad_guard_f32', ptr(g, (torch.float32,)), g.numel(), ptr(gscale, (torch.float32,)), float(max_norm), float(skip_threshold),
         ptr(state, (torch.int64,)), ws.data_ptr(), ws.numel(), stream_ptr())


def adamax_guarded_step(p, g, exp_avg, exp_inf, mask, lr, schedule, beta1, beta2, eps, weight_decay, step_count, ema, decay, lr_out, state):
    """The Adamax step of a guarded training step: nothing at all when state's skip flag is set, else adamax_step / adamax_ema_step /
    adamax_sched_step (`schedule` None or a struct, `ema` None or a buffer) with the guard's scale in the place of gscale."""
    if ema is not None and ema.numel() != p.numel():
        raise _C.LvaeHipError("ema has %d elements, the parameters %d" % (ema.numel(), p.numel()))
    call('lvae_adamax_guarded_step_f32', ptr(p), ptr(g), ptr(exp_avg), ptr(exp_inf), ptr(mask), p.numel(), float(lr),
         None if schedule is None else C.byref(schedule), beta1, beta2, eps, weight_decay, step_count.data_ptr(), ptr(ema), float(decay),
         ptr(lr_out, (torch.float32,)), ptr(state, (torch.int64,)), stream_ptr())
    prepared.weights_written()


def adam_step(p, g, exp_avg, exp_avg_sq, mask, lr, schedule, beta1, beta2, eps, weight_decay, decoupled, gscale, step_count, ema=None,
              decay=0.0, lr_out=None, state=None):
    """One torch.optim.Adam (`decoupled` False: L2 decay) or AdamW (True: decoupled decay) step over the arena, every option in one entry
    point: `schedule` None or a struct, `ema` None or a buffer, `state` None or a guard's state (then without `gscale`: the guard's scale
    stands in its place, and a skipped step stores nothing), `lr_out` (device float[1], optional) receives the lr applied. The betas go
    down as doubles: the kernel forms the bias corrections in double from the device step counter."""
    if ema is not None and ema.numel() != p.numel():
        raise _C.LvaeHipError("ema has %d elements, the parameters %d" % (ema.numel(), p.numel()))
    call('lvae_adam_step_f32', ptr(p), ptr(g), ptr(exp_avg), ptr(exp_avg_sq), ptr(mask), p.numel(), float(lr),
         None if schedule is None else C.byref(schedule), float(beta1), float(beta2), float(eps), float(weight_decay), int(bool(decoupled)),
         ptr(gscale, (torch.float32,)), step_count.data_ptr(), ptr(ema), float(decay), ptr(lr_out, (torch.float32,)),
         ptr(state, (torch.int64,)), stream_ptr())
    prepared.weights_written()


def copy_table(pairs, device):
    """[(dst, src)] pairs of contiguous fp32 device tensors of equal length -> the device table multi_copy takes (int64 [len][3]: struct
    lvae_copy_entry). The caller keeps the tensors alive and in place for as long as the table is used."""
    rows = []
    for dst, src in pairs:
        if dst.numel() != src.numel() or not (dst.is_contiguous() and src.is_contiguous()):
            raise _C.LvaeHipError("copy_table: an entry needs two contiguous buffers of one length")
        rows.append([ptr(dst, (torch.float32,)), ptr(src, (torch.float32,)), dst.numel()])
    if not rows:
        raise _C.LvaeHipError("copy_table: no entries")
    return torch.tensor(rows, dtype=torch.int64).to(device)


def multi_copy(table, flag=None, want=0):
    """Every entry of a copy_table in one launch (one workgroup per entry); with `flag` (device int32[1]) only when flag[0] == want."""
    if table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != 3 or not table.is_contiguous():
        raise _C.LvaeHipError("multi_copy: the table is a contiguous device int64 [entries][3]")
    call('lvae_multi_copy_f32', ptr(table, (torch.int64,)), table.shape[0], ptr(flag, (torch.int32,)), int(want), stream_ptr())


def bn_recal_table(pairs, device):
    """[(stat, acc)] pairs of contiguous device tensors of equal length, stat float32 and acc float64 -> the device table bn_recal_fold and
    bn_recal_finish take (int64 [len][3]: struct lvae_bn_recal_entry). The caller keeps the tensors alive and in place for as long as the
    table is used."""
    rows = []
    for stat, acc in pairs:
        if stat.numel() != acc.numel() or stat.numel() < 1 or not (stat.is_contiguous() and acc.is_contiguous()):
            raise _C.LvaeHipError("bn_recal_table: an entry needs two contiguous buffers of one length")
        rows.append([ptr(stat, (torch.float32,)), ptr(acc, (torch.float64,)), stat.numel()])
    if not rows:
        raise _C.LvaeHipError("bn_recal_table: no entries")
    return torch.tensor(rows, dtype=torch.int64).to(device)


def _bn_recal_args(table, count, what):
    if table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != 3 or not table.is_contiguous():
        raise _C.LvaeHipError("%s: the table is a contiguous device int64 [entries][3]" % what)
    if count.dtype != torch.int64 or count.numel() != 2 or not count.is_contiguous():
        raise _C.LvaeHipError("%s: the count is a contiguous device int64[2] (folds so far, finish's ticket)" % what)


def bn_recal_fold(table, count):
    """acc += (double)stat for every entry of a bn_recal_table, count[0] += 1: one launch, one workgroup per entry."""
    _bn_recal_args(table, count, 'bn_recal_fold')
    call('lvae_bn_recal_fold_f64', ptr(table, (torch.int64,)), table.shape[0], ptr(count, (torch.int64,)), stream_ptr())


def bn_recal_finish(table, count, flag):
    """stat = (float)(acc / count[0]) for every entry, then the accumulators and the count are cleared: one launch. flag (device int32[1])
    is set to 1 when a value written is not finite; the caller clears it."""
    _bn_recal_args(table, count, 'bn_recal_finish')
    if flag.dtype != torch.int32 or flag.numel() != 1:
        raise _C.LvaeHipError("bn_recal_finish: the flag is a device int32[1]")
    call('lvae_bn_recal_finish_f32', ptr(table, (torch.int64,)), table.shape[0], ptr(count, (torch.int64,)), ptr(flag, (torch.int32,)),
         stream_ptr())


def swap(a, b):
    """a <-> b in place, one pass (two contiguous fp32 buffers of one length). The caller says when weights moved (weights_written)."""
    if a.numel() != b.numel() or not (a.is_contiguous() and b.is_contiguous()):
        raise _C.LvaeHipError("swap needs two contiguous buffers of one length")
    call('lvae_swap_f32', ptr(a, (torch.float32,)), ptr(b, (torch.float32,)), a.numel(), stream_ptr())


def l2norm(x, out=None):
    if out is None:
        out = torch.empty((1,), dtype=torch.float32, device=x.device)
    need = _C.load().lvae_sumsq_workspace(x.numel())
    ws = workspace(need, x.device)
    call('lvae_l2norm_f32', ptr(x), x.numel(), ptr(out), ws.data_ptr(), ws.numel(), stream_ptr())
    return out


def rng_fill(out, kind, lo, hi, seed, offset, stream_id):
    """kind: 'normal' | 'uniform' | 'bernoulli' (keep-prob lo, kept value hi). offset: device int64[1] step counter."""
    k = {'normal': 0, 'uniform': 1, 'bernoulli': 2}[kind]
    call('lvae_rng_fill_f32', ptr(out), out.numel(), k, float(lo), float(hi), int(seed) & (2 ** 64 - 1),
         offset.data_ptr() if offset is not None else None, int(stream_id), stream_ptr())
    return out


def counter_advance(counter, by=1):
    call('lvae_counter_advance', counter.data_ptr(), int(by), stream_ptr())


def counter_advance_unless(counter, by, flag):
    """counter += by unless flag[0] != 0 (device int32[1]: the gradient guard's skip flag)."""
    call('lvae_counter_advance_unless', counter.data_ptr(), int(by), ptr(flag, (torch.int32,)), stream_ptr())


def _batch_gather_args(name, table, channels_last, out, index, steps_per_epoch, global_batch):
    """The checks batch_gather and batch_gather_aug share -> (N, C, H, W, n)."""
    if table.dim() != 4 or table.dtype not in (torch.uint8, torch.float32) or not table.is_contiguous():
        raise _C.LvaeHipError("%s: the image table must be a contiguous 4-d uint8 or float32 tensor" % name)
    N = table.shape[0]
    Cn, H, W = (table.shape[3], table.shape[1], table.shape[2]) if channels_last else tuple(table.shape[1:])
    n = out.shape[0]
    if out.dtype != torch.float32 or tuple(out.shape) != (n, Cn, H, W) or not out.is_contiguous():
        raise _C.LvaeHipError("%s: out must be contiguous float32 (n, %d, %d, %d), got %s %s" % (name, Cn, H, W, out.dtype,
                                                                                                tuple(out.shape)))
    if index is not None and index.numel() != int(steps_per_epoch) * int(global_batch):
        raise _C.LvaeHipError("%s: the index table has %d entries, an epoch %d x %d" % (name, index.numel(), steps_per_epoch,
                                                                                       global_batch))
    return N, Cn, H, W, n


def batch_gather(table, channels_last, out, index=None, cursor=None, steps_per_epoch=0, global_batch=0, lo=0, base=0):
    """out (n, C, H, W) float32 <- n images of `table` (uint8 (N,C,H,W), uint8 (N,H,W,C) with channels_last, or float32 (N,C,H,W)).
    With `index` (device int32 [steps_per_epoch * global_batch]) row r is image index[(cursor[0] % steps_per_epoch) * global_batch + lo + r]
    (`cursor`: device int64[1] of completed steps, None = position 0); without it, image base + r. uint8 -> float32 as v / 255."""
    N, Cn, H, W, n = _batch_gather_args('batch_gather', table, channels_last, out, index, steps_per_epoch, global_batch)
    call('lvae_batch_gather_f32', ptr(table), _C.FEED_U8 if table.dtype == torch.uint8 else _C.FEED_F32, int(bool(channels_last)), N, Cn,
         H, W, ptr(index, (torch.int32,)), ptr(cursor, (torch.int64,)), int(steps_per_epoch), int(global_batch), int(lo), int(base), n,
         ptr(out, (torch.float32,)), stream_ptr())
    return out


AUG_MODES = {None: _C.AUG_NONE, 'none': _C.AUG_NONE, 'binarize': _C.AUG_BINARIZE, 'dequantize': _C.AUG_DEQUANTIZE}


def feed_aug(seed, mode=None, hflip=False, fixed=False, position=0):
    """An lvae_feed_aug: mode None | 'binarize' | 'dequantize', rows mirrored at random with hflip, the per-image `fixed` noise
    (binarize_fixed), and the position that stands in for the cursor when a call has none."""
    if mode not in AUG_MODES:
        raise ValueError("feed augmentation mode %r (one of None, 'binarize', 'dequantize')" % (mode,))
    return _C.FeedAug(int(seed) & (2 ** 64 - 1), int(position), AUG_MODES[mode], int(bool(hflip)), int(bool(fixed)))


def batch_gather_aug(table, channels_last, out, aug, index=None, cursor=None, steps_per_epoch=0, global_batch=0, lo=0, base=0, position=0):
    """batch_gather with the batch augmented in the same launch (lvae_batch_gather_aug_f32). aug: a `feed_aug` (its own position is
    replaced by `position`): Bernoulli draws of every pixel ('binarize'), uniform noise below one 8-bit step ('dequantize', uint8
    tables), rows mirrored in W (hflip). The noise is a pure function of (aug.seed, cursor[0] or `position`, lo + r, element), or with
    aug.fixed / without an index table of (aug.seed, image number, element): the same call gives the same batch, eager or captured."""
    N, Cn, H, W, n = _batch_gather_args('batch_gather_aug', table, channels_last, out, index, steps_per_epoch, global_batch)
    a = _C.FeedAug(aug.seed, int(position), aug.mode, aug.hflip, aug.fixed)
    call('lvae_batch_gather_aug_f32', ptr(table), _C.FEED_U8 if table.dtype == torch.uint8 else _C.FEED_F32, int(bool(channels_last)), N,
         Cn, H, W, ptr(index, (torch.int32,)), ptr(cursor, (torch.int64,)), int(steps_per_epoch), int(global_batch), int(lo), int(base), n,
         ptr(out, (torch.float32,)), C.byref(a), stream_ptr())
    return out


NN_MAX_K = 32


def nn_l2(queries, table, k, exclude=None):
    """The k rows of `table` ((N, D) contiguous uint8, a value meaning v / 255, or float32) nearest to each row of `queries` ((Q, D)
    contiguous float32) by squared L2 distance -> (index int32 (Q, k), dist float32 (Q, k)), ascending by (distance, row); slots without
    an eligible row hold (-1, +inf). exclude: None, or a device int32 tensor (Q,) naming a row each query skips (-1: none). The distance
    is sum (q - t)^2 with the difference taken first: a query equal to a row gives exactly 0, and a pair's bits do not depend on Q, N, k
    or exclude (lvae_nn_l2_f32). Two launches on the current stream, no host wait."""
    pq, pt = ptr(queries, (torch.float32,)), ptr(table, (torch.uint8, torch.float32))   # (CPU tensors are refused here)
    if queries.dim() != 2 or table.dim() != 2 or queries.shape[1] != table.shape[1] or not (queries.is_contiguous() and table.is_contiguous()):
        raise _C.LvaeHipError("nn_l2: queries (Q, D) and table (N, D) must be contiguous and share D, got %s strides %s and %s strides %s"
                              % (tuple(queries.shape), queries.stride(), tuple(table.shape), table.stride()))
    Q, D = (int(s) for s in queries.shape)
    N = int(table.shape[0])
    if not 1 <= int(k) <= NN_MAX_K:
        raise ValueError("k must be between 1 and %d, got %r" % (NN_MAX_K, k))
    if exclude is not None and (exclude.dtype != torch.int32 or tuple(exclude.shape) != (Q,) or not exclude.is_contiguous()):
        raise _C.LvaeHipError("nn_l2: exclude must be a contiguous int32 tensor of shape (%d,), got %s %s" % (Q, exclude.dtype, tuple(exclude.shape)))
    index = torch.empty((Q, int(k)), dtype=torch.int32, device=queries.device)
    dist = torch.empty((Q, int(k)), dtype=torch.float32, device=queries.device)
    ws = workspace(_C.load().lvae_nn_l2_workspace(Q, N, int(k)), queries.device)
    call('lvae_nn_l2_f32', pq, Q, pt, _C.FEED_U8 if table.dtype == torch.uint8 else _C.FEED_F32, N, D, ptr(exclude, (torch.int32,)), int(k),
         ptr(index, (torch.int32,)), ptr(dist, (torch.float32,)), ws.data_ptr(), ws.numel(), stream_ptr())
    return index, dist


SPECTRAL_MAX_K, SPECTRAL_MAX_COUT = 4096, 1024   # what lvae_spectral_step_f32 holds of one matrix in LDS


def spectral_table(rows, device):
    """[(param offset, grad offset, K, Cout, u offset, v offset)] -> the device table spectral_step takes (int64 [len][6]: struct
    lvae_spectral_entry). ValueError for an empty list or a matrix the kernel does not take."""
    if not rows:
        raise ValueError("spectral_table: no entries")
    for r in rows:
        if len(r) != 6 or not (1 <= r[2] <= SPECTRAL_MAX_K and 1 <= r[3] <= SPECTRAL_MAX_COUT):
            raise ValueError("spectral_table: an entry is (param offset, grad offset, K <= %d, Cout <= %d, u offset, v offset), got %r"
                             % (SPECTRAL_MAX_K, SPECTRAL_MAX_COUT, tuple(r)))
    return torch.tensor([list(map(int, r)) for r in rows], dtype=torch.int64).to(device)


def spectral_step(table, params, grads, u_in, u_out, v_out, sigma_out, lam=0.0, gscale=None, max_workgroups=0):
    """One power-iteration step for every entry of a spectral_table in one launch: u_in -> v_out, u_out (may be u_in), sigma_out; with
    `grads` also grads[entry] += (lam / gscale) v' u'^T, with grads=None nothing but the iterate is written."""
    if table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != 6 or not table.is_contiguous():
        raise _C.LvaeHipError("spectral_step: the table is a contiguous device int64 [entries][6]")
    if u_in.numel() != u_out.numel() or sigma_out.numel() != table.shape[0]:
        raise _C.LvaeHipError("spectral_step: u_in and u_out have one length, sigma_out one float per entry")
    for t in (params, grads, u_in, u_out, v_out, sigma_out):
        if t is not None and not t.is_contiguous():
            raise _C.LvaeHipError("spectral_step: every buffer is contiguous")
    f = (torch.float32,)
    call('lvae_spectral_step_f32', ptr(table, (torch.int64,)), table.shape[0], ptr(params, f), params.numel(), ptr(grads, f),
         0 if grads is None else grads.numel(), ptr(u_in, f), ptr(u_out, f), u_in.numel(), ptr(v_out, f), v_out.numel(), ptr(sigma_out, f),
         float(lam), ptr(gscale, f), int(max_workgroups), stream_ptr())


def spectral_reduce(sigma, out):
    """out[0] = sum of the sigmas, out[1] = their maximum (device float[2]); one launch."""
    if out.numel() != 2 or not (sigma.is_contiguous() and out.is_contiguous()):
        raise _C.LvaeHipError("spectral_reduce: out is a contiguous device float[2]")
    call('lvae_spectral_reduce_f32', ptr(sigma, (torch.float32,)), sigma.numel(), ptr(out, (torch.float32,)), stream_ptr())
    return out
