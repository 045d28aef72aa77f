"""Kernel routing of the convolution entry points, asked through the host-only queries (no GPU, no launch).

Every query of a family (workspace, variant, statistics rows, folded BatchNorm finalize, bf16 storage, weight-gradient workspace /
variant / apply) must answer for the kernel the launch takes. The table covers every convolution of the BASELINE configs at their
batch sizes (forward, dgrad view, weight gradient) in both precisions and both forms, with the workspace absent, sized, too small and
only 8-byte aligned, and both statistics modes. The descriptors carry fake, never-dereferenced pointers: this module never calls a
launch entry point. Expected answers: conv_routing_expected.json next to this file.

The 1x1 gate / concat-dgrad family (`gate:` and `merge:` cases, also with form F32_MFMA) answers through its own queries: the kernel of the
gate forward and its statistics rows on the forward view, the single-shot gate backward, the persistent gate backward's workspace and
whether it takes a deferred apply on the 128 -> 64 dgrad view, and the one-launch concat dgrad of a merge convolution at split = C1.
DECLINES lists descriptors those kernels refuse, with the answers written down from the kernels' conditions.

The weight gradient is routed through one ordered table of kernel families (img -> bf16 -> Winograd -> 1x1 -> tile -> thin -> generic).
WGRAD_DECLINES lists descriptors one family refuses and the next takes. `schedule:` cases are the answer of
lvae_conv2d_wgrad_grouped_schedule, [launches, launch_of...], for the forward convolutions of a config and for the synthetic lists
SCHEDULE_LISTS at the edges of the grouping rule; tests/test_kernels_gpu.py runs the same lists on the GPU.
"""
import ctypes as C
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
EXPECTED = os.path.join(HERE, 'conv_routing_expected.json')

PREC_F32, PREC_BF16 = 0, 1
FORM_AUTO, FORM_F32_MFMA, FORM_SIX_PRODUCT_DIRECT = 0, 1, 3
GATHER_CONV, GATHER_TRANSPOSED = 0, 1
STATS_BN_FWD, STATS_BN_BWD = 0, 1
DT_BF16 = 1

# (name, colour channels, image side, downsample flags, images per GPU): BASELINE configs[0], [1], [2] / [3] per GPU, [4] per GPU
CONFIGS = [
    ('mnist3', 1, 28, [1, 1, 1], 64),
    ('mnist12', 1, 28, [0, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0], 256),
    ('cifar15', 3, 32, [0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0], 256),
    ('celeba20', 3, 64, [0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], 128),
]
NF, ZD = 64, 32   # n_filters, z_dims


def _down(h):
    return (h + 2 - 3) // 2 + 1   # 3x3 stride 2 pad 1


def convs(color, img, downsample):
    """(tag, Cin1, Cin2, Cout, k, stride, pad, transposed, H, W, OH, OW) of every distinct convolution of the model: 5x5 stride-2 stem,
    residual-block 3x3, gate 1x1 (64 -> 128), merge 1x1 (64 + 64 -> 64), stochastic 3x3 (64 -> 2z, z -> 64), stride-2 3x3 and its
    transposed up-sampling, and the likelihood head."""
    out = set()
    h = (img + 4 - 5) // 2 + 1
    out.add(('stem', color, 0, NF, 5, 2, 2, False, img, img, h, h))
    out.add(('head', NF, 0, 100 if color == 3 else 1, 3, 1, 1, False, img, img, img, img))
    for ds in downsample:
        if ds:
            out.add(('down', NF, 0, NF, 3, 2, 1, False, h, h, _down(h), _down(h)))
            out.add(('up', NF, 0, NF, 3, 2, 1, True, _down(h), _down(h), h, h))
            h = _down(h)
        for tag, c1, c2, co, k in (('res', NF, 0, NF, 3), ('gate', NF, 0, 2 * NF, 1), ('merge', NF, NF, NF, 1), ('q', NF, 0, 2 * ZD, 3),
                                   ('z', ZD, 0, NF, 3)):
            out.add((tag, c1, c2, co, k, 1, k // 2, False, h, h, h, h))
    return sorted(out)


_BASE = 1 << 32


def _fake(i):
    return _BASE + (i << 24)   # distinct, 256-byte aligned, never dereferenced


def make_desc(N, H, W, OH, OW, C1, C2, Cout, k, stride, pad, gather, wsk, wsn, prec, form):
    from lvae_amd._C import ConvDesc
    d = ConvDesc()
    d.x, d.x2, d.C1, d.C2 = _fake(1), (_fake(2) if C2 else None), C1, C2
    d.w, d.w_stap, d.w_sk, d.w_sn = _fake(3), (C1 + C2) * Cout, wsk, wsn
    d.bias, d.y = _fake(4), _fake(5)
    d.N, d.H, d.W, d.OH, d.OW, d.Cout = N, H, W, OH, OW, Cout
    d.KH = d.KW = k
    d.stride, d.pad, d.gather, d.precision, d.form = stride, pad, gather, prec, form
    return d


def views(N, conv):
    """(view, descriptor factory) pairs: the forward convolution and, for a plain convolution without a second source, its dgrad view"""
    tag, C1, C2, Cout, k, s, p, tr, H, W, OH, OW = conv
    g = GATHER_TRANSPOSED if tr else GATHER_CONV
    out = [('fwd', lambda pr, fm: make_desc(N, H, W, OH, OW, C1, C2, Cout, k, s, p, g, Cout, 1, pr, fm))]
    if not tr and C2 == 0:
        out.append(('dgrad', lambda pr, fm: make_desc(N, OH, OW, H, W, Cout, 0, C1, k, s, p, GATHER_TRANSPOSED, 1, Cout, pr, fm)))
    return out


WS = ('none', 'sized', 'small', 'align8')
STATS = (STATS_BN_FWD, STATS_BN_BWD)
CONV_QUERIES = ('lvae_conv2d_workspace', 'lvae_conv2d_variant', 'lvae_conv2d_stats_rows', 'lvae_conv2d_folds_bn_finalize',
                'lvae_conv2d_stats_buffer_rows', 'lvae_resblock_bf16_storage')
WGRAD_QUERIES = ('lvae_conv2d_wgrad_workspace', 'lvae_conv2d_wgrad_variant', 'lvae_conv2d_wgrad_apply_ok')


def variants(mk, need, bf16_storage):
    """The descriptors of one convolution, in a fixed order: storage (fp32, then bf16 when asked) x workspace WS x statistics mode STATS"""
    for st in ((False, True) if bf16_storage else (False,)):
        for ws in WS:
            for mode in STATS:
                d = mk()
                if st:
                    d.x_dtype = d.y_dtype = DT_BF16
                if ws != 'none':
                    want = need if need else 4096
                    d.workspace = _fake(6) + (8 if ws == 'align8' else 0)
                    d.workspace_bytes = want // 2 if ws == 'small' else want
                d.stats_out, d.stats_pivot, d.stats_mode = _fake(7), _fake(8), mode
                if mode == STATS_BN_BWD:
                    d.stats_x = _fake(9)
                yield d


GATE_FWD_QUERIES = ('lvae_conv1x1_gate_variant', 'lvae_conv1x1_gate_stats_rows')
GATE_BWD_QUERIES = ('lvae_conv1x1_gate_bwd_ok', 'lvae_conv1x1_gate_bwd_wgrad_workspace', 'lvae_conv1x1_gate_bwd_wgrad_apply_ok')


def gate_fwd_desc(N, H, W, C, prec, form):
    return make_desc(N, H, W, H, W, C, 0, 2 * C, 1, 1, 0, GATHER_CONV, 2 * C, 1, prec, form)


def gate_bwd_desc(N, H, W, C, prec, form):
    """the dgrad view of the gate convolution C -> 2C: what both gate backwards are described by"""
    return make_desc(N, H, W, H, W, 2 * C, 0, C, 1, 1, 0, GATHER_TRANSPOSED, 1, 2 * C, prec, form)


def merge_dgrad_desc(N, H, W, C1, C2, Cout, prec, form):
    return make_desc(N, H, W, H, W, Cout, 0, C1 + C2, 1, 1, 0, GATHER_TRANSPOSED, 1, Cout, prec, form)


def gate_table(lib):
    """gate: [variant, stats_rows, gate_bwd_ok, persistent-backward workspace, apply_ok]; merge: [dgrad_cat_ok at split = C1]"""
    ask = lambda names, d: [int(getattr(lib, q)(C.byref(d))) for q in names]
    out = {}
    for cname, color, img, downsample, N in CONFIGS:
        for tag, C1, C2, Cout, k, s, p, tr, H, W, OH, OW in convs(color, img, downsample):
            for prec in (PREC_F32, PREC_BF16):
                for form in (FORM_AUTO, FORM_SIX_PRODUCT_DIRECT, FORM_F32_MFMA):
                    base = '%s/N%d/%dx%d/%d+%d->%d/p%d/f%d' % (tag, N, H, W, C1, C2, Cout, prec, form)
                    if tag == 'gate':
                        out['gate:' + base] = (ask(GATE_FWD_QUERIES, gate_fwd_desc(N, H, W, C1, prec, form)) +
                                               ask(GATE_BWD_QUERIES, gate_bwd_desc(N, H, W, C1, prec, form)))
                    elif tag == 'merge':
                        out['merge:' + base] = [int(lib.lvae_conv1x1_dgrad_cat_ok(C.byref(merge_dgrad_desc(N, H, W, C1, C2, Cout, prec, form)), C1))]
    return out


def _mod(d, **fields):
    for k, v in fields.items():
        setattr(d, k, v)
    return d


GATE_PERSISTENT, GATE_SINGLE_SHOT = 1, 2
# Descriptors the 1x1 kernels decline (or take by another kernel), on the 16x16 level at batch 256 (65536 pixels: 512 workgroups of the
# persistent forward, 256 slabs of [64][128] + [128] floats of the persistent backward) unless a shape is given. The answers follow from
# the conditions of the kernels: the single-shot kernel needs 1x1 / stride 1, at most 128 reduction and output channels (multiples of 4; 8
# for the gate), 16-byte aligned descriptor pointers and a unit weight stride along one axis with the other a multiple of 4; the
# persistent forward is 64 -> 128 with x aligned, any weight strides, bf16 storage only at bf16 precision; the persistent backward is the
# 128 -> 64 view with w_sk = 1, w_sn % 4 == 0, w / y / out_scale aligned, at least 16384 pixels, bf16 storage only at bf16 precision.
_BIG = (256, 16, 16)
_WS = 256 * (64 * 128 + 128) * 4
DECLINES = [   # (name, kind, descriptor factory, expected)
    ('w+4', 'fwd', lambda: _mod(gate_fwd_desc(*_BIG, 64, PREC_F32, FORM_AUTO), w=_fake(3) + 4), [GATE_PERSISTENT, 512]),
    ('w+4', 'bwd', lambda: _mod(gate_bwd_desc(*_BIG, 64, PREC_F32, FORM_AUTO), w=_fake(3) + 4), [0, 0, 0]),
    ('w+4', 'cat64', lambda: _mod(merge_dgrad_desc(*_BIG, 64, 64, 64, PREC_F32, FORM_AUTO), w=_fake(3) + 4), [0]),
    ('w+4 small', 'fwd', lambda: _mod(gate_fwd_desc(4, 8, 8, 16, PREC_F32, FORM_AUTO), w=_fake(3) + 4), [0, 0]),
    ('aligned small', 'fwd', lambda: gate_fwd_desc(4, 8, 8, 16, PREC_F32, FORM_AUTO), [GATE_SINGLE_SHOT, 4]),
    ('aligned small', 'bwd', lambda: gate_bwd_desc(4, 8, 8, 16, PREC_F32, FORM_AUTO), [1, 0, 0]),
    ('split 62', 'cat62', lambda: merge_dgrad_desc(*_BIG, 64, 64, 64, PREC_F32, FORM_AUTO), [0]),
    ('split Cout', 'cat128', lambda: merge_dgrad_desc(*_BIG, 64, 64, 64, PREC_F32, FORM_AUTO), [0]),
    ('split 64', 'cat64', lambda: merge_dgrad_desc(*_BIG, 64, 64, 64, PREC_F32, FORM_AUTO), [1]),
    ('132 reduction channels', 'fwd', lambda: gate_fwd_desc(*_BIG, 132, PREC_F32, FORM_AUTO), [0, 0]),
    ('132 reduction channels', 'bwd', lambda: _mod(gate_bwd_desc(*_BIG, 64, PREC_F32, FORM_AUTO), C1=132), [0, 0, 0]),
    ('132 reduction channels', 'cat64', lambda: _mod(merge_dgrad_desc(*_BIG, 64, 64, 64, PREC_F32, FORM_AUTO), C1=132), [0]),
    ('no unit stride', 'fwd', lambda: _mod(gate_fwd_desc(*_BIG, 64, PREC_F32, FORM_AUTO), w_sk=256, w_sn=2), [GATE_PERSISTENT, 512]),
    ('no unit stride small', 'fwd', lambda: _mod(gate_fwd_desc(4, 8, 8, 16, PREC_F32, FORM_AUTO), w_sk=64, w_sn=2), [0, 0]),
    ('no unit stride', 'bwd', lambda: _mod(gate_bwd_desc(*_BIG, 64, PREC_F32, FORM_AUTO), w_sk=2, w_sn=256), [0, 0, 0]),
    ('no unit stride', 'cat64', lambda: _mod(merge_dgrad_desc(*_BIG, 64, 64, 64, PREC_F32, FORM_AUTO), w_sk=2, w_sn=128), [0]),
    ('w_sn 130', 'bwd', lambda: _mod(gate_bwd_desc(*_BIG, 64, PREC_F32, FORM_AUTO), w_sn=130), [0, 0, 0]),
    ('w_sn 130', 'cat64', lambda: _mod(merge_dgrad_desc(*_BIG, 64, 64, 64, PREC_F32, FORM_AUTO), w_sn=130), [0]),
    ('w_sn 18 small', 'fwd', lambda: _mod(gate_fwd_desc(4, 8, 8, 16, PREC_F32, FORM_AUTO), w_sk=1, w_sn=18), [0, 0]),
    ('bf16 x at fp32', 'fwd', lambda: _mod(gate_fwd_desc(*_BIG, 64, PREC_F32, FORM_AUTO), x_dtype=DT_BF16), [0, 0]),
    ('bf16 x at fp32', 'bwd', lambda: _mod(gate_bwd_desc(*_BIG, 64, PREC_F32, FORM_AUTO), x_dtype=DT_BF16), [1, 0, 0]),
    ('bf16 x at bf16', 'fwd', lambda: _mod(gate_fwd_desc(*_BIG, 64, PREC_BF16, FORM_AUTO), x_dtype=DT_BF16), [GATE_PERSISTENT, 512]),
    ('bf16 x at bf16', 'bwd', lambda: _mod(gate_bwd_desc(*_BIG, 64, PREC_BF16, FORM_AUTO), x_dtype=DT_BF16), [1, _WS, 1]),
    ('bf16 x', 'cat64', lambda: _mod(merge_dgrad_desc(*_BIG, 64, 64, 64, PREC_BF16, FORM_AUTO), x_dtype=DT_BF16), [0]),
    ('Cout 24', 'fwd', lambda: gate_fwd_desc(3, 3, 3, 12, PREC_F32, FORM_AUTO), [GATE_SINGLE_SHOT, 0]),
    ('f32 mfma', 'bwd', lambda: gate_bwd_desc(*_BIG, 64, PREC_F32, FORM_F32_MFMA), [1, _WS, 0]),
    ('f32 mfma at bf16', 'bwd', lambda: gate_bwd_desc(*_BIG, 64, PREC_BF16, FORM_F32_MFMA), [1, _WS, 1]),
    ('16383 pixels', 'bwd', lambda: gate_bwd_desc(1, 127, 129, 64, PREC_F32, FORM_AUTO), [1, 0, 0]),
]


def same_conv_desc(N, H, W, C1, C2, Cout, k, prec=PREC_F32, form=FORM_AUTO):
    """a stride-1 "same" convolution (k = 1 or 3) as the weight gradient sees it"""
    return make_desc(N, H, W, H, W, C1, C2, Cout, k, 1, k // 2, GATHER_CONV, Cout, 1, prec, form)


# Lists of (N, C1, C2, Cout, H, W, k) stride-1 "same" convolutions whose gradients go out in one grouped call, at the edges of the
# schedule: a group flushes at its family's capacity (12 tile, 12 Winograd, 32 whole-image), a tile or Winograd gradient left alone goes
# out singly after all groups, a whole-image group of one stays in place, Winograd groups form per image width and only below 65536 pixels.
_TILE = (4, 64, 0, 64, 16, 16, 3)         # 1024 pixels: below the Winograd floor, above the whole-image sizes -> tile kernel <64, 3>
_IMG = (16, 64, 0, 64, 2, 2, 3)           # whole-image kernel, 3x3 kind
_IMG1 = (20, 64, 0, 128, 4, 4, 1)         # whole-image kernel, 1x1 kind
_WINO16 = (64, 64, 0, 64, 16, 16, 3)      # 16384 pixels: Winograd, width 16
_WINO32 = (16, 64, 0, 64, 32, 32, 3)      # 16384 pixels: Winograd, width 32
_WINO8 = (257, 64, 0, 128, 8, 8, 3)       # Winograd, width 8, two output-channel blocks (64 -> 128 is not a whole-image shape)
_WINO_BIG = (256, 64, 0, 64, 16, 16, 3)   # 65536 pixels: Winograd, fills the chip alone
_MERGE = (4, 64, 64, 64, 16, 16, 1)       # merge 1x1 over cat(x, x2): tile kernel <128, 1>
_ODD = (2, 16, 0, 6, 16, 16, 3)           # Cout % 4 != 0: generic kernel
SCHEDULE_LISTS = {
    'tile13': [_TILE] * 13,
    'img34': [_IMG] * 34,
    'wino_same_width': [_WINO16, _WINO16],
    'wino_two_widths': [_WINO16, _WINO32],
    'wino_65536': [_WINO_BIG, _WINO_BIG],
    'merge_x2': [_MERGE, _MERGE],
    'mixed': [_WINO32, _IMG, _ODD, _TILE, _WINO8, _MERGE, _IMG1, _WINO16, _WINO_BIG, _IMG, _WINO8, _TILE, _WINO32, _IMG1, _MERGE, _WINO16,
              _TILE, _IMG],
}


def schedule(lib, descs):
    """[launches, launch_of[0], launch_of[1], ...] of lvae_conv2d_wgrad_grouped_schedule"""
    from lvae_amd._C import ConvDesc
    n = len(descs)
    arr = (ConvDesc * n)(*descs)
    launch_of = (C.c_int32 * n)(*([-1] * n))
    return [int(lib.lvae_conv2d_wgrad_grouped_schedule(arr, n, launch_of))] + list(launch_of)


# Descriptors one weight-gradient family refuses and a later one takes: (name, descriptor factory, [workspace, variant, apply_ok]). The
# answers follow from the kernels' conditions; every workspace is slabs * (taps * Cin * Cout + Cout) * 4 bytes unless noted.
WG_GENERIC, WG_IMG, WG_BF16, WG_WINO, WG_1X1, WG_TILE, WG_THIN = range(7)
_L8 = (256, 8, 8, 64, 0, 64, 3)   # the 8x8 level at batch 256: 16384 pixels, a whole-image shape


def _slabs(n, taps, cin, cout):
    return n * (taps * cin * cout + cout) * 4


_WINO_SLAB = 2 * 16 * 32 * 64 + 64   # floats per Winograd range and output-channel block: 2 ci blocks x 16 positions x 32 ci x 64 co, + bias
WGRAD_DECLINES = [
    # the whole-image kernel: 64 tiles of one image, 8 per workgroup -> 32 slabs
    ('8x8 level', lambda: same_conv_desc(*_L8), [_slabs(32, 9, 64, 64), WG_IMG, 0]),
    # x only 4-byte aligned: img, Winograd and tile all load x in 16-byte pieces; not a stem -> generic, 512 / 9 taps -> 57 pixel ranges
    ('x+4', lambda: _mod(same_conv_desc(*_L8), x=_fake(1) + 4), [_slabs(57, 9, 64, 64), WG_GENERIC, 0]),
    # in_scale without in_shift: only img spells the refusal out; Winograd takes it: 256 chunks of 16 tiles, at least 4 per range -> 64
    # ranges (W = 8: no deferred apply)
    ('in_scale without in_shift', lambda: _mod(same_conv_desc(*_L8), in_scale=_fake(10)), [64 * _WINO_SLAB * 4, WG_WINO, 0]),
    # the direct 1x1 kernel starts at 32768 pixels (256 workgroups); one pixel less has an odd width, which the tile kernel refuses -> generic
    ('1x1 at 32768 pixels', lambda: same_conv_desc(128, 16, 16, 64, 0, 128, 1), [_slabs(256, 1, 64, 128), WG_1X1, 0]),
    ('1x1 at 32767 pixels', lambda: same_conv_desc(7, 31, 151, 64, 0, 128, 1), [_slabs(64, 1, 64, 128), WG_GENERIC, 0]),
    # the Winograd floor of 16384 pixels: N = 64 has 256 chunks of 16 tiles, at least 4 per range -> 64 ranges, and takes a deferred apply
    # (64 -> 64, W = 16); N = 63 goes to the tile kernel, whose two LDS buffers hold 64-pixel tiles of a 16-wide image with 64 input
    # channels (128-pixel ones need 170 KB) -> 252 tiles, fewer than the 256 workgroups wanted -> 252 slabs
    ('3x3 at 16384 pixels', lambda: same_conv_desc(64, 16, 16, 64, 0, 64, 3), [64 * _WINO_SLAB * 4, WG_WINO, 1]),
    ('3x3 at 16128 pixels', lambda: same_conv_desc(63, 16, 16, 64, 0, 64, 3), [_slabs(252, 9, 64, 64), WG_TILE, 0]),
    # the stem (5x5 stride 2 on 3 channels): the thin kernel wants at least 32 images, one slab each; below, the generic kernel with
    # 512 / 25 taps -> 21 wanted, 31 * 256 pixels / 256 = 31 possible -> 21 pixel ranges
    ('stem at N = 32', lambda: make_desc(32, 32, 32, 16, 16, 3, 0, 64, 5, 2, 2, GATHER_CONV, 64, 1, PREC_F32, FORM_AUTO),
     [_slabs(32, 25, 3, 64), WG_THIN, 0]),
    ('stem at N = 31', lambda: make_desc(31, 32, 32, 16, 16, 3, 0, 64, 5, 2, 2, GATHER_CONV, 64, 1, PREC_F32, FORM_AUTO),
     [_slabs(21, 25, 3, 64), WG_GENERIC, 0]),
    # odd W: the tile kernel pairs pixels -> generic, 960 pixels / 256 -> 4 ranges
    ('odd W', lambda: same_conv_desc(4, 16, 15, 64, 0, 64, 3), [_slabs(4, 9, 64, 64), WG_GENERIC, 0]),
    # bf16-stored x at bf16 precision: img wants fp32 storage, the bf16 kernel takes it. 256x16x16: 512 tiles of 128 pixels -> the half-slab
    # form with 128 pixel ranges; 256x8x8: only 128 tiles of 128 pixels, fewer than CUs -> 256 tiles of 64, 2 per workgroup -> 128 slabs of
    # the whole-slab form
    ('bf16 x at bf16, 16x16', lambda: _mod(same_conv_desc(256, 16, 16, 64, 0, 64, 3, PREC_BF16), x_dtype=DT_BF16), [_slabs(128, 9, 64, 64), WG_BF16, 0]),
    ('bf16 x at bf16, 8x8', lambda: _mod(same_conv_desc(*_L8, PREC_BF16), x_dtype=DT_BF16), [_slabs(128, 9, 64, 64), WG_BF16, 0]),
    # 64 -> 128 3x3 at 257x8x8: more than img's 64 output channels -> Winograd with two output-channel blocks: 257 chunks, 128 / 2 = 64
    # ranges wanted -> 5 chunks per range -> 52 ranges
    ('3x3 64 -> 128 on 8x8', lambda: same_conv_desc(257, 8, 8, 64, 0, 128, 3), [52 * 2 * _WINO_SLAB * 4, WG_WINO, 0]),
]


def table():
    """{case id: answers}. conv: one [workspace, variant, stats_rows, folds, stats_buffer_rows, bf16_storage] per descriptor of
    variants(); wgrad: [workspace, variant, apply_ok]; grouped: the grouped workspace of all forward convolutions of a config; schedule:
    how the grouped call issues them, and the lists of SCHEDULE_LISTS."""
    from lvae_amd import _C
    lib = _C.load()
    ask = lambda names, d: [int(getattr(lib, q)(C.byref(d))) for q in names]
    out = {}
    for cname, color, img, downsample, N in CONFIGS:
        for prec in (PREC_F32, PREC_BF16):
            for form in (FORM_AUTO, FORM_SIX_PRODUCT_DIRECT):
                group = []
                for conv in convs(color, img, downsample):
                    for view, mk in views(N, conv):
                        base = '%s/N%d/%s/%dx%d/%d+%d->%d/k%ds%dp%d%s/p%d/f%d' % (
                            conv[0], N, view, conv[8], conv[9], conv[1], conv[2], conv[3], conv[4], conv[5], conv[6],
                            't' if conv[7] else '', prec, form)
                        m = lambda: mk(prec, form)
                        if view == 'fwd':
                            group.append(m())
                            out['wgrad:' + base] = ask(WGRAD_QUERIES, m())
                        need = lib.lvae_conv2d_workspace(C.byref(m()))
                        bf16_storage = prec == PREC_BF16 and conv[0] == 'res'
                        out['conv:' + base] = [ask(CONV_QUERIES, d) for d in variants(m, need, bf16_storage)]
                arr = (_C.ConvDesc * len(group))(*group)
                out['grouped:%s/p%d/f%d' % (cname, prec, form)] = int(lib.lvae_conv2d_wgrad_grouped_workspace(arr, len(group)))
                out['schedule:%s/p%d/f%d' % (cname, prec, form)] = schedule(lib, group)
    for name, specs in SCHEDULE_LISTS.items():
        out['schedule:%s/p0/f0' % name] = schedule(lib, [same_conv_desc(N, H, W, C1, C2, Cout, k) for N, C1, C2, Cout, H, W, k in specs])
    out.update(gate_table(lib))
    return out


def test_gate_plan_declines():
    import lvae_amd  # noqa: F401
    from lvae_amd import _C
    lib = _C.load()
    bad = []
    for name, kind, mk, want in DECLINES:
        d = mk()
        if kind == 'fwd':
            got = [int(getattr(lib, q)(C.byref(d))) for q in GATE_FWD_QUERIES]
        elif kind == 'bwd':
            got = [int(getattr(lib, q)(C.byref(d))) for q in GATE_BWD_QUERIES]
        else:
            got = [int(lib.lvae_conv1x1_dgrad_cat_ok(C.byref(d), int(kind[3:])))]
        if got != want:
            bad.append('%s (%s): got %s, expected %s' % (name, kind, got, want))
    assert not bad, '\n'.join(bad)


def test_wgrad_plan_declines():
    import lvae_amd  # noqa: F401
    from lvae_amd import _C
    lib = _C.load()
    bad = []
    for name, mk, want in WGRAD_DECLINES:
        d = mk()
        got = [int(getattr(lib, q)(C.byref(d))) for q in WGRAD_QUERIES]
        if got != want:
            bad.append('%s: got %s, expected %s' % (name, got, want))
    assert not bad, '\n'.join(bad)


def test_conv_routing_table():
    import lvae_amd  # noqa: F401
    with open(EXPECTED) as f:
        expected = json.load(f)
    got = table()
    assert sorted(got) == sorted(expected)
    bad = ['%s: got %s, expected %s' % (k, got[k], expected[k]) for k in sorted(got) if got[k] != expected[k]]
    assert not bad, '%d of %d entries differ:\n%s' % (len(bad), len(got), '\n'.join(bad[:40]))


if __name__ == '__main__':   # regenerate the expected answers from the current tree
    import sys
    sys.path.insert(0, os.path.dirname(HERE))
    import lvae_amd  # noqa: F401
    t = table()
    with open(EXPECTED, 'w') as f:   # one case per line
        f.write('{\n%s\n}\n' % ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(t[k], separators=(',', ':'))) for k in sorted(t)))
