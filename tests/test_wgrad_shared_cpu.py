"""How the shared launch of a stochastic layer's two or three Winograd weight gradients splits the chip (lvae_conv2d_wgrad_shared_schedule),
and what a 32-channel problem's single plan is: host-only queries, no GPU. A chunk is 16 Winograd tiles = 64 pixels; range r of a problem
takes chunks [r * cpr, min(total, (r + 1) * cpr)); a range is one workgroup per block of 32 input channels."""
import ctypes

import pytest

import lvae_amd  # noqa: F401
from lvae_amd import _C

MIN_CPR = 4   # LVAE_WINO_WGRAD_MIN_CPR of csrc/conv3x3_wgrad_wino.hip: a slab is worth writing from four chunks up


def desc(N, H, W, C1=64, Cout=64, prec=_C.PREC_F32):
    d = _C.ConvDesc()
    d.x, d.w, d.C1, d.C2 = 1 << 32, 1 << 33, C1, 0   # aligned, never dereferenced
    d.w_stap, d.w_sk, d.w_sn = C1 * Cout, Cout, 1
    d.N, d.H, d.W, d.OH, d.OW, d.Cout = N, H, W, H, W, Cout
    d.KH = d.KW = 3
    d.stride, d.pad, d.gather, d.precision = 1, 1, _C.GATHER_CONV, prec
    return d


def array(ds):
    arr = (_C.ConvDesc * len(ds))()
    for i, d in enumerate(ds):
        ctypes.memmove(ctypes.byref(arr, i * ctypes.sizeof(_C.ConvDesc)), ctypes.byref(d), ctypes.sizeof(_C.ConvDesc))
    return arr


def schedule(ds, aps=None):
    out = (ctypes.c_int32 * (3 * len(ds)))()
    ok = _C.load().lvae_conv2d_wgrad_shared_schedule(array(ds), aps, len(ds), out)
    return tuple(tuple(out[3 * i:3 * i + 3]) for i in range(len(ds))) if ok else None


def layer(N, H, W, n):
    """conv_out (32 -> 64), conv_in_q and, with n = 3, conv_in_p (64 -> 64)"""
    return [desc(N, H, W, C1=32)] + [desc(N, H, W) for _ in range(n - 1)]


@pytest.mark.parametrize('shape', [(64, 16, 16), (67, 16, 16), (256, 16, 16), (256, 8, 8), (16, 32, 32)])
@pytest.mark.parametrize('n', [1, 2, 3])
def test_shared_schedule_covers_every_chunk_once_inside_the_chip(shape, n):
    N, H, W = shape
    ds = layer(N, H, W, n)
    lib = _C.load()
    assert lib.lvae_conv2d_wgrad_shared_ok(array(ds), None, n) == 1
    sched = schedule(ds)
    total = N * H * W // 64
    assert sum(wgs for _, _, wgs in sched) <= 256          # one workgroup per CU
    for d, (ranges, cpr, wgs) in zip(ds, sched):
        assert ranges >= 1 and wgs == ranges * (d.C1 // 32)   # one workgroup per range and block of 32 input channels
        # ranges of cpr chunks from chunk 0 up: every chunk in exactly one range, none empty, only the last may be short
        assert (ranges - 1) * cpr < total <= ranges * cpr
        assert cpr >= MIN_CPR
    cprs = [cpr for _, cpr, _ in sched]
    assert max(cprs) - min(cprs) <= 1                      # chunks per workgroup: equal up to one rounding step
    # not one chunk per range fewer: the split is the tightest that fits (or stands at the least chunks per range)
    fits = lambda c: sum((d.C1 // 32) * -(-total // c) for d in ds) <= 256
    assert max(cprs) == MIN_CPR or not fits(max(cprs) - 1)
    piece = lambda d, r: (r * ((d.C1 // 32) * 32 * 16 * 64 + 64) * 4 + 255) // 256 * 256
    assert lib.lvae_conv2d_wgrad_shared_workspace(array(ds), n) == sum(piece(d, r) for d, (r, _, _) in zip(ds, sched))


def test_headline_splits_are_the_recorded_ones():
    """256x16x16, 1,024 chunks per problem, 1 + 2 + 2 workgroups per range: 5 x ceil(1024 / c) <= 256 from c = 21 (49 ranges, 245
    workgroups); with two problems 3 x ceil(1024 / c) <= 256 from c = 13. At the floor of 16,384 pixels (256 chunks): c = 6 and c = 4."""
    assert schedule(layer(256, 16, 16, 3)) == ((49, 21, 49), (49, 21, 98), (49, 21, 98))
    assert schedule(layer(256, 16, 16, 2)) == ((79, 13, 79), (79, 13, 158))
    assert schedule(layer(64, 16, 16, 3)) == ((43, 6, 43), (43, 6, 86), (43, 6, 86))
    assert schedule(layer(64, 16, 16, 2)) == ((64, 4, 64), (64, 4, 128))
    # the order of the problems is the caller's
    assert schedule([desc(256, 16, 16), desc(256, 16, 16, C1=32), desc(256, 16, 16)]) == ((49, 21, 98), (49, 21, 49), (49, 21, 98))


def test_query_declines_what_it_must():
    lib = _C.load()
    ok = lambda ds, aps=None: lib.lvae_conv2d_wgrad_shared_ok(array(ds), aps, len(ds))
    assert ok(layer(64, 16, 16, 3)) == 1
    assert ok([desc(64, 16, 16, C1=32), desc(64, 16, 32)]) == 0                         # mixed widths
    assert ok([desc(64, 16, 16, C1=32), desc(65, 16, 16)]) == 0                         # mixed batch sizes
    assert ok([desc(64, 16, 16, C1=48), desc(64, 16, 16)]) == 0                         # 48 input channels: not this kernel family
    assert lib.lvae_conv2d_wgrad_variant(ctypes.byref(desc(64, 16, 16, C1=48))) != _C.WGRAD_VARIANT_WINO
    assert ok([desc(64, 16, 16, C1=32), desc(64, 16, 16, Cout=128)]) == 0               # more than one group of output channels
    assert ok([desc(16, 16, 16, C1=32), desc(16, 16, 16)]) == 0                         # below the Winograd family's 16,384 pixels
    assert ok(layer(64, 16, 16, 3) + [desc(64, 16, 16)]) == 0 and ok([]) == 0           # four problems, none
    # a problem whose dy a deferred BatchNorm-backward apply has yet to form (the pair launch's problem A) is not taken
    ap = _C.BnApply()
    for which in range(3):
        aps = (ctypes.c_void_p * 3)()
        assert ok(layer(64, 16, 16, 3), aps) == 1                                       # three null entries: no apply anywhere
        aps[which] = ctypes.addressof(ap)
        assert ok(layer(64, 16, 16, 3), aps) == 0 and schedule(layer(64, 16, 16, 3), aps) is None
    for field in ('x_dtype', 'y_dtype'):
        ds = layer(64, 16, 16, 3)
        setattr(ds[1], field, _C.DT_BF16)
        assert ok(ds) == 0                                                              # bf16 storage
    ds = [desc(64, 16, 16, C1=32, prec=_C.PREC_BF16), desc(64, 16, 16, prec=_C.PREC_BF16)]
    assert ok(ds) == 0 and schedule(ds) is None and lib.lvae_conv2d_wgrad_shared_workspace(array(ds), 2) == 0


def test_one_problem_alone_fills_the_chip_and_the_routing_table_is_what_it_was():
    lib = _C.load()
    d32, d64 = desc(256, 16, 16, C1=32), desc(256, 16, 16)
    # one input-channel block: one workgroup per range, 256 ranges of 4 chunks; two blocks: the single launch's 128 ranges of 8
    assert schedule([d32]) == ((256, 4, 256),) and schedule([d64]) == ((128, 8, 256),)
    assert schedule([desc(64, 16, 16, C1=32)]) == ((64, 4, 64),)          # at the floor the least chunks per range decide
    # a slab is [32][16][64] weights per input-channel block + [64] bias
    assert lib.lvae_conv2d_wgrad_shared_workspace(array([d32]), 1) == 256 * (32 * 16 * 64 + 64) * 4
    # lvae_conv2d_wgrad_f32 and its queries: 32 input channels stay in the tile family, 64 keep their Winograd plan
    assert lib.lvae_conv2d_wgrad_variant(ctypes.byref(d32)) == _C.WGRAD_VARIANT_TILE
    assert lib.lvae_conv2d_wgrad_variant(ctypes.byref(d64)) == _C.WGRAD_VARIANT_WINO
    assert lib.lvae_conv2d_wgrad_workspace(ctypes.byref(d64)) == 128 * (2 * 32 * 16 * 64 + 64) * 4
    assert lib.lvae_conv2d_wgrad_apply_ok(ctypes.byref(d64)) == 1
    assert lib.lvae_conv2d_wgrad_apply_ok(ctypes.byref(d32)) == 0                       # the apply in front is the 64 -> 64 form only
    assert lib.lvae_conv2d_wgrad_pair_ok(ctypes.byref(d32), ctypes.byref(d32)) == 0


def test_the_switch_is_on_by_default():
    from lvae_amd import resblock as RB
    assert RB.Switches({}).wgrad_shared is True
    assert RB.Switches({'LVAE_WGRAD_SHARED': '0'}).wgrad_shared is False


def test_abi_version_is_still_17():
    assert _C.ABI_VERSION == 17 and _C.load().lvae_abi_version() == 17
