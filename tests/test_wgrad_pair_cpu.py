"""How the pair launch of a residual block's two Winograd weight gradients splits the chip (lvae_conv2d_wgrad_pair_schedule): a host-only
query, no GPU. A chunk is 16 Winograd tiles = 64 pixels; range r of a problem takes chunks [r * cpr, min(total, (r + 1) * cpr))."""
import ctypes

import pytest

import lvae_amd  # noqa: F401
from lvae_amd import _C

MIN_CPR = 4   # LVAE_WINO_WGRAD_MIN_CPR of csrc/conv3x3_wgrad_wino.hip: a slab is worth writing from four chunks up


def desc(N, H, W, Cout=64, prec=_C.PREC_F32):
    d = _C.ConvDesc()
    d.x, d.w, d.C1, d.C2 = 1 << 32, 1 << 33, 64, 0   # aligned, never dereferenced
    d.w_stap, d.w_sk, d.w_sn = 64 * Cout, Cout, 1
    d.N, d.H, d.W, d.OH, d.OW, d.Cout = N, H, W, H, W, Cout
    d.KH = d.KW = 3
    d.stride, d.pad, d.gather, d.precision = 1, 1, _C.GATHER_CONV, prec
    return d


def schedule(a, b):
    out = (ctypes.c_int32 * 6)()
    ok = _C.load().lvae_conv2d_wgrad_pair_schedule(ctypes.byref(a), ctypes.byref(b), out)
    return (tuple(out[:3]), tuple(out[3:])) if ok else None


@pytest.mark.parametrize('shape', [(64, 16, 16), (70, 16, 16), (130, 16, 16), (256, 16, 16), (16, 32, 32), (19, 32, 32), (256, 32, 32)])
def test_pair_schedule_covers_every_chunk_once_inside_the_chip(shape):
    N, H, W = shape
    a, b = desc(N, H, W), desc(N, H, W)
    lib = _C.load()
    assert lib.lvae_conv2d_wgrad_pair_ok(ctypes.byref(a), ctypes.byref(b)) == 1
    sa, sb = schedule(a, b)
    total = N * H * W // 64
    assert sa[2] + sb[2] <= 256                       # one workgroup per CU
    for ranges, cpr, wgs in (sa, sb):
        assert ranges >= 1 and wgs == 2 * ranges      # two input-channel blocks per range
        assert (ranges - 1) * cpr < total <= ranges * cpr   # every chunk in exactly one range, no range empty
        assert cpr >= min(MIN_CPR, total)
    assert sa[1] <= sb[1]                             # A's chunks cost more: never the longer ranges
    # the workspace holds both problems' slabs ([2][32][16][64] weights + [64] bias per range), each piece 256-byte aligned
    piece = lambda r: (r * (2 * 32 * 16 * 64 + 64) * 4 + 255) // 256 * 256
    assert lib.lvae_conv2d_wgrad_pair_workspace(ctypes.byref(a), ctypes.byref(b)) == piece(sa[0]) + piece(sb[0])


def test_headline_split_is_the_recorded_one():
    """256x16x16, 1,024 chunks: 74 ranges of 14 chunks for conv1 with the apply in front, 54 of 19 for conv2 (profiles/wgrad_pair_ab.txt)."""
    assert schedule(desc(256, 16, 16), desc(256, 16, 16)) == ((74, 14, 148), (54, 19, 108))


@pytest.mark.parametrize('shape', [(64, 16, 16), (16, 32, 32)])
def test_at_the_least_pixel_count_both_problems_keep_the_single_launch_split(shape):
    """256 chunks, at least four per range: conv1 cannot use more than 64 of its 74 ranges, conv2 gets the rest, and both gradients are summed
    exactly as their single launches sum them (64 ranges of 4 chunks), with the chip full."""
    assert schedule(desc(*shape), desc(*shape)) == ((64, 4, 128), (64, 4, 128))


def test_query_declines_what_is_no_pair():
    ok = lambda a, b: _C.load().lvae_conv2d_wgrad_pair_ok(ctypes.byref(a), ctypes.byref(b))
    assert ok(desc(64, 16, 16), desc(64, 16, 16)) == 1
    assert ok(desc(64, 16, 16), desc(65, 16, 16)) == 0          # different geometries
    assert ok(desc(64, 16, 16), desc(64, 16, 16, Cout=128)) == 0
    assert ok(desc(64, 16, 16, Cout=128), desc(64, 16, 16)) == 0
    assert ok(desc(256, 8, 8), desc(256, 8, 8)) == 0            # no apply in front of the 8x8 level's gradient
    assert ok(desc(16, 16, 16), desc(16, 16, 16)) == 0          # below the Winograd family's 16,384 pixels
    for field in ('x_dtype', 'y_dtype'):
        for which in (0, 1):
            pair = [desc(64, 16, 16), desc(64, 16, 16)]
            setattr(pair[which], field, _C.DT_BF16)
            assert ok(*pair) == 0                               # bf16 storage
    a, b = desc(64, 16, 16, prec=_C.PREC_BF16), desc(64, 16, 16, prec=_C.PREC_BF16)
    assert ok(a, b) == 0 and schedule(a, b) is None
    assert _C.load().lvae_conv2d_wgrad_pair_workspace(ctypes.byref(a), ctypes.byref(b)) == 0


def test_single_gradient_schedules_are_what_they_were():
    """the pair re-splits the ranges only inside its own launch: a gradient alone still gets 128 ranges' worth of workspace"""
    d = desc(256, 16, 16)
    assert _C.load().lvae_conv2d_wgrad_workspace(ctypes.byref(d)) == 128 * (2 * 32 * 16 * 64 + 64) * 4
    assert _C.load().lvae_conv2d_wgrad_apply_ok(ctypes.byref(d)) == 1


def test_the_switch_is_on_by_default_capped_at_16_and_planned_once():
    from lvae_amd import resblock as RB
    d = RB.Switches({})
    assert (d.wgrad_pair, d.wgrad_pair_maxw) == (True, 16)
    s = RB.Switches({'LVAE_WGRAD_PAIR': '0', 'LVAE_WGRAD_PAIR_MAXW': '32'})
    assert (s.wgrad_pair, s.wgrad_pair_maxw) == (False, 32)
    fields = RB.BlockPlan._fields
    assert fields.index('wgrad_pair') == fields.index('wgrad_absorbs_apply') + 1   # decided together, in plan_block


def test_abi_version_is_still_17():
    assert _C.ABI_VERSION == 17 and _C.load().lvae_abi_version() == 17
