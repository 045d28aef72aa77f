"""Host side of the fused stochastic block (csrc/stoch_img.hip): what lvae_stoch_block_ok accepts and declines, asked without a GPU (the
query reads the descriptor only; the pointers below are not memory), and the binding of the new entry points."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def _C():
    import lvae_amd  # noqa: F401
    from lvae_amd import _C
    return _C


def conv(_C, N, H, W, cin, cout, w=0x10000, x=0x200000, y=0x300000):
    d = _C.ConvDesc()
    d.x, d.y, d.w, d.bias = x, y, w, 0x400000
    d.C1, d.Cout, d.N, d.H, d.W, d.OH, d.OW = cin, cout, N, H, W, H, W
    d.KH, d.KW, d.stride, d.pad, d.gather = 3, 3, 1, 1, _C.GATHER_CONV
    d.w_stap, d.w_sk, d.w_sn = cin * cout, cout, 1
    return d


def block(_C, N, H, W, cin=64, Z=32, top=False, mode=0):
    b = _C.StochBlock()
    if top:
        b.p_given, b.p_bcast = 0x500000, 1
    else:
        b.conv_p = conv(_C, N, H, W, cin, 2 * Z)
    b.conv_q = conv(_C, N, H, W, cin, 2 * Z, w=0x20000)
    b.conv_out = conv(_C, N, H, W, Z, cin, w=0x30000)
    b.mode, b.eps = mode, 0x600000
    return b


def ok(_C, b):
    return int(_C.load().lvae_stoch_block_ok(ctypes.byref(b)))


def test_accepts_whole_image_levels(_C):
    for N, H, W in ((1, 8, 8), (3, 8, 8), (256, 8, 8), (5, 4, 4), (256, 4, 4), (9, 2, 2), (256, 2, 2), (2, 4, 8), (3, 2, 4), (1, 1, 1), (256, 1, 1)):
        for top in (False, True):
            for mode in (0, 1, 2):
                assert ok(_C, block(_C, N, H, W, top=top, mode=mode)) == 1, (N, H, W, top, mode)


def test_declines_each_single_violation(_C):
    N, H, W = 4, 8, 8
    assert ok(_C, block(_C, N, H, W)) == 1
    assert ok(_C, block(_C, N, 8, 16)) == 0          # H*W = 128
    assert ok(_C, block(_C, N, 16, 16)) == 0
    assert ok(_C, block(_C, N, 3, 3)) == 0           # 9 does not divide 64
    assert ok(_C, block(_C, N, H, W, Z=16)) == 0
    assert ok(_C, block(_C, N, H, W, cin=32)) == 0
    for name in ('conv_p', 'conv_q', 'conv_out'):    # an unaligned weight view
        b = block(_C, N, H, W)
        getattr(b, name).w += 4
        assert ok(_C, b) == 0, name
    b = block(_C, N, H, W)
    b.conv_q = _C.ConvDesc()                          # q absent
    assert ok(_C, b) == 0
    for mode in (-1, 3):
        assert ok(_C, block(_C, N, H, W, mode=mode)) == 0
    b = block(_C, N, H, W, top=True)
    b.p_given = 0                                     # neither conv_in_p nor a given p_params
    assert ok(_C, b) == 0
    for field, value in (('stride', 2), ('pad', 0), ('KH', 1), ('gather', 1), ('x_dtype', 1), ('y_dtype', 1)):
        b = block(_C, N, H, W)
        setattr(b.conv_q, field, value)
        assert ok(_C, b) == 0, field
    b = block(_C, N, H, W)
    b.conv_q.x += 4                                   # an unaligned operand
    assert ok(_C, b) == 0
    b = block(_C, N, H, W)
    b.eps += 8
    assert ok(_C, b) == 0
    assert int(_C.load().lvae_stoch_block_ok(None)) == 0


def bwd_block(_C, N, H, W, cin=64, Z=32, top=False, mode=0):
    def dgrad(cout, cin_, w):   # the dgrad view of a cin_ -> cout convolution
        d = conv(_C, N, H, W, cout, cin_, w=w)
        d.gather, d.w_sk, d.w_sn = _C.GATHER_TRANSPOSED, 1, cout
        return d
    b = _C.StochBlockBwd()
    b.dgrad_out, b.dgrad_q = dgrad(cin, Z, 0x30000), dgrad(2 * Z, cin, 0x20000)
    if top:
        b.dgrad_p.x, b.p_bcast = 0x700000, 1
    else:
        b.dgrad_p = dgrad(2 * Z, cin, 0x10000)
    b.p, b.q, b.z, b.eps, b.mode = 0x500000, 0x510000, 0x520000, 0x600000, mode
    return b


def test_backward_query_follows_the_forward(_C):
    ok_b = lambda b: int(_C.load().lvae_stoch_block_bwd_ok(ctypes.byref(b)))
    for N, H, W in ((1, 8, 8), (256, 8, 8), (5, 4, 4), (256, 2, 2), (2, 4, 8), (1, 1, 1)):
        for top in (False, True):
            assert ok_b(bwd_block(_C, N, H, W, top=top)) == 1, (N, H, W, top)
    assert ok_b(bwd_block(_C, 4, 8, 16)) == 0 and ok_b(bwd_block(_C, 4, 8, 8, Z=16)) == 0 and ok_b(bwd_block(_C, 4, 8, 8, cin=32)) == 0
    assert ok_b(bwd_block(_C, 4, 8, 8, mode=3)) == 0
    b = bwd_block(_C, 4, 8, 8)
    b.dgrad_q.w += 4
    assert ok_b(b) == 0
    b = bwd_block(_C, 4, 8, 8)
    b.dgrad_q.gather = _C.GATHER_CONV   # a forward descriptor is not a dgrad
    assert ok_b(b) == 0
    b = bwd_block(_C, 4, 8, 8)
    b.z += 4
    assert ok_b(b) == 0
    assert int(_C.load().lvae_stoch_block_bwd_ok(None)) == 0
    assert _C.load().lvae_stoch_block_bwd_f32(ctypes.byref(bwd_block(_C, 4, 16, 16)), None) != 0


def test_weight_scratch_and_launch_errors(_C):
    lib = _C.load()
    d = conv(_C, 4, 8, 8, 64, 64)
    full = lib.lvae_stoch_block_workspace(ctypes.byref(d))
    assert full == 9 * 3 * 64 * 64 * 2                # nine taps, three bf16 piece planes of a 64 x 64 tile
    assert lib.lvae_stoch_block_workspace(ctypes.byref(conv(_C, 4, 8, 8, 32, 64))) == full   # the reduction dimension is padded to 64
    assert lib.lvae_stoch_block_workspace(ctypes.byref(conv(_C, 4, 8, 8, 128, 64))) == 0
    entry = (ctypes.c_char * lib.lvae_conv2d_prepare_entry_bytes())()
    assert lib.lvae_stoch_block_prepare_entry(ctypes.byref(d), ctypes.cast(entry, ctypes.c_void_p)) != 0   # no scratch attached
    # a declined descriptor is an error of the launch, before anything is dereferenced
    assert lib.lvae_stoch_block_fwd_f32(ctypes.byref(block(_C, 4, 16, 16)), None) != 0
    assert b'lvae_stoch_block_ok' in lib.lvae_last_error()


def test_abi_and_bindings(_C):
    hdr = open(os.path.join(ROOT, 'include', 'lvae_hip.h')).read()
    assert int(re.search(r'#define LVAE_ABI_VERSION (\d+)', hdr).group(1)) == _C.ABI_VERSION == 17 == _C.load().lvae_abi_version()
    for name in ('lvae_stoch_block_ok', 'lvae_stoch_block_workspace', 'lvae_stoch_block_prepare_entry', 'lvae_stoch_block_fwd_f32',
                 'lvae_stoch_block_bwd_ok', 'lvae_stoch_block_bwd_f32'):
        assert name in _C.SIGNATURES and name in hdr, name
        assert getattr(_C.load(), name).argtypes == _C.SIGNATURES[name][1]
    # the mirror has the header's fields in the header's order
    for struct, mirror in (('lvae_stoch_block', _C.StochBlock), ('lvae_stoch_block_bwd', _C.StochBlockBwd)):
        body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (struct, struct), hdr, re.S).group(1)
        names = [n for decl in body.split(';') for n in re.findall(r'\*?\s*(\w+)\s*(?:,|$)', decl.split('/*')[0].strip())]
        assert names == [f[0] for f in mirror._fields_], struct
