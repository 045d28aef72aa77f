"""Host side of the two-workgroups-per-tile form of the whole-image plain launches (lvae_rb_ext.nsplit): the plan's decision is a
host-only query, the switch defaults to "the library decides", and the three plain launches of a block hand the switch on."""
import ctypes as C
import inspect


def ask(N, H, epi=0, force=0, precision=0):
    import lvae_amd  # noqa: F401
    from lvae_amd import _C
    d = _C.ConvDesc()
    d.N, d.H, d.W, d.OH, d.OW, d.C1, d.Cout = N, H, H, H, H, 64, 64
    d.KH, d.KW, d.stride, d.pad, d.precision = 3, 3, 1, 1, precision
    e = _C.RbExt()
    e.epilogue, e.nsplit = epi, force
    lib = _C.load()
    return int(lib.lvae_resblock_conv_nsplit(C.byref(d), C.byref(e))), int(lib.lvae_resblock_conv_rows(C.byref(d)))


def test_plan_splits_32_pixel_plain_tiles_while_the_doubled_grid_fits():
    from lvae_amd import _C
    assert ask(256, 4) == (2, 128) and ask(256, 2) == (2, 32) and ask(1, 2) == (2, 1)   # rows stay tiles
    assert ask(258, 4) == (1, 129) and ask(258, 4, force=2) == (2, 129)
    assert ask(512, 4) == (1, 256) and ask(600, 4, force=2) == (1, 150)                 # 64-pixel tiles never split
    assert ask(256, 8) == (1, 256) and ask(256, 8, force=2) == (1, 256)
    assert ask(256, 4, epi=_C.RB_EPI_GATE, force=2) == (1, 128) and ask(256, 4, force=1) == (1, 128)
    assert ask(256, 4, precision=_C.PREC_BF16, force=2) == (1, 128)
    assert ask(256, 16) == (0, 0)
    lib = _C.load()
    assert lib.lvae_resblock_conv_nsplit(None, None) == 0


def test_switch_defaults_to_the_plan_and_reaches_the_three_plain_launches():
    from lvae_amd import kernels as K, ops, resblock as RB
    assert RB.Switches({}).rb_nsplit == 0 and RB.Switches({'LVAE_RB_NSPLIT': '1'}).rb_nsplit == 1
    for fn in (K.rb_conv, K.rb_gate_dgrad, K.rb_apply_dgrad):
        assert inspect.signature(fn).parameters['nsplit'].default == 0
    assert inspect.getsource(ops).count('nsplit=RB.switches.rb_nsplit') == 3
