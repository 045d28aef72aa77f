"""Training on the K-sample importance-weighted bound, the parts that need no GPU: the --iw-train-samples flag and its refusals, the run
description, and the new entry points of the library and their bindings."""
import ctypes
import os

import pytest

NEW_SYMBOLS = ['lvae_iw_loss_fwd_f32', 'lvae_iw_loss_bwd_f32', 'lvae_iw_loss_fwd_anneal_f32', 'lvae_iw_loss_bwd_anneal_f32',
               'lvae_repeat_samples_fwd_f32', 'lvae_repeat_samples_bwd_f32']


def _exp():
    import lvae_amd  # noqa: F401
    from lvae_amd.experiment import experiment_manager as E
    return E


def _parse(*argv):
    return _exp().build_parser().parse_args(list(argv))


def test_parser_accepts_the_flag_and_defaults_to_the_elbo():
    assert _parse('--iw-train-samples', '4').iw_train_samples == 4
    assert _parse().iw_train_samples == 1
    E = _exp()
    assert E.LVAEExperiment._check_args(_parse('--iw-train-samples', '4')).iw_train_samples == 4


@pytest.mark.parametrize('argv,names', [
    (('--iw-train-samples', '0'), ('--iw-train-samples',)),
    (('--iw-train-samples', '-3'), ('--iw-train-samples',)),
    (('--iw-train-samples', '4', '--freebits', '1.0'), ('--iw-train-samples', '--freebits')),
    (('--iw-train-samples', '4', '--analytical-kl'), ('--iw-train-samples', '--analytical-kl')),
])
def test_check_args_rejects_what_makes_the_bound_meaningless(argv, names):
    E = _exp()
    with pytest.raises(SystemExit) as e:
        E.LVAEExperiment._check_args(_parse(*argv))
    for name in names:   # the message names the flags
        assert name in str(e.value), str(e.value)


def test_free_bits_and_analytical_kl_stay_legal_with_one_sample():
    E = _exp()
    E.LVAEExperiment._check_args(_parse('--freebits', '1.0', '--analytical-kl'))
    E.LVAEExperiment._check_args(_parse('--iw-train-samples', '1', '--freebits', '1.0', '--analytical-kl'))


def test_run_description_names_the_objective():
    E = _exp()
    d = E.LVAEExperiment._make_run_description
    args = ('-d', 'cifar10', '--zdims', '8', '8', '--downsample', '1', '1', '--beta-anneal', '100', '--gated')
    plain = d(E.LVAEExperiment._check_args(_parse(*args)))
    one = d(E.LVAEExperiment._check_args(_parse(*args, '--iw-train-samples', '1')))
    four = d(E.LVAEExperiment._check_args(_parse(*args, '--iw-train-samples', '4')))
    assert four.count(',iw4') == 1
    assert ',iw' not in plain and one == plain                       # K = 1: the description is today's
    assert four.replace(',iw4', '') == plain                          # ... and K = 4 adds exactly that
    # today's string, spelled out
    assert plain == 'cifar10,2ly,2bpl,64ch,gate,block=bacdbacd,b100,elu,drop=0.2,seed54321'
    # a namespace from before the flag existed still describes itself
    ns = E.LVAEExperiment._check_args(_parse(*args))
    del ns.iw_train_samples
    assert d(ns) == plain


def test_library_exports_and_binds_the_new_entry_points():
    import lvae_amd  # noqa: F401
    from lvae_amd import _C
    assert os.path.exists(_C.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_C.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _C.SIGNATURES, name
        assert getattr(_C.load(), name).argtypes == _C.SIGNATURES[name][1]
    # the two forms of beta: a float argument, or a device counter (pointer) plus the ramp length (int64)
    assert _C.SIGNATURES['lvae_iw_loss_fwd_f32'][1][2] is ctypes.c_float
    assert _C.SIGNATURES['lvae_iw_loss_fwd_anneal_f32'][1][2:4] == [ctypes.c_void_p, ctypes.c_int64]
    assert _C.ABI_VERSION == lib.lvae_abi_version()   # additions keep the version: a library without them fails at load


def test_glue_and_wrappers_exist():
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels, ops
    import inspect
    from lvae_amd import engine
    from lvae_amd.models.lvae import LadderVAE
    for name in ('IwLossFn', 'IwLossAnnealFn', 'RepeatSamplesFn'):
        assert hasattr(ops, name), name
    for name in ('iw_loss_fwd', 'iw_loss_bwd', 'iw_loss_fwd_anneal', 'iw_loss_bwd_anneal', 'repeat_samples', 'repeat_samples_bwd'):
        assert hasattr(kernels, name), name
    assert inspect.signature(LadderVAE.forward).parameters['n_samples'].default == 1
    assert inspect.signature(engine.forward_pass).parameters['iw_samples'].default == 1
    assert inspect.signature(engine.TrainStep.__init__).parameters['iw_samples'].default == 1


def test_mask_plan_keeps_one_group_for_one_sample_and_two_for_more():
    """The Dropout2d masks of a forward are drawn in one launch per shape: (B, C) for every block at K = 1, as before; with K > 1 the
    bottom-up blocks' at (B, C), then the top-down blocks' at (K * B, C)."""
    import lvae_amd  # noqa: F401
    from lvae_amd.models.lvae import LadderVAE
    m = LadderVAE(3, [8, 8, 8], blocks_per_layer=2, downsample=[0, 1, 1], merge_type='residual', n_filters=8, dropout=0.2, img_shape=(32, 32),
                  likelihood_form='discr_log_mix', res_block_type='bacdbacd', gated=True, stochastic_skip=True)
    m.train()
    one = m._mask_plan(4)
    assert isinstance(one, tuple) and one == m._mask_plan(4, 1) and one[1:] == (4, 8, 0.2)
    bu, td = m._mask_plan(4, 3)
    assert bu[1:] == (4, 8, 0.2) and td[1:] == (12, 8, 0.2)
    assert bu[0] + td[0] == one[0]
    assert bu[0] == 2 * (1 + 3 * 2)                       # stem block + 3 levels of 2 blocks, two masks each
    m.eval()
    assert m._mask_plan(4, 3) is None
