"""Gradient accumulation over micro-batches, the parts that need no GPU: the --accum-steps flag and its refusals, the run description, the
checkpoint record, the function that cuts a step's rows into micro-batches, the feed's host arithmetic when a step takes several batches,
and the new entry point of the library with its binding."""
import ctypes
import inspect
import os

import pytest
import torch


def _exp():
    import lvae_amd  # noqa: F401
    from lvae_amd.experiment import experiment_manager as E
    return E


def _parse(*argv):
    return _exp().build_parser().parse_args(list(argv))


def test_parser_accepts_the_flag_and_defaults_to_one_batch_per_step():
    E = _exp()
    print('yardstick | --accum-steps 4 parses to %r, the default to %r' % (_parse('--accum-steps', '4').accum_steps, _parse().accum_steps))
    assert _parse('--accum-steps', '4').accum_steps == 4
    assert _parse().accum_steps == 1
    assert E.LVAEExperiment._check_args(_parse('--accum-steps', '4')).accum_steps == 4
    assert E.LVAEExperiment._check_args(_parse('--accum-steps', '1')).accum_steps == 1


@pytest.mark.parametrize('m', ['0', '-1', '-7'])
def test_check_args_refuses_less_than_one_micro_batch(m):
    E = _exp()
    with pytest.raises(SystemExit) as e:
        E.LVAEExperiment._check_args(_parse('--accum-steps', m))
    print('yardstick | --accum-steps %s is refused with: %s' % (m, e.value))
    assert '--accum-steps' in str(e.value) and m in str(e.value)


def test_run_description_names_the_accumulation():
    E = _exp()
    d = E.LVAEExperiment._make_run_description
    args = ('-d', 'cifar10', '--zdims', '8', '8', '--downsample', '1', '1', '--beta-anneal', '100', '--gated')
    plain = d(E.LVAEExperiment._check_args(_parse(*args)))
    one = d(E.LVAEExperiment._check_args(_parse(*args, '--accum-steps', '1')))
    four = d(E.LVAEExperiment._check_args(_parse(*args, '--accum-steps', '4')))
    both = d(E.LVAEExperiment._check_args(_parse(*args, '--accum-steps', '4', '--iw-train-samples', '2')))
    print('yardstick | run descriptions: plain %r | M = 4 %r | with iw2 %r' % (plain, four, both))
    assert plain == 'cifar10,2ly,2bpl,64ch,gate,block=bacdbacd,b100,elu,drop=0.2,seed54321'   # today's string, spelled out
    assert one == plain and ',acc' not in plain                      # M = 1: the description is today's
    assert four.count(',acc4') == 1 and four.replace(',acc4', '') == plain
    assert ',iw2,acc4,' in both
    ns = E.LVAEExperiment._check_args(_parse(*args))                 # a namespace from before the flag existed still describes itself
    del ns.accum_steps
    assert d(ns) == plain


def test_checkpoint_record_and_its_default():
    import lvae_amd  # noqa: F401
    from lvae_amd import checkpoint as CK
    rec = [CK.accum_steps_record({'model': {}, 'accum_steps': 3}), CK.accum_steps_record({'model': {}, 'global_step': 5}),
           CK.accum_steps_record({'some.weight': torch.zeros(1)})]
    print('yardstick | accum_steps of a file with the key %r, without it %r, of a bare state_dict %r' % tuple(rec))
    assert rec == [3, 1, 1]
    src = inspect.getsource(CK.save_checkpoint)
    assert "ck['accum_steps'] = int(getattr(model, 'accum_steps', 1))" in src   # a model from before the flag writes 1


def test_micro_slices_cuts_equal_parts_in_order():
    import lvae_amd  # noqa: F401
    from lvae_amd.engine import micro_slices
    print('yardstick | micro_slices(12, 3) = %r, (4, 1) = %r, (7, 7) = %r' % (micro_slices(12, 3), micro_slices(4, 1), micro_slices(7, 7)))
    assert micro_slices(12, 3) == [(0, 4), (4, 8), (8, 12)]
    assert micro_slices(4, 1) == [(0, 4)]
    assert micro_slices(7, 7) == [(j, j + 1) for j in range(7)]
    x = torch.arange(24).view(12, 2)
    parts = [x[lo:hi] for lo, hi in micro_slices(x.shape[0], 3)]
    assert torch.equal(torch.cat(parts), x) and all(p.shape == (4, 2) and p.is_contiguous() for p in parts)


@pytest.mark.parametrize('rows,m', [(10, 3), (4, 8), (0, 2), (8, 0), (8, -2)])
def test_micro_slices_refuses_rows_that_do_not_divide(rows, m):
    import lvae_amd  # noqa: F401
    from lvae_amd.engine import micro_slices
    with pytest.raises(ValueError) as e:
        micro_slices(rows, m)
    print('yardstick | micro_slices(%d, %d) is refused with: %s' % (rows, m, e.value))
    assert str(m) in str(e.value)


def _feed(n=40, batch=4):
    import lvae_amd  # noqa: F401
    from lvae_amd.data import DeviceDataset
    imgs = (torch.arange(n, dtype=torch.uint8).view(n, 1, 1, 1) * torch.ones(1, 1, 2, 2, dtype=torch.uint8))
    return DeviceDataset(imgs, batch, seed=11)


def test_feed_arithmetic_when_an_epoch_ends_inside_a_step():
    """N = 40, batch 4: 10 micro-batches per epoch. M = 3: optimizer step 4 takes micro-batches 10, 11, 12, the last of epoch 0 and the first
    two of epoch 1."""
    ds = _feed()
    M = 3
    assert ds.steps_per_epoch == 10 and ds.steps_per_epoch % M != 0
    epochs = {s: [ds.epoch_of((s - 1) * M + j + 1) for j in range(M)] for s in range(1, 8)}
    print('yardstick | epochs of the micro-batches of steps 1..7: %r' % epochs)
    assert epochs[3] == [0, 0, 0] and epochs[4] == [0, 1, 1] and epochs[5] == [1, 1, 1] and epochs[7] == [1, 1, 2]
    assert [ds.step_epoch(s, M) for s in range(1, 8)] == [0, 0, 0, 0, 1, 1, 1]   # of a step's FIRST micro-batch
    for s in range(1, 8):
        want = torch.cat([ds.indices((s - 1) * M + j + 1) for j in range(M)])
        got = ds.step_indices(s, M)
        assert got.shape == (M * 4,) and torch.equal(got, want), s
    four = ds.step_indices(4, M)
    from lvae_amd.data import epoch_permutation
    assert torch.equal(four[:4], epoch_permutation(11, 0, 40)[36:40]) and torch.equal(four[4:], epoch_permutation(11, 1, 40)[:8])
    # one micro-batch per step is what there was
    assert torch.equal(ds.step_indices(7, 1), ds.indices(7)) and ds.step_epoch(11, 1) == ds.epoch_of(11) == 1
    with pytest.raises(ValueError):
        ds.step_indices(0, M)
    with pytest.raises(ValueError):
        ds.step_indices(1, 0)


def test_attach_puts_the_cursor_at_completed_steps_times_m():
    """attach() itself, on host memory: the device-side calls it makes are stood in for (the index upload needs pinned memory)."""
    ds = _feed()
    ds.device = torch.device('cpu')
    loaded = []
    ds._load_index = loaded.append

    class Model:
        global_step = 2

    ds.attach(Model(), 3)
    print('yardstick | cursor after attach at global step 2 with M = 3: %d (index table of epoch %r)' % (int(ds.cursor.item()), loaded))
    assert int(ds.cursor.item()) == 6 and ds.micro == 3 and loaded == [0]
    assert ds.cursor_at(2) == 6 and ds.cursor_at(2, 1) == 2
    Model.global_step = 4                                   # 12 micro-batches done: epoch 1 has begun
    ds.attach(Model(), 3)
    assert int(ds.cursor.item()) == 12 and loaded == [0, 1]
    ds.attach(Model())                                      # the default is one batch per step, as before
    assert int(ds.cursor.item()) == 4 and ds.micro == 1 and loaded == [0, 1, 0]
    with pytest.raises(ValueError):
        ds.attach(Model(), 0)


def test_library_exports_and_binds_micro_fold():
    import lvae_amd  # noqa: F401
    from lvae_amd import _C, kernels
    assert os.path.exists(_C.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_C.LIB_PATH)
    name = 'lvae_micro_fold_f64'
    assert hasattr(lib, name) and name in _C.SIGNATURES
    assert getattr(_C.load(), name).argtypes == _C.SIGNATURES[name][1]
    P, I = ctypes.c_void_p, ctypes.c_int32
    assert _C.SIGNATURES[name][1] == [P] * 8 + [I, I] + [P] * 4
    assert _C.ABI_VERSION == lib.lvae_abi_version()   # an addition keeps the version: a library without it fails at load
    assert hasattr(kernels, 'micro_fold') and kernels.MICRO_FIXED == 7
    from lvae_amd import engine
    assert inspect.signature(engine.TrainStep.__init__).parameters['accum_steps'].default == 1


def test_overlapped_exchange_is_refused_with_more_than_one_micro_batch():
    """The refusal comes before anything is allocated or probed, so a model on the host and a stand-in for the exchange show it."""
    import lvae_amd  # noqa: F401
    from lvae_amd.engine import TrainStep
    from lvae_amd.models.lvae import LadderVAE

    class Exchange:
        world, active, on_gpu, capturable, overlap, mode = 1, True, False, False, True, 'overlap'

    m = LadderVAE(3, [8, 8], blocks_per_layer=1, downsample=[1, 1], merge_type='residual', n_filters=8, dropout=0.2, img_shape=(32, 32),
                  likelihood_form='discr_log_mix', res_block_type='bacdbacd', gated=True, stochastic_skip=True)
    with pytest.raises(ValueError) as e:
        TrainStep(m, None, allreduce=Exchange(), accum_steps=2)
    print('yardstick | accum_steps=2 with the overlapped exchange is refused with: %s' % e.value)
    assert 'LVAE_DDP_MODE' in str(e.value) and 'split' in str(e.value) and 'accum_steps=2' in str(e.value)
    with pytest.raises(ValueError):
        TrainStep(m, None, accum_steps=0)
