"""BatchNorm recalibration without a GPU: the C surface, the command lines' refusals and the helper that picks the training batches."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT


def test_symbols_bindings_and_abi_numbers():
    import lvae_amd  # noqa: F401
    from lvae_amd import _C, kernels as K
    hdr = open(os.path.join(ROOT, 'include', 'lvae_hip.h')).read()
    P, I = _C._P, _C._I
    assert _C.SIGNATURES['lvae_bn_recal_fold_f64'] == (_C.C.c_int, [P, I, P, P])
    assert _C.SIGNATURES['lvae_bn_recal_finish_f32'] == (_C.C.c_int, [P, I, P, P, P])
    for name in ('lvae_bn_recal_fold_f64', 'lvae_bn_recal_finish_f32'):
        assert re.search(r'\bint %s\(' % name, hdr), name
        assert getattr(_C.load(), name).argtypes == _C.SIGNATURES[name][1]
    body = hdr[hdr.index('typedef struct lvae_bn_recal_entry {'):hdr.index('} lvae_bn_recal_entry;')]
    assert re.findall(r'(\w+);', body) == [f[0] for f in _C.BnRecalEntry._fields_] == ['stat', 'acc', 'n']
    assert _C.C.sizeof(_C.BnRecalEntry) == _C.C.sizeof(_C.CopyEntry) == 24   # the table is an int64 [entries][3], like copy_table's
    # an addition: the number stays, a library without the symbols fails at load
    assert int(re.search(r'#define LVAE_ABI_VERSION (\d+)', hdr).group(1)) == _C.ABI_VERSION == _C.load().lvae_abi_version()
    for name in ('bn_recal_table', 'bn_recal_fold', 'bn_recal_finish'):
        assert callable(getattr(K, name))
    assert 'bn_recal.hip' in open(os.path.join(ROOT, 'ladder-vae-pytorch_amd', 'csrc', 'Makefile')).read()
    with pytest.raises(_C.LvaeHipError):   # host memory is refused: there is no CPU path
        K.bn_recal_table([(torch.zeros(4), torch.zeros(4, dtype=torch.float64))], 'cpu')


def test_trainer_refuses_bn_batches_without_an_average():
    from lvae_amd.experiment.experiment_manager import LVAEExperiment as X, build_parser
    p = build_parser()
    assert p.parse_args([]).ema_bn_batches == 0   # off by default
    with pytest.raises(SystemExit, match='--ema-decay'):
        X._check_args(p.parse_args(['--ema-bn-batches', '4']))
    with pytest.raises(SystemExit, match='--ema-decay'):
        X._check_args(p.parse_args(['--ema-bn-batches', '4', '--ema-decay', '0']))
    with pytest.raises(SystemExit, match='negative'):
        X._check_args(p.parse_args(['--ema-bn-batches', '-1', '--ema-decay', '0.9']))
    args = X._check_args(p.parse_args(['--ema-bn-batches', '4', '--ema-decay', '0.9']))
    assert args.ema_bn_batches == 4
    X._check_args(p.parse_args(['--ema-decay', '0.9']))   # the average without the flag: as before


def test_evaluator_refusals(capsys):
    from lvae_amd.evaluate import parse_eval_args
    with pytest.raises(SystemExit):   # no training split
        parse_eval_args(['--synthetic', '--recalibrate-bn', 'data'])
    assert 'training split' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse_eval_args(['--synthetic', '--recalibrate-bn', 'prior', '--recalibrate-batches', '0'])
    with pytest.raises(SystemExit):   # one temperature for the prior source
        parse_eval_args(['--synthetic', '--recalibrate-bn', 'prior', '--temperature', '0.5', '0.6', '0.7'])
    with pytest.raises(SystemExit):
        parse_eval_args(['--synthetic', '--recalibrate-bn', 'posterior'])
    a = parse_eval_args(['--synthetic', '--recalibrate-bn', 'prior', '--temperature', '0.7', '--ps'])
    assert (a.recalibrate_bn, a.recalibrate_batches, a.temperature) == ('prior', 20, [0.7])
    a = parse_eval_args(['--data-npz', 'x.npz', '--recalibrate-bn', 'data', '--recalibrate-batches', '5'])
    assert (a.recalibrate_bn, a.recalibrate_batches) == ('data', 5)
    assert parse_eval_args(['--synthetic', '--ps']).recalibrate_bn is None


def test_test_line_names_the_recalibration():
    from lvae_amd.experiment.experiment_manager import LVAEExperiment as X
    m = {'elbo/elbo': -1.0, 'elbo/recons': 2.0, 'elbo/kl': 3.0}
    plain = X.test_log_str(dict(m, weights='ema'), 7, 0)
    line = X.test_log_str(dict(m, weights='ema', **{'bn_recal/rounds': 4}), 7, 0)
    assert '[averaged weights]   [BatchNorm recalibrated on 4 batches]   ELBO' in line
    assert 'recalibrated' not in plain and line.replace('[BatchNorm recalibrated on 4 batches]   ', '') == plain


def test_first_batches_float_set():
    from lvae_amd.data import first_batches
    x = torch.rand(11, 3, 4, 5, generator=torch.Generator().manual_seed(1))
    b = first_batches(x, 2, 4)
    assert len(b) == 2 and all(t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (4, 3, 4, 5) for t in b)
    assert torch.equal(torch.cat(b), x[:8])                      # the first N * B rows, stored order
    assert torch.equal(torch.cat(first_batches(x.double(), 1, 4)), x[:4])
    b = first_batches(x, 5, 4)                                   # N * B = 20 > 11: stops at the last whole batch
    assert len(b) == 2 and torch.equal(torch.cat(b), x[:8])
    assert len(first_batches(x, 1, 11)) == 1
    with pytest.raises(ValueError, match='do not fill one batch'):
        first_batches(x, 3, 12)
    with pytest.raises(ValueError):
        first_batches(x, 0, 4)


def test_first_batches_uint8_sets():
    from lvae_amd.data import first_batches
    rng = np.random.default_rng(2)
    u = torch.from_numpy(rng.integers(0, 256, size=(7, 3, 4, 4), dtype=np.uint8))
    b = first_batches(u, 2, 3)
    assert len(b) == 2 and b[0].dtype == torch.float32
    assert torch.equal(torch.cat(b), u[:6].float().div(255.0))   # a byte means v / 255, the gather's rule
    nhwc = u.permute(0, 2, 3, 1).contiguous()                    # CelebA's storage
    c = first_batches(nhwc, 2, 3, channels_last=True)
    assert all(torch.equal(p, q) and q.is_contiguous() for p, q in zip(b, c))
    assert len(first_batches(nhwc, 9, 3, channels_last=True)) == 2
    with pytest.raises(ValueError, match='do not fill one batch'):
        first_batches(nhwc, 1, 8, channels_last=True)
