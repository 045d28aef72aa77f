"""The spectral regulariser without a GPU: the float64 reference (tests/spectral_ref.py) against torch.nn.utils.spectral_norm and
torch.linalg.svdvals, the table builder on a CPU arena, the trainer's flags and the checkpoint note."""
import argparse
import math

import pytest
import torch
from torch import nn

import spectral_ref as R
from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the reference
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('transposed', [False, True], ids=['conv', 'conv-transposed'])
def test_reference_step_is_torchs_spectral_norm(transposed):
    """One step from the same u: u, v, sigma of torch.nn.utils.spectral_norm(n_power_iterations=1) on a Conv2d / ConvTranspose2d in float64."""
    torch.manual_seed(5)
    conv = (nn.ConvTranspose2d(6, 5, 3) if transposed else nn.Conv2d(6, 5, 3)).double()
    w = conv.weight.detach().clone()
    conv = torch.nn.utils.spectral_norm(conv, n_power_iterations=1)   # dim 1 for the transposed convolution: u has Cout elements
    u0 = R.start_u(5)
    with torch.no_grad():
        conv.weight_u.copy_(u0)
    conv.train()
    conv(torch.zeros(1, 6, 8, 8, dtype=torch.float64))
    r = R.step(w, u0, transposed)
    M = R.out_first(w, transposed).reshape(5, -1)
    sigma_t = torch.dot(conv.weight_u, M @ conv.weight_v)
    torch.testing.assert_close(r['u'], conv.weight_u.detach(), rtol=1e-13, atol=1e-15)
    torch.testing.assert_close(r['v'].reshape(-1), conv.weight_v.detach(), rtol=1e-13, atol=1e-15)
    torch.testing.assert_close(r['sigma'], sigma_t.detach(), rtol=1e-13, atol=0)
    torch.testing.assert_close(conv.weight.detach() * r['sigma'], w, rtol=1e-12, atol=1e-15)
    # and the arena's matrix of the same weight has the same singular values
    torch.testing.assert_close(torch.linalg.svdvals(R.arena_matrix(w, transposed)), torch.linalg.svdvals(M), rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize('shape', R.SHAPES, ids=lambda s: '%dx%d' % s)
def test_reference_chain_reaches_the_largest_singular_value(shape):
    K_, C = shape
    A = R.builder(K_, C)
    sv = torch.linalg.svdvals(A)
    ratio = float(sv[1] / sv[0]) if sv.numel() > 1 else 0.0
    assert ratio <= 0.55, 'the builder no longer separates its first singular value: sigma_2 / sigma_1 = %.3f' % ratio   # a condition
    w = R.logical_weight(A, K_, 1, 1)
    u0 = R.start_u(C)
    r64 = R.steps(w, u0, 20)
    rel = abs(float(r64['sigma']) - float(sv[0])) / float(sv[0])
    r32 = R.steps(w.float(), u0.float(), 20)
    ds = abs(float(r32['sigma']) - float(r64['sigma'])) / float(r64['sigma'])
    du = float((r32['u'].double() - r64['u']).abs().max())
    print('builder %4dx%-3d sigma_2/sigma_1 %.3f | 20 float64 steps: relative error %.2e | float32 chain: sigma %.2e, u %.2e'
          % (K_, C, ratio, rel, ds, du))
    assert rel <= 1e-10
    assert torch.allclose(R.arena_matrix(w), A)   # the builder's matrix is the arena matrix of the weight the chain ran on


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the table builder on a CPU arena
# ---------------------------------------------------------------------------------------------------------------------------------
class _Net(nn.Module):
    def __init__(self):
        import lvae_amd  # noqa: F401
        from lvae_amd.lib.nn import BatchNorm2dParams, Conv2dParams
        super().__init__()
        self.plain = Conv2dParams(3, 8, 3, padding=1)
        self.bn = BatchNorm2dParams(8)
        self.strided = Conv2dParams(8, 6, 3, stride=2, padding=1)
        self.up = Conv2dParams(6, 5, 3, stride=2, padding=1, transposed=True, output_padding=1)
        self.gate = Conv2dParams(5, 10, 1)
        self.frozen = Conv2dParams(4, 4, 3)
        self.frozen.weight.requires_grad_(False)
        self.extra = nn.Parameter(torch.randn(37))


def test_table_lists_every_trainable_convolution_once_and_views_the_permuted_weight():
    import lvae_amd  # noqa: F401
    from lvae_amd.arena import ParamArena
    from lvae_amd.spectral import SpectralReg, conv_matrices
    torch.manual_seed(1)
    net = _Net()
    logical = {k: p.detach().clone() for k, p in net.named_parameters()}
    arena = ParamArena(net, 'cpu')
    rows = conv_matrices(net, arena)
    assert [r[0] for r in rows] == ['plain.weight', 'strided.weight', 'up.weight', 'gate.weight']      # once each, the frozen one left out
    want = {'plain.weight': (27, 8), 'strided.weight': (72, 6), 'up.weight': (54, 5), 'gate.weight': (5, 10)}
    for name, poff, goff, k, c in rows:
        off, n = arena.slots[name]
        assert (k, c) == want[name] and poff == goff == off and k * c == n and off + n <= arena.n_train
        view = arena.params[poff:poff + k * c].view(k, c)
        assert torch.equal(view, R.arena_matrix(logical[name], transposed=name == 'up.weight')), name
    every = conv_matrices(net, arena, trainable_only=False)
    assert [r[0] for r in every][-1] == 'frozen.weight' and every[-1][2] == -1 and every[-1][1] >= arena.n_train
    # the device table and the state's layout
    sr = SpectralReg(0.5, warm_iters=0, seed=9)
    assert sr.build(net, arena) and not sr.build(net, arena)
    t = sr.table.tolist()
    assert [row[:4] for row in t] == [[r[1], r[2], r[3], r[4]] for r in rows]
    assert [row[4] for row in t] == [0, 8, 14, 19] and [row[5] for row in t] == [0, 27, 99, 153]
    assert sr.u.numel() == 29 and sr.v.numel() == 158 and sr.sigma.numel() == 4 and sr.names == [r[0] for r in rows]
    # the seeded start: unit vectors that depend on the seed and the entry's number only
    again = SpectralReg(0.1, warm_iters=3, seed=9)
    again.build(net, arena)
    other = SpectralReg(0.5, seed=10)
    other.build(net, arena)
    assert torch.equal(sr.u, again.u) and not torch.equal(sr.u, other.u)
    for lo, hi in ((0, 8), (8, 14), (14, 19), (19, 29)):
        assert abs(float(sr.u[lo:hi].double().norm()) - 1.0) < 1e-6
    # a moved arena: the table is rebuilt, the iterate is kept
    sr.u.mul_(0.5)
    kept = sr.u.clone()
    arena2 = ParamArena(net, 'cpu')
    assert not sr.build(net, arena2) and torch.equal(sr.u, kept)
    with pytest.raises(ValueError):
        SpectralReg(-1.0)
    with pytest.raises(ValueError):
        SpectralReg(math.nan)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. flags, _check_args, run description
# ---------------------------------------------------------------------------------------------------------------------------------
def _args(*extra):
    import lvae_amd  # noqa: F401
    from lvae_amd.experiment.experiment_manager import build_parser
    return build_parser().parse_args(['--synthetic'] + list(extra))


def test_flags_check_and_run_description():
    import lvae_amd  # noqa: F401
    from lvae_amd.experiment.experiment_manager import LVAEExperiment as E
    a = E._check_args(_args())
    assert a.spectral_reg == 0.0 and a.spectral_warm_iters == 10 and E._make_spectral(a) is None
    assert ',sr' not in E._make_run_description(a)
    a = E._check_args(_args('--spectral-reg', '0.01', '--spectral-warm-iters', '3', '--seed', '7'))
    assert ',sr0.01,seed7' in E._make_run_description(a)
    sr = E._make_spectral(a)
    assert (sr.lam, sr.warm_iters, sr.seed) == (0.01, 3, 7)
    for bad in ('-0.5', 'nan', 'inf'):
        with pytest.raises(SystemExit):
            E._check_args(_args('--spectral-reg', bad))
    with pytest.raises(SystemExit):
        E._check_args(_args('--spectral-reg', '0.1', '--spectral-warm-iters', '-1'))
    # a parsed namespace from before the flags existed still checks and describes
    old = argparse.Namespace(**{k: v for k, v in vars(_args()).items() if not k.startswith('spectral')})
    assert ',sr' not in E._make_run_description(E._check_args(old))


def test_every_rule_offers_the_regulariser():
    import inspect
    import lvae_amd  # noqa: F401
    from lvae_amd import optim
    for rule in (optim.Adamax, optim.Adam, optim.AdamW, optim.ArenaOptimizer):
        assert inspect.signature(rule.__init__).parameters['spectral'].default is None


def test_train_line_suffix():
    import lvae_amd  # noqa: F401
    from lvae_amd.main import spectral_metrics, spectral_suffix
    m = {}
    spectral_metrics({'loss': torch.tensor(1.0)}, m)
    assert m == {} and spectral_suffix(m) == ''
    spectral_metrics({'sr_sum': torch.tensor(12.5), 'sr_max': torch.tensor(3.25)}, m)
    assert m == {'spectral/sum': 12.5, 'spectral/max': 3.25} and spectral_suffix(m) == '   sr: 12.5   max: 3.25'


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the checkpoint note
# ---------------------------------------------------------------------------------------------------------------------------------
class _Opt:
    def __init__(self, spectral):
        self.spectral = spectral


def test_checkpoint_note_round_trip_and_warning(tmp_path):
    import lvae_amd  # noqa: F401
    from lvae_amd.arena import ParamArena
    from lvae_amd.checkpoint import spectral_record, spectral_warning
    from lvae_amd.spectral import SpectralReg
    torch.manual_seed(2)
    net = _Net()
    arena = ParamArena(net, 'cpu')
    sr = SpectralReg(0.25, warm_iters=0, seed=4)
    sr.build(net, arena)
    sr.v.copy_(torch.randn(sr.v.numel()))
    sr.sigma.copy_(torch.rand(4))
    path = str(tmp_path / 'ck.pt')
    torch.save({'model': {}, 'spectral': sr.state_dict()}, path)
    ck = torch.load(path)
    note = spectral_record(ck)
    assert set(note) == {'lam', 'u', 'v', 'sigma', 'shapes'} and note['lam'] == 0.25
    # into a regulariser that has its iterate already, and into one that builds it later: bit for bit
    now, later = SpectralReg(0.25, seed=99), SpectralReg(0.25, seed=99)
    now.build(net, arena)
    assert not torch.equal(now.u, sr.u)
    now.load_state_dict(note)
    later.load_state_dict(note)
    later.build(net, arena)
    later._take_loaded()
    for other in (now, later):
        assert torch.equal(other.state, sr.state) and other.lam == 0.25
    assert spectral_warning(path, ck, _Opt(now)) is None
    # the command line's lambda runs; one line says that the file's was another
    mine = SpectralReg(0.5)
    mine.load_state_dict(note)
    assert mine.lam == 0.5
    line = spectral_warning(path, ck, _Opt(mine))
    assert line == 'warning: %s was written with --spectral-reg 0.25; continuing with 0.5' % path
    # a file without the entry, an optimizer without a regulariser, a bare state_dict
    assert spectral_record({'model': {}}) is None and spectral_warning(path, {'model': {}}, _Opt(mine)) is None
    assert spectral_warning(path, ck, _Opt(None)) is None and spectral_record({'some.weight': torch.zeros(1)}) is None
    # the state of other convolutions is refused
    wrong = dict(note, shapes=[[27, 8], [72, 6], [54, 5], [5, 11]])
    bad = SpectralReg(0.25)
    bad.build(net, arena)
    with pytest.raises(ValueError):
        bad.load_state_dict(wrong)
