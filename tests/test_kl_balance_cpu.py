"""KL balancing without a GPU: the reference's own properties, that the tests' inputs tell a wrong reference from the right one, the fixed
weights of the named rules, validation, the trainer's flag, the run description, the train-line suffix, the checkpoint note."""
import argparse
import math

import pytest
import torch

import kl_balance_ref as R
from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)
from spectral_ref import close_elem


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the reference
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', R.SHAPES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('akind', R.ALPHAS)
def test_coefficients_average_one(shape, kind, akind):
    L, N = shape
    g = R.gamma(R.kl_values(kind, L, N).double(), R.alpha_values(akind, L).double())
    assert bool(torch.isfinite(g).all()) and bool((g > 0).all())
    assert abs(float(g.mean()) - 1.0) <= 1e-12
    if L == 1:
        assert float(g[0]) == 1.0   # exactly


def test_dead_ladder_gets_the_inverse_weights():
    alpha = R.alpha_values('spread', 7).double()
    g = R.gamma(torch.zeros(7, 33, dtype=torch.float64), alpha)
    want = (1 / alpha) / (1 / alpha).mean()
    assert float((g - want).abs().max()) <= 1e-15 * float(want.max())
    assert bool(torch.isfinite(R.gamma(torch.zeros(7, 33, dtype=torch.float64), alpha)).all())
    assert not bool(torch.isfinite(R.gamma(torch.zeros(7, 33, dtype=torch.float64), alpha, floor=0.0)).all())   # what the 0.01 is for


@pytest.mark.parametrize('akind', R.ALPHAS)
def test_a_layer_whose_kl_grows_pays_more_and_the_others_less(akind):
    L, N = 5, 40
    kl, alpha = R.kl_values('random', L, N).double(), R.alpha_values(akind, L).double()
    g0 = R.gamma(kl, alpha)
    for row in range(L):
        up = kl.clone()
        up[row] *= 3.0
        g1 = R.gamma(up, alpha)
        assert float(g1[row]) > float(g0[row])
        assert all(float(g1[j]) < float(g0[j]) for j in range(L) if j != row)


def test_inactive_is_the_plain_bookkeeping_and_gamma_is_detached():
    L, N = 4, 9
    kl, alpha = R.kl_values('random', L, N).double(), R.alpha_values('spread', L).double()
    for fb in R.FREE_BITS:
        off = R.forward(kl, alpha, fb, False)
        assert torch.equal(off['coeff'], torch.ones(L, dtype=torch.float64))
        assert float(off['kl_loss']) == float(R.clamp(kl, fb).mean(dim=1).sum())
        on = R.forward(kl, alpha, fb, True)
        for k in ('kl_sep', 'kl_avg', 'kl'):
            assert torch.equal(on[k], off[k])
        # d kl_loss / d kl = [clamp passes] gamma_l / N: no term from d gamma / d kl
        d = R.backward(kl, alpha, fb, True, g_scal=torch.tensor([1.0, 0.0], dtype=torch.float64))
        passes = torch.ones_like(kl) if fb < 1e-6 else (kl >= fb).double()
        assert torch.allclose(d, passes * on['coeff'][:, None] / N, rtol=1e-14, atol=0)


def test_beta_forms():
    want = {'beta0': True, 'beta0.3': True, 'beta1': False, 'anneal-inside': True, 'anneal-at': False, 'anneal-past': False}
    assert {name: R.active(const, counter) for name, const, counter in R.BETAS} == want
    assert R.beta_of(None, 3) == float(torch.tensor(0.3, dtype=torch.float32)) and R.beta_of(None, 5, anneal_steps=0) == 1.0


@pytest.mark.parametrize('shape', [s for s in R.SHAPES if s[0] > 1], ids=lambda s: '%dx%d' % s)
def test_the_inputs_tell_a_wrong_reference_from_the_right_one(shape):
    """A rule with alpha ignored, and one with the 0.01 left out, must FAIL the element-wise rule on the non-uniform cases: otherwise the
    kernel tests would pass a kernel that made either mistake."""
    L, N = shape
    kl, alpha = R.kl_values('random', L, N), R.alpha_values('spread', L)
    assert float(alpha.max() / alpha.min()) == 4096.0 and float(kl.min()) < 0 < float(kl.max())
    r64, r32 = R.gamma(kl.double(), alpha.double()), R.gamma(kl, alpha)
    close_elem('the right rule in float32 %dx%d' % shape, r32, r64, r32)
    for name, wrong in (('alpha ignored', dict(use_alpha=False)), ('no 0.01', dict(floor=0.0))):
        bad = R.gamma(kl.double(), alpha.double(), **wrong)
        with pytest.raises(AssertionError):
            close_elem('%s %dx%d' % (name, L, N), bad, r64, r32)
        # and through the gradient the blocks receive, with the kernel tests' upstream gradients
        g_sep, g_avg, gs = R.upstream(L, N)
        d64, d32 = R.backward(kl.double(), alpha.double(), 0.0, True, g_sep, g_avg, gs), R.backward(kl, alpha, 0.0, True, g_sep, g_avg, gs)
        with pytest.raises(AssertionError):
            close_elem('dkl, %s %dx%d' % (name, L, N), d64 + (bad - r64)[:, None] * gs[0].double() / N, d64, d32)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the fixed weights
# ---------------------------------------------------------------------------------------------------------------------------------
def test_alpha_tables_of_the_named_configs():
    import lvae_amd  # noqa: F401
    from lvae_amd import configs
    from lvae_amd.balance import RULES, alpha_table, latent_ratios
    # CIFAR-15: four 16x16-relative groups of 4, 4, 4 and 3 layers, bottom first
    r, g = latent_ratios(configs.CIFAR15['downsample'])
    assert r == [8] * 4 + [4] * 4 + [2] * 4 + [1] * 3 and g == [4] * 12 + [3] * 3
    assert alpha_table('equal', configs.CIFAR15['downsample']) == [1.0] * 15
    assert alpha_table('linear', configs.CIFAR15['downsample']) == [8.0] * 4 + [4.0] * 4 + [2.0] * 4 + [1.0] * 3
    assert alpha_table('sqrt', configs.CIFAR15['downsample']) == pytest.approx([math.sqrt(8)] * 4 + [2.0] * 4 + [math.sqrt(2)] * 4 + [1.0] * 3, rel=1e-15)
    # square: r^2 / g = 16, 4, 1, 1/3 -> divided by the minimum
    assert alpha_table('square', configs.CIFAR15['downsample']) == pytest.approx([48.0] * 4 + [12.0] * 4 + [3.0] * 4 + [1.0] * 3, rel=1e-15)
    # BASELINE configs[1]: the 12-layer MNIST model, four groups of three
    r, g = latent_ratios(configs.MNIST12['downsample'])
    assert r == [8] * 3 + [4] * 3 + [2] * 3 + [1] * 3 and g == [3] * 12
    assert alpha_table('square', configs.MNIST12['downsample']) == [64.0] * 3 + [16.0] * 3 + [4.0] * 3 + [1.0] * 3
    assert alpha_table('linear', configs.MNIST12['downsample']) == [8.0] * 3 + [4.0] * 3 + [2.0] * 3 + [1.0] * 3
    assert alpha_table('sqrt', configs.MNIST12['downsample']) == pytest.approx([math.sqrt(8)] * 3 + [2.0] * 3 + [math.sqrt(2)] * 3 + [1.0] * 3, rel=1e-15)
    # without downsampling every layer has the smallest latent: all rules are `equal`
    for rule in RULES:
        assert alpha_table(rule, [0, 0, 0, 0]) == [1.0] * 4
    assert latent_ratios([1, 1, 1]) == ([4, 2, 1], [1, 1, 1])   # the top layer's own downsampling lies below its latent
    with pytest.raises(ValueError):
        alpha_table('cubic', [0, 1])


def _tiny(downsample=(1, 1)):
    import lvae_amd  # noqa: F401
    from lvae_amd.models.lvae import LadderVAE
    return LadderVAE(1, [4] * len(downsample), downsample=list(downsample), merge_type='residual', n_filters=8, dropout=0.1, img_shape=(16, 16),
                     likelihood_form='bernoulli', res_block_type='bacdbacd', gated=True)


def test_attach_validates_and_builds_the_weights():
    import lvae_amd  # noqa: F401
    from lvae_amd.balance import KlBalance
    m = _tiny()
    assert m.kl_balance is None and not any('balance' in k for k in m.state_dict())
    keys = list(m.state_dict())
    kb = KlBalance('square').attach(m)
    assert kb.alpha.tolist() == [4.0, 1.0] and kb.coeff.tolist() == [1.0, 1.0] and kb.record() == 'square'
    assert KlBalance([2, 0.5]).attach(m).alpha.tolist() == [2.0, 0.5] and KlBalance([2, 0.5]).record() == [2.0, 0.5]
    for bad in ([1.0], [1.0, 2.0, 3.0], [1.0, 0.0], [1.0, -2.0], [1.0, float('nan')], [float('inf'), 1.0], [1.0, 1e-60], [1.0, 1e60], [1.0, 'x']):
        with pytest.raises(ValueError):
            KlBalance(bad).attach(m)
    with pytest.raises(ValueError):
        KlBalance('cubic')
    # the beta source: one of the two
    kb.bind(beta=0.3)
    assert kb.beta_source() == {'beta': 0.3, 'step': None, 'anneal_steps': 0}
    counter = torch.zeros(1, dtype=torch.int64)
    kb.bind(step=counter, anneal_steps=7)
    assert kb.beta_source()['step'] is counter and kb.beta_source()['anneal_steps'] == 7
    for kw in (dict(), dict(beta=0.5, step=counter)):
        with pytest.raises(ValueError):
            kb.bind(**kw)
    with pytest.raises(RuntimeError):
        KlBalance('equal').beta_source()   # before attach()
    # the property is no parameter and no buffer
    m.kl_balance = kb
    assert list(m.state_dict()) == keys and not any(p is kb.alpha for p in m.parameters())


def test_the_engine_refuses_the_iw_bound():
    import lvae_amd  # noqa: F401
    from lvae_amd import engine
    from lvae_amd.balance import KlBalance
    m = _tiny()
    with pytest.raises(ValueError, match='importance-weighted'):
        engine.bind_kl_balance(m, KlBalance('equal'), beta=0.5, iw_samples=2)
    assert m.kl_balance is None
    kb = KlBalance('equal')
    engine.bind_kl_balance(m, kb, beta=0.5)
    assert m.kl_balance is kb and kb.beta == 0.5 and kb.step is None


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the trainer's flag
# ---------------------------------------------------------------------------------------------------------------------------------
def _args(*extra):
    import lvae_amd  # noqa: F401
    from lvae_amd.experiment.experiment_manager import build_parser
    return build_parser().parse_args(['--synthetic'] + list(extra))


def test_flag_check_and_run_description(capsys):
    import lvae_amd  # noqa: F401
    from lvae_amd.experiment.experiment_manager import LVAEExperiment as E
    a = E._check_args(_args())
    assert a.kl_balance is None and E._make_kl_balance(a) is None and ',klb' not in E._make_run_description(a)
    a = E._check_args(_args('--kl-balance', 'square', '--beta-anneal', '50', '--seed', '7'))
    assert E._make_run_description(a).endswith(',klb-square,seed7') and ',b50,' in E._make_run_description(a)
    assert E._make_kl_balance(a).record() == 'square'
    for rule in ('equal', 'sqrt', 'linear'):
        assert ',klb-%s,' % rule in E._make_run_description(E._check_args(_args('--kl-balance', rule, '--beta-anneal', '5')))
    # without a warm-up beta is 1 and the flag would do nothing: refused, and the message says so
    with pytest.raises(SystemExit) as e:
        E._check_args(_args('--kl-balance', 'square'))
    assert '--beta-anneal' in str(e.value) and 'beta is 1' in str(e.value) and 'do nothing' in str(e.value)
    with pytest.raises(SystemExit) as e:
        E._check_args(_args('--kl-balance', 'square', '--beta-anneal', '50', '--iw-train-samples', '4'))
    assert '--iw-train-samples' in str(e.value)
    with pytest.raises(SystemExit):
        _args('--kl-balance', 'cubic')   # argparse's choices
    capsys.readouterr()
    # a parsed namespace from before the flag existed still checks and describes
    old = argparse.Namespace(**{k: v for k, v in vars(_args()).items() if k != 'kl_balance'})
    assert ',klb' not in E._make_run_description(E._check_args(old)) and E._make_kl_balance(old) is None


class _Kb:
    def __init__(self, coeff):
        self.coeff = torch.tensor(coeff)


def test_train_line_suffix():
    import lvae_amd  # noqa: F401
    from lvae_amd.main import balance_metrics, balance_suffix
    m = {}
    balance_metrics(None, m)
    assert m == {} and balance_suffix(m, 3, 50) == ''
    balance_metrics(_Kb([0.25, 1.5, 1.25]), m)
    assert m == {'kl_balance/coeff_0': 0.25, 'kl_balance/coeff_1': 1.5, 'kl_balance/coeff_2': 1.25}      # what --history records, no more
    assert balance_suffix(m, 50, 50) == '   klb: 0.25..1.5'   # step 50 ran with beta = 49 / 50
    m = {}
    balance_metrics(_Kb([1.0, 1.0, 1.0]), m)
    assert balance_suffix(m, 51, 50) == '   klb: off'         # step 51 ran with beta = 1
    assert balance_suffix(m, 50, 50) == '   klb: 1..1'        # all 1 while active (one layer, say) is not `off`
    assert m == {'kl_balance/coeff_%d' % i: 1.0 for i in range(3)}


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the checkpoint note
# ---------------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_note_and_resume_warning(tmp_path):
    import lvae_amd  # noqa: F401
    from lvae_amd.balance import KlBalance
    from lvae_amd.checkpoint import kl_balance_record, kl_balance_warning, save_checkpoint
    m = _tiny()
    path = str(tmp_path / 'plain.pt')
    save_checkpoint(path, m)
    ck = torch.load(path)
    assert 'kl_balance' not in ck and kl_balance_record(ck) is None and kl_balance_warning(path, ck, None) is None
    assert kl_balance_warning(path, ck, 'square') == 'warning: %s was written with no KL balancing; continuing with --kl-balance square' % path
    m.kl_balance_record = 'square'                           # what the trainer sets from --kl-balance
    path = str(tmp_path / 'rule.pt')
    save_checkpoint(path, m)
    ck = torch.load(path)
    assert kl_balance_record(ck) == 'square' and kl_balance_warning(path, ck, 'square') is None
    assert kl_balance_warning(path, ck, 'linear') == 'warning: %s was written with --kl-balance square; continuing with --kl-balance linear' % path
    assert kl_balance_warning(path, ck, None) == 'warning: %s was written with --kl-balance square; continuing with no KL balancing' % path
    assert set(ck['model']) == set(m.state_dict())          # the weights' keys do not know about it
    m.kl_balance_record = None
    m.kl_balance = KlBalance([2.0, 0.5])                    # an explicit list, set through the engine: its record is the list
    path = str(tmp_path / 'list.pt')
    save_checkpoint(path, m)
    assert kl_balance_record(torch.load(path)) == [2.0, 0.5]
    assert kl_balance_record({'some.weight': torch.zeros(1)}) is None
