"""Posteriors parameterised relative to the prior, the parts that need no GPU: the reference formula of the residual core against
torch.distributions, the inputs on which it and the absolute formula part ways, the --residual-posterior flag, the run description, the
checkpoint note and the refusal to load weights under the other setting."""
import os
import re

import pytest
import torch

import residual_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exp():
    import lvae_amd  # noqa: F401
    from lvae_amd.experiment import experiment_manager as E
    return E


def _parse(*argv):
    return _exp().build_parser().parse_args(list(argv))


@pytest.mark.parametrize('bcast', [False, True], ids=['p-per-image', 'p-broadcast'])
def test_helper_in_float64_is_torch_distributions(bcast):
    """float64 helper == kl_divergence(Normal(mu_p + dmu, ...), Normal(mu_p, ...)) and the two log_probs, to 1e-12 relative."""
    from torch.distributions import Normal, kl_divergence
    N, H, W, Z = 3, 4, 5, 6
    g = torch.Generator().manual_seed(11)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    p = torch.cat((r(1 if bcast else N, H, W, Z), 1.5 * r(1 if bcast else N, H, W, Z)), -1)
    d = torch.cat((r(N, H, W, Z), 0.7 * r(N, H, W, Z)), -1)
    eps, zf = r(N, H, W, Z), 1.5 * r(N, H, W, Z)
    pd = Normal(p[..., :Z], (p[..., Z:] / 2).exp())
    qd = Normal(p[..., :Z] + d[..., :Z], ((p[..., Z:] + d[..., Z:]) / 2).exp())
    worst = 0.0
    for mode in (0, 1, 2):
        z = qd.mean + qd.stddev * eps if mode == 0 else qd.mean if mode == 1 else zf
        want = {'z': z, 'lp_e': pd.log_prob(z), 'lq_e': qd.log_prob(z), 'kan_e': kl_divergence(qd, pd), 'q': p + d}
        for analytical in (False, True):
            o = RR.residual_core(p, d, zf if mode == 2 else eps, mode, analytical, Z, N)
            want['kl_e'] = want['kan_e'] if analytical else want['lq_e'] - want['lp_e']
            for k, w in want.items():
                w = w.expand_as(o[k])
                # relative to the element, with the magnitude of the terms a difference is formed from as the floor for kl_e = lq - lp
                scale = w.abs() if k != 'kl_e' else want['lq_e'].abs() + want['lp_e'].abs()
                err = float(((o[k] - w).abs() / scale.clamp(min=1e-300)).max())
                worst = max(worst, err)
                assert err <= 1e-12, (mode, analytical, k, err)
            assert torch.equal(o['ks'], o['kan_e'].sum(-1)) and o['lp'].shape == (N,)
    print('yardstick | helper (float64) against torch.distributions: largest relative error %.3e (bound 1e-12)' % worst)


def test_discriminating_inputs_separate_the_residual_from_the_absolute_formula():
    """A condition, not a measurement: on |mu_p| >> sigma_p the float32 residual formula is inside the element-wise rule by construction,
    while the absolute float32 formula fed fl32(p + d) is outside it at more than half of the elements and of the per-pixel sums. It keeps
    the GPU test from passing an implementation that adds before the kernel."""
    N, HW, Z = 3, 80, 32
    p, d, eps = RR.discriminating_inputs(N, HW, Z)
    r64 = RR.residual_core(p.double(), d.double(), eps.double(), 0, True, Z, N)
    r32 = RR.residual_core(p, d, eps, 0, True, Z, N)
    q32 = p + d   # fl32(p + d): what a torch add in front of the absolute kernel hands it
    ab32 = RR.absolute_kl(q32, p, Z)
    ab64 = RR.absolute_kl(q32.double(), p.double(), Z)   # the absolute formula itself in float64, on the rounded sum
    be, bs = RR.elem_bound(r64['kan_e'], r32['kan_e']), RR.elem_bound(r64['ks'], r32['ks'])
    assert bool(((r32['kan_e'].double() - r64['kan_e']).abs() <= be).all()) and bool(((r32['ks'].double() - r64['ks']).abs() <= bs).all())
    out = {}
    for name, ab in (('float32', ab32.double()), ('float64', ab64)):
        out[name] = (float(((ab - r64['kan_e']).abs() > be).double().mean()), float(((ab.sum(-1) - r64['ks']).abs() > bs).double().mean()),
                     float((ab - r64['kan_e']).abs().max()))
    print('yardstick | residual float32: max error %.3e (median element %.3f) | absolute on fl32(p + d): float32 max error %.3e, outside the '
          'rule at %.1f %% of elements and %.1f %% of per-pixel sums; evaluated in float64 %.1f %% and %.1f %%'
          % (float((r32['kan_e'].double() - r64['kan_e']).abs().max()), float(r64['kan_e'].median()), out['float32'][2],
             100 * out['float32'][0], 100 * out['float32'][1], 100 * out['float64'][0], 100 * out['float64'][1]))
    assert out['float32'][0] > 0.5 and out['float32'][1] > 0.5
    assert out['float64'][0] > 0.5 and out['float64'][1] > 0.5   # the offset is lost in the rounding of mu_q, not in the formula


def test_parser_flag_and_run_description():
    E = _exp()
    assert _parse().residual_posterior is False and _parse('--residual-posterior').residual_posterior is True
    d = E.LVAEExperiment._make_run_description
    args = ('-d', 'cifar10', '--zdims', '8', '8', '--downsample', '1', '1', '--beta-anneal', '100', '--gated')
    plain = d(E.LVAEExperiment._check_args(_parse(*args)))
    res = d(E.LVAEExperiment._check_args(_parse(*args, '--residual-posterior')))
    both = d(E.LVAEExperiment._check_args(_parse(*args, '--residual-posterior', '--accum-steps', '4', '--iw-train-samples', '2')))
    print('yardstick | run descriptions: plain %r | residual %r | with iw2 and acc4 %r' % (plain, res, both))
    assert plain == 'cifar10,2ly,2bpl,64ch,gate,block=bacdbacd,b100,elu,drop=0.2,seed54321'   # today's string, spelled out
    assert res.count(',resq') == 1 and res.replace(',resq', '') == plain
    assert ',iw2,acc4,resq,' in both
    ns = E.LVAEExperiment._check_args(_parse(*args))   # a namespace from before the flag existed still describes itself
    del ns.residual_posterior
    assert d(ns) == plain


def _tiny_model():
    import lvae_amd  # noqa: F401
    from lvae_amd.models.lvae import LadderVAE
    torch.manual_seed(0)
    return LadderVAE(1, [4, 4], blocks_per_layer=1, downsample=[1, 1], merge_type='residual', n_filters=8, dropout=0.1, img_shape=(16, 16),
                     likelihood_form='bernoulli', res_block_type='bacdbacd', gated=True)


def test_property_reaches_every_layer_and_adds_no_parameter():
    m = _tiny_model()
    keys = list(m.state_dict())
    assert m.residual_posterior is False and all(not l.stochastic.residual_posterior for l in m.top_down_layers)
    m.residual_posterior = True
    assert m.residual_posterior is True and all(l.stochastic.residual_posterior for l in m.top_down_layers)   # the top layer included
    assert list(m.state_dict()) == keys
    m.residual_posterior = False
    assert m.residual_posterior is False


def test_checkpoint_note_default_and_refused_mismatch(tmp_path):
    from lvae_amd import checkpoint as CK
    rec = [CK.residual_posterior_record({'model': {}, 'residual_posterior': True}), CK.residual_posterior_record({'model': {}, 'global_step': 5}),
           CK.residual_posterior_record({'some.weight': torch.zeros(1)})]
    assert rec == [True, False, False]   # a file without the note, and a bare state_dict, are absolute
    m = _tiny_model()
    m.residual_posterior = True
    res_file, abs_file, old_file = (str(tmp_path / n) for n in ('res.pt', 'abs.pt', 'old.pt'))
    CK.save_checkpoint(res_file, m)
    assert torch.load(res_file)['residual_posterior'] is True
    a = _tiny_model()
    CK.save_checkpoint(abs_file, a)
    assert torch.load(abs_file)['residual_posterior'] is False
    old = torch.load(abs_file)
    del old['residual_posterior']
    torch.save(old, old_file)
    before = {k: v.clone() for k, v in a.state_dict().items()}
    for path, model in ((res_file, a), (abs_file, m), (old_file, m)):
        with pytest.raises(ValueError) as e:
            CK.load_checkpoint(path, model)
        print('yardstick | refused: %s' % e.value)
        assert 'residual' in str(e.value) and 'absolute' in str(e.value)   # names both settings
    assert all(torch.equal(v, a.state_dict()[k]) for k, v in before.items())   # refused before anything was loaded
    CK.load_checkpoint(res_file, m)   # matching settings load
    CK.load_checkpoint(abs_file, a)
    CK.load_checkpoint(old_file, a)   # a file without the note loads as absolute


def test_library_exports_and_binds_the_residual_core():
    import ctypes
    import lvae_amd  # noqa: F401
    from lvae_amd import _C, kernels, ops
    lib = ctypes.CDLL(_C.LIB_PATH)
    hdr = open(os.path.join(ROOT, 'include', 'lvae_hip.h')).read()
    for name in ('lvae_normal_stochastic_res_fwd_f32', 'lvae_normal_stochastic_res_bwd_f32'):
        assert hasattr(lib, name) and name in _C.SIGNATURES and re.search(r'\b%s\s*\(' % name, hdr)
    assert len(_C.SIGNATURES['lvae_normal_stochastic_res_fwd_f32'][1]) == 16 and len(_C.SIGNATURES['lvae_normal_stochastic_res_bwd_f32'][1]) == 18
    assert hasattr(kernels, 'normal_stochastic_res_fwd') and hasattr(kernels, 'normal_stochastic_res_bwd') and hasattr(ops, 'NormalStochResFn')
    assert 'stochastic_residual.hip' in open(os.path.join(ROOT, 'ladder-vae-pytorch_amd', 'csrc', 'Makefile')).read()
