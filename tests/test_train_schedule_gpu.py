"""The trainer's KL warm-up inside the captured step, the test pass with full metrics, and exact resume, on the GPU."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu


def _fresh_table():
    from lvae_amd import kernels as K
    K.prepared.entries.clear()
    K.prepared.table = None


def _model(cfg, sd, noise):
    import lvae_amd  # noqa: F401
    from lvae_amd.models.lvae import LadderVAE
    torch.manual_seed(0)
    m = LadderVAE(**cfg)
    m.load_state_dict(sd)
    m.cuda().train()
    m.noise = noise
    return m


def _images(n, seed):
    return torch.floor(256 * torch.rand(n, 3, 32, 32, generator=torch.Generator().manual_seed(seed))) / 255


def _train_state(m, opt):
    sd = m.state_dict()   # (flushes the host-counted num_batches_tracked)
    bufs = {k: v.detach().clone() for k, v in sd.items() if not k.endswith(('weight', 'bias', 'top_prior_params'))}
    return {'params': m.arena.params.detach().clone(), 'exp_avg': opt.exp_avg.clone(), 'exp_inf': opt.exp_inf.clone(),
            'adamax_step': opt.step_count.clone(), **bufs}


def _assert_same_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _run_steps(m, opt, xs, use_graph=True, beta_anneal=0, between=None):
    from lvae_amd.engine import TrainStep
    st = TrainStep(m, opt, use_graph=use_graph, beta_anneal=beta_anneal)
    outs = []
    for i, x in enumerate(xs):
        outs.append({k: v.detach().clone() for k, v in st(x.cuda()).items()})
        if between is not None:
            between(m.global_step)
    torch.cuda.synchronize()
    return outs, st


def test_annealed_graph_equals_annealed_eager_and_moves_beta():
    from lvae_amd.engine import linear_anneal
    from lvae_amd.noise import FrozenNoise
    from lvae_amd.optim import Adamax
    g = load_golden('tiny_cifar')
    cfg = dict(g.cfg, free_bits=0.0)   # kl_loss is then the reported kl
    noise = FrozenNoise(seed=11)
    x = _images(4, 1)
    res = {}
    for use_graph in (True, False):
        _fresh_table()
        m = _model(cfg, g.state_dict(), noise)
        opt = Adamax(m, lr=1e-3)
        outs, st = _run_steps(m, opt, [x] * 6, use_graph=use_graph, beta_anneal=4)
        assert st.use_graph == use_graph and (st.graph_a is not None) == use_graph
        assert int(m.global_step_dev.item()) == m.global_step == 6
        res[use_graph] = (outs, _train_state(m, opt))
    (og, sg), (oe, se) = res[True], res[False]
    for k, (a, b) in enumerate(zip(og, oe)):
        for key in ('loss', 'elbo', 'recons', 'kl'):
            assert torch.equal(a[key], b[key]), (k, key, float(a[key]), float(b[key]))
        beta = float(linear_anneal(k, 0.0, 1.0, 4))   # step k + 1 runs with k completed steps
        want = float(a['recons']) + beta * float(a['kl'])
        assert abs(float(a['loss']) - want) <= 2e-6 * abs(want) + 1e-6, (k, beta, float(a['loss']), want)
    _assert_same_state(sg, se)
    # the ramp really moved: with identical inputs the loss differs between beta 0, 0.25, 0.5 and beta 1
    assert len({float(o['loss']) for o in og[:5]}) == 5


def test_annealed_step_matches_oracle_at_beta_quarter():
    from oracle import lvae_ref as R
    from lvae_amd.engine import forward_pass
    from lvae_amd.noise import TapeNoise
    g = load_golden('tiny_cifar')
    sd = g.state_dict()
    x = g.t('x')
    tape = R.Tape(gen=torch.Generator().manual_seed(5))
    pkeys = [k for k in sd if R.is_parameter_key(k)]
    for k in pkeys:
        sd[k].requires_grad_(True)
    fp, _ = R.forward_pass(sd, g.cfg, x, tape, beta=0.25, param_keys=pkeys)
    fp['loss'].backward()
    m = _model(g.cfg, g.state_dict(), TapeNoise(tape.entries))
    m.global_step = 1                                       # one completed step of a 4-step ramp: beta 0.25, read on the device
    m.zero_grad()
    out = forward_pass(m, x.cuda(), beta=1.0, beta_anneal=4)
    out['loss'].backward()
    assert m.noise.exhausted()
    for k in ('loss', 'elbo', 'recons', 'kl'):
        a, b = float(out[k]), float(fp[k])
        assert abs(a - b) <= 1e-5 * abs(b), (k, a, b)
    worst = (0.0, None)
    for k, p in m.named_parameters():
        ref = sd[k].grad
        if ref is None or float(ref.norm()) < 1e-5:
            assert p.grad is None or float(p.grad.norm()) < 1e-4, k
            continue
        e = float((p.grad.cpu().double() - ref.double()).norm() / ref.double().norm())
        worst = max(worst, (e, k))
    assert worst[0] < 1e-4, worst


def _oracle_summary(sd, cfg, batches, tape, S):
    from oracle import lvae_ref as R
    L = len(cfg['z_dims'])
    tot = {'iw': 0.0, 'elbo': 0.0, 'recons': 0.0, 'kl': 0.0, 'n': 0, 'layers': [0.0] * L}
    with torch.no_grad():
        for x in batches:
            e, rec, kl, lay = [], [], [], torch.zeros(L, dtype=torch.float64)
            for _ in range(S):
                mo = R.lvae_forward({k: v.clone() for k, v in sd.items()}, cfg, x, tape, training=False)
                e.append((mo['ll'] - mo['kl_sep']).double())
                rec.append(-mo['ll'].double())
                kl.append(mo['kl_sep'].double())
                lay += mo['kl_avg_layerwise'].double() * x.shape[0]
            e = torch.stack(e)
            tot['iw'] += float((torch.logsumexp(e, 0) - math.log(S)).sum())
            tot['elbo'] += float(e.mean(0).sum())
            tot['recons'] += float(torch.stack(rec).mean(0).sum())
            tot['kl'] += float(torch.stack(kl).mean(0).sum())
            tot['layers'] = [a + float(b) / S for a, b in zip(tot['layers'], lay)]
            tot['n'] += x.shape[0]
    n = tot['n']
    out = {'elbo/elbo': tot['elbo'] / n, 'elbo/recons': tot['recons'] / n, 'elbo/kl': tot['kl'] / n}
    for i in range(L):
        out['kl_layers/kl_layer_%d' % i] = tot['layers'][i] / n
    if S > 1:
        out['elbo/elbo_IW_%d' % S] = tot['iw'] / n
    return out


@pytest.mark.parametrize('S', [1, 5])
def test_test_pass_matches_oracle(S):
    from oracle import lvae_ref as R
    from lvae_amd.evaluate import test_pass
    from lvae_amd.noise import TapeNoise
    g = load_golden('tiny_cifar')
    xs = [_images(5, 2), _images(3, 3)]                    # unequal batches, neither a multiple of 32 images
    tape = R.Tape(gen=torch.Generator().manual_seed(7))
    ref = _oracle_summary(g.state_dict(), g.cfg, xs, tape, S)
    m = _model(g.cfg, g.state_dict(), None)
    noise = TapeNoise(tape.entries)
    res = test_pass(m, [x.cuda() for x in xs], S, noise=noise)
    assert noise.exhausted() and m.training and m.noise is None
    assert res.pop('n_images') == 8
    assert set(res) == set(ref), (sorted(res), sorted(ref))
    for k in ref:
        torch.testing.assert_close(torch.tensor(res[k]), torch.tensor(ref[k], dtype=torch.float64).float(), rtol=1e-5, atol=1e-4,
                                   msg=k)


def test_test_pass_graph_equals_eager_and_repeats():
    from lvae_amd.evaluate import test_pass
    from lvae_amd.noise import PhiloxNoise
    g = load_golden('tiny_cifar')
    m = _model(g.cfg, g.state_dict(), PhiloxNoise(1))
    xs = [_images(5, 2).cuda(), _images(3, 3).cuda(), _images(5, 4).cuda()]
    a = PhiloxNoise(seed=21)
    rg = test_pass(m, xs, 6, noise=a)                      # captured per batch shape, replayed
    assert len(m._test_graphs) == 2
    re_ = test_pass(m, xs, 6, noise=PhiloxNoise(seed=21), use_graph=False)
    assert rg == re_, (rg, re_)
    a.step.zero_()                                         # re-seeded: the same pass again, from the captured graphs
    graphs = dict(m._test_graphs)
    assert test_pass(m, xs, 6, noise=a) == rg
    assert all(m._test_graphs[k] is v for k, v in graphs.items()) and len(m._test_graphs) == 2
    r1 = test_pass(m, xs[:1], 1, noise=PhiloxNoise(seed=21), use_graph=False)
    assert set(r1) == {'elbo/elbo', 'elbo/recons', 'elbo/kl', 'kl_layers/kl_layer_0', 'kl_layers/kl_layer_1',
                       'kl_layers/kl_layer_2', 'n_images'}
    assert m.noise.step is None                            # the model's own stream was never drawn from


def test_test_pass_does_not_perturb_training():
    from lvae_amd.evaluate import test_pass
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax
    g = load_golden('tiny_cifar')
    xs = [_images(4, 10 + k) for k in range(6)]
    xt = [_images(5, 30).cuda(), _images(3, 31).cuda()]
    res = {}
    for with_tests in (False, True):
        _fresh_table()
        m = _model(g.cfg, g.state_dict(), PhiloxNoise(seed=3))
        opt = Adamax(m, lr=1e-3)
        seen = []

        def between(step):
            if with_tests and step in (2, 4):
                seen.append(test_pass(m, xt, 1 if step == 2 else 8))

        outs, st = _run_steps(m, opt, xs, use_graph=True, between=between)
        assert st.graph_a is not None
        assert len(seen) == (2 if with_tests else 0)
        res[with_tests] = (outs, _train_state(m, opt), int(m.noise.step.item()))
    (o0, s0, n0), (o1, s1, n1) = res[False], res[True]
    assert n0 == n1 == 6
    for a, b in zip(o0, o1):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    _assert_same_state(s0, s1)


def test_resume_is_exact_in_graph_mode(tmp_path):
    from lvae_amd.checkpoint import load_checkpoint, save_checkpoint
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax
    g = load_golden('tiny_cifar')
    xs = [_images(4, 50 + k) for k in range(6)]
    _fresh_table()
    m = _model(g.cfg, g.state_dict(), PhiloxNoise(seed=3))
    opt = Adamax(m, lr=1e-3)
    straight, _ = _run_steps(m, opt, xs, beta_anneal=4)
    s_straight = _train_state(m, opt)

    _fresh_table()
    m1 = _model(g.cfg, g.state_dict(), PhiloxNoise(seed=3))
    opt1 = Adamax(m1, lr=1e-3)
    first, _ = _run_steps(m1, opt1, xs[:3], beta_anneal=4)
    path = str(tmp_path / 'model_3.pt')
    save_checkpoint(path, m1, opt1)
    ck = torch.load(path)
    assert ck['noise']['step'] == 3 and ck['global_step_dev'] == 3 and ck['global_step'] == 3
    del m1, opt1
    _fresh_table()
    from lvae_amd.models.lvae import LadderVAE
    torch.manual_seed(123)
    m2 = LadderVAE(**g.cfg).cuda().train()                # other weights and another noise seed: all of it comes from the file
    m2.noise = PhiloxNoise(seed=999)
    opt2 = Adamax(m2, lr=1e-3)
    load_checkpoint(path, m2, opt2)
    rest, st = _run_steps(m2, opt2, xs[3:], beta_anneal=4)
    assert st.graph_a is not None
    for a, b in zip(straight, first + rest):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    _assert_same_state(s_straight, _train_state(m2, opt2))
    # a bare reference state_dict still loads
    bare = str(tmp_path / 'bare.pt')
    torch.save(g.state_dict(), bare)
    load_checkpoint(bare, m2)


def test_main_end_to_end(tmp_path):
    ck = tmp_path / 'ck'
    argv = ['-d', 'cifar10', '--zdims', '8', '8', '--downsample', '1', '1', '--nfilters', '16', '--skip', '--gated', '--freebits', '1.0',
            '--batch-size', '8', '--synthetic', '--seed', '3', '--synthetic-test', '64', '--test-batch-size', '24',
            '--ts-log-every', '2', '--ll-every', '4', '--ll-samples', '8', '--checkpoint-every', '2', '--keep-checkpoint-max', '2',
            '--checkpoint-dir', str(ck), '--beta-anneal', '3', '--steps', '8', '--log-every', '4']
    p = subprocess.run([sys.executable, '-m', 'lvae_amd.main'] + argv, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    tests = {int(mt.group(1)): line for line in p.stdout.splitlines() for mt in [re.search(r'\[step (\d+), epoch \d+\]', line)] if mt}
    assert sorted(tests) == [2, 4, 6, 8], p.stdout
    iw = sorted(k for k, line in tests.items() if 'marginal log-likelihood (8)' in line)
    assert iw == [4, 8], p.stdout
    for line in tests.values():
        v = [float(t) for t in re.findall(r'ELBO (\S+)', line)]
        assert v and all(math.isfinite(x) for x in v), line
    assert sorted(os.listdir(ck)) == ['model_6.pt', 'model_8.pt']
    saved = torch.load(str(ck / 'model_8.pt'))
    assert saved['global_step'] == 8 and saved['global_step_dev'] == 8 and saved['noise']['step'] == 8
