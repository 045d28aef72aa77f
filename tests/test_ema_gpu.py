"""The exponential moving average of the weights kept inside the Adamax kernel: the kernel against the plain Adamax entry point and against
a float64 recurrence, captured against eager, the test pass on the averaged weights, checkpoints and exact resume, and the trainer."""
import math
import os
import re
import subprocess
import sys

import numpy as np
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
    for x in xs:
        outs.append({k: v.detach().clone() for k, v in st(x.cuda()).items()})
        if between is not None:
            between(m.global_step)
    torch.cuda.synchronize()
    return outs, st


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the Adamax update is untouched
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['plain', 'mask', 'wd', 'gscale', 'mask+wd+gscale'])
def test_adamax_update_is_bitwise_the_plain_entry_points(case):
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels as K
    n = 4 * 12347                                          # not a multiple of the grid: the grid-stride loop has a ragged end
    gen = torch.Generator().manual_seed(17)
    p0 = torch.randn(n, generator=gen)
    mask = (torch.rand(n, generator=gen) > 0.3).float().cuda() if 'mask' in case else None
    wd = 1e-2 if 'wd' in case else 0.0
    gscale = torch.tensor([0.5]).cuda() if 'gscale' in case else None
    pa, pb = p0.clone().cuda(), p0.clone().cuda()
    ma, mb, ua, ub = (torch.zeros(n).cuda() for _ in range(4))
    ema0 = (p0 + 1.0).cuda()                               # away from p: a frozen element that moved would show
    ema = ema0.clone()
    sa, sb = torch.zeros(1, dtype=torch.int64).cuda(), torch.zeros(1, dtype=torch.int64).cuda()
    for _ in range(5):
        g = torch.randn(n, generator=gen).cuda()
        K.adamax_step(pa, g, ma, ua, mask, 2e-3, 0.9, 0.999, 1e-8, wd, gscale, sa)
        K.counter_advance(sa)
        K.adamax_ema_step(pb, g, mb, ub, mask, 2e-3, 0.9, 0.999, 1e-8, wd, gscale, sb, ema, 0.9)
        K.counter_advance(sb)
    torch.cuda.synchronize()
    assert not torch.equal(pa, p0.cuda())
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(ua, ub)
    if mask is not None:
        frozen = mask == 0
        assert int(frozen.sum()) > 1000
        assert torch.equal(ema[frozen], ema0[frozen]) and torch.equal(pb[frozen], p0.cuda()[frozen])
        assert bool((ema[~frozen] != ema0[~frozen]).all())
    else:
        assert bool((ema != ema0).all())


def test_swap_exchanges_in_place_with_a_tail():
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels as K
    for n in (4 * 70001, 4 * 513 + 3, 2):
        a0, b0 = torch.randn(n).cuda(), torch.randn(n).cuda()
        a, b = a0.clone(), b0.clone()
        K.swap(a, b)
        assert torch.equal(a, b0) and torch.equal(b, a0)
        K.swap(a, b)
        assert torch.equal(a, a0) and torch.equal(b, b0)
    with pytest.raises(K._C.LvaeHipError):
        K.swap(a0[1:], b0[1:])                             # 4-byte offset: not 16-byte aligned (n = 2 buffers are 512-byte aligned)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the average is right
# ---------------------------------------------------------------------------------------------------------------------------------
def _ema_trajectory(decay, k, n=8192):
    """k steps of the kernel on positive weights that drift steadily -> (fp32 p after every step as float64 rows, the kernel's ema, p0)."""
    from lvae_amd import kernels as K
    gen = torch.Generator().manual_seed(5)
    p0 = 0.5 + torch.rand(n, generator=gen)                                       # [0.5, 1.5): positive, so is every average of them
    g = torch.sign(torch.randn(n, generator=gen)) * (0.5 + torch.rand(n, generator=gen))   # the same gradient every step: a steady drift
    p, g = p0.clone().cuda(), g.cuda()
    m, u = torch.zeros(n).cuda(), torch.zeros(n).cuda()
    ema = p.clone()
    step = torch.zeros(1, dtype=torch.int64).cuda()
    seq = []
    for _ in range(k):
        K.adamax_ema_step(p, g, m, u, None, 1e-2, 0.9, 0.999, 1e-8, 0.0, None, step, ema, decay)   # |p_new - p| <= lr: p stays in [0.1, 1.9]
        K.counter_advance(step)
        seq.append(p.cpu().double())
    return seq, ema.cpu(), p0


def _reference(p0, seq, decay):
    """The recurrence in float64 on the kernel's fp32 p sequence, with the kernel's fp32 constants d and w = fl(1 - d) -> (average, bound).

    Bound, from the arithmetic (u = 2^-24, the relative size of one fp32 rounding to nearest; the library is built without contraction,
    and a fused multiply-add would only drop a rounding): the kernel forms r = fl(p - e), t = fl(r * w), e' = fl(e + t). All p and e here
    are positive and at most M, so |p - e| <= M, |r * w| <= M (w <= 1) and |e + t| <= M up to second-order terms: each of the three
    roundings adds at most u * M, and an error E already in e reaches e' = e * (1 - w) + p * w scaled by 1 - w (= d to within u). Hence
        E_0 = 0,   E_k <= (1 - w_k) * E_{k-1} + 3 * u * M * (1 + 2^-20),
    the last factor covering the second-order terms. Nothing in it comes from what the kernel returns except the p sequence itself."""
    from lvae_amd.optim import ema_decay_at
    u = 2.0 ** -24
    e = p0.double().clone()
    M = max(float(p0.abs().max()), max(float(p.abs().max()) for p in seq))
    E = 0.0
    for n, p in enumerate(seq):
        d = ema_decay_at(decay, n)
        w = float(np.float32(1.0) - d)
        e = e + (p - e) * w
        E = (1.0 - w) * E + 3.0 * u * M * (1.0 + 2.0 ** -20)
    return e, E


def test_average_matches_float64_recurrence_within_rounding():
    from lvae_amd.optim import ema_decay_at
    decay, k = 0.75, 40
    assert float(ema_decay_at(decay, 25)) < decay == float(ema_decay_at(decay, 26))   # the ramp reaches `decay` inside the run
    seq, ema, p0 = _ema_trajectory(decay, k)
    assert float(seq[-1].min()) > 0.0 and float((seq[-1] - p0.double()).abs().min()) > 0.05   # the weights really drifted
    ref, bound = _reference(p0, seq, decay)
    err = float((ema.double() - ref).abs().max())
    print('ema vs float64 recurrence: max abs error %.3e, bound %.3e' % (err, bound))
    assert err <= bound, (err, bound)
    # the bound discriminates: the same comparison against a recurrence whose decay is off by 1e-3 falls outside it
    for other in (decay + 1e-3, decay - 1e-3):
        ref2, bound2 = _reference(p0, seq, other)
        err2 = float((ema.double() - ref2).abs().max())
        print('against decay %.4f: max abs error %.3e, bound %.3e' % (other, err2, bound2))
        assert err2 > bound2, (other, err2, bound2)


def test_decay_zero_makes_the_average_a_copy():
    # d = 0, w = 1: e' = fl(e + fl(p - e)). e is the previous p (by induction) and a step moves p by at most lr = 0.01 while p >= 0.1, so
    # p / 2 <= e <= 2 p: the difference is exact (Sterbenz) and the sum is p itself.
    seq, ema, p0 = _ema_trajectory(0.0, 7)
    assert torch.equal(ema.double(), seq[-1]) and not torch.equal(ema, p0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. captured equals eager, and averaging never alters the trajectory
# ---------------------------------------------------------------------------------------------------------------------------------
def test_captured_average_equals_eager_and_training_is_unchanged():
    from lvae_amd.noise import FrozenNoise
    from lvae_amd.optim import Adamax
    g = load_golden('tiny_cifar')
    noise = FrozenNoise(seed=11)
    xs = [_images(4, 60 + k) for k in range(6)]
    res = {}
    for tag, use_graph, decay in (('graph', True, 0.99), ('eager', False, 0.99), ('off', True, 0.0)):
        _fresh_table()
        m = _model(g.cfg, g.state_dict(), noise)
        opt = Adamax(m, lr=1e-3, ema_decay=decay)
        outs, st = _run_steps(m, opt, xs, use_graph=use_graph)
        assert (st.graph_a is not None) == use_graph and int(opt.step_count.item()) == 6
        assert (opt.ema is None) == (decay == 0.0) and ('ema' in opt.state_dict()) == (decay > 0.0)
        res[tag] = (outs, _train_state(m, opt), None if opt.ema is None else opt.ema.clone(), m.arena.n_train)
    n_train = res['graph'][3]
    ema_g, ema_e = res['graph'][2], res['eager'][2]
    assert ema_g.numel() == n_train and ema_g.dtype == torch.float32
    assert torch.equal(ema_g, ema_e)
    params = res['graph'][1]['params'][:n_train]
    moved = params != _model(g.cfg, g.state_dict(), None).pack().params[:n_train]
    assert int(moved.sum()) > n_train // 4
    assert bool((ema_g[moved] != params[moved]).any())     # an average, not a copy of the last iterate
    for tag in ('graph', 'eager'):
        _assert_same_state(res[tag][1], res['off'][1])
        for a, b in zip(res[tag][0], res['off'][0]):
            for k in a:
                assert torch.equal(a[k], b[k]), (tag, k)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the test pass uses the average and disturbs nothing
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('use_graph', [True, False])
def test_test_pass_uses_the_average_and_leaves_training_alone(use_graph):
    from lvae_amd.checkpoint import ema_state_dict_reference_layout, state_dict_reference_layout
    from lvae_amd.evaluate import test_pass
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax
    g = load_golden('tiny_cifar')
    xs = [_images(4, 10 + k) for k in range(6)]
    xt = [_images(5, 30).cuda(), _images(3, 31).cuda()]
    S = 4
    res = {}
    for with_tests in (False, True):
        _fresh_table()
        m = _model(g.cfg, g.state_dict(), PhiloxNoise(seed=3))
        opt = Adamax(m, lr=1e-3, ema_decay=0.9)
        tnoise = PhiloxNoise(seed=21)
        seen, avg_sd, raw_sd, graphs = {}, {}, {}, []

        def between(step):
            if step not in (2, 4):
                return
            avg_sd[step] = ema_state_dict_reference_layout(m, opt)   # (both runs take the snapshots; only one runs the passes)
            raw_sd[step] = state_dict_reference_layout(m)
            if not with_tests:
                return
            before, ema_before = m.arena.params.clone(), opt.ema.clone()
            if tnoise.step is not None:
                tnoise.step.zero_()                                   # every pass draws the same noise: only the weights differ
            seen[step] = test_pass(m, xt, S, noise=tnoise, optimizer=opt, use_graph=use_graph)
            torch.cuda.synchronize()
            assert torch.equal(m.arena.params, before) and torch.equal(opt.ema, ema_before)
            assert m.training and m.noise is not tnoise
            if use_graph:
                graphs.append(dict(m._test_graphs))

        outs, st = _run_steps(m, opt, xs, use_graph=True, between=between)
        assert st.graph_a is not None
        res[with_tests] = (outs, _train_state(m, opt), opt.ema.clone(), int(m.noise.step.item()))
        if with_tests:
            if use_graph:   # one captured plan per batch shape, made by the first pass and replayed by the second
                assert len(graphs[0]) == 2 and graphs[1].keys() == graphs[0].keys()
                assert all(graphs[1][k] is v for k, v in graphs[0].items())
            assert seen[2] != seen[4]
            for step in (2, 4):
                assert seen[step].pop('weights') == 'ema'
                m2 = _model(g.cfg, avg_sd[step], PhiloxNoise(1))
                want = test_pass(m2, xt, S, noise=PhiloxNoise(seed=21), use_graph=use_graph)
                assert 'weights' not in want
                assert seen[step] == want, (step, seen[step], want)   # bitwise: every total is the same double
                m3 = _model(g.cfg, raw_sd[step], PhiloxNoise(1))
                raw = test_pass(m3, xt, S, noise=PhiloxNoise(seed=21), use_graph=use_graph)
                assert raw['n_images'] == want['n_images'] == 8
                assert raw['elbo/elbo'] != want['elbo/elbo'] and raw['elbo/recons'] != want['elbo/recons']
                del m2, m3
    (o0, s0, e0, n0), (o1, s1, e1, n1) = res[False], res[True]
    assert n0 == n1 == 6
    for a, b in zip(o0, o1):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    _assert_same_state(s0, s1)
    assert torch.equal(e0, e1)


def test_test_pass_without_an_average_is_the_plain_pass():
    from lvae_amd.evaluate import test_pass
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax
    g = load_golden('tiny_cifar')
    m = _model(g.cfg, g.state_dict(), PhiloxNoise(1))
    opt = Adamax(m, lr=1e-3)
    xt = [_images(5, 30).cuda()]
    a = test_pass(m, xt, 2, noise=PhiloxNoise(seed=21), optimizer=opt, use_graph=False)
    b = test_pass(m, xt, 2, noise=PhiloxNoise(seed=21), use_graph=False)
    assert a == b and 'weights' not in a
    with pytest.raises(RuntimeError):
        with opt.swap_ema():
            pass


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. checkpoints
# ---------------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_carries_the_average_and_resume_is_exact(tmp_path):
    from lvae_amd import evaluate
    from lvae_amd.checkpoint import load_checkpoint, load_ema_weights, save_checkpoint
    from lvae_amd.models.lvae import LadderVAE
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax
    g = load_golden('tiny_cifar')
    xs = [_images(4, 50 + k) for k in range(6)]
    _fresh_table()
    m = _model(g.cfg, g.state_dict(), PhiloxNoise(seed=3))
    opt = Adamax(m, lr=1e-3, ema_decay=0.99)
    straight, _ = _run_steps(m, opt, xs, beta_anneal=4)
    s_straight, ema_straight = _train_state(m, opt), opt.ema.clone()

    _fresh_table()
    m1 = _model(g.cfg, g.state_dict(), PhiloxNoise(seed=3))
    opt1 = Adamax(m1, lr=1e-3, ema_decay=0.99)
    first, _ = _run_steps(m1, opt1, xs[:3], beta_anneal=4)
    path = str(tmp_path / 'model_3.pt')
    save_checkpoint(path, m1, opt1)
    ck = torch.load(path)
    # a complete state dict in the layout of ck['model']: same keys, shapes, contiguous CPU tensors; parameters averaged, buffers as they are
    assert list(ck['ema']) == list(ck['model']) and ck['ema_decay'] == 0.99
    trainable = {k for k, p in m1.named_parameters() if p.requires_grad}
    differ = 0
    for k, v in ck['model'].items():
        e = ck['ema'][k]
        assert e.shape == v.shape and e.dtype == v.dtype and e.is_contiguous() and e.device.type == 'cpu', k
        if k in trainable:
            differ += int(not torch.equal(e, v))
        else:
            assert torch.equal(e, v), k
    assert differ > len(trainable) // 2
    n_train1 = m1.arena.n_train
    ema1, params1 = opt1.ema.clone(), m1.arena.params.clone()
    del m1, opt1

    _fresh_table()
    torch.manual_seed(123)
    m2 = LadderVAE(**g.cfg).cuda().train()                # other weights and another noise seed: all of it comes from the file
    m2.noise = PhiloxNoise(seed=999)
    opt2 = Adamax(m2, lr=1e-3, ema_decay=0.99)
    opt2._state()                                         # (the average exists already, seeded from the other weights)
    load_checkpoint(path, m2, opt2)
    assert torch.equal(opt2.ema, ema1) and torch.equal(m2.arena.params, params1)
    rest, st = _run_steps(m2, opt2, xs[3:], beta_anneal=4)
    assert st.graph_a is not None
    for a, b in zip(straight, first + rest):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    _assert_same_state(s_straight, _train_state(m2, opt2))
    assert torch.equal(opt2.ema, ema_straight)

    # the averaged weights of the file as a model: what `evaluate --ema` loads
    m3 = LadderVAE(**g.cfg).cuda()
    load_ema_weights(path, m3)
    assert torch.equal(m3.pack().params[:n_train1], ema1) and m3.global_step == 3
    assert torch.equal(m3.pack().params[n_train1:], params1[n_train1:])

    # an old-style file: no 'ema'. It loads, and an averaging optimizer starts its average from the loaded weights
    old = str(tmp_path / 'old_3.pt')
    torch.save({k: v for k, v in ck.items() if k not in ('ema', 'ema_decay', 'test_noise')}, old)
    m4 = LadderVAE(**g.cfg).cuda().train()
    m4.noise = PhiloxNoise(seed=999)
    opt4 = Adamax(m4, lr=1e-3, ema_decay=0.99)
    opt4._state()
    load_checkpoint(old, m4, opt4)
    assert torch.equal(m4.arena.params, params1) and torch.equal(opt4.ema, params1[:n_train1])
    opt5 = Adamax(m4, lr=1e-3)                             # and into a plain optimizer as before
    load_checkpoint(old, m4, opt5)
    assert opt5.ema is None and int(opt5.step_count.item()) == 3
    bare = str(tmp_path / 'bare.pt')
    torch.save(g.state_dict(), bare)
    load_checkpoint(bare, m4, opt4)
    assert torch.equal(opt4.ema, m4.arena.params[:n_train1])
    # evaluate --ema refuses files without averaged weights, by name
    for bad in (old, bare):
        with pytest.raises(ValueError, match='no averaged weights'):
            load_ema_weights(bad, m3)
        with pytest.raises(SystemExit, match='no averaged weights'):
            evaluate.main(_TINY_ARGV + ['--checkpoint', bad, '--ema', '--ll'])
    with pytest.raises(SystemExit, match='--checkpoint'):
        evaluate.main(_TINY_ARGV + ['--ema', '--ll'])


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. end to end
# ---------------------------------------------------------------------------------------------------------------------------------
_TINY_ARGV = ['-d', 'cifar10', '--zdims', '8', '8', '--downsample', '1', '1', '--nfilters', '16', '--skip', '--gated', '--freebits', '1.0',
              '--batch-size', '8', '--synthetic', '--seed', '3']


def _lines(stdout):
    """{step: [log lines of that step, throughput removed]} of a trainer run."""
    out = {}
    for line in stdout.splitlines():
        mt = re.search(r'\[step (\d+)[,\]]', line)
        if mt:
            out.setdefault(int(mt.group(1)), []).append(re.sub(r'\s*\[\d+ img/s\]', '', line))
    return out


def test_main_end_to_end_with_average_and_resume(tmp_path):
    ck = tmp_path / 'ck'
    argv = _TINY_ARGV + ['--synthetic-test', '64', '--test-batch-size', '24', '--ts-log-every', '6', '--ll-every', '12', '--ll-samples', '4',
                         '--checkpoint-every', '12', '--keep-checkpoint-max', '3', '--checkpoint-dir', str(ck), '--beta-anneal', '5',
                         '--steps', '24', '--log-every', '6', '--ema-decay', '0.99']
    p = subprocess.run([sys.executable, '-m', 'lvae_amd.main'] + argv, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    full = _lines(p.stdout)
    assert sorted(full) == [6, 12, 18, 24], p.stdout
    for step, lines in full.items():
        tests = [ln for ln in lines if 'epoch' in ln]
        assert len(tests) == 1 and len(lines) == 2, lines
        assert '[averaged weights]' in tests[0], tests[0]
        assert ('marginal log-likelihood (4)' in tests[0]) == (step % 12 == 0), tests[0]
        v = [float(t) for t in re.findall(r'ELBO:? (\S+)', ' '.join(lines))]
        assert len(v) == 2 and all(math.isfinite(x) for x in v), lines
    assert sorted(os.listdir(ck)) == ['model_12.pt', 'model_24.pt']
    saved = torch.load(str(ck / 'model_12.pt'))
    assert saved['global_step'] == 12 and list(saved['ema']) == list(saved['model']) and saved['ema_decay'] == 0.99
    assert any(not torch.equal(saved['ema'][k], saved['model'][k]) for k in saved['model'])

    # resumed from step 12, the run prints the remaining lines again, character for character (throughput aside)
    ck2 = tmp_path / 'ck2'
    argv2 = [a if a != str(ck) else str(ck2) for a in argv] + ['--resume', str(ck / 'model_12.pt')]
    p2 = subprocess.run([sys.executable, '-m', 'lvae_amd.main'] + argv2, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p2.returncode == 0, p2.stdout[-3000:] + p2.stderr[-3000:]
    rest = _lines(p2.stdout)
    assert sorted(rest) == [18, 24], p2.stdout
    for step in (18, 24):
        assert rest[step] == full[step], (step, rest[step], full[step])
    a, b = torch.load(str(ck / 'model_24.pt')), torch.load(str(ck2 / 'model_24.pt'))
    for k in a['ema']:
        assert torch.equal(a['ema'][k], b['ema'][k]) and torch.equal(a['model'][k], b['model'][k]), k

    # the stored average evaluates offline, and the line says which weights it used
    ev = _TINY_ARGV + ['--checkpoint', str(ck / 'model_24.pt'), '--ema', '--ll', '--ll-samples', '4', '--n-test', '32', '--test-batch-size', '16']
    p3 = subprocess.run([sys.executable, '-m', 'lvae_amd.evaluate'] + ev, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p3.returncode == 0, p3.stdout[-3000:] + p3.stderr[-3000:]
    assert '[averaged weights]' in p3.stdout and 'marginal log-likelihood (4)' in p3.stdout, p3.stdout
