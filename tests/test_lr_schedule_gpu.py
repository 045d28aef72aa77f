"""The learning rate computed inside the Adamax kernel from the device step counter: a constant schedule against the unscheduled entry
points (bitwise), a warm-up + cosine schedule against torch.optim.Adamax, the lr the kernel reports against the host function, the
captured step against eager launches, exact resume, and the default path's launches."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from test_ema_gpu import _assert_same_state, _fresh_table, _images, _model, _train_state

pytestmark = pytest.mark.gpu


def _spacing(x):
    return float(np.spacing(np.float32(x)))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_ema', [False, True], ids=['plain', 'ema'])
@pytest.mark.parametrize('case', ['plain', 'mask', 'wd', 'gscale', 'mask+wd+gscale'])
def test_constant_schedule_is_bitwise_the_unscheduled_entry_points(case, with_ema):
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
    ea, eb = ((p0 + 1.0).cuda(), (p0 + 1.0).cuda()) if with_ema else (None, None)
    sa, sb = torch.zeros(1, dtype=torch.int64).cuda(), torch.zeros(1, dtype=torch.int64).cuda()
    sched = K.lr_schedule_struct(2e-3, 'constant', 0, 0, 0.0, 0.1)
    lr_out = torch.zeros(1).cuda()
    for _ in range(5):
        g = torch.randn(n, generator=gen).cuda()
        if with_ema:
            K.adamax_ema_step(pa, g, ma, ua, mask, 2e-3, 0.9, 0.999, 1e-8, wd, gscale, sa, ea, 0.9)
        else:
            K.adamax_step(pa, g, ma, ua, mask, 2e-3, 0.9, 0.999, 1e-8, wd, gscale, sa)
        K.counter_advance(sa)
        K.adamax_sched_step(pb, g, mb, ub, mask, sched, 0.9, 0.999, 1e-8, wd, gscale, sb, eb, 0.9, lr_out)
        K.counter_advance(sb)
    torch.cuda.synchronize()
    assert not torch.equal(pa, p0.cuda())
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(ua, ub)
    if with_ema:
        assert torch.equal(ea, eb) and not torch.equal(ea, (p0 + 1.0).cuda())
    assert lr_out.item() == np.float32(2e-3)


@pytest.mark.parametrize('wd', [0.0, 1e-2])
def test_kernel_follows_the_schedule_against_torch(wd):
    """torch.optim.Adamax on the CPU, its lr set to LrSchedule.at before every step, against the scheduled kernel: warm-up over 3 steps,
    then a cosine that reaches base / 10 four steps later, at the eighth step. Tolerances of test_adamax_weight_decay_matches_torch
    (rtol 2e-6, atol 2e-7). The unscheduled kernel, which runs every step at 2e-3 where this one runs from 6.7e-4 up to 2e-3 and down to
    2e-4, is run beside it and misses the same reference by orders of magnitude."""
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels as K
    from lvae_amd.optim import LrSchedule
    base, steps = 2e-3, 8
    sched = LrSchedule('cosine', warmup_steps=3, decay_steps=4, min_lr=base / 10)
    lrs = [sched.at(base, k) for k in range(steps)]
    assert lrs[2] == np.float32(base) == lrs[3] and lrs[7] == np.float32(base / 10) and max(lrs) / min(lrs) > 9.9
    g = torch.Generator().manual_seed(10)
    n = 4100
    p0, grads = torch.randn(n, generator=g), [torch.randn(n, generator=g) for _ in range(steps)]
    pr = p0.clone().requires_grad_(True)
    opt = torch.optim.Adamax([pr], lr=base, weight_decay=wd)
    pd, m, u = p0.cuda(), torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
    pc, mc, uc = p0.cuda(), torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
    step = torch.zeros(1, dtype=torch.int64, device='cuda')
    st = sched.struct(base)
    for k, gr in enumerate(grads):
        opt.param_groups[0]['lr'] = lrs[k]
        pr.grad = gr.clone()
        opt.step()
        K.adamax_sched_step(pd, gr.cuda(), m, u, None, st, 0.9, 0.999, 1e-8, wd, None, step)
        K.adamax_step(pc, gr.cuda(), mc, uc, None, base, 0.9, 0.999, 1e-8, wd, None, step)
        K.counter_advance(step)
    got, want = pd.cpu(), pr.detach()
    err = (got - want).abs()
    print('scheduled kernel vs torch.optim.Adamax, %d steps, wd %g: max abs error %.3e, max of error / (2e-7 + 2e-6 |ref|) %.3f'
          % (steps, wd, float(err.max()), float((err / (2e-7 + 2e-6 * want.abs())).max())))
    # the comparison sees the schedule: the constant-lr kernel is hundreds of tolerances away from the same reference
    assert float(((pc.cpu() - want).abs() / (2e-7 + 2e-6 * want.abs())).max()) > 100.0
    torch.testing.assert_close(got, want, rtol=2e-6, atol=2e-7)


def test_lr_out_matches_the_host_function():
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels as K
    from lvae_amd.optim import LrSchedule
    n = 4100
    gen = torch.Generator().manual_seed(3)
    lr_out = torch.zeros(1).cuda()
    for sched, base, steps in ((LrSchedule('cosine', 3, 7, 1e-4), 2e-3, 13), (LrSchedule('linear', 0, 5, 0.0), 1e-3, 7),
                               (LrSchedule('step', 2, 3, 1e-5, 0.5), 3e-4, 14), (LrSchedule('exp', 1, 4, 1e-5, 0.3), 3e-4, 16)):
        p, m, u = torch.randn(n, generator=gen).cuda(), torch.zeros(n).cuda(), torch.zeros(n).cuda()
        step = torch.zeros(1, dtype=torch.int64).cuda()
        st = sched.struct(base)
        seen = []
        for k in range(steps):
            K.adamax_sched_step(p, torch.randn(n, generator=gen).cuda(), m, u, None, st, 0.9, 0.999, 1e-8, 0.0, None, step, None, 0.0, lr_out)
            K.counter_advance(step)
            seen.append(lr_out.item())
        for k, got in enumerate(seen):
            want = sched.at(base, k)
            assert abs(got - want) <= _spacing(want), (sched, k, got, want)
        assert len(set(seen)) > 3
    # a counter beyond 2^24 is not rounded on its way into the schedule
    sched = LrSchedule('constant', warmup_steps=2 ** 25)
    p, m, u = torch.randn(8, generator=gen).cuda(), torch.zeros(8).cuda(), torch.zeros(8).cuda()
    p0 = p.clone()
    step = torch.full((1,), 2 ** 24 + 1, dtype=torch.int64).cuda()
    K.adamax_sched_step(p, torch.randn(8, generator=gen).cuda(), m, u, None, sched.struct(3e-4), 0.9, 0.999, 1e-8, 0.0, None, step, None, 0.0,
                        lr_out)
    torch.cuda.synchronize()
    want = float(np.float32(3e-4)) * (2 ** 24 + 2) / 2 ** 25
    assert abs(lr_out.item() - want) <= _spacing(want) and abs(sched.at(3e-4, 2 ** 24 + 1) - want) <= _spacing(want)
    assert bool((p != p0).all())
    # lr_out is optional
    K.adamax_sched_step(p, p0, m, u, None, sched.struct(3e-4), 0.9, 0.999, 1e-8, 0.0, None, step)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the whole step
# ---------------------------------------------------------------------------------------------------------------------------------
W, T = 2, 3
STEPS = W + T + 2
LR = 1e-3
_runs = {}


def _schedule():
    from lvae_amd.optim import LrSchedule
    return LrSchedule('cosine', warmup_steps=W, decay_steps=T, min_lr=LR / 10)


def _xs():
    return [_images(4, 80 + k) for k in range(STEPS)]


def _steps(m, opt, xs, use_graph, names=None):
    """runs the steps; with `names`, also records the name of every C-ABI call the Python passes make (as test_summary_gpu counts them)"""
    from lvae_amd import _C
    from lvae_amd import kernels as K
    from lvae_amd.engine import TrainStep
    real = _C.call

    def counted(name, *args):
        names.append(name)
        return real(name, *args)

    if names is not None:
        _C.call = K.call = counted
    try:
        st = TrainStep(m, opt, use_graph=use_graph)
        outs = [{k: v.detach().clone() for k, v in st(x.cuda()).items()} for x in xs]
        torch.cuda.synchronize()
    finally:
        _C.call = K.call = real
    assert (st.graph_a is not None) == (use_graph and len(xs) > 2)
    return outs


def _run(use_graph, decay, scheduled):
    """STEPS steps of the small model from the same weights, images and noise stream (computed once per combination)."""
    key = (use_graph, decay, scheduled)
    if key not in _runs:
        from lvae_amd.noise import PhiloxNoise
        from lvae_amd.optim import Adamax
        g = load_golden('tiny_cifar')
        _fresh_table()
        m = _model(g.cfg, g.state_dict(), PhiloxNoise(seed=3))
        opt = Adamax(m, lr=LR, ema_decay=decay, schedule=_schedule() if scheduled else None)
        names = []
        outs = _steps(m, opt, _xs(), use_graph, names)
        assert int(opt.step_count.item()) == STEPS
        _runs[key] = {'outs': outs, 'state': _train_state(m, opt), 'ema': None if opt.ema is None else opt.ema.clone(),
                      'lr_now': None if opt.lr_now is None else opt.lr_now.clone(), 'lr': opt.current_lr(), 'calls': names,
                      'sd': opt.state_dict()['schedule']}
    return _runs[key]


@pytest.mark.parametrize('decay', [0.0, 0.99], ids=['plain', 'ema'])
def test_captured_step_equals_eager_and_follows_the_schedule(decay):
    graph, eager, const = _run(True, decay, True), _run(False, decay, True), _run(True, decay, False)
    _assert_same_state(graph['state'], eager['state'])
    assert torch.equal(graph['lr_now'], eager['lr_now']) and graph['lr_now'].dtype == torch.float32
    for a, b in zip(graph['outs'], eager['outs']):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    if decay:
        assert torch.equal(graph['ema'], eager['ema'])
    # the last step ran at the floor of the schedule: the replayed graph did not keep the lr it was captured with
    want = _schedule().at(LR, STEPS - 1)
    assert want == np.float32(LR / 10) and abs(graph['lr'] - want) <= _spacing(want)
    assert graph['sd'] == _schedule().state_dict() and const['sd'] is None and const['lr_now'] is None and const['lr'] == LR
    # and the weights are not those of the constant-lr run (whose first step already differs: lr / 2 against lr)
    assert not torch.equal(graph['state']['params'], const['state']['params'])
    assert torch.equal(graph['outs'][0]['loss'], const['outs'][0]['loss']) and not torch.equal(graph['outs'][-1]['loss'], const['outs'][-1]['loss'])


def test_resume_in_the_middle_of_the_schedule_is_exact(tmp_path):
    from lvae_amd.checkpoint import load_checkpoint, save_checkpoint
    from lvae_amd.models.lvae import LadderVAE
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax
    straight = _run(True, 0.99, True)
    g = load_golden('tiny_cifar')
    xs = _xs()
    _fresh_table()
    m1 = _model(g.cfg, g.state_dict(), PhiloxNoise(seed=3))
    opt1 = Adamax(m1, lr=LR, ema_decay=0.99, schedule=_schedule())
    first = _steps(m1, opt1, xs[:3], True)                 # two eager steps and the capture: in the middle of the decay
    path = str(tmp_path / 'model_3.pt')
    save_checkpoint(path, m1, opt1)
    ck = torch.load(path)
    assert ck['lr_schedule'] == dict(_schedule().state_dict(), base_lr=LR) and ck['optimizer']['step'] == 3
    del m1, opt1

    _fresh_table()
    torch.manual_seed(123)
    m2 = LadderVAE(**g.cfg).cuda().train()                 # other weights and another noise seed: all of it comes from the file
    m2.noise = PhiloxNoise(seed=999)
    opt2 = Adamax(m2, lr=LR, ema_decay=0.99, schedule=_schedule())
    load_checkpoint(path, m2, opt2)
    rest = _steps(m2, opt2, xs[3:], True)
    for a, b in zip(straight['outs'], first + rest):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    _assert_same_state(straight['state'], _train_state(m2, opt2))
    assert torch.equal(opt2.ema, straight['ema']) and torch.equal(opt2.lr_now, straight['lr_now'])

    # a file from before the schedule existed (no 'lr_schedule') loads, into a scheduled and into a plain optimizer
    old = str(tmp_path / 'old_3.pt')
    torch.save({k: v for k, v in ck.items() if k != 'lr_schedule'}, old)
    for opt3 in (Adamax(m2, lr=LR, ema_decay=0.99, schedule=_schedule()), Adamax(m2, lr=LR)):
        assert 'lr_schedule' not in load_checkpoint(old, m2, opt3)
        assert int(opt3.step_count.item()) == 3


def test_default_path_issues_the_launches_it_issued():
    """Without a schedule the step does not reach the new entry point, and with one it issues the same calls in the same order, the
    scheduled Adamax in the place of the plain one: no launch more in either."""
    plain, sched = _run(True, 0.0, False)['calls'], _run(True, 0.0, True)['calls']
    assert 'lvae_adamax_sched_step_f32' not in plain and 'lvae_lr_schedule_at' not in plain
    assert plain.count('lvae_adamax_step_f32') == 3        # the two eager steps and the capture go through Python; replays do not
    assert plain.count('lvae_counter_advance') == sched.count('lvae_counter_advance')
    assert [n.replace('lvae_adamax_sched_step_f32', 'lvae_adamax_step_f32') for n in sched] == plain
    # with the average: the ema entry point as before
    plain_ema, sched_ema = _run(True, 0.99, False)['calls'], _run(True, 0.99, True)['calls']
    assert plain_ema.count('lvae_adamax_ema_step_f32') == 3 and 'lvae_adamax_sched_step_f32' not in plain_ema
    assert [n.replace('lvae_adamax_sched_step_f32', 'lvae_adamax_ema_step_f32') for n in sched_ema] == plain_ema
    assert len(plain_ema) == len(plain)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the trainer
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('window', [False, True], ids=['last-step', 'window-summaries'])
def test_trainer_prints_and_records_the_rate(window, tmp_path, capsys):
    import json
    import re
    from lvae_amd import main as lmain
    from lvae_amd.optim import LrSchedule
    _fresh_table()
    hist, ck = str(tmp_path / 'history.jsonl'), str(tmp_path / 'end.pt')
    argv = ['-d', 'cifar10', '--zdims', '8', '8', '--downsample', '1', '1', '--nfilters', '16', '--skip', '--gated', '--freebits', '1.0',
            '--batch-size', '8', '--synthetic', '--seed', '3', '--steps', '6', '--log-every', '2', '--history', hist, '--save-checkpoint', ck,
            '--lr', '1e-3', '--lr-warmup', '2', '--lr-schedule', 'cosine', '--lr-decay-steps', '3', '--lr-min', '1e-4']
    lmain.main(argv + (['--window-summaries'] if window else []))
    out = capsys.readouterr().out
    sched = LrSchedule('cosine', 2, 3, 1e-4)
    lines = [ln for ln in out.splitlines() if re.search(r'\[step \d+\]', ln)]
    assert len(lines) == 3, out
    for ln, step in zip(lines, (2, 4, 6)):
        # the rate of the step the line falls due at: n = step - 1 completed steps before it
        assert '[step %d]' % step in ln and '   lr: {:.3g}   ['.format(sched.at(1e-3, step - 1)) in ln, ln
        assert ('averaged over' in ln) == window
    recs = [json.loads(r) for r in open(hist)]
    assert [r['step'] for r in recs] == [2, 4, 6]
    for r in recs:
        want = sched.at(1e-3, r['step'] - 1)
        assert abs(r['metrics']['lr/lr'] - want) <= _spacing(want), r
    assert torch.load(ck)['lr_schedule'] == dict(sched.state_dict(), base_lr=1e-3)
    _fresh_table()
