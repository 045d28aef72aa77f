"""The windowed training log on the device: the fold / take kernels against a float64 statement, non-finite steps, refusals, the fold inside
the training step (eager, captured, split form), window semantics, checkpoints and the trainer's --window-summaries / --history."""
import json
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

WORKER = os.path.join(ROOT, 'tests', 'summary_worker.py')
SCALARS = ('loss', 'elbo', 'recons', 'kl', 'l2')


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


def _fold_row(K, row, L, acc, grad=True, gscale=None):
    """row: device float32 [6 + L] = loss, elbo, recons, kl, l2, grad_norm, kl_layers."""
    K.summary_fold(row[0:1], row[1:2], row[2:3], row[3:4], row[4:5], row[6:6 + L], acc, grad_norm=row[5:6] if grad else None, gscale=gscale)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the kernels against a float64 statement
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', [0, 1, 3, 20, 64])
def test_fold_is_the_sequential_float64_sum_of_the_float32_values(L):
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels as K
    gen = torch.Generator().manual_seed(100 + L)
    half = torch.full((1,), 0.5, device='cuda')
    for case in ('no grad_norm', 'grad_norm', 'grad_norm * 0.5'):
        acc = torch.zeros(8 + L, dtype=torch.float64, device='cuda')
        out = torch.full((8 + L,), -1.0, dtype=torch.float64, device='cuda')
        for window in range(2):                           # the second window starts clean
            vals = torch.randn(37, 6 + L, generator=gen) * 10.0 ** torch.randint(-3, 4, (37, 6 + L), generator=gen).float()
            dev = vals.cuda()
            for k in range(37):
                _fold_row(K, dev[k], L, acc, grad=case != 'no grad_norm', gscale=half if case.endswith('0.5') else None)
            K.summary_take(acc, out)
            torch.cuda.synchronize()
            want = [37.0, 0.0]
            for i in range(6 + L):
                s = 0.0
                for k in range(37):
                    v = vals[k, i]
                    if i == 5:
                        v = torch.zeros(()) if case == 'no grad_norm' else v * torch.tensor(0.5) if case.endswith('0.5') else v
                    s += float(v)                          # float32 -> Python float widens exactly
                want.append(s)
            got = out.cpu().tolist()
            assert got == want, (case, window, [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b])
            assert torch.equal(acc, torch.zeros_like(acc))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. non-finite values (fed as inputs)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_nonfinite_steps_are_skipped_and_counted():
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels as K
    L = 3
    nan, inf = math.nan, math.inf
    #        loss elbo recons kl   l2   grad  kl_0 kl_1 kl_2
    rows = [[1.5, -1.0, 2.0, 0.5, 3.0, 4.0, 0.1, 0.2, 0.3],
            [nan, -2.0, 2.5, 0.5, 3.0, 4.0, 0.1, 0.2, 0.3],     # skipped
            [inf, -2.0, 2.5, 0.5, 3.0, 4.0, 0.1, 0.2, 0.3],     # skipped
            [2.5, -2.0, 2.5, 0.5, 3.0, inf, 0.1, 0.2, 0.3],     # finite loss, infinite gradient norm: skipped
            [3.5, -3.0, 1.0, 0.25, 3.0, 5.0, 0.4, nan, 0.6],    # a NaN in one layer's KL: NOT skipped, shows in that layer only
            [0.5, -4.0, 1.5, 0.75, 3.0, 6.0, 0.7, 0.8, 0.9]]
    vals = torch.tensor(rows, dtype=torch.float32)
    dev = vals.cuda()
    acc = torch.zeros(8 + L, dtype=torch.float64, device='cuda')
    out = torch.empty_like(acc)
    for k in range(len(rows)):
        _fold_row(K, dev[k], L, acc)
    K.summary_take(acc, out)
    got = out.cpu().tolist()
    good = [0, 4, 5]
    assert got[0] == 3.0 and got[1] == 3.0
    for i in range(6 + L):
        s = 0.0
        for k in good:
            s += float(vals[k, i])
        if i == 7:
            assert math.isnan(got[2 + i]) and math.isnan(s)
        else:
            assert got[2 + i] == s and math.isfinite(s), i
    from lvae_amd import summary
    m = summary.means(got, L, True)
    assert m['steps'] == 3 and m['nonfinite_steps'] == 3 and math.isnan(m['kl_layers/kl_layer_1'])
    assert all(math.isfinite(v) for k, v in m.items() if k != 'kl_layers/kl_layer_1')
    # a window of bad steps only: counted, nothing averaged
    for k in (1, 2, 3):
        _fold_row(K, dev[k], L, acc)
    K.summary_take(acc, out)
    assert out.cpu().tolist() == [0.0, 3.0] + [0.0] * (6 + L)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_library_refuses_bad_arguments():
    import lvae_amd  # noqa: F401
    from lvae_amd import _C
    from lvae_amd import kernels as K
    f = torch.ones(80, device='cuda')
    acc = torch.zeros(8 + 65 + 1, dtype=torch.float64, device='cuda')
    out = torch.zeros_like(acc)
    sp = _C.stream_ptr()

    def fold(L, acc_ptr, kl=f.data_ptr()):
        p = f.data_ptr()
        _C.call('lvae_summary_fold_f64', p, p + 4, p + 8, p + 12, p + 16, p + 20, None, kl, L, acc_ptr, sp)

    fold(64, acc.data_ptr())                               # the largest L is taken
    for L, acc_ptr in ((65, acc.data_ptr()), (-1, acc.data_ptr()), (3, None), (3, acc.data_ptr() + 4)):
        with pytest.raises(_C.LvaeHipError):
            fold(L, acc_ptr)
    with pytest.raises(_C.LvaeHipError):
        fold(3, acc.data_ptr(), kl=None)
    with pytest.raises(_C.LvaeHipError):                   # a CPU accumulator, a CPU scalar
        K.summary_fold(f[0:1], f[1:2], f[2:3], f[3:4], f[4:5], f[8:11], torch.zeros(11, dtype=torch.float64))
    with pytest.raises(_C.LvaeHipError):
        K.summary_fold(torch.ones(1), f[1:2], f[2:3], f[3:4], f[4:5], f[8:11], acc[:11])
    with pytest.raises(_C.LvaeHipError):                   # the accumulator and the per-layer KLs disagree
        K.summary_fold(f[0:1], f[1:2], f[2:3], f[3:4], f[4:5], f[8:12], acc[:11])
    for n, a, o in ((0, acc.data_ptr(), out.data_ptr()), (73, acc.data_ptr(), out.data_ptr()), (8, None, out.data_ptr()),
                    (8, acc.data_ptr(), None), (8, acc.data_ptr(), acc.data_ptr()), (8, acc.data_ptr() + 4, out.data_ptr())):
        with pytest.raises(_C.LvaeHipError):
            _C.call('lvae_summary_take_f64', a, n, o, sp)
    with pytest.raises(_C.LvaeHipError):
        K.summary_take(acc[:11], torch.zeros(11, dtype=torch.float64))
    torch.cuda.synchronize()
    # none of the refused calls touched the accumulator: it holds the one accepted step
    assert acc.cpu().tolist() == [1.0, 0.0] + [1.0] * (6 + 64) + [0.0, 0.0]


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. / 5. the fold inside the step: training is untouched, captured equals eager
# ---------------------------------------------------------------------------------------------------------------------------------
def _count_calls(monkeypatch):
    from lvae_amd import _C
    from lvae_amd import kernels as K
    names = []
    real = _C.call

    def counted(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(_C, 'call', counted)
    monkeypatch.setattr(K, 'call', counted)
    return names


def _six_steps(use_graph, with_summary, names=None):
    from lvae_amd.engine import TrainStep
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax
    from lvae_amd.summary import TrainSummary
    g = load_golden('tiny_cifar')
    _fresh_table()
    m = _model(g.cfg, g.state_dict(), PhiloxNoise(seed=3))
    opt = Adamax(m, lr=1e-3)
    summ = TrainSummary(len(g.cfg['z_dims']), 'cuda') if with_summary else None
    st = TrainStep(m, opt, use_graph=use_graph, summary=summ)
    n0 = len(names) if names is not None else 0
    outs = []
    for k in range(6):
        outs.append({key: v.detach().clone() for key, v in st(_images(4, 60 + k).cuda()).items()})
    torch.cuda.synchronize()
    assert (st.graph_a is not None) == use_graph and int(opt.step_count.item()) == 6
    return {'outs': outs, 'state': _train_state(m, opt), 'vector': summ.take_vector() if summ else None,
            'calls': list(names[n0:]) if names is not None else None}


def test_training_is_untouched_and_captured_equals_eager(monkeypatch):
    import lvae_amd  # noqa: F401
    names = _count_calls(monkeypatch)
    eager = _six_steps(False, True)
    plain = _six_steps(True, False, names)
    graph = _six_steps(True, True, names)
    # 4. parameters, Adamax state, BatchNorm buffers and the returned scalars: bit for bit, with and without a summary
    for run in (graph, eager):
        assert run['state'].keys() == plain['state'].keys()
        for k in plain['state']:
            assert torch.equal(run['state'][k], plain['state'][k]), k
        for a, b in zip(run['outs'], plain['outs']):
            for k in a:
                assert torch.equal(a[k], b[k]), k
    # without a summary the step is what it was: the fold is never reached, and the gradient norm is not computed. Of the six steps, three
    # go through Python (two eager ones and the capture): with a summary each of them issues exactly two more calls, nothing else changes
    assert 'lvae_summary_fold_f64' not in plain['calls'] and plain['calls'].count('lvae_l2norm_f32') == 3
    assert graph['calls'].count('lvae_summary_fold_f64') == 3 and graph['calls'].count('lvae_l2norm_f32') == 6
    stripped = []                                           # the run with a summary minus each fold and the l2norm in front of it
    for n in graph['calls']:
        if n == 'lvae_summary_fold_f64':
            assert stripped.pop() == 'lvae_l2norm_f32'
            continue
        stripped.append(n)
    # (the take at the end is the last call of the run with a summary)
    assert stripped[-1] == 'lvae_summary_take_f64' and stripped[:-1] == plain['calls']
    assert len(graph['calls']) == len(plain['calls']) + 2 * 3 + 1
    # the fold sits immediately before Adamax
    at = [j for j, n in enumerate(graph['calls']) if n == 'lvae_summary_fold_f64']
    assert all(graph['calls'][j + 1] == 'lvae_adamax_step_f32' for j in at)
    # 5. captured equals eager: six steps folded (a replay folds once), the same sums bit for bit
    assert graph['vector'][0].item() == 6.0 and graph['vector'][1].item() == 0.0
    assert torch.equal(graph['vector'], eager['vector'])
    # and they are the float64 sums of what the steps returned
    for slot, k in enumerate(SCALARS):
        s = 0.0
        for o in graph['outs']:
            s += float(o[k])
        assert graph['vector'][2 + slot].item() == s, k
    assert graph['vector'][7].item() > 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. window semantics
# ---------------------------------------------------------------------------------------------------------------------------------
def test_windows_of_one_and_of_three():
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels as K
    from lvae_amd.engine import TrainStep
    from lvae_amd.experiment.experiment_manager import LVAEExperiment
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax
    from lvae_amd.summary import TrainSummary
    g = load_golden('tiny_cifar')
    _fresh_table()
    m = _model(g.cfg, g.state_dict(), PhiloxNoise(seed=3))
    opt = Adamax(m, lr=1e-3)
    L = len(g.cfg['z_dims'])
    summ = TrainSummary(L, 'cuda')
    st = TrainStep(m, opt, use_graph=True, summary=summ)
    empty = summ.take()
    assert empty['steps'] == 0 and math.isnan(empty['loss/loss']) and 'l2/grad' not in empty
    for k in range(4):                                     # two eager steps, the capture, one replay
        out = st(_images(4, 80 + k).cuda())
        want = LVAEExperiment.get_metrics_dict(out)        # (.item() widens the float32 exactly)
        want['l2/grad'] = float(K.l2norm(m.arena.grads))   # the arena still holds the gradient Adamax applied
        w = summ.take()
        assert w.pop('steps') == 1 and w.pop('nonfinite_steps') == 0
        assert w == want, (k, w, want)
    assert st.graph_a is not None
    three = []
    for k in range(3):
        out = st(_images(4, 90 + k).cuda())
        d = LVAEExperiment.get_metrics_dict(out)
        d['l2/grad'] = float(K.l2norm(m.arena.grads))
        three.append(d)
    w = summ.take()
    assert w.pop('steps') == 3 and w.pop('nonfinite_steps') == 0
    assert set(w) == set(three[0])
    for k in w:
        assert w[k] == (0.0 + three[0][k] + three[1][k] + three[2][k]) / 3.0, k
    assert len({d['loss/loss'] for d in three}) == 3       # three different steps


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. forced exchange on one GPU, split form: the fold sits in graph B and sees the scaled gradient
# ---------------------------------------------------------------------------------------------------------------------------------
def test_split_form_folds_in_graph_b_with_the_gradient_scale(tmp_path):
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / 'split.json')
    env = dict(os.environ)
    env.update(RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
    env.pop('LVAE_DDP_MODE', None)
    p = subprocess.run([sys.executable, WORKER, 'split', out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    rows = json.load(open(out))
    assert len(rows) == 5 and [r['graph_b'] for r in rows] == [False, False, True, True, True]
    for r in rows:
        w = r['window']
        assert w['steps'] == 1 and w['nonfinite_steps'] == 0          # one fold per call: it is in graph B, once
        assert w['loss/loss'] == r['loss']
        assert r['raw_norm'] > 0.0 and w['l2/grad'] == float(np.float32(r['raw_norm']) * np.float32(0.5))


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. checkpoint and resume in the middle of a window
# ---------------------------------------------------------------------------------------------------------------------------------
def test_resume_in_the_middle_of_a_window_is_exact(tmp_path):
    import lvae_amd  # noqa: F401
    from lvae_amd.checkpoint import load_checkpoint, save_checkpoint
    from lvae_amd.engine import TrainStep
    from lvae_amd.models.lvae import LadderVAE
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax
    from lvae_amd.summary import TrainSummary
    g = load_golden('tiny_cifar')
    L = len(g.cfg['z_dims'])
    xs = [_images(4, 50 + k) for k in range(8)]

    def run(m, opt, summ, batches):
        st = TrainStep(m, opt, use_graph=True, summary=summ)
        for x in batches:
            st(x.cuda())
        torch.cuda.synchronize()

    _fresh_table()
    m = _model(g.cfg, g.state_dict(), PhiloxNoise(seed=3))
    opt, summ = Adamax(m, lr=1e-3), TrainSummary(L, 'cuda')
    run(m, opt, summ, xs)
    straight = summ.take_vector()
    assert straight[0].item() == 8.0

    _fresh_table()
    m1 = _model(g.cfg, g.state_dict(), PhiloxNoise(seed=3))
    opt1, summ1 = Adamax(m1, lr=1e-3), TrainSummary(L, 'cuda')
    run(m1, opt1, summ1, xs[:5])
    path, bare = str(tmp_path / 'model_5.pt'), str(tmp_path / 'no_summary.pt')
    save_checkpoint(path, m1, opt1, summary=summ1)         # in the middle of the window: nothing was taken
    save_checkpoint(bare, m1, opt1)
    ck = torch.load(path)
    assert isinstance(ck['summary'], list) and all(type(v) is float for v in ck['summary']) and ck['summary'][0] == 5.0
    assert 'summary' not in torch.load(bare)
    del m1, opt1, summ1

    _fresh_table()
    torch.manual_seed(123)
    m2 = LadderVAE(**g.cfg).cuda().train()                 # other weights and another noise seed: all of it comes from the file
    m2.noise = PhiloxNoise(seed=999)
    opt2, summ2 = Adamax(m2, lr=1e-3), TrainSummary(L, 'cuda')
    load_checkpoint(path, m2, opt2, summary=summ2)
    run(m2, opt2, summ2, xs[5:])
    assert torch.equal(summ2.take_vector(), straight)

    # a checkpoint written without a summary loads, and the window is empty (whatever the summary held)
    summ3 = TrainSummary(L, 'cuda')
    summ3.load_state([float(i + 1) for i in range(8 + L)])
    assert summ3.state() == [float(i + 1) for i in range(8 + L)]
    load_checkpoint(bare, m2, opt2, summary=summ3)
    assert summ3.state() == [0.0] * (8 + L)
    load_checkpoint(bare, m2, opt2)                        # and as before without one


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. the trainer
# ---------------------------------------------------------------------------------------------------------------------------------
_TINY_ARGV = ['-d', 'cifar10', '--zdims', '8', '8', '--downsample', '1', '1', '--nfilters', '16', '--skip', '--gated', '--freebits', '1.0',
              '--batch-size', '8', '--synthetic', '--seed', '3']


def _train_lines(stdout):
    out = {}
    for line in stdout.splitlines():
        mt = re.search(r'\[step (\d+)\]', line)
        if mt:
            out[int(mt.group(1))] = re.sub(r'\s*\[\d+ img/s\]', '', line)
    return out


def test_main_window_summaries_and_history(tmp_path):
    hist, hist2 = str(tmp_path / 'h.jsonl'), str(tmp_path / 'h2.jsonl')
    argv = _TINY_ARGV + ['--steps', '12', '--log-every', '4']
    runs = {}
    for tag, extra in (('window', ['--window-summaries', '--history', hist]), ('last', ['--history', hist2])):
        p = subprocess.run([sys.executable, '-m', 'lvae_amd.main'] + argv + extra, cwd=ROOT, capture_output=True, text=True, encoding='utf-8',
                           env=dict(os.environ, PYTHONIOENCODING='utf-8'), timeout=600)
        assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
        runs[tag] = _train_lines(p.stdout)
        assert sorted(runs[tag]) == [4, 8, 12], p.stdout
    suffix = re.compile(r'   grad: \S+   \[averaged over 4 steps × 1 ranks\]$')
    for step in (4, 8, 12):
        w, last = runs['window'][step], runs['last'][step]
        assert 'averaged over 4 steps' in w and suffix.search(w), w
        assert 'averaged' not in last and 'grad:' not in last, last
        assert suffix.sub('', w) != last                   # a mean of four steps, not the fourth
    recs = [json.loads(ln) for ln in open(hist).read().splitlines()]
    assert [(r['step'], r['split'], r['steps'], r['nonfinite_steps']) for r in recs] == [(4, 'train', 4, 0), (8, 'train', 4, 0),
                                                                                       (12, 'train', 4, 0)]
    for r in recs:
        assert {'loss/loss', 'elbo/elbo', 'elbo/recons', 'elbo/kl', 'l2/l2', 'l2/grad', 'kl_layers/kl_layer_0',
                'kl_layers/kl_layer_1'} == set(r['metrics'])
        assert '{:.5g}'.format(r['metrics']['loss/loss']) in runs['window'][r['step']]
    recs2 = [json.loads(ln) for ln in open(hist2).read().splitlines()]
    assert [(r['step'], r['split']) for r in recs2] == [(4, 'train'), (8, 'train'), (12, 'train')]
    assert all('steps' not in r and 'l2/grad' not in r['metrics'] for r in recs2)
    for r in recs2:
        assert '{:.5g}'.format(r['metrics']['loss/loss']) in runs['last'][r['step']]
