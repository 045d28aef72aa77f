"""Host side of the windowed training log (lvae_amd.summary): the means of a summed accumulator, the reduction over two gloo ranks, the
trainer's two flags and the JSONL history writer. No GPU."""
import json
import math
import os
import socket
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, 'tests', 'summary_worker.py')


def test_means_of_hand_made_vectors():
    import lvae_amd  # noqa: F401
    from lvae_amd import summary
    from lvae_amd.experiment.experiment_manager import LVAEExperiment
    #      steps bad  loss   elbo  recons  kl    l2   grad   kl_0  kl_1  kl_2
    vec = [4.0, 1.0, 10.0, -20.0, 18.0, 2.0, 40.0, 6.0, 1.0, 0.5, 0.25]
    m = summary.means(vec, 3, True)
    assert m == {'loss/loss': 2.5, 'elbo/elbo': -5.0, 'elbo/recons': 4.5, 'elbo/kl': 0.5, 'l2/l2': 10.0,
                 'kl_layers/kl_layer_0': 0.25, 'kl_layers/kl_layer_1': 0.125, 'kl_layers/kl_layer_2': 0.0625,
                 'l2/grad': 1.5, 'steps': 4, 'nonfinite_steps': 1}
    # the keys are get_metrics_dict's, in its order, then the three more
    one = {k: torch.tensor(1.0) for k in ('loss', 'elbo', 'recons', 'kl', 'l2')}
    one['kl_avg_layerwise'] = torch.ones(3)
    keys = list(LVAEExperiment.get_metrics_dict(one))
    assert list(m)[:len(keys)] == keys and list(m)[len(keys):] == ['l2/grad', 'steps', 'nonfinite_steps']
    # without gradient norms the slot is not reported
    m2 = summary.means(vec, 3, False)
    assert 'l2/grad' not in m2 and list(m2)[:len(keys)] == keys and m2['loss/loss'] == 2.5
    # L = 0
    assert list(summary.means(vec[:8], 0, False)) == keys[:5] + ['steps', 'nonfinite_steps']
    # an empty window: NaN means, counts as they are
    m0 = summary.means([0.0, 2.0] + [0.0] * 9, 3, True)
    assert m0['steps'] == 0 and m0['nonfinite_steps'] == 2
    assert all(math.isnan(v) for k, v in m0.items() if k not in ('steps', 'nonfinite_steps'))
    # a NaN in one layer's sum stays in that layer
    m3 = summary.means(vec[:9] + [math.nan, 0.25], 3, True)
    assert math.isnan(m3['kl_layers/kl_layer_1']) and m3['kl_layers/kl_layer_2'] == 0.0625 and m3['loss/loss'] == 2.5
    # the train line prints from it
    line = LVAEExperiment.train_log_str(m, 8) + summary.train_line_suffix(m, 1)
    assert 'loss: 2.5' in line and 'grad: 1.5' in line and '[1 non-finite steps]' in line and '[averaged over 4 steps × 1 ranks]' in line
    assert 'non-finite' not in summary.train_line_suffix(m2 | {'nonfinite_steps': 0}, 1)
    assert '[averaged over 2 steps × 2 ranks]' in summary.train_line_suffix(m, 2)
    try:
        summary.means(vec, 2, True)
    except ValueError:
        pass
    else:
        raise AssertionError('a vector of the wrong length was accepted')


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_gloo_ranks_get_the_mean_over_both_ranks_steps(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import summary_worker as W
    out = str(tmp_path / 'means.json')
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ)
        env.update(RANK=str(rank), WORLD_SIZE='2', LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        env.pop('LVAE_FORCE_DIST', None)
        procs.append(subprocess.Popen([sys.executable, WORKER, 'gloo', out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = [p.communicate(timeout=120)[0].decode() for p in procs]
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-3000:]
    got = [json.load(open(out + '.%d' % r)) for r in range(2)]
    assert got[0] == got[1] and got[0]['ranks'] == 2
    m = got[0]['means']
    steps = W.rank_steps(0) + W.rank_steps(1)          # five steps in all
    names = ['loss/loss', 'elbo/elbo', 'elbo/recons', 'elbo/kl', 'l2/l2', 'l2/grad', 'kl_layers/kl_layer_0', 'kl_layers/kl_layer_1']
    for i, k in enumerate(names):
        assert m[k] == sum(s[i] for s in steps) / 5.0, k   # float64; every value is dyadic, so the sums are exact in any order
    assert m['steps'] == 5 and m['nonfinite_steps'] == 1   # summed over the ranks
    assert m['l2/l2'] == 7.0                               # the same on every rank: the mean is that value


def test_parser_has_both_flags_off_by_default():
    import lvae_amd  # noqa: F401
    from lvae_amd.experiment.experiment_manager import build_parser
    a = build_parser().parse_args([])
    assert a.window_summaries is False and a.history == ''
    b = build_parser().parse_args(['--window-summaries', '--history', 'log.jsonl'])
    assert b.window_summaries is True and b.history == 'log.jsonl'


def test_history_appends_json_lines(tmp_path):
    import lvae_amd  # noqa: F401
    from lvae_amd.summary import History
    path = str(tmp_path / 'h.jsonl')
    h = History(path)
    h.write(4, 'train', {'loss/loss': 2.5, 'steps': 4, 'nonfinite_steps': 0}, steps=4, nonfinite_steps=0)
    assert len(open(path).read().splitlines()) == 1        # flushed line by line
    h.write(4, 'test', {'elbo/elbo': -3.0}, epoch=1)
    h.close()
    h2 = History(path)                                     # a second open appends
    h2.write(8, 'train', {'loss/loss': 2.0})
    h2.close()
    recs = [json.loads(ln) for ln in open(path).read().splitlines()]
    assert recs == [{'step': 4, 'split': 'train', 'metrics': {'loss/loss': 2.5}, 'steps': 4, 'nonfinite_steps': 0},
                    {'step': 4, 'split': 'test', 'epoch': 1, 'metrics': {'elbo/elbo': -3.0}},
                    {'step': 8, 'split': 'train', 'metrics': {'loss/loss': 2.0}}]
