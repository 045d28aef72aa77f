"""Host side of the trainer's test-pass, checkpoint and KL warm-up flags: the schedule helper, checkpoint rotation, the flag defaults,
the warm-up formula the device reproduces, and the new C ABI symbols. No GPU needed."""
import os
import re

import numpy as np

import lvae_amd  # noqa: F401
from lvae_amd.schedule import TrainSchedule, checkpoint_path, checkpoints_to_delete

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_schedule_tests_ll_and_checkpoints():
    s = TrainSchedule(test_every=2, ll_every=4, ll_samples=8, checkpoint_every=2, has_test=True, checkpoint_dir='ck')
    got = {k: s.at(k) for k in range(1, 9)}
    assert got == {1: (0, False), 2: (1, True), 3: (0, False), 4: (8, True), 5: (0, False), 6: (1, True), 7: (0, False),
                   8: (8, True)}


def test_schedule_without_test_split_or_checkpoint_dir():
    s = TrainSchedule(2, 4, 8, 2, has_test=False, checkpoint_dir='')
    assert all(s.at(k) == (0, False) for k in range(1, 20))
    s = TrainSchedule(3, 0, 100, 0, has_test=True, checkpoint_dir='ck')   # 0 disables a cadence
    assert [k for k in range(1, 10) if s.at(k)[0]] == [3, 6, 9] and not any(s.at(k)[1] for k in range(1, 10))
    assert TrainSchedule(5, 5, 1, 1, True).at(5) == (1, False)   # --ll-samples 1: a plain test pass


def test_checkpoint_rotation():
    names = ['model_2.pt', 'model_10.pt', 'model_4.pt', 'model_8.pt', 'model_6.pt', 'notes.txt', 'model_x.pt', 'model_3.pt.tmp']
    assert sorted(checkpoints_to_delete(names, 2)) == ['model_2.pt', 'model_4.pt', 'model_6.pt']   # numeric, not lexical, order
    assert checkpoints_to_delete(names, 5) == []
    assert checkpoints_to_delete(names, 0) == []
    assert checkpoints_to_delete(['model_6.pt', 'model_8.pt'], 2) == []
    assert checkpoint_path('d', 6) == os.path.join('d', 'model_6.pt')


def test_flags_parse_with_reference_defaults():
    from lvae_amd.experiment.experiment_manager import build_parser
    a = build_parser().parse_args([])
    assert (a.test_log_every, a.loglikelihood_every, a.loglikelihood_samples) == (10000, 50000, 100)
    assert (a.checkpoint_every, a.keep_checkpoint_max, a.beta_anneal) == (100000, 2, 0)
    assert a.checkpoint_dir == '' and a.synthetic_test == 0 and a.resume == ''
    a = build_parser().parse_args(['--ts-log-every', '2', '--ll-every', '4', '--ll-samples', '8', '--checkpoint-every', '2',
                                   '--keep-checkpoint-max', '3', '--max-epochs', '5', '--beta-anneal', '3', '--checkpoint-dir', 'ck',
                                   '--synthetic-test', '64'])
    assert (a.test_log_every, a.loglikelihood_every, a.loglikelihood_samples, a.checkpoint_every, a.keep_checkpoint_max,
            a.max_epochs, a.beta_anneal, a.checkpoint_dir, a.synthetic_test) == (2, 4, 8, 2, 3, 5, 3, 'ck', 64)
    s = TrainSchedule.from_args(a, has_test=True)
    assert s.at(4) == (8, True) and s.at(2) == (1, True)


def _device_beta(step, steps):
    """lvae_elbo_loss_*_anneal_f32's beta: min(max(step / steps, 0), 1) in double, rounded to float once; 1 when steps <= 0."""
    if steps <= 0:
        return np.float32(1.0)
    r = np.float64(step) / np.float64(steps)
    return np.float32(np.float64(0.0) + (np.float64(1.0) - np.float64(0.0)) * min(max(r, 0.0), 1.0))


def test_linear_anneal_rounds_like_the_device():
    from lvae_amd.engine import linear_anneal
    cases = [(s, n) for n in (1, 3, 7, 1000, 12345, 2 ** 31 + 11) for s in (0, 1, n // 3, n - 1, n, n + 1, 10 * n, 2 ** 40)]
    cases += [(5, 0), (5, -3), (0, 0)]
    for s, n in cases:
        host = np.float32(float(linear_anneal(s, 0.0, 1.0, n)))
        assert host.tobytes() == _device_beta(s, n).tobytes(), (s, n, host, _device_beta(s, n))
    assert float(linear_anneal(4, 0.0, 1.0, 4)) == 1.0 and float(linear_anneal(9, 0.0, 1.0, 4)) == 1.0
    assert float(linear_anneal(3, 0.0, 1.0, 0)) == 1.0


def test_new_symbols_are_declared_and_bound():
    from lvae_amd import _C
    hdr = open(os.path.join(ROOT, 'include', 'lvae_hip.h')).read()
    for name in ('lvae_elbo_loss_fwd_anneal_f32', 'lvae_elbo_loss_bwd_anneal_f32', 'lvae_eval_online_f32', 'lvae_eval_totals_f64'):
        assert re.search(r'\bint %s\(' % name, hdr), name
        assert name in _C.SIGNATURES, name
    assert int(re.search(r'#define LVAE_ABI_VERSION (\d+)', hdr).group(1)) == _C.ABI_VERSION == 17
    # the warm-up entry points take the device step counter instead of a float beta
    assert 'const int64_t* step, int64_t anneal_steps' in hdr
