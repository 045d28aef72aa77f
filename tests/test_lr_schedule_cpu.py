"""The learning-rate schedule on the host (no GPU): lvae_lr_schedule_at, the function the scheduled Adamax kernel runs on the device,
against torch.optim.lr_scheduler and at its boundaries; validation in Python and through the C entry points; the struct's layout; the
trainer's flags; the checkpoint record."""
import argparse
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

BASE = 3e-4


def f32(x):
    """the double value of x rounded to float32: what a float field of struct lvae_lr_schedule holds"""
    return float(np.float32(x))


def within_one_spacing(got, want):
    return abs(float(got) - want) <= float(np.spacing(np.float32(want)))


def _torch_lrs(make, steps, lr):
    p = torch.zeros(1, requires_grad=True)
    opt = torch.optim.SGD([p], lr=lr)
    sched = make(opt)
    out = []
    for _ in range(steps):
        out.append(sched.get_last_lr()[0])
        opt.step()
        sched.step()
    return out


def _cases():
    from torch.optim import lr_scheduler as L
    from lvae_amd.optim import LrSchedule
    # The struct carries base_lr, min_lr and gamma as float32 (like the `lr` argument of the unscheduled entry points), so the rate that is
    # scheduled is fl32(3e-4), the floor fl32(3e-5) and the factor fl32(0.9): torch, in double, is given exactly those values. With the
    # decimal constants themselves the two sides would schedule different numbers (0.9 ** 19 and fl32(0.9) ** 19 are 4e-7 apart, relatively,
    # six float32 spacings) and the comparison would measure that instead of the schedule.
    lo, g9 = f32(3e-5), f32(0.9)
    return [
        ('warm-up', lambda o: L.LinearLR(o, start_factor=1 / 5, total_iters=4), LrSchedule('constant', warmup_steps=5), 12),
        ('cosine', lambda o: L.CosineAnnealingLR(o, T_max=40, eta_min=lo), LrSchedule('cosine', decay_steps=40, min_lr=3e-5), 41),
        ('step', lambda o: L.StepLR(o, step_size=4, gamma=.5), LrSchedule('step', decay_steps=4, gamma=.5), 20),
        ('exp', lambda o: L.ExponentialLR(o, gamma=g9), LrSchedule('exp', decay_steps=1, gamma=.9), 20),
        ('linear', lambda o: L.LinearLR(o, 1.0, lo / f32(BASE), total_iters=10), LrSchedule('linear', decay_steps=10, min_lr=3e-5), 16),
    ]


@pytest.mark.parametrize('case', range(5), ids=['warm-up', 'cosine', 'step', 'exp', 'linear'])
def test_schedule_agrees_with_torch_schedulers(case):
    import lvae_amd  # noqa: F401
    name, make, sched, steps = _cases()[case]
    want = _torch_lrs(make, steps, f32(BASE))
    got = [sched.at(BASE, n) for n in range(steps)]
    worst = max(abs(g - w) / float(np.spacing(np.float32(w))) for g, w in zip(got, want))
    print('%s: worst distance from torch %.3f float32 spacings over %d steps' % (name, worst, steps))
    assert len(set(want)) > 3                                 # the rate moves
    for n, (g, w) in enumerate(zip(got, want)):
        assert within_one_spacing(g, w), (name, n, g, w)


def _formula(kind, n, W, T, base, min_lr=0.0, gamma=0.1):
    """the issue's definition, in Python doubles on the float32 values the struct holds"""
    base, min_lr, gamma = f32(base), f32(min_lr), f32(gamma)
    if n < W:
        return base * (n + 1) / W
    t, m = n - W, min_lr / base
    f = {'constant': lambda: 1.0,
         'cosine': lambda: m + (1 - m) * 0.5 * (1 + math.cos(math.pi * min(t, T) / T)),
         'linear': lambda: 1 - (1 - m) * min(t, T) / T,
         'step': lambda: max(m, gamma ** (t // T)),
         'exp': lambda: max(m, gamma ** (t / T))}[kind]()
    return base * f


@pytest.mark.parametrize('kind', ['constant', 'cosine', 'linear', 'step', 'exp'])
def test_boundaries_floor_and_flat_tail(kind):
    import lvae_amd  # noqa: F401
    from lvae_amd.optim import LrSchedule
    W, T, lo, gamma = 7, 9, 2e-5, 0.25
    s = LrSchedule(kind, warmup_steps=W, decay_steps=T, min_lr=lo, gamma=gamma)
    at = lambda n: s.at(BASE, n)  # noqa: E731
    assert at(0) == np.float32(f32(BASE) / W) and at(0) > 0                        # the first step is not zero
    assert at(W - 1) == np.float32(BASE) and at(W) == np.float32(BASE)             # the warm-up ends at base; the decay starts there
    for n in (0, 1, W - 2, W - 1, W, W + 1, W + T - 1, W + T, W + T + 1, W + 3 * T, W + 40 * T, 10 ** 12):
        assert within_one_spacing(at(n), _formula(kind, n, W, T, BASE, lo, gamma)), (kind, n)
    if kind == 'constant':
        assert all(at(n) == np.float32(BASE) for n in (W + 1, W + T, 10 ** 12))
    if kind in ('cosine', 'linear'):
        assert at(W + T - 1) > at(W + T) == np.float32(lo)                         # reaches the floor at W + T ...
        assert at(W + T + 1) == at(W + 5 * T) == at(10 ** 12) == np.float32(lo)    # ... and stays
    if kind == 'step':
        assert at(W + T - 1) == np.float32(BASE) and at(W + T) == at(W + 2 * T - 1) == np.float32(f32(BASE) * 0.25)
        assert at(W + 2 * T) == np.float32(lo) == at(10 ** 12)                     # 1/16 of 3e-4 is below the floor
    if kind == 'exp':
        assert at(W + T) == np.float32(f32(BASE) * 0.25) and at(W + 1) < at(W)
        assert at(W + 2 * T) == np.float32(lo) == at(10 ** 12)
    # without warm-up the first step already runs at base
    assert LrSchedule(kind, 0, T, lo, gamma).at(BASE, 0) == np.float32(BASE)


def test_large_counter_does_not_pass_through_a_float():
    import lvae_amd  # noqa: F401
    from lvae_amd.optim import LrSchedule
    W = 2 ** 25
    s = LrSchedule('constant', warmup_steps=W)
    assert s.at(BASE, 2 ** 24 + 1) == np.float32(f32(BASE) * (2 ** 24 + 2) / W)
    # float32(2^24 + odd) is a neighbouring even number: a counter that passed through a float is off by one step, which is about one
    # float32 spacing of the result, so it shows at some of these steps (not at every one: the two may round to the same float)
    ns = range(2 ** 24 + 1, 2 ** 24 + 100, 2)
    assert all(s.at(BASE, n) == np.float32(f32(BASE) * (n + 1) / W) for n in ns)
    assert any(s.at(BASE, n) != np.float32(f32(BASE) * (float(np.float32(n)) + 1) / W) for n in ns)
    assert LrSchedule('linear', 3, 2 ** 40, 0.0).at(BASE, 3 + 2 ** 39 + 1) == np.float32(f32(BASE) * (1 - (2 ** 39 + 1) / 2 ** 40))


BAD_PYTHON = [dict(kind='triangle'), dict(kind='cosine'), dict(kind='cosine', decay_steps=0), dict(kind='linear', decay_steps=-4),
              dict(kind='step', decay_steps=0), dict(kind='exp', decay_steps=0), dict(warmup_steps=-1), dict(min_lr=-1e-6),
              dict(gamma=0.0), dict(gamma=-0.5), dict(gamma=1.5), dict(gamma=float('nan')), dict(min_lr=float('nan'))]


@pytest.mark.parametrize('kw', BAD_PYTHON, ids=lambda kw: ','.join('%s=%s' % kv for kv in kw.items()))
def test_constructor_rejects(kw):
    import lvae_amd  # noqa: F401
    from lvae_amd.optim import LrSchedule
    with pytest.raises(ValueError):
        LrSchedule(**kw)


def test_base_lr_is_checked_where_it_is_known():
    import lvae_amd  # noqa: F401
    from lvae_amd.optim import Adamax, LrSchedule
    s = LrSchedule('cosine', 2, 5, min_lr=1e-4)
    for base in (0.0, -1e-3, 5e-5, float('nan')):                                 # not positive, or below min_lr
        with pytest.raises(ValueError):
            s.at(base, 0)
        with pytest.raises(ValueError):
            Adamax(None, lr=base, schedule=s)
    assert s.at(1e-4, 10 ** 6) == np.float32(1e-4)                                # min_lr == base is allowed


# (base_lr, min_lr, gamma, kind, warmup_steps, decay_steps)
BAD_C = [(0.0, 0.0, 0.1, 0, 0, 0), (-1.0, 0.0, 0.1, 0, 0, 0), (float('nan'), 0.0, 0.1, 0, 0, 0),
         (1e-3, -1e-9, 0.1, 0, 0, 0), (1e-3, 2e-3, 0.1, 0, 0, 0), (1e-3, float('nan'), 0.1, 0, 0, 0),
         (1e-3, 0.0, 0.0, 0, 0, 0), (1e-3, 0.0, 1.5, 0, 0, 0), (1e-3, 0.0, float('nan'), 0, 0, 0),
         (1e-3, 0.0, 0.1, 0, -1, 0), (1e-3, 0.0, 0.1, 5, 0, 10), (1e-3, 0.0, 0.1, -1, 0, 10),
         (1e-3, 0.0, 0.1, 1, 0, 0), (1e-3, 0.0, 0.1, 2, 0, 0), (1e-3, 0.0, 0.1, 3, 0, -2), (1e-3, 0.0, 0.1, 4, 0, 0)]


@pytest.mark.parametrize('fields', BAD_C)
def test_c_entry_points_reject(fields):
    """LVAE_EINVAL from both entry points, before anything is launched or dereferenced (the pointers below are not memory)."""
    import lvae_amd  # noqa: F401
    from lvae_amd import _C
    lib = _C.load()
    s = _C.LrScheduleStruct(*fields)
    lr = ctypes.c_float(-7.0)
    assert lib.lvae_lr_schedule_at(ctypes.byref(s), 3, ctypes.byref(lr)) == -1 and lr.value == -7.0
    assert b'lvae_lr_schedule_at' in lib.lvae_last_error()
    fake = 4096
    assert lib.lvae_adamax_sched_step_f32(fake, fake, fake, fake, None, 4, ctypes.byref(s), 0.9, 0.999, 1e-8, 0.0, None, fake, None, 0.0,
                                          None, None) == -1
    assert b'lvae_adamax_sched_step_f32' in lib.lvae_last_error()


def test_c_entry_point_accepts_what_python_accepts():
    import lvae_amd  # noqa: F401
    from lvae_amd import _C
    lib = _C.load()
    lr = ctypes.c_float()
    for fields in [(1e-3, 0.0, 0.1, 0, 0, 0), (1e-3, 1e-3, 1.0, 1, 0, 1), (1e-3, 0.0, 0.1, 4, 3, 2), (1e-3, 0.0, 0.1, 0, 5, -1)]:
        assert lib.lvae_lr_schedule_at(ctypes.byref(_C.LrScheduleStruct(*fields)), 0, ctypes.byref(lr)) == 0, fields
    assert lib.lvae_lr_schedule_at(None, 0, ctypes.byref(lr)) == -1
    assert lib.lvae_lr_schedule_at(ctypes.byref(_C.LrScheduleStruct(1e-3, 0.0, 0.1, 0, 0, 0)), 0, None) == -1


def test_struct_layout_matches_header():
    import lvae_amd  # noqa: F401
    from lvae_amd import _C
    from test_cabi import ROOT, _header_fields
    assert _header_fields('lvae_lr_schedule') == [f[0] for f in _C.LrScheduleStruct._fields_]
    assert ctypes.sizeof(_C.LrScheduleStruct) == 32
    hdr = open(os.path.join(ROOT, 'include', 'lvae_hip.h')).read()
    enum = hdr[hdr.index('LVAE_LR_CONSTANT'):]
    enum = enum[:enum.index('}')]
    assert [int(v) for v in re.findall(r'LVAE_LR_[A-Z]+ = (\d+)', enum)] == [0, 1, 2, 3, 4]
    assert _C.LR_KINDS == {'constant': 0, 'cosine': 1, 'linear': 2, 'step': 3, 'exp': 4}
    assert [n.lower() for n in re.findall(r'LVAE_LR_([A-Z]+) =', enum)] == list(_C.LR_KINDS)


def _args(*argv):
    import lvae_amd  # noqa: F401
    from lvae_amd.experiment.experiment_manager import LVAEExperiment, build_parser
    return LVAEExperiment, build_parser().parse_args(list(argv))


def test_parser_and_check_args():
    from lvae_amd.optim import LrSchedule
    X, a = _args()
    assert (a.lr_schedule, a.lr_warmup, a.lr_decay_steps, a.lr_min, a.lr_gamma) == ('constant', 0, 0, 0.0, 0.1)
    assert X._make_schedule(X._check_args(a)) is None                             # no flag, no schedule: the plain optimizer step
    X, a = _args('--lr-schedule', 'constant', '--lr-decay-steps', '50', '--lr-min', '1e-5')
    assert X._make_schedule(X._check_args(a)) is None
    X, a = _args('--lr-warmup', '5')
    assert X._make_schedule(X._check_args(a)) == LrSchedule('constant', 5)
    X, a = _args('--lr', '1e-3', '--lr-schedule', 'cosine', '--lr-warmup', '100', '--lr-decay-steps', '900', '--lr-min', '1e-5')
    assert X._make_schedule(X._check_args(a)) == LrSchedule('cosine', 100, 900, 1e-5, 0.1)
    X, a = _args('--lr-schedule', 'step', '--lr-decay-steps', '30', '--lr-gamma', '0.5')
    assert X._make_schedule(X._check_args(a)) == LrSchedule('step', 0, 30, 0.0, 0.5)
    for kind in ('cosine', 'linear', 'step', 'exp'):
        X, a = _args('--lr-schedule', kind)
        with pytest.raises(SystemExit, match='--lr-decay-steps'):
            X._check_args(a)
    X, a = _args('--lr', '1e-4', '--lr-min', '2e-4', '--lr-warmup', '3')
    with pytest.raises(SystemExit, match='--lr-min'):
        X._check_args(a)
    X, a = _args('--lr-schedule', 'exp', '--lr-decay-steps', '10', '--lr-gamma', '2')
    with pytest.raises(SystemExit, match='gamma'):
        X._make_schedule(X._check_args(a))
    with pytest.raises(SystemExit):
        _args('--lr-schedule', 'triangle')
    # an older caller's namespace without the new attributes still passes the check and gets no schedule
    X, a = _args()
    old = argparse.Namespace(**{k: v for k, v in vars(a).items() if not k.startswith('lr_')})
    assert X._make_schedule(X._check_args(old)) is None


def test_checkpoint_record_round_trips(tmp_path):
    import lvae_amd  # noqa: F401
    from lvae_amd.checkpoint import lr_schedule_record
    from lvae_amd.optim import Adamax, LrSchedule
    s = LrSchedule('exp', 4, 250, 1e-6, 0.3)
    opt = Adamax(None, lr=2e-3, schedule=s)
    rec = lr_schedule_record(opt)
    assert rec == {'kind': 'exp', 'warmup_steps': 4, 'decay_steps': 250, 'min_lr': 1e-6, 'gamma': 0.3, 'base_lr': 2e-3}
    path = str(tmp_path / 'ck.pt')
    torch.save({'model': {}, 'lr_schedule': rec}, path)
    back = torch.load(path)['lr_schedule']
    assert back == rec
    again = LrSchedule(**{k: back[k] for k in LrSchedule.FIELDS})
    assert again == s and again.at(back['base_lr'], 100) == s.at(2e-3, 100)
    assert lr_schedule_record(Adamax(None)) is None


def test_no_schedule_by_default():
    import lvae_amd  # noqa: F401
    from lvae_amd.optim import Adamax
    opt = Adamax(None)
    assert opt.schedule is None and opt.lr_now is None and opt.current_lr() == 3e-4
