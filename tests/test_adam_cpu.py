"""The second update rule without a GPU: the trainer's flags and their checks, the run description, the C ABI's new symbol, the constructors'
argument checks and the rule hand-over of saved optimizer state."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ['-d', 'cifar10', '--zdims', '8', '8', '--downsample', '1', '1', '--synthetic']


def _parse(flags):
    import lvae_amd  # noqa: F401
    from lvae_amd.experiment.experiment_manager import LVAEExperiment, build_parser
    return LVAEExperiment._check_args(build_parser().parse_args(BASE + flags))


def test_parser_defaults_and_accepts_the_three_flags():
    args = _parse([])
    assert args.optimizer == 'adamax' and list(args.betas) == [0.9, 0.999] and args.opt_eps == 1e-8
    assert args.lr == 3e-4 and args.weight_decay == 0.0          # --lr and --wd keep their defaults
    for rule in ('adamax', 'adam', 'adamw'):
        args = _parse(['--optimizer', rule, '--betas', '0.8', '0.95', '--opt-eps', '1e-6'])
        assert args.optimizer == rule and list(args.betas) == [0.8, 0.95] and args.opt_eps == 1e-6
    import lvae_amd  # noqa: F401
    from lvae_amd.experiment.experiment_manager import build_parser
    with pytest.raises(SystemExit):
        build_parser().parse_args(BASE + ['--optimizer', 'sgd'])
    with pytest.raises(SystemExit):
        build_parser().parse_args(BASE + ['--betas', '0.9'])


@pytest.mark.parametrize('flags', [['--betas', '1.0', '0.999'], ['--betas', '0.9', '1.0'], ['--betas', '-0.1', '0.9'], ['--betas', 'nan', '0.9'],
                                   ['--opt-eps', '-0.5'], ['--opt-eps', 'nan']])
def test_check_args_refuses(flags):
    with pytest.raises(SystemExit) as e:
        _parse(flags)
    assert flags[0] in str(e.value)


def test_run_description_is_unchanged_by_default_and_names_the_rule():
    import lvae_amd  # noqa: F401
    from lvae_amd.experiment.experiment_manager import LVAEExperiment
    d = LVAEExperiment._make_run_description
    plain = d(_parse([]))
    # the description of the default arguments, as it was before there was a second rule
    assert plain == 'cifar10,2ly,2bpl,64ch,block=bacdbacd,elu,drop=0.2,seed54321'
    assert d(_parse(['--optimizer', 'adamax'])) == plain
    assert d(_parse(['--optimizer', 'adam'])) == plain.replace(',seed', ',adam,seed')
    assert d(_parse(['--optimizer', 'adamw', '--wd', '0.01'])) == plain.replace(',seed', ',wd=0.01,adamw,seed')
    assert d(_parse(['--betas', '0.9', '0.9'])) == plain.replace(',seed', ',b0.9-0.9,seed')
    assert ',adamw,b0.9-0.95,clip100,seed' in d(_parse(['--optimizer', 'adamw', '--betas', '0.9', '0.95', '--max-grad-norm', '100']))
    # an args object from before the flags existed describes itself as it did
    old = _parse([])
    del old.optimizer, old.betas, old.opt_eps
    assert d(old) == plain and LVAEExperiment._check_args(old) is old


def test_abi_gains_the_symbol_and_keeps_its_version():
    import lvae_amd  # noqa: F401
    from lvae_amd import _C
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'lvae_hip.h')).read(), flags=re.S)
    assert int(re.search(r'#define LVAE_ABI_VERSION (\d+)', hdr).group(1)) == 17 == _C.ABI_VERSION
    m = re.search(r'int\s+lvae_adam_step_f32\s*\(([^;]*)\)\s*;', hdr)
    assert m, 'include/lvae_hip.h does not declare lvae_adam_step_f32'
    params = [' '.join(a.split()) for a in m.group(1).split(',')]
    assert [a.split()[-1] for a in params] == ['p', 'g', 'exp_avg', 'exp_avg_sq', 'mask', 'n', 'lr', 'schedule', 'beta1', 'beta2', 'eps',
                                               'weight_decay', 'decoupled', 'gscale', 'step_count', 'ema', 'decay', 'lr_out', 'guard', 'stream']
    res, args = _C.SIGNATURES['lvae_adam_step_f32']
    assert res is ctypes.c_int and len(args) == len(params)
    for a, ty in zip(params, args):
        if a.startswith('double'):
            assert ty is ctypes.c_double, a          # the betas go down as doubles: the bias corrections are formed from them
        elif a.startswith('float '):
            assert ty is ctypes.c_float, a
        elif a.startswith('int32_t'):
            assert ty is ctypes.c_int32, a
        elif a.startswith('int64_t'):
            assert ty is ctypes.c_int64, a
        elif 'lvae_lr_schedule*' in a:
            assert ty is ctypes.POINTER(_C.LrScheduleStruct), a
        else:
            assert '*' in a and ty is ctypes.c_void_p, a
    assert hasattr(ctypes.CDLL(_C.LIB_PATH), 'lvae_adam_step_f32')
    assert _C.load().lvae_adam_step_f32.argtypes == args


def test_argument_checks_that_precede_every_launch_need_no_gpu():
    """a call refused for its arguments launches nothing, so its code can be read here"""
    import lvae_amd  # noqa: F401
    from lvae_amd import _C
    fn = _C.load().lvae_adam_step_f32
    assert fn(None, None, None, None, None, 8, 1e-3, None, 0.9, 0.999, 1e-8, 0.0, 0, None, None, None, 0.0, None, None, None) == -1


def test_constructors_validate_their_arguments():
    import lvae_amd  # noqa: F401
    from lvae_amd.optim import RULES, Adam, AdamW, Adamax, LrSchedule, check_rule
    for cls in (Adam, AdamW):
        for bad in (dict(lr=-1e-3), dict(betas=(1.0, 0.999)), dict(betas=(0.9, 1.0)), dict(betas=(-0.1, 0.9)), dict(betas=(0.9,)),
                    dict(betas=(float('nan'), 0.9)), dict(eps=-1e-8), dict(weight_decay=-1e-2), dict(ema_decay=1.0), dict(ema_decay=-0.1),
                    dict(lr=float('nan'))):
            with pytest.raises(ValueError):
                cls(None, **bad)
        with pytest.raises(ValueError):
            cls(None, lr=1e-3, schedule=LrSchedule('cosine', 0, 5, min_lr=1e-2))      # min_lr above the base rate
    a, w, x = Adam(None), AdamW(None), Adamax(None)
    assert (a.rule, w.rule, x.rule) == ('adam', 'adamw', 'adamax') and set(RULES) == {'adam', 'adamw', 'adamax'}
    assert (a.lr, a.betas, a.eps, a.weight_decay, a.decoupled) == (1e-3, (0.9, 0.999), 1e-8, 0.0, False)
    assert (w.lr, w.betas, w.eps, w.weight_decay, w.decoupled) == (1e-3, (0.9, 0.999), 1e-8, 1e-2, True)
    assert Adam(None, decoupled_weight_decay=True, weight_decay=0.1).rule == 'adamw'
    assert (x.lr, x.betas, x.eps, x.weight_decay) == (3e-4, (0.9, 0.999), 1e-8, 0.0)
    for o in (a, w):
        assert o.exp_avg is None and o.exp_avg_sq is None and o.step_count is None and o.ema is None and o.lr_now is None
        assert o.gscale is None and o.guard is None and o.schedule is None and not hasattr(o, 'exp_inf')
    assert x.exp_inf is None and not hasattr(x, 'exp_avg_sq')
    # saved state goes from adam to adamw and back; exp_inf against exp_avg_sq is refused with both names
    assert check_rule('adam', 'adamw') == check_rule('adamw', 'adam') == 'exp_avg_sq' and check_rule('adamax', 'adamax') == 'exp_inf'
    for was, now in (('adamax', 'adam'), ('adamw', 'adamax')):
        with pytest.raises(ValueError) as e:
            check_rule(was, now)
        assert was in str(e.value) and now in str(e.value)
