"""The gradient guard's host side: the layout of its device struct, the argument checks of GradGuard and of the command line, the run
description, and its state dict through a checkpoint file. No GPU."""
import ctypes
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_struct(struct):
    """[(type, name)] of a struct of include/lvae_hip.h, in order"""
    hdr = open(os.path.join(ROOT, 'include', 'lvae_hip.h')).read()
    body = hdr[hdr.index('typedef struct %s {' % struct):hdr.index('} %s;' % struct)]
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    body = body[body.index('{') + 1:]
    out = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            ty, name = decl.rsplit(None, 1)
            out.append((ty.strip(), name.strip()))
    return out


def test_guard_struct_layouts_match_header():
    import lvae_amd  # noqa: F401
    from lvae_amd import _C
    ctype = {'float': ctypes.c_float, 'int32_t': ctypes.c_int32, 'uint64_t': ctypes.c_uint64, 'int64_t': ctypes.c_int64,
             'float*': ctypes.c_void_p, 'const float*': ctypes.c_void_p}
    for struct, cls in (('lvae_grad_guard_state', _C.GradGuardState), ('lvae_copy_entry', _C.CopyEntry)):
        fields = _header_struct(struct)
        assert [n for _, n in fields] == [f[0] for f in cls._fields_]
        assert [ctype[t] for t, _ in fields] == [f[1] for f in cls._fields_]
    S = _C.GradGuardState
    assert ctypes.sizeof(S) == 32 and ctypes.alignment(S) == 8
    assert [getattr(S, f).offset for f in ('norm', 'scale', 'skip', 'reserved_', 'clipped', 'skipped')] == [0, 4, 8, 12, 16, 24]
    assert ctypes.sizeof(_C.CopyEntry) == 24 and [getattr(_C.CopyEntry, f).offset for f in ('dst', 'src', 'n')] == [0, 8, 16]
    # additions to the ABI: the library, the header and the binding agree, and a library without the symbols fails at load
    assert _C.load().lvae_abi_version() == _C.ABI_VERSION
    for name in ('lvae_grad_guard_f32', 'lvae_adamax_guarded_step_f32', 'lvae_counter_advance_unless', 'lvae_multi_copy_f32'):
        assert name in _C.SIGNATURES


def test_grad_guard_refuses_bad_limits():
    import lvae_amd  # noqa: F401
    from lvae_amd.optim import GradGuard
    for bad in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError):
            GradGuard(max_norm=bad)
    for bad in (-1e-9, -math.inf, math.nan):
        with pytest.raises(ValueError):
            GradGuard(skip_threshold=bad)
    g = GradGuard(max_norm=2, skip_threshold=0)            # T = 0 is valid: it skips every non-zero gradient
    assert g.limits() == {'max_norm': 2.0, 'skip_threshold': 0.0} and g.counts() == (0, 0)
    assert GradGuard(skip_threshold=math.inf).limits() == {'max_norm': None, 'skip_threshold': math.inf}
    assert GradGuard().limits() == {'max_norm': None, 'skip_threshold': None}     # non-finite steps only


def test_state_dict_round_trip_through_a_file(tmp_path):
    import lvae_amd  # noqa: F401
    from lvae_amd.optim import GradGuard
    a = GradGuard(max_norm=100.0, skip_threshold=1e4)
    a.load_state_dict({'clipped': 7, 'skipped': 3})
    path = str(tmp_path / 'guard.pt')
    torch.save({'grad_guard': a.state_dict()}, path)
    sd = torch.load(path)['grad_guard']
    assert sd == {'max_norm': 100.0, 'skip_threshold': 1e4, 'clipped': 7, 'skipped': 3}
    b = GradGuard(max_norm=5.0)                            # the resumed run's own limits are the ones that run
    b.load_state_dict(sd)
    assert b.counts() == (7, 3) and b.limits() == {'max_norm': 5.0, 'skip_threshold': None}
    assert b.state_dict() == {'max_norm': 5.0, 'skip_threshold': None, 'clipped': 7, 'skipped': 3}


BASE = ['-d', 'cifar10', '--zdims', '8', '8', '--downsample', '1', '1', '--synthetic']


@pytest.mark.parametrize('flags', [['--max-grad-norm', '-1'], ['--max-grad-norm', '0'], ['--max-grad-norm', 'inf'], ['--max-grad-norm', 'nan'],
                                   ['--grad-skip-threshold', '-0.5'], ['--grad-skip-threshold', 'nan']])
def test_check_args_refuses(flags):
    import lvae_amd  # noqa: F401
    from lvae_amd.experiment.experiment_manager import LVAEExperiment, build_parser
    with pytest.raises(SystemExit) as e:
        LVAEExperiment._check_args(build_parser().parse_args(BASE + flags))
    assert flags[0] in str(e.value)


def test_flags_default_off_and_reach_the_guard_and_the_description():
    import lvae_amd  # noqa: F401
    from lvae_amd.experiment.experiment_manager import LVAEExperiment, build_parser
    args = LVAEExperiment._check_args(build_parser().parse_args(BASE))
    assert args.max_grad_norm is None and args.grad_skip_threshold is None and LVAEExperiment._make_guard(args) is None
    plain = LVAEExperiment._make_run_description(args)
    assert 'clip' not in plain and ',skip' not in plain
    args = LVAEExperiment._check_args(build_parser().parse_args(BASE + ['--max-grad-norm', '200', '--grad-skip-threshold', 'inf']))
    guard = LVAEExperiment._make_guard(args)
    assert guard.limits() == {'max_norm': 200.0, 'skip_threshold': math.inf}
    assert ',clip200,skipinf,seed' in LVAEExperiment._make_run_description(args)
    args = LVAEExperiment._check_args(build_parser().parse_args(BASE + ['--grad-skip-threshold', '0']))
    assert LVAEExperiment._make_guard(args).limits() == {'max_norm': None, 'skip_threshold': 0.0}
    assert ',skip0,seed' in LVAEExperiment._make_run_description(args)
