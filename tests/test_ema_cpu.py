"""Host side of the weight average kept inside the optimizer step: the --ema-decay flag, the two C ABI entry points, and the Python
restatement of the decay ramp the device applies. No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import lvae_amd  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ema_decay_flag_parses_and_is_bounded():
    from lvae_amd.experiment.experiment_manager import build_parser
    assert build_parser().parse_args([]).ema_decay == 0.0
    assert build_parser().parse_args(['--ema-decay', '0.999']).ema_decay == 0.999
    assert build_parser().parse_args(['--ema-decay', '0']).ema_decay == 0.0
    for bad in ('1.0', '-0.1', '1.5'):
        with pytest.raises(SystemExit):
            build_parser().parse_args(['--ema-decay', bad])


def test_optimizer_refuses_decay_outside_unit_interval():
    from lvae_amd.optim import Adamax
    for bad in (1.0, -1e-3, 2.0):
        with pytest.raises(ValueError):
            Adamax(None, ema_decay=bad)
    assert Adamax(None).ema_decay == 0.0 and Adamax(None).ema is None


def test_entry_points_are_declared_bound_and_exported():
    from lvae_amd import _C
    hdr = open(os.path.join(ROOT, 'include', 'lvae_hip.h')).read()
    for name in ('lvae_adamax_ema_step_f32', 'lvae_swap_f32'):
        assert re.search(r'\bint %s\(' % name, hdr), name
        assert name in _C.SIGNATURES, name
    assert 'const uint64_t* step_count, float* ema, float decay, void* stream);' in hdr
    assert 'int lvae_swap_f32(float* a, float* b, int64_t n, void* stream);' in hdr
    # same arguments as lvae_adamax_step_f32 plus (ema, decay) in front of the stream
    base, ema = _C.SIGNATURES['lvae_adamax_step_f32'][1], _C.SIGNATURES['lvae_adamax_ema_step_f32'][1]
    assert ema == base[:-1] + [ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p]
    # Additions only: the version stays where tests/test_train_schedule_cpu.py pins it, and header, binding and library agree on it
    lib = ctypes.CDLL(_C.LIB_PATH)
    assert hasattr(lib, 'lvae_adamax_ema_step_f32') and hasattr(lib, 'lvae_swap_f32')
    assert int(re.search(r'#define LVAE_ABI_VERSION (\d+)', hdr).group(1)) == _C.ABI_VERSION == lib.lvae_abi_version()


def test_decay_ramp_restatement():
    from lvae_amd.optim import ema_decay_at
    f = np.float32
    for decay in (0.0, 0.75, 0.99, 0.999, 0.9999):
        for n in (0, 1, 9, 10 ** 4):
            want = min(f(decay), f(f(1) + f(n)) / f(f(10) + f(n)))
            got = ema_decay_at(decay, n)
            assert isinstance(got, np.float32) and got.tobytes() == f(want).tobytes(), (decay, n, got, want)
            assert abs(float(got) - min(decay, (1 + n) / (10 + n))) <= 2.0 ** -24   # one fp32 rounding of a value below 1
    assert float(ema_decay_at(0.999, 0)) == float(f(0.1)) and float(ema_decay_at(0.999, 9)) == float(f(10) / f(19))
    assert float(ema_decay_at(0.999, 10 ** 4)) == float(f(0.999)) and float(ema_decay_at(0.0, 5)) == 0.0
