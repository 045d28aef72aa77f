"""Host side of latent interpolation: the declared and exported symbols, their bindings, the evaluation flags and the temperature
normaliser as the new callers use it. No GPU needed."""
import ctypes
import os
import re

import pytest

import lvae_amd  # noqa: F401
from lvae_amd.evaluate import parse_eval_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = ['-d', 'cifar10', '--zdims', '8', '8', '--downsample', '1', '1', '--nfilters', '16', '--synthetic']   # L = 2


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'lvae_hip.h')).read(), flags=re.S)


def test_header_declares_and_binding_types_the_new_symbols():
    from lvae_amd import _C
    hdr = _header()
    m = re.search(r'int\s+lvae_latent_interp_f32\s*\(([^)]*)\)\s*;', hdr)
    assert m, 'include/lvae_hip.h does not declare lvae_latent_interp_f32'
    params = [' '.join(p.split()) for p in m.group(1).split(',')]
    assert params == ['const float* za', 'const float* zb', 'const float* t', 'int32_t B', 'int64_t n', 'int32_t T', 'int32_t mode',
                      'float* out', 'void* workspace', 'size_t workspace_bytes', 'void* stream']
    res, args = _C.SIGNATURES['lvae_latent_interp_f32']
    assert res is ctypes.c_int and len(args) == len(params)
    assert args[3] is _C._I and args[4] is _C._L and args[5] is _C._I and args[6] is _C._I and args[9] is _C._Z
    m = re.search(r'size_t\s+lvae_latent_interp_workspace\s*\(([^)]*)\)\s*;', hdr)
    assert m, 'include/lvae_hip.h does not declare lvae_latent_interp_workspace'
    assert [' '.join(p.split()) for p in m.group(1).split(',')] == ['int32_t B', 'int32_t T']
    assert _C.SIGNATURES['lvae_latent_interp_workspace'] == (_C._Z, [_C._I, _C._I])
    assert int(re.search(r'#define LVAE_ABI_VERSION (\d+)', hdr).group(1)) == _C.ABI_VERSION == 17   # an addition: the version stays
    assert 'latent_interp.hip' in open(os.path.join(ROOT, 'ladder-vae-pytorch_amd', 'csrc', 'Makefile')).read()


def test_library_exports_the_new_symbols():
    from lvae_amd import _C
    lib = ctypes.CDLL(_C.LIB_PATH)
    for name in ('lvae_latent_interp_f32', 'lvae_latent_interp_workspace'):
        assert hasattr(lib, name), name
    assert _C.load().lvae_abi_version() == 17


def test_workspace_query_and_argument_checks_need_no_device():
    """The query is host arithmetic, and the argument checks return before any HIP call (the pointers below are never read)."""
    from lvae_amd import _C
    lib = _C.load()
    assert lib.lvae_latent_interp_workspace(12, 8) >= 0
    assert lib.lvae_latent_interp_workspace(0, 8) == 0 and lib.lvae_latent_interp_workspace(3, -1) == 0
    assert lib.lvae_latent_interp_f32(None, None, None, 2, 8, 3, 1, None, None, 0, None) != 0
    assert b'lvae_latent_interp_f32' in lib.lvae_last_error()


def test_kernels_wrapper_refuses_on_the_host():
    import torch
    from lvae_amd import _C, kernels as K
    a, t = torch.zeros(2, 8), torch.linspace(0, 1, 3)
    with pytest.raises(ValueError):
        K.latent_interp(a, torch.zeros(2, 9), t, 'slerp')
    with pytest.raises(ValueError):
        K.latent_interp(a, torch.zeros(3, 8), t, 'lerp')
    for mode in ('nlerp', 1, None, 'SLERP'):
        with pytest.raises(ValueError):
            K.latent_interp(a, a, t, mode)
    with pytest.raises(_C.LvaeHipError):   # CPU tensors: the HIP path never runs on host memory
        K.latent_interp(a, a.clone(), t, 'slerp')


def test_eval_flags_defaults():
    a = parse_eval_args(MODEL)
    assert a.interp is False
    assert a.interp_layers == [2]           # L only
    assert a.interp_steps == 8
    assert a.interp_mode == 'slerp'


def test_eval_flags_values():
    a = parse_eval_args(MODEL + ['--interp', '--interp-layers', '2', '1', '--interp-steps', '3', '--interp-mode', 'lerp', '--temperature', '0.8'])
    assert a.interp is True and a.interp_layers == [2, 1] and a.interp_steps == 3 and a.interp_mode == 'lerp' and a.temperature == [0.8]
    a = parse_eval_args(MODEL + ['--interp-steps', '1', '--interp-layers', '1'])
    assert a.interp_steps == 1 and a.interp_layers == [1] and not a.interp
    a = parse_eval_args(MODEL + ['--cond-samples'])   # the neighbouring flags keep their defaults
    assert a.cond_layers == [0, 1, 2] and a.cond_variations == 7 and not a.interp


@pytest.mark.parametrize('extra,message', [
    (['--interp-layers', '0'], '--interp-layers takes values'), (['--interp-layers', '3'], '--interp-layers takes values'),
    (['--interp-layers', '1', '-1'], '--interp-layers takes values'),
    (['--interp-steps', '0'], '--interp-steps must be'), (['--interp-steps', '-4'], '--interp-steps must be'),
    (['--interp-mode', 'cubic'], '--interp-mode')], ids=lambda v: ' '.join(v) if isinstance(v, list) else '')
def test_eval_flags_rejected(extra, message, capsys):
    with pytest.raises(SystemExit):
        parse_eval_args(MODEL + extra)
    assert message in capsys.readouterr().err   # the validation's own message: an unknown-flag exit does not satisfy this


def test_layer_temperatures_is_unchanged_for_the_new_callers():
    import torch
    from lvae_amd.models.lvae import layer_temperatures
    assert layer_temperatures(3, None) == [None, None, None]
    assert layer_temperatures(3, 0.5) == [0.5, 0.5, 0.5]
    assert layer_temperatures(3, [0.7, 1, 0.0]) == [0.7, 1.0, 0.0]
    rows = torch.tensor([0.0, 0.5])
    assert all(v is rows for v in layer_temperatures(3, rows))
    for bad in ([0.5, 0.5], -0.1, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            layer_temperatures(3, bad)
