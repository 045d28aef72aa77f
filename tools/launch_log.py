"""The sequence of C-ABI calls of a few passes, one line per call, for comparing two checkouts: `python tools/launch_log.py OUT.txt`.

Wraps `_C.call` (and the name `kernels.call` it was imported under) and writes the entry name and, for every lvae_conv_desc / lvae_rb_ext /
lvae_bn_apply / lvae_bn_fold argument, its non-pointer fields and per pointer field only whether it is null. Per model: two eager training
steps (the second one has the cross-block prefetch links) and one eval-mode forward. Prints the line count and the sha256 of the log."""
import ctypes as C
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
from conftest import load_golden  # noqa: E402
from lvae_amd import _C, configs, kernels  # noqa: E402
from lvae_amd.engine import TrainStep  # noqa: E402
from lvae_amd.models.lvae import LadderVAE  # noqa: E402
from lvae_amd.noise import PhiloxNoise  # noqa: E402
from lvae_amd.optim import Adamax  # noqa: E402

lines = []
_real_call = _C.call


def _field(v):
    if isinstance(v, C.Array):
        return '[%s]' % ','.join(_field(e) for e in v)
    return repr(v)


def _struct(s):
    out = []
    for name, typ in s._fields_:
        v = getattr(s, name)
        if typ is C.c_void_p:
            v = 'null' if not v else 'set'
        elif isinstance(v, C.Array) and v._type_ is C.c_void_p:
            v = '[%s]' % ','.join('null' if not e else 'set' for e in v)
        else:
            v = _field(v)
        out.append('%s=%s' % (name, v))
    return '%s(%s)' % (type(s).__name__, ' '.join(out))


def _logged_call(name, *args):
    structs = [getattr(a, '_obj', None) for a in args]
    lines.append(' '.join([name] + [_struct(s) for s in structs if isinstance(s, (_C.ConvDesc, _C.RbExt, _C.BnApply, _C.BnFold))]))
    return _real_call(name, *args)


def passes(tag, cfg, batch, dtype, state_dict=None):
    lines.append('# %s batch %d %s' % (tag, batch, dtype))
    torch.manual_seed(0)
    model = LadderVAE(**cfg)
    if state_dict is not None:
        model.load_state_dict(state_dict)
    model.cuda().train()
    model.compute_dtype = dtype
    model.noise = PhiloxNoise(seed=42)
    x = configs.synthetic_images(cfg, batch, torch.Generator().manual_seed(1)).cuda()
    step = TrainStep(model, Adamax(model, lr=3e-4), use_graph=False)
    for i in range(2):
        lines.append('# %s training step %d' % (tag, i))
        step(x)
    lines.append('# %s eval forward' % tag)
    model.eval()
    with torch.no_grad():
        model(x)
    torch.cuda.synchronize()


def main(path):
    _C.call = kernels.call = _logged_call
    passes('cifar15', configs.CIFAR15, 256, 'f32')
    passes('cifar15', configs.CIFAR15, 256, 'bf16')
    passes('mnist3', configs.MNIST3, 64, 'f32')
    for name in ('tiny_cifar', 'tiny_mnist', 'tiny_bacdbac', 'tiny_cabdcabd', 'tiny_nobn_selu'):
        g = load_golden(name)
        passes(name, g.cfg, g.t('x').shape[0], 'f32', g.state_dict())
    text = '\n'.join(lines) + '\n'
    with open(path, 'w') as f:
        f.write(text)
    print('%s: %d lines, sha256 %s' % (path, len(lines), hashlib.sha256(text.encode()).hexdigest()))


if __name__ == '__main__':
    main(sys.argv[1])
