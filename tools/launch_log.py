"""The sequence of C-ABI calls of a few passes, one line per call, for comparing two checkouts: `python tools/launch_log.py OUT.txt`.

Wraps `_C.call` (and the name `kernels.call` it was imported under) and writes the entry name and, for every lvae_conv_desc / lvae_rb_ext /
lvae_bn_apply / lvae_bn_fold argument, its non-pointer fields and per pointer field only whether it is null. Per model: two eager training
steps (the second one has the cross-block prefetch links) and one eval-mode forward. Then, per small golden model, the sampling and evaluation
passes (`sampling_passes`), each from a fresh PhiloxNoise(seed=42), each followed by one line per returned tensor with the sha256 of its
bytes: two checkouts that write the same file issue the same calls, draw the same noise and compute the same bits. Prints the line count and
the sha256 of the log."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
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


def _digest(name, v):
    """One `= name sha256` line per tensor under v (dicts, lists and tuples are walked; numbers are written out; None says so)."""
    if isinstance(v, dict):
        for k in v:
            _digest('%s.%s' % (name, k), v[k])
    elif isinstance(v, (list, tuple)):
        for i, e in enumerate(v):
            _digest('%s.%d' % (name, i), e)
    elif torch.is_tensor(v):
        a = v.detach().cpu().contiguous().numpy()
        lines.append('= %s %s %s %s' % (name, a.dtype, tuple(a.shape), hashlib.sha256(a.tobytes()).hexdigest()))
    elif isinstance(v, np.ndarray):
        lines.append('= %s %s %s %s' % (name, v.dtype, tuple(v.shape), hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()))
    else:
        lines.append('= %s %r' % (name, v))


def sampling_passes(tag, cfg, x, state_dict):
    """Every public sampling and evaluation pass once, eager, in eval mode (the last one in train mode, under grad)."""
    from lvae_amd import evaluate
    from lvae_amd.latent import LatentStats
    torch.manual_seed(0)
    model = LadderVAE(**cfg)
    model.load_state_dict(state_dict)
    model.cuda().eval()
    x = x.cuda()
    B, L = int(x.shape[0]), model.n_layers
    h = min(2, B // 2)                       # the two halves of interpolate: x[:2] and x[2:4] where the golden has four images
    mask = evaluate.make_mask('left', 0.5, (B,) + tuple(x.shape[2:])).cuda()

    def run(name, fn, grad=False):
        lines.append('# %s %s' % (tag, name))
        model.noise = PhiloxNoise(seed=42)
        with torch.set_grad_enabled(grad):
            _digest(name, fn())
        torch.cuda.synchronize()

    def decode_top():
        z = model.encode(x)
        return model.decode([None] * (L - 1) + [z[L - 1]])

    def train_forward():
        model.train()
        model.zero_grad()
        out = model(x, n_samples=2)
        (out['ll'].sum() - out['kl_loss']).backward()
        out['grads'] = torch.cat([p.grad.reshape(-1) for _, p in sorted(model.named_parameters()) if p.grad is not None])
        model.eval()
        return out

    run('sample_prior', lambda: model.sample_prior(4))
    run('sample_prior t=0.7', lambda: model.sample_prior(4, temperature=0.7))
    run('sample_prior mode/constant', lambda: model.sample_prior(4, mode_layers=range(1), constant_layers=range(2, L)))
    for k in (0, 1, L):
        run('sample_conditional k=%d' % k, lambda: model.sample_conditional(x, k, 3))
    run('sample_conditional k=1 use_mode', lambda: model.sample_conditional(x, 1, 3, use_mode=True))
    run('sample_conditional k=1 temperatures', lambda: model.sample_conditional(x, 1, 3, temperature=[0.0] + [0.5] * (L - 1)))
    run('encode k=1', lambda: model.encode(x, 1))
    run('encode', lambda: model.encode(x))
    run('decode top forced', decode_top)
    run('interpolate k=1 slerp', lambda: model.interpolate(x[:h], x[h:2 * h], n_steps=3, n_top_layers=1, mode='slerp'))
    run('interpolate k=L lerp', lambda: model.interpolate(x[:h], x[h:2 * h], n_steps=3, n_top_layers=L, mode='lerp'))
    run('interpolate k=L sampled', lambda: model.interpolate(x[:h], x[h:2 * h], n_steps=3, n_top_layers=L, use_mode=False))
    run('inpaint', lambda: model.inpaint(x, mask, n_iters=3, init='noise', final='sample', return_history=True, use_graph=False))
    run('iw_log_likelihood', lambda: evaluate.iw_log_likelihood(model, x, 3, use_graph=False))
    run('test_pass', lambda: evaluate.test_pass(model, [x], 2, noise=PhiloxNoise(seed=42), use_graph=False))
    run('test_pass latent_stats', lambda: evaluate.test_pass(model, [x], 2, noise=PhiloxNoise(seed=42), use_graph=False,
                                                             latent_stats=LatentStats(model, 'cuda')))
    run('topdown_pass', lambda: model.topdown_pass(model.bottomup_pass(model.pad_input(x))))
    run('train forward n_samples=2 + backward', train_forward, grad=True)


def main(path):
    _C.call = kernels.call = _logged_call
    passes('cifar15', configs.CIFAR15, 256, 'f32')
    passes('cifar15', configs.CIFAR15, 256, 'bf16')
    passes('mnist3', configs.MNIST3, 64, 'f32')
    for name in ('tiny_cifar', 'tiny_mnist', 'tiny_bacdbac', 'tiny_cabdcabd', 'tiny_nobn_selu'):
        g = load_golden(name)
        passes(name, g.cfg, g.t('x').shape[0], 'f32', g.state_dict())
    for name in ('tiny_cifar', 'tiny_mnist', 'tiny_cabdcabd'):
        g = load_golden(name)
        sampling_passes(name, g.cfg, g.t('x'), g.state_dict())
    text = '\n'.join(lines) + '\n'
    with open(path, 'w') as f:
        f.write(text)
    print('%s: %d lines, sha256 %s' % (path, len(lines), hashlib.sha256(text.encode()).hexdigest()))


if __name__ == '__main__':
    main(sys.argv[1])
