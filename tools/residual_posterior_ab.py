"""What --residual-posterior costs: python tools/residual_posterior_ab.py [--pairs P] [--steps K] [--out FILE]
1. bench.py's headline workload (CIFAR-15, fp32, batch 256, captured step) on two models with the same weights, A absolute and B with
   residual_posterior set, each with its own optimizer and its own captured step. By arithmetic the residual core moves the bytes of the
   absolute one (q_out is not written in training), and the levels of 8x8 and below lose their one-launch stochastic block: four launches
   instead of one, each way. After both are warmed up and captured, P rounds are run; in every round each form runs K steps between two
   device events, A then B, so that whatever else the box does falls on both.
2. The core alone at 256 x 256 x 32 (N x HW x Z, the 16x16 level of that model): forward and backward of the absolute and of the residual
   entry points, interleaved the same way, with the HBM bytes each call has to move (computed from the shapes: every tensor read or
   written once) over its time.
Writes every round and the medians to FILE (profiles/residual_posterior_ab.txt).
Measurement tooling only; bench.py has no such flag and stays the yardstick."""
import argparse
import os
import statistics
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import torch  # noqa: E402

import lvae_amd  # noqa: E402,F401
from lvae_amd import kernels as K  # noqa: E402
from lvae_amd.configs import CIFAR15, synthetic_images  # noqa: E402
from lvae_amd.engine import TrainStep  # noqa: E402
from lvae_amd.models.lvae import LadderVAE  # noqa: E402
from lvae_amd.noise import PhiloxNoise  # noqa: E402
from lvae_amd.optim import Adamax  # noqa: E402

HBM_ACHIEVABLE = 6.29e12   # bytes/s


def timed(fn, k):
    """ms per call of k calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for i in range(k):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / k


def med_spread(rounds, j):
    col = [r[j] for r in rounds]
    return statistics.median(col), max(col) - min(col)


def step_ab(args, dev, lines):
    gen = torch.Generator().manual_seed(1234)
    ring = [synthetic_images(CIFAR15, args.batch, gen).to(dev) for _ in range(4)]
    steps = {}
    for name, residual in (('A absolute', False), ('B residual', True)):
        torch.manual_seed(42)
        model = LadderVAE(**CIFAR15).to(dev)
        model.train()
        model.noise = PhiloxNoise(seed=42, rank=0)
        model.residual_posterior = residual
        st = TrainStep(model, Adamax(model, lr=3e-4), use_graph=True)
        for i in range(max(args.warmup, 3)):
            st(ring[i % 4])
        assert st.graph_a is not None   # captured
        steps[name] = st
    rounds = [[timed(lambda i, st=st: st(ring[i % 4]), args.steps) for st in steps.values()] for _ in range(args.pairs)]
    lines += ['CIFAR-15 fp32 captured step, batch %d, on %s; %d rounds, in each every form runs %d steps between two device events.'
              % (args.batch, torch.cuda.get_device_name(0), args.pairs, args.steps), 'ms per step:', '']
    for i, r in enumerate(rounds):
        lines.append('  round %d   ' % (i + 1) + '   '.join('%s %.3f' % (nm.split()[0], t) for nm, t in zip(steps, r)))
    lines += ['', 'medians:']
    med = []
    for j, nm in enumerate(steps):
        m, s = med_spread(rounds, j)
        med.append(m)
        lines.append('  %-12s %8.3f ms/step   %8.0f img/s   (spread over the rounds, max - min: %.3f ms)' % (nm, m, args.batch / m * 1e3, s))
    lines += ['', '  B / A = %.4f (B - A %+.3f ms per step)' % (med[1] / med[0], med[1] - med[0]), '']


def core_ab(args, dev, lines):
    N, H, W, Z = 256, 16, 16, 32
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    p, q, d = r(N, H, W, 2 * Z), r(N, H, W, 2 * Z), 0.5 * r(N, H, W, 2 * Z)
    eps, dz = r(N, H, W, Z), r(N, H, W, Z)
    gl = [r(N), r(N), r(N), r(N, H, W)]
    z = K.normal_stochastic_fwd(p, q, eps, 0, False, Z, N)[0]
    el = N * H * W * Z * 4   # bytes of one [N,HW,Z] tensor; the [N] and [N,HW] tensors are left out (under 1 %)
    forms = {
        'fwd absolute': (lambda i: K.normal_stochastic_fwd(p, q, eps, 0, False, Z, N), 6 * el),                       # p, q 2+2, eps, z
        'fwd residual': (lambda i: K.normal_stochastic_res_fwd(p, d, eps, 0, False, Z, N, need_q=False), 6 * el),    # p, d 2+2, eps, z
        'bwd absolute': (lambda i: K.normal_stochastic_bwd(p, q, eps, z, dz, *gl, 0, False, Z), 11 * el),            # p, q, eps, z, dz, dp, dq
        'bwd residual': (lambda i: K.normal_stochastic_res_bwd(p, d, eps, None, dz, *gl, 0, False, Z), 10 * el),     # p, d, eps, dz, dp, dd
    }
    for fn, _ in forms.values():
        for i in range(5):
            fn(i)
    rounds = [[timed(fn, args.core_calls) for fn, _ in forms.values()] for _ in range(args.pairs)]
    lines += ['The core alone at %d x %d x %d (N x HW x Z), mode 0, Monte-Carlo KL, allocations of the outputs included; %d rounds of %d calls.'
              % (N, H * W, Z, args.pairs, args.core_calls), 'Bytes: every [N,HW,Z] tensor the call reads or writes, once.', '']
    for j, (nm, (_, nbytes)) in enumerate(forms.items()):
        m, s = med_spread(rounds, j)
        rate = nbytes / (m * 1e-3)
        lines.append('  %-14s %8.2f us   (spread %.2f us)   %6.1f MB   %5.2f TB/s = %4.1f %% of the %.2f TB/s achievable'
                     % (nm, m * 1e3, s * 1e3, nbytes / 1e6, rate / 1e12, 100 * rate / HBM_ACHIEVABLE, HBM_ACHIEVABLE / 1e12))
    lines.append('')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--core-calls', type=int, default=200, dest='core_calls')
    ap.add_argument('--out', default=os.path.join(root, 'profiles', 'residual_posterior_ab.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('this measurement needs the GPU: nothing is timed without one')
    dev = torch.device('cuda', 0)
    lines = []
    step_ab(args, dev, lines)
    core_ab(args, dev, lines)
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
