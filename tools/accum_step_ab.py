"""What an optimizer step over M micro-batches costs: python tools/accum_step_ab.py [--pairs P] [--steps K] [--out FILE]
bench.py's headline workload (CIFAR-15, fp32, captured step) at 256 images per optimizer step, in three forms on one model, each with its own
optimizer and its own captured step: A the plain step at batch 256, B accum_steps=2 at micro-batches of 128, C accum_steps=4 at
micro-batches of 64. By arithmetic B and C cost M plain passes at the smaller batch, one arena pass for zero_grad (which A pays too) and M
one-wave launches; how much of B - A and C - A the smaller per-pass batch explains is read off two more forms, the plain step at batch 128
(D) and at batch 64 (E): M x D and M x E are what the passes alone cost at that size, optimizer launch included M times instead of once.
All forms train the same weights. After every form is warmed up and captured, P rounds are run; in every round each form runs K steps
between two device events, in the order A, B, C, D, E, so that whatever else the box does falls on all of them.
Writes every round and the medians to FILE (profiles/accum_step_ab.txt).
Measurement tooling only; bench.py has no such flag and stays the yardstick."""
import argparse
import os
import statistics
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import torch  # noqa: E402

import lvae_amd  # noqa: E402,F401
from lvae_amd.configs import CIFAR15, synthetic_images  # noqa: E402
from lvae_amd.engine import TrainStep  # noqa: E402
from lvae_amd.models.lvae import LadderVAE  # noqa: E402
from lvae_amd.noise import PhiloxNoise  # noqa: E402
from lvae_amd.optim import Adamax  # noqa: E402


def timed(step, ring, k):
    """ms per step of k steps between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for i in range(k):
        step(ring[i % len(ring)])
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--images', type=int, default=256, help='images per optimizer step of A, B and C')
    ap.add_argument('--out', default=os.path.join(root, 'profiles', 'accum_step_ab.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('this measurement needs the GPU: nothing is timed without one')
    if args.images % 4:
        raise SystemExit('--images must divide by 4')
    dev = torch.device('cuda', 0)
    gen = torch.Generator().manual_seed(1234)
    n = args.images
    rings = {b: [synthetic_images(CIFAR15, b, gen).to(dev) for _ in range(4)] for b in (n, n // 2, n // 4)}
    torch.manual_seed(42)
    model = LadderVAE(**CIFAR15).to(dev)
    model.train()
    model.noise = PhiloxNoise(seed=42, rank=0)
    forms = [('A plain, batch %d' % n, 1, n, n), ('B accum 2 x %d' % (n // 2), 2, n, n), ('C accum 4 x %d' % (n // 4), 4, n, n),
             ('D plain, batch %d' % (n // 2), 1, n // 2, n // 2), ('E plain, batch %d' % (n // 4), 1, n // 4, n // 4)]
    steps = {}
    for name, m, rows, images in forms:
        st = TrainStep(model, Adamax(model, lr=3e-4), use_graph=True, accum_steps=m)
        for i in range(max(args.warmup, 3)):
            st(rings[rows][i % 4])
        assert st.graph_a is not None and (st.graph_p is not None) == (m > 1)
        steps[name] = (st, rings[rows], images)
    rounds = []
    for _ in range(args.pairs):
        rounds.append([timed(st, ring, args.steps) for st, ring, _ in steps.values()])
    names = list(steps)
    lines = ['CIFAR-15 fp32 captured step on %s, one model; %d rounds, in each every form runs %d steps between two device events.'
             % (torch.cuda.get_device_name(0), args.pairs, args.steps), 'ms per optimizer step:', '']
    for i, r in enumerate(rounds):
        lines.append('  round %d   ' % (i + 1) + '   '.join('%s %.3f' % (nm.split()[0], t) for nm, t in zip(names, r)))
    med = [statistics.median(r[j] for r in rounds) for j in range(len(names))]
    spread = [max(r[j] for r in rounds) - min(r[j] for r in rounds) for j in range(len(names))]
    lines += ['', 'medians:']
    for nm, t, s in zip(names, med, spread):
        lines.append('  %-24s %8.3f ms/step   %8.0f img/s   (spread over the rounds, max - min: %.3f ms)' % (nm, t, steps[nm][2] / t * 1e3, s))
    a, b, c, d, e = med
    lines += ['', 'against the plain step at batch %d (A):' % n,
              '  B / A = %.3f (B - A %+.3f ms); two plain steps at batch %d cost 2 x D = %.3f ms = %.3f x A, so the smaller per-pass batch'
              % (b / a, b - a, n // 2, 2 * d, 2 * d / a),
              '    explains %+.3f ms of B - A and the accumulation itself (prologue, folds, one optimizer launch instead of two) %+.3f ms'
              % (2 * d - a, b - 2 * d),
              '  C / A = %.3f (C - A %+.3f ms); four plain steps at batch %d cost 4 x E = %.3f ms = %.3f x A, so the smaller per-pass batch'
              % (c / a, c - a, n // 4, 4 * e, 4 * e / a),
              '    explains %+.3f ms of C - A and the accumulation itself (prologue, folds, one optimizer launch instead of four) %+.3f ms'
              % (4 * e - a, c - 4 * e)]
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
