"""Step time under the gradient guard: python tools/grad_guard_step_ab.py [--pairs P] [--steps K] [--out FILE]
bench.py's headline workload (CIFAR-15, fp32, batch 256, captured step) with two optimizers on one model, each with its own captured step:
A the plain Adamax (the default path), B under a GradGuard whose limits are never reached (max_norm 1e30, skip_threshold inf), so B applies
the very updates A would and pays for the guard alone: the save of the BatchNorm statistics, one more read of the gradient arena with the
decision, the flagged restore, and the flag reads of the guarded Adamax and its counter. Both train the same weights, so they share the
model's buffers and transformed-weight table. After both are warmed up and captured, P pairs of K timed steps each are run alternately
(A, B, A, B, ...), so that whatever else the box does falls on both. Writes every pair and the medians to FILE (profiles/grad_guard_step_ab.txt).
Measurement tooling only; bench.py has no such flag and stays the yardstick."""
import argparse
import math
import os
import statistics
import sys
import time

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import torch  # noqa: E402

import lvae_amd  # noqa: E402,F401
from lvae_amd.configs import CIFAR15, synthetic_images  # noqa: E402
from lvae_amd.engine import TrainStep  # noqa: E402
from lvae_amd.models.lvae import LadderVAE  # noqa: E402
from lvae_amd.noise import PhiloxNoise  # noqa: E402
from lvae_amd.optim import Adamax, GradGuard  # noqa: E402


def timed(step, ring, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(k):
        step(ring[i % len(ring)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=5)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--out', default=os.path.join(root, 'profiles', 'grad_guard_step_ab.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('this measurement needs the GPU: nothing is timed without one')
    dev = torch.device('cuda', 0)
    gen = torch.Generator().manual_seed(1234)
    ring = [synthetic_images(CIFAR15, args.batch, gen).to(dev) for _ in range(8)]
    torch.manual_seed(42)
    model = LadderVAE(**CIFAR15).to(dev)
    model.train()
    model.noise = PhiloxNoise(seed=42, rank=0)
    model.pack()
    guard = GradGuard(max_norm=1e30, skip_threshold=math.inf)
    steps = {'A plain': TrainStep(model, Adamax(model, lr=3e-4), use_graph=True),
             'B guarded': TrainStep(model, Adamax(model, lr=3e-4, guard=guard), use_graph=True)}
    for st in steps.values():
        for i in range(max(args.warmup, 3)):
            st(ring[i % 8])
        assert st.graph_a is not None
    rows = []
    for _ in range(args.pairs):
        rows.append([timed(st, ring, args.steps) for st in steps.values()])
    lines = ['CIFAR-15 fp32 batch %d captured step, plain Adamax (A) against the same step under an idle gradient guard (B), one model, on %s.'
             % (args.batch, torch.cuda.get_device_name(0)),
             '%d interleaved pairs of %d timed steps (host clock around a synchronised window), ms/step:' % (args.pairs, args.steps), '']
    lines += ['  pair %d   A %.3f   B %.3f   B - A %+.3f' % (i + 1, a, b, b - a) for i, (a, b) in enumerate(rows)]
    ma, mb = statistics.median(r[0] for r in rows), statistics.median(r[1] for r in rows)
    lines += ['', '  median   A %.3f   B %.3f   B - A %+.3f ms (%+.2f %%)' % (ma, mb, mb - ma, (mb - ma) / ma * 100),
              '  spread of A over the pairs (max - min): %.3f ms' % (max(r[0] for r in rows) - min(r[0] for r in rows)),
              '  gradient arena: %.1f MB; clipped / skipped steps of B: %d / %d; norm of B\'s last gradient: %.4g'
              % ((model.arena.grads.numel() * 4 / 1e6,) + guard.counts() + (guard.norm.item(),))]
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
