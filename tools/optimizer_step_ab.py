"""Step time under Adam against Adamax, and the two optimizer launches alone: python tools/optimizer_step_ab.py [--pairs P] [--steps K] [--out FILE]
bench.py's headline workload (CIFAR-15, fp32, batch 256, captured step) with two optimizers on one model, each with its own captured step:
A the plain Adamax (the default path), B the plain Adam. Both train the same weights, so they share the model's buffers and transformed-weight
table and differ in the optimizer launch alone. After both are warmed up and captured, P pairs of K timed steps each are run alternately
(A, B, A, B, ...), so that whatever else the box does falls on both.
Then the two launches alone, on buffers of their own of the arena's size: both warmed up, R rounds alternated (A, B, A, B, ...), each round L
launches between two device events. Both rules read four arrays and write three, so by arithmetic they cost the same; Adam adds two double
pow and a double sqrt per thread before the loop and an IEEE sqrt and a second division per element. The same once more at one sweep of
the full grid, so that a line through the two sizes separates the prologue's share of the difference from the element loop's.
Writes every pair, every round and the medians to FILE (profiles/optimizer_step_ab.txt).
Measurement tooling only; bench.py has no such flag and stays the yardstick."""
import argparse
import os
import statistics
import sys
import time

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import torch  # noqa: E402

import lvae_amd  # noqa: E402,F401
from lvae_amd import kernels as K  # noqa: E402
from lvae_amd.configs import CIFAR15, synthetic_images  # noqa: E402
from lvae_amd.engine import TrainStep  # noqa: E402
from lvae_amd.models.lvae import LadderVAE  # noqa: E402
from lvae_amd.noise import PhiloxNoise  # noqa: E402
from lvae_amd.optim import Adam, Adamax  # noqa: E402


def timed(step, ring, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(k):
        step(ring[i % len(ring)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


def launches_alone(n, dev, rounds, per_round):
    """[(adamax us, adam us)] per round: `per_round` launches of each rule between two device events, on buffers of their own."""
    gen = torch.Generator().manual_seed(7)
    g = torch.randn(n, generator=gen).to(dev)
    bufs = {}
    for rule in ('adamax', 'adam'):
        bufs[rule] = (torch.randn(n, generator=gen).to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev),
                      torch.zeros(1, dtype=torch.int64, device=dev))

    def launch(rule):
        p, m, s, count = bufs[rule]
        if rule == 'adamax':
            K.adamax_step(p, g, m, s, None, 3e-4, 0.9, 0.999, 1e-8, 0.0, None, count)
        else:
            K.adam_step(p, g, m, s, None, 3e-4, None, 0.9, 0.999, 1e-8, 0.0, False, None, count)
        K.counter_advance(count)

    def events(rule):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per_round):
            launch(rule)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / per_round * 1e3       # (includes the counter's own one-thread launch, the same for both)

    for rule in bufs:
        events(rule)
    return [(events('adamax'), events('adam')) for _ in range(rounds)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=5)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(root, 'profiles', 'optimizer_step_ab.txt'))
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
    n = model.pack().n_train
    steps = {'A adamax': TrainStep(model, Adamax(model, lr=3e-4), use_graph=True),
             'B adam': TrainStep(model, Adam(model, lr=3e-4), use_graph=True)}
    for st in steps.values():
        for i in range(max(args.warmup, 3)):
            st(ring[i % 8])
        assert st.graph_a is not None
    rows = []
    for _ in range(args.pairs):
        rows.append([timed(st, ring, args.steps) for st in steps.values()])
    lines = ['CIFAR-15 fp32 batch %d captured step, plain Adamax (A) against plain Adam (B), one model, on %s.'
             % (args.batch, torch.cuda.get_device_name(0)),
             '%d interleaved pairs of %d timed steps (host clock around a synchronised window), ms/step:' % (args.pairs, args.steps), '']
    lines += ['  pair %d   A %.3f   B %.3f   B - A %+.3f' % (i + 1, a, b, b - a) for i, (a, b) in enumerate(rows)]
    ma, mb = statistics.median(r[0] for r in rows), statistics.median(r[1] for r in rows)
    lines += ['', '  median   A %.3f   B %.3f   B - A %+.3f ms (%+.2f %%)' % (ma, mb, mb - ma, (mb - ma) / ma * 100),
              '  spread of A over the pairs (max - min): %.3f ms' % (max(r[0] for r in rows) - min(r[0] for r in rows)), '']
    alone = launches_alone(n, dev, args.rounds, args.launches)
    lines += ['The optimizer launch alone over %d elements (the arena\'s trainable prefix; four arrays read, three written: %.1f MB per launch),'
              % (n, 7 * 4 * n / 1e6),
              '%d alternated rounds of %d launches between two device events, us/launch (with the step counter\'s one-thread launch):'
              % (args.rounds, args.launches), '']
    lines += ['  round %d   adamax %.2f   adam %.2f   adam - adamax %+.2f' % (i + 1, a, b, b - a) for i, (a, b) in enumerate(alone)]
    xa, xb = statistics.median(r[0] for r in alone), statistics.median(r[1] for r in alone)
    lines += ['', '  median   adamax %.2f   adam %.2f   adam - adamax %+.2f us (%+.2f %%)' % (xa, xb, xb - xa, (xb - xa) / xa * 100),
              '  spread of adamax over the rounds (max - min): %.2f us' % (max(r[0] for r in alone) - min(r[0] for r in alone)),
              '  at the medians: adamax %.0f GB/s, adam %.0f GB/s' % (7 * 4 * n / xa / 1e3, 7 * 4 * n / xb / 1e3), '']
    # one sweep of the full grid (2048 blocks x 256 threads x 4 elements): every thread runs its prologue and one iteration, so the
    # difference there is the prologue's plus one seventh of the arena's per-element share; two sizes separate the two
    n1 = 2048 * 256 * 4
    small = launches_alone(n1, dev, args.rounds, args.launches)
    sa, sb = statistics.median(r[0] for r in small), statistics.median(r[1] for r in small)
    per_elem = ((xb - xa) - (sb - sa)) / (n - n1)
    lines += ['The same over %d elements, one sweep of the full grid: median adamax %.2f   adam %.2f   adam - adamax %+.2f us'
              % (n1, sa, sb, sb - sa),
              '  spread of adamax over the rounds (max - min): %.2f us' % (max(r[0] for r in small) - min(r[0] for r in small)),
              '  a line through the two sizes: %+.2f us per launch whatever its size (the prologue: two double pow and a double sqrt in'
              % ((sb - sa) - per_elem * n1),
              '  each of 524288 threads) and %+.2f us over the arena from the element loop (sqrt and a second division per element)'
              % (per_elem * n)]
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
