"""Step time with the log summary on: python tools/summary_step_ab.py [--pairs P] [--steps K] [--warmup W] [--batch B] [--out FILE]
Interleaved pairs of bench.py's CIFAR-15 step (batch 256, fp32, one GPU, captured) without and with a summary.TrainSummary, in ONE process
on ONE model: two TrainSteps share the model and the optimizer (every step of either is a real training step), each is warmed up and
captured, then P times: K timed steps of the plain step, K timed steps of the step that folds. Prints each pair, the medians, the median
difference and the run-to-run spread of the plain step in those same pairs. bench.py itself has no such switch and stays the yardstick.
Measurement tooling only (profiles/summary_step_ab.txt)."""
import argparse
import os
import statistics
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import torch  # noqa: E402

import bench  # noqa: E402  (imports the package)
from lvae_amd.engine import TrainStep  # noqa: E402
from lvae_amd.models.lvae import LadderVAE  # noqa: E402
from lvae_amd.noise import PhiloxNoise  # noqa: E402
from lvae_amd.optim import Adamax  # noqa: E402
from lvae_amd.summary import TrainSummary  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=8)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    torch.manual_seed(42)
    model = LadderVAE(**bench.CIFAR15).to(dev)
    model.train()
    model.noise = PhiloxNoise(seed=42)
    model.pack()
    opt = Adamax(model, lr=3e-4)
    summ = TrainSummary(len(bench.CIFAR15['z_dims']), dev)
    steps = {'plain': TrainStep(model, opt, use_graph=True), 'summary': TrainStep(model, opt, use_graph=True, summary=summ)}
    ring = [b.to(dev) for b in bench.synth_batches(8, args.batch, 1234)]
    for st in steps.values():
        for i in range(max(args.warmup, 3)):   # >= 3: two eager steps + the capture replay
            st(ring[i % 8])
    lines = ['# ms/step, %d timed steps per entry, batch %d, interleaved in one process' % (args.steps, args.batch),
             '# pair   plain   summary   difference']
    ms = {'plain': [], 'summary': []}
    for p in range(args.pairs):
        for tag, st in steps.items():
            dt, _ = bench.time_steps(st, ring, args.steps, 1, dev)
            ms[tag].append(dt / args.steps * 1e3)
        summ.take()                             # what a log line does, once per pair, outside the timed windows
        lines.append('%4d   %8.4f   %8.4f   %+8.4f' % (p, ms['plain'][-1], ms['summary'][-1], ms['summary'][-1] - ms['plain'][-1]))
    diffs = [b - a for a, b in zip(ms['plain'], ms['summary'])]
    lines.append('median plain %.4f ms   median summary %.4f ms   median difference %+.4f ms (%+.3f %%)' % (
        statistics.median(ms['plain']), statistics.median(ms['summary']), statistics.median(diffs),
        100.0 * statistics.median(diffs) / statistics.median(ms['plain'])))
    lines.append('spread of the plain step over the pairs: min %.4f   max %.4f   (max - min %.4f ms)' % (
        min(ms['plain']), max(ms['plain']), max(ms['plain']) - min(ms['plain'])))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
