"""Test-pass time with the latent statistics on: python tools/latent_stats_ab.py [--pairs P] [--batches K] [--batch B] [--samples S] [--out FILE]
Interleaved pairs of evaluate.test_pass on bench.py's CIFAR-15 model (fp32, one GPU, captured sample graphs) without and with a
latent.LatentStats, in ONE process on ONE model: both forms are warmed up (their graphs captured), then P times: one timed pass of K
batches of B images without the object, one with it. A timed pass ends in its device-to-host copy, so the host clock around it covers
all of its work. Prints each pair, the medians, the median difference and ratio, and the spread of the plain pass in those same pairs.
Measurement tooling only (profiles/latent_stats_ab.txt)."""
import argparse
import os
import statistics
import sys
import time

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import torch  # noqa: E402

import bench  # noqa: E402  (imports the package)
from lvae_amd.evaluate import test_pass  # noqa: E402
from lvae_amd.latent import LatentStats  # noqa: E402
from lvae_amd.models.lvae import LadderVAE  # noqa: E402
from lvae_amd.noise import PhiloxNoise  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=6)
    ap.add_argument('--batches', type=int, default=4)
    ap.add_argument('--batch', type=int, default=1000)
    ap.add_argument('--samples', type=int, default=1)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    torch.manual_seed(42)
    model = LadderVAE(**bench.CIFAR15).to(dev)
    model.train()
    model.noise = PhiloxNoise(seed=42)
    model.pack()
    stats = LatentStats(model, dev)
    noise = PhiloxNoise(seed=7)
    xs = [b.to(dev) for b in bench.synth_batches(args.batches, args.batch, 1234)]
    forms = {'plain': None, 'latent': stats}

    def one(tag):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        res = test_pass(model, xs, args.samples, noise=noise, latent_stats=forms[tag])
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, res

    for tag in forms:                                # captures the plan of each form, then one replayed pass
        one(tag)
        one(tag)
    lines = ['# ms per test pass of %d batches x %d images, %d sample(s) per image, interleaved in one process' % (
        args.batches, args.batch, args.samples), '# pair   plain   latent   difference']
    ms = {'plain': [], 'latent': []}
    res = None
    for p in range(args.pairs):
        for tag in forms:
            dt, r = one(tag)
            ms[tag].append(dt)
            res = r if tag == 'latent' else res
        lines.append('%4d   %9.3f   %9.3f   %+9.3f' % (p, ms['plain'][-1], ms['latent'][-1], ms['latent'][-1] - ms['plain'][-1]))
    diffs = [b - a for a, b in zip(ms['plain'], ms['latent'])]
    mp, ml = statistics.median(ms['plain']), statistics.median(ms['latent'])
    lines.append('median plain %.3f ms   median latent %.3f ms   median difference %+.3f ms   ratio of medians %.4f' % (
        mp, ml, statistics.median(diffs), ml / mp))
    lines.append('spread of the plain pass over the pairs: min %.3f   max %.3f   (max - min %.3f ms)' % (
        min(ms['plain']), max(ms['plain']), max(ms['plain']) - min(ms['plain'])))
    L = len(bench.CIFAR15['z_dims'])
    row = [2 * stats.units(i) * 4 for i in range(L)]   # bytes of one image's (mu | logvar) tensor of layer i
    folded = sum(args.batch * r + (r if i == L - 1 else args.batch * r) for i, r in enumerate(row))   # q, and p (the top prior once)
    lines.append('bytes the folds read per batch (p and q of %d layers, fp32, top prior once): %.1f MB' % (L, folded / 1e6))
    lines.append('active units of the last pass (untrained weights): KL %d, variance %d of %d' % (
        res['latent/active_kl'], res['latent/active_var'], sum(stats.units(i) for i in range(L))))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
