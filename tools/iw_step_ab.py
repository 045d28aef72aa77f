"""Step time of training on the K-sample importance-weighted bound: python tools/iw_step_ab.py [--pairs P] [--steps S] [--k K] [--batch B] [--out FILE]
The CIFAR-15 architecture (fp32, captured step, no free bits: the bound has none) with two steps on one model, each with its own captured
graph: A the plain ELBO step at batch K * B (256), B the importance-weighted step with K (4) samples of B (64) images. Both run the
top-down pass, final_top_down and the likelihood on K * B rows; B runs the bottom-up pass on B rows instead of K * B and pays one
broadcast copy per level and its sum going back. After both are warmed up and captured, P pairs of S timed steps each are run alternately
(A, B, A, B, ...), so that whatever else the box does falls on both. Writes every pair and the medians to FILE
(profiles/iw_step_ab.txt). Measurement tooling only; bench.py has no such flag and stays the yardstick."""
import argparse
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
from lvae_amd.optim import Adamax  # noqa: E402


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
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--k', type=int, default=4)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--out', default=os.path.join(root, 'profiles', 'iw_step_ab.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('this measurement needs the GPU: nothing is timed without one')
    dev = torch.device('cuda', 0)
    cfg = dict(CIFAR15, free_bits=0.0)
    gen = torch.Generator().manual_seed(1234)
    rows_a = args.k * args.batch
    rings = {'A': [synthetic_images(cfg, rows_a, gen).to(dev) for _ in range(4)],
             'B': [synthetic_images(cfg, args.batch, gen).to(dev) for _ in range(4)]}
    torch.manual_seed(42)
    model = LadderVAE(**cfg).to(dev)
    model.train()
    model.noise = PhiloxNoise(seed=42, rank=0)
    model.pack()
    steps = {'A': TrainStep(model, Adamax(model, lr=3e-4), use_graph=True),
             'B': TrainStep(model, Adamax(model, lr=3e-4), use_graph=True, iw_samples=args.k)}
    for name, st in steps.items():
        for i in range(max(args.warmup, 3)):
            out = st(rings[name][i % 4])
        assert st.graph_a is not None
    ess = float(out['ess'])
    pairs = []
    for _ in range(args.pairs):
        pairs.append([timed(steps[n], rings[n], args.steps) for n in ('A', 'B')])
    lines = ['CIFAR-15 fp32 captured step without free bits on %s: A the ELBO step at batch %d, B the importance-weighted step with K = %d '
             'samples of %d images' % (torch.cuda.get_device_name(0), rows_a, args.k, args.batch),
             '(the same %d top-down rows; B runs the bottom-up pass on %d). %d interleaved pairs of %d timed steps (host clock around a '
             'synchronised window), ms/step:' % (rows_a, args.batch, args.pairs, args.steps), '']
    lines += ['  pair %d   A %.3f   B %.3f   B - A %+.3f' % (i + 1, a, b, b - a) for i, (a, b) in enumerate(pairs)]
    ma, mb = statistics.median(r[0] for r in pairs), statistics.median(r[1] for r in pairs)
    lines += ['', '  median   A %.3f   B %.3f   B - A %+.3f ms (%+.2f %%)' % (ma, mb, mb - ma, (mb - ma) / ma * 100),
              '  spread of A over the pairs (max - min): %.3f ms' % (max(r[0] for r in pairs) - min(r[0] for r in pairs)),
              '  images per second: A %.0f (of %d rows each one image)   B %.0f (of %d images with %d samples each)'
              % (rows_a / ma * 1e3, rows_a, args.batch / mb * 1e3, args.batch, args.k),
              '  effective sample size of B at its last warm-up step: %.3f of %d' % (ess, args.k)]
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
