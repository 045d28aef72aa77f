"""Cost of the spectral regulariser: python tools/spectral_reg_ab.py [--rounds R] [--steps K] [--parent DIR] [--out FILE]
Three measurements, written to FILE (profiles/spectral_reg_ab.txt):

1. Flag on against off. bench.py's headline workload (CIFAR-15, fp32, batch 256, captured step) with two optimizers on one model, each
   with its own captured step: A the plain Adamax (the default path), B with a SpectralReg(lam) on it, which pays for the power-iteration
   launch over every convolution weight and the reduce of the sigmas. After both are warmed up and captured, R rounds of K steps each are
   run alternately (A, B, A, B, ...), each round between two device events.
2. The launch alone, over the same model's table: N launches between two device events, with the bytes it has to move (every weight matrix
   read once from HBM: the second pass finds it in L2; its gradient slot read and written) and the share of 6.29 TB/s that makes; the
   shape of the table beside it (entries, the largest, the one-workgroup-per-matrix critical path). The iterate-only launch likewise.
3. Flag off, with --parent DIR (a built tree of the parent commit): bench.py of this tree against bench.py of DIR, three interleaved pairs
   of processes. Without --parent this part says "not measured".
Measurement tooling only; bench.py has no such flag and stays the yardstick."""
import argparse
import json
import os
import statistics
import subprocess
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
from lvae_amd.spectral import SpectralReg  # noqa: E402

HBM_COPY = 6.29e12   # bytes/s a streaming copy reaches on this part


def timed(step, ring, k):
    """ms/step of k steps between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for i in range(k):
        step(ring[i % len(ring)])
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / k


def launches(fn, n):
    """us/launch of n calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def bench_value(tree, steps, warmup):
    p = subprocess.run([sys.executable, os.path.join(tree, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup)],
                       cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=900)
    if p.returncode != 0:
        raise SystemExit('bench.py in %s failed (%d)' % (tree, p.returncode))
    return float(json.loads(p.stdout.decode().strip().splitlines()[-1])['value'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--lam', type=float, default=0.01)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--parent', default='', help='a built tree of the parent commit: bench.py there against bench.py here')
    ap.add_argument('--bench-steps', type=int, default=30, dest='bench_steps')
    ap.add_argument('--out', default=os.path.join(root, 'profiles', 'spectral_reg_ab.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('this measurement needs the GPU: nothing is timed without one')
    lines = []
    if args.parent:   # first, in processes of their own, before this one holds the device's memory
        pairs = [(bench_value(args.parent, args.bench_steps, 5), bench_value(root, args.bench_steps, 5)) for _ in range(3)]
        lines += ['Flag off: bench.py --gpus 1 --steps %d --warmup 5, the parent commit (P) against this tree (T), three interleaved pairs of '
                  'processes, images/s:' % args.bench_steps, '']
        lines += ['  pair %d   P %.1f   T %.1f   T - P %+.1f' % (i + 1, p, t, t - p) for i, (p, t) in enumerate(pairs)]
        mp, mt = statistics.median(p for p, _ in pairs), statistics.median(t for _, t in pairs)
        lines += ['', '  median   P %.1f   T %.1f   T - P %+.1f images/s (%+.2f %%); spread of P over the pairs (max - min): %.1f images/s'
                  % (mp, mt, mt - mp, (mt - mp) / mp * 100, max(p for p, _ in pairs) - min(p for p, _ in pairs)), '']
    else:
        lines += ['Flag off against the parent commit: not measured (no --parent tree given). Without the flag the step calls the entry points '
                  'it called before and issues the launches it issued before.', '']
    dev = torch.device('cuda', 0)
    gen = torch.Generator().manual_seed(1234)
    ring = [synthetic_images(CIFAR15, args.batch, gen).to(dev) for _ in range(8)]
    torch.manual_seed(42)
    model = LadderVAE(**CIFAR15).to(dev)
    model.train()
    model.noise = PhiloxNoise(seed=42, rank=0)
    arena = model.pack()
    sr = SpectralReg(args.lam, warm_iters=10, seed=42)
    steps = {'A plain': TrainStep(model, Adamax(model, lr=3e-4), use_graph=True),
             'B spectral': TrainStep(model, Adamax(model, lr=3e-4, spectral=sr), use_graph=True)}
    for st in steps.values():
        for i in range(max(args.warmup, 3)):
            st(ring[i % 8])
        assert st.graph_a is not None
    rows = [[timed(st, ring, args.steps) for st in steps.values()] for _ in range(args.rounds)]
    lines += ['CIFAR-15 fp32 batch %d captured step, plain Adamax (A) against the same step with --spectral-reg %g (B), one model, on %s.'
              % (args.batch, args.lam, torch.cuda.get_device_name(0)),
              '%d interleaved rounds of %d steps, each round between two device events, ms/step:' % (args.rounds, args.steps), '']
    lines += ['  round %d   A %.3f   B %.3f   B - A %+.3f' % (i + 1, a, b, b - a) for i, (a, b) in enumerate(rows)]
    ma, mb = statistics.median(r[0] for r in rows), statistics.median(r[1] for r in rows)
    lines += ['', '  median   A %.3f   B %.3f   B - A %+.3f ms (%+.2f %%)' % (ma, mb, mb - ma, (mb - ma) / ma * 100),
              '  spread of A over the rounds (max - min): %.3f ms' % (max(r[0] for r in rows) - min(r[0] for r in rows)),
              '  sum / max of the spectral norms after B\'s last step: %.5g / %.5g' % (float(sr.sr_sum), float(sr.sr_max)), '']
    # the launch alone
    shapes = sr.shapes
    w_bytes = 4 * sum(k * c for k, c in shapes)
    vec_bytes = 4 * sum(2 * c + k for k, c in shapes)
    t_step = launches(lambda: sr.step(model), args.launches)
    sr.open = False
    t_iter = launches(sr.iterate, args.launches)
    t_red = launches(sr.finish, args.launches)
    need_step, need_iter = 3 * w_bytes + vec_bytes, w_bytes + vec_bytes
    kmax = max(shapes, key=lambda s: s[0] * s[1])
    lines += ['The launches alone, over this model\'s table, %d launches between two device events each:' % args.launches,
              '  table: %d matrices, %.2f MB of weights (arena: %.1f MB), K from %d to %d, Cout from %d to %d, largest %dx%d (%.0f KB)'
              % (len(shapes), w_bytes / 1e6, arena.params.numel() * 4 / 1e6, min(k for k, _ in shapes), max(k for k, _ in shapes),
                 min(c for _, c in shapes), max(c for _, c in shapes), kmax[0], kmax[1], kmax[0] * kmax[1] * 4 / 1e3),
              '  step (iterate + gradient)   %.1f us; HBM bytes it needs: weights once %.2f MB + gradient slots read and written %.2f MB + '
              'vectors %.2f MB = %.2f MB -> %.0f GB/s, %.1f %% of 6.29 TB/s (the weights are read twice: the second pass finds them in L2)'
              % (t_step, w_bytes / 1e6, 2 * w_bytes / 1e6, vec_bytes / 1e6, need_step / 1e6, need_step / t_step / 1e3,
                 need_step / (t_step * 1e-6) / HBM_COPY * 100),
              '  iterate only                %.1f us; %.2f MB -> %.0f GB/s, %.1f %% of 6.29 TB/s'
              % (t_iter, need_iter / 1e6, need_iter / t_iter / 1e3, need_iter / (t_iter * 1e-6) / HBM_COPY * 100),
              '  reduce of the sigmas        %.1f us' % t_red,
              '  one workgroup owns a matrix from its first load to its last store: %d workgroups of 512 threads over 256 CUs, so the launch '
              'lasts as long as its largest matrices take one workgroup, not as long as the bytes take the chip.' % len(shapes)]
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
