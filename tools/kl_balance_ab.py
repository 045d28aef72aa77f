"""Cost of KL balancing: python tools/kl_balance_ab.py [--rounds R] [--steps K] [--parent DIR] [--out FILE]
Three measurements, written to FILE (profiles/kl_balance_ab.txt):

1. Flag off, with --parent DIR (a built tree of the parent commit): bench.py of this tree against bench.py of DIR, three interleaved pairs
   of processes. Without --parent this part says "not measured".
2. Flag on against off. bench.py's headline workload (CIFAR-15, fp32, batch 256, captured step) under a KL warm-up longer than the run
   (beta < 1 at every step, so the rule is active), two captured steps on one model: A the plain step, B with KlBalance('square'), which
   replaces the one-workgroup KL bookkeeping launch and its backward by the balanced ones. After both are warmed up and captured, R rounds
   of K steps each are run alternately (A, B, A, B, ...), each round between two device events.
3. The two launches alone against the ones they replace, on a (15, 256) matrix: N launches between two device events each.
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
from lvae_amd import kernels as K  # noqa: E402
from lvae_amd.balance import KlBalance  # noqa: E402
from lvae_amd.configs import CIFAR15, synthetic_images  # noqa: E402
from lvae_amd.engine import TrainStep  # noqa: E402
from lvae_amd.models.lvae import LadderVAE  # noqa: E402
from lvae_amd.noise import PhiloxNoise  # noqa: E402
from lvae_amd.optim import Adamax  # noqa: E402

ANNEAL = 10 ** 6   # longer than any run here: beta < 1 throughout


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
    tree = os.path.abspath(tree)   # (the process runs in `tree`: a relative DIR would be looked up from there)
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
    ap.add_argument('--rule', default='square')
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--parent', default='', help='a built tree of the parent commit: bench.py there against bench.py here')
    ap.add_argument('--bench-steps', type=int, default=30, dest='bench_steps')
    ap.add_argument('--out', default=os.path.join(root, 'profiles', 'kl_balance_ab.txt'))
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
    model.pack()
    kb = KlBalance(args.rule)
    steps = {}
    for name, balance in (('A plain', None), ('B balanced', kb)):   # A is captured before B's constructor sets the model's property
        st = steps[name] = TrainStep(model, Adamax(model, lr=3e-4), use_graph=True, beta_anneal=ANNEAL, kl_balance=balance)
        for i in range(max(args.warmup, 3)):
            st(ring[i % 8])
        assert st.graph_a is not None
    rows = [[timed(st, ring, args.steps) for st in steps.values()] for _ in range(args.rounds)]
    coeff = kb.coeff.tolist()
    lines += ['CIFAR-15 fp32 batch %d captured step under a KL warm-up longer than the run, plain (A) against the same step with '
              '--kl-balance %s (B), one model, on %s.' % (args.batch, args.rule, torch.cuda.get_device_name(0)),
              '%d interleaved rounds of %d steps, each round between two device events, ms/step:' % (args.rounds, args.steps), '']
    lines += ['  round %d   A %.3f   B %.3f   B - A %+.3f' % (i + 1, a, b, b - a) for i, (a, b) in enumerate(rows)]
    ma, mb = statistics.median(r[0] for r in rows), statistics.median(r[1] for r in rows)
    lines += ['', '  median   A %.3f   B %.3f   B - A %+.3f ms (%+.2f %%)' % (ma, mb, mb - ma, (mb - ma) / ma * 100),
              '  spread of A over the rounds (max - min): %.3f ms' % (max(r[0] for r in rows) - min(r[0] for r in rows)),
              '  coefficients of B\'s last step: %.4g..%.4g' % (min(coeff), max(coeff)), '']
    # the launches alone
    L, N = len(CIFAR15['z_dims']), args.batch
    kl = (torch.randn(L, N, generator=torch.Generator().manual_seed(5)) + 0.5).to(dev)
    g_scal = torch.tensor([0.5, 0.0], device=dev)
    t_pf = launches(lambda: K.kl_bookkeeping_fwd(kl, 1.0), args.launches)
    t_bf = launches(lambda: K.kl_balance_fwd(kl, 1.0, kb.alpha, beta=0.5), args.launches)
    t_pb = launches(lambda: K.kl_bookkeeping_bwd(kl, 1.0, None, None, g_scal), args.launches)
    t_bb = launches(lambda: K.kl_balance_bwd(kl, 1.0, kb.coeff, None, None, g_scal), args.launches)
    lines += ['The launches alone on a (%d, %d) matrix, %d launches between two device events each (with the output allocations of the '
              'Python binding):' % (L, N, args.launches),
              '  forward    plain %.1f us   balanced %.1f us   (one workgroup each; the balanced one sweeps the matrix twice and sums |kl| too)'
              % (t_pf, t_bf),
              '  backward   plain %.1f us   balanced %.1f us' % (t_pb, t_bb)]
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
