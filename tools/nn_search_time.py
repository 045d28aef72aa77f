"""Time of the exact nearest-neighbour search (kernels.nn_l2) against torch's matrix form on a float32 copy of the same table.

Not a test. Three shapes: Q = 144 queries against a CIFAR-sized uint8 table (50 000 x 3 072), an MNIST-sized one (60 000 x 784) and a
float32 feature table (50 000 x 2 688). The yardstick is torch.cdist(q, t32).pow(2).topk(k, largest=False) on the same device: it needs the
float32 copy (four times the bytes of a uint8 table) and forms |q|^2 + |t|^2 - 2 q.t, so it is not the same computation, only what a user
would otherwise write. Both forms are warmed up, then timed alternately with device events over `--reps` rounds of `--inner` calls; the
file reports the median and the spread of the rounds, the bytes each form holds, the search's pair-elements per second, and how far the
two forms' distances and neighbours differ.

  python tools/nn_search_time.py [--out profiles/nn_search.txt] [--k 7] [--reps 7] [--inner 5]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [('cifar-sized uint8', 144, 50000, 3072, 'u8'), ('mnist-sized uint8', 144, 60000, 784, 'u8'),
          ('latent float32', 144, 50000, 2688, 'f32')]


def timed(fn, inner):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / inner   # ms per call


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'nn_search.txt'))
    p.add_argument('--k', type=int, default=7)
    p.add_argument('--reps', type=int, default=7)
    p.add_argument('--inner', type=int, default=5)
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('nn_search_time needs the GPU: a CPU run says nothing about it')
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels as K
    dev = torch.device('cuda', 0)
    lines = ['nearest-neighbour search: kernels.nn_l2 (exact form, table searched where it lies) against '
             'torch.cdist(q, t32).pow(2).topk(k, largest=False) (float32 copy of the table)',
             'device %s, k %d, %d rounds of %d calls each, forms alternated; ms per call: median [min, max] of the rounds'
             % (torch.cuda.get_device_name(0), args.k, args.reps, args.inner)]
    for name, Q, N, D, kind in SHAPES:
        gen = torch.Generator().manual_seed(N + D)
        if kind == 'u8':
            table = torch.randint(0, 256, (N, D), dtype=torch.uint8, generator=gen).to(dev)
            t32 = table.float().div_(255.0)
            queries = torch.rand((Q, D), generator=gen).to(dev)
        else:
            table = torch.randn((N, D), generator=gen).to(dev)
            t32 = table
            queries = torch.randn((Q, D), generator=gen).to(dev)

        def ours():
            return K.nn_l2(queries, table, args.k)

        def yard():
            return torch.cdist(queries, t32).pow(2).topk(args.k, largest=False)

        for _ in range(3):
            ours(), yard()
        torch.cuda.synchronize()
        a, b = [], []
        for _ in range(args.reps):
            a.append(timed(ours, args.inner))
            b.append(timed(yard, args.inner))
        (i_k, d_k), (d_y, i_y) = ours(), yard()
        torch.cuda.synchronize()
        agree = float((i_k.long() == i_y).float().mean())
        rel = float(((d_k - d_y).abs() / d_k.abs().clamp_min(1e-30)).max())
        ws = K._C.load().lvae_nn_l2_workspace(Q, N, args.k)
        ma, mb = statistics.median(a), statistics.median(b)
        lines += ['',
                  '%s: Q %d, N %d, D %d' % (name, Q, N, D),
                  '  nn_l2      %8.3f ms [%.3f, %.3f]   table %.1f MB + workspace %.2f MB   %.3g pair-elements/s'
                  % (ma, min(a), max(a), table.numel() * table.element_size() / 1e6, ws / 1e6, Q * N * D / (ma * 1e-3)),
                  '  cdist+topk %8.3f ms [%.3f, %.3f]   table %.1f MB (float32) + distances %.1f MB'
                  % (mb, min(b), max(b), t32.numel() * 4 / 1e6, Q * N * 4 / 1e6),
                  '  nn_l2 / cdist+topk time %.2f; same neighbour in %.4f of the slots; largest relative difference of a distance %.2e'
                  % (ma / mb, agree, rel)]
        del table, t32, queries
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
