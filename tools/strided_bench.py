"""Isolated timing of the resampling 3x3 convolutions of a step at batch 256, 64 channels: the stride-2 convolution of the `down` blocks, the
transposed stride-2 convolution of the `up` blocks, and the input gradient of each:  python tools/strided_bench.py [--reps R] [--img 32|64]
(--img 64 adds the 32x32 <-> 16x16 level of the 64x64 config).

Each launch is timed inside a captured graph of 50 back-to-back launches (no host time between them), replayed R times; the figure is
microseconds per launch, median and [min, max] over the replays. `pm` is lvae_conv2d_position_major of the launch (- where the library
has no such query). Run it under each tree to compare two libraries."""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import lvae_amd  # noqa: F401
from lvae_amd import kernels as K

B, C, N_LAUNCH = 256, 64, 50


def graph_time(fn, reps):
    """us per launch of fn, [median, min, max] over `reps` replays of a graph of N_LAUNCH launches"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            for _ in range(N_LAUNCH):
                fn()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / N_LAUNCH * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def position_major(x, w, g, dgrad, in_hw=None):
    lib = K._C.load()
    if not hasattr(lib, 'lvae_conv2d_position_major'):
        return '-'
    N, H, W, _ = x.shape
    if dgrad:
        d = K._desc(g, w, x, None, N, H, W, in_hw[0], in_hw[1], g.Cin, g.s_co, g.s_ci, K.GATHER_CONV if g.transposed else K.GATHER_TRANSPOSED,
                    y=torch.empty(N, in_hw[0], in_hw[1], g.Cin, device='cuda'))
    else:
        OH, OW = g.out_size(H, W)
        d = K._desc(g, w, x, None, N, H, W, OH, OW, g.Cout, g.s_ci, g.s_co, K.GATHER_TRANSPOSED if g.transposed else K.GATHER_CONV,
                    y=torch.empty(N, OH, OW, g.Cout, device='cuda'))
    lib.lvae_conv2d_position_major.restype = ctypes.c_int32
    return str(lib.lvae_conv2d_position_major(ctypes.byref(d)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--img', type=int, default=32, choices=[32, 64], help='image size of the model whose resampling levels are timed')
    a = ap.parse_args()
    top = a.img // 2
    print('# layer  launch  in -> out  pm  us/launch median [min, max]  fp32-MFMA floor us')
    for transposed in (False, True):
        for H in [h for h in (32, 16, 8, 4) if h <= top] if not transposed else [h for h in (2, 4, 8, 16) if h < top]:   # the resampling levels
            w = torch.randn(3, 3, C, C, device='cuda').permute(2, 3, 0, 1) * 0.05 if transposed else \
                torch.randn(3, 3, C, C, device='cuda').permute(3, 2, 0, 1) * 0.05
            g = K.ConvGeom(w, 2, 1, transposed=transposed, output_padding=1 if transposed else 0)
            x = torch.randn(B, H, H, C, device='cuda')
            b = torch.randn(C, device='cuda')
            y = K.conv2d(x, w, g, bias=b)
            OH = y.shape[1]
            dy = torch.randn_like(y)
            floor = 2.0 * B * max(H, OH) ** 2 / 4 * C * C * 9 / 157.3e12 * 1e6
            name = 'up  ' if transposed else 'down'
            for kind, fn, src, dst, pm in (
                    ('fwd  ', lambda: K.conv2d(x, w, g, bias=b), H, OH, position_major(x, w, g, False)),
                    ('dgrad', lambda: K.conv2d_dgrad(dy, w, g, (H, H)), OH, H, position_major(dy, w, g, True, (H, H)))):
                med, lo, hi = graph_time(fn, a.reps)
                print('%s  %s  %2dx%-2d -> %2dx%-2d  %s  %6.1f [%6.1f, %6.1f]  %5.1f' % (name, kind, src, src, dst, dst, pm, med, lo, hi, floor))


if __name__ == '__main__':
    main()
