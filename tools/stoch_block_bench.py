"""Isolated timing of the stochastic block at the low-resolution levels of a step (batch 256, 64 channels, Z = 32): the one launch of
csrc/stoch_img.hip against the four launches it replaces, forward (conv_in_p, conv_in_q, the elementwise core, conv_out) and backward
(dgrad of conv_out, the core's backward, the dgrads of conv_in_q and conv_in_p; the weight gradients are queued launches on both sides):
    python tools/stoch_block_bench.py [--reps R] [--batch B]
The noise tensor is given (its fill launch is on both sides of the comparison in a step and on neither here); the weights' pre-split /
pre-transformed copies are prepared once, as a step does. Each form is timed inside a captured graph of 50 back-to-back calls, replayed R
times; the figures are microseconds per call, median and [min, max] over the replays. `top`: the block without conv_in_p (three launches)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import lvae_amd  # noqa: F401
from lvae_amd import kernels as K
from lvae_amd import resblock as RB
from lvae_amd.lib.stochastic import NormalStochasticBlock2d

C, Z, N_CALLS = 64, 32, 50


class Given:
    def __init__(self, eps):
        self.eps = eps

    def normal(self, shape, device):
        return self.eps


def graph_time(fn, reps):
    """us per call of fn, [median, min, max] over `reps` replays of a graph of N_CALLS calls"""
    for _ in range(2):
        fn()
    K.prepared.prepare_all()
    fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            for _ in range(N_CALLS):
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
        ts.append(e0.elapsed_time(e1) / N_CALLS * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--batch', type=int, default=256)
    a = ap.parse_args()
    B = a.batch
    print('# level  block  pass  composed us/call median [min, max]  fused us/call median [min, max]  fused - composed')
    for H, top in ((8, False), (4, False), (2, False), (2, True)):
        torch.manual_seed(H)
        blk = NormalStochasticBlock2d(C, Z, C, transform_p_params=not top).cuda()
        for m in blk.children():   # the layout the gradient arena packs a model's weights in ([KH][KW][Cin][Cout]): what the composed kernels are routed by
            m.weight.data = m.weight.data.permute(2, 3, 1, 0).contiguous().permute(3, 2, 0, 1)
        xp = 0.5 * torch.randn(1, H, H, 2 * Z, device='cuda') if top else torch.randn(B, H, H, C, device='cuda')
        xq = torch.randn(B, H, H, C, device='cuda')
        noise = Given(torch.randn(B, H, H, Z, device='cuda'))
        res = {}
        for on in (False, True):
            def fn():
                RB.switches.stoch_block = on
                with torch.no_grad():
                    blk(xp, xq, noise=noise, need_kl_elementwise=False)
            res[on] = graph_time(fn, a.reps)
        RB.switches.stoch_block = True
        # backward, on what a forward left
        with torch.no_grad():
            _, d = blk(xp, xq, noise=noise, need_kl_elementwise=False)
        p, q, z = d['p_params'], d['q_params'], d['z']
        cv = lambda m: (m.weight, m.geom(), m.bias)
        cvp, cvq, cvo = (None if top else cv(blk.conv_in_p)), cv(blk.conv_in_q), cv(blk.conv_out)
        d_out, g = torch.randn(B, H, H, C, device='cuda'), [torch.randn(B, device='cuda') for _ in range(3)]
        gks = torch.randn(B, H, H, device='cuda')

        def composed():
            dz = K.conv2d_dgrad(d_out, cvo[0], cvo[1], (H, H))
            dp, dq = K.normal_stochastic_bwd(p, q, noise.eps, z, dz, g[0], g[1], g[2], gks, 0, False, Z)
            K.conv2d_dgrad(dq, cvq[0], cvq[1], (H, H))
            if not top:
                K.conv2d_dgrad(dp, cvp[0], cvp[1], (H, H))

        def one():
            assert K.stoch_block_bwd(d_out, cvp, cvq, cvo, p, q, z, noise.eps, None, g[0], g[1], g[2], gks, 0, False) is not None
        bres = {False: graph_time(composed, a.reps), True: graph_time(one, a.reps)}
        for name, rr in (('fwd', res), ('bwd', bres)):
            (cm, cl, ch), (fm, fl, fh) = rr[False], rr[True]
            print('%2dx%-2d  %-5s  %s  %6.1f [%6.1f, %6.1f]   %6.1f [%6.1f, %6.1f]   %+6.1f' % (H, H, 'top' if top else 'inner', name, cm, cl, ch, fm, fl, fh, fm - cm))


if __name__ == '__main__':
    main()
