"""Times the two Winograd weight gradients of a residual block at 256 x H x H x 64, alone, back to back and as the pair launch:
python tools/wgrad_pair_bench.py [H] [liblvae_hip.so]. With a -DLVAE_TUNING_ENV library LVAE_WINO_PAIR_RANGES_A sweeps the pair's split
(one process per value: the library reads it once). Measurement tooling only."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import lvae_amd  # noqa: F401
from lvae_amd import _C
if len(sys.argv) > 2:
    _C.LIB_PATH = os.path.abspath(sys.argv[2])
from lvae_amd import kernels as K
from conv_bench import packed

H = int(sys.argv[1]) if len(sys.argv) > 1 else 16
B, C = 256, 64
rn = lambda *s: torch.randn(*s, device='cuda')
x, dh, y1, dy2 = rn(B, H, H, C), rn(B, H, H, C), rn(B, H, H, C), rn(B, H, H, C)
w1, w2 = packed(C, C, 3), packed(C, C, 3)
g1, g2 = K.ConvGeom(w1, 1, 1), K.ConvGeom(w2, 1, 1)
dw1, dw2, db1, db2 = torch.zeros_like(w1), torch.zeros_like(w2), torch.zeros(C, device='cuda'), torch.zeros(C, device='cuda')
dga, dbe = torch.zeros(C, device='cuda'), torch.zeros(C, device='cuda')
c1 = K.bn_stats(x, None, None, None, None)
c2 = K.bn_stats(y1, None, None, None, None)
parts = rn(256, 2, C)
drop = (torch.rand(B, C, device='cuda') < 0.8).float() / 0.8
out = torch.empty_like(x)


def grad_a():
    K.conv2d_wgrad_apply(x, w1, g1, dw1, db1, K.BnBwdApply(parts, dh, y1, c2, 'elu', dga, dbe, drop=drop, out=out), in_scale=c1[0], in_shift=c1[1], in_act='elu')


def grad_b():
    K.conv2d_wgrad(y1, dy2, w2, g2, dw2, db2, in_scale=c2[0], in_shift=c2[1], in_act='elu')


def both():
    grad_b()
    grad_a()


def pair():
    K.conv2d_wgrad_pair(x, w1, g1, dw1, db1, K.BnBwdApply(parts, dh, y1, c2, 'elu', dga, dbe, drop=drop, out=out), dy2, w2, g2, dw2, db2,
                        in_scale=c1[0], in_shift=c1[1], in_act='elu', in_scale_b=c2[0], in_shift_b=c2[1], in_act_b='elu')


def timed(run, reps=20, replays=7):
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(reps):
            run()
    gr.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(replays):
        e0.record()
        gr.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / reps * 1000)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


print('pair schedule %dx%d: %s  (LVAE_WINO_PAIR_RANGES_A=%s)' % (H, H, K.conv2d_wgrad_pair_schedule(x, w1, g1, y1, w2, g2), os.environ.get('LVAE_WINO_PAIR_RANGES_A')))
for name, run in (('A: conv1 + apply (kernel + reduce)', grad_a), ('B: conv2 (kernel + reduce)', grad_b), ('A and B back to back', both), ('pair', pair)):
    print('%-36s %6.1f us  [%.1f, %.1f]' % ((name,) + timed(run)))
