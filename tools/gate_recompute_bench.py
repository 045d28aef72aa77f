"""Times conv2 + gate forward (with and without the ab store) and the persistent gate backward in its stored and its recompute form at
256 x H x H x 64, with and without a deferred apply: python tools/gate_recompute_bench.py [H] [liblvae_hip.so]. 20 back-to-back calls inside
one captured graph, 7 replays, as tools/wgrad_pair_bench.py. Measurement tooling only."""
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
y1, x, dout, xb, dh, add = (rn(B, H, H, C) for _ in range(6))
w2, wg = packed(C, C, 3), packed(2 * C, C, 1)
g2, gg = K.ConvGeom(w2, 1, 1), K.ConvGeom(wg, 1, 0)
b2, bg = rn(C) * 0.1, rn(2 * C) * 0.5
drop = (torch.rand(B, C, device='cuda') < 0.8).float() / 0.8
coef = K.bn_stats(y1, None, None, None, None)
cb = K.bn_stats(xb, None, None, None, None)
parts = rn(256, 2, C)
dw, db, dga, dbe = torch.zeros_like(wg), torch.zeros(2 * C, device='cuda'), torch.zeros(C, device='cuda'), torch.zeros(C, device='cuda')
out = torch.empty_like(x)
pivot = coef[2]



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


fwd = lambda want: K.rb_conv_gate(y1, w2, g2, b2, 'elu', drop, wg, gg, bg, x, 'elu', coef=coef, stats_pivot=pivot, want_ab=want)
y2, ab = fwd(True)[:2]
K.prepared.prepare_all()   # the planes of both directions: no launch rewrites them inside the timed graphs
pend = lambda: K.BnBwdApply(parts, dh, xb, cb, 'elu', dga, dbe, add=add, out=out)

runs = (('forward, ab stored', lambda: fwd(True)),
        ('forward, no ab', lambda: fwd(False)),
        ('backward, stored form', lambda: K.conv1x1_gate_bwd_wgrad(dout, ab, y2, wg, gg, 'elu', dw, db, out_scale=drop)),
        ('backward, recompute form', lambda: K.conv1x1_gate_bwd_wgrad_recompute(dout, y2, wg, gg, bg, 'elu', dw, db, out_scale=drop)),
        ('backward + apply, stored form', lambda: K.conv1x1_gate_bwd_wgrad(out, ab, y2, wg, gg, 'elu', dw, db, out_scale=drop, apply=pend())),
        ('backward + apply, recompute form', lambda: K.conv1x1_gate_bwd_wgrad_recompute(out, y2, wg, gg, bg, 'elu', dw, db, out_scale=drop, apply=pend())))
print('256 x %d x %d x 64, us per call (backward: kernel + slab reduce): median [min, max]' % (H, H))
for name, run in runs:
    print('%-36s %6.1f  [%.1f, %.1f]' % ((name,) + timed(run)))
