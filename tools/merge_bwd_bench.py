"""Times the backward of a merge 1x1 convolution (128 -> 64 over the concat of two 64-channel tensors) at 256 x H x H, the launches it ran
before against the persistent launch (kernels.conv1x1_cat_bwd), with and without the BatchNorm-backward apply of the block behind it:
python tools/merge_bwd_bench.py [H] [batch] [liblvae_hip.so]. Measurement tooling only."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import lvae_amd  # noqa: F401
from lvae_amd import _C
if len(sys.argv) > 3:
    _C.LIB_PATH = os.path.abspath(sys.argv[3])
from lvae_amd import kernels as K
from conv_bench import packed

H = int(sys.argv[1]) if len(sys.argv) > 1 else 16
B = int(sys.argv[2]) if len(sys.argv) > 2 else 256
C = 64
rn = lambda *s: torch.randn(*s, device='cuda')


def timed(run, reps=20, replays=7):
    """us per call: `reps` calls back to back inside one captured graph, median [min, max] of `replays` replays (tools/wgrad_pair_bench.py)"""
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


x1, x2, dy, xbn, dh, add = (rn(B, H, H, C) for _ in range(6))
w = packed(C, 2 * C, 1)
g = K.ConvGeom(w, 1, 0)
dw, db = torch.zeros_like(w), torch.zeros(C, device='cuda')
coef = K.bn_stats(xbn, torch.ones(C, device='cuda'), torch.zeros(C, device='cuda'), None, None)
parts = rn(128, 2, C)   # as many partial rows as the Winograd dgrad of this level leaves
dgam, dbet = torch.zeros(C, device='cuda'), torch.zeros(C, device='cuda')
out = torch.empty_like(dy)
pend = K.BnBwdApply(parts, dh, xbn, coef, 'elu', dgam, dbet, add=add, out=out)


def old(with_apply):
    d = dy
    if with_apply:   # the block's BatchNorm-1 apply (+ finalize), then the tile weight gradient (+ reduce) and the concat dgrad
        d = K.affine_act_bwd_parts(parts, dh, xbn, coef[0], coef[1], 'elu', coef[2], coef[3], dgam, dbet, add=add, out=out)
    K.conv2d_wgrad(x1, d, w, g, dw, db, x2=x2)
    assert K.conv1x1_dgrad_cat(d, w, g, C) is not None


def new(with_apply):
    assert K.conv1x1_cat_bwd(out if with_apply else dy, x1, x2, w, g, dw, db, apply=pend if with_apply else None) is not None


print('merge 1x1 backward at %d x %d x %d, us per call, median [min, max]' % (B, H, H))
for name, run in (('wgrad + reduce + concat dgrad (3 launches)', lambda: old(False)), ('persistent launch + reduce', lambda: new(False)),
                  ('apply + finalize + the three (5 launches)', lambda: old(True)), ('persistent launch with the apply + reduce', lambda: new(True))):
    print('%-44s %6.1f us  [%.1f, %.1f]' % ((name,) + timed(run)))
