"""Times the weight gradients of a stochastic layer's convolutions at 256 x H x H (conv_out 32 -> 64, conv_in_q and conv_in_p 64 -> 64),
as single launches back to back and as the shared launch of three and of two problems:
python tools/wgrad_shared_bench.py [H] [liblvae_hip.so]. Measurement tooling only."""
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
B, C, Z = 256, 64, 32
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


def entry(cin):
    w = packed(C, cin, 3)
    return (rn(B, H, H, cin), rn(B, H, H, C), w, K.ConvGeom(w, 1, 1), torch.zeros_like(w), torch.zeros(C, device='cuda'), {})


out, in_q, in_p = entry(Z), entry(C), entry(C)


def singles(items):
    for x, dy, w, g, dw, db, kw in items:
        K.conv2d_wgrad(x, dy, w, g, dw, db, **kw)


print('shared schedule %dx%d, three problems: %s' % (H, H, K.conv2d_wgrad_shared_schedule([(e[0], e[2], e[3]) for e in (out, in_q, in_p)])))
print('shared schedule %dx%d, two problems:   %s' % (H, H, K.conv2d_wgrad_shared_schedule([(e[0], e[2], e[3]) for e in (out, in_q)])))
for name, run in (('conv_out alone, tile kernel + reduce', lambda: singles([out])), ('conv_out alone, this kernel + reduce', lambda: K.conv2d_wgrad_shared([out])),
                  ('conv_in_q alone (kernel + reduce)', lambda: singles([in_q])),
                  ('three single launches back to back', lambda: singles([out, in_q, in_p])), ('shared launch of three', lambda: K.conv2d_wgrad_shared([out, in_q, in_p])),
                  ('two single launches back to back', lambda: singles([out, in_q])), ('shared launch of two', lambda: K.conv2d_wgrad_shared([out, in_q]))):
    print('%-38s %6.1f us  [%.1f, %.1f]' % ((name,) + timed(run)))
