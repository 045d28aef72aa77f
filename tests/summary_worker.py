"""Worker process of the log-summary tests (tests/test_summary_cpu.py and tests/test_summary_gpu.py start it; not collected by pytest).

  gloo   rank RANK of WORLD_SIZE over gloo, no GPU: holds its own CPU accumulator of a log window, reduces it as TrainSummary.take does and
         writes the means it gets to OUT.<rank>
  split  one rank over RCCL with LVAE_FORCE_DIST=1 in the default split form (fwd+bwd graph | exchange | Adamax graph) on the tiny CIFAR
         model, with a summary and a gradient scale of 0.5: writes, per step, the window of one it took and the raw gradient norm
usage: python tests/summary_worker.py MODE OUT"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

L = 2


def rank_steps(rank):
    """The per-step values [loss, elbo, recons, kl, l2, grad, kl_layer_0, kl_layer_1] one rank folded: rank 0 three steps, rank 1 two and
    one non-finite step. All are small dyadic numbers, so float64 sums of them are exact in any order."""
    n = 3 if rank == 0 else 2
    return [[1.5 + rank + 0.25 * k, -2.0 - k, 3.0 + 0.5 * rank, 0.125 * (k + 1), 7.0, 0.5 * (rank + 1) + k, 1.0 + k, 0.25 * rank]
            for k in range(n)]


def accumulator(rank):
    steps = rank_steps(rank)
    sums = [sum(s[i] for s in steps) for i in range(6 + L)]
    return [float(len(steps)), float(rank)] + sums   # rank 1 saw one non-finite step


def gloo(out):
    from lvae_amd import dist as ldist
    from lvae_amd import summary
    rank, world, _ = ldist.init_from_env('gloo')
    vec = torch.tensor(accumulator(rank), dtype=torch.float64)
    vec, ranks = summary.reduce_sums(vec)
    m = summary.means(vec.tolist(), L, True)
    with open(out + '.%d' % rank, 'w') as f:
        json.dump({'means': m, 'ranks': ranks}, f)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def split(out, steps=5):
    os.environ['LVAE_FORCE_DIST'] = '1'
    from conftest import load_golden
    from lvae_amd import dist as ldist
    from lvae_amd import kernels as K
    from lvae_amd.engine import TrainStep
    from lvae_amd.models.lvae import LadderVAE
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax
    from lvae_amd.summary import TrainSummary
    ldist.init_from_env('nccl')
    g = load_golden('tiny_cifar')
    torch.manual_seed(0)
    m = LadderVAE(**g.cfg)
    m.load_state_dict(g.state_dict())
    m.cuda().train()
    m.noise = PhiloxNoise(seed=3)
    opt = Adamax(m, lr=1e-3)
    arena = m.pack()
    ldist.broadcast_flat(arena.params)
    ar = ldist.GradAllReduce(arena.grads, segments=arena.segments)
    assert ar.comm is not None, ar.comm_error
    assert ar.mode == 'split' and not ar.overlap
    summ = TrainSummary(len(g.cfg['z_dims']), 'cuda')
    step = TrainStep(m, opt, use_graph=True, allreduce=ar, summary=summ)
    opt._state()
    opt.gscale = torch.full((1,), 0.5, device='cuda')   # what a second rank would make it; set before the first step and the capture
    gen = torch.Generator().manual_seed(9)
    rows = []
    for _ in range(steps):
        x = torch.floor(256 * torch.rand(4, 3, 32, 32, generator=gen)) / 255
        res = step(x.cuda())
        loss = float(res['loss'])
        raw = float(K.l2norm(arena.grads))             # the exchanged gradient is still in the arena
        w = summ.take()
        rows.append({'loss': loss, 'raw_norm': raw, 'window': w, 'graph_b': step.graph_b is not None})
    torch.cuda.synchronize()
    assert step.graph_a is not None and step.graph_b is not None and 'split' in step.exchange_description()
    with open(out, 'w') as f:
        json.dump(rows, f)
    ar.close()
    torch.distributed.destroy_process_group()


if __name__ == '__main__':
    import lvae_amd  # noqa: F401
    {'gloo': gloo, 'split': split}[sys.argv[1]](sys.argv[2])
