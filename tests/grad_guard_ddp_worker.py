"""Worker process of the gradient guard's exchange-form test (tests/test_grad_guard_gpu.py starts it; not collected by pytest).

  single   one rank, no process group, no guard: five captured steps, the reference point
  split    one forced rank over RCCL (LVAE_FORCE_DIST=1), one message after backward between the fwd+bwd graph and the Adamax graph, under
           an idle guard; then a NaN batch and a clean one
  overlap  the same with completion-ordered buckets exchanged during backward inside the one captured graph
usage: python tests/grad_guard_ddp_worker.py MODE OUT.pt
"""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = dict(color_ch=3, z_dims=[8, 8], blocks_per_layer=1, downsample=[1, 1], nonlin='elu', merge_type='residual', batchnorm=True,
           stochastic_skip=True, n_filters=16, dropout=0.2, free_bits=1.0, learn_top_prior=True, img_shape=(32, 32),
           likelihood_form='discr_log_mix', res_block_type='bacdbacd', gated=True, no_initial_downscaling=False, analytical_kl=False)
BATCH, CLEAN = 8, 5


def batches(n):
    g = torch.Generator().manual_seed(77)
    return [torch.floor(256 * torch.rand(BATCH, 3, 32, 32, generator=g)) / 255 for _ in range(n)]


def snapshot(m, opt):
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    sd.update(exp_avg=opt.exp_avg.clone(), exp_inf=opt.exp_inf.clone(), adamax_step=opt.step_count.clone(), params=m.arena.params.detach().clone())
    return sd


def main():
    mode, out = sys.argv[1], sys.argv[2]
    import lvae_amd  # noqa: F401
    from lvae_amd import dist as ldist
    from lvae_amd.engine import TrainStep
    from lvae_amd.models.lvae import LadderVAE
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax, GradGuard
    ar = None
    if mode != 'single':
        os.environ['LVAE_FORCE_DIST'] = '1'
        os.environ['LVAE_DDP_MODE'] = mode
        ldist.init_from_env('nccl')
    torch.manual_seed(42)
    m = LadderVAE(**CFG).cuda().train()
    m.noise = PhiloxNoise(seed=5, rank=0)
    opt = Adamax(m, lr=1e-3, guard=None if mode == 'single' else GradGuard(max_norm=1e30, skip_threshold=math.inf))
    arena = m.pack()
    if mode != 'single':
        ldist.broadcast_flat(arena.params)
        ar = ldist.GradAllReduce(arena.grads, segments=arena.segments, bucket_mb=0.25 if mode == 'overlap' else None)
        assert ar.comm is not None, ar.comm_error
    step = TrainStep(m, opt, use_graph=True, allreduce=ar)
    assert mode == 'single' or step.overlap == (mode == 'overlap')
    xs = batches(CLEAN + 2)
    losses = [float(step(x.cuda())['loss']) for x in xs[:CLEAN]]
    torch.cuda.synchronize()
    res = {'losses': losses, 'sd': {k: v.detach().cpu().clone() for k, v in m.state_dict().items()},
           'graphs': (step.graph_a is not None, step.graph_b is not None)}
    if mode != 'single':
        res['counts_idle'] = opt.guard.counts()
        before = snapshot(m, opt)
        bad = xs[CLEAN].clone()
        bad[3, 0, 9, 9] = math.nan
        res['bad_loss'] = float(step(bad.cuda())['loss'])
        after = snapshot(m, opt)
        tracked = [k for k in before if k.endswith('num_batches_tracked')]
        res['unchanged'] = all(torch.equal(before[k], after[k]) for k in before if k not in tracked)
        res['tracked_advanced'] = bool(tracked) and all(int(after[k]) == int(before[k]) + 1 for k in tracked)
        res['next_loss'] = float(step(xs[CLEAN + 1].cuda())['loss'])
        torch.cuda.synchronize()
        last = snapshot(m, opt)
        res['moved_after'] = (not torch.equal(last['params'], after['params'])) and bool(torch.isfinite(last['params']).all())
        res['counts_end'] = opt.guard.counts()
        ar.close()
        torch.distributed.destroy_process_group()
    torch.save(res, out)


if __name__ == '__main__':
    main()
