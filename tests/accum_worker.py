"""Worker process of the accumulated step's exchange test (tests/test_accum_gpu.py starts it; not collected by pytest).

  plain        one rank, no process group: TrainStep(accum_steps=M), the reference point
  rccl1_split  one rank over RCCL with LVAE_FORCE_DIST=1 in split form: prologue graph | M micro-pass replays | ONE exchange | epilogue graph
usage: python tests/accum_worker.py MODE OUT.pt STEPS M
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MICRO = 4   # images per micro-batch


def batches(steps, m):
    g = torch.Generator().manual_seed(77)
    return [torch.floor(256 * torch.rand(MICRO * m, 3, 32, 32, generator=g)) / 255 for _ in range(steps)]


def build():
    import lvae_amd  # noqa: F401
    from conftest import load_golden
    from lvae_amd.models.lvae import LadderVAE
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax
    g = load_golden('tiny_cifar')
    torch.manual_seed(0)
    m = LadderVAE(**g.cfg)
    m.load_state_dict(g.state_dict())
    m.cuda().train()
    m.noise = PhiloxNoise(seed=5)
    return m, Adamax(m, lr=1e-3)


def dump(path, model, opt, extra):
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    torch.save({'sd': sd, 'exp_avg': opt.exp_avg.cpu(), 'exp_inf': opt.exp_inf.cpu(), 'opt_step': int(opt.step_count.item()),
                'extra': extra}, path)


def main():
    mode, out, steps, M = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
    import lvae_amd  # noqa: F401
    from lvae_amd import dist as ldist
    from lvae_amd.engine import TrainStep
    if mode == 'plain':
        m, opt = build()
        step = TrainStep(m, opt, use_graph=True, accum_steps=M)
        losses = [float(step(x.cuda())['loss']) for x in batches(steps, M)]
        torch.cuda.synchronize()
        assert step.graph_p is not None and step.graph_a is not None and step.graph_b is not None
        dump(out, m, opt, {'losses': losses})
    elif mode == 'rccl1_split':
        os.environ['LVAE_FORCE_DIST'] = '1'
        os.environ.pop('LVAE_DDP_MODE', None)
        rank, world, _ = ldist.init_from_env('nccl')
        m, opt = build()
        arena = m.pack()
        ldist.broadcast_flat(arena.params)
        ar = ldist.GradAllReduce(arena.grads, segments=arena.segments)
        assert ar.comm is not None, ar.comm_error
        assert ar.mode == 'split' and not ar.overlap and len(ar.buckets) == 1
        runs, real = [], ar.run

        def counted():
            runs.append(m.global_step)
            return real()

        ar.run = counted
        step = TrainStep(m, opt, use_graph=True, allreduce=ar, accum_steps=M)
        gscale = float(opt.gscale.item())
        losses = [float(step(x.cuda())['loss']) for x in batches(steps, M)]
        torch.cuda.synchronize()
        assert step.graph_p is not None and step.graph_a is not None and step.graph_b is not None
        dump(out, m, opt, {'losses': losses, 'runs': runs, 'launched': ar.launched, 'gscale': gscale})
        ar.close()
        torch.distributed.destroy_process_group()
    else:
        raise SystemExit('unknown mode ' + mode)


if __name__ == '__main__':
    main()
