"""`python -m lvae_amd.main <flags>` — training entry point with the reference's flag surface (main.py:1-13 there is
`Trainer(LVAEExperiment()).run()` on boilr; here a minimal loop on the HIP engine, one process per GPU).

Launch N ranks with:  python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 -m lvae_amd.main ...
"""
import os
import time

import numpy as np
import torch

from . import dist as ldist
from .checkpoint import lr_schedule_record, save_checkpoint
from .data import DeviceDataset
from .balance import klb_suffix
from .engine import TrainStep, linear_anneal
from .evaluate import image_pass, test_pass
from .experiment.experiment_manager import LVAEExperiment
from .images import write_png
from .latent import LatentStats, latent_line_suffix
from .quality import ImageQuality, quality_line_suffix
from .schedule import TrainSchedule, checkpoint_path, checkpoints_to_delete
from .summary import History, TrainSummary, train_line_suffix


def synthetic_batch(exp, batch, gen):
    shape = (batch, exp.color_ch) + tuple(exp.img_size)
    u = torch.rand(shape, generator=gen)
    return (u > 0.5).float() if exp.args.likelihood == 'bernoulli' else torch.floor(256 * u) / 255


def _shard(x, rank, world):
    n = x.shape[0]
    return x[n * rank // world:n * (rank + 1) // world]


def image_table(dataset):
    """(images, channels_last) of a DatasetLoader data set as it is stored: the float NCHW tensor of a TensorDataset, or CelebA's uint8 NHWC
    array, which --device-data keeps as it is (the per-item permute / float / div happens in the gather instead)."""
    if hasattr(dataset, 'tensors'):
        return dataset.tensors[0], False
    return dataset.data, True


def fixed_binarized(exp, images, channels_last=False):
    """--binarize: a host image set with its one fixed binarization per image (data.binarize_fixed: a function of --seed and the image's
    number in `images`), as float 0/1 NCHW; without the flag, `images` as they are. -> (images, channels_last)."""
    if not getattr(exp.args, 'binarize', False):
        return images, channels_last
    from .data import binarize_fixed
    return binarize_fixed(images, exp.args.seed, channels_last=channels_last).float(), False


def test_batches(exp, loader, npz, rank, world, on_device=False):
    """A callable returning this rank's shard of the test set as an iterable of NCHW batches, or None when there is no test split
    (DatasetLoader.test, a 'test' key of --data-npz, or --synthetic-test N fixed seeded images). on_device (--device-data): the shard is
    kept in device memory and the batches are gathered from it (data.DeviceDataset.batches). Under --binarize the whole split gets its
    fixed binarization first, before it is cut over the ranks: the test lines are the same at every world size."""
    args = exp.args
    bs = args.test_batch_size
    if loader is not None and getattr(loader, 'test', None) is not None:
        if on_device:
            # the same images per rank as below: every test batch is split over the ranks, in batches of one rank's part of a full one
            imgs, channels_last = fixed_binarized(exp, *image_table(loader.test.dataset))
            mine = torch.cat([_shard(imgs[i:i + bs], rank, world) for i in range(0, imgs.shape[0], bs)])
            per = max(1, _shard(imgs[:bs], rank, world).shape[0])
            ds = DeviceDataset(mine, None, args.seed, device=exp.device, channels_last=channels_last)
            return lambda: ds.batches(per)
        return lambda: (xs for xs in (_shard(b[0], rank, world) for b in loader.test) if xs.shape[0])
    if npz is not None and 'test' in npz:
        data = _shard(fixed_binarized(exp, torch.from_numpy(npz['test']).float())[0], rank, world)
    elif args.synthetic and args.synthetic_test > 0:
        data = _shard(synthetic_batch(exp, args.synthetic_test, torch.Generator().manual_seed(args.seed + 7919)), rank, world)
    else:
        return None
    if on_device:
        ds = DeviceDataset(data, None, args.seed, device=exp.device)
        return lambda: ds.batches(bs)
    return lambda: (data[i:i + bs] for i in range(0, data.shape[0], bs))


def recal_batches(exp, loader, data, feed):
    """--ema-bn-batches N: a callable returning the first N batches of --batch-size training images in stored order (data.first_batches), the
    same on every rank and at every world size; None without the flag. From the HBM table under --device-data, else from the data set's
    or the .npz's host tensor; under --synthetic the N batches rank 0 of a one-rank run trains on first, from a generator of their own.
    Neither the loader, nor the device cursor, nor a training generator is consumed."""
    args = exp.args
    n = getattr(args, 'ema_bn_batches', 0)
    if n <= 0:
        return None
    from .data import first_batches
    channels_last = False
    if feed is not None:
        src = feed
    elif loader is not None:
        src, channels_last = image_table(loader.train.dataset)
    elif data is not None:
        src = data
    else:
        gen = torch.Generator().manual_seed(args.seed)
        src = torch.cat([synthetic_batch(exp, args.batch_size, gen) for _ in range(n)])
    if (src.N if feed is not None else int(src.shape[0])) < args.batch_size:
        raise SystemExit('--ema-bn-batches: the training set does not fill one batch of %d' % args.batch_size)
    if feed is None and getattr(args, 'binarize', False):   # the images first_batches will read, fixed-binarized (a feed does that itself)
        src, channels_last = fixed_binarized(exp, src[:n * args.batch_size], channels_last)
    return lambda: first_batches(src, n, args.batch_size, channels_last)


def lr_suffix(m):
    """What a scheduled lr appends to a train line: the lr of the step the line falls due at."""
    return '   lr: {:.3g}'.format(m['lr/lr']) if 'lr/lr' in m else ''


def guard_suffix(m):
    """What a gradient guard appends to a train line: the norm of the gradient of the step the line falls due at (with --window-summaries
    the window's mean is already there) and the steps clipped / skipped since the previous train line."""
    if 'grad/clipped' not in m:
        return ''
    s = '   grad: {:.3g}'.format(m['grad/norm']) if 'grad/norm' in m else ''
    return s + '   clipped: {}   skipped: {}'.format(m['grad/clipped'], m['grad/skipped'])


def guard_metrics(guard, gscale, seen, m, with_norm):
    """Adds the guard's numbers to the metrics of a train line (one device-to-host read each); -> the cumulative counts, for the next line."""
    now = guard.counts()
    m['grad/clipped'], m['grad/skipped'] = now[0] - seen[0], now[1] - seen[1]
    if with_norm:
        # (the product in fp32, as the summary's grad slot and the guard's decision form it)
        m['grad/norm'] = float(np.float32(guard.norm.item()) * np.float32(1.0 if gscale is None else gscale.item()))
    return now


def spectral_suffix(m):
    """What --spectral-reg appends to a train line: the sum and the largest of the convolutions' spectral norms, of the step the line falls
    due at."""
    return '   sr: {:.5g}   max: {:.4g}'.format(m['spectral/sum'], m['spectral/max']) if 'spectral/sum' in m else ''


def spectral_metrics(out, m):
    if 'sr_sum' in out:
        m['spectral/sum'], m['spectral/max'] = out['sr_sum'].item(), out['sr_max'].item()


def balance_metrics(balance, m):
    """Adds the KL-balancing coefficients of the step a train line falls due at as `kl_balance/coeff_<i>` (one device-to-host read; of an
    accumulated step, its last micro-pass). Nothing else: these keys are what --history records."""
    if balance is None:
        return
    for i, c in enumerate(balance.coeff.tolist()):
        m['kl_balance/coeff_%d' % i] = c


def balance_suffix(m, step, beta_anneal):
    """What --kl-balance appends to a train line: `klb: <min>..<max>` of the coefficients, or `klb: off` once beta has reached 1. Step
    `step` ran with the beta of `step - 1` completed steps: the schedule the device counter follows, restated on the host for the word
    `off` alone (the coefficients themselves cannot say it: they can all be 1 while the rule is active, with one layer for instance)."""
    coeff = [v for k, v in m.items() if k.startswith('kl_balance/coeff_')]
    if not coeff:
        return ''
    return klb_suffix(coeff, linear_anneal(step - 1, 0.0, 1.0, beta_anneal) < 1.0)


def iw_suffix(m, k):
    """What --iw-train-samples K > 1 appends to a train line: the K-sample bound (at beta = 1) and the effective sample size of the weights,
    of the step the line falls due at."""
    return '   IW({}): {:.5g}   ESS: {:.3g}'.format(k, m['elbo/iw_train'], m['iw/ess']) if 'elbo/iw_train' in m else ''


IMG_NROWS = 8   # pictures of --ts-img-every: 8 x 8 samples, 32 input / reconstruction pairs


def main(argv=None):
    rank, world, local = ldist.init_from_env()
    if torch.cuda.is_available():
        torch.cuda.set_device(local)
    exp = LVAEExperiment(argv=argv)
    args = exp.args
    loader = None
    if not (args.synthetic or args.data_npz):
        from .data import DatasetLoader  # the reference's on-disk formats (experiment/data.py); nothing is downloaded here
        try:
            loader = DatasetLoader(args)
        except RuntimeError as e:
            raise SystemExit("%s\n(or pass --synthetic / --data-npz FILE)" % e)
    model, opt = exp.model, exp.optimizer
    # --window-summaries: every step folds its metrics into a device accumulator; a train line is the mean since the previous one
    summary = TrainSummary(len(args.z_dims), exp.device) if args.window_summaries else None
    if args.resume:
        from .checkpoint import load_checkpoint, rule_warning
        # (weights, optimizer state and average, global step, the rank-0 noise stream's position and the open log window)
        ck = load_checkpoint(args.resume, model, opt, summary=summary)
        if rank == 0 and rule_warning(args.resume, ck, opt):
            print(rule_warning(args.resume, ck, opt))
        was = ck.get('lr_schedule') if isinstance(ck, dict) and 'model' in ck else None
        if rank == 0 and was != lr_schedule_record(opt):
            print('warning: %s was written with the lr schedule %s; continuing with %s' % (args.resume, was, lr_schedule_record(opt)))
        was_guard = ck.get('grad_guard') if isinstance(ck, dict) and 'model' in ck else None
        if rank == 0 and opt.guard is not None and was_guard is not None and \
                {k: was_guard.get(k) for k in ('max_norm', 'skip_threshold')} != opt.guard.limits():
            print('warning: %s was written with the gradient limits %s; continuing with %s'
                  % (args.resume, {k: was_guard.get(k) for k in ('max_norm', 'skip_threshold')}, opt.guard.limits()))
        was_iw = ck.get('iw_train_samples', 1) if isinstance(ck, dict) and 'model' in ck else 1
        if rank == 0 and was_iw != args.iw_train_samples:
            print('warning: %s was written with --iw-train-samples %d; continuing with %d' % (args.resume, was_iw, args.iw_train_samples))
        from .checkpoint import spectral_warning
        line = spectral_warning(args.resume, ck, opt)
        if rank == 0 and line:
            print(line)
        from .checkpoint import accum_steps_record
        if rank == 0 and accum_steps_record(ck) != args.accum_steps:
            print('warning: %s was written with --accum-steps %d; continuing with %d' % (args.resume, accum_steps_record(ck), args.accum_steps))
        from .checkpoint import augment_record
        if rank == 0 and augment_record(ck) != exp.augment_record(args):
            print('warning: %s was written with the feed augmentation %s; continuing with %s' % (args.resume, augment_record(ck),
                                                                                              exp.augment_record(args)))
        from .checkpoint import kl_balance_warning
        line = kl_balance_warning(args.resume, ck, args.kl_balance)
        if rank == 0 and line:
            print(line)
        del ck
    model.noise.seed ^= rank * 0x9E3779B9
    model.train()
    arena = model.pack()
    per_rank = args.batch_size // max(1, world)
    data = npz = None
    if args.data_npz:
        npz = np.load(args.data_npz)
        data = torch.from_numpy(npz['data']).float()
    tests = test_batches(exp, loader, npz, rank, world, on_device=args.device_data)
    feed = None
    if args.device_data:
        if args.batch_size % world:
            raise SystemExit('--batch-size must be divisible by the world size')
        # the whole training set in device memory; the step gathers its own batch, in an order that is a function of (--seed, step)
        imgs, channels_last = image_table(loader.train.dataset) if loader is not None else (data, False)
        # (--binarize / --hflip / --dequantize: the gather augments the batch it forms)
        feed = DeviceDataset(imgs, args.batch_size, args.seed, rank=rank, world=world, device=exp.device, channels_last=channels_last,
                             augment=exp.feed_augment(args))
    recal = recal_batches(exp, loader, data, feed)     # --ema-bn-batches: what the averaged weights' BatchNorm statistics are re-estimated on
    sched = TrainSchedule.from_args(args, tests is not None)
    if args.simple_data_dependent_init and not args.resume:
        # experiment_manager.py:61-72: the first batch_size training images (parity unpinned, see init.py)
        from .init import data_dependent_init
        x0 = loader.train.dataset.tensors[0][:args.batch_size] if loader is not None else data[:args.batch_size] if data is not None else synthetic_batch(exp, args.batch_size, torch.Generator().manual_seed(args.seed))
        x0 = fixed_binarized(exp, x0)[0]               # --binarize: the init sees 0/1 images, as training will
        n = data_dependent_init(model, x0.to(exp.device))
        if rank == 0:
            print('data-dependent init: %d convolutions rescaled' % n)
    ldist.broadcast_flat(arena.params)
    accum = args.accum_steps
    # (an accumulated step exchanges once, after its last micro-pass: the split form, unless LVAE_DDP_MODE insists, which TrainStep refuses)
    ar_mode = 'split' if accum > 1 and os.environ.get('LVAE_DDP_MODE') is None else None
    allreduce = ldist.GradAllReduce(arena.grads, segments=arena.segments, mode=ar_mode) if world > 1 else None
    # --kl-balance: the KL bookkeeping of every training pass balances the layers' terms while that beta is below 1
    balance = exp._make_kl_balance(args)
    # --beta-anneal: beta is read on the device from a step counter the step advances itself, so the captured graph replays with it
    step_fn = TrainStep(model, opt, beta=1.0, use_graph=not args.no_graph, allreduce=allreduce, beta_anneal=args.beta_anneal,
                        feed=feed, summary=summary, iw_samples=args.iw_train_samples, accum_steps=accum, kl_balance=balance)
    history = History(args.history) if args.history and rank == 0 else None
    guard_seen = opt.guard.counts() if opt.guard is not None else None   # (after --resume: the file's counts)
    # --latent-stats: the first sample of every test batch also folds each layer's posterior into a device accumulator
    latent = LatentStats(model, exp.device, args.latent_kl_threshold, args.latent_var_threshold) if args.latent_stats and tests is not None else None
    # --image-quality: the first sample of every test batch is also judged against its image (mse, PSNR, SSIM), summed on the device
    quality = ImageQuality(exp.device) if args.image_quality and tests is not None else None
    if rank == 0:
        print(exp.run_description)
        print('parameters: %d   world size: %d   per-rank batch: %d' % (sum(p.numel() for p in model.parameters()), world,
                                                                       args.batch_size // world))
    if args.batch_size % world:
        raise SystemExit('--batch-size must be divisible by the world size')
    per_rank = args.batch_size // world
    gen = torch.Generator().manual_seed(args.seed + 1000 * rank)
    steps = args.steps or args.max_steps
    first = model.global_step + 1                      # > 1 after --resume: the run continues where the checkpoint left it
    if feed is not None and rank == 0:
        print('device data: %d images, %.1f MB as %s in device memory, %d steps per epoch' % (feed.N, feed.nbytes / 1e6, feed.kind,
                                                                                          feed.steps_per_epoch))
    if not (loader is not None or data is not None):
        for _ in range((first - 1) * accum):           # the synthetic batches the resumed steps already consumed
            synthetic_batch(exp, per_rank, gen)
    batches = None
    epoch = 0
    t0, seen = time.time(), 0
    for step in range(first, steps + 1):
        if feed is not None:
            epoch = feed.step_epoch(step, accum)       # of the step's first micro-batch
            if epoch >= args.max_epochs:
                break
        elif loader is not None:
            lo, hi = ldist.shard_batch(args.batch_size, rank, world)
            xs = []
            for _ in range(accum):                     # one optimizer step: `accum` batches of --batch-size
                if batches is None:
                    batches = iter(loader.train)
                try:
                    xb = next(batches)[0]
                except StopIteration:                  # next epoch: reshuffled by the DataLoader
                    epoch += 1
                    if epoch >= args.max_epochs:
                        break
                    batches = iter(loader.train)
                    xb = next(batches)[0]
                xs.append(xb[lo:hi])
            if len(xs) < accum:
                break
            x = xs[0] if accum == 1 else torch.cat(xs)
        elif data is not None:
            lo, hi = ldist.shard_batch(args.batch_size, rank, world)
            if accum == 1:
                idx = torch.randint(0, data.shape[0], (args.batch_size,), generator=torch.Generator().manual_seed(args.seed + step))
                x = data[idx[lo:hi]]
            else:                                      # micro-batch j of step s is the batch a plain run draws at its step (s - 1) * M + j
                x = torch.cat([data[torch.randint(0, data.shape[0], (args.batch_size,),
                                                  generator=torch.Generator().manual_seed(args.seed + (step - 1) * accum + j + 1))[lo:hi]]
                               for j in range(accum)])
        else:
            x = synthetic_batch(exp, per_rank, gen) if accum == 1 else torch.cat([synthetic_batch(exp, per_rank, gen) for _ in range(accum)])
        out = step_fn() if feed is not None else step_fn(x.to(exp.device, non_blocking=True))
        seen += args.batch_size * accum
        if summary is not None and (step % args.log_every == 0 or step == steps):
            m = summary.take()                         # a collective: every rank takes its window, rank 0 prints the mean over all
            if rank == 0:
                dt = time.time() - t0
                if opt.schedule is not None:
                    m['lr/lr'] = opt.current_lr()      # of this step, not a window mean: the accumulator's layout stays as it is
                if 'iw' in out:                        # likewise of this step (and of rank 0)
                    m['elbo/iw_train'], m['iw/ess'] = out['iw'].item(), out['ess'].item()
                if opt.guard is not None:              # every rank decides alike: rank 0's counts are the run's
                    guard_seen = guard_metrics(opt.guard, opt.gscale, guard_seen, m, False)
                spectral_metrics(out, m)               # of this step: the accumulator's layout stays as it is
                balance_metrics(balance, m)            # likewise (of this step's last micro-pass, of rank 0)
                print(exp.train_log_str(m, step) + train_line_suffix(m, summary.ranks) + lr_suffix(m) + '   [{:.0f} img/s]'.format(seen / dt)
                      + iw_suffix(m, args.iw_train_samples) + guard_suffix(m) + spectral_suffix(m)
                      + balance_suffix(m, step, args.beta_anneal))
                if history is not None:
                    history.write(step, 'train', m, steps=m['steps'], nonfinite_steps=m['nonfinite_steps'])
            t0, seen = time.time(), 0
        elif rank == 0 and (step % args.log_every == 0 or step == steps):
            m = exp.get_metrics_dict(out)
            dt = time.time() - t0
            if opt.schedule is not None:
                m['lr/lr'] = opt.current_lr()
            if opt.guard is not None:
                guard_seen = guard_metrics(opt.guard, opt.gscale, guard_seen, m, True)
            spectral_metrics(out, m)
            balance_metrics(balance, m)
            print(exp.train_log_str(m, step) + lr_suffix(m) + '   [{:.0f} img/s]'.format(seen / dt) + iw_suffix(m, args.iw_train_samples)
                  + guard_suffix(m) + spectral_suffix(m) + balance_suffix(m, step, args.beta_anneal))
            if history is not None:
                history.write(step, 'train', m)
            t0, seen = time.time(), 0
        n_samples, ckpt = sched.at(step)
        if n_samples:
            if data is not None and loader is None and feed is None:
                epoch = step * args.batch_size * accum // data.shape[0]
            # (--ema-decay: on the averaged weights)
            res = test_pass(model, tests(), n_samples, optimizer=opt, latent_stats=latent, bn_recal=recal, image_quality=quality)
            if rank == 0:
                line = exp.test_log_str(res, step, epoch)
                if latent is not None:
                    line += latent_line_suffix(res, latent.kl_threshold, latent.var_threshold)
                if quality is not None:
                    line += quality_line_suffix(res)
                print(line, flush=True)
                if history is not None:
                    history.write(step, 'test', res, epoch=epoch)
            t0, seen = time.time(), 0                  # the training throughput excludes test passes
        if rank == 0 and args.img_dir and sched.images_at(step):
            # boilr's sample_<step>.png / reconstruction_<step>.png; rank 0 alone, no collective. The reconstructions show the first test
            # batch of this rank's shard, so without a test split there are none
            x_img = next(iter(tests()), None) if tests is not None else None
            sample_grid, recon_grid = image_pass(model, IMG_NROWS, x=x_img, step=step, optimizer=opt, bn_recal=recal)
            os.makedirs(args.img_dir, exist_ok=True)
            write_png(os.path.join(args.img_dir, 'sample_%d.png' % step), sample_grid)
            if recon_grid is not None:
                write_png(os.path.join(args.img_dir, 'reconstruction_%d.png' % step), recon_grid)
            t0, seen = time.time(), 0                  # nor the pictures
        if ckpt and rank == 0:
            os.makedirs(args.checkpoint_dir, exist_ok=True)
            save_checkpoint(checkpoint_path(args.checkpoint_dir, step), model, opt, summary=summary, bn_recal=recal)
            for name in checkpoints_to_delete(os.listdir(args.checkpoint_dir), args.keep_checkpoint_max):
                os.remove(os.path.join(args.checkpoint_dir, name))
    if args.save_checkpoint and rank == 0:
        save_checkpoint(args.save_checkpoint, model, opt, summary=summary, bn_recal=recal)
    if history is not None:
        history.close()
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
