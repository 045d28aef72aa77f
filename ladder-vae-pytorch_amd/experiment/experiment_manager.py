"""Experiment glue on the HIP engine — the hooks of the reference's experiment/experiment_manager.py:17-415
(`LVAEExperiment`) that the training hot path needs, re-hosted without `boilr` (absent):

  * the command-line flag surface of `_add_args` (:107-259) and the overridden defaults (:88-103), plus the boilr-owned
    flags seen at call sites (--seed, --batch-size, --lr, ...), plus engine flags (--synthetic, --steps, --no-graph);
  * `_check_args` (:262-290), `_make_run_description` (:293-320);
  * `_make_model` (:38-74), `_make_optimizer` (:76-81, Adamax) and `forward_pass` (:322-367);
  * `train_log_str` / `test_log_str` / `get_metrics_dict` (:369-415).

Out of scope: tensorboard, dataset downloads. main.py drives a minimal loop over a dataset, synthetic batches
or an .npz file with the same log lines, test passes, log-likelihood estimates, checkpoint rotation (schedule.py) and picture grids (images.py).
"""
import argparse

import torch

from .. import engine
from ..models.lvae import LadderVAE
from ..noise import PhiloxNoise
from ..optim import Adam, AdamW, Adamax, GradGuard, LrSchedule

DATASETS = {
    # name: (color_ch, (H, W), default likelihood)  — experiment/data.py:32-97, experiment_manager.py:279-288
    'static_mnist': (1, (28, 28), 'bernoulli'),
    'cifar10': (3, (32, 32), 'discr_log_mix'),
    'svhn': (3, (32, 32), 'discr_log_mix'),
    'celeba': (3, (64, 64), 'discr_log_mix'),
    'multi_dsprites_binary_rgb': (3, (64, 64), 'bernoulli'),
    'multi_mnist_binary': (1, (64, 64), 'bernoulli'),
}


def build_parser():
    p = argparse.ArgumentParser(description='Ladder VAE on MI355X (HIP engine)', allow_abbrev=False,
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    # boilr-owned flags visible at the reference's call sites, with the defaults of experiment_manager.py:88-103
    p.add_argument('--batch-size', type=int, default=64, dest='batch_size')
    p.add_argument('--test-batch-size', type=int, default=1000, dest='test_batch_size')
    p.add_argument('--lr', type=float, default=3e-4)
    p.add_argument('--seed', type=int, default=54321)
    p.add_argument('--tr-log-every', type=int, default=10000, dest='train_log_every')
    p.add_argument('--ts-log-every', type=int, default=10000, dest='test_log_every')
    p.add_argument('--ts-img-every', type=int, default=-1, dest='test_imgs_every')
    p.add_argument('--checkpoint-every', type=int, default=100000, dest='checkpoint_every')
    p.add_argument('--keep-checkpoint-max', type=int, default=2, dest='keep_checkpoint_max')
    p.add_argument('--max-steps', type=int, default=10 ** 10, dest='max_steps')
    p.add_argument('--max-epochs', type=int, default=10 ** 7, dest='max_epochs')
    p.add_argument('--nocuda', action='store_true', dest='no_cuda')
    p.add_argument('--descr', type=str, default='', dest='additional_descr')
    p.add_argument('--dry-run', action='store_true', dest='dry_run')
    p.add_argument('--resume', type=str, default='')
    p.add_argument('--ll-every', type=int, default=50000, dest='loglikelihood_every')
    p.add_argument('--ll-samples', type=int, default=100, dest='loglikelihood_samples')
    # experiment_manager.py:107-259
    p.add_argument('-d', '--dataset', type=str, choices=list(DATASETS), default='static_mnist', dest='dataset_name')
    p.add_argument('--likelihood', type=str, choices=['bernoulli', 'gaussian', 'discr_log', 'discr_log_mix'], default=None)
    p.add_argument('--zdims', type=int, nargs='+', default=[32, 32, 32], dest='z_dims')
    p.add_argument('--blocks-per-layer', type=int, default=2, dest='blocks_per_layer')
    p.add_argument('--nfilters', type=int, default=64, dest='n_filters')
    p.add_argument('--no-bn', action='store_true', dest='no_batch_norm')
    p.add_argument('--skip', action='store_true', dest='skip_connections')
    p.add_argument('--gated', action='store_true', dest='gated')
    p.add_argument('--downsample', type=int, nargs='+', default=[1, 1, 1])
    p.add_argument('--learn-top-prior', action='store_true', dest='learn_top_prior')
    p.add_argument('--residual-type', type=str, default='bacdbacd', dest='residual_type')
    p.add_argument('--merge-layers', type=str, choices=['linear', 'residual'], default='residual', dest='merge_layers')
    p.add_argument('--beta-anneal', type=int, default=0, dest='beta_anneal')
    p.add_argument('--data-dep-init', action='store_true', dest='simple_data_dependent_init')
    p.add_argument('--wd', type=float, default=0.0, dest='weight_decay')
    p.add_argument('--nonlin', type=str, choices=['relu', 'leakyrelu', 'elu', 'selu'], default='elu')
    p.add_argument('--dropout', type=float, default=0.2)
    p.add_argument('--freebits', type=float, default=0.0, dest='free_bits')
    p.add_argument('--analytical-kl', action='store_true', dest='analytical_kl')
    p.add_argument('--no-initial-downscaling', action='store_true', dest='no_initial_downscaling')
    # engine flags (new)
    p.add_argument('--synthetic', action='store_true', help='train on synthetic batches (no dataset files needed)')
    p.add_argument('--data-npz', type=str, default='', help="train on an .npz with key 'data' (N,C,H,W) float32 in [0,1]")
    p.add_argument('--dtype', type=str, choices=['f32', 'bf16'], default='f32', dest='compute_dtype',
                   help='bf16: bf16 matrix-core operands, fp32 accumulate / statistics / KL / likelihood')
    p.add_argument('--steps', type=int, default=0, help='stop after this many steps (0: --max-steps)')
    p.add_argument('--no-graph', action='store_true', help='launch eagerly instead of replaying a captured hipGraph')
    p.add_argument('--log-every', type=int, default=100)
    p.add_argument('--save-checkpoint', type=str, default='', help='write a reference-layout checkpoint here at the end')
    p.add_argument('--checkpoint-dir', type=str, default='', dest='checkpoint_dir',
                   help='write <dir>/model_<step>.pt every --checkpoint-every steps, keeping the newest --keep-checkpoint-max')
    p.add_argument('--synthetic-test', type=int, default=0, dest='synthetic_test', metavar='N',
                   help='with --synthetic: a fixed seeded test set of N images for the --ts-log-every / --ll-every test passes')
    p.add_argument('--img-dir', type=str, default='', dest='img_dir', metavar='DIR',
                   help='trainer: write DIR/sample_<step>.png and, with a test split, DIR/reconstruction_<step>.png every --ts-img-every '
                        'steps; evaluate: also write the picture grids of --ps, --layer-repr and --recons there')
    p.add_argument('--device-data', action='store_true', dest='device_data',
                   help='keep the training set (and the test split) in device memory and gather every batch inside the step; the data '
                        'order is then a function of --seed and the step, so runs with a data set repeat and --resume continues exactly. '
                        'With a data set (-d) or --data-npz; not with --synthetic')
    p.add_argument('--binarize', action='store_true',
                   help='with --device-data and the bernoulli likelihood: dynamic binarization, every grey pixel drawn afresh as Bernoulli(value) '
                        'each time the gather visits it, inside the gather launch; test, data-dependent-init and recalibration images get one fixed '
                        'binarization per image (a function of --seed and the image number)')
    p.add_argument('--hflip', action='store_true',
                   help='with --device-data: mirror each training image left-right with probability 1/2, inside the gather launch')
    p.add_argument('--dequantize', action='store_true',
                   help='with --device-data, 8-bit data and the gaussian likelihood: train on (b + u) / 256 with u uniform in (0, 1), added inside '
                        'the gather launch')
    p.add_argument('--ema-decay', type=_ema_decay, default=0.0, dest='ema_decay', metavar='D',
                   help='keep an exponential moving average of the weights inside the optimizer step (decay ramps up as min(D, (1+n)/(10+n))); '
                        'test and log-likelihood passes then use the averaged weights and checkpoints carry them. 0: off')
    p.add_argument('--ema-bn-batches', type=int, default=0, dest='ema_bn_batches', metavar='N',
                   help='with --ema-decay: before every test, log-likelihood and picture pass on the averaged weights, re-estimate the BatchNorm '
                        'running statistics for them on the first N batches of --batch-size training images (train-mode forwards, equal-weight '
                        'mean of the batch statistics), and put the live statistics back afterwards; checkpoints store the recalibrated '
                        "statistics in their 'ema' entry. 0: off (the averaged weights are evaluated with the live weights' statistics)")
    p.add_argument('--window-summaries', action='store_true', dest='window_summaries',
                   help='the train line prints the mean of every step since the previous train line, over all ranks (summed on the device '
                        'inside the step), with the gradient norm and the number of non-finite steps, instead of the last step of rank 0')
    p.add_argument('--history', type=str, default='', metavar='FILE',
                   help='rank 0 appends one JSON object per printed train and test line to FILE (JSONL)')
    p.add_argument('--latent-stats', action='store_true', dest='latent_stats',
                   help='every test / log-likelihood pass also counts, per stochastic layer, the latent units in use (summed on the device '
                        'during the pass): units whose mean KL(q||p) over the test images exceeds --latent-kl-threshold, and units whose '
                        'posterior mean varies over them by more than --latent-var-threshold; printed after the test line')
    p.add_argument('--lr-schedule', type=str, choices=['constant', 'cosine', 'linear', 'step', 'exp'], default='constant', dest='lr_schedule',
                   help='after --lr-warmup: keep --lr, or bring it down over --lr-decay-steps steps (cosine / linear: to --lr-min; step: times '
                        '--lr-gamma every --lr-decay-steps steps; exp: times --lr-gamma per --lr-decay-steps steps, continuously; both not '
                        'below --lr-min). Computed on the device from the optimizer step counter, inside the captured step')
    p.add_argument('--lr-warmup', type=int, default=0, dest='lr_warmup', metavar='N', help='raise the lr linearly over the first N steps')
    p.add_argument('--lr-decay-steps', type=int, default=0, dest='lr_decay_steps', metavar='T')
    p.add_argument('--lr-min', type=float, default=0.0, dest='lr_min')
    p.add_argument('--lr-gamma', type=float, default=0.1, dest='lr_gamma')
    p.add_argument('--iw-train-samples', type=int, default=1, dest='iw_train_samples', metavar='K',
                   help='train on the K-sample importance-weighted bound instead of the ELBO: K samples per image share one bottom-up pass '
                        '(--batch-size stays images per step); the train line adds the bound and the effective sample size of the weights. '
                        'Not with --freebits or --analytical-kl. 1: the ELBO')
    p.add_argument('--residual-posterior', action='store_true', dest='residual_posterior',
                   help="every layer's inference path predicts its posterior as an offset from the prior of the same layer (NVAE's residual "
                        'normal): mu_q = mu_p + dmu, logvar_q = logvar_p + dlv, and the KL is formed from the offset. Same parameters and '
                        'state_dict; checkpoints note the setting, and --resume under the other one is refused. Off by default')
    p.add_argument('--accum-steps', type=int, default=1, dest='accum_steps', metavar='M',
                   help='every optimizer step consumes M micro-batches of --batch-size images: the gradient applied is the mean over all '
                        'M * batch-size images, BatchNorm normalises over one micro-batch, and steps (--log-every, the lr schedule, beta '
                        'warm-up, test and checkpoint cadence) count optimizer steps. 1: one batch per step')
    p.add_argument('--max-grad-norm', type=float, default=None, dest='max_grad_norm', metavar='G',
                   help='clip the gradient to the global L2 norm G before the optimizer step (the factor of torch.nn.utils.clip_grad_norm_), '
                        'decided on the device inside the captured step; steps with a non-finite gradient are then skipped. Off by default')
    p.add_argument('--grad-skip-threshold', type=float, default=None, dest='grad_skip_threshold', metavar='T',
                   help='skip every step whose gradient norm exceeds T or is not finite: weights, optimizer state, average and BatchNorm '
                        'statistics stay as they were, the run moves on to the next batch. inf: skip non-finite steps only. Off by default')
    p.add_argument('--optimizer', type=str, choices=['adamax', 'adam', 'adamw'], default='adamax',
                   help="the update rule, on the same arena, average, schedule and guard: adamax (the reference's), adam (--wd is L2 decay "
                        'added to the gradient) or adamw (--wd is decoupled decay: the weights shrink by lr * wd per step)')
    p.add_argument('--betas', type=float, nargs=2, default=[0.9, 0.999], metavar=('B1', 'B2'), help='the moments\' decay rates, for every rule')
    p.add_argument('--opt-eps', type=float, default=1e-8, dest='opt_eps', metavar='E', help='the eps of the update rule, for every rule')
    p.add_argument('--image-quality', action='store_true', dest='image_quality',
                   help='every test / log-likelihood pass also measures its reconstructions against the test images on the device (the first '
                        "sample of every batch: the likelihood's mean, or its sample where it has none): the mean PSNR and SSIM are printed "
                        "after the test line and --history records the quality/* values")
    p.add_argument('--spectral-reg', type=float, default=0.0, dest='spectral_reg', metavar='LAMBDA',
                   help="add LAMBDA times the sum of the convolution weights' spectral norms to the objective (NVAE's spectral regularisation): "
                        'one power-iteration step per optimizer step over every convolution, inside the captured step; the train line adds '
                        'the sum and the largest of the norms. The printed loss does not include the penalty. 0: off')
    p.add_argument('--spectral-warm-iters', type=int, default=10, dest='spectral_warm_iters', metavar='N',
                   help='with --spectral-reg: power iterations run before the first step, from the seeded start vectors')
    p.add_argument('--kl-balance', type=str, choices=['equal', 'sqrt', 'linear', 'square'], default=None, dest='kl_balance', metavar='RULE',
                   help="with --beta-anneal: NVAE's KL balancing. While beta < 1 the per-layer KL terms of the objective are reweighted by "
                        'coefficients that average 1 (a layer whose KL is small pays less, one whose KL is large pays more), decided on the '
                        "device inside the captured step; exactly 1 once beta has reached 1. RULE sets the layers' fixed weights from their "
                        'latent height r relative to the smallest: equal 1, sqrt sqrt(r), linear r, square r^2 / (layers of that size), '
                        "NVAE's choice. The train line adds the range of the coefficients; the printed loss is the balanced objective, ELBO, "
                        'KL and recons stay the plain numbers. Off by default')
    p.add_argument('--latent-kl-threshold', type=float, default=0.01, dest='latent_kl_threshold', metavar='T')
    p.add_argument('--latent-var-threshold', type=float, default=0.01, dest='latent_var_threshold', metavar='T')
    return p


def _ema_decay(s):
    d = float(s)
    if not 0.0 <= d < 1.0:
        raise argparse.ArgumentTypeError('--ema-decay must lie in [0, 1), got %s' % s)
    return d


class LVAEExperiment:
    """Holds args, model, optimizer; `forward_pass` is the hot path (experiment_manager.py:322-367)."""

    def __init__(self, args=None, argv=None):
        if args is None:
            args = build_parser().parse_args(argv)
        self.args = self._check_args(args)
        self.run_description = self._make_run_description(self.args)
        if self.args.no_cuda or not torch.cuda.is_available():
            raise RuntimeError("the HIP engine needs an MI355X: no CPU path exists in the product (--nocuda is rejected)")
        self.device = torch.device('cuda', torch.cuda.current_device())
        self.color_ch, self.img_size, _ = DATASETS[self.args.dataset_name]
        self.model = self._make_model()
        self.optimizer = self._make_optimizer()

    @classmethod
    def _check_args(cls, args):
        if len(args.z_dims) != len(args.downsample):
            raise RuntimeError("length of list of latent dimensions ({}) does not match length of list of downsampling "
                               "factors ({})".format(len(args.z_dims), len(args.downsample)))
        if getattr(args, 'device_data', False) and args.synthetic:
            raise SystemExit("--device-data feeds the step from a data set kept in device memory; --synthetic has none "
                             "(use --device-data with -d DATASET or --data-npz FILE)")
        aug = [f for f in ('binarize', 'hflip', 'dequantize') if getattr(args, f, False)]
        if aug and not getattr(args, 'device_data', False):
            raise SystemExit("--%s augments the batch inside the device-fed gather: it needs --device-data" % aug[0])
        if 'binarize' in aug and 'dequantize' in aug:
            raise SystemExit("--binarize and --dequantize exclude each other: one makes 0/1 pixels, the other continuous ones")
        likelihood = args.likelihood if args.likelihood is not None else DATASETS[args.dataset_name][2]
        if 'binarize' in aug and likelihood != 'bernoulli':
            raise SystemExit("--binarize makes 0/1 images: it needs --likelihood bernoulli, not %s" % likelihood)
        if 'dequantize' in aug and likelihood != 'gaussian':
            raise SystemExit("--dequantize needs --likelihood gaussian, not %s: the discretized heads need the k/255 grid" % likelihood)
        if getattr(args, 'lr_schedule', 'constant') != 'constant' and args.lr_decay_steps <= 0:
            raise SystemExit("--lr-schedule %s needs --lr-decay-steps > 0" % args.lr_schedule)
        if getattr(args, 'lr_min', 0.0) > args.lr:
            raise SystemExit("--lr-min %g exceeds --lr %g" % (args.lr_min, args.lr))
        iw = getattr(args, 'iw_train_samples', 1)
        if iw < 1:
            raise SystemExit("--iw-train-samples must be at least 1, got %d" % iw)
        if iw > 1 and args.free_bits > 0:
            raise SystemExit("--iw-train-samples %d cannot be combined with --freebits %g: the free-bits clamp has no importance-weighted form" % (iw, args.free_bits))
        if iw > 1 and args.analytical_kl:
            raise SystemExit("--iw-train-samples %d cannot be combined with --analytical-kl: the importance weights need the Monte-Carlo "
                             "log q - log p of the drawn sample" % iw)
        bn_batches = getattr(args, 'ema_bn_batches', 0)
        if bn_batches < 0:
            raise SystemExit("--ema-bn-batches must not be negative, got %d" % bn_batches)
        if bn_batches > 0 and not getattr(args, 'ema_decay', 0.0) > 0.0:
            raise SystemExit("--ema-bn-batches %d recalibrates BatchNorm for the averaged weights: it needs --ema-decay > 0" % bn_batches)
        if getattr(args, 'accum_steps', 1) < 1:
            raise SystemExit("--accum-steps must be at least 1, got %d" % args.accum_steps)
        g, t = getattr(args, 'max_grad_norm', None), getattr(args, 'grad_skip_threshold', None)
        if g is not None and not (g > 0.0 and g != float('inf')):
            raise SystemExit("--max-grad-norm must be a positive finite number, got %g" % g)
        if t is not None and not t >= 0.0:
            raise SystemExit("--grad-skip-threshold must not be negative, got %g" % t)
        betas = getattr(args, 'betas', [0.9, 0.999])
        if len(betas) != 2 or not all(0.0 <= b < 1.0 for b in betas):
            raise SystemExit("--betas must be two numbers in [0, 1), got %s" % ' '.join('%g' % b for b in betas))
        if not getattr(args, 'opt_eps', 1e-8) >= 0.0:
            raise SystemExit("--opt-eps must not be negative, got %g" % args.opt_eps)
        lam = getattr(args, 'spectral_reg', 0.0)
        if not (lam >= 0.0 and lam != float('inf')):
            raise SystemExit("--spectral-reg must be a finite number that is not negative, got %g" % lam)
        if getattr(args, 'spectral_warm_iters', 10) < 0:
            raise SystemExit("--spectral-warm-iters must not be negative, got %d" % args.spectral_warm_iters)
        klb = getattr(args, 'kl_balance', None)
        if klb is not None and args.beta_anneal == 0:
            raise SystemExit("--kl-balance %s balances the KL terms while beta < 1: without --beta-anneal beta is 1 from the first step and "
                             "the flag would do nothing (add --beta-anneal STEPS)" % klb)
        if klb is not None and iw > 1:
            raise SystemExit("--kl-balance %s cannot be combined with --iw-train-samples %d: the importance-weighted bound is formed from "
                             "the per-row KL and has no balanced form" % (klb, iw))
        assert args.weight_decay >= 0.0
        assert 0.0 <= args.dropout <= 1.0
        if args.dropout < 1e-5:
            args.dropout = None
        assert args.free_bits >= 0.0
        args.batch_norm = not args.no_batch_norm
        if args.likelihood is None:
            args.likelihood = DATASETS[args.dataset_name][2]
        return args

    @staticmethod
    def _make_run_description(args):
        s = args.dataset_name
        s += ',{}ly'.format(len(args.z_dims))
        s += ',{}bpl'.format(args.blocks_per_layer)
        s += ',{}ch'.format(args.n_filters)
        if args.skip_connections:
            s += ',skip'
        if args.gated:
            s += ',gate'
        s += ',block=' + args.residual_type
        if args.beta_anneal != 0:
            s += ',b{}'.format(args.beta_anneal)
        if getattr(args, 'iw_train_samples', 1) > 1:
            s += ',iw{}'.format(args.iw_train_samples)
        if getattr(args, 'accum_steps', 1) > 1:
            s += ',acc{}'.format(args.accum_steps)
        if getattr(args, 'residual_posterior', False):
            s += ',resq'
        for flag, word in (('binarize', ',binarize'), ('hflip', ',hflip'), ('dequantize', ',dequant')):
            if getattr(args, flag, False):
                s += word
        s += ',{}'.format(args.nonlin)
        if args.free_bits > 0:
            s += ',freeb={}'.format(args.free_bits)
        if args.dropout is not None:
            s += ',drop={}'.format(args.dropout)
        if args.learn_top_prior:
            s += ',learnp'
        if args.weight_decay > 0.0:
            s += ',wd={}'.format(args.weight_decay)
        if getattr(args, 'optimizer', 'adamax') != 'adamax':
            s += ',' + args.optimizer
        if list(getattr(args, 'betas', [0.9, 0.999])) != [0.9, 0.999]:
            s += ',b{:g}-{:g}'.format(*args.betas)
        if getattr(args, 'max_grad_norm', None) is not None:
            s += ',clip{:g}'.format(args.max_grad_norm)
        if getattr(args, 'grad_skip_threshold', None) is not None:
            s += ',skip{:g}'.format(args.grad_skip_threshold)
        if getattr(args, 'spectral_reg', 0.0) > 0.0:
            s += ',sr{:g}'.format(args.spectral_reg)
        if getattr(args, 'kl_balance', None) is not None:
            s += ',klb-{}'.format(args.kl_balance)
        s += ',seed{}'.format(args.seed)
        if len(args.additional_descr) > 0:
            s += ',' + args.additional_descr
        return s

    def _make_model(self):
        a = self.args
        torch.manual_seed(a.seed)
        model = LadderVAE(self.color_ch, z_dims=a.z_dims, blocks_per_layer=a.blocks_per_layer, downsample=a.downsample,
                          merge_type=a.merge_layers, batchnorm=a.batch_norm, nonlin=a.nonlin,
                          stochastic_skip=a.skip_connections, n_filters=a.n_filters, dropout=a.dropout,
                          res_block_type=a.residual_type, free_bits=a.free_bits, learn_top_prior=a.learn_top_prior,
                          img_shape=self.img_size, likelihood_form=a.likelihood, gated=a.gated,
                          no_initial_downscaling=a.no_initial_downscaling, analytical_kl=a.analytical_kl).to(self.device)
        model.noise = PhiloxNoise(seed=a.seed)
        model.compute_dtype = a.compute_dtype
        model.residual_posterior = getattr(a, 'residual_posterior', False)   # (noted in checkpoints and checked on load)
        model.iw_train_samples = getattr(a, 'iw_train_samples', 1)   # (noted in checkpoints: checkpoint.save_checkpoint)
        model.accum_steps = getattr(a, 'accum_steps', 1)             # (likewise)
        model.ema_bn_batches = getattr(a, 'ema_bn_batches', 0)       # (likewise, when it is not 0)
        model.augment = self.augment_record(a)                        # (likewise, when there is one)
        # (the KlBalance itself reaches the model through engine.TrainStep(kl_balance=), which binds its beta source)
        model.kl_balance_record = getattr(a, 'kl_balance', None)      # (likewise: the rule of --kl-balance)
        return model

    @staticmethod
    def feed_augment(args):
        """The data.FeedAugment of --binarize / --hflip / --dequantize; None without any."""
        from ..data import FeedAugment
        aug = FeedAugment(getattr(args, 'binarize', False), getattr(args, 'hflip', False), getattr(args, 'dequantize', False))
        return aug if aug else None

    @classmethod
    def augment_record(cls, args):
        """What a checkpoint notes under 'augment': the FeedAugment's record and the data seed its noise comes from; None without any."""
        aug = cls.feed_augment(args)
        return None if aug is None else dict(aug.record(), seed=int(args.seed))

    @staticmethod
    def _make_schedule(args):
        """The LrSchedule of the --lr-* flags; None (the plain optimizer step) unless one of them asks for a moving lr."""
        if getattr(args, 'lr_warmup', 0) <= 0 and getattr(args, 'lr_schedule', 'constant') == 'constant':
            return None
        try:
            return LrSchedule(args.lr_schedule, args.lr_warmup, args.lr_decay_steps, args.lr_min, args.lr_gamma)
        except ValueError as e:
            raise SystemExit(str(e))

    @staticmethod
    def _make_guard(args):
        """The GradGuard of --max-grad-norm / --grad-skip-threshold; None (the plain step) without either."""
        g, t = getattr(args, 'max_grad_norm', None), getattr(args, 'grad_skip_threshold', None)
        return None if g is None and t is None else GradGuard(max_norm=g, skip_threshold=t)

    @staticmethod
    def _make_spectral(args):
        """The SpectralReg of --spectral-reg / --spectral-warm-iters; None (the plain step) at 0."""
        if not getattr(args, 'spectral_reg', 0.0) > 0.0:
            return None
        from ..spectral import SpectralReg
        return SpectralReg(args.spectral_reg, warm_iters=getattr(args, 'spectral_warm_iters', 10), seed=args.seed)

    @staticmethod
    def _make_kl_balance(args):
        """The balance.KlBalance of --kl-balance; None (the plain KL bookkeeping) without the flag."""
        if getattr(args, 'kl_balance', None) is None:
            return None
        from ..balance import KlBalance
        return KlBalance(args.kl_balance)

    def _make_optimizer(self):
        a = self.args
        rule = {'adamax': Adamax, 'adam': Adam, 'adamw': AdamW}[getattr(a, 'optimizer', 'adamax')]
        return rule(self.model, lr=a.lr, betas=tuple(getattr(a, 'betas', (0.9, 0.999))), eps=getattr(a, 'opt_eps', 1e-8),
                    weight_decay=a.weight_decay, ema_decay=getattr(a, 'ema_decay', 0.0), schedule=self._make_schedule(a),
                    guard=self._make_guard(a), spectral=self._make_spectral(a))

    def beta(self):
        if self.args.beta_anneal != 0:
            return engine.linear_anneal(self.model.global_step, 0.0, 1.0, self.args.beta_anneal)
        return 1.0

    def forward_pass(self, x, y=None):
        x = x.to(self.device, non_blocking=True)
        return engine.forward_pass(self.model, x, self.beta(), iw_samples=getattr(self.args, 'iw_train_samples', 1))

    @classmethod
    def train_log_str(cls, summaries, step, epoch=None):
        s = "       [step {}]   loss: {:.5g}   ELBO: {:.5g}   recons: {:.3g}   KL: {:.3g}"
        return s.format(step, summaries['loss/loss'], summaries['elbo/elbo'], summaries['elbo/recons'], summaries['elbo/kl'])

    @classmethod
    def test_log_str(cls, summaries, step, epoch=None):
        s = "       "
        if epoch is not None:
            s += "[step {}, epoch {}]   ".format(step, epoch)
        if summaries.get('weights') == 'ema':
            s += "[averaged weights]   "
        if summaries.get('bn_recal/rounds'):
            s += "[BatchNorm recalibrated on {} batches]   ".format(summaries['bn_recal/rounds'])
        s += "ELBO {:.5g}   recons: {:.3g}   KL: {:.3g}".format(summaries['elbo/elbo'], summaries['elbo/recons'],
                                                               summaries['elbo/kl'])
        for k in summaries.keys():
            if k.find('elbo_IW') > -1:
                s += "   marginal log-likelihood ({}) {:.5g}".format(k.split('_')[-1], summaries[k])
                break
        return s

    @classmethod
    def get_metrics_dict(cls, results):
        d = {'loss/loss': results['loss'].item(), 'elbo/elbo': results['elbo'].item(),
             'elbo/recons': results['recons'].item(), 'elbo/kl': results['kl'].item(), 'l2/l2': results['l2'].item()}
        if 'iw' in results:   # a step trained on the K-sample bound (--iw-train-samples): the bound at beta = 1, the weights' effective sample size
            d['elbo/iw_train'], d['iw/ess'] = results['iw'].item(), results['ess'].item()
        if 'kl_avg_layerwise' in results:
            for i in range(len(results['kl_avg_layerwise'])):
                d['kl_layers/kl_layer_{}'.format(i)] = results['kl_avg_layerwise'][i].item()
        return d
