"""BatchNorm statistics that belong to the weights being evaluated.

`--ema-decay` averages the trainable parameters only: the averaged weights would otherwise be evaluated with the running_mean / running_var
the LIVE weights' activations produced. Likewise the sampling features (`sample_prior(temperature=t)`, `sample_conditional`, `decode`,
`interpolate`) push activations of another spread through BatchNorms whose statistics were collected at t = 1 under the posterior.
`recalibrate_bn` re-estimates the statistics the way torch.optim.swa_utils.update_bn does (momentum=None: the equal-weight mean of the
per-batch means and unbiased variances), without touching a convolution kernel:

  * every BatchNorm2dParams gets momentum 1 for the duration, so a train-mode forward leaves exactly its batch statistics in the running
    buffers, in every fused form (`bn_update_running` of csrc/bn_stats.h is the one place they are written: 0 * r0 + 1 * s);
  * after each forward one launch adds all of them, widened to double, to an accumulator (kernels.bn_recal_fold), and after the last one a
    second launch writes the means back (kernels.bn_recal_finish), reading the number of rounds on the device: a round can be captured as
    a hipGraph and replayed (passes.replay_loop), eager and replayed results agree bit for bit.

The old statistics stay in a shadow (one launch, as optim.GradGuard keeps them for a skipped step): `restore()` puts them back, which is what
the trainer does after a test pass on the averaged weights. A BatchNorm no round ran (the bottom-up and merge layers under the prior source)
gets its old statistics back inside the call, bit for bit.
"""
import contextlib

import torch

from . import kernels as K
from .noise import PhiloxNoise
from .passes import replay_loop

RECAL_NOISE_TAG = 0xB7C4A1      # the recalibration noise stream's seed is the model's seed with these bits flipped
RECAL_NOISE_STRIDE = 1 << 20    # and its counter starts at step * this (the rule of evaluate.image_pass)
GRAPH_MIN_ROUNDS = 8


def recal_noise(model, step=0):
    """A fresh PhiloxNoise made from the model's seed and `step`: never `model.noise` or `model.test_noise`, so a recalibration draws the
    same numbers whatever ran before it and leaves every other stream where it stands."""
    dev = next(model.parameters()).device
    noise = PhiloxNoise(0)
    noise.seed = (model.noise.seed if isinstance(model.noise, PhiloxNoise) else 0) ^ RECAL_NOISE_TAG
    noise.step = torch.full((1,), int(step) * RECAL_NOISE_STRIDE, dtype=torch.int64, device=dev)
    return noise


class BnRecalibrator:
    """Owns, for one model: the shadow of every running_mean / running_var with the tables that save and restore it, the table that sets
    the statistics to 0 / 1, the float64 accumulators with their fold / finish table, the device round count and the non-finite flag.
    Built on first use and again when the buffers have moved (`.to()`, load into new storages)."""

    def __init__(self, model):
        self.model = model
        self._key = None
        self.bns, self.bufs = [], []
        self.shadow = self.acc = self.count = self.flag = None
        self._save = self._restore = self._reset = self._table = self._init = self._parts = None

    def attach(self):
        bns = self.model.bn_modules()
        bufs = [b for bn in bns for b in (bn.running_mean, bn.running_var)]
        key = tuple(b.data_ptr() for b in bufs)
        if key == self._key:
            return self
        self._key, self.bns, self.bufs = key, bns, bufs
        self.shadow = self._save = self._restore = self._reset = self._table = None
        if not bufs:
            return self
        dev = bufs[0].device
        sizes = [b.numel() for b in bufs]
        self.shadow = torch.zeros(sum(sizes), dtype=torch.float32, device=dev)
        self._init = torch.cat([torch.full((n,), float(i % 2), dtype=torch.float32) for i, n in enumerate(sizes)]).to(dev)   # mean 0, var 1
        self.acc = torch.zeros(sum(sizes), dtype=torch.float64, device=dev)
        self.count = torch.zeros(2, dtype=torch.int64, device=dev)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self._parts = torch.split(self.shadow, sizes)
        self._save = K.copy_table(list(zip(self._parts, bufs)), dev)
        self._restore = K.copy_table(list(zip(bufs, self._parts)), dev)
        self._reset = K.copy_table(list(zip(bufs, torch.split(self._init, sizes))), dev)
        self._table = K.bn_recal_table(list(zip(bufs, torch.split(self.acc, sizes))), dev)
        return self

    @property
    def n_bn(self):
        return len(self.bns)

    def restore(self):
        """The statistics the last `run` found, back into the running buffers (one launch). Nothing to do for a model without BatchNorm."""
        if self._restore is not None:
            K.multi_copy(self._restore)

    def _restore_untouched(self, touched):
        """The shadow back into both statistics of every BatchNorm no round ran (they hold the 0 / 1 they were set to): one launch."""
        pairs = [(self.bufs[j], self._parts[j]) for i, t in enumerate(touched) if not t for j in (2 * i, 2 * i + 1)]
        if pairs:
            K.multi_copy(K.copy_table(pairs, self.bufs[0].device))

    def run(self, batches=None, *, n_prior=0, prior_batch=None, temperature=None, noise=None, use_graph=None, step=0):
        """See `recalibrate_bn`."""
        model = self.model
        n_prior = int(n_prior)
        if (batches is None) == (n_prior <= 0):
            raise ValueError("recalibrate_bn takes exactly one source: `batches`, or n_prior > 0 rounds from the prior")
        dev = next(model.parameters()).device
        if batches is not None:
            batches = [b for b in batches]
            if not batches:
                raise ValueError("recalibrate_bn: `batches` is empty")
            rounds, source = len(batches), 'data'
        else:
            if prior_batch is None or int(prior_batch) < 1:
                raise ValueError("the prior source needs prior_batch >= 1 rows per round, got %r" % (prior_batch,))
            from .models.lvae import layer_temperatures
            layer_temperatures(model.n_layers, temperature)   # (refused here, before anything is changed)
            rounds, source, prior_batch = n_prior, 'prior', int(prior_batch)
        if noise is None:
            noise = recal_noise(model, step)
        on_device = isinstance(noise, PhiloxNoise)
        same_shape = batches is None or all(tuple(b.shape) == tuple(batches[0].shape) for b in batches)
        if use_graph is None:
            use_graph = on_device and same_shape and rounds >= GRAPH_MIN_ROUNDS
        elif use_graph and not on_device:
            raise ValueError("use_graph needs on-device noise (PhiloxNoise): a noise tape runs eagerly")
        elif use_graph and not same_shape:
            raise ValueError("use_graph needs batches of one shape")
        use_graph = bool(use_graph) and rounds > 2   # (the two eager rounds are all there is otherwise)
        self.attach()
        info = {'rounds': rounds, 'source': source, 'n_bn': self.n_bn}
        if not self.bns:
            return info
        bns = self.bns
        pending0, momentum0 = [bn._pending for bn in bns], [bn.momentum for bn in bns]
        was_training, old_noise = model.training, model.noise
        balance, model.kl_balance = getattr(model, 'kl_balance', None), None   # (train-mode forwards, but no training: the plain bookkeeping)
        K.multi_copy(self._save)
        done = False
        keep = []
        try:
            # 0 / 1 first: with momentum 1 the update is 0 * r0 + s, and a non-finite r0 would come through the product
            K.multi_copy(self._reset)
            self.acc.zero_()
            self.count.zero_()
            self.flag.zero_()
            for bn in bns:
                bn.momentum = 1.0
            model.train()
            model.noise = noise
            from .evaluate import _EvalWeights
            with torch.no_grad(), _EvalWeights(keep):
                if source == 'data':
                    cur = [batches[0].to(dev).contiguous().float().clone()]   # with one shape: the static input of a captured round

                    def forward():
                        model(cur[0])

                    def between(i, _):
                        if i + 1 < rounds and same_shape:
                            cur[0].copy_(batches[i + 1].to(dev))
                        elif i + 1 < rounds:
                            cur[0] = batches[i + 1].to(dev).contiguous().float()
                else:
                    def forward():
                        model.sample_prior(prior_batch, temperature=temperature)
                    between = None

                def one_round():
                    forward()
                    K.bn_recal_fold(self._table, self.count)

                replay_loop(one_round, rounds, use_graph, between)
                touched = [bn._pending != p0 for bn, p0 in zip(bns, pending0)]
                K.bn_recal_finish(self._table, self.count, self.flag)
                self._restore_untouched(touched)
                bad = bool(self.flag.item())   # (a host wait: the scratch buffers this pass registered may go after it)
            if bad:
                raise RuntimeError("BatchNorm recalibration produced a non-finite statistic (%s source, %d rounds): the old statistics are back"
                                   % (source, rounds))
            done = True
        finally:
            for bn, p0, m0 in zip(bns, pending0, momentum0):
                bn._pending, bn.momentum = p0, m0
            model.noise = old_noise
            model.train(was_training)
            model.kl_balance = balance
            if not done:
                K.multi_copy(self._restore)
                self.acc.zero_()
                self.count.zero_()
                torch.cuda.current_stream(dev).synchronize()
        return info


def recalibrator(model):
    """The model's BnRecalibrator (made on first use; not a parameter, buffer or submodule)."""
    r = model.__dict__.get('_bn_recalibrator')
    if r is None:
        r = model.__dict__['_bn_recalibrator'] = BnRecalibrator(model)
    return r


def recalibrate_bn(model, batches=None, *, n_prior=0, prior_batch=None, temperature=None, noise=None, use_graph=None, step=0):
    """Re-estimate every BatchNorm's running statistics for the weights the model holds now -> {'rounds', 'source', 'n_bn'}.

    Two sources, exactly one of them:
      * batches: an iterable of NCHW image batches (host or device). One round is a full train-mode `model(x)` followed by a fold;
      * n_prior rounds of prior_batch rows: one round is a train-mode top-down pass from the prior at `temperature` (the path of
        `sample_prior`, which obeys the module's mode) followed by a fold. The BatchNorms that pass does not run (bottom-up, first block,
        the merge layers) keep their statistics bit for bit.
    The statistics end as the equal-weight mean over the rounds of each BatchNorm's batch mean and unbiased batch variance (update_bn's
    momentum=None rule). Runs under torch.no_grad() in train mode, dropout as in training. The noise is `noise`, or a fresh PhiloxNoise
    from the model's seed and `step` (`recal_noise`): model.noise and model.test_noise are never drawn from.

    use_graph=None: with on-device noise, batches of one shape and 8 rounds or more, two rounds run eagerly, one is captured and replayed
    for the rest (passes.replay_loop; the next batch is copied into the static input between replays). Eager and replayed agree bit for bit.

    On return, and when the body raises: the training flag, model.noise, every BatchNorm's momentum and `_pending` (so num_batches_tracked)
    are what they were. The statistics the call found stay in a shadow: `restore_bn(model)` puts them back. When a statistic comes out
    non-finite the shadow is restored and RuntimeError is raised."""
    return recalibrator(model).run(batches, n_prior=n_prior, prior_batch=prior_batch, temperature=temperature, noise=noise,
                                   use_graph=use_graph, step=step)


def restore_bn(model):
    """The running statistics as the last `recalibrate_bn(model, ...)` found them (one launch)."""
    recalibrator(model).restore()


@contextlib.contextmanager
def recalibrated(model, batches=None, **kw):
    """Inside: the model with recalibrated statistics (`recalibrate_bn(model, batches, **kw)`, whose dict is yielded); on exit the
    statistics it found are back, also when the body raises."""
    info = recalibrate_bn(model, batches, **kw)
    try:
        yield info
    finally:
        restore_bn(model)
