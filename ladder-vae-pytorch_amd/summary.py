"""Training-log summaries: the mean of every step's metrics since the previous train line, over all ranks.

The reference's `train_log_str` receives `summaries`: boilr's trainer adds every step's metrics to a summarizer, prints their mean at a
log step and starts again. Here the sums live in a small float64 accumulator on the device (as evaluate.test_pass keeps its totals):
a launch inside the step folds the step's fp32 scalars into it (kernels.summary_fold, captured with the step), and a log line costs one
take launch, one all-reduce over the ranks and one device-to-host copy. The host never synchronises between two lines.

Accumulator layout (lvae_summary_fold_f64): [steps folded, non-finite steps, loss, elbo, recons, kl, l2, grad, kl_layer_0 ... kl_layer_{L-1}].
"""
import json
import math

import torch

from . import kernels as K

N_FIXED = K.SUMMARY_FIXED
SUM_KEYS = ('loss/loss', 'elbo/elbo', 'elbo/recons', 'elbo/kl', 'l2/l2', 'l2/grad')   # slots 2..7


def means(vector, L, with_grad):
    """The summed accumulator (8 + L numbers, one rank's or the sum over ranks) -> the dict a train line prints: the keys of
    `LVAEExperiment.get_metrics_dict` in its order, 'l2/grad' when gradient norms were folded, 'steps' (finite steps averaged, over all
    ranks) and 'nonfinite_steps'. Every mean is sum / steps; with steps == 0 every mean is NaN (the caller says so)."""
    v = [float(x) for x in vector]
    if len(v) != N_FIXED + L:
        raise ValueError("a summary vector of %d layers has %d entries, got %d" % (L, N_FIXED + L, len(v)))
    steps = v[0]

    def mean(s):
        return s / steps if steps > 0 else math.nan

    d = {k: mean(s) for k, s in zip(SUM_KEYS[:5], v[2:7])}
    for i in range(L):
        d['kl_layers/kl_layer_{}'.format(i)] = mean(v[N_FIXED + i])
    if with_grad:
        d['l2/grad'] = mean(v[7])
    d['steps'] = int(steps)
    d['nonfinite_steps'] = int(v[1])
    return d


def reduce_sums(vector, process_group=None):
    """Per-rank accumulator -> the sum over all ranks, in place (one all-reduce, the evaluate.reduce_eval_sums pattern; a CPU tensor goes
    over gloo). -> (vector, ranks summed)."""
    dist = torch.distributed
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(process_group) > 1:
        dist.all_reduce(vector, group=process_group)
        return vector, dist.get_world_size(process_group)
    return vector, 1


class TrainSummary:
    """Owns the device accumulator of one training run's log window and a buffer to take it into."""

    def __init__(self, n_layers, device):
        self.L = int(n_layers)
        if not 0 <= self.L <= K.SUMMARY_MAX_LAYERS:
            raise ValueError("a summary holds the KL of at most %d layers, got %d" % (K.SUMMARY_MAX_LAYERS, self.L))
        self.acc = torch.zeros(N_FIXED + self.L, dtype=torch.float64, device=device)
        self.taken = torch.zeros_like(self.acc)
        self.with_grad = False
        self.ranks = 1      # ranks summed by the last take()

    def fold(self, out, grad_norm=None, gscale=None):
        """One step's scalars (the dict TrainStep._fwd_bwd returns: device tensors) into the window. One launch, nothing else."""
        if grad_norm is not None:
            self.with_grad = True
        K.summary_fold(out['loss'], out['elbo'], out['recons'], out['kl'], out['l2'], out['kl_avg_layerwise'], self.acc,
                       grad_norm=grad_norm, gscale=gscale)

    def take_vector(self, process_group=None):
        """The window's sums over all ranks as a CPU float64 vector; the window starts again. A collective: every rank calls it."""
        K.summary_take(self.acc, self.taken)
        vec, self.ranks = reduce_sums(self.taken, process_group)
        return vec.cpu()

    def take(self, process_group=None):
        vec = self.take_vector(process_group)
        return means(vec.tolist(), self.L, self.with_grad or vec[7].item() != 0.0)

    def state(self):
        """The accumulator as a list of Python floats (for checkpoints; float64 survives the round trip exactly)."""
        return self.acc.cpu().tolist()

    def load_state(self, vector):
        """Restores `state()`: a run resumed in the middle of a window prints the train line of the uninterrupted run."""
        v = torch.tensor([float(x) for x in vector], dtype=torch.float64)
        if v.numel() != self.acc.numel():
            raise ValueError("the stored summary has %d entries, this model's %d" % (v.numel(), self.acc.numel()))
        self.acc.copy_(v)
        self.with_grad = self.with_grad or float(v[7]) != 0.0


def train_line_suffix(m, ranks):
    """What --window-summaries appends to a train line built from `means`' dict."""
    s = ''
    if 'l2/grad' in m:
        s += '   grad: {:.3g}'.format(m['l2/grad'])
    if m['nonfinite_steps'] > 0:
        s += '   [{} non-finite steps]'.format(m['nonfinite_steps'])
    if m['steps'] == 0:
        return s + '   [no finite step to average]'
    per_rank = m['steps'] / ranks
    return s + '   [averaged over {:g} steps × {} ranks]'.format(per_rank, ranks)


class History:
    """--history FILE: one JSON object per printed log line, appended and flushed line by line."""

    def __init__(self, path):
        self.f = open(path, 'a')

    def write(self, step, split, metrics, epoch=None, **extra):
        rec = {'step': int(step), 'split': split}
        if epoch is not None:
            rec['epoch'] = int(epoch)
        # ('latent_arrays' of a test pass with --latent-stats: whole arrays, not a line's numbers; the 'latent/*' counts stay)
        rec['metrics'] = {k: v for k, v in metrics.items() if k not in extra and k != 'latent_arrays'}
        rec.update(extra)
        self.f.write(json.dumps(rec) + '\n')
        self.f.flush()

    def close(self):
        self.f.close()
