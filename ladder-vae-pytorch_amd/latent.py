"""Latent usage of a test pass: how many units of every stochastic layer the model actually uses.

A unit is one (channel, y, x) position of a layer's latent, U_i = Z_i * h_i * w_i of them. Over the images of a test pass (one ancestral
sample each) two measures are kept per unit: the mean analytical KL(q || p) (the Ladder VAE paper's measure) and the variance of the
posterior mean mu_q (the "active units" of the IWAE paper). A unit is KL-active when its mean KL exceeds `kl_threshold`, mean-active when
the variance of mu_q exceeds `var_threshold`.

The sums live in one flat float64 buffer on the device, as evaluate.test_pass keeps its totals and summary.TrainSummary its window:

    [ n_images | layer 0: sum mu_q [U_0], sum mu_q^2 [U_0], sum KL [U_0] | layer 1: ... | ... ]      (units in NHWC order: (y * w + x) * Z + c)

The stochastic block of layer i folds a batch into `slot(i)` (kernels.latent_stats_fold: two launches, captured with the sample when the
pass replays graphs), `count(n)` adds the batch's images to slot 0, and `take()` costs one all-reduce of the buffer, one finalize launch
per layer and one device-to-host copy of the results. The sums are additive, so ranks that fold shards of a test set get, after the
all-reduce, what one rank gets on the whole set, up to double rounding.
"""
import numpy as np
import torch

from . import kernels as K


def layer_shapes(model):
    """[(Z_i, h_i, w_i)] of the model's stochastic layers at its own (padded) image size, bottom layer first. Needs no device."""
    h, w = model.get_padded_size(model.img_shape)
    f = 1 if model.no_initial_downscaling else 2
    shapes = []
    for z, d in zip(model.z_dims, model.downsample):
        f *= 2 ** int(d)
        shapes.append((int(z), h // f, w // f))
    return shapes


def layout(shapes):
    """(offsets, total) of the flat accumulator for layers of the given (Z, h, w): slot 0 is the image count, layer i owns
    [offsets[i], offsets[i] + 3 * U_i)."""
    offsets, at = [], 1
    for z, h, w in shapes:
        offsets.append(at)
        at += 3 * z * h * w
    return offsets, at


class LatentStats:
    """Owns the device accumulator of one model's latent statistics and the buffer its results are taken into."""

    def __init__(self, model, device, kl_threshold=0.01, var_threshold=0.01):
        self.shapes = layer_shapes(model)
        self.offsets, total = layout(self.shapes)
        self.kl_threshold, self.var_threshold = float(kl_threshold), float(var_threshold)
        self.buf = torch.zeros(total, dtype=torch.float64, device=device)
        self.out = torch.empty(total - 1 + 4 * len(self.shapes), dtype=torch.float64, device=device)   # per layer: [3][U] then 4 numbers
        self.n_local = 0      # this rank's image count, as the host knows it (the buffer's slot 0 is what the all-reduce carries)

    def units(self, i):
        z, h, w = self.shapes[i]
        return z * h * w

    def reset(self):
        self.buf.zero_()
        self.n_local = 0

    def slot(self, i):
        """The (3, U_i) view layer i's stochastic block folds into."""
        return self.buf[self.offsets[i]:self.offsets[i] + 3 * self.units(i)].view(3, self.units(i))

    def count(self, n):
        """Adds the image count of a batch whose first sample was folded."""
        self.buf[:1] += int(n)
        self.n_local += int(n)

    def merge(self, other):
        """Adds another object's sums and image count (a shard folded separately on this device): what the all-reduce of take() does
        between ranks."""
        self.buf += other.buf
        self.n_local += other.n_local

    def take(self, process_group=None):
        """The statistics of everything folded since the last take(), over all ranks; the accumulator starts again. A collective: every
        rank calls it. -> {'latent/units_layer_<i>', 'latent/active_kl_layer_<i>', 'latent/active_var_layer_<i>', 'latent/active_kl',
        'latent/active_var' (ints), 'n_images', 'arrays': per layer {'kl', 'mu_mean', 'mu_var'} as float64 (Z, h, w) numpy arrays}."""
        from .evaluate import reduce_eval_sums
        dist = torch.distributed
        many = dist.is_available() and dist.is_initialized() and dist.get_world_size(process_group) > 1
        reduce_eval_sums(self.buf, process_group)
        # the finalize launch takes the image count as a number: one rank knows it; several ranks read the summed slot 0 (8 bytes)
        n = int(self.buf[0].item()) if many else self.n_local
        if n <= 0:
            raise ValueError("LatentStats.take(): no image was folded since the last take()")
        at = 0
        for i in range(len(self.shapes)):
            U = self.units(i)
            K.latent_stats_finalize(self.slot(i), n, self.kl_threshold, self.var_threshold, self.out[at:at + 3 * U],
                                    self.out[at + 3 * U:at + 3 * U + 4])
            at += 3 * U + 4
        host = self.out.cpu().numpy()
        self.reset()
        res, arrays, at = {}, [], 0
        tot_kl = tot_var = 0
        for i, (z, h, w) in enumerate(self.shapes):
            U = z * h * w
            unit = host[at:at + 3 * U].reshape(3, h, w, z).transpose(0, 3, 1, 2)
            n_kl, n_var, n_units, _ = host[at + 3 * U:at + 3 * U + 4]
            at += 3 * U + 4
            res['latent/units_layer_%d' % i] = int(n_units)
            res['latent/active_kl_layer_%d' % i] = int(n_kl)
            res['latent/active_var_layer_%d' % i] = int(n_var)
            tot_kl += int(n_kl)
            tot_var += int(n_var)
            arrays.append({'kl': np.ascontiguousarray(unit[0]), 'mu_mean': np.ascontiguousarray(unit[1]),
                           'mu_var': np.ascontiguousarray(unit[2])})
        res['latent/active_kl'], res['latent/active_var'] = tot_kl, tot_var
        res['n_images'] = n
        res['arrays'] = arrays
        return res


def latent_line_suffix(res, kl_threshold, var_threshold):
    """What --latent-stats appends to a test line: per layer active / all units (bottom layer first, top layer last) and the totals, for
    both measures. `res` holds the 'latent/*' integers of LatentStats.take()."""
    L = sum(1 for k in res if k.startswith('latent/units_layer_'))
    total = sum(res['latent/units_layer_%d' % i] for i in range(L))

    def part(name, key, thr):
        per = ' '.join('%d/%d' % (res['latent/active_%s_layer_%d' % (key, i)], res['latent/units_layer_%d' % i]) for i in range(L))
        return '{}>{:g}: {}  [{}/{}]'.format(name, thr, per, res['latent/active_' + key], total)

    return '   active units ' + part('KL', 'kl', kl_threshold) + '   ' + part('var', 'var', var_threshold)


def save_npz(path, arrays, kl_threshold, var_threshold, n_images):
    """latent_stats.npz of the evaluation CLI: kl_layer_<i>, mu_mean_layer_<i>, mu_var_layer_<i> (float64 (Z, h, w)), the two thresholds
    and the image count."""
    out = {'kl_threshold': np.float64(kl_threshold), 'var_threshold': np.float64(var_threshold), 'n_images': np.int64(n_images)}
    for i, a in enumerate(arrays):
        out['kl_layer_%d' % i], out['mu_mean_layer_%d' % i], out['mu_var_layer_%d' % i] = a['kl'], a['mu_mean'], a['mu_var']
    np.savez(path, **out)
