"""LadderVAE on the MI355X HIP engine — drop-in for the reference's models/lvae.py:15-372.

Same constructor keyword arguments and defaults, the same 12-key forward() dict (shapes in the reference's NCHW
convention: tensors are returned as permuted views of the engine's NHWC buffers, no copy), the same helper methods
(`bottomup_pass`, `topdown_pass`, `sample_prior`, `pad_input`, `get_padded_size`, `get_top_prior_param_shape`),
attributes (`n_layers`, `img_shape`, `likelihood`, `global_step`), exceptions, and state_dict key scheme.

Differences by design (not by omission):
  * `logp` (data['logprob_p'] of topdown_pass) is computed by one kernel from the per-layer rows and carries no autograd graph
    (the reference never differentiates it: it is a logged metric, experiment/experiment_manager.py does not read it);
  * every arithmetic op is a hand-written gfx950 kernel from liblvae_hip.so; the model refuses to run on CPU;
  * parameters live in one flat arena (arena.py); their gradients are accumulated in place by the wgrad kernels;
  * noise comes from `self.noise` (noise.PhiloxNoise on device; noise.TapeNoise to replay the reference's draws);
  * engine-only methods beside the reference's: `sample_conditional`, `encode`, `decode`, `interpolate`, `inpaint` (forward only), and
    the `mask` keyword of forward(): the ELBO of the observed pixels of a partly observed image.

Every pass, the reference's and the engine's own, is built from four private pieces: `_encode_image` (image -> pad -> NHWC -> bottom-up),
`_walk` (THE top-down loop: one call site of TopDownLayer, driven by a per-layer list of `LayerZ` that says where each z comes from, with
the one seam where rows are repeated for K samples, then `_final_top_down`), `_pictures` (crop -> likelihood without a target -> NCHW
dict) and, for the loops that run a round many times, passes.replay_loop. The public methods check arguments and build the list.

The boilr helpers the reference imports (pad/crop, Interpolate, free_bits_kl) are restated — parity unpinned
(SURVEY.md §8c).
"""
import numbers
from collections import namedtuple

import numpy as np
import torch
from torch import nn

from .. import kernels as K
from .. import ops
from ..arena import ParamArena
from ..lib.likelihoods import (BernoulliLikelihood, DiscretizedLogisticLikelihood, DiscretizedLogisticMixLikelihood,
                               GaussianLikelihood)
from ..lib.nn import BatchNorm2dParams, Conv2dParams, Placeholder, act_name
from ..noise import PhiloxNoise
from ..passes import eval_mode, replay_loop
from .lvae_layers import BottomUpDeterministicResBlock, BottomUpLayer, TopDownDeterministicResBlock, TopDownLayer


def _nchw(t):
    """NHWC engine tensor -> logical NCHW view (no copy)."""
    return None if t is None else t.permute(0, 3, 1, 2)


def _nchw_params(params):
    """The `params` entry of a likelihood's info (a tensor, or a dict of them) as NCHW views."""
    return {k: _nchw(v) for k, v in params.items()} if isinstance(params, dict) else _nchw(params)


# Where one layer's z comes from, for LadderVAE._walk. posterior: inference mode (needs the layer's bottom-up value), else generative mode.
# use_mode: the mean instead of a draw. constant: force_constant_output. temperature: of a prior draw (None: the plain draw; not with
# use_mode or forced). forced: an NHWC z to take instead (forced_latent). last: the walk stops behind this layer: the layers below launch
# nothing (their entries are not read) and the tail is not run.
LayerZ = namedtuple('LayerZ', 'posterior use_mode constant temperature forced last', defaults=(False, False, False, None, None, False))


def layer_temperatures(L, value):
    """The `temperature` argument of sample_prior / sample_conditional as a list of L entries indexed like z_dims (layer 0 is the bottom):
    None -> L times None; a number -> L copies; a sequence of L numbers -> kept, as floats; a tensor (per-row temperatures, checked where
    they are used) -> the same tensor at every layer. ValueError for a wrong length and for a negative or non-finite number; the values of
    a tensor live on the device and are NOT validated, here or later: they are the caller's responsibility."""
    if value is None or torch.is_tensor(value):
        return [value] * L
    values = [value] * L if isinstance(value, numbers.Real) else list(value)
    if len(values) != L:
        raise ValueError("temperature has %d values for %d layers: give one, or one per layer" % (len(values), L))
    values = [float(v) for v in values]
    for v in values:
        if not 0.0 <= v < float('inf'):   # (NaN fails both comparisons)
            raise ValueError("a temperature must be a finite number >= 0, got %r" % (v,))
    return values


def _untempered(temps):
    return all(t is None or (not torch.is_tensor(t) and t == 1.0) for t in temps)


class _SharedDraws:
    """Round a noise source, for the decoding half of LadderVAE.interpolate: a `normal` draw of T * B rows (a prior layer's eps) is ONE draw
    of B rows from the source, repeated for the T steps (K.repeat_samples: step-major, no launch for one step). Every other draw passes
    through."""

    def __init__(self, src, B, T):
        self.src, self.B, self.T = src, int(B), int(T)

    def normal(self, shape_nhwc, device):
        assert shape_nhwc[0] == self.T * self.B, (tuple(shape_nhwc), self.T, self.B)
        eps = self.src.normal((self.B,) + tuple(shape_nhwc[1:]), device)
        return eps if self.T == 1 else K.repeat_samples(eps, self.T)

    def dropout_mask(self, N, C, p, device):
        return self.src.dropout_mask(N, C, p, device)

    def uniform(self, shape, lo, hi, device, channel_last=True):
        return self.src.uniform(shape, lo, hi, device, channel_last)


class LadderVAE(nn.Module):

    def __init__(self, color_ch, z_dims, blocks_per_layer=2, downsample=None, nonlin='elu', merge_type=None,
                 batchnorm=True, stochastic_skip=False, n_filters=32, dropout=None, free_bits=0.0,
                 learn_top_prior=False, img_shape=None, likelihood_form=None, res_block_type=None, gated=False,
                 no_initial_downscaling=False, analytical_kl=False):
        super().__init__()
        self.global_step = 0  # boilr.models.BaseGenerativeModel attribute, read by forward_pass for beta annealing
        self.color_ch = color_ch
        self.z_dims = z_dims
        self.blocks_per_layer = blocks_per_layer
        self.downsample = downsample
        self.n_layers = len(self.z_dims)
        self.stochastic_skip = stochastic_skip
        self.n_filters = n_filters
        self.dropout = dropout
        self.free_bits = free_bits
        self.learn_top_prior = learn_top_prior
        self.img_shape = tuple(img_shape)
        self.res_block_type = res_block_type
        self.gated = gated
        self.no_initial_downscaling = no_initial_downscaling
        if self.downsample is None:
            self.downsample = [0] * self.n_layers
        self.overall_downscale_factor = int(np.power(2, sum(self.downsample)))
        if not no_initial_downscaling:
            self.overall_downscale_factor *= 2
        assert max(self.downsample) <= self.blocks_per_layer
        assert len(self.downsample) == self.n_layers
        if nonlin not in ('relu', 'leakyrelu', 'elu', 'selu'):
            raise KeyError(nonlin)
        self.act = act_name(nonlin)

        stride = 1 if no_initial_downscaling else 2
        self.first_bottom_up = nn.ModuleList([
            Conv2dParams(color_ch, n_filters, 5, stride=stride, padding=2),
            Placeholder(self.act),
            BottomUpDeterministicResBlock(c_in=n_filters, c_out=n_filters, nonlin=nonlin, batchnorm=batchnorm,
                                          dropout=dropout, res_block_type=res_block_type),
        ])
        self.top_down_layers = nn.ModuleList([])
        self.bottom_up_layers = nn.ModuleList([])
        for i in range(self.n_layers):
            is_top = i == self.n_layers - 1
            self.bottom_up_layers.append(
                BottomUpLayer(n_res_blocks=self.blocks_per_layer, n_filters=n_filters,
                              downsampling_steps=self.downsample[i], nonlin=nonlin, batchnorm=batchnorm, dropout=dropout,
                              res_block_type=res_block_type, gated=gated))
            self.top_down_layers.append(
                TopDownLayer(z_dim=z_dims[i], n_res_blocks=blocks_per_layer, n_filters=n_filters, is_top_layer=is_top,
                             downsampling_steps=self.downsample[i], nonlin=nonlin, merge_type=merge_type,
                             batchnorm=batchnorm, dropout=dropout, stochastic_skip=stochastic_skip,
                             learn_top_prior=learn_top_prior, top_prior_param_shape=self.get_top_prior_param_shape(),
                             res_block_type=res_block_type, gated=gated, analytical_kl=analytical_kl))
        modules = []
        if not no_initial_downscaling:
            modules.append(Placeholder('bilinear x2'))
        for i in range(blocks_per_layer):
            modules.append(TopDownDeterministicResBlock(c_in=n_filters, c_out=n_filters, nonlin=nonlin,
                                                        batchnorm=batchnorm, dropout=dropout,
                                                        res_block_type=res_block_type, gated=gated))
        self.final_top_down = nn.ModuleList(modules)

        if likelihood_form == 'bernoulli':
            self.likelihood = BernoulliLikelihood(n_filters, color_ch)
        elif likelihood_form == 'gaussian':
            self.likelihood = GaussianLikelihood(n_filters, color_ch)
        elif likelihood_form == 'discr_log':
            self.likelihood = DiscretizedLogisticLikelihood(n_filters, color_ch, 256)
        elif likelihood_form == 'discr_log_mix':
            self.likelihood = DiscretizedLogisticMixLikelihood(n_filters)
        else:
            raise RuntimeError("Unrecognized likelihood '{}'".format(likelihood_form))

        self.noise = PhiloxNoise(seed=0)
        self.arena = None
        # engine attribute (not a constructor argument of the reference): 'f32', or 'bf16' = bf16 matrix-core operands with fp32
        # accumulation, statistics, KL and likelihood (the arithmetic of the reference under torch.autocast(bfloat16)) for the
        # convolutions that have a bf16 kernel (lvae_conv2d_bf16); activations, parameters and gradients stay fp32 in HBM
        self.compute_dtype = 'f32'
        # engine attribute, set after construction like compute_dtype: a balance.KlBalance (attached to this model and bound to a beta
        # source) makes a TRAINING forward balance the per-layer terms of `kl_loss` while beta < 1 (NVAE's KL balancing); `kl_sep`,
        # `kl_avg_layerwise` and `kl` stay the plain numbers. None, or eval mode: the plain bookkeeping, launch for launch. No parameter,
        # no buffer: the state_dict does not know about it
        self.kl_balance = None
        self.grad_tracker = None  # dist.GradAllReduce when gradients are exchanged while backward runs (engine.TrainStep sets it)

    @property
    def residual_posterior(self):
        """Engine attribute (not a constructor argument of the reference), set after construction like compute_dtype: every layer's
        conv_in_q predicts its posterior as an offset from the prior of the same layer, mu_q = mu_p + dmu, logvar_q = logvar_p + dlv
        (NVAE's residual normal; the top layer's prior is the broadcast top_prior_params). No parameter is added or renamed: the same
        state_dict means a different model under the other setting, which is why checkpoints note it."""
        return all(layer.stochastic.residual_posterior for layer in self.top_down_layers)

    @residual_posterior.setter
    def residual_posterior(self, value):
        for layer in self.top_down_layers:
            layer.stochastic.residual_posterior = bool(value)

    # ------------------------------------------------------------------------------------------------------------
    # engine plumbing
    # ------------------------------------------------------------------------------------------------------------
    def _apply(self, fn, *a, **kw):
        self.arena = None  # .to()/.cuda() re-create the parameter storages; re-pack lazily
        return super()._apply(fn, *a, **kw)

    def pack(self, device=None):
        """Move all parameters into the flat arena (idempotent). Called lazily by the first forward."""
        if device is None:
            device = next(self.parameters()).device
        device = torch.device(device)
        if device.type != 'cuda':
            raise K._C.LvaeHipError("LadderVAE (HIP engine) runs on an MI355X only: move the model with .cuda() first; "
                                    "there is no CPU fallback (the CPU restatement lives in oracle/ for tests)")
        first = next(self.parameters())
        if self.arena is None or not self.arena.owns(first) or first.device != device:
            if first.device != device:
                super()._apply(lambda t: t.to(device))
            self.arena = ParamArena(self, device, segment_of=self.grad_segment_of)
        return self.arena

    def grad_segments(self):
        """Parameter-name prefixes in the order their gradients complete during backward = reverse execution order of forward
        (forward: stem, bottom_up_layers[0..L-1], top_down_layers[L-1..0], final_top_down, likelihood — models/lvae.py:172-315).
        The last segment (stem + first block) also takes `top_prior_params`, whose gradient arrives through autograd's own
        accumulation node rather than from one of our backward launches."""
        L = self.n_layers
        return (['likelihood.', 'final_top_down.'] + ['top_down_layers.%d.' % i for i in range(L)] +
                ['bottom_up_layers.%d.' % i for i in reversed(range(L))] + ['first_bottom_up.'])

    def grad_segment_of(self, name):
        segs = self.grad_segments()
        if name.endswith('top_prior_params'):
            return len(segs) - 1
        for i, pre in enumerate(segs):
            if name.startswith(pre):
                return i
        raise KeyError(name)

    def _mark(self, x, prefix):
        """Backward of this identity node runs once every backward launch of segment `prefix` has been issued (x is the segment's
        input, and every node of the segment is an ancestor of x's gradient); it tells the gradient exchange so."""
        if self.grad_tracker is None or not torch.is_grad_enabled() or not x.requires_grad:
            return x
        return ops.segment_mark(x, self.grad_tracker, self.grad_segments().index(prefix))

    def zero_grad(self, set_to_none=False):
        if self.arena is not None:
            self.arena.zero_grad()
        else:
            super().zero_grad(set_to_none=set_to_none)

    def bn_modules(self):
        return [m for m in self.modules() if isinstance(m, BatchNorm2dParams)]

    def _mask_plan(self, N, n_samples=1):
        """(number of Dropout2d draws of one training forward, N, C, p) when they all share one shape, else None. With n_samples = K > 1 the
        draws have two shapes and the plan is a list of two such groups in draw order: the bottom-up masks at N images, then the top-down
        ones at K * N rows."""
        if not self.training or not self.dropout:
            return None
        if getattr(self, '_n_drop', None) is None:
            from ..lib.nn import ResidualBlock
            drops = lambda root: sum(sum(m._drops) for m in root.modules() if isinstance(m, ResidualBlock))
            self._n_drop = drops(self)
            self._n_drop_bu = drops(self.first_bottom_up) + drops(self.bottom_up_layers)
        if n_samples == 1:
            return (self._n_drop, N, self.n_filters, float(self.dropout))
        return [(self._n_drop_bu, N, self.n_filters, float(self.dropout)),
                (self._n_drop - self._n_drop_bu, n_samples * N, self.n_filters, float(self.dropout))]

    def _begin(self, ref_tensor, batch=None, n_samples=1):
        self.pack(ref_tensor.device if ref_tensor is not None else None)
        K.set_precision(self.compute_dtype)
        self.noise.begin(next(self.parameters()).device, self._mask_plan(batch, n_samples) if batch else None)

    # ------------------------------------------------------------------------------------------------------------
    # reference API
    # ------------------------------------------------------------------------------------------------------------
    def forward(self, x, n_samples=1, mask=None, mask_fill=0.0):
        """mask, mask_fill: engine-only keywords — the ELBO of a partly observed image. mask: bool or uint8, (B,H,W) or (B,1,H,W), on the
        device of x; non-zero = observed, one flag per pixel for all its colours. The encoder sees x where observed and mask_fill (a finite
        number, or a (B,C,H,W) tensor) where missing: one select launch in front of the pad; x itself is read nowhere else, so what it holds
        under a hidden pixel changes no output bit. `ll`, and through it the loss and every gradient, counts the observed pixels only (the
        masked likelihood kernels: the gradient at a missing pixel's parameters is exactly zero). The dict gains a 13th key, `out_filled`
        (NCHW): x where observed, the likelihood's sample where missing. ValueError for a mask of the wrong shape, dtype or device, a
        non-finite mask_fill, and n_samples > 1 with a mask. mask=None issues exactly the launches of a call without the keyword.

        n_samples: engine-only keyword — K > 1 draws K importance samples per image (engine.forward_pass(iw_samples=K) trains on their
        bound). The bottom-up pass is a deterministic function of the image and runs ONCE, on the B images; each level's output is repeated
        for the K samples (ops.RepeatSamplesFn, whose backward sums their gradients) and the top-down pass, final_top_down, the crop and the
        likelihood run on K * B rows, sample-major (row k * B + b). The dict keeps its 12 keys: `ll`, `kl_sep`, `z`, `kl_spatial` and `out_*`
        have K * B rows; `kl`, `kl_avg_layerwise` and `logp` are means over all rows. Two consequences: BatchNorm normalises over the B images
        going bottom-up and over the K * B rows going top-down, and the bottom-up Dropout2d masks are shared by the K samples of an image
        (the top-down ones are drawn per row). n_samples = 1 draws, launches and returns exactly what a call without the keyword does."""
        if not x.is_cuda:
            raise K._C.LvaeHipError("LadderVAE (HIP engine) needs a GPU tensor; got %s" % x.device)
        n_samples = int(n_samples)
        if n_samples < 1:
            raise ValueError("n_samples must be at least 1, got %d" % n_samples)
        if mask is not None:
            if n_samples > 1:
                raise ValueError("a mask together with n_samples > 1 is not supported")
            if x.dim() != 4:
                raise ValueError("x must be (B, C, H, W), got %s" % (tuple(x.shape),))
            mask = K.pixel_mask(mask, x.shape[0], x.shape[2], x.shape[3], x.device)
            mask_fill = self._mask_fill(mask_fill, x, 'mask_fill')
        self._begin(x, batch=x.shape[0], n_samples=n_samples)
        if mask is not None:
            x = K.mask_select(x.contiguous().float(), mask_fill, mask, True)   # from here on the truth under a hidden pixel is gone
        bu_values, x_nhwc, img_size = self._encode_image(x)
        if n_samples > 1:
            # behind the fan-out of _bottomup, in front of the segment marks of _walk: the gradient fan-in stays as it is
            bu_values = [ops.RepeatSamplesFn.apply(b, n_samples) for b in bu_values]
            x_nhwc = K.repeat_samples(x_nhwc, n_samples)
        out, td_data = self._topdown(bu_values)
        out = self._mark(self._crop(out, img_size), 'likelihood.')
        if mask is None:
            ll, likelihood_info = self.likelihood(out, x_nhwc, self.noise)
        else:
            ll, likelihood_info = self.likelihood(out, x_nhwc, self.noise, mask=mask)

        kl_ln = ops.StackFn.apply(*td_data['kl'])  # (L, N)
        if self.kl_balance is not None and self.training:
            # the same bookkeeping with the terms of kl_loss balanced over the layers while beta < 1; the other three keep their bits
            kl_sep, kl_avg_layerwise, kl_loss, kl, coeff = ops.KlBalanceFn.apply(kl_ln, float(self.free_bits), self.kl_balance)
            self.kl_balance.coeff = coeff.detach()
        else:
            kl_sep, kl_avg_layerwise, kl_loss, kl = ops.KLBookFn.apply(kl_ln, float(self.free_bits))
        self.noise.end()

        res = {
            'll': ll,
            'z': [_nchw(z) for z in td_data['z']],
            'kl': kl,
            'kl_sep': kl_sep,
            'kl_avg_layerwise': kl_avg_layerwise,
            'kl_spatial': td_data['kl_spatial'],
            'kl_loss': kl_loss,
            'logp': td_data['logprob_p'],
            'out_mean': _nchw(likelihood_info['mean']),
            'out_mode': _nchw(likelihood_info['mode']),
            'out_sample': _nchw(likelihood_info['sample']),
            'likelihood_params': _nchw_params(likelihood_info['params']),
        }
        if mask is not None:
            res['out_filled'] = _nchw(likelihood_info['filled'])
        return res

    @staticmethod
    def _mask_fill(fill, x, what):
        """A fill for the missing pixels of the NCHW batch x: a finite number (returned as a float) or a tensor of x's shape on its device
        (returned contiguous float32). ValueError otherwise."""
        if torch.is_tensor(fill) and fill.dim() > 0:
            if tuple(fill.shape) != tuple(x.shape) or fill.device != x.device:
                raise ValueError("%s must be a number or a %s tensor on %s, got %s on %s" % (what, tuple(x.shape), x.device, tuple(fill.shape), fill.device))
            return fill.contiguous().float()
        try:
            fill = float(fill)
        except (TypeError, ValueError):
            raise ValueError("%s must be a number or a %s tensor, got %r" % (what, tuple(x.shape), fill))
        if not np.isfinite(fill):
            raise ValueError("%s must be finite, got %r" % (what, fill))
        return fill

    def _bottomup(self, x):
        stem, _, block = self.first_bottom_up
        x = stem(x, out_act=self.act)
        x = block(x, self.noise)
        bu_values = []
        for i in range(self.n_layers):
            x = self.bottom_up_layers[i](self._mark(x, 'bottom_up_layers.%d.' % i), self.noise)
            if i + 1 < self.n_layers:
                x, x_td = ops.fanout(x, 2)   # consumers: the next bottom-up layer and this level's top-down layer
            else:
                x_td = x
            bu_values.append(x_td)
        return bu_values

    def _encode_image(self, x, nchw=True, need_image=True):
        """The image prelude of every pass that looks at pictures: x (NCHW; with nchw=False an NHWC engine tensor) contiguous float32 ->
        centred zero pad to the padded size, as NHWC, one kernel (models/lvae.py:176, 317-325) -> bottom-up pass. Returns (bu_values,
        x_nhwc, img_size): x_nhwc is the unpadded NHWC image the likelihood compares with (the padded tensor itself when nothing was
        padded, else one more copy launch; None with need_image=False, which issues no launch for it), img_size = (H, W). Between
        _begin and noise.end()."""
        x = x.contiguous().float()
        img_size = tuple(int(s) for s in (x.shape[2:] if nchw else x.shape[1:3]))
        x_pad = K.pad_crop(x, nchw, self.get_padded_size(img_size), False)
        x_nhwc = None
        if need_image:
            x_nhwc = x_pad if img_size == tuple(x_pad.shape[1:3]) else K.pad_crop(x, nchw, img_size, False)
        return self._bottomup(x_pad), x_nhwc, img_size

    @staticmethod
    def _crop(out, img_size):
        """NHWC centre crop to img_size; no launch when it has that size already."""
        img_size = tuple(int(s) for s in img_size)
        return out if tuple(out.shape[1:3]) == img_size else ops.CropFn.apply(out, img_size)

    def bottomup_pass(self, x):
        """models/lvae.py:216-227. x: padded image (N,C,Hp,Wp); returns the list of per-level NCHW feature maps."""
        self._begin(x)
        x_pad = K.pad_crop(x.contiguous().float(), True, x.shape[2:], False)
        out = [_nchw(b) for b in self._bottomup(x_pad)]
        self.noise.end()  # the next call draws fresh dropout masks
        return out

    def _walk(self, plan, bu_values=None, rows=None, noise=None, mats=None, latent_stats=None, n_samples=1):
        """The one top-down walk, layers L-1 .. 0 and then final_top_down; every public method builds `plan` and calls it.

        plan: L LayerZ entries indexed like z_dims (layer 0 is the bottom), saying where each layer's z comes from. A posterior layer runs
        in inference mode on bu_values[i], by the code path of forward(); every other layer runs in generative mode on `rows` rows and takes
        its noise from `noise` (default self.noise). An entry with `last` is the one way to stop: the walk ends behind that layer,
        everything below it launches nothing, the tail is not run and `out` is None (encode(): with all L layers, layer 0 is the last).
        mats: an optional (lp_mat, kl_mat) pair of [L][rows] matrices; the stochastic kernel of layer i writes its per-sample log p(z)
        and KL straight into rows i, and `logprob_p` is their sum of row means (models/lvae.py:301; a metric, without a graph). Without
        it the kernel wrapper allocates and `logprob_p` is None: the walk invents no matrices for a caller that has none.
        latent_stats: a latent.LatentStats whose slot i the stochastic block of a posterior layer i folds its (mu | logvar) tensors
        into; None issues exactly the launches of a pass without it.
        n_samples = K: the one seam where what the posterior layers hand down, on B rows, is repeated to the K * B rows of what follows,
        sample-major (K.repeat_samples): in front of the first prior layer below a posterior one, or in front of final_top_down when
        every layer is posterior. A plan without a posterior layer has no seam (the top layer broadcasts its prior over `rows` itself),
        and K = 1 launches nothing.
        Segment marks: the walk always calls _mark at every layer and in front of the tail, whoever calls it; _mark is the identity
        without a gradient tracker or without grad, so the sampling paths issue nothing for it and forward() keeps its graph node for node.

        Returns (out NHWC, {'z', 'kl', 'kl_spatial': per layer, None where the layer has none or did not run; 'logprob_p'})."""
        L = self.n_layers
        noise = self.noise if noise is None else noise
        z, kl, kl_spatial = [None] * L, [None] * L, [None] * L
        data = {'z': z, 'kl': kl, 'kl_spatial': kl_spatial, 'logprob_p': None}
        out = None
        for i in reversed(range(L)):
            src = plan[i]
            bu_value = bu_values[i] if src.posterior else None
            if n_samples > 1 and not src.posterior and i + 1 < L and plan[i + 1].posterior:
                out = K.repeat_samples(out, n_samples)
            if out is not None:
                out = self._mark(out, 'top_down_layers.%d.' % i)
            elif bu_value is not None:
                bu_value = self._mark(bu_value, 'top_down_layers.%d.' % i)
            out, _, aux = self.top_down_layers[i](out, skip_connection_input=out, inference_mode=src.posterior, bu_value=bu_value,
                                                  n_img_prior=None if src.posterior else rows, use_mode=src.use_mode,
                                                  force_constant_output=src.constant, forced_latent=src.forced, noise=noise,
                                                  rows=None if mats is None else (mats[0][i], mats[1][i]),
                                                  stats=None if latent_stats is None else latent_stats.slot(i),
                                                  temperature=src.temperature)
            z[i], kl[i], kl_spatial[i] = aux['z'], aux['kl_samplewise'], aux['kl_spatial']
            if src.last:
                return None, data
        if mats is not None:
            with torch.no_grad():
                data['logprob_p'] = K.sum_of_row_means(mats[0]).view(())
        if n_samples > 1 and plan[0].posterior:
            out = K.repeat_samples(out, n_samples)
        return self._final_top_down(self._mark(out, 'final_top_down.'), noise), data

    def _final_top_down(self, out, noise):
        for mod in self.final_top_down:
            out = ops.UpsampleFn.apply(out) if isinstance(mod, Placeholder) else mod(out, noise)
        return out

    def _topdown(self, bu_values=None, n_img_prior=None, mode_layers=None, constant_layers=None, forced_latent=None, latent_stats=None):
        """The reference's pass (models/lvae.py:229-315) as a plan for _walk: all-posterior on NHWC bu_values or all-prior on n_img_prior
        rows, forced_latent NCHW per layer or None, with the [L][N] matrices that give `logprob_p`. latent_stats: as in _walk."""
        mode_layers = [] if mode_layers is None else mode_layers
        constant_layers = [] if constant_layers is None else constant_layers
        inference_mode = bu_values is not None
        if inference_mode != (n_img_prior is None):
            raise RuntimeError("Number of images for top-down generation has to be given if and only if we're "
                               "not doing inference")
        if inference_mode and (len(mode_layers) > 0 or len(constant_layers) > 0):
            raise RuntimeError("Prior experiments (e.g. sampling from mode) are not compatible with inference mode")
        forced = [None if fl is None else fl.permute(0, 2, 3, 1).contiguous() for fl in forced_latent or [None] * self.n_layers]
        plan = [LayerZ(inference_mode, i in mode_layers, i in constant_layers, None, forced[i]) for i in range(self.n_layers)]
        n_rows = bu_values[0].shape[0] if inference_mode else int(n_img_prior)
        mats = tuple(torch.empty((self.n_layers, n_rows), dtype=torch.float32, device=next(self.parameters()).device) for _ in range(2))
        return self._walk(plan, bu_values, n_img_prior, mats=mats, latent_stats=latent_stats)

    def topdown_pass(self, bu_values=None, n_img_prior=None, mode_layers=None, constant_layers=None,
                     forced_latent=None):
        """models/lvae.py:229-315 (NCHW in / NCHW out wrapper of the engine's NHWC pass)."""
        self._begin(bu_values[0] if bu_values is not None else None)
        if bu_values is not None:
            bu_values = [b.permute(0, 2, 3, 1).contiguous() for b in bu_values]
        out, data = self._topdown(bu_values, n_img_prior, mode_layers, constant_layers, forced_latent)
        self.noise.end()  # every call returns a fresh sample, as the reference's rsample() does
        data = dict(data)
        data['z'] = [_nchw(t) for t in data['z']]
        return _nchw(out), data

    def pad_input(self, x):
        """models/lvae.py:317-325 — centred zero pad to a multiple of the overall downscale factor (NCHW in/out)."""
        size = self.get_padded_size(x.size())
        return K.pad_crop(x.contiguous().float(), True, size, True)

    def get_padded_size(self, size):
        """models/lvae.py:327-349."""
        dwnsc = self.overall_downscale_factor
        if len(size) == 4:
            size = size[2:]
        if len(size) != 2:
            raise RuntimeError("input size must be either (N, C, H, W) or (H, W), but it has length {} (size={})".format(
                len(size), size))
        return list(((s - 1) // dwnsc + 1) * dwnsc for s in size)

    def sample_prior(self, n_imgs, mode_layers=None, constant_layers=None, temperature=None):
        """models/lvae.py:351-362. temperature: engine-only keyword — z = mu_p + t * sigma_p * eps at every layer that samples: a float,
        a sequence of L floats indexed like z_dims, or a device float tensor (n_imgs,) of per-row temperatures used at every layer. A layer
        in mode_layers ignores its temperature; a layer at 0.0 draws no noise. None or 1.0 is the call without the keyword, bit for bit."""
        temps = layer_temperatures(self.n_layers, temperature)
        self._begin(None)
        if _untempered(temps):   # the reference's call, with its matrices
            out, data = self._topdown(n_img_prior=n_imgs, mode_layers=mode_layers, constant_layers=constant_layers)
        else:
            in_mode, constant = mode_layers or (), constant_layers or ()
            plan = [LayerZ(False, i in in_mode, i in constant, None if i in in_mode else t) for i, t in enumerate(temps)]
            out, data = self._walk(plan, rows=int(n_imgs))
        return self._pictures(out, self.img_shape, data['z'])['sample']

    def sample_conditional(self, x, n_top_layers, n_samples=1, temperature=None, use_mode=False):
        """Engine-only: images that share the top k = n_top_layers latents of x. The k top layers take z from the posterior of x (as
        forward() does; with use_mode its mean), the layers below are sampled from the prior K = n_samples times per image at
        `temperature` (as in sample_prior), then final_top_down, the crop and the likelihood without a target. x (B, C, H, W); k = 0 is
        K * B prior samples (no bottom-up pass: x only gives B), k = L is K likelihood draws of one reconstruction pass. Rows are
        sample-major (row k * B + b). Obeys the module's train / eval mode, like sample_prior.

        Noise, in this order: one `normal` draw per layer that samples, top to bottom, of shape (rows, h, w, Z) with rows = B for a
        posterior layer and K * B for a prior layer (none for a posterior layer under use_mode, none for a prior layer at temperature 0.0),
        then the likelihood's draws.

        Returns {'sample', 'mean', 'mode'} (NCHW, K * B rows; None where the likelihood has none), 'likelihood_params', and 'z': L NCHW
        tensors, B rows for the posterior layers and K * B rows for the prior layers."""
        if not x.is_cuda:
            raise K._C.LvaeHipError("LadderVAE (HIP engine) needs a GPU tensor; got %s" % x.device)
        L = self.n_layers
        if x.dim() != 4:
            raise ValueError("x must be (B, C, H, W), got %s" % (tuple(x.shape),))
        n_top, n_samples = int(n_top_layers), int(n_samples)
        if not 0 <= n_top <= L:
            raise ValueError("n_top_layers must be in 0..%d, got %d" % (L, n_top))
        if n_samples < 1:
            raise ValueError("n_samples must be at least 1, got %d" % n_samples)
        temps = layer_temperatures(L, temperature)
        self._begin(x)
        bu_values = self._encode_image(x, need_image=False)[0] if n_top > 0 else None
        plan = [LayerZ(True, use_mode) if i >= L - n_top else LayerZ(temperature=t) for i, t in enumerate(temps)]
        out, data = self._walk(plan, bu_values, n_samples * int(x.shape[0]), n_samples=n_samples)
        return self._pictures(out, x.shape[2:], data['z'])

    # ------------------------------------------------------------------------------------------------------------
    # engine-only: encode / decode / interpolate (forward only: run them under torch.no_grad())
    # ------------------------------------------------------------------------------------------------------------
    def _top_k(self, n_top_layers):
        k = self.n_layers if n_top_layers is None else int(n_top_layers)
        if not 1 <= k <= self.n_layers:
            raise ValueError("n_top_layers must be in 1..%d, got %d" % (self.n_layers, k))
        return k

    def _pictures(self, out, img_size, z):
        """The tail of every pass that makes pictures: crop, likelihood without a target, noise.end() -> the dict of sample_conditional"""
        _, info = self.likelihood(self._crop(out, img_size), None, self.noise)
        self.noise.end()
        return {'sample': _nchw(info['sample']), 'mean': _nchw(info['mean']), 'mode': _nchw(info['mode']),
                'likelihood_params': _nchw_params(info['params']), 'z': [_nchw(t) for t in z]}

    def _posterior_plan(self, n_top, use_mode):
        """Layers L-1 .. L-n_top from the posterior (with use_mode its mean); the walk stops behind layer L-n_top."""
        return [LayerZ(True, use_mode, last=i == self.n_layers - n_top) for i in range(self.n_layers)]

    @staticmethod
    def _forced_plan(forced, temps):
        """Generative mode: layer i takes forced[i] (NHWC) where it is given and draws from its prior at temps[i] where it is None."""
        return [LayerZ(temperature=t) if f is None else LayerZ(forced=f) for f, t in zip(forced, temps)]

    def encode(self, x, n_top_layers=None, use_mode=True):
        """Engine-only: the latents of the top k = n_top_layers layers (None: all L) of the NCHW batch x, from its posterior as forward()
        draws them; with use_mode (the default) the posterior means, drawing no noise. Returns a list of L entries indexed like z_dims: NCHW
        z for layers L-k .. L-1, None below (those layers launch nothing). k = 0 is a ValueError: there is nothing to encode. Noise (use_mode
        False only): one `normal` draw per encoded layer, top to bottom. Obeys the module's train / eval mode."""
        if not x.is_cuda:
            raise K._C.LvaeHipError("LadderVAE (HIP engine) needs a GPU tensor; got %s" % x.device)
        if x.dim() != 4:
            raise ValueError("x must be (B, C, H, W), got %s" % (tuple(x.shape),))
        n_top = self._top_k(n_top_layers)
        self._begin(x)
        _, data = self._walk(self._posterior_plan(n_top, use_mode), self._encode_image(x, need_image=False)[0])
        self.noise.end()
        return [_nchw(t) for t in data['z']]

    def _forced_rows(self, z, what):
        """z: a list of L NCHW tensors or None -> ([NHWC contiguous or None], their common row count or None)"""
        L = self.n_layers
        z = list(z)
        if len(z) != L:
            raise ValueError("%s must have one entry per layer (%d), got %d" % (what, L, len(z)))
        rows, forced = None, [None] * L
        for i, t in enumerate(z):
            if t is None:
                continue
            if not t.is_cuda:
                raise K._C.LvaeHipError("LadderVAE (HIP engine) needs GPU tensors; %s[%d] is on %s" % (what, i, t.device))
            if t.dim() != 4 or t.shape[1] != self.z_dims[i]:
                raise ValueError("%s[%d] must be (N, %d, h, w), got %s" % (what, i, self.z_dims[i], tuple(t.shape)))
            if rows is not None and t.shape[0] != rows:
                raise ValueError("the entries of %s disagree about the number of rows: %d and %d" % (what, rows, t.shape[0]))
            rows = int(t.shape[0])
            forced[i] = t.float().permute(0, 2, 3, 1).contiguous()   # (no copy for what encode() returned)
        return forced, rows

    def decode(self, z, n_imgs=None, temperature=None):
        """Engine-only: pictures from latents. z: a list of L entries indexed like z_dims, each an NCHW tensor or None. A given layer is
        forced (forced_latent, generative mode); a None layer is drawn from its prior at `temperature`, by the rules of sample_prior (a float,
        L floats, or a device tensor of per-row temperatures; 0.0 draws no noise). A forced layer below a sampled one is legal. The number of
        rows is that of the forced tensors; n_imgs is needed only when every entry is None (ValueError when it is missing then, and when it
        contradicts the forced tensors). Noise: one `normal` draw per layer that samples, top to bottom, then the likelihood's draws. Returns
        the dict of sample_conditional: 'sample', 'mean', 'mode', 'likelihood_params', 'z' (all L layers). Obeys train / eval mode."""
        forced, rows = self._forced_rows(z, 'z')
        if rows is None:
            if n_imgs is None:
                raise ValueError("n_imgs is needed when no layer is forced")
            rows = int(n_imgs)
            if rows < 1:
                raise ValueError("n_imgs must be at least 1, got %d" % rows)
        elif n_imgs is not None and int(n_imgs) != rows:
            raise ValueError("n_imgs = %d, but the forced latents have %d rows" % (int(n_imgs), rows))
        temps = layer_temperatures(self.n_layers, temperature)
        self._begin(next((t for t in forced if t is not None), None))
        out, data = self._walk(self._forced_plan(forced, temps), rows=rows)
        return self._pictures(out, self.img_shape, data['z'])

    def interpolate(self, x_a, x_b, n_steps=8, n_top_layers=None, mode='slerp', t=None, use_mode=True, temperature=None):
        """Engine-only: the path between the images of x_a and x_b (B, C, H, W) in the latents of the top k = n_top_layers layers (None: all
        L). The 2B rows [x_a; x_b] are encoded in one bottom-up pass and the top k layers run on them in inference mode, so each endpoint's
        chain is conditioned on its own latents (use_mode, the default: the posterior means). Per layer i >= L-k one launch
        (kernels.latent_interp) moves z from x_a's to x_b's at the steps t, spherically (mode 'slerp') or linearly ('lerp'): t defaults to
        linspace(0, 1, n_steps); a float32 device tensor (T,) is taken as it is (any finite value, not validated). The T * B rows, step-major
        (row j * B + b), are then decoded with those layers forced; the layers below draw from their prior at `temperature` (as in
        sample_prior) ONCE per pair: the (B, h, w, Z) draw is repeated for the T steps, so a pair's pictures differ only through the
        interpolated latents. Then final_top_down, the crop and the likelihood without a target.

        Noise, in this order: with use_mode False one `normal` draw of 2B rows per posterior layer, top to bottom; one `normal` draw of B
        rows per prior layer that samples (none at temperature 0.0); the likelihood's draws on T * B rows.

        Returns the dict of decode() plus 'z_a', 'z_b' (the endpoints' NCHW latents per layer, None below L-k) and 't'. Obeys the module's
        train / eval mode like sample_conditional; eval is what is meant: BatchNorm in train mode would couple the 2B rows."""
        if not (x_a.is_cuda and x_b.is_cuda):
            raise K._C.LvaeHipError("LadderVAE (HIP engine) needs GPU tensors; got %s and %s" % (x_a.device, x_b.device))
        if x_a.dim() != 4 or tuple(x_a.shape) != tuple(x_b.shape):
            raise ValueError("x_a and x_b must have one shape (B, C, H, W), got %s and %s" % (tuple(x_a.shape), tuple(x_b.shape)))
        if mode not in K.INTERP_MODES:
            raise ValueError("mode must be 'slerp' or 'lerp', got %r" % (mode,))
        L, B = self.n_layers, int(x_a.shape[0])
        n_top = self._top_k(n_top_layers)
        if t is None:
            if int(n_steps) < 1:
                raise ValueError("n_steps must be at least 1, got %d" % int(n_steps))
            t = torch.linspace(0.0, 1.0, int(n_steps), dtype=torch.float32, device=x_a.device)
        elif not torch.is_tensor(t) or t.dim() != 1 or t.shape[0] < 1 or t.dtype != torch.float32:
            raise ValueError("t must be a float32 device tensor of shape (T,)")
        T = int(t.shape[0])
        temps = layer_temperatures(L, temperature)
        self._begin(x_a)
        bu_values = self._encode_image(torch.cat((x_a, x_b)), need_image=False)[0]
        z_ab = self._walk(self._posterior_plan(n_top, use_mode), bu_values)[1]['z']
        z_a = [None if v is None else v[:B] for v in z_ab]   # (row slices of a contiguous tensor: contiguous)
        z_b = [None if v is None else v[B:] for v in z_ab]
        forced = [None if v is None else K.latent_interp(z_a[i], z_b[i], t, mode) for i, v in enumerate(z_ab)]
        out, data = self._walk(self._forced_plan(forced, temps), rows=T * B, noise=_SharedDraws(self.noise, B, T))
        res = self._pictures(out, x_a.shape[2:], data['z'])
        res.update(z_a=[_nchw(v) for v in z_a], z_b=[_nchw(v) for v in z_b], t=t)
        return res

    INPAINT_INITS = ('zeros', 'mean', 'noise')

    @torch.no_grad()
    def inpaint(self, x, mask, n_iters=10, init='zeros', final='sample', return_history=False, use_graph=None):
        """Engine-only: complete the missing pixels of the NCHW batch x by the pseudo-Gibbs chain of Rezende, Mohamed & Wierstra 2014
        (appendix F). mask as in forward(): non-zero = observed. Eval mode under no_grad; the training flag is restored.

        The completion is kept NHWC. It starts as x where observed and `init` where missing: 'zeros', 'mean' (0.5), 'noise' (one uniform
        [0, 1) draw of x's shape, NCHW on a tape, from the model's noise source) or a (B,C,H,W) tensor. One round pads it, runs the
        bottom-up pass, the top-down pass and the crop, and then the masked likelihood head with `filled` written over the completion: the
        observed pixels keep x, the missing ones take a draw from p(x|z). What x holds under a hidden pixel is never read. final='mean'
        replaces the missing pixels by the head's mean of the last round (one select launch); ValueError for the logistic mixture, which
        has none.

        Noise: begin / the 'noise' draw if any / end once, then per round begin, the draws of forward() in its order, end.
        use_graph=None: the loop of evaluate.iw_log_likelihood (passes.replay_loop) — with PhiloxNoise and n_iters >= 8 two rounds run
        eagerly (they count), one round is captured as a hipGraph and replayed for the rest, with a device copy of that round's ll (and
        history frame) between replays and no host wait; a noise tape always runs eagerly. Eager and replayed runs from one noise
        position agree bit for bit.

        Returns {'completed' (B,C,H,W): observed pixels bit for bit those of x; 'll_observed' (n_iters, B): each round's masked ll, of the
        completion that ENTERED the round; with return_history 'history' (n_iters + 1, B, C, H, W), frame 0 the initial fill (final='mean'
        changes `completed` only)}."""
        if not x.is_cuda:
            raise K._C.LvaeHipError("LadderVAE (HIP engine) needs a GPU tensor; got %s" % x.device)
        if x.dim() != 4:
            raise ValueError("x must be (B, C, H, W), got %s" % (tuple(x.shape),))
        n_iters = int(n_iters)
        if n_iters < 1:
            raise ValueError("n_iters must be at least 1, got %d" % n_iters)
        if final not in ('sample', 'mean'):
            raise ValueError("final must be 'sample' or 'mean', got %r" % (final,))
        if final == 'mean' and isinstance(self.likelihood, DiscretizedLogisticMixLikelihood):
            raise ValueError("final='mean': the discretized logistic mixture has no mean")
        B, C, H, W = (int(s) for s in x.shape)
        dev = x.device
        mask = K.pixel_mask(mask, B, H, W, dev)
        if isinstance(init, str):
            if init not in self.INPAINT_INITS:
                raise ValueError("init must be one of %s or a (B, C, H, W) tensor, got %r" % (self.INPAINT_INITS, init))
        else:
            init = self._mask_fill(init, x, 'init')
            if not torch.is_tensor(init):
                raise ValueError("init must be one of %s or a (B, C, H, W) tensor" % (self.INPAINT_INITS,))
        if use_graph is None:
            use_graph = isinstance(self.noise, PhiloxNoise) and n_iters >= 8
        elif use_graph and not isinstance(self.noise, PhiloxNoise):
            raise ValueError("use_graph needs on-device noise (PhiloxNoise): a noise tape runs eagerly")
        use_graph = bool(use_graph) and n_iters > 2   # (the two eager rounds are all there is otherwise)
        with eval_mode(self):
            self._begin(x)
            img_size = (H, W)
            cur = K.pad_crop(x.contiguous().float(), True, img_size, False)   # NHWC
            if torch.is_tensor(init):
                fill = K.pad_crop(init, True, img_size, False)
            elif init == 'noise':
                fill = self.noise.uniform((B, H, W, C), 0.0, 1.0, dev, channel_last=False)
            else:
                fill = 0.5 if init == 'mean' else 0.0
            K.mask_select(cur, fill, mask, False, out=cur)
            self.noise.end()
            ll_obs = torch.empty((n_iters, B), dtype=torch.float32, device=dev)
            hist = torch.empty((n_iters + 1, B, C, H, W), dtype=torch.float32, device=dev) if return_history else None
            if hist is not None:
                hist[0].copy_(K.pad_crop(cur, False, img_size, True))

            def one_round():
                self.noise.begin(dev)                 # every round: same call sites, next RNG step
                out, _ = self._topdown(self._encode_image(cur, nchw=False, need_image=False)[0])
                ll, info = self.likelihood(self._crop(out, img_size), cur, self.noise, mask=mask, filled_out=cur)
                frame = K.pad_crop(cur, False, img_size, True) if hist is not None else None
                self.noise.end()
                return ll, info, frame

            def keep(r, res):                         # device copies in stream order; the host does not wait
                ll_obs[r].copy_(res[0])
                if hist is not None:
                    hist[r + 1].copy_(res[2])

            _, info, _ = replay_loop(one_round, n_iters, use_graph, keep)
            if final == 'mean':
                K.mask_select(cur, info['mean'].contiguous(), mask, False, out=cur)
            res = {'completed': K.pad_crop(cur, False, img_size, True), 'll_observed': ll_obs}
            if hist is not None:
                res['history'] = hist
            return res

    def get_top_prior_param_shape(self, n_imgs=1):
        """models/lvae.py:364-372."""
        dwnsc = self.overall_downscale_factor
        sz = self.get_padded_size(self.img_shape)
        return (n_imgs, self.z_dims[-1] * 2, sz[0] // dwnsc, sz[1] // dwnsc)
