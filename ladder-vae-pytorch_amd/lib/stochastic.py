"""Stochastic layer on HIP kernels — mirrors the reference's lib/stochastic.py:7-112 (NormalStochasticBlock2d)
and :209-226 (kl_normal_mc): same constructor, same `forward` keyword arguments, same keys in the returned dict.
Tensors are NHWC inside the engine; `data['z']` etc. are returned NHWC and converted by the model.
"""
import torch
from torch import nn

from .. import kernels as K
from .. import ops
from .. import resblock as RB
from .nn import Conv2dParams


class NormalStochasticBlock2d(nn.Module):
    """conv to (mu, logvar) of q (and of p unless top layer), sample z, conv_out(z); log p(z), log q(z), KL."""

    def __init__(self, c_in, c_vars, c_out, kernel=3, transform_p_params=True):
        super().__init__()
        assert kernel % 2 == 1
        pad = kernel // 2
        self.transform_p_params = transform_p_params
        self.c_in, self.c_out, self.c_vars = c_in, c_out, c_vars
        if transform_p_params:
            self.conv_in_p = Conv2dParams(c_in, 2 * c_vars, kernel, padding=pad)
        self.conv_in_q = Conv2dParams(c_in, 2 * c_vars, kernel, padding=pad)
        self.conv_out = Conv2dParams(c_vars, c_out, kernel, padding=pad)
        # engine attribute (not a constructor argument of the reference; LadderVAE.residual_posterior sets it): conv_in_q predicts the
        # posterior as an offset from the prior of this layer, mu_q = mu_p + dmu, logvar_q = logvar_p + dlv
        self.residual_posterior = False

    def forward(self, p_params, q_params=None, forced_latent=None, use_mode=False, force_constant_output=False,
                analytical_kl=False, noise=None, n_img=None, need_kl_elementwise=True, rows=None, stats=None, temperature=None,
                need_q_params=True):
        """residual_posterior (attribute) with q_params given: conv_in_q's output is the offset d = (dmu | dlv) and the core is
        ops.NormalStochResFn, which forms z, both log-probabilities and the KL from the offset; the two convolutions, the core and conv_out
        run as separate launches (the one-launch block of the low-resolution levels is declined). `data['q_params']` is then q_out = p + d,
        detached, or None with need_q_params=False (engine-only keyword: nothing is written for it), and `kl_elementwise` is the value
        composed from (z, p_params, q_out), detached: the sums that carry gradient are the core's. Without q_params nothing changes.
        need_kl_elementwise=False (engine-only keyword, used by TopDownLayer which drops that key, models/lvae_layers.py:163-170):
        skip the pass that materialises `kl_elementwise` (lib/stochastic.py:88-91); the per-sample and per-pixel sums do not need it.
        temperature (engine-only keyword): None or 1.0 is the pass without it. Any other value draws z = mu_p + (t * sigma_p) * eps from the
        prior (lvae_normal_prior_sample_f32; `logprob_p` stays that of the untempered prior): a float, where 0.0 draws no noise and gives
        z = mu_p exactly, or a device float tensor (N,) of per-row temperatures. Sampling only: no q_params, forced_latent or use_mode
        beside it, and no backward."""
        assert (forced_latent is None) or (not use_mode)
        tempered = temperature is not None and (torch.is_tensor(temperature) or float(temperature) != 1.0)
        if tempered and (q_params is not None or forced_latent is not None or use_mode):
            raise ValueError("temperature applies to a draw from the prior: it cannot be combined with q_params, forced_latent or use_mode")
        if not self.transform_p_params:
            assert p_params.size(3) == 2 * self.c_vars
        residual = self.residual_posterior and q_params is not None
        if (q_params is not None and not residual and not tempered and not need_kl_elementwise and not force_constant_output
                and RB.switches.stoch_block):
            fused = self._fused(p_params, q_params, forced_latent, use_mode, analytical_kl, noise, n_img, rows, stats)
            if fused is not None:
                return fused
        # the layer's weight gradients as one launch where the library shares it (ops.WgradShare: training passes of the 16x16 level)
        share = None
        if q_params is not None and not tempered and not force_constant_output:
            ins = ([(p_params, self.conv_in_p)] if self.transform_p_params else []) + [(q_params, self.conv_in_q)]
            z_like = q_params.detach()[..., :self.c_vars]   # conv_out's input: z has q_params' rows and c_vars channels (only its shape is read)
            share = ops.WgradShare.plan(ins + [(z_like, self.conv_out)])
        if self.transform_p_params:
            p_params = ops.conv(p_params, self.conv_in_p, share=share and (share, True))
        if q_params is not None:
            q_params = ops.conv(q_params, self.conv_in_q, share=share and (share, True))
        ref = q_params if q_params is not None else p_params
        N = ref.shape[0] if n_img is None else n_img
        H, W = ref.shape[1], ref.shape[2]
        dev = ref.device
        if tempered:
            return self._tempered(p_params, temperature, force_constant_output, noise, N, H, W, rows)
        if forced_latent is not None:
            mode, src = 2, forced_latent.contiguous()
        elif use_mode:
            mode, src = 1, None
        else:
            mode, src = 0, noise.normal((N, H, W, self.c_vars), dev)
        # rows: engine-only keyword — (N,) views the kernel writes log p(z) and the KL into (rows of the model's [L][N] matrices)
        if residual:
            # q_params is the offset up to here; from here on it is q_out = p_params + d (None where nobody reads it)
            outs = ops.NormalStochResFn.apply(p_params, q_params, src, mode, bool(analytical_kl), self.c_vars, N, rows,
                                              bool(need_q_params or need_kl_elementwise or stats is not None))
            q_params = outs[5]
        else:
            outs = ops.NormalStochFn.apply(p_params, q_params, src, mode, bool(analytical_kl), self.c_vars, N, rows)
        if stats is not None and q_params is not None:
            # stats: engine-only keyword — the float64 (3, U) sums of this layer's latent usage (latent.LatentStats.slot); a pure read of
            # the two parameter tensors, outside autograd
            with torch.no_grad():
                K.latent_stats_fold(p_params.detach(), q_params.detach(), stats, N)
        z = outs[0]
        if force_constant_output:
            # lib/stochastic.py:71-73 — prior experiments only (no gradient flows here)
            if torch.is_grad_enabled() and z.requires_grad:
                raise RuntimeError("force_constant_output is a sampling-time option; run it under torch.no_grad()")
            z = z[0:1].expand_as(z).contiguous()
            p_params = p_params[0:1].expand(N, -1, -1, -1).contiguous()
        out = ops.conv(z, self.conv_out, share=share and (share, False))
        data = {'z': z, 'p_params': p_params, 'q_params': q_params, 'logprob_p': outs[1], 'logprob_q': None,
                'kl_elementwise': None, 'kl_samplewise': None, 'kl_spatial': None}
        if residual or q_params is not None:
            data['logprob_q'], data['kl_samplewise'], data['kl_spatial'] = outs[2], outs[3], outs[4]
            if need_kl_elementwise and residual:
                with torch.no_grad():   # composed from the rounded q_out: a report, not the arithmetic of the sums above
                    data['kl_elementwise'] = K.kl_elementwise_fwd(p_params.detach(), q_params, z.detach(), bool(analytical_kl))
            elif need_kl_elementwise:
                data['kl_elementwise'] = ops.KlElementwiseFn.apply(z, p_params, q_params, bool(analytical_kl))
        return out, data

    def _fused(self, p_in, q_in, forced_latent, use_mode, analytical_kl, noise, n_img, rows, stats):
        """forward() on the low-resolution levels: the two input convolutions, the elementwise core and conv_out in one launch
        (ops.StochBlockFn) where the library takes the call (lvae_stoch_block_ok), else None. Declined here or there: no q_params, tempered
        draws, need_kl_elementwise, force_constant_output, levels above 8x8, other channel counts."""
        has_p = self.transform_p_params
        N = q_in.shape[0] if n_img is None else n_img
        cv = lambda m: (m.weight, m.geom(), m.bias)
        mode = 2 if forced_latent is not None else 1 if use_mode else 0
        if not K.stoch_block_ok(p_in if has_p else None, cv(self.conv_in_p) if has_p else None, None if has_p else p_in, q_in,
                                cv(self.conv_in_q), cv(self.conv_out), mode, N):
            return None
        H, W = q_in.shape[1], q_in.shape[2]
        src = forced_latent.contiguous() if mode == 2 else None if mode == 1 else noise.normal((N, H, W, self.c_vars), q_in.device)
        params = [t for m in ((self.conv_in_p,) if has_p else ()) + (self.conv_in_q, self.conv_out) for t in (m.weight, m.bias)]
        outs = ops.StochBlockFn.apply(p_in if has_p else None, None if has_p else p_in, q_in, src, self, mode, bool(analytical_kl), N, rows, *params)
        out, z, q_params, lp, lq, kl, ks = outs[:7]
        p_params = outs[7] if has_p else p_in
        if stats is not None:
            with torch.no_grad():
                K.latent_stats_fold(p_params.detach(), q_params.detach(), stats, N)
        return out, {'z': z, 'p_params': p_params, 'q_params': q_params, 'logprob_p': lp, 'logprob_q': lq, 'kl_elementwise': None,
                     'kl_samplewise': kl, 'kl_spatial': ks}

    def _tempered(self, p_params, temperature, force_constant_output, noise, N, H, W, rows):
        """The prior draw of forward() at a temperature: same dict, same force_constant_output, one `normal` draw unless the scalar is 0."""
        if torch.is_grad_enabled() and p_params.requires_grad:
            raise RuntimeError("a tempered prior draw has no backward; run it under torch.no_grad()")
        p_params = p_params.detach()
        if torch.is_tensor(temperature):   # (kernels.normal_prior_sample checks its type and shape, the binding its device)
            scalar, row_t = 1.0, temperature
        else:
            scalar, row_t = float(temperature), None
            if not (0.0 <= scalar < float('inf')):
                raise ValueError("temperature must be a finite number >= 0, got %r" % (temperature,))
        eps = None if row_t is None and scalar == 0.0 else noise.normal((N, H, W, self.c_vars), p_params.device)
        z, logprob_p = K.normal_prior_sample(p_params, eps, self.c_vars, N, scalar, row_t, rows=rows)
        if force_constant_output:   # lib/stochastic.py:71-73
            z = z[0:1].expand_as(z).contiguous()
            p_params = p_params[0:1].expand(N, -1, -1, -1).contiguous()
        out = self.conv_out(z)
        return out, {'z': z, 'p_params': p_params, 'q_params': None, 'logprob_p': logprob_p, 'logprob_q': None,
                     'kl_elementwise': None, 'kl_samplewise': None, 'kl_spatial': None}


def kl_normal_mc(z, p_mulv, q_mulv):
    """lib/stochastic.py:209-226 on the HIP kernel: elementwise log q(z) - log p(z). NHWC tensors (mu | logvar on the channel
    axis); p_mulv / q_mulv may have batch size 1 (broadcast over the batch of z), as the reference's broadcasting allows."""
    return ops.KlElementwiseFn.apply(z.contiguous(), p_mulv.contiguous(), q_mulv.contiguous(), False)
