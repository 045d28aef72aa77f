"""The torch formula of the residual stochastic core (csrc/stochastic_residual.hip): a helper of the residual-posterior tests, not a test.

The posterior is given as an offset d = (dmu | dlv) from the prior p = (mu_p | logvar_p) of the same layer, mu_q = mu_p + dmu and
logvar_q = logvar_p + dlv, and every output is formed from the offset, never from the rounded sum p + d. The helper is dtype-generic: on
float64 tensors it is r64, on float32 CPU tensors r32, the two references of docs/ELEMENTWISE_PARITY.md; gradients come from autograd.
"""
import math

import torch

LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)


def residual_core(p, d, e, mode, analytical, Z, N):
    """p (N|1,H,W,2Z), d (N,H,W,2Z); e = eps (mode 0), unused (mode 1) or the forced latent (mode 2), (N,H,W,Z). Returns a dict:
    z (N,H,W,Z); the per-sample sums lp, lq, kl with lp_abs, lq_abs, kl_abs, the sums of their terms' magnitudes; ks (N,H,W), the analytical KL
    summed over Z; q = p + d; and the element-wise terms lp_e, lq_e, kan_e, kl_e."""
    pmu, plv, dmu, dlv = p[..., :Z], p[..., Z:], d[..., :Z], d[..., Z:]
    sq = (plv / 2).exp() * (dlv / 2).exp()
    ivp = (-plv).exp()
    if mode == 0:
        se = sq * e
        z, a, u = (pmu + dmu) + se, dmu + se, e
    elif mode == 1:
        z, a, u = pmu + dmu, dmu, torch.zeros_like(dmu)
    else:
        z = e
        a = z - pmu
        u = (a - dmu) / sq
    ap, uu = a * a * ivp, u * u
    lp = (-0.5 * ap - 0.5 * plv - LOG_SQRT_2PI).expand(N, *dmu.shape[1:])
    lq = -0.5 * uu - 0.5 * (plv + dlv) - LOG_SQRT_2PI
    kan = 0.5 * (torch.expm1(dlv) - dlv + dmu * dmu * ivp)
    kl = kan if analytical else 0.5 * (ap - uu) - 0.5 * dlv
    s = lambda t: t.sum((1, 2, 3))
    return {'z': z.expand(N, *dmu.shape[1:]), 'lp': s(lp), 'lp_abs': s(lp.abs()), 'lq': s(lq), 'lq_abs': s(lq.abs()), 'kl': s(kl),
            'kl_abs': s(kl.abs()), 'ks': kan.sum(-1), 'q': p + d, 'lp_e': lp, 'lq_e': lq, 'kan_e': kan, 'kl_e': kl}


def absolute_kl(q, p, Z):
    """The analytical KL as the absolute core forms it (normal_kl of csrc/lvae_common.h) from q and p, in the dtype of its arguments."""
    qmu, qlv, pmu, plv = q[..., :Z], q[..., Z:], p[..., :Z], p[..., Z:]
    qs, ps = (qlv / 2).exp(), (plv / 2).exp()
    vr = (qs / ps) ** 2
    t = (qmu - pmu) / ps
    return 0.5 * (vr + t * t - 1.0 - vr.log())


def discriminating_inputs(N=3, HW=80, Z=32, seed=2020):
    """Float32 inputs with |mu_p| >> sigma_p, where a trained deep ladder lives: mu_p ~ U(-100, 100), logvar_p ~ U(-10, -4),
    dmu ~ U(-1, 1) sigma_p, dlv ~ U(-0.5, 0.5). Returns p, d (N,HW,1,2Z) and eps (N,HW,1,Z)."""
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi: torch.rand(N, HW, 1, Z, generator=g, dtype=torch.float64) * (hi - lo) + lo
    pmu, plv = u(-100., 100.), u(-10., -4.)
    dmu, dlv = u(-1., 1.) * (plv / 2).exp(), u(-0.5, 0.5)
    eps = torch.randn(N, HW, 1, Z, generator=g, dtype=torch.float64)
    return torch.cat((pmu, plv), -1).float(), torch.cat((dmu, dlv), -1).float(), eps.float()


def elem_bound(r64, r32):
    """The element-wise rule of docs/ELEMENTWISE_PARITY.md, per element."""
    r64, r32 = r64.detach().double(), r32.detach().double()
    return 2.0 * float((r32 - r64).abs().max()) + 1e-5 * r64.abs() + 1e-6


def sum_bound(r64, r32, abs_terms):
    """The per-sample-sum rule of docs/ELEMENTWISE_PARITY.md, per sum."""
    r64, r32 = r64.detach().double(), r32.detach().double()
    return 2.0 * float((r32 - r64).abs().max()) + 4e-6 * abs_terms.detach().double()
