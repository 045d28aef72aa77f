"""The reference of KL balancing (lvae_amd/balance.py, csrc/kl_balance.hip), in plain torch on the CPU at the dtype of its inputs
(float64: r64, float32: r32), with gradients by autograd and gamma detached:

    m_l     = mean_n |kl[l][n]| + 0.01
    gamma_l = (m_l / alpha_l) / mean_j (m_j / alpha_j)      while the rule is active (beta < 1), else 1
    kl_loss = sum_l gamma_l * mean_n c(kl[l][n])            c(v) = v if free_bits < 1e-6 else max(v, free_bits)
    kl_sep[n] = sum_l kl[l][n]     kl_avg_layerwise[l] = mean_n kl[l][n]     kl = mean_n kl_sep[n]       (plain)

Also the kernel tests' shapes, inputs and beta forms. The comparison rules are those of docs/ELEMENTWISE_PARITY.md as tests/spectral_ref.py
writes them (close_elem, close_sum): no tolerance is chosen here.
"""
import numpy as np
import torch

FLOOR = 0.01

SHAPES = [(1, 1), (1, 257), (3, 1), (3, 255), (3, 256), (3, 257), (20, 1000)]   # thread-stride edges, one layer, one row
FREE_BITS = [0.0, 0.5]
ANNEAL_STEPS = 10
# (name, constant beta or None, counter or None): the counter inside, at and past ANNEAL_STEPS
BETAS = [('beta0', 0.0, None), ('beta0.3', 0.3, None), ('beta1', 1.0, None), ('anneal-inside', None, 3), ('anneal-at', None, ANNEAL_STEPS),
         ('anneal-past', None, 25)]


def beta_of(const, counter, anneal_steps=ANNEAL_STEPS):
    """The float32 beta of a form: the constant, or linear_anneal(counter, 0, 1, anneal_steps) formed in double and rounded once."""
    if counter is None:
        return float(np.float32(const))
    if anneal_steps <= 0:
        return 1.0
    return float(np.float32(min(max(counter / float(anneal_steps), 0.0), 1.0)))


def active(const, counter, anneal_steps=ANNEAL_STEPS):
    return beta_of(const, counter, anneal_steps) < 1.0


def clamp(kl, free_bits):
    """The free-bits clamp as kl_book_fwd_kernel applies it (its gradient passes where kl >= free_bits, as torch.clamp's does)."""
    return kl if free_bits < 1e-6 else torch.clamp(kl, min=free_bits)


def gamma(kl, alpha, is_active=True, floor=FLOOR, use_alpha=True):
    """The coefficients (L,), constants of the gradient. floor / use_alpha: the two wrong references the tests must tell from the right one."""
    kl = kl.detach()
    if not is_active:
        return torch.ones(kl.shape[0], dtype=kl.dtype)
    q = kl.abs().mean(dim=1) + floor
    if use_alpha:
        q = q / alpha.to(kl.dtype)
    return q / q.mean()


def forward(kl, alpha, free_bits, is_active, **wrong):
    """dict(kl_sep, kl_avg, kl_loss, kl, coeff, loss_abs): loss_abs is the sum of the absolute terms gamma_l |c(kl[l][n])| / N of kl_loss,
    the yardstick of the sum rule."""
    L, N = kl.shape
    g = gamma(kl, alpha, is_active, **wrong)
    c = clamp(kl, free_bits)
    kl_sep = kl.sum(dim=0)
    return {'kl_sep': kl_sep, 'kl_avg': kl.mean(dim=1), 'kl_loss': (g * c.mean(dim=1)).sum(), 'kl': kl_sep.mean(), 'coeff': g,
            'loss_abs': (g[:, None] * c.detach().abs()).sum() / N}


def backward(kl, alpha, free_bits, is_active, g_sep=None, g_avg=None, g_scal=None):
    """dkl (L, N) by autograd: the gradient of <g_sep, kl_sep> + <g_avg, kl_avg> + g_scal[0] kl_loss + g_scal[1] kl, absent ones zero."""
    x = kl.detach().clone().requires_grad_(True)
    r = forward(x, alpha, free_bits, is_active)
    tot = (x * 0).sum()
    if g_sep is not None:
        tot = tot + (g_sep.to(x.dtype) * r['kl_sep']).sum()
    if g_avg is not None:
        tot = tot + (g_avg.to(x.dtype) * r['kl_avg']).sum()
    if g_scal is not None:
        tot = tot + g_scal[0].to(x.dtype) * r['kl_loss'] + g_scal[1].to(x.dtype) * r['kl']
    tot.backward()
    return x.grad


# ---- inputs of the kernel tests (float32 values: what the device gets is what the references read) ---------------------------------------
def _gen(L, N, salt):
    return torch.Generator().manual_seed(1000003 * L + 1009 * N + salt)


def kl_values(kind, L, N):
    """'random': KLs with negative entries, every layer at its own scale between 0.1 and 5 and its own positive shift. 'zeros': the dead
    ladder. 'cond': one layer at 1e4 beside layers at 1e-6, the conditioning of the normalisation."""
    g = _gen(L, N, 1)
    if kind == 'random':
        scale = torch.logspace(-1, 0.7, L, dtype=torch.float64)[torch.randperm(L, generator=g)]
        kl = (torch.randn(L, N, generator=g, dtype=torch.float64) + 0.5) * scale[:, None]
    elif kind == 'zeros':
        kl = torch.zeros(L, N, dtype=torch.float64)
    elif kind == 'cond':
        kl = 1e-6 * (0.5 + torch.rand(L, N, generator=g, dtype=torch.float64))
        kl[L // 2] = 1e4 * (0.5 + torch.rand(N, generator=g, dtype=torch.float64))
    else:
        raise KeyError(kind)
    return kl.float()


KINDS = ['random', 'zeros', 'cond']


def alpha_values(kind, L):
    """'uniform': all 1. 'spread': 4 ** (6 l / (L - 1)), from 1 to 4096 (the `square` rule over seven resolutions), in float32."""
    if kind == 'uniform' or L == 1:
        return torch.ones(L, dtype=torch.float32)
    return torch.pow(torch.tensor(4.0, dtype=torch.float64), 6.0 * torch.arange(L, dtype=torch.float64) / (L - 1)).float()


ALPHAS = ['uniform', 'spread']


def upstream(L, N):
    """Non-trivial g_sep (N,), g_avg (L,), g_scalars (2,) in float32. The scalars' gradients are of the order of N, so that their part of
    dkl, gamma_l g / N, is of the order of gamma_l: above the rule's absolute term at every N, where a wrong gamma shows."""
    g = _gen(L, N, 2)
    return (torch.randn(N, generator=g).float(), torch.randn(L, generator=g).float(),
            (N * (torch.tensor([0.7, -1.3]) + 0.1 * torch.randn(2, generator=g))).float())
