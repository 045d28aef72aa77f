"""The reference of the spectral regulariser's power iteration (lvae_amd/spectral.py, csrc/spectral.hip), in plain torch on the CPU, at the
dtype of its inputs (float64: r64, float32: r32). It works on the LOGICAL weight of a convolution, (Cout, Cin, KH, KW) plain or
(Cin, Cout, KH, KW) transposed, the way torch.nn.utils.spectral_norm does (dim 0 / dim 1: the output channels index u), and returns v in
the logical shape (Cin, KH, KW): comparing it with the kernel's v, which is ordered (kh, kw, cin) like the arena, also checks the arena's
permutation.

    M  = weight with Cout first, flattened: [Cout][Cin * KH * KW]
    s  = M^T u      v' = s / max(|s|, 1e-12)
    t  = M v'       u' = t / max(|t|, 1e-12)       sigma = |t|
    d(lam * sigma) / dW = lam * u' v'^T in the weight's logical shape, u' and v' constants

Also the tests' input builder and the two comparison rules of docs/ELEMENTWISE_PARITY.md.
"""
import math

import torch

EPS = 1e-12

# (K, Cout) of the kernel tests: what each stands for is in tests/test_spectral_gpu.py
SHAPES = [(75, 64), (576, 64), (64, 128), (128, 64), (288, 64), (576, 100), (576, 1), (576, 3), (1600, 64), (9, 2)]


def out_first(weight, transposed=False):
    """The logical weight with the output channels first: (Cout, Cin, KH, KW)."""
    return weight.transpose(0, 1) if transposed else weight


def arena_matrix(weight, transposed=False):
    """The [KH*KW*Cin][Cout] matrix the arena stores for a logical weight: rows (kh, kw, cin), columns cout."""
    w = out_first(weight, transposed)
    return w.permute(2, 3, 1, 0).reshape(-1, w.shape[0])


def logical_weight(A, cin, kh, kw, transposed=False):
    """The inverse of arena_matrix: the logical weight whose arena matrix is A ([kh*kw*cin][cout])."""
    w = A.reshape(kh, kw, cin, A.shape[1]).permute(3, 2, 0, 1)
    return (w.transpose(0, 1) if transposed else w).contiguous()


def arena_order(v):
    """A logical v (Cin, KH, KW) in the arena's row order (kh, kw, cin), flat."""
    return v.permute(1, 2, 0).reshape(-1)


def step(weight, u, transposed=False):
    """One power-iteration step from u (Cout) -> dict(s, v, t, u, sigma, s_abs, t_abs): s and v in the logical shape (Cin, KH, KW); s_abs /
    t_abs are the sums of the absolute terms of each s / t element (the yardstick of the per-sum rule), sigma_abs that of sigma = v'^T M^T u',
    sum |v'_k| |M_ck| |u'_c|."""
    w = out_first(weight, transposed)
    M = w.reshape(w.shape[0], -1)
    s = M.t() @ u
    v = s / s.norm().clamp_min(EPS)
    t = M @ v
    sigma = t.norm()
    un = t / sigma.clamp_min(EPS)
    return {'s': s.reshape(w.shape[1:]), 'v': v.reshape(w.shape[1:]), 't': t, 'u': un, 'sigma': sigma,
            's_abs': (M.abs().t() @ u.abs()).reshape(w.shape[1:]), 't_abs': M.abs() @ v.abs(), 'sigma_abs': (M.abs() @ v.abs()) @ un.abs()}


def steps(weight, u, n, transposed=False):
    """n steps; the last step's dict."""
    r = None
    for _ in range(n):
        r = step(weight, u, transposed)
        u = r['u']
    return r


def grad_increment(r, lam, gscale=1.0, transposed=False):
    """(lam / gscale) u' v'^T in the weight's logical shape, from a step's dict (same dtype)."""
    coef = torch.tensor(lam, dtype=r['u'].dtype) / torch.tensor(gscale, dtype=r['u'].dtype)
    g = (coef * r['v']).unsqueeze(0) * r['u'].view(-1, 1, 1, 1)
    return g.transpose(0, 1) if transposed else g


def builder(K, C, seed=0):
    """A = R / sqrt(K) + 4 a b^T in float64 ([K][C]): R standard normal, a and b unit vectors, seeded per shape. One dominant singular
    value near 4 over a bulk below 1 + sqrt(C / K), so that 20 power iterations converge far below fp32's resolution."""
    g = torch.Generator().manual_seed(1000003 * K + 1009 * C + seed)
    R = torch.randn(K, C, generator=g, dtype=torch.float64)
    a = torch.randn(K, generator=g, dtype=torch.float64)
    b = torch.randn(C, generator=g, dtype=torch.float64)
    return R / math.sqrt(K) + 4.0 * torch.outer(a / a.norm(), b / b.norm())


def start_u(C, seed=0):
    g = torch.Generator().manual_seed(77 + 13 * C + seed)
    u = torch.randn(C, generator=g, dtype=torch.float64)
    return u / u.norm()


# ---- the comparison rules of docs/ELEMENTWISE_PARITY.md: no tolerance is chosen per test -------------------------------------------------
def close_elem(tag, got, r64, r32):
    """|kernel - r64| <= 2 max|r32 - r64| + 1e-5 |r64| + 1e-6, element-wise; prints before it asserts."""
    got, r64, r32 = got.detach().double().cpu().reshape(-1), r64.detach().double().reshape(-1), r32.detach().double().reshape(-1)
    assert got.shape == r64.shape == r32.shape, (tag, got.shape, r64.shape, r32.shape)
    assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(r32).all()), tag + ': a reference value is not finite'
    e32 = float((r32 - r64).abs().max())
    err, bound = (got - r64).abs(), 2 * e32 + 1e-5 * r64.abs() + 1e-6
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))
    k = int((err / bound).argmax())
    print('yardstick | %-58s | kernel %.3e | r32 %.3e | bound %.3e | n %d' % (tag, float(err[k]), e32, float(bound[k]), err.numel()))
    assert bool((err <= bound).all()), '%s: |kernel - r64| = %.6e at flat element %d, bound %.6e (r32 error %.3e)' % (
        tag, float(err[k]), k, float(bound[k]), e32)
    return float(err[k]), e32, float(bound[k])


def close_sum(tag, got, r64, r32, abs_terms):
    """|kernel - r64| <= 2 max|r32 - r64| + 4e-6 sum_i |term_i| (abs_terms: that sum per element, in float64)."""
    got, r64, r32 = got.detach().double().cpu().reshape(-1), r64.detach().double().reshape(-1), r32.detach().double().reshape(-1)
    abs_terms = abs_terms.detach().double().reshape(-1)
    assert got.shape == r64.shape == r32.shape == abs_terms.shape, (tag, got.shape, r64.shape, r32.shape, abs_terms.shape)
    assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(r32).all()), tag + ': a reference value is not finite'
    e32 = float((r32 - r64).abs().max())
    err, bound = (got - r64).abs(), 2 * e32 + 4e-6 * abs_terms
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))
    k = int((err / bound.clamp_min(1e-300)).argmax())
    print('yardstick | %-58s | kernel %.3e | r32 %.3e | bound %.3e | n %d' % (tag, float(err[k]), e32, float(bound[k]), err.numel()))
    assert bool((err <= bound).all()), '%s: |kernel - r64| = %.6e at flat element %d, bound %.6e (r32 error %.3e)' % (
        tag, float(err[k]), k, float(bound[k]), e32)
    return float(err[k]), e32, float(bound[k])
