"""Float64 references of the five activation ids (None, elu, relu, leakyrelu, selu) the fused kernels carry, and the kink tools of
tests/test_activations_gpu.py. Plain torch on the CPU; tests/test_act_ref_cpu.py pins everything here without a GPU.

The derivatives of relu, leakyrelu and selu jump at 0. A kernel that forms a pre-activation in fp32 and a float64 reference can land on
opposite sides of that jump, and one such element in 10^6 costs about 1e-3 of norm-relative error. So a backward test whose kernel forms
the pre-activation itself keeps every pre-activation at least MARGIN away from 0:

  - x * scale + shift with handed coefficients (stats_act, lvae_bn_apply.act): `move_off_kink` moves every x whose float64
    pre-activation is within MARGIN of 0 to the pre-activation +-MOVE_TO. The kernels take the coefficients as given, so the statistics
    in the coefficient block need not be those of the moved x.
  - a pre-activation the kernel reduces itself (the recompute form of the gate backward): `zero_near_kink` zeroes the upstream gradient
    at the elements within MARGIN of 0.

Both report how many elements they touched (at most CAP of the tensor: a condition of the test, not a measurement), and `affine_bound` /
`reduction_bound` give the worst-case fp32 rounding error of the pre-activation, which has to stay below MARGIN.

The input builders at the bottom are shared by the GPU tests and the CPU test (same seeds, same shapes), listed in KINK_INPUTS."""
import functools

import torch

LEAKY_SLOPE = 0.01
SELU_ALPHA = 1.6732632423543772848170429916717   # kSeluAlpha / kSeluScale of csrc/lvae_common.h
SELU_SCALE = 1.0507009873554804934193349852946
NAMES = (None, 'elu', 'relu', 'leakyrelu', 'selu')
KINKED = ('relu', 'leakyrelu', 'selu')

MARGIN = 1e-4     # no pre-activation closer to 0 than this
MOVE_TO = 2e-4    # where a moved pre-activation lands
CAP = 1e-3        # largest fraction of a tensor that may be moved or zeroed
EPS32 = 2.0 ** -24


def act(x, name):
    x = x.double()
    if name in (None, 'none'):
        return x.clone()
    if name == 'elu':
        return torch.where(x > 0, x, torch.expm1(x))
    if name == 'relu':
        return torch.where(x > 0, x, torch.zeros_like(x))
    if name == 'leakyrelu':
        return torch.where(x > 0, x, LEAKY_SLOPE * x)
    if name == 'selu':
        return SELU_SCALE * torch.where(x > 0, x, SELU_ALPHA * torch.expm1(x))
    raise KeyError(name)


def act_grad(x, name):
    """d act / dx at x; at 0 the value from the left, as `x > 0 ? ... : ...` gives it"""
    x = x.double()
    one = torch.ones_like(x)
    if name in (None, 'none'):
        return one
    if name == 'elu':
        return torch.where(x > 0, one, torch.exp(x))
    if name == 'relu':
        return torch.where(x > 0, one, 0 * one)
    if name == 'leakyrelu':
        return torch.where(x > 0, one, LEAKY_SLOPE * one)
    if name == 'selu':
        return SELU_SCALE * torch.where(x > 0, one, SELU_ALPHA * torch.exp(x))
    raise KeyError(name)


def act_grad_from_out(y, name):
    """the same derivative written from the output y = act(x) (act_grad_from_out of csrc/lvae_common.h)"""
    y = y.double()
    one = torch.ones_like(y)
    if name in (None, 'none'):
        return one
    if name == 'elu':
        return torch.where(y > 0, one, y + 1)
    if name == 'relu':
        return torch.where(y > 0, one, 0 * one)
    if name == 'leakyrelu':
        return torch.where(y > 0, one, LEAKY_SLOPE * one)
    if name == 'selu':
        return torch.where(y > 0, SELU_SCALE * one, y + SELU_SCALE * SELU_ALPHA)
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------------------------
# kink tools. Tensors are channel-last (..., C); a coefficient block is (4, C) float32: scale, shift, mean, rstd.

def bn_coef(x, gamma, beta, eps=1e-5, dtype=torch.float32):
    """the coefficient block of a training-mode BatchNorm over x (..., C), from float64 statistics (rounded to fp32, as a kernel is handed it)"""
    flat = x.double().reshape(-1, x.shape[-1])
    mean, var = flat.mean(0), flat.var(0, unbiased=False)
    rstd = 1 / torch.sqrt(var + eps)
    scale = gamma.double() * rstd
    return torch.stack([scale, beta.double() - mean * scale, mean, rstd]).to(dtype).contiguous()


def preact(x, coef):
    return x.double() * coef[0].double() + coef[1].double()


def near_kink(pre):
    return pre.abs() < MARGIN


def move_off_kink(x, coef):
    """x (float32) with every element whose float64 pre-activation x * scale + shift lies within MARGIN of 0 moved to the pre-activation
    +-MOVE_TO (the side it was on; exactly 0 goes up). Returns (moved x, number of elements moved)."""
    u = preact(x, coef)
    near = near_kink(u)
    target = torch.where(u >= 0, torch.full_like(u, MOVE_TO), torch.full_like(u, -MOVE_TO))
    moved = ((target - coef[1].double()) / coef[0].double()).float()
    out = torch.where(near, moved, x)
    assert not bool(near_kink(preact(out, coef)).any())
    return out, int(near.sum())


def affine_bound(x, coef):
    """worst-case rounding error of x * scale + shift in fp32: (k + 2) * 2^-24 * sum |term| with k = 2 terms"""
    return float(4 * EPS32 * ((x.double() * coef[0].double()).abs() + coef[1].double().abs()).max())


def reduction_bound(abs_terms, k):
    """worst-case rounding error of a k-term fp32 sum whose absolute terms add up to abs_terms: (k + 2) * 2^-24 * sum |term|"""
    return float((k + 2) * EPS32 * abs_terms.max())


def zero_near_kink(grad, pre):
    """grad with the elements zeroed whose float64 pre-activation lies within MARGIN of 0. Returns (grad, number zeroed)."""
    near = near_kink(pre)
    return torch.where(near, torch.zeros_like(grad), grad), int(near.sum())


def bn_bwd_sums(dh, x, coef, act_name):
    """g = dh * act'(x * scale + shift) and xhat, float64: what a dgrad epilogue sums (sum g, sum g * xhat) for the BatchNorm backward"""
    g = dh.double() * act_grad(preact(x, coef), act_name)
    xh = (x.double() - coef[2].double()) * coef[3].double()
    return g, xh


def bn_bwd_apply(dh, x, coef, act_name, rows):
    """The BatchNorm-backward apply in float64: (partial rows [rows][2][C] as float32, dx = BN'(dh; x) without `add`, sum g, sum g * xhat)."""
    C = x.shape[-1]
    g, xh = bn_bwd_sums(dh, x, coef, act_name)
    gf, gx = g.reshape(-1, C), (g * xh).reshape(-1, C)
    parts = torch.stack([torch.stack([a.sum(0), b.sum(0)]) for a, b in zip(gf.tensor_split(rows), gx.tensor_split(rows))])
    dx = (g - gf.mean(0) - xh * gx.mean(0)) * coef[0].double()
    return parts.float().contiguous(), dx, gf.sum(0), gx.sum(0)


# ---------------------------------------------------------------------------------------------------------------------------------
# input builders (CPU tensors; made once per argument tuple and never modified by the tests)

@functools.lru_cache(maxsize=None)
def affine_input(seed, N, H, W, C=64, x_scale=2.0, x_shift=1.0):
    """A BatchNorm input x (N, H, W, C) with both signs of the pre-activation, its coefficient block, moved off the kink (rule 3).
    Returns dict(x, coef, moved, numel, bound)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, C, generator=g) * x_scale + x_shift
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    coef = bn_coef(x, gamma, beta)
    xm, moved = move_off_kink(x, coef)
    return dict(x=xm, coef=coef, moved=moved, numel=x.numel(), bound=affine_bound(xm, coef))


@functools.lru_cache(maxsize=None)
def apply_input(seed, N, H, W, act_name, rows, C=64):
    """A deferred BatchNorm-backward apply (lvae_bn_apply): x, coefficient block, dh, add, partial rows, and dy = BN'(dh; x) in float64
    (without add), sum g and sum g * xhat. x is moved off the kink (rule 3)."""
    p = dict(affine_input(seed, N, H, W, C, 1.0, 0.0))
    g = torch.Generator().manual_seed(seed + 1)
    p['dh'], p['add'] = torch.randn(N, H, W, C, generator=g), torch.randn(N, H, W, C, generator=g)
    p['parts'], p['dy'], p['sg'], p['sgx'] = bn_bwd_apply(p['dh'], p['x'], p['coef'], act_name, rows)
    p['act'] = act_name
    return p


@functools.lru_cache(maxsize=None)
def gate_input(seed, N, H, W, C=64):
    """Operands of a gate convolution whose pre-activations the backward forms itself (rule 4): y (N, H, W, C), w (2C, C, 1, 1), b (2C),
    dout, the float64 pre-activations ab (N, H, W, 2C), dout zeroed where the activated half lies within MARGIN of 0."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(N, H, W, C, generator=g)
    w = torch.randn(2 * C, C, 1, 1, generator=g) / C ** 0.5
    b = torch.randn(2 * C, generator=g)
    dout = torch.randn(N, H, W, C, generator=g)
    w2 = w[:, :, 0, 0].double()
    ab = y.double().reshape(-1, C) @ w2.t() + b.double()
    abs_terms = y.double().abs().reshape(-1, C) @ w2[:C].abs().t() + b[:C].double().abs()
    pre = ab[:, :C].reshape(N, H, W, C)
    dz, zeroed = zero_near_kink(dout, pre)
    return dict(y=y, w=w, b=b, dout=dz, ab=ab.reshape(N, H, W, 2 * C), near=near_kink(pre), zeroed=zeroed, numel=dout.numel(),
                bound=reduction_bound(abs_terms, C + 1))


# every kinked input set of tests/test_activations_gpu.py: (builder, arguments). tests/test_act_ref_cpu.py asserts the caps for each.
KINK_INPUTS = [
    # BatchNorm-backward sums in the dgrad epilogues (stats_act)
    (affine_input, (46, 3, 8, 8)), (affine_input, (46, 37, 4, 4)), (affine_input, (46, 66, 16, 16)), (affine_input, (46, 200, 16, 16)), (affine_input, (46, 256, 16, 16)),
    # deferred applies (ap.act): weight gradient, persistent gate backward, merge backward, the small-level block chain
    (apply_input, (70, 70, 16, 16, 'relu', 256)), (apply_input, (71, 70, 16, 16, 'selu', 256)),
    (apply_input, (72, 64, 16, 16, 'leakyrelu', 256)), (apply_input, (73, 64, 16, 16, 'relu', 3)),
    (apply_input, (74, 64, 16, 16, 'elu', 256)), (apply_input, (75, 70, 16, 16, 'selu', 7)),
    (apply_input, (76, 4, 8, 8, 'leakyrelu', 3)), (apply_input, (77, 37, 2, 2, 'selu', 7)),
    (apply_input, (78, 4, 8, 8, 'relu', 1)), (apply_input, (79, 4, 8, 8, 'selu', 3)), (apply_input, (82, 4, 8, 8, 'leakyrelu', 1)),
    (apply_input, (83, 4, 8, 8, 'relu', 3)), (apply_input, (84, 4, 8, 8, 'selu', 1)),
    # the recompute form of the gate backward
    (gate_input, (80, 64, 16, 16)), (gate_input, (81, 70, 16, 16)),
]
