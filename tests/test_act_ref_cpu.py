"""tests/act_ref.py without a GPU: the float64 activations and derivatives against torch's own and autograd, the derivative written from
the output, the kink tools, and the caps of every kinked input set tests/test_activations_gpu.py uses (same seeds, same shapes)."""
import os

import pytest
import torch
import torch.nn.functional as F

import act_ref as R

torch.set_num_threads(min(16, os.cpu_count() or 1))

TORCH = {None: lambda t: t, 'elu': F.elu, 'relu': F.relu, 'leakyrelu': lambda t: F.leaky_relu(t, 0.01), 'selu': F.selu}


def grid():
    g = torch.Generator().manual_seed(1)
    x = torch.cat([torch.randn(4096, generator=g, dtype=torch.float64) * 3, torch.linspace(-1e-3, 1e-3, 401, dtype=torch.float64),
                   torch.tensor([-30.0, -1e-12, 1e-12, 30.0], dtype=torch.float64)])
    return x[x != 0]


@pytest.mark.parametrize('name', R.NAMES)
def test_activation_and_derivative_are_torchs(name):
    x = grid().requires_grad_(True)
    y = TORCH[name](x)
    torch.testing.assert_close(R.act(x.detach(), name), y.detach(), rtol=1e-14, atol=1e-15)
    y.sum().backward()
    torch.testing.assert_close(R.act_grad(x.detach(), name), x.grad, rtol=1e-14, atol=1e-15)


def test_constants_are_the_kernels():
    src = open(os.path.join(os.path.dirname(__file__), '..', 'ladder-vae-pytorch_amd', 'csrc', 'lvae_common.h')).read()
    assert 'kSeluAlpha = 1.6732632423543772848170429916717f' in src and 'kSeluScale = 1.0507009873554804934193349852946f' in src
    assert '0.01f * x' in src
    assert (R.LEAKY_SLOPE, R.SELU_ALPHA, R.SELU_SCALE) == (0.01, 1.6732632423543772848170429916717, 1.0507009873554804934193349852946)
    assert R.NAMES == (None, 'elu', 'relu', 'leakyrelu', 'selu')


@pytest.mark.parametrize('name', R.NAMES)
def test_derivative_from_the_output_is_the_derivative(name):
    x = grid()
    torch.testing.assert_close(R.act_grad_from_out(R.act(x, name), name), R.act_grad(x, name), rtol=1e-12, atol=1e-14)


def test_derivative_at_zero_is_the_left_one():
    z = torch.zeros(1, dtype=torch.float64)
    assert float(R.act_grad(z, 'relu')) == 0.0 and float(R.act_grad(z, 'leakyrelu')) == 0.01
    assert float(R.act_grad(z, 'selu')) == R.SELU_SCALE * R.SELU_ALPHA and float(R.act_grad(z, 'elu')) == 1.0


def test_move_off_kink_moves_exactly_the_near_elements():
    C = 8
    g = torch.Generator().manual_seed(2)
    x = torch.randn(50, C, generator=g)
    coef = R.bn_coef(x, torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3)
    planted = ((torch.tensor([0.0, 5e-5, -5e-5, 9.9e-5, -1.5e-4]).double() - coef[1, 3].double()) / coef[0, 3].double()).float()
    x[:5, 3] = planted
    before = R.preact(x, coef)
    near = R.near_kink(before)
    assert int(near[:5, 3].sum()) == 4 and not bool(near[4, 3])
    xm, moved = R.move_off_kink(x, coef)
    assert moved == int(near.sum()) >= 4
    assert torch.equal(xm[~near], x[~near])
    after = R.preact(xm, coef)
    assert float(after.abs().min()) > R.MARGIN
    torch.testing.assert_close(after[near].abs(), torch.full_like(after[near], R.MOVE_TO), rtol=0, atol=1e-6)
    assert bool((torch.sign(after[near]) == torch.where(before[near] >= 0, 1.0, -1.0)).all())   # each stays on its side, 0 goes up


def test_zero_near_kink_and_bounds():
    pre = torch.tensor([[0.0, 5e-5, -9e-5, 1.1e-4, -3.0]], dtype=torch.float64)
    grad, n = R.zero_near_kink(torch.ones(1, 5), pre)
    assert n == 3 and grad.tolist() == [[0.0, 0.0, 0.0, 1.0, 1.0]]
    x = torch.tensor([[2.0, -4.0]])
    coef = torch.tensor([[1.5, 0.5], [0.25, -1.0], [0.0, 0.0], [1.0, 1.0]])
    assert R.affine_bound(x, coef) == 4 * 2.0 ** -24 * 3.25
    assert R.reduction_bound(torch.tensor([1.0, 7.0]), 65) == 67 * 2.0 ** -24 * 7.0


def test_bn_backward_apply_is_autograd():
    """bn_bwd_apply == autograd of act(batch_norm(x)) for every activation, with x off the kink"""
    C = 8
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(3, 5, 5, C, generator=g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    dh = torch.randn(3, 5, 5, C, generator=g)
    for name in R.NAMES:
        x, _ = R.move_off_kink(x0, R.bn_coef(x0, gamma, beta))
        coef = R.bn_coef(x, gamma, beta, dtype=torch.float64)   # (the statistics of the moved x: this test differentiates through them)
        xr = x.double().requires_grad_(True)
        ga, be = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        h = TORCH[name](F.batch_norm(xr.permute(0, 3, 1, 2), None, None, ga, be, True, 0.1, 1e-5))
        h.backward(dh.double().permute(0, 3, 1, 2))
        parts, dx, sg, sgx = R.bn_bwd_apply(dh, x, coef, name, 7)
        torch.testing.assert_close(dx, xr.grad, rtol=1e-9, atol=1e-10)
        torch.testing.assert_close(sg, be.grad, rtol=1e-9, atol=1e-10)
        torch.testing.assert_close(sgx, ga.grad, rtol=1e-9, atol=1e-10)
        torch.testing.assert_close(parts.double().sum(0), torch.stack([sg, sgx]), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize('builder,args', R.KINK_INPUTS, ids=lambda v: getattr(v, '__name__', '-'.join(str(a) for a in v) if isinstance(v, tuple) else None))
def test_caps_of_every_kinked_input_of_the_gpu_file(builder, args):
    """at most CAP of the elements moved or zeroed; the worst-case rounding error of the pre-activation below MARGIN; nothing left near 0"""
    p = builder(*args)
    touched = p['moved'] if 'moved' in p else p['zeroed']
    print('%s%s: %d of %d touched (%.2e), rounding bound %.2e' % (builder.__name__, args, touched, p['numel'], touched / p['numel'], p['bound']))
    assert touched <= R.CAP * p['numel']
    assert p['bound'] < R.MARGIN
    if 'coef' in p:
        pre = R.preact(p['x'], p['coef'])
        assert float(pre.abs().min()) > R.MARGIN
        assert 0.3 < float((pre < 0).double().mean()) < 0.7    # both signs, about half the mass negative
    else:
        assert not bool((p['dout'] != 0)[p['near']].any()) and p['zeroed'] == int(p['near'].sum())
        assert 0.3 < float((p['ab'][..., :64] < 0).double().mean()) < 0.7
