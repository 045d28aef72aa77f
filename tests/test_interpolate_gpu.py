"""Interpolation between two images in the latents of the top k layers: the interpolation kernel against its formula, its exact endpoints
and refusals, LadderVAE.interpolate against the CPU oracle on one noise tape, identities of encode / decode / interpolate on the device,
their ValueErrors, and the evaluation CLI.

Kernel: the two rules of docs/ELEMENTWISE_PARITY.md, unchanged; the element-wise one applies: |kernel - r64| <= 2 max|r32 - r64| +
1e-5 |r64| + 1e-6. r64 is the formula of include/lvae_hip.h in float64 on the CPU (row sums, the angle 2 atan2(|a^ - c^|, |a^ + c^|), both
coefficients and their combination); r32 is those float64 coefficients rounded to float32 and combined in float32, the kernel's own design.
Every comparison prints `yardstick | case | kernel error | r32 error | bound` before it asserts (run with -s)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden

pytestmark = pytest.mark.gpu

INF, NAN = float('inf'), float('nan')
MODES = ('lerp', 'slerp')
MIN_SIN = 1e-6   # the fallback threshold of the header


@pytest.fixture(scope='module')
def K():
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels
    return kernels


def close_elem(tag, got, r64, r32):
    got, r64, r32 = got.detach().double().cpu(), r64.detach().double(), r32.detach().double()
    assert got.shape == r64.shape == r32.shape, (tag, got.shape, r64.shape, r32.shape)
    e32 = float((r32 - r64).abs().max())
    bound = (2.0 * e32 + 1e-5 * r64.abs() + 1e-6).reshape(-1)
    err = (got - r64).abs().reshape(-1)
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, INF))
    k = int(torch.argmax(err / bound))
    print('yardstick | %-62s | kernel %.3e | r32 %.3e | bound %.3e | n %d' % (tag, float(err[k]), e32, float(bound[k]), err.numel()))
    assert bool((err <= bound).all()), '%s: |kernel - r64| = %.6e at flat element %d, bound %.6e (r32 error %.3e)' % (
        tag, float(err[k]), k, float(bound[k]), e32)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. lvae_latent_interp_f32 against its formula
# ---------------------------------------------------------------------------------------------------------------------------------
def coefficients64(a, c, t, mode):
    """(wa, wc), each (T, B) float64: the header's formula. a, c (B, n) and t (T,) float32 on the CPU."""
    a, c, t = a.double(), c.double(), t.double()
    T, B = t.shape[0], a.shape[0]
    wa, wc = (1.0 - t)[:, None].repeat(1, B), t[:, None].repeat(1, B)
    if mode == 'slerp':
        for b in range(B):
            na, nc = a[b].pow(2).sum().sqrt(), c[b].pow(2).sum().sqrt()
            if float(na) == 0.0 or float(nc) == 0.0:
                continue
            ah, ch = a[b] / na, c[b] / nc
            omega = 2.0 * torch.atan2((ah - ch).pow(2).sum().sqrt(), (ah + ch).pow(2).sum().sqrt())
            s = torch.sin(omega)
            if float(s) < MIN_SIN:
                continue
            wa[:, b], wc[:, b] = torch.sin((1.0 - t) * omega) / s, torch.sin(t * omega) / s
    return wa, wc


def interp_ref(a, c, t, mode):
    """(r64, r32), each (T * B, n), step-major; rows at t == 0 / t == 1 are a / c themselves (the endpoints are branches)"""
    wa, wc = coefficients64(a, c, t, mode)
    r64 = wa[:, :, None] * a.double()[None] + wc[:, :, None] * c.double()[None]
    r32 = wa.float()[:, :, None] * a[None] + wc.float()[:, :, None] * c[None]
    for j, tj in enumerate(t.tolist()):
        if tj == 0.0:
            r64[j], r32[j] = a.double(), a
        elif tj == 1.0:
            r64[j], r32[j] = c.double(), c
    return r64.reshape(-1, a.shape[1]), r32.reshape(-1, a.shape[1])


def _off_by_one_float(t):
    """a contiguous device copy of t that starts 4 bytes past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, device='cuda')
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def _run(K, a, c, t, mode, misaligned=False):
    if not misaligned:
        return K.latent_interp(a.cuda(), c.cuda(), t.cuda(), mode)
    from lvae_amd import _C
    B, n, T = a.shape[0], a.shape[1], t.shape[0]
    ad, cd, td = _off_by_one_float(a), _off_by_one_float(c), t.cuda()
    out = _off_by_one_float(torch.zeros(T * B, n))
    ws = K.workspace(_C.load().lvae_latent_interp_workspace(B, T), out.device)
    K.call('lvae_latent_interp_f32', K.ptr(ad), K.ptr(cd), K.ptr(td), B, n, T, K.INTERP_MODES[mode], K.ptr(out), ws.data_ptr(), ws.numel(),
           K.stream_ptr())
    return out


# (B, n, T, misaligned). A workgroup of the apply launch takes 1,024 four-element groups (16-byte map) or 1,024 elements (scalar map) of a
# row: 16-byte map, 64 groups = less than a workgroup; 2,400 groups = two full passes and a ragged third; scalar map, shorter than a
# workgroup; scalar map, 4,500 elements = four passes and a ragged fifth; one element, one pair; one step; za, zb and out each one float off
# a 16-byte boundary (a result check: nothing here observes which map ran), short and with 4,800 elements (past one pass)
CASES = [(3, 256, 5, False), (2, 9600, 4, False), (2, 15, 3, False), (2, 4500, 3, False), (1, 1, 2, False), (1, 4, 1, False),
         (3, 128, 3, True), (2, 4800, 3, True)]


def _t_vectors(T):
    first = torch.tensor([0.5]) if T == 1 else torch.linspace(0.0, 1.0, T)   # (the one-step case is a single t = 0.5)
    return [('linspace', first), ('extrapolated', torch.tensor([-0.5, 0.25, 1.5])), ('0 and 1 inside', torch.tensor([0.3, 0.0, 1.0, 0.7]))]


@pytest.mark.parametrize('case', CASES, ids=lambda c: '%dx%dx%d%s' % (c[0], c[1], c[2], '-misaligned' if c[3] else ''))
def test_latent_interp_kernel_cases(K, case):
    B, n, T, misaligned = case
    g = torch.Generator().manual_seed(300 + n + T)
    a, c = torch.randn(B, n, generator=g), torch.randn(B, n, generator=g) * 1.5 + 0.25
    jobs = []
    for mode in MODES:
        for name, t in _t_vectors(T):
            r64, r32 = interp_ref(a, c, t, mode)
            assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(r32).all()), 'a reference value is not finite'
            jobs.append(('latent_interp %dx%d%s %s t %s' % (B, n, ' misaligned' if misaligned else '', mode, name), mode, t, r64, r32))
    for tag, mode, t, r64, r32 in jobs:   # every reference exists before the first tensor goes to the device
        out = _run(K, a, c, t, mode, misaligned)
        assert tuple(out.shape) == (t.shape[0] * B, n)
        close_elem(tag, out, r64, r32)
        for j, tj in enumerate(t.tolist()):
            if tj in (0.0, 1.0):
                assert torch.equal(out[j * B:(j + 1) * B].cpu(), a if tj == 0.0 else c), tag + ': an endpoint is not bit-exact'


def _edge_pairs(n):
    g = torch.Generator().manual_seed(41 + n)
    a = torch.randn(2, n, generator=g)
    u, v = a[:, :n // 2], a[:, n // 2:2 * (n // 2)]
    quarter = torch.cat((-v, u) + ((torch.zeros(2, 1),) if n % 2 else ()), 1)   # orthogonal to a (n even) and of its norm
    a_orth = torch.cat((u, v) + ((torch.zeros(2, 1),) if n % 2 else ()), 1)
    rolled = torch.roll(a, 1, 1)                                                # some angle, exactly the norm of a
    return [('c == a', a, a.clone(), True), ('c == -a', a, -a, False),
            ('a == 0 / c == 0', torch.stack((torch.zeros(n), a[1])), torch.stack((a[0], torch.zeros(n))), False),
            ('nearly parallel', a, a + 1e-3 * torch.randn(2, n, generator=g), False),
            ('orthogonal', a_orth, quarter, True),
            ('scaled by 1e19', a * 1e19, rolled * 1e19, True), ('scaled by 1e-30', a * 1e-30, rolled * 1e-30, True)]


@pytest.mark.parametrize('n', [300, 15], ids=['float4', 'scalar'])
def test_latent_interp_slerp_value_edges(K, n):
    """Zero, parallel and antipodal pairs take the lerp coefficients; the nearly parallel pair matches the float64 slerp; sums of squares
    past float32's range and below it change nothing; where |a| == |c| every step in [0, 1] keeps that norm to 1e-5 relative."""
    t = torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0, -0.5, 1.5])
    inside = [j for j, tj in enumerate(t.tolist()) if 0.0 <= tj <= 1.0]
    jobs = []
    for name, a, c, same_norm in _edge_pairs(n):
        r64, r32 = interp_ref(a, c, t, 'slerp')
        assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(r32).all()), 'a reference value is not finite'
        jobs.append((name, a, c, same_norm, r64, r32))
    wa, wc = coefficients64(jobs[3][1], jobs[3][2], t, 'slerp')
    assert float((wa[1] - 0.75).abs().max()) > 0.0   # (the nearly parallel pair is not in the fallback: its coefficients are slerp's)
    for name, a, c, same_norm, r64, r32 in jobs:
        out = _run(K, a, c, t, 'slerp')
        close_elem('latent_interp slerp 2x%d %s' % (n, name), out, r64, r32)
        if same_norm:
            norms = out.double().cpu().view(t.shape[0], 2, n).pow(2).sum(2).sqrt()[inside]
            want = a.double().pow(2).sum(1).sqrt()[None].expand_as(norms)
            rel = float(((norms - want).abs() / want).max())
            print('norm      | slerp 2x%d %-20s | max relative deviation of |out_j| from |a| %.3e' % (n, name, rel))
            assert rel <= 1e-5, (name, rel)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the endpoints are branches
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [256, 15], ids=['float4', 'scalar'])
@pytest.mark.parametrize('mode', MODES)
def test_latent_interp_endpoints_are_bit_exact(K, mode, n):
    B = 3
    g = torch.Generator().manual_seed(9)
    a, c = torch.randn(B, n, generator=g), torch.randn(B, n, generator=g)
    t = torch.tensor([0.0, 0.5, 1.0])
    out = _run(K, a, c, t, mode).cpu()
    assert torch.equal(out[:B], a) and torch.equal(out[2 * B:], c)
    for wild in (INF, -INF, NAN):
        other = torch.full((B, n), wild)
        mixed = c.clone()
        mixed.view(-1)[0::3] = wild            # and a row that only holds some
        for o in (other, mixed):
            out = _run(K, a, o, t, mode).cpu()   # t = 0: a, whatever zb holds
            assert torch.equal(out[:B], a) and not bool(torch.isnan(out[:B]).any()), (mode, n, wild)
            out = _run(K, o, c, t, mode).cpu()   # t = 1: c, whatever za holds
            assert torch.equal(out[2 * B:], c) and not bool(torch.isnan(out[2 * B:]).any()), (mode, n, wild)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_latent_interp_refusals_leave_the_buffers_alone(K):
    from lvae_amd import _C
    lib = _C.load()
    B, n, T = 2, 8, 3
    za, zb, t = torch.randn(B, n).cuda(), torch.randn(B, n).cuda(), torch.linspace(0, 1, T).cuda()
    need = lib.lvae_latent_interp_workspace(B, T)
    out, ws = torch.full((T * B, n), 7.0).cuda(), torch.full((max(need, 4) // 4 + 4,), 7.0).cuda()
    P = lambda v: None if v is None else v.data_ptr()
    ok = dict(za=za, zb=zb, t=t, B=B, n=n, T=T, mode=1, out=out, ws=ws, ws_bytes=ws.numel() * 4)
    bad = [dict(za=None), dict(zb=None), dict(t=None), dict(out=None),
           dict(B=0), dict(n=0), dict(T=0), dict(B=-1), dict(n=-8), dict(T=-3),
           dict(mode=-1), dict(mode=2), dict(mode=7)]
    if need > 0:
        bad += [dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=None)]
    for change in bad:
        a = dict(ok, **change)
        rc = lib.lvae_latent_interp_f32(P(a['za']), P(a['zb']), P(a['t']), a['B'], a['n'], a['T'], a['mode'], P(a['out']), P(a['ws']),
                                        a['ws_bytes'], K.stream_ptr())
        assert rc != 0, change
        assert lib.lvae_last_error(), change
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 7.0).all())
    a = ok   # the legal call, on the same buffers
    assert lib.lvae_latent_interp_f32(P(a['za']), P(a['zb']), P(a['t']), B, n, T, 1, P(out), P(ws), a['ws_bytes'], K.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:B], za) and torch.equal(out[2 * B:], zb)
    with pytest.raises(_C.LvaeHipError):
        K.latent_interp(za.cpu(), zb.cpu(), t.cpu(), 'slerp')
    with pytest.raises(ValueError):
        K.latent_interp(za, zb[:, :4].contiguous(), t, 'slerp')
    with pytest.raises(ValueError):
        K.latent_interp(za, zb, t, 'cubic')


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. LadderVAE.interpolate against the CPU oracle, on one noise tape
# ---------------------------------------------------------------------------------------------------------------------------------
class SharedTape:
    """Round an oracle tape. A `normal` draw is handed out multiplied by `t`, the temperature of the layer that is drawing (1 everywhere
    else); while `share` = (B, T) it is one draw of B rows from the tape, repeated for the T steps."""

    def __init__(self, tape):
        self.tape, self.t, self.share = tape, 1.0, None

    def draw(self, kind, shape, **kw):
        if kind != 'normal':
            return self.tape.draw(kind, shape, **kw)
        if self.share is None:
            return self.tape.draw(kind, shape, **kw) * self.t
        B, T = self.share
        assert shape[0] == T * B
        return self.tape.draw(kind, (B,) + tuple(shape[1:]), **kw).repeat(T, 1, 1, 1) * self.t


def ref_interpolate(sd, cfg, x_a, x_b, k, T, mode, temps, tape, use_mode=True):
    """interpolate composed from the oracle's pieces (eval mode): bottom-up on the 2B rows, the top k layers in inference mode, the float64
    formula per layer, the forced layers in generative mode on T * B rows, the layers below from the prior at temps[i] with the B-row draw
    repeated T times (at 0 through use_mode=True: no draw), final_top_down, crop, likelihood without a target.
    Returns (likelihood info, [z], [z of the 2B rows or None])."""
    from oracle import lvae_ref as R
    L, B = len(cfg['z_dims']), x_a.shape[0]
    tt = SharedTape(tape)
    x = torch.cat((x_a, x_b))
    bu = R.bottomup_pass(sd, cfg, R.pad_img_tensor(x, R.get_padded_size(cfg, x.shape)), tt, False)
    out, z_ab = None, [None] * L
    for i in reversed(range(L - k, L)):
        out, _, aux = R.top_down_layer(sd, i, cfg, tt, False, out, out, True, bu[i], None, None, use_mode, False)
        z_ab[i] = aux['z']
    t = torch.linspace(0.0, 1.0, T)
    out, z = None, [None] * L
    for i in reversed(range(L)):
        if z_ab[i] is not None:
            a, c = z_ab[i][:B].reshape(B, -1), z_ab[i][B:].reshape(B, -1)
            wa, wc = coefficients64(a, c, t, mode)
            forced = (wa[:, :, None] * a[None] + wc[:, :, None] * c[None]).reshape((T * B,) + tuple(z_ab[i].shape[1:]))
            tt.t, tt.share = 1.0, None
            out, _, aux = R.top_down_layer(sd, i, cfg, tt, False, out, out, False, None, T * B, forced, False, False)
        else:
            tt.t, tt.share = (1.0 if temps[i] is None else float(temps[i])), (B, T)
            out, _, aux = R.top_down_layer(sd, i, cfg, tt, False, out, out, False, None, T * B, None, tt.t == 0.0, False)
        z[i] = aux['z']
    tt.t, tt.share = 1.0, None
    j0 = 0
    if not cfg['no_initial_downscaling']:
        out = F.interpolate(out, scale_factor=2, mode='bilinear', align_corners=False)
        j0 = 1
    for j in range(cfg['blocks_per_layer']):
        out = R.resampling_block(sd, 'final_top_down.%d' % (j0 + j), out, cfg, 'top-down', False, cfg['gated'], tt, False)
    out = R.crop_img_tensor(out, x_a.shape[2:])
    _, info = R.likelihood(sd, cfg, out, None, tt)
    return info, z, z_ab


def build(g, training=False):
    import lvae_amd  # noqa: F401
    from lvae_amd.models.lvae import LadderVAE
    torch.manual_seed(0)
    m = LadderVAE(**g.cfg)
    m.load_state_dict(g.state_dict(), strict=True)
    m.cuda()
    m.train(training)
    return m


def _oracle_temps(name):
    from test_conditional_gpu import ORACLE_TEMPS
    return ORACLE_TEMPS[name]


N_STEPS = 3
# (golden, k, mode, use_mode): every k of tiny_cifar, k in 1..2 of the other two, slerp at the posterior means; one lerp case, one sampled
ORACLE_CASES = ([('tiny_cifar', k, 'slerp', True) for k in (1, 2, 3)] + [(name, k, 'slerp', True) for name in ('tiny_eval', 'tiny_gauss') for k in (1, 2)]
                + [('tiny_cifar', 2, 'lerp', True), ('tiny_cifar', 2, 'slerp', False)])
_REF = {}


def _halves(x):
    B = x.shape[0] // 2
    assert B >= 1
    return x[:B], x[B:2 * B]


def _oracle_reference(name, k, mode, use_mode):
    """float64 oracle of one case, computed once: (info, z, z_ab, tape entries)"""
    from oracle import lvae_ref as R
    key = (name, k, mode, use_mode)
    if key not in _REF:
        g = load_golden(name)
        sd = {kk: (v.double() if v.is_floating_point() else v) for kk, v in g.state_dict().items()}
        tape = R.Tape(gen=torch.Generator().manual_seed(23 + k))
        x_a, x_b = _halves(g.t('x').double())
        with torch.no_grad():
            info, z, z_ab = ref_interpolate(sd, g.cfg, x_a, x_b, k, N_STEPS, mode, _oracle_temps(name), tape, use_mode)
        _REF[key] = (info, z, z_ab, tape.entries)
    return _REF[key]


def _compare_likelihood(tag, form, out, info, entries, tol):
    if form == 'bernoulli':
        mean_ref = info['mean']
        torch.testing.assert_close(out['mean'].cpu(), mean_ref.float(), **tol)
        torch.testing.assert_close(out['likelihood_params'].cpu(), mean_ref.float(), **tol)
        u = torch.as_tensor(entries[-1]).double()
        clear = (u - mean_ref).abs() > 2e-4
        inside = int((~clear).sum())
        print('bernoulli | %s | %d of %d pixels inside the 2e-4 margin' % (tag, inside, clear.numel()))
        assert inside <= 1e-3 * clear.numel()
        assert torch.equal(out['sample'].cpu()[clear], (u < mean_ref).float()[clear])
    elif form == 'gaussian':
        for key in ('mean', 'mode', 'sample'):
            torch.testing.assert_close(out[key].cpu(), info[key].float(), **tol)
        torch.testing.assert_close(out['likelihood_params']['mean'].cpu(), info['params']['mean'].float(), **tol)
        torch.testing.assert_close(out['likelihood_params']['logvar'].cpu(), info['params']['logvar'].float(), **tol)
    else:
        assert out['mean'] is None and out['mode'] is None
        torch.testing.assert_close(out['likelihood_params']['all_params'].cpu(), info['params']['all_params'].float(), **tol)
        torch.testing.assert_close(out['sample'].cpu(), info['sample'].float(), **tol)


@pytest.mark.parametrize('name,k,mode,use_mode', ORACLE_CASES, ids=lambda v: str(v))
def test_interpolate_matches_oracle(name, k, mode, use_mode):
    from lvae_amd.noise import TapeNoise
    info, z_ref, z_ab_ref, entries = _oracle_reference(name, k, mode, use_mode)
    g = load_golden(name)
    L, T = len(g.cfg['z_dims']), N_STEPS
    x_a, x_b = _halves(g.t('x'))
    B = x_a.shape[0]
    m = build(g)
    m.noise = TapeNoise(entries)
    with torch.no_grad():
        out = m.interpolate(x_a.cuda(), x_b.cuda(), n_steps=T, n_top_layers=k, mode=mode, use_mode=use_mode, temperature=_oracle_temps(name))
    assert m.noise.exhausted()
    assert not m.training
    assert torch.equal(out['t'].cpu(), torch.linspace(0.0, 1.0, T))
    for i in range(L):
        assert tuple(out['z'][i].shape) == tuple(z_ref[i].shape) and out['z'][i].shape[0] == T * B
        torch.testing.assert_close(out['z'][i].cpu(), z_ref[i].float(), rtol=1e-4, atol=1e-4)
        if i >= L - k:
            torch.testing.assert_close(out['z_a'][i].cpu(), z_ab_ref[i][:B].float(), rtol=1e-4, atol=1e-4)
            torch.testing.assert_close(out['z_b'][i].cpu(), z_ab_ref[i][B:].float(), rtol=1e-4, atol=1e-4)
        else:
            assert out['z_a'][i] is None and out['z_b'][i] is None
    assert out['sample'].shape[0] == T * B and tuple(out['sample'].shape[1:]) == tuple(x_a.shape[1:])
    _compare_likelihood('%s k=%d' % (name, k), g.cfg['likelihood_form'], out, info, entries, dict(rtol=1e-4, atol=2e-4))


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. identities on the device (PhiloxNoise: a fresh source of the same seed starts at the same step)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def cifar():
    g = load_golden('tiny_cifar')
    return build(g), g.t('x').cuda()


def _fresh(m, seed=5):
    from lvae_amd.noise import PhiloxNoise
    m.noise = PhiloxNoise(seed)
    return m


def _params(out):
    p = out['likelihood_params']
    return p['all_params'] if isinstance(p, dict) and 'all_params' in p else p


@pytest.mark.parametrize('k', [1, 3])
@pytest.mark.parametrize('mode', MODES)
def test_interpolate_ends_at_the_endpoints_latents(cifar, mode, k):
    m, x = cifar
    x_a, x_b = _halves(x)
    L, B, T = m.n_layers, x_a.shape[0], 4
    with torch.no_grad():
        out = _fresh(m).interpolate(x_a, x_b, n_steps=T, n_top_layers=k, mode=mode)
        enc_a = _fresh(m).encode(x_a, k)
    assert len(out['z']) == len(out['z_a']) == len(out['z_b']) == L and tuple(out['t'].shape) == (T,)
    for i in range(L):
        assert out['z'][i].shape[0] == T * B
        if i < L - k:
            assert out['z_a'][i] is None and out['z_b'][i] is None and enc_a[i] is None
            continue
        assert torch.equal(out['z'][i][:B], out['z_a'][i])
        assert torch.equal(out['z'][i][-B:], out['z_b'][i])
        # (eval mode: a row of the 2B-row pass is the row of a B-row pass, up to what the kernels' batch tiling rounds differently)
        torch.testing.assert_close(out['z_a'][i], enc_a[i], rtol=1e-4, atol=1e-4)
        mid = out['z'][i][B:2 * B]
        assert float((mid - out['z_a'][i]).abs().max()) > 1e-3 and float((mid - out['z_b'][i]).abs().max()) > 1e-3


def test_interpolate_between_an_image_and_itself_stands_still(cifar):
    m, x = cifar
    L, B, T = m.n_layers, x.shape[0], 4
    with torch.no_grad():
        out = _fresh(m).interpolate(x, x, n_steps=T)
    for i in range(L):
        rows = out['z'][i].reshape(T, B, -1)
        for j in range(1, T):
            torch.testing.assert_close(rows[j], rows[0], rtol=1e-6, atol=0.0)
    p = _params(out).reshape(T, B, -1)
    for j in range(1, T):   # the pictures' parameters follow, at the tolerances of the oracle comparison
        torch.testing.assert_close(p[j], p[0], rtol=1e-4, atol=2e-4)


def test_interpolate_ends_are_the_conditional_pictures_and_decode_inverts_encode(cifar):
    m, x = cifar
    x_a, x_b = _halves(x)
    L, B = m.n_layers, x_a.shape[0]
    tol = dict(rtol=1e-4, atol=2e-4)
    with torch.no_grad():
        ends = _fresh(m).interpolate(x_a, x_b, t=torch.tensor([0.0, 1.0], device='cuda'), use_mode=True)
        cond_a = _fresh(m).sample_conditional(x_a, L, 1, use_mode=True)
        cond_b = _fresh(m).sample_conditional(x_b, L, 1, use_mode=True)
        z = _fresh(m).encode(x_a)
        dec = _fresh(m).decode(z)
    assert all(v is not None and v.shape[0] == B for v in z) and len(z) == L
    torch.testing.assert_close(_params(ends)[:B], _params(cond_a), **tol)
    torch.testing.assert_close(_params(ends)[B:], _params(cond_b), **tol)
    torch.testing.assert_close(_params(dec), _params(cond_a), **tol)
    for i in range(L):
        torch.testing.assert_close(z[i], cond_a['z'][i], rtol=1e-4, atol=1e-4)
        assert torch.equal(dec['z'][i], z[i])   # a forced layer hands back what it was given
    assert set(dec) == set(cond_a) == {'sample', 'mean', 'mode', 'likelihood_params', 'z'}
    assert set(ends) == set(dec) | {'z_a', 'z_b', 't'}


def test_decode_of_nothing_is_sample_prior_and_partial_forcing_is_legal(cifar):
    m, x = cifar
    L = m.n_layers
    with torch.no_grad():
        a = _fresh(m).sample_prior(5).clone()
        b = _fresh(m).decode([None] * L, n_imgs=5)['sample'].clone()
        assert torch.equal(a, b)
        c = _fresh(m).sample_prior(5, temperature=0.5).clone()
        d = _fresh(m).decode([None] * L, n_imgs=5, temperature=0.5)['sample'].clone()
        assert torch.equal(c, d) and not torch.equal(a, c)
        z = _fresh(m).encode(x, 2)
        assert z[0] is None and z[1] is not None and z[2] is not None
        top = _fresh(m).decode(z, temperature=0.0)                      # the bottom layer at its prior mean
        low = _fresh(m).decode([z[0], z[1], None], temperature=0.0)     # a forced layer below a sampled one
    assert top['z'][0].shape[0] == x.shape[0] and torch.equal(top['z'][1], z[1]) and torch.equal(top['z'][2], z[2])
    assert torch.equal(low['z'][1], z[1]) and low['z'][2].shape[0] == x.shape[0]
    assert bool(torch.isfinite(_params(top)).all()) and bool(torch.isfinite(_params(low)).all())


def test_interpolate_shares_one_prior_draw_per_pair(cifar):
    """k = 2: the bottom layer draws (B, h, w, Z) once. At t = [0.5, 0.5, 0.5] the three steps of a pair are one picture's latents."""
    m, x = cifar
    x_a, x_b = _halves(x)
    B = x_a.shape[0]
    with torch.no_grad():
        out = _fresh(m).interpolate(x_a, x_b, n_top_layers=2, t=torch.full((3,), 0.5, device='cuda'))
    rows = out['z'][0].reshape(3, B, -1)
    assert torch.equal(rows[0], rows[1]) and torch.equal(rows[0], rows[2])
    if B > 1:
        assert float((rows[0][0] - rows[0][1]).abs().max()) > 1e-3   # pairs differ


def test_interpolate_bf16(cifar):
    m, x = cifar
    x_a, x_b = _halves(x)
    B, T = x_a.shape[0], 3
    m.compute_dtype = 'bf16'
    try:
        with torch.no_grad():
            out = _fresh(m).interpolate(x_a, x_b, n_steps=T)
        pics = out['mean'] if out['mean'] is not None else out['sample']
        assert tuple(pics.shape) == (T * B,) + tuple(x_a.shape[1:]) and bool(torch.isfinite(pics).all())
        for i in range(m.n_layers):
            assert torch.equal(out['z'][i][:B], out['z_a'][i]) and torch.equal(out['z'][i][-B:], out['z_b'][i])
    finally:
        m.compute_dtype = 'f32'


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. ValueErrors
# ---------------------------------------------------------------------------------------------------------------------------------
def test_guards(cifar):
    m, x = cifar
    x_a, x_b = _halves(x)
    L = m.n_layers
    with torch.no_grad():
        for k in (0, -1, L + 1):
            with pytest.raises(ValueError):
                m.encode(x, k)
            with pytest.raises(ValueError):
                m.interpolate(x_a, x_b, n_top_layers=k)
        with pytest.raises(ValueError):
            m.interpolate(x_a, x_b[:, :, :16])
        with pytest.raises(ValueError):
            m.interpolate(x_a, x[:x_a.shape[0] + 1])
        for n in (0, -2):
            with pytest.raises(ValueError):
                m.interpolate(x_a, x_b, n_steps=n)
        with pytest.raises(ValueError):
            m.interpolate(x_a, x_b, mode='cubic')
        with pytest.raises(ValueError):
            m.interpolate(x_a, x_b, temperature=[0.5, 0.5])
        z = _fresh(m).encode(x)
        with pytest.raises(ValueError):
            m.decode([None] * L)                       # nothing forced and no n_imgs
        with pytest.raises(ValueError):
            m.decode(z, n_imgs=x.shape[0] + 1)         # contradicts the forced tensors
        with pytest.raises(ValueError):
            m.decode(z[:2])                            # one entry per layer
        with pytest.raises(ValueError):
            m.decode([z[0], z[1][:1], z[2]])           # rows disagree
        with pytest.raises(ValueError):
            m.decode(z, temperature=-1.0)
        out = _fresh(m).interpolate(x_a, x_b, n_steps=1)   # legal: one step, t = 0
        assert out['z'][L - 1].shape[0] == x_a.shape[0] and torch.equal(out['z'][L - 1], out['z_a'][L - 1])


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the evaluation CLI
# ---------------------------------------------------------------------------------------------------------------------------------
def test_interp_cli(tmp_path, monkeypatch):
    import lvae_amd  # noqa: F401
    from lvae_amd import evaluate as leval
    from lvae_amd.images import grid_shape
    from test_images_cpu import decode_png
    monkeypatch.chdir(tmp_path)
    img_dir = str(tmp_path / 'pics')
    argv = ['-d', 'cifar10', '--zdims', '8', '8', '--downsample', '1', '1', '--nfilters', '16', '--skip', '--gated',
            '--freebits', '1.0', '--batch-size', '8', '--synthetic', '--seed', '3', '--n-test', '16']
    leval.main(argv + ['--interp', '--interp-steps', '3', '--img-dir', img_dir])
    L, T = 2, 3
    pairs = min(leval.IMG_GRID_N, 16 // 2)
    data = torch.floor(256 * torch.rand((16, 3, 32, 32), generator=torch.Generator().manual_seed(3))) / 255   # main.synthetic_batch
    a = np.load(str(tmp_path / ('interp_top%d.npy' % L)))
    assert a.shape == (pairs, T + 2, 3, 32, 32)
    assert np.array_equal(a[:, 0], data[0:2 * pairs:2].numpy()) and np.array_equal(a[:, -1], data[1:2 * pairs:2].numpy())
    assert np.isfinite(a).all() and a.min() >= 0.0 and a.max() <= 1.0
    assert np.abs(a[:, 1] - a[:, 3]).max() > 1e-3    # a path, not one picture three times
    assert not os.path.exists(str(tmp_path / 'interp_top1.npy'))   # the default is k = L only
    png = decode_png(open(os.path.join(img_dir, 'interp_top%d.png' % L), 'rb').read())
    assert png.shape == tuple(grid_shape(pairs * (T + 2), T + 2, 32, 32)) + (3,)
