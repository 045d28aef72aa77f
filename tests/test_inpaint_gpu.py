"""Masked likelihoods and inpainting on the device: the four masked heads and the select kernel against float64, their exact properties
(all observed = the unmasked entry point bit for bit; nothing observed; poison under the mask; aliasing; refusals), LadderVAE.forward(x, mask)
and LadderVAE.inpaint against the CPU oracle on one noise tape, their identities on the device, their ValueErrors, and the evaluation CLI.

Kernels: the two rules of docs/ELEMENTWISE_PARITY.md, unchanged (close_elem / close_sum of tests/test_elementwise_gpu.py). r64 is the
reference of tests/test_inpaint_cpu.py in float64 (the oracle's own likelihood functions on single pixels, times the mask, summed; gradients by
autograd), r32 the same in float32. Models: the tolerances tests/test_interpolate_gpu.py uses for these goldens (rtol 1e-4, atol 2e-4, and its
Bernoulli rule), parameter gradients at the relative L2 of tests/test_model_gpu.py (1e-4). A thresholded draw (the Bernoulli u < mean, the
mixture's Gumbel arg-max) within 2e-4 of its threshold is left out, at most 1e-3 of the pixels; the counts are printed.
Every comparison prints its figures before it asserts (run with -s); every reference exists before the first tensor goes to the device."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_elementwise_gpu import close_elem, close_sum, finite
from test_inpaint_cpu import (CAP, MARGIN, double_sd, forward_reference, golden_mask, head_inputs, head_reference, inpaint_reference,
                              ref_forward_masked, unsure_pixels)

pytestmark = pytest.mark.gpu

NAN, INF = float('nan'), float('inf')
TOL = dict(rtol=1e-4, atol=2e-4)   # tests/test_interpolate_gpu.py, for the same goldens


@pytest.fixture(scope='module')
def K():
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels
    return kernels


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def nchw(t):
    return None if t is None else t.permute(0, 3, 1, 2).cpu()


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the masked heads against float64
# ---------------------------------------------------------------------------------------------------------------------------------
# (form, N, HW, C, nmix). Per-image kernels (one workgroup of 256 threads per image, elements of a pixel consecutive): one element; one pixel
# of three colours; 258 elements = just past one sweep, with pixel 85 split across the sweep boundary (elements 255 | 256, 257); 300
# one-colour pixels. The mixture (128 pixels per workgroup, 64 for 20 components): 130 pixels = a tail of 2 and a workgroup that straddles the
# two images; one pixel.
HEAD_CASES = ([(f, N, HW, C, 0) for f in ('bernoulli', 'gaussian', 'discr_log') for (N, HW, C) in ((1, 1, 1), (3, 1, 3), (2, 86, 3), (2, 300, 1))]
              + [('discr_log_mix', 2, 65, 3, nmix) for nmix in (10, 20, 1)] + [('discr_log_mix', 1, 1, 3, 10)])
CASE_ID = lambda c: '%s-%dx%dx%d%s' % (c[0], c[1], c[2], c[3], '-nmix%d' % c[4] if c[4] else '')


def masks_for(N, HW, seed):
    """[(name, (N, HW, 1) uint8)]: non-zero = observed"""
    g = torch.Generator().manual_seed(seed)
    one_obs = torch.zeros(N, HW, 1, dtype=torch.uint8)
    one_obs[N - 1, HW // 2] = 1
    one_miss = torch.ones(N, HW, 1, dtype=torch.uint8)
    one_miss[0, HW - 1] = 0
    rnd = (torch.rand(N, HW, 1, generator=g) < 0.5).to(torch.uint8)
    vals = rnd * torch.where(torch.rand(N, HW, 1, generator=g) < 0.5, 2, 255).to(torch.uint8)
    return [('all', torch.ones(N, HW, 1, dtype=torch.uint8)), ('none', torch.zeros(N, HW, 1, dtype=torch.uint8)), ('one observed', one_obs),
            ('one missing', one_miss), ('random', rnd), ('values 2 and 255', vals)]


def device_inputs(form, raw, x, entries):
    """the head's arguments on the device, NHWC: (params, x, [noise tensors])"""
    if form == 'discr_log_mix':
        noise = [torch.as_tensor(e).float().contiguous().cuda() for e in entries]      # channel-last already
    else:
        noise = [nhwc(torch.as_tensor(entries[0]).float())]
    return nhwc(raw), nhwc(x), noise


def run_head(K, form, p, x, noise, mask=None, filled=None):
    """one head on the device -> dict(ll, dll, mean, mode, sample, filled), everything the entry point writes"""
    masked = mask is not None
    if form == 'bernoulli':
        r = K.bernoulli_masked_fwd(p, x, noise[0], mask, True, filled) if masked else K.bernoulli_fwd(p, x, noise[0], True) + (None,)
        mean, mode, sample, ll, dll, fl = r
        return dict(ll=ll, dll=dll, mean=mean, mode=mode, sample=sample, filled=fl)
    if form == 'gaussian':
        r = K.gaussian_masked_fwd(p, x, noise[0], mask, True, filled) if masked else K.gaussian_fwd(p, x, noise[0], True) + (None,)
        sample, ll, dll, fl = r
        return dict(ll=ll, dll=dll, mean=None, mode=None, sample=sample, filled=fl)
    if form == 'discr_log':
        r = K.discr_logistic_masked_fwd(p, x, noise[0], mask, True, filled) if masked else K.discr_logistic_fwd(p, x, noise[0], True) + (None,)
        mean, ls, sample, ll, dll, fl = r
        return dict(ll=ll, dll=dll, mean=mean, mode=ls, sample=sample, filled=fl)
    sample = K.dmol_sample(p, noise[0], noise[1])
    ll, dll, fl = K.dmol_ll_masked_fwd(p, x, mask, sample, True, filled) if masked else K.dmol_ll_fwd(p, x, True) + (None,)
    return dict(ll=ll, dll=dll, mean=None, mode=None, sample=sample, filled=fl)


def same_bits(a, b):
    """bit-identical, NaN included"""
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _case(form, N, HW, C, nmix):
    from oracle import lvae_ref as R
    raw, x = head_inputs(form, N, HW, C, nmix or 10, 500 + 7 * HW + C + nmix)
    tape = R.Tape(gen=torch.Generator().manual_seed(17 + HW))
    head_reference(form, raw, x, torch.ones(N, HW, 1, dtype=torch.bool), tape, torch.float64)   # records the head's draws
    return raw, x, tape.entries


@pytest.mark.parametrize('case', HEAD_CASES, ids=CASE_ID)
def test_masked_heads_match_float64(K, case):
    from oracle import lvae_ref as R
    form, N, HW, C, nmix = case
    raw, x, entries = _case(*case)
    jobs = []
    for name, m8 in masks_for(N, HW, 3 + HW):
        mb = m8 != 0
        r64 = head_reference(form, raw, x, mb, R.Tape(entries=entries), torch.float64)
        r32 = head_reference(form, raw, x, mb, R.Tape(entries=entries), torch.float32)
        finite(r64['ll'], r64['dll'], r64['filled'], r32['ll'], r32['dll'], r32['filled'])
        unsure = unsure_pixels(form, r64['dec'], entries) | unsure_pixels(form, r32['dec'], entries)
        assert int(unsure.sum()) <= max(1, 0.01 * unsure.numel())
        jobs.append((name, m8, mb, r64, r32, unsure))
    p, xd, noise = device_inputs(form, raw, x, entries)
    plain = run_head(K, form, p, xd, noise)
    for name, m8, mb, r64, r32, unsure in jobs:
        tag = '%s %s' % (CASE_ID(case), name)
        out = run_head(K, form, p, xd, noise, m8.cuda())
        torch.cuda.synchronize()
        close_sum(tag + ' ll', out['ll'], r64['ll'], r32['ll'], r64['ll_abs'])
        close_elem(tag + ' dll', nchw(out['dll']), r64['dll'], r32['dll'])
        if out['mean'] is not None:     # (the Gaussian head's mean is a view of its parameters: the entry point writes none)
            close_elem(tag + ' mean', nchw(out['mean']), r64['mean'], r32['mean'])
        sure = (~unsure)[:, None].expand_as(r64['filled'])
        close_elem(tag + ' filled', nchw(out['filled'])[sure], r64['filled'][sure], r32['filled'][sure])
        # exact properties: the pictures are the unmasked call's; filled is a select of x and the draw; no gradient under the mask
        for key in ('mean', 'mode', 'sample'):
            assert same_bits(out[key], plain[key]), (tag, key)
        obs = mb[..., None].expand_as(x.permute(0, 2, 3, 1)).cuda()
        assert torch.equal(out['filled'], torch.where(obs, xd, out['sample'])), tag
        hidden = (~mb)[..., None].expand_as(out['dll'].cpu())
        at_hidden = out['dll'].cpu()[hidden]
        assert bool((at_hidden == 0).all()) and not bool(torch.signbit(at_hidden).any()), tag
        if name == 'all':
            assert same_bits(out['ll'], plain['ll']) and same_bits(out['dll'], plain['dll']) and torch.equal(out['filled'], xd), tag
        if name == 'none':
            assert bool((out['ll'] == 0).all()) and not bool(torch.signbit(out['ll']).any()), tag
            assert torch.equal(out['filled'], out['sample']), tag
        if name == 'values 2 and 255':   # any non-zero byte is "observed": the bits of the 0 / 1 mask
            ones = run_head(K, form, p, xd, noise, (m8 != 0).to(torch.uint8).cuda())
            assert all(same_bits(out[k], ones[k]) for k in out), tag


@pytest.mark.parametrize('case', [c for c in HEAD_CASES if c[2] > 1], ids=CASE_ID)
def test_masked_ll_is_additive(K, case):
    form, N, HW, C, nmix = case
    from oracle import lvae_ref as R
    raw, x, entries = _case(*case)
    every = torch.ones(N, HW, 1, dtype=torch.bool)
    r64 = head_reference(form, raw, x, every, R.Tape(entries=entries), torch.float64)
    r32 = head_reference(form, raw, x, every, R.Tape(entries=entries), torch.float32)
    finite(r64['ll'], r32['ll'])
    m8 = masks_for(N, HW, 3 + HW)[4][1]
    p, xd, noise = device_inputs(form, raw, x, entries)
    a = run_head(K, form, p, xd, noise, m8.cuda())['ll'].double().cpu()
    b = run_head(K, form, p, xd, noise, (1 - m8).cuda())['ll'].double().cpu()
    close_sum('%s ll(mask) + ll(~mask)' % CASE_ID(case), a + b, r64['ll'], r32['ll'], r64['ll_abs'])


POISON_CASES = [('bernoulli', 2, 86, 3, 0), ('gaussian', 2, 86, 3, 0), ('discr_log', 2, 86, 3, 0), ('discr_log_mix', 2, 65, 3, 10),
                ('discr_log_mix', 2, 65, 3, 20)]


@pytest.mark.parametrize('case', POISON_CASES, ids=CASE_ID)
def test_poison_under_the_mask_changes_nothing_and_filled_may_be_x(K, case):
    form, N, HW, C, nmix = case
    raw, x, entries = _case(*case)
    m8 = masks_for(N, HW, 3 + HW)[4][1]
    assert 0 < int(m8.sum()) < m8.numel()
    p, xd, noise = device_inputs(form, raw, x, entries)
    md = m8.cuda()
    good = run_head(K, form, p, xd, noise, md)
    hidden_x = (md == 0)[..., None].expand_as(xd)
    hidden_p = (md == 0)[..., None].expand_as(p)
    obs_x = ~hidden_x
    out = run_head(K, form, p, torch.where(hidden_x, torch.full_like(xd, NAN), xd), noise, md)          # x is not read under the mask
    assert all(same_bits(out[k], good[k]) for k in out), CASE_ID(case)
    for wild in (NAN, INF, -INF):
        out = run_head(K, form, torch.where(hidden_p, torch.full_like(p, wild), p), xd, noise, md)
        assert same_bits(out['ll'], good['ll']) and same_bits(out['dll'], good['dll']), (CASE_ID(case), wild)
        assert bool((out['dll'][hidden_p] == 0).all()) and bool(torch.isfinite(out['ll']).all())
        assert torch.equal(out['filled'][obs_x], xd[obs_x])
    # filled aliasing x: the bits of the call with a buffer of its own
    x2 = xd.clone()
    out = run_head(K, form, p, x2, noise, md, filled=x2)
    assert out['filled'].data_ptr() == x2.data_ptr()
    assert all(same_bits(out[k], good[k]) for k in out), CASE_ID(case)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the select kernel
# ---------------------------------------------------------------------------------------------------------------------------------
def _off_by_one_float(t):
    """a contiguous device copy of t that starts 4 bytes past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, device='cuda')
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


# (N, C, H, W): 35 pixels (no 16-byte map in either layout for C = 1; channel-last C = 3 neither), 32 pixels (both maps), 1,296 pixels (more
# than one workgroup), one pixel
@pytest.mark.parametrize('shape', [(2, 1, 5, 7), (2, 3, 5, 7), (2, 1, 4, 8), (2, 3, 4, 8), (2, 3, 36, 36), (1, 1, 1, 1), (1, 3, 1, 1)], ids=str)
@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
def test_mask_select_is_torch_where(K, layout, shape):
    N, C, H, W = shape
    is_nchw = layout == 'nchw'
    g = torch.Generator().manual_seed(N + C + H * W)
    full = (N, C, H, W) if is_nchw else (N, H, W, C)
    a, b = torch.randn(full, generator=g), torch.randn(full, generator=g)
    m8 = (torch.rand(N, H, W, generator=g) < 0.5).to(torch.uint8) * 200
    mb = (m8 != 0)[:, None] if is_nchw else (m8 != 0)[..., None]
    mb = mb.expand(full)
    a = torch.where(mb, a, torch.full_like(a, NAN))    # the value not taken is never looked at
    b = torch.where(mb, torch.full_like(b, NAN), b)
    want_t, want_s = torch.where(mb, a, b), torch.where(mb, a, torch.full_like(a, 0.375))
    assert bool(torch.isfinite(want_t).all())
    md = m8.cuda()
    for mis in (False, True):
        put = _off_by_one_float if mis else (lambda t: t.cuda())
        ad, bd = put(a), put(b)
        out = K.mask_select(ad, bd, md, is_nchw, out=put(torch.zeros(full)))
        assert torch.equal(out.cpu(), want_t), (layout, shape, mis)
        assert torch.equal(K.mask_select(ad, 0.375, md, is_nchw).cpu(), want_s), (layout, shape, mis)
        a2 = put(a)
        assert K.mask_select(a2, bd, md, is_nchw, out=a2) is a2 and torch.equal(a2.cpu(), want_t)      # out aliases a
        b2 = put(b)
        assert K.mask_select(ad, b2, md, is_nchw, out=b2) is b2 and torch.equal(b2.cpu(), want_t)      # out aliases b
        a3 = put(a)
        K.mask_select(a3, 0.375, md, is_nchw, out=a3)
        assert torch.equal(a3.cpu(), want_s)
    every, nothing = torch.ones_like(md), torch.zeros_like(md)
    assert same_bits(K.mask_select(a.cuda(), b.cuda(), every, is_nchw), a.cuda())
    assert same_bits(K.mask_select(a.cuda(), b.cuda(), nothing, is_nchw), b.cuda())


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_buffers_alone(K):
    from lvae_amd import _C
    lib = _C.load()
    N, HW, C, nmix = 2, 5, 3, 10
    P = HW * C
    S = 7.0
    dv = lambda *shape: torch.rand(*shape).cuda()
    sent = lambda *shape: torch.full(shape, S).cuda()
    mask = torch.ones(N, HW, dtype=torch.uint8).cuda()
    st = K.stream_ptr()
    need = lib.lvae_dmol_workspace(N, HW)
    outs = {}

    def entry(name, fn, ok, bad, written):
        outs[name] = written
        for idx, value in bad:
            args = list(ok)
            args[idx] = value
            rc = fn(*[v.data_ptr() if torch.is_tensor(v) else v for v in args])
            assert rc != 0 and lib.lvae_last_error(), (name, idx, value)
            if name == 'dmol' and idx == 8:
                assert rc == -3, (name, rc)       # LVAE_EWORKSPACE
            elif not (name == 'dmol' and idx == 7):
                assert rc == -1, (name, idx, rc)  # LVAE_EINVAL
        torch.cuda.synchronize()
        for t in written:
            assert bool((t == S).all()), name
        assert fn(*[v.data_ptr() if torch.is_tensor(v) else v for v in ok]) == 0, name     # the legal call, on the same buffers
        torch.cuda.synchronize()
        for t in written:
            assert not bool((t == S).all()), name

    mean, mode, sample, ll, dll, filled = sent(N, P), sent(N, P), sent(N, P), sent(N), sent(N, P), sent(N, P)
    entry('bernoulli', lib.lvae_bernoulli_masked_fwd_f32,
          [dv(N, P), dv(N, P), dv(N, P), N, P, C, mean, mode, sample, ll, dll, mask, filled, st],
          [(0, None), (1, None), (2, None), (9, None), (11, None), (3, 0), (3, -1), (4, 0), (5, 0), (5, 2), (5, -3)],
          [mean, mode, sample, ll, dll, filled])
    sample, ll, dll, filled = sent(N, P), sent(N), sent(N, 2 * P), sent(N, P)
    entry('gaussian', lib.lvae_gaussian_masked_fwd_f32,
          [dv(N, 2 * P), dv(N, P), dv(N, P), N, HW, C, sample, ll, dll, mask, filled, st],
          [(0, None), (1, None), (2, None), (7, None), (9, None), (3, 0), (4, 0), (5, 0), (4, -5)],
          [sample, ll, dll, filled])
    mean, ls, sample, ll, dll, filled = sent(N, P), sent(N, P), sent(N, P), sent(N), sent(N, 2 * P), sent(N, P)
    entry('discr_logistic', lib.lvae_discr_logistic_masked_fwd_f32,
          [dv(N, 2 * P), dv(N, P), dv(N, P).clamp(1e-7, 1 - 1e-7), N, HW, C, mean, ls, sample, ll, dll, mask, filled, st],
          [(0, None), (1, None), (2, None), (9, None), (11, None), (3, 0), (4, 0), (5, 0)],
          [mean, ls, sample, ll, dll, filled])
    ll, dll, ws, filled = sent(N), sent(N, HW * 10 * nmix), sent(need // 4 + 4), sent(N, HW * 3)
    entry('dmol', lib.lvae_dmol_ll_masked_fwd_f32,
          [torch.randn(N, HW * 10 * nmix).cuda(), dv(N, HW * 3), N, HW, nmix, ll, dll, ws, ws.numel() * 4, mask, dv(N, HW * 3), filled, st],
          [(0, None), (1, None), (5, None), (7, None), (9, None), (10, None), (2, 0), (3, 0), (4, 0), (4, 7), (4, 11), (8, need - 1), (8, 0)],
          [ll, dll, ws, filled])
    out = sent(N, C, HW)
    entry('select', lib.lvae_mask_select_f32, [dv(N, C, HW), dv(N, C, HW), 0.0, mask, N, C, HW, 1, out, st],
          [(0, None), (3, None), (8, None), (4, 0), (5, 0), (6, 0), (4, -2), (6, -5)], [out])
    # the Python layer: a mask without its image, a mask of the wrong kind, host tensors
    from lvae_amd.lib.likelihoods import GaussianLikelihood
    with pytest.raises(ValueError):
        K.gaussian_masked_fwd(dv(N, HW, 1, 2 * C), None, dv(N, HW, 1, C), mask.view(N, HW, 1), True)
    with pytest.raises(ValueError):
        K.gaussian_masked_fwd(dv(N, HW, 1, 2 * C), dv(N, HW, 1, C), dv(N, HW, 1, C), mask.view(N, HW, 1).float(), True)
    with pytest.raises(ValueError):
        K.mask_select(dv(N, C, HW, 1), 0.0, mask.view(N, HW, 1)[:1], True)
    with pytest.raises(_C.LvaeHipError):
        K.mask_select(torch.zeros(N, C, HW, 1), 0.0, mask.view(N, HW, 1), True)
    head = GaussianLikelihood(8, C).cuda()
    with pytest.raises(ValueError):
        head(dv(N, 4, 4, 8), None, None, mask=torch.ones(N, 4, 4, dtype=torch.uint8).cuda())


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the model against the oracle, on one noise tape
# ---------------------------------------------------------------------------------------------------------------------------------
GOLDENS = ('tiny_mnist', 'tiny_cifar', 'tiny_gauss', 'tiny_discrlog')


def build(g, training=False):
    import lvae_amd  # noqa: F401
    from lvae_amd.models.lvae import LadderVAE
    torch.manual_seed(0)
    m = LadderVAE(**g.cfg)
    m.load_state_dict(g.state_dict(), strict=True)
    m.cuda()
    m.train(training)
    return m


def compare_pictures(tag, form, got, want, unsure, what):
    """a completed / filled picture (B, C, H, W) against the oracle's, the unsure pixels left out; prints their count"""
    n = int(unsure.sum())
    print('thresholded | %s %s | %d of %d pixels inside the %g margin' % (tag, what, n, unsure.numel(), MARGIN))
    assert n <= CAP * unsure.numel(), (tag, n)
    sure = (~unsure)[:, None].expand_as(want)
    got, want = got.cpu()[sure], want.float()[sure]
    if form == 'bernoulli':
        assert torch.equal(got, want), '%s %s: %d pixels differ' % (tag, what, int((got != want).sum()))
    else:
        torch.testing.assert_close(got, want, **TOL)


def compare_params(form, out_params, out_mean, dec):
    if form == 'bernoulli':
        torch.testing.assert_close(out_mean.cpu(), dec['mean'].float(), **TOL)
        torch.testing.assert_close(out_params.cpu(), dec['mean'].float(), **TOL)
    elif form == 'discr_log_mix':
        assert out_mean is None
        torch.testing.assert_close(out_params['all_params'].cpu(), dec['all_params'].float(), **TOL)
    else:
        torch.testing.assert_close(out_mean.cpu(), dec['mean'].float(), **TOL)
        for k, v in dec.items():
            torch.testing.assert_close(out_params[k].cpu(), v.float(), **TOL)


@pytest.mark.parametrize('name', GOLDENS)
def test_masked_forward_matches_oracle(name):
    from lvae_amd.noise import TapeNoise
    ref = forward_reference(name)
    g = load_golden(name)
    form = g.cfg['likelihood_form']
    unsure = unsure_pixels(form, ref['dec'], ref['entries'])
    m = build(g)
    m.noise = TapeNoise(ref['entries'])
    x = g.t('x').cuda()
    with torch.no_grad():
        out = m(x, mask=ref['mask'].cuda(), mask_fill=0.25)
    assert m.noise.exhausted() and len(out) == 13
    mo = ref['mo']
    print('masked ll   | %s | engine %s | oracle %s' % (name, out['ll'].cpu().tolist(), ref['ll'].tolist()))
    torch.testing.assert_close(out['ll'].cpu(), ref['ll'].float(), **TOL)
    torch.testing.assert_close(out['kl_sep'].cpu(), mo['kl_sep'].float(), **TOL)
    for i, z in enumerate(out['z']):
        torch.testing.assert_close(z.cpu(), mo['z'][i].float(), **TOL)
    compare_params(form, out['likelihood_params'], out['out_mean'], ref['dec'])
    compare_pictures(name, form, out['out_sample'], mo['out_sample'], unsure, 'out_sample')
    compare_pictures(name, form, out['out_filled'], ref['filled'], unsure, 'out_filled')
    obs = ref['mask'][:, None].expand_as(x).cuda()
    assert torch.equal(out['out_filled'][obs], x[obs])
    # (B, 1, H, W) and uint8 are the same mask; a tensor fill of 0.25 is the scalar's
    m.noise = TapeNoise(ref['entries'])
    with torch.no_grad():
        again = m(x, mask=(ref['mask'][:, None].to(torch.uint8) * 3).cuda(), mask_fill=torch.full_like(x, 0.25))
    assert same_bits(again['ll'], out['ll']) and same_bits(again['out_filled'], out['out_filled']) and same_bits(again['kl_sep'], out['kl_sep'])


@pytest.mark.parametrize('name', GOLDENS)
def test_inpaint_two_rounds_match_oracle(name):
    from oracle import lvae_ref as R
    from lvae_amd.noise import TapeNoise
    ref = inpaint_reference(name)
    g = load_golden(name)
    form = g.cfg['likelihood_form']
    mask, x = ref['mask'], g.t('x')
    m = build(g, training=True)       # inpaint() itself goes to eval mode, and back
    m.noise = TapeNoise(ref['tapes'][0] + ref['tapes'][1])
    out = m.inpaint(x.cuda(), mask.cuda(), n_iters=2, init='zeros', return_history=True)
    assert m.noise.exhausted() and m.training
    assert tuple(out['ll_observed'].shape) == (2, x.shape[0]) and tuple(out['history'].shape) == (3,) + tuple(x.shape)
    obs = mask[:, None].expand_as(x)
    assert torch.equal(out['history'][0].cpu(), torch.where(obs, x, torch.zeros_like(x)))
    # round 1 against the oracle's round 1
    ll1, filled1, dec1 = ref['rounds'][0]
    print('ll_observed | %s round 1 | engine %s | oracle %s' % (name, out['ll_observed'][0].cpu().tolist(), ll1.tolist()))
    torch.testing.assert_close(out['ll_observed'][0].cpu(), ll1.float(), **TOL)
    compare_pictures(name, form, out['history'][1], filled1, unsure_pixels(form, dec1, ref['tapes'][0]), 'round 1')
    # round 2: the oracle starts from the engine's own round-1 completion, so that a kernel's error does not compound
    with torch.no_grad():
        start = out['history'][1].cpu().double()
        _, ll2, filled2, dec2 = ref_forward_masked(double_sd(g), g.cfg, start, mask, start, R.Tape(entries=ref['tapes'][1]))
    print('ll_observed | %s round 2 | engine %s | oracle %s' % (name, out['ll_observed'][1].cpu().tolist(), ll2.tolist()))
    torch.testing.assert_close(out['ll_observed'][1].cpu(), ll2.float(), **TOL)
    compare_pictures(name, form, out['completed'], filled2, unsure_pixels(form, dec2, ref['tapes'][1]), 'completed')
    assert torch.equal(out['completed'], out['history'][2])
    assert torch.equal(out['completed'].cpu()[obs], x[obs])


GRAD_KEYS = ('likelihood.parameter_net.weight', 'first_bottom_up.0.weight', 'top_down_layers.0.stochastic.conv_in_q.weight')


@pytest.mark.parametrize('name', ['tiny_gauss', 'tiny_cifar'])
def test_masked_forward_gradients_match_float64_autograd(name):
    from oracle import lvae_ref as R
    from lvae_amd.noise import TapeNoise
    g = load_golden(name)
    sd, x, mask = double_sd(g), g.t('x').double(), golden_mask(g, 20)
    for k in GRAD_KEYS:
        sd[k].requires_grad_(True)
    tape = R.Tape(gen=torch.Generator().manual_seed(31))
    mo, ll, _, _ = ref_forward_masked(sd, g.cfg, x, mask, 0.5, tape, training=True)
    loss_ref = (-ll).mean() + mo['kl_loss']
    loss_ref.backward()
    finite(loss_ref.detach(), *[sd[k].grad for k in GRAD_KEYS])
    m = build(g, training=True)
    m.noise = TapeNoise(tape.entries)
    m.zero_grad()
    out = m(g.t('x').cuda(), mask=mask.cuda(), mask_fill=0.5)
    assert m.noise.exhausted()
    loss = (-out['ll']).mean() + out['kl_loss']
    loss.backward()
    print('masked loss | %s | engine %.6f | oracle %.6f' % (name, float(loss), float(loss_ref)))
    torch.testing.assert_close(loss.detach().cpu(), loss_ref.detach().float(), rtol=1e-5, atol=0)
    grads = dict(m.named_parameters())
    for k in GRAD_KEYS:
        want = sd[k].grad
        e = float((grads[k].grad.cpu().double() - want).norm() / want.norm())
        print('gradient    | %s %s | relative L2 %.3e | bound 1e-4' % (name, k, e))
        assert float(want.norm()) > 1e-5 and e < 1e-4, (k, e)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. properties on the device
# ---------------------------------------------------------------------------------------------------------------------------------
def _fresh(m, seed=5):
    from lvae_amd.noise import PhiloxNoise
    m.noise = PhiloxNoise(seed)
    return m


@pytest.fixture(scope='module')
def models():
    out = {}
    for name in GOLDENS:
        g = load_golden(name)
        out[name] = (build(g), g.t('x').cuda(), golden_mask(g, 30).cuda())
    return out


@pytest.mark.parametrize('name', GOLDENS)
def test_the_truth_under_the_mask_changes_nothing(models, name):
    m, x, mask = models[name]
    obs = mask[:, None].expand_as(x)
    other = torch.where(obs, x, torch.full_like(x, NAN))     # whatever: not-a-numbers
    with torch.no_grad():
        a, b = _fresh(m)(x, mask=mask, mask_fill=0.5), _fresh(m)(other, mask=mask, mask_fill=0.5)
    assert set(a) == set(b) and len(a) == 13
    for k in a:
        va, vb = a[k], b[k]
        if isinstance(va, dict):
            assert all(same_bits(va[q], vb[q]) for q in va), k
        elif isinstance(va, (list, tuple)):
            assert all(same_bits(p, q) for p, q in zip(va, vb)), k
        else:
            assert same_bits(va, vb), k
    assert bool(torch.isfinite(a['ll']).all()) and torch.equal(a['out_filled'][obs], x[obs])
    ia = _fresh(m).inpaint(x, mask, n_iters=3, return_history=True)
    ib = _fresh(m).inpaint(other, mask, n_iters=3, return_history=True)
    for k in ('completed', 'll_observed', 'history'):
        assert same_bits(ia[k], ib[k]), k
    assert bool(torch.isfinite(ia['completed']).all()) and not m.training
    for frame in ia['history']:
        assert torch.equal(frame[obs], x[obs])
    assert torch.equal(ia['completed'][obs], x[obs]) and torch.equal(ia['completed'], ia['history'][-1])
    assert float((ia['history'][1] - ia['history'][0])[~obs].abs().max()) > 0.0    # the missing pixels do move


def test_inpaint_init_forms_and_final_mean(models):
    m, x, mask = models['tiny_gauss']
    obs = mask[:, None].expand_as(x)
    start = {}
    for init in ('zeros', 'mean', 'noise', torch.full_like(x, 0.75)):
        out = _fresh(m).inpaint(x, mask, n_iters=1, init=init, return_history=True)
        key = init if isinstance(init, str) else 'tensor'
        start[key] = out['history'][0]
        assert torch.equal(start[key][obs], x[obs]) and tuple(out['history'].shape) == (2,) + tuple(x.shape)
    assert bool((start['zeros'][~obs] == 0.0).all()) and bool((start['mean'][~obs] == 0.5).all()) and bool((start['tensor'][~obs] == 0.75).all())
    noise = start['noise'][~obs]
    assert 0.0 <= float(noise.min()) and float(noise.max()) < 1.0 and float(noise.std()) > 0.2
    # final='mean': the missing pixels are the head's mean of the last round, the chain itself is the same
    a = _fresh(m).inpaint(x, mask, n_iters=2, final='sample', return_history=True)
    b = _fresh(m).inpaint(x, mask, n_iters=2, final='mean', return_history=True)
    assert same_bits(a['history'], b['history']) and same_bits(a['ll_observed'], b['ll_observed'])
    assert torch.equal(b['completed'][obs], x[obs]) and not torch.equal(a['completed'][~obs], b['completed'][~obs])
    with torch.no_grad():
        m.noise.step -= 1    # the draws of the last round again, on its input
        fwd = m(a['history'][1], mask=mask, mask_fill=a['history'][1])   # (the chain feeds the whole completion to the encoder)
    assert torch.equal(b['completed'][~obs], fwd['out_mean'][~obs])
    assert same_bits(fwd['out_filled'], a['completed']) and same_bits(fwd['ll'], a['ll_observed'][1])
    for name in ('tiny_mnist', 'tiny_discrlog'):   # the other heads with a mean
        mm, xx, mk = models[name]
        out = _fresh(mm).inpaint(xx, mk, n_iters=1, final='mean')
        oo = mk[:, None].expand_as(xx)
        assert torch.equal(out['completed'][oo], xx[oo]) and bool(torch.isfinite(out['completed']).all())


@pytest.mark.parametrize('name', ['tiny_cifar', 'tiny_mnist'])
def test_replayed_rounds_are_the_eager_rounds(models, name):
    m, x, mask = models[name]
    eager = _fresh(m, 11).inpaint(x, mask, n_iters=10, init='noise', return_history=True, use_graph=False)
    replay = _fresh(m, 11).inpaint(x, mask, n_iters=10, init='noise', return_history=True)      # PhiloxNoise and >= 8 rounds: the graph
    for k in ('completed', 'll_observed', 'history'):
        assert same_bits(eager[k], replay[k]), k
    forced = _fresh(m, 11).inpaint(x, mask, n_iters=4, init='noise', use_graph=True)
    assert same_bits(forced['ll_observed'], eager['ll_observed'][:4])
    assert not same_bits(eager['ll_observed'][0], eager['ll_observed'][9])       # fresh noise every round


def _record_calls(K, monkeypatch):
    names, real = [], K.call
    monkeypatch.setattr(K, 'call', lambda name, *args: (names.append(name), real(name, *args))[1])
    return names


HEAD_ENTRY = {'bernoulli': 'lvae_bernoulli%s_fwd_f32', 'gaussian': 'lvae_gaussian%s_fwd_f32', 'discr_log': 'lvae_discr_logistic%s_fwd_f32',
              'discr_log_mix': 'lvae_dmol_ll%s_fwd_f32'}


@pytest.mark.parametrize('name', GOLDENS)
def test_without_a_mask_nothing_changes(K, models, name, monkeypatch):
    m, x, mask = models[name]
    form = load_golden(name).cfg['likelihood_form']
    names = _record_calls(K, monkeypatch)
    with torch.no_grad():
        a = _fresh(m)(x)
        plain = list(names)
        del names[:]
        b = _fresh(m)(x, mask=None)
        none = list(names)
        del names[:]
        c = _fresh(m)(x, mask=mask)
        masked = list(names)
    assert plain == none and len(a) == len(b) == 12 and 'out_filled' not in b
    assert not any('masked' in n or 'mask_select' in n for n in plain)
    assert plain.count(HEAD_ENTRY[form] % '') == 1
    for k in ('ll', 'kl_sep', 'out_sample', 'kl_loss'):
        assert same_bits(a[k], b[k]), k
    # with a mask: one select in front, the masked head in the unmasked one's place, nothing else
    want = [HEAD_ENTRY[form] % '_masked' if n == HEAD_ENTRY[form] % '' else n for n in plain]
    first = masked.index('lvae_mask_select_f32')
    assert masked[:first] + masked[first + 1:] == want and masked.count('lvae_mask_select_f32') == 1
    assert first <= 1                             # (nothing but the noise source's begin precedes the select)
    every = torch.ones_like(mask)
    with torch.no_grad():
        d = _fresh(m)(x, mask=every)
    assert same_bits(d['ll'], a['ll']) and same_bits(d['out_filled'], x) and same_bits(d['kl_sep'], a['kl_sep'])


def test_masked_forward_and_inpaint_bf16(models):
    m, x, mask = models['tiny_cifar']
    obs = mask[:, None].expand_as(x)
    m.compute_dtype = 'bf16'
    try:
        with torch.no_grad():
            out = _fresh(m)(x, mask=mask)
        assert bool(torch.isfinite(out['ll']).all()) and torch.equal(out['out_filled'][obs], x[obs])
        res = _fresh(m).inpaint(x, mask, n_iters=2)
        assert bool(torch.isfinite(res['completed']).all()) and bool(torch.isfinite(res['ll_observed']).all())
        assert torch.equal(res['completed'][obs], x[obs])
    finally:
        m.compute_dtype = 'f32'


def test_value_errors(models):
    m, x, mask = models['tiny_gauss']
    B, C, H, W = x.shape
    bad_masks = [mask.float(), mask.to(torch.int64), mask[:, :-1], mask[:1], mask[:, None].expand(B, C, H, W), mask.cpu(), [[1]]]
    with torch.no_grad():
        for bad in bad_masks:
            with pytest.raises(ValueError):
                m(x, mask=bad)
            with pytest.raises(ValueError):
                m.inpaint(x, bad)
        for fill in (NAN, INF, -INF, 'grey', torch.zeros(B, C, H, W + 1).cuda(), torch.zeros(B, C, H, W)):
            with pytest.raises(ValueError):
                m(x, mask=mask, mask_fill=fill)
        with pytest.raises(ValueError):
            m(x, n_samples=2, mask=mask)
        for kw in (dict(n_iters=0), dict(n_iters=-1), dict(init='ones'), dict(init=0.5), dict(init=torch.zeros(B, C, H, W + 1).cuda()),
                   dict(final='mode'), dict(final=None)):
            with pytest.raises(ValueError):
                m.inpaint(x, mask, **kw)
        with pytest.raises(ValueError):
            m.inpaint(x[0], mask)
    cm, cx, cmask = models['tiny_cifar']
    with pytest.raises(ValueError):
        cm.inpaint(cx, cmask, final='mean')             # the mixture has no mean
    from lvae_amd.noise import TapeNoise
    cm.noise = TapeNoise([])
    with pytest.raises(ValueError):
        cm.inpaint(cx, cmask, use_graph=True)           # a tape runs eagerly
    _fresh(cm)
    assert not m.training and not cm.training
    out = _fresh(m)(x, mask=mask.bool())                # legal, under autograd, in eval mode
    assert out['ll'].requires_grad and not out['out_filled'].requires_grad


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the evaluation CLI
# ---------------------------------------------------------------------------------------------------------------------------------
def test_inpaint_cli(tmp_path, monkeypatch, capsys):
    import lvae_amd  # noqa: F401
    from lvae_amd import evaluate as leval
    from lvae_amd.images import grid_shape
    from test_images_cpu import decode_png
    monkeypatch.chdir(tmp_path)
    img_dir = str(tmp_path / 'pics')
    argv = ['-d', 'cifar10', '--zdims', '8', '8', '--downsample', '1', '1', '--nfilters', '16', '--skip', '--gated',
            '--freebits', '1.0', '--batch-size', '8', '--synthetic', '--seed', '3', '--n-test', '16']
    leval.main(argv + ['--inpaint', '--inpaint-mask', 'left', 'center', 'random', '--inpaint-frac', '0.25', '--inpaint-iters', '3',
                       '--inpaint-init', 'mean', '--img-dir', img_dir])
    n = min(leval.IMG_GRID_N, 16)
    data = torch.floor(256 * torch.rand((16, 3, 32, 32), generator=torch.Generator().manual_seed(3))) / 255   # main.synthetic_batch
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('inpaint ')]
    assert len(lines) == 3 and all('mse on the missing pixels' in l and 'll_observed' in l for l in lines)
    for j, kind in enumerate(('left', 'center', 'random')):
        a = np.load(str(tmp_path / ('inpaint_%s.npy' % kind)))
        assert a.shape == (n, 3, 3, 32, 32) and np.isfinite(a).all() and a.min() >= 0.0 and a.max() <= 1.0
        mask = leval.make_mask(kind, 0.25, (n, 32, 32), 3 + j)[:, None].expand(n, 3, 32, 32).numpy()
        assert np.array_equal(a[:, 0], data[:n].numpy())
        assert np.array_equal(a[:, 1][mask], data[:n].numpy()[mask]) and (a[:, 1][~mask] == 0.5).all()
        assert np.array_equal(a[:, 2][mask], data[:n].numpy()[mask]) and not np.array_equal(a[:, 2][~mask], a[:, 1][~mask])
        png = decode_png(open(os.path.join(img_dir, 'inpaint_%s.png' % kind), 'rb').read())
        assert png.shape == tuple(grid_shape(n * 3, 3, 32, 32)) + (3,)
    assert not os.path.exists(str(tmp_path / 'inpaint_right.npy'))
