"""Masked likelihoods and inpainting, the part that needs no GPU: the mask maker, the evaluation CLI's argument checks, the new C-ABI
symbols, and the float64 references tests/test_inpaint_gpu.py compares the device against (they live here, so that they are pinned to the
oracle on every machine).

The references restate no likelihood formula. A head's per-pixel terms are the oracle's own functions (`log_bernoulli`,
`discretized_mix_logistic_ll`, `log_discretized_logistic`, and the Gaussian expression of `oracle.lvae_ref.likelihood`) called on the pixels
reshaped to (N * HW, C, 1, 1) images: their sum over an "image" is then one pixel's term. A masked ll is those terms times the mask, summed;
gradients are autograd's. The head's decoding of the conv output (sigmoid, chunk, + 0.5, clamp) and its draws are the oracle's too:
`likelihood()` is called with an identity 3x3 convolution, which is exact in floating point."""
import ctypes
import math
import os
import re

import pytest
import torch

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ('bernoulli', 'gaussian', 'discr_log', 'discr_log_mix')
GOLDENS = ('tiny_mnist', 'tiny_cifar', 'tiny_gauss', 'tiny_discrlog')
MARGIN = 2e-4   # a thresholded draw this close to its threshold is left out of a comparison (the margin of tests/test_interpolate_gpu.py)
CAP = 1e-3      # ... at most this share of the pixels (the cap of its _compare_likelihood)


# ---------------------------------------------------------------------------------------------------------------------------------
# the references (shared with tests/test_inpaint_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def decoded(form, info):
    """the parameters of a head as the oracle's likelihood() returns them -> {name: NCHW tensor}"""
    if form == 'bernoulli':
        return {'mean': info['mean']}
    if form == 'discr_log_mix':
        return {'all_params': info['params']['all_params']}
    return dict(info['params'])


def pixel_ll(form, dec, x, per_element=False):
    """Per-pixel log-likelihood terms (B, H, W) of the NCHW image x under the decoded parameters `dec`: the oracle's functions on the pixels
    as (B * H * W, C, 1, 1) images. per_element (not for the mixture, whose colours are coupled): (B, H, W, C), every element its own image."""
    from oracle import lvae_ref as R
    B, C, H, W = x.shape
    if per_element:
        assert form != 'discr_log_mix'
        px = lambda t: t.permute(0, 2, 3, 1).reshape(-1, 1, 1, 1)
        shape = (B, H, W, C)
    else:
        px = lambda t: t.permute(0, 2, 3, 1).reshape(B * H * W, t.shape[1], 1, 1)
        shape = (B, H, W)
    if form == 'bernoulli':
        t = R.log_bernoulli(px(x), px(dec['mean']))
    elif form == 'gaussian':
        mean, lv = px(dec['mean']), px(dec['logvar'])
        t = (-0.5 * ((px(x) - mean) ** 2 / lv.exp() + lv + math.log(2 * math.pi))).sum((1, 2, 3))   # oracle.lvae_ref.likelihood, 'gaussian'
    elif form == 'discr_log':
        t = R.log_discretized_logistic(px(x) * (255 / 256) + 1 / 512, px(dec['mean']), px(dec['logscale']))
    else:
        t = R.discretized_mix_logistic_ll(px(x) * 2 - 1, px(dec['all_params']))
    return t.view(shape)


def masked_ll(form, dec, x, mask):
    """(ll (B,), sum of |term| (B,)) over the observed pixels; mask (B, H, W) bool. The |terms| are per element where the head has
    independent elements and per pixel for the mixture."""
    m = mask.to(x.dtype)
    ll = (pixel_ll(form, dec, x) * m).sum((1, 2))
    with torch.no_grad():
        if form == 'discr_log_mix':
            abs_terms = (pixel_ll(form, dec, x).abs() * m).sum((1, 2))
        else:
            abs_terms = (pixel_ll(form, dec, x, per_element=True).abs() * m[..., None]).sum((1, 2, 3))
    return ll, abs_terms


def identity_head(n_params, dt):
    """the state dict of a likelihood whose 3x3 parameter convolution hands its input through (exact: products with 1 and sums with 0)"""
    w = torch.zeros(n_params, n_params, 3, 3, dtype=dt)
    w[torch.arange(n_params), torch.arange(n_params), 1, 1] = 1.0
    return {'likelihood.parameter_net.weight': w, 'likelihood.parameter_net.bias': torch.zeros(n_params, dtype=dt)}


def head_reference(form, raw, x, mask, tape, dt):
    """One head on raw conv outputs `raw` (N, Cp, H, W) and the image x (N, C, H, W) under mask (N, H, W) bool, in dtype dt, the draws from
    `tape` -> dict: ll, ll_abs, dll (N, Cp, H, W), ll_full (the oracle's own unmasked ll), mean / mode / sample as the oracle returns them,
    filled = where(mask, x, sample), dec (the decoded parameters)."""
    from oracle import lvae_ref as R
    leaf = raw.detach().to(dt).clone().requires_grad_(True)
    xx = x.to(dt)
    ll_full, info = R.likelihood(identity_head(raw.shape[1], dt), {'likelihood_form': form}, leaf, xx, tape)
    dec = decoded(form, info)
    ll, ll_abs = masked_ll(form, dec, xx, mask)
    ll.sum().backward()
    sample = info['sample'].detach().to(dt)
    return {'ll': ll.detach(), 'll_abs': ll_abs, 'dll': leaf.grad.detach(), 'll_full': ll_full.detach(),
            'mean': None if info['mean'] is None else info['mean'].detach(), 'mode': None if info['mode'] is None else info['mode'].detach(),
            'sample': sample, 'filled': torch.where(mask[:, None], xx, sample), 'dec': {k: v.detach() for k, v in dec.items() if v is not None}}


def unsure_pixels(form, dec, entries):
    """(B, H, W) bool: the pixels whose thresholded draw sits within MARGIN of its threshold, from the oracle's parameters and the tape
    entries of the likelihood (the last one or two of a pass). Bernoulli: |u - mean| of any channel; the mixture: the two largest
    Gumbel-perturbed logits. The other heads draw nothing thresholded."""
    if form == 'bernoulli':
        u = torch.as_tensor(entries[-1]).double()
        return ((u - dec['mean'].double()).abs() <= MARGIN).any(1)
    if form == 'discr_log_mix':
        l = dec['all_params'].double().permute(0, 2, 3, 1)
        nmix = l.shape[-1] // 10
        u = torch.as_tensor(entries[-2]).double()
        top = (l[..., :nmix] - torch.log(-torch.log(u))).topk(min(2, nmix), dim=-1).values
        return (top[..., 0] - top[..., -1] <= MARGIN) if nmix > 1 else torch.zeros(l.shape[:3], dtype=torch.bool)
    return torch.zeros(dec['mean'].shape[0], *dec['mean'].shape[2:], dtype=torch.bool)


def ref_forward_masked(sd, cfg, x, mask, fill, tape, training=False):
    """forward(x, mask, mask_fill) from the oracle's pieces: lvae_forward on where(mask, x, fill), the masked ll recomputed from its
    likelihood parameters by the per-pixel trick. Returns (the oracle's dict, ll (B,), filled (B, C, H, W), dec)."""
    from oracle import lvae_ref as R
    form = cfg['likelihood_form']
    xin = torch.where(mask[:, None], x, fill if torch.is_tensor(fill) else torch.full_like(x, float(fill)))
    mo = R.lvae_forward(sd, cfg, xin, tape, training)
    dec = decoded(form, {'mean': mo['out_mean'], 'params': mo['likelihood_params']})
    ll, _ = masked_ll(form, dec, xin, mask)
    return mo, ll, torch.where(mask[:, None], xin, mo['out_sample'].to(xin.dtype)), dec


def double_sd(g):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in g.state_dict().items()}


def golden_mask(g, seed=0):
    """the mask the model tests put on a golden's batch: per image the left half, a centred box, random at 0.5, and again the left half"""
    from lvae_amd.evaluate import make_mask
    B, _, H, W = g.t('x').shape
    kinds = ['left', 'center', 'random', 'left']
    return torch.stack([make_mask(kinds[b % 4], 0.5, (H, W), seed + b) for b in range(B)])


_REF = {}


def inpaint_reference(name):
    """Two Gibbs rounds of the golden `name` in float64 from the all-zeros start, the draws recorded: round 2 here runs on the oracle's own
    round-1 completion (the GPU test runs it again on the engine's). Returns dict(mask, tapes [entries of round 1, of round 2],
    rounds [(ll, filled, dec) per round])."""
    from oracle import lvae_ref as R
    if name not in _REF:
        g = load_golden(name)
        sd, x, mask = double_sd(g), g.t('x').double(), golden_mask(g)
        cur = torch.where(mask[:, None], x, torch.zeros_like(x))
        tapes, rounds = [], []
        with torch.no_grad():
            for r in range(2):
                tape = R.Tape(gen=torch.Generator().manual_seed(71 + r))
                _, ll, filled, dec = ref_forward_masked(sd, g.cfg, cur, mask, cur, tape)
                tapes.append(tape.entries)
                rounds.append((ll, filled, dec))
                cur = filled
        _REF[name] = dict(mask=mask, tapes=tapes, rounds=rounds)
    return _REF[name]


def forward_reference(name):
    """forward(x, mask, mask_fill=0.25) of the golden `name` in float64, eval mode -> dict(mask, entries, mo, ll, filled, dec)"""
    from oracle import lvae_ref as R
    key = ('fwd', name)
    if key not in _REF:
        g = load_golden(name)
        mask = golden_mask(g, 10)
        tape = R.Tape(gen=torch.Generator().manual_seed(61))
        with torch.no_grad():
            mo, ll, filled, dec = ref_forward_masked(double_sd(g), g.cfg, g.t('x').double(), mask, 0.25, tape)
        _REF[key] = dict(mask=mask, entries=tape.entries, mo=mo, ll=ll, filled=filled, dec=dec)
    return _REF[key]


# ---------------------------------------------------------------------------------------------------------------------------------
# make_mask
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(28, 28), (3, 16, 16), (2, 1, 9, 14)], ids=str)
@pytest.mark.parametrize('frac', [0.5, 0.3, 0.1])
def test_make_mask_strips_and_box(shape, frac):
    from lvae_amd.evaluate import make_mask
    H, W = shape[-2:]
    lead = 1
    for s in shape[:-2]:
        lead *= s
    h, w = int(round(frac * H)), int(round(frac * W))
    for kind, hidden in (('left', H * w), ('right', H * w), ('top', h * W), ('bottom', h * W), ('center', h * w)):
        m = make_mask(kind, frac, shape, 0)
        assert m.dtype == torch.bool and tuple(m.shape) == tuple(shape) and not m.is_cuda
        assert int((~m).sum()) == lead * hidden, (kind, frac)
    m = make_mask('left', frac, shape, 0)
    assert not bool(m[..., :, :w].any()) and bool(m[..., :, w:].all())
    m = make_mask('right', frac, shape, 0)
    assert not bool(m[..., :, W - w:].any()) and bool(m[..., :, :W - w].all())
    m = make_mask('top', frac, shape, 0)
    assert not bool(m[..., :h, :].any()) and bool(m[..., h:, :].all())
    m = make_mask('bottom', frac, shape, 0)
    assert not bool(m[..., H - h:, :].any()) and bool(m[..., :H - h, :].all())
    m = make_mask('center', frac, shape, 0)
    t, l = (H - h) // 2, (W - w) // 2
    assert not bool(m[..., t:t + h, l:l + w].any())


def test_make_mask_random_is_seeded_and_has_the_share():
    from lvae_amd.evaluate import make_mask
    a, b, c = make_mask('random', 0.3, (64, 64), 5), make_mask('random', 0.3, (64, 64), 5), make_mask('random', 0.3, (64, 64), 6)
    assert a.dtype == torch.bool and torch.equal(a, b) and not torch.equal(a, c)
    n = 64 * 64
    for frac in (0.3, 0.5, 0.9):
        for seed in range(4):
            hidden = int((~make_mask('random', frac, (64, 64), seed)).sum())
            assert abs(hidden - frac * n) <= 3.0 * math.sqrt(n * frac * (1.0 - frac)), (frac, seed, hidden)
    for bad in (dict(kind='diagonal'), dict(frac=-0.1), dict(frac=1.5), dict(shape=(8,))):
        with pytest.raises(ValueError):
            make_mask(**dict(dict(kind='left', frac=0.5, shape=(8, 8), seed=0), **bad))


# ---------------------------------------------------------------------------------------------------------------------------------
# parse_eval_args
# ---------------------------------------------------------------------------------------------------------------------------------
BASE = ['-d', 'cifar10', '--zdims', '8', '8', '--downsample', '1', '1', '--synthetic']


def test_parse_eval_args_accepts_the_inpaint_flags():
    from lvae_amd.evaluate import MASK_KINDS, parse_eval_args
    a = parse_eval_args(BASE)
    assert a.inpaint is False and a.inpaint_mask == ['left'] and a.inpaint_frac == 0.5 and a.inpaint_iters == 10
    assert a.inpaint_init == 'zeros' and a.inpaint_final == 'sample'
    a = parse_eval_args(BASE + ['--inpaint', '--inpaint-mask'] + list(MASK_KINDS) + ['--inpaint-frac', '0.25', '--inpaint-iters', '1',
                                '--inpaint-init', 'noise'])
    assert a.inpaint and a.inpaint_mask == list(MASK_KINDS) and a.inpaint_frac == 0.25 and a.inpaint_iters == 1 and a.inpaint_init == 'noise'
    a = parse_eval_args(BASE + ['--inpaint', '--inpaint-final', 'mean', '--likelihood', 'gaussian', '--inpaint-init', 'mean'])
    assert a.inpaint_final == 'mean'
    a = parse_eval_args(['-d', 'static_mnist', '--zdims', '8', '--downsample', '1', '--inpaint-final', 'mean'])   # Bernoulli by default
    assert a.inpaint_final == 'mean'


@pytest.mark.parametrize('extra', [['--inpaint-frac', '0'], ['--inpaint-frac', '1'], ['--inpaint-frac', '-0.2'], ['--inpaint-frac', '1.5'],
                                   ['--inpaint-frac', 'nan'], ['--inpaint-iters', '0'], ['--inpaint-iters', '-3'],
                                   ['--inpaint-final', 'mean'],                                        # cifar10: the mixture by default
                                   ['--inpaint-final', 'mean', '--likelihood', 'discr_log_mix'],
                                   ['--inpaint-mask', 'diagonal'], ['--inpaint-mask', 'left', 'Left'],
                                   ['--inpaint-init', 'ones'], ['--inpaint-final', 'mode']], ids=lambda e: ' '.join(e))
def test_parse_eval_args_refuses(extra):
    from lvae_amd.evaluate import parse_eval_args
    with pytest.raises(SystemExit):
        parse_eval_args(BASE + ['--inpaint'] + extra)


# ---------------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = {'lvae_bernoulli_masked_fwd_f32': 14, 'lvae_dmol_ll_masked_fwd_f32': 13, 'lvae_gaussian_masked_fwd_f32': 12,
               'lvae_discr_logistic_masked_fwd_f32': 14, 'lvae_mask_select_f32': 10}


def test_library_exports_the_masked_entry_points():
    import lvae_amd  # noqa: F401
    from lvae_amd import _C
    lib = ctypes.CDLL(_C.LIB_PATH)
    hdr = open(os.path.join(ROOT, 'include', 'lvae_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name, n_args in NEW_SYMBOLS.items():
        assert hasattr(lib, name), name
        res, args = _C.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == n_args, name
        decl = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % name, hdr).group(1)
        params = [p.strip() for p in decl.split(',')]
        assert len(params) == n_args, (name, params)
        for p, a in zip(params, args):   # pointers as void*, the scalars by their width
            want = (ctypes.c_void_p if '*' in p else ctypes.c_int64 if p.startswith('int64_t') else ctypes.c_size_t if p.startswith('size_t')
                    else ctypes.c_float if p.startswith('float') else ctypes.c_int32)
            assert a is want, (name, p, a)
        assert 'const uint8_t* mask' in decl
    assert _C.ABI_VERSION == 17 and _C.load().lvae_abi_version() == 17
    from lvae_amd import kernels as K
    for fn in ('bernoulli_masked_fwd', 'dmol_ll_masked_fwd', 'gaussian_masked_fwd', 'discr_logistic_masked_fwd', 'mask_select', 'pixel_mask'):
        assert callable(getattr(K, fn))


def test_the_model_and_the_heads_take_a_mask():
    import inspect
    import lvae_amd  # noqa: F401
    from lvae_amd.lib.likelihoods import LikelihoodModule
    from lvae_amd.models.lvae import LadderVAE
    sig = inspect.signature(LadderVAE.forward)
    assert list(sig.parameters)[:5] == ['self', 'x', 'n_samples', 'mask', 'mask_fill']
    assert sig.parameters['mask'].default is None and sig.parameters['mask_fill'].default == 0.0
    sig = inspect.signature(LadderVAE.inpaint)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[3:]] == [
        ('n_iters', 10), ('init', 'zeros'), ('final', 'sample'), ('return_history', False), ('use_graph', None)]
    assert list(inspect.signature(LikelihoodModule.forward).parameters)[:5] == ['self', 'input_', 'x', 'noise', 'mask']
    K = lvae_amd.kernels
    with pytest.raises(ValueError):
        K.pixel_mask(torch.ones(2, 4, 4), 2, 4, 4, 'cpu')                      # dtype
    with pytest.raises(ValueError):
        K.pixel_mask(torch.ones(2, 4, 5, dtype=torch.bool), 2, 4, 4, 'cpu')    # shape
    m = K.pixel_mask(torch.ones(2, 1, 4, 4, dtype=torch.bool), 2, 4, 4, 'cpu')
    assert m.dtype == torch.uint8 and tuple(m.shape) == (2, 4, 4)


# ---------------------------------------------------------------------------------------------------------------------------------
# the references themselves
# ---------------------------------------------------------------------------------------------------------------------------------
def head_inputs(form, N, HW, C, nmix, seed):
    """raw conv outputs (N, Cp, HW, 1) and an image (N, C, HW, 1) of a head, on the CPU, float32"""
    g = torch.Generator().manual_seed(seed)
    if form == 'bernoulli':
        raw = torch.rand(N, C, HW, 1, generator=g) * 16 - 8
        x = (torch.rand(N, C, HW, 1, generator=g) < 0.5).float()
    elif form == 'gaussian':
        raw = torch.cat((torch.rand(N, C, HW, 1, generator=g) * 4 - 2, torch.rand(N, C, HW, 1, generator=g) * 5 - 3), 1)
        x = torch.rand(N, C, HW, 1, generator=g)
    elif form == 'discr_log':
        raw = torch.cat((torch.rand(N, C, HW, 1, generator=g) * 2 - 1, torch.rand(N, C, HW, 1, generator=g) * 6 - 4), 1)
        x = torch.floor(256 * torch.rand(N, C, HW, 1, generator=g)) / 255
    else:
        assert C == 3
        raw = torch.randn(N, 10 * nmix, HW, 1, generator=g)
        x = torch.floor(256 * torch.rand(N, 3, HW, 1, generator=g)) / 255
    return raw, x


@pytest.mark.parametrize('form', FORMS)
def test_per_pixel_terms_sum_to_the_oracles_ll(form):
    from oracle import lvae_ref as R
    N, HW, C = 2, 37, 3
    raw, x = head_inputs(form, N, HW, C, 10, 3)
    every = torch.ones(N, HW, 1, dtype=torch.bool)
    ref = head_reference(form, raw, x, every, R.Tape(gen=torch.Generator().manual_seed(1)), torch.float64)
    torch.testing.assert_close(ref['ll'], ref['ll_full'], rtol=1e-12, atol=1e-12)
    assert bool((ref['ll_abs'] >= ref['ll'].abs() - 1e-9).all())
    if form != 'discr_log_mix':   # and element by element
        el = pixel_ll(form, ref['dec'], x.double(), per_element=True)
        torch.testing.assert_close(el.sum((1, 2, 3)), ref['ll_full'], rtol=1e-12, atol=1e-12)
    half = torch.rand(N, HW, 1, generator=torch.Generator().manual_seed(2)) < 0.5
    a = head_reference(form, raw, x, half, R.Tape(gen=torch.Generator().manual_seed(1)), torch.float64)
    b = head_reference(form, raw, x, ~half, R.Tape(gen=torch.Generator().manual_seed(1)), torch.float64)
    torch.testing.assert_close(a['ll'] + b['ll'], ref['ll_full'], rtol=1e-12, atol=1e-12)
    hidden = (~half)[:, None].expand_as(a['dll'])
    assert float(a['dll'][hidden].abs().max()) == 0.0 and float(a['dll'][~hidden].abs().max()) > 0.0
    assert torch.equal(a['filled'][half[:, None].expand_as(x)], x.double()[half[:, None].expand_as(x)])


@pytest.mark.parametrize('name', GOLDENS)
def test_the_oracle_alone_stays_inside_the_cap(name):
    """the seeds of the model tests: few enough thresholded draws sit within MARGIN of their threshold, in float64, before any GPU runs"""
    g = load_golden(name)
    form = g.cfg['likelihood_form']
    ref = inpaint_reference(name)
    counts = []
    for r in range(2):
        unsure = unsure_pixels(form, ref['rounds'][r][2], ref['tapes'][r])
        counts.append(int(unsure.sum()))
        assert counts[-1] <= CAP * unsure.numel(), (name, r, counts)
    fwd = forward_reference(name)
    unsure = unsure_pixels(form, fwd['dec'], fwd['entries'])
    counts.append(int(unsure.sum()))
    assert counts[-1] <= CAP * unsure.numel(), (name, counts)
    print('thresholded draws within %g | %s | %s of %d pixels' % (MARGIN, name, counts, unsure.numel()))


def test_one_gibbs_round_keeps_the_observed_pixels():
    """float64 toy check of the host-side reference: after a round the observed pixels are x's, the missing ones the model's draw, and
    ll_observed does not depend on what the truth holds under the mask"""
    from oracle import lvae_ref as R
    g = load_golden('tiny_gauss')
    sd, x, mask = double_sd(g), g.t('x').double(), golden_mask(g)
    obs = mask[:, None].expand_as(x)
    assert bool(obs.any()) and bool((~obs).any())
    start = torch.where(obs, x, torch.zeros_like(x))
    with torch.no_grad():
        tape = R.Tape(gen=torch.Generator().manual_seed(4))
        mo, ll, filled, _ = ref_forward_masked(sd, g.cfg, start, mask, start, tape)
        other = torch.where(obs, x, torch.rand(x.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(9)))
        _, ll2, filled2, _ = ref_forward_masked(sd, g.cfg, torch.where(obs, other, torch.zeros_like(x)), mask, start, R.Tape(entries=tape.entries))
    assert torch.equal(filled[obs], x[obs])
    assert torch.equal(filled[~obs], mo['out_sample'][~obs]) and not torch.equal(filled[~obs], start[~obs])
    assert torch.equal(ll, ll2) and torch.equal(filled, filled2)
    assert bool(torch.isfinite(ll).all()) and tuple(ll.shape) == (x.shape[0],)
