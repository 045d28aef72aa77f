"""The spectral regulariser on the device: lvae_spectral_step_f32 / lvae_spectral_reduce_f32 against the float64 reference of
tests/spectral_ref.py on a hand-built arena, and spectral.SpectralReg inside whole training steps of the tiny_cifar golden (batch 4).

No tolerance is chosen here. r64 is the reference in float64 on the CPU, r32 the same in float32 on the CPU, and the two rules of
docs/ELEMENTWISE_PARITY.md apply:
    element-wise (v', u', the gradient)        |kernel - r64| <= 2 max|r32 - r64| + 1e-5 |r64| + 1e-6
    per-sum (sigma, sr_sum)                    |kernel - r64| <= 2 max|r32 - r64| + 4e-6 sum_i |term_i|     (terms |v'_k| |A_kc| |u'_c|)
Every comparison prints `yardstick | case | kernel error | r32 error | bound` before it asserts (run with -s)."""
import math

import pytest
import torch

import spectral_ref as R
from conftest import load_golden
from test_ema_gpu import _fresh_table, _images, _model

pytestmark = pytest.mark.gpu

# (K, Cout) -> (cin, kh, kw, transposed): what the shape stands for in the model
GEOM = {(75, 64): (3, 5, 5, False),      # stem 5x5x3
        (576, 64): (64, 3, 3, False),    # the common 3x3
        (64, 128): (64, 1, 1, False),    # gate
        (128, 64): (128, 1, 1, False),   # merge
        (288, 64): (32, 3, 3, True),     # conv_out (here as a transposed convolution's weight: the same physical layout)
        (576, 100): (64, 3, 3, False),   # DMoL head: Cout no multiple of 64
        (576, 1): (64, 3, 3, False),     # Bernoulli head
        (576, 3): (64, 3, 3, False),     # Gaussian head
        (1600, 64): (64, 5, 5, False),   # 5x5x64
        (9, 2): (1, 3, 3, False)}        # smaller than a wave
LAM = 0.37


def _K():
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels as K
    return K


class HandArena:
    """params / grads of one layout: a non-convolution slot of 37 floats (padded to 64) in front of every matrix, every slot padded to a
    multiple of 64 floats, everything (padding included) filled with random non-zero values; the matrices are `mats` ([K][C] float32)."""

    def __init__(self, mats, seed=0):
        g = torch.Generator().manual_seed(4242 + seed)
        rnd = lambda n: torch.randn(n, generator=g) + 3.0 * torch.sign(torch.randn(n, generator=g))   # (non-zero)
        pad = lambda n: (n + 63) // 64 * 64
        self.rows, parts, off, uo, vo = [], [], 0, 0, 0
        self.inside = []
        for A in mats:
            parts.append(rnd(64))
            off += 64
            k, c = A.shape
            slot = rnd(pad(k * c))
            slot[:k * c] = A.reshape(-1)
            parts.append(slot)
            self.rows.append((off, off, k, c, uo, vo))
            self.inside.append((off, off + k * c))
            off, uo, vo = off + pad(k * c), uo + c, vo + k
        parts.append(rnd(64))
        self.params = torch.cat(parts)
        self.grads = rnd(self.params.numel())
        self.nu, self.nv = uo, vo
        self.mask = torch.zeros(self.params.numel(), dtype=torch.bool)
        for lo, hi in self.inside:
            self.mask[lo:hi] = True

    def run(self, u0, lam=LAM, gscale=None, grads='random', steps=1, max_workgroups=0, iterate_only=False):
        """`steps` launches from u0 -> dict of CPU tensors: u, v, sigma, grads, params, metrics."""
        K = _K()
        table = K.spectral_table(self.rows, 'cuda')
        params = self.params.cuda()
        g = (self.grads.clone() if grads == 'random' else torch.zeros_like(self.grads)).cuda()
        u, v = u0.clone().cuda(), torch.full((self.nv,), 7.0, device='cuda')
        sigma, metrics = torch.full((len(self.rows),), -1.0, device='cuda'), torch.zeros(2, device='cuda')
        gs = None if gscale is None else torch.tensor([gscale], dtype=torch.float32, device='cuda')
        for _ in range(steps):
            K.spectral_step(table, params, None if iterate_only else g, u, u, v, sigma, lam, gs, max_workgroups)
        K.spectral_reduce(sigma, metrics)
        torch.cuda.synchronize()
        return {'u': u.cpu(), 'v': v.cpu(), 'sigma': sigma.cpu(), 'grads': g.cpu(), 'params': params.cpu(), 'metrics': metrics.cpu()}


@pytest.fixture(scope='module')
def case():
    """The hand-built arena of the ten shapes and the one-step references, computed once on the CPU before anything goes to the device."""
    ws, mats, u0s, r64, r32 = [], [], [], [], []
    for (k, c) in R.SHAPES:
        cin, kh, kw, tr = GEOM[(k, c)]
        assert cin * kh * kw == k
        w = R.logical_weight(R.builder(k, c).float(), cin, kh, kw, tr)    # the fp32 weight the device holds, in its logical shape
        u0 = R.start_u(c).float()
        ws.append(w)
        mats.append(R.arena_matrix(w, tr).contiguous())
        u0s.append(u0)
        r64.append(R.step(w.double(), u0.double(), tr))
        r32.append(R.step(w, u0, tr))
    return {'arena': HandArena(mats), 'w': ws, 'u0': torch.cat(u0s), 'r64': r64, 'r32': r32}


def _split(flat, sizes):
    return list(torch.split(flat, sizes))


@pytest.mark.parametrize('gscale', [None, 0.5, 0.125], ids=['gscale-null', 'gscale-half', 'gscale-eighth'])
def test_one_step_against_float64(case, gscale):
    ar = case['arena']
    out = ar.run(case['u0'], gscale=gscale)
    us, vs = _split(out['u'], [c for _, c in R.SHAPES]), _split(out['v'], [k for k, _ in R.SHAPES])
    gs = 1.0 if gscale is None else gscale
    for i, (k, c) in enumerate(R.SHAPES):
        tr = GEOM[(k, c)][3]
        r64, r32 = case['r64'][i], case['r32'][i]
        tag = 'spectral_step %4dx%-3d gscale %-5s ' % (k, c, gscale)
        R.close_elem(tag + "v'", vs[i], R.arena_order(r64['v']), R.arena_order(r32['v']))
        R.close_elem(tag + "u'", us[i], r64['u'], r32['u'])
        R.close_sum(tag + 'sigma', out['sigma'][i:i + 1], r64['sigma'], r32['sigma'], r64['sigma_abs'])
        lo, hi = ar.inside[i]
        g0 = R.logical_weight(ar.grads[lo:hi].view(k, c), *GEOM[(k, c)])
        want64 = g0.double() + R.grad_increment(r64, LAM, gs, tr)
        want32 = g0 + R.grad_increment(r32, LAM, gs, tr)
        R.close_elem(tag + 'grad', R.logical_weight(out['grads'][lo:hi].view(k, c), *GEOM[(k, c)]), want64, want32)
    # the two numbers of the train line
    s64 = sum(r['sigma'] for r in case['r64'])
    s32 = torch.stack([r['sigma'] for r in case['r32']]).sum()
    R.close_sum('spectral_reduce sr_sum', out['metrics'][0:1], s64, s32, sum(r['sigma_abs'] for r in case['r64']))
    assert float(out['metrics'][1]) == float(out['sigma'].max())
    # every element outside the listed matrices keeps its bits: the other slots, the padding, and the parameters themselves
    assert torch.equal(out['grads'][~ar.mask], ar.grads[~ar.mask])
    assert not torch.equal(out['grads'][ar.mask], ar.grads[ar.mask])
    assert torch.equal(out['params'], ar.params)


def test_increment_scales_exactly_with_gscale_and_iterate_only_touches_no_gradient(case):
    ar = case['arena']
    one = ar.run(case['u0'], grads='zero')                       # from zero gradients the slots hold the increment itself
    for gscale, factor in ((0.5, 2.0), (0.125, 8.0)):
        scaled = ar.run(case['u0'], grads='zero', gscale=gscale)
        assert torch.equal(scaled['grads'], one['grads'] * factor)
        for k in ('u', 'v', 'sigma', 'metrics'):
            assert torch.equal(scaled[k], one[k]), k
    assert float(one['grads'][ar.mask].abs().max()) > 0 and float(one['grads'][~ar.mask].abs().max()) == 0
    it = ar.run(case['u0'], iterate_only=True)
    assert torch.equal(it['grads'], ar.grads)
    for k in ('u', 'v', 'sigma', 'metrics'):
        assert torch.equal(it[k], one[k]), k


def test_same_bits_twice_and_at_every_grid(case):
    ar = case['arena']
    ref = ar.run(case['u0'], steps=3)
    for wgs in (0, 1, 3, 7, len(R.SHAPES), 1000):
        again = ar.run(case['u0'], steps=3, max_workgroups=wgs)
        for k in ref:
            assert torch.equal(ref[k], again[k]), (wgs, k)


def test_twenty_steps_reach_the_largest_singular_value(case):
    ar = case['arena']
    out = ar.run(case['u0'], steps=20, iterate_only=True)
    c_of = [c for _, c in R.SHAPES]
    u0s = _split(case['u0'], c_of)
    for i, (k, c) in enumerate(R.SHAPES):
        tr = GEOM[(k, c)][3]
        w = case['w'][i]
        sv = torch.linalg.svdvals(R.arena_matrix(w.double(), tr))[0]
        r32 = R.steps(w, u0s[i], 20, tr)
        r64 = R.steps(w.double(), u0s[i].double(), 20, tr)
        R.close_sum('20 steps %4dx%-3d sigma against svdvals' % (k, c), out['sigma'][i:i + 1], sv, r32['sigma'], r64['sigma_abs'])


@pytest.mark.parametrize('scale', [0.0, 1e-30, 1e-14], ids=['zero', 'times-1e-30', 'times-1e-14'])
def test_zero_and_tiny_matrices_follow_the_clamped_formula(scale):
    """A norm below 1e-12 is replaced by 1e-12: v' = s / 1e-12, u' = t / 1e-12, sigma = |t| itself. A zero matrix gives zeros and no NaN.
    (At 1e-30 t underflows fp32 altogether; at 1e-14 both norms are below the clamp and nothing underflows.)"""
    shapes = [(576, 64), (75, 64), (9, 2)]
    ws, mats, u0s = [], [], []
    for k, c in shapes:
        w = R.logical_weight((R.builder(k, c) * scale).float(), *GEOM[(k, c)])
        ws.append(w)
        mats.append(R.arena_matrix(w).contiguous())
        u0s.append(R.start_u(c).float())
    ar = HandArena(mats, seed=1)
    ref = [(R.step(w.double(), u.double()), R.step(w, u)) for w, u in zip(ws, u0s)]
    out = ar.run(torch.cat(u0s))
    for k in ('u', 'v', 'sigma', 'grads', 'metrics'):
        assert bool(torch.isfinite(out[k]).all()), k
    us, vs = _split(out['u'], [c for _, c in shapes]), _split(out['v'], [k for k, _ in shapes])
    for i, (k, c) in enumerate(shapes):
        r64, r32 = ref[i]
        tag = 'scale %g %3dx%-2d ' % (scale, k, c)
        R.close_elem(tag + "v'", vs[i], R.arena_order(r64['v']), R.arena_order(r32['v']))
        R.close_elem(tag + "u'", us[i], r64['u'], r32['u'])
        R.close_sum(tag + 'sigma', out['sigma'][i:i + 1], r64['sigma'], r32['sigma'], r64['sigma_abs'])
        assert float(r64['s'].norm()) < 1e-12 and float(r64['sigma']) < 1e-12           # the case is what it says: both norms are clamped
        if scale == 0.0:
            assert float(vs[i].abs().max()) == 0 and float(us[i].abs().max()) == 0 and float(out['sigma'][i]) == 0
            lo, hi = ar.inside[i]
            assert torch.equal(out['grads'][lo:hi], ar.grads[lo:hi])                    # a zero increment
        if scale == 1e-14:                                                              # far from the unclamped unit vectors
            assert 0 < float(vs[i].double().norm()) < 0.5 and 0 < float(out['sigma'][i]) < 1e-12
    assert torch.equal(out['grads'][~ar.mask], ar.grads[~ar.mask])


def test_an_entry_outside_its_buffers_is_refused_on_the_device():
    """Offsets that leave a buffer, or a matrix larger than the kernel's arrays: sigma = NaN for that entry, nothing written, the others run."""
    K = _K()
    A = R.builder(9, 2).float()
    params = torch.cat([A.reshape(-1), torch.zeros(46)]).cuda()
    g0 = torch.ones(64)
    table = torch.tensor([[0, 0, 9, 2, 0, 0], [60, 0, 9, 2, 2, 9], [0, 60, 9, 2, 2, 9], [0, 0, 9, 2, 3, 9], [0, 0, 9, 2, 2, 10],
                          [0, 0, 5000, 1, 2, 9], [-1, 0, 9, 2, 2, 9]], dtype=torch.int64).cuda()
    g, u, v = g0.clone().cuda(), torch.cat([R.start_u(2).float()] * 2).cuda(), torch.zeros(18).cuda()
    u_before = u.clone()
    sigma = torch.zeros(7).cuda()
    K.spectral_step(table, params, g, u, u, v, sigma, 1.0)
    met = K.spectral_reduce(sigma, torch.zeros(2).cuda())
    torch.cuda.synchronize()
    s = sigma.cpu()
    assert math.isfinite(float(s[0])) and float(s[0]) > 0 and bool(torch.isnan(s[1:]).all())
    assert torch.equal(u[2:], u_before[2:]) and float(v[9:].abs().max()) == 0 and torch.equal(g[18:].cpu(), g0[18:])
    assert bool(torch.isnan(met.cpu()).all())                   # a NaN sigma shows in both numbers of the train line
    with pytest.raises(ValueError):
        K.spectral_table([(0, 0, 5000, 1, 0, 0)], 'cuda')


# ---------------------------------------------------------------------------------------------------------------------------------
# whole steps: the tiny_cifar golden (a strided and a transposed convolution among its weights), batch 4
# ---------------------------------------------------------------------------------------------------------------------------------
LR = 1e-3


def _make(rule='adamax', lam=0.05, guard=None, full=False, warm=3, seed=11, boost=False):
    import lvae_amd  # noqa: F401
    from lvae_amd import optim
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.spectral import SpectralReg
    g = load_golden('tiny_cifar')
    _fresh_table()
    sd = g.state_dict()
    if boost:
        sd = _boosted(g.cfg, sd)
    m = _model(g.cfg, sd, PhiloxNoise(seed=3))
    sr = None if lam is None else SpectralReg(lam, warm_iters=warm, seed=seed)
    gd = None if guard is None else optim.GradGuard(**guard)
    kw = dict(lr=LR, guard=gd, spectral=sr)
    if full:
        kw.update(ema_decay=0.99, schedule=optim.LrSchedule('cosine', warmup_steps=2, decay_steps=3, min_lr=LR / 10))
    opt = {'adamax': optim.Adamax, 'adam': optim.Adam, 'adamw': optim.AdamW}[rule](m, **kw)
    return m, opt


def _state(m, opt):
    from lvae_amd.optim import RULES
    sd = m.state_dict()
    st = {k: v.detach().clone() for k, v in sd.items() if not k.endswith(('weight', 'bias', 'top_prior_params'))}
    st.update(params=m.arena.params.detach().clone(), exp_avg=opt.exp_avg.clone(), second=getattr(opt, RULES[opt.rule]).clone(),
              opt_step=opt.step_count.clone())
    if opt.ema is not None:
        st['ema'] = opt.ema.clone()
    if opt.spectral is not None:
        st.update(sr_state=opt.spectral.state.clone(), sr_metrics=opt.spectral.metrics.clone())
    return st


def _same(a, b, but=()):
    assert a.keys() == b.keys()
    for k in a:
        if k not in but:
            assert torch.equal(a[k], b[k]), k


def _loop(m, opt, xs, use_graph, accum=1, hook=None):
    from lvae_amd.engine import TrainStep
    st = TrainStep(m, opt, use_graph=use_graph, accum_steps=accum)
    outs = []
    for k, x in enumerate(xs):
        before = hook(k, None) if hook else None
        outs.append({key: v.detach().clone() for key, v in st(x.cuda()).items()})
        if hook:
            hook(k, before)
    torch.cuda.synchronize()
    assert (st.graph_a is not None) == (use_graph and len(xs) > 2)
    return outs


def _same_outs(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.keys() == y.keys() and {'sr_sum', 'sr_max'} <= set(x)
        for k in x:
            assert torch.equal(torch.nan_to_num(x[k], nan=-12345.0), torch.nan_to_num(y[k], nan=-12345.0)), k


def test_the_step_adds_autograds_gradient_of_the_penalty():
    """d/dW of lam * sum_i u'_i^T W_i v'_i with u', v' detached, by autograd in float64 on every convolution's LOGICAL weight, against what
    one step leaves in the zeroed gradient arena, read through the parameters' logical .grad views (so the arena's permutation of plain,
    strided and transposed weights is part of the check)."""
    from lvae_amd.lib.nn import Conv2dParams
    lam = 0.3
    m, opt = _make(lam=lam, warm=2)
    sr = opt.spectral.attach(m)
    named = dict(m.named_parameters())
    transposed = {k + '.weight': mod.transposed for k, mod in m.named_modules() if isinstance(mod, Conv2dParams)}
    assert set(sr.names) == set(transposed) and any(transposed.values()) and not all(transposed.values())
    u0s = _split(sr.u.detach().cpu().clone(), [c for _, c in sr.shapes])
    jobs = []
    for name, u0 in zip(sr.names, u0s):                      # every reference before the launch
        w = named[name].detach().cpu().clone()
        want = []
        for dt in (torch.float64, torch.float32):
            wd = w.to(dt).requires_grad_(True)
            r = R.step(wd.detach(), u0.to(dt), transposed[name])
            M = R.out_first(wd, transposed[name]).reshape(r['u'].numel(), -1)
            (lam * torch.dot(r['u'], M @ r['v'].reshape(-1))).backward()
            want.append(wd.grad)
        jobs.append((name, want[0], want[1]))
    m.arena.zero_grad()
    sr.step(m)
    sr.finish()
    torch.cuda.synchronize()
    other = [p for k, p in named.items() if k not in transposed and p.requires_grad]
    assert other and all(float(p.grad.abs().max()) == 0 for p in other)        # biases, BatchNorm, the prior: untouched
    for name, r64, r32 in jobs:
        R.close_elem('penalty gradient %s' % name, named[name].grad, r64, r32)
    assert float(sr.sr_sum) > 0 and float(sr.sr_max) == float(sr.sigma.max())


XS = [_images(4, 60 + k) for k in range(4)]
FULL = dict(rule='adamw', guard=dict(max_norm=1e30, skip_threshold=math.inf), full=True)


@pytest.mark.parametrize('form', ['plain', 'adamw+ema+schedule+guard+accum2'])
def test_captured_steps_equal_eager_steps_bit_for_bit(form):
    """Two eager steps, the capture and a replay against four eager steps: weights, moments, u, v, sigma and every metric."""
    kw, accum = (dict(), 1) if form == 'plain' else (FULL, 2)
    xs = _xs_for(accum)
    runs = []
    for use_graph in (True, False):
        m, opt = _make(**kw)
        outs = _loop(m, opt, xs, use_graph, accum=accum)
        runs.append((outs, _state(m, opt)))
    _same_outs(runs[0][0], runs[1][0])
    _same(runs[0][1], runs[1][1])
    sums = [float(o['sr_sum']) for o in runs[0][0]]
    assert all(math.isfinite(s) and s > 0 for s in sums) and len(set(sums)) == len(sums)      # the iterate moves with the weights
    # and the regulariser is in the update: the run without it ends elsewhere
    m, opt = _make(lam=None, **kw)
    _loop(m, opt, xs, True, accum=accum)
    assert not torch.equal(_state(m, opt)['params'], runs[0][1]['params'])


def _xs_for(accum):
    return XS if accum == 1 else [torch.cat([_images(4, 60 + 2 * k), _images(4, 61 + 2 * k)]) for k in range(4)]


def _one_launch(sr, arena):
    """What ONE iterate of the kernel makes of the regulariser's current u on the arena's current weights (a launch on copies)."""
    u, v, s = sr.u.clone(), torch.zeros_like(sr.v), torch.zeros_like(sr.sigma)
    _K().spectral_step(sr.table, arena.params, None, u, u, v, s)
    torch.cuda.synchronize()
    return u, v, s


@pytest.mark.parametrize('use_graph', [True, False], ids=['captured', 'eager'])
@pytest.mark.parametrize('form', ['plain', 'accum2', 'guarded'])
def test_a_train_step_iterates_exactly_once(form, use_graph):
    """Every step of a TrainStep (eager, the capture, a replay) moves u, v, sigma by exactly one power iteration on the weights the step
    started from, and counts the launches of the Python passes: one lvae_spectral_step_f32 and one lvae_spectral_reduce_f32 per step."""
    from lvae_amd import _C
    from lvae_amd import kernels as K
    accum = 2 if form == 'accum2' else 1
    m, opt = _make(guard=dict(max_norm=1e30, skip_threshold=math.inf) if form == 'guarded' else None)
    sr = opt.spectral
    calls, real = [], _C.call

    def counted(name, *args):
        calls.append(name)
        return real(name, *args)

    def hook(k, before):
        if before is None:
            ref = _one_launch(sr, m.arena)
            calls.clear()
            return ref
        torch.cuda.synchronize()
        for got, want, name in zip((sr.u, sr.v, sr.sigma), before, 'uvs'):
            assert torch.equal(got, want), (k, name)
        python_pass = not use_graph or k <= 2               # two eager steps, then the capture; a replay runs no Python pass
        n = {c: calls.count(c) for c in ('lvae_spectral_step_f32', 'lvae_spectral_reduce_f32')}
        assert n == ({'lvae_spectral_step_f32': 1, 'lvae_spectral_reduce_f32': 1} if python_pass else
                     {'lvae_spectral_step_f32': 0, 'lvae_spectral_reduce_f32': 0}), (k, n)
        assert not sr.open and not sr.done

    sr.prepare(m, guarded=form == 'guarded')                # (before the first reference launch: the warm start is not a step)
    _C.call = K.call = counted
    try:
        _loop(m, opt, _xs_for(accum), use_graph, accum=accum, hook=hook)
    finally:
        _C.call = K.call = real


@pytest.mark.parametrize('accum', [1, 2], ids=['plain', 'accum2'])
def test_a_train_step_adds_the_penalty_once_and_the_update_sees_lambda(accum):
    """One eager TrainStep step with the regulariser against the same step without it (same weights, images and noise, so the same data
    gradient): the gradient arena differs by (lam / gscale) v' u'^T of ONE reference step, in the convolution weights only. Under
    accum_steps = 2 the arena holds the sum over the two micro-passes and gscale is 1/2: the arena gains 2 lam v' u'^T, the update sees lam."""
    from lvae_amd.lib.nn import Conv2dParams
    lam = 0.3
    xs = _xs_for(accum)[:1]
    plain, plain_opt = _make(lam=None)
    _loop(plain, plain_opt, xs, False, accum=accum)
    base = {k: p.grad.detach().cpu().clone() for k, p in plain.named_parameters() if p.requires_grad}
    del plain, plain_opt
    m, opt = _make(lam=lam, warm=2)
    sr = opt.spectral.attach(m)
    named = dict(m.named_parameters())
    transposed = {k + '.weight': mod.transposed for k, mod in m.named_modules() if isinstance(mod, Conv2dParams)}
    u0s = _split(sr.u.detach().cpu().clone(), [c for _, c in sr.shapes])
    jobs = []
    for name, u0 in zip(sr.names, u0s):
        w = named[name].detach().cpu().clone()
        r64, r32 = R.step(w.double(), u0.double(), transposed[name]), R.step(w, u0, transposed[name])
        jobs.append((name, base[name].double() + R.grad_increment(r64, lam, 1.0 / accum, transposed[name]),
                     base[name] + R.grad_increment(r32, lam, 1.0 / accum, transposed[name]), r64['u'], r32['u']))
    _loop(m, opt, xs, False, accum=accum)
    assert (opt.gscale is None) == (accum == 1) and (accum == 1 or float(opt.gscale) == 0.5)
    for k, p in named.items():
        if p.requires_grad and k not in transposed:
            assert torch.equal(p.grad.cpu(), base[k]), k     # biases, BatchNorm, the prior: the data gradient, bit for bit
    for (name, want64, want32, u64, u32), got_u in zip(jobs, _split(sr.u.detach().cpu(), [c for _, c in sr.shapes])):
        R.close_elem('TrainStep accum %d gradient %s' % (accum, name), named[name].grad, want64, want32)
        R.close_elem("TrainStep accum %d u' %s" % (accum, name), got_u, u64, u32)
        inc = (named[name].grad.cpu().double() - base[name].double()).norm()
        want = (want64 - base[name].double()).norm()
        assert 0.9 * float(want) <= float(inc) <= 1.1 * float(want), (name, float(inc), float(want))   # once, not twice: a condition


@pytest.mark.parametrize('use_graph', [True, False], ids=['captured', 'eager'])
def test_a_skipped_step_leaves_the_iterate_and_everything_else(use_graph):
    bad = 3                                                    # a replayed step when captured
    xs = [x.clone() for x in XS] + [_images(4, 70)]
    xs[bad][1, 2, 5, 7] = math.nan                             # one NaN pixel: a NaN gradient
    m, opt = _make(guard=dict(max_norm=1e30, skip_threshold=math.inf))
    seen = {}

    def hook(k, before):
        if before is None:
            return _state(m, opt)
        seen[k] = (before, _state(m, opt))

    outs = _loop(m, opt, xs, use_graph, hook=hook)
    b0, b1 = seen[bad]
    tracked = [k for k in b0 if k.endswith('num_batches_tracked')]
    _same(b0, b1, but=tracked)
    assert math.isnan(float(outs[bad]['loss'])) and opt.guard.counts() == (0, 1)
    assert not bool(torch.isnan(b1['sr_state']).any()) and math.isfinite(float(outs[bad]['sr_sum']))
    n0, n1 = seen[bad + 1]                                     # the next step proceeds
    assert not torch.equal(n0['params'], n1['params']) and not torch.equal(n0['sr_state'], n1['sr_state'])
    assert math.isfinite(float(outs[bad + 1]['loss'])) and bool(torch.isfinite(n1['sr_state']).all())
    c0, c1 = seen[bad - 1]                                     # as did the one before
    assert not torch.equal(c0['sr_state'], c1['sr_state'])


def test_resume_continues_bit_for_bit(tmp_path):
    from lvae_amd.checkpoint import load_checkpoint, save_checkpoint, spectral_warning
    from lvae_amd.models.lvae import LadderVAE
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import AdamW
    from lvae_amd.spectral import SpectralReg
    m, opt = _make(rule='adamw')
    straight = _loop(m, opt, XS, False)
    want = _state(m, opt)
    m1, opt1 = _make(rule='adamw')
    first = _loop(m1, opt1, XS[:2], False)
    path = str(tmp_path / 'model_2.pt')
    save_checkpoint(path, m1, opt1)
    ck = torch.load(path)
    assert set(ck['spectral']) >= {'lam', 'u', 'v', 'sigma'} and ck['spectral']['lam'] == 0.05
    g = load_golden('tiny_cifar')
    _fresh_table()
    torch.manual_seed(123)
    m2 = LadderVAE(**g.cfg).cuda().train()
    m2.noise = PhiloxNoise(seed=999)
    opt2 = AdamW(m2, lr=LR, spectral=SpectralReg(0.05, warm_iters=7, seed=5))     # another seed and warm start: the file's iterate wins
    ck = load_checkpoint(path, m2, opt2)
    assert spectral_warning(path, ck, opt2) is None
    rest = _loop(m2, opt2, XS[2:], False)
    _same_outs(straight, first + rest)
    _same(want, _state(m2, opt2))
    # the command line's lambda runs, and a line says so
    opt3 = AdamW(m2, lr=LR, spectral=SpectralReg(0.5))
    ck = load_checkpoint(path, m2, opt3)
    assert 'written with --spectral-reg 0.05; continuing with 0.5' in spectral_warning(path, ck, opt3) and opt3.spectral.lam == 0.5
    # a file without the entry warm-starts afresh; a file with it loads into an optimizer without a regulariser
    old = str(tmp_path / 'old.pt')
    torch.save({k: v for k, v in ck.items() if k != 'spectral'}, old)
    opt4 = AdamW(m2, lr=LR, spectral=SpectralReg(0.05, warm_iters=2, seed=5))
    load_checkpoint(old, m2, opt4)
    fresh = SpectralReg(0.05, warm_iters=2, seed=5).attach(m2)
    assert torch.equal(opt4.spectral.attach(m2).state, fresh.state) and float(fresh.sigma.min()) > 0
    load_checkpoint(path, m2, AdamW(m2, lr=LR))


def test_the_penalty_alone_lowers_the_sum_of_the_norms():
    """A zero data gradient and lam = 1: ten Adam steps move the weights against v' u'^T only. The claim is the direction."""
    m, opt = _make(rule='adam', lam=1.0, warm=10)
    sr = opt.spectral.attach(m)
    sums = []
    for _ in range(10):
        opt.zero_grad()
        opt.step()                                             # (runs the spectral step itself: nobody else has)
        sums.append(float(sr.sr_sum))
    print('sr_sum over ten penalty-only Adam steps: %s' % ' '.join('%.5g' % s for s in sums))
    assert all(math.isfinite(s) for s in sums) and sums[-1] < sums[0]
    assert int(opt.step_count.item()) == 10 and not sr.open


def _boosted(cfg, sd):
    """The golden weights with the first singular direction of every convolution weight doubled: default-initialised convolutions lie close
    to the Marchenko-Pastur edge, where power iteration converges slowly and a reference that separates sigma_1 is hard to state."""
    import lvae_amd  # noqa: F401
    from lvae_amd.lib.nn import Conv2dParams
    from lvae_amd.models.lvae import LadderVAE
    out = dict(sd)
    for k, mod in LadderVAE(**cfg).named_modules():
        if isinstance(mod, Conv2dParams):
            w = R.out_first(sd[k + '.weight'].double(), mod.transposed)
            U, S, Vh = torch.linalg.svd(w.reshape(w.shape[0], -1), full_matrices=False)
            S[0] *= 2
            out[k + '.weight'] = R.out_first(((U * S) @ Vh).reshape(w.shape), mod.transposed).float().contiguous()
    return out


def test_offline_norms_agree_with_svdvals():
    """spectral_norms(model, 50) against torch.linalg.svdvals of each logical weight, for the weights with sigma_2 / sigma_1 <= 0.9 (the
    others converge too slowly for 50 iterations to say anything); r32 is the 50-step float32 chain on the CPU from the same start."""
    from lvae_amd.lib.nn import Conv2dParams
    from lvae_amd.spectral import initial_u, spectral_norms
    m, _ = _make(lam=None, boost=True)
    arena = m.pack()
    named = dict(m.named_parameters())
    convs = {k + '.weight': mod for k, mod in m.named_modules() if isinstance(mod, Conv2dParams)}
    names = [n for n in arena.names if n in convs]
    jobs, left_out = [], 0
    for i, name in enumerate(names):
        w, tr = named[name].detach().cpu().clone(), convs[name].transposed
        sv = torch.linalg.svdvals(R.out_first(w.double(), tr).reshape(convs[name].c_out, -1))
        if sv.numel() > 1 and float(sv[1] / sv[0]) > 0.9:
            left_out += 1
            continue
        u0 = initial_u(17, i, convs[name].c_out)
        jobs.append((name, sv[0], R.steps(w, u0, 50, tr)['sigma'], R.steps(w.double(), u0.double(), 50, tr)['sigma_abs']))
    print('%d of %d convolution weights left out (sigma_2 / sigma_1 > 0.9)' % (left_out, len(names)))
    assert 2 * left_out <= len(names)                          # a condition of the test, met by the reference alone
    got = spectral_norms(m, 50, seed=17)
    assert list(got) == names
    for name, sv, r32, abs_terms in jobs:
        R.close_sum('spectral_norms %s' % name, torch.tensor([got[name]]), sv, r32, abs_terms)
