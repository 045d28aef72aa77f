"""Adam / AdamW on the flat arena (lvae_adam_step_f32, optim.Adam, optim.AdamW, --optimizer).

References: torch.optim.Adam and torch.optim.AdamW on the CPU with foreach=False, r64 in float64 and r32 in float32 from the same start and
gradients. Rule of docs/ELEMENTWISE_PARITY.md for p, exp_avg and exp_avg_sq: |kernel - r64| <= 2 max|r32 - r64| + 1e-5 |r64| + 1e-6. The one
sharper bound (the bias corrections) is derived at its test. Every comparison prints a `yardstick | ...` line before it asserts."""
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_ema_gpu import _fresh_table, _images, _model

pytestmark = pytest.mark.gpu

LR0, B1, B2, EPS = 2e-3, 0.9, 0.999, 1e-8
KINDS = [('adam', 0.0), ('adam', 1e-2), ('adamw', 1e-2)]
KIND_IDS = ['adam', 'adam-l2', 'adamw']
EINVAL, EALIGN = -1, -2


def _K():
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels as K
    return K


def _ref(kind, p0, grads, wd, dtype, lr=LR0, lrs=None, step0=0, m0=None, v0=None):
    """torch.optim.Adam / AdamW (single-tensor loop) over `grads` from p0 -> (p, exp_avg, exp_avg_sq). `lrs`: the lr of each step;
    step0, m0, v0: the state to start from (torch keeps it in state['step'], state['exp_avg'], state['exp_avg_sq'])."""
    p = p0.clone().to(dtype).requires_grad_(True)
    cls = torch.optim.AdamW if kind == 'adamw' else torch.optim.Adam
    opt = cls([p], lr=lr, betas=(B1, B2), eps=EPS, weight_decay=wd, foreach=False)
    if step0 or m0 is not None:
        zero = torch.zeros_like(p)
        opt.state[p] = {'step': torch.tensor(float(step0)), 'exp_avg': zero.clone() if m0 is None else m0.clone().to(dtype),
                        'exp_avg_sq': zero.clone() if v0 is None else v0.clone().to(dtype)}
    for k, g in enumerate(grads):
        if lrs is not None:
            opt.param_groups[0]['lr'] = lrs[k]
        p.grad = g.clone().to(dtype)
        opt.step()
    st = opt.state[p]
    assert float(st['step']) == step0 + len(grads)
    return p.detach(), st['exp_avg'].clone(), st['exp_avg_sq'].clone()


def _use_of_bound(got, r64, r32, where=None):
    """max over the elements of |got - r64| / (2 max|r32 - r64| + 1e-5 |r64| + 1e-6), the project's rule; `where`: a mask of the elements to
    look at (those finite in all three)."""
    got, r32 = got.detach().cpu().double(), r32.double()
    if where is None:
        where = torch.ones_like(r64, dtype=torch.bool)
    assert bool(where.any())
    spread = float((r32 - r64)[where].abs().max())
    bound = 2.0 * spread + 1e-5 * r64.abs() + 1e-6
    return float(((got - r64).abs() / bound)[where].max())


def _check(what, got3, r64, r32, where=None):
    for name, got, a, b in zip(('p', 'exp_avg', 'exp_avg_sq'), got3, r64, r32):
        use = _use_of_bound(got, a, b, where)
        print('yardstick | %s | %s | use of the bound 2 max|r32 - r64| + 1e-5 |r64| + 1e-6: %.3f' % (what, name, use))
        assert use <= 1.0, (what, name, use)


class _Dev:
    """p, exp_avg, exp_avg_sq and the step counter of one kernel-level run on the device"""

    def __init__(self, p0, m0=None, v0=None, step0=0, ema=None):
        self.p = p0.clone().cuda()
        self.m = torch.zeros_like(self.p) if m0 is None else m0.clone().cuda()
        self.v = torch.zeros_like(self.p) if v0 is None else v0.clone().cuda()
        self.step = torch.full((1,), step0, dtype=torch.int64, device='cuda')
        self.ema = None if ema is None else ema.clone().cuda()

    def run(self, g, kind='adam', wd=0.0, lr=LR0, sched=None, mask=None, gscale=None, decay=0.0, lr_out=None, state=None, advance=True):
        K = _K()
        K.adam_step(self.p, g.cuda(), self.m, self.v, mask, lr, sched, B1, B2, EPS, wd, kind == 'adamw', gscale, self.step, self.ema, decay,
                    lr_out, state)
        if advance:
            K.counter_advance(self.step)
        return self

    def all(self):
        return (self.p, self.m, self.v) + (() if self.ema is None else (self.ema,))


def _same_bits(a, b):
    for x, y in zip(a.all(), b.all()):
        assert torch.equal(x, y)


def _guard_state(scale, skip):
    st = torch.zeros(4, dtype=torch.int64, device='cuda')     # struct lvae_grad_guard_state
    st.view(torch.float32)[1] = scale
    st.view(torch.int32)[2] = skip
    return st


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------------------------------------
# n = 4: one vector; 4 * 12347: a ragged end of the grid-stride loop; 2 101 252: above grid_for's cap of 2048 blocks x 256 threads x 4
# elements, so a second sweep (once)
@pytest.mark.parametrize('kind,wd,n', [(k, w, n) for (k, w) in KINDS for n in (4, 4 * 12347)] + [('adamw', 1e-2, 2101252)],
                         ids=['%s-%d' % (i, n) for i in KIND_IDS for n in (4, 4 * 12347)] + ['adamw-2101252'])
def test_eight_steps_match_torch(kind, wd, n):
    gen = torch.Generator().manual_seed(11)
    p0, grads = torch.randn(n, generator=gen), [torch.randn(n, generator=gen) for _ in range(8)]
    d = _Dev(p0)
    for g in grads:
        d.run(g, kind, wd)
    torch.cuda.synchronize()
    assert int(d.step.item()) == 8
    _check('8 steps, %s wd %g, n %d' % (kind, wd, n), d.all(), _ref(kind, p0, grads, wd, torch.float64), _ref(kind, p0, grads, wd, torch.float32))


@pytest.mark.parametrize('step0', [0, 9, 999])
def test_bias_corrections_are_formed_in_double(step0):
    """One step from p = m = v = 0 with the counter preset: p = -step_size * m / (sqrt(v) / rs + eps) is then a product of the bias
    corrections and a quotient near +-1 (|g| in [0.5, 2], so eps = 1e-8 does not matter), and its relative error shows how 1 - beta^t was
    formed. Bound: 2 max rel|r32 - r64| + 2^-23, torch's own float32 error twice over plus one float spacing, about 7e-7. A kernel that
    forms 1 - beta^t in fp32 sits at 4e-6 to 7e-6 (1 - 0.999f alone misses 1 - 0.999 by 1.3e-5 relative) and fails."""
    n = 4096
    gen = torch.Generator().manual_seed(23 + step0)
    g = (0.5 + 1.5 * torch.rand(n, generator=gen)) * (2.0 * torch.randint(0, 2, (n,), generator=gen) - 1.0)
    p0 = torch.zeros(n)
    d = _Dev(p0, step0=step0).run(g)
    r64, r32 = _ref('adam', p0, [g], 0.0, torch.float64, step0=step0)[0], _ref('adam', p0, [g], 0.0, torch.float32, step0=step0)[0]
    assert float(r64.abs().min()) > 0.0
    rel = float(((d.p.cpu().double() - r64).abs() / r64.abs()).max())
    rel32 = float(((r32.double() - r64).abs() / r64.abs()).max())
    bound = 2.0 * rel32 + 2.0 ** -23
    print('yardstick | first update, counter %d | p | max relative error %.3e, torch float32 %.3e, bound %.3e' % (step0, rel, rel32, bound))
    assert int(d.step.item()) == step0 + 1
    assert rel <= bound, (rel, bound)


@pytest.mark.parametrize('kind,wd', [('adam', 0.0), ('adamw', 1e-2)], ids=['adam', 'adamw'])
@pytest.mark.parametrize('case', ['zero', 'huge', 'overflow', 'tiny', 'nan'])
def test_edge_values(case, kind, wd):
    """One step each on a gradient of zeros, of 1e20, of 1e25, of 1e-30 (its square is 0) and with a single NaN: the pattern of NaN and Inf
    is torch float32's, and the finite elements meet the rule. The square of 1e20 is Inf in fp32, but torch float32 forms
    ((1 - beta2) * g) * g = 1e17 * 1e20 = 1e37, which is finite, and so does the kernel: v stays finite and p moves by lr. At 1e25 the same
    product is Inf: v = Inf, m / Inf = 0 and p is left to the decay alone, as torch float32 gives."""
    n = 4 * 300
    gen = torch.Generator().manual_seed(31)
    p0 = torch.randn(n, generator=gen)
    g = {'zero': torch.zeros(n), 'huge': torch.full((n,), 1e20), 'overflow': torch.full((n,), 1e25),
         'tiny': torch.full((n,), 1e-30), 'nan': torch.randn(n, generator=gen)}[case]
    if case == 'nan':
        g[517] = math.nan
    d = _Dev(p0).run(g, kind, wd)
    got = [t.cpu() for t in d.all()]
    r64, r32 = _ref(kind, p0, [g], wd, torch.float64), _ref(kind, p0, [g], wd, torch.float32)
    finite = torch.ones(n, dtype=torch.bool)
    for name, x, b, a in zip('pmv', got, r32, r64):
        assert torch.equal(torch.isnan(x), torch.isnan(b)) and torch.equal(torch.isinf(x), torch.isinf(b)), name
        finite &= torch.isfinite(x) & torch.isfinite(b) & torch.isfinite(a)
    p, m, v = got
    if case == 'zero':
        keep = np.float32(1.0 - float(np.float32(LR0)) * float(np.float32(wd)))       # 1 without decay
        assert torch.equal(p, p0 * float(keep)) and (wd == 0.0 or not torch.equal(p, p0))
        assert not m.any() and not v.any()
    elif case == 'huge':
        assert bool(torch.isfinite(v).all()) and float(v.min()) > 9e36 and bool(torch.isfinite(p).all()) and not torch.equal(p, p0)
    elif case == 'overflow':
        assert bool(torch.isinf(v).all()) and bool(torch.isfinite(m).all())
        assert torch.equal(p, r32[0]) and (wd != 0.0 or torch.equal(p, p0))           # m / Inf = 0: only the decay moves p
        finite = torch.isfinite(r32[2])                                               # (none: nothing left for the rule in v)
    elif case == 'tiny':
        assert not v.any() and bool((m > 0).all())
    else:
        for x in got:
            assert bool(torch.isnan(x[517])) and int(torch.isnan(x).sum()) == 1
    if bool(finite.any()):
        _check('edge %s, %s' % (case, kind), got, r64, r32, finite)


@pytest.mark.parametrize('kind,wd', [('adam', 1e-2), ('adamw', 1e-2)], ids=['l2', 'decoupled'])
def test_frozen_elements_keep_their_bits(kind, wd):
    n = 4 * 12347
    gen = torch.Generator().manual_seed(41)
    p0, m0, v0, e0 = (torch.randn(n, generator=gen), torch.randn(n, generator=gen), torch.rand(n, generator=gen),
                      torch.randn(n, generator=gen))
    mask = (torch.rand(n, generator=gen) > 0.3).float()
    d = _Dev(p0, m0, v0, step0=3, ema=e0).run(torch.randn(n, generator=gen), kind, wd, mask=mask.cuda(), decay=0.9)
    frozen = mask == 0
    assert 1000 < int(frozen.sum()) < n - 1000
    for x, x0 in zip(d.all(), (p0, m0, v0, e0)):
        x = x.cpu()
        assert torch.equal(x[frozen], x0[frozen])
        assert float((x[~frozen] != x0[~frozen]).float().mean()) > 0.99     # (an update below one float spacing leaves an element as it was)


@pytest.mark.parametrize('kind,wd', KINDS, ids=KIND_IDS)
def test_exact_identities(kind, wd):
    """gscale, a constant schedule, the average, and the guard: each against the plain call, bit for bit, over three steps."""
    from lvae_amd.optim import ema_decay_at
    K = _K()
    n = 4 * 12347
    gen = torch.Generator().manual_seed(43)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) for _ in range(3)]
    plain = _Dev(p0)
    for g in grads:
        plain.run(g, kind, wd)
    assert not torch.equal(plain.p, p0.cuda())

    # gscale = 0.5 is the call on the gradient halved beforehand (the halving is exact); under adamw the decay is not scaled
    half, scaled = _Dev(p0), _Dev(p0)
    gs = torch.tensor([0.5]).cuda()
    for g in grads:
        half.run(g * 0.5, kind, wd)
        scaled.run(g, kind, wd, gscale=gs)
    _same_bits(half, scaled)
    assert not torch.equal(half.p, plain.p)

    # a constant schedule without warm-up is the call with lr = base_lr, and lr_out holds it
    sched, lr_out = K.lr_schedule_struct(LR0, 'constant', 0, 0, 0.0, 0.1), torch.zeros(1).cuda()
    sc = _Dev(p0)
    for g in grads:
        sc.run(g, kind, wd, lr=123.0, sched=sched, lr_out=lr_out)       # (`lr` is ignored under a schedule)
    _same_bits(plain, sc)
    assert lr_out.item() == np.float32(LR0)
    # lr_out without a schedule: the rate applied
    lr_out.zero_()
    _Dev(p0).run(grads[0], kind, wd, lr_out=lr_out)
    assert lr_out.item() == np.float32(LR0)

    # with the average: p, m, v are those of the call without it, and the average follows the ramp of ema_decay_at, one fp32 rounding
    # per operation (e + (p_new - e) * (1 - d))
    e0 = p0 + 1.0
    av = _Dev(p0, ema=e0)
    want = e0.clone()
    for k, g in enumerate(grads):
        av.run(g, kind, wd, decay=0.75)
        w = np.float32(1.0) - ema_decay_at(0.75, k)
        want = want + (av.p.cpu() - want) * float(w)
        assert torch.equal(av.ema.cpu(), want), k
    assert torch.equal(av.p, plain.p) and torch.equal(av.m, plain.m) and torch.equal(av.v, plain.v)
    assert float(ema_decay_at(0.75, 0)) == float(np.float32(0.1)) and not torch.equal(av.ema.cpu(), e0)

    # guard.skip = 1: every buffer and lr_out keep their bits
    sk = _Dev(p0, torch.randn(n, generator=gen), torch.rand(n, generator=gen), step0=5, ema=e0)
    before = [t.clone() for t in sk.all()]
    lr_out.fill_(7.0)
    for s in (None, sched):
        sk.run(grads[0], kind, wd, sched=s, decay=0.75, lr_out=lr_out, state=_guard_state(0.5, 1), advance=False)
    torch.cuda.synchronize()
    for x, x0 in zip(sk.all(), before):
        assert torch.equal(x, x0)
    assert lr_out.item() == 7.0

    # skip = 0 and scale = s: the unguarded call with gscale -> s
    s = 0.3125
    guarded, un = _Dev(p0, ema=e0), _Dev(p0, ema=e0)
    st, gs = _guard_state(s, 0), torch.tensor([s]).cuda()
    for g in grads:
        guarded.run(g, kind, wd, sched=sched, decay=0.75, lr_out=lr_out, state=st)
        un.run(g, kind, wd, sched=sched, decay=0.75, gscale=gs)
    _same_bits(guarded, un)
    assert lr_out.item() == np.float32(LR0) and not torch.equal(guarded.p, plain.p)


def test_guard_scale_leaves_the_decoupled_decay_unscaled():
    """AdamW under a guard that clips by four: torch.optim.AdamW on the clipped gradient, whose decay is lr * wd whatever the gradient."""
    n, wd, s = 4 * 12347, 1e-2, 0.25
    gen = torch.Generator().manual_seed(47)
    p0, grads = torch.randn(n, generator=gen), [torch.randn(n, generator=gen) for _ in range(8)]
    d, st = _Dev(p0), _guard_state(s, 0)
    for g in grads:
        d.run(g, 'adamw', wd, state=st)
    clipped = [g * s for g in grads]
    r64, r32 = _ref('adamw', p0, clipped, wd, torch.float64), _ref('adamw', p0, clipped, wd, torch.float32)
    _check('adamw, guard scale 0.25', d.all(), r64, r32)
    # the comparison sees the difference: a decay scaled with the gradient (wd / 4) is outside the rule
    other = _ref('adamw', p0, clipped, wd * s, torch.float64)
    assert _use_of_bound(other[0], r64[0], r32[0]) > 10.0


@pytest.mark.parametrize('kind,wd', [('adam', 1e-2), ('adamw', 1e-2)], ids=['adam-l2', 'adamw'])
def test_kernel_follows_the_schedule_against_torch(kind, wd):
    """torch on the CPU with its lr set to LrSchedule.at before every step against the scheduled kernel: warm-up over 3 steps, then a cosine
    that reaches base / 10 four steps later. The constant-rate kernel, run beside it, misses the same reference by more than 100 bounds."""
    from lvae_amd.optim import LrSchedule
    base, steps, n = LR0, 8, 4100
    sched = LrSchedule('cosine', warmup_steps=3, decay_steps=4, min_lr=base / 10)
    lrs = [sched.at(base, k) for k in range(steps)]
    assert lrs[2] == np.float32(base) == lrs[3] and lrs[7] == np.float32(base / 10) and max(lrs) / min(lrs) > 9.9
    gen = torch.Generator().manual_seed(10)
    p0, grads = torch.randn(n, generator=gen), [torch.randn(n, generator=gen) for _ in range(steps)]
    sd, cd, st, lr_out = _Dev(p0), _Dev(p0), sched.struct(base), torch.zeros(1).cuda()
    for k, g in enumerate(grads):
        sd.run(g, kind, wd, sched=st, lr_out=lr_out)
        cd.run(g, kind, wd, lr=base)
        assert abs(lr_out.item() - lrs[k]) <= float(np.spacing(np.float32(lrs[k])))
    r64, r32 = _ref(kind, p0, grads, wd, torch.float64, lrs=lrs), _ref(kind, p0, grads, wd, torch.float32, lrs=lrs)
    const = _use_of_bound(cd.p, r64[0], r32[0])
    print('yardstick | schedule, %s | p of the constant-rate run | use of the bound %.1f' % (kind, const))
    assert const > 100.0
    _check('warm-up + cosine, %s' % kind, sd.all(), r64, r32)


def test_argument_checks_return_their_codes():
    import lvae_amd  # noqa: F401
    from lvae_amd import _C
    fn = _C.load().lvae_adam_step_f32
    n = 16
    p, g, m, v, e = (torch.zeros(n + 4, device='cuda') for _ in range(5))
    step, gs, st = torch.zeros(1, dtype=torch.int64, device='cuda'), torch.ones(1, device='cuda'), _guard_state(1.0, 0)
    stream = _C.stream_ptr()

    def rc(n=n, b1=B1, b2=B2, eps=EPS, wd=0.0, gscale=None, ema=None, decay=0.0, state=None, sched=None):
        return fn(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), None, n, LR0, sched, b1, b2, eps, wd, 0, gscale, step.data_ptr(),
                  ema, decay, None, state, stream)

    assert rc() == 0
    assert rc(gscale=gs.data_ptr(), state=st.data_ptr()) == EINVAL          # both guard and gscale
    assert rc(gscale=gs.data_ptr()) == 0 and rc(state=st.data_ptr()) == 0
    assert rc(n=6) == EALIGN and rc(n=0) == EINVAL
    assert rc(b2=1.0) == EINVAL and rc(b1=1.0) == EINVAL and rc(b1=-0.1) == EINVAL and rc(b2=math.nan) == EINVAL
    assert rc(eps=-1e-8) == EINVAL and rc(wd=-1e-2) == EINVAL and rc(eps=0.0) == 0
    assert rc(ema=e.data_ptr(), decay=1.0) == EINVAL and rc(ema=e.data_ptr(), decay=-0.1) == EINVAL
    assert rc(ema=e.data_ptr(), decay=0.5) == 0
    assert rc(ema=e.data_ptr() + 4, decay=0.5) == EALIGN                    # a misaligned ema
    assert rc(state=st.data_ptr() + 4) == EALIGN
    bad = _C.LrScheduleStruct(0.0, 0.0, 0.1, 0, 0, 0)                         # base_lr = 0
    assert rc(sched=ctypes.byref(bad)) == EINVAL
    torch.cuda.synchronize()
    assert b'lvae_adam_step_f32' in _C.load().lvae_last_error()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the whole step (the tiny_cifar golden, batch 4; two eager steps, the capture, four replays)
# ---------------------------------------------------------------------------------------------------------------------------------
W, T = 2, 3
STEPS = W + T + 2
LR = 1e-3
GUARD = dict(max_norm=100.0, skip_threshold=math.inf)
_runs = {}


def _schedule():
    from lvae_amd.optim import LrSchedule
    return LrSchedule('cosine', warmup_steps=W, decay_steps=T, min_lr=LR / 10)


def _xs():
    return [_images(4, 80 + k) for k in range(STEPS)]


def _make(rule, full):
    """the small model and an optimizer of `rule` ('adamax', 'adam', 'adamw'): plain, or `full` with average + schedule + guard together"""
    from lvae_amd import optim
    from lvae_amd.noise import PhiloxNoise
    g = load_golden('tiny_cifar')
    _fresh_table()
    m = _model(g.cfg, g.state_dict(), PhiloxNoise(seed=3))
    cls = {'adamax': optim.Adamax, 'adam': optim.Adam, 'adamw': optim.AdamW}[rule]
    extra = dict(ema_decay=0.99, schedule=_schedule(), guard=optim.GradGuard(**GUARD)) if full else {}
    return m, cls(m, lr=LR, weight_decay=1e-2, **extra)


def _steps(m, opt, xs, use_graph, names=None):
    """runs the steps; with `names`, also records the name of every C-ABI call the Python passes make"""
    from lvae_amd import _C
    from lvae_amd import kernels as K
    from lvae_amd.engine import TrainStep
    real = _C.call

    def counted(name, *args):
        names.append(name)
        return real(name, *args)

    if names is not None:
        _C.call = K.call = counted
    try:
        st = TrainStep(m, opt, use_graph=use_graph)
        outs = [{k: v.detach().clone() for k, v in st(x.cuda()).items()} for x in xs]
        torch.cuda.synchronize()
    finally:
        _C.call = K.call = real
    assert (st.graph_a is not None) == (use_graph and len(xs) > 2)
    return outs


def _state(m, opt):
    from lvae_amd.optim import RULES
    sd = m.state_dict()   # (flushes the host-counted num_batches_tracked)
    st = {k: v.detach().clone() for k, v in sd.items() if not k.endswith(('weight', 'bias', 'top_prior_params'))}
    st.update(params=m.arena.params.detach().clone(), exp_avg=opt.exp_avg.clone(), second=getattr(opt, RULES[opt.rule]).clone(),
              step=opt.step_count.clone())
    if opt.ema is not None:
        st['ema'] = opt.ema.clone()
    if opt.lr_now is not None:
        st['lr_now'] = opt.lr_now.clone()
    if opt.guard is not None:
        st['guard_counts'] = torch.tensor(opt.guard.counts())
    return st


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _run(rule, full, use_graph):
    key = (rule, full, use_graph)
    if key not in _runs:
        m, opt = _make(rule, full)
        names = []
        outs = _steps(m, opt, _xs(), use_graph, names)
        assert int(opt.step_count.item()) == STEPS
        _runs[key] = {'outs': outs, 'state': _state(m, opt), 'calls': names, 'lr': opt.current_lr()}
    return _runs[key]


@pytest.mark.parametrize('full', [False, True], ids=['plain', 'ema+schedule+guard'])
@pytest.mark.parametrize('rule', ['adam', 'adamw'])
def test_captured_step_equals_eager_steps(rule, full):
    graph, eager = _run(rule, full, True), _run(rule, full, False)
    _assert_same(graph['state'], eager['state'])
    for a, b in zip(graph['outs'], eager['outs']):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    assert ('ema' in graph['state']) == ('lr_now' in graph['state']) == ('guard_counts' in graph['state']) == full
    if full:   # the last step ran at the floor of the schedule: the replayed graph did not keep the lr it was captured with
        want = _schedule().at(LR, STEPS - 1)
        assert want == np.float32(LR / 10) and abs(graph['lr'] - want) <= float(np.spacing(np.float32(want)))
    else:
        assert graph['lr'] == LR
    # the two rules differ in the decay alone, and they do differ; neither is Adamax
    other = _run('adamw' if rule == 'adam' else 'adam', full, True)
    assert not torch.equal(graph['state']['params'], other['state']['params'])
    assert torch.equal(graph['outs'][0]['loss'], other['outs'][0]['loss'])


@pytest.mark.parametrize('rule', ['adam', 'adamw'])
def test_one_eager_step_against_torch(rule):
    """The gradient and the parameters as they stand immediately before the update, then float64 torch on those vectors, by the rule."""
    m, opt = _make(rule, False)
    seen = {}
    update = opt._update

    def spy(arena, guard_state):
        seen['g'], seen['p'] = arena.grads.detach().cpu().clone(), arena.params[:arena.n_train].detach().cpu().clone()
        return update(arena, guard_state)

    opt._update = spy
    _steps(m, opt, _xs()[:1], False)
    arena = m.arena
    assert seen['g'].numel() == seen['p'].numel() == arena.n_train and float(seen['g'].abs().max()) > 0.0
    got = (arena.params[:arena.n_train], opt.exp_avg, opt.exp_avg_sq)
    r64, r32 = (_ref(rule, seen['p'], [seen['g']], 1e-2, dt, lr=LR) for dt in (torch.float64, torch.float32))
    assert not torch.equal(got[0].cpu(), seen['p'])
    _check('one eager step of the model, %s' % rule, got, r64, r32)


def test_resume_in_the_middle_is_exact_and_rules_do_not_mix(tmp_path):
    from lvae_amd.checkpoint import load_checkpoint, optimizer_state_by_name, rule_warning, save_checkpoint
    from lvae_amd.models.lvae import LadderVAE
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adam, AdamW, Adamax, GradGuard
    straight = _run('adamw', True, True)
    g = load_golden('tiny_cifar')
    xs = _xs()
    m1, opt1 = _make('adamw', True)
    first = _steps(m1, opt1, xs[:3], True)                 # two eager steps and the capture: in the middle of the decay
    path = str(tmp_path / 'model_3.pt')
    save_checkpoint(path, m1, opt1)
    ck = torch.load(path)
    assert ck['optimizer']['rule'] == 'adamw' and ck['optimizer']['step'] == 3
    named = dict(m1.named_parameters())
    assert set(ck['optimizer']['state']) == {k for k, p in named.items() if p.requires_grad}
    for name, st in ck['optimizer']['state'].items():      # torch's own key names, the parameters' logical shapes
        assert set(st) == {'exp_avg', 'exp_avg_sq'}
        assert st['exp_avg'].shape == st['exp_avg_sq'].shape == named[name].shape and bool((st['exp_avg_sq'] >= 0).all())
    sd = opt1.state_dict()
    assert sd['rule'] == 'adamw' and sd['exp_avg_sq'] is opt1.exp_avg_sq and 'exp_inf' not in sd
    del m1, opt1

    def other_model():
        _fresh_table()
        torch.manual_seed(123)
        m = LadderVAE(**g.cfg).cuda().train()              # other weights and another noise seed: all of it comes from the file
        m.noise = PhiloxNoise(seed=999)
        return m

    m2 = other_model()
    opt2 = AdamW(m2, lr=LR, weight_decay=1e-2, ema_decay=0.99, schedule=_schedule(), guard=GradGuard(**GUARD))
    assert rule_warning(path, load_checkpoint(path, m2, opt2), opt2) is None
    rest = _steps(m2, opt2, xs[3:], True)
    for a, b in zip(straight['outs'], first + rest):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    _assert_same(straight['state'], _state(m2, opt2))

    # adamw -> adam loads (the state is the same) and has a warning line to print; the optimizer's own rule is the one that runs
    opt3 = Adam(m2, lr=LR)
    line = rule_warning(path, load_checkpoint(path, m2, opt3), opt3)
    assert line.startswith('warning: ') and 'adamw' in line and line.endswith('continuing with adam') and '\n' not in line
    assert opt3.rule == 'adam' and int(opt3.step_count.item()) == 3 and float(opt3.exp_avg_sq.max()) > 0.0
    opt3.load_state_dict(sd)
    # a file written under adamw is refused by Adamax, before anything is loaded
    m3 = other_model()
    opt4 = Adamax(m3, lr=LR)
    opt4._state()
    before = m3.arena.params.clone()
    with pytest.raises(ValueError) as e:
        load_checkpoint(path, m3, opt4)
    assert 'adamw' in str(e.value) and 'adamax' in str(e.value) and 'exp_inf' in str(e.value) and 'exp_avg_sq' in str(e.value)
    assert not opt4.exp_inf.any() and torch.equal(m3.arena.params, before)
    with pytest.raises(ValueError):
        opt4.load_state_dict(sd)
    # and the reverse: an Adamax file by Adam; an old file, without 'rule', is an Adamax file
    load_checkpoint(path, m3, None)                        # (weights alone still load)
    _steps(m3, opt4, xs[:1], False)
    apath, old = str(tmp_path / 'adamax.pt'), str(tmp_path / 'old.pt')
    save_checkpoint(apath, m3, opt4)
    ack = torch.load(apath)
    assert ack['optimizer']['rule'] == 'adamax' and set(next(iter(ack['optimizer']['state'].values()))) == {'exp_avg', 'exp_inf'}
    ack['optimizer'] = {k: v for k, v in ack['optimizer'].items() if k != 'rule'}
    torch.save(ack, old)
    for file in (apath, old):
        for cls in (Adam, AdamW):
            with pytest.raises(ValueError) as e:
                load_checkpoint(file, m3, cls(m3, lr=LR))
            assert 'adamax' in str(e.value) and cls(None).rule in str(e.value)
        opt5 = Adamax(m3, lr=LR)
        assert rule_warning(file, load_checkpoint(file, m3, opt5), opt5) is None
        assert int(opt5.step_count.item()) == 1
        mine, its = optimizer_state_by_name(m3, opt5)['state'], optimizer_state_by_name(m3, opt4)['state']
        for name in its:
            assert torch.equal(mine[name]['exp_inf'], its[name]['exp_inf']) and torch.equal(mine[name]['exp_avg'], its[name]['exp_avg'])
            assert float(its[name]['exp_inf'].min()) > 0.0
    _fresh_table()


def test_default_path_issues_the_launches_it_issued():
    """With Adamax the step does not reach the new entry point; with Adam it issues the same calls in the same order, the new entry point in
    the place of the Adamax one, and no call more: plain, and with average + schedule + guard."""
    adamax, adam = _run('adamax', False, True)['calls'], _run('adam', False, True)['calls']
    assert 'lvae_adam_step_f32' not in adamax
    assert adamax.count('lvae_adamax_step_f32') == 3       # the two eager steps and the capture go through Python; replays do not
    assert adam.count('lvae_adam_step_f32') == 3 and not [n for n in adam if 'adamax' in n]
    assert [n.replace('lvae_adam_step_f32', 'lvae_adamax_step_f32') for n in adam] == adamax
    adamax, adamw = _run('adamax', True, True)['calls'], _run('adamw', True, True)['calls']
    assert 'lvae_adam_step_f32' not in adamax and adamax.count('lvae_adamax_guarded_step_f32') == 3
    assert [n.replace('lvae_adam_step_f32', 'lvae_adamax_guarded_step_f32') for n in adamw] == adamax


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the trainer
# ---------------------------------------------------------------------------------------------------------------------------------
def test_trainer_runs_adamw(tmp_path, capsys):
    import re
    from lvae_amd import main as lmain
    _fresh_table()
    ck = str(tmp_path / 'end.pt')
    argv = ['-d', 'cifar10', '--zdims', '8', '8', '--downsample', '1', '1', '--nfilters', '16', '--skip', '--gated', '--freebits', '1.0',
            '--batch-size', '8', '--synthetic', '--seed', '3', '--steps', '6', '--log-every', '2', '--save-checkpoint', ck, '--lr', '1e-3',
            '--optimizer', 'adamw', '--wd', '0.01', '--betas', '0.9', '0.9', '--lr-warmup', '2', '--max-grad-norm', '100']
    lmain.main(argv)
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if re.search(r'\[step \d+\]', ln)]
    assert len(lines) == 3 and all('[step %d]' % s in ln for ln, s in zip(lines, (2, 4, 6))), out
    descr = [ln for ln in out.splitlines() if ln.startswith('cifar10,')]
    assert len(descr) == 1 and ',adamw,' in descr[0] and ',b0.9-0.9' in descr[0] and ',wd=0.01,' in descr[0], out
    saved = torch.load(ck)
    assert saved['optimizer']['rule'] == 'adamw' and saved['optimizer']['step'] == 6
    assert saved['optimizer']['betas'] == (0.9, 0.9) and saved['optimizer']['weight_decay'] == 0.01
    assert set(next(iter(saved['optimizer']['state'].values()))) == {'exp_avg', 'exp_avg_sq'}
    _fresh_table()
