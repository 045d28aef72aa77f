"""The gradient guard: the decision kernel against float64 statements and lvae_l2norm_f32, the guarded Adamax against the unguarded entry
points (bitwise) and on a skipped step, the flagged multi-copy, and whole steps: an idle guard changes no bit, a clipped step follows
float64 Adamax on the clipped gradient, a skipped step leaves model and optimizer as if it had not happened, eagerly and captured, across
a resume, in both exchange forms and in the trainer."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from test_ema_gpu import _assert_same_state, _fresh_table, _images, _model, _train_state

pytestmark = pytest.mark.gpu

U = 2.0 ** -24   # unit roundoff of fp32


def _K():
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels as K
    return K


def _new_state():
    return torch.zeros(4, dtype=torch.int64, device='cuda')


def _read(state):
    torch.cuda.synchronize()
    f, i = state.view(torch.float32).cpu().numpy(), state.view(torch.int32).cpu()
    return {'norm': f[0], 'scale': f[1], 'skip': int(i[2]), 'clipped': int(state[2]), 'skipped': int(state[3])}


def _guard(g, gscale=None, G=0.0, T=-1.0, state=None):
    K = _K()
    state = _new_state() if state is None else state
    gs = None if gscale is None else torch.tensor([gscale], dtype=torch.float32, device='cuda')
    K.grad_guard(g.cuda(), gs, G, T, state)
    return _read(state)


def _bits(x):
    return np.float32(x).view(np.int32).item()


def _ulps(a, b):
    return abs(_bits(a) - _bits(b))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the decision
# ---------------------------------------------------------------------------------------------------------------------------------
CAP = 256 * 8                      # grid_for's cap on the number of blocks
SIZES = {'one-block': 1000, 'two-blocks': 8 * 256 + 5, 'grid-stride': CAP * 256 + 1031}


@pytest.mark.parametrize('gscale', [None, 0.5], ids=['gscale-null', 'gscale-half'])
@pytest.mark.parametrize('size', list(SIZES))
def test_norm_is_l2norms_and_scale_is_the_clip_factor(size, gscale):
    """norm: bitwise lvae_l2norm_f32's, and within the fp32 bound of the float64 norm. With B = min(ceil(n / 2048), 2048) blocks, a term of
    the sum passes through 1 rounding (its square), at most k = ceil(n / (256 B)) additions in its thread, 6 + 3 in its block's reduction,
    ceil(B / 256) + 6 + 3 in the final block: all terms are positive, so the sum's relative error is at most d u / (1 - d u) with
    d = k + ceil(B / 256) + 19, and the square root halves it and adds one rounding. scale: within 1 ulp of
    float32(gscale min(1, G / (e + 1e-6))) stated in float64 on e = float32(norm gscale), the norm Adamax would have applied."""
    K = _K()
    n = SIZES[size]
    blocks = min((n + 2047) // 2048, CAP)
    assert (blocks == 1) == (size == 'one-block') and (blocks == 2) == (size == 'two-blocks')
    assert (n > CAP * 256) == (size == 'grid-stride')       # more elements than one pass of the full grid of 256-thread blocks
    g = torch.randn(n, generator=torch.Generator().manual_seed(n))
    ref = K.l2norm(g.cuda()).cpu().numpy()[0]
    exact = float(g.double().pow(2).sum().sqrt())
    d = math.ceil(n / (256 * blocks)) + math.ceil(blocks / 256) + 19
    bound = (0.5 * d * U / (1 - d * U) + U) * 1.001
    G = 0.5 * exact * (gscale or 1.0)                       # clips by about one half
    r = _guard(g, gscale, G=G)
    print('%s: norm %.9g, float64 %.9g, relative error %.3e (bound %.3e)' % (size, r['norm'], exact, abs(float(r['norm']) - exact) / exact, bound))
    assert _bits(r['norm']) == _bits(ref)
    assert abs(float(r['norm']) - exact) <= bound * exact
    e = float(np.float32(r['norm']) * np.float32(gscale or 1.0))
    want = np.float32((gscale or 1.0) * min(1.0, float(np.float32(G)) / (e + 1e-6)))
    assert _ulps(r['scale'], want) <= 1, (float(r['scale']), float(want))
    assert r['skip'] == 0 and r['clipped'] == 1 and r['skipped'] == 0
    # not reached: the factor is gscale itself, bit for bit
    r = _guard(g, gscale, G=4.0 * G)
    assert float(r['scale']) == (gscale or 1.0) and r['clipped'] == 0 and r['skip'] == 0


def _vec(n, **at):
    g = torch.zeros(n)
    for i, v in at.items():
        g[int(i[1:])] = v
    return g


def test_decision_edges():
    n = 2053
    five = _vec(n, _0=3.0, _2052=4.0)                       # norm 5 exactly
    # all zeros: scale 1, no 0 / 0; T = 0 does not skip a zero gradient
    r = _guard(torch.zeros(n), G=1.0, T=0.0)
    assert float(r['norm']) == 0.0 and float(r['scale']) == 1.0 and r['skip'] == 0 and r['clipped'] == 0
    # norm == G: the factor G / (G + 1e-6) < 1 of clip_grad_norm_, and not counted as clipped
    r = _guard(five, G=5.0)
    assert float(r['norm']) == 5.0 and r['clipped'] == 0 and r['skip'] == 0
    assert _ulps(r['scale'], np.float32(5.0 / (5.0 + 1e-6))) <= 1 and float(r['scale']) < 1.0
    r = _guard(five, G=float(np.nextafter(np.float32(5), np.float32(0))))
    assert r['clipped'] == 1
    # either side of T
    below, above = float(np.nextafter(np.float32(5), np.float32(0))), float(np.nextafter(np.float32(5), np.float32(9)))
    assert _guard(five, T=below)['skip'] == 1 and _guard(five, T=5.0)['skip'] == 0 and _guard(five, T=above)['skip'] == 0
    r = _guard(five, T=below)
    assert r['skipped'] == 1 and r['clipped'] == 0 and float(r['scale']) == 0.0
    # T = 0 skips every non-zero gradient, T = inf none that is finite
    assert _guard(_vec(n, _7=1e-3), T=0.0)['skip'] == 1 and _guard(five * 1e15, T=math.inf)['skip'] == 0
    # gscale enters the decision: e = 2.5
    assert _guard(five, 0.5, T=3.0)['skip'] == 0 and _guard(five, 0.5, T=2.0)['skip'] == 1
    r = _guard(five, 0.5, G=2.5)
    assert r['clipped'] == 0 and _ulps(r['scale'], np.float32(0.5 * 2.5 / (2.5 + 1e-6))) <= 1
    assert _guard(five, 0.5, G=2.0)['clipped'] == 1
    # not finite: always skipped, with every combination of limits
    bad = {'nan-last': _vec(n, _0=1.0, _2052=math.nan), 'inf-first': _vec(n, _0=math.inf, _9=1.0), 'neg-inf-middle': _vec(n, _1026=-math.inf),
           'overflow': torch.full((8,), 1e20)}
    for name, g in bad.items():
        for G, T in ((0.0, -1.0), (1.0, -1.0), (0.0, 1e30), (1.0, math.inf), (math.inf, -1.0)):
            r = _guard(g, G=G, T=T)
            assert r['skip'] == 1 and r['skipped'] == 1 and r['clipped'] == 0 and float(r['scale']) == 0.0, (name, G, T)
    assert math.isinf(float(_guard(bad['overflow'])['norm'])) and math.isnan(float(_guard(bad['nan-last'])['norm']))
    # denormals: their squares vanish, the norm is 0 as lvae_l2norm_f32's, nothing is skipped or clipped
    tiny = torch.full((n,), 1e-40)
    r = _guard(tiny, G=1.0, T=1.0)
    assert _bits(r['norm']) == _bits(_K().l2norm(tiny.cuda()).cpu().numpy()[0]) and float(r['scale']) == 1.0 and r['skip'] == 0
    # clipping off (0, negative, inf, NaN), threshold off, both off: a huge finite gradient passes untouched
    big = five * 1e15
    for G in (0.0, -3.0, math.inf, math.nan):
        r = _guard(big, 0.5, G=G, T=-1.0)
        assert float(r['scale']) == 0.5 and r['skip'] == 0 and r['clipped'] == 0, G
    assert _guard(big, G=1.0, T=-1.0)['skip'] == 0 and _guard(big, G=0.0, T=1.0)['skip'] == 1
    # the counters accumulate
    st = _new_state()
    _guard(five, G=1.0, state=st)
    _guard(bad['nan-last'], G=1.0, state=st)
    _guard(five, G=1.0, T=9.0, state=st)
    r = _guard(five, G=9.0, T=9.0, state=st)
    assert (r['clipped'], r['skipped'], r['skip']) == (2, 1, 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the guarded Adamax, the counter and the copy
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', ['plain', 'ema', 'sched', 'ema+sched'])
@pytest.mark.parametrize('n', [4, 1028])
def test_guarded_adamax_is_bitwise_the_unguarded_one_and_a_skipped_step_is_nothing(n, form):
    K = _K()
    gen = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=gen)
    ema_on, sched_on = 'ema' in form, 'sched' in form
    sched = K.lr_schedule_struct(2e-3, 'cosine', 2, 5, 2e-4, 0.1) if sched_on else None
    pa, pb = p0.cuda(), p0.cuda()
    ma, mb, ua, ub = (torch.zeros(n).cuda() for _ in range(4))
    ea, eb = ((p0 + 1.0).cuda(), (p0 + 1.0).cuda()) if ema_on else (None, None)
    sa, sb = torch.zeros(1, dtype=torch.int64).cuda(), torch.zeros(1, dtype=torch.int64).cuda()
    la, lb = torch.full((1,), 7.0).cuda(), torch.full((1,), 7.0).cuda()
    state = _new_state()
    skip = state.view(torch.int32)[2:3]
    for k in range(4):
        g = torch.randn(n, generator=gen).cuda()
        K.grad_guard(g, None, 0.05 * math.sqrt(n), -1.0, state)          # clips by about twenty
        scale = state.view(torch.float32)[1:2].clone()
        assert 0.0 < scale.item() < 1.0
        K.adamax_guarded_step(pa, g, ma, ua, None, 2e-3, sched, 0.9, 0.999, 1e-8, 1e-2, sa, ea, 0.9, la, state)
        K.counter_advance_unless(sa, 1, skip)
        if sched_on:
            K.adamax_sched_step(pb, g, mb, ub, None, sched, 0.9, 0.999, 1e-8, 1e-2, scale, sb, eb, 0.9, lb)
        elif ema_on:
            K.adamax_ema_step(pb, g, mb, ub, None, 2e-3, 0.9, 0.999, 1e-8, 1e-2, scale, sb, eb, 0.9)
        else:
            K.adamax_step(pb, g, mb, ub, None, 2e-3, 0.9, 0.999, 1e-8, 1e-2, scale, sb)
        K.counter_advance(sb)
    torch.cuda.synchronize()
    assert sa.item() == sb.item() == 4 and not torch.equal(pa, p0.cuda())
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(ua, ub) and torch.equal(la, lb)
    assert (la.item() != 7.0) == sched_on
    if ema_on:
        assert torch.equal(ea, eb) and not torch.equal(ea, (p0 + 1.0).cuda())
    # a skipped step: an all-NaN gradient under the flag leaves every buffer and the counter bit for bit
    before = [t.clone() for t in (pa, ma, ua, la, sa)] + ([ea.clone()] if ema_on else [])
    g = torch.full((n,), math.nan).cuda()
    K.grad_guard(g, None, 1.0, -1.0, state)
    K.adamax_guarded_step(pa, g, ma, ua, None, 2e-3, sched, 0.9, 0.999, 1e-8, 1e-2, sa, ea, 0.9, la, state)
    K.counter_advance_unless(sa, 1, skip)
    torch.cuda.synchronize()
    assert skip.item() == 1 and int(state[3]) == 1
    for a, b in zip(before, [pa, ma, ua, la, sa] + ([ea] if ema_on else [])):
        assert torch.equal(a, b) and not bool(torch.isnan(b.float()).any())


@pytest.mark.parametrize('flag,copies', [(None, True), (1, True), (0, False)], ids=['no-flag', 'flag-matches', 'flag-differs'])
def test_multi_copy_copies_its_entries_and_nothing_else(flag, copies):
    K = _K()
    sizes, gap = [1, 3, 64, 65], 5
    src = [torch.randn(s, generator=torch.Generator().manual_seed(s)).cuda() for s in sizes]
    total = gap + sum(s + gap for s in sizes)
    dst = torch.full((total,), -1.0).cuda()
    views, off = [], gap
    for s in sizes:
        views.append(dst[off:off + s])
        off += s + gap
    table = K.copy_table(list(zip(views, src)), dst.device)
    f = None if flag is None else torch.tensor([flag], dtype=torch.int32).cuda()
    K.multi_copy(table, f, 1)
    torch.cuda.synchronize()
    inside = torch.zeros(total, dtype=torch.bool)
    off = gap
    for s, v, x in zip(sizes, views, src):
        assert torch.equal(v, x) if copies else bool((v == -1.0).all())
        inside[off:off + s] = True
        off += s + gap
    assert bool((dst.cpu()[~inside] == -1.0).all())        # the canaries around every destination
    for x, s in zip(src, sizes):
        assert torch.equal(x, torch.randn(s, generator=torch.Generator().manual_seed(s)).cuda())


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the whole step (the tiny_cifar golden, batch 4; two eager steps, the capture, four replays)
# ---------------------------------------------------------------------------------------------------------------------------------
STEPS, BAD, LR = 7, 4, 1e-3       # the bad batch falls on a replayed step (index 4: the second replay)
IDLE = dict(max_norm=1e30, skip_threshold=math.inf)
_runs = {}


def _schedule():
    from lvae_amd.optim import LrSchedule
    return LrSchedule('cosine', warmup_steps=2, decay_steps=3, min_lr=LR / 10)


def _xs(bad=False):
    xs = [_images(4, 80 + k) for k in range(STEPS)]
    if bad:
        xs[BAD] = xs[BAD].clone()
        xs[BAD][1, 2, 5, 7] = math.nan                      # one NaN pixel
    return xs


def _full_state(m, opt):
    st = _train_state(m, opt)
    if opt.ema is not None:
        st['ema'] = opt.ema.clone()
    if opt.lr_now is not None:
        st['lr_now'] = opt.lr_now.clone()
    return st


def _make(guard=None, plain=False, seed_model=None):
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax, GradGuard
    g = load_golden('tiny_cifar')
    _fresh_table()
    m = _model(g.cfg, g.state_dict(), PhiloxNoise(seed=3))
    gd = None if guard is None else GradGuard(**guard)
    opt = Adamax(m, lr=LR, guard=gd) if plain else Adamax(m, lr=LR, ema_decay=0.99, schedule=_schedule(), guard=gd)
    return m, opt


def _loop(m, opt, xs, use_graph, summary=None, calls=None, hook=None, first=0):
    """runs the steps; `calls` records (name, first argument) of every C-ABI call of the Python passes; hook(k, st, before | None)"""
    from lvae_amd import _C
    from lvae_amd import kernels as K
    from lvae_amd.engine import TrainStep
    real = _C.call

    def counted(name, *args):
        calls.append((name, args[0] if args else None))
        return real(name, *args)

    if calls is not None:
        _C.call = K.call = counted
    outs = []
    try:
        st = TrainStep(m, opt, use_graph=use_graph, summary=summary)
        for k, x in enumerate(xs, first):
            snap = hook(k, st, None) if hook is not None else None
            outs.append({key: v.detach().clone() for key, v in st(x.cuda()).items()})
            if hook is not None:
                hook(k, st, snap)
        torch.cuda.synchronize()
    finally:
        _C.call = K.call = real
    assert (st.graph_a is not None) == (use_graph and len(xs) > 2)
    return outs


def _run(use_graph, guard, bad=False, plain=False, summary=False):
    key = (use_graph, None if guard is None else tuple(sorted(guard.items())), bad, plain, summary)
    if key not in _runs:
        from lvae_amd.summary import TrainSummary
        m, opt = _make(guard, plain)
        calls = []
        sm = TrainSummary(len(load_golden('tiny_cifar').cfg['z_dims']), 'cuda') if summary else None
        outs = _loop(m, opt, _xs(bad), use_graph, summary=sm, calls=calls)
        _runs[key] = {'outs': outs, 'state': _full_state(m, opt), 'calls': calls, 'counts': None if opt.guard is None else opt.guard.counts(),
                      'grads_ptr': m.arena.grads.data_ptr(), 'acc': None if sm is None else sm.acc.clone(), 'global_step': m.global_step}
    return _runs[key]


def _same_outs(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for k in x:                                        # (a NaN, the bad step's loss, equals a NaN here)
            assert torch.equal(torch.nan_to_num(x[k], nan=-12345.0), torch.nan_to_num(y[k], nan=-12345.0)), k


@pytest.mark.parametrize('plain', [False, True], ids=['ema+schedule', 'plain'])
def test_idle_guard_changes_no_bit_eager_or_captured(plain):
    ref, graph, eager = _run(True, None, plain=plain), _run(True, IDLE, plain=plain), _run(False, IDLE, plain=plain)
    _assert_same_state(ref['state'], graph['state'])
    _assert_same_state(graph['state'], eager['state'])
    _same_outs(ref['outs'], graph['outs'])
    _same_outs(graph['outs'], eager['outs'])
    assert graph['counts'] == eager['counts'] == (0, 0) and int(graph['state']['adamax_step']) == STEPS


def test_clipped_step_follows_float64_adamax_on_the_clipped_gradient():
    """One step from the golden weights with G = half the norm of that step's gradient: parameters, exp_avg and exp_inf against float64 Adamax on
    g min(1, G / (norm + 1e-6)), by the rule of test_adamax_weight_decay_matches_torch (rtol 2e-6, atol 2e-7). Then seven steps under the same
    limit, captured against eager."""
    m, opt = _make(IDLE, plain=True)
    _loop(m, opt, _xs()[:1], False)
    norm1 = opt.guard.norm.item()
    assert math.isfinite(norm1) and norm1 > 0
    G = 0.5 * norm1
    m, opt = _make(dict(max_norm=G), plain=True)
    p0 = m.pack().params[:m.arena.n_train].detach().clone().double()
    _loop(m, opt, _xs()[:1], False)
    assert _bits(opt.guard.norm.item()) == _bits(norm1) and opt.guard.counts() == (1, 0)
    g = m.arena.grads.detach().double() * min(1.0, float(np.float32(G)) / (norm1 + 1e-6))
    exp_avg, exp_inf = 0.1 * g, g.abs() + 1e-8
    want = p0 - (LR / (1 - 0.9)) * exp_avg / exp_inf
    got = m.arena.params[:m.arena.n_train].detach().double()
    err = (got - want).abs()
    print('clipped step: norm %.6g, G %.6g, max abs error %.3e, max of error / (2e-7 + 2e-6 |ref|) %.3f'
          % (norm1, G, float(err.max()), float((err / (2e-7 + 2e-6 * want.abs())).max())))
    torch.testing.assert_close(got, want, rtol=2e-6, atol=2e-7)
    torch.testing.assert_close(opt.exp_avg.double(), exp_avg, rtol=2e-6, atol=2e-7)
    torch.testing.assert_close(opt.exp_inf.double(), exp_inf, rtol=2e-6, atol=2e-7)
    # the comparison sees the factor: Adamax's first update is lr sign(g) whatever the factor, but the moments of the unclipped gradient
    # are hundreds of tolerances away
    assert float((opt.exp_avg.double() - 0.1 * m.arena.grads.double()).abs().max()) > 100 * 2e-7
    graph, eager = _run(True, dict(max_norm=G)), _run(False, dict(max_norm=G))
    _assert_same_state(graph['state'], eager['state'])
    _same_outs(graph['outs'], eager['outs'])
    assert graph['counts'] == eager['counts'] and graph['counts'][0] >= 1 and graph['counts'][1] == 0
    assert not torch.equal(graph['state']['params'], _run(True, IDLE)['state']['params'])


@pytest.mark.parametrize('use_graph', [True, False], ids=['captured', 'eager'])
def test_nonfinite_step_is_skipped_and_leaves_everything_as_it_was(use_graph):
    m, opt = _make(IDLE)
    seen = {}

    def hook(k, st, before):
        if before is None:
            return (_full_state(m, opt), m.global_step) if k in (BAD, BAD + 1) else None
        if k == BAD:
            assert use_graph == (st.graph_a is not None)    # a replayed step, not the capture
            seen['bad'] = (before, (_full_state(m, opt), m.global_step))
        if k == BAD + 1:
            seen['next'] = (before, (_full_state(m, opt), m.global_step))

    outs = _loop(m, opt, _xs(bad=True), use_graph, hook=hook)
    (b0, gs0), (b1, gs1) = seen['bad']
    assert b0.keys() == b1.keys() and gs1 == gs0 + 1
    tracked = [k for k in b0 if k.endswith('num_batches_tracked')]
    stats = [k for k in b0 if k.endswith(('running_mean', 'running_var'))]
    assert tracked and len(stats) == 2 * len(tracked) and {'params', 'exp_avg', 'exp_inf', 'adamax_step', 'ema', 'lr_now'} <= set(b0)
    for k in b0:
        if k in tracked:
            assert int(b1[k]) == int(b0[k]) + 1, k
        else:
            assert torch.equal(b0[k], b1[k]), k
            assert not bool(torch.isnan(b1[k].float()).any()), k
    assert math.isnan(outs[BAD]['loss'].item())
    assert opt.guard.counts() == (0, 1) and int(opt.step_count.item()) == STEPS - 1
    # the following clean step is finite and moves the weights
    (n0, _), (n1, _) = seen['next']
    assert all(math.isfinite(outs[BAD + 1][k].item()) for k in ('loss', 'elbo', 'recons', 'kl'))
    assert not torch.equal(n0['params'], n1['params']) and int(n1['adamax_step']) == int(n0['adamax_step']) + 1
    assert bool(torch.isfinite(n1['params']).all()) and not any(torch.equal(n0[k], n1[k]) for k in stats)


def test_skipped_step_is_as_if_it_had_not_happened():
    """The twin of the NaN run sees a clean batch at the bad step, skipped by T = 0. (The threshold is an argument of a captured launch, so
    the twin runs that one step through eager launches, which the other tests show to equal a replay bit for bit.) From the next step on
    the two runs agree in every output and in their final state."""
    nan_run = _run(True, IDLE, bad=True)
    m, opt = _make(IDLE)

    def hook(k, st, before):
        if k == BAD:
            st.use_graph = before is not None               # eager for this step only
            opt.guard.skip_threshold = 0.0 if before is None else math.inf
        return 0

    outs = _loop(m, opt, _xs(bad=False), True, hook=hook)
    assert opt.guard.counts() == (0, 1) and math.isfinite(outs[BAD]['loss'].item())
    _same_outs(nan_run['outs'][:BAD], outs[:BAD])
    _same_outs(nan_run['outs'][BAD + 1:], outs[BAD + 1:])
    _assert_same_state(nan_run['state'], _full_state(m, opt))
    assert nan_run['global_step'] == m.global_step == STEPS and nan_run['counts'] == (0, 1)
    # and the skipped step did count as a step of the run: the later steps are not those of the run that never saw it
    assert not torch.equal(nan_run['outs'][BAD + 1]['loss'], _run(True, IDLE)['outs'][BAD + 1]['loss'])


GUARD_CALLS = {'lvae_grad_guard_f32', 'lvae_adamax_guarded_step_f32', 'lvae_counter_advance_unless', 'lvae_multi_copy_f32'}


def test_launch_record():
    """Without a guard the step reaches none of the new entry points; with one it issues the same calls in the same order plus, per Python
    pass, the save at the head and guard | restore before the guarded Adamax. With a summary the guard's norm is the one folded: no
    lvae_l2norm_f32 on the gradient arena."""
    plain, guarded = _run(True, None, plain=True), _run(True, IDLE, plain=True)
    names = [n for n, _ in plain['calls']]
    assert not GUARD_CALLS & set(names) and names.count('lvae_adamax_step_f32') == 3
    gnames = [n for n, _ in guarded['calls']]
    assert gnames.count('lvae_multi_copy_f32') == 6 and gnames.count('lvae_grad_guard_f32') == 3
    i = gnames.index('lvae_grad_guard_f32')
    assert gnames[i:i + 4] == ['lvae_grad_guard_f32', 'lvae_multi_copy_f32', 'lvae_adamax_guarded_step_f32', 'lvae_counter_advance_unless']
    back = {'lvae_adamax_guarded_step_f32': 'lvae_adamax_step_f32', 'lvae_counter_advance_unless': 'lvae_counter_advance'}
    assert [back.get(n, n) for n in gnames if n not in ('lvae_grad_guard_f32', 'lvae_multi_copy_f32')] == names
    # the scheduled, averaging optimizer: same story
    a, b = [n for n, _ in _run(True, None)['calls']], [n for n, _ in _run(True, IDLE)['calls']]
    back['lvae_adamax_guarded_step_f32'] = 'lvae_adamax_sched_step_f32'
    assert [back.get(n, n) for n in b if n not in ('lvae_grad_guard_f32', 'lvae_multi_copy_f32')] == a
    # with a summary
    s_plain, s_guard = _run(True, None, summary=True), _run(True, IDLE, summary=True)
    on_grads = lambda r: [n for n, p in r['calls'] if n == 'lvae_l2norm_f32' and p == r['grads_ptr']]
    assert len(on_grads(s_plain)) == 3 and len(on_grads(s_guard)) == 0
    assert [n for n, _ in s_guard['calls']].count('lvae_summary_fold_f64') == 3
    assert torch.equal(s_plain['acc'], s_guard['acc']) and float(s_guard['acc'][7]) > 0    # the window's grad sum, bit for bit
    _assert_same_state(s_plain['state'], s_guard['state'])


def test_resume_behind_a_skipped_step_is_exact(tmp_path):
    from lvae_amd.checkpoint import load_checkpoint, save_checkpoint
    from lvae_amd.models.lvae import LadderVAE
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax, GradGuard
    straight = _run(True, IDLE, bad=True)
    xs = _xs(bad=True)
    cut = BAD + 1
    m1, opt1 = _make(IDLE)
    first = _loop(m1, opt1, xs[:cut], True)
    path = str(tmp_path / ('model_%d.pt' % cut))
    save_checkpoint(path, m1, opt1)
    ck = torch.load(path)
    assert ck['grad_guard'] == dict(IDLE, clipped=0, skipped=1) and ck['optimizer']['step'] == cut - 1 and ck['global_step'] == cut
    del m1, opt1
    g = load_golden('tiny_cifar')
    _fresh_table()
    torch.manual_seed(123)
    m2 = LadderVAE(**g.cfg).cuda().train()
    m2.noise = PhiloxNoise(seed=999)
    opt2 = Adamax(m2, lr=LR, ema_decay=0.99, schedule=_schedule(), guard=GradGuard(**IDLE))
    load_checkpoint(path, m2, opt2)
    assert opt2.guard.counts() == (0, 1)
    rest = _loop(m2, opt2, xs[cut:], False)                # (two steps left: eager launches, which equal replays)
    _same_outs(straight['outs'], first + rest)
    _assert_same_state(straight['state'], _full_state(m2, opt2))
    assert opt2.guard.counts() == straight['counts'] == (0, 1)
    # a file from before the guard existed loads, into a guarded and into a plain optimizer; the guard keeps its counts
    old = str(tmp_path / 'old.pt')
    torch.save({k: v for k, v in ck.items() if k != 'grad_guard'}, old)
    for opt3 in (Adamax(m2, lr=LR, ema_decay=0.99, schedule=_schedule(), guard=GradGuard(**IDLE)), Adamax(m2, lr=LR)):
        assert 'grad_guard' not in load_checkpoint(old, m2, opt3)
        assert int(opt3.step_count.item()) == cut - 1 and (opt3.guard is None or opt3.guard.counts() == (0, 0))
    # and a guarded file into an unguarded optimizer
    load_checkpoint(path, m2, Adamax(m2, lr=LR))


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. both exchange forms on one forced rank (the pattern of tests/test_ddp_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------------------
WORKER = os.path.join(ROOT, 'tests', 'grad_guard_ddp_worker.py')


def _worker(mode, out):
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.update(RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
    env.pop('LVAE_FORCE_DIST', None)
    env.pop('LVAE_DDP_MODE', None)
    p = subprocess.run([sys.executable, WORKER, mode, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    return torch.load(out)


@pytest.fixture(scope='module')
def single_rank(tmp_path_factory):
    return _worker('single', str(tmp_path_factory.mktemp('guard_ddp') / 'single.pt'))


@pytest.mark.parametrize('form', ['split', 'overlap'])
def test_exchange_forms_idle_match_single_rank_and_skip_the_nan_batch(form, single_rank, tmp_path):
    """Five clean steps under an idle guard against the unguarded single-rank run (tolerances of tests/test_ddp_gpu.py: the exchange goes
    through RCCL's out-of-place copy, the arithmetic is the same), then a NaN batch on a replayed step: skipped, nothing moved, and the
    clean step after it is finite."""
    r = _worker(form, str(tmp_path / (form + '.pt')))
    la, lb = single_rank['losses'], r['losses']
    assert max(abs(u - v) / abs(u) for u, v in zip(la, lb)) < 1e-6, (la, lb)
    worst = 0.0
    for k, v in single_rank['sd'].items():
        if v.dtype.is_floating_point:
            worst = max(worst, float((r['sd'][k].double() - v.double()).norm()) / (float(v.double().norm()) + 1e-12))
    assert worst < 1e-6
    assert r['graphs'] == ((True, True) if form == 'split' else (True, False))
    assert r['counts_idle'] == (0, 0) and r['counts_end'] == (0, 1) and r['unchanged'] and r['tracked_advanced']
    assert math.isnan(r['bad_loss']) and math.isfinite(r['next_loss']) and r['moved_after']


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the trainer
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('window', [False, True], ids=['last-step', 'window-summaries'])
def test_trainer_prints_and_records_the_counts(window, tmp_path, capsys):
    import json
    import re
    from lvae_amd import main as lmain
    _fresh_table()
    hist, ck = str(tmp_path / 'history.jsonl'), str(tmp_path / 'end.pt')
    argv = ['-d', 'cifar10', '--zdims', '8', '8', '--downsample', '1', '1', '--nfilters', '16', '--skip', '--gated', '--freebits', '1.0',
            '--batch-size', '8', '--synthetic', '--seed', '3', '--steps', '6', '--log-every', '2', '--history', hist, '--save-checkpoint', ck,
            '--lr', '1e-3', '--max-grad-norm', '1e-3', '--grad-skip-threshold', 'inf']
    lmain.main(argv + (['--window-summaries'] if window else []))
    out = capsys.readouterr().out
    assert ',clip0.001,skipinf,' in out
    lines = [ln for ln in out.splitlines() if re.search(r'\[step \d+\]', ln)]
    assert len(lines) == 3, out
    for ln in lines:
        assert re.search(r'   grad: \S+.*   clipped: 2   skipped: 0$', ln), ln     # every step's norm is far above 1e-3
    recs = [json.loads(r) for r in open(hist)]
    assert [r['step'] for r in recs] == [2, 4, 6]
    for r in recs:
        assert r['metrics']['grad/clipped'] == 2 and r['metrics']['grad/skipped'] == 0, r
    assert torch.load(ck)['grad_guard'] == {'max_norm': 1e-3, 'skip_threshold': math.inf, 'clipped': 6, 'skipped': 0}
    _fresh_table()
