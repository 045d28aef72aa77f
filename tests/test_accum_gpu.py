"""Gradient accumulation over micro-batches inside the training step: the fold kernel against float64 means; accum_steps=1 against the step
without the argument; the eager schedule against the same passes issued by hand; captured against eager under every update rule; the
accumulated gradient against separately computed ones and against the CPU oracle; the guard; device-fed data with a resume; and the split
exchange on one forced RCCL rank. The tiny_cifar golden throughout, micro-batches of 4 images."""
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

MICRO = 4
SCALARS = ('loss', 'elbo', 'recons', 'kl', 'l2')


def _K():
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels as K
    return K


def _state(m, opt):
    """_train_state for any update rule, with the average and the scheduled lr when there are any."""
    from lvae_amd.optim import RULES
    sd = m.state_dict()   # (flushes the host-counted num_batches_tracked)
    second = RULES[opt.rule]
    st = {k: v.detach().clone() for k, v in sd.items() if not k.endswith(('weight', 'bias', 'top_prior_params'))}
    st.update(params=m.arena.params.detach().clone(), exp_avg=opt.exp_avg.clone(), opt_step=opt.step_count.clone())
    st[second] = getattr(opt, second).clone()
    if opt.ema is not None:
        st['ema'] = opt.ema.clone()
    if opt.lr_now is not None:
        st['lr_now'] = opt.lr_now.clone()
    return st


def _differing(a, b):
    return [k for k in a if not torch.equal(a[k], b[k])]


def _golden_model(noise):
    g = load_golden('tiny_cifar')
    _fresh_table()
    return _model(g.cfg, g.state_dict(), noise), g


def _steps(m, opt, xs, **kw):
    from lvae_amd.engine import TrainStep
    st = TrainStep(m, opt, **kw)
    outs = [{k: v.detach().clone() for k, v in st(x.cuda()).items()} for x in xs]
    torch.cuda.synchronize()
    return outs, st


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the fold kernel
# ---------------------------------------------------------------------------------------------------------------------------------
def _fold_call(K, row, L, M, acc, count, out, with_iw):
    K.micro_fold(row[0:1], row[1:2], row[2:3], row[3:4], row[4:5], row[7:7 + L], M, acc, count, out,
                 iw=row[5:6] if with_iw else None, ess=row[6:7] if with_iw else None)


def _fold_means(vals, M, with_iw):
    s = torch.zeros(vals.shape[1], dtype=torch.float64)
    for j in range(M):                                     # the sequential float64 sum in call order
        s = s + vals[j].double()
    mean = (s / M).float()
    if not with_iw:
        mean[5:7] = 0.0
    return mean


@pytest.mark.parametrize('with_iw', [True, False], ids=['iw+ess', 'null-iw'])
@pytest.mark.parametrize('L', [1, 15, 64])
@pytest.mark.parametrize('M', [1, 2, 3, 7])
def test_fold_kernel_writes_float64_means_on_the_last_call_and_starts_again(M, L, with_iw):
    K = _K()
    n = 7 + L
    gen = torch.Generator().manual_seed(1000 * M + 10 * L + with_iw)
    acc = torch.zeros(n, dtype=torch.float64, device='cuda')
    count = torch.zeros(1, dtype=torch.int64, device='cuda')
    out = torch.full((n,), -7.0, device='cuda')
    before = out.clone()
    firsts = None
    # values of mixed magnitude, so that a float32 sum would round differently from the float64 one
    vals = (torch.randn(M, n, generator=gen) * torch.tensor([1e4, 1.0, 1e-3])[torch.randint(0, 3, (M, n), generator=gen)]).float()
    dev = vals.cuda()
    for rnd in range(2):                                   # the second round repeats the first: the same bits come out
        part = torch.zeros(n, dtype=torch.float64)
        for j in range(M):
            _fold_call(K, dev[j], L, M, acc, count, out, with_iw)
            part = part + vals[j].double()
            if not with_iw:
                part[5:7] = 0.0
            if j < M - 1:
                print('yardstick | M=%d L=%d pass %d: counter %d, output changed in %d slots' %
                      (M, L, j + 1, int(count.item()), int((out != before).sum())))
                assert torch.equal(out, before) and int(count.item()) == j + 1          # untouched before the M-th call
                assert torch.equal(acc.cpu(), part)
        want = _fold_means(vals, M, with_iw)
        got = out.cpu()
        print('yardstick | M=%d L=%d iw=%s round %d: %d of %d slots differ from the float64 mean, acc max %g, counter %d' %
              (M, L, with_iw, rnd, int((got != want).sum()), n, float(acc.abs().max()), int(count.item())))
        assert torch.equal(got, want)
        assert float(acc.abs().max()) == 0.0 and int(count.item()) == 0               # cleared for the next step
        if rnd == 0:
            firsts = (vals, got.clone())
            assert not torch.equal(out, before)
            before = out.clone()
        else:
            assert torch.equal(got.view(torch.int32), firsts[1].view(torch.int32))


def test_fold_kernel_nan_reaches_its_own_mean_only():
    K = _K()
    L, M = 3, 3
    n = 7 + L
    vals = torch.randn(M, n, generator=torch.Generator().manual_seed(5))
    vals[1, 3] = math.nan                                  # the kl of pass 2 of 3
    vals[2, 8] = math.inf                                  # and an Inf in a layer's KL of pass 3
    acc = torch.zeros(n, dtype=torch.float64, device='cuda')
    count = torch.zeros(1, dtype=torch.int64, device='cuda')
    out = torch.zeros(n, device='cuda')
    dev = vals.cuda()
    for j in range(M):
        _fold_call(K, dev[j], L, M, acc, count, out, True)
    got, want = out.cpu(), _fold_means(vals, M, True)
    print('yardstick | NaN in slot 3 of pass 2, Inf in slot 8 of pass 3: non-finite means in slots %r' %
          [i for i in range(n) if not math.isfinite(float(got[i]))])
    assert math.isnan(float(got[3])) and math.isinf(float(got[8]))
    keep = [i for i in range(n) if i not in (3, 8)]
    assert torch.equal(got[keep], want[keep]) and bool(torch.isfinite(got[keep]).all())
    assert float(acc.abs().max()) == 0.0 and int(count.item()) == 0


def test_fold_kernel_argument_checks():
    import lvae_amd  # noqa: F401
    from lvae_amd import _C
    K = _K()
    f = torch.zeros(7 + 65, device='cuda')
    acc = torch.zeros(7 + 65, dtype=torch.float64, device='cuda')
    count = torch.zeros(1, dtype=torch.int64, device='cuda')
    out = torch.full((7 + 65,), 3.0, device='cuda')
    p, sp = f.data_ptr(), _C.stream_ptr()

    def raw(M=2, L=3, **null):
        a = dict(loss=p, elbo=p + 4, recons=p + 8, kl=p + 12, l2=p + 16, iw=None, ess=None, kl_layers=p + 28, acc=acc.data_ptr(),
                 count=count.data_ptr(), out=out.data_ptr())
        a.update(null)
        _C.call('lvae_micro_fold_f64', a['loss'], a['elbo'], a['recons'], a['kl'], a['l2'], a['iw'], a['ess'], a['kl_layers'], L, M, a['acc'],
                a['count'], a['out'], sp)

    refused = []
    cases = [dict(M=0), dict(M=-1), dict(L=65), dict(L=-1)] + [{k: None} for k in ('loss', 'elbo', 'recons', 'kl', 'l2', 'kl_layers', 'acc',
                                                                                 'count', 'out')]
    for case in cases:
        with pytest.raises(_C.LvaeHipError) as e:
            raw(**case)
        refused.append((case, str(e.value)))
    torch.cuda.synchronize()
    print('yardstick | refused: %s' % '; '.join('%r' % (c,) for c, _ in refused))
    assert all('lvae_micro_fold_f64' in msg for _, msg in refused)
    assert float(acc.abs().max()) == 0.0 and int(count.item()) == 0 and bool((out == 3.0).all())   # nothing was launched
    raw(M=1, L=64)                                         # the largest L is taken, and L = 0 needs no kl_layers
    raw(M=1, L=0, kl_layers=None)
    with pytest.raises(_C.LvaeHipError):                   # the wrapper: an output that does not match the accumulator
        K.micro_fold(f[0:1], f[1:2], f[2:3], f[3:4], f[4:5], f[7:10], 2, acc[:10], count, out[:9])
    with pytest.raises(_C.LvaeHipError):
        K.micro_fold(f[0:1], f[1:2], f[2:3], f[3:4], f[4:5], f[7:11], 2, acc[:10], count, out[:10])
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. accum_steps = 1 is the step there was
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('use_graph', [False, True], ids=['eager', 'captured'])
def test_one_micro_batch_is_the_present_step_bit_for_bit(use_graph):
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax
    xs = [_images(MICRO, 30 + k) for k in range(4)]
    runs = []
    for kw in ({}, {'accum_steps': 1}):
        m, _ = _golden_model(PhiloxNoise(seed=3))
        opt = Adamax(m, lr=1e-3)
        outs, st = _steps(m, opt, xs, use_graph=use_graph, **kw)
        assert (st.graph_a is not None) == use_graph and st.graph_p is None and opt.gscale is None
        runs.append((outs, _train_state(m, opt)))
    diff = _differing(runs[0][1], runs[1][1])
    print('yardstick | accum_steps=1 against no argument (%s): %d of %d state tensors differ' %
          ('captured' if use_graph else 'eager', len(diff), len(runs[0][1])))
    _assert_same_state(runs[0][1], runs[1][1])
    for a, b in zip(runs[0][0], runs[1][0]):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the eager schedule against the same passes issued by hand
# ---------------------------------------------------------------------------------------------------------------------------------
def _hand_pass(m, x):
    from lvae_amd import ops
    from lvae_amd.engine import forward_pass
    K = _K()
    K.prepared.prepare_all()
    out = forward_pass(m, x)
    ops.set_wgrad_grouping(16384)                           # (TrainStep's default: small layers' weight gradients share launches)
    out['loss'].backward()
    ops.flush_wgrad_group()
    ops.set_wgrad_grouping(None)
    return {k: out[k].detach().clone() for k in SCALARS + ('kl_avg_layerwise',)}


def _f32_mean(values):
    s = 0.0
    for v in values:                                       # (float() widens the float32 exactly)
        s += float(v)
    return float(np.float32(s / len(values)))


@pytest.mark.parametrize('M', [2, 3])
def test_eager_schedule_equals_the_passes_issued_by_hand(M):
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax
    xs = [_images(MICRO * M, 40 + k) for k in range(2)]
    m, _ = _golden_model(PhiloxNoise(seed=3))
    opt = Adamax(m, lr=1e-3)
    outs, st = _steps(m, opt, xs, use_graph=False, accum_steps=M)
    got = _state(m, opt)
    assert st.graph_a is None and float(opt.gscale.item()) == float(np.float32(1.0 / M))
    # by hand, through the public pieces
    m2, _ = _golden_model(PhiloxNoise(seed=3))
    opt2 = Adamax(m2, lr=1e-3)
    opt2._state()
    opt2.gscale = torch.full((1,), 1.0 / M, dtype=torch.float32, device='cuda')
    passes = []
    for x in xs:
        opt2.zero_grad()
        passes.append([_hand_pass(m2, x[j * MICRO:(j + 1) * MICRO].cuda()) for j in range(M)])
        opt2.step()
    torch.cuda.synchronize()
    want = _state(m2, opt2)
    diff = _differing(want, got)
    print('yardstick | M=%d eager against the hand-written loop: %d of %d state tensors differ %r' % (M, len(diff), len(want), diff[:4]))
    _assert_same_state(want, got)
    tracked = [k for k in got if k.endswith('num_batches_tracked')]
    assert tracked and all(int(got[k]) == 2 * M for k in tracked) and int(got['opt_step']) == 2 and m.global_step == 2
    for s, (out, per_pass) in enumerate(zip(outs, passes)):
        for k in SCALARS:
            ref = _f32_mean([p[k] for p in per_pass])
            print('yardstick | M=%d step %d %s: returned %r, float64 mean of the passes rounded to fp32 %r' % (M, s + 1, k, float(out[k]), ref))
            assert float(out[k]) == ref, (s, k)
        layers = [_f32_mean([p['kl_avg_layerwise'][i] for p in per_pass]) for i in range(out['kl_avg_layerwise'].numel())]
        assert out['kl_avg_layerwise'].tolist() == layers, (s, out['kl_avg_layerwise'].tolist(), layers)
    assert 'iw' not in outs[0] and 'ess' not in outs[0]


def test_rows_that_do_not_divide_are_refused_and_leave_the_step_uncounted():
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax
    from lvae_amd.engine import TrainStep
    m, _ = _golden_model(PhiloxNoise(seed=3))
    st = TrainStep(m, Adamax(m, lr=1e-3), use_graph=False, accum_steps=3)
    with pytest.raises(ValueError):
        st(_images(8, 1).cuda())
    assert m.global_step == 0 and int(st._mcount.item()) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. captured against eager
# ---------------------------------------------------------------------------------------------------------------------------------
def _optimizer(form, m):
    from lvae_amd.optim import Adamax, AdamW, LrSchedule
    if form == 'adamax+ema':
        return Adamax(m, lr=1e-3, ema_decay=0.99)
    if form == 'adamw+cosine':
        return AdamW(m, lr=1e-3, schedule=LrSchedule('cosine', warmup_steps=1, decay_steps=3, min_lr=1e-4))
    return Adamax(m, lr=1e-3)


@pytest.mark.parametrize('form', ['plain', 'beta_anneal', 'adamax+ema', 'adamw+cosine'])
def test_captured_equals_eager(form):
    from lvae_amd.noise import PhiloxNoise
    M = 3
    xs = [_images(MICRO * M, 50 + k) for k in range(4)]
    runs = {}
    for use_graph in (False, True):
        m, _ = _golden_model(PhiloxNoise(seed=3))
        opt = _optimizer(form, m)
        outs, st = _steps(m, opt, xs, use_graph=use_graph, accum_steps=M, beta_anneal=5 if form == 'beta_anneal' else 0)
        assert (st.graph_p is not None) == (st.graph_a is not None) == (st.graph_b is not None) == use_graph
        state = _state(m, opt)
        if form == 'beta_anneal':
            state['beta_counter'] = m.global_step_dev.clone()
        state['noise_counter'] = m.noise.step.clone()
        runs[use_graph] = (outs, state, m.global_step)
    (eo, es, eg), (go, gs, gg) = runs[False], runs[True]
    diff = _differing(es, gs)
    print('yardstick | %s, M=3, four steps: captured against eager, %d of %d state tensors differ %r' % (form, len(diff), len(es), diff[:4]))
    _assert_same_state(es, gs)
    for a, b in zip(eo, go):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    tracked = [k for k in gs if k.endswith('num_batches_tracked')]
    print('yardstick | num_batches_tracked %r, optimizer steps %d, noise counter %d' %
          (sorted({int(gs[k]) for k in tracked}), int(gs['opt_step']), int(gs['noise_counter'])))
    assert tracked and all(int(gs[k]) == 12 for k in tracked)
    assert int(gs['opt_step']) == 4 and eg == gg == 4 and int(gs['noise_counter']) == 12
    if form == 'beta_anneal':
        assert int(gs['beta_counter']) == 4                # one advance per optimizer step
    if form == 'adamw+cosine':
        assert float(gs['lr_now']) == float(es['lr_now']) and 0.0 < float(gs['lr_now']) < 1e-3
    assert len({float(o['loss']) for o in go}) == 4


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the accumulated gradient against separately computed ones
# ---------------------------------------------------------------------------------------------------------------------------------
def test_accumulated_gradient_is_the_sum_of_the_passes_gradients():
    """Each separate gradient comes from a zeroed arena with the noise counter at the value its pass saw, on a model brought to where that
    pass found it: a model's first pass lets every Winograd convolution transform its own weights, later passes read the table
    prepare_all() writes, and the two forms differ in the last bits (measured here: relative L2 1.4e-6 between the second micro-batch's
    gradient computed the one way and the other). With the passes on the same path every element of the accumulated arena equals
    fp32(g1 + g2): each parameter receives one add per backward."""
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax
    M = 2
    x = _images(MICRO * M, 61)
    m, _ = _golden_model(PhiloxNoise(seed=3))
    opt = Adamax(m, lr=0.0)                                 # the arena still holds the gradient after the step
    p0 = m.pack().params.detach().clone()
    _steps(m, opt, [x], use_graph=False, accum_steps=M)
    assert torch.equal(m.arena.params, p0) and int(m.noise.step.item()) == M
    acc = m.arena.grads.detach().double().cpu()
    segments = [tuple(sg[-2:]) for sg in m.arena.segments]
    total = torch.zeros_like(acc)
    for j in range(M):
        m2, _ = _golden_model(PhiloxNoise(seed=3))
        m2.pack().zero_grad()
        for i in range(j):                                  # the passes before it (lr = 0: the weights are the same ones)
            _hand_pass(m2, x[i * MICRO:(i + 1) * MICRO].cuda())
        m2.arena.zero_grad()
        if j:
            assert int(m2.noise.step.item()) == j           # the counter pass j saw
        _hand_pass(m2, x[j * MICRO:(j + 1) * MICRO].cuda())
        torch.cuda.synchronize()
        total += m2.arena.grads.detach().double().cpu()
    worst, exact = 0.0, 0
    for lo, hi in segments:
        ref = total[lo:hi]
        rel = float((acc[lo:hi] - ref).norm() / ref.norm()) if float(ref.norm()) > 0 else float((acc[lo:hi] - ref).norm())
        worst = max(worst, rel)
        exact += int(torch.equal(acc[lo:hi], ref.float().double()))
    print('yardstick | accumulated against the float64 sum of %d separate gradients: worst relative L2 over %d segments %.3g (bound 1e-6); '
          '%d segments equal the fp32-rounded sum exactly; whole arena max abs difference from the fp32-rounded sum %.3g' %
          (M, len(segments), worst, exact, float((acc - total.float().double()).abs().max())))
    assert len(segments) > 3 and float(total.norm()) > 0
    assert worst <= 1e-6, worst


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the accumulated step against the CPU oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def test_accumulated_step_matches_the_mean_of_the_oracles_gradients():
    import lvae_amd  # noqa: F401
    from lvae_amd.noise import TapeNoise
    from lvae_amd.optim import Adamax
    from oracle import lvae_ref as R
    M = 2
    g = load_golden('tiny_cifar')
    init = g.state_dict()
    x = _images(MICRO * M, 71)
    ref_grads, entries, ref_loss = None, [], []
    for j in range(M):                                     # each micro-batch is an independent reference run: its own statistics and noise
        sd = {k: v.clone() for k, v in init.items()}
        pkeys = [k for k in sd if R.is_parameter_key(k)]
        for k in pkeys:
            sd[k].requires_grad_(True)
        tape = R.Tape(gen=torch.Generator().manual_seed(100 + j))
        fp, _ = R.forward_pass(sd, g.cfg, x[j * MICRO:(j + 1) * MICRO], tape, param_keys=pkeys)
        fp['loss'].backward()
        entries += list(tape.entries)
        ref_loss.append(float(fp['loss'].detach()))
        gr = {k: sd[k].grad if sd[k].grad is not None else torch.zeros_like(sd[k]) for k in pkeys}
        ref_grads = gr if ref_grads is None else {k: ref_grads[k] + gr[k] for k in gr}
    ref_grads = {k: v / M for k, v in ref_grads.items()}
    _fresh_table()
    m = _model(g.cfg, init, TapeNoise(entries))            # one tape holding both passes' draws, in order
    opt = Adamax(m, lr=0.0)
    outs, _ = _steps(m, opt, [x], use_graph=False, accum_steps=M)
    assert m.noise.exhausted()
    mean_loss = sum(ref_loss) / M
    print('yardstick | returned mean loss %r against the mean of the oracle\'s two losses %r: relative %.3g (bound 1e-5)' %
          (float(outs[0]['loss']), mean_loss, abs(float(outs[0]['loss']) - mean_loss) / abs(mean_loss)))
    assert abs(float(outs[0]['loss']) - mean_loss) <= 1e-5 * abs(mean_loss)
    scale = float(opt.gscale.item())
    assert scale == 0.5
    worst, seen = 0.0, 0
    for k, p in m.named_parameters():
        ref = ref_grads[k].double()
        got = p.grad.detach().cpu().double() * scale       # the mean the update applies: the arena's sum times gscale
        if float(ref.norm()) < 1e-5 * max(1.0, ref.numel() ** 0.5):
            continue
        seen += 1
        worst = max(worst, float((got - ref).norm() / ref.norm()))
    print('yardstick | mean gradient against the oracle\'s: worst relative L2 over %d tensors %.3g (bound 1e-4)' % (seen, worst))
    assert seen > 10 and worst <= 1e-4, worst


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the guard
# ---------------------------------------------------------------------------------------------------------------------------------
def _guard_run(bad, twin):
    """Five steps of M = 3 (two eager, the capture, two replays); the bad step is the first replay. bad: a NaN pixel in its second
    micro-batch. twin: a clean batch there, skipped by a threshold of 0 instead (that one step through eager launches: the threshold is an
    argument of a captured launch)."""
    from lvae_amd.engine import TrainStep
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax, GradGuard
    M, BAD = 3, 3
    xs = [_images(MICRO * M, 80 + k) for k in range(5)]
    if bad:
        xs[BAD] = xs[BAD].clone()
        xs[BAD][MICRO + 1, 2, 5, 7] = math.nan             # one NaN pixel, in the second micro-batch
    m, _ = _golden_model(PhiloxNoise(seed=3))
    opt = Adamax(m, lr=1e-3, ema_decay=0.99, guard=GradGuard(skip_threshold=math.inf))
    st = TrainStep(m, opt, use_graph=True, accum_steps=M)
    snaps, outs = {}, []
    for k, x in enumerate(xs):
        if k == BAD:
            snaps['before'] = (_state(m, opt), m.global_step, int(m.noise.step.item()), opt.guard.counts())
            if twin:
                st.use_graph, opt.guard.skip_threshold = False, 0.0
        outs.append({key: v.detach().clone() for key, v in st(x.cuda()).items()})
        if k == BAD:
            st.use_graph, opt.guard.skip_threshold = True, math.inf
            snaps['after'] = (_state(m, opt), m.global_step, int(m.noise.step.item()), opt.guard.counts())
    torch.cuda.synchronize()
    assert st.graph_a is not None
    return outs, snaps, _state(m, opt)


def test_nan_in_one_micro_batch_skips_the_whole_step():
    outs, snaps, final = _guard_run(bad=True, twin=False)
    (b, gs0, n0, c0), (a, gs1, n1, c1) = snaps['before'], snaps['after']
    tracked = [k for k in b if k.endswith('num_batches_tracked')]
    stats = [k for k in b if k.endswith(('running_mean', 'running_var'))]
    moved = [k for k in b if k not in tracked and not torch.equal(a[k], b[k])]
    print('yardstick | skipped step: %d of %d tensors moved %r; global step %d -> %d, noise counter %d -> %d, skipped %d -> %d, '
          'num_batches_tracked +%r; mean loss %r' % (len(moved), len(b) - len(tracked), moved[:4], gs0, gs1, n0, n1, c0[1], c1[1],
                                                    sorted({int(a[k]) - int(b[k]) for k in tracked}), float(outs[3]['loss'])))
    assert tracked and len(stats) == 2 * len(tracked) and {'params', 'exp_avg', 'exp_inf', 'opt_step', 'ema'} <= set(b)
    for k in b:
        if k in tracked:
            assert int(a[k]) == int(b[k]) + 3, k
        else:
            assert torch.equal(a[k], b[k]), k
            assert not bool(torch.isnan(a[k].float()).any()), k
    assert gs1 == gs0 + 1 and n1 == n0 + 3 and c1 == (c0[0], c0[1] + 1)
    assert math.isnan(float(outs[3]['loss']))
    # the next clean step equals a clean step taken from that state: the twin skipped a clean batch there instead
    touts, tsnaps, tfinal = _guard_run(bad=False, twin=True)
    assert tsnaps['after'][3] == c1 and math.isfinite(float(touts[3]['loss']))
    _assert_same_state(tsnaps['after'][0], a)
    diff = _differing(final, tfinal)
    print('yardstick | after the next clean step: %d of %d tensors differ from the twin that skipped a clean batch' % (len(diff), len(final)))
    _assert_same_state(final, tfinal)
    for k in outs[4]:
        assert torch.equal(outs[4][k], touts[4][k]), k
    assert all(math.isfinite(float(outs[4][k])) for k in SCALARS) and not torch.equal(final['params'], a['params'])


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. device-fed data
# ---------------------------------------------------------------------------------------------------------------------------------
def _fed_run(images, how, n_steps, M=3, resume=None, save=None):
    from lvae_amd.checkpoint import load_checkpoint, save_checkpoint
    from lvae_amd.data import DeviceDataset
    from lvae_amd.engine import TrainStep
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax
    m, _ = _golden_model(PhiloxNoise(seed=3))
    m.accum_steps = M
    opt = Adamax(m, lr=1e-3)
    if resume is not None:
        load_checkpoint(resume, m, opt)
    ds = DeviceDataset(images, MICRO, seed=17)
    st = TrainStep(m, opt, use_graph=True, feed=ds if how == 'fed' else None, accum_steps=M)
    first = m.global_step + 1
    for s in range(first, n_steps + 1):
        if how == 'fed':
            st()
        else:
            st(torch.cat([ds.batch((s - 1) * M + j + 1) for j in range(M)]))
        if save is not None and s == save[0]:
            save_checkpoint(save[1], m, opt)
    torch.cuda.synchronize()
    assert st.graph_a is not None or n_steps - first < 2
    return _state(m, opt), (int(ds.cursor.item()) if how == 'fed' else None), m.global_step


def test_device_fed_accumulation_equals_host_fed_and_resumes_exactly(tmp_path):
    images = _images(40, 5)                                # batch 4: ten micro-batches per epoch; M = 3: an epoch ends inside step 4
    hand, _, _ = _fed_run(images, 'hand', 5)
    ck = str(tmp_path / 'step2.pt')
    fed, cursor, gs = _fed_run(images, 'fed', 5, save=(2, ck))
    diff = _differing(hand, fed)
    print('yardstick | device-fed against host-fed (N=40, batch 4, M=3, five steps): %d of %d state tensors differ; cursor %d' %
          (len(diff), len(hand), cursor))
    _assert_same_state(hand, fed)
    assert cursor == 15 and gs == 5
    saved = torch.load(ck)
    assert saved['accum_steps'] == 3 and saved['global_step'] == 2
    resumed, cursor2, gs2 = _fed_run(images, 'fed', 5, resume=ck)
    diff = _differing(fed, resumed)
    print('yardstick | stopped after step 2 and resumed: %d of %d state tensors differ; cursor %d' % (len(diff), len(fed), cursor2))
    _assert_same_state(fed, resumed)
    assert cursor2 == 15 and gs2 == 5


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. the exchange path: one forced rank over RCCL, split form
# ---------------------------------------------------------------------------------------------------------------------------------
WORKER = os.path.join(ROOT, 'tests', 'accum_worker.py')


def _worker(mode, out, steps, M):
    from test_ddp_gpu import _free_port
    env = dict(os.environ)
    env.update(RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_free_port()),
               HSA_ENABLE_IPC_MODE_LEGACY='0')
    env.pop('LVAE_FORCE_DIST', None)
    env.pop('LVAE_DDP_MODE', None)
    p = subprocess.run([sys.executable, WORKER, mode, out, str(steps), str(M)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=600)
    assert p.returncode == 0, p.stdout.decode()[-3000:]


def test_forced_rccl_rank_split_exchange_runs_once_per_step_and_changes_no_bit(tmp_path):
    a, b = str(tmp_path / 'plain.pt'), str(tmp_path / 'split.pt')
    steps, M = 4, 2
    _worker('plain', a, steps, M)
    _worker('rccl1_split', b, steps, M)
    ra, rb = torch.load(a), torch.load(b)
    diff = [k for k in ra['sd'] if not torch.equal(ra['sd'][k], rb['sd'][k])]
    diff += [k for k in ('exp_avg', 'exp_inf') if not torch.equal(ra[k], rb[k])]
    print('yardstick | forced RCCL rank, split, M=2, four steps: %d tensors differ from the plain accumulated step; exchanges at global '
          'steps %r; gscale %r' % (len(diff), rb['extra']['runs'], rb['extra']['gscale']))
    assert not diff, diff
    assert ra['extra']['losses'] == rb['extra']['losses'] and ra['opt_step'] == rb['opt_step'] == steps
    assert rb['extra']['runs'] == [1, 2, 3, 4]             # once per optimizer step, not once per micro-pass
    assert rb['extra']['launched'] == [0] and rb['extra']['gscale'] == 0.5
    for k in ra['sd']:
        if k.endswith('num_batches_tracked'):
            assert int(ra['sd'][k]) == int(rb['sd'][k]) == steps * M, k


# ---------------------------------------------------------------------------------------------------------------------------------
# 10. the trainer
# ---------------------------------------------------------------------------------------------------------------------------------
def test_trainer_accumulates_and_resumes_exactly(tmp_path):
    """--accum-steps 3 on device-fed data (43 images, batch 4: ten micro-batches per epoch, so step 4 crosses into epoch 1): four steps in
    one run against two steps, a checkpoint and two more from it."""
    import re
    from test_device_data_gpu import _ckpt_tensors, _main
    path = str(tmp_path / 'data.npz')
    np.savez(path, data=_images(43, 40).numpy())
    base = ['-d', 'cifar10', '--zdims', '8', '8', '--downsample', '1', '1', '--nfilters', '16', '--skip', '--gated', '--freebits', '1.0',
            '--batch-size', '4', '--seed', '3', '--log-every', '1', '--device-data', '--data-npz', path, '--accum-steps', '3']
    full, half, rest = (str(tmp_path / n) for n in ('full.pt', 'half.pt', 'rest.pt'))
    tr_a, _, out_a = _main(base + ['--steps', '4', '--save-checkpoint', full])
    tr_1, _, _ = _main(base + ['--steps', '2', '--save-checkpoint', half])
    tr_2, _, out_2 = _main(base + ['--steps', '4', '--resume', half, '--save-checkpoint', rest])
    print('yardstick | train lines of the whole run %r, of the resumed one %r' % (sorted(tr_a), sorted(tr_2)))
    assert sorted(tr_a) == [1, 2, 3, 4] and sorted(tr_1) == [1, 2] and sorted(tr_2) == [3, 4]
    assert re.search(r',acc3,', out_a) and '10 steps per epoch' in out_a and 'warning' not in out_2
    assert {**tr_1, **tr_2} == tr_a and len(set(tr_a.values())) == 4
    (fa, ma), (fb, mb) = _ckpt_tensors(full), _ckpt_tensors(rest)
    differ = [k for k in fa if not torch.equal(fa[k], fb[k])]
    print('yardstick | final checkpoints: %d of %d tensors differ; (global step, optimizer step, noise) %r' % (len(differ), len(fa), ma[:3]))
    assert ma == mb and ma[0] == 4 and ma[1] == 4 and ma[2]['step'] == 12
    assert fa.keys() == fb.keys() and not differ
    assert torch.load(full)['accum_steps'] == torch.load(half)['accum_steps'] == 3
    for k, v in torch.load(full)['model'].items():
        if k.endswith('num_batches_tracked'):
            assert int(v) == 12, k


# ---------------------------------------------------------------------------------------------------------------------------------
# 11. giving a step up
# ---------------------------------------------------------------------------------------------------------------------------------
def _fed_step(images, M=2):
    from lvae_amd.data import DeviceDataset
    from lvae_amd.engine import TrainStep
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax
    m, _ = _golden_model(PhiloxNoise(seed=7))
    ds = DeviceDataset(images, MICRO, seed=17)
    return m, ds, TrainStep(m, Adamax(m, lr=1e-3), use_graph=True, feed=ds, accum_steps=M)


@pytest.mark.parametrize('where', ['capture', 'eager'])
def test_abandoned_step_leaves_a_clean_state(where, monkeypatch):
    """An exception in the second micro-pass of an eager step (after the first one ran: the fold holds its scalars and the cursor has moved)
    or inside the capture of the micro-pass graph: the graphs are dropped, global_step and num_batches_tracked are put back, the fold's
    accumulator and counter are zero and the cursor stands at completed * M. The step then runs again; after a failed capture (during
    which nothing ran) the run ends where a run that never failed ends, within the bound tests/test_model_gpu.py sets for the same property
    of the plain step (a renewed capture lets the convolutions transform their own weights once more)."""
    K = _K()
    from lvae_amd import ops
    images = _images(40, 9)
    M = 2
    m0, ds0, s0 = _fed_step(images, M)
    for _ in range(5):
        s0()
    torch.cuda.synchronize()
    ref = m0.arena.params.clone()

    m1, ds1, s1 = _fed_step(images, M)
    fail_at = 2 if where == 'capture' else 1               # the third call captures; the second is an eager warm-up step
    for _ in range(fail_at):
        s1()
    real, calls = K.micro_fold, []

    def refusing(*a, **kw):
        calls.append(1)
        if where == 'capture' or len(calls) == 2:          # eager: the first micro-pass completes, the second fails
            raise RuntimeError('simulated failure in a micro-pass')
        return real(*a, **kw)

    monkeypatch.setattr(K, 'micro_fold', refusing)
    with pytest.raises(RuntimeError, match='simulated failure'):
        s1()
    monkeypatch.setattr(K, 'micro_fold', real)
    torch.cuda.synchronize()
    sd = m1.state_dict()
    tracked = sorted({int(sd[k]) for k in sd if k.endswith('num_batches_tracked')})
    print('yardstick | %s: after the failure global step %d, cursor %d, fold counter %d, fold accumulator max %g, num_batches_tracked %r' %
          (where, m1.global_step, int(ds1.cursor.item()), int(s1._mcount.item()), float(s1._macc.abs().max()), tracked))
    assert s1.graph_p is None and s1.graph_a is None and s1.graph_b is None and not ops._side.get('group_q')
    assert all(e['stamp'] is None for e in K.prepared.entries.values())
    assert m1.global_step == fail_at and int(ds1.cursor.item()) == fail_at * M
    assert int(s1._mcount.item()) == 0 and float(s1._macc.abs().max()) == 0.0 and tracked == [fail_at * M]
    for _ in range(5 - fail_at):
        s1()
    torch.cuda.synchronize()
    assert s1.graph_a is not None and m1.global_step == m0.global_step == 5 and int(ds1.cursor.item()) == int(ds0.cursor.item()) == 10
    if where == 'capture':                                 # nothing of the failed step ran: the same draws, the same batches
        worst = float((m1.arena.params - ref).abs().max())
        print('yardstick | capture: parameters after five steps against the run that never failed, max abs difference %.3g (bound 1e-6)' % worst)
        assert worst < 1e-6
        sd0, sd1 = m0.state_dict(), m1.state_dict()
        assert all(int(sd0[k]) == int(sd1[k]) == 10 for k in sd0 if k.endswith('num_batches_tracked'))
    else:
        assert bool(torch.isfinite(m1.arena.params).all())
