"""KL balancing on the GPU: kernels.kl_balance_fwd / kl_balance_bwd against tests/kl_balance_ref.py at the thread-stride edges and, bit for
bit, against the plain bookkeeping kernels where the rule is inactive or does not apply; balance.KlBalance inside the model's forward and
inside whole training steps of the tiny_cifar golden (batch 4), captured against eager across the end of the warm-up."""
import pytest
import torch

import kl_balance_ref as R
from conftest import load_golden
from spectral_ref import close_elem, close_sum
from test_ema_gpu import _fresh_table, _images, _model

pytestmark = pytest.mark.gpu


def _K():
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels as K
    return K


def _finite(*ts):
    for t in ts:
        assert t is None or bool(torch.isfinite(t).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# the two kernels
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def refs():
    """{(kind, akind, fb, active, L, N): (kl, alpha, r64, r32)}: every forward reference once, shared and left unchanged."""
    out = {}
    for L, N in R.SHAPES:
        for kind in R.KINDS:
            for akind in R.ALPHAS:
                kl, alpha = R.kl_values(kind, L, N), R.alpha_values(akind, L)
                _finite(kl, alpha)
                for fb in R.FREE_BITS:
                    for act in (True, False):
                        r64, r32 = R.forward(kl.double(), alpha.double(), fb, act), R.forward(kl, alpha, fb, act)
                        _finite(*r64.values(), *r32.values())
                        out[kind, akind, fb, act, L, N] = (kl, alpha, r64, r32)
    return out


def _launch_fwd(K, kl_d, fb, alpha_d, const, counter):
    if counter is None:
        return K.kl_balance_fwd(kl_d, fb, alpha_d, beta=const)
    step = torch.full((1,), counter, dtype=torch.int64, device='cuda')
    return K.kl_balance_fwd(kl_d, fb, alpha_d, beta=0.0, step=step, anneal_steps=R.ANNEAL_STEPS)   # (the constant is ignored)


@pytest.mark.parametrize('shape', R.SHAPES, ids=lambda s: '%dx%d' % s)
def test_forward_against_float64_and_the_plain_kernel(refs, shape):
    K = _K()
    L, N = shape
    for kind in R.KINDS:
        for akind in R.ALPHAS:
            kl, alpha = refs[kind, akind, 0.0, True, L, N][:2]
            kl_d, alpha_d = kl.cuda(), alpha.cuda()
            for fb in R.FREE_BITS:
                psep, pavg, pscal = K.kl_bookkeeping_fwd(kl_d, fb)
                for name, const, counter in R.BETAS:
                    act = R.active(const, counter)
                    _, _, r64, r32 = refs[kind, akind, fb, act, L, N]
                    ksep, kavg, scal, coeff = _launch_fwd(K, kl_d, fb, alpha_d, const, counter)
                    tag = '%s %s fb=%g %s %dx%d' % (kind, akind, fb, name, L, N)
                    # the plain numbers carry the plain kernel's bits, whatever beta is
                    assert torch.equal(ksep, psep) and torch.equal(kavg, pavg) and torch.equal(scal[1], pscal[1]), tag
                    if not act:   # the inactive condition, to the bit
                        assert torch.equal(scal[0], pscal[0]), tag
                        assert torch.equal(coeff, torch.ones(L, device='cuda')), tag
                    elif L == 1:
                        assert float(coeff[0]) == 1.0, tag
                    close_elem('coeff ' + tag, coeff, r64['coeff'], r32['coeff'])
                    close_sum('kl_loss ' + tag, scal[0], r64['kl_loss'], r32['kl_loss'], r64['loss_abs'])
                    if act:
                        assert abs(float(coeff.double().mean()) - 1.0) <= 1e-6, tag


@pytest.mark.parametrize('shape', R.SHAPES, ids=lambda s: '%dx%d' % s)
def test_backward_against_autograd_and_the_plain_kernel(shape):
    K = _K()
    L, N = shape
    g_sep, g_avg, g_scal = R.upstream(L, N)
    forms = [(g_sep, g_avg, g_scal), (None, g_avg, g_scal), (g_sep, None, g_scal), (g_sep, g_avg, None)]
    dev = lambda t: None if t is None else t.cuda()
    for kind in R.KINDS:
        for akind in R.ALPHAS:
            kl, alpha = R.kl_values(kind, L, N), R.alpha_values(akind, L)
            kl_d, alpha_d = kl.cuda(), alpha.cuda()
            for fb in R.FREE_BITS:
                for act in (True, False):
                    jobs = []
                    for i, (a, b, c) in enumerate(forms):                 # every reference before the launches
                        r64 = R.backward(kl.double(), alpha.double(), fb, act, a, b, c)
                        r32 = R.backward(kl, alpha, fb, act, a, b, c)
                        _finite(r64, r32, a, b, c)
                        jobs.append((i, a, b, c, r64, r32))
                    coeff = K.kl_balance_fwd(kl_d, fb, alpha_d, beta=0.3 if act else 1.0)[3]
                    for i, a, b, c, r64, r32 in jobs:
                        tag = 'dkl %s %s fb=%g %s form %d %dx%d' % (kind, akind, fb, 'active' if act else 'inactive', i, L, N)
                        dkl = K.kl_balance_bwd(kl_d, fb, coeff, dev(a), dev(b), dev(c))
                        close_elem(tag, dkl, r64, r32)
                        if not act:   # to the bit
                            assert torch.equal(dkl, K.kl_bookkeeping_bwd(kl_d, fb, dev(a), dev(b), dev(c))), tag
                        assert torch.equal(dkl, K.kl_balance_bwd(kl_d, fb, coeff, dev(a), dev(b), dev(c))), tag   # same inputs, same bits


def test_same_bits_twice_and_a_caller_owned_coeff():
    K = _K()
    kl, alpha = R.kl_values('random', 20, 1000).cuda(), R.alpha_values('spread', 20).cuda()
    a = K.kl_balance_fwd(kl, 0.5, alpha, beta=0.3)
    mine = torch.full((20,), -7.0, device='cuda')
    b = K.kl_balance_fwd(kl, 0.5, alpha, beta=0.3, coeff=mine)
    assert b[3] is mine and all(torch.equal(x, y) for x, y in zip(a, b))


def test_bad_arguments_are_refused():
    K = _K()
    from lvae_amd import _C
    kl, alpha = torch.zeros(3, 5, device='cuda'), torch.ones(3, device='cuda')
    out = [torch.zeros(5, device='cuda'), torch.zeros(3, device='cuda'), torch.zeros(2, device='cuda'), torch.zeros(3, device='cuda')]
    p = [t.data_ptr() for t in out]
    st = _C.stream_ptr()
    good = [kl.data_ptr(), 3, 5, 0.0, alpha.data_ptr(), 0.3, None, 0] + p + [st]
    _C.call('lvae_kl_balance_fwd_f32', *good)
    for i, bad in ((0, None), (1, 0), (1, -1), (2, 0), (4, None), (8, None), (9, None), (10, None), (11, None)):
        args = list(good)
        args[i] = bad
        with pytest.raises(_C.LvaeHipError):
            _C.call('lvae_kl_balance_fwd_f32', *args)
    dkl = torch.zeros(3, 5, device='cuda')
    good = [kl.data_ptr(), 3, 5, 0.0, out[3].data_ptr(), None, None, None, dkl.data_ptr(), st]
    _C.call('lvae_kl_balance_bwd_f32', *good)
    for i, bad in ((0, None), (1, 0), (2, -3), (4, None), (8, None)):
        args = list(good)
        args[i] = bad
        with pytest.raises(_C.LvaeHipError):
            _C.call('lvae_kl_balance_bwd_f32', *args)
    with pytest.raises(ValueError):
        K.kl_balance_fwd(kl, 0.0, torch.ones(4, device='cuda'))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# the model and whole steps: the tiny_cifar golden, batch 4
# ---------------------------------------------------------------------------------------------------------------------------------
LR = 1e-3


def _make(balance='square', counter=None):
    import lvae_amd  # noqa: F401
    from lvae_amd import optim
    from lvae_amd.balance import KlBalance
    from lvae_amd.noise import PhiloxNoise
    g = load_golden('tiny_cifar')
    _fresh_table()
    m = _model(g.cfg, g.state_dict(), PhiloxNoise(seed=3))
    if counter is not None:
        m.global_step = counter
    return m, optim.Adamax(m, lr=LR), None if balance is None else KlBalance(balance)


def _state(m, opt):
    sd = m.state_dict()
    st = {k: v.detach().clone() for k, v in sd.items() if not k.endswith(('weight', 'bias', 'top_prior_params'))}
    st.update(params=m.arena.params.detach().clone(), exp_avg=opt.exp_avg.clone(), exp_inf=opt.exp_inf.clone(), opt_step=opt.step_count.clone())
    return st


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _same_value(a, b, where):
    if isinstance(a, dict):
        assert isinstance(b, dict) and a.keys() == b.keys(), where
        for k in a:
            _same_value(a[k], b[k], '%s.%s' % (where, k))
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), where
        for k, (p, q) in enumerate(zip(a, b)):
            _same_value(p, q, '%s[%d]' % (where, k))
    elif a is None or b is None:
        assert a is None and b is None, where
    else:
        assert torch.equal(a, b), where


def _same_dicts(a, b):
    assert len(a) == 12
    _same_value(a, b, 'out')


def test_train_forward_balances_the_loss():
    from lvae_amd import engine
    from lvae_amd.balance import latent_ratios
    m, _, kb = _make()
    m.free_bits = 0.0
    x = _images(4, 60).cuda()
    engine.bind_kl_balance(m, kb, beta=0.3)
    assert m.kl_balance is kb and m.training
    mo = m(x)
    assert len(mo) == 12 and kb.coeff.shape == (m.n_layers,)
    coeff, kavg = kb.coeff.double().cpu(), mo['kl_avg_layerwise'].detach().double().cpu()
    assert bool(torch.isfinite(coeff).all()) and bool((coeff != 1).any()) and abs(float(coeff.mean()) - 1) <= 1e-6
    close_sum('kl_loss = sum coeff * kl_avg', mo['kl_loss'].detach(), (coeff * kavg).sum(), (coeff.float() * kavg.float()).sum(), (coeff * kavg.abs()).sum())
    assert abs(float(mo['kl_loss'].detach()) - float(kavg.sum())) > 1e-3 * abs(float(kavg.sum()))     # and it is not the plain one
    # the latents' heights are what the named rules assume
    heights = [z.shape[2] for z in mo['z']]
    assert [h // min(heights) for h in heights] == latent_ratios(m.downsample)[0]
    # the loss head: loss = recons + beta * kl_loss with the pass's own coefficients (kl_loss recomputed in float64)
    out = engine.forward_pass(m, x, beta=0.3, kl_balance=kb)
    coeff, kavg = kb.coeff.double().cpu(), out['kl_avg_layerwise'].detach().double().cpu()
    beta, recons = torch.tensor(0.3, dtype=torch.float32).double(), out['recons'].detach().double().cpu()
    want = recons + beta * (coeff * kavg).sum()
    close_sum('loss = recons + beta * kl_loss', out['loss'], want, want.float(), recons.abs() + beta * (coeff * kavg.abs()).sum())


def test_eval_mode_is_the_model_without_the_property():
    from lvae_amd import engine
    x = _images(4, 61).cuda()
    outs = []
    for balance in ('square', None):
        m, _, kb = _make(balance)
        if kb is not None:
            engine.bind_kl_balance(m, kb, beta=0.3)
        m.eval()
        with torch.no_grad():
            outs.append(m(x))
        if kb is not None:
            assert torch.equal(kb.coeff, torch.ones_like(kb.coeff))     # no training forward has written it
    _same_dicts(*outs)


def test_the_iw_bound_is_refused():
    from lvae_amd import engine
    from lvae_amd.balance import KlBalance
    m, opt, kb = _make()
    m.free_bits = 0.0
    with pytest.raises(ValueError, match='no balanced form'):
        engine.forward_pass(m, _images(4, 60).cuda(), beta=0.3, iw_samples=2, kl_balance=kb)
    with pytest.raises(ValueError, match='no balanced form'):
        engine.TrainStep(m, opt, iw_samples=2, kl_balance=KlBalance('equal'))
    assert m.kl_balance is None


def _run(use_graph, accum, balance='square', counter=None, steps=6, anneal=3):
    from lvae_amd.engine import TrainStep
    m, opt, kb = _make(balance, counter)
    st = TrainStep(m, opt, use_graph=use_graph, beta_anneal=anneal, accum_steps=accum, kl_balance=kb)
    coeffs = []
    for k in range(steps):
        x = _images(4, 60 + k) if accum == 1 else torch.cat([_images(4, 60 + 2 * k), _images(4, 61 + 2 * k)])
        st(x.cuda())
        if kb is not None:
            coeffs.append(kb.coeff.clone())
    torch.cuda.synchronize()
    assert (st.graph_a is not None) == use_graph
    return _state(m, opt), coeffs


@pytest.mark.parametrize('accum', [1, 2], ids=['plain', 'accum2'])
def test_captured_steps_equal_eager_steps_across_the_end_of_the_warm_up(accum):
    """Six steps with beta_anneal = 3: two eager steps, the capture and three replays against six eager steps. The fourth step's beta is 1,
    decided inside the replayed graph."""
    (cap, ccap), (eag, ceag) = _run(True, accum), _run(False, accum)
    _same(cap, eag)
    assert len(ccap) == len(ceag) == 6
    one = torch.ones_like(ccap[0])
    for k, (a, b) in enumerate(zip(ccap, ceag)):
        assert torch.equal(a, b), k
        assert bool(torch.isfinite(a).all())
        assert torch.equal(a, one) == (k >= 3), k      # steps 0..2: beta = k / 3 < 1; steps 3..5: exactly 1
    # and the balance is in the update: a run without it ends elsewhere
    plain, _ = _run(True, accum, balance=None)
    assert not torch.equal(plain['params'], cap['params'])


def test_after_the_warm_up_the_property_changes_no_bit():
    (a, ca), (b, _) = _run(True, 1, counter=5, steps=4), _run(True, 1, balance=None, counter=5, steps=4)
    _same(a, b)
    assert all(torch.equal(c, torch.ones_like(c)) for c in ca)


def test_recalibration_keeps_the_plain_bookkeeping(monkeypatch):
    """BatchNorm recalibration runs train-mode forwards without training: with the attribute set it must issue the plain bookkeeping launch,
    leave `coeff` alone, put the attribute back, and find the statistics a model without the attribute finds."""
    from lvae_amd import engine
    from lvae_amd import kernels as K
    from lvae_amd.recalibrate import recalibrate_bn
    x = _images(4, 62).cuda()
    batches = [_images(4, 70 + k) for k in range(3)]
    calls = []
    plain_fwd, balanced_fwd = K.kl_bookkeeping_fwd, K.kl_balance_fwd
    monkeypatch.setattr(K, 'kl_bookkeeping_fwd', lambda *a, **kw: (calls.append('plain'), plain_fwd(*a, **kw))[1])
    monkeypatch.setattr(K, 'kl_balance_fwd', lambda *a, **kw: (calls.append('balanced'), balanced_fwd(*a, **kw))[1])
    stats = []
    for balance in ('square', None):
        m, _, kb = _make(balance)
        if kb is not None:
            engine.bind_kl_balance(m, kb, beta=0.3)
        m(x)                                                  # one training forward: `coeff` is this pass's
        assert calls == ['plain' if kb is None else 'balanced']
        kept = None if kb is None else (kb.coeff, kb.coeff.clone())
        del calls[:]
        info = recalibrate_bn(m, [b.clone() for b in batches], use_graph=False)
        assert info['rounds'] == 3 and calls == ['plain'] * 3
        del calls[:]
        if kb is not None:
            assert m.kl_balance is kb and kb.coeff is kept[0] and torch.equal(kb.coeff, kept[1]) and bool((kept[1] != 1).any())
        stats.append({k: v.detach().clone() for k, v in m.state_dict().items() if 'running_' in k})
    assert stats[0] and stats[0].keys() == stats[1].keys()
    for k in stats[0]:
        assert torch.equal(stats[0][k], stats[1][k]), k
