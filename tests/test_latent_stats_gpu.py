"""Latent-usage statistics on the GPU (csrc/latent_stats.hip, lvae_amd.latent): the fold and finalize kernels against float64 torch /
numpy on identical inputs, their argument checks, the statistics of a test pass against the CPU oracle, and that a test pass is otherwise
untouched by them: eager and replayed, on averaged weights, and over two shards."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu


def _fresh_table():
    from lvae_amd import kernels as K
    K.prepared.entries.clear()
    K.prepared.table = None


def _model(cfg, sd, noise):
    import lvae_amd  # noqa: F401
    from lvae_amd.models.lvae import LadderVAE
    torch.manual_seed(0)
    m = LadderVAE(**cfg)
    m.load_state_dict(sd)
    m.cuda().train()
    m.noise = noise
    return m


def _images(n, seed):
    return torch.floor(256 * torch.rand(n, 3, 32, 32, generator=torch.Generator().manual_seed(seed))) / 255


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) the kernels against float64 on identical inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def _params(n, HW, Z, gen, mu_of=None):
    """(n, 1, HW, 2Z) fp32 (mu | logvar): mu ~ N(0, 0.3^2), logvar ~ U(-0.5, 0.5), drawn on the CPU"""
    mu = 0.3 * torch.randn(n, 1, HW, Z, generator=gen) if mu_of is None else mu_of(torch.randn(n, 1, HW, Z, generator=gen))
    lv = torch.rand(n, 1, HW, Z, generator=gen) - 0.5
    return torch.cat([mu, lv], dim=3).float().contiguous()


def _ref_sums(p, q):
    """float64 (3, U): sum mu_q, sum mu_q^2, sum KL(q || p) over the images, units in NHWC order"""
    Z = q.shape[3] // 2
    p, q = p.double(), q.double()
    qmu, qlv, pmu, plv = q[..., :Z], q[..., Z:], p[..., :Z], p[..., Z:]
    kl = 0.5 * ((qlv - plv).exp() + (qmu - pmu) ** 2 / plv.exp() - 1.0 - (qlv - plv))
    return torch.stack([qmu.sum(0).reshape(-1), (qmu * qmu).sum(0).reshape(-1), kl.expand_as(qmu).sum(0).reshape(-1)])


def _fold(p, q):
    from lvae_amd import kernels as K
    Z = q.shape[3] // 2
    sums = torch.zeros(3, q.shape[1] * q.shape[2] * Z, dtype=torch.float64, device='cuda')
    K.latent_stats_fold(p.cuda(), q.cuda(), sums)
    return sums


def _close(got, ref, rel, abs_=0.0):
    d = (got - ref).abs()
    bad = d > rel * ref.abs() + abs_
    assert not bool(bad.any()), (int(bad.sum()), float(d.max()), float((d / ref.abs().clamp_min(1e-300)).max()))


CASES = [(4, 4, 32, 0),      # the 2x2 level: fewer units than one workgroup
         (4, 4, 32, 1),      # the top layer's broadcast prior
         (37, 64, 32, 0),    # a batch that the slices do not divide
         (64, 256, 32, 0),   # several unit blocks x several batch slices
         (5, 9, 6, 0),       # Z not a multiple of 4, odd HW: the one-channel-per-thread form
         (1, 16, 32, 0)]     # one image: the variance is exactly 0, nothing is NaN


@pytest.mark.parametrize('N,HW,Z,p_bcast', CASES)
def test_fold_and_finalize_match_float64(N, HW, Z, p_bcast):
    from lvae_amd import kernels as K
    gen = torch.Generator().manual_seed(1000 * N + HW + Z + p_bcast)
    q = _params(N, HW, Z, gen)
    p = _params(1 if p_bcast else N, HW, Z, gen)
    ref = _ref_sums(p, q)
    sums = _fold(p, q)
    got = sums.cpu()
    _close(got[0], ref[0], 1e-12)                          # double sums of fp32 values: only the order differs
    _close(got[1], ref[1], 1e-12)
    _close(got[2] / N, ref[2] / N, 1e-5, 1e-6)             # the fp32 formula: four O(1) terms, < 10 roundings of 6e-8, doubled
    # three batches one after another = one fold of their concatenation
    if N >= 3:
        a, b = N // 3, 2 * N // 3
        parts = torch.zeros_like(sums)
        for lo, hi in ((0, a), (a, b), (b, N)):
            K.latent_stats_fold((p if p_bcast else p[lo:hi]).cuda(), q[lo:hi].cuda(), parts)
        _close(parts.cpu(), got, 1e-12)
    # finalize
    U = HW * Z
    unit = torch.full((3, U), float('nan'), dtype=torch.float64, device='cuda')
    layer = torch.full((4,), float('nan'), dtype=torch.float64, device='cuda')
    K.latent_stats_finalize(sums, N, 0.01, 0.01, unit, layer)
    unit, layer = unit.cpu(), layer.cpu()
    assert bool(torch.isfinite(unit).all()) and bool((unit[2] >= 0).all())
    mu = q[..., :Z].double().reshape(N, U).numpy()
    _close(unit[2], torch.from_numpy(np.var(mu, axis=0, ddof=0)), 1e-9, 1e-15)
    _close(unit[1], torch.from_numpy(mu.mean(0)), 1e-12, 1e-15)
    assert torch.equal(unit[0], got[2] * (1.0 / N))
    if N == 1:
        assert bool((unit[2] == 0).all())
    assert layer.tolist()[:3] == [float((unit[0] > 0.01).sum()), float((unit[2] > 0.01).sum()), float(U)]
    _close(layer[3], unit[0].sum(), 1e-12)
    assert 0 < layer[0] <= U                                # (p and q differ: the KL of most units is far above 0.01)


def test_launches_give_the_same_bits_again():
    gen = torch.Generator().manual_seed(5)
    q, p = _params(37, 64, 32, gen), _params(37, 64, 32, gen)
    assert torch.equal(_fold(p, q), _fold(p, q))


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) cancellation
# ---------------------------------------------------------------------------------------------------------------------------------
def test_variance_of_a_large_mean_needs_the_double_sums():
    from lvae_amd import kernels as K
    gen = torch.Generator().manual_seed(9)
    N, HW, Z = 64, 4, 32
    q = _params(N, HW, Z, gen, mu_of=lambda e: 100.0 + 0.01 * e)
    p = _params(N, HW, Z, gen)
    sums = _fold(p, q)
    unit = torch.empty((3, HW * Z), dtype=torch.float64, device='cuda')
    layer = torch.empty((4,), dtype=torch.float64, device='cuda')
    K.latent_stats_finalize(sums, N, 0.01, 0.01, unit, layer)
    ref = torch.from_numpy(np.var(q[..., :Z].double().reshape(N, HW * Z).numpy(), axis=0, ddof=0))
    assert 2e-5 < float(ref.min()) and float(ref.max()) < 5e-4   # about 1e-4, below mean^2 = 1e4 by eight orders: fp32 sums hold none of it
    _close(unit[2].cpu(), ref, 1e-6)


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) bad arguments
# ---------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch():
    import lvae_amd  # noqa: F401
    from lvae_amd import _C
    gen = torch.Generator().manual_seed(2)
    N, HW, Z = 8, 16, 32
    q, p = _params(N, HW, Z, gen).cuda(), _params(N, HW, Z, gen).cuda()
    sums = torch.zeros(3, HW * Z, dtype=torch.float64, device='cuda')
    lib = _C.load()
    need = lib.lvae_latent_stats_workspace(N, HW, Z)
    assert need >= 3 * HW * Z * 8 and lib.lvae_latent_stats_workspace(0, HW, Z) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device='cuda')
    sp = _C.stream_ptr()
    args = lambda n, nbytes: (p.data_ptr(), 0, q.data_ptr(), n, HW, Z, sums.data_ptr(), ws.data_ptr(), nbytes, sp)
    for n, nbytes in ((N, need - 1), (0, need)):
        assert lib.lvae_latent_stats_fold_f32(*args(n, nbytes)) == -1          # LVAE_EINVAL
        with pytest.raises(_C.LvaeHipError):
            _C.call('lvae_latent_stats_fold_f32', *args(n, nbytes))
    with pytest.raises(_C.LvaeHipError):
        _C.call('lvae_latent_stats_fold_f32', None, 0, q.data_ptr(), N, HW, Z, sums.data_ptr(), ws.data_ptr(), need, sp)
    unit = torch.zeros((3, HW * Z), dtype=torch.float64, device='cuda')
    layer = torch.zeros((4,), dtype=torch.float64, device='cuda')
    with pytest.raises(_C.LvaeHipError):
        _C.call('lvae_latent_stats_finalize_f64', sums.data_ptr(), HW * Z, 0, 0.01, 0.01, unit.data_ptr(), layer.data_ptr(), sp)
    torch.cuda.synchronize()
    assert not bool(sums.any()) and not bool(ws.any()) and not bool(unit.any()) and not bool(layer.any())   # nothing was launched
    _C.call('lvae_latent_stats_fold_f32', *args(N, need))                      # and the same call with enough room goes through
    assert bool(sums.any())


# ---------------------------------------------------------------------------------------------------------------------------------
# (d) a test pass against the CPU oracle
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def oracle_pass():
    """tiny_cifar in eval mode over three batches of 4: the oracle's noise tape and, per layer, float64 per-unit kl / mu_mean / mu_var
    (Z, h, w) restated from the p_params / q_params its stochastic blocks saw. Computed once; nothing under oracle/ changes."""
    from oracle import lvae_ref as R
    g = load_golden('tiny_cifar')
    gen = torch.Generator().manual_seed(7)
    xs = [g.t('x')] + [torch.floor(256 * torch.rand(4, 3, 32, 32, generator=gen)) / 255 for _ in range(2)]
    tape = R.Tape(gen=torch.Generator().manual_seed(11))
    seen, orig = [], R.stochastic_block

    def recording(*a, **kw):
        out, data = orig(*a, **kw)
        seen.append((data['p_params'], data['q_params']))
        return out, data

    R.stochastic_block = recording
    try:
        with torch.no_grad():
            for x in xs:
                R.lvae_forward({k: v.clone() for k, v in g.state_dict().items()}, g.cfg, x, tape, training=False)
    finally:
        R.stochastic_block = orig
    L = len(g.cfg['z_dims'])
    assert len(seen) == 3 * L
    ref = []
    for i in range(L):                                     # a forward visits the layers top first
        calls = [seen[b * L + (L - 1 - i)] for b in range(3)]
        q = torch.cat([c[1] for c in calls]).double()
        p = torch.cat([c[0].expand_as(c[1]) for c in calls]).double()
        Z = q.shape[1] // 2
        qmu, qlv, pmu, plv = q[:, :Z], q[:, Z:], p[:, :Z], p[:, Z:]
        kl = 0.5 * ((qlv - plv).exp() + (qmu - pmu) ** 2 / plv.exp() - 1.0 - (qlv - plv))
        ref.append({'kl': kl.mean(0).numpy(), 'mu_mean': qmu.mean(0).numpy(), 'mu_var': qmu.var(0, unbiased=False).numpy()})
    return g, xs, tape.entries, ref


def _pass_on_tape(g, xs, entries, cfg=None, **thresholds):
    from lvae_amd.evaluate import test_pass
    from lvae_amd.latent import LatentStats
    from lvae_amd.noise import TapeNoise
    _fresh_table()
    m = _model(cfg or g.cfg, g.state_dict(), None)
    noise = TapeNoise(entries)
    stats = LatentStats(m, 'cuda', **thresholds)
    res = test_pass(m, [x.cuda() for x in xs], 1, noise=noise, latent_stats=stats)
    assert noise.exhausted() and res['n_images'] == 12
    return res


def test_test_pass_statistics_match_the_oracle(oracle_pass):
    """Per-unit kl, mu_mean and mu_var of every layer within 1e-3 |ref| + 1e-5 of the float64 restatement of the oracle's tensors (loose on
    purpose: this pins the plumbing; the arithmetic is pinned by the kernel tests), and the counts of active units outside the band around
    the threshold. Largest deviation measured on an MI355X: not measured yet (the test prints it per layer and array, in units of the
    bound; run with -s). A deviation above a tenth of the bound wants an explanation, not a wider bound."""
    g, xs, entries, ref = oracle_pass
    res = _pass_on_tape(g, xs, entries, kl_threshold=0.01, var_threshold=1e-3)
    L = len(ref)
    arrays = res['latent_arrays']
    assert len(arrays) == L and [a['kl'].shape for a in arrays] == [r['kl'].shape for r in ref] == [(8, 16, 16), (8, 8, 8), (8, 4, 4)]
    worst = {}
    for i in range(L):
        for k in ('kl', 'mu_mean', 'mu_var'):
            got, want = arrays[i][k], ref[i][k]
            assert got.dtype == np.float64
            ratio = float((np.abs(got - want) / (1e-3 * np.abs(want) + 1e-5)).max())
            worst[k] = max(worst.get(k, 0.0), ratio)
            print('layer %d %s: largest deviation %.4f of the bound' % (i, k, ratio))
            assert ratio <= 1.0, (i, k, ratio)
    print('largest deviation in units of the bound:', worst)
    tot = {'kl': 0, 'var': 0}
    for i in range(L):
        U = ref[i]['kl'].size
        assert res['latent/units_layer_%d' % i] == U
        for key, name, thr in (('kl', 'kl', 0.01), ('var', 'mu_var', 1e-3)):
            want, got = ref[i][name], arrays[i][name]
            band = np.abs(want - thr) <= 1e-3 * np.abs(want) + 1e-5        # units the value tolerance cannot place
            assert band.sum() <= 0.03 * U, (i, key, int(band.sum()))
            active = int(((want > thr) & ~band).sum())
            assert 0 < active and int(((want <= thr) & ~band).sum()) > 0   # both sides of the threshold are populated
            assert int(((got > thr) & ~band).sum()) == active, (i, key)
            n = res['latent/active_%s_layer_%d' % (key, i)]
            assert n == int((got > thr).sum()) and active <= n <= active + int(band.sum()), (i, key, n, active)
            tot[key] += n
    assert res['latent/active_kl'] == tot['kl'] and res['latent/active_var'] == tot['var']
    # the reference's counts themselves (units in the band: KL 0, 1, 0 and variance 22, 6, 0)
    assert [int((r['kl'] > 0.01).sum()) for r in ref] == [1584, 417, 87]
    assert [int((r['mu_var'] > 1e-3).sum()) for r in ref] == [1386, 238, 12]


def test_per_unit_kl_sums_to_the_layers_kl(oracle_pass):
    """sum_u kl[u] against the pass's own kl_layers/kl_layer_<i>. The per-unit KL is analytical whatever `analytical_kl` is, and the
    fixture's layer KL is the Monte-Carlo one (log q(z) - log p(z)), which differs from it by sampling noise (39.99 against 43.28 in layer
    0): the two are the same quantity, and are compared, on the model with analytical_kl=True (same weights, same draws)."""
    g, xs, entries, ref = oracle_pass
    assert g.cfg['analytical_kl'] is False
    res = _pass_on_tape(g, xs, entries, cfg=dict(g.cfg, analytical_kl=True))
    for i, a in enumerate(res['latent_arrays']):
        got, want = float(a['kl'].sum()), res['kl_layers/kl_layer_%d' % i]
        print('layer %d: sum of per-unit KL %.6f, kl_layer %.6f' % (i, got, want))
        assert abs(got - want) <= 1e-5 * abs(want) + 1e-4, (i, got, want)
        assert abs(got - float(ref[i]['kl'].sum())) <= 1e-3 * float(ref[i]['kl'].sum())   # and the oracle's, whatever the flag
    # default thresholds: 0.01 for both
    assert res['latent/active_var'] == sum(int((a['mu_var'] > 0.01).sum()) for a in res['latent_arrays'])


# ---------------------------------------------------------------------------------------------------------------------------------
# (e) the pass is otherwise untouched
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_pass_is_bit_for_bit_the_pass_without_statistics():
    from lvae_amd.evaluate import test_pass
    from lvae_amd.latent import LatentStats
    from lvae_amd.noise import PhiloxNoise
    g = load_golden('tiny_cifar')
    m = _model(g.cfg, g.state_dict(), PhiloxNoise(1))
    xs = [_images(5, 2).cuda(), _images(5, 3).cuda()]
    stats = LatentStats(m, 'cuda')
    out = {}
    for use_graph in (False, True):
        plain_noise, noise = PhiloxNoise(seed=21), PhiloxNoise(seed=21)
        plain = test_pass(m, xs, 3, noise=plain_noise, use_graph=use_graph)
        with_stats = test_pass(m, xs, 3, noise=noise, use_graph=use_graph, latent_stats=stats)
        assert int(noise.step.item()) == int(plain_noise.step.item()) >= 2 * 3   # the counter moved exactly as in the plain pass
        for k in plain:
            assert with_stats[k] == plain[k], (use_graph, k, with_stats[k], plain[k])
        extra = set(with_stats) - set(plain)
        assert 'latent_arrays' in extra and all(k == 'latent_arrays' or k.startswith('latent/') for k in extra)
        assert not bool(stats.buf.any()) and stats.n_local == 0   # take() left the accumulator empty
        out[use_graph] = with_stats
        if use_graph:
            # a second pass on the same object (and the same captured plan) starts from zero
            plans = dict(m._test_graphs)
            noise.step.zero_()
            again = test_pass(m, xs, 3, noise=noise, use_graph=True, latent_stats=stats)
            assert all(m._test_graphs[k] is v for k, v in plans.items()) and len(m._test_graphs) == len(plans)
            assert _same(again, with_stats)
    # replayed = eager, bit for bit, statistics included; and the plain plans were not replaced by the ones that fold
    assert _same(out[True], out[False])
    assert sorted(k[-1] is None for k in m._test_graphs) == [False, True]
    # only the first sample of a batch is folded: the statistics of a 3-sample pass are those of a 1-sample pass on the same first draws
    first = test_pass(m, xs[:1], 1, noise=PhiloxNoise(seed=21), use_graph=False, latent_stats=stats)
    three = test_pass(m, xs[:1], 3, noise=PhiloxNoise(seed=21), use_graph=False, latent_stats=stats)
    assert first['n_images'] == three['n_images'] == 5
    assert all(np.array_equal(a[k], b[k]) for a, b in zip(first['latent_arrays'], three['latent_arrays']) for k in a)


def _same(a, b):
    if a.keys() != b.keys():
        return False
    for k in a:
        if k == 'latent_arrays':
            if not all(np.array_equal(x[n], y[n]) for x, y in zip(a[k], b[k]) for n in x):
                return False
        elif a[k] != b[k]:
            return False
    return True


# ---------------------------------------------------------------------------------------------------------------------------------
# (f) averaged weights
# ---------------------------------------------------------------------------------------------------------------------------------
def test_statistics_of_the_averaged_weights():
    from lvae_amd.checkpoint import ema_state_dict_reference_layout
    from lvae_amd.engine import TrainStep
    from lvae_amd.evaluate import test_pass
    from lvae_amd.latent import LatentStats
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax
    g = load_golden('tiny_cifar')
    _fresh_table()
    m = _model(g.cfg, g.state_dict(), PhiloxNoise(seed=3))
    opt = Adamax(m, lr=1e-3, ema_decay=0.5)
    st = TrainStep(m, opt, use_graph=False)
    for k in range(2):
        st(_images(4, 10 + k).cuda())
    xt = [_images(5, 30).cuda(), _images(3, 31).cuda()]
    avg_sd = ema_state_dict_reference_layout(m, opt)
    before = m.arena.params.clone()
    got = test_pass(m, xt, 2, noise=PhiloxNoise(seed=21), optimizer=opt, use_graph=False, latent_stats=LatentStats(m, 'cuda'))
    torch.cuda.synchronize()
    assert torch.equal(m.arena.params, before)            # the parameters are back, bit for bit
    assert got.pop('weights') == 'ema'
    m2 = _model(g.cfg, avg_sd, PhiloxNoise(1))
    want = test_pass(m2, xt, 2, noise=PhiloxNoise(seed=21), use_graph=False, latent_stats=LatentStats(m2, 'cuda'))
    assert _same(got, want)
    m3 = _model(g.cfg, g.state_dict(), PhiloxNoise(1))    # and they are not the statistics of other weights
    other = test_pass(m3, xt, 2, noise=PhiloxNoise(seed=21), use_graph=False, latent_stats=LatentStats(m3, 'cuda'))
    assert not np.array_equal(other['latent_arrays'][0]['kl'], got['latent_arrays'][0]['kl'])


# ---------------------------------------------------------------------------------------------------------------------------------
# (g) two shards
# ---------------------------------------------------------------------------------------------------------------------------------
def test_two_shards_added_give_the_whole_set():
    """What take()'s all-reduce does between ranks, stated in one process: the buffers of two objects that folded one shard each, added,
    finalize to what one object that folded both shards gives."""
    from lvae_amd.latent import LatentStats
    from lvae_amd.noise import PhiloxNoise
    g = load_golden('tiny_cifar')
    m = _model(g.cfg, g.state_dict(), PhiloxNoise(1))
    m.eval()
    xa, xb = _images(5, 40).cuda(), _images(3, 41).cuda()

    def fold(stats, x, seed):
        from lvae_amd.evaluate import _test_bottom_up
        with torch.no_grad():
            m.noise = PhiloxNoise(seed)
            bu, _ = _test_bottom_up(m, x)
            m.noise.begin(x.device)
            m._topdown(bu, latent_stats=stats)
            m.noise.end()
        stats.count(x.shape[0])

    whole, a, b = LatentStats(m, 'cuda'), LatentStats(m, 'cuda'), LatentStats(m, 'cuda')
    fold(whole, xa, 1)
    fold(whole, xb, 2)
    fold(a, xa, 1)
    fold(b, xb, 2)
    assert float(a.buf[0]) == 5 and float(b.buf[0]) == 3 and bool(b.buf[1:].any())
    a.merge(b)
    assert float(a.buf[0]) == float(whole.buf[0]) == 8
    one, two = whole.take(), a.take()
    assert one['n_images'] == two['n_images'] == 8
    for k in one:
        if k.startswith('latent/'):
            assert one[k] == two[k], k
    for x, y in zip(one['arrays'], two['arrays']):
        for n in x:
            d = np.abs(x[n] - y[n])
            assert bool((d <= 1e-12 * np.abs(x[n])).all()), (n, float(d.max()))
    with pytest.raises(ValueError):
        whole.take()                                       # nothing folded since the last take()
