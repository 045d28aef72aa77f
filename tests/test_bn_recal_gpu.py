"""BatchNorm recalibration on the GPU: the two kernels bit for bit against a sequential float64 loop, the recalibrated statistics of a
model against the CPU oracle for both sources, and what the call promises: eager equals replayed, everything else is put back, training
is not perturbed, the trainer's test pass and checkpoint use the recalibrated statistics, the evaluator runs end to end.

Tolerance of the oracle comparisons (ORACLE_TOL below). The rule: the worst absolute and relative error of the running statistics after
ONE ordinary train-mode forward of the engine as it was BEFORE this feature (the forward pass is the same code now), against the oracle
on the same inputs; twice that is allowed. Measured on an MI355X, for each of the three data batches the test uses (golden weights, the
statistics zeroed first so that a statistic reads as running / 0.1 on both sides, as the oracle's has to be read anyway), per
statistics tensor t of one BatchNorm:
    absolute  a(t) = max_c |engine - oracle|            relative  r(t) = a(t) / max_c |oracle|   (normwise: a channel mean near 0 has no
                                                                                                   meaningful error relative to itself)
    tiny_mnist: worst a = 1.862645e-07, worst r = 1.150611e-06        tiny_cifar: worst a = 2.235174e-07, worst r = 1.822751e-06
The recalibrated output plays no part in these numbers (measured by a script that never calls recalibrate_bn), and the same bounds hold
for the prior source."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

STAT = ('running_mean', 'running_var')
# name -> (worst absolute, worst relative) error of one ordinary forward; the tests allow twice each
ORACLE_TOL = {'tiny_mnist': (1.862645e-07, 1.150611e-06), 'tiny_cifar': (2.235174e-07, 1.822751e-06)}


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the kernels
# ---------------------------------------------------------------------------------------------------------------------------------
LENGTHS = (1, 3, 64, 100, 257)
SPECIAL = np.array([1e-30, -0.0, 3e38, -3e38, 1.0000001, -1e-30, 0.0, 16777217.0], dtype=np.float32)


def _values(n, seed):
    """n float32 values with the special ones written over the front (as many as fit)"""
    v = np.random.default_rng(seed).standard_normal(n).astype(np.float32)
    k = min(n, SPECIAL.size)
    v[:k] = np.roll(SPECIAL, seed)[:k]
    return v


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def _ref_mean(folds):
    """the sequential float64 loop: acc += x per fold, then / n, then float32"""
    acc = np.zeros(folds[0].shape, dtype=np.float64)
    for x in folds:
        acc += x
    with np.errstate(over='ignore', invalid='ignore'):
        return (acc / len(folds)).astype(np.float32)


def _table():
    from lvae_amd import kernels as K
    stats = [torch.zeros(n, dtype=torch.float32, device='cuda') for n in LENGTHS]
    accs = [torch.zeros(n, dtype=torch.float64, device='cuda') for n in LENGTHS]
    count = torch.zeros(2, dtype=torch.int64, device='cuda')
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    return K, stats, accs, K.bn_recal_table(list(zip(stats, accs)), 'cuda'), count, flag


@pytest.mark.parametrize('n_folds', [1, 3])
def test_fold_and_finish_match_sequential_float64_bit_for_bit(n_folds):
    K, stats, accs, table, count, flag = _table()
    assert tuple(table.shape) == (len(LENGTHS), 3) and table.dtype == torch.int64
    KEPT = 3                                              # entry 3 (100 values) is written once and never rewritten between folds
    for cycle in range(2):                                # a second cycle on the same table: same inputs, same bits
        folds = [[_values(n, 10 * f + e) for e, n in enumerate(LENGTHS)] for f in range(n_folds)]
        for f in range(n_folds):
            for e, s in enumerate(stats):
                if f == 0 or e != KEPT:
                    s.copy_(torch.from_numpy(folds[f][e]))
            K.bn_recal_fold(table, count)
            assert count.tolist() == [f + 1, 0]
        K.bn_recal_finish(table, count, flag)
        torch.cuda.synchronize()
        for e, s in enumerate(stats):
            want = _ref_mean([folds[0][e] if e == KEPT else folds[f][e] for f in range(n_folds)])
            assert np.array_equal(_bits(s.cpu().numpy()), _bits(want)), (cycle, e)
        # the entry nobody rewrote comes back bit for bit (its one -0.0 aside, which n additions to +0.0 return as +0.0)
        kept, got = folds[0][KEPT], stats[KEPT].cpu().numpy()
        nz = _bits(kept) != _bits(np.float32(-0.0))
        assert np.array_equal(_bits(got)[nz], _bits(kept)[nz]) and (got[~nz] == 0).all() and int((~nz).sum()) == 1
        assert count.tolist() == [0, 0] and flag.item() == 0
        assert all(int((a != 0).sum()) == 0 for a in accs)


def test_a_non_finite_mean_sets_the_flag_and_nothing_else_does():
    K, stats, accs, table, count, flag = _table()
    for e, s in enumerate(stats):
        s.copy_(torch.from_numpy(_values(LENGTHS[e], e)))   # 3e38 and -3e38 once each: finite after one fold
    K.bn_recal_fold(table, count)
    K.bn_recal_finish(table, count, flag)
    assert flag.item() == 0
    for bad in (float('inf'), float('nan')):
        flag.zero_()
        stats[2][63] = bad                                   # the last element of the 64-entry
        K.bn_recal_fold(table, count)
        stats[2][63] = 1.0
        K.bn_recal_fold(table, count)
        K.bn_recal_finish(table, count, flag)
        assert flag.item() == 1 and count.tolist() == [0, 0]
        assert not np.isfinite(float(stats[2][63])) and bool(torch.isfinite(stats[4]).all())
        stats[2][63] = 1.0
    flag.zero_()
    before = [s.clone() for s in stats]
    K.bn_recal_finish(table, count, flag)                    # no fold since the last finish: nothing is written
    assert all(torch.equal(a, b) for a, b in zip(stats, before)) and flag.item() == 0 and count.tolist() == [0, 0]


def test_wrappers_refuse_what_the_kernels_cannot_take():
    K, stats, accs, table, count, flag = _table()
    E = K._C.LvaeHipError
    with pytest.raises(E):
        K.bn_recal_table([(stats[0], accs[1])], 'cuda')                        # two lengths
    with pytest.raises(E):
        K.bn_recal_table([(stats[0], stats[0])], 'cuda')                       # a float32 accumulator
    with pytest.raises(E):
        K.bn_recal_table([], 'cuda')
    with pytest.raises(E):
        K.bn_recal_fold(table, count[:1])                                      # the count is int64[2]
    with pytest.raises(E):
        K.bn_recal_finish(table, count, flag.to(torch.int64))
    with pytest.raises(E):
        K.bn_recal_fold(table.view(-1), count)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. a model's recalibrated statistics against the CPU oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def _model(cfg, sd, noise, training=True):
    import lvae_amd  # noqa: F401
    from lvae_amd.models.lvae import LadderVAE
    torch.manual_seed(0)
    m = LadderVAE(**cfg)
    m.load_state_dict(sd)
    m.cuda().train(training)
    m.noise = noise
    return m


def _stat_keys(sd):
    return [k for k in sd if k.endswith(STAT)]


def _batches(g, n=3):
    """n batches of 4 images in the data's own format: the golden batch first, then seeded ones"""
    x0 = g.t('x')
    out = [x0]
    for b in range(1, n):
        u = torch.rand(x0.shape, generator=torch.Generator().manual_seed(900 + b))
        out.append((u > 0.5).float() if g.cfg['likelihood_form'] == 'bernoulli' else torch.floor(256 * u) / 255)
    return out


def _scrambled(sd, poison=False):
    """the state dict with every running statistic replaced by seeded values (a fresh model's 0 / 1 would hide a statistic that was not
    put back); with poison a NaN mean and an Inf variance in the first BatchNorm of the final top-down block, which both sources run"""
    gen = torch.Generator().manual_seed(77)
    sd = {k: v.clone() for k, v in sd.items()}
    for k in _stat_keys(sd):
        r = torch.randn(sd[k].shape, generator=gen)
        sd[k] = r if k.endswith('running_mean') else r.abs() + 0.5
    if poison:
        k = next(k for k in sd if k.startswith('final_top_down.') and k.endswith('running_mean'))
        sd[k][0] = float('nan')
        sd[k.replace('running_mean', 'running_var')][1] = float('inf')
    return sd


class _Tempered:
    """Round an oracle tape (tests/test_conditional_gpu.py's TemperedTape): the tape records the unscaled draw, a `normal` draw is
    handed out multiplied by t."""

    def __init__(self, tape, t):
        self.tape, self.t = tape, t

    def draw(self, kind, shape, **kw):
        d = self.tape.draw(kind, shape, **kw)
        return d * self.t if kind == 'normal' else d


def oracle_rounds(g, source, xs=None, rounds=3, rows=4, temperature=0.7):
    """The oracle's per-round batch statistics. Its BatchNorm has momentum 0.1 built in: the running statistics are zeroed before each
    round and the batch statistic is read as running / 0.1 (float64). -> ([{key: statistic} per round], [tape entries per round],
    the keys whose BatchNorm ran)."""
    from oracle import lvae_ref as R
    sd = g.state_dict()
    keys = _stat_keys(sd)
    per_round, tapes, ran = [], [], None
    for b in range(rounds):
        for k in keys:
            sd[k].zero_()
        nbt = {k: int(sd[k]) for k in sd if k.endswith('num_batches_tracked')}
        tape = R.Tape(gen=torch.Generator().manual_seed(40 + b))
        with torch.no_grad():
            if source == 'data':
                R.lvae_forward(sd, g.cfg, xs[b], tape, training=True)
            else:
                R.sample_prior(sd, g.cfg, rows, _Tempered(tape, temperature), training=True)
        per_round.append({k: sd[k].double() / 0.1 for k in keys})
        tapes.append(tape.entries)
        now = {k.rsplit('.', 1)[0] for k in nbt if int(sd[k]) == nbt[k] + 1}
        assert ran is None or ran == now
        ran = now
    return per_round, tapes, [k for k in keys if k.rsplit('.', 1)[0] in ran]


def stat_errors(got, want, keys):
    """(worst absolute, worst normwise relative) error over the statistics tensors `keys`: got {key: tensor}, want {key: float64 tensor}"""
    worst_a = worst_r = 0.0
    for k in keys:
        a = float((got[k].double().cpu() - want[k]).abs().max())
        worst_a, worst_r = max(worst_a, a), max(worst_r, a / float(want[k].abs().max()))
    return worst_a, worst_r


def _check_against_oracle(name, source, got, want, keys):
    tol_a, tol_r = ORACLE_TOL[name]
    assert all(bool(torch.isfinite(got[k]).all()) for k in keys)
    a, r = stat_errors(got, want, keys)
    print('%s, %s source: worst |engine - oracle| = %.3e (allowed %.3e), worst relative = %.3e (allowed %.3e), %d tensors'
          % (name, source, a, 2 * tol_a, r, 2 * tol_r, len(keys)))
    assert a <= 2 * tol_a and r <= 2 * tol_r, (a, r)


def _mean_of_rounds(per_round, keys):
    return {k: sum(r[k] for r in per_round) / len(per_round) for k in keys}


@pytest.mark.parametrize('name', ['tiny_mnist', 'tiny_cifar'])
def test_data_source_matches_oracle(name):
    from lvae_amd.noise import TapeNoise
    from lvae_amd.recalibrate import recalibrate_bn
    g = load_golden(name)
    xs = _batches(g)
    per_round, tapes, ran = oracle_rounds(g, 'data', xs)
    keys = _stat_keys(g.state_dict())
    assert ran == keys                                               # a full forward runs every BatchNorm
    noise = TapeNoise([e for t in tapes for e in t])
    m = _model(g.cfg, _scrambled(g.state_dict(), poison=True), None)
    info = recalibrate_bn(m, xs, noise=noise)
    assert info == {'rounds': 3, 'source': 'data', 'n_bn': len(keys) // 2} and noise.exhausted()
    got = {k: v.detach().clone() for k, v in m.state_dict().items() if k in keys}
    _check_against_oracle(name, 'data', got, _mean_of_rounds(per_round, keys), keys)


@pytest.mark.parametrize('name', ['tiny_mnist', 'tiny_cifar'])
def test_prior_source_matches_oracle_and_leaves_the_rest_alone(name):
    """Which BatchNorms a train-mode pass from the prior runs is read off the oracle (its num_batches_tracked): the top-down blocks, the
    final top-down blocks and, with stochastic_skip (both goldens), every layer's skip_connection_merger, which the generative path applies
    too (oracle/lvae_ref.py top_down_layer) and which is therefore compared with the oracle like them. The bottom-up layers, the first
    bottom-up block and every merge layer are not run: their statistics are bit for bit what they were."""
    from lvae_amd.noise import TapeNoise
    from lvae_amd.recalibrate import recalibrate_bn
    g = load_golden(name)
    per_round, tapes, ran = oracle_rounds(g, 'prior')
    keys = _stat_keys(g.state_dict())
    idle = [k for k in keys if k.startswith(('bottom_up_layers.', 'first_bottom_up.')) or '.merge.' in k]
    assert idle and sorted(idle + ran) == sorted(keys)               # the oracle ran exactly the others
    assert any('.skip_connection_merger.' in k for k in ran) and not any('.skip_connection_merger.' in k for k in idle)
    noise = TapeNoise([e for t in tapes for e in t])
    old = _scrambled(g.state_dict(), poison=True)
    m = _model(g.cfg, old, None)
    info = recalibrate_bn(m, n_prior=3, prior_batch=4, temperature=0.7, noise=noise)
    assert info == {'rounds': 3, 'source': 'prior', 'n_bn': len(keys) // 2} and noise.exhausted()
    got = {k: v.detach().clone() for k, v in m.state_dict().items() if k in keys}
    _check_against_oracle(name, 'prior', got, _mean_of_rounds(per_round, ran), ran)
    for k in idle:
        assert np.array_equal(_bits(got[k].cpu().numpy()), _bits(old[k].numpy())), k


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. what the call promises
# ---------------------------------------------------------------------------------------------------------------------------------
def _images(n, seed):
    return torch.floor(256 * torch.rand(n, 3, 32, 32, generator=torch.Generator().manual_seed(seed))) / 255


def _stats(m):
    return torch.cat([b.detach().reshape(-1) for bn in m.bn_modules() for b in (bn.running_mean, bn.running_var)]).clone()


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.fixture(scope='module')
def cifar():
    from lvae_amd.noise import PhiloxNoise
    g = load_golden('tiny_cifar')
    return _model(g.cfg, _scrambled(g.state_dict()), PhiloxNoise(seed=5))


@pytest.mark.parametrize('source', ['data', 'prior'])
def test_eager_equals_replayed_for_nine_rounds(cifar, source):
    from lvae_amd.recalibrate import recalibrate_bn, restore_bn
    m = cifar
    old = _stats(m)
    kw = dict(batches=[_images(4, 200 + k) for k in range(9)]) if source == 'data' else dict(n_prior=9, prior_batch=4, temperature=0.7)
    res = {}
    for tag, use_graph in (('eager', False), ('graph', True), ('auto', None)):   # (auto: 9 rounds of one shape on Philox noise -> replayed)
        info = recalibrate_bn(m, use_graph=use_graph, step=3, **kw)
        assert info['rounds'] == 9
        res[tag] = _stats(m)
        restore_bn(m)
        assert _same_bits(_stats(m), old)
    assert bool(torch.isfinite(res['eager']).all()) and not torch.equal(res['eager'], old)
    assert _same_bits(res['eager'], res['graph']) and _same_bits(res['eager'], res['auto'])
    recalibrate_bn(m, use_graph=False, step=4, **kw)                            # another step: other draws, other statistics
    assert not torch.equal(_stats(m), res['eager'])
    restore_bn(m)


@pytest.mark.parametrize('training', [True, False])
def test_restore_puts_everything_back(cifar, training):
    from lvae_amd.recalibrate import recalibrate_bn, recalibrated, restore_bn
    m = cifar
    m.train(training)
    with torch.no_grad():
        m.sample_prior(2)                                                       # the model's own stream stands somewhere
    bns = m.bn_modules()
    for i, bn in enumerate(bns):
        bn._pending = i % 3
    bns[0].momentum = 0.25
    before = dict(stats=_stats(m), pending=[bn._pending for bn in bns], momentum=[bn.momentum for bn in bns], noise=m.noise,
                  step=int(m.noise.step.item()), nbt=[int(bn.num_batches_tracked) for bn in bns])

    def unchanged(with_stats):
        assert [bn._pending for bn in bns] == before['pending'] and [bn.momentum for bn in bns] == before['momentum']
        assert [int(bn.num_batches_tracked) for bn in bns] == before['nbt']
        assert m.training == training and all(mod.training == training for mod in m.modules())
        assert m.noise is before['noise'] and int(m.noise.step.item()) == before['step']
        assert _same_bits(_stats(m), before['stats']) == with_stats

    recalibrate_bn(m, [_images(4, 300 + k) for k in range(3)])
    unchanged(False)
    restore_bn(m)
    unchanged(True)
    with recalibrated(m, n_prior=2, prior_batch=3) as info:
        assert info['source'] == 'prior'
        unchanged(False)
    unchanged(True)
    # a non-finite statistic: RuntimeError, and the old statistics are back without a restore
    bad = _images(4, 310)
    bad[1, 2, 5, 5] = float('nan')
    with pytest.raises(RuntimeError, match='non-finite'):
        recalibrate_bn(m, [_images(4, 311), bad])
    unchanged(True)
    with pytest.raises(ValueError):
        recalibrate_bn(m)                                                       # no source
    with pytest.raises(ValueError):
        recalibrate_bn(m, [_images(4, 1)], n_prior=2, prior_batch=2)            # two sources
    with pytest.raises(ValueError):
        recalibrate_bn(m, n_prior=2, prior_batch=2, temperature=-1.0)
    unchanged(True)
    bns[0].momentum = 0.1
    for bn in bns:
        bn._pending = 0
    m.train()


def _fresh_table():
    from lvae_amd import kernels as K
    K.prepared.entries.clear()
    K.prepared.table = None


def _train_state(m, opt):
    sd = m.state_dict()   # (flushes the host-counted num_batches_tracked)
    bufs = {k: v.detach().clone() for k, v in sd.items() if not k.endswith(('weight', 'bias', 'top_prior_params'))}
    return {'params': m.arena.params.detach().clone(), 'exp_avg': opt.exp_avg.clone(), 'exp_inf': opt.exp_inf.clone(),
            'adamax_step': opt.step_count.clone(), 'ema': opt.ema.clone(), 'noise_step': m.noise.step.clone(), **bufs}


@pytest.mark.parametrize('use_graph', [True, False], ids=['captured', 'eager'])
def test_recalibrated_test_pass_between_steps(use_graph, tmp_path):
    """Four training steps with a recalibrated test pass (and a checkpoint) between steps 2 and 3 leave the parameters, the optimizer
    state, the average, the running statistics and every step's outputs bit for bit those of four steps without. The pass itself equals
    the pass of a second model that was loaded with the 'ema' weights and recalibrated on the same batches by hand, its ELBO differs from
    the unrecalibrated pass, and the checkpoint's 'ema' buffers are that second model's."""
    from lvae_amd.checkpoint import ema_state_dict_reference_layout, save_checkpoint, state_dict_reference_layout
    from lvae_amd.engine import TrainStep
    from lvae_amd.evaluate import test_pass
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax
    from lvae_amd.recalibrate import recalibrate_bn
    g = load_golden('tiny_cifar')
    xs = [_images(4, 10 + k) for k in range(4)]
    xt = [_images(5, 30).cuda(), _images(3, 31).cuda()]
    recal = [_images(4, 400 + k) for k in range(3)]
    S, path = 2, str(tmp_path / 'model_2.pt')
    res, seen = {}, {}
    for with_pass in (False, True):
        _fresh_table()
        m = _model(g.cfg, g.state_dict(), PhiloxNoise(seed=3))
        m.ema_bn_batches = 3
        opt = Adamax(m, lr=1e-3, ema_decay=0.9)
        st = TrainStep(m, opt, use_graph=use_graph)
        outs = []
        for i, x in enumerate(xs):
            outs.append({k: v.detach().clone() for k, v in st(x.cuda()).items()})
            if with_pass and i == 1:
                seen['avg_sd'], seen['raw_sd'] = ema_state_dict_reference_layout(m, opt), state_dict_reference_layout(m)
                seen['plain'] = test_pass(m, xt, S, noise=PhiloxNoise(seed=21), optimizer=opt, use_graph=use_graph)
                seen['recal'] = test_pass(m, xt, S, noise=PhiloxNoise(seed=21), optimizer=opt, use_graph=use_graph, bn_recal=lambda: recal)
                save_checkpoint(path, m, opt, bn_recal=lambda: recal)
                assert m.training and m.global_step == 2
        torch.cuda.synchronize()
        assert (st.graph_a is not None) == use_graph
        res[with_pass] = (outs, _train_state(m, opt))
    for a, b in zip(res[False][0], res[True][0]):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    assert res[False][1].keys() == res[True][1].keys()
    for k in res[False][1]:
        assert torch.equal(res[False][1][k], res[True][1][k]), k

    plain, got = seen['plain'], seen['recal']
    assert plain.pop('weights') == got.pop('weights') == 'ema' and 'bn_recal/rounds' not in plain and got.pop('bn_recal/rounds') == 3
    m2 = _model(g.cfg, seen['avg_sd'], PhiloxNoise(seed=3))        # the seed and the step place the recalibration's own noise stream
    assert recalibrate_bn(m2, recal, step=2)['rounds'] == 3
    want = test_pass(m2, xt, S, noise=PhiloxNoise(seed=21), use_graph=use_graph)
    assert got == want, (got, want)                                 # bitwise: every total is the same double
    assert got['elbo/elbo'] != plain['elbo/elbo'] and got['elbo/recons'] != plain['elbo/recons']
    print('test ELBO on the averaged weights: %.6f with the live statistics, %.6f recalibrated' % (plain['elbo/elbo'], got['elbo/elbo']))

    ck = torch.load(path)
    assert ck['ema_bn_batches'] == 3 and list(ck['ema']) == list(ck['model'])
    sd2 = state_dict_reference_layout(m2)
    differ = 0
    for k, v in ck['model'].items():
        assert torch.equal(v, seen['raw_sd'][k]), k                 # 'model' is untouched
        if k.endswith(STAT):
            assert torch.equal(ck['ema'][k], sd2[k]), k             # the recalibrated statistics of the averaged weights
            differ += int(not torch.equal(ck['ema'][k], v))
        else:
            assert torch.equal(ck['ema'][k], seen['avg_sd'][k]), k
    assert differ == len(_stat_keys(ck['model']))
    path0 = str(tmp_path / 'plain.pt')
    save_checkpoint(path0, m2)                                      # without the source: no note
    assert 'ema_bn_batches' not in torch.load(path0)


_TINY_ARGV = ['-d', 'cifar10', '--zdims', '8', '8', '--downsample', '1', '1', '--nfilters', '16', '--skip', '--gated', '--freebits', '1.0',
              '--batch-size', '8', '--synthetic', '--seed', '3']


def test_evaluate_recalibrates_on_the_prior_end_to_end(tmp_path, monkeypatch, capsys):
    from lvae_amd import evaluate
    from lvae_amd.checkpoint import save_checkpoint
    from lvae_amd.experiment.experiment_manager import LVAEExperiment
    monkeypatch.chdir(tmp_path)
    exp = LVAEExperiment(args=evaluate.parse_eval_args(_TINY_ARGV))
    path = str(tmp_path / 'tiny.pt')
    save_checkpoint(path, exp.model)
    del exp
    evaluate.main(_TINY_ARGV + ['--checkpoint', path, '--ps'])
    assert 'recalibrated' not in capsys.readouterr().out
    plain = np.load('prior_samples.npy')
    evaluate.main(_TINY_ARGV + ['--checkpoint', path, '--ps', '--recalibrate-bn', 'prior', '--recalibrate-batches', '3', '--temperature', '0.7'])
    out = capsys.readouterr().out
    assert 'BatchNorm recalibrated for the weights on the prior: 3 top-down passes of 8 rows at temperature 0.7' in out, out
    cold = np.load('prior_samples.npy')
    assert cold.shape == plain.shape == (64, 3, 32, 32) and np.isfinite(cold).all() and cold.min() >= 0.0 and cold.max() <= 1.0
    assert not np.array_equal(cold, plain)


def test_first_batches_reads_the_device_table():
    from lvae_amd.data import DeviceDataset, first_batches
    u8 = _images(11, 500)                                            # every value k / 255: kept as uint8 in device memory
    f32 = torch.rand(11, 3, 32, 32, generator=torch.Generator().manual_seed(501))
    for imgs, kind in ((u8, 'uint8'), (f32, 'float32')):
        ds = DeviceDataset(imgs, 4, seed=1, device=torch.device('cuda', 0))
        assert ds.kind == kind
        got = first_batches(ds, 5, 4)                                # 20 > 11: the two whole batches
        want = first_batches(imgs, 5, 4)
        assert len(got) == len(want) == 2 and all(g.is_cuda and torch.equal(g.cpu(), w) for g, w in zip(got, want))
        assert ds.cursor is None                                     # the feed's cursor is not even created
    with pytest.raises(ValueError, match='do not fill one batch'):
        first_batches(DeviceDataset(u8, None, seed=1, device=torch.device('cuda', 0)), 1, 12)


def test_trainer_recalibrates_before_its_test_passes(tmp_path):
    import json
    import re
    import subprocess
    import sys
    from conftest import ROOT
    hist, ck = tmp_path / 'history.jsonl', tmp_path / 'last.pt'
    argv = _TINY_ARGV + ['--synthetic-test', '24', '--test-batch-size', '24', '--ts-log-every', '3', '--steps', '6', '--log-every', '3',
                         '--ema-decay', '0.9', '--ema-bn-batches', '2', '--history', str(hist), '--save-checkpoint', str(ck)]
    p = subprocess.run([sys.executable, '-m', 'lvae_amd.main'] + argv, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    tests = [ln for ln in p.stdout.splitlines() if 'epoch' in ln]
    assert len(tests) == 2 and all('[averaged weights]   [BatchNorm recalibrated on 2 batches]   ELBO' in ln for ln in tests), p.stdout
    assert all(np.isfinite(float(re.search(r'ELBO (\S+)', ln).group(1))) for ln in tests)
    recs = [json.loads(ln) for ln in open(hist)]
    assert [r['metrics'].get('bn_recal/rounds') for r in recs if r['split'] == 'test'] == [2, 2]
    assert all('bn_recal/rounds' not in r['metrics'] for r in recs if r['split'] == 'train')
    saved = torch.load(str(ck))
    assert saved['ema_bn_batches'] == 2
    assert any(not torch.equal(saved['ema'][k], saved['model'][k]) for k in saved['model'] if k.endswith(STAT))
    q = subprocess.run([sys.executable, '-m', 'lvae_amd.main'] + _TINY_ARGV + ['--steps', '1', '--ema-bn-batches', '2'], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert q.returncode != 0 and '--ema-decay' in q.stderr                  # refused before anything runs
