"""Device-resident training data on the GPU: the gather kernel bit for bit, the cursor across epochs (eager and captured), fed training
equal to hand-fed training, two ranks, the device-resident test split, and the trainer with --device-data including exact resume."""
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bytes(n, shape, seed):
    return torch.randint(0, 256, (n,) + shape, dtype=torch.uint8, generator=_gen(seed))


def _unit(u8_nchw):
    return u8_nchw.float().div_(255)


def _images(n, seed):
    return torch.floor(256 * torch.rand(n, 3, 32, 32, generator=_gen(seed))) / 255


def _all_bytes_first(n):
    t = _bytes(n, (1, 16, 16), 9)
    t[0] = torch.arange(256, dtype=torch.uint8).view(1, 16, 16)
    return t


# name: (host images, channels_last, global batch, the float NCHW images the gather must reproduce)
def _gather_cases():
    c = {}
    t = _bytes(40, (3, 32, 32), 1)
    c['u8_chw_3x32x32'] = (t, False, 8, _unit(t))
    t = _bytes(33, (1, 28, 28), 2)
    c['u8_chw_1x28x28'] = (t, False, 8, _unit(t))
    t = _bytes(12, (64, 64, 3), 3)
    c['u8_hwc_64x64x3'] = (t, True, 4, _unit(t.permute(0, 3, 1, 2).contiguous()))
    t = torch.rand(20, 3, 32, 32, generator=_gen(4)) * 3 - 1
    c['f32_chw'] = (t, False, 8, t)
    t = _bytes(9, (1, 5, 7), 5)
    c['u8_tail_1x5x7'] = (t, False, 4, _unit(t))
    t = torch.randn(9, 1, 5, 7, generator=_gen(6))
    c['f32_tail_1x5x7'] = (t, False, 4, t)
    t = _bytes(9, (5, 7, 3), 7)
    c['u8_hwc_tail_5x7x3'] = (t, True, 4, _unit(t.permute(0, 3, 1, 2).contiguous()))
    t = _bytes(23, (3, 32, 32), 8)
    c['five_rows'] = (t, False, 5, _unit(t))
    t = _all_bytes_first(4)
    c['every_byte_value'] = (t, False, 4, _unit(t))          # N = B: every batch holds image 0 = arange(256)
    t = _images(16, 10)
    c['f32_stored_as_bytes'] = (t, False, 4, t)              # ToTensor-law floats go to HBM as uint8 and come back as the same floats
    return c


CASES = _gather_cases()


@pytest.mark.parametrize('name', sorted(CASES))
def test_gather_is_bit_equal(name):
    from lvae_amd.data import DeviceDataset
    images, channels_last, B, want_all = CASES[name]
    ds = DeviceDataset(images, B, seed=11, channels_last=channels_last)
    if name == 'f32_stored_as_bytes':
        assert ds.kind == 'uint8'
    if name == 'f32_chw':
        assert ds.kind == 'float32'
    spe = ds.steps_per_epoch
    for s in (1, 2, spe, spe + 1, 3 * spe + 2, 1):
        got = ds.batch(s)
        want = want_all[ds.indices(s)]
        assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == tuple(want.shape)
        assert torch.equal(got.cpu(), want), (name, s)
    if name == 'every_byte_value':
        row = ds.indices(1).tolist().index(0)
        assert torch.equal(ds.batch(1)[row].cpu().view(-1), torch.arange(256, dtype=torch.uint8).float().div_(255.0))


@pytest.mark.parametrize('name', ['u8_chw_3x32x32', 'u8_hwc_64x64x3', 'f32_chw', 'u8_tail_1x5x7'])
def test_storage_order_batches(name):
    from lvae_amd.data import DeviceDataset
    images, channels_last, _, want_all = CASES[name]
    ds = DeviceDataset(images, None, seed=0, channels_last=channels_last)
    n = 7
    got = list(ds.batches(n))
    sizes = [b.shape[0] for b in got]
    assert sizes == [n] * (ds.N // n) + ([ds.N % n] if ds.N % n else []) and sizes[-1] < n      # the last one is short
    assert torch.equal(torch.cat(got).cpu(), want_all)
    assert [b.shape[0] for b in ds.batches(ds.N)] == [ds.N]


def test_entry_point_refuses_bad_arguments():
    from lvae_amd import _C
    from lvae_amd import kernels as K
    table = _bytes(6, (1, 4, 4), 0).cuda()
    out = torch.empty(4, 1, 4, 4, device='cuda')
    idx = torch.zeros(8, dtype=torch.int32, device='cuda')
    with pytest.raises(_C.LvaeHipError):
        K.batch_gather(table, False, out, base=3)                                            # images 3..6 of 6
    with pytest.raises(_C.LvaeHipError):
        K.batch_gather(table, False, out, index=idx, steps_per_epoch=2, global_batch=4, lo=1)  # rows 1..4 of a batch of 4
    with pytest.raises(_C.LvaeHipError):
        K.batch_gather(table, False, out, index=idx, steps_per_epoch=3, global_batch=4)      # table length != epoch
    with pytest.raises(_C.LvaeHipError):
        K.batch_gather(table, False, out.double())
    with pytest.raises(_C.LvaeHipError):
        K.batch_gather(table.cpu(), False, out)
    # an index outside the table is never dereferenced: the row is NaN
    bad = torch.tensor([0, 6, -1, 5], dtype=torch.int32, device='cuda')
    got = K.batch_gather(table, False, out, index=bad, steps_per_epoch=1, global_batch=4).cpu()
    assert torch.equal(got[0], _unit(table.cpu()[0])) and torch.equal(got[3], _unit(table.cpu()[5]))
    assert bool(got[1].isnan().all()) and bool(got[2].isnan().all())


class _Counted:
    """What attach() needs of a model."""

    def __init__(self, step):
        self.global_step = step


@pytest.mark.parametrize('use_graph', [False, True])
def test_cursor_walks_through_epochs(use_graph):
    """N = 10, B = 4: two steps per epoch, so seven steps cross three index-table replacements."""
    from lvae_amd.data import DeviceDataset
    images = _bytes(10, (3, 8, 8), 21)
    ds = DeviceDataset(images, 4, seed=3).attach(_Counted(0))
    assert ds.steps_per_epoch == 2
    out = ds.new_batch()
    graph = None
    if use_graph:
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ds.gather(out)
            ds.advance()
    assert int(ds.cursor.item()) == 0                      # capturing ran nothing
    seen = []
    for s in range(1, 8):
        ds.before_step(s - 1)
        if graph is not None:
            graph.replay()
        else:
            ds.gather(out)
            ds.advance()
        seen.append(out.clone())                           # (stream-ordered: reads this step's batch)
    assert int(ds.cursor.item()) == 7
    for s, got in zip(range(1, 8), seen):
        assert torch.equal(got.cpu(), _unit(images)[ds.indices(s)]), s
    assert len({tuple(ds.indices(s).tolist()) for s in (1, 3, 5, 7)}) > 1
    # a resumed run: attached at 5 completed steps, the next batch is step 6's, in the middle of epoch 2
    ds2 = DeviceDataset(images, 4, seed=3).attach(_Counted(5))
    got = ds2.gather(ds2.new_batch())
    assert torch.equal(got.cpu(), _unit(images)[ds.indices(6)])
    # a gather that is not followed by its advance (an abandoned step) leaves the position alone
    assert int(ds2.cursor.item()) == 5


def test_two_ranks_on_one_device():
    from lvae_amd.data import DeviceDataset
    images = _bytes(26, (3, 32, 32), 31)
    whole = DeviceDataset(images, 8, seed=4)
    parts = [DeviceDataset(images, 8, seed=4, rank=r, world=2) for r in (0, 1)]
    for s in (1, 2, 3, 4, 7):
        got = torch.cat([p.batch(s) for p in parts])
        assert got.shape[0] == 8
        assert torch.equal(got, whole.batch(s)), s
        assert torch.equal(got.cpu(), _unit(images)[whole.indices(s)]), s
    for p in parts:
        p.attach(_Counted(3))
    got = torch.cat([p.gather(p.new_batch()) for p in parts])
    assert torch.equal(got.cpu(), _unit(images)[whole.indices(4)])


# ---- training ---------------------------------------------------------------------------------------------------------
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


def _train_state(m, opt):
    sd = m.state_dict()   # (flushes the host-counted num_batches_tracked)
    bufs = {k: v.detach().clone() for k, v in sd.items() if not k.endswith(('weight', 'bias', 'top_prior_params'))}
    return {'params': m.arena.params.detach().clone(), 'exp_avg': opt.exp_avg.clone(), 'exp_inf': opt.exp_inf.clone(),
            'adamax_step': opt.step_count.clone(), **bufs}


def _assert_same_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _train(images, n_steps, how):
    """how: 'fed-graph' | 'fed-eager' | 'hand-graph' (the existing step, given images[indices(s)] by hand)."""
    from lvae_amd.data import DeviceDataset
    from lvae_amd.engine import TrainStep
    from lvae_amd.noise import FrozenNoise
    from lvae_amd.optim import Adamax
    g = load_golden('tiny_cifar')
    _fresh_table()
    m = _model(g.cfg, g.state_dict(), FrozenNoise(seed=11))
    opt = Adamax(m, lr=1e-3)
    ds = DeviceDataset(images, 4, seed=17)
    fed = how.startswith('fed')
    st = TrainStep(m, opt, use_graph=how.endswith('graph'), feed=ds if fed else None)
    outs, xs = [], []
    for s in range(1, n_steps + 1):
        out = st() if fed else st(images[ds.indices(s)].cuda())
        outs.append({k: v.detach().clone() for k, v in out.items()})
        if fed:
            xs.append(st.static_x.clone())
    torch.cuda.synchronize()
    assert (st.graph_a is not None) == how.endswith('graph')
    if fed:
        assert int(ds.cursor.item()) == m.global_step == n_steps
        for s, x in zip(range(1, n_steps + 1), xs):
            assert torch.equal(x.cpu(), images[ds.indices(s)]), s
    return outs, _train_state(m, opt)


def test_fed_training_equals_hand_fed_training():
    images = _images(24, 5)                                # B = 4: six steps per epoch, eight steps reach epoch 1
    runs = {how: _train(images, 8, how) for how in ('hand-graph', 'fed-graph', 'fed-eager')}
    ref_outs, ref_state = runs['hand-graph']
    assert len({float(o['loss']) for o in ref_outs}) == 8
    for how in ('fed-graph', 'fed-eager'):
        outs, state = runs[how]
        for s, (a, b) in enumerate(zip(outs, ref_outs), 1):
            for key in ('loss', 'elbo', 'recons', 'kl'):
                assert torch.equal(a[key], b[key]), (how, s, key, float(a[key]), float(b[key]))
        _assert_same_state(state, ref_state)


def test_step_takes_a_batch_or_a_feed_not_both():
    from lvae_amd.data import DeviceDataset
    from lvae_amd.engine import TrainStep
    from lvae_amd.noise import FrozenNoise
    from lvae_amd.optim import Adamax
    g = load_golden('tiny_cifar')
    _fresh_table()
    m = _model(g.cfg, g.state_dict(), FrozenNoise(seed=11))
    opt = Adamax(m, lr=1e-3)
    images = _images(8, 6)
    fed = TrainStep(m, opt, feed=DeviceDataset(images, 4, seed=1))
    with pytest.raises(ValueError):
        fed(images[:4].cuda())
    plain = TrainStep(m, opt)
    with pytest.raises(ValueError):
        plain()
    assert m.global_step == 0


def test_device_resident_test_split():
    from lvae_amd.data import DeviceDataset
    from lvae_amd.evaluate import test_pass
    from lvae_amd.noise import PhiloxNoise
    g = load_golden('tiny_cifar')
    images = _images(13, 8)
    bs = 5                                                 # batches of 5, 5 and 3
    res = {}
    for on_device in (False, True):
        _fresh_table()
        m = _model(g.cfg, g.state_dict(), PhiloxNoise(1))
        if on_device:
            batches = DeviceDataset(images, None, seed=0).batches(bs)
        else:
            batches = (images[i:i + bs] for i in range(0, 13, bs))
        res[on_device] = test_pass(m, batches, 4, noise=PhiloxNoise(seed=21))
    assert res[True]['n_images'] == 13
    assert res[True] == res[False], (res[True], res[False])


# ---- the trainer ------------------------------------------------------------------------------------------------------
ARGV = ['-d', 'cifar10', '--zdims', '8', '8', '--downsample', '1', '1', '--nfilters', '16', '--skip', '--gated', '--freebits', '1.0',
        '--batch-size', '8', '--seed', '3', '--test-batch-size', '8', '--ts-log-every', '2', '--ll-every', '4', '--ll-samples', '4',
        '--log-every', '1', '--device-data']


def _npz(tmp_path):
    path = str(tmp_path / 'data.npz')
    np.savez(path, data=_images(43, 40).numpy(), test=_images(20, 41).numpy())   # 5 steps per epoch, 3 images never fill a batch
    return path


def _main(argv):
    p = subprocess.run([sys.executable, '-m', 'lvae_amd.main'] + argv, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = [re.sub(r'\s*\[\d+ img/s\]', '', line) for line in p.stdout.splitlines() if re.search(r'\[step \d+', line)]
    train = {int(re.search(r'\[step (\d+)\]', line).group(1)): line for line in lines if re.search(r'\[step \d+\]', line)}
    test = {int(re.search(r'\[step (\d+), epoch', line).group(1)): line for line in lines if 'epoch' in line}
    return train, test, p.stdout


def _ckpt_tensors(path):
    ck = torch.load(path)
    flat = {'model.' + k: v for k, v in ck['model'].items()}
    for name, st in ck['optimizer']['state'].items():
        flat['avg.' + name], flat['inf.' + name] = st['exp_avg'], st['exp_inf']
    meta = (ck['global_step'], ck['optimizer']['step'], ck['noise'], ck.get('test_noise'))
    return flat, meta


def test_trainer_repeats_and_resumes_exactly(tmp_path):
    npz = _npz(tmp_path)
    base = ARGV + ['--data-npz', npz]
    full, half, rest = (str(tmp_path / n) for n in ('full.pt', 'half.pt', 'rest.pt'))
    tr_a, te_a, out_a = _main(base + ['--steps', '8', '--save-checkpoint', full])
    assert sorted(tr_a) == list(range(1, 9)) and sorted(te_a) == [2, 4, 6, 8], out_a
    assert 'device data: 43 images' in out_a and 'as uint8' in out_a and '5 steps per epoch' in out_a
    assert [int(re.search(r'epoch (\d+)', te_a[s]).group(1)) for s in (2, 4, 6, 8)] == [0, 0, 1, 1]   # (step - 1) // 5
    assert len(set(tr_a.values())) == 8
    # the same flags again: the same lines
    tr_b, te_b, _ = _main(base + ['--steps', '8'])
    assert tr_b == tr_a and te_b == te_a
    # four steps, a checkpoint in the middle of epoch 0, four more from it: the same lines and the same final state
    tr_1, te_1, _ = _main(base + ['--steps', '4', '--save-checkpoint', half])
    tr_2, te_2, _ = _main(base + ['--steps', '8', '--resume', half, '--save-checkpoint', rest])
    assert sorted(tr_2) == [5, 6, 7, 8]
    assert {**tr_1, **tr_2} == tr_a and {**te_1, **te_2} == te_a
    (fa, ma), (fb, mb) = _ckpt_tensors(full), _ckpt_tensors(rest)
    assert ma == mb and ma[0] == 8
    assert fa.keys() == fb.keys()
    for k in fa:
        assert torch.equal(fa[k], fb[k]), k


def test_trainer_honours_max_epochs(tmp_path):
    npz = _npz(tmp_path)
    tr, te, out = _main(ARGV + ['--data-npz', npz, '--steps', '50', '--max-epochs', '1', '--no-graph'])
    assert sorted(tr) == [1, 2, 3, 4, 5], out              # one epoch of five steps, eager launches
