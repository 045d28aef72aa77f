"""The augmenting gather on the GPU: the kernel bit for bit against the numpy restatement of its noise rule (tests/feed_aug_ref.py) at every
shape where the thread map changes; the plain entry point unchanged; the cursor, two ranks and a captured graph; fed training equal to
hand-fed training; the fixed binarization; and the trainer with --binarize --hflip including exact resume."""
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

import feed_aug_ref as R

pytestmark = pytest.mark.gpu


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bytes(n, shape, seed):
    return torch.randint(0, 256, (n,) + shape, dtype=torch.uint8, generator=_gen(seed))


def _unit_floats(n, shape, seed):
    t = torch.rand((n,) + shape, generator=_gen(seed))
    t.view(-1)[::7] = 0.0
    t.view(-1)[3::11] = 1.0
    return t


def _chw(table, channels_last):
    return table.permute(0, 3, 1, 2).contiguous() if channels_last else table


def _same_bits(got, want):
    got = got.detach().cpu().numpy()
    return got.dtype == want.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))


def _mixed_seed(P, gs):
    """An augmentation seed, found on the CPU, under which some of the rows gs flip at cursor P and some do not."""
    for k in range(1000):
        s = R.aug_seed(k)
        flips = [R.row_flips(s, P, g) for g in gs]
        if any(flips) and not all(flips):
            return s
    raise AssertionError('no seed with mixed flips')


# name: (host table, channels_last, why)
SHAPES = {
    'u8_chw_1x5x7': (_bytes(11, (1, 5, 7), 1), False),        # row tail, element path
    'u8_chw_2x4x6': (_bytes(11, (2, 4, 6), 2), False),        # chw % 4 == 0 but W % 4 != 0: a flip must leave the vector path
    'u8_chw_1x28x28': (_bytes(11, (1, 28, 28), 3), False),    # MNIST
    'u8_chw_3x32x32': (_bytes(11, (3, 32, 32), 4), False),    # CIFAR, more than one block
    'u8_hwc_8x8x3': (_bytes(11, (8, 8, 3), 5), True),         # channels-last, vector path
    'u8_hwc_5x7x3': (_bytes(11, (5, 7, 3), 6), True),         # channels-last, tail
    'f32_chw_3x8x8': (_unit_floats(11, (3, 8, 8), 7), False),
}
B, SPE = 6, 3


def _index(N, seed, n=SPE * B):
    return torch.randint(0, N, (n,), dtype=torch.int32, generator=_gen(seed))


def _gather(table, channels_last, aug, index, P, lo=0, n=B, cursor=True, global_batch=B):
    from lvae_amd import kernels as K
    chw = _chw(table, channels_last).shape[1:]
    out = torch.full((n,) + tuple(chw), -7.0, device='cuda')
    cur = torch.tensor([P], dtype=torch.int64, device='cuda') if cursor else None
    return K.batch_gather_aug(table.cuda(), channels_last, out, aug, index=index.cuda(), cursor=cur, steps_per_epoch=index.numel() // global_batch,
                              global_batch=global_batch, lo=lo, position=0 if cursor else P)


@pytest.mark.parametrize('hflip', [False, True], ids=['noflip', 'flip'])
@pytest.mark.parametrize('mode', [None, 'binarize', 'dequantize'], ids=['none', 'binarize', 'dequantize'])
@pytest.mark.parametrize('name', sorted(SHAPES))
def test_kernel_equals_restatement(name, mode, hflip):
    from lvae_amd import _C
    from lvae_amd import kernels as K
    table, channels_last = SHAPES[name]
    P = 4
    seed = _mixed_seed(P, range(B))
    index = _index(table.shape[0], 20)
    aug = K.feed_aug(seed, mode, hflip=hflip)
    if mode == 'dequantize' and table.dtype == torch.float32:
        with pytest.raises(_C.LvaeHipError):
            _gather(table, channels_last, aug, index, P)
        return
    got = _gather(table, channels_last, aug, index, P)
    rows = _chw(table, channels_last)[index[(P % SPE) * B:(P % SPE + 1) * B].long()].numpy()
    want, flipped = R.augment(rows, seed, P, list(range(B)), mode, hflip)
    assert (0 < len(flipped) < B) if hflip else flipped == []
    assert _same_bits(got, want), (name, mode, hflip)
    if mode == 'binarize':
        assert set(np.unique(want)) <= {0.0, 1.0} and 0.2 < want.mean() < 0.8
    if mode == 'dequantize':
        assert float(want.max()) < 1.0 and not np.array_equal(want, R.plain(rows))


@pytest.mark.parametrize('mode', ['binarize', 'dequantize'])
def test_every_byte_value(mode):
    from lvae_amd import kernels as K
    table = _bytes(4, (1, 16, 16), 9)
    table[0] = torch.arange(256, dtype=torch.uint8).view(1, 16, 16)
    index = torch.tensor([0, 2, 0, 1, 0, 3], dtype=torch.int32)
    P = 0
    seed = _mixed_seed(P, [0, 2, 4])
    got = _gather(table, False, K.feed_aug(seed, mode, hflip=True), index, P)
    want, flipped = R.augment(table[index.long()].numpy(), seed, P, list(range(6)), mode, True)
    assert {0, 2, 4} & set(flipped) and {0, 2, 4} - set(flipped)      # image 0 is seen flipped and unflipped
    assert _same_bits(got, want)
    flat = want[0 if 0 not in flipped else (2 if 2 not in flipped else 4)].reshape(-1)   # an unflipped arange(256)
    if mode == 'binarize':
        assert flat[0] == 0.0 and flat[255] == 1.0
    else:   # every byte's value stays in its bin (the sum b + u may round up to the bin's end)
        b = np.arange(256, dtype=np.float64)
        assert (flat >= b / 256).all() and (flat <= np.minimum((b + 1) / 256, 1 - 2.0 ** -24)).all() and (np.diff(flat) > 0).all()


def test_rows_of_a_rank_a_high_position_and_bad_indices():
    from lvae_amd import kernels as K
    table, channels_last = SHAPES['u8_chw_1x28x28']
    chw = _chw(table, channels_last)
    index = _index(table.shape[0], 21)
    # lo > 0: rows 2 .. 5 of the global batch draw the noise of their place in it
    P = 7
    seed = _mixed_seed(P, range(2, 6))
    aug = K.feed_aug(seed, 'binarize', hflip=True)
    got = _gather(table, channels_last, aug, index, P, lo=2, n=4)
    start = (P % SPE) * B + 2
    want, flipped = R.augment(chw[index[start:start + 4].long()].numpy(), seed, P, [2, 3, 4, 5], 'binarize', True)
    assert 0 < len(flipped) < 4 and _same_bits(got, want)
    whole = _gather(table, channels_last, aug, index, P)
    assert torch.equal(whole[2:6], got)
    # a position past 2^32, given explicitly: the high half reaches the key
    P = 2 ** 32 + 5
    seed = _mixed_seed(P, range(B))
    aug = K.feed_aug(seed, 'dequantize', hflip=True)
    got = _gather(table, channels_last, aug, index, P, cursor=False)
    rows = chw[index[(P % SPE) * B:(P % SPE + 1) * B].long()].numpy()
    want, flipped = R.augment(rows, seed, P, list(range(B)), 'dequantize', True)
    assert 0 < len(flipped) < B and _same_bits(got, want)
    assert torch.equal(got, _gather(table, channels_last, aug, index, P, cursor=True))         # the cursor and the position are one rule
    one = index[:B]                                                                            # one step per epoch: the same images at every P
    aug = K.feed_aug(seed, 'dequantize')
    hi, lo5 = (_gather(table, channels_last, aug, one, p, cursor=False) for p in (P, 5))
    assert _same_bits(hi, R.augment(chw[one.long()].numpy(), seed, P, list(range(B)), 'dequantize')[0])
    assert not torch.equal(hi, lo5) and float((hi - lo5).abs().max()) <= 1.0 / 256                 # other noise in the same bins
    # an index outside the table is never an address: the row is NaN, whatever the augmentation
    bad = torch.tensor([0, table.shape[0], -1, 5, 2 ** 31 - 1, 1], dtype=torch.int32)
    got = _gather(table, channels_last, K.feed_aug(seed, 'binarize', hflip=True), bad, 0).cpu()
    want, _ = R.augment(chw[torch.tensor([0, 0, 0, 5, 0, 1])].numpy(), seed, 0, list(range(B)), 'binarize', True)
    for r in range(B):
        if r in (1, 2, 4):
            assert bool(got[r].isnan().all()), r
        else:
            assert _same_bits(got[r], want[r]), r


def test_argument_checks():
    from lvae_amd import _C
    from lvae_amd import kernels as K
    table = _bytes(6, (1, 4, 4), 0).cuda()
    out = torch.empty(4, 1, 4, 4, device='cuda')
    idx = torch.zeros(8, dtype=torch.int32, device='cuda')
    aug = K.feed_aug(1, 'binarize')
    with pytest.raises(ValueError):
        K.feed_aug(1, 'posterize')
    with pytest.raises(_C.LvaeHipError):
        K.batch_gather_aug(table, False, out, aug, base=3)                                            # images 3..6 of 6
    with pytest.raises(_C.LvaeHipError):
        K.batch_gather_aug(table, False, out, aug, index=idx, steps_per_epoch=2, global_batch=4, lo=1)  # rows 1..4 of a batch of 4
    with pytest.raises(_C.LvaeHipError):
        K.batch_gather_aug(table, False, out, aug, index=idx, steps_per_epoch=3, global_batch=4)      # table length != epoch
    with pytest.raises(_C.LvaeHipError):
        K.batch_gather_aug(table, False, out.double(), aug)
    with pytest.raises(_C.LvaeHipError):
        K.batch_gather_aug(table.cpu(), False, out, aug)
    with pytest.raises(_C.LvaeHipError):
        K.batch_gather_aug(table, False, out, aug, index=idx, steps_per_epoch=2, global_batch=4, position=-1)
    with pytest.raises(_C.LvaeHipError):
        K.batch_gather_aug(table, False, out, _C.FeedAug(1, 0, 7, 0, 0))                             # no such mode
    with pytest.raises(_C.LvaeHipError):
        K.batch_gather_aug(table.float(), False, out, K.feed_aug(1, 'dequantize'))                   # float32 tables have no bytes


@pytest.mark.parametrize('name', sorted(SHAPES))
def test_plain_entry_point_is_unchanged(name):
    """lvae_batch_gather_f32 against the augmenting entry point with nothing on, and against the values themselves."""
    from lvae_amd import kernels as K
    table, channels_last = SHAPES[name]
    index = _index(table.shape[0], 22)
    chw = _chw(table, channels_last)
    for P in (0, 4):
        cur = torch.tensor([P], dtype=torch.int64, device='cuda')
        plain = K.batch_gather(table.cuda(), channels_last, torch.empty((B,) + tuple(chw.shape[1:]), device='cuda'), index=index.cuda(), cursor=cur,
                               steps_per_epoch=SPE, global_batch=B)
        none = _gather(table, channels_last, K.feed_aug(5), index, P)
        rows = chw[index[(P % SPE) * B:(P % SPE + 1) * B].long()]
        assert torch.equal(plain, none)
        assert _same_bits(plain, R.plain(rows.numpy()))
    plain = K.batch_gather(table.cuda(), channels_last, torch.empty((3,) + tuple(chw.shape[1:]), device='cuda'), base=2)
    assert torch.equal(plain, K.batch_gather_aug(table.cuda(), channels_last, torch.empty_like(plain), K.feed_aug(5), base=2))
    assert _same_bits(plain, R.plain(chw[2:5].numpy()))


# ---- the data set ------------------------------------------------------------------------------------------------------
class _Counted:
    def __init__(self, step):
        self.global_step = step


def _want_batch(ds, images, step):
    """What the restatement says the GLOBAL batch of micro-batch `step` is."""
    rows = images[ds.indices(step)].numpy()
    want, _ = R.augment(rows, R.aug_seed(ds.seed), step - 1, list(range(ds.batch_size)), ds.augment.mode, ds.augment.hflip)
    return want


def _record_calls(monkeypatch):
    from lvae_amd import kernels as K
    names, real = [], K.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(K, 'call', call)
    return names


def test_unaugmented_feed_issues_the_launches_it_issued(monkeypatch):
    from lvae_amd.data import DeviceDataset, FeedAugment, first_batches
    images = _bytes(10, (3, 8, 8), 21)
    for augment, gather_name in ((None, 'lvae_batch_gather_f32'), (FeedAugment(), 'lvae_batch_gather_f32'),
                                 (FeedAugment(hflip=True), 'lvae_batch_gather_aug_f32')):
        ds = DeviceDataset(images, 4, seed=3, augment=augment).attach(_Counted(0))
        names = _record_calls(monkeypatch)
        ds.gather(ds.new_batch())
        ds.advance()
        ds.batch(2)
        assert names == [gather_name, 'lvae_counter_advance', gather_name], (augment, names)
        del names[:]
        list(ds.batches(4))
        first_batches(ds, 2, 4)
        assert names == ['lvae_batch_gather_f32'] * 5                       # storage-order reads: only a binarizing set changes them
        monkeypatch.undo()
    ds = DeviceDataset(images, 4, seed=3, augment=FeedAugment(binarize=True))
    names = _record_calls(monkeypatch)
    list(ds.batches(4))
    assert names == ['lvae_batch_gather_aug_f32'] * 3


@pytest.mark.parametrize('augment', ['binarize+hflip', 'dequantize+hflip'])
def test_gather_at_the_cursor_equals_batch_of_the_step(augment):
    from lvae_amd.data import DeviceDataset, FeedAugment
    images = _bytes(10, (1, 8, 8), 23)
    aug = FeedAugment(binarize='binarize' in augment, dequantize='dequantize' in augment, hflip=True)
    ds = DeviceDataset(images, 4, seed=3, augment=aug)
    spe = ds.steps_per_epoch
    assert spe == 2
    seen = {}
    for c in (0, 1, spe, spe + 1, 5):
        ds.attach(_Counted(c))
        got = ds.gather(ds.new_batch())
        assert int(ds.cursor.item()) == c
        assert torch.equal(got, ds.batch(c + 1)), c
        assert _same_bits(got, _want_batch(ds, images, c + 1)), c
        seen[c] = got.clone()
    assert not torch.equal(seen[0], seen[spe])


def test_same_images_new_noise_each_epoch():
    """N = B: every epoch is the same set of images. The plain feed repeats their pixels, the augmenting one draws them again."""
    from lvae_amd.data import DeviceDataset, FeedAugment
    images = _bytes(4, (1, 8, 8), 24)
    plain = DeviceDataset(images, 4, seed=3)
    aug = DeviceDataset(images, 4, seed=3, augment=FeedAugment(binarize=True))
    by_image = lambda ds, s: ds.batch(s)[ds.indices(s).argsort().cuda()]
    assert torch.equal(by_image(plain, 1), by_image(plain, 2))
    a, b = by_image(aug, 1), by_image(aug, 2)
    assert not torch.equal(a, b) and 0.02 < float((a != b).float().mean()) < 0.6


def test_two_ranks_on_one_device_see_the_global_batch():
    from lvae_amd.data import DeviceDataset, FeedAugment
    images = _bytes(26, (3, 8, 8), 31)
    aug = FeedAugment(dequantize=True, hflip=True)
    whole = DeviceDataset(images, 8, seed=4, augment=aug)
    parts = [DeviceDataset(images, 8, seed=4, rank=r, world=2, augment=aug) for r in (0, 1)]
    for s in (1, 2, 3, 4, 7):
        got = torch.cat([p.batch(s) for p in parts])
        assert got.shape[0] == 8 and torch.equal(got, whole.batch(s)), s
        assert _same_bits(got, _want_batch(whole, images, s)), s
    for p in parts:
        p.attach(_Counted(3))
    got = torch.cat([p.gather(p.new_batch()) for p in parts])
    assert _same_bits(got, _want_batch(whole, images, 4))


def test_captured_graph_across_an_epoch_boundary_equals_eager():
    """N = 10, B = 4: two steps per epoch, so seven replays cross three index-table replacements; the noise follows the cursor."""
    from lvae_amd.data import DeviceDataset, FeedAugment
    images = _bytes(10, (3, 8, 8), 21)
    aug = FeedAugment(binarize=True, hflip=True)
    seen = {}
    for use_graph in (False, True):
        ds = DeviceDataset(images, 4, seed=3, augment=aug).attach(_Counted(0))
        out = ds.new_batch()
        graph = None
        if use_graph:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                ds.gather(out)
                ds.advance()
            assert int(ds.cursor.item()) == 0
        seen[use_graph] = []
        for s in range(1, 8):
            ds.before_step(s - 1)
            if graph is not None:
                graph.replay()
            else:
                ds.gather(out)
                ds.advance()
            seen[use_graph].append(out.clone())
        assert int(ds.cursor.item()) == 7
    for s in range(1, 8):
        assert torch.equal(seen[True][s - 1], seen[False][s - 1]), s
        assert _same_bits(seen[True][s - 1], _want_batch(ds, images, s)), s


# ---- the fixed binarization -----------------------------------------------------------------------------------------------
def test_binarize_fixed():
    from lvae_amd.data import DeviceDataset, FeedAugment, binarize_fixed, first_batches
    images = _bytes(13, (1, 28, 28), 41)
    want = R.binarize_fixed(images.numpy(), 5)
    got = binarize_fixed(images, 5)
    assert got.dtype == torch.uint8 and not got.is_cuda and tuple(got.shape) == (13, 1, 28, 28)
    assert np.array_equal(got.numpy(), want) and set(np.unique(want)) == {0, 1}
    # however the set is cut into launches, and from floats of the same values
    assert torch.equal(binarize_fixed(images, 5, chunk=4), got)
    assert torch.equal(binarize_fixed(images.float().div(255), 5), got)
    assert not torch.equal(binarize_fixed(images, 6), got)
    # an image's binarization depends on its number: a later part of the set alone is numbered from 0 again
    assert torch.equal(binarize_fixed(images[:5], 5), got[:5]) and not torch.equal(binarize_fixed(images[5:], 5), got[5:])
    # black stays black, white stays white
    bw = torch.cat([torch.zeros(1, 1, 28, 28), torch.ones(1, 1, 28, 28)])
    assert torch.equal(binarize_fixed(bw, 5).float(), bw)
    # channels-last storage gives the same NCHW result
    hwc = _bytes(5, (6, 7, 3), 42)
    assert np.array_equal(binarize_fixed(hwc, 2, channels_last=True).numpy(), R.binarize_fixed(hwc.permute(0, 3, 1, 2).numpy(), 2))
    # the storage-order reads of a binarizing set return it, whatever the batch size; a set that only flips returns the images
    ds = DeviceDataset(images, 4, seed=5, rank=1, world=2, augment=FeedAugment(binarize=True, hflip=True))
    for n in (4, 13):
        assert torch.equal(torch.cat(list(ds.batches(n))).cpu(), got.float())
    fb = first_batches(ds, 5, 4)
    assert len(fb) == 3 and torch.equal(torch.cat(fb).cpu(), got[:12].float())
    ds = DeviceDataset(images, 4, seed=5, augment=FeedAugment(hflip=True))
    assert torch.equal(torch.cat(list(ds.batches(5))).cpu(), images.float().div(255))


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


def _train(images, augment, n_steps, how, M):
    """how: 'fed-graph' | 'fed-eager' | 'hand-graph' (the step given feed.batch(...) of its micro-batches by hand)."""
    from lvae_amd.data import DeviceDataset
    from lvae_amd.engine import TrainStep
    from lvae_amd.noise import FrozenNoise
    from lvae_amd.optim import Adamax
    g = load_golden('tiny_cifar')
    _fresh_table()
    m = _model(g.cfg, g.state_dict(), FrozenNoise(seed=11))
    opt = Adamax(m, lr=1e-3)
    ds = DeviceDataset(images, 4, seed=17, augment=augment)
    fed = how.startswith('fed')
    st = TrainStep(m, opt, use_graph=how.endswith('graph'), feed=ds if fed else None, accum_steps=M)
    outs = []
    for s in range(1, n_steps + 1):
        out = st() if fed else st(torch.cat([ds.batch((s - 1) * M + j + 1) for j in range(M)]))
        outs.append({k: v.detach().clone() for k, v in out.items()})
    torch.cuda.synchronize()
    assert (st.graph_a is not None) == how.endswith('graph')
    if fed:
        assert int(ds.cursor.item()) == m.global_step * M == n_steps * M
    return outs, _train_state(m, opt)


@pytest.mark.parametrize('M,augment', [(1, 'binarize+hflip'), (2, 'dequantize+hflip')])
def test_fed_training_with_augmentation_equals_hand_fed_training(M, augment):
    from lvae_amd.data import FeedAugment
    images = torch.floor(256 * torch.rand(12, 3, 32, 32, generator=_gen(5))) / 255   # B = 4: three micro-batches per epoch
    aug = FeedAugment(binarize='binarize' in augment, dequantize='dequantize' in augment, hflip=True)
    n_steps = 5 if M == 1 else 3                                                       # both reach epoch 1
    runs = {how: _train(images, aug, n_steps, how, M) for how in ('hand-graph', 'fed-graph', 'fed-eager')}
    ref_outs, ref_state = runs['hand-graph']
    assert len({float(o['loss']) for o in ref_outs}) == n_steps
    for how in ('fed-graph', 'fed-eager'):
        outs, state = runs[how]
        for s, (a, b) in enumerate(zip(outs, ref_outs), 1):
            for key in ('loss', 'elbo', 'recons', 'kl'):
                assert torch.equal(a[key], b[key]), (how, s, key, float(a[key]), float(b[key]))
        assert state.keys() == ref_state.keys()
        for k in state:
            assert torch.equal(state[k], ref_state[k]), (how, k)


# ---- the trainer ------------------------------------------------------------------------------------------------------
ARGV = ['-d', 'static_mnist', '--likelihood', 'bernoulli', '--zdims', '8', '8', '--downsample', '1', '1', '--nfilters', '16', '--skip', '--gated',
        '--batch-size', '8', '--seed', '3', '--test-batch-size', '8', '--ts-log-every', '2', '--ll-every', '4', '--ll-samples', '4',
        '--log-every', '1', '--device-data', '--binarize', '--hflip']


def _run(module, argv):
    p = subprocess.run([sys.executable, '-m', module] + argv, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return p.stdout


def _main(argv):
    out = _run('lvae_amd.main', argv)
    lines = [re.sub(r'\s*\[\d+ img/s\]', '', line) for line in out.splitlines() if re.search(r'\[step \d+', line)]
    train = {int(re.search(r'\[step (\d+)\]', line).group(1)): line for line in lines if re.search(r'\[step \d+\]', line)}
    test = {int(re.search(r'\[step (\d+), epoch', line).group(1)): line for line in lines if 'epoch' in line}
    return train, test, out


def _ckpt_tensors(path):
    ck = torch.load(path)
    flat = {'model.' + k: v for k, v in ck['model'].items()}
    for name, st in ck['optimizer']['state'].items():
        flat['avg.' + name], flat['inf.' + name] = st['exp_avg'], st['exp_inf']
    meta = (ck['global_step'], ck['optimizer']['step'], ck['noise'], ck.get('test_noise'), ck.get('augment'))
    return flat, meta


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """Every trainer run of this file, once: grey 28x28 images, N = batch, so an epoch is one step and always the same eight images."""
    tmp = tmp_path_factory.mktemp('feed_aug')
    npz = str(tmp / 'grey.npz')
    grey = lambda n, seed: (torch.floor(256 * torch.rand(n, 1, 28, 28, generator=_gen(seed))) / 255).numpy()
    np.savez(npz, data=grey(8, 40), test=grey(12, 41))
    base = ARGV + ['--data-npz', npz]
    full, half, rest = (str(tmp / n) for n in ('full.pt', 'half.pt', 'rest.pt'))
    r = {'full': full, 'rest': rest, 'npz': npz}
    r['a'] = _main(base + ['--steps', '8', '--save-checkpoint', full])
    r['b'] = _main(base + ['--steps', '8'])
    r['first'] = _main(base + ['--steps', '4', '--save-checkpoint', half])
    r['second'] = _main(base + ['--steps', '8', '--resume', half, '--save-checkpoint', rest])
    r['other'] = _main([a for a in base if a != '--hflip'] + ['--steps', '5', '--resume', half])
    r['eval'] = _run('lvae_amd.evaluate', [a for a in base if a not in ('--device-data', '--hflip')] + ['--checkpoint', full, '--ll'])
    return r


def test_trainer_repeats(runs):
    tr_a, te_a, out_a = runs['a']
    assert sorted(tr_a) == list(range(1, 9)) and sorted(te_a) == [2, 4, 6, 8], out_a
    assert ',binarize,hflip,' in out_a and '1 steps per epoch' in out_a
    tr_b, te_b, _ = runs['b']
    assert tr_b == tr_a and te_b == te_a
    assert 'warning' not in out_a


def test_trainer_resumes_exactly(runs):
    tr_a, te_a, _ = runs['a']
    (tr_1, te_1, _), (tr_2, te_2, out_2) = runs['first'], runs['second']
    assert sorted(tr_2) == [5, 6, 7, 8] and 'warning' not in out_2
    assert {**tr_1, **tr_2} == tr_a and {**te_1, **te_2} == te_a
    (fa, ma), (fb, mb) = _ckpt_tensors(runs['full']), _ckpt_tensors(runs['rest'])
    assert ma == mb and ma[0] == 8
    assert ma[4] == {'binarize': True, 'hflip': True, 'dequantize': False, 'seed': 3}
    assert fa.keys() == fb.keys()
    for k in fa:
        assert torch.equal(fa[k], fb[k]), k


def test_trainer_epochs_do_not_repeat(runs):
    """Every step is one epoch over the same eight images. (The lines of two steps differ through the weights and the latent draws as
    well: that the pixels themselves are drawn again is test_same_images_new_noise_each_epoch's.)"""
    tr_a, te_a, _ = runs['a']
    assert [int(re.search(r'epoch (\d+)', te_a[s]).group(1)) for s in (2, 4, 6, 8)] == [1, 3, 5, 7]
    assert tr_a[1] != tr_a[2] and len(set(tr_a.values())) == 8


def test_resuming_with_other_flags_warns(runs):
    tr, _, out = runs['other']
    assert sorted(tr) == [5]
    warn = [line for line in out.splitlines() if line.startswith('warning') and 'feed augmentation' in line]
    assert len(warn) == 1 and "'hflip': True" in warn[0] and "'hflip': False" in warn[0]


def test_evaluate_binarizes_with_the_checkpoints_seed(runs):
    out = runs['eval']
    assert 'evaluation images binarized: fixed, seed 3' in out
    assert re.search(r'ELBO -?[\d.]+', out), out
