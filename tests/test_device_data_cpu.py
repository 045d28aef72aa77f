"""Device-resident training data, the parts that need no GPU: the data order as a function of (seed, step), the storage decision,
and the trainer's flag."""
import pytest
import torch


def test_epoch_permutation_is_a_pure_permutation():
    from lvae_amd.data import epoch_permutation
    for n in (1, 10, 257, 50000):
        p = epoch_permutation(7, 3, n)
        assert p.dtype == torch.int64 and p.shape == (n,)
        assert torch.equal(torch.sort(p).values, torch.arange(n))
    a = epoch_permutation(54321, 2, 257)
    torch.manual_seed(99)                       # neither the process-wide generator ...
    torch.randperm(1000)
    epoch_permutation(1, 1, 33)                 # ... nor an earlier call changes it
    assert torch.equal(epoch_permutation(54321, 2, 257), a)
    assert not torch.equal(epoch_permutation(3, 0, 257), epoch_permutation(3, 1, 257))
    assert not torch.equal(epoch_permutation(3, 0, 257), epoch_permutation(4, 0, 257))


def _bytes(n, shape, seed):
    return torch.randint(0, 256, (n,) + shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def test_indices_cover_an_epoch_and_follow_the_permutations():
    from lvae_amd.data import DeviceDataset, epoch_permutation
    ds = DeviceDataset(_bytes(26, (1, 4, 4), 0), 4, seed=5)
    assert ds.steps_per_epoch == 6 and ds.N == 26
    epoch0 = torch.cat([ds.indices(s) for s in range(1, 7)])
    assert epoch0.shape == (24,) and len(set(epoch0.tolist())) == 24
    assert int(epoch0.min()) >= 0 and int(epoch0.max()) < 26
    assert torch.equal(epoch0, epoch_permutation(5, 0, 26)[:24])
    assert torch.equal(ds.indices(7), epoch_permutation(5, 1, 26)[:4])          # step 7 begins epoch 1
    assert torch.equal(ds.indices(12), epoch_permutation(5, 1, 26)[20:24])
    assert torch.equal(ds.indices(3), epoch0[8:12])                              # going back is allowed: no hidden position
    assert [ds.epoch_of(s) for s in (1, 6, 7, 12, 13)] == [0, 0, 1, 1, 2]
    with pytest.raises(ValueError):
        ds.indices(0)


def test_two_shards_make_the_global_batch():
    from lvae_amd.data import DeviceDataset
    imgs = _bytes(26, (1, 4, 4), 1)
    whole = DeviceDataset(imgs, 4, seed=5)
    parts = [DeviceDataset(imgs, 4, seed=5, rank=r, world=2) for r in (0, 1)]
    assert [(p.lo, p.hi) for p in parts] == [(0, 2), (2, 4)] and (whole.lo, whole.hi) == (0, 4)
    for s in (1, 6, 7, 20):
        got = torch.cat([p.indices(s)[p.lo:p.hi] for p in parts])
        assert torch.equal(got, whole.indices(s))


def test_too_few_images_for_one_batch():
    from lvae_amd.data import DeviceDataset
    with pytest.raises(ValueError):
        DeviceDataset(_bytes(3, (1, 4, 4), 2), 4, seed=0)
    with pytest.raises(ValueError):
        DeviceDataset(_bytes(8, (1, 4, 4), 2), 4, seed=0, rank=0, world=3)     # the global batch does not split evenly
    DeviceDataset(_bytes(3, (1, 4, 4), 2), None, seed=0)                        # storage order only: no batch to fill


def test_device_storage_keeps_what_round_trips_as_bytes():
    from lvae_amd.data import device_storage
    g = torch.Generator().manual_seed(3)
    x = torch.floor(256 * torch.rand(64, 3, 32, 32, generator=g)) / 255        # the law of ToTensor data
    a, kind = device_storage(x)
    assert kind == 'uint8' and a.dtype == torch.uint8 and a.shape == x.shape
    assert torch.equal(a.float().div_(255.0), x)
    every = (torch.arange(256).float() / 255).view(1, 1, 16, 16)               # all 256 values
    a, kind = device_storage(every)
    assert kind == 'uint8' and torch.equal(a.view(-1), torch.arange(256, dtype=torch.uint8))
    b = (torch.rand(16, 1, 28, 28, generator=g) > 0.5).float()                 # 0/1 data
    a, kind = device_storage(b)
    assert kind == 'uint8' and set(a.unique().tolist()) <= {0, 255}
    r = torch.rand(8, 3, 8, 8, generator=g)
    a, kind = device_storage(r)
    assert kind == 'float32' and a.dtype == torch.float32 and torch.equal(a, r)
    for bad in (x.clone().index_put_((torch.tensor(0),) * 4, torch.tensor(float('nan'))), x + 1.0, -x - 1 / 255):
        a, kind = device_storage(bad)
        assert kind == 'float32' and a.dtype == torch.float32
        assert torch.equal(a.isnan(), bad.isnan()) and torch.equal(a.nan_to_num(7.0), bad.nan_to_num(7.0))
    u = _bytes(5, (3, 4, 4), 4)
    a, kind = device_storage(u)
    assert kind == 'uint8' and torch.equal(a, u)


def test_dataset_reports_its_storage():
    from lvae_amd.data import DeviceDataset
    x = torch.floor(256 * torch.rand(10, 3, 8, 8, generator=torch.Generator().manual_seed(1))) / 255
    ds = DeviceDataset(x, 2, seed=0)
    assert ds.kind == 'uint8' and ds.nbytes == 10 * 3 * 8 * 8 and ds.chw == (3, 8, 8)
    ds = DeviceDataset(_bytes(10, (8, 6, 3), 0), 2, seed=0, channels_last=True)
    assert ds.chw == (3, 8, 6) and ds.rows == 2
    with pytest.raises(ValueError):
        DeviceDataset(torch.rand(10, 8, 6, 3), 2, seed=0, channels_last=True)
    with pytest.raises(ValueError):
        DeviceDataset(torch.rand(10, 8, 6), 2, seed=0)


def test_device_data_flag():
    from lvae_amd.experiment.experiment_manager import LVAEExperiment, build_parser
    p = build_parser()
    assert p.parse_args([]).device_data is False
    args = LVAEExperiment._check_args(p.parse_args(['--device-data', '--data-npz', 'x.npz']))
    assert args.device_data is True
    with pytest.raises(SystemExit) as e:
        LVAEExperiment._check_args(p.parse_args(['--device-data', '--synthetic']))
    assert '--device-data' in str(e.value) and '--synthetic' in str(e.value)


def test_gather_symbol_is_declared_and_bound():
    import os
    import re
    from lvae_amd import _C
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, 'include', 'lvae_hip.h')).read()
    assert re.search(r'\bint lvae_batch_gather_f32\(', hdr)
    assert len(_C.SIGNATURES['lvae_batch_gather_f32'][1]) == 16
    assert hasattr(_C.load(), 'lvae_batch_gather_f32')
