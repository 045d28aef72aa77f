"""The device-fed gather's augmentation without a GPU: properties of the numpy restatement of its noise rule (tests/feed_aug_ref.py), the
refusals of data.FeedAugment and of the trainer's flags, the records that go into checkpoints and run descriptions, and the C header."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import feed_aug_ref as R
from oracle.philox_ref import U01_MAX


# ---- the restatement ----------------------------------------------------------------------------------------------------
def test_binarize_keeps_black_and_white():
    u = R.pixel_u(4096, R.aug_seed(3), 5, 2)
    assert float(u.min()) >= 2.0 ** -25 and float(u.max()) <= float(U01_MAX)
    assert not R.binarize(np.zeros(4096, np.float32), u).any()
    assert R.binarize(np.ones(4096, np.float32), u).all()
    grey = R.binarize(np.full(4096, 0.25, np.float32), u)
    assert set(np.unique(grey)) == {0.0, 1.0} and 0.2 < grey.mean() < 0.3
    # the bounds of u themselves: the smallest draw is above 0, the largest below 1
    assert R.binarize(np.float32(0), np.float32(2.0 ** -25)) == 0 and R.binarize(np.float32(1), U01_MAX) == 1


def test_dequantized_values_stay_in_their_bin():
    b = np.arange(256, dtype=np.uint8).repeat(64)
    u = R.pixel_u(b.size, R.aug_seed(11), 1, 0)
    x = R.dequantize(b, u)
    assert x.dtype == np.float32
    lo = b.astype(np.float64) / 256
    hi = np.minimum((b.astype(np.float64) + 1) / 256, 1 - 2.0 ** -24)
    assert (x >= lo).all() and (x <= hi).all()
    # 255 + (1 - 2^-24) rounds to 256 in fp32: without the clamp the value would be 1.0
    assert np.float32(255) + U01_MAX == np.float32(256)
    top = R.dequantize(np.array([255], np.uint8), np.array([U01_MAX]))
    assert top[0] == U01_MAX and top[0] < 1


def test_rows_steps_and_tags_draw_different_words():
    s = R.aug_seed(3)
    base = R.pixel_words(64, s, 4, 9)
    assert np.array_equal(base, R.pixel_words(64, s, 4, 9))
    for other in (R.pixel_words(64, s, 5, 9), R.pixel_words(64, s, 4, 10), R.pixel_words(64, s, 4, 9, R.TAG_FIXED),
                  R.pixel_words(64, s, 4, 9, R.TAG_FLIP), R.pixel_words(64, s, 4 + 2 ** 32, 9), R.pixel_words(64, s + 1, 4, 9)):
        assert not np.array_equal(base, other)
        assert (base == other).mean() < 0.1
    # a shorter row is a prefix: element e of a row draws the same word whatever the row's length
    assert np.array_equal(R.pixel_words(35, s, 4, 9), base[:35])


def test_flip_counts_are_pinned():
    for seed, want in ((3, 2025), (11, 2005)):
        s = R.aug_seed(seed)
        assert sum(R.row_flips(s, P, g) for P in (0, 7) for g in range(2048)) == want


def test_flip_mirrors_the_source_not_the_noise():
    rows = np.arange(2 * 1 * 2 * 4, dtype=np.uint8).reshape(2, 1, 2, 4)
    s = R.aug_seed(3)
    P = next(P for P in range(64) if R.row_flips(s, P, 0) and not R.row_flips(s, P, 1))
    out, flipped = R.augment(rows, s, P, [0, 1], None, hflip=True)
    assert flipped == [0]
    assert np.array_equal(out[0], R.plain(rows[0][:, :, ::-1])) and np.array_equal(out[1], R.plain(rows[1]))
    # under dequantize the noise of an output element is the same flipped or not
    deq_f, _ = R.augment(rows, s, P, [0, 1], 'dequantize', hflip=True)
    deq_n, _ = R.augment(rows[:, :, :, ::-1], s, P, [0, 1], 'dequantize', hflip=False)
    assert np.array_equal(deq_f[0], deq_n[0])
    # fixed: never flipped, P plays no part
    fx, flipped = R.augment(rows, s, P, [0, 1], 'binarize', hflip=True, fixed=True)
    assert flipped == [] and np.array_equal(fx, R.augment(rows, s, 0, [0, 1], 'binarize', fixed=True)[0])


def test_aug_seed():
    assert R.aug_seed(0) == 0x5851F42D4C957F2D
    assert R.aug_seed(3) == (3 * 0x9E3779B97F4A7C15 + 0x5851F42D4C957F2D) % 2 ** 63
    from lvae_amd.data import aug_seed
    for s in (0, 3, 11, 54321, 2 ** 40 + 1):
        assert aug_seed(s) == R.aug_seed(s) and 0 <= aug_seed(s) < 2 ** 63


# ---- FeedAugment and the flags -----------------------------------------------------------------------------------------
def test_feed_augment():
    from lvae_amd.data import FeedAugment
    assert not FeedAugment() and FeedAugment().mode is None
    assert FeedAugment(binarize=True).mode == 'binarize' and FeedAugment(dequantize=True, hflip=True).mode == 'dequantize'
    assert FeedAugment(hflip=True) and FeedAugment(hflip=True).mode is None
    with pytest.raises(ValueError):
        FeedAugment(binarize=True, dequantize=True)
    assert FeedAugment(binarize=True, hflip=True).record() == {'binarize': True, 'hflip': True, 'dequantize': False}
    assert FeedAugment().record() == {'binarize': False, 'hflip': False, 'dequantize': False}


def test_dataset_takes_an_augment_and_refuses_dequantizing_floats():
    import torch
    from lvae_amd.data import DeviceDataset, FeedAugment
    grid = torch.randint(0, 256, (8, 1, 4, 4), dtype=torch.uint8)
    assert DeviceDataset(grid, 4, seed=1).augment is None
    assert DeviceDataset(grid, 4, seed=1, augment=FeedAugment()).augment is None          # nothing on: today's path
    assert DeviceDataset(grid, 4, seed=1, augment=FeedAugment(dequantize=True)).augment.dequantize
    assert DeviceDataset(grid.float().div(255), 4, seed=1, augment=FeedAugment(dequantize=True)).kind == 'uint8'
    with pytest.raises(ValueError):
        DeviceDataset(torch.rand(8, 1, 4, 4), 4, seed=1, augment=FeedAugment(dequantize=True))   # not k/255: kept as float32
    assert DeviceDataset(torch.rand(8, 1, 4, 4), 4, seed=1, augment=FeedAugment(binarize=True)).kind == 'float32'


def _parse(*argv):
    from lvae_amd.experiment.experiment_manager import build_parser
    return build_parser().parse_args(list(argv))


def _check(*argv):
    from lvae_amd.experiment.experiment_manager import LVAEExperiment
    return LVAEExperiment._check_args(_parse(*argv))


NPZ = ('--device-data', '--data-npz', 'x.npz')


def test_flags_default_to_off_and_are_accepted():
    a = _check(*NPZ)
    assert (a.binarize, a.hflip, a.dequantize) == (False, False, False)
    a = _check(*NPZ, '--binarize', '--hflip')                                  # static_mnist: bernoulli by default
    assert a.binarize and a.hflip and not a.dequantize
    a = _check(*NPZ, '-d', 'cifar10', '--likelihood', 'gaussian', '--dequantize', '--hflip')
    assert a.dequantize and a.hflip
    assert _check(*NPZ, '-d', 'cifar10', '--hflip').hflip                      # a flip suits every likelihood


@pytest.mark.parametrize('argv', [
    ('--synthetic', '--binarize'), ('--synthetic', '--hflip'), ('--synthetic', '--likelihood', 'gaussian', '--dequantize'),
    ('--data-npz', 'x.npz', '--hflip'),                                                      # no --device-data
    NPZ + ('--binarize', '--likelihood', 'gaussian'), NPZ + ('-d', 'cifar10', '--binarize'),   # not bernoulli
    NPZ + ('--dequantize',), NPZ + ('-d', 'cifar10', '--dequantize'), NPZ + ('--likelihood', 'discr_log', '--dequantize'),
    NPZ + ('--binarize', '--dequantize'), NPZ + ('--likelihood', 'gaussian', '--binarize', '--dequantize'),
])
def test_check_args_refusals(argv):
    with pytest.raises(SystemExit) as e:
        _check(*argv)
    assert isinstance(e.value.code, str) and '--' in e.value.code              # a message, not an exit status


def test_refusal_messages_name_the_reason():
    for argv, word in ((('--synthetic', '--hflip'), '--device-data'), (NPZ + ('--binarize', '--likelihood', 'gaussian'), 'bernoulli'),
                       (NPZ + ('-d', 'cifar10', '--dequantize'), 'gaussian'), (NPZ + ('--binarize', '--dequantize'), 'exclude')):
        with pytest.raises(SystemExit) as e:
            _check(*argv)
        assert word in e.value.code, e.value.code


# ---- records ---------------------------------------------------------------------------------------------------------
def test_run_description_suffixes():
    from lvae_amd.experiment.experiment_manager import LVAEExperiment as E
    d = E._make_run_description
    plain = d(_check(*NPZ))
    assert 'binarize' not in plain and 'hflip' not in plain and 'dequant' not in plain
    assert ',binarize,' in d(_check(*NPZ, '--binarize')) and ',hflip' not in d(_check(*NPZ, '--binarize'))
    both = d(_check(*NPZ, '--binarize', '--hflip'))
    assert ',binarize,hflip,' in both
    deq = d(_check(*NPZ, '--likelihood', 'gaussian', '--dequantize', '--hflip'))
    assert ',hflip,dequant,' in deq and 'binarize' not in deq
    assert both.replace(',binarize,hflip', '') == plain
    ns = _check(*NPZ)                                                          # a namespace from before the flags still describes itself
    for k in ('binarize', 'hflip', 'dequantize'):
        delattr(ns, k)
    assert d(ns) == plain


def test_checkpoint_record():
    from lvae_amd.checkpoint import augment_record
    from lvae_amd.experiment.experiment_manager import LVAEExperiment as E
    assert E.augment_record(_check(*NPZ)) is None and E.feed_augment(_check(*NPZ)) is None
    rec = E.augment_record(_check(*NPZ, '--binarize', '--hflip', '--seed', '7'))
    assert rec == {'binarize': True, 'hflip': True, 'dequantize': False, 'seed': 7}
    assert E.feed_augment(_check(*NPZ, '--hflip')).record() == {'binarize': False, 'hflip': True, 'dequantize': False}
    assert augment_record({'model': {}, 'augment': rec}) == rec
    assert augment_record({'model': {}}) is None                               # a file without the key means none
    assert augment_record({'w': 0}) is None                                    # a bare state_dict


def test_evaluate_flags():
    from lvae_amd.evaluate import parse_eval_args
    a = parse_eval_args(['--synthetic', '--ll', '--binarize'])
    assert a.eval_binarize and not a.binarize and a.binarize_seed is None      # not the trainer's flag: --device-data is not asked for
    assert parse_eval_args(['--synthetic', '--ll', '--binarize', '--binarize-seed', '9']).binarize_seed == 9
    assert not parse_eval_args(['--synthetic', '--ll']).eval_binarize
    for argv in (['--synthetic', '--ll', '--binarize-seed', '9'], ['--synthetic', '--ll', '--hflip'],
                 ['--synthetic', '--ll', '-d', 'cifar10', '--binarize']):
        with pytest.raises(SystemExit):
            parse_eval_args(argv)


# ---- the header and the binding -------------------------------------------------------------------------------------------
def _header():
    hdr = open(os.path.join(ROOT, 'include', 'lvae_hip.h')).read()
    return re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)


def _header_fields(struct):
    hdr = _header()
    body = hdr[hdr.index('typedef struct %s {' % struct):hdr.index('} %s;' % struct)]
    body = body[body.index('{') + 1:]
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            ty, names = decl.rsplit(' ', 1)[0].strip(), decl.rsplit(' ', 1)[1]
            fields += [(n.strip(), ty) for n in names.split(',')]
    return fields


def test_header_declares_the_struct_and_the_entry_point():
    import ctypes as C
    import lvae_amd  # noqa: F401
    from lvae_amd import _C
    hdr = _header()
    assert 'lvae_batch_gather_aug_f32' in sorted(set(re.findall(r'\b(lvae_[a-z0-9_]+)\s*\(', hdr)))
    assert 'lvae_batch_gather_aug_f32' in _C.SIGNATURES and 'lvae_batch_gather_f32' in _C.SIGNATURES
    fields = _header_fields('lvae_feed_aug')
    assert fields == [('seed', 'uint64_t'), ('position', 'int64_t'), ('mode', 'int32_t'), ('hflip', 'int32_t'), ('fixed', 'int32_t')]
    ctype = {'uint64_t': C.c_uint64, 'int64_t': C.c_int64, 'int32_t': C.c_int32}
    assert [(n, ctype[t]) for n, t in fields] == list(_C.FeedAug._fields_)
    assert C.sizeof(_C.FeedAug) == 32 and _C.FeedAug.mode.offset == 16 and _C.FeedAug.fixed.offset == 24
    # the aug entry point takes the plain one's arguments, then the struct, then the stream
    plain, aug = _C.SIGNATURES['lvae_batch_gather_f32'][1], _C.SIGNATURES['lvae_batch_gather_aug_f32'][1]
    assert aug == plain[:-1] + [C.POINTER(_C.FeedAug)] + plain[-1:]
    enum = re.search(r'enum \{ LVAE_AUG_NONE = (\d+), LVAE_AUG_BINARIZE = (\d+), LVAE_AUG_DEQUANTIZE = (\d+) \}', hdr)
    assert tuple(int(v) for v in enum.groups()) == (_C.AUG_NONE, _C.AUG_BINARIZE, _C.AUG_DEQUANTIZE)
    for name, val in (('PIXEL', R.TAG_PIXEL), ('FLIP', R.TAG_FLIP), ('FIXED', R.TAG_FIXED)):
        assert int(re.search(r'#define LVAE_AUG_TAG_%s (0x[0-9A-Fa-f]+)' % name, hdr).group(1), 16) == val == getattr(_C, 'AUG_TAG_' + name)
    assert int(re.search(r'#define LVAE_ABI_VERSION (\d+)', hdr).group(1)) == _C.ABI_VERSION


def test_philox_is_defined_once():
    csrc = os.path.join(ROOT, 'ladder-vae-pytorch_amd', 'csrc')
    where = [f for f in sorted(os.listdir(csrc)) if f.endswith(('.hip', '.h', '.inc'))
             and re.search(r'void\s+philox4\s*\(', open(os.path.join(csrc, f)).read())]
    assert where == ['philox.h']
    for f in ('misc.hip', 'batch_feed.hip'):
        assert '#include "philox.h"' in open(os.path.join(csrc, f)).read(), f
