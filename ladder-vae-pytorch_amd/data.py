"""Data pipeline of the reference (experiment/data.py:17-115, lib/datasets.py:9-72) without torchvision and without
downloads (there is no network here): the same on-disk formats, the same tensors.

* static_mnist: `binarized_mnist_{train,valid,test}.npz` (key `data`, float32 (N,1,28,28)) under ./data/static_bin_mnist/;
  a Larochelle `.amat` text file next to a missing `.npz` is converted exactly as the reference does after its download
  (lib/datasets.py:55-64). train = train + valid concatenated (:14-18), labels are NaN (:21), both splits are shuffled once at
  load (`shuffle_init=True`, experiment/data.py:43-50).
* cifar10: the `cifar-10-batches-py` pickle batches under ./data/cifar10/ — uint8 HWC -> float CHW / 255 (`ToTensor`, :47-52).
* svhn: `train_32x32.mat` / `test_32x32.mat` under ./data/svhn/ (scipy.io) — same `ToTensor` scaling (:64).
* celeba: pre-decoded aligned images `celeba_aligned_uint8.npy` ((N,218,178,3) uint8, memory-mapped) + the stock
  `list_eval_partition.txt` under ./data/celeba/ — CenterCrop(148) + Resize((64,64)) + ToTensor (:76-80) restated on the arrays:
  torchvision's crop offsets (round((218-148)/2) = 35, round((178-148)/2) = 15) and Pillow's two-pass fixed-point antialiased
  bilinear resize, bit for bit (tests/golden/celeba_resize.npz was made with Pillow itself). JPEG decoding is not on this path.
Loaders: train shuffled with drop_last, test in order with `test_batch_size` (:99-106).

`DeviceDataset` (below the loaders) keeps a whole image set in device memory instead and lets the training step gather its own batch:
the order is a pure function of (seed, global step), so a run with real data repeats and resumes exactly.
"""
import os
import pickle

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset, TensorDataset


def amat_to_npz(path_amat, path_npz=None):
    """One line of 784 space-separated 0/1 per image -> float32 (N,1,28,28) saved compressed under key `data`."""
    with open(path_amat) as f:
        rows = [np.array(line.split(), dtype=np.float32) for line in f if line.strip()]
    x = np.stack(rows).reshape(-1, 1, 28, 28)
    if path_npz is None:
        path_npz = path_amat[:-len('.amat')] + '.npz'
    np.savez_compressed(path_npz, data=x)
    return x


class StaticBinaryMnist(TensorDataset):
    """lib/datasets.py:9-72."""

    def __init__(self, folder, train, shuffle_init=False):
        splits = ['train', 'valid'] if train else ['test']
        x = np.concatenate([self._load(folder, sp, shuffle_init) for sp in splits], axis=0)
        labels = torch.full((len(x),), float('nan'))
        super().__init__(torch.from_numpy(x), labels)

    @staticmethod
    def _load(folder, split, shuffle_init):
        npz = os.path.join(folder, 'binarized_mnist_%s.npz' % split)
        amat = os.path.join(folder, 'binarized_mnist_%s.amat' % split)
        if os.path.exists(npz):
            x = np.load(npz)['data']
        elif os.path.exists(amat):
            x = amat_to_npz(amat, npz)
        else:
            raise RuntimeError("Dataset file '%s' not found and nothing can be downloaded here: place binarized_mnist_%s.npz "
                               "(or the .amat it is made from) in %s" % (npz, split, folder))
        x = np.ascontiguousarray(x, dtype=np.float32)
        if shuffle_init:
            np.random.shuffle(x)
        return x


def _cifar10(folder, train):
    root = os.path.join(folder, 'cifar-10-batches-py')
    names = ['data_batch_%d' % i for i in range(1, 6)] if train else ['test_batch']
    xs, ys = [], []
    for n in names:
        path = os.path.join(root, n)
        if not os.path.exists(path):
            raise RuntimeError("CIFAR10 batch '%s' not found and nothing can be downloaded here" % path)
        with open(path, 'rb') as f:
            d = pickle.load(f, encoding='latin1')
        xs.append(np.asarray(d['data'], dtype=np.uint8).reshape(-1, 3, 32, 32))
        ys.append(np.asarray(d['labels'] if 'labels' in d else d['fine_labels'], dtype=np.int64))
    x = torch.from_numpy(np.concatenate(xs)).float().div_(255.0)   # ToTensor: 0, 1/255, ..., 1
    return TensorDataset(x, torch.from_numpy(np.concatenate(ys)))


def _svhn(folder, train):
    from scipy.io import loadmat
    path = os.path.join(folder, '%s_32x32.mat' % ('train' if train else 'test'))
    if not os.path.exists(path):
        raise RuntimeError("SVHN file '%s' not found and nothing can be downloaded here" % path)
    m = loadmat(path)
    x = torch.from_numpy(np.transpose(m['X'], (3, 2, 0, 1)).copy()).float().div_(255.0)
    y = torch.from_numpy(m['y'].astype(np.int64).squeeze() % 10)
    return TensorDataset(x, y)


# ---------------------------------------------------------------------------------------------------------------------
# CelebA (experiment/data.py:76-89): transforms.CenterCrop(148) -> transforms.Resize((64, 64)) -> transforms.ToTensor()
# ---------------------------------------------------------------------------------------------------------------------
_PRECISION_BITS = 32 - 8 - 2  # Pillow's 8-bit resampler: coefficients in 22-bit fixed point


def _pil_bilinear_coeffs(in_size, out_size):
    """Pillow `precompute_coeffs` + `normalize_coeffs_8bpc` for the BILINEAR filter over the whole axis: per output position the first
    source index, the tap count and the integer taps (antialiased: the triangle is widened by the downscale factor)."""
    scale = in_size / out_size
    fscale = max(scale, 1.0)
    support = 1.0 * fscale
    ksize = int(np.ceil(support)) * 2 + 1
    xmin = np.zeros(out_size, dtype=np.int64)
    kk = np.zeros((out_size, ksize), dtype=np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), in_size)
        w = np.array([max(0.0, 1.0 - abs((x + lo - center + 0.5) / fscale)) for x in range(hi - lo)], dtype=np.float64)
        ww = w.sum()
        if ww != 0.0:
            w = w / ww
        xmin[xx] = lo
        kk[xx, :hi - lo] = np.where(w < 0, -0.5 + w * (1 << _PRECISION_BITS), 0.5 + w * (1 << _PRECISION_BITS)).astype(np.int64)
    return xmin, kk


def _pil_resample_axis(a, axis, out_size):
    """One pass of Pillow's 8-bit resampler along `axis` of a uint8 array: sum of integer taps, rounded, clipped to [0, 255]."""
    xmin, kk = _pil_bilinear_coeffs(a.shape[axis], out_size)
    idx = np.minimum(xmin[:, None] + np.arange(kk.shape[1])[None, :], a.shape[axis] - 1)   # taps beyond the edge have weight 0
    g = np.take(a, idx.reshape(-1), axis=axis).astype(np.int64)
    shp = list(a.shape)
    shp[axis:axis + 1] = [out_size, kk.shape[1]]
    g = g.reshape(shp)
    kshape = [1] * g.ndim
    kshape[axis], kshape[axis + 1] = out_size, kk.shape[1]
    acc = (g * kk.reshape(kshape)).sum(axis=axis + 1) + (1 << (_PRECISION_BITS - 1))
    return np.clip(acc >> _PRECISION_BITS, 0, 255).astype(np.uint8)


def celeba_transform_uint8(imgs, crop=148, size=64):
    """(N,H,W,3) uint8 aligned CelebA images -> (N,size,size,3) uint8: torchvision CenterCrop(crop) then Pillow's
    Image.resize((size, size), BILINEAR) — horizontal pass first, then vertical, each rounded to 8 bits as Pillow does."""
    imgs = np.asarray(imgs)
    H, W = imgs.shape[1:3]
    top, left = int(round((H - crop) / 2.0)), int(round((W - crop) / 2.0))
    c = imgs[:, top:top + crop, left:left + crop, :]
    return _pil_resample_axis(_pil_resample_axis(c, 2, size), 1, size)


class CelebAArrays(Dataset):
    """torchvision.datasets.CelebA(split=...) + the transform above, from pre-decoded arrays. Items: (float32 (3,64,64) in [0,1], 0).
    The resized set is kept as uint8 (2.5 GB for the 202,599 images); ToTensor's /255 happens per item, as in the reference."""

    SPLITS = {'train': 0, 'valid': 1, 'test': 2}

    def __init__(self, folder, split, chunk=2048):
        arr = os.path.join(folder, 'celeba_aligned_uint8.npy')
        part = os.path.join(folder, 'list_eval_partition.txt')
        if not (os.path.exists(arr) and os.path.exists(part)):
            raise RuntimeError("CelebA needs '%s' ((N,218,178,3) uint8, the aligned images decoded once) and '%s'; nothing can be "
                               "downloaded or JPEG-decoded here" % (arr, part))
        raw = np.load(arr, mmap_mode='r')
        with open(part) as f:
            which = np.array([int(line.split()[1]) for line in f if line.strip()], dtype=np.int64)
        if len(which) != raw.shape[0]:
            raise RuntimeError("CelebA: %d partition lines for %d images" % (len(which), raw.shape[0]))
        idx = np.nonzero(which == self.SPLITS[split])[0]
        out = np.empty((len(idx), 64, 64, 3), dtype=np.uint8)
        for i in range(0, len(idx), chunk):
            out[i:i + chunk] = celeba_transform_uint8(raw[idx[i:i + chunk]])
        self.data = torch.from_numpy(out)

    def __len__(self):
        return self.data.shape[0]

    def __getitem__(self, i):
        return self.data[i].permute(2, 0, 1).float().div_(255.0), 0


FOLDERS = {'static_mnist': './data/static_bin_mnist/', 'cifar10': './data/cifar10/', 'svhn': './data/svhn/',
           'celeba': './data/celeba/'}


class DatasetLoader:
    """experiment/data.py:17-115: `.train`, `.test` (DataLoaders), `.data_shape`, `.img_size`, `.color_ch`."""

    def __init__(self, args, folder=None):
        name = args.dataset_name
        folder = folder or FOLDERS.get(name)
        if name == 'static_mnist':
            train_set = StaticBinaryMnist(folder, train=True, shuffle_init=True)
            test_set = StaticBinaryMnist(folder, train=False, shuffle_init=True)
        elif name == 'cifar10':
            train_set, test_set = _cifar10(folder, True), _cifar10(folder, False)
        elif name == 'svhn':
            train_set, test_set = _svhn(folder, True), _svhn(folder, False)
        elif name == 'celeba':
            train_set, test_set = CelebAArrays(folder, 'train'), CelebAArrays(folder, 'valid')
        else:
            raise RuntimeError("data set '%s' has no loader in this build (static_mnist, cifar10, svhn, celeba; or --data-npz / "
                               "--synthetic)" % name)
        self.train = DataLoader(train_set, batch_size=args.batch_size, shuffle=True, drop_last=True)
        self.test = DataLoader(test_set, batch_size=args.test_batch_size, shuffle=False)
        self.data_shape = self.train.dataset[0][0].size()
        self.img_size = self.data_shape[1:]
        self.color_ch = self.data_shape[0]


# ---------------------------------------------------------------------------------------------------------------------
# Device-resident data: the image table in HBM, one gather launch per batch (csrc/batch_feed.hip)
# ---------------------------------------------------------------------------------------------------------------------
def epoch_permutation(seed, epoch, n):
    """The order in which epoch `epoch` (0-based) visits the n images: a pure function of its arguments, identical on every rank."""
    mix = (int(seed) * 0x9E3779B1 + int(epoch) * 0x85EBCA77 + 0x165667B1) % (1 << 63)
    return torch.randperm(int(n), generator=torch.Generator().manual_seed(mix))


def device_storage(x):
    """(array, kind) a host image set is kept as on the device: float32 images whose every value is k/255 exactly (ToTensor data, 0/1
    data) become uint8 — a quarter of the memory, and the gather's v/255 gives back the same floats bit for bit — anything else stays
    float32, unchanged. uint8 input stays uint8. kind is 'uint8' or 'float32'."""
    x = torch.as_tensor(x)
    if x.dtype == torch.uint8:
        return x.contiguous(), 'uint8'
    x = x.float().contiguous()
    q = (x * 255.0).round()
    if bool(((q >= 0) & (q <= 255)).all()):
        u = q.to(torch.uint8)
        if torch.equal(u.float().div_(255.0), x):
            return u, 'uint8'
    return x, 'float32'


def aug_seed(seed):
    """The seed of the feed's augmentation noise, from the run's data seed (kept apart from epoch_permutation's mix of the same seed)."""
    return (int(seed) * 0x9E3779B97F4A7C15 + 0x5851F42D4C957F2D) & (2 ** 63 - 1)


class FeedAugment:
    """What the device-fed gather does to a training batch on its way (csrc/batch_feed.hip): binarize draws every pixel afresh as
    Bernoulli(value) each time it is visited (dynamic binarization), hflip mirrors each row left-right with probability 1/2,
    dequantize adds uniform noise below one 8-bit step: (b + u) / 256. The noise is a pure function of (seed, feed cursor, place in the
    global batch, element): nothing advances, nothing has to be saved, and every world size sees the same images."""

    def __init__(self, binarize=False, hflip=False, dequantize=False):
        self.binarize, self.hflip, self.dequantize = bool(binarize), bool(hflip), bool(dequantize)
        if self.binarize and self.dequantize:
            raise ValueError("binarize and dequantize exclude each other: one makes 0/1 pixels, the other continuous ones")

    @property
    def mode(self):
        return 'binarize' if self.binarize else 'dequantize' if self.dequantize else None

    def __bool__(self):
        return self.binarize or self.hflip or self.dequantize

    def record(self):
        """A plain dict for checkpoints and the run description."""
        return {'binarize': self.binarize, 'hflip': self.hflip, 'dequantize': self.dequantize}

    def describe(self):
        """The run description's suffix: ',binarize' / ',hflip' / ',dequant' for what is on."""
        return ''.join(s for on, s in ((self.binarize, ',binarize'), (self.hflip, ',hflip'), (self.dequantize, ',dequant')) if on)


def binarize_fixed(images, seed, channels_last=False, chunk=4096):
    """A host image set (float (N,C,H,W) with values in [0, 1], uint8 (N,C,H,W), or uint8 (N,H,W,C) with channels_last; a byte means
    v / 255) -> a host uint8 (N,C,H,W) tensor of 0/1: pixel e of image i is 1 where the fixed draw of (aug_seed(seed), i, e) lies below
    its value. One binarization per (seed, image number): independent of how the set is cut into batches, of rank and of world size, so
    a test split binarized once gives the same lines everywhere. Runs the gather kernel over the set, `chunk` images a launch."""
    from . import kernels as K
    host, _ = device_storage(images)
    N = int(host.shape[0])
    chw = (host.shape[3], host.shape[1], host.shape[2]) if channels_last else tuple(host.shape[1:])
    aug = K.feed_aug(aug_seed(seed), 'binarize', fixed=True)
    out = torch.empty((N,) + tuple(chw), dtype=torch.uint8)
    table = host.to(torch.device('cuda', torch.cuda.current_device()))
    for base in range(0, N, int(chunk)):
        n = min(int(chunk), N - base)
        x = K.batch_gather_aug(table, channels_last, torch.empty((n,) + tuple(chw), dtype=torch.float32, device=table.device), aug, base=base)
        out[base:base + n] = x.to(torch.uint8).cpu()
    return out


class DeviceDataset:
    """N images in device memory; the batch of global step s is rows indices(s)[lo:hi] of it, gathered by one HIP launch.

    images: host uint8 (N,C,H,W), uint8 (N,H,W,C) with channels_last=True, or float32 (N,C,H,W) (stored as uint8 when `device_storage`
    says every value survives). batch_size is GLOBAL (this rank gets dist.shard_batch(batch_size, rank, world) of it); None makes a set
    that is only read in storage order (`batches`, a test split). steps_per_epoch = N // batch_size (drop_last, as the reference's train
    loader); epoch e visits epoch_permutation(seed, e, N)[:steps_per_epoch * batch_size].

    On the device: the image table, an int32 index table with the current epoch's order, and `cursor`, an int64[1] holding the number of
    completed steps (of completed micro-batches when a step accumulates over several: `attach(model, micro)`; `step`, `steps_per_epoch`
    and `indices` then count micro-batches, `step_indices` / `step_epoch` optimizer steps). A training step gathers through (index table,
    cursor) and advances the cursor as its last launch; before a step that
    begins a new epoch the host replaces the index table with a copy ordered on the step's stream (`before_step`), so a captured graph
    keeps the addresses it baked in. Host-side queries (`indices`, sizes) need no GPU; device memory is taken on first use.

    augment: a FeedAugment, or None. With one, `gather` and `batch` augment the batch in the gather launch, from noise that is a function
    of (aug_seed(seed), cursor, place in the global batch, element); `batches` and `first_batches`, which read the set in storage order
    for evaluation and recalibration, apply the per-image fixed binarization (`binarize_fixed`) when it binarizes, and nothing else."""

    def __init__(self, images, batch_size, seed, rank=0, world=1, device=None, channels_last=False, augment=None):
        from .dist import shard_batch
        images = torch.as_tensor(images)
        if images.dim() != 4:
            raise ValueError("DeviceDataset needs (N, C, H, W) images (or (N, H, W, C) with channels_last), got shape %s" % (tuple(images.shape),))
        if channels_last and images.dtype != torch.uint8:
            raise ValueError("channels_last storage is for uint8 images")
        self.host, self.kind = device_storage(images)
        self.channels_last = bool(channels_last)
        self.N = int(images.shape[0])
        self.chw = (images.shape[3], images.shape[1], images.shape[2]) if channels_last else tuple(images.shape[1:])
        self.seed, self.rank, self.world, self.device = int(seed), int(rank), int(world), device
        self.augment = augment if augment else None   # (a FeedAugment with nothing on is no augmentation)
        if self.augment is not None and self.augment.dequantize and self.kind != 'uint8':
            raise ValueError("dequantize needs 8-bit data: this image set is kept as float32 (not every value is k/255)")
        self.batch_size = None if batch_size is None else int(batch_size)
        if self.batch_size is not None:
            if self.batch_size < 1 or self.N < self.batch_size:
                raise ValueError("%d images do not fill one batch of %d" % (self.N, self.batch_size))
            self.lo, self.hi = shard_batch(self.batch_size, rank, world)
            self.steps_per_epoch = self.N // self.batch_size
        self.micro = 1                  # batches of batch_size per optimizer step (attach): > 1 when the step accumulates over micro-batches
        self.table = self.index = self.cursor = None
        self._index_epoch = None        # the epoch whose order the device index table holds (or will, once the queued copy has run)
        self._perm = (None, None)
        self._stage, self._stage_done, self._next_stage = [None, None], [None, None], 0

    # ---- host side -------------------------------------------------------------------------------------------------
    @property
    def nbytes(self):
        """Bytes of device memory the image table takes."""
        return self.host.numel() * self.host.element_size()

    @property
    def rows(self):
        """Images per step on this rank."""
        return self.hi - self.lo

    def _order(self, epoch):
        if self._perm[0] != epoch:
            self._perm = (epoch, epoch_permutation(self.seed, epoch, self.N)[:self.steps_per_epoch * self.batch_size])
        return self._perm[1]

    def epoch_of(self, step):
        """0-based epoch of the 1-based global step."""
        return (int(step) - 1) // self.steps_per_epoch

    def indices(self, step):
        """The global batch's image numbers of global step `step` (1-based, as model.global_step counts): a host int64 tensor [batch_size]."""
        if step < 1:
            raise ValueError("steps count from 1")
        pos = (int(step) - 1) % self.steps_per_epoch
        return self._order(self.epoch_of(step))[pos * self.batch_size:(pos + 1) * self.batch_size].clone()

    def step_indices(self, step, micro=None):
        """The image numbers optimizer step `step` (1-based) consumes when every step takes `micro` batches (default: what `attach` was
        told): the `indices` of its micro-batches (step - 1) * micro + 1 ... step * micro, concatenated. An epoch may end inside a step."""
        m = self.micro if micro is None else int(micro)
        if m < 1:
            raise ValueError("a step takes at least one batch, got %d" % m)
        if step < 1:
            raise ValueError("steps count from 1")
        return torch.cat([self.indices((int(step) - 1) * m + j + 1) for j in range(m)])

    def step_epoch(self, step, micro=None):
        """0-based epoch of the FIRST micro-batch of optimizer step `step` (1-based): the epoch --max-epochs compares."""
        m = self.micro if micro is None else int(micro)
        return self.epoch_of((int(step) - 1) * m + 1)

    def cursor_at(self, global_step, micro=None):
        """Where the cursor stands after `global_step` completed optimizer steps of `micro` batches each (what `attach` writes)."""
        m = self.micro if micro is None else int(micro)
        return int(global_step) * m

    # ---- device side -----------------------------------------------------------------------------------------------
    def _dev(self):
        if self.table is None:
            if self.device is None:
                self.device = torch.device('cuda', torch.cuda.current_device())
            self.table = self.host.to(self.device)
        return self.table

    def _load_index(self, epoch):
        """Queue the order of `epoch` into the device index table on the current stream. Two pinned staging buffers alternate, and one is
        rewritten only after the copy that last read it has finished."""
        if self._index_epoch == epoch:
            return
        self._dev()
        n = self.steps_per_epoch * self.batch_size
        if self.index is None:
            self.index = torch.empty(n, dtype=torch.int32, device=self.device)
        k = self._next_stage
        self._next_stage ^= 1
        if self._stage[k] is None:
            self._stage[k] = torch.empty(n, dtype=torch.int32).pin_memory()
            self._stage_done[k] = torch.cuda.Event()
        else:
            self._stage_done[k].synchronize()
        self._stage[k].copy_(self._order(epoch))
        self.index.copy_(self._stage[k], non_blocking=True)
        self._stage_done[k].record(torch.cuda.current_stream(self.device))
        self._index_epoch = epoch

    def attach(self, model, micro=1):
        """Start (or, after a resume, continue) feeding `model`, `micro` batches per optimizer step: the cursor takes
        model.global_step * micro, the batches the completed steps consumed."""
        micro = int(micro)
        if micro < 1:
            raise ValueError("a step takes at least one batch, got %d" % micro)
        self.micro = micro
        self._dev()
        if self.cursor is None:
            self.cursor = torch.empty(1, dtype=torch.int64, device=self.device)
        self.cursor.fill_(self.cursor_at(model.global_step))
        self._load_index(self.cursor_at(model.global_step) // self.steps_per_epoch)
        return self

    def before_step(self, completed_steps):
        """Host part of a fed step, outside any graph: when the step after `completed_steps` begins an epoch, replace the index table."""
        self._load_index(int(completed_steps) // self.steps_per_epoch)

    def new_batch(self, n=None):
        return torch.empty((self.rows if n is None else n,) + tuple(self.chw), dtype=torch.float32, device=self._dev().device)

    def gather(self, out):
        """This rank's batch at the device cursor into `out` (one launch, capturable)."""
        from . import kernels as K
        if self.augment is not None:
            return K.batch_gather_aug(self.table, self.channels_last, out, self._aug(), index=self.index, cursor=self.cursor,
                                      steps_per_epoch=self.steps_per_epoch, global_batch=self.batch_size, lo=self.lo)
        return K.batch_gather(self.table, self.channels_last, out, index=self.index, cursor=self.cursor,
                              steps_per_epoch=self.steps_per_epoch, global_batch=self.batch_size, lo=self.lo)

    def _aug(self, fixed=False):
        """The kernel's description of this set's augmentation; fixed: the per-image binarization alone (storage-order reads)."""
        from . import kernels as K
        if fixed:
            return K.feed_aug(aug_seed(self.seed), 'binarize', fixed=True)
        return K.feed_aug(aug_seed(self.seed), self.augment.mode, hflip=self.augment.hflip)

    def _in_order(self, n, base):
        """n images from image `base` on in storage order (fixed-binarized when the set binarizes)."""
        from . import kernels as K
        if self.augment is not None and self.augment.binarize:
            return K.batch_gather_aug(self._dev(), self.channels_last, self.new_batch(n), self._aug(fixed=True), base=base)
        return K.batch_gather(self._dev(), self.channels_last, self.new_batch(n), base=base)

    def advance(self):
        """The step is complete: cursor += 1 (one launch, capturable; the last of a step, so an abandoned step does not move it)."""
        from . import kernels as K
        K.counter_advance(self.cursor, 1)

    def batch(self, step):
        """This rank's batch of global step `step`, gathered eagerly at a host-given position (the cursor is neither read nor moved)."""
        from . import kernels as K
        self._load_index(self.epoch_of(step))
        pos = (int(step) - 1) % self.steps_per_epoch
        index = self.index[pos * self.batch_size:(pos + 1) * self.batch_size]
        if self.augment is not None:   # the noise of the cursor value that step reads: step - 1 completed micro-batches
            return K.batch_gather_aug(self.table, self.channels_last, self.new_batch(), self._aug(), index=index, steps_per_epoch=1,
                                      global_batch=self.batch_size, lo=self.lo, position=int(step) - 1)
        return K.batch_gather(self.table, self.channels_last, self.new_batch(), index=index,
                              steps_per_epoch=1, global_batch=self.batch_size, lo=self.lo)

    def batches(self, n):
        """Consecutive device batches of n images in storage order, the last one short."""
        for base in range(0, self.N, int(n)):
            yield self._in_order(min(int(n), self.N - base), base)


def first_batches(images, n_batches, batch_size, channels_last=False):
    """The first n_batches * batch_size images of a training set in STORED order, as float32 NCHW batches of batch_size: what BatchNorm
    recalibration (recalibrate.py) runs the averaged weights on. The same on every rank and at every world size; no loader, cursor or
    generator is consumed. images: a host tensor as `image_table` returns it (float NCHW; uint8 NCHW, or uint8 NHWC with channels_last:
    a value means v / 255, the gather's rule), or a DeviceDataset, whose HBM table is read (one gather launch per batch; a set that binarizes gives its fixed binarization). A set shorter
    than n_batches * batch_size stops at its last whole batch; ValueError when it does not fill one. -> a list of batches."""
    n_batches, batch_size = int(n_batches), int(batch_size)
    if n_batches < 1 or batch_size < 1:
        raise ValueError("first_batches needs at least one batch of at least one image, got %d x %d" % (n_batches, batch_size))
    N = images.N if isinstance(images, DeviceDataset) else int(images.shape[0])
    whole = min(n_batches, N // batch_size)
    if whole < 1:
        raise ValueError("%d images do not fill one batch of %d" % (N, batch_size))
    if isinstance(images, DeviceDataset):
        return [images._in_order(batch_size, i * batch_size) for i in range(whole)]
    out = []
    for i in range(whole):
        x = torch.as_tensor(images[i * batch_size:(i + 1) * batch_size])
        if x.dtype == torch.uint8:
            x = (x.permute(0, 3, 1, 2) if channels_last else x).float().div_(255.0)
        out.append(x.float().contiguous())
    return out
