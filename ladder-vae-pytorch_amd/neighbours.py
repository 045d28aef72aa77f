"""Nearest training images of samples, on the device: is a sample new, or a training image given back?

  * `NeighbourIndex(table)` wraps a table that already sits in HBM (uint8 or float32 images, or (N, D) feature rows; `from_dataset` shares
    the image table of a data.DeviceDataset without a copy) and `query` returns each query's k nearest rows by squared L2 distance through
    one exact search kernel (kernels.nn_l2, csrc/neighbours.hip): no float32 copy of a uint8 table, and the distance formed as
    sum (q - t)^2, so a near-duplicate keeps its distance and a duplicate gives exactly 0;
  * `latent_features(model, images, k)` gives the rows for a search in the latents of the top k layers (the posterior means of
    LadderVAE.encode): neighbours there show what each level of the ladder stores;
  * `closeness_summary(d_samples, d_heldout)` is the number pair beside the figure: how close samples lie to the training set against how
    close held-out images lie to it (host code).
"""
import numpy as np
import torch

from . import kernels as K
from .passes import eval_mode

QUERY_ROWS = 4096   # rows per search call of a long query set (the results do not depend on the cut)


class NeighbourIndex:
    """A search table in device memory. table: (N, C, H, W) uint8 or float32 images, (N, H, W, C) uint8 with channels_last, or (N, D)
    float32 / uint8 feature rows; contiguous, on the GPU, never copied or converted."""

    def __init__(self, table, channels_last=False):
        if not isinstance(table, torch.Tensor) or not table.is_cuda:
            raise K._C.LvaeHipError("NeighbourIndex needs a device tensor (no CPU fallback exists)")
        if table.dtype not in (torch.uint8, torch.float32) or table.dim() not in (2, 4) or not table.is_contiguous() or table.shape[0] < 1:
            raise ValueError("the table must be a contiguous uint8 or float32 tensor (N, C, H, W), (N, H, W, C) or (N, D), got %s %s"
                             % (table.dtype, tuple(table.shape)))
        if channels_last and (table.dim() != 4 or table.dtype != torch.uint8):
            raise ValueError("channels_last is the layout of uint8 image tables (N, H, W, C), as in data.DeviceDataset")
        self.table, self.channels_last = table, bool(channels_last)
        self.N = int(table.shape[0])
        self.flat = table.view(self.N, -1)
        self.D = int(self.flat.shape[1])
        if table.dim() == 4:
            self.chw = (table.shape[3], table.shape[1], table.shape[2]) if channels_last else tuple(table.shape[1:])
            self.chw = tuple(int(s) for s in self.chw)
        else:
            self.chw = None

    @classmethod
    def from_dataset(cls, ds):
        """The image table of a data.DeviceDataset, shared (no copy), in the layout the data set keeps it in."""
        return cls(ds._dev(), ds.channels_last)

    def _query_rows(self, x):
        """x as float32 (Q, D) rows in the table's element order: the queries are permuted, never the table."""
        if x.dim() == 2:
            rows = x
        elif x.dim() == 4 and self.chw is not None and tuple(int(s) for s in x.shape[1:]) == self.chw:
            rows = (x.permute(0, 2, 3, 1) if self.channels_last else x).reshape(x.shape[0], -1)
        else:
            raise ValueError("queries must be (Q, %d) rows%s, got %s" % (self.D, '' if self.chw is None else ' or (Q, %d, %d, %d) images' % self.chw,
                                                                            tuple(x.shape)))
        if rows.shape[1] != self.D or rows.shape[0] < 1:
            raise ValueError("queries must have %d elements per row and at least one row, got %s" % (self.D, tuple(x.shape)))
        return rows.to(torch.float32).contiguous()

    def query(self, x, k=1, exclude=None, max_rows=QUERY_ROWS):
        """-> (index int64 (Q, k), dist float32 (Q, k)) of the k nearest table rows of every query, nearest first, ties to the lower row;
        (-1, +inf) where fewer than k rows are eligible. x: device NCHW images or (Q, D) rows (for a channels_last table rows are in its
        HWC order). exclude: None, or (Q,) integers: the table row each query skips (-1: none), for queries that are table rows
        themselves. Long query sets are searched max_rows at a time; the result does not depend on the cut."""
        rows = self._query_rows(x)
        Q = int(rows.shape[0])
        if exclude is not None:
            exclude = torch.as_tensor(exclude, device=rows.device).to(torch.int64)
            if tuple(exclude.shape) != (Q,):
                raise ValueError("exclude must have shape (%d,), got %s" % (Q, tuple(exclude.shape)))
            exclude = exclude.clamp(-1, 2 ** 31 - 1).to(torch.int32)   # (rows past the int32 range do not exist: such an entry skips nothing)
        step = max(1, int(max_rows))
        idx, dist = [], []
        for lo in range(0, Q, step):
            i, d = K.nn_l2(rows[lo:lo + step], self.flat, k, None if exclude is None else exclude[lo:lo + step].contiguous())
            idx.append(i)
            dist.append(d)
        return torch.cat(idx).to(torch.int64), torch.cat(dist)

    def rows(self, index):
        """The table rows `index` (any shape, int64; -1 gives zeros) as float32 in the layout queries are given in: (..., C, H, W) for
        an image table, (..., D) for a feature table; uint8 values as v / 255."""
        index = torch.as_tensor(index, device=self.table.device).to(torch.int64)
        flat = index.reshape(-1)
        if self.table.dtype == torch.uint8:
            # the gather of the training feed: the same v / 255 (an IEEE division, which torch's division by a scalar on the device is not)
            # and the same HWC -> CHW order; a row outside the table comes out as NaN and is zeroed below
            table = self.table if self.table.dim() == 4 else self.table.view(self.N, 1, 1, self.D)
            shape = self.chw if self.chw is not None else (1, 1, self.D)
            got = torch.empty((flat.numel(),) + shape, dtype=torch.float32, device=self.table.device)
            if flat.numel():
                K.batch_gather(table, self.channels_last, got, index=flat.clamp(-1, self.N).to(torch.int32), steps_per_epoch=1,
                               global_batch=flat.numel())
            got = got.view((flat.numel(),) + (self.chw if self.chw is not None else (self.D,)))
        else:
            got = self.table[flat.clamp(0, self.N - 1)]
        got[(flat < 0) | (flat >= self.N)] = 0.0
        return got.view(tuple(index.shape) + tuple(got.shape[1:]))


@torch.no_grad()
def latent_features(model, images, n_top_layers=None, batch_size=256):
    """(N, Dz) float32 on the device: per image the posterior means of the top k = n_top_layers layers (None: all), each flattened (C, H, W)
    and concatenated top layer first. model.encode in eval mode, batch_size images at a time; images: NCHW, host or device."""
    dev = next(model.parameters()).device
    with eval_mode(model):
        out = []
        for lo in range(0, int(images.shape[0]), int(batch_size)):
            x = images[lo:lo + int(batch_size)].to(dev).contiguous().float()
            z = model.encode(x, n_top_layers)
            out.append(torch.cat([t.reshape(t.shape[0], -1) for t in reversed(z) if t is not None], 1))
        return torch.cat(out).contiguous()


def closeness_summary(d_samples, d_heldout):
    """Nearest-neighbour distances of samples against those of held-out images (arrays or tensors, any shape; host code). Returns a dict:
    'samples' and 'heldout' -> {'median', 'q10', 'q90'} (numpy's linear quantiles) and 'below_heldout_q01': the share of samples whose
    distance lies below the 1 % quantile of the held-out distances. Samples that sit closer to the training set than held-out images ever
    do are training images given back."""
    def arr(d):
        d = d.detach().cpu().numpy() if isinstance(d, torch.Tensor) else np.asarray(d)
        d = d.astype(np.float64).reshape(-1)
        if d.size == 0:
            raise ValueError("closeness_summary needs at least one distance per set")
        return d

    ds, dh = arr(d_samples), arr(d_heldout)

    def quantiles(d):
        q10, med, q90 = np.quantile(d, [0.1, 0.5, 0.9])
        return {'median': float(med), 'q10': float(q10), 'q90': float(q90)}

    return {'samples': quantiles(ds), 'heldout': quantiles(dh), 'below_heldout_q01': float(np.mean(ds < np.quantile(dh, 0.01)))}


def closeness_line(space, s):
    return ('nn %s: nearest squared distance, samples median %.5g (10%% %.5g, 90%% %.5g) | held-out median %.5g (10%% %.5g, 90%% %.5g) | '
            'samples below the held-out 1%% quantile: %.3f'
            % (space, s['samples']['median'], s['samples']['q10'], s['samples']['q90'], s['heldout']['median'], s['heldout']['q10'],
               s['heldout']['q90'], s['below_heldout_q01']))
