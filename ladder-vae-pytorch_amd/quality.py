"""Image quality of what the model makes of an image: mean squared error, PSNR and SSIM, measured on the device.

`image_quality(a, b)` judges the images b against the references a and returns one value per image (kernels.image_quality: the SSIM of
Wang, Bovik, Sheikh & Simoncelli 2004, 11 x 11 Gaussian window of sigma 1.5 at the valid positions, with second moments centred on the
window's own means; include/lvae_hip.h states every formula). Images are measured clamped to [0, data_range] by default, as pictures are
written.

`ImageQuality` keeps the sums of a pass in one float64 buffer on the device, as latent.LatentStats keeps its sums:

    [ images | sum mse | sum of the PSNRs that are finite | images with mse == 0 | sum ssim ]

`fold(a, b)` costs one quality launch pair and one fold launch (capturable: evaluate.test_pass replays them with the first sample of a
batch), `take()` one all-reduce of the five doubles and one device-to-host copy. The fold adds images in order, so a pass gives the same
bits launched eagerly or replayed; sums of shards add up to the sums of the whole set up to double rounding.

PSNR is reported twice: 'quality/psnr' is the mean of the per-image PSNRs (over the images whose PSNR is finite: an exact reconstruction
has none, and 'quality/exact' counts those), 'quality/psnr_of_mean_mse' is the PSNR of the mean squared error over all images, the
figure most papers quote. For a head without a mean (the logistic mixture) the picture judged is a sample, so its PSNR carries the
sampling noise: it measures the pictures the model writes, not a point estimate.
"""
import math

import torch

from . import kernels as K

COUNT_WHERE = {'observed': 1, 'missing': 0}   # which side of a mask of OBSERVED pixels is measured


def _count_where(count):
    if count not in COUNT_WHERE:
        raise ValueError("count must be 'observed' or 'missing', got %r" % (count,))
    return COUNT_WHERE[count]


def _rows(a, b, mask, count, data_range, clamp, channel_last, out=None):
    if not (torch.is_tensor(a) and torch.is_tensor(b)) or tuple(a.shape) != tuple(b.shape) or a.dim() != 4:
        raise ValueError("image_quality: need two 4-d image sets of one shape, got %s and %s"
                         % (tuple(getattr(a, 'shape', ())), tuple(getattr(b, 'shape', ()))))
    N, H, W = (a.shape[0], a.shape[1], a.shape[2]) if channel_last else (a.shape[0], a.shape[2], a.shape[3])
    if H < K.IQ_WINDOW or W < K.IQ_WINDOW:
        raise ValueError("image_quality: images of %d x %d are smaller than the %d x %d window" % (H, W, K.IQ_WINDOW, K.IQ_WINDOW))
    count_where = _count_where(count)
    if not (a.is_cuda and b.is_cuda):
        raise K._C.LvaeHipError("image_quality needs GPU tensors (no CPU fallback exists); got %s and %s" % (a.device, b.device))
    if mask is not None:
        mask = K.pixel_mask(mask, N, H, W, a.device)
    return K.image_quality(a, b, mask, count_where, data_range, clamp, channel_last, out)


@torch.no_grad()
def image_quality(a, b, mask=None, count='observed', data_range=1.0, clamp=True, channel_last=False):
    """{'mse', 'psnr', 'ssim'}: (N,) float32 device tensors, b judged against a. a, b: float32 device image sets of one shape, (N, C, H, W)
    or with channel_last (N, H, W, C), each stored NCHW or channel-last (also a view of the first C channels of a wider channel-last
    buffer: nothing is copied). mask: bool or uint8, (N, H, W) or (N, 1, H, W), True = observed; count='observed' measures the observed
    pixels (and the SSIM positions whose centre is observed), count='missing' the others: what an inpainting filled in. ValueError for
    mismatched shapes or images below 11 x 11, LvaeHipError for CPU tensors."""
    rows = _rows(a, b, mask, count, data_range, clamp, channel_last)
    return {'mse': rows[:, 0], 'psnr': rows[:, 1], 'ssim': rows[:, 2]}


class ImageQuality:
    """Owns the device sums of one pass's image quality."""

    def __init__(self, device, data_range=1.0, clamp=True):
        self.data_range, self.clamp = float(data_range), bool(clamp)
        self.buf = torch.zeros(K.IQ_SUMS, dtype=torch.float64, device=device)
        self._rows = {}        # batch size -> the (N, 3) buffer its quality launch writes: a captured fold keeps its address
        self.last_ptrs = None  # (a.data_ptr(), b.data_ptr()) of the last fold: what the kernel was handed

    def reset(self):
        self.buf.zero_()

    @torch.no_grad()
    def fold(self, a, b, mask=None, count='observed', channel_last=False):
        """Adds the images b judged against a (as in image_quality) to the sums: the quality launches and one fold launch."""
        n = int(a.shape[0])
        rows = self._rows.get(n)
        if rows is None or rows.device != a.device:
            rows = self._rows[n] = torch.empty((n, 3), dtype=torch.float32, device=a.device)
        _rows(a, b, mask, count, self.data_range, self.clamp, channel_last, rows)
        self.last_ptrs = (a.data_ptr(), b.data_ptr())
        K.image_quality_fold(rows, self.buf)

    def merge(self, other):
        """Adds another object's sums (a shard folded separately on this device): what the all-reduce of take() does between ranks."""
        self.buf += other.buf

    def take(self, process_group=None):
        """The means of everything folded since the last take(), over all ranks; the sums start again. A collective: every rank calls it.
        -> {'quality/mse', 'quality/psnr' (mean over the images with a finite PSNR; NaN when there is none), 'quality/ssim',
        'quality/psnr_of_mean_mse', 'quality/exact' (images with mse == 0), 'n_images'}."""
        from .evaluate import reduce_eval_sums
        n, mse, psnr, exact, ssim = reduce_eval_sums(self.buf, process_group).cpu().tolist()
        self.reset()
        if n <= 0:
            raise ValueError("ImageQuality.take(): no image was folded since the last take()")
        mean_mse = mse / n
        if mean_mse == 0:
            of_mean = math.inf
        elif 0 < mean_mse < math.inf:
            of_mean = 10.0 * math.log10(self.data_range * self.data_range / mean_mse)
        else:   # a NaN image shows here too
            of_mean = -math.inf if mean_mse == math.inf else math.nan
        return {'quality/mse': mean_mse, 'quality/psnr': psnr / (n - exact) if n > exact else math.nan, 'quality/ssim': ssim / n,
                'quality/psnr_of_mean_mse': of_mean, 'quality/exact': int(exact), 'n_images': int(n)}


def quality_line_suffix(res):
    """What --image-quality appends to a test line. `res` holds the 'quality/*' values of ImageQuality.take()."""
    return '   PSNR: %.2f dB   SSIM: %.4f' % (res['quality/psnr'], res['quality/ssim'])
