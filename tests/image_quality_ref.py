"""The float64 statement of what lvae_image_quality_f32 computes (include/lvae_hip.h): mean squared error, PSNR and the SSIM of Wang, Bovik,
Sheikh & Simoncelli (2004) with an 11 x 11 Gaussian window of sigma 1.5 at the "valid" positions, in numpy. `dtype` switches the arithmetic:
float64 is the yardstick (r64), float32 (r32) runs the same centred formulas in the kernel's precision and gives the element-wise rule of
docs/ELEMENTWISE_PARITY.md its error scale. Not a test module: the CPU and GPU tests import it."""
import numpy as np

WIN, SIGMA = 11, 1.5


def window(dtype=np.float64):
    """The 121 weights: the outer product of the normalised one-dimensional Gaussian, formed in double, rounded once to `dtype`."""
    d = np.arange(WIN, dtype=np.float64) - WIN // 2
    g = np.exp(-(d * d) / (2.0 * SIGMA * SIGMA))
    g /= g.sum()
    return np.outer(g, g).astype(dtype)


def _windows(x):
    """(..., H - 10, W - 10, 11, 11) view of the windows of x (..., H, W)."""
    return np.lib.stride_tricks.sliding_window_view(x, (WIN, WIN), axis=(-2, -1))


def clamp(x, data_range):
    """x < 0 -> 0, x > R -> R; a NaN stays."""
    x = np.array(x, copy=True)
    x[x < 0] = 0
    x[x > data_range] = data_range
    return x


def moments(a, b, dtype=np.float64):
    """(mu_a, mu_b, var_a, var_b, cov) at every valid position of a, b (..., H, W): the mean about the window's centre pixel,
    mu = x_c + sum w (x - x_c), and the second moments about those means, sum w (x - mu)^2: never E[x^2] - mu^2."""
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
    w = window(dtype)
    wa, wb = _windows(a), _windows(b)
    ca, cb = wa[..., WIN // 2, WIN // 2], wb[..., WIN // 2, WIN // 2]
    mu_a = ca + (w * (wa - ca[..., None, None])).sum((-2, -1), dtype=dtype)
    mu_b = cb + (w * (wb - cb[..., None, None])).sum((-2, -1), dtype=dtype)
    da, db = wa - mu_a[..., None, None], wb - mu_b[..., None, None]
    var_a = (w * da * da).sum((-2, -1), dtype=dtype)
    var_b = (w * db * db).sum((-2, -1), dtype=dtype)
    cov = (w * da * db).sum((-2, -1), dtype=dtype)
    return mu_a, mu_b, var_a, var_b, cov


def ssim_map(a, b, data_range=1.0, dtype=np.float64):
    """SSIM at every valid position of a, b (..., H, W) -> (..., H - 10, W - 10)."""
    mu_a, mu_b, var_a, var_b, cov = moments(a, b, dtype)
    R = dtype(data_range)
    C1, C2 = (dtype(0.01) * R) ** 2, (dtype(0.03) * R) ** 2
    two = dtype(2)
    return ((two * (mu_a * mu_b) + C1) * (two * cov + C2)) / (((mu_a * mu_a + mu_b * mu_b) + C1) * ((var_a + var_b) + C2))


def psnr_db(mse, data_range=1.0, dtype=np.float64):
    """10 log10(R^2 / mse); +inf for mse == 0, NaN for a NaN."""
    mse = np.asarray(mse, dtype=dtype)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(mse == 0, dtype(np.inf), dtype(10) * np.log10(dtype(data_range) * dtype(data_range) / mse)).astype(dtype)


def image_quality(a, b, mask=None, count_where=1, data_range=1.0, clamp_images=True, dtype=np.float64):
    """(N, 3) = mse, psnr_db, ssim of the NCHW image sets a (the reference) and b. mask: None or (N, H, W), a pixel is counted when
    (mask != 0) == (count_where != 0): mse runs over the counted pixels and all channels, ssim over channels and the positions whose centre
    pixel is counted (the windows read every pixel they cover). Nothing counted: NaN."""
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
    N, C, H, W = a.shape
    if clamp_images:
        a, b = clamp(a, data_range), clamp(b, data_range)
    counted = np.ones((N, H, W), dtype=bool) if mask is None else ((np.asarray(mask) != 0) == (count_where != 0))
    centre = counted[:, WIN // 2:H - WIN // 2, WIN // 2:W - WIN // 2]
    sm = ssim_map(a, b, data_range, dtype)
    out = np.empty((N, 3), dtype=dtype)
    with np.errstate(divide='ignore', invalid='ignore'):
        for n in range(N):
            sq = ((a[n] - b[n]) ** 2)[:, counted[n]]
            out[n, 0] = sq.sum(dtype=dtype) / dtype(sq.size) if sq.size else np.nan
            sel = sm[n][:, centre[n]]
            out[n, 2] = sel.sum(dtype=dtype) / dtype(sel.size) if sel.size else np.nan
    out[:, 1] = psnr_db(out[:, 0], data_range, dtype)
    return out


def parity_bound(r32, r64):
    """The element-wise rule of docs/ELEMENTWISE_PARITY.md: |kernel - r64| <= 2 max|r32 - r64| + 1e-5 |r64| + 1e-6, the maximum taken over
    the finite entries of the column the element belongs to."""
    r32, r64 = np.asarray(r32, dtype=np.float64), np.asarray(r64, dtype=np.float64)
    fin = np.isfinite(r32) & np.isfinite(r64)
    scale = np.array([np.abs(r32[:, k] - r64[:, k])[fin[:, k]].max(initial=0.0) for k in range(r64.shape[1])])
    return 2.0 * scale[None, :] + 1e-5 * np.abs(r64) + 1e-6
