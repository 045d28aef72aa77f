// Sample and reconstruction pictures formed on the device: N float images -> one uint8 RGB grid, laid out as torchvision's make_grid
// (padding 2) followed by save_image, and boilr's img_grid_pad_value (white padding when the pictures have dark edges) as an integer
// count. Both restated from their published behaviour; neither package is a dependency. Rare and small (at most 144 x 3 x 64 x 64
// floats in, 1.9 MB out): one thread per grid pixel, plain loads and stores.
#include "lvae_common.h"

namespace lvae {

constexpr int kGridPad = 2;

// One image set: NCHW contiguous, or NHWC contiguous (what the engine's outputs are; the model returns them as NCHW views).
struct ImgSrc {
  const float* p;
  int nhwc;
};

__device__ __forceinline__ float img_at(ImgSrc s, int n, int c, int y, int x, int C, int H, int W) {
  const size_t i = s.nhwc ? (((size_t)n * H + y) * W + x) * C + c : (((size_t)n * C + c) * H + y) * W + x;
  return s.p[i];
}

// Grid image k: a[k] alone, or a[k/2] for even k and b[k/2] for odd k (input, reconstruction, input, reconstruction, ...).
__device__ __forceinline__ ImgSrc pick(ImgSrc a, ImgSrc b, int k, int* n) {
  if (b.p == nullptr) {
    *n = k;
    return a;
  }
  *n = k >> 1;
  return (k & 1) ? b : a;
}

// save_image's byte: clamp(v * 255 + 0.5, 0, 255) truncated, the product and the sum each rounded to fp32 (the intrinsics are never
// contracted into one fused operation, whatever the compiler flags). NaN fails the first comparison and maps to 0.
__device__ __forceinline__ unsigned char to_byte(float v) {
  const float t = __fadd_rn(__fmul_rn(v, 255.0f), 0.5f);
  return (unsigned char)(int)(t > 0.0f ? (t < 255.0f ? t : 255.0f) : 0.0f);
}

// Border values of one image in a fixed order: rows 0 and H-1 in full, then columns 0 and W-1 of rows 1 .. H-2.
__host__ __device__ inline int border_per_image(int H, int W) { return 2 * W + 2 * (H > 2 ? H - 2 : 0); }

// count[0] += number of border values below `threshold`, count[1] += number of NaN border values. A border value is the mean over the
// channels, in channel order, of the pixel clamped to [0, 1] (a NaN stays a NaN, as in torch.clamp), divided by C in fp32.
// Integer counts: one LDS reduction per workgroup and one integer atomic each, so the result does not depend on the order of arrival.
__global__ __launch_bounds__(256) void border_count_kernel(ImgSrc a, ImgSrc b, int N, int C, int H, int W, float threshold,
                                                           int* __restrict__ count) {
  __shared__ int red[2][256];
  const int per = border_per_image(H, W);
  const long long total = (long long)N * per;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  int below = 0, nan = 0;
  if (i < total) {
    const int k = (int)(i / per), j = (int)(i % per);
    int y, x;
    if (j < W) {
      y = 0, x = j;
    } else if (j < 2 * W) {
      y = H - 1, x = j - W;
    } else {
      y = 1 + ((j - 2 * W) >> 1), x = ((j - 2 * W) & 1) ? W - 1 : 0;
    }
    int n;
    const ImgSrc s = pick(a, b, k, &n);
    float sum = 0.0f;
    for (int c = 0; c < C; ++c) {
      const float v = img_at(s, n, c, y, x, C, H, W);
      sum = __fadd_rn(sum, v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v));
    }
    const float m = __fdiv_rn(sum, (float)C);
    below = m < threshold;
    nan = m != m;
  }
  red[0][threadIdx.x] = below;
  red[1][threadIdx.x] = nan;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x < 2 && red[threadIdx.x][0]) atomicAdd(&count[threadIdx.x], red[threadIdx.x][0]);
}

// grid [Hg][Wg][3] uint8, Hg = (H+2)*ymaps + 2, Wg = (W+2)*xmaps + 2. Image k sits at row (k / xmaps)*(H+2) + 2, column
// (k % xmaps)*(W+2) + 2; everything else, the cells past the last image included, has the padding colour. With `count` the colour is
// chosen here from the border counts (white when the lower median of the n_b border values is below the threshold, i.e. when at least
// (n_b - 1)/2 + 1 of them are, and none is NaN: torch.median returns NaN then, and NaN < t is false); else it is `pad_value`.
__global__ __launch_bounds__(256) void image_grid_kernel(ImgSrc a, ImgSrc b, int N, int C, int H, int W, int xmaps, int Hg, int Wg,
                                                         const int* __restrict__ count, float pad_value,
                                                         unsigned char* __restrict__ grid) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)Hg * Wg) return;
  const int gy = (int)(i / Wg), gx = (int)(i % Wg);
  float pad = pad_value;
  if (count != nullptr) {
    const long long n_b = (long long)N * border_per_image(H, W);
    pad = (count[1] == 0 && (long long)count[0] >= (n_b - 1) / 2 + 1) ? 1.0f : 0.0f;
  }
  unsigned char r, g, bl;
  r = g = bl = to_byte(pad);
  const int yy = gy - kGridPad, xx = gx - kGridPad;
  if (yy >= 0 && xx >= 0) {
    const int cy = yy / (H + kGridPad), iy = yy % (H + kGridPad), cx = xx / (W + kGridPad), ix = xx % (W + kGridPad);
    const int k = cy * xmaps + cx;
    if (iy < H && ix < W && cx < xmaps && k < N) {
      int n;
      const ImgSrc s = pick(a, b, k, &n);
      r = to_byte(img_at(s, n, 0, iy, ix, C, H, W));
      if (C == 3) {
        g = to_byte(img_at(s, n, 1, iy, ix, C, H, W));
        bl = to_byte(img_at(s, n, 2, iy, ix, C, H, W));
      } else {
        g = bl = r;   // a single channel is replicated to three
      }
    }
  }
  unsigned char* o = grid + (size_t)i * 3;
  o[0] = r, o[1] = g, o[2] = bl;
}

static bool grid_args_ok(const float* a, int a_nhwc, const float* b, int b_nhwc, int N, int C, int H, int W) {
  // (the bound keeps every index of a source and of the grid far inside 63 bits and the image count inside int)
  return a && N > 0 && (C == 1 || C == 3) && H > 0 && W > 0 && H <= 16384 && W <= 16384 && N <= (1 << 20) &&
         (a_nhwc == 0 || a_nhwc == 1) && (b_nhwc == 0 || b_nhwc == 1) && (b == nullptr || N % 2 == 0);
}

}  // namespace lvae

using namespace lvae;

extern "C" int lvae_image_border_count_f32(const float* a, int32_t a_nhwc, const float* b, int32_t b_nhwc, int32_t N, int32_t C,
                                           int32_t H, int32_t W, float threshold, int32_t* count, void* stream) {
  LVAE_REQUIRE(grid_args_ok(a, a_nhwc, b, b_nhwc, N, C, H, W) && count, LVAE_EINVAL,
               "lvae_image_border_count_f32: bad args (C must be 1 or 3; with a second source N counts both and is even)");
  hipError_t e = hipMemsetAsync(count, 0, 2 * sizeof(int32_t), (hipStream_t)stream);
  LVAE_REQUIRE(e == hipSuccess, (int)e, "lvae_image_border_count_f32: memset failed: %s", hipGetErrorString(e));
  const long long total = (long long)N * border_per_image(H, W);
  hipLaunchKernelGGL(border_count_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     ImgSrc{a, a_nhwc}, ImgSrc{b, b_nhwc}, N, C, H, W, threshold, count);
  LVAE_LAUNCH_CHECK("image_border_count");
  return 0;
}

extern "C" int lvae_image_grid_u8(const float* a, int32_t a_nhwc, const float* b, int32_t b_nhwc, int32_t N, int32_t C, int32_t H,
                                  int32_t W, int32_t nrow, const int32_t* border_count, float pad_value, uint8_t* grid,
                                  int64_t grid_bytes, void* stream) {
  LVAE_REQUIRE(grid_args_ok(a, a_nhwc, b, b_nhwc, N, C, H, W) && grid && nrow > 0, LVAE_EINVAL,
               "lvae_image_grid_u8: bad args (C must be 1 or 3; with a second source N counts both and is even)");
  const int xmaps = nrow < N ? nrow : N, ymaps = (N + xmaps - 1) / xmaps;
  const long long Hg = (long long)(H + kGridPad) * ymaps + kGridPad, Wg = (long long)(W + kGridPad) * xmaps + kGridPad;
  LVAE_REQUIRE(Hg <= INT32_MAX && Wg <= INT32_MAX && Hg * Wg <= (1LL << 40) && grid_bytes == Hg * Wg * 3, LVAE_EINVAL,
               "lvae_image_grid_u8: the grid buffer has %lld bytes, the layout needs %lld x %lld x 3", (long long)grid_bytes, Hg, Wg);
  hipLaunchKernelGGL(image_grid_kernel, dim3((unsigned)((Hg * Wg + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ImgSrc{a, a_nhwc},
                     ImgSrc{b, b_nhwc}, N, C, H, W, xmaps, (int)Hg, (int)Wg, border_count, pad_value, grid);
  LVAE_LAUNCH_CHECK("image_grid");
  return 0;
}
