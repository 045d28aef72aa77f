// Image quality of reconstructions: per image the mean squared error, the PSNR and the SSIM (Wang, Bovik, Sheikh & Simoncelli 2004: 11 x 11
// Gaussian window, sigma 1.5, "valid" positions) of b judged against a; include/lvae_hip.h states the formulas.
//   tile      one workgroup per (32 x 32 tile of window positions, channel, image): its 42 x 42 pixels of a and b go to LDS (clamped on the
//             way), then every thread walks positions of the tile: window means about the centre pixel, second moments about those means,
//             the ratio with every product and sum rounded on its own. The tile's squared-error sum over the pixels it owns, its SSIM sum
//             and the two counts go to the workspace.
//   finish    one thread per image adds its partials in (channel, tile) order and forms mse, psnr, ssim.
//   fold      one workgroup adds a batch's rows to five double sums in image order.
// Fixed orders and no atomics throughout: an image's floats depend on its pixels, C, H, W, the mask and the flags alone, and a replayed graph
// gives the eager bits. The pixels are read once from HBM (channel-last images: once per channel, from cache); the arithmetic, 2 x 121
// taps twice per position out of LDS, is the cost.
#include <math.h>

#include "lvae_common.h"

namespace lvae {

constexpr int kIqWin = 11;                      // window edge
constexpr int kIqHalo = kIqWin - 1;             // pixels a tile reads beyond its positions, per direction
constexpr int kIqTile = 32;                     // window positions per tile edge
constexpr int kIqIn = kIqTile + kIqHalo;        // pixels per tile edge
constexpr int kIqLd = kIqIn + 1;                // LDS row stride (odd)
constexpr int kIqMaxEdge = 32768;

struct IqPartial {
  float sq_sum, ssim_sum;    // over the counted pixels this tile owns; over its positions with a counted centre
  uint32_t n_pix, n_pos;
};

struct IqArgs {
  const float* a;
  const float* b;
  const uint8_t* mask;
  IqPartial* part;           // [N][C][tiles]
  int64_t a_sn, a_sc, a_sy, a_sx, b_sn, b_sc, b_sy, b_sx;   // strides in floats
  int count_where, C, H, W, tiles_y, tiles_x, clamp;
  float R, C1, C2;
  float w[kIqWin * kIqWin];
};

static __device__ __forceinline__ float iq_clamp(float v, float R, int clamp) {
  if (!clamp) return v;
  return v < 0.f ? 0.f : (v > R ? R : v);   // (both comparisons are false for a NaN: it stays)
}

__global__ __launch_bounds__(256) void image_quality_tile_kernel(IqArgs g) {
  __shared__ float sa[kIqIn * kIqLd];
  __shared__ float sb[kIqIn * kIqLd];
  __shared__ float red_f[2][256];
  __shared__ uint32_t red_n[2][256];
  const int t = threadIdx.x;
  const int tiles = g.tiles_y * g.tiles_x;
  const int64_t id = blockIdx.x;
  const int tile = (int)(id % tiles);
  const int64_t nc = id / tiles;
  const int c = (int)(nc % g.C);
  const int64_t n = nc / g.C;
  const int ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
  const int y0 = ty * kIqTile, x0 = tx * kIqTile;
  const int oh = min(kIqTile, g.H - kIqHalo - y0), ow = min(kIqTile, g.W - kIqHalo - x0);   // positions of this tile: 1 .. 32 each way
  const int ih = oh + kIqHalo, iw = ow + kIqHalo;                                           // its pixels: y0 + ih <= H, x0 + iw <= W

  const float* pa = g.a + n * g.a_sn + c * g.a_sc;
  const float* pb = g.b + n * g.b_sn + c * g.b_sc;
  for (int p = t; p < ih * iw; p += 256) {
    const int y = p / iw, x = p - y * iw;
    sa[y * kIqLd + x] = iq_clamp(pa[(y0 + y) * g.a_sy + (x0 + x) * g.a_sx], g.R, g.clamp);
    sb[y * kIqLd + x] = iq_clamp(pb[(y0 + y) * g.b_sy + (x0 + x) * g.b_sx], g.R, g.clamp);
  }
  __syncthreads();

  const uint8_t* pm = g.mask ? g.mask + n * g.H * g.W : nullptr;
  // squared error: the tile owns the pixels of its positions' rows and columns, the last tile of a direction also the halo
  const int ph = ty == g.tiles_y - 1 ? ih : oh, pw = tx == g.tiles_x - 1 ? iw : ow;
  float sq = 0.f;
  uint32_t n_pix = 0;
  for (int p = t; p < ph * pw; p += 256) {
    const int y = p / pw, x = p - y * pw;
    if (pm && ((pm[(int64_t)(y0 + y) * g.W + x0 + x] != 0) != (g.count_where != 0))) continue;
    const float d = sa[y * kIqLd + x] - sb[y * kIqLd + x];
    sq += d * d;
    ++n_pix;
  }

  float ss = 0.f;
  uint32_t n_pos = 0;
  for (int p = t; p < oh * ow; p += 256) {
    const int y = p / ow, x = p - y * ow;
    if (pm && ((pm[(int64_t)(y0 + y + kIqWin / 2) * g.W + x0 + x + kIqWin / 2] != 0) != (g.count_where != 0))) continue;
    const float* wa = sa + y * kIqLd + x;
    const float* wb = sb + y * kIqLd + x;
    const float ca = wa[(kIqWin / 2) * kIqLd + kIqWin / 2], cb = wb[(kIqWin / 2) * kIqLd + kIqWin / 2];
    float ma = 0.f, mb = 0.f;
#pragma unroll 1   // (a row's 11 weights at a time in scalar registers: all 121 do not fit)
    for (int i = 0; i < kIqWin; ++i)
#pragma unroll
      for (int j = 0; j < kIqWin; ++j) {
        const float w = g.w[i * kIqWin + j];
        ma = __fmaf_rn(w, wa[i * kIqLd + j] - ca, ma);
        mb = __fmaf_rn(w, wb[i * kIqLd + j] - cb, mb);
      }
    const float mu_a = ca + ma, mu_b = cb + mb;
    float vaa = 0.f, vab = 0.f, vbb = 0.f;
#pragma unroll 1
    for (int i = 0; i < kIqWin; ++i)
#pragma unroll
      for (int j = 0; j < kIqWin; ++j) {
        const float w = g.w[i * kIqWin + j];
        const float da = wa[i * kIqLd + j] - mu_a, db = wb[i * kIqLd + j] - mu_b;
        const float wda = __fmul_rn(w, da), wdb = __fmul_rn(w, db);
        vaa = __fmaf_rn(wda, da, vaa);
        vab = __fmaf_rn(wda, db, vab);
        vbb = __fmaf_rn(wdb, db, vbb);
      }
    // every product and sum on its own: with a == b numerator and denominator are the same float
    const float num = __fmul_rn(__fadd_rn(__fmul_rn(2.f, __fmul_rn(mu_a, mu_b)), g.C1), __fadd_rn(__fmul_rn(2.f, vab), g.C2));
    const float den = __fmul_rn(__fadd_rn(__fadd_rn(__fmul_rn(mu_a, mu_a), __fmul_rn(mu_b, mu_b)), g.C1), __fadd_rn(__fadd_rn(vaa, vbb), g.C2));
    ss = __fadd_rn(ss, __fdiv_rn(num, den));
    ++n_pos;
  }

  red_f[0][t] = sq;
  red_f[1][t] = ss;
  red_n[0][t] = n_pix;
  red_n[1][t] = n_pos;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      red_f[0][t] += red_f[0][t + s];
      red_f[1][t] += red_f[1][t + s];
      red_n[0][t] += red_n[0][t + s];
      red_n[1][t] += red_n[1][t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    IqPartial r;
    r.sq_sum = red_f[0][0];
    r.ssim_sum = red_f[1][0];
    r.n_pix = red_n[0][0];
    r.n_pos = red_n[1][0];
    g.part[id] = r;
  }
}

// out[n] = (mse, psnr_db, ssim) from the image's C * tiles partials, added in (channel, tile) order.
__global__ __launch_bounds__(64) void image_quality_finish_kernel(const IqPartial* __restrict__ part, int N, int per_image, float R,
                                                                   float* __restrict__ out) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= N) return;
  const IqPartial* p = part + (int64_t)n * per_image;
  float sq = 0.f, ss = 0.f;
  uint64_t n_pix = 0, n_pos = 0;
  for (int k = 0; k < per_image; ++k) {
    const IqPartial r = p[k];
    sq += r.sq_sum;
    ss += r.ssim_sum;
    n_pix += r.n_pix;
    n_pos += r.n_pos;
  }
  const float mse = __fdiv_rn(sq, (float)n_pix);   // nothing counted: 0 / 0 = NaN
  float psnr;
  if (mse == 0.f)
    psnr = INFINITY;
  else
    psnr = (float)(10.0 * log10((double)R * (double)R / (double)mse));   // (a NaN mse gives a NaN)
  out[3 * (int64_t)n + 0] = mse;
  out[3 * (int64_t)n + 1] = psnr;
  out[3 * (int64_t)n + 2] = __fdiv_rn(ss, (float)n_pos);
}

// sums[0..4] = images, sum mse, sum psnr (those that are not +inf), images with mse == 0, sum ssim: thread k owns sums[k] and adds the rows
// in image order, starting from what sums[k] holds, so the total is one sequential double sum over every image ever folded.
__global__ __launch_bounds__(256) void image_quality_fold_kernel(const float* __restrict__ per_image, int N, double* __restrict__ sums) {
  __shared__ float rows[256 * 3];
  const int t = threadIdx.x;
  double acc = t < 5 ? sums[t] : 0.0;
  for (int base = 0; base < N; base += 256) {
    const int cnt = N - base < 256 ? N - base : 256;
    for (int i = t; i < cnt * 3; i += 256) rows[i] = per_image[(int64_t)base * 3 + i];
    __syncthreads();
    if (t < 5) {
      for (int k = 0; k < cnt; ++k) {
        const float mse = rows[3 * k], psnr = rows[3 * k + 1], ssim = rows[3 * k + 2];
        if (t == 0) acc += 1.0;
        if (t == 1) acc += (double)mse;
        if (t == 2 && !(psnr == INFINITY)) acc += (double)psnr;
        if (t == 3 && mse == 0.f) acc += 1.0;
        if (t == 4) acc += (double)ssim;
      }
    }
    __syncthreads();
  }
  if (t < 5) sums[t] = acc;
}

// The 121 weights: exp(-(dy^2 + dx^2) / (2 sigma^2)) as the outer product of the normalised one-dimensional window, in double, rounded once.
static const float* iq_weights() {
  static float w[kIqWin * kIqWin];
  static const bool ready = [] {
    double g1[kIqWin], sum = 0.0;
    for (int k = 0; k < kIqWin; ++k) {
      const double d = (double)(k - kIqWin / 2);
      g1[k] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
      sum += g1[k];
    }
    for (int k = 0; k < kIqWin; ++k) g1[k] /= sum;
    for (int i = 0; i < kIqWin; ++i)
      for (int j = 0; j < kIqWin; ++j) w[i * kIqWin + j] = (float)(g1[i] * g1[j]);
    return true;
  }();
  (void)ready;
  return w;
}

static inline int64_t iq_tiles(int32_t edge) { return ((int64_t)edge - kIqHalo + kIqTile - 1) / kIqTile; }

static inline bool iq_sizes_ok(int32_t N, int32_t C, int32_t H, int32_t W) {
  if (N <= 0 || C < 1 || C > 4 || H < kIqWin || W < kIqWin || H > kIqMaxEdge || W > kIqMaxEdge) return false;
  return (int64_t)N * C * iq_tiles(H) * iq_tiles(W) <= (int64_t)INT32_MAX;   // one workgroup each
}

}  // namespace lvae

using namespace lvae;

extern "C" size_t lvae_image_quality_workspace(int32_t N, int32_t C, int32_t H, int32_t W) {
  if (!iq_sizes_ok(N, C, H, W)) return 0;
  return (size_t)((int64_t)N * C * iq_tiles(H) * iq_tiles(W)) * sizeof(IqPartial);
}

extern "C" int lvae_image_quality_f32(const float* a, int32_t a_nhwc, int64_t a_ld, const float* b, int32_t b_nhwc, int64_t b_ld,
                                      const uint8_t* mask, int32_t count_where, int32_t N, int32_t C, int32_t H, int32_t W, float data_range,
                                      int32_t clamp, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  LVAE_REQUIRE(a && b && out, LVAE_EINVAL, "lvae_image_quality_f32: null a, b or out");
  LVAE_REQUIRE(N > 0 && C >= 1 && C <= 4, LVAE_EINVAL, "lvae_image_quality_f32: N %d must be positive, C %d from 1 to 4", (int)N, (int)C);
  LVAE_REQUIRE(H >= kIqWin && W >= kIqWin && H <= kIqMaxEdge && W <= kIqMaxEdge, LVAE_EINVAL,
               "lvae_image_quality_f32: H %d, W %d must be from %d to %d", (int)H, (int)W, kIqWin, kIqMaxEdge);
  LVAE_REQUIRE(iq_sizes_ok(N, C, H, W), LVAE_EINVAL, "lvae_image_quality_f32: N %d x C %d images of %d x %d are more tiles than one launch holds",
               (int)N, (int)C, (int)H, (int)W);
  if (a_nhwc && a_ld == 0) a_ld = C;
  if (b_nhwc && b_ld == 0) b_ld = C;
  LVAE_REQUIRE((!a_nhwc || a_ld >= C) && (!b_nhwc || b_ld >= C), LVAE_EINVAL, "lvae_image_quality_f32: pixel stride %lld / %lld below C = %d",
               (long long)a_ld, (long long)b_ld, (int)C);
  LVAE_REQUIRE(isfinite(data_range) && data_range > 0.f, LVAE_EINVAL, "lvae_image_quality_f32: data_range %g must be finite and positive",
               (double)data_range);
  const size_t need = lvae_image_quality_workspace(N, C, H, W);
  LVAE_REQUIRE(workspace && workspace_bytes >= need, LVAE_EWORKSPACE,
               "lvae_image_quality_f32: workspace of %zu bytes, lvae_image_quality_workspace asks for %zu", workspace ? workspace_bytes : (size_t)0,
               need);
  LVAE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, LVAE_EALIGN, "lvae_image_quality_f32: workspace not 8-byte aligned");
  IqArgs g;
  g.a = a;
  g.b = b;
  g.mask = mask;
  g.part = reinterpret_cast<IqPartial*>(workspace);
  const int64_t HW = (int64_t)H * W;
  if (a_nhwc) { g.a_sn = HW * a_ld; g.a_sc = 1; g.a_sy = (int64_t)W * a_ld; g.a_sx = a_ld; }
  else { g.a_sn = HW * C; g.a_sc = HW; g.a_sy = W; g.a_sx = 1; }
  if (b_nhwc) { g.b_sn = HW * b_ld; g.b_sc = 1; g.b_sy = (int64_t)W * b_ld; g.b_sx = b_ld; }
  else { g.b_sn = HW * C; g.b_sc = HW; g.b_sy = W; g.b_sx = 1; }
  g.count_where = count_where ? 1 : 0;
  g.C = C;
  g.H = H;
  g.W = W;
  g.tiles_y = (int)iq_tiles(H);
  g.tiles_x = (int)iq_tiles(W);
  g.clamp = clamp ? 1 : 0;
  g.R = data_range;
  g.C1 = (0.01f * data_range) * (0.01f * data_range);
  g.C2 = (0.03f * data_range) * (0.03f * data_range);
  const float* w = iq_weights();
  for (int k = 0; k < kIqWin * kIqWin; ++k) g.w[k] = w[k];
  const int per_image = C * g.tiles_y * g.tiles_x;
  hipLaunchKernelGGL(image_quality_tile_kernel, dim3((unsigned)((int64_t)N * per_image)), dim3(256), 0, (hipStream_t)stream, g);
  LVAE_LAUNCH_CHECK("image_quality_tile");
  hipLaunchKernelGGL(image_quality_finish_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, g.part, (int)N, per_image,
                     data_range, out);
  LVAE_LAUNCH_CHECK("image_quality_finish");
  return 0;
}

extern "C" int lvae_image_quality_fold_f64(const float* per_image, int32_t N, double* sums, void* stream) {
  LVAE_REQUIRE(per_image && sums, LVAE_EINVAL, "lvae_image_quality_fold_f64: null pointer");
  LVAE_REQUIRE(N > 0, LVAE_EINVAL, "lvae_image_quality_fold_f64: N = %d must be positive", (int)N);
  LVAE_REQUIRE((reinterpret_cast<uintptr_t>(sums) & 7) == 0, LVAE_EALIGN, "lvae_image_quality_fold_f64: sums not 8-byte aligned");
  hipLaunchKernelGGL(image_quality_fold_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, per_image, (int)N, sums);
  LVAE_LAUNCH_CHECK("image_quality_fold");
  return 0;
}
