// Latent usage of a test pass: per latent unit (one (pixel, channel) position of one stochastic layer) the sums over images of the posterior
// mean, of its square and of the analytical KL(q || p), from which the active-unit counts of the LVAE and IWAE papers follow.
//   fold      one batch's (mu | logvar) tensors of p and q -> double partial sums per batch slice (grid: unit blocks x batch slices)
//   reduce    the slices in slice order, added to the caller's running sums: fixed order, no atomics, so a replayed graph gives the eager bits
//   finalize  sums / n -> per-unit KL, mean and population variance of mu_q, and the layer's counts, by ONE workgroup in a fixed order
// The KL of an element is normal_kl() in fp32, the function lvae_normal_stochastic_fwd_f32 sums into kl_spatial; every sum is carried in double.
// HBM-bound: q is read once, p once unless it is the broadcast top prior.
#include "lvae_common.h"

namespace lvae {

constexpr int kLatentMinImagesPerSlice = 16;   // fewer images per slice: the double partials cost more traffic than the fp32 inputs
constexpr int kLatentTargetBlocks = 1024;      // 4 workgroups of 256 per CU

// Batch slicing of one fold: a function of (N, HW, Z) alone (the workspace query has no pointers to look at), the same for both kernel forms.
static inline int latent_images_per_slice(int N, int64_t U) {
  const int64_t unit_blocks = (U + 1023) / 1024;   // workgroups over the units at 4 channels per thread
  const int64_t max_slices = kLatentTargetBlocks / unit_blocks > 1 ? kLatentTargetBlocks / unit_blocks : 1;
  const int64_t per = ((int64_t)N + max_slices - 1) / max_slices;
  return (int)(per > kLatentMinImagesPerSlice ? per : kLatentMinImagesPerSlice);
}

static inline int latent_slices(int N, int64_t U) {
  const int per = latent_images_per_slice(N, U);
  return (N + per - 1) / per;
}

struct LatentFoldArgs {
  const float* p;
  const float* q;
  double* part;   // [slices][3][U]
  int p_bcast, N, HW, Z, per_slice;
};

template <int V> struct LatentVec;
template <> struct LatentVec<1> { typedef float type; };
template <> struct LatentVec<4> { typedef f32x4 type; };
template <int V> __device__ __forceinline__ float latent_lane(const typename LatentVec<V>::type& v, int j);
template <> __device__ __forceinline__ float latent_lane<1>(const float& v, int) { return v; }
template <> __device__ __forceinline__ float latent_lane<4>(const f32x4& v, int j) { return v[j]; }

// A thread owns V consecutive channels of one pixel (V = 4: 16-byte loads; the Z / V threads of a pixel read its mu half and then its logvar
// half contiguously) and walks the images of its slice, two in flight.
template <int V>
__global__ __launch_bounds__(256) void latent_fold_kernel(LatentFoldArgs a) {
  typedef typename LatentVec<V>::type vec;
  const int Z = a.Z, ZV = Z / V;
  const int64_t U = (int64_t)a.HW * Z;
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // group of V units
  if (g >= U / V) return;
  const int pix = (int)(g / ZV), c = (int)(g - (int64_t)pix * ZV) * V;
  const size_t row = (size_t)pix * 2 * Z + c, img = (size_t)a.HW * 2 * Z;
  const int n0 = blockIdx.y * a.per_slice, n1 = n0 + a.per_slice < a.N ? n0 + a.per_slice : a.N;
  double s_mu[V], s_sq[V], s_kl[V];
#pragma unroll
  for (int j = 0; j < V; ++j) s_mu[j] = s_sq[j] = s_kl[j] = 0.0;
  vec pmu = *reinterpret_cast<const vec*>(a.p + row), plv = *reinterpret_cast<const vec*>(a.p + row + Z);
  constexpr int UN = 2;
  for (int n = n0; n < n1; n += UN) {
    vec qmu[UN], qlv[UN], pm[UN], pl[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int nn = n + u < n1 ? n + u : n1 - 1;   // (a clamped image is loaded and not added)
      qmu[u] = *reinterpret_cast<const vec*>(a.q + nn * img + row);
      qlv[u] = *reinterpret_cast<const vec*>(a.q + nn * img + row + Z);
      pm[u] = a.p_bcast ? pmu : *reinterpret_cast<const vec*>(a.p + nn * img + row);
      pl[u] = a.p_bcast ? plv : *reinterpret_cast<const vec*>(a.p + nn * img + row + Z);
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      if (n + u >= n1) break;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float m = latent_lane<V>(qmu[u], j);
        const float k = normal_kl(m, latent_lane<V>(qlv[u], j), latent_lane<V>(pm[u], j), latent_lane<V>(pl[u], j));
        s_mu[j] += (double)m;
        s_sq[j] += (double)m * (double)m;
        s_kl[j] += (double)k;
      }
    }
  }
  double* out = a.part + (size_t)blockIdx.y * 3 * U + (size_t)pix * Z + c;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    out[j] = s_mu[j];
    out[U + j] = s_sq[j];
    out[2 * U + j] = s_kl[j];
  }
}

// sums[i] += part[0][i] + part[1][i] + ... in slice order, i < 3U
__global__ __launch_bounds__(256) void latent_reduce_kernel(const double* __restrict__ part, int slices, int64_t n3u, double* __restrict__ sums) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n3u; i += (int64_t)gridDim.x * 256) {
    double s = 0.0;
    for (int k = 0; k < slices; ++k) s += part[(size_t)k * n3u + i];
    sums[i] += s;
  }
}

// unit_out [3][U] = kl, mu_mean, mu_var (population variance, clamped at 0); layer_out [4] = KL-active units, mean-active units, U, sum of kl.
// One workgroup, fixed reduction order (as eval_totals_kernel).
__global__ __launch_bounds__(256) void latent_finalize_kernel(const double* __restrict__ sums, int64_t U, int64_t n_images, double kl_threshold,
                                                               double var_threshold, double* __restrict__ unit_out, double* __restrict__ layer_out) {
  __shared__ double red[3][256];
  const int t = threadIdx.x;
  const double inv_n = 1.0 / (double)n_images;
  double a[3] = {0.0, 0.0, 0.0};
  for (int64_t u = t; u < U; u += 256) {
    const double mean = sums[u] * inv_n;
    const double var = fmax(sums[U + u] * inv_n - mean * mean, 0.0);
    const double kl = sums[2 * U + u] * inv_n;
    unit_out[u] = kl;
    unit_out[U + u] = mean;
    unit_out[2 * U + u] = var;
    a[0] += kl > kl_threshold ? 1.0 : 0.0;
    a[1] += var > var_threshold ? 1.0 : 0.0;
    a[2] += kl;
  }
  for (int k = 0; k < 3; ++k) red[k][t] = a[k];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s)
      for (int k = 0; k < 3; ++k) red[k][t] += red[k][t + s];
    __syncthreads();
  }
  if (t == 0) {
    layer_out[0] = red[0][0];
    layer_out[1] = red[1][0];
    layer_out[2] = (double)U;
    layer_out[3] = red[2][0];
  }
}

}  // namespace lvae

using namespace lvae;

extern "C" size_t lvae_latent_stats_workspace(int32_t N, int32_t HW, int32_t Z) {
  if (N <= 0 || HW <= 0 || Z <= 0) return 0;
  const int64_t U = (int64_t)HW * Z;
  return (size_t)latent_slices(N, U) * 3 * (size_t)U * sizeof(double);
}

extern "C" int lvae_latent_stats_fold_f32(const float* p, int32_t p_bcast, const float* q, int32_t N, int32_t HW, int32_t Z, double* sums,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  LVAE_REQUIRE(p && q && sums && workspace, LVAE_EINVAL, "lvae_latent_stats_fold_f32: null pointer");
  LVAE_REQUIRE(N > 0 && HW > 0 && Z > 0, LVAE_EINVAL, "lvae_latent_stats_fold_f32: N %d, HW %d, Z %d must be positive", (int)N, (int)HW, (int)Z);
  LVAE_REQUIRE((int64_t)HW * Z < ((int64_t)1 << 29), LVAE_EINVAL, "lvae_latent_stats_fold_f32: %lld units in one layer", (long long)HW * Z);
  LVAE_REQUIRE(workspace_bytes >= lvae_latent_stats_workspace(N, HW, Z), LVAE_EINVAL,
               "lvae_latent_stats_fold_f32: workspace of %zu bytes, lvae_latent_stats_workspace asks for %zu", workspace_bytes,
               lvae_latent_stats_workspace(N, HW, Z));
  LVAE_REQUIRE((reinterpret_cast<uintptr_t>(sums) & 7) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, LVAE_EALIGN,
               "lvae_latent_stats_fold_f32: sums or workspace not 8-byte aligned");
  const int64_t U = (int64_t)HW * Z;
  const int per = latent_images_per_slice(N, U), slices = latent_slices(N, U);
  LatentFoldArgs a{p, q, reinterpret_cast<double*>(workspace), p_bcast ? 1 : 0, N, HW, Z, per};
  const bool v4 = Z % 4 == 0 && al16(p) && al16(q);
  const int64_t groups = v4 ? U / 4 : U;
  const int block = groups <= 64 ? 64 : 256;
  const dim3 grid((unsigned)((groups + block - 1) / block), (unsigned)slices);
  if (v4)
    hipLaunchKernelGGL(latent_fold_kernel<4>, grid, dim3(block), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(latent_fold_kernel<1>, grid, dim3(block), 0, (hipStream_t)stream, a);
  LVAE_LAUNCH_CHECK("latent_stats_fold");
  hipLaunchKernelGGL(latent_reduce_kernel, dim3(grid_for(3 * U, 256)), dim3(256), 0, (hipStream_t)stream, a.part, slices, 3 * U, sums);
  LVAE_LAUNCH_CHECK("latent_stats_reduce");
  return 0;
}

extern "C" int lvae_latent_stats_finalize_f64(const double* sums, int64_t U, int64_t n_images, double kl_threshold, double var_threshold,
                                              double* unit_out, double* layer_out, void* stream) {
  LVAE_REQUIRE(sums && unit_out && layer_out, LVAE_EINVAL, "lvae_latent_stats_finalize_f64: null pointer");
  LVAE_REQUIRE(U > 0, LVAE_EINVAL, "lvae_latent_stats_finalize_f64: U = %lld", (long long)U);
  LVAE_REQUIRE(n_images > 0, LVAE_EINVAL, "lvae_latent_stats_finalize_f64: n_images = %lld must be positive", (long long)n_images);
  hipLaunchKernelGGL(latent_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, sums, U, n_images, kl_threshold, var_threshold,
                     unit_out, layer_out);
  LVAE_LAUNCH_CHECK("latent_stats_finalize");
  return 0;
}
