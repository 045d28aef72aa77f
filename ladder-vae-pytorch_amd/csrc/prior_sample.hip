// Tempered draw from a layer's prior (sampling only, no backward): z = mu + (t * exp(lv / 2)) * eps with a temperature t per call or per
// row, z = mu exactly (a branch, eps never read) where t == 0, and log p(z) under the UNTEMPERED prior summed per row. The element-wise
// function is normal_logprob of lvae_common.h, the one the stochastic block's forward uses. HBM-bound: reads p and eps once, writes z once.
//
// A row's sum has a fixed order and no float atomics, so one workgroup owns a row. What made the scalar stochastic forward slow
// (stoch_core.h, in front of stoch_fwd_v4_map) was one dependent round trip per 256 elements of that row; here a workgroup is 1,024
// threads and every thread requests all the loads of an iteration before it uses the first: 8,192 elements (float4 map) or 4,096 (scalar
// map) are in flight per round trip, so the 16x16x32 level is one trip and a 32x32x32 level four.
#include "lvae_host.h"

namespace lvae {

struct PriorSampleArgs {
  const float* p;
  const float* eps;
  const float* row_t;
  float t;
  int p_bcast, HW, Z;
  float* z;
  float* logprob_p;
};

constexpr int kPsThreads = 1024;

// sum over the 1,024 threads in a fixed order (lanes by the shuffle tree, then waves 0..15); valid in every thread. `red` = 16 floats of LDS.
__device__ __forceinline__ float block_sum_1024(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int w = 1; w < kPsThreads / 64; ++w) s += red[w];
  return s;
}

__device__ __forceinline__ float tempered_draw(float mu, float lv, float eps, float tn, bool draw) {
  return draw ? mu + (tn * expf(0.5f * lv)) * eps : mu;
}

// Z % 4 == 0 and 16-byte aligned p, eps, z: a thread takes 4 consecutive channels of a pixel
__global__ __launch_bounds__(kPsThreads) void prior_sample_v4_kernel(PriorSampleArgs a) {
  __shared__ float red[kPsThreads / 64];
  const int n = blockIdx.x, t = threadIdx.x;
  const int Z = a.Z, Z4 = Z >> 2, per4 = a.HW * Z4;  // 4-channel groups of this row
  const float tn = a.row_t ? a.row_t[n] : a.t;
  const bool draw = tn != 0.f;                       // uniform over the workgroup
  const float* pn = a.p + (a.p_bcast ? 0 : (size_t)n * a.HW * 2 * Z);
  const float* en = a.eps + (size_t)n * a.HW * Z;    // dereferenced only when draw (a.eps may be null otherwise)
  float* zn = a.z + (size_t)n * a.HW * Z;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  constexpr int U = 2;
  float s_lp = 0.f;
  for (int base = 0; base < per4; base += kPsThreads * U) {
    f32x4 mu[U], lv[U], ev[U];
    int e[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      e[u] = base + u * kPsThreads + t;
      ok[u] = e[u] < per4;
      const int ee = ok[u] ? e[u] : 0;
      const int pix = ee / Z4, c = (ee - pix * Z4) * 4;
      const size_t b = (size_t)pix * 2 * Z + c;
      mu[u] = *reinterpret_cast<const f32x4*>(pn + b);
      lv[u] = *reinterpret_cast<const f32x4*>(pn + b + Z);
      ev[u] = draw ? *reinterpret_cast<const f32x4*>(en + (size_t)ee * 4) : zero4;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!ok[u]) continue;
      f32x4 zv;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        zv[j] = tempered_draw(mu[u][j], lv[u][j], ev[u][j], tn, draw);
        s_lp += normal_logprob(zv[j], mu[u][j], lv[u][j]);
      }
      *reinterpret_cast<f32x4*>(zn + (size_t)e[u] * 4) = zv;
    }
  }
  s_lp = block_sum_1024(s_lp, red);
  if (t == 0) a.logprob_p[n] = s_lp;
}

// any Z, any alignment: one element per thread and slot
__global__ __launch_bounds__(kPsThreads) void prior_sample_kernel(PriorSampleArgs a) {
  __shared__ float red[kPsThreads / 64];
  const int n = blockIdx.x, t = threadIdx.x;
  const int Z = a.Z, per = a.HW * Z;
  const float tn = a.row_t ? a.row_t[n] : a.t;
  const bool draw = tn != 0.f;
  const float* pn = a.p + (a.p_bcast ? 0 : (size_t)n * a.HW * 2 * Z);
  const float* en = a.eps + (size_t)n * per;
  float* zn = a.z + (size_t)n * per;
  constexpr int U = 4;
  float s_lp = 0.f;
  for (int base = 0; base < per; base += kPsThreads * U) {
    float mu[U], lv[U], ev[U];
    int e[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      e[u] = base + u * kPsThreads + t;
      ok[u] = e[u] < per;
      const int ee = ok[u] ? e[u] : 0;
      const int pix = ee / Z, c = ee - pix * Z;
      const size_t b = (size_t)pix * 2 * Z + c;
      mu[u] = pn[b];
      lv[u] = pn[b + Z];
      ev[u] = draw ? en[ee] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!ok[u]) continue;
      const float z = tempered_draw(mu[u], lv[u], ev[u], tn, draw);
      s_lp += normal_logprob(z, mu[u], lv[u]);
      zn[e[u]] = z;
    }
  }
  s_lp = block_sum_1024(s_lp, red);
  if (t == 0) a.logprob_p[n] = s_lp;
}

}  // namespace lvae

using namespace lvae;

extern "C" int lvae_normal_prior_sample_f32(const float* p, int32_t p_bcast, const float* eps, float temperature,
                                            const float* row_temperature, int32_t N, int32_t HW, int32_t Z, float* z,
                                            float* logprob_p, void* stream) {
  LVAE_REQUIRE(p && z && logprob_p, LVAE_EINVAL, "lvae_normal_prior_sample_f32: p, z or logprob_p missing");
  LVAE_REQUIRE(N > 0 && HW > 0 && Z > 0, LVAE_EINVAL, "lvae_normal_prior_sample_f32: N %d, HW %d, Z %d", N, HW, Z);
  LVAE_REQUIRE((int64_t)HW * 2 * Z <= INT32_MAX, LVAE_EINVAL, "lvae_normal_prior_sample_f32: a row of %d x %d exceeds 32-bit indexing", HW, Z);
  LVAE_REQUIRE(temperature >= 0.f && temperature <= 3.4028234664e38f, LVAE_EINVAL,
               "lvae_normal_prior_sample_f32: temperature %g is negative or not finite", (double)temperature);
  LVAE_REQUIRE(eps || (!row_temperature && temperature == 0.f), LVAE_EINVAL,
               "lvae_normal_prior_sample_f32: eps may be absent only with a scalar temperature of 0");
  const PriorSampleArgs a{p, eps, row_temperature, temperature, p_bcast, HW, Z, z, logprob_p};
  // the default limit: neither kernel has dynamic LDS
  if (Z % 4 == 0 && al16(p) && al16_or_null(eps) && al16(z))
    return launch_lds<prior_sample_v4_kernel>("normal_prior_sample", dim3(N), dim3(kPsThreads), 0, 64 * 1024, (hipStream_t)stream, a);
  return launch_lds<prior_sample_kernel>("normal_prior_sample", dim3(N), dim3(kPsThreads), 0, 64 * 1024, (hipStream_t)stream, a);
}
