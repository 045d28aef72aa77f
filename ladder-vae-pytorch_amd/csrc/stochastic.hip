// NormalStochasticBlock2d elementwise core (lib/stochastic.py:45-99, 209-226), absolute form: reparameterised sample, log p(z),
// log q(z), Monte-Carlo and analytical KL with their per-sample and per-pixel reductions, and the hand-written backward. The element
// arithmetic (abs_terms / abs_grads and their prior-only counterparts) and the thread maps are in stoch_core.h; this file holds the
// policy that joins them, the kernels and the entry points. HBM-bound: reads p, q, eps once and writes z once.
#include "stoch_core.h"

namespace lvae {

struct StochArgs {
  const float* p;
  const float* q;
  const float* eps;
  int p_bcast, N, HW, Z, mode, analytical;
};

struct StochBwdArgs {
  const float *p, *q, *eps, *z, *dz, *g_lp, *g_lq, *g_kl, *g_ks;
  int p_bcast, N, HW, Z, mode, analytical;
};

// q may be absent (the prior-only block); no q_out: q is the caller's own tensor
struct StochAbs {
  static constexpr bool kSecondOptional = true, kWritesQ = false;
  template <class A>
  static __device__ __forceinline__ const float* second(const A& a) { return a.q; }
  static __device__ __forceinline__ StochTerms terms(float pmu, float plv, float qmu, float qlv, float e, int mode, int analytical) {
    return abs_terms(pmu, plv, qmu, qlv, e, mode, analytical);
  }
  static __device__ __forceinline__ StochTerms terms_prior(float pmu, float plv, float e, int mode) { return abs_terms_prior(pmu, plv, e, mode); }
  static __device__ __forceinline__ float kan(float pmu, float plv, float qmu, float qlv) { return normal_kl(qmu, qlv, pmu, plv); }
  static __device__ __forceinline__ StochGrads grads(float pmu, float plv, float qmu, float qlv, float e, float z, float dzu, float G_lp,
                                                     float G_lq, float G_an, int mode) {
    return abs_grads(pmu, plv, qmu, qlv, e, z, dzu, G_lp, G_lq, G_an, mode);
  }
  static __device__ __forceinline__ StochGrads grads_prior(float pmu, float plv, float e, float z, float dzu, float glp, int mode) {
    return abs_grads_prior(pmu, plv, e, z, dzu, glp, mode);
  }
  static __device__ __forceinline__ bool needs_z(int) { return true; }
};

__global__ __launch_bounds__(256) void stoch_fwd_kernel(StochArgs a, float* __restrict__ z_out, float* logprob_p, float* logprob_q,
                                                         float* kl_samplewise, float* kl_spatial) {
  stoch_fwd_map<StochAbs>(a, z_out, nullptr, logprob_p, logprob_q, kl_samplewise, kl_spatial);
}

__global__ __launch_bounds__(256) void stoch_fwd_v4_kernel(StochArgs a, float* __restrict__ z_out, float* logprob_p, float* logprob_q,
                                                            float* kl_samplewise, float* kl_spatial) {
  stoch_fwd_v4_map<StochAbs>(a, z_out, nullptr, logprob_p, logprob_q, kl_samplewise, kl_spatial);
}

// (the scalar map: a 16-byte absolute backward is a speed change of its own, to be measured)
__global__ __launch_bounds__(256) void stoch_bwd_kernel(StochBwdArgs a, float* __restrict__ dp, float* __restrict__ dq) {
  stoch_bwd_map<StochAbs>(a, dp, dq);
}

// Elementwise KL (lib/stochastic.py:88-91 `kl_elementwise`, :209-226 kl_normal_mc): out[n,pix,c] = log q(z) - log p(z) (Monte
// Carlo) or KL(q || p) (analytical). Not on the training path (TopDownLayer consumes the per-sample sums of stoch_fwd_kernel);
// kept as its own pass so the training step does not write a tensor nobody reads. The two kernels keep their own arithmetic: they
// evaluate one of the two KLs, never both, and the backward forms -g x where abs_grads forms G_lp x - G_an y with one weight zero,
// which is another sequence of roundings (and of infinities).
struct KlElemArgs {
  const float *p, *q, *z, *g;
  int p_bcast, q_bcast, HW, Z, analytical;
  int64_t total;
};

__global__ __launch_bounds__(256) void kl_elem_fwd_kernel(KlElemArgs a, float* __restrict__ out) {
  const int Z = a.Z;
  const int64_t per = (int64_t)a.HW * Z;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.total; i += (int64_t)gridDim.x * 256) {
    const int64_t n = i / per;
    const int e = (int)(i - n * per);
    const int pix = e / Z, c = e - pix * Z;
    const size_t pb = ((a.p_bcast ? 0 : (size_t)n * a.HW) + pix) * 2 * Z, qb = ((a.q_bcast ? 0 : (size_t)n * a.HW) + pix) * 2 * Z;
    const float pmu = a.p[pb + c], plv = a.p[pb + Z + c], qmu = a.q[qb + c], qlv = a.q[qb + Z + c];
    out[i] = a.analytical ? normal_kl(qmu, qlv, pmu, plv) : normal_logprob(a.z[i], qmu, qlv) - normal_logprob(a.z[i], pmu, plv);
  }
}

// g = d/d(out); writes dp, dq (full batch shape; the caller reduces a broadcast operand) and dz (Monte Carlo only, else zeros)
__global__ __launch_bounds__(256) void kl_elem_bwd_kernel(KlElemArgs a, float* __restrict__ dp, float* __restrict__ dq,
                                                           float* __restrict__ dz) {
  const int Z = a.Z;
  const int64_t per = (int64_t)a.HW * Z;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.total; i += (int64_t)gridDim.x * 256) {
    const int64_t n = i / per;
    const int e = (int)(i - n * per);
    const int pix = e / Z, c = e - pix * Z;
    const size_t pb = ((a.p_bcast ? 0 : (size_t)n * a.HW) + pix) * 2 * Z, qb = ((a.q_bcast ? 0 : (size_t)n * a.HW) + pix) * 2 * Z;
    const size_t ob = ((size_t)n * a.HW + pix) * 2 * Z;
    const float pmu = a.p[pb + c], plv = a.p[pb + Z + c], qmu = a.q[qb + c], qlv = a.q[qb + Z + c];
    const float g = a.g[i];
    const float ivp = expf(-plv);
    float dpmu, dplv, dqmu, dqlv, dzz = 0.f;
    if (a.analytical) {
      const float dmu = qmu - pmu, vr = expf(qlv - plv);
      dpmu = -g * dmu * ivp;
      dplv = g * 0.5f * (1.f - vr - dmu * dmu * ivp);
      dqmu = g * dmu * ivp;
      dqlv = g * 0.5f * (vr - 1.f);
    } else {
      const float z = a.z[i], ivq = expf(-qlv), dpz = z - pmu, dqz = z - qmu;
      dpmu = -g * dpz * ivp;
      dplv = -g * 0.5f * (dpz * dpz * ivp - 1.f);
      dqmu = g * dqz * ivq;
      dqlv = g * 0.5f * (dqz * dqz * ivq - 1.f);
      dzz = g * (dpz * ivp - dqz * ivq);
    }
    dp[ob + c] = dpmu;
    dp[ob + Z + c] = dplv;
    dq[ob + c] = dqmu;
    dq[ob + Z + c] = dqlv;
    if (dz) dz[i] = dzz;
  }
}

}  // namespace lvae

using namespace lvae;

extern "C" int lvae_normal_stochastic_fwd_f32(const float* p, int32_t p_bcast, const float* q, const float* eps,
                                              int32_t N, int32_t HW, int32_t Z, int32_t mode, int32_t analytical_kl,
                                              float* z, float* logprob_p, float* logprob_q, float* kl_samplewise,
                                              float* kl_spatial, void* stream) {
  LVAE_REQUIRE(p && z && logprob_p && N > 0 && HW > 0 && Z > 0, LVAE_EINVAL, "lvae_normal_stochastic_fwd_f32: bad args");
  LVAE_REQUIRE((int64_t)HW * Z * 2 <= INT32_MAX, LVAE_EINVAL, "lvae_normal_stochastic_fwd_f32: HW * Z too large");
  LVAE_REQUIRE(mode >= 0 && mode <= 2, LVAE_EINVAL, "lvae_normal_stochastic_fwd_f32: mode %d", mode);
  LVAE_REQUIRE(mode == 1 || eps, LVAE_EINVAL, "lvae_normal_stochastic_fwd_f32: eps / forced latent missing");
  LVAE_REQUIRE(!q || (logprob_q && kl_samplewise), LVAE_EINVAL, "lvae_normal_stochastic_fwd_f32: q outputs missing");
  StochArgs a{p, q, eps, p_bcast, N, HW, Z, mode, analytical_kl};
  const int z4 = Z >> 2;
  if (Z % 4 == 0 && z4 <= 16 && (z4 & (z4 - 1)) == 0 && al16(p) && al16_or_null(q) && al16_or_null(eps) && al16(z))
    hipLaunchKernelGGL(stoch_fwd_v4_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, a, z, logprob_p, logprob_q, kl_samplewise, kl_spatial);
  else
    hipLaunchKernelGGL(stoch_fwd_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, a, z, logprob_p, logprob_q,
                       kl_samplewise, kl_spatial);
  LVAE_LAUNCH_CHECK("normal_stochastic_fwd");
  return 0;
}

extern "C" int lvae_normal_stochastic_bwd_f32(const float* p, int32_t p_bcast, const float* q, const float* eps,
                                              const float* z, const float* dz, const float* g_lp, const float* g_lq,
                                              const float* g_kl, const float* g_ks, int32_t N, int32_t HW, int32_t Z,
                                              int32_t mode, int32_t analytical_kl, float* dp, float* dq, void* stream) {
  LVAE_REQUIRE(p && z && dp && N > 0 && HW > 0 && Z > 0, LVAE_EINVAL, "lvae_normal_stochastic_bwd_f32: bad args");
  LVAE_REQUIRE((int64_t)HW * Z * 2 <= INT32_MAX, LVAE_EINVAL, "lvae_normal_stochastic_bwd_f32: HW * Z too large");
  LVAE_REQUIRE((q == nullptr) == (dq == nullptr), LVAE_EINVAL, "lvae_normal_stochastic_bwd_f32: q/dq mismatch");
  LVAE_REQUIRE(mode != 0 || eps, LVAE_EINVAL, "lvae_normal_stochastic_bwd_f32: eps missing");
  StochBwdArgs a{p, q, eps, z, dz, g_lp, g_lq, g_kl, g_ks, p_bcast, N, HW, Z, mode, analytical_kl};
  const int64_t total = (int64_t)N * HW * Z;
  hipLaunchKernelGGL(stoch_bwd_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, a, dp, dq);
  LVAE_LAUNCH_CHECK("normal_stochastic_bwd");
  return 0;
}

extern "C" int lvae_kl_elementwise_fwd_f32(const float* p, int32_t p_bcast, const float* q, int32_t q_bcast, const float* z,
                                           int32_t N, int32_t HW, int32_t Z, int32_t analytical_kl, float* out, void* stream) {
  LVAE_REQUIRE(p && q && out && N > 0 && HW > 0 && Z > 0, LVAE_EINVAL, "lvae_kl_elementwise_fwd_f32: bad args");
  LVAE_REQUIRE(analytical_kl || z, LVAE_EINVAL, "lvae_kl_elementwise_fwd_f32: z missing");
  KlElemArgs a{p, q, z, nullptr, p_bcast, q_bcast, HW, Z, analytical_kl, (int64_t)N * HW * Z};
  hipLaunchKernelGGL(kl_elem_fwd_kernel, dim3(grid_for(a.total, 256)), dim3(256), 0, (hipStream_t)stream, a, out);
  LVAE_LAUNCH_CHECK("kl_elementwise_fwd");
  return 0;
}

extern "C" int lvae_kl_elementwise_bwd_f32(const float* p, int32_t p_bcast, const float* q, int32_t q_bcast, const float* z,
                                           const float* g, int32_t N, int32_t HW, int32_t Z, int32_t analytical_kl, float* dp,
                                           float* dq, float* dz, void* stream) {
  LVAE_REQUIRE(p && q && g && dp && dq && N > 0 && HW > 0 && Z > 0, LVAE_EINVAL, "lvae_kl_elementwise_bwd_f32: bad args");
  LVAE_REQUIRE(analytical_kl || z, LVAE_EINVAL, "lvae_kl_elementwise_bwd_f32: z missing");
  KlElemArgs a{p, q, z, g, p_bcast, q_bcast, HW, Z, analytical_kl, (int64_t)N * HW * Z};
  hipLaunchKernelGGL(kl_elem_bwd_kernel, dim3(grid_for(a.total, 256)), dim3(256), 0, (hipStream_t)stream, a, dp, dq, dz);
  LVAE_LAUNCH_CHECK("kl_elementwise_bwd");
  return 0;
}
