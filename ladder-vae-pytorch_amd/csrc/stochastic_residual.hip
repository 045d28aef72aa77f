// NormalStochasticBlock2d elementwise core with the posterior given RELATIVE to the prior of the same layer (the residual normal of
// NVAE, Vahdat & Kautz 2020, section 3.2): mu_q = mu_p + dmu, logvar_q = logvar_p + dlv, with d = (dmu | dlv) the output of conv_in_q.
// The thread maps, reductions and modes are stoch_core.h's, shared with stochastic.hip; the arithmetic (res_terms / res_grads, in the same
// header) is not the absolute one: every quantity is formed from the offset, never from the rounded sum p + d. With s_p = exp(lv_p / 2),
// s_q = s_p exp(dlv / 2), a = z - mu_p and u = (z - mu_q) / s_q:
//   mode 0: z = (mu_p + dmu) + s_q eps, a = dmu + s_q eps, u = eps      mode 1: z = mu_p + dmu, a = dmu, u = 0
//   mode 2: z given, a = z - mu_p, u = (a - dmu) / s_q
//   log p(z) = -a^2 exp(-lv_p) / 2 - lv_p / 2 - log sqrt(2 pi)          log q(z) = -u^2 / 2 - (lv_p + dlv) / 2 - log sqrt(2 pi)
//   analytical KL = (expm1(dlv) - dlv + dmu^2 exp(-lv_p)) / 2           Monte-Carlo KL = (a^2 exp(-lv_p) - u^2) / 2 - dlv / 2
// (the Monte-Carlo KL is log q - log p with the two terms both hold, lv_p / 2 and the constant, cancelled on paper instead of in fp32).
// With |mu_p| >> s_p the absolute formula loses dmu in the rounding of mu_q before the kernel sees it; here it arrives intact.
// Backward: dd is the gradient of the offset; dp the TOTAL gradient of the prior parameters: their own terms plus what flows through
// q = p + d, summed on paper term by term. In modes 0 / 1 that leaves d/dmu_p = dz alone (a and u do not depend on mu_p), and the lv_p
// part of the analytical KL is -G dmu^2 exp(-lv_p) / 2: the (variance ratio - 1) terms of the absolute form cancel and never appear.
// HBM-bound: reads p, d, eps once, writes z once and, only where the caller wants absolute posterior parameters, q_out = p + d once.
#include "stoch_core.h"

namespace lvae {

struct StochResArgs {
  const float* p;
  const float* d;
  const float* eps;
  int p_bcast, N, HW, Z, mode, analytical;
};

struct StochResBwdArgs {
  const float *p, *d, *eps, *z, *dz, *g_lp, *g_lq, *g_kl, *g_ks;
  int p_bcast, N, HW, Z, mode, analytical;
};

// d is always there; q_out = p + d is written where the caller passes one; the backward reads z only where it was forced (mode 2)
struct StochRes {
  static constexpr bool kSecondOptional = false, kWritesQ = true;
  template <class A>
  static __device__ __forceinline__ const float* second(const A& a) { return a.d; }
  static __device__ __forceinline__ StochTerms terms(float pmu, float plv, float dmu, float dlv, float e, int mode, int analytical) {
    return res_terms(pmu, plv, dmu, dlv, e, mode, analytical);
  }
  static __device__ __forceinline__ float kan(float, float plv, float dmu, float dlv) { return res_kan(dmu, dlv, expf(-plv)); }
  static __device__ __forceinline__ StochGrads grads(float pmu, float plv, float dmu, float dlv, float e, float z, float dzu, float G_lp,
                                                     float G_lq, float G_an, int mode) {
    return res_grads(pmu, plv, dmu, dlv, e, z, dzu, G_lp, G_lq, G_an, mode);
  }
  static __device__ __forceinline__ bool needs_z(int mode) { return mode == 2; }
};

__global__ __launch_bounds__(256) void stoch_res_fwd_kernel(StochResArgs a, float* __restrict__ z_out, float* __restrict__ q_out,
                                                             float* logprob_p, float* logprob_q, float* kl_samplewise,
                                                             float* kl_spatial) {
  stoch_fwd_map<StochRes>(a, z_out, q_out, logprob_p, logprob_q, kl_samplewise, kl_spatial);
}

__global__ __launch_bounds__(256) void stoch_res_fwd_v4_kernel(StochResArgs a, float* __restrict__ z_out, float* __restrict__ q_out,
                                                                float* logprob_p, float* logprob_q, float* kl_samplewise,
                                                                float* kl_spatial) {
  stoch_fwd_v4_map<StochRes>(a, z_out, q_out, logprob_p, logprob_q, kl_samplewise, kl_spatial);
}

__global__ __launch_bounds__(256) void stoch_res_bwd_kernel(StochResBwdArgs a, float* __restrict__ dp, float* __restrict__ dd) {
  stoch_bwd_map<StochRes>(a, dp, dd);
}

__global__ __launch_bounds__(256) void stoch_res_bwd_v4_kernel(StochResBwdArgs a, float* __restrict__ dp, float* __restrict__ dd) {
  stoch_bwd_v4_map<StochRes>(a, dp, dd);
}

}  // namespace lvae

using namespace lvae;

extern "C" int lvae_normal_stochastic_res_fwd_f32(const float* p, int32_t p_bcast, const float* d, const float* eps, int32_t N,
                                                  int32_t HW, int32_t Z, int32_t mode, int32_t analytical_kl, float* z, float* q_out,
                                                  float* logprob_p, float* logprob_q, float* kl_samplewise, float* kl_spatial,
                                                  void* stream) {
  LVAE_REQUIRE(p && d && z && logprob_p && logprob_q && kl_samplewise && N > 0 && HW > 0 && Z > 0, LVAE_EINVAL,
               "lvae_normal_stochastic_res_fwd_f32: bad args");
  LVAE_REQUIRE((int64_t)HW * Z * 2 <= INT32_MAX, LVAE_EINVAL, "lvae_normal_stochastic_res_fwd_f32: HW * Z too large");
  LVAE_REQUIRE(mode >= 0 && mode <= 2, LVAE_EINVAL, "lvae_normal_stochastic_res_fwd_f32: mode %d", mode);
  LVAE_REQUIRE(mode == 1 || eps, LVAE_EINVAL, "lvae_normal_stochastic_res_fwd_f32: eps / forced latent missing");
  StochResArgs a{p, d, eps, p_bcast, N, HW, Z, mode, analytical_kl};
  const int z4 = Z >> 2;
  if (Z % 4 == 0 && z4 <= 16 && (z4 & (z4 - 1)) == 0 && al16(p) && al16(d) && al16_or_null(eps) && al16(z) && al16_or_null(q_out))
    hipLaunchKernelGGL(stoch_res_fwd_v4_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, a, z, q_out, logprob_p, logprob_q,
                       kl_samplewise, kl_spatial);
  else
    hipLaunchKernelGGL(stoch_res_fwd_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, a, z, q_out, logprob_p, logprob_q,
                       kl_samplewise, kl_spatial);
  LVAE_LAUNCH_CHECK("normal_stochastic_res_fwd");
  return 0;
}

extern "C" int lvae_normal_stochastic_res_bwd_f32(const float* p, int32_t p_bcast, const float* d, const float* eps, const float* z,
                                                  const float* dz, const float* g_lp, const float* g_lq, const float* g_kl,
                                                  const float* g_ks, int32_t N, int32_t HW, int32_t Z, int32_t mode,
                                                  int32_t analytical_kl, float* dp, float* dd, void* stream) {
  LVAE_REQUIRE(p && d && dp && dd && N > 0 && HW > 0 && Z > 0, LVAE_EINVAL, "lvae_normal_stochastic_res_bwd_f32: bad args");
  LVAE_REQUIRE((int64_t)HW * Z * 2 <= INT32_MAX, LVAE_EINVAL, "lvae_normal_stochastic_res_bwd_f32: HW * Z too large");
  LVAE_REQUIRE(mode >= 0 && mode <= 2, LVAE_EINVAL, "lvae_normal_stochastic_res_bwd_f32: mode %d", mode);
  LVAE_REQUIRE(mode != 0 || eps, LVAE_EINVAL, "lvae_normal_stochastic_res_bwd_f32: eps missing");
  LVAE_REQUIRE(mode != 2 || z, LVAE_EINVAL, "lvae_normal_stochastic_res_bwd_f32: forced latent missing");
  StochResBwdArgs a{p, d, eps, z, dz, g_lp, g_lq, g_kl, g_ks, p_bcast, N, HW, Z, mode, analytical_kl};
  const int64_t total = (int64_t)N * HW * Z;
  if (Z % 4 == 0 && al16(p) && al16(d) && al16_or_null(eps) && al16_or_null(z) && al16_or_null(dz) && al16(dp) && al16(dd))
    hipLaunchKernelGGL(stoch_res_bwd_v4_kernel, dim3(grid_for(total / 4, 256)), dim3(256), 0, (hipStream_t)stream, a, dp, dd);
  else
    hipLaunchKernelGGL(stoch_res_bwd_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, a, dp, dd);
  LVAE_LAUNCH_CHECK("normal_stochastic_res_bwd");
  return 0;
}
