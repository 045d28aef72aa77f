// NormalStochasticBlock2d elementwise core with the posterior given RELATIVE to the prior of the same layer (the residual normal of
// NVAE, Vahdat & Kautz 2020, section 3.2): mu_q = mu_p + dmu, logvar_q = logvar_p + dlv, with d = (dmu | dlv) the output of conv_in_q.
// The thread maps, reductions and modes are those of stochastic.hip; the arithmetic is not: every quantity is formed from the offset,
// never from the rounded sum p + d. With s_p = exp(lv_p / 2), s_q = s_p exp(dlv / 2), a = z - mu_p and u = (z - mu_q) / s_q:
//   mode 0: z = (mu_p + dmu) + s_q eps, a = dmu + s_q eps, u = eps      mode 1: z = mu_p + dmu, a = dmu, u = 0
//   mode 2: z given, a = z - mu_p, u = (a - dmu) / s_q
//   log p(z) = -a^2 exp(-lv_p) / 2 - lv_p / 2 - log sqrt(2 pi)          log q(z) = -u^2 / 2 - (lv_p + dlv) / 2 - log sqrt(2 pi)
//   analytical KL = (expm1(dlv) - dlv + dmu^2 exp(-lv_p)) / 2           Monte-Carlo KL = (a^2 exp(-lv_p) - u^2) / 2 - dlv / 2
// (the Monte-Carlo KL is log q - log p with the two terms both hold, lv_p / 2 and the constant, cancelled on paper instead of in fp32).
// With |mu_p| >> s_p the absolute formula loses dmu in the rounding of mu_q before the kernel sees it; here it arrives intact.
// HBM-bound: reads p, d, eps once, writes z once and, only where the caller wants absolute posterior parameters, q_out = p + d once.
#include "lvae_common.h"

namespace lvae {

struct ResTerms {
  float z, lp, lq, kan, kl;   // kl: the term of kl_samplewise (analytical or Monte Carlo); kan: always the analytical one
};

// one element of the forward; e = eps (mode 0) or the forced latent (mode 2)
__device__ __forceinline__ ResTerms res_terms(float pmu, float plv, float dmu, float dlv, float e, int mode, int analytical) {
  const float sp = expf(0.5f * plv);
  const float sq = sp * expf(0.5f * dlv);   // a product, not exp of the sum: d = 0 gives the prior's own sigma, bit for bit
  const float ivp = expf(-plv);
  ResTerms r;
  float a, u;
  if (mode == 0) {
    const float se = sq * e;
    r.z = (pmu + dmu) + se;
    a = dmu + se;
    u = e;
  } else if (mode == 1) {
    r.z = pmu + dmu;
    a = dmu;
    u = 0.f;
  } else {
    r.z = e;
    a = e - pmu;
    u = (a - dmu) / sq;
  }
  const float ap = a * a * ivp, uu = u * u;
  r.lp = -0.5f * ap - 0.5f * plv - kLogSqrt2Pi;
  r.lq = -0.5f * uu - 0.5f * (plv + dlv) - kLogSqrt2Pi;
  r.kan = 0.5f * (expm1f(dlv) - dlv + dmu * dmu * ivp);
  r.kl = analytical ? r.kan : 0.5f * (ap - uu) - 0.5f * dlv;
  return r;
}

struct StochResArgs {
  const float* p;
  const float* d;
  const float* eps;
  int p_bcast, N, HW, Z, mode, analytical;
};

// scalar map: one element per thread and pass, as stoch_fwd_kernel
__global__ __launch_bounds__(256) void stoch_res_fwd_kernel(StochResArgs a, float* __restrict__ z_out, float* __restrict__ q_out,
                                                             float* logprob_p, float* logprob_q, float* kl_samplewise,
                                                             float* kl_spatial) {
  __shared__ float red[4];
  const int n = blockIdx.x, t = threadIdx.x;
  const int Z = a.Z, per = a.HW * Z;
  const float* pn = a.p + (a.p_bcast ? 0 : (size_t)n * a.HW * 2 * Z);
  const float* dn = a.d + (size_t)n * a.HW * 2 * Z;
  float* qo = q_out ? q_out + (size_t)n * a.HW * 2 * Z : nullptr;
  const bool zpow2 = (Z & (Z - 1)) == 0 && Z <= 64;
  float s_lp = 0.f, s_lq = 0.f, s_kl = 0.f;
  // whole 256-element passes: every lane of a wave takes part in the shuffles
  const int passes = (per + 255) / 256;
  for (int it = 0; it < passes; ++it) {
    const int e = it * 256 + t;
    const bool ok = e < per;
    float kan = 0.f;
    int pix = 0;
    if (ok) {
      pix = e / Z;
      const int c = e - pix * Z;
      const size_t b = (size_t)pix * 2 * Z + c;
      const float pmu = pn[b], plv = pn[b + Z], dmu = dn[b], dlv = dn[b + Z];
      const size_t zi = (size_t)n * per + e;
      const ResTerms r = res_terms(pmu, plv, dmu, dlv, a.mode != 1 ? a.eps[zi] : 0.f, a.mode, a.analytical);
      z_out[zi] = r.z;
      if (qo) {
        qo[b] = pmu + dmu;
        qo[b + Z] = plv + dlv;
      }
      s_lp += r.lp;
      s_lq += r.lq;
      s_kl += r.kl;
      kan = r.kan;
    }
    if (kl_spatial && zpow2) {
      float v = kan;
      for (int o = Z >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (ok && (e % Z) == 0) kl_spatial[(size_t)n * a.HW + pix] = v;
    }
  }
  if (kl_spatial && !zpow2) {
    for (int pix = t; pix < a.HW; pix += 256) {
      float v = 0.f;
      for (int c = 0; c < Z; ++c) {
        const size_t b = (size_t)pix * 2 * Z + c;
        const float dmu = dn[b], dlv = dn[b + Z];
        v += 0.5f * (expm1f(dlv) - dlv + dmu * dmu * expf(-pn[b + Z]));
      }
      kl_spatial[(size_t)n * a.HW + pix] = v;
    }
  }
  s_lp = block_sum_256(s_lp, red);
  s_lq = block_sum_256(s_lq, red);
  s_kl = block_sum_256(s_kl, red);
  if (t == 0) {
    logprob_p[n] = s_lp;
    logprob_q[n] = s_lq;
    kl_samplewise[n] = s_kl;
  }
}

// 16-byte map (Z % 4 == 0, Z / 4 a power of two <= 16, 16-byte aligned tensors), as stoch_fwd_v4_kernel: a thread takes 4 consecutive
// channels of a pixel, two 1,024-element passes are in flight per iteration, the per-pixel KL is a shuffle reduction over Z / 4 lanes.
__global__ __launch_bounds__(256) void stoch_res_fwd_v4_kernel(StochResArgs a, float* __restrict__ z_out, float* __restrict__ q_out,
                                                                float* logprob_p, float* logprob_q, float* kl_samplewise,
                                                                float* kl_spatial) {
  __shared__ float red[4];
  const int n = blockIdx.x, t = threadIdx.x;
  const int Z = a.Z, Z4 = Z >> 2, per4 = a.HW * Z4;   // 4-channel groups of this sample
  const float* pn = a.p + (a.p_bcast ? 0 : (size_t)n * a.HW * 2 * Z);
  const float* dn = a.d + (size_t)n * a.HW * 2 * Z;
  const float* en = a.eps ? a.eps + (size_t)n * a.HW * Z : nullptr;
  float* zn = z_out + (size_t)n * a.HW * Z;
  float* qo = q_out ? q_out + (size_t)n * a.HW * 2 * Z : nullptr;
  float s_lp = 0.f, s_lq = 0.f, s_kl = 0.f;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  constexpr int U = 2;
  for (int it = 0; it * 256 * U < per4; ++it) {
    f32x4 pmu[U], plv[U], dmu[U], dlv[U], ev[U];
    int pix[U], c[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = (it * U + u) * 256 + t;
      ok[u] = e < per4;
      const int ee = ok[u] ? e : 0;   // lanes past the end read group 0 (in bounds) and write nothing
      pix[u] = ee / Z4;
      c[u] = (ee - pix[u] * Z4) * 4;
      const size_t b = (size_t)pix[u] * 2 * Z + c[u];
      pmu[u] = *reinterpret_cast<const f32x4*>(pn + b);
      plv[u] = *reinterpret_cast<const f32x4*>(pn + b + Z);
      dmu[u] = *reinterpret_cast<const f32x4*>(dn + b);
      dlv[u] = *reinterpret_cast<const f32x4*>(dn + b + Z);
      ev[u] = a.mode != 1 ? *reinterpret_cast<const f32x4*>(en + (size_t)pix[u] * Z + c[u]) : zero4;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      f32x4 zv;
      float kan = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const ResTerms r = res_terms(pmu[u][j], plv[u][j], dmu[u][j], dlv[u][j], ev[u][j], a.mode, a.analytical);
        zv[j] = r.z;
        if (ok[u]) {
          s_lp += r.lp;
          s_lq += r.lq;
          s_kl += r.kl;
          kan += r.kan;
        }
      }
      if (ok[u]) {
        *reinterpret_cast<f32x4*>(zn + (size_t)pix[u] * Z + c[u]) = zv;
        if (qo) {
          const size_t b = (size_t)pix[u] * 2 * Z + c[u];
          *reinterpret_cast<f32x4*>(qo + b) = pmu[u] + dmu[u];
          *reinterpret_cast<f32x4*>(qo + b + Z) = plv[u] + dlv[u];
        }
      }
      if (kl_spatial) {   // all lanes take part in the shuffles; the Z / 4 lanes of a pixel are consecutive
        float v = kan;
        for (int o = Z4 >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (ok[u] && c[u] == 0) kl_spatial[(size_t)n * a.HW + pix[u]] = v;
      }
    }
  }
  s_lp = block_sum_256(s_lp, red);
  s_lq = block_sum_256(s_lq, red);
  s_kl = block_sum_256(s_kl, red);
  if (t == 0) {
    logprob_p[n] = s_lp;
    logprob_q[n] = s_lq;
    kl_samplewise[n] = s_kl;
  }
}

// Backward. dd is the gradient of the offset; dp the TOTAL gradient of the prior parameters: their own terms plus what flows through
// q = p + d, summed on paper term by term. In modes 0 / 1 that leaves d/dmu_p = dz alone (a and u do not depend on mu_p), and the lv_p
// part of the analytical KL is -G dmu^2 exp(-lv_p) / 2: the (variance ratio - 1) terms of the absolute form cancel and never appear.
struct StochResBwdArgs {
  const float *p, *d, *eps, *z, *dz, *g_lp, *g_lq, *g_kl, *g_ks;
  int p_bcast, N, HW, Z, mode, analytical;
};

struct ResGrads {
  float pmu, plv, dmu, dlv;
};

// G_lp, G_lq, G_an: the upstream weights of log p, log q and the analytical KL of this element; e = eps (mode 0); z read in mode 2 only
__device__ __forceinline__ ResGrads res_grads(float pmu, float plv, float dmu, float dlv, float e, float z, float dzu, float G_lp,
                                              float G_lq, float G_an, int mode) {
  const float sq = expf(0.5f * plv) * expf(0.5f * dlv);
  const float ivp = expf(-plv);
  float a, uu = 0.f;   // uu: u^2 where u depends on the parameters (mode 2); in modes 0 / 1 u is eps or 0, a constant
  float qterm = 0.f;   // G_lq u / s_q (mode 2)
  if (mode == 0) a = dmu + sq * e;
  else if (mode == 1) a = dmu;
  else {
    a = z - pmu;
    const float u = (a - dmu) / sq;
    uu = u * u;
    qterm = G_lq * u / sq;
  }
  const float t_lp = G_lp * a * ivp;
  const float k_mu = G_an * dmu * ivp;
  const float lq_lv = G_lq * 0.5f * (uu - 1.f);
  ResGrads g;
  g.dlv = lq_lv + G_an * 0.5f * expm1f(dlv);
  g.plv = G_lp * 0.5f * (a * a * ivp - 1.f) + lq_lv - 0.5f * k_mu * dmu;
  if (mode <= 1) {
    const float Gz = dzu - t_lp;   // everything that reaches z: the upstream gradient and log p's own (log q's: none, u is constant)
    g.pmu = dzu;
    g.dmu = Gz + k_mu;
    if (mode == 0) {
      const float w = Gz * 0.5f * sq * e;
      g.plv += w;
      g.dlv += w;
    }
  } else {
    g.pmu = t_lp + qterm;
    g.dmu = qterm + k_mu;
  }
  return g;
}

__device__ __forceinline__ void res_weights(const StochResBwdArgs& a, int n, int pix, float& G_lp, float& G_lq, float& G_an) {
  const float glp = a.g_lp ? a.g_lp[n] : 0.f;
  const float gkl = a.g_kl ? a.g_kl[n] : 0.f;
  G_lp = glp - (a.analytical ? 0.f : gkl);
  G_lq = (a.g_lq ? a.g_lq[n] : 0.f) + (a.analytical ? 0.f : gkl);
  G_an = (a.g_ks ? a.g_ks[(size_t)n * a.HW + pix] : 0.f) + (a.analytical ? gkl : 0.f);
}

__global__ __launch_bounds__(256) void stoch_res_bwd_kernel(StochResBwdArgs a, float* __restrict__ dp, float* __restrict__ dd) {
  const int Z = a.Z;
  const int64_t per = (int64_t)a.HW * Z, total = per * a.N;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int n = (int)(i / per);
    const int e = (int)(i - (int64_t)n * per);
    const int pix = e / Z, c = e - pix * Z;
    const size_t pb = ((a.p_bcast ? 0 : (size_t)n * a.HW) + pix) * 2 * Z + c, ob = ((size_t)n * a.HW + pix) * 2 * Z + c;
    float G_lp, G_lq, G_an;
    res_weights(a, n, pix, G_lp, G_lq, G_an);
    const ResGrads g = res_grads(a.p[pb], a.p[pb + Z], a.d[ob], a.d[ob + Z], a.mode == 0 ? a.eps[i] : 0.f, a.mode == 2 ? a.z[i] : 0.f,
                                 a.dz ? a.dz[i] : 0.f, G_lp, G_lq, G_an, a.mode);
    dp[ob] = g.pmu;
    dp[ob + Z] = g.plv;
    dd[ob] = g.dmu;
    dd[ob + Z] = g.dlv;
  }
}

// 16-byte map of the backward (Z % 4 == 0 and 16-byte aligned tensors): 4 consecutive channels of a pixel per thread, grid-stride
__global__ __launch_bounds__(256) void stoch_res_bwd_v4_kernel(StochResBwdArgs a, float* __restrict__ dp, float* __restrict__ dd) {
  const int Z = a.Z, Z4 = Z >> 2;
  const int64_t per4 = (int64_t)a.HW * Z4, total4 = per4 * a.N;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
    const int n = (int)(i / per4);
    const int e = (int)(i - (int64_t)n * per4);
    const int pix = e / Z4, c = (e - pix * Z4) * 4;
    const size_t pb = ((a.p_bcast ? 0 : (size_t)n * a.HW) + pix) * 2 * Z + c, ob = ((size_t)n * a.HW + pix) * 2 * Z + c;
    const size_t zi = ((size_t)n * a.HW + pix) * Z + c;
    const f32x4 pmu = *reinterpret_cast<const f32x4*>(a.p + pb), plv = *reinterpret_cast<const f32x4*>(a.p + pb + Z);
    const f32x4 dmu = *reinterpret_cast<const f32x4*>(a.d + ob), dlv = *reinterpret_cast<const f32x4*>(a.d + ob + Z);
    const f32x4 ev = a.mode == 0 ? *reinterpret_cast<const f32x4*>(a.eps + zi) : zero4;
    const f32x4 zv = a.mode == 2 ? *reinterpret_cast<const f32x4*>(a.z + zi) : zero4;
    const f32x4 dzv = a.dz ? *reinterpret_cast<const f32x4*>(a.dz + zi) : zero4;
    float G_lp, G_lq, G_an;
    res_weights(a, n, pix, G_lp, G_lq, G_an);
    f32x4 o_pmu, o_plv, o_dmu, o_dlv;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const ResGrads g = res_grads(pmu[j], plv[j], dmu[j], dlv[j], ev[j], zv[j], dzv[j], G_lp, G_lq, G_an, a.mode);
      o_pmu[j] = g.pmu;
      o_plv[j] = g.plv;
      o_dmu[j] = g.dmu;
      o_dlv[j] = g.dlv;
    }
    *reinterpret_cast<f32x4*>(dp + ob) = o_pmu;
    *reinterpret_cast<f32x4*>(dp + ob + Z) = o_plv;
    *reinterpret_cast<f32x4*>(dd + ob) = o_dmu;
    *reinterpret_cast<f32x4*>(dd + ob + Z) = o_dlv;
  }
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
