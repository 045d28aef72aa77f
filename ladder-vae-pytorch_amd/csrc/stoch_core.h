// The elementwise core of NormalStochasticBlock2d (lib/stochastic.py:45-99, 209-226), written once: the arithmetic of one element in its
// two forms, the upstream weights of the backward, and the four thread maps of the stand-alone kernels as templates over an element
// policy. stochastic.hip (absolute posterior) and stochastic_residual.hip (posterior as an offset from the prior) instantiate the maps;
// the fused block of the small levels (stoch_img.hip) has a map of its own, its tile's, and calls the absolute element functions.
// The library is built with -ffp-contract=off and without fast-math: the order of operations written here is the order that runs.
#pragma once
#include "lvae_common.h"

namespace lvae {

// One element of the forward. kl: the term of kl_samplewise (analytical or Monte Carlo); kan: always the analytical one (kl_spatial).
struct StochTerms {
  float z, lp, lq, kan, kl;
};

// One element of the backward: the gradients of the prior's (mu, logvar) and of the second operand's, s = q (absolute) or d (residual).
struct StochGrads {
  float pmu, plv, smu, slv;
};

// ---------------------------------------------------------------------------------------------------------------------------
// absolute form: q = (qmu | qlv) are the posterior's own parameters; e = eps (mode 0) or the forced latent (mode 2)
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ StochTerms abs_terms(float pmu, float plv, float qmu, float qlv, float e, int mode, int analytical) {
  StochTerms r;
  if (mode == 0) r.z = qmu + expf(0.5f * qlv) * e;
  else if (mode == 1) r.z = qmu;
  else r.z = e;  // forced latent is passed through the eps pointer
  r.lp = normal_logprob(r.z, pmu, plv);
  r.lq = normal_logprob(r.z, qmu, qlv);
  r.kan = normal_kl(qmu, qlv, pmu, plv);
  r.kl = analytical ? r.kan : (r.lq - r.lp);
  return r;
}

// without a posterior: z is drawn from p and only log p(z) exists
__device__ __forceinline__ StochTerms abs_terms_prior(float pmu, float plv, float e, int mode) {
  StochTerms r = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (mode == 0) r.z = pmu + expf(0.5f * plv) * e;
  else if (mode == 1) r.z = pmu;
  else r.z = e;
  r.lp = normal_logprob(r.z, pmu, plv);
  return r;
}

// G_lp, G_lq, G_an: the upstream weights of log p, log q and the analytical KL of this element (stoch_weights); e = eps (mode 0)
__device__ __forceinline__ StochGrads abs_grads(float pmu, float plv, float qmu, float qlv, float e, float z, float dzu, float G_lp,
                                                float G_lq, float G_an, int mode) {
  const float ivp = expf(-plv);  // 1/sigma_p^2
  const float dpz = z - pmu;
  const float ivq = expf(-qlv);
  const float dqz = z - qmu;
  const float Gz = dzu - G_lp * dpz * ivp - G_lq * dqz * ivq;
  const float dmu = qmu - pmu;
  const float vr = expf(qlv - plv);
  StochGrads g;
  g.pmu = G_lp * dpz * ivp - G_an * dmu * ivp;
  g.plv = G_lp * 0.5f * (dpz * dpz * ivp - 1.f) + G_an * 0.5f * (1.f - vr - dmu * dmu * ivp);
  g.smu = G_lq * dqz * ivq + G_an * dmu * ivp;
  g.slv = G_lq * 0.5f * (dqz * dqz * ivq - 1.f) + G_an * 0.5f * (vr - 1.f);
  if (mode <= 1) g.smu += Gz;
  if (mode == 0) g.slv += Gz * 0.5f * expf(0.5f * qlv) * e;
  return g;
}

// without a posterior: glp is the upstream gradient of logprob_p itself
__device__ __forceinline__ StochGrads abs_grads_prior(float pmu, float plv, float e, float z, float dzu, float glp, int mode) {
  const float ivp = expf(-plv);
  const float dpz = z - pmu;
  const float Gz = dzu - glp * dpz * ivp;
  StochGrads g = {glp * dpz * ivp, glp * 0.5f * (dpz * dpz * ivp - 1.f), 0.f, 0.f};
  if (mode <= 1) g.pmu += Gz;
  if (mode == 0) g.plv += Gz * 0.5f * expf(0.5f * plv) * e;
  return g;
}

// The upstream weights of one element from the gradients of logprob_p, logprob_q, kl_samplewise (per sample) and kl_spatial (per pixel):
// the Monte-Carlo KL is log q - log p, the analytical one a term of its own.
__device__ __forceinline__ void stoch_weights(float glp, float glq, float gkl, float gks, int analytical, float& G_lp, float& G_lq,
                                              float& G_an) {
  G_lp = glp - (analytical ? 0.f : gkl);
  G_lq = glq + (analytical ? 0.f : gkl);
  G_an = gks + (analytical ? gkl : 0.f);
}

// ---------------------------------------------------------------------------------------------------------------------------
// residual form: mu_q = mu_p + dmu, logvar_q = logvar_p + dlv (the derivation is in front of stochastic_residual.hip)
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float res_kan(float dmu, float dlv, float ivp) { return 0.5f * (expm1f(dlv) - dlv + dmu * dmu * ivp); }

// one element of the forward; e = eps (mode 0) or the forced latent (mode 2)
__device__ __forceinline__ StochTerms res_terms(float pmu, float plv, float dmu, float dlv, float e, int mode, int analytical) {
  const float sp = expf(0.5f * plv);
  const float sq = sp * expf(0.5f * dlv);   // a product, not exp of the sum: d = 0 gives the prior's own sigma, bit for bit
  const float ivp = expf(-plv);
  StochTerms r;
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
  r.kan = res_kan(dmu, dlv, ivp);
  r.kl = analytical ? r.kan : 0.5f * (ap - uu) - 0.5f * dlv;
  return r;
}

// smu / slv: the gradient of the offset; pmu / plv: the TOTAL gradient of the prior parameters (their own terms plus what flows through
// q = p + d). e = eps (mode 0); z read in mode 2 only
__device__ __forceinline__ StochGrads res_grads(float pmu, float plv, float dmu, float dlv, float e, float z, float dzu, float G_lp,
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
  StochGrads g;
  g.slv = lq_lv + G_an * 0.5f * expm1f(dlv);
  g.plv = G_lp * 0.5f * (a * a * ivp - 1.f) + lq_lv - 0.5f * k_mu * dmu;
  if (mode <= 1) {
    const float Gz = dzu - t_lp;   // everything that reaches z: the upstream gradient and log p's own (log q's: none, u is constant)
    g.pmu = dzu;
    g.smu = Gz + k_mu;
    if (mode == 0) {
      const float w = Gz * 0.5f * sq * e;
      g.plv += w;
      g.slv += w;
    }
  } else {
    g.pmu = t_lp + qterm;
    g.smu = qterm + k_mu;
  }
  return g;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The thread maps. A policy P supplies
//   second(a)                     the second operand of an argument block (q or d), [N][HW][2Z]
//   terms / terms_prior           one element of the forward (terms_prior only where kSecondOptional)
//   grads / grads_prior           one element of the backward
//   kan(pmu, plv, smu, slv)       one element's analytical KL, for the per-pixel loop of a Z that the shuffles do not cover
//   needs_z(mode)                 whether the backward reads z in this mode
//   kSecondOptional               the second operand may be null: the prior-only block (z from p, logprob_p alone)
//   kWritesQ                      a q_out = p + s tensor is written where the caller passes one
// Forward: one 256-thread workgroup per sample; the Z channels of a pixel are contiguous (NHWC), so the per-pixel KL is a shuffle
// reduction over the lanes of a pixel, in which every lane of a wave takes part. Backward: grid-stride over the batch.
// ---------------------------------------------------------------------------------------------------------------------------
template <class P>
__device__ __forceinline__ StochTerms stoch_terms(bool has_s, float pmu, float plv, float smu, float slv, float e, int mode,
                                                  int analytical) {
  if constexpr (P::kSecondOptional)
    if (!has_s) return P::terms_prior(pmu, plv, e, mode);
  return P::terms(pmu, plv, smu, slv, e, mode, analytical);
}

// the per-sample sums of a forward workgroup: block_sum_256 of each, in this order
__device__ __forceinline__ void stoch_store_sums(bool has_s, int n, float s_lp, float s_lq, float s_kl, float* logprob_p,
                                                 float* logprob_q, float* kl_samplewise) {
  __shared__ float red[4];
  s_lp = block_sum_256(s_lp, red);
  if (threadIdx.x == 0) logprob_p[n] = s_lp;
  if (has_s) {
    s_lq = block_sum_256(s_lq, red);
    s_kl = block_sum_256(s_kl, red);
    if (threadIdx.x == 0) {
      logprob_q[n] = s_lq;
      kl_samplewise[n] = s_kl;
    }
  }
}

// forward, scalar map: one element per thread and pass
template <class P, class A>
__device__ __forceinline__ void stoch_fwd_map(const A& a, float* __restrict__ z_out, float* __restrict__ q_out, float* logprob_p,
                                              float* logprob_q, float* kl_samplewise, float* kl_spatial) {
  const int n = blockIdx.x, t = threadIdx.x;
  const int Z = a.Z, per = a.HW * Z;
  const bool has_s = !P::kSecondOptional || P::second(a) != nullptr;
  const float* pn = a.p + (a.p_bcast ? 0 : (size_t)n * a.HW * 2 * Z);
  const float* sn = has_s ? P::second(a) + (size_t)n * a.HW * 2 * Z : nullptr;
  float* qo = P::kWritesQ && q_out ? q_out + (size_t)n * a.HW * 2 * Z : nullptr;
  const bool zpow2 = (Z & (Z - 1)) == 0 && Z <= 64;
  float s_lp = 0.f, s_lq = 0.f, s_kl = 0.f;
  // iterate in whole 256-element passes so that every lane of a wave takes part in the shuffles
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
      const float pmu = pn[b], plv = pn[b + Z], smu = has_s ? sn[b] : 0.f, slv = has_s ? sn[b + Z] : 0.f;
      const size_t zi = (size_t)n * per + e;
      const StochTerms r = stoch_terms<P>(has_s, pmu, plv, smu, slv, a.mode != 1 ? a.eps[zi] : 0.f, a.mode, a.analytical);
      z_out[zi] = r.z;
      if (qo) {
        qo[b] = pmu + smu;
        qo[b + Z] = plv + slv;
      }
      s_lp += r.lp;
      s_lq += r.lq;
      s_kl += r.kl;
      kan = r.kan;
    }
    if (has_s && kl_spatial && zpow2) {
      float v = kan;
      for (int o = Z >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (ok && (e % Z) == 0) kl_spatial[(size_t)n * a.HW + pix] = v;
    }
  }
  if (has_s && kl_spatial && !zpow2) {
    for (int pix = t; pix < a.HW; pix += 256) {
      float v = 0.f;
      for (int c = 0; c < Z; ++c) {
        const size_t b = (size_t)pix * 2 * Z + c;
        v += P::kan(pn[b], pn[b + Z], sn[b], sn[b + Z]);
      }
      kl_spatial[(size_t)n * a.HW + pix] = v;
    }
  }
  stoch_store_sums(has_s, n, s_lp, s_lq, s_kl, logprob_p, logprob_q, kl_samplewise);
}

// forward, 16-byte map, for Z a multiple of 4 with Z / 4 a power of two <= 16 (every model of BASELINE.json: Z = 32) and 16-byte aligned
// tensors: a thread takes 4 consecutive channels of a pixel (16-byte loads / stores), two 1,024-element passes are in flight per
// iteration, the per-pixel KL is a shuffle reduction over the Z / 4 lanes of a pixel. The scalar map issues one dependent round trip
// per 256 elements from ONE workgroup per sample: 32 round trips at 16x16 x 32 (measured 19 us per launch averaged over the 15 levels of
// the CIFAR model, ~45 us at the 16x16 levels, for 50 MB = 10 us of HBM time).
template <class P, class A>
__device__ __forceinline__ void stoch_fwd_v4_map(const A& a, float* __restrict__ z_out, float* __restrict__ q_out, float* logprob_p,
                                                 float* logprob_q, float* kl_samplewise, float* kl_spatial) {
  const int n = blockIdx.x, t = threadIdx.x;
  const int Z = a.Z, Z4 = Z >> 2, per4 = a.HW * Z4;   // 4-channel groups of this sample
  const bool has_s = !P::kSecondOptional || P::second(a) != nullptr;
  const float* pn = a.p + (a.p_bcast ? 0 : (size_t)n * a.HW * 2 * Z);
  const float* sn = has_s ? P::second(a) + (size_t)n * a.HW * 2 * Z : nullptr;
  const float* en = a.eps ? a.eps + (size_t)n * a.HW * Z : nullptr;
  float* zn = z_out + (size_t)n * a.HW * Z;
  float* qo = P::kWritesQ && q_out ? q_out + (size_t)n * a.HW * 2 * Z : nullptr;
  float s_lp = 0.f, s_lq = 0.f, s_kl = 0.f;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  constexpr int U = 2;
  for (int it = 0; it * 256 * U < per4; ++it) {
    f32x4 pmu[U], plv[U], smu[U], slv[U], ev[U];
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
      smu[u] = has_s ? *reinterpret_cast<const f32x4*>(sn + b) : zero4;
      slv[u] = has_s ? *reinterpret_cast<const f32x4*>(sn + b + Z) : zero4;
      ev[u] = a.mode != 1 ? *reinterpret_cast<const f32x4*>(en + (size_t)pix[u] * Z + c[u]) : zero4;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      f32x4 zv = zero4;
      float kan = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (ok[u]) {   // (a wave whose lanes are all past the end skips the arithmetic)
          const StochTerms r = stoch_terms<P>(has_s, pmu[u][j], plv[u][j], smu[u][j], slv[u][j], ev[u][j], a.mode, a.analytical);
          zv[j] = r.z;
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
          *reinterpret_cast<f32x4*>(qo + b) = pmu[u] + smu[u];
          *reinterpret_cast<f32x4*>(qo + b + Z) = plv[u] + slv[u];
        }
      }
      if (has_s && kl_spatial) {   // all lanes take part in the shuffles; the Z / 4 lanes of a pixel are consecutive
        float v = kan;
        for (int o = Z4 >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (ok[u] && c[u] == 0) kl_spatial[(size_t)n * a.HW + pix[u]] = v;
      }
    }
  }
  stoch_store_sums(has_s, n, s_lp, s_lq, s_kl, logprob_p, logprob_q, kl_samplewise);
}

// backward, scalar map: one element per thread, grid-stride. ds is null exactly where the second operand is.
template <class P, class A>
__device__ __forceinline__ void stoch_bwd_map(const A& a, float* __restrict__ dp, float* __restrict__ ds) {
  const int Z = a.Z;
  const int64_t per = (int64_t)a.HW * Z, total = per * a.N;
  const bool has_s = !P::kSecondOptional || P::second(a) != nullptr;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int n = (int)(i / per);
    const int e = (int)(i - (int64_t)n * per);
    const int pix = e / Z, c = e - pix * Z;
    const size_t pb = ((a.p_bcast ? 0 : (size_t)n * a.HW) + pix) * 2 * Z + c, ob = ((size_t)n * a.HW + pix) * 2 * Z + c;
    const float pmu = a.p[pb], plv = a.p[pb + Z];
    const float ev = a.mode == 0 ? a.eps[i] : 0.f, z = P::needs_z(a.mode) ? a.z[i] : 0.f, dzu = a.dz ? a.dz[i] : 0.f;
    const float glp = a.g_lp ? a.g_lp[n] : 0.f;
    if (has_s) {
      float G_lp, G_lq, G_an;
      stoch_weights(glp, a.g_lq ? a.g_lq[n] : 0.f, a.g_kl ? a.g_kl[n] : 0.f, a.g_ks ? a.g_ks[(size_t)n * a.HW + pix] : 0.f,
                    a.analytical, G_lp, G_lq, G_an);
      const StochGrads g = P::grads(pmu, plv, P::second(a)[ob], P::second(a)[ob + Z], ev, z, dzu, G_lp, G_lq, G_an, a.mode);
      dp[ob] = g.pmu;
      dp[ob + Z] = g.plv;
      ds[ob] = g.smu;
      ds[ob + Z] = g.slv;
    } else if constexpr (P::kSecondOptional) {
      const StochGrads g = P::grads_prior(pmu, plv, ev, z, dzu, glp, a.mode);
      dp[ob] = g.pmu;
      dp[ob + Z] = g.plv;
    }
  }
}

// backward, 16-byte map (Z % 4 == 0 and 16-byte aligned tensors): 4 consecutive channels of a pixel per thread, grid-stride. It has no
// prior-only branch: the absolute backward runs on the scalar map.
template <class P, class A>
__device__ __forceinline__ void stoch_bwd_v4_map(const A& a, float* __restrict__ dp, float* __restrict__ ds) {
  static_assert(!P::kSecondOptional, "the 16-byte backward map needs the second operand");
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
    const f32x4 smu = *reinterpret_cast<const f32x4*>(P::second(a) + ob), slv = *reinterpret_cast<const f32x4*>(P::second(a) + ob + Z);
    const f32x4 ev = a.mode == 0 ? *reinterpret_cast<const f32x4*>(a.eps + zi) : zero4;
    const f32x4 zv = P::needs_z(a.mode) ? *reinterpret_cast<const f32x4*>(a.z + zi) : zero4;
    const f32x4 dzv = a.dz ? *reinterpret_cast<const f32x4*>(a.dz + zi) : zero4;
    float G_lp, G_lq, G_an;
    stoch_weights(a.g_lp ? a.g_lp[n] : 0.f, a.g_lq ? a.g_lq[n] : 0.f, a.g_kl ? a.g_kl[n] : 0.f,
                  a.g_ks ? a.g_ks[(size_t)n * a.HW + pix] : 0.f, a.analytical, G_lp, G_lq, G_an);
    f32x4 o_pmu, o_plv, o_smu, o_slv;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const StochGrads g = P::grads(pmu[j], plv[j], smu[j], slv[j], ev[j], zv[j], dzv[j], G_lp, G_lq, G_an, a.mode);
      o_pmu[j] = g.pmu;
      o_plv[j] = g.plv;
      o_smu[j] = g.smu;
      o_slv[j] = g.slv;
    }
    *reinterpret_cast<f32x4*>(dp + ob) = o_pmu;
    *reinterpret_cast<f32x4*>(dp + ob + Z) = o_plv;
    *reinterpret_cast<f32x4*>(ds + ob) = o_smu;
    *reinterpret_cast<f32x4*>(ds + ob + Z) = o_slv;
  }
}

}  // namespace lvae
