// The BatchNorm and statistics arithmetic every kernel shares (gfx950 only): ONE definition per formula. Training is deterministic and a
// resumed run continues bit for bit, so a kernel that folds one of these steps and one that does not must produce identical bits.
//
// Partial rows. A producer's statistics epilogue writes one row [2][C] per workgroup: (sum dl, sum dl^2) of dl = value - pivot
// (LVAE_STATS_BN_FWD), or (sum g, sum g * xhat) of the BatchNorm-backward reduction (LVAE_STATS_BN_BWD). The pivot row follows the
// forward rows. A consumer sums the rows in an order of its own (its load schedule), in double across its groups, and finishes here.
#pragma once
#include "lvae_common.h"

namespace lvae {

// ---- BatchNorm finalize of one channel from its pivoted sums sa = sum (x - pivot), sb = sum (x - pivot)^2 over M values
struct BnChannel {
  float scale, shift, mean, rstd;
  double m2, var;  // sum (x - mean)^2 (clamped at 0) and the biased variance: what the running variance is formed from
};
__device__ __forceinline__ BnChannel bn_finalize_channel(double sa, double sb, float pivot, int64_t M, float eps, float gamma, float beta) {
  const double inv_m = 1.0 / (double)M, dm = sa * inv_m;  // dm = mean - pivot
  BnChannel r;
  r.m2 = sb - sa * dm;
  if (r.m2 < 0.0) r.m2 = 0.0;
  const double mean = (double)pivot + dm;
  r.var = r.m2 * inv_m;
  r.rstd = (float)(1.0 / sqrt(r.var + (double)eps));
  r.scale = gamma * r.rstd;
  r.shift = beta - (float)mean * r.scale;
  r.mean = (float)mean;
  return r;
}
// the variance with the M - 1 divisor (the biased one when M == 1): a double division, so only the one writer of a launch asks for it
__device__ __forceinline__ float bn_unbiased_var(const BnChannel& r, int64_t M) { return (float)(M > 1 ? r.m2 / ((double)M - 1.0) : r.var); }
// the [4][C] coefficient block the backward reads: scale, shift, mean, rstd
__device__ __forceinline__ void bn_store_coef(float* coef_out, int C, int c, const BnChannel& r) {
  coef_out[c] = r.scale;
  coef_out[C + c] = r.shift;
  coef_out[2 * C + c] = r.mean;
  coef_out[3 * C + c] = r.rstd;
}
// momentum update of the running statistics from their previous values rm0 / rv0
__device__ __forceinline__ void bn_update_running(float* running_mean, float* running_var, int c, float rm0, float rv0, float momentum,
                                                  const BnChannel& r, int64_t M) {
  running_mean[c] = (1.f - momentum) * rm0 + momentum * r.mean;
  running_var[c] = (1.f - momentum) * rv0 + momentum * bn_unbiased_var(r, M);
}

// ---- BatchNorm backward: from sa = sum g, sb = sum g * xhat over M values to the two means of the apply and the parameter gradients
// (dbeta / dgamma: what one workgroup of the launch adds to them), and dx = (g - c1 - xhat * c2) * scale, for float or f32x4 operands
struct BnBwdChannel {
  float c1, c2, dbeta, dgamma;
};
template <typename Int>
__device__ __forceinline__ BnBwdChannel bn_bwd_finish(double sa, double sb, Int M) {
  return BnBwdChannel{(float)(sa / (double)M), (float)(sb / (double)M), (float)sa, (float)sb};
}
template <typename T>
__device__ __forceinline__ T bn_bwd_apply(T g, T x, T c1, T c2, T mean, T rstd, T scale) {
  return (g - c1 - (x - mean) * rstd * c2) * scale;
}

// ---- statistics epilogue of the convolution kernels: four channels per lane
// coefficients of channels col .. col + 3 from d.stats_pivot, a [Cout] pivot row (forward) or the [4][Cout] block of bn_store_coef
// (backward: piv = scale, then shift, mean, rstd); zero where the lane is off (`on`: statistics wanted) or its channels are past Cout
__device__ __forceinline__ void stats_load_coef4(const float* block, int Cout, int col, bool on, bool bwd, f32x4& piv, f32x4& bsh, f32x4& bmu,
                                                 f32x4& brs) {
  piv = f32x4{0.f, 0.f, 0.f, 0.f};
  if (on && col < Cout) piv = *reinterpret_cast<const f32x4*>(block + col);
  bsh = bmu = brs = piv;
  if (on && bwd && col < Cout) {
    bsh = *reinterpret_cast<const f32x4*>(block + Cout + col);
    bmu = *reinterpret_cast<const f32x4*>(block + 2 * Cout + col);
    brs = *reinterpret_cast<const f32x4*>(block + 3 * Cout + col);
  }
}
// LVAE_STATS_BN_FWD: pivoted sum and sum of squares of the stored values
__device__ __forceinline__ void stats_fwd_accum4(f32x4 v, f32x4 piv, f32x4& st1, f32x4& st2) {
  const f32x4 dl = v - piv;
  st1 += dl;
  st2 += dl * dl;
}
// LVAE_STATS_BN_BWD: v = gradient w.r.t. act(BN(x)), xv = that BatchNorm's input; sums of g = v * act'(x * scale + shift) and of g * xhat
__device__ __forceinline__ void stats_bwd_accum4(f32x4 v, f32x4 xv, f32x4 scale, f32x4 shift, f32x4 mean, f32x4 rstd, int act, f32x4& st1,
                                                 f32x4& st2) {
  const f32x4 ag = act_grad4(xv * scale + shift, act);
#pragma unroll
  for (int j = 0; j < 4; ++j) {  // element by element: the files compiled without the SLP vectorizer keep scalar instructions
    const float gj = v[j] * ag[j];
    st1[j] += gj;
    st2[j] += gj * (xv[j] - mean[j]) * rstd[j];
  }
}
// PG pixel groups x CW channels -> one row of partials per workgroup, summed in a fixed order. Thread (group, channels cv .. cv + 4 NV - 1
// of the workgroup's CW) hands in its sums; `red` = 2 * PG * CW floats of LDS whose contents are dead by now. The sums go to row `row`
// of stats_out [rows][2][Cout] at channel co0; channels past Cout are dropped.
// store_pivot (one workgroup of the launch): the pivot row is stored behind the pivot_row partial rows. It travels with the
// partials because a consumer that finalizes them in its own prologue (lvae_bn_fold) must not read running_mean, which it updates.
template <int PG, int CW, int NV>
__device__ __forceinline__ void stats_reduce_groups(float* red, int group, int cv, const f32x4 (&st1)[NV], const f32x4 (&st2)[NV],
                                                    float* stats_out, size_t row, int Cout, int co0, bool store_pivot, const float* pivot,
                                                    size_t pivot_row) {
  const int t = threadIdx.x;
  __syncthreads();
#pragma unroll
  for (int h = 0; h < NV; ++h) {
    *reinterpret_cast<f32x4*>(red + group * CW + cv + 4 * h) = st1[h];
    *reinterpret_cast<f32x4*>(red + PG * CW + group * CW + cv + 4 * h) = st2[h];
  }
  __syncthreads();
  if (t < 2 * CW) {
    const int c = t % CW, which = t / CW;
    float v = 0.f;
#pragma unroll
    for (int r = 0; r < PG; ++r) v += red[which * PG * CW + r * CW + c];
    if (co0 + c < Cout) {
      stats_out[(row * 2 + which) * Cout + co0 + c] = v;
      if (store_pivot && which == 0) stats_out[(pivot_row * 2) * Cout + co0 + c] = pivot[co0 + c];
    }
  }
}
template <int PG, int CW>
__device__ __forceinline__ void stats_reduce_groups(float* red, int group, int cv, f32x4 st1, f32x4 st2, float* stats_out, size_t row, int Cout,
                                                    int co0, bool store_pivot, const float* pivot, size_t pivot_row) {
  const f32x4 s1[1] = {st1}, s2[1] = {st2};
  stats_reduce_groups<PG, CW, 1>(red, group, cv, s1, s2, stats_out, row, Cout, co0, store_pivot, pivot, pivot_row);
}

}  // namespace lvae
