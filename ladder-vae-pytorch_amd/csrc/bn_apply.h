// The BatchNorm-backward apply as the fused backward launches form it themselves (gfx950 only): dx = BN'(dh; x) [* drop] [+ add] from the
// partial rows a producer's statistics epilogue left (bn_stats.h), described by a lvae_bn_apply. ONE definition of the value, of the
// coefficient rows a 512-thread workgroup keeps in LDS and of the reduction that fills them: the launches that take an apply must agree
// bit for bit with each other and with the stand-alone apply (norm_act.hip).
#pragma once
#include "bn_stats.h"

namespace lvae {

// The six coefficients of channels c .. c + 3, and dx of those channels without the launch's own `* drop` / `+ add`
struct ApRows {
  f32x4 sc, sh, mu, rs, c1, c2;  // scale, shift, mean, rstd of the forward; mean(g), mean(g xhat) of the backward
};
__device__ __forceinline__ f32x4 ap_value4(const ApRows& k, f32x4 dh, f32x4 x, int act) {
  return bn_bwd_apply(dh * act_grad4(x * k.sc + k.sh, act), x, k.c1, k.c2, k.mu, k.rs, k.sc);
}

// ---- the coefficient rows of a 64-channel apply in LDS, Cf [6][64] floats: the block ap.coef [4][64], then c1 and c2
constexpr int AP_SCALE = 0, AP_SHIFT = 64, AP_MEAN = 128, AP_RSTD = 192, AP_C1 = 256, AP_C2 = 320, AP_CF = 384;

__device__ __forceinline__ ApRows ap_rows(const float* Cf, int c) {
  const auto row = [&](int at) { return *reinterpret_cast<const f32x4*>(Cf + at + c); };
  return ApRows{row(AP_SCALE), row(AP_SHIFT), row(AP_MEAN), row(AP_RSTD), row(AP_C1), row(AP_C2)};
}
__device__ __forceinline__ f32x4 ap_value4(const float* Cf, f32x4 dh, f32x4 x, int c, int act) { return ap_value4(ap_rows(Cf, c), dh, x, act); }

// The 512-thread reduction of ap.parts [rows][2][64] into Cf. Thread (q = t & 31, rg = t >> 5) sums rows rg + 16 u + 128 k (8 independent
// 16-byte loads in flight; rows past the end read row 0 and are not added) into scr [16][128]; threads 0..63 add the 16 groups in double
// and finish. The workgroup with `writes_params` (one of the launch) accumulates dgamma / dbeta. scr must be dead; it is free again on
// return. (conv3x3_wgrad_wino_body.inc keeps a copy of this, word for word: see there.)
__device__ __forceinline__ void ap_reduce(const lvae_bn_apply& ap, float* scr, float* Cf, bool writes_params) {
  const int t = threadIdx.x, q = t & 31, rg = t >> 5, rows = ap.rows;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int r = rg; r < rows; r += 16 * 8) {
    f32x4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int rr = r + 16 * u;
      v[u] = *reinterpret_cast<const f32x4*>(ap.parts + (size_t)(rr < rows ? rr : 0) * 128 + q * 4);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (r + 16 * u < rows) acc += v[u];
  }
  *reinterpret_cast<f32x4*>(scr + rg * 128 + q * 4) = acc;
  if (t < 256) Cf[t] = ap.coef[t];
  __syncthreads();
  if (t < 64) {
    double sa = 0.0, sb = 0.0;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      sa += (double)scr[g * 128 + t];
      sb += (double)scr[g * 128 + 64 + t];
    }
    const BnBwdChannel r = bn_bwd_finish(sa, sb, ap.M);
    Cf[AP_C1 + t] = r.c1;
    Cf[AP_C2 + t] = r.c2;
    if (writes_params) {
      if (ap.dbeta) ap.dbeta[t] += r.dbeta;
      if (ap.dgamma) ap.dgamma[t] += r.dgamma;
    }
  }
  __syncthreads();  // scr is read and Cf is published
}

}  // namespace lvae
