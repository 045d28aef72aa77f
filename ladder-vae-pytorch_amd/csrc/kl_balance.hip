// KL balancing over the layers of the ladder during the KL warm-up (NVAE §3.2): the bookkeeping of misc.hip (kl_book_fwd_kernel /
// kl_book_bwd_kernel) with a per-layer coefficient gamma_l on the terms of kl_loss, decided on the device from the step's own beta.
//
//   m_l     = (1/N) sum_n |kl[l][n]| + 0.01
//   gamma_l = (m_l / alpha_l) / ((1/L) sum_j m_j / alpha_j)      while beta < 1, else 1
//   kl_loss = sum_l gamma_l * (1/N) sum_n c(kl[l][n])            c: the free-bits clamp of kl_book_fwd_kernel
//
// NVAE's code multiplies by sum_j m_j before it normalises to mean 1; the factor cancels in the quotient and is left out. gamma is a
// constant of the gradient: the backward reads it from `coeff` and never forms it again.
//
// The forward is one workgroup, like kl_book_fwd_kernel. The per-layer sums of kl and of c(kl) are formed in that kernel's order with the
// same block_sum_256, so kl_avg_layerwise, kl_sep and kl carry its bits; the sum of |kl| is a third block_sum_256 per layer. The L-element
// part (m_l / alpha_l, their mean, gamma_l) is double, rounded to float once. It takes two sweeps over the matrix (the mean needs every
// layer before the first gamma): the second sweep forms a layer's |kl| sum again, with the same bits, which keeps L unbounded and the LDS
// at four floats. With beta >= 1 gamma_l is the constant 1.0f by a select, and 1.0f * x is x: every output then has the bits of the
// plain bookkeeping, forward and backward. No atomics anywhere.
#include "lvae_common.h"

namespace lvae {

constexpr double kKlBalanceFloor = 0.01;   // keeps a dead layer's coefficient finite (NVAE: kl_balancer_coeff)

__device__ __forceinline__ double kl_balance_q(float sum_abs, int N, float alpha) {
  return ((double)sum_abs / (double)N + kKlBalanceFloor) / (double)alpha;
}

__global__ __launch_bounds__(256) void kl_balance_fwd_kernel(const float* __restrict__ kl, int L, int N, float free_bits,
                                                              const float* __restrict__ alpha, float beta, const int64_t* step,
                                                              int64_t anneal_steps, float* kl_sep, float* kl_avg, float* scalars,
                                                              float* coeff) {
  __shared__ float red[4];
  const int t = threadIdx.x;
  const bool active = (step ? anneal_beta(step, anneal_steps) : beta) < 1.f;
  // sweep 1: the mean of m_l / alpha_l (every thread holds the same block sums, so every thread holds the same double)
  double qsum = 0.0;
  for (int l = 0; l < L; ++l) {
    float sa = 0.f;
    for (int n = t; n < N; n += 256) sa += fabsf(kl[(size_t)l * N + n]);
    sa = block_sum_256(sa, red);
    qsum += kl_balance_q(sa, N, alpha[l]);
  }
  const double qmean = qsum / (double)L;
  // sweep 2: kl_book_fwd_kernel's sums, and the layer's coefficient on its term of kl_loss
  float kl_loss = 0.f;
  for (int l = 0; l < L; ++l) {
    float s = 0.f, sc = 0.f, sa = 0.f;
    for (int n = t; n < N; n += 256) {
      const float v = kl[(size_t)l * N + n];
      s += v;
      sc += free_bits < 1e-6f ? v : fmaxf(v, free_bits);
      sa += fabsf(v);
    }
    s = block_sum_256(s, red);
    sc = block_sum_256(sc, red);
    sa = block_sum_256(sa, red);
    const float g = active ? (float)(kl_balance_q(sa, N, alpha[l]) / qmean) : 1.0f;
    if (t == 0) {
      kl_avg[l] = s / (float)N;
      coeff[l] = g;
    }
    kl_loss += g * (sc / (float)N);
  }
  float tot = 0.f;
  for (int n = t; n < N; n += 256) {
    float s = 0.f;
    for (int l = 0; l < L; ++l) s += kl[(size_t)l * N + n];
    kl_sep[n] = s;
    tot += s;
  }
  tot = block_sum_256(tot, red);
  if (t == 0) {
    scalars[0] = kl_loss;
    scalars[1] = tot / (float)N;
  }
}

__global__ __launch_bounds__(256) void kl_balance_bwd_kernel(const float* __restrict__ kl, int L, int N, float free_bits,
                                                              const float* __restrict__ coeff, const float* g_sep, const float* g_avg,
                                                              const float* g_scalars, float* __restrict__ dkl) {
  const float g_loss = g_scalars ? g_scalars[0] : 0.f, g_kl = g_scalars ? g_scalars[1] : 0.f;
  const float invn = 1.f / (float)N;
  const int64_t total = (int64_t)L * N;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int l = (int)(i / N), n = (int)(i - (int64_t)l * N);
    float g = g_kl * invn;
    if (g_sep) g += g_sep[n];
    if (g_avg) g += g_avg[l] * invn;
    if (free_bits < 1e-6f || kl[i] >= free_bits) g += coeff[l] * g_loss * invn;
    dkl[i] = g;
  }
}

}  // namespace lvae

using namespace lvae;

extern "C" int lvae_kl_balance_fwd_f32(const float* kl, int32_t L, int32_t N, float free_bits, const float* alpha, float beta,
                                       const int64_t* step, int64_t anneal_steps, float* kl_sep, float* kl_avg_layerwise,
                                       float* scalars, float* coeff, void* stream) {
  LVAE_REQUIRE(kl && alpha && kl_sep && kl_avg_layerwise && scalars && coeff && L > 0 && N > 0, LVAE_EINVAL,
               "lvae_kl_balance_fwd_f32: bad args");
  hipLaunchKernelGGL(kl_balance_fwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, kl, L, N, free_bits, alpha, beta, step,
                     anneal_steps, kl_sep, kl_avg_layerwise, scalars, coeff);
  LVAE_LAUNCH_CHECK("kl_balance_fwd");
  return 0;
}

extern "C" int lvae_kl_balance_bwd_f32(const float* kl, int32_t L, int32_t N, float free_bits, const float* coeff, const float* g_sep,
                                       const float* g_avg, const float* g_scalars, float* dkl, void* stream) {
  LVAE_REQUIRE(kl && coeff && dkl && L > 0 && N > 0, LVAE_EINVAL, "lvae_kl_balance_bwd_f32: bad args");
  hipLaunchKernelGGL(kl_balance_bwd_kernel, dim3(grid_for((int64_t)L * N, 256)), dim3(256), 0, (hipStream_t)stream, kl, L, N,
                     free_bits, coeff, g_sep, g_avg, g_scalars, dkl);
  LVAE_LAUNCH_CHECK("kl_balance_bwd");
  return 0;
}
