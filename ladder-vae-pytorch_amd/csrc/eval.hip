// Test-pass metrics (the reference's test summaries: ELBO, recons, KL, per-layer KL and the importance-weighted bound) folded on the
// device. Per image, S samples are folded online into double state; a finished batch is then reduced by ONE workgroup in a fixed order
// into a double accumulator, so a whole test pass costs one device-to-host copy and its totals are reproducible bit for bit.
#include "lvae_common.h"

namespace lvae {

// state (double): [0,N) running max of elbo_sep, [N,2N) sum of exp(elbo - max), [2N,3N) sum of elbo, [3N,4N) sum of -ll,
// [4N,5N) sum of kl_sep, [5N,5N+L) sum over samples of kl_avg_layerwise[l] * N (the per-layer KL summed over the batch).
//   mode 0: initialise;  mode 1: fold in one sample
__global__ __launch_bounds__(256) void eval_online_kernel(const float* __restrict__ elbo, const float* __restrict__ ll,
                                                          const float* __restrict__ kl_sep, const float* __restrict__ kl_avg,
                                                          double* __restrict__ state, int N, int L, int mode) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (blockIdx.x == 0)
    for (int l = threadIdx.x; l < L; l += 256) state[5 * (size_t)N + l] = mode == 0 ? 0.0 : state[5 * (size_t)N + l] + (double)kl_avg[l] * (double)N;
  if (n >= N) return;
  if (mode == 0) {
    state[n] = -INFINITY;
    for (int k = 1; k < 5; ++k) state[(size_t)k * N + n] = 0.0;
    return;
  }
  const double e = (double)elbo[n], m0 = state[n], m1 = fmax(m0, e);
  state[N + n] = state[N + n] * exp(m0 - m1) + exp(e - m1);   // exp(-inf) = 0 on the first sample
  state[n] = m1;
  state[2 * (size_t)N + n] += e;
  state[3 * (size_t)N + n] += -(double)ll[n];
  state[4 * (size_t)N + n] += (double)kl_sep[n];
}

// totals (double) += [sum_n iw[n], sum_n elbo[n], sum_n recons[n], sum_n kl[n], N, per-layer KL sums [L]], each per-image value being
// the mean over the S samples (iw[n] = max + log(sumexp) - log S). One workgroup, fixed reduction order, no atomics.
__global__ __launch_bounds__(256) void eval_totals_kernel(const double* __restrict__ state, int N, int L, int S, double* totals) {
  __shared__ double red[4][256];
  const int t = threadIdx.x;
  const double inv_s = 1.0 / (double)S, log_s = log((double)S);
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  for (int n = t; n < N; n += 256) {
    a[0] += state[n] + log(state[N + n]) - log_s;
    a[1] += state[2 * (size_t)N + n] * inv_s;
    a[2] += state[3 * (size_t)N + n] * inv_s;
    a[3] += state[4 * (size_t)N + n] * inv_s;
  }
  for (int k = 0; k < 4; ++k) red[k][t] = a[k];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s)
      for (int k = 0; k < 4; ++k) red[k][t] += red[k][t + s];
    __syncthreads();
  }
  if (t < 4) totals[t] += red[t][0];
  if (t == 4) totals[4] += (double)N;
  for (int l = t; l < L; l += 256) totals[5 + l] += state[5 * (size_t)N + l] * inv_s;
}

}  // namespace lvae

using namespace lvae;

extern "C" int lvae_eval_online_f32(const float* elbo_sep, const float* ll, const float* kl_sep, const float* kl_avg_layerwise,
                                    double* state, int32_t N, int32_t L, int32_t mode, void* stream) {
  LVAE_REQUIRE(state && N > 0 && L > 0 && (mode == 0 || mode == 1), LVAE_EINVAL, "lvae_eval_online_f32: bad args");
  LVAE_REQUIRE(mode == 0 || (elbo_sep && ll && kl_sep && kl_avg_layerwise), LVAE_EINVAL, "lvae_eval_online_f32: inputs missing");
  hipLaunchKernelGGL(eval_online_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, elbo_sep, ll, kl_sep,
                     kl_avg_layerwise, state, N, L, mode);
  LVAE_LAUNCH_CHECK("eval_online");
  return 0;
}

extern "C" int lvae_eval_totals_f64(const double* state, int32_t N, int32_t L, int32_t S, double* totals, void* stream) {
  LVAE_REQUIRE(state && totals && N > 0 && L > 0 && S > 0, LVAE_EINVAL, "lvae_eval_totals_f64: bad args");
  hipLaunchKernelGGL(eval_totals_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, state, N, L, S, totals);
  LVAE_LAUNCH_CHECK("eval_totals");
  return 0;
}
