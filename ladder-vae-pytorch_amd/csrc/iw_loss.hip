// Training on the K-sample importance-weighted bound (IWAE, Burda et al.): the loss head over [K][B] sample-major rows (row n = k*B + b,
// the layout of lvae_iw_logmeanexp_f32) and the broadcast of a bottom-up tensor over the K samples with its fixed-order sum going back.
#include "lvae_common.h"

namespace lvae {

// sum over a 256-thread block in a fixed order; result valid in every thread. `red` = 4 doubles of LDS.
__device__ __forceinline__ double block_sum_256_f64(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// torch.logsumexp's pivot: the maximum, or 0 when that is infinite (all rows -inf: bound -inf; a +inf row: bound +inf; the weights are NaN
// in both cases, as torch.softmax gives them)
__device__ __forceinline__ double lse_pivot(double mx) { return isinf(mx) ? 0.0 : mx; }

// One workgroup; thread t owns images t, t + 256, ... and strides over their K rows (coalesced in the sample-major layout). K*B is a few
// ten thousand at most, so the arithmetic is double throughout: the outputs are the float64 formula rounded once. step != NULL: beta is
// read on the device (anneal_beta, as lvae_elbo_loss_fwd_anneal_f32 reads it).
__global__ __launch_bounds__(256) void iw_loss_fwd_kernel(const float* __restrict__ ll, const float* __restrict__ kl_sep, float beta_arg,
                                                           const int64_t* step, int64_t anneal_steps, int K, int B,
                                                           float* __restrict__ elbo_sep, float* __restrict__ w, float* __restrict__ bound,
                                                           float* scalars) {
  __shared__ double red[4];
  const double beta = step ? anneal_beta(step, anneal_steps) : beta_arg;
  const double logK = log((double)K);
  double s_bound = 0.0, s_elbo = 0.0, s_nll = 0.0, s_iw = 0.0, s_ess = 0.0;
  for (int b = threadIdx.x; b < B; b += 256) {
    double mx = -INFINITY, mx1 = -INFINITY;
    for (int k = 0; k < K; ++k) {
      const size_t n = (size_t)k * B + b;
      const double l = ll[n], q = kl_sep[n], e = l - q;
      mx = fmax(mx, l - beta * q);
      mx1 = fmax(mx1, e);
      elbo_sep[n] = (float)e;
      s_elbo += e;
      s_nll -= l;
    }
    mx = lse_pivot(mx), mx1 = lse_pivot(mx1);
    double s = 0.0, s1 = 0.0;
    for (int k = 0; k < K; ++k) {
      const size_t n = (size_t)k * B + b;
      const double l = ll[n], q = kl_sep[n];
      s += exp(l - beta * q - mx);   // exp(-inf) = 0 exactly: a -inf row among finite ones weighs nothing
      s1 += exp(l - q - mx1);
    }
    const double bd = mx + log(s) - logK;
    bound[b] = (float)bd;
    s_bound += bd;
    s_iw += mx1 + log(s1) - logK;
    double sw2 = 0.0;
    for (int k = 0; k < K; ++k) {
      const size_t n = (size_t)k * B + b;
      const double wk = exp((double)ll[n] - beta * (double)kl_sep[n] - mx) / s;
      w[n] = (float)wk;
      sw2 += wk * wk;
    }
    s_ess += 1.0 / sw2;
  }
  s_bound = block_sum_256_f64(s_bound, red);
  s_elbo = block_sum_256_f64(s_elbo, red);
  s_nll = block_sum_256_f64(s_nll, red);
  s_iw = block_sum_256_f64(s_iw, red);
  s_ess = block_sum_256_f64(s_ess, red);
  if (threadIdx.x == 0) {
    const double rows = (double)K * (double)B;
    scalars[0] = (float)(-s_bound / (double)B);
    scalars[1] = (float)(s_elbo / rows);
    scalars[2] = (float)(s_nll / rows);
    scalars[3] = (float)(s_iw / (double)B);
    scalars[4] = (float)(s_ess / (double)B);
  }
}

// d_ll[n] = -g w[n] / B, d_kl_sep[n] = g beta w[n] / B (a weight of exactly 1 gives exactly -g / B)
__global__ __launch_bounds__(256) void iw_loss_bwd_kernel(const float* g_loss, const float* __restrict__ w, float beta_arg, const int64_t* step,
                                                           int64_t anneal_steps, int rows, int B, float* __restrict__ d_ll,
                                                           float* __restrict__ d_kl_sep) {
  const float g = g_loss[0], beta = step ? anneal_beta(step, anneal_steps) : beta_arg;
  for (int n = blockIdx.x * 256 + threadIdx.x; n < rows; n += gridDim.x * 256) {
    d_ll[n] = -g * w[n] / (float)B;
    d_kl_sep[n] = g * beta * w[n] / (float)B;
  }
}

// Broadcast over samples. `in` is 16-byte aligned (checked by the entry point) but copy k of `out` starts n floats further on, which is a
// multiple of 16 bytes only when n % 4 == 0: the copies are addressed through a 4-byte aligned vector type, for which the compiler emits
// the 16-byte access where the target allows it unaligned and splits it where not.
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

__global__ __launch_bounds__(256) void repeat_samples_fwd_kernel(const float* __restrict__ in, int64_t n, int K, float* __restrict__ out) {
  const int64_t nv = n >> 2, stride = (int64_t)gridDim.x * 256;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nv; v += stride) {
    const f32x4 x = reinterpret_cast<const f32x4*>(in)[v];
    for (int k = 0; k < K; ++k) *reinterpret_cast<f32x4u*>(out + (size_t)k * n + 4 * v) = x;
  }
  for (int64_t i = 4 * nv + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {   // scalar tail: n % 4 elements
    const float x = in[i];
    for (int k = 0; k < K; ++k) out[(size_t)k * n + i] = x;
  }
}

// din[i] = ((dout[0][i] + dout[1][i]) + ...) + dout[K-1][i]: the sequential float32 sum in ascending k
__global__ __launch_bounds__(256) void repeat_samples_bwd_kernel(const float* __restrict__ dout, int64_t n, int K, float* __restrict__ din) {
  const int64_t nv = n >> 2, stride = (int64_t)gridDim.x * 256;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nv; v += stride) {
    f32x4 acc = *reinterpret_cast<const f32x4u*>(dout + 4 * v);
    for (int k = 1; k < K; ++k) acc += *reinterpret_cast<const f32x4u*>(dout + (size_t)k * n + 4 * v);
    reinterpret_cast<f32x4*>(din)[v] = acc;
  }
  for (int64_t i = 4 * nv + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    float acc = dout[i];
    for (int k = 1; k < K; ++k) acc += dout[(size_t)k * n + i];
    din[i] = acc;
  }
}

static int iw_loss_fwd(const char* who, const float* ll, const float* kl_sep, float beta, const int64_t* step, int64_t anneal_steps,
                       int32_t K, int32_t B, float* elbo_sep, float* w, float* bound, float* scalars, void* stream) {
  LVAE_REQUIRE(ll && kl_sep && elbo_sep && w && bound && scalars && K > 0 && B > 0 && (int64_t)K * B <= INT32_MAX, LVAE_EINVAL,
               "%s: bad args", who);
  hipLaunchKernelGGL(iw_loss_fwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ll, kl_sep, beta, step, anneal_steps, K, B, elbo_sep,
                     w, bound, scalars);
  LVAE_LAUNCH_CHECK(who);
  return 0;
}

static int iw_loss_bwd(const char* who, const float* g_loss, const float* w, float beta, const int64_t* step, int64_t anneal_steps, int32_t K,
                       int32_t B, float* d_ll, float* d_kl_sep, void* stream) {
  LVAE_REQUIRE(g_loss && w && d_ll && d_kl_sep && K > 0 && B > 0 && (int64_t)K * B <= INT32_MAX, LVAE_EINVAL, "%s: bad args", who);
  hipLaunchKernelGGL(iw_loss_bwd_kernel, dim3(grid_for((int64_t)K * B, 256)), dim3(256), 0, (hipStream_t)stream, g_loss, w, beta, step,
                     anneal_steps, K * B, B, d_ll, d_kl_sep);
  LVAE_LAUNCH_CHECK(who);
  return 0;
}

}  // namespace lvae

using namespace lvae;

extern "C" int lvae_iw_loss_fwd_f32(const float* ll, const float* kl_sep, float beta, int32_t K, int32_t B, float* elbo_sep, float* w,
                                    float* bound, float* scalars, void* stream) {
  return iw_loss_fwd("lvae_iw_loss_fwd_f32", ll, kl_sep, beta, nullptr, 0, K, B, elbo_sep, w, bound, scalars, stream);
}

extern "C" int lvae_iw_loss_bwd_f32(const float* g_loss, const float* w, float beta, int32_t K, int32_t B, float* d_ll, float* d_kl_sep,
                                    void* stream) {
  return iw_loss_bwd("lvae_iw_loss_bwd_f32", g_loss, w, beta, nullptr, 0, K, B, d_ll, d_kl_sep, stream);
}

extern "C" int lvae_iw_loss_fwd_anneal_f32(const float* ll, const float* kl_sep, const int64_t* step, int64_t anneal_steps, int32_t K,
                                           int32_t B, float* elbo_sep, float* w, float* bound, float* scalars, void* stream) {
  LVAE_REQUIRE(step, LVAE_EINVAL, "lvae_iw_loss_fwd_anneal_f32: bad args");
  return iw_loss_fwd("lvae_iw_loss_fwd_anneal_f32", ll, kl_sep, 0.f, step, anneal_steps, K, B, elbo_sep, w, bound, scalars, stream);
}

extern "C" int lvae_iw_loss_bwd_anneal_f32(const float* g_loss, const float* w, const int64_t* step, int64_t anneal_steps, int32_t K,
                                           int32_t B, float* d_ll, float* d_kl_sep, void* stream) {
  LVAE_REQUIRE(step, LVAE_EINVAL, "lvae_iw_loss_bwd_anneal_f32: bad args");
  return iw_loss_bwd("lvae_iw_loss_bwd_anneal_f32", g_loss, w, 0.f, step, anneal_steps, K, B, d_ll, d_kl_sep, stream);
}

extern "C" int lvae_repeat_samples_fwd_f32(const float* in, int64_t n, int32_t K, float* out, void* stream) {
  LVAE_REQUIRE(in && out && n > 0 && K > 0, LVAE_EINVAL, "lvae_repeat_samples_fwd_f32: bad args");
  LVAE_REQUIRE(al16(in) && al16(out), LVAE_EALIGN, "lvae_repeat_samples_fwd_f32: in and out must be 16-byte aligned");
  hipLaunchKernelGGL(repeat_samples_fwd_kernel, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream, in, n, K, out);
  LVAE_LAUNCH_CHECK("lvae_repeat_samples_fwd_f32");
  return 0;
}

extern "C" int lvae_repeat_samples_bwd_f32(const float* dout, int64_t n, int32_t K, float* din, void* stream) {
  LVAE_REQUIRE(dout && din && n > 0 && K > 0, LVAE_EINVAL, "lvae_repeat_samples_bwd_f32: bad args");
  LVAE_REQUIRE(al16(dout) && al16(din), LVAE_EALIGN, "lvae_repeat_samples_bwd_f32: dout and din must be 16-byte aligned");
  hipLaunchKernelGGL(repeat_samples_bwd_kernel, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream, dout, n, K, din);
  LVAE_LAUNCH_CHECK("lvae_repeat_samples_bwd_f32");
  return 0;
}
