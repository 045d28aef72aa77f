// Interpolation between two sets of latent rows (sampling only, no backward): out[j*B + b] = wa(b, j) * za[b] + wc(b, j) * zb[b] for the T
// steps t[j], linear (wa = 1 - t, wc = t) or spherical (wa = sin((1 - t) W) / sin W, wc = sin(t W) / sin W with W the angle between the two
// rows). t == 0 and t == 1 are branches: the row is a copy of za[b] / zb[b] bit for bit, whatever the other row holds.
//
// Two launches. The coefficients need four sums over a row, in a fixed order and without float atomics, so one workgroup of 1,024 threads
// owns a pair (as a row's sum in prior_sample.hip): double partial sums per thread, lanes by the shuffle tree, waves 0..15 in order. It reads
// the two rows twice (norms, then the chord and its complement of the normalised rows; the second pass finds them in L2) and writes 2 * T
// floats per pair into the workspace. With the usual 12 pairs that launch leaves most of the chip idle, but it moves 2 of the 2 + T row
// sets of the whole call; the part that writes the T * B rows is a launch of its own over every row chunk, where the chip is full and a
// workgroup's row, step and coefficients are uniform (scalar loads, and the endpoint branch does not diverge).
//
// The angle is never taken from acos of a cosine, which loses everything for nearly parallel rows: W = 2 atan2(|a^ - c^|, |a^ + c^|) in
// double, the coefficients in double, each rounded once to float and combined in float (two products, one sum; -ffp-contract=off).
#include "lvae_host.h"

namespace lvae {

struct InterpCoefArgs {
  const float* za;
  const float* zb;
  const float* t;
  int B, T, mode;
  int64_t n;
  float* coef;  // [B][T][2]
};

struct InterpApplyArgs {
  const float* za;
  const float* zb;
  const float* t;
  const float* coef;
  int B, T;
  int64_t n;       // elements of a row
  int64_t chunks;  // workgroup-sized pieces of a row
  int64_t total;   // T * B * chunks
  float* out;
};

constexpr int kLiThreads = 1024;   // coefficient launch
constexpr int kLiApply = 256;      // apply launch
constexpr int kLiUnroll = 4;       // 16-byte groups (or elements, scalar map) per thread and chunk
constexpr double kLiMinSin = 1e-6; // below it (parallel or antipodal rows) the pair takes the lerp coefficients

// sum of two doubles over the 1,024 threads in a fixed order; valid in every thread. `red` = 32 doubles of LDS.
__device__ __forceinline__ void block_sum2_f64(double& u, double& v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    u += __shfl_xor(u, o, 64);
    v += __shfl_xor(v, o, 64);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = u;
    red[16 + (threadIdx.x >> 6)] = v;
  }
  __syncthreads();
  u = red[0], v = red[16];
#pragma unroll
  for (int w = 1; w < kLiThreads / 64; ++w) u += red[w], v += red[16 + w];
}

__global__ __launch_bounds__(kLiThreads) void latent_interp_coef_kernel(InterpCoefArgs a) {
  __shared__ double red[32];
  const int b = blockIdx.x, tid = threadIdx.x;
  bool slerp = a.mode == 1;
  double omega = 0.0, sin_omega = 0.0;
  if (slerp) {  // uniform over the launch
    const float* ra = a.za + (size_t)b * a.n;
    const float* rc = a.zb + (size_t)b * a.n;
    double saa = 0.0, scc = 0.0;
    for (int64_t i = tid; i < a.n; i += kLiThreads) {
      const double x = ra[i], y = rc[i];
      saa += x * x;
      scc += y * y;
    }
    block_sum2_f64(saa, scc, red);
    const double na = sqrt(saa), nc = sqrt(scc);
    slerp = na > 0.0 && nc > 0.0;  // uniform over the workgroup: every thread holds the same sums
    if (slerp) {
      const double ia = 1.0 / na, ic = 1.0 / nc;
      double sd = 0.0, ss = 0.0;
      for (int64_t i = tid; i < a.n; i += kLiThreads) {
        const double x = ra[i] * ia, y = rc[i] * ic;
        sd += (x - y) * (x - y);
        ss += (x + y) * (x + y);
      }
      block_sum2_f64(sd, ss, red);
      omega = 2.0 * atan2(sqrt(sd), sqrt(ss));
      sin_omega = sin(omega);
      slerp = !(sin_omega < kLiMinSin);
    }
  }
  for (int j = tid; j < a.T; j += kLiThreads) {
    const double t = a.t[j];
    double wa = 1.0 - t, wc = t;
    if (slerp) {
      wa = sin((1.0 - t) * omega) / sin_omega;
      wc = sin(t * omega) / sin_omega;
    }
    float* o = a.coef + ((size_t)b * a.T + j) * 2;
    o[0] = (float)wa;
    o[1] = (float)wc;
  }
}

// n % 4 == 0 and 16-byte aligned za, zb, out: a thread takes kLiUnroll groups of 4 consecutive elements of its workgroup's row chunk
__global__ __launch_bounds__(kLiApply) void latent_interp_apply_v4_kernel(InterpApplyArgs a) {
  const int64_t n4 = a.n >> 2;
  for (int64_t w = blockIdx.x; w < a.total; w += gridDim.x) {
    const int64_t row = w / a.chunks, chunk = w - row * a.chunks;
    const int j = (int)(row / a.B), b = (int)(row - (int64_t)j * a.B);
    const float t = a.t[j];
    const float wa = a.coef[((size_t)b * a.T + j) * 2], wc = a.coef[((size_t)b * a.T + j) * 2 + 1];
    const f32x4* ra = reinterpret_cast<const f32x4*>(a.za + (size_t)b * a.n);
    const f32x4* rc = reinterpret_cast<const f32x4*>(a.zb + (size_t)b * a.n);
    f32x4* ro = reinterpret_cast<f32x4*>(a.out + (size_t)row * a.n);
    const int64_t base = chunk * (kLiApply * kLiUnroll) + threadIdx.x;
#pragma unroll
    for (int u = 0; u < kLiUnroll; ++u) {
      const int64_t e = base + u * kLiApply;
      if (e >= n4) continue;
      if (t == 0.f) {
        ro[e] = ra[e];
      } else if (t == 1.f) {
        ro[e] = rc[e];
      } else {
        const f32x4 x = ra[e], y = rc[e];
        f32x4 r;
#pragma unroll
        for (int q = 0; q < 4; ++q) r[q] = wa * x[q] + wc * y[q];
        ro[e] = r;
      }
    }
  }
}

// any n, any alignment: one element per thread and slot
__global__ __launch_bounds__(kLiApply) void latent_interp_apply_kernel(InterpApplyArgs a) {
  for (int64_t w = blockIdx.x; w < a.total; w += gridDim.x) {
    const int64_t row = w / a.chunks, chunk = w - row * a.chunks;
    const int j = (int)(row / a.B), b = (int)(row - (int64_t)j * a.B);
    const float t = a.t[j];
    const float wa = a.coef[((size_t)b * a.T + j) * 2], wc = a.coef[((size_t)b * a.T + j) * 2 + 1];
    const float* ra = a.za + (size_t)b * a.n;
    const float* rc = a.zb + (size_t)b * a.n;
    float* ro = a.out + (size_t)row * a.n;
    const int64_t base = chunk * (kLiApply * kLiUnroll) + threadIdx.x;
#pragma unroll
    for (int u = 0; u < kLiUnroll; ++u) {
      const int64_t e = base + u * kLiApply;
      if (e >= a.n) continue;
      if (t == 0.f) {
        ro[e] = ra[e];
      } else if (t == 1.f) {
        ro[e] = rc[e];
      } else {
        ro[e] = wa * ra[e] + wc * rc[e];
      }
    }
  }
}

}  // namespace lvae

using namespace lvae;

extern "C" size_t lvae_latent_interp_workspace(int32_t B, int32_t T) {
  if (B <= 0 || T <= 0) return 0;
  return (size_t)B * (size_t)T * 2 * sizeof(float);
}

extern "C" int lvae_latent_interp_f32(const float* za, const float* zb, const float* t, int32_t B, int64_t n, int32_t T, int32_t mode,
                                      float* out, void* workspace, size_t workspace_bytes, void* stream) {
  LVAE_REQUIRE(za && zb && t && out, LVAE_EINVAL, "lvae_latent_interp_f32: za, zb, t or out missing");
  LVAE_REQUIRE(B > 0 && n > 0 && T > 0, LVAE_EINVAL, "lvae_latent_interp_f32: B %d, n %lld, T %d", B, (long long)n, T);
  LVAE_REQUIRE(mode == 0 || mode == 1, LVAE_EINVAL, "lvae_latent_interp_f32: mode %d is neither 0 (lerp) nor 1 (slerp)", mode);
  LVAE_REQUIRE((int64_t)B * T <= INT32_MAX, LVAE_EINVAL, "lvae_latent_interp_f32: %d x %d rows exceed 32-bit indexing", T, B);
  LVAE_REQUIRE(n <= (INT64_MAX >> 3) / ((int64_t)B * T), LVAE_EINVAL, "lvae_latent_interp_f32: %d x %d rows of %lld exceed 64-bit byte offsets",
               T, B, (long long)n);
  const size_t need = lvae_latent_interp_workspace(B, T);
  LVAE_REQUIRE(workspace && workspace_bytes >= need, LVAE_EWORKSPACE, "lvae_latent_interp_f32: workspace of %zu bytes, %zu needed",
               workspace ? workspace_bytes : (size_t)0, need);
  LVAE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, LVAE_EALIGN, "lvae_latent_interp_f32: workspace is not 4-byte aligned");
  float* coef = static_cast<float*>(workspace);
  const InterpCoefArgs c{za, zb, t, B, T, mode, n, coef};
  // the default limit: no kernel here has dynamic LDS
  int rc = launch_lds<latent_interp_coef_kernel>("latent_interp (coefficients)", dim3(B), dim3(kLiThreads), 0, 64 * 1024, (hipStream_t)stream, c);
  if (rc) return rc;
  const bool v4 = n % 4 == 0 && al16(za) && al16(zb) && al16(out);
  const int64_t per = (int64_t)kLiApply * kLiUnroll;
  const int64_t chunks = ((v4 ? n / 4 : n) + per - 1) / per;
  const int64_t total = (int64_t)B * T * chunks;
  const InterpApplyArgs a{za, zb, t, coef, B, T, n, chunks, total, out};
  const dim3 grid((unsigned)(total < (1 << 20) ? total : (1 << 20)));
  if (v4) return launch_lds<latent_interp_apply_v4_kernel>("latent_interp", grid, dim3(kLiApply), 0, 64 * 1024, (hipStream_t)stream, a);
  return launch_lds<latent_interp_apply_kernel>("latent_interp", grid, dim3(kLiApply), 0, 64 * 1024, (hipStream_t)stream, a);
}
