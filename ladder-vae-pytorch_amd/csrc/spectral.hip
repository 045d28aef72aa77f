// Spectral regularisation of the convolution weights (NVAE §3.2): one power-iteration step per optimizer step for EVERY convolution of
// the model in one launch, and the penalty's gradient lambda * v' u'^T added into the weights' gradient slots.
//
// A weight lies in the arena as a row-major matrix A of K = KH*KW*Cin rows and Cout contiguous columns. Per table entry, from the
// persistent u (length Cout), by torch.nn.utils.spectral_norm's rule:
//   s = A u,    v' = s / max(|s|, 1e-12)        t = A^T v',  u' = t / max(|t|, 1e-12)        sigma = |t|
//   grad[k][c] += (lambda / gscale) * v'[k] * u'[c]
//
// One workgroup of 512 threads owns a matrix from its first load to its last store (entries beyond the grid: a grid-stride loop), so every
// sum has one order whatever the grid and no atomics exist: a row's dot product is summed by the lanes that share the row and their
// shuffle tree, a column's by G row groups in sequence and then the G partial sums in order, the two norms in double over the threads'
// strided partial sums, lanes by the shuffle tree, waves 0..7 in order. s / v' and t / u' live in LDS (K <= 4096, Cout <= 1024); the second
// pass over A (for t) and the gradient pass find the matrix the workgroup has just read in L2, so the weights come from HBM once.
// The division is IEEE (v' = s / d, not s * (1 / d)) and nothing is contracted (-ffp-contract=off).
//
// An entry that does not lie inside the buffers the call names, or whose K / Cout exceed the LDS arrays, is not touched: its sigma is NaN.
#include "lvae_common.h"

namespace lvae {

constexpr int kSrThreads = 512;
constexpr int kSrWaves = kSrThreads / 64;
constexpr int kSrMaxK = 4096;
constexpr int kSrMaxC = 1024;
constexpr int kSrMaxGroups = 64;   // row groups of the column pass: the partial sums of a column are added by one thread, in order
constexpr float kSrEps = 1e-12f;   // torch.nn.utils.spectral_norm's eps

struct SpectralArgs {
  const lvae_spectral_entry* table;
  int n_entries;
  const float* params;
  float* grads;   // null: iterate only
  const float* u_in;
  float* u_out;   // may be u_in: an entry's u is in LDS before its u' is stored
  float* v_out;
  float* sigma_out;
  const float* gscale;
  float lam;
  int64_t n_params, n_grads, n_u, n_v;
};

// sum of one double over the 512 threads in a fixed order; valid in every thread. `red` = kSrWaves doubles of LDS.
__device__ __forceinline__ double sr_block_sum_f64(double x, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  x = red[0];
#pragma unroll
  for (int w = 1; w < kSrWaves; ++w) x += red[w];
  return x;
}

__global__ __launch_bounds__(kSrThreads) void spectral_step_kernel(SpectralArgs a) {
  __shared__ float sh_v[kSrMaxK];      // s, then v'
  __shared__ float sh_u[kSrMaxC];      // u, then u'
  __shared__ float sh_part[kSrMaxC];   // the column pass's partial sums [G][Cout], then t
  __shared__ double red[kSrWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float gs = a.gscale ? a.gscale[0] : 1.f;
  const float coef = a.lam / gs;
  for (int e = blockIdx.x; e < a.n_entries; e += gridDim.x) {
    const lvae_spectral_entry en = a.table[e];
    bool ok = en.K >= 1 && en.K <= kSrMaxK && en.Cout >= 1 && en.Cout <= kSrMaxC;
    const int64_t kc = ok ? en.K * en.Cout : 0;
    ok = ok && en.param_off >= 0 && en.param_off <= a.n_params - kc && en.u_off >= 0 && en.u_off <= a.n_u - en.Cout && en.v_off >= 0 &&
         en.v_off <= a.n_v - en.K;
    if (a.grads) ok = ok && en.grad_off >= 0 && en.grad_off <= a.n_grads - kc;
    if (!ok) {   // uniform over the workgroup
      if (tid == 0) a.sigma_out[e] = __builtin_nanf("");
      continue;
    }
    const int K = (int)en.K, C = (int)en.Cout;
    const float* A = a.params + en.param_off;
    // the lanes that share a row: 64, or the power of two that holds a short row, so that a wave takes 64 / L rows at a time
    int L = 64;
    if (C <= 32) {
      L = 1;
      while (L < C) L <<= 1;
    }
    const int R = 64 / L, sub = lane / L, l = lane - sub * L;
    const int rows_per_pass = kSrWaves * R;

    for (int c = tid; c < C; c += kSrThreads) sh_u[c] = a.u_in[en.u_off + c];
    __syncthreads();

    // s = A u
    for (int kb = wave * R; kb < K; kb += 4 * rows_per_pass) {   // (uniform over the wave: every lane meets the shuffles)
      float acc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = kb + j * rows_per_pass + sub;
        acc[j] = 0.f;
        if (k < K) {
          const float* row = A + (size_t)k * C;
          for (int c = l; c < C; c += L) acc[j] += row[c] * sh_u[c];
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        for (int o = L >> 1; o > 0; o >>= 1) acc[j] += __shfl_xor(acc[j], o, 64);
        const int k = kb + j * rows_per_pass + sub;
        if (l == 0 && k < K) sh_v[k] = acc[j];
      }
    }
    __syncthreads();
    double ss = 0.0;
    for (int k = tid; k < K; k += kSrThreads) ss += (double)sh_v[k] * (double)sh_v[k];
    ss = sr_block_sum_f64(ss, red);
    const float ds = fmaxf((float)sqrt(ss), kSrEps);
    for (int k = tid; k < K; k += kSrThreads) {
      const float v = sh_v[k] / ds;
      sh_v[k] = v;
      a.v_out[en.v_off + k] = v;
    }
    __syncthreads();

    // t = A^T v': G row groups, a thread per (group, column)
    int G = kSrThreads / C;
    G = G < 1 ? 1 : (G > kSrMaxGroups ? kSrMaxGroups : G);
    for (int idx = tid; idx < G * C; idx += kSrThreads) {   // (more than one turn only when G == 1)
      const int g = idx / C, c = idx - g * C;
      float acc = 0.f;
#pragma unroll 4
      for (int k = g; k < K; k += G) acc += A[(size_t)k * C + c] * sh_v[k];
      sh_part[idx] = acc;
    }
    __syncthreads();
    float tc[2] = {0.f, 0.f};   // Cout <= 2 * kSrThreads
    for (int c = tid, q = 0; c < C; c += kSrThreads, ++q) {
      float acc = sh_part[c];
      for (int g = 1; g < G; ++g) acc += sh_part[g * C + c];
      tc[q] = acc;
    }
    double st = (double)tc[0] * (double)tc[0] + (double)tc[1] * (double)tc[1];
    st = sr_block_sum_f64(st, red);   // (its barriers also order the reads of sh_part above before the stores below)
    const float sigma = (float)sqrt(st);
    const float dt = fmaxf(sigma, kSrEps);
    for (int c = tid, q = 0; c < C; c += kSrThreads, ++q) {
      const float u = tc[q] / dt;
      sh_u[c] = u;
      a.u_out[en.u_off + c] = u;
    }
    if (tid == 0) a.sigma_out[e] = sigma;
    __syncthreads();

    // grad += (lambda / gscale) v' u'^T, by the thread map of the first pass
    if (a.grads) {
      float* Gd = a.grads + en.grad_off;
      for (int k = wave * R + sub; k < K; k += rows_per_pass) {
        const float cv = coef * sh_v[k];
        float* row = Gd + (size_t)k * C;
        for (int c = l; c < C; c += L) row[c] = row[c] + cv * sh_u[c];
      }
    }
    __syncthreads();   // the next entry reuses the LDS arrays
  }
}

// out[0] = sum of the sigmas, out[1] = their maximum (NaN if one is NaN). One workgroup: thread j adds entries j, j + 256, ... in double,
// lanes by the shuffle tree, waves 0..3 in order; the sum is rounded to float once.
__global__ __launch_bounds__(256) void spectral_reduce_kernel(const float* __restrict__ sigma, int n, float* out) {
  __shared__ double red_s[4];
  __shared__ float red_m[4];
  double s = 0.0;
  float m = 0.f;   // a sigma is a norm: never negative
  for (int i = threadIdx.x; i < n; i += 256) {
    const float x = sigma[i];
    s += (double)x;
    m = (x > m || x != x) ? x : m;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    const float y = __shfl_xor(m, o, 64);
    m = (m != m) ? m : ((y > m || y != y) ? y : m);
  }
  if ((threadIdx.x & 63) == 0) red_s[threadIdx.x >> 6] = s, red_m[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x != 0) return;
  s = red_s[0], m = red_m[0];
  for (int w = 1; w < 4; ++w) {
    s += red_s[w];
    const float y = red_m[w];
    m = (m != m) ? m : ((y > m || y != y) ? y : m);
  }
  out[0] = (float)s;
  out[1] = m;
}

}  // namespace lvae

using namespace lvae;

extern "C" int lvae_spectral_step_f32(const lvae_spectral_entry* table, int32_t n_entries, const float* params, int64_t n_params, float* grads,
                                      int64_t n_grads, const float* u_in, float* u_out, int64_t n_u, float* v_out, int64_t n_v,
                                      float* sigma_out, float lambda, const float* gscale, int32_t max_workgroups, void* stream) {
  LVAE_REQUIRE(table && n_entries > 0 && params && u_in && u_out && v_out && sigma_out, LVAE_EINVAL,
               "lvae_spectral_step_f32: table, params, u_in, u_out, v_out or sigma_out missing, or no entries");
  LVAE_REQUIRE(n_params > 0 && n_u > 0 && n_v > 0 && (!grads || n_grads > 0), LVAE_EINVAL,
               "lvae_spectral_step_f32: the lengths of params, grads, u and v bound every entry and must be positive");
  LVAE_REQUIRE((reinterpret_cast<uintptr_t>(table) & 7) == 0, LVAE_EALIGN, "lvae_spectral_step_f32: misaligned table");
  LVAE_REQUIRE(max_workgroups >= 0, LVAE_EINVAL, "lvae_spectral_step_f32: max_workgroups %d", max_workgroups);
  LVAE_REQUIRE(!grads || (lambda >= 0.f && lambda <= 3.402823466e38f), LVAE_EINVAL, "lvae_spectral_step_f32: lambda must be finite and not negative");
  const int grid = max_workgroups > 0 && max_workgroups < n_entries ? max_workgroups : n_entries;
  const SpectralArgs a{table, n_entries, params, grads, u_in, u_out, v_out, sigma_out, gscale, lambda, n_params, grads ? n_grads : 0, n_u, n_v};
  hipLaunchKernelGGL(spectral_step_kernel, dim3(grid), dim3(kSrThreads), 0, (hipStream_t)stream, a);
  LVAE_LAUNCH_CHECK("spectral_step");
  return 0;
}

extern "C" int lvae_spectral_reduce_f32(const float* sigma, int32_t n_entries, float* out, void* stream) {
  LVAE_REQUIRE(sigma && out && n_entries > 0, LVAE_EINVAL, "lvae_spectral_reduce_f32: bad args");
  hipLaunchKernelGGL(spectral_reduce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, sigma, n_entries, out);
  LVAE_LAUNCH_CHECK("spectral_reduce");
  return 0;
}
