// Weight / bias gradient of the implicit-GEMM convolution on fp32 MFMA.
//
//   dW[tap][ci][co] = sum_{m=(n,oh,ow)} T(x)[m @ tap][ci] * dy[m][co]        db[co] = sum_m dy[m][co]
//
// GEMM view per tap: M' = ci (A = T(x)^T), N' = co (B = dy), K' = output pixels. Both operands are pixel-major
// in memory (NHWC), i.e. already "k-major": the LDS stages are [pixel][channel] and the MFMA fragments are
// ds_read_b32 of 32 consecutive channels (conflict free). The pixel range is split over `ksplit` workgroups
// per (tap, ci-tile, co-tile); each writes its 64x64 partial to a slab, and a second kernel sums the slabs in a
// fixed order (bitwise reproducible, no float atomics) and accumulates into the gradient arena.
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <vector>

#include "lvae_host.h"

namespace lvae {

constexpr int KP = 32;   // pixels per stage
constexpr int CT = 64;   // channel tile (both ci and co)

struct WgradArgs {
  lvae_conv_desc d;
  const float* dy;
  float* slab_w;   // [ksplit][taps][Cin][Cout]
  float* slab_b;   // [ksplit][Cout]
  int M, ohw, Cin, ntaps, ncit, ncot, ksplit, px_per_split;
};

__device__ __forceinline__ bool tap_coord_w(int o, int k, int stride, int pad, int limit, int gather, int& i) {
  if (gather == LVAE_GATHER_CONV) {
    i = o * stride - pad + k;
    return i >= 0 && i < limit;
  }
  int t = o + pad - k;
  if (t < 0) return false;
  i = t / stride;
  return (t - i * stride == 0) && i < limit;
}

template <bool X_VEC, bool Y_VEC>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(WgradArgs a) {
  kernarg_warmup<(sizeof(WgradArgs) < 1024 ? sizeof(WgradArgs) : 1024)>();
  __shared__ __attribute__((aligned(16))) float Xs[2][KP][CT];
  __shared__ __attribute__((aligned(16))) float Ys[2][KP][CT];
  const lvae_conv_desc& d = a.d;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int wci = wave >> 1, wco = wave & 1;

  int bid = blockIdx.x;
  const int ks = bid % a.ksplit;
  bid /= a.ksplit;
  const int cot = bid % a.ncot;
  bid /= a.ncot;
  const int cit = bid % a.ncit;
  const int tap = bid / a.ncit;
  const int kh = tap / d.KW, kw = tap - kh * d.KW;
  const int ci0 = cit * CT, co0 = cot * CT;
  const int p_begin = ks * a.px_per_split;
  const int p_end = min(a.M, p_begin + a.px_per_split);
  const bool do_bias = (a.slab_b != nullptr) && tap == 0 && cit == 0;

  // vector staging: thread -> pixel row (t>>4) + 16*p, channels (t&15)*4
  const int prow = t >> 4, c4 = (t & 15) * 4;
  f32x4 xr[2], yr[2];
  float xs_[8], ys_[8];
  f32x4 bsum = {0.f, 0.f, 0.f, 0.f};
  float bsum_s = 0.f;

  f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
  float sc_s = 1.f, sh_s = 0.f;
  if (X_VEC) {
    if (d.in_scale && ci0 + c4 < a.Cin) {
      sc = *reinterpret_cast<const f32x4*>(d.in_scale + ci0 + c4);
      sh = *reinterpret_cast<const f32x4*>(d.in_shift + ci0 + c4);
    }
  } else if (d.in_scale && ci0 + (t & 63) < a.Cin) {
    sc_s = d.in_scale[ci0 + (t & 63)];
    sh_s = d.in_shift[ci0 + (t & 63)];
  }

  auto load_x_pixel = [&](int m, int& n, int& ih, int& iw) -> bool {
    if (m >= p_end) return false;
    n = m / a.ohw;
    int rem = m - n * a.ohw;
    int oh = rem / d.OW, ow = rem - oh * d.OW;
    return tap_coord_w(oh, kh, d.stride, d.pad, d.H, d.gather, ih) &&
           tap_coord_w(ow, kw, d.stride, d.pad, d.W, d.gather, iw);
  };

  auto load_stage = [&](int p0) {
    if (X_VEC) {
      const int ci = ci0 + c4;
      const float* src = d.x;
      int cs = ci, cstride = d.C1;
      if (ci >= d.C1) {
        src = d.x2;
        cs = ci - d.C1;
        cstride = d.C2;
      }
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        int n, ih, iw;
        if (ci < a.Cin && load_x_pixel(p0 + prow + 16 * p, n, ih, iw)) {
          v = *reinterpret_cast<const f32x4*>(src + ((size_t)(n * d.H + ih) * d.W + iw) * cstride + cs);
          if (d.in_scale) {
            v = v * sc + sh;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = act_fwd(v[j], d.in_act);
          }
        }
        xr[p] = v;
      }
    } else {
      const int ci = ci0 + (t & 63);
      const float* src = d.x;
      int cs = ci, cstride = d.C1;
      if (ci >= d.C1) {
        src = d.x2;
        cs = ci - d.C1;
        cstride = d.C2;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float v = 0.f;
        int n, ih, iw;
        if (ci < a.Cin && load_x_pixel(p0 + (t >> 6) + 4 * e, n, ih, iw)) {
          v = src[((size_t)(n * d.H + ih) * d.W + iw) * cstride + cs];
          if (d.in_scale) v = act_fwd(v * sc_s + sh_s, d.in_act);
        }
        xs_[e] = v;
      }
    }
    if (Y_VEC) {
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int m = p0 + prow + 16 * p;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (m < p_end && co0 + c4 < d.Cout) v = *reinterpret_cast<const f32x4*>(a.dy + (size_t)m * d.Cout + co0 + c4);
        yr[p] = v;
        if (do_bias) bsum += v;
      }
    } else {
      const int co = co0 + (t & 63);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int m = p0 + (t >> 6) + 4 * e;
        float v = (m < p_end && co < d.Cout) ? a.dy[(size_t)m * d.Cout + co] : 0.f;
        ys_[e] = v;
        if (do_bias) bsum_s += v;
      }
    }
  };

  auto store_stage = [&](int buf) {
    if (X_VEC) {
#pragma unroll
      for (int p = 0; p < 2; ++p) *reinterpret_cast<f32x4*>(&Xs[buf][prow + 16 * p][c4]) = xr[p];
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) Xs[buf][(t >> 6) + 4 * e][t & 63] = xs_[e];
    }
    if (Y_VEC) {
#pragma unroll
      for (int p = 0; p < 2; ++p) *reinterpret_cast<f32x4*>(&Ys[buf][prow + 16 * p][c4]) = yr[p];
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) Ys[buf][(t >> 6) + 4 * e][t & 63] = ys_[e];
    }
  };

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  const int nstages = (p_end - p_begin + KP - 1) / KP;
  if (nstages > 0) {
    load_stage(p_begin);
    store_stage(0);
  }
  __syncthreads();
  for (int s = 0; s < nstages; ++s) {
    const int buf = s & 1;
    if (s + 1 < nstages) load_stage(p_begin + (s + 1) * KP);
    const float* xa = &Xs[buf][lh][wci * 32 + li];
    const float* yb = &Ys[buf][lh][wco * 32 + li];
#pragma unroll
    for (int kk = 0; kk < KP; kk += 2)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[kk * CT], yb[kk * CT], acc, 0, 0, 0);
    if (s + 1 < nstages) store_stage(buf ^ 1);
    __syncthreads();
  }

  // partial tile -> slab [ks][tap][Cin][Cout]; C/D layout: col = lane&31 (co), row = (r&3)+8*(r>>2)+4*lh (ci)
  float* slab = a.slab_w + ((size_t)ks * a.ntaps + tap) * a.Cin * d.Cout;
  const int co = co0 + wco * 32 + li;
  if (co < d.Cout) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ci = ci0 + wci * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      if (ci < a.Cin) slab[(size_t)ci * d.Cout + co] = acc[r];
    }
  }

  if (do_bias) {
    // reduce the per-thread column sums over the pixel rows of the block through LDS (reuse Ys[0])
    __syncthreads();
    float* red = &Ys[0][0][0];
    if (Y_VEC) {
#pragma unroll
      for (int j = 0; j < 4; ++j) red[prow * CT + c4 + j] = bsum[j];
      __syncthreads();
      if (t < CT) {
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) s += red[r * CT + t];
        if (co0 + t < d.Cout) a.slab_b[(size_t)ks * d.Cout + co0 + t] = s;
      }
    } else {
      red[(t >> 6) * CT + (t & 63)] = bsum_s;
      __syncthreads();
      if (t < CT) {
        float s = red[t] + red[CT + t] + red[2 * CT + t] + red[3 * CT + t];
        if (co0 + t < d.Cout) a.slab_b[(size_t)ks * d.Cout + co0 + t] = s;
      }
    }
  }
}

// dw[tap*stap + ci*sk + co*sn] += sum_ks slab[ks][tap][ci][co] ;  db[co] += sum_ks slab_b[ks][co]
// The slab rows [taps*Cin*Cout | Cout] are contiguous and a multiple of 4 floats on the vector path: 256 threads =
// 16 float4 elements x 16 split lanes (1 KB per wave load), LDS tree in a fixed order -> deterministic.
template <int V>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ slab_w, const float* __restrict__ slab_b,
                                                            int ksplit, int ntaps, int Cin, int Cout, int64_t stap, int64_t sk,
                                                            int64_t sn, float* dw, float* db) {
  __shared__ float red[16][16 * 4];
  const int per = ntaps * Cin * Cout;
  const int e = threadIdx.x & 15, q = threadIdx.x >> 4;
  const int idx = (blockIdx.x * 16 + e) * V;  // first float of this thread's element group
  float s[V];
  for (int j = 0; j < V; ++j) s[j] = 0.f;
  const float* src = nullptr;
  int64_t stride = 0;
  if (idx < per) {
    src = slab_w + idx;
    stride = per;
  } else if (db && idx < per + Cout) {
    src = slab_b + (idx - per);
    stride = Cout;
  }
  if (src) {
    // 8 independent loads per round trip, added in slab order (a rolled loop pays one memory latency per slab: 7.7 us for 256 slabs)
    for (int k0 = q; k0 < ksplit; k0 += 16 * 8) {
      if (V == 4) {
        f32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int k = k0 + 16 * u;
          v[u] = *reinterpret_cast<const f32x4*>(src + (size_t)(k < ksplit ? k : q) * stride);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (k0 + 16 * u < ksplit)
            for (int j = 0; j < 4; ++j) s[j] += v[u][j];
      } else {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int k = k0 + 16 * u;
          v[u] = src[(size_t)(k < ksplit ? k : q) * stride];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (k0 + 16 * u < ksplit) s[0] += v[u];
      }
    }
  }
  for (int j = 0; j < V; ++j) red[q][e * 4 + j] = s[j];
  __syncthreads();
  if (q != 0 || !src) return;
  for (int j = 0; j < V; ++j) {
    float t = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) t += red[r][e * 4 + j];
    const int i = idx + j;
    if (i < per) {
      const int co = i % Cout, r2 = i / Cout, ci = r2 % Cin, tap = r2 / Cin;
      dw[tap * stap + ci * sk + co * sn] += t;
    } else if (i < per + Cout) {
      db[i - per] += t;
    }
  }
}

// one gradient's slabs as its plan lays them out. Cin = C1 + C2 also for the families that read x only (bf16, 1x1, thin): their plans
// require x2 == nullptr, and conv_desc_check ties C2 == 0 to that.
int wgrad_op_reduce(const WgradOp& o, hipStream_t s) {
  const lvae_conv_desc* d = o.d;
  wgrad_reduce_launch(o.slab_w(), o.slab_b(), o.plan.slabs, d->KH * d->KW, d->C1 + d->C2, d->Cout, d->w_stap, d->w_sk, d->w_sn, o.dw, o.db, s);
  LVAE_LAUNCH_CHECK("conv2d_wgrad_reduce");
  return 0;
}

void wgrad_reduce_launch(const float* slab_w, const float* slab_b, int ksplit, int ntaps, int Cin, int Cout, int64_t stap,
                         int64_t sk, int64_t sn, float* dw, float* db, hipStream_t s) {
  const int per = ntaps * Cin * Cout, tot = per + (db ? Cout : 0);
  const bool v4 = (per % 4 == 0) && (Cout % 4 == 0) && ((reinterpret_cast<uintptr_t>(slab_w) & 15) == 0) &&
                  (!slab_b || (reinterpret_cast<uintptr_t>(slab_b) & 15) == 0);
  if (v4)
    hipLaunchKernelGGL(wgrad_reduce_kernel<4>, dim3((tot / 4 + 15) / 16), dim3(256), 0, s, slab_w, slab_b, ksplit, ntaps, Cin,
                       Cout, stap, sk, sn, dw, db);
  else
    hipLaunchKernelGGL(wgrad_reduce_kernel<1>, dim3((tot + 15) / 16), dim3(256), 0, s, slab_w, slab_b, ksplit, ntaps, Cin,
                       Cout, stap, sk, sn, dw, db);
}

struct ReduceGroup {
  ReduceArgs p[kMaxReduceGroup];
};

// blockIdx.y = problem; same element mapping as wgrad_reduce_kernel<4> (all grouped problems are float4-aligned)
__global__ __launch_bounds__(256) void wgrad_reduce_grouped_kernel(ReduceGroup g) {
  kernarg_warmup<(sizeof(ReduceGroup) < 1024 ? sizeof(ReduceGroup) : 1024)>();
  __shared__ float red[16][16 * 4];
  const ReduceArgs& a = g.p[blockIdx.y];
  const int per = a.ntaps * a.Cin * a.Cout;
  const int e = threadIdx.x & 15, q = threadIdx.x >> 4;
  const int idx = (blockIdx.x * 16 + e) * 4;
  if ((int)blockIdx.x * 64 >= per + (a.slab_b ? a.Cout : 0)) return;  // uniform per workgroup
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  const float* src = nullptr;
  int64_t stride = 0;
  if (idx < per) {
    src = a.slab_w + idx;
    stride = per;
  } else if (a.db && idx < per + a.Cout) {
    src = a.slab_b + (idx - per);
    stride = a.Cout;
  }
  if (src)
    for (int k0 = q; k0 < a.ksplit; k0 += 16 * 8) {  // 8 independent loads per round trip, added in slab order
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int k = k0 + 16 * u;
        v[u] = *reinterpret_cast<const f32x4*>(src + (size_t)(k < a.ksplit ? k : q) * stride);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (k0 + 16 * u < a.ksplit) s += v[u];
    }
  *reinterpret_cast<f32x4*>(&red[q][e * 4]) = s;
  __syncthreads();
  if (q != 0 || !src) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float t = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) t += red[r][e * 4 + j];
    const int i = idx + j;
    if (i < per) {
      const int co = i % a.Cout, r2 = i / a.Cout, ci = r2 % a.Cin, tap = r2 / a.Cin;
      a.dw[tap * a.stap + ci * a.sk + co * a.sn] += t;
    } else if (i < per + a.Cout) {
      a.db[i - per] += t;
    }
  }
}

void wgrad_reduce_grouped_launch(const ReduceArgs* r, int n, hipStream_t s) {
  ReduceGroup g;
  int max_tot = 0;
  for (int i = 0; i < n; ++i) {
    g.p[i] = r[i];
    const int tot = r[i].ntaps * r[i].Cin * r[i].Cout + (r[i].db ? r[i].Cout : 0);
    if (tot > max_tot) max_tot = tot;
  }
  for (int i = n; i < kMaxReduceGroup; ++i) g.p[i] = g.p[0];
  hipLaunchKernelGGL(wgrad_reduce_grouped_kernel, dim3((max_tot / 4 + 15) / 16, n), dim3(256), 0, s, g);
}

// ---------------------------------------------------------------------------------------------------------
// Weight gradient of the stem convolutions (5x5 stride 2 on the 1- or 3-channel image): the reduction dimension of the
// implicit GEMM is wide (all pixels) but its M side is only KH*KW*Cin <= 76 rows, far too thin for the MFMA tile kernels
// (the generic kernel spends 550 us on 0.6 GFLOP). One workgroup per image: the zero-padded image (<= 32 KB) and the
// image's dy tile sit in LDS; thread = (co, one of 4 k-groups) keeps 19 accumulators in registers and walks the output
// pixels (LDS broadcast read of x, one dy value per pixel). Partials go to the usual split-K slabs [image][k][co].
// ---------------------------------------------------------------------------------------------------------
struct ThinWgradArgs {
  lvae_conv_desc d;
  const float* dy;
  float* slab_w;
  float* slab_b;
  int K, PH, PW;  // K = KH*KW*Cin; padded image height / width
};

__global__ __launch_bounds__(256) void conv_wgrad_thin_kernel(ThinWgradArgs a) {
  kernarg_warmup<(sizeof(ThinWgradArgs) < 1024 ? sizeof(ThinWgradArgs) : 1024)>();
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const lvae_conv_desc& d = a.d;
  const int t = threadIdx.x, n = blockIdx.x;
  const int Cin = d.C1, npx = d.OH * d.OW;
  float* xs = smem;                                   // [PH][PW][Cin], zero border
  float* ys = smem + ((a.PH * a.PW * Cin + 3) & ~3);  // [npx][64]
  for (int i = t; i < a.PH * a.PW * Cin; i += 256) {
    const int ci = i % Cin, r = i / Cin, pw = r % a.PW, ph = r / a.PW;
    const int ih = ph - d.pad, iw = pw - d.pad;
    xs[i] = ((unsigned)ih < (unsigned)d.H && (unsigned)iw < (unsigned)d.W) ? d.x[((size_t)(n * d.H + ih) * d.W + iw) * Cin + ci] : 0.f;
  }
  for (int i = t; i < npx * 64; i += 256) {
    const int co = i & 63, px = i >> 6;
    ys[i] = co < d.Cout ? a.dy[((size_t)n * npx + px) * d.Cout + co] : 0.f;
  }
  __syncthreads();
  const int co = t & 63, kg = t >> 6;
  int koff[19];
#pragma unroll
  for (int kk = 0; kk < 19; ++kk) {
    int k = kg * 19 + kk;
    if (k >= a.K) k = 0;  // surplus slots recompute k = 0; never stored
    const int ci = k % Cin, tap = k / Cin, kw = tap % d.KW, kh = tap / d.KW;
    koff[kk] = (kh * a.PW + kw) * Cin + ci;
  }
  float acc[19];
#pragma unroll
  for (int kk = 0; kk < 19; ++kk) acc[kk] = 0.f;
  float bsum = 0.f;
  for (int oh = 0; oh < d.OH; ++oh) {
    for (int ow = 0; ow < d.OW; ++ow) {
      const float g = ys[(oh * d.OW + ow) * 64 + co];
      const float* xb = xs + ((oh * d.stride) * a.PW + ow * d.stride) * Cin;
      bsum += g;
#pragma unroll
      for (int kk = 0; kk < 19; ++kk) acc[kk] += xb[koff[kk]] * g;
    }
  }
  if (co < d.Cout) {
    float* slab = a.slab_w + (size_t)n * a.K * d.Cout;
#pragma unroll
    for (int kk = 0; kk < 19; ++kk) {
      const int k = kg * 19 + kk;
      if (k < a.K) slab[(size_t)k * d.Cout + co] = acc[kk];
    }
    if (a.slab_b && kg == 0) a.slab_b[(size_t)n * d.Cout + co] = bsum;
  }
}

static size_t thin_lds(const lvae_conv_desc* d) {
  return ((size_t)((d->H + 2 * d->pad) * (d->W + 2 * d->pad) * d->C1 + 3) / 4 * 4 + (size_t)d->OH * d->OW * 64) * sizeof(float);
}

static bool thin_wgrad_plan(const lvae_conv_desc* d, WgradPlan& p) {
  const int K = d->KH * d->KW * d->C1;
  if (d->gather != LVAE_GATHER_CONV || d->x2 != nullptr || d->C2 != 0 || d->in_scale != nullptr) return false;
  if (K > 76 || d->Cout > 64 || d->OH * d->OW > 1024 || d->N < 32 || d->N > 65535) return false;
  if (thin_lds(d) > 160 * 1024) return false;
  p.set_slabs(d->N, (size_t)K * d->Cout, d->Cout);
  return true;
}

static int thin_wgrad_launch(const WgradOp& o, hipStream_t s) {
  const lvae_conv_desc* d = o.d;
  ThinWgradArgs ta;
  ta.d = *d;
  ta.dy = o.dy;
  ta.K = d->KH * d->KW * d->C1;
  ta.PH = d->H + 2 * d->pad;
  ta.PW = d->W + 2 * d->pad;
  ta.slab_w = o.slab_w();
  ta.slab_b = o.slab_b();
  const int rc = launch_lds<conv_wgrad_thin_kernel>("conv_wgrad_thin", dim3(d->N), dim3(256), thin_lds(d), 160 * 1024, s, ta);
  return rc ? rc : wgrad_op_reduce(o, s);
}

static void wgrad_plan(const lvae_conv_desc* d, int& ksplit, int& px_per_split, int& ncit, int& ncot) {
  const int Cin = d->C1 + d->C2, M = d->N * d->OH * d->OW, ntaps = d->KH * d->KW;
  ncit = (Cin + CT - 1) / CT;
  ncot = (d->Cout + CT - 1) / CT;
  const int tiles = ntaps * ncit * ncot;
  int want = (512 + tiles - 1) / tiles;           // ~2 workgroups per CU in total
  if (want > 64) want = 64;                       // bound the slab traffic of small (1x1) filters
  int maxsplit = (M + 255) / 256;                 // at least 8 stages per workgroup
  ksplit = want < 1 ? 1 : want;
  if (ksplit > maxsplit) ksplit = maxsplit;
  if (ksplit < 1) ksplit = 1;
  px_per_split = (M + ksplit - 1) / ksplit;
  px_per_split = (px_per_split + KP - 1) / KP * KP;
  ksplit = (M + px_per_split - 1) / px_per_split;
}

// the generic kernel takes every descriptor
static bool generic_wgrad_plan(const lvae_conv_desc* d, WgradPlan& p) {
  int ksplit, pps, ncit, ncot;
  wgrad_plan(d, ksplit, pps, ncit, ncot);
  p.set_slabs(ksplit, (size_t)d->KH * d->KW * (d->C1 + d->C2) * d->Cout, d->Cout);
  return true;
}

static int generic_wgrad_launch(const WgradOp& o, hipStream_t s) {
  const lvae_conv_desc* d = o.d;
  WgradArgs a;
  a.d = *d;
  a.dy = o.dy;
  a.M = d->N * d->OH * d->OW;
  a.ohw = d->OH * d->OW;
  a.Cin = d->C1 + d->C2;
  a.ntaps = d->KH * d->KW;
  wgrad_plan(d, a.ksplit, a.px_per_split, a.ncit, a.ncot);
  a.slab_w = o.slab_w();
  a.slab_b = o.slab_b();
  const bool xv = (d->C1 % 4 == 0) && (d->C2 % 4 == 0) && al16(d->x) && (!d->x2 || al16(d->x2)) &&
                  (!d->in_scale || (al16(d->in_scale) && al16(d->in_shift)));
  const bool yv = (d->Cout % 4 == 0) && al16(o.dy);
  const int grid = a.ksplit * a.ncot * a.ncit * a.ntaps;
  if (xv && yv) hipLaunchKernelGGL((conv_wgrad_kernel<true, true>), dim3(grid), dim3(256), 0, s, a);
  else if (xv) hipLaunchKernelGGL((conv_wgrad_kernel<true, false>), dim3(grid), dim3(256), 0, s, a);
  else if (yv) hipLaunchKernelGGL((conv_wgrad_kernel<false, true>), dim3(grid), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((conv_wgrad_kernel<false, false>), dim3(grid), dim3(256), 0, s, a);
  LVAE_LAUNCH_CHECK("conv2d_wgrad");
  return wgrad_op_reduce(o, s);
}

// The kernel of a weight gradient: the first family of this table, in its order, whose alignment needs dy and the workspace meet and whose
// plan takes the descriptor. Every lvae_conv2d_wgrad_* query and launch reads the routed plan; the queries, which see no dy, answer for
// 16-byte aligned dy and workspace.
struct WgradFamily {
  int32_t variant;                                    // LVAE_WGRAD_VARIANT_*
  bool (*plan)(const lvae_conv_desc*, WgradPlan&);
  bool dy16, ws16;                                    // needs 16-byte aligned dy / workspace
};
// (The cross-file plans are called through lambdas: tests/test_csrc_layout.py counts a function of lvae_host.h as used by a file that calls
// it, and a bare name in a table is no call.)
static const WgradFamily kWgradFamilies[] = {
    {LVAE_WGRAD_VARIANT_IMG, [](auto d, auto& p) { return conv_wgrad_img_plan(d, p); }, true, true},       // fp32-stored operands of the <= 8x8 levels
    {LVAE_WGRAD_VARIANT_BF16, [](auto d, auto& p) { return conv3x3_wgrad_bf16_plan(d, p); }, true, true},  // precision = LVAE_PREC_BF16
    {LVAE_WGRAD_VARIANT_WINO, [](auto d, auto& p) { return conv_wgrad_wino_plan(d, p); }, true, true},
    {LVAE_WGRAD_VARIANT_DIRECT_1X1, [](auto d, auto& p) { return conv1x1_wgrad_plan(d, p); }, false, false},
    {LVAE_WGRAD_VARIANT_TILE, [](auto d, auto& p) { return conv_wgrad_tile_plan(d, p); }, true, false},
    {LVAE_WGRAD_VARIANT_THIN, thin_wgrad_plan, false, false},
    {LVAE_WGRAD_VARIANT_GENERIC, generic_wgrad_plan, false, false},   // takes everything
};

static WgradPlan wgrad_route(const lvae_conv_desc* d, bool dy16, bool ws16) {
  static const bool halo_off = tune("LVAE_DISABLE_HALO", 0) != 0;  // A/B switch (tuning builds only): the generic kernel for everything
  for (const WgradFamily& f : kWgradFamilies) {
    WgradPlan p;
    p.variant = f.variant;
    if ((f.dy16 && !dy16) || (f.ws16 && !ws16) || (halo_off && f.variant != LVAE_WGRAD_VARIANT_GENERIC)) continue;
    if (f.plan(d, p)) return p;
  }
  return WgradPlan{};   // not reached: the last family takes everything
}

// runs n gradients of one plan: one (n = 1), or a group of wgrad_schedule
static int wgrad_launch(const WgradOp* o, int n, hipStream_t s) {
  switch (o->plan.variant) {
    case LVAE_WGRAD_VARIANT_IMG: return conv_wgrad_img_grouped(o, n, s);
    case LVAE_WGRAD_VARIANT_BF16: return conv3x3_wgrad_bf16_launch(*o, s);
    case LVAE_WGRAD_VARIANT_WINO: return conv_wgrad_wino_launch(o, n, s);
    case LVAE_WGRAD_VARIANT_DIRECT_1X1: return conv1x1_wgrad_launch(*o, s);
    case LVAE_WGRAD_VARIANT_TILE: return conv_wgrad_tile_launch(o, n, s);
    case LVAE_WGRAD_VARIANT_THIN: return thin_wgrad_launch(*o, s);
    default: return generic_wgrad_launch(*o, s);
  }
}

static const std::pair<int32_t, int> kWgradGroupings[] = {   // (variant, capacity) of the families with a grouped launch, in issue order
    {LVAE_WGRAD_VARIANT_TILE, kWgradTileGroup}, {LVAE_WGRAD_VARIANT_WINO, kWgradWinoGroup}, {LVAE_WGRAD_VARIANT_IMG, kWgradImgGroup}};
constexpr int kWgradMaxGroup = std::max({kWgradTileGroup, kWgradWinoGroup, kWgradImgGroup});

// How n routed gradients go out, as the entries of each launch in issue order; a pure function of the plans. First the groups: family by
// family, by ascending key inside a family, entries in index order, a full group flushed at the family's capacity. Then, one by one in
// index order, everything else: plans without a key, and a tile or Winograd gradient left alone in its group (those two families have a
// single-gradient kernel; the whole-image family has one kernel, so its group of one stays in place).
static std::vector<std::vector<int>> wgrad_schedule(const WgradOp* ops, int n) {
  std::vector<std::vector<int>> launches;
  std::vector<char> grouped(n, 0);
  for (const auto& [variant, cap] : kWgradGroupings) {
    std::map<int32_t, std::vector<int>> members;   // key -> its entries
    for (int i = 0; i < n; ++i)
      if (ops[i].plan.variant == variant && ops[i].plan.group >= 0) members[ops[i].plan.group].push_back(i);
    for (const auto& km : members)
      for (size_t m0 = 0; m0 < km.second.size(); m0 += cap) {
        const size_t m1 = std::min(km.second.size(), m0 + cap);
        if (m1 - m0 == 1 && variant != LVAE_WGRAD_VARIANT_IMG) continue;
        launches.emplace_back(km.second.begin() + m0, km.second.begin() + m1);
        for (const int i : launches.back()) grouped[i] = 1;
      }
  }
  for (int i = 0; i < n; ++i)
    if (!grouped[i]) launches.push_back({i});
  return launches;
}

// the checks of one gradient's operands against its routed plan (have: the bytes behind o.workspace; who: the entry point, and the entry)
static int wgrad_op_check(const WgradOp& o, size_t have, const char* who) {
  LVAE_REQUIRE(have >= o.plan.workspace, LVAE_EWORKSPACE,
               "%s: workspace %zu < %zu (the kernel taken for this dy / workspace alignment; lvae_conv2d_wgrad_workspace assumes 16-byte "
               "aligned ones)", who, have, o.plan.workspace);
  LVAE_REQUIRE((o.d->x_dtype == LVAE_DT_F32 && o.d->y_dtype == LVAE_DT_F32) || o.plan.takes_bf16_storage, LVAE_EINVAL,
               "%s: bf16-stored x / dy need the bf16 weight-gradient kernel, which does not take this shape (lvae_resblock_bf16_storage(d) == 0)", who);
  return 0;
}

}  // namespace lvae

using namespace lvae;

extern "C" size_t lvae_conv2d_wgrad_workspace(const lvae_conv_desc* d) { return d ? wgrad_route(d, true, true).workspace : 0; }

extern "C" int32_t lvae_conv2d_wgrad_variant(const lvae_conv_desc* d) {
  return d ? wgrad_route(d, true, true).variant : LVAE_WGRAD_VARIANT_GENERIC;
}

extern "C" int32_t lvae_conv2d_wgrad_apply_ok(const lvae_conv_desc* d) { return d && wgrad_route(d, true, true).apply_ok ? 1 : 0; }

extern "C" int lvae_conv2d_wgrad_f32(const lvae_conv_desc* d, const float* dy, float* dw, float* db, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  int rc = conv_desc_check(d, "lvae_conv2d_wgrad_f32");
  if (rc) return rc;
  LVAE_REQUIRE(dy && dw && workspace, LVAE_EINVAL, "lvae_conv2d_wgrad_f32: null dy/dw/workspace");
  const WgradOp o{d, wgrad_route(d, al16(dy), al16(workspace)), dy, dw, db, workspace};
  rc = wgrad_op_check(o, workspace_bytes, "lvae_conv2d_wgrad_f32");
  return rc ? rc : wgrad_launch(&o, 1, (hipStream_t)stream);
}

extern "C" int lvae_conv2d_wgrad_apply_f32(const lvae_conv_desc* d, const lvae_bn_apply* ap, float* dw, float* db, void* workspace,
                                           size_t workspace_bytes, void* stream) {
  const char* who = "lvae_conv2d_wgrad_apply_f32";
  int rc = conv_desc_check(d, who);
  if (rc) return rc;
  const WgradOp o{d, wgrad_route(d, true, true), nullptr, dw, db, workspace};
  LVAE_REQUIRE(o.plan.apply_ok, LVAE_EINVAL,
               "%s: shape not supported (the Winograd-domain fp32 weight gradient of a 64 -> 64 layer, W = 16 or 32): "
               "use lvae_affine_act_bwd_parts_f32 + lvae_conv2d_wgrad_f32", who);
  LVAE_REQUIRE(dw && workspace, LVAE_EINVAL, "%s: null dw / workspace", who);
  rc = bn_apply_check(who, ap, (int64_t)d->N * d->H * d->W, BN_AP_DROP);
  if (rc) return rc;
  LVAE_REQUIRE(workspace_bytes >= o.plan.workspace, LVAE_EWORKSPACE, "%s: workspace %zu < %zu", who, workspace_bytes, o.plan.workspace);
  LVAE_REQUIRE(al16(workspace), LVAE_EALIGN, "%s: workspace must be 16-byte aligned", who);
  return conv_wgrad_wino_apply_launch(o, ap, (hipStream_t)stream);
}

// The pair of a residual block (A = conv1 with the apply in front, B = conv2): both routed to the Winograd family, A with apply_ok, one
// geometry, 64 output channels, fp32 arithmetic and storage. Reads plans only; pa / pb come back as the pair launch splits them.
static bool wgrad_pair_route(const lvae_conv_desc* a, const lvae_conv_desc* b, WgradPlan& pa, WgradPlan& pb, int32_t* sched) {
  if (!a || !b) return false;
  pa = wgrad_route(a, true, true);
  pb = wgrad_route(b, true, true);
  if (pa.variant != LVAE_WGRAD_VARIANT_WINO || pb.variant != LVAE_WGRAD_VARIANT_WINO || !pa.apply_ok) return false;
  const bool same = a->N == b->N && a->H == b->H && a->W == b->W && a->OH == b->OH && a->OW == b->OW && a->C1 == b->C1 && a->C2 == b->C2 &&
                    a->KH == b->KH && a->KW == b->KW && a->stride == b->stride && a->pad == b->pad && a->gather == b->gather;
  const auto f32 = [](const lvae_conv_desc* d) { return d->precision == LVAE_PREC_F32 && d->x_dtype == LVAE_DT_F32 && d->y_dtype == LVAE_DT_F32; };
  if (!same || a->Cout != 64 || b->Cout != 64 || !f32(a) || !f32(b)) return false;
  return conv_wgrad_wino_pair_plan(a, b, pa, pb, sched);
}
// a gradient's 256-byte aligned piece of a workspace that several share (the pair below, the grouped call)
static size_t wgrad_piece(const WgradPlan& aligned) { return (aligned.workspace + 255) / 256 * 256; }

extern "C" int32_t lvae_conv2d_wgrad_pair_ok(const lvae_conv_desc* a, const lvae_conv_desc* b) {
  WgradPlan pa, pb;
  return wgrad_pair_route(a, b, pa, pb, nullptr) ? 1 : 0;
}

extern "C" size_t lvae_conv2d_wgrad_pair_workspace(const lvae_conv_desc* a, const lvae_conv_desc* b) {
  WgradPlan pa, pb;
  return wgrad_pair_route(a, b, pa, pb, nullptr) ? wgrad_piece(pa) + wgrad_piece(pb) : 0;
}

extern "C" int32_t lvae_conv2d_wgrad_pair_schedule(const lvae_conv_desc* a, const lvae_conv_desc* b, int32_t* sched) {
  WgradPlan pa, pb;
  return sched && wgrad_pair_route(a, b, pa, pb, sched) ? 1 : 0;
}

extern "C" int lvae_conv2d_wgrad_pair_f32(const lvae_conv_desc* a, const lvae_bn_apply* ap, const lvae_conv_desc* b, const float* dy_b,
                                          float* dw_a, float* db_a, float* dw_b, float* db_b, void* workspace, size_t workspace_bytes,
                                          void* stream) {
  const char* who = "lvae_conv2d_wgrad_pair_f32";
  int rc = conv_desc_check(a, who);
  if (!rc) rc = conv_desc_check(b, who);
  if (rc) return rc;
  WgradPlan pa, pb;
  LVAE_REQUIRE(wgrad_pair_route(a, b, pa, pb, nullptr), LVAE_EINVAL,
               "%s: not a pair (two Winograd-domain fp32 weight gradients of 64 -> 64 layers of one geometry, W = 16 or 32, fp32 storage; "
               "lvae_conv2d_wgrad_pair_ok): use lvae_conv2d_wgrad_apply_f32 + lvae_conv2d_wgrad_f32", who);
  LVAE_REQUIRE(dy_b && dw_a && dw_b && workspace, LVAE_EINVAL, "%s: null dy of B / dw / workspace", who);
  rc = bn_apply_check(who, ap, (int64_t)a->N * a->H * a->W, BN_AP_DROP);
  if (rc) return rc;
  const size_t piece_a = wgrad_piece(pa), need = piece_a + wgrad_piece(pb);
  LVAE_REQUIRE(workspace_bytes >= need, LVAE_EWORKSPACE, "%s: workspace %zu < %zu", who, workspace_bytes, need);
  LVAE_REQUIRE(al16(workspace) && al16(dy_b), LVAE_EALIGN, "%s: %s must be 16-byte aligned", who, al16(workspace) ? "dy_b" : "workspace");
  const WgradOp oa{a, pa, nullptr, dw_a, db_a, workspace}, ob{b, pb, dy_b, dw_b, db_b, static_cast<char*>(workspace) + piece_a};
  return conv_wgrad_wino_pair_launch(oa, ap, ob, (hipStream_t)stream);
}

// The shared launch of n = 1 to 3 gradients that each have a real dy (aps, if not null: the deferred apply in front of each, all null —
// a gradient whose dy an apply still has to form belongs to the pair launch): all shapes of the Winograd family, one N, H, W, at most 64
// output channels, fp32 arithmetic and storage. The call is an explicit request for that family: neither the table's order (the 8x8 level's
// single gradients go to the whole-image family first) nor the grouped call's pixel limit is asked. Reads plans only; p[i] come back as the
// shared launch splits them.
static bool wgrad_shared_route(const lvae_conv_desc* descs, const lvae_bn_apply* const* aps, int32_t n, WgradPlan* p, int32_t* sched) {
  if (!descs || n < 1 || n > kWgradWinoShared) return false;
  const lvae_conv_desc* d[kWgradWinoShared];
  for (int i = 0; i < n; ++i) {
    d[i] = &descs[i];
    if (aps && aps[i]) return false;
    p[i] = WgradPlan{};
    p[i].variant = LVAE_WGRAD_VARIANT_WINO;
    if (d[i]->Cout > 64) return false;
    if (d[i]->precision != LVAE_PREC_F32 || d[i]->x_dtype != LVAE_DT_F32 || d[i]->y_dtype != LVAE_DT_F32) return false;
    if (d[i]->N != d[0]->N || d[i]->H != d[0]->H || d[i]->W != d[0]->W) return false;
  }
  return conv_wgrad_wino_shared_plan(d, n, p, sched);
}

extern "C" int32_t lvae_conv2d_wgrad_shared_ok(const lvae_conv_desc* descs, const lvae_bn_apply* const* aps, int32_t n) {
  WgradPlan p[kWgradWinoShared];
  return wgrad_shared_route(descs, aps, n, p, nullptr) ? 1 : 0;
}

extern "C" size_t lvae_conv2d_wgrad_shared_workspace(const lvae_conv_desc* descs, int32_t n) {
  WgradPlan p[kWgradWinoShared];
  if (!wgrad_shared_route(descs, nullptr, n, p, nullptr)) return 0;
  size_t tot = 0;
  for (int i = 0; i < n; ++i) tot += wgrad_piece(p[i]);
  return tot;
}

extern "C" int32_t lvae_conv2d_wgrad_shared_schedule(const lvae_conv_desc* descs, const lvae_bn_apply* const* aps, int32_t n, int32_t* sched) {
  WgradPlan p[kWgradWinoShared];
  return sched && wgrad_shared_route(descs, aps, n, p, sched) ? 1 : 0;
}

extern "C" int lvae_conv2d_wgrad_shared_f32(const lvae_conv_desc* descs, const float* const* dy, float* const* dw, float* const* db, int32_t n,
                                            void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "lvae_conv2d_wgrad_shared_f32";
  LVAE_REQUIRE(descs && dy && dw && db && n >= 1 && n <= kWgradWinoShared && workspace, LVAE_EINVAL, "%s: bad arguments (1 to 3 gradients)", who);
  for (int i = 0; i < n; ++i) {
    const int rc = conv_desc_check(&descs[i], who);
    if (rc) return rc;
    LVAE_REQUIRE(dy[i] && dw[i], LVAE_EINVAL, "%s: null dy/dw at %d (a gradient whose dy an apply has yet to form is not taken here)", who, i);
  }
  WgradPlan p[kWgradWinoShared];
  LVAE_REQUIRE(wgrad_shared_route(descs, nullptr, n, p, nullptr), LVAE_EINVAL,
               "%s: not a shared launch (1 to 3 Winograd-domain fp32 weight gradients of one N, H, W with 32 or 64 input and at most 64 output "
               "channels, fp32 storage; lvae_conv2d_wgrad_shared_ok): use lvae_conv2d_wgrad_f32 per gradient", who);
  size_t need = 0;
  for (int i = 0; i < n; ++i) need += wgrad_piece(p[i]);
  LVAE_REQUIRE(workspace_bytes >= need, LVAE_EWORKSPACE, "%s: workspace %zu < %zu", who, workspace_bytes, need);
  LVAE_REQUIRE(al16(workspace), LVAE_EALIGN, "%s: workspace must be 16-byte aligned", who);
  WgradOp ops[kWgradWinoShared];
  char* ws = static_cast<char*>(workspace);
  for (int i = 0; i < n; ++i) {
    LVAE_REQUIRE(al16(dy[i]), LVAE_EALIGN, "%s: dy[%d] must be 16-byte aligned", who, i);
    for (int j = 0; j < i; ++j) LVAE_REQUIRE(dw[i] != dw[j], LVAE_EINVAL, "%s: entries %d and %d accumulate into one dw", who, j, i);
    ops[i] = WgradOp{&descs[i], p[i], dy[i], dw[i], db[i], ws};
    ws += wgrad_piece(p[i]);
  }
  return conv_wgrad_wino_shared_launch(ops, n, (hipStream_t)stream);
}

extern "C" int lvae_conv2d_wgrad_bf16(const lvae_conv_desc* d, const float* dy, float* dw, float* db, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  LVAE_REQUIRE(d != nullptr, LVAE_EINVAL, "lvae_conv2d_wgrad_bf16: null descriptor");
  lvae_conv_desc dd = *d;
  dd.precision = LVAE_PREC_BF16;
  return lvae_conv2d_wgrad_f32(&dd, dy, dw, db, workspace, workspace_bytes, stream);
}

// n independent weight gradients; same result as n calls of lvae_conv2d_wgrad_f32. Every entry is routed once (again only where its dy or
// its workspace is not 16-byte aligned) and owns a 256-byte aligned piece of the workspace; wgrad_schedule says which entries share a launch.

extern "C" size_t lvae_conv2d_wgrad_grouped_workspace(const lvae_conv_desc* descs, int32_t n) {
  size_t tot = 0;
  for (int i = 0; descs && i < n; ++i) tot += wgrad_piece(wgrad_route(&descs[i], true, true));
  return tot;
}

extern "C" int32_t lvae_conv2d_wgrad_grouped_schedule(const lvae_conv_desc* descs, int32_t n, int32_t* launch_of) {
  if (!descs || !launch_of || n <= 0) return 0;
  std::vector<WgradOp> ops(n);
  for (int i = 0; i < n; ++i) ops[i].plan = wgrad_route(&descs[i], true, true);
  const std::vector<std::vector<int>> launches = wgrad_schedule(ops.data(), n);
  for (size_t l = 0; l < launches.size(); ++l)
    for (const int i : launches[l]) launch_of[i] = (int32_t)l;
  return (int32_t)launches.size();
}

extern "C" int lvae_conv2d_wgrad_grouped_f32(const lvae_conv_desc* descs, const float* const* dy, float* const* dw,
                                             float* const* db, int32_t n, void* workspace, size_t workspace_bytes,
                                             void* stream) {
  const char* who = "lvae_conv2d_wgrad_grouped_f32";
  LVAE_REQUIRE(descs && dy && dw && db && n > 0 && n <= 4096 && workspace, LVAE_EINVAL, "%s: bad arguments", who);
  std::vector<WgradOp> ops(n);
  char* ws = static_cast<char*>(workspace);
  for (int i = 0; i < n; ++i) {
    const lvae_conv_desc* d = &descs[i];
    int rc = conv_desc_check(d, who);
    if (rc) return rc;
    LVAE_REQUIRE(dy[i] && dw[i], LVAE_EINVAL, "%s: null dy/dw at %d", who, i);
    WgradPlan p = wgrad_route(d, true, true);
    const size_t piece = wgrad_piece(p);
    LVAE_REQUIRE((size_t)(ws - static_cast<char*>(workspace)) + piece <= workspace_bytes, LVAE_EWORKSPACE, "%s: workspace %zu < %zu", who,
                 workspace_bytes, lvae_conv2d_wgrad_grouped_workspace(descs, n));
    if (!al16(dy[i]) || !al16(ws)) p = wgrad_route(d, al16(dy[i]), al16(ws));
    ops[i] = WgradOp{d, p, dy[i], dw[i], db[i], ws};
    char entry[64];
    snprintf(entry, sizeof entry, "%s: entry %d", who, i);
    rc = wgrad_op_check(ops[i], piece, entry);
    if (rc) return rc;
    ws += piece;
  }
  WgradOp group[kWgradMaxGroup];
  for (const std::vector<int>& l : wgrad_schedule(ops.data(), n)) {
    for (size_t j = 0; j < l.size(); ++j) group[j] = ops[l[j]];
    const int rc = wgrad_launch(group, (int)l.size(), (hipStream_t)stream);
    if (rc) return rc;
  }
  return 0;
}
