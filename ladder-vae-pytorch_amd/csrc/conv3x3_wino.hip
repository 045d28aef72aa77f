// Winograd F(2x2, 3x3) for the large 3x3 / stride 1 / pad 1 convolutions (forward and dgrad), fp32 throughout.
//
// On gfx950 the fp32 MFMA runs at the fp32 vector rate, and these layers are bound by it. Winograd's
// minimal filtering computes each 2x2 output block from a 4x4 input block with 16 instead of 36 multiplies per
// (ci, co) pair: 2.25x less MFMA work, same fp32 data, transforms are exact +/- combinations (F(2,3) has only
// 0, +-1, +-1/2 coefficients, so the extra rounding is a few ulp).
//
//   U[p] = G g G^T        (16 position matrices [Cout][Cin], made by wino_weight_kernel / wino_weight_batched_kernel)
//   V[p] = B^T d B        (input transform, in registers, straight from the LDS-resident halo patch)
//   M[p] = V[p] * U[p]    (16 independent GEMMs over Cin on v_mfma_f32_32x32x2_f32)
//   Y    = A^T M A        (inverse transform: lane-local, because accumulator register r of every position holds the same
//                          (tile, co) element)
//
// Workgroup: 128 output pixels = 32 Winograd tiles x 64 output channels, 4 waves. Wave i owns row i of the 4x4 position
// grid (positions 4i..4i+3) for all 32 tiles and all 64 channels: its share of the input transform needs only two rows of
// the 4x4 pixel block (8 ds_read_b128 + 32 VALU per 8 channels) and feeds 32 MFMAs, so the vector ALU — which the fp32
// MFMA shares its datapath with — stays almost idle. U fragments come straight from L2 (U is laid out so that one wave
// load is 1 KB contiguous), which removes every barrier from the reduction loop except the four that publish the
// 16-channel slices of the halo patch; those slices are fetched one ahead of the MFMAs that consume them.
// The inverse transform is separable: each wave reduces its row to R[i][b] = sum_j M[i][j] A[j][b] lane-locally,
// the four rows meet in LDS, and the store pass forms Y[a][b] = sum_i A[a][i] R[i][b] with bias/dropout/activation.
#include <stdlib.h>
#include <string.h>

#include "bf16_frag.h"
#include "bn_stats.h"
#include "lvae_host.h"

// build-time experiment switches of the profiling builds (tools/wino_ab.sh); the defaults are the product
#ifndef LVAE_W1_RING
#define LVAE_W1_RING 3
#endif

namespace lvae {

struct WinoArgs {
  lvae_conv_desc d;
  const float* U;  // [16][8][2][Npad][4]: position, k/8, (k/4)&1, n, k&3; six-product form: bf16 [16][4 k16][Npad/32][3 pieces][64 lanes][8]
  int TH, TW, NI, tiles_h, halo_w, halo_h, halo_px, ntn, Npad, tiles_x, wt_per_img, n_wt, Cin;
  uint32_t m_thw, m_per_img, m_halo_w, m_tiles_x, m_wt_per_img, m_tw;
  lvae_bn_fold f;   // copy of *d.in_fold (f.parts == nullptr: none): BatchNorm finalize of the input in the prologue, wino_fold_bn
  int store_pivot;  // the statistics epilogue also stores its pivot behind the partial rows (for a consumer that folds the finalize)
  // GateLayer2d fused behind the convolution (conv3x3_wino2_kernel<true>, lvae_resblock_conv_f32 with LVAE_RB_EPI_GATE): pre-split 1x1
  // weights [k-step 4][32-column tile 4][piece 3][lane][8] (resblock_img.hip's layout), bias [128], residual rows, outputs
  const __bf16* g_ws;
  const float* g_bias;
  const float* g_res;
  float* g_ab;
  float* g_out;
  float* g_stats;
  const float* g_pivot;
  int g_act;
};

// Six-product form (conv3x3_wino_kernel<.., SPL = true>): U[p][k][n] split exactly into three bf16 pieces, stored in the B-fragment order of
// v_mfma_f32_32x32x16_bf16: [position 16][k16 step 4][32-channel output block][piece 3][lane 64][8], lane = 32 * ((k >> 3) & 1) + (n & 31),
// element = k & 7, so that one wave load is 1 KB contiguous.
__device__ __forceinline__ void store_u_split(__bf16* U3, int NB, int p, int k, int n, float v) {
  const size_t base = (((size_t)(p * 4 + (k >> 4)) * NB + (n >> 5)) * 3 * 64 + ((k >> 3) & 1) * 32 + (n & 31)) * 8 + (k & 7);
  float r = v;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const __bf16 b = (__bf16)r;
    U3[base + (size_t)q * 512] = b;
    r -= (float)b;  // exact: the remainder of a round-to-nearest to 8 bits has at most 16 significant bits
  }
}

// ---- weight transform: U[p] = (G g G^T)[p] with g[kh][kw] = w[tap(kh,kw)][k][n] (taps flipped for dgrad); split != 0: store_u_split
__global__ __launch_bounds__(256) void wino_weight_kernel(const float* __restrict__ w, int64_t stap, int64_t sk, int64_t sn,
                                                           int K, int Kpad, int N, int Npad, int flip, float* __restrict__ U, int split) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= Npad * Kpad) return;
  // consecutive threads -> consecutive floats of one position slab [8][2][Npad][4]
  const int e = idx & 3, n = (idx >> 2) % Npad, kq = (idx >> 2) / Npad;  // kq = k / 4
  const int k = kq * 4 + e;
  float g[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const int tap = flip ? (2 - a) * 3 + (2 - b) : a * 3 + b;
      g[a][b] = (n < N && k < K) ? w[tap * stap + (int64_t)k * sk + (int64_t)n * sn] : 0.f;
    }
  // G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]]
  float t[4][3];
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    t[0][b] = g[0][b];
    t[1][b] = 0.5f * (g[0][b] + g[1][b] + g[2][b]);
    t[2][b] = 0.5f * (g[0][b] - g[1][b] + g[2][b]);
    t[3][b] = g[2][b];
  }
  const size_t slab = (size_t)Npad * Kpad;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const float u0 = t[a][0], u1 = 0.5f * (t[a][0] + t[a][1] + t[a][2]), u2 = 0.5f * (t[a][0] - t[a][1] + t[a][2]), u3 = t[a][2];
    if (split) {
      __bf16* U3 = reinterpret_cast<__bf16*>(U);
      store_u_split(U3, Npad >> 5, a * 4, k, n, u0);
      store_u_split(U3, Npad >> 5, a * 4 + 1, k, n, u1);
      store_u_split(U3, Npad >> 5, a * 4 + 2, k, n, u2);
      store_u_split(U3, Npad >> 5, a * 4 + 3, k, n, u3);
    } else {
      float* dst = U + (size_t)(a * 4) * slab + idx;
      dst[0] = u0;
      dst[slab] = u1;
      dst[2 * slab] = u2;
      dst[3 * slab] = u3;
    }
  }
}

// ---- the same transform for many weight tensors in one launch (blockIdx.y = entry): lvae_conv2d_prepare_weights
struct WinoPrepEntry {
  const float* w;
  float* U;
  int64_t stap, sk, sn;
  int32_t K, N, Npad, flip;
  int32_t Kpad, pad_;
};
static_assert(sizeof(WinoPrepEntry) == 64, "entry layout is part of the C ABI (lvae_conv2d_prepare_entry)");

__global__ __launch_bounds__(256) void wino_weight_batched_kernel(const WinoPrepEntry* __restrict__ entries) {
  const WinoPrepEntry e = entries[blockIdx.y];
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (e.pad_ != 0 && e.pad_ != 16) return;  // a pre-split bf16 entry of the direct kernel: conv3x3_bf16.hip's batched kernel handles it
  if (idx >= e.Npad * e.Kpad) return;
  const int c = idx & 3, n = (idx >> 2) % e.Npad, kq = (idx >> 2) / e.Npad;
  const int k = kq * 4 + c;
  float g[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const int tap = e.flip ? (2 - a) * 3 + (2 - b) : a * 3 + b;
      g[a][b] = (n < e.N && k < e.K) ? e.w[tap * e.stap + (int64_t)k * e.sk + (int64_t)n * e.sn] : 0.f;
    }
  float t[4][3];
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    t[0][b] = g[0][b];
    t[1][b] = 0.5f * (g[0][b] + g[1][b] + g[2][b]);
    t[2][b] = 0.5f * (g[0][b] - g[1][b] + g[2][b]);
    t[3][b] = g[2][b];
  }
  const size_t slab = (size_t)e.Npad * e.Kpad;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const float u0 = t[a][0], u1 = 0.5f * (t[a][0] + t[a][1] + t[a][2]), u2 = 0.5f * (t[a][0] - t[a][1] + t[a][2]), u3 = t[a][2];
    if (e.pad_ == 16) {  // six-product form
      __bf16* U3 = reinterpret_cast<__bf16*>(e.U);
      store_u_split(U3, e.Npad >> 5, a * 4, k, n, u0);
      store_u_split(U3, e.Npad >> 5, a * 4 + 1, k, n, u1);
      store_u_split(U3, e.Npad >> 5, a * 4 + 2, k, n, u2);
      store_u_split(U3, e.Npad >> 5, a * 4 + 3, k, n, u3);
    } else {
      float* dst = e.U + (size_t)(a * 4) * slab + idx;
      dst[0] = u0;
      dst[slab] = u1;
      dst[2 * slab] = u2;
      dst[3 * slab] = u3;
    }
  }
}

constexpr int WLDO = 68;  // R row stride (floats)

// Folded BatchNorm finalize (lvae_bn_fold, same contract as conv3x3_pos_kernel's): every workgroup reduces the producer's partial rows
// [rows][2][C] (+ the pivot row) to the scale / shift of its input transform instead of waiting for a finalize launch of its own
// (5 us + a launch boundary in front of a 20-30 us kernel, 196 times per step); the rows come from L2 with 16-byte loads, eight in flight
// per thread, while the first halo slice is still on its way from HBM. Fixed summation order (thread -> (float4 of the row, row group),
// fp32 within a group, double across groups): deterministic, and every workgroup computes identical coefficients. `writer` (one workgroup)
// publishes (scale, shift, mean, rstd) for the backward and applies the momentum update of the running statistics.
// scratch: [NT / 32][128] floats (may alias memory that is written only after this returns); coef: [128] = scale[64], shift[64]. C <= 64.
template <int NT>
__device__ __forceinline__ void wino_fold_bn(const lvae_bn_fold& f, int C, float* scratch, float* coef, int t, bool writer) {
  constexpr int G = NT / 32;
  const int q = t & 31, g = t >> 5, rows = f.rows;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (2 * q < C)  // float4 q of a row = [sum C][sum of squares C]
    for (int r = g; r < rows; r += 8 * G) {
      f32x4 p[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int rr = r + u * G;
        p[u] = *reinterpret_cast<const f32x4*>(f.parts + ((size_t)(rr < rows ? rr : 0) * 2) * C + 4 * q);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (r + u * G < rows) s += p[u];
    }
  *reinterpret_cast<f32x4*>(scratch + g * 128 + 4 * q) = s;
  __syncthreads();
  if (t < C) {
    double sa = 0.0, sb = 0.0;
#pragma unroll
    for (int k = 0; k < G; ++k) {
      sa += (double)scratch[k * 128 + t];
      sb += (double)scratch[k * 128 + C + t];
    }
    const float pivot = f.parts[((size_t)rows * 2) * C + t];  // the producer's pivot, stored behind its partial rows
    const float gam = f.gamma ? f.gamma[t] : 1.f, bet = f.beta ? f.beta[t] : 0.f;
    const BnChannel r = bn_finalize_channel(sa, sb, pivot, f.M, f.eps, gam, bet);
    coef[t] = r.scale;
    coef[64 + t] = r.shift;
    if (writer) {
      if (f.coef_out) bn_store_coef(f.coef_out, C, t, r);
      if (f.running_mean) bn_update_running(f.running_mean, f.running_var, t, f.running_mean[t], f.running_var[t], f.momentum, r, f.M);
    }
  }
  __syncthreads();
}

// In-kernel phase stamps of the profiling builds (-DLVAE_WINO_DBG with bit 64; tools/wino_phase.sh): s_memtime per wave at the phase
// boundaries, written to a buffer of their own that nothing else reads. Never compiled into the product.
#if defined(LVAE_WINO_DBG) && (LVAE_WINO_DBG & 64)
__device__ unsigned long long g_wino_stamps[8192 * 8];
#define WINO_STAMP(i)                                                                                           \
  do {                                                                                                          \
    if ((threadIdx.x & 63) == 0 && blockIdx.x < 1024)                                                           \
      g_wino_stamps[(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 8 + (i)] = __builtin_amdgcn_s_memtime(); \
  } while (0)
#else
#define WINO_STAMP(i) do {} while (0)
#endif

// CIN: reduction channels padded to 64 or 128 (the DMoL head's dgrad reduces over 100).
// NH: 32-wide output-channel blocks per workgroup. 2 = the layout described above. 1 (64 channels split over two workgroups) is
// for layers with fewer than 256 pixel tiles (the 8x8 level at batch 256): it fills all CUs, halves the dependent MFMA chain
// of a wave, and — one wave per SIMD, nothing else to hide an L2 round trip — keeps its U fragments three k-steps ahead in a
// register ring pinned with sched_barrier.
// MT: 32-tile row blocks per wave. 1 = the layout described above (128 output pixels per workgroup, two workgroups per CU).
// 2 (a round-2 experiment, no longer instantiated) = 256 output pixels per workgroup, ONE workgroup per CU,
// one wave per SIMD with the whole 512-entry register file (sixteen 32x32 accumulators per wave, in AGPRs): every U fragment a wave
// fetches from L2 feeds two MFMAs instead of one (the U stream is 262 KB per workgroup whatever its tile) and a 16x16 level at batch
// 256 is exactly one image per CU. Measured: 46.2 us against 33.6 us at 256x16x16, 165 against 122 us at 32x32 (step 40.3 vs 37.1 ms).
// With one wave per SIMD nothing covers a wave's LDS round trips, the slice barriers or the prologue / epilogue of the only resident
// workgroup, and re-reading U was not what held the two-workgroup form back (reading every k-step's fragments from one hot 8 KB
// changed its time by 1 %).
//
// SPL (six-product form, CIN = 64, MT = 1): the 16 position GEMMs run on the bf16 matrix unit. The input transform is done in fp32 exactly as
// above, for 8 channels per lane and 16-channel step; each transformed value and each U element (pre-split by the weight transform) is an
// exact sum of three bf16 pieces, and the six piece products of order <= 2^-16 are accumulated in fp32 (dropped terms < 2^-24 of a
// product: fp32-equivalent, same parity tolerances). Why: v_mfma_f32_32x32x2_f32 executes on the vector ALU's lanes, so in the fp32 form
// the kernel's 1,726 vector instructions per wave ADD to its 13.65 us of MFMA time (SQ counters: 50 % MFMA, 21 % VALU, 29 % parked);
// v_mfma_f32_32x32x16_bf16 has its own unit, costs 6/16 per fp32-equivalent product and runs beside the vector work.
template <int CIN, int NH, int MT, bool SPL>
__global__ __launch_bounds__(256, MT == 1 ? 2 : 1) void conv3x3_wino_kernel(WinoArgs a) {
  kernarg_warmup<(sizeof(WinoArgs) < 1024 ? sizeof(WinoArgs) : 1024)>();
  static_assert(!SPL || (CIN == 64 && MT == 1 && NH == 2), "six-product form: 64 reduction channels, 128-pixel workgroups");
  constexpr int WLDA = CIN + 4;     // halo pixel stride (floats)
  constexpr int KSTEPS = CIN / 8, NSLICE = CIN / 16;
  constexpr int CW = 32 * NH;       // output channels of this workgroup
  constexpr int C4N = CW / 4;       // float4 per output pixel
  constexpr int PG = 256 / C4N;     // pixel groups of the store pass
  constexpr int NT = 32 * MT;       // Winograd tiles of this workgroup
  constexpr int QN = 4 * NT / PG;   // store passes
  constexpr int RING = NH == 1 ? 3 : 2;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;  // [halo_px][WLDA]; reused as R[4][2][32][WLDO] by the epilogue
  const lvae_conv_desc& d = a.d;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int li = lane & 31, lh = lane >> 5;
#ifdef LVAE_WINO_DBG  // compile-time phase-skip mask of the profiling builds (tools/wino_phase.sh); never defined in the product
  constexpr int dbg = LVAE_WINO_DBG;  // 1: no halo loads, 2: no transform/split/MFMA, 4: no output stores, 8: U from one hot KB, 16: no epilogue at all, 32: no split (MFMAs on raw bits)
#else
  constexpr int dbg = 0;
#endif
  WINO_STAMP(0);
  int bid = blockIdx.x;
  {
    const int nwg = gridDim.x, xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  const int tile_n = bid % a.ntn;
  const int tm = bid / a.ntn;
  const int th_idx = tm % a.tiles_h, ig = tm / a.tiles_h;
  const int n0 = ig * a.NI, oh0 = th_idx * a.TH, co0 = tile_n * CW;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  // ---- halo patch in four 16-channel slices; slot = (pixel, float4 within the slice)
  constexpr int SLOTS = MT == 1 ? 4 : 6;  // per thread and slice: halo_px <= 64 * SLOTS (checked by the launcher)
  const int per_img = a.halo_h * a.halo_w;
  const int hc4 = (t & 3) * 4;
  unsigned hoff[SLOTS];   // global offset (floats) of the pixel, or ~0u when it is padding
  int hlds[SLOTS];        // LDS offset (floats), or -1 when the slot does not exist
#pragma unroll
  for (int u = 0; u < SLOTS; ++u) {
    const int px = (t >> 2) + 64 * u;
    const int img = fastdiv(px, a.m_per_img), r = px - img * per_img;
    const int hy = fastdiv(r, a.m_halo_w), hx = r - hy * a.halo_w;
    const int n = n0 + img, ih = oh0 + hy - 1, iw = hx - 1;
    const bool ok = (n < d.N) & ((unsigned)ih < (unsigned)d.H) & ((unsigned)iw < (unsigned)d.W);
    hoff[u] = ok ? (unsigned)(((n * d.H + ih) * d.W + iw) * a.Cin + hc4) : ~0u;
    hlds[u] = px < a.halo_px ? px * WLDA + hc4 : -1;
  }
  f32x4 hreg[SLOTS];
  unsigned hlive = 0;
  auto load_slice = [&](int c) {
#pragma unroll
    for (int u = 0; u < SLOTS; ++u) {
      const bool live = hoff[u] != ~0u && 16 * c + hc4 < a.Cin;  // channels beyond Cin (CIN padding) read as zero
      const unsigned off = live ? hoff[u] + 16 * c : 0u;
      if (dbg & 1) hreg[u] = zero4;
      else hreg[u] = *reinterpret_cast<const f32x4*>(d.x + off);
      hlive = live ? hlive | (1u << u) : hlive & ~(1u << u);
    }
  };
  __shared__ __attribute__((aligned(16))) float s_coef[128];  // scale[64], shift[64] of a folded BatchNorm finalize
  const bool folded = CIN == 64 && a.f.parts != nullptr;
  const bool bn_in = d.in_scale != nullptr || folded;
  auto store_slice = [&](int c) {
    f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = zero4;
    if (bn_in && 16 * c + hc4 < a.Cin) {
      if (folded) {
        sc = *reinterpret_cast<const f32x4*>(s_coef + 16 * c + hc4);
        sh = *reinterpret_cast<const f32x4*>(s_coef + 64 + 16 * c + hc4);
      } else {
        sc = *reinterpret_cast<const f32x4*>(d.in_scale + 16 * c + hc4);
        sh = *reinterpret_cast<const f32x4*>(d.in_shift + 16 * c + hc4);
      }
    }
#pragma unroll
    for (int u = 0; u < SLOTS; ++u) {
      if (hlds[u] >= 0) {
        f32x4 w = zero4;
        if ((hlive >> u) & 1u) {
          w = hreg[u];
          if (bn_in) w = act_fwd4(w * sc + sh, d.in_act);
        }
        *reinterpret_cast<f32x4*>(As + hlds[u] + 16 * c) = w;
      }
    }
  };
  load_slice(0);

  // ---- this lane's Winograd tile -> top-left halo pixel; this wave's two pixel rows of the 4x4 block
  // B^T rows: [1,0,-1,0], [0,1,1,0], [0,-1,1,0], [0,1,0,-1]  ->  t = d[ra] + sgn * d[rb]
  const int ra = wave == 0 ? 0 : (wave == 2 ? 2 : 1);
  const int rb = wave == 0 ? 2 : (wave == 1 ? 2 : (wave == 2 ? 1 : 3));
  const float sgn = wave == 1 ? 1.f : -1.f;
  const float* pa[MT];
  const float* pb[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    int wt = li + 32 * m;
    if (wt >= a.n_wt) wt = 0;  // unused tile slots compute on a valid address; their results are never stored
    const int wimg = fastdiv(wt, a.m_wt_per_img), wr = wt - wimg * a.wt_per_img;
    const int wty = fastdiv(wr, a.m_tiles_x), wtx = wr - wty * a.tiles_x;
    const int pbase = (wimg * a.halo_h + 2 * wty) * a.halo_w + 2 * wtx;
    pa[m] = As + (size_t)(pbase + ra * a.halo_w) * WLDA + (SPL ? 8 : 4) * lh;
    pb[m] = As + (size_t)(pbase + rb * a.halo_w) * WLDA + (SPL ? 8 : 4) * lh;
  }

  f32x16 acc[MT][4][NH];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int h = 0; h < NH; ++h)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][j][h][r] = 0.f;

  if (folded) wino_fold_bn<256>(a.f, a.Cin, smem, s_coef, t, bid == 0);  // scratch: the halo patch, written only from here on
  store_slice(0);
  load_slice(1);
  __syncthreads();
  WINO_STAMP(1);
  if (!SPL) {
    // ---- U fragments of this wave: positions 4*wave + j, channel halves h; one float4 per (j, h, k-step), straight from L2
    const size_t slab = (size_t)a.Npad * CIN;
    const float* ub = a.U + (size_t)(4 * wave) * slab + ((size_t)lh * a.Npad + co0 + li) * 4;
    const size_t kstep = (size_t)2 * a.Npad * 4;
    f32x4 bf[RING][4][NH];
    auto load_u = [&](int ks, int buf) {
  #pragma unroll
      for (int j = 0; j < 4; ++j)
  #pragma unroll
        for (int h = 0; h < NH; ++h) bf[buf][j][h] = *reinterpret_cast<const f32x4*>(ub + j * slab + ks * kstep + h * 128);
    };
  #pragma unroll
    for (int q = 0; q < RING - 1; ++q) load_u(q, q);

  #pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
      if (ks + RING - 1 < KSTEPS) load_u(ks + RING - 1, (ks + RING - 1) % RING);
      if (NH == 1) __builtin_amdgcn_sched_barrier(0);  // keep the fetch ahead: the scheduler otherwise sinks it next to its use
  #pragma unroll
      for (int m = 0; m < MT; ++m) {
        f32x4 tt[4];
  #pragma unroll
        for (int c = 0; c < 4; ++c) {
          const f32x4 da = *reinterpret_cast<const f32x4*>(pa[m] + c * WLDA + ks * 8);
          const f32x4 db = *reinterpret_cast<const f32x4*>(pb[m] + c * WLDA + ks * 8);
  #pragma unroll
          for (int e = 0; e < 4; ++e) tt[c][e] = __builtin_fmaf(sgn, db[e], da[e]);  // sgn = +-1: exact
        }
        f32x4 vv[4];
        vv[0] = tt[0] - tt[2];
        vv[1] = tt[1] + tt[2];
        vv[2] = tt[2] - tt[1];
        vv[3] = tt[1] - tt[3];
  #pragma unroll
        for (int j = 0; j < 4; ++j)
  #pragma unroll
          for (int h = 0; h < NH; ++h)
  #pragma unroll
            for (int e = 0; e < 4; ++e)
              acc[m][j][h] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv[j][e], bf[ks % RING][j][h][e], acc[m][j][h], 0, 0, 0);
      }
      if (NH == 1) __builtin_amdgcn_sched_barrier(0);
      if ((ks & 1) && ks < KSTEPS - 1) {  // publish the next 16-channel slice, start fetching the one after
        const int c = (ks + 1) >> 1;
        store_slice(c);
        if (c + 1 < NSLICE) load_slice(c + 1);
        __syncthreads();
      }
    }
  } else {
    // ---- six-product form: U pieces of (position 4*wave + j, k16 step s, channel block h, piece q) are 1 KB wave loads. An (s, j)
    // iteration is only 6 * NH MFMAs of 32 cycles, far shorter than an L2 round trip, so the pieces are fetched two iterations ahead
    // (ring of 3, what 256 registers allow: 31.7 us with a ring of 2, 30.4 us with 3 at 256x16x16).
    const int NB = a.Npad >> 5;
    const __bf16* u3 = reinterpret_cast<const __bf16*>(a.U) + ((size_t)(co0 >> 5) * 3 * 64 + lane) * 8;
    constexpr int BR = LVAE_W1_RING;
    bf16x8 bq[BR][NH][3];
    auto load_b = [&](int it, int buf) {  // it = 4 s + j
      const __bf16* p = u3 + ((dbg & 8) ? (size_t)0 : (size_t)((4 * wave + (it & 3)) * 4 + (it >> 2)) * NB * 1536);
#pragma unroll
      for (int h = 0; h < NH; ++h)
#pragma unroll
        for (int q = 0; q < 3; ++q) bq[buf][h][q] = *reinterpret_cast<const bf16x8*>(p + (h * 3 + q) * 512);
    };
#pragma unroll
    for (int it = 0; it < (BR < 4 * NSLICE ? BR - 1 : BR); ++it) load_b(it, it);
#pragma unroll
    for (int s16 = 0; s16 < NSLICE; ++s16) {
      f32x4 tl[4], th[4];  // t = d[ra] + sgn * d[rb] for the four pixel columns, channels 16 s + 8 lh + {0..3 | 4..7}
      if (!(dbg & 2)) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const f32x4 dal = *reinterpret_cast<const f32x4*>(pa[0] + c * WLDA + s16 * 16);
        const f32x4 dah = *reinterpret_cast<const f32x4*>(pa[0] + c * WLDA + s16 * 16 + 4);
        const f32x4 dbl = *reinterpret_cast<const f32x4*>(pb[0] + c * WLDA + s16 * 16);
        const f32x4 dbh = *reinterpret_cast<const f32x4*>(pb[0] + c * WLDA + s16 * 16 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          tl[c][e] = __builtin_fmaf(sgn, dbl[e], dal[e]);  // sgn = +-1: exact
          th[c][e] = __builtin_fmaf(sgn, dbh[e], dah[e]);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int it = 4 * s16 + j;
        if (BR < 4 * NSLICE && it + BR - 1 < 4 * NSLICE) load_b(it + BR - 1, (it + BR - 1) % BR);
        const f32x4 vl = j == 0 ? tl[0] - tl[2] : (j == 1 ? tl[1] + tl[2] : (j == 2 ? tl[2] - tl[1] : tl[1] - tl[3]));
        const f32x4 vh = j == 0 ? th[0] - th[2] : (j == 1 ? th[1] + th[2] : (j == 2 ? th[2] - th[1] : th[1] - th[3]));
        bf16x8 af[3];
        if (dbg & 32) {
          af[0] = __builtin_bit_cast(bf16x8, vl);
          af[1] = __builtin_bit_cast(bf16x8, vh);
          af[2] = __builtin_bit_cast(bf16x8, vl + vh);
        } else {
        split_frag<3>(vl, vh, af);
        }
#pragma unroll
        for (int h = 0; h < NH; ++h) acc[0][j][h] = mfma_pieces<3>(af, bq[it % BR][h], acc[0][j][h]);
      }
      } else {  // dbg & 2: keep the U stream alive, nothing else
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int it = 4 * s16 + j;
          if (BR < 4 * NSLICE && it + BR - 1 < 4 * NSLICE) load_b(it + BR - 1, (it + BR - 1) % BR);
#pragma unroll
          for (int h = 0; h < NH; ++h)
#pragma unroll
            for (int q = 0; q < 3; ++q) acc[0][j][h][q] += (float)bq[it % BR][h][q][0];
        }
      }
      if (s16 < NSLICE - 1) {  // publish the next 16-channel slice, start fetching the one after
        store_slice(s16 + 1);
        if (s16 + 2 < NSLICE) load_slice(s16 + 2);
        __syncthreads();
      }
    }
  }
  WINO_STAMP(2);
  __syncthreads();  // every wave is done with the halo patch: LDS becomes R[wave][b][tile][co]
  WINO_STAMP(3);
  if (dbg & 16) {
    float keep = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int h = 0; h < NH; ++h) keep += acc[0][j][h][j + h];
    if (keep == 12345.678f) d.y[t] = 1.f;
    return;
  }

  // ---- R[i][b] = sum_j M[i][j] A[j][b], A^T = [[1,1,1,0],[0,1,-1,-1]]; accumulator register r <-> tile (r&3) + 8(r>>2) + 4lh
  float* Rs = smem;  // R[wave i][b][NT tiles][WLDO]
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int h = 0; h < NH; ++h)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int tile = 32 * m + (r & 3) + 8 * (r >> 2) + 4 * lh;
        const float r0 = acc[m][0][h][r] + acc[m][1][h][r] + acc[m][2][h][r];
        const float r1 = acc[m][1][h][r] - acc[m][2][h][r] - acc[m][3][h][r];
        float* o = Rs + (size_t)((wave * 2) * NT + tile) * WLDO + h * 32 + li;
        o[0] = r0;
        o[NT * WLDO] = r1;
      }
  __syncthreads();
  WINO_STAMP(4);
  {
    const int c4 = (t % C4N) * 4, col = co0 + c4;
    f32x4 st1 = zero4, st2 = zero4, piv, bsh, bmu, brs;  // BatchNorm partials of the stored values (d.stats_out)
    stats_load_coef4(d.stats_pivot, d.Cout, col, d.stats_out != nullptr, d.stats_mode == LVAE_STATS_BN_BWD, piv, bsh, bmu, brs);
    if (col < d.Cout) {
      f32x4 bias = zero4;
      if (d.bias) bias = *reinterpret_cast<const f32x4*>(d.bias + col);
      const int thw = a.TH * a.TW;
      const int nvalid = min(a.NI, d.N - n0) * thw;
      float* yb = d.y + ((size_t)(n0 * d.H + oh0) * d.W) * d.Cout + col;
#pragma unroll
      for (int q = 0; q < QN; ++q) {
        const int p = t / C4N + PG * q;
        if (p < nvalid) {
          const int img = fastdiv(p, a.m_thw), pr = p - img * thw;
          const int oy = fastdiv(pr, a.m_tw), ox = pr - oy * a.TW;
          const int tile = img * a.wt_per_img + (oy >> 1) * a.tiles_x + (ox >> 1);
          const float* rp = Rs + (size_t)((ox & 1) * NT + tile) * WLDO + c4;  // R[i][b = ox&1][tile]
          const f32x4 R0 = *reinterpret_cast<const f32x4*>(rp);
          const f32x4 R1 = *reinterpret_cast<const f32x4*>(rp + 2 * NT * WLDO);
          const f32x4 R2 = *reinterpret_cast<const f32x4*>(rp + 4 * NT * WLDO);
          const f32x4 R3 = *reinterpret_cast<const f32x4*>(rp + 6 * NT * WLDO);
          f32x4 v = (oy & 1) ? (R1 - R2 - R3) : (R0 + R1 + R2);
          v = v + bias;
          if (d.out_scale) v = v * *reinterpret_cast<const f32x4*>(d.out_scale + (size_t)(n0 + img) * d.Cout + col);
          v = act_fwd4(v, d.out_act);
          if (!(dbg & 4) || v[0] == 12345.678f) store_wt4(yb + (size_t)p * d.Cout, v);
          if (d.stats_mode == LVAE_STATS_BN_BWD) {
            if (d.stats_out) {
              const f32x4 xv = *reinterpret_cast<const f32x4*>(d.stats_x + (size_t)((n0 * d.H + oh0) * d.W + p) * d.Cout + col);
              stats_bwd_accum4(v, xv, piv, bsh, bmu, brs, d.stats_act, st1, st2);
            }
          } else {
            stats_fwd_accum4(v, piv, st1, st2);
          }
        }
      }
    }
    WINO_STAMP(5);
    if (d.stats_out)  // PG pixel groups x CW channels -> one row of partials per pixel tile, the pivot row behind them; R is dead
      stats_reduce_groups<PG, CW>(smem, t / C4N, c4, st1, st2, d.stats_out, tm, d.Cout, co0, a.store_pivot && tm == 0, d.stats_pivot,
                                  gridDim.x / a.ntn);
  }
}


// ------------------------------------------------------------------------------------------------------------------------------------
// conv3x3_wino2_kernel (round 3): the six-product form on 256 output pixels (64 Winograd tiles = two 32-tile blocks) x 64 output
// channels per workgroup, 8 waves, ONE workgroup per CU.
//
// Why: in-kernel stamps of conv3x3_wino_kernel<64, 2, 1, true> at 256x16x16 (tools/wino_stamps.py; per wave: prologue 4.1 k cycles,
// GEMM loop 25.7 k, inverse transform + stores 8.8 k) and its phase-skip builds (U pieces from one hot KB: 25.3 -> 20.8 us) say the loop
// is bound by the stream of pre-split U pieces: 393 KB per workgroup, two workgroups per CU = 786 KB per CU through the L2 -> L1 -> VGPR
// path, which delivers about 70 GB/s per CU (MI355X_MICROARCH.md, "Indexed rows"): 11 us of the 12 us the loop takes. The MFMAs (12.3 k
// cycles per SIMD) and the vector work fit beside it. The stream shrinks only if a fetched fragment feeds more MFMAs, so here a wave
// owns TWO positions (one of the two column pairs of a position row) for BOTH tile blocks: every 1 KB U fragment it loads is the B operand of
// two MFMAs instead of one, the workgroup's 393 KB serve 256 pixels, and the per-CU stream halves. The register budget is unchanged
// (2 blocks x 2 positions x 2 channel halves x 16 accumulators), an (s, position) iteration is 24 MFMAs = 768 cycles, so a ring of
// two fragment sets (one iteration ahead) covers an L2 round trip; three sets spill (29.8 vs 23.6 us).
//   * input transform: the wave needs three of the four pixel columns of its two block rows (t = d[ra] +- d[rb] for columns
//     (0, 2, 1) or (2, 1, 3)): v_first = L0 - L1, v_second = L1 +- L2; 12 ds_read_b128 + 40 VALU per block and 16-channel step.
//   * inverse transform: R[i][b] = sum_j M[i][j] A[j][b] needs both column pairs of row i, i.e. two waves: each writes its partial sums
//     (pair 0: M0 + M1, M1; pair 1: M2, -M2 - M3) and the store pass adds them while it forms Y = A^T R. The eight partial arrays of one
//     32-tile block are 139 KB of LDS, so the two blocks go through the exchange one after the other (the first block's stores drain
//     while the second block is exchanged).
//   * memory order of the epilogue: its stores are write-through stores in inline asm (store_wt4), which the compiler's wait bookkeeping
//     does not see, and a wave's memory counter retires in order. So every global read of the epilogue (bias, statistics coefficients,
//     the Dropout2d mask and stats_x rows of BOTH blocks) is requested around block 0's exchange, branch-free (rows that are not wanted
//     read a dummy address and are replaced afterwards), and closed once (close_load) in front of the first store; every barrier behind
//     it is lds_barrier(). Between the first and the last store no wave waits for memory: 0 full drains behind a write-through store in
//     the compiled code, where there were 5 (profiles/wino2_epilogue_isa.txt, profiles/wino2_epilogue_ab.txt).
// Eligibility (wino2_tile): six-product form, exactly 64 tiles per workgroup whose blocks are the first and second 128 pixels of the
// workgroup's pixel tile, and at least 256 such workgroups; everything else keeps conv3x3_wino_kernel.
// ------------------------------------------------------------------------------------------------------------------------------------
#ifndef LVAE_W2_PAIRSPLIT
#define LVAE_W2_PAIRSPLIT 1
#endif

constexpr int W2_LDS_R = 8 * 2 * 32 * WLDO * 4;  // bytes of the partial-sum exchange of one block

// GATE: the block's GateLayer2d (lib/nn.py:118-126) and residual add run behind the convolution, per 128-pixel block: the store pass keeps
// its four rows of y2 = (conv + bias) * Dropout2d mask in registers (besides storing them for the backward), the rows are split into three
// bf16 planes over the dead partial sums, the 8 waves run the 128 x 128 x 64 gate GEMM as six-product MFMAs (wave = 32 rows x {32 a-columns,
// the matching 32 b-columns}), and a second pass stores ab, out = act(a) * sigmoid(b) + x and the BatchNorm partials of out. There is no
// BatchNorm between conv2 and the gate, so nothing crosses workgroups: the 85 MB gate launch of a 256x16x16 block (25 us in the step)
// becomes ~50 MB of stores and one residual read inside a launch that is already there.
// Memory order as above, within 256 VGPRs: the wave's gate weights (96 VGPRs) are requested ONCE, where block 0's exchange has freed
// acc[0], and kept for block 1; bias, gate bias and the statistics pivot wait in s_coef between their uses; block 0's mask and residual
// rows are requested in front of the exchange. What does not fit beside the gate weights, the gate accumulators and acc[1] are the 32
// VGPRs of block 1's mask and residual rows (66 spilled VGPRs when they are requested with block 0's): they are requested in front of
// block 1's exchange, where the gate accumulators have died, and closed behind its barrier. That wait, the only one behind a store,
// covers block 0's gate stores, which have had the exchange to drain.
template <bool GATE>
__global__ __launch_bounds__(512) void conv3x3_wino2_kernel(WinoArgs a) {
  kernarg_warmup<sizeof(WinoArgs)>();
  constexpr int CIN = 64, WLDA = CIN + 4, NSLICE = CIN / 16, CW = 64, C4N = CW / 4, PG = 512 / C4N, NH = 2;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;  // [halo_px][WLDA]; reused as the partial sums [wave 8][b 2][32 tiles][WLDO] by the epilogue
  const lvae_conv_desc& d = a.d;
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int prow = wave >> 1, jp = wave & 1;  // position row i, column pair: positions 4 i + 2 jp + {0, 1}
  WINO_STAMP(0);
#ifdef LVAE_WINO_DBG  // compile-time phase-skip mask of the profiling builds (tools/wino_ab.sh); never defined in the product
  constexpr int dbg = LVAE_WINO_DBG;  // 1: no halo loads, 4: no output stores, 8: U from one hot KB, 16: no epilogue at all, 32: no split (MFMAs on raw bits)
#else
  constexpr int dbg = 0;
#endif
  int bid = blockIdx.x;
  {
    const int nwg = gridDim.x, xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  const int tile_n = bid % a.ntn;
  const int tm = bid / a.ntn;
  const int th_idx = tm % a.tiles_h, ig = tm / a.tiles_h;
  const int n0 = ig * a.NI, oh0 = th_idx * a.TH, co0 = tile_n * CW;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  // ---- halo patch in four 16-channel slices; slot = (pixel, float4 within the slice); 128 pixels per pass of the 512 threads
  constexpr int SLOTS = 3;  // halo_px <= 384 (checked by the launcher)
  const int per_img = a.halo_h * a.halo_w;
  const int hc4 = (t & 3) * 4;
  unsigned hoff[SLOTS];
  int hlds[SLOTS];
#pragma unroll
  for (int u = 0; u < SLOTS; ++u) {
    const int px = (t >> 2) + 128 * u;
    const int img = fastdiv(px, a.m_per_img), r = px - img * per_img;
    const int hy = fastdiv(r, a.m_halo_w), hx = r - hy * a.halo_w;
    const int n = n0 + img, ih = oh0 + hy - 1, iw = hx - 1;
    const bool ok = (n < d.N) & ((unsigned)ih < (unsigned)d.H) & ((unsigned)iw < (unsigned)d.W) & (px < a.halo_px);
    hoff[u] = ok ? (unsigned)(((n * d.H + ih) * d.W + iw) * a.Cin + hc4) : ~0u;
    // slots beyond the patch write to a dump row of their own behind it (the LDS allocation is sized by the epilogue's exchange, far larger)
    hlds[u] = px < a.halo_px ? px * WLDA + hc4 : a.halo_px * WLDA + 4 * t;
  }
  // scale[64], shift[64] of a folded BatchNorm finalize; GATE: behind the loop the epilogue's per-channel rows bias[64], g_bias[128], g_pivot[64]
  __shared__ __attribute__((aligned(16))) float s_coef[GATE ? 256 : 128];
  const bool folded = a.f.parts != nullptr;
  const bool bn_in = d.in_scale != nullptr || folded;
  f32x4 hreg[SLOTS];
  unsigned hlive = 0;
  auto load_slice = [&](int c) {
#pragma unroll
    for (int u = 0; u < SLOTS; ++u) {
      const bool live = hoff[u] != ~0u && 16 * c + hc4 < a.Cin;
      const unsigned off = live ? hoff[u] + 16 * c : 0u;
      if (dbg & 1) hreg[u] = zero4;
      else hreg[u] = *reinterpret_cast<const f32x4*>(d.x + off);
      hlive = live ? hlive | (1u << u) : hlive & ~(1u << u);
    }
  };
  auto store_slice = [&](int c) {  // straight-line: one wave-uniform branch (fused input transform or not), selects instead of lane branches
    if (bn_in) {
      const int cc = 16 * c + hc4 < a.Cin ? 16 * c + hc4 : 0;
      f32x4 sc, sh;
      if (folded) {
        sc = *reinterpret_cast<const f32x4*>(s_coef + cc);
        sh = *reinterpret_cast<const f32x4*>(s_coef + 64 + cc);
      } else {
        sc = *reinterpret_cast<const f32x4*>(d.in_scale + cc);
        sh = *reinterpret_cast<const f32x4*>(d.in_shift + cc);
      }
#pragma unroll
      for (int u = 0; u < SLOTS; ++u) {
        f32x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = hreg[u][e] * sc[e] + sh[e];
        w = act_fwd4(w, d.in_act);
        const bool live = (hlive >> u) & 1u;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = live ? w[e] : 0.f;
        *reinterpret_cast<f32x4*>(As + hlds[u] + 16 * c) = w;
      }
    } else {
#pragma unroll
      for (int u = 0; u < SLOTS; ++u) {
        f32x4 w = hreg[u];
        const bool live = (hlive >> u) & 1u;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = live ? w[e] : 0.f;
        *reinterpret_cast<f32x4*>(As + hlds[u] + 16 * c) = w;
      }
    }
  };
  load_slice(0);

  // ---- this lane's two Winograd tiles (one per block) -> the two pixel rows of the 4x4 block this wave's position row combines,
  // and its three pixel columns in the order (L0, L1, L2) = (0, 2, 1) | (2, 1, 3): first position L0 - L1, second L1 + s2 * L2
  const int ra = prow == 0 ? 0 : (prow == 2 ? 2 : 1);
  const int rb = prow == 0 ? 2 : (prow == 1 ? 2 : (prow == 2 ? 1 : 3));
  const float sgn = prow == 1 ? 1.f : -1.f;
  const float s2 = jp ? -1.f : 1.f;
  const int col0 = jp ? 2 : 0, col1 = jp ? 1 : 2, col2 = jp ? 3 : 1;
  const float* pa[2];
  const float* pb[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int wt = li + 32 * m;  // n_wt == 64 (launcher)
    const int wimg = fastdiv(wt, a.m_wt_per_img), wr = wt - wimg * a.wt_per_img;
    const int wty = fastdiv(wr, a.m_tiles_x), wtx = wr - wty * a.tiles_x;
    const int pbase = (wimg * a.halo_h + 2 * wty) * a.halo_w + 2 * wtx;
    pa[m] = As + (size_t)(pbase + ra * a.halo_w) * WLDA + 8 * lh;
    pb[m] = As + (size_t)(pbase + rb * a.halo_w) * WLDA + 8 * lh;
  }

  f32x16 acc[2][2][NH];  // [block][position of the pair][channel half]
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int h = 0; h < NH; ++h)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][j][h][r] = 0.f;

  if (folded) wino_fold_bn<512>(a.f, a.Cin, smem, s_coef, t, bid == 0);  // scratch: the halo patch, written only from here on
  store_slice(0);
  load_slice(1);
  __syncthreads();
  WINO_STAMP(1);
  {
    // U pieces of (position p, k16 step s, channel block h, piece q): 1 KB wave loads, fetched two (s, position) iterations ahead
    const int NB = a.Npad >> 5;
    const __bf16* u3 = reinterpret_cast<const __bf16*>(a.U) + ((size_t)(co0 >> 5) * 3 * 64 + lane) * 8;
#ifndef LVAE_W2_RING
#define LVAE_W2_RING 2
#endif
    constexpr int BR = LVAE_W2_RING, NIT = 2 * NSLICE;
    bf16x8 bq[BR][NH][3];
    auto load_b = [&](int it, int buf) {  // it = 2 s + jj
      const __bf16* p = u3 + ((dbg & 8) ? (size_t)0 : (size_t)((4 * prow + 2 * jp + (it & 1)) * 4 + (it >> 1)) * NB * 1536);
#pragma unroll
      for (int h = 0; h < NH; ++h)
#pragma unroll
        for (int q = 0; q < 3; ++q) bq[buf][h][q] = *reinterpret_cast<const bf16x8*>(p + (h * 3 + q) * 512);
    };
#pragma unroll
    for (int it = 0; it < BR - 1; ++it) load_b(it, it);
    // Software pipeline: the A fragments (transform + exact three-piece split, ~60 vector instructions) of step k + 1 are computed
    // while the 12 MFMAs of step k occupy the matrix unit; the last step of a 16-channel slice overlaps the staging of the next
    // slice instead. Steps of a slice: (position jj, block m) = (0,0) (0,1) (1,0) (1,1).
    auto make_af = [&](const f32x4 (&tl)[2][3], const f32x4 (&th)[2][3], int jj, int m, bf16x8 (&af)[3]) {
      f32x4 vl, vh;
      if (jj == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {  // element by element: a packed f32 instruction beside MFMAs costs more than its two halves
          vl[e] = tl[m][0][e] - tl[m][1][e];
          vh[e] = th[m][0][e] - th[m][1][e];
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          vl[e] = __builtin_fmaf(s2, tl[m][2][e], tl[m][1][e]);  // s2 = +-1: exact
          vh[e] = __builtin_fmaf(s2, th[m][2][e], th[m][1][e]);
        }
      }
      if (dbg & 32) {
        af[0] = __builtin_bit_cast(bf16x8, vl);
        af[1] = __builtin_bit_cast(bf16x8, vh);
        af[2] = __builtin_bit_cast(bf16x8, vl + vh);
        return;
      }
#if LVAE_W2_PAIRSPLIT
      split8_3(vl, vh, af);
#else
      split_frag<3>(vl, vh, af);
#endif
    };
#pragma unroll
    for (int s16 = 0; s16 < NSLICE; ++s16) {
      f32x4 tl[2][3], th[2][3];  // t = d[ra] + sgn * d[rb] for the columns (L0, L1, L2), channels 16 s + 8 lh + {0..3 | 4..7}
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {
          const int c = cc == 0 ? col0 : (cc == 1 ? col1 : col2);
          const f32x4 dal = *reinterpret_cast<const f32x4*>(pa[m] + c * WLDA + s16 * 16);
          const f32x4 dah = *reinterpret_cast<const f32x4*>(pa[m] + c * WLDA + s16 * 16 + 4);
          const f32x4 dbl = *reinterpret_cast<const f32x4*>(pb[m] + c * WLDA + s16 * 16);
          const f32x4 dbh = *reinterpret_cast<const f32x4*>(pb[m] + c * WLDA + s16 * 16 + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            tl[m][cc][e] = __builtin_fmaf(sgn, dbl[e], dal[e]);  // sgn = +-1: exact
            th[m][cc][e] = __builtin_fmaf(sgn, dbh[e], dah[e]);
          }
        }
      bf16x8 afc[3], afn[3];
      make_af(tl, th, 0, 0, afc);
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        const int jj = st >> 1, m = st & 1, it = 2 * s16 + jj;
        if (m == 0 && it + BR - 1 < NIT) load_b(it + BR - 1, (it + BR - 1) % BR);
        if (st < 3) {
          make_af(tl, th, (st + 1) >> 1, (st + 1) & 1, afn);
        } else if (s16 < NSLICE - 1) {
          store_slice(s16 + 1);
          if (s16 + 2 < NSLICE) load_slice(s16 + 2);
        }
#pragma unroll
        for (int h = 0; h < NH; ++h)
          acc[m][jj][h] = mfma_pieces<3>(afc, bq[it % BR][h], acc[m][jj][h]);
        if (st < 3) {
#pragma unroll
          for (int q = 0; q < 3; ++q) afc[q] = afn[q];
        }
      }
      if (s16 < NSLICE - 1) __syncthreads();  // the next 16-channel slice is published
    }
  }
  WINO_STAMP(2);
  __syncthreads();  // every wave is done with the halo patch: LDS becomes the partial sums of one block
  WINO_STAMP(3);
  if (dbg & 16) {
    float keep = 0.f;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int h = 0; h < NH; ++h) keep += acc[m][j][h][m + j + h];
    if (keep == 12345.678f) d.y[t] = 1.f;
    return;
  }

  // ---- epilogue, one 32-tile block at a time. Partial sums of R[i][b] = sum_j M[i][j] A[j][b], A^T = [[1,1,1,0],[0,1,-1,-1]]:
  // pair 0 holds (M0, M1) -> (M0 + M1, M1); pair 1 holds (M2, M3) -> (M2, -M2 - M3). Accumulator register r <-> tile (r&3) + 8(r>>2) + 4lh.
  float* Rs = smem;  // [wave][b][32 tiles][WLDO]
  const int c4 = (t % C4N) * 4, col = co0 + c4;
  f32x4 st1 = zero4, st2 = zero4;  // BatchNorm partials of the stored values (d.stats_out)
  const int thw = a.TH * a.TW;
  const int nvalid = min(a.NI, d.N - n0) * thw;
  float* yb = d.y + ((size_t)(n0 * d.H + oh0) * d.W) * d.Cout + col;
  // Everything the epilogue reads from memory is requested BEFORE the kernel's first write-through store and closed (close_load) in
  // front of it: the wave's memory counter retires in order, so a load issued behind such a store, or one the compiler still has open
  // when the store goes out, can only be waited for together with the store's trip to memory (tools/wino2_stats_cost.py: the
  // BatchNorm-backward sums cost 27.6 vs 21.2 us per dgrad launch when their x rows were loaded row by row between the stores).
  // Between the blocks only LDS crosses waves, so every barrier from here on is lds_barrier(). One exception, GATE only: the rows of
  // block 1 do not fit beside the gate weights, the gate accumulators and acc[1] (see the header comment); they are requested where the
  // gate accumulators of block 0 have died, in front of block 1's exchange, and closed behind it.
  const int prow0 = t / C4N;                                       // this thread's rows of a block: prow0 + PG q
  const size_t grow0 = (size_t)(n0 * d.H + oh0) * d.W;             // global pixel row of the workgroup's row 0
  const int gwm = wave >> 1, gwn = wave & 1;                       // GATE: this wave's 32 rows, its a-half column tile (b-half: 2 + gwn)
  const bool want_sx = !GATE && d.stats_out != nullptr && d.stats_mode == LVAE_STATS_BN_BWD && col < d.Cout;
  // Straight-line, as store_slice: a row that is not wanted is loaded from a dummy address (the head of x) and replaced when it is closed,
  // so no lane branch and no wait of its own stands between the requests.
  const bool want_aux = GATE ? a.g_res != nullptr : want_sx;
  const float* const dummy = d.x + c4;
  // (the address goes through an empty asm: left in sight, the compiler loads from both addresses under a lane branch and selects)
  auto pick = [&](bool want, const float* p) {
    const float* r = want ? p : dummy;
    asm("" : "+v"(r));
    return (const __attribute__((address_space(1))) f32x4*)(uintptr_t)r;  // still global memory: no flat load, which would count as LDS traffic too
  };
  // the values of stats_load_coef4 (bn_stats.h) and the bias, requested the same way
  // (GATE takes no statistics of y2: its partials are those of `out`, around g_pivot)
  const bool want_piv = !GATE && d.stats_out != nullptr && col < d.Cout, want_bwd = want_piv && d.stats_mode == LVAE_STATS_BN_BWD;
  const bool want_bias = d.bias != nullptr && col < d.Cout;
  f32x4 piv = zero4, bsh = zero4, bmu = zero4, brs = zero4;
  if (!GATE) {
    piv = *pick(want_piv, d.stats_pivot + col);
    bsh = *pick(want_bwd, d.stats_pivot + d.Cout + col);
    bmu = *pick(want_bwd, d.stats_pivot + 2 * d.Cout + col);
    brs = *pick(want_bwd, d.stats_pivot + 3 * d.Cout + col);
  }
  f32x4 bias = *pick(want_bias, d.bias + col);
  const bool want_msk = d.out_scale != nullptr && col < d.Cout;
  f32x4 msk[2][128 / PG], aux[2][128 / PG];  // Dropout2d mask rows; stats_x rows of the BatchNorm-backward sums | GATE: residual rows
  int rpc[2][128 / PG], rimg[2][128 / PG];   // row and image of each request, ahead of the requests (fastdiv branches on its magic)
  auto index_rows = [&](int m) {
#pragma unroll
    for (int q = 0; q < 128 / PG; ++q) {
      const int p = 128 * m + prow0 + PG * q;
      rpc[m][q] = p < nvalid ? p : 0;
      rimg[m][q] = fastdiv(rpc[m][q], a.m_thw);
    }
  };
  index_rows(0);
  if (!GATE) index_rows(1);
  auto load_rows = [&](int m) {
#pragma unroll
    for (int q = 0; q < 128 / PG; ++q) {
      const int pc = rpc[m][q];
      const float* ap = GATE ? a.g_res + (grow0 + pc) * 64 + c4 : d.stats_x + (size_t)((n0 * d.H + oh0) * d.W + pc) * d.Cout + col;
      aux[m][q] = *pick(want_aux, ap);
      const int imgq = rimg[m][q];
      msk[m][q] = *pick(want_msk, d.out_scale + (size_t)(n0 + imgq) * d.Cout + col);
    }
  };
  auto close_rows = [&](int m) {
#pragma unroll
    for (int q = 0; q < 128 / PG; ++q) {
      close_load(aux[m][q]);
      close_load(msk[m][q]);
      const bool keep = want_aux && (!GATE || 128 * m + prow0 + PG * q < nvalid);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        aux[m][q][e] = keep ? aux[m][q][e] : 0.f;
        msk[m][q][e] = want_msk ? msk[m][q][e] : 1.f;
      }
    }
  };
  bf16x8 gqa[GATE ? 4 : 1][3], gqb[GATE ? 4 : 1][3];  // GATE: the wave's gate weights, loaded once for both blocks
  // GATE: the gate's bias halves and the pivot of its statistics (16 registers with the bias, which do not fit beside the gate weights:
  // once closed they wait in s_coef, dead since the barrier behind the loop, and are read back where they are used)
  const bool want_gb = GATE && a.g_bias != nullptr, want_gp = GATE && a.g_stats != nullptr;
  f32x4 gba0 = *pick(want_gb, a.g_bias + c4);
  f32x4 gbb0 = *pick(want_gb, a.g_bias + 64 + c4);
  f32x4 gpiv0 = *pick(want_gp, a.g_pivot + c4);
  load_rows(0);
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    if (m) {
      WINO_STAMP(5);
      lds_barrier();  // the last pass of block 0 has read its LDS area; its write-through stores drain meanwhile
      if (GATE) {
        index_rows(1);
        load_rows(1);
      }
    }
#pragma unroll
    for (int h = 0; h < NH; ++h)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int tile = (r & 3) + 8 * (r >> 2) + 4 * lh;
        const float m0 = acc[m][0][h][r], m1 = acc[m][1][h][r];
        const float r0 = jp ? m0 : m0 + m1;
        const float r1 = jp ? -m0 - m1 : m1;
        float* o = Rs + (size_t)((wave * 2) * 32 + tile) * WLDO + h * 32 + li;
        o[0] = r0;
        o[32 * WLDO] = r1;
      }
    if (m == 0) {  // acc[0] is dead: its registers take what is left to request
      if (GATE) {
        const __bf16* gws = a.g_ws + lane * 8;
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            gqa[s4][k] = *reinterpret_cast<const bf16x8*>(gws + ((size_t)(s4 * 4 + gwn) * 3 + k) * 512);
            gqb[s4][k] = *reinterpret_cast<const bf16x8*>(gws + ((size_t)(s4 * 4 + 2 + gwn) * 3 + k) * 512);
          }
      } else {
        load_rows(1);
      }
    }
    lds_barrier();
    if (m == 0) WINO_STAMP(4); else WINO_STAMP(6);
    if (m == 0) {  // the one wait for memory of the epilogue, in front of the first store
      if (!GATE) {
        close_load(piv);
        close_load(bsh);
        close_load(bmu);
        close_load(brs);
        close_load(bias);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          piv[e] = want_piv ? piv[e] : 0.f;
          bsh[e] = want_bwd ? bsh[e] : piv[e];
          bmu[e] = want_bwd ? bmu[e] : piv[e];
          brs[e] = want_bwd ? brs[e] : piv[e];
          bias[e] = want_bias ? bias[e] : 0.f;
        }
      }
      close_rows(0);
      if (GATE) {
        // the per-channel rows go into s_coef for the later passes (published by the barrier behind this store pass, which itself
        // takes the bias from the register)
        close_load(bias);
        close_load(gba0);
        close_load(gbb0);
        close_load(gpiv0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          bias[e] = want_bias ? bias[e] : 0.f;
          gba0[e] = want_gb ? gba0[e] : 0.f;
          gbb0[e] = want_gb ? gbb0[e] : 0.f;
          gpiv0[e] = want_gp ? gpiv0[e] : 0.f;
        }
        if (prow0 == 0) {
          *reinterpret_cast<f32x4*>(s_coef + c4) = bias;
          *reinterpret_cast<f32x4*>(s_coef + 64 + c4) = gba0;
          *reinterpret_cast<f32x4*>(s_coef + 128 + c4) = gbb0;
          *reinterpret_cast<f32x4*>(s_coef + 192 + c4) = gpiv0;
        }
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            close_load(gqa[s4][k]);
            close_load(gqb[s4][k]);
          }
      } else {
        close_rows(1);
      }
    } else if (GATE) {
      close_rows(1);
    }
    f32x4 gy[GATE ? 128 / PG : 1];   // GATE: this thread's rows of y2 (zero for rows past the batch)
    if (GATE) {
#pragma unroll
      for (int q = 0; q < 128 / PG; ++q) gy[q] = zero4;
    }
    if (GATE && m == 1) bias = *reinterpret_cast<const f32x4*>(s_coef + c4);
    if (col < d.Cout) {
#pragma unroll
      for (int q = 0; q < 128 / PG; ++q) {
        const int p = 128 * m + prow0 + PG * q;
        if (p < nvalid) {
          const int img = fastdiv(p, a.m_thw), pr = p - img * thw;
          const int oy = fastdiv(pr, a.m_tw), ox = pr - oy * a.TW;
          const int tile = (img * a.wt_per_img + (oy >> 1) * a.tiles_x + (ox >> 1)) & 31;
          // R[i][b = ox&1][tile] = partial of wave 2 i + partial of wave 2 i + 1; Y[a = oy&1] = R0 + R1 + R2 | R1 - R2 - R3
          const float* rp = Rs + (size_t)((ox & 1) * 32 + tile) * WLDO + c4;
          constexpr int WS = 2 * 32 * WLDO;  // floats per wave
          const int i0 = (oy & 1) ? 1 : 0;
          f32x4 Rr[3];
#pragma unroll
          for (int k = 0; k < 3; ++k)
            Rr[k] = *reinterpret_cast<const f32x4*>(rp + (2 * (i0 + k)) * WS) + *reinterpret_cast<const f32x4*>(rp + (2 * (i0 + k) + 1) * WS);
          f32x4 v = (oy & 1) ? (Rr[0] - Rr[1] - Rr[2]) : (Rr[0] + Rr[1] + Rr[2]);
          v = (v + bias) * msk[m][q];
          v = act_fwd4(v, d.out_act);
          if (!(dbg & 4) || v[0] == 12345.678f) store_wt4(yb + (size_t)p * d.Cout, v);
          if (GATE) {
            gy[q] = v;
          } else if (d.stats_mode == LVAE_STATS_BN_BWD) {
            if (d.stats_out) {
              const f32x4 xv = aux[m][q];
              stats_bwd_accum4(v, xv, piv, bsh, bmu, brs, d.stats_act, st1, st2);
            }
          } else {
            stats_fwd_accum4(v, piv, st1, st2);
          }
        }
      }
    }
    if (GATE) {
      constexpr int LDKG = 72, G_PLANE = 128 * LDKG, LDG = 132;   // bf16 row pitch of the y2 planes; float row pitch of the pre-activations
      const size_t grow = grow0 + 128 * m;                         // global pixel row of this block's row 0
      lds_barrier();   // the store pass has read the partial sums: the area becomes the y2 planes [3][128][72] bf16
      __bf16* Gs = reinterpret_cast<__bf16*>(smem);
#pragma unroll
      for (int q = 0; q < 128 / PG; ++q) {
        bf16x4 pl3[3];
        split4<3>(gy[q], pl3);
#pragma unroll
        for (int k = 0; k < 3; ++k) *reinterpret_cast<bf16x4*>(Gs + k * G_PLANE + (prow0 + PG * q) * LDKG + c4) = pl3[k];
      }
      lds_barrier();
      f32x16 acca, accb;
#pragma unroll
      for (int r = 0; r < 16; ++r) acca[r] = accb[r] = 0.f;
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        bf16x8 af[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) af[k] = *reinterpret_cast<const bf16x8*>(Gs + k * G_PLANE + (gwm * 32 + li) * LDKG + 16 * s4 + 8 * lh);
#pragma unroll
        for (int kk = 0; kk < PieceOrder<3>::N; ++kk) {
          acca = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[PieceOrder<3>::A[kk]], gqa[s4][PieceOrder<3>::B[kk]], acca, 0, 0, 0);
          accb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[PieceOrder<3>::A[kk]], gqb[s4][PieceOrder<3>::B[kk]], accb, 0, 0, 0);
        }
      }
      lds_barrier();   // the planes are dead: the area becomes the pre-activation tile [128][132] floats
      float* Qs = smem;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = gwm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        Qs[row * LDG + gwn * 32 + li] = acca[r];
        Qs[row * LDG + 64 + gwn * 32 + li] = accb[r];
      }
      lds_barrier();
      const f32x4 gba = *reinterpret_cast<const f32x4*>(s_coef + 64 + c4), gbb = *reinterpret_cast<const f32x4*>(s_coef + 128 + c4);
      const f32x4 gpiv = *reinterpret_cast<const f32x4*>(s_coef + 192 + c4);
#pragma unroll
      for (int q = 0; q < 128 / PG; ++q) {
        const int pl = prow0 + PG * q;
        if (128 * m + pl < nvalid) {
          const f32x4 av = *reinterpret_cast<const f32x4*>(Qs + pl * LDG + c4) + gba;
          const f32x4 bv = *reinterpret_cast<const f32x4*>(Qs + pl * LDG + 64 + c4) + gbb;
          if (a.g_ab) {
            store_wt4(a.g_ab + (grow + pl) * 128 + c4, av);
            store_wt4(a.g_ab + (grow + pl) * 128 + 64 + c4, bv);
          }
          f32x4 o = act_fwd4(av, a.g_act);
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] *= sigmoidf_(bv[j]);
          o += aux[m][q];
          store_wt4(a.g_out + (grow + pl) * 64 + c4, o);
          stats_fwd_accum4(o, gpiv, st1, st2);
        }
      }
    }
  }
  WINO_STAMP(7);
  float* const so = GATE ? a.g_stats : d.stats_out;
  // PG pixel groups x CW channels -> one row of partials per workgroup, the pivot row behind them (the partial sums in LDS are dead)
  if (GATE && so != nullptr)  // BatchNorm partials of `out` (the next block's first BatchNorm)
    stats_reduce_groups<PG, CW>(smem, t / C4N, c4, st1, st2, so, tm, 64, 0, tm == 0, a.g_pivot, gridDim.x / a.ntn);
  if (!GATE && d.stats_out)
    stats_reduce_groups<PG, CW>(smem, t / C4N, c4, st1, st2, d.stats_out, tm, d.Cout, co0, a.store_pivot && tm == 0, d.stats_pivot,
                                gridDim.x / a.ntn);
}


static int wino_kpad(const lvae_conv_desc* d) { return d->C1 <= 64 ? 64 : 128; }
static bool kpad_is64(const lvae_conv_desc* d) { return d->C1 <= 64; }

static bool wino_tile_for(const lvae_conv_desc* d, int budget, int max_halo, int& TH, int& NI) {
  TH = 0;
  for (int c = 2; c <= d->H; c += 2)
    if (d->H % c == 0 && c * d->W <= budget) TH = c;
  if (TH == 0) return false;
  NI = TH < d->H ? 1 : budget / (TH * d->W);
  if (NI < 1) NI = 1;
  if (NI > d->N) NI = d->N;
  return NI * (TH + 2) * (d->W + 2) <= max_halo;
}

// layers with fewer pixel tiles than CUs run 32-channel workgroups (conv3x3_wino_kernel<64, 1, 1, false>)
static bool wino_narrow(const lvae_conv_desc* d, int TH, int NI) {
  static const int narrow_tiles = (int)tune("LVAE_WINO_NARROW_TILES", 256);
  return kpad_is64(d) && ((d->N + NI - 1) / NI) * (d->H / TH) < narrow_tiles;
}

// six-product form (conv3x3_wino_kernel<64, 2, 1, true>): fp32 precision, 64 reduction channels, at least 256 pixel tiles (the
// 32-channel workgroups of smaller layers are latency chains, one wave per SIMD: 17.5 us in this form against 16.4 us on the fp32 MFMA);
// d->form = LVAE_FORM_F32_MFMA keeps the position GEMMs on the fp32 MFMA
static bool wino_split_form(const lvae_conv_desc* d) {
  if (d->precision != LVAE_PREC_F32 || !kpad_is64(d) || d->form == LVAE_FORM_F32_MFMA) return false;
  int TH, NI;
  return wino_tile_for(d, 128, 256, TH, NI) && !wino_narrow(d, TH, NI);
}

static size_t conv3x3_wino_workspace(const lvae_conv_desc* d) {
  const int ntn = (d->Cout + 63) / 64;
  if (wino_split_form(d)) return (size_t)16 * 4 * (2 * ntn) * 3 * 1024;  // bf16 pieces [16][4 k16][Npad/32][3][64 lanes][8]
  return (size_t)16 * ntn * 64 * wino_kpad(d) * sizeof(float);  // 16 position slabs [Kpad/8][2][Npad][4]
}

static bool conv3x3_wino_eligible(const lvae_conv_desc* d) {
  static const bool off = tune("LVAE_DISABLE_WINO", 0) != 0;  // A/B switch (tuning builds only)
  if (off) return false;
  const int Cin = d->C1;
  if (d->KH != 3 || d->KW != 3 || d->stride != 1 || d->pad != 1 || d->x2 != nullptr || d->OH != d->H || d->OW != d->W) return false;
  if (Cin < 36 || Cin > 128 || Cin % 4 != 0 || d->Cout % 4 != 0 || (d->H & 1) || (d->W & 1) || d->W > 128) return false;
  if (!al16_or_null(d->x) || !al16_or_null(d->y) || !al16_or_null(d->bias) || !al16_or_null(d->in_scale) || !al16_or_null(d->in_shift) || !al16_or_null(d->out_scale)) return false;
  const int64_t M = (int64_t)d->N * d->H * d->W;
  static const int64_t min_m = tune("LVAE_WINO_MIN_M", 256 * 64);
  if (M < min_m || M * 128 >= ((int64_t)1 << 31)) return false;  // large layers only: smaller ones are latency bound
  return true;
}

// Pixel tile of a workgroup: whole rows, even height, <= 128 pixels (32 Winograd tiles); whole images when several fit. (A 256-pixel,
// one-workgroup-per-CU form, MT = 2, was built and measured in round 2: 46.2 us against 33.6 us at 256x16x16; it is no longer compiled.)
struct WinoTile {
  int TH, NI, mt;
};

// conv3x3_wino2_kernel (256 pixels, 8 waves, six-product form): exactly 64 Winograd tiles per workgroup whose two 32-tile blocks are the
// first and the second 128 pixels of the pixel tile (image widths 8, 16, 32, 64), and at least 256 such workgroups
static bool wino2_tile(const lvae_conv_desc* d, int& TH, int& NI) {
  static const bool off = tune("LVAE_DISABLE_WINO2", 0) != 0;  // A/B switch (tuning builds only)
  if (off || !wino_split_form(d) || !wino_tile_for(d, 256, 384, TH, NI)) return false;
  const int tiles_x = d->W / 2, wt_per_img = (TH / 2) * tiles_x;
  if (NI * wt_per_img != 64 || 32 % tiles_x != 0) return false;
  if (wt_per_img % 32 != 0 && 32 % wt_per_img != 0) return false;
  const int64_t groups = (int64_t)((d->N + NI - 1) / NI) * (d->H / TH) * ((d->Cout + 63) / 64);
  return groups >= 256;
}

static bool wino_tile(const lvae_conv_desc* d, WinoTile& w) {
  int TH, NI;
  if (wino2_tile(d, TH, NI)) {
    w = WinoTile{TH, NI, 2};
    return true;
  }
  if (!wino_tile_for(d, 128, 256, TH, NI)) return false;
  w = WinoTile{TH, NI, 1};
  return true;
}

static size_t wino_lds_bytes(const lvae_conv_desc* d, const WinoTile& w) {
  size_t lds = (size_t)w.NI * (w.TH + 2) * (d->W + 2) * (wino_kpad(d) + 4) * sizeof(float);
  const size_t lds_r = w.mt == 2 ? (size_t)W2_LDS_R : (size_t)4 * 2 * 32 * WLDO * sizeof(float);
  return lds < lds_r ? lds_r : lds;
}

// Folded BatchNorm finalize of the input (lvae_bn_fold, wino_fold_bn): 64-channel inputs, and launches of at most two workgroups per CU
// (every workgroup re-reads the producer's partial rows from L2: 128-256 KB each; with four rounds per CU a finalize launch is cheaper)
static bool wino_folds(const lvae_conv_desc* d, const WinoTile& w) {
  static const bool off = tune("LVAE_DISABLE_WINO_FOLD", 0) != 0;  // A/B switch (tuning builds only)
  if (off || d->C1 > 64) return false;
  const bool narrow = w.mt == 1 && wino_narrow(d, w.TH, w.NI);
  const int64_t wgs = (int64_t)((d->N + w.NI - 1) / w.NI) * (d->H / w.TH) * (narrow ? (d->Cout + 31) / 32 : (d->Cout + 63) / 64);
  static const int64_t max_wgs = tune("LVAE_WINO_FOLD_MAX_WGS", 512);
  return wgs <= max_wgs;
}

// plan: the transformed weights in d->workspace (assume_ws: in a sized, 16-byte aligned one, as lvae_conv2d_workspace asks), a pixel
// tile within the LDS limit; one statistics row per pixel tile
bool conv3x3_wino_plan(const lvae_conv_desc* d, bool assume_ws, ConvPlan& p) {
  if (!conv3x3_wino_eligible(d)) return false;
  const size_t ws = conv3x3_wino_workspace(d);
  if (!assume_ws && (d->workspace == nullptr || (size_t)d->workspace_bytes < ws || !al16_or_null(d->workspace))) return false;
  WinoTile w;
  if (!wino_tile(d, w) || wino_lds_bytes(d, w) > 159 * 1024) return false;  // + 512 bytes of static LDS (s_coef)
  p = ConvPlan{};
  p.variant = wino_split_form(d) ? LVAE_VARIANT_WINO_SIX : LVAE_VARIANT_WINO_F32;
  p.rows = ((d->N + w.NI - 1) / w.NI) * (d->H / w.TH);
  p.folds = wino_folds(d, w);
  p.workspace = ws;
  return true;
}

// rows of BatchNorm partials of `out` (= workgroups) when the 256-pixel six-product kernel can run `d` with the GateLayer2d fused behind it
// (lvae_resblock_conv_f32, LVAE_RB_EPI_GATE, for shapes the whole-image kernels of resblock_img.hip do not take): 0 = it cannot
int conv3x3_wino2_gate_rows(const lvae_conv_desc* d) {
  if (d->C1 != 64 || d->Cout != 64 || d->out_act != LVAE_ACT_NONE || d->gather != LVAE_GATHER_CONV) return 0;
  ConvPlan p;
  WinoTile w;
  if (!conv3x3_wino_plan(d, false, p) || (d->in_fold != nullptr && !p.folds) || !wino_tile(d, w) || w.mt != 2) return 0;
  return p.rows;
}

// Runs the plan conv3x3_wino_plan(d) accepted (for a gate: conv3x3_wino2_gate_rows(d) > 0); d->workspace holds the transformed weights
// (written here first unless d->workspace_ready), d->in_fold only when the plan folds.
static int wino_launch(const lvae_conv_desc* d, const lvae_rb_ext* gate, hipStream_t s) {
  WinoTile wtile;
  wino_tile(d, wtile);
  const int Cin = d->C1;
  WinoArgs a;
  a.d = *d;
  const int TH = wtile.TH, NI = wtile.NI, mt = wtile.mt;
  const bool split = wino_split_form(d);
  a.TH = TH;
  a.TW = d->W;
  a.NI = NI;
  a.tiles_h = d->H / TH;
  a.halo_h = TH + 2;
  a.halo_w = d->W + 2;
  a.halo_px = NI * a.halo_h * a.halo_w;
  a.tiles_x = d->W / 2;
  a.wt_per_img = (TH / 2) * a.tiles_x;
  a.n_wt = NI * a.wt_per_img;
  a.Npad = (d->Cout + 63) / 64 * 64;
  const bool narrow = mt == 1 && wino_narrow(d, TH, NI);  // fewer pixel tiles than CUs: 32-channel workgroups
  a.ntn = narrow ? (d->Cout + 31) / 32 : (d->Cout + 63) / 64;
  a.m_thw = fastdiv_magic(TH * d->W);
  a.m_tw = fastdiv_magic(d->W);
  a.m_per_img = fastdiv_magic(a.halo_h * a.halo_w);
  a.m_halo_w = fastdiv_magic(a.halo_w);
  a.m_tiles_x = fastdiv_magic(a.tiles_x);
  a.m_wt_per_img = fastdiv_magic(a.wt_per_img);
  const int kpad = wino_kpad(d);
  a.Cin = Cin;
  const size_t lds = wino_lds_bytes(d, wtile);
  const bool folds = wino_folds(d, wtile);
  a.f = lvae_bn_fold{};
  if (d->in_fold != nullptr) a.f = *d->in_fold;
  a.d.in_fold = nullptr;
  a.store_pivot = folds && d->stats_out != nullptr && d->stats_mode == LVAE_STATS_BN_FWD;
  a.g_ws = nullptr;
  a.g_bias = a.g_res = a.g_pivot = nullptr;
  a.g_ab = a.g_out = a.g_stats = nullptr;
  a.g_act = 0;
  if (gate != nullptr) {
    a.g_ws = static_cast<const __bf16*>(gate->gate_ws);
    a.g_bias = gate->gate_bias;
    a.g_res = gate->res;
    a.g_ab = gate->ab;
    a.g_out = gate->out;
    a.g_stats = gate->out_stats;
    a.g_pivot = gate->out_stats_pivot;
    a.g_act = gate->act;
  }
  float* U = static_cast<float*>(d->workspace);
  a.U = U;
  const int Npad = a.Npad;
  if (!d->workspace_ready) {
    hipLaunchKernelGGL(wino_weight_kernel, dim3((Npad * kpad + 255) / 256), dim3(256), 0, s, d->w, d->w_stap, d->w_sk, d->w_sn, Cin,
                       kpad, d->Cout, Npad, d->gather == LVAE_GATHER_TRANSPOSED ? 1 : 0, U, split ? 1 : 0);
    LVAE_LAUNCH_CHECK("wino_weight");
  }
  const int img_groups = (d->N + NI - 1) / NI;
  const dim3 grid(img_groups * a.tiles_h * a.ntn);
  const char* name = "conv3x3_wino";
  if (mt == 2 && gate != nullptr) return launch_lds<conv3x3_wino2_kernel<true>>(name, grid, dim3(512), lds, 159 * 1024, s, a);
  if (mt == 2) return launch_lds<conv3x3_wino2_kernel<false>>(name, grid, dim3(512), lds, 159 * 1024, s, a);
  if (split) return launch_lds<conv3x3_wino_kernel<64, 2, 1, true>>(name, grid, dim3(256), lds, 80 * 1024, s, a);
  if (narrow) return launch_lds<conv3x3_wino_kernel<64, 1, 1, false>>(name, grid, dim3(256), lds, 80 * 1024, s, a);
  if (kpad == 64) return launch_lds<conv3x3_wino_kernel<64, 2, 1, false>>(name, grid, dim3(256), lds, 80 * 1024, s, a);
  return launch_lds<conv3x3_wino_kernel<128, 2, 1, false>>(name, grid, dim3(256), lds, 159 * 1024, s, a);
}

int conv3x3_wino_launch(const lvae_conv_desc* d, hipStream_t s) { return wino_launch(d, nullptr, s); }

int conv3x3_wino2_gate_launch(const lvae_conv_desc* d, const lvae_rb_ext* gate, hipStream_t s) { return wino_launch(d, gate, s); }

}  // namespace lvae

using namespace lvae;

extern "C" size_t lvae_conv2d_prepare_entry_bytes(void) { return sizeof(WinoPrepEntry); }

extern "C" int lvae_conv2d_prepare_entry(const lvae_conv_desc* d, void* entry) {
  LVAE_REQUIRE(d && entry, LVAE_EINVAL, "lvae_conv2d_prepare_entry: null pointer");
  ConvPlan pos;
  if (!conv3x3_pos_plan(d, pos)) {
    const int form = conv3x3_bf16_form(d);
    if (form != 0) {
      LVAE_REQUIRE(d->workspace && (size_t)d->workspace_bytes >= conv3x3_bf16_workspace(d, form) && al16_or_null(d->workspace), LVAE_EINVAL,
                   "lvae_conv2d_prepare_entry: no scratch for the pre-split weights");
      conv3x3_bf16_prep_entry(d, form, entry);
      return 0;
    }
  }
  LVAE_REQUIRE(conv3x3_wino_eligible(d) && d->workspace && (size_t)d->workspace_bytes >= conv3x3_wino_workspace(d) &&
                   al16_or_null(d->workspace),
               LVAE_EINVAL, "lvae_conv2d_prepare_entry: descriptor has no weight pre-transform (lvae_conv2d_workspace(d) == 0) or no scratch");
  WinoPrepEntry e;
  e.w = d->w;
  e.U = static_cast<float*>(d->workspace);
  e.stap = d->w_stap;
  e.sk = d->w_sk;
  e.sn = d->w_sn;
  e.K = d->C1;
  e.N = d->Cout;
  e.Npad = (d->Cout + 63) / 64 * 64;
  e.flip = d->gather == LVAE_GATHER_TRANSPOSED ? 1 : 0;
  e.Kpad = wino_kpad(d);
  e.pad_ = wino_split_form(d) ? 16 : 0;  // kind: 0 fp32 position slabs, 16 six-product bf16 pieces (1 / 3: conv3x3_bf16.hip's entries)
  memcpy(entry, &e, sizeof(e));
  return 0;
}

extern "C" int lvae_conv2d_prepare_weights(const void* entries, int32_t n, int32_t max_cout, void* stream) {
  LVAE_REQUIRE(entries && n > 0 && n < 65536 && max_cout > 0, LVAE_EINVAL, "lvae_conv2d_prepare_weights: bad arguments");
  const int npad = (max_cout + 63) / 64 * 64;
  hipLaunchKernelGGL(wino_weight_batched_kernel, dim3((npad * 128 + 255) / 256, n), dim3(256), 0, (hipStream_t)stream,
                     static_cast<const WinoPrepEntry*>(entries));
  LVAE_LAUNCH_CHECK("wino_weight_batched");
  return conv3x3_bf16_prepare_batched(entries, n, npad, (hipStream_t)stream);  // entries of the bf16-pipe kernels (kind != 0)
}

#if defined(LVAE_WINO_DBG) && (LVAE_WINO_DBG & 64)
extern "C" int lvae_debug_wino_stamps(void* host_out, size_t bytes) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(lvae::g_wino_stamps), bytes < sizeof(lvae::g_wino_stamps) ? bytes : sizeof(lvae::g_wino_stamps));
}
#endif
