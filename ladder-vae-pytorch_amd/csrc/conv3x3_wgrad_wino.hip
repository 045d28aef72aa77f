// Weight gradient of the large 3x3 / stride 1 / pad 1 convolutions in the Winograd F(2x2,3x3) domain, fp32.
//
//   dg = G^T [ sum_tiles (B^T d B) (.) (A dY A^T) ] G          per (ci, co)
//
// i.e. 16 position GEMMs dU[p][ci][co] = sum_tiles V[p][tile][ci] * W[p][tile][co] with the tile index as the reduction
// dimension: 2.25x fewer fp32 MFMAs than the direct sum over pixels. V = B^T d B comes from the 4x4 input block of the
// tile (with the fused BatchNorm/activation prologue applied while the block is staged), W = A dY A^T from the 2x2 block
// of the output gradient; both transforms have coefficients 0/+-1, so they are exact adds.
//
// Workgroup = (range of 16-tile chunks, block of 32 input channels, group of 64 output channels), 8 waves: wave =
// (position row i, half of the chunk's tiles). The split is over INPUT channels so that the BatchNorm/activation prologue
// (the expensive part of staging) is done once per element; dY, which needs no arithmetic, is the operand staged twice.
// Each wave keeps dU[4i..4i+3][32 ci][64 co] in 128 accumulator registers; per MFMA k-step (two tiles, one per lane half)
// it reads two rows of the 4x4 block (8 ds_read_b32), the 2x2 dY block for both co halves (8 ds_read_b32), spends 22 VALU
// on the row-i transforms and issues 8 MFMAs. Chunks are double-buffered in LDS (pixel strides 48 / 80 floats keep the
// two lane halves on disjoint banks) and fetched one chunk ahead through registers. At the end the two tile halves are
// added through LDS and the workgroup writes one partial slab; conv_wgrad_wino_reduce sums the slabs in a fixed order
// (deterministic), applies G^T . G and accumulates into dw with the caller's strides.
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "bn_apply.h"
#include "lvae_host.h"

namespace lvae {

struct WgWinoArgs {
  lvae_conv_desc d;
  const float* dy;
  float* slab_w;  // [nranges][ncib ci blocks][ncog][32 ci][16 positions][64 co]: 4 KB contiguous per input channel
  float* slab_b;  // [nranges][ncog][64] or nullptr
  int nranges, ncog, cpr, total_chunks, cpi;
  uint32_t m_cpi;
  int ncib, pad_;  // blocks of 32 input channels: C1 / 32 = 1 or 2
};

constexpr int WG_XS = 48;  // x halo pixel stride (floats, 32 channels + pad): 2 pixels = 96 = 32 mod 64 banks
constexpr int WG_DS = 80;  // dy pixel stride (floats, 64 channels + pad): 2 pixels = 160 = 32 mod 64 banks

template <int TPR>  // Winograd tiles per image row (W / 2): 4, 8 or 16; a chunk is 16 tiles = 16 / TPR tile rows
__global__ __launch_bounds__(512, 2) void conv_wgrad_wino_kernel(WgWinoArgs a) {
  kernarg_warmup<sizeof(WgWinoArgs)>();
  const int nwg_ = gridDim.x, bid_ = blockIdx.x;
  constexpr bool AP = false;
  const lvae_bn_apply ap = lvae_bn_apply{};
#include "conv3x3_wgrad_wino_body.inc"
}

// the same kernel with the BatchNorm-backward apply that produces its dY operand in front (see the body's header)
struct WgWinoApArgs {
  WgWinoArgs w;
  lvae_bn_apply ap;
};
template <int TPR>
__global__ __launch_bounds__(512, 2) void conv_wgrad_wino_ap_kernel(WgWinoApArgs g) {
  kernarg_warmup<sizeof(WgWinoApArgs)>();
  const WgWinoArgs& a = g.w;
  const lvae_bn_apply& ap = g.ap;
  const int nwg_ = gridDim.x, bid_ = blockIdx.x;
  constexpr bool AP = true;
#include "conv3x3_wgrad_wino_body.inc"
}

struct WgWinoGroup {
  WgWinoArgs p[kWgradWinoGroup];
};
static_assert(sizeof(WgWinoGroup) <= 4096, "kernel argument block");

// several independent problems in one launch (blockIdx.y = problem): the 8x8 level fills half the CUs per problem
template <int TPR>
__global__ __launch_bounds__(512, 2) void conv_wgrad_wino_grouped_kernel(WgWinoGroup g) {
  kernarg_warmup<(sizeof(WgWinoGroup) < 1024 ? sizeof(WgWinoGroup) : 1024)>();
  const WgWinoArgs& a = g.p[blockIdx.y];
  const int nwg_ = a.nranges * a.ncog * a.ncib;
  if ((int)blockIdx.x >= nwg_) return;  // uniform per workgroup, before any barrier
  const int bid_ = blockIdx.x;
  constexpr bool AP = false;
  const lvae_bn_apply ap = lvae_bn_apply{};
#include "conv3x3_wgrad_wino_body.inc"
}

// The two gradients of one residual block in one launch: problem A (conv1) forms its dY with the BatchNorm-backward apply in front, as
// conv_wgrad_wino_ap_kernel does, problem B (conv2) has a real dY. Workgroups [0, nwg_a) are A's, the rest B's; each problem has its own
// range split (wg_wino_pair_plan), its own XCD remap and its own "workgroup 0" / "input-channel block 0" roles, all from the problem-local
// index. Half the ranges per gradient and twice the chunks per workgroup: half the slab traffic, one prologue and one epilogue per CU.
struct WgWinoPairArgs {
  WgWinoArgs a, b;
  lvae_bn_apply ap;
  int nwg_a, pad_;
};
static_assert(sizeof(WgWinoPairArgs) <= 4096, "kernel argument block");

template <int TPR>
__global__ __launch_bounds__(512, 2) void conv_wgrad_wino_pair_kernel(WgWinoPairArgs g) {
  kernarg_warmup<(sizeof(WgWinoPairArgs) < 1024 ? sizeof(WgWinoPairArgs) : 1024)>();
  if ((int)blockIdx.x < g.nwg_a) {  // uniform per workgroup, before any barrier
    const WgWinoArgs& a = g.a;
    const lvae_bn_apply& ap = g.ap;
    const int nwg_ = g.nwg_a, bid_ = blockIdx.x;
    constexpr bool AP = true;
#include "conv3x3_wgrad_wino_body.inc"
  } else {
    const WgWinoArgs& a = g.b;
    const lvae_bn_apply ap = lvae_bn_apply{};
    const int nwg_ = (int)gridDim.x - g.nwg_a, bid_ = (int)blockIdx.x - g.nwg_a;
    constexpr bool AP = false;
#include "conv3x3_wgrad_wino_body.inc"
  }
}

// Two or three problems with a real dY and one image width (the gradients of a stochastic layer's convolutions: 32 -> 64 and 64 -> 64) in
// one launch: the single kernel's body behind a workgroup-uniform problem select. Problem i owns the workgroups [first[i], first[i + 1])
// (first[n] = the grid) and has its own range split (wg_wino_shared_split), XCD remap and "workgroup 0" roles from the problem-local index.
constexpr int kWgWinoShared = kWgradWinoShared;
struct WgWinoSharedArgs {
  WgWinoArgs p[kWgWinoShared];
  int first[kWgWinoShared + 1];
};
static_assert(sizeof(WgWinoSharedArgs) <= 4096, "kernel argument block");

template <int TPR>
__global__ __launch_bounds__(512, 2) void conv_wgrad_wino_shared_kernel(WgWinoSharedArgs g) {
  kernarg_warmup<(sizeof(WgWinoSharedArgs) < 1024 ? sizeof(WgWinoSharedArgs) : 1024)>();
  const int sel = (int)blockIdx.x < g.first[1] ? 0 : ((int)blockIdx.x < g.first[2] ? 1 : 2);   // uniform per workgroup
  const WgWinoArgs& a = g.p[sel];
  const int nwg_ = g.first[sel + 1] - g.first[sel], bid_ = (int)blockIdx.x - g.first[sel];
  constexpr bool AP = false;
  const lvae_bn_apply ap = lvae_bn_apply{};
#include "conv3x3_wgrad_wino_body.inc"
}

struct WinoReduceArgs {
  const float* slab_w;
  const float* slab_b;
  int nranges, ncog, Cout, ncib;
  int64_t stap, sk, sn;
  float* dw;
  float* db;
};
struct WinoReduceGroup {
  WinoReduceArgs p[kWgradWinoGroup];
};
struct WinoReducePair {
  WinoReduceArgs p[2];
};
struct WinoReduceShared {
  WinoReduceArgs p[kWgWinoShared];
};

// dw[tap(a,b)][ci][co] += (G^T (sum_ranges slab) G)[a][b], 1024-thread workgroups, ranges summed in eight slices (slice = range mod 8,
// ascending inside a slice, then a balanced tree over the slices: the same order in both forms, so they agree bitwise).
//   HALF (single gradient): workgroup = (ci, half of a group of 64 co), threads = 8 float4 columns x 16 positions x 8 slices, so each
//     range contributes sixteen 128-byte pieces (whole cache lines). 128 workgroups per 64x64 gradient instead of 64: the pass is bound
//     by how many bytes a CU keeps in flight, not by HBM (64 workgroups: 9.7 us for 33.5 MB, 128: 9.0 us; 256 workgroups of 64-byte
//     pieces: 31 us).
//   !HALF (grouped launch, up to 12 gradients = 768 workgroups already): workgroup = (ci, 64 co), threads = 16 float4 columns x
//     16 positions x 4, each carrying two slices; halving these workgroups as well cost 12 us per launch.
template <bool HALF>
__device__ __forceinline__ void wino_reduce_body(const WinoReduceArgs& a, int bx, float* red, float (*red_b)[64]) {
  constexpr int CW = HALF ? 32 : 64;   // output channels per workgroup; red is [8][16][CW]
  const int ncog = a.ncog, nranges = a.nranges;
  const int half = HALF ? (bx & 1) : 0, cc = HALF ? (bx >> 1) : bx, ci = cc / ncog, cog = cc % ncog;
  const int t = threadIdx.x;
  const int q = HALF ? (t & 7) : (t & 15), p = HALF ? ((t >> 3) & 15) : ((t >> 4) & 15), rs = HALF ? (t >> 7) : (t >> 8);
  const float* src = a.slab_w + ((((size_t)(ci >> 5) * ncog + cog) * 32 + (ci & 31)) * 16 + p) * 64 + half * 32 + q * 4;
  const size_t rstride = (size_t)a.ncib * ncog * 32 * 16 * 64;
  // slab rows p = 4 i + b, b < 3: the producer has applied the column half of G^T dU G (row 4 i + 3 is never written)
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if ((p & 3) != 3) {
    if (HALF) {
#pragma unroll 8
      for (int r = rs; r < nranges; r += 8) s += *reinterpret_cast<const f32x4*>(src + r * rstride);
      *reinterpret_cast<f32x4*>(red + (rs * 16 + p) * CW + q * 4) = s;
    } else {
      f32x4 s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int r = rs; r < nranges; r += 8) {
        s += *reinterpret_cast<const f32x4*>(src + r * rstride);
        if (r + 4 < nranges) s1 += *reinterpret_cast<const f32x4*>(src + (r + 4) * rstride);
      }
      *reinterpret_cast<f32x4*>(red + (rs * 16 + p) * CW + q * 4) = s;
      *reinterpret_cast<f32x4*>(red + ((rs + 4) * 16 + p) * CW + q * 4) = s1;
    }
  }
  const bool do_b = a.db != nullptr && ci == 0 && half == 0;
  if (do_b) {
    const int co = t & 63, slice = t >> 6;
    float v = 0.f;
#pragma unroll 4
    for (int r = slice; r < nranges; r += 16) v += a.slab_b[(size_t)(r * ncog + cog) * 64 + co];
    red_b[slice][co] = v;
  }
  __syncthreads();
  if (t < 3 * CW && cog * 64 + half * 32 + (t % CW) < a.Cout) {
    const int co = t % CW, ga = t / CW;  // output row a of G^T dU G
    float u[4][3];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        const float* rp = red + (i * 4 + b) * CW + co;
        u[i][b] = ((rp[0] + rp[16 * CW]) + (rp[32 * CW] + rp[48 * CW])) + ((rp[64 * CW] + rp[80 * CW]) + (rp[96 * CW] + rp[112 * CW]));
      }
    // the row half: G^T = [[1,.5,.5,0],[0,.5,-.5,0],[0,.5,.5,1]]
    float* o = a.dw + (int64_t)ci * a.sk + (int64_t)(cog * 64 + half * 32 + co) * a.sn + (int64_t)(ga * 3) * a.stap;
#pragma unroll
    for (int b = 0; b < 3; ++b)
      o[b * a.stap] += ga == 0 ? u[0][b] + 0.5f * (u[1][b] + u[2][b]) : (ga == 1 ? 0.5f * (u[1][b] - u[2][b]) : 0.5f * (u[1][b] + u[2][b]) + u[3][b]);
  }
  if (do_b && t >= 256 && t < 320 && cog * 64 + t - 256 < a.Cout) {
    const int co = t - 256;
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) v += red_b[k][co];
    a.db[cog * 64 + co] += v;
  }
}

__global__ __launch_bounds__(1024) void conv_wgrad_wino_reduce_kernel(WinoReduceArgs a) {
  kernarg_warmup<sizeof(WinoReduceArgs)>();
  __shared__ __attribute__((aligned(16))) float red[8 * 16 * 32];
  __shared__ float red_b[16][64];
  wino_reduce_body<true>(a, blockIdx.x, red, red_b);
}

// the two gradients of a pair launch (blockIdx.y = problem), each in the HALF form over its own range count
__global__ __launch_bounds__(1024) void conv_wgrad_wino_reduce_pair_kernel(WinoReducePair g) {
  kernarg_warmup<sizeof(WinoReducePair)>();
  __shared__ __attribute__((aligned(16))) float red[8 * 16 * 32];
  __shared__ float red_b[16][64];
  wino_reduce_body<true>(g.p[blockIdx.y], blockIdx.x, red, red_b);
}

// the gradients of a shared launch (blockIdx.y = problem), each in the HALF form over its own range count and input channels
__global__ __launch_bounds__(1024) void conv_wgrad_wino_reduce_shared_kernel(WinoReduceShared g) {
  kernarg_warmup<sizeof(WinoReduceShared)>();
  const WinoReduceArgs& a = g.p[blockIdx.y];
  if ((int)blockIdx.x >= 64 * a.ncib * a.ncog) return;   // uniform per workgroup, before any barrier
  __shared__ __attribute__((aligned(16))) float red[8 * 16 * 32];
  __shared__ float red_b[16][64];
  wino_reduce_body<true>(a, blockIdx.x, red, red_b);
}

__global__ __launch_bounds__(1024) void conv_wgrad_wino_reduce_grouped_kernel(WinoReduceGroup g) {
  kernarg_warmup<(sizeof(WinoReduceGroup) < 1024 ? sizeof(WinoReduceGroup) : 1024)>();
  const WinoReduceArgs& a = g.p[blockIdx.y];
  if ((int)blockIdx.x >= 32 * a.ncib * a.ncog) return;   // uniform per workgroup, before any barrier
  __shared__ __attribute__((aligned(16))) float red[8 * 16 * 64];
  __shared__ float red_b[16][64];
  wino_reduce_body<false>(a, blockIdx.x, red, red_b);
}

static int wg_wino_min_cpr() {   // slab traffic: at least this many chunks per slab
  static const int v = (int)std::max<int64_t>(1, tune("LVAE_WINO_WGRAD_MIN_CPR", 4));
  return v;
}

// budget: the ranges this gradient may spread over, counted for two input-channel blocks (budget x 2 = its workgroups: a 32-channel problem,
// one workgroup per range, spreads over twice as many): 128 when it has the chip to itself
static bool wg_wino_plan(const lvae_conv_desc* d, WgWinoArgs& a, int budget = 128) {
  static const bool off = tune("LVAE_DISABLE_WINO_WGRAD", 0) != 0 || tune("LVAE_DISABLE_WINO", 0) != 0;  // A/B switch (tuning builds only)
  if (off) return false;
  if (d->KH != 3 || d->KW != 3 || d->stride != 1 || d->pad != 1 || d->gather != LVAE_GATHER_CONV) return false;
  if ((d->C1 != 64 && d->C1 != 32) || d->C2 != 0 || d->x2 != nullptr || d->Cout % 4 != 0 || d->Cout > 256) return false;
  if (d->OH != d->H || d->OW != d->W || (d->H & 1)) return false;
  if (d->W != 8 && d->W != 16 && d->W != 32) return false;
  const int tpr = d->W / 2, tr = 16 / tpr;
  if ((d->H / 2) % tr != 0) return false;
  if (!al16_or_null(d->x) || !al16_or_null(d->in_scale) || !al16_or_null(d->in_shift)) return false;
  const int64_t M = (int64_t)d->N * d->H * d->W;
  static const int64_t min_m = tune("LVAE_WINO_WGRAD_MIN_M", 256 * 64);
  if (M < min_m || M * 256 >= ((int64_t)1 << 31)) return false;
  a.ncog = (d->Cout + 63) / 64;
  a.ncib = d->C1 / 32;
  a.pad_ = 0;
  a.cpi = (d->H / 2) / tr;
  a.total_chunks = d->N * a.cpi;
  int nranges = 2 * budget / (a.ncog * a.ncib);  // 128 of 64 channels: 256 workgroups with the two input-channel blocks
  if (nranges < 1) nranges = 1;
  const int min_cpr = wg_wino_min_cpr();
  if (nranges > a.total_chunks / min_cpr) nranges = a.total_chunks / min_cpr;  // slab traffic: at least min_cpr chunks per slab
  if (nranges < 1) nranges = 1;
  a.cpr = (a.total_chunks + nranges - 1) / nranges;
  a.nranges = (a.total_chunks + a.cpr - 1) / a.cpr;
  a.m_cpi = fastdiv_magic(a.cpi);
  return true;
}

// The family's row of the routing table: 64 input channels only. A 32-channel gradient keeps the kernel the table has always given it
// (lvae_conv2d_wgrad_f32 and the grouped call are unchanged for it); it enters this family on the explicit request of
// lvae_conv2d_wgrad_shared_f32 alone, which plans through wg_wino_plan.
// group key: the image width (one kernel instantiation per width); problems of at least LVAE_WINO_GROUP_MAX_M pixels fill the chip alone
bool conv_wgrad_wino_plan(const lvae_conv_desc* d, WgradPlan& p) {
  static const int64_t group_max_m = tune("LVAE_WINO_GROUP_MAX_M", 65536);
  WgWinoArgs a;
  if (d->C1 != 64 || !wg_wino_plan(d, a)) return false;
  p.group = (int64_t)d->N * d->H * d->W < group_max_m ? d->W : -1;
  p.set_slabs(a.nranges, (size_t)a.ncog * a.ncib * 16 * 32 * 64, (size_t)a.ncog * 64);
  p.apply_ok = d->precision == LVAE_PREC_F32 && d->C1 == 64 && d->Cout == 64 && (d->W == 16 || d->W == 32) && d->x_dtype == LVAE_DT_F32 && d->y_dtype == LVAE_DT_F32;
  return true;
}

// The pair launch shares 128 ranges (256 workgroups, one per CU) between conv1's gradient with the apply in front (A) and conv2's (B).
// A's chunks cost more (dy1 is formed from dh2 and y1 while a chunk is staged), so an even split would leave B's CUs idle: A gets
// kWgWinoPairRangesA of the 128. At 256x16x16 (1,024 chunks) that is 74 ranges of 14 chunks against 54 of 19. Measured at that shape, back
// to back in a captured graph (tools/wgrad_pair_bench.py, a tuning build sweeping the constant): 68 -> 80.6 us per pair, 70 and 72 -> 76.9,
// 74 -> 73.4, 76 -> 75.5, 78 -> 78.7, 80 -> 81.2, against 89.6 us for the two single launches (A 53.0, B 41.0 with their reduces: 58 : 42
// after the reduce, as the in-step rows 47.0 / 34.6 us suggested). profiles/wgrad_pair_ab.txt has the table.
constexpr int kWgWinoPairRangesA = 74;
static int wg_wino_pair_ranges_a() {
  static const int v = (int)std::min<int64_t>(127, std::max<int64_t>(1, tune("LVAE_WINO_PAIR_RANGES_A", kWgWinoPairRangesA)));  // (swept in tuning builds only)
  return v;
}

// The split itself. Ranges that one problem cannot use — its least chunks per range, or the rounding of its range length — go to the
// other: B is planned with what A left, then A again with what B left (at the family's minimum of 16,384 pixels both end at 64 ranges of
// 4 chunks, the single launches' own split, and the chip is full).
static bool wg_wino_pair_split(const lvae_conv_desc* da, const lvae_conv_desc* db, WgWinoArgs& a, WgWinoArgs& b) {
  if (da->C1 != 64 || db->C1 != 64) return false;   // (the caller's apply_ok says so too)
  if (!wg_wino_plan(da, a, wg_wino_pair_ranges_a()) || a.ncog != 1 || a.nranges >= 128) return false;
  if (!wg_wino_plan(db, b, 128 - a.nranges) || b.ncog != 1) return false;
  return wg_wino_plan(da, a, 128 - b.nranges);
}

// both gradients of a pair as the pair launch splits them (the caller has checked that the pair is one: conv_wgrad.hip); sched = ranges,
// chunks per range and workgroups of A, then of B
bool conv_wgrad_wino_pair_plan(const lvae_conv_desc* da, const lvae_conv_desc* db, WgradPlan& pa, WgradPlan& pb, int32_t* sched) {
  WgWinoArgs a, b;
  if (!wg_wino_pair_split(da, db, a, b)) return false;
  pa.set_slabs(a.nranges, (size_t)2 * 16 * 32 * 64, 64);
  pb.set_slabs(b.nranges, (size_t)2 * 16 * 32 * 64, 64);
  if (sched) {
    const int32_t v[6] = {a.nranges, a.cpr, a.nranges * 2, b.nranges, b.cpr, b.nranges * 2};
    std::copy(v, v + 6, sched);
  }
  return true;
}

// The shared launch's split of the 256 workgroups: every problem gets ranges of the same length c, the least c (from the least chunks per
// range up) at which all ranges fit, a range of a 64-channel problem taking two workgroups and one of a 32-channel problem one. The chunks
// per workgroup are then equal over the problems up to each problem's short last range, and a problem that cannot use a share of its own
// (few chunks) leaves it to the others by construction. At 256x16x16 with {32, 64, 64} channels: 5 x ceil(1024 / c) <= 256 from c = 21,
// 49 ranges per problem, 245 workgroups (20 chunks per workgroup would take 260). One problem alone (n = 1: how a 32-channel gradient is
// run, and tested, by itself) gets what wg_wino_plan gives a gradient that has the chip: 256 ranges of 4 chunks with 32 input channels,
// 128 of 8 with 64.
static bool wg_wino_shared_split(const lvae_conv_desc* const* d, int n, WgWinoArgs* a) {
  if (n < 1 || n > kWgWinoShared) return false;
  int max_chunks = 1;
  for (int i = 0; i < n; ++i) {
    if (!wg_wino_plan(d[i], a[i]) || a[i].ncog != 1 || d[i]->W != d[0]->W) return false;
    max_chunks = std::max(max_chunks, a[i].total_chunks);
  }
  for (int c = wg_wino_min_cpr(); c <= max_chunks; ++c) {
    int wgs = 0;
    for (int i = 0; i < n; ++i) wgs += a[i].ncib * ((a[i].total_chunks + c - 1) / c);
    if (wgs > 256) continue;
    for (int i = 0; i < n; ++i) {
      a[i].cpr = std::min(c, a[i].total_chunks);
      a[i].nranges = (a[i].total_chunks + a[i].cpr - 1) / a[i].cpr;
    }
    return true;
  }
  return false;
}

// the gradients of a shared launch as it splits them; sched = ranges, chunks per range and workgroups of each problem in turn
bool conv_wgrad_wino_shared_plan(const lvae_conv_desc* const* d, int n, WgradPlan* p, int32_t* sched) {
  WgWinoArgs a[kWgWinoShared];
  if (!wg_wino_shared_split(d, n, a)) return false;
  for (int i = 0; i < n; ++i) {
    p[i].set_slabs(a[i].nranges, (size_t)a[i].ncib * 16 * 32 * 64, 64);
    if (sched) {
      sched[3 * i] = a[i].nranges;
      sched[3 * i + 1] = a[i].cpr;
      sched[3 * i + 2] = a[i].nranges * a[i].ncib;
    }
  }
  return true;
}

// f(tiles per row) with the value as a compile-time constant
template <typename F>
static int with_tpr(int W, F f) {
  if (W == 8) return f(std::integral_constant<int, 4>{});
  if (W == 16) return f(std::integral_constant<int, 8>{});
  return f(std::integral_constant<int, 16>{});
}

// LDS of the three kernels: two chunk buffers of x halo + dy, or the exchange of the two tile halves at the end
static size_t wg_wino_lds(int W) {
  const int tpr = W / 2, hp = (2 * (16 / tpr) + 2) * (W + 2);
  return std::max((size_t)2 * (hp * WG_XS + 64 * WG_DS), (size_t)(4 * 4 * 2 * 16 * 64 + 128)) * sizeof(float);
}

// the kernel arguments and the slab reduce of one gradient (dy null: formed by a deferred apply); returns the kernel's workgroups
static int wino_fill_planned(const WgradOp& o, WgWinoArgs& a, WinoReduceArgs& r) {   // a: planned (wg_wino_plan / wg_wino_pair_split)
  a.d = *o.d;
  a.dy = o.dy;
  a.slab_w = o.slab_w();
  a.slab_b = o.slab_b();
  r = WinoReduceArgs{a.slab_w, a.slab_b, a.nranges, a.ncog, o.d->Cout, a.ncib, o.d->w_stap, o.d->w_sk, o.d->w_sn, o.dw, o.db};
  return a.nranges * a.ncog * a.ncib;
}
static int wino_fill(const WgradOp& o, WgWinoArgs& a, WinoReduceArgs& r) {
  wg_wino_plan(o.d, a);
  return wino_fill_planned(o, a, r);
}

// one gradient of a plan with apply_ok whose dY is ap's result (16-byte aligned workspace and ap operands: the entry point checked them)
int conv_wgrad_wino_apply_launch(const WgradOp& o, const lvae_bn_apply* ap, hipStream_t s) {
  WgWinoApArgs g;
  WinoReduceArgs r;
  const int wgs = wino_fill(o, g.w, r);
  g.ap = *ap;
  auto launch = [&](auto tpr) {
    return launch_lds<conv_wgrad_wino_ap_kernel<decltype(tpr)::value>>("conv_wgrad_wino_ap", dim3(wgs), dim3(512), wg_wino_lds(o.d->W),
                                                                       160 * 1024, s, g);
  };
  const int rc = o.d->W == 16 ? launch(std::integral_constant<int, 8>{}) : launch(std::integral_constant<int, 16>{});   // apply_ok: W = 16 or 32
  if (rc) return rc;
  hipLaunchKernelGGL(conv_wgrad_wino_reduce_kernel, dim3(128 * r.ncog), dim3(1024), 0, s, r);
  LVAE_LAUNCH_CHECK("conv_wgrad_wino_reduce");
  return 0;
}

// the pair of conv_wgrad_wino_pair_plan: a.plan / b.plan are that function's, ap forms A's dY (operands checked by the entry point)
int conv_wgrad_wino_pair_launch(const WgradOp& a, const lvae_bn_apply* ap, const WgradOp& b, hipStream_t s) {
  WgWinoPairArgs g;
  WinoReducePair rg;
  wg_wino_pair_split(a.d, b.d, g.a, g.b);
  g.nwg_a = wino_fill_planned(a, g.a, rg.p[0]);
  const int nwg_b = wino_fill_planned(b, g.b, rg.p[1]);
  g.ap = *ap;
  g.pad_ = 0;
  auto launch = [&](auto tpr) {
    return launch_lds<conv_wgrad_wino_pair_kernel<decltype(tpr)::value>>("conv_wgrad_wino_pair", dim3(g.nwg_a + nwg_b), dim3(512), wg_wino_lds(a.d->W),
                                                                         160 * 1024, s, g);
  };
  const int rc = a.d->W == 16 ? launch(std::integral_constant<int, 8>{}) : launch(std::integral_constant<int, 16>{});   // apply_ok: W = 16 or 32
  if (rc) return rc;
  hipLaunchKernelGGL(conv_wgrad_wino_reduce_pair_kernel, dim3(128, 2), dim3(1024), 0, s, rg);
  LVAE_LAUNCH_CHECK("conv_wgrad_wino_reduce_pair");
  return 0;
}

// the n gradients of conv_wgrad_wino_shared_plan (o[i].plan: that function's; real, 16-byte aligned dy and workspaces: the entry point
// checked them)
int conv_wgrad_wino_shared_launch(const WgradOp* o, int n, hipStream_t s) {
  WgWinoSharedArgs g;
  WinoReduceShared rg;
  const lvae_conv_desc* d[kWgWinoShared];
  for (int i = 0; i < n; ++i) d[i] = o[i].d;
  if (!wg_wino_shared_split(d, n, g.p)) return LVAE_EINVAL;
  g.first[0] = 0;
  for (int i = 0; i < kWgWinoShared; ++i) {
    if (i < n) {
      g.first[i + 1] = g.first[i] + wino_fill_planned(o[i], g.p[i], rg.p[i]);
    } else {   // no workgroup selects it
      g.p[i] = g.p[0];
      g.first[i + 1] = g.first[i];
    }
  }
  const size_t lds = wg_wino_lds(o->d->W);
  const int rc = with_tpr(o->d->W, [&](auto tpr) {
    return launch_lds<conv_wgrad_wino_shared_kernel<decltype(tpr)::value>>("conv_wgrad_wino_shared", dim3(g.first[n]), dim3(512), lds, 160 * 1024, s, g);
  });
  if (rc) return rc;
  hipLaunchKernelGGL(conv_wgrad_wino_reduce_shared_kernel, dim3(128, n), dim3(1024), 0, s, rg);
  LVAE_LAUNCH_CHECK("conv_wgrad_wino_reduce_shared");
  return 0;
}

// n <= kWgradWinoGroup gradients of one plan.group, each with its own workspace (16-byte aligned dy and workspace: the route checked
// them). One gradient runs the single kernel and the half-workgroup reduce, several the grouped kernel and the grouped reduce.
int conv_wgrad_wino_launch(const WgradOp* o, int n, hipStream_t s) {
  WgWinoGroup g;
  WinoReduceGroup rg;
  int max_wgs = 0, max_ncog = 0;
  for (int i = 0; i < n; ++i) {
    max_wgs = std::max(max_wgs, wino_fill(o[i], g.p[i], rg.p[i]));
    max_ncog = std::max(max_ncog, g.p[i].ncog);
  }
  for (int i = n; i < kWgradWinoGroup; ++i) {
    g.p[i] = g.p[0];
    rg.p[i] = rg.p[0];
  }
  const size_t lds = wg_wino_lds(o->d->W);
  const int rc = with_tpr(o->d->W, [&](auto tpr) {
    constexpr int T = decltype(tpr)::value;
    if (n == 1) return launch_lds<conv_wgrad_wino_kernel<T>>("conv_wgrad_wino", dim3(max_wgs), dim3(512), lds, 160 * 1024, s, g.p[0]);
    return launch_lds<conv_wgrad_wino_grouped_kernel<T>>("conv_wgrad_wino_grouped", dim3(max_wgs, n), dim3(512), lds, 160 * 1024, s, g);
  });
  if (rc) return rc;
  if (n == 1) hipLaunchKernelGGL(conv_wgrad_wino_reduce_kernel, dim3(64 * g.p[0].ncib * max_ncog), dim3(1024), 0, s, rg.p[0]);
  else hipLaunchKernelGGL(conv_wgrad_wino_reduce_grouped_kernel, dim3(64 * max_ncog, n), dim3(1024), 0, s, rg);
  LVAE_LAUNCH_CHECK(n == 1 ? "conv_wgrad_wino_reduce" : "conv_wgrad_wino_reduce_grouped");
  return 0;
}

}  // namespace lvae
