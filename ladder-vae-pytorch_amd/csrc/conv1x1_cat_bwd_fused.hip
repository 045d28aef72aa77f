// Backward of the merge / skip-merge 1x1 convolution (MergeLayer, SkipConnectionMerger: 128 -> 64 over the never-materialised channel concat
// (x1 | x2), models/lvae_layers.py:347-359) as ONE persistent kernel: input gradient of both halves AND the weight / bias gradient.
//
//   dy[m, co]       = given, or BN'(ap.dh; ap.x)[m, co] + ap.add[m, co]   (the deferred last apply of the residual block that reads the merge output)
//   dx1[m, ci]      = sum_co dy[m, co] * W[co, ci]          dx2[m, ci] = sum_co dy[m, co] * W[co, 64 + ci]
//   dW[co, ci]     += sum_m  (x1 | x2)[m, ci] * dy[m, co]   db[co]    += sum_m dy[m, co]
//
// The transposed twin of conv1x1_gate_bwd_fused_bf16_kernel<3> (conv1x1_gate_bwd_fused.hip) without the gate arithmetic: a workgroup loops
// over 64-pixel tiles (one workgroup per CU at most), splits dy and the two x tiles exactly into three bf16 planes in LDS once, and uses the
// dy planes as the A operand of the dgrad GEMM (waves 0-3, [64 px][128 ci], W pre-split in LDS once per workgroup) and as the B operand of
// the weight-gradient GEMM (waves 4-7, [128 ci][64 co] in registers across all tiles of the workgroup; both operands through the
// transposing LDS read of bf16_frag.h). Six-product form only (PieceOrder<3>: fp32-equivalent). Before, this was five launches: the block's
// BatchNorm-1 apply and its finalize, the tile weight gradient and its slab reduce, the concat dgrad: dy written once and read twice
// (167 MB at 256x16x16). Here dy is never stored unless ap.out asks for it: 84 MB read, 33.5 MB written. Per-workgroup partials go to the
// usual slabs ([workgroup][128 ci][64 co] + [workgroup][64]) and are summed in a fixed order (wgrad_reduce_launch): deterministic. No
// workgroup waits for another: the loop is tile = blockIdx.x, += gridDim.x and nothing else.
#include "bf16_frag.h"
#include "bn_apply.h"
#include "lvae_host.h"

namespace lvae {

struct CbfArgs {
  const float* dy;   // [M][64] (not read with a deferred apply)
  const float* x1;   // [M][64]
  const float* x2;   // [M][64]
  const float* w;    // element (k = co, n = ci) at w[k + n * w_sn]
  int64_t w_sn;
  float* dx1;        // [M][64]
  float* dx2;        // [M][64]
  float* slab_w;     // [nwg][128 ci][64 co]
  float* slab_b;     // [nwg][64] or null
  int M, ntiles;
  lvae_bn_apply ap;  // deferred BatchNorm-backward apply that produces dy (ap.parts == nullptr: dy is given); ap.out may be null
};

constexpr int CB_LDD = 72;    // dy row pitch in bf16 (64 channels + 8: 144 bytes, 16-byte multiples for ds_read_b128)
constexpr int CB_LDX = 136;   // (x1 | x2) row pitch in bf16
constexpr int CB_LDO = 128;   // dx staging row pitch in floats: no padding (the 160 KB are full), 32-column blocks swapped in every other group of 4 rows
// three planes of each tile, the dx staging tile, the deferred apply's coefficient rows [6][64], the dgrad's pre-split W fragments
// [4 k-steps][4 column blocks][3][64 lanes][8]
constexpr size_t cbf_lds() {
  return (size_t)3 * (64 * CB_LDD + 64 * CB_LDX) * 2 + (size_t)64 * CB_LDO * 4 + AP_CF * 4 + (size_t)4 * 4 * 3 * 64 * 16;
}
static_assert(cbf_lds() <= 160 * 1024, "one workgroup's LDS");

__device__ __forceinline__ int cb_swz(int row) { return ((row >> 2) & 1) << 5; }   // rows r and r + 4 of one accumulator store go to different bank halves

template <bool AP>
__global__ __launch_bounds__(512) void conv1x1_cat_bwd_fused_kernel(CbfArgs a) {
  kernarg_warmup<sizeof(CbfArgs)>();
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  constexpr int D_PLANE = 64 * CB_LDD, X_PLANE = 64 * CB_LDX;
  __bf16* Ds = reinterpret_cast<__bf16*>(smem_raw);                  // [3][64 px][72]: dy tile
  __bf16* Xs = Ds + 3 * D_PLANE;                                     // [3][64 px][136]: (x1 | x2) tile
  float* Os = reinterpret_cast<float*>(Xs + 3 * X_PLANE);            // [64 px][128]: dx staging (fp32)
  float* Cf = Os + 64 * CB_LDO;                                      // the deferred apply's coefficient rows (bn_apply.h)
  bf16x8* Wf = reinterpret_cast<bf16x8*>(Cf + AP_CF);               // [4][4][3][64]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const bool wg_role = wave >= 4;  // waves 4-7: weight gradient; waves 0-3: dgrad
  const int wm = (wave & 3) >> 1, wn = wave & 1, li = lane & 31, lh = lane >> 5, G = lane >> 4, i16 = lane & 15;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  if (AP) ap_reduce(a.ap, Os, Cf, blockIdx.x == 0);   // the producer's partial rows -> Cf, through the (still unused) staging tile

  // dgrad waves: W[co = 16 s + 8 lh + 0..7][ci = 32 cb + li] as the B fragment of k-step s and column block cb, three pieces, in LDS in
  // fragment order (wave cb writes its block once; published by the first barrier of the tile loop)
  if (!wg_role) {
    const int cb = wave;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float* wp = a.w + (int64_t)(cb * 32 + li) * a.w_sn + 16 * s + 8 * lh;
      bf16x8 v[3];
      split_frag<3>(*reinterpret_cast<const f32x4*>(wp), *reinterpret_cast<const f32x4*>(wp + 4), v);
#pragma unroll
      for (int q = 0; q < 3; ++q) Wf[((s * 4 + cb) * 3 + q) * 64 + lane] = v[q];
    }
  }

  // raw operands of one tile: thread -> 2 rows (r0, r0 + 32), channels c4 .. c4 + 3 of dy (or dh, x, add) and of x1, x2
  f32x4 pg[2], p1[2], p2[2];
  f32x4 px[AP ? 2 : 1], pd[AP ? 2 : 1];
  const int c4 = (t & 15) * 4, r0 = t >> 4;
  const bool ap_add = AP && a.ap.add != nullptr, ap_out = AP && a.ap.out != nullptr;
  // one of the thread's two rows of a tile: requested as soon as the row before it in the same registers has been consumed, so that the
  // loads of tile t + 1 fly under the rest of tile t (the loop's barriers wait for LDS only)
  auto prefetch_row = [&](int tile, int u) {
    const int m = tile * 64 + r0 + 32 * u;
    const size_t mc = m < a.M ? (size_t)m : 0;  // clamped address; the values of rows past the end are zeroed below
    if (AP) {
      pg[u] = *reinterpret_cast<const f32x4*>(a.ap.dh + mc * 64 + c4);
      px[u] = *reinterpret_cast<const f32x4*>(a.ap.x + mc * 64 + c4);
      pd[u] = ap_add ? *reinterpret_cast<const f32x4*>(a.ap.add + mc * 64 + c4) : zero4;
    } else {
      pg[u] = *reinterpret_cast<const f32x4*>(a.dy + mc * 64 + c4);
    }
    p1[u] = *reinterpret_cast<const f32x4*>(a.x1 + mc * 64 + c4);
    p2[u] = *reinterpret_cast<const f32x4*>(a.x2 + mc * 64 + c4);
  };

  // weight-gradient accumulators of this wave: co block wn, ci blocks 2 wm + {0, 1} (wm = 0: the channels of x1, 1: of x2)
  f32x16 accw[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) accw[j][r] = 0.f;
  f32x4 bs = zero4;  // bias-gradient partials of this thread's channels (fp32 dy, not the split operand)
  // transposed-read addresses of this lane (bf16_frag.h): pixel row 8 (G >> 1) + (i16 >> 2) of a k-step, channel 16 (G & 1) + 4 (i16 & 3) of a block
  const int trow = 8 * (G >> 1) + (i16 >> 2), tch = 16 * (G & 1) + 4 * (i16 & 3);
  using PO = PieceOrder<3>;

  int tile = blockIdx.x;
  if (tile < a.ntiles) {
    prefetch_row(tile, 0);
    prefetch_row(tile, 1);
  }
  for (; tile < a.ntiles; tile += gridDim.x) {
    const int m0 = tile * 64;
    const bool more = tile + (int)gridDim.x < a.ntiles;
    // ---- dy (given or formed) and the x rows from the prefetched registers; everything the next tile reads is requested before the
    // first write-through store of this one
    f32x4 g[2], v1[2], v2[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      g[u] = v1[u] = v2[u] = zero4;
      if (m0 + r0 + 32 * u < a.M) {
        g[u] = AP ? ap_value4(Cf, pg[u], px[u], c4, a.ap.act) + pd[u] : pg[u];
        v1[u] = p1[u];
        v2[u] = p2[u];
      }
      if (more) prefetch_row(tile + gridDim.x, u);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = r0 + 32 * u;
      if (ap_out && m0 + r < a.M) store_wt4(a.ap.out + (size_t)(m0 + r) * 64 + c4, g[u]);
      bs += g[u];
      bf16x4 qg[3], q1[3], q2[3];
      split4<3>(g[u], qg);
      split4<3>(v1[u], q1);
      split4<3>(v2[u], q2);
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        *reinterpret_cast<bf16x4*>(Ds + q * D_PLANE + r * CB_LDD + c4) = qg[q];
        *reinterpret_cast<bf16x4*>(Xs + q * X_PLANE + r * CB_LDX + c4) = q1[q];
        *reinterpret_cast<bf16x4*>(Xs + q * X_PLANE + r * CB_LDX + 64 + c4) = q2[q];
      }
    }
    lds_barrier();  // the dy / x tiles are published; the prefetched rows stay in flight

    if (!wg_role) {
      // ---- dgrad: dx[32 px (wm)][2 x 32 ci (half wn: 0 = dx1, 1 = dx2)] = dy[px][0:64] . W, 4 k-steps of 16
      f32x16 accx[2];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) accx[j][r] = 0.f;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        bf16x8 af[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) af[q] = *reinterpret_cast<const bf16x8*>(Ds + q * D_PLANE + (wm * 32 + li) * CB_LDD + 16 * s + 8 * lh);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          bf16x8 bw[3];
#pragma unroll
          for (int q = 0; q < 3; ++q) bw[q] = Wf[((s * 4 + wn * 2 + j) * 3 + q) * 64 + lane];
#pragma unroll
          for (int k = 0; k < PO::N; ++k) accx[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[PO::A[k]], bw[PO::B[k]], accx[j], 0, 0, 0);
        }
      }
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          Os[row * CB_LDO + (((wn * 2 + j) * 32 + li) ^ cb_swz(row))] = accx[j][r];
        }
    } else {
      // ---- weight gradient: dW[2 x 32 ci (wm)][32 co (wn)] += (x1 | x2)^T . dy, k = pixel: 4 k-steps of 16 pixels
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        bf16x8 bf[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const __bf16* dp = Ds + q * D_PLANE + (16 * s + trow) * CB_LDD + wn * 32 + tch;
          bf[q] = tr_frag(dp, dp + 4 * CB_LDD);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          bf16x8 af[3];
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            const __bf16* xp = Xs + q * X_PLANE + (16 * s + trow) * CB_LDX + (wm * 2 + j) * 32 + tch;
            af[q] = tr_frag(xp, xp + 4 * CB_LDX);
          }
#pragma unroll
          for (int k = 0; k < PO::N; ++k) accw[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[PO::A[k]], bf[PO::B[k]], accw[j], 0, 0, 0);
        }
      }
    }
    lds_barrier();  // dy / x tiles are dead (the next iteration overwrites them), the dx staging tile is complete
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = r0 + 32 * u, m = m0 + r;
      if (m < a.M) {
        const f32x4 lo = *reinterpret_cast<const f32x4*>(Os + r * CB_LDO + (c4 ^ cb_swz(r)));
        const f32x4 hi = *reinterpret_cast<const f32x4*>(Os + r * CB_LDO + ((64 + c4) ^ cb_swz(r)));
        store_wt4(a.dx1 + (size_t)m * 64 + c4, lo);
        store_wt4(a.dx2 + (size_t)m * 64 + c4, hi);
      }
    }
    // no barrier here: the next write to the staging tile comes after the next iteration's first barrier
  }

  // ---- this workgroup's weight / bias gradient partials -> slabs (128-byte row segments straight from the accumulators)
  float* sw = a.slab_w + (size_t)blockIdx.x * 128 * 64;
  if (wg_role) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        sw[(size_t)((wm * 2 + j) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * 64 + wn * 32 + li] = accw[j][r];
  }
  if (a.slab_b) {
    __syncthreads();  // the last tile's dx staging reads are done
    float* red = Os;  // [32 row groups][64] floats = 8 KB of the 32 KB staging tile
    *reinterpret_cast<f32x4*>(red + r0 * 64 + c4) = bs;
    __syncthreads();
    if (t < 64) {
      float v = 0.f;
#pragma unroll
      for (int gq = 0; gq < 32; ++gq) v += red[gq * 64 + t];
      a.slab_b[(size_t)blockIdx.x * 64 + t] = v;
    }
  }
}

// workgroups (= weight-gradient slabs) for M pixels: one per CU, fewer when there are fewer tiles or the caller caps them. Never more
// than tiles: every workgroup writes a slab it has accumulated into.
static int cbf_nwg(int64_t M, int max_workgroups) {
  const int64_t ntiles = (M + 63) / 64;
  const int64_t cap = max_workgroups > 0 && max_workgroups < 256 ? max_workgroups : 256;
  return (int)(ntiles < cap ? ntiles : cap);
}

// `d` describes the dgrad over the concat exactly as for lvae_conv1x1_dgrad_cat_f32 (d->x = dy or null, C1 = 64 = the convolution's output
// channels, Cout = 128 = C1 + C2 of the forward, weight strides of the transposed view; d->y is not used). False when this kernel does not
// take it; p.workspace: bytes of its slabs at the default grid. The operands the descriptor does not carry are assumed 16-byte aligned.
static bool conv1x1_cat_bwd_plan(const lvae_conv_desc* d, int split, bool with_apply, ConvPlan& p) {
  static const bool off = tune("LVAE_DISABLE_CAT_BWD_FUSED", 0) != 0;  // A/B switch (tuning builds only)
  (void)with_apply;  // the deferred apply exists in every form of this kernel
  if (off || d == nullptr) return false;
  if (d->KH != 1 || d->KW != 1 || d->stride != 1 || d->pad != 0 || d->OH != d->H || d->OW != d->W) return false;
  if (d->C1 != 64 || d->C2 != 0 || d->x2 != nullptr || d->Cout != 128 || split != 64) return false;
  if (d->w == nullptr || d->w_sk != 1 || d->w_sn < 64 || d->w_sn % 4 != 0 || !al16_or_null(d->w) || !al16_or_null(d->x)) return false;
  if (d->bias != nullptr || d->in_scale != nullptr || d->in_shift != nullptr || d->out_scale != nullptr || d->stats_out != nullptr) return false;
  if (d->in_act != 0 || d->out_act != 0 || d->in_fold != nullptr) return false;
  if (d->precision != LVAE_PREC_F32 || d->form == LVAE_FORM_F32_MFMA) return false;  // six-product form only
  if (d->x_dtype != LVAE_DT_F32 || d->y_dtype != LVAE_DT_F32) return false;          // fp32-stored operands only
  if (d->N <= 0 || d->H <= 0 || d->W <= 0) return false;
  const int64_t M = (int64_t)d->N * d->H * d->W;
  if (M >= ((int64_t)1 << 31) - 64) return false;
  p = ConvPlan{};
  p.workspace = (size_t)cbf_nwg(M, 0) * (128 * 64 + 64) * sizeof(float);
  return true;
}

}  // namespace lvae

using namespace lvae;

extern "C" size_t lvae_conv1x1_cat_bwd_workspace(const lvae_conv_desc* d, int32_t split) {
  ConvPlan p;
  return conv1x1_cat_bwd_plan(d, split, false, p) ? p.workspace : 0;
}

extern "C" int32_t lvae_conv1x1_cat_bwd_apply_ok(const lvae_conv_desc* d, int32_t split) {
  ConvPlan p;
  return conv1x1_cat_bwd_plan(d, split, true, p) ? 1 : 0;
}

#define CBF_REQUIRE_AL16(p) LVAE_REQUIRE(al16_or_null(p), LVAE_EALIGN, "lvae_conv1x1_cat_bwd_f32: " #p " must be 16-byte aligned")

extern "C" int lvae_conv1x1_cat_bwd_f32(const lvae_conv_desc* d, const float* x1, const float* x2, float* dx1, float* dx2, float* dweight,
                                        float* dbias, const lvae_bn_apply* ap, void* workspace, size_t workspace_bytes,
                                        int32_t max_workgroups, void* stream) {
  const char* who = "lvae_conv1x1_cat_bwd_f32";
  const bool with_ap = ap != nullptr && ap->parts != nullptr;
  LVAE_REQUIRE(d && (d->x || with_ap) && x1 && x2 && dx1 && dx2 && dweight && workspace, LVAE_EINVAL, "%s: null pointer", who);
  LVAE_REQUIRE(max_workgroups >= 0, LVAE_EINVAL, "%s: negative max_workgroups", who);
  ConvPlan p;
  LVAE_REQUIRE(conv1x1_cat_bwd_plan(d, 64, with_ap, p), LVAE_EINVAL,
               "%s: not taken (needs the dgrad view of a 1x1 / stride-1 convolution over a 64 + 64 channel concat with 64 output channels: "
               "C1 = 64, Cout = 128, w_sk = 1, 16-byte aligned dy and w, fp32 tensors, precision LVAE_PREC_F32 and not LVAE_FORM_F32_MFMA); "
               "use lvae_conv2d_wgrad_f32 + lvae_conv1x1_dgrad_cat_f32", who);
  if (with_ap) {
    const int rc = bn_apply_check(who, ap, (int64_t)d->N * d->H * d->W, BN_AP_ADD | BN_AP_OUT_OPTIONAL);
    if (rc) return rc;
  }
  LVAE_REQUIRE(workspace_bytes >= p.workspace, LVAE_EWORKSPACE, "%s: workspace %zu < %zu", who, workspace_bytes, p.workspace);
  CBF_REQUIRE_AL16(x1);
  CBF_REQUIRE_AL16(x2);
  CBF_REQUIRE_AL16(dx1);
  CBF_REQUIRE_AL16(dx2);
  CBF_REQUIRE_AL16(workspace);
  CbfArgs a;
  a.ap = lvae_bn_apply{};
  if (with_ap) a.ap = *ap;
  a.dy = d->x;
  a.x1 = x1;
  a.x2 = x2;
  a.w = d->w;
  a.w_sn = d->w_sn;
  a.dx1 = dx1;
  a.dx2 = dx2;
  a.M = d->N * d->H * d->W;
  a.ntiles = (a.M + 63) / 64;
  const int nwg = cbf_nwg(a.M, max_workgroups);
  a.slab_w = static_cast<float*>(workspace);
  a.slab_b = dbias ? a.slab_w + (size_t)nwg * 128 * 64 : nullptr;
  constexpr size_t lds = cbf_lds();
  const dim3 grid(nwg), block(512);
  hipStream_t s = (hipStream_t)stream;
  const int rc = with_ap ? launch_lds<conv1x1_cat_bwd_fused_kernel<true>>(who, grid, block, lds, (int)lds, s, a)
                         : launch_lds<conv1x1_cat_bwd_fused_kernel<false>>(who, grid, block, lds, (int)lds, s, a);
  if (rc) return rc;
  // slabs are [nwg][ci][co]: the weight element (ci, co) lives at dweight[ci * w_sn + co * w_sk] (the weight's own strides)
  wgrad_reduce_launch(a.slab_w, a.slab_b, nwg, 1, 128, 64, 0, d->w_sn, d->w_sk, dweight, dbias, s);
  LVAE_LAUNCH_CHECK("lvae_conv1x1_cat_bwd_f32 reduce");
  return 0;
}
