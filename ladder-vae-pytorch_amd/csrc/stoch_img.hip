// Fused stochastic block of the low-resolution levels (H*W <= 64): one launch per level and direction on whole-image tiles, as the residual
// blocks of these levels run (resblock_img.hip). NormalStochasticBlock2d (lib/stochastic.py:45-99) between two residual chains is
//
//   p_params = conv_in_p(x_p)            3x3, 64 -> 2Z   (the top layer has none: p_params is the given, broadcast parameter)
//   q_params = conv_in_q(x_q)            3x3, 64 -> 2Z
//   z, log p(z), log q(z), KL            the elementwise core, absolute form (abs_terms of stoch_core.h), per-image and per-pixel sums
//   out      = conv_out(z)               3x3, Z -> 64
//
// and has no BatchNorm: nothing in it needs a value of another workgroup once a workgroup's tile is whole images (the halo of each 3x3
// convolution is inside the tile; logprob_p / logprob_q / kl_samplewise are sums over one image, kl_spatial over the Z channels of one
// pixel). One-kernel-per-op this was four launches behind the noise fill (two convolutions of ~9-13 us, the core at ~12 us, conv_out at
// 6-12 us), each a tile's latency on a mostly idle chip; here the chain is one pass per tile with p_params / q_params / z staying in LDS
// between the stages, and its backward (stoch_img_bwd_kernel, below) the same chain in reverse from d_out. Everything that reached memory
// still does (p_params, q_params, z, out and the four reductions; dp, dq and the two input gradients): the weight gradients, the latent
// statistics and the returned dict read them as before.
//
// Arithmetic: resblock_img.hip's — the tile's patch (zero ring included) as three exact bf16 piece planes in LDS, weights pre-split once
// per step in MFMA fragment order and streamed from L2, six piece products per fp32 product on v_mfma_f32_32x32x16_bf16 (PieceOrder<3>),
// whatever the descriptor's precision says: the block has no bf16-operand form. The elementwise core calls the element functions of
// stoch_core.h that the stand-alone kernels of stochastic.hip call (abs_terms, abs_grads, stoch_weights); the thread map is this tile's.
#include <string.h>

#include <type_traits>

#include "bf16_frag.h"
#include "lvae_host.h"
#include "stoch_core.h"

namespace lvae {

struct StochImgArgs {
  const float *xp, *xq;                   // inputs of conv_in_p / conv_in_q [N][HW][64] (xp unused without conv_in_p)
  const float *bias_p, *bias_q, *bias_o;  // [64] or null
  const __bf16 *Wp, *Wq, *Wo;             // pre-split weights [tap][k-step 4][plane 3][n half 2][lane 64][8] (bf_weight_kernel; conv_out: k-steps 2, 3 zero)
  const float* p_in;                      // without conv_in_p: the given p_params [N | 1][HW][64]
  const float* eps;                       // [N][HW][32]: noise (mode 0) or the forced latent (mode 2); unused in mode 1
  float *p_out, *q_out, *z, *out;         // p_out null without conv_in_p
  float *lp, *lq, *kl, *ks;               // [N], [N], [N], [N][HW] (ks may be null)
  // backward: Wp / Wq / Wo are the planes of the dgrad direction, p_in / p_bcast the p_params that were used, eps as in the forward
  const float *d_out, *q_in, *z_in;       // [N][HW][64], q_params [N][HW][64], z [N][HW][32]
  const float *dz_ext, *g_lp, *g_lq, *g_kl, *g_ks;   // upstream gradients beside d_out: [N][HW][32], [N], [N], [N], [N][HW]; each may be null
  float *dp, *dq, *dxp, *dxq;             // [N][HW][64] each (dxp unused without conv_in_p)
  int N, W, NI, HW, halo_w, halo_h, halo_px, nwg, p_bcast, mode, analytical;
  uint32_t m_hw, m_w, m_per_img, m_halo_w;
};

constexpr int SI_LDK = 72;          // bf16 elements per patch row (64 channels + 8 pad = 144 bytes)
constexpr int SI_LDO = 68;          // floats per staged output row (64 + 4)
constexpr int SI_SCR_BYTES = 1024;  // per-row sums [3][64] in front of the tile regions
constexpr int SI_Z = 32;            // latent channels (2Z = 64 = the convolutions' width)
enum { SI_K64_N64, SI_K32_N64, SI_K64_N32 };   // reduction x output channels of a convolution inside the kernels (stoch_img_body.inc)

// 64 (MI = 2) or 32 (MI = 1) pixels x 64 channels per workgroup, 4 waves. The 64 -> 64 convolutions run as rb_conv_kernel's reduction loop:
// wave w owns the w-th 16-channel block of every tap for the whole tile (no B fragment fetched twice, a three-deep register ring over the
// L2 latency), the four partial tiles are summed through LDS. conv_out reduces over 32 channels only: wave w takes k block (w & 1) and
// output half (w >> 1), two partial tiles.
template <int MI, bool HAS_P>
__global__ __launch_bounds__(256) void stoch_img_fwd_kernel(StochImgArgs a) {
#include "stoch_img_body.inc"
  const size_t main_bytes = max((size_t)SPLIT * a_plane * 2, (size_t)4 * OSW * 4);
  float* Ps = reinterpret_cast<float*>(mainr + main_bytes);   // p_params tile [BM][LDO], then q_params tile
  float* Qs = Ps + OSW;

  // ---- everything the stages read from memory is requested now (plain loads the compiler tracks), behind the weight touches
  pf_issue();
  f32x4 xq[NQ], xp[NQ], ev[MI];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    if (HAS_P) xp[q] = *reinterpret_cast<const f32x4*>(a.xp + grow[q] * 64 + c4);
    else xp[q] = *reinterpret_cast<const f32x4*>(a.p_in + (a.p_bcast ? (size_t)pr[q] : grow[q]) * 64 + c4);
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) xq[q] = *reinterpret_cast<const f32x4*>(a.xq + grow[q] * 64 + c4);
#pragma unroll
  for (int u = 0; u < MI; ++u) ev[u] = a.mode != 1 ? *reinterpret_cast<const f32x4*>(a.eps + erow[u] * Z + ec) : zero4;
  const f32x4 bias_p = HAS_P && a.bias_p ? *reinterpret_cast<const f32x4*>(a.bias_p + c4) : zero4;
  const f32x4 bias_q = a.bias_q ? *reinterpret_cast<const f32x4*>(a.bias_q + c4) : zero4;
  const f32x4 bias_o = a.bias_o ? *reinterpret_cast<const f32x4*>(a.bias_o + c4) : zero4;

  // =====================================================================================================================
  // p_params = conv_in_p(x_p) + bias  (or the given parameter) -> memory and the Ps tile
  // =====================================================================================================================
  if (HAS_P) {
    zero_ring();
#pragma unroll
    for (int q = 0; q < NQ; ++q) put4(hp[q], ok[q] ? xp[q] : zero4);
    pf_drain();
    conv(a.Wp, 0, K64N64{});
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int p = p0 + 16 * q;
      const f32x4 v = os_sum4(p) + bias_p;
      if (ok[q]) store_wt4(a.p_out + grow[q] * 64 + c4, v);
      *reinterpret_cast<f32x4*>(Ps + p * LDO + c4) = v;
    }
    lds_barrier();   // the partial tiles are read: the region becomes the patch of x_q
  } else {
#pragma unroll
    for (int q = 0; q < NQ; ++q) *reinterpret_cast<f32x4*>(Ps + (p0 + 16 * q) * LDO + c4) = xp[q];
    pf_drain();
  }

  // =====================================================================================================================
  // q_params = conv_in_q(x_q) + bias -> memory and the Qs tile
  // =====================================================================================================================
  zero_ring();
#pragma unroll
  for (int q = 0; q < NQ; ++q) put4(hp[q], ok[q] ? xq[q] : zero4);
  conv(a.Wq, 0, K64N64{});
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int p = p0 + 16 * q;
    const f32x4 v = os_sum4(p) + bias_q;
    if (ok[q]) store_wt4(a.q_out + grow[q] * 64 + c4, v);
    *reinterpret_cast<f32x4*>(Qs + p * LDO + c4) = v;
  }
  lds_barrier();   // Ps / Qs complete; the partial tiles are read: the region becomes the patch of z

  // =====================================================================================================================
  // elementwise core (abs_terms per element): z -> memory and the patch; kl_spatial; per-row sums -> scr
  // =====================================================================================================================
  zero_ring();
#pragma unroll
  for (int u = 0; u < MI; ++u) {
    const int p = er0 + 32 * u;
    const f32x4 pmu = *reinterpret_cast<const f32x4*>(Ps + p * LDO + ec), plv = *reinterpret_cast<const f32x4*>(Ps + p * LDO + Z + ec);
    const f32x4 qmu = *reinterpret_cast<const f32x4*>(Qs + p * LDO + ec), qlv = *reinterpret_cast<const f32x4*>(Qs + p * LDO + Z + ec);
    f32x4 zv;
    float kan = 0.f, s_lp = 0.f, s_lq = 0.f, s_kl = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const StochTerms r = abs_terms(pmu[j], plv[j], qmu[j], qlv[j], ev[u][j], a.mode, a.analytical);
      zv[j] = r.z;
      s_lp += r.lp;
      s_lq += r.lq;
      kan += r.kan;
      s_kl += r.kl;
    }
    if (!eok[u]) zv = zero4;
    if (eok[u]) store_wt4(a.z + erow[u] * Z + ec, zv);
    put4(hz[u], zv);
    // the Z / 4 = 8 lanes of a pixel are consecutive: per-pixel sums in a fixed order (all lanes take part in the shuffles)
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) {
      kan += __shfl_xor(kan, o, 64);
      s_lp += __shfl_xor(s_lp, o, 64);
      s_lq += __shfl_xor(s_lq, o, 64);
      s_kl += __shfl_xor(s_kl, o, 64);
    }
    if ((t & 7) == 0) {
      if (eok[u] && a.ks) a.ks[erow[u]] = kan;
      scr[p] = s_lp;
      scr[64 + p] = s_lq;
      scr[128 + p] = s_kl;
    }
  }

  // =====================================================================================================================
  // out = conv_out(z) + bias; the per-image sums (HW rows each, ascending) by the first 3 NI threads behind the patch barrier
  // =====================================================================================================================
  {
    // (inside conv: barrier -> loop -> barrier -> partial tiles; scr is read after its first barrier has published it)
    conv(a.Wo, 0, K32N64{});
    if (t < 3 * a.NI) {
      const int which = t / a.NI, img = t - which * a.NI;
      if (n0 + img < a.N) {
        float v = 0.f;
        for (int r = 0; r < HW; ++r) v += scr[which * 64 + img * HW + r];
        float* dst = which == 0 ? a.lp : which == 1 ? a.lq : a.kl;
        dst[n0 + img] = v;
      }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int p = p0 + 16 * q;
      const f32x4 v = os_sum2(p) + bias_o;
      if (ok[q]) store_wt4(a.out + grow[q] * 64 + c4, v);
    }
  }
}

// Backward of the same block from d_out, per tile: dz = dgrad(conv_out)(d_out) stays in LDS; the per-element backward of the absolute form
// (abs_grads, stoch_core.h) with the g_lp / g_lq / g_kl / g_ks rows give dp and dq, which are stored (the queued whole-image weight gradients read them
// as dy) and staged as patches for the two input-gradient convolutions. Without conv_in_p only dp is written (the caller sums a broadcast
// parameter's gradient over the batch).
template <int MI, bool HAS_P>
__global__ __launch_bounds__(256) void stoch_img_bwd_kernel(StochImgArgs a) {
#include "stoch_img_body.inc"
  (void)scr;
  (void)pr;
  // ---- everything the stages read from memory is requested now (plain loads the compiler tracks), behind the weight touches
  pf_issue();
  f32x4 go[NQ], pmu[MI], plv[MI], qmu[MI], qlv[MI], zv[MI], ev[MI], dzx[MI];
  float glp[MI], glq[MI], gkl[MI], gks[MI];
#pragma unroll
  for (int q = 0; q < NQ; ++q) go[q] = *reinterpret_cast<const f32x4*>(a.d_out + grow[q] * 64 + c4);
#pragma unroll
  for (int u = 0; u < MI; ++u) {
    const size_t prow = a.p_bcast ? (size_t)epr[u] : erow[u];
    pmu[u] = *reinterpret_cast<const f32x4*>(a.p_in + prow * 64 + ec);
    plv[u] = *reinterpret_cast<const f32x4*>(a.p_in + prow * 64 + Z + ec);
    qmu[u] = *reinterpret_cast<const f32x4*>(a.q_in + erow[u] * 64 + ec);
    qlv[u] = *reinterpret_cast<const f32x4*>(a.q_in + erow[u] * 64 + Z + ec);
    zv[u] = *reinterpret_cast<const f32x4*>(a.z_in + erow[u] * Z + ec);
    ev[u] = a.mode == 0 ? *reinterpret_cast<const f32x4*>(a.eps + erow[u] * Z + ec) : zero4;
    dzx[u] = a.dz_ext ? *reinterpret_cast<const f32x4*>(a.dz_ext + erow[u] * Z + ec) : zero4;
    glp[u] = a.g_lp ? a.g_lp[eimg[u]] : 0.f;
    glq[u] = a.g_lq ? a.g_lq[eimg[u]] : 0.f;
    gkl[u] = a.g_kl ? a.g_kl[eimg[u]] : 0.f;
    gks[u] = a.g_ks ? a.g_ks[erow[u]] : 0.f;
  }

  // ---- dz = dgrad of conv_out (64 -> 32 channels, taps mirrored) + the upstream gradient of z itself
  zero_ring();
#pragma unroll
  for (int q = 0; q < NQ; ++q) put4(hp[q], ok[q] ? go[q] : zero4);
  pf_drain();
  conv(a.Wo, 1, K64N32{});
  f32x4 dzv[MI];
#pragma unroll
  for (int u = 0; u < MI; ++u) dzv[u] = os_sum4_at(er0 + 32 * u, ec) + dzx[u];
  lds_barrier();   // the partial tiles are read: the region becomes the patch of dp (or dq)

  // ---- elementwise backward (abs_grads per element): dp, dq -> memory; dp (dq without conv_in_p) -> the patch
  zero_ring();
  f32x4 dqm[MI], dql[MI];
#pragma unroll
  for (int u = 0; u < MI; ++u) {
    float G_lp, G_lq, G_an;
    stoch_weights(glp[u], glq[u], gkl[u], gks[u], a.analytical, G_lp, G_lq, G_an);
    f32x4 dpm, dpl;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const StochGrads g = abs_grads(pmu[u][j], plv[u][j], qmu[u][j], qlv[u][j], ev[u][j], zv[u][j], dzv[u][j], G_lp, G_lq, G_an, a.mode);
      dpm[j] = g.pmu;
      dpl[j] = g.plv;
      dqm[u][j] = g.smu;
      dql[u][j] = g.slv;
    }
    if (!eok[u]) dpm = dpl = dqm[u] = dql[u] = zero4;
    if (eok[u]) {
      store_wt4(a.dp + erow[u] * 64 + ec, dpm);
      store_wt4(a.dp + erow[u] * 64 + Z + ec, dpl);
      store_wt4(a.dq + erow[u] * 64 + ec, dqm[u]);
      store_wt4(a.dq + erow[u] * 64 + Z + ec, dql[u]);
    }
    if (HAS_P) {
      put4(hz[u], dpm);
      put4(hz[u] + Z, dpl);
    }
  }

  // ---- d x_p = dgrad of conv_in_p (dp)
  if (HAS_P) {
    conv(a.Wp, 1, K64N64{});
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      if (ok[q]) store_wt4(a.dxp + grow[q] * 64 + c4, os_sum4(p0 + 16 * q));
    lds_barrier();   // the partial tiles are read: the region becomes the patch of dq
    zero_ring();
  }

  // ---- d x_q = dgrad of conv_in_q (dq)
#pragma unroll
  for (int u = 0; u < MI; ++u) {
    put4(hz[u], dqm[u]);
    put4(hz[u] + Z, dql[u]);
  }
  conv(a.Wq, 1, K64N64{});
#pragma unroll
  for (int q = 0; q < NQ; ++q)
    if (ok[q]) store_wt4(a.dxq + grow[q] * 64 + c4, os_sum4(p0 + 16 * q));
}

// ---------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------

// forward: the p_params / q_params tiles behind the patch region
static size_t si_lds_bytes(int mi, int halo_px, bool fwd = true) {
  const size_t BM = 32 * mi, patch = (size_t)3 * halo_px * SI_LDK * 2, os = BM * SI_LDO * 4;
  return SI_SCR_BYTES + (patch > 4 * os ? patch : 4 * os) + (fwd ? 2 * os : 0);
}

// a 3x3 / stride 1 / pad 1 convolution on fp32 NHWC tensors with C1 -> Cout channels whose weight view can be pre-split
static bool si_conv_ok(const lvae_conv_desc& d, int C1, int Cout, int N, int H, int W, int gather = LVAE_GATHER_CONV) {
  return d.w != nullptr && d.KH == 3 && d.KW == 3 && d.stride == 1 && d.pad == 1 && d.gather == gather && d.x2 == nullptr && d.C2 == 0 &&
         d.C1 == C1 && d.Cout == Cout && d.N == N && d.H == H && d.W == W && d.OH == H && d.OW == W && d.x_dtype == LVAE_DT_F32 &&
         d.y_dtype == LVAE_DT_F32 && d.in_scale == nullptr && d.in_fold == nullptr && d.out_scale == nullptr && d.in_act == LVAE_ACT_NONE &&
         d.out_act == LVAE_ACT_NONE && d.stats_out == nullptr && al16(d.w) &&
         al16_or_null(d.bias) && al16_or_null(d.x) && al16_or_null(d.y) && al16_or_null(d.workspace);
}

// Tile size by resblock_img.hip's rule: 64 pixels, or 32 where 64-pixel tiles would fill at most half the CUs. False: the patch does not fit.
static bool si_geometry(int N, int H, int W, StochImgArgs& a, int& mi, bool fwd) {
  const int HW = H * W;
  mi = (HW <= 16 && 32 % HW == 0 && ((int64_t)N * HW + 63) / 64 <= 128) ? 1 : 2;
  const int BM = 32 * mi;
  a = StochImgArgs{};
  a.N = N;
  a.W = W;
  a.HW = HW;
  a.NI = BM / HW;
  a.halo_h = H + 2;
  a.halo_w = W + 2;
  a.halo_px = a.NI * a.halo_h * a.halo_w;
  a.nwg = (N + a.NI - 1) / a.NI;
  a.m_hw = fastdiv_magic(HW);
  a.m_w = fastdiv_magic(W);
  a.m_per_img = fastdiv_magic(a.halo_h * a.halo_w);
  a.m_halo_w = fastdiv_magic(a.halo_w);
  return si_lds_bytes(mi, a.halo_px, fwd) <= 160 * 1024;
}

// Every condition the fused forward depends on: kernel 3 / stride 1 / pad 1, 64 input channels, Z = 32, H*W a divisor of 64, fp32 NHWC
// storage, 16-byte aligned operands and weight views, q present, mode 0 | 1 | 2.
static bool stoch_img_plan(const lvae_stoch_block* b, StochImgArgs& a, int& mi) {
  static const bool off = tune("LVAE_DISABLE_STOCH_IMG", 0) != 0;  // A/B switch (tuning builds only)
  if (off || b == nullptr) return false;
  const lvae_conv_desc &q = b->conv_q, &o = b->conv_out;
  const int N = q.N, H = q.H, W = q.W;
  if (N < 1 || H < 1 || W < 1 || (int64_t)H * W > 64) return false;
  const int HW = H * W;
  if (64 % HW != 0 || (int64_t)N * HW * 64 >= ((int64_t)1 << 31)) return false;
  if (b->mode < 0 || b->mode > 2) return false;
  if (!si_conv_ok(q, 64, 2 * SI_Z, N, H, W) || !si_conv_ok(o, SI_Z, 64, N, H, W)) return false;
  const bool has_p = b->conv_p.w != nullptr;
  if (has_p && !si_conv_ok(b->conv_p, 64, 2 * SI_Z, N, H, W)) return false;
  if (!has_p && (b->p_given == nullptr || !al16(b->p_given))) return false;
  if (!al16_or_null(b->eps) || !al16_or_null(b->kl_spatial)) return false;
  return si_geometry(N, H, W, a, mi, true);
}

template <int MI, bool HAS_P>
static int si_launch(const StochImgArgs& a, hipStream_t s) {
  return launch_lds<stoch_img_fwd_kernel<MI, HAS_P>>("stoch_block_fwd", dim3(a.nwg), dim3(256), si_lds_bytes(MI, a.halo_px), 160 * 1024, s, a);
}

// runs the plan; cannot decline
static int stoch_img_fwd_launch(const StochImgArgs& a, int mi, bool has_p, hipStream_t s) {
  if (mi == 1) return has_p ? si_launch<1, true>(a, s) : si_launch<1, false>(a, s);
  return has_p ? si_launch<2, true>(a, s) : si_launch<2, false>(a, s);
}

// The backward's conditions: the forward's, on the three dgrad descriptors (LVAE_GATHER_TRANSPOSED; C1 / Cout in the direction of use).
static bool stoch_img_bwd_plan(const lvae_stoch_block_bwd* b, StochImgArgs& a, int& mi) {
  static const bool off = tune("LVAE_DISABLE_STOCH_IMG", 0) != 0;  // A/B switch (tuning builds only)
  if (off || b == nullptr) return false;
  const lvae_conv_desc &q = b->dgrad_q, &o = b->dgrad_out;
  const int N = q.N, H = q.H, W = q.W;
  if (N < 1 || H < 1 || W < 1 || (int64_t)H * W > 64) return false;
  const int HW = H * W;
  if (64 % HW != 0 || (int64_t)N * HW * 64 >= ((int64_t)1 << 31)) return false;
  if (b->mode < 0 || b->mode > 2) return false;
  if (!si_conv_ok(q, 2 * SI_Z, 64, N, H, W, LVAE_GATHER_TRANSPOSED) || !si_conv_ok(o, 64, SI_Z, N, H, W, LVAE_GATHER_TRANSPOSED)) return false;
  const bool has_p = b->dgrad_p.w != nullptr;
  if (has_p && !si_conv_ok(b->dgrad_p, 2 * SI_Z, 64, N, H, W, LVAE_GATHER_TRANSPOSED)) return false;
  if (!has_p && !al16_or_null(b->dgrad_p.x)) return false;
  if (!al16_or_null(b->p) || !al16_or_null(b->q) || !al16_or_null(b->z) || !al16_or_null(b->eps) || !al16_or_null(b->dz)) return false;
  return si_geometry(N, H, W, a, mi, false);
}

template <int MI, bool HAS_P>
static int si_bwd_launch(const StochImgArgs& a, hipStream_t s) {
  return launch_lds<stoch_img_bwd_kernel<MI, HAS_P>>("stoch_block_bwd", dim3(a.nwg), dim3(256), si_lds_bytes(MI, a.halo_px, false), 160 * 1024, s, a);
}

// runs the plan; cannot decline
static int stoch_img_bwd_launch(const StochImgArgs& a, int mi, bool has_p, hipStream_t s) {
  if (mi == 1) return has_p ? si_bwd_launch<1, true>(a, s) : si_bwd_launch<1, false>(a, s);
  return has_p ? si_bwd_launch<2, true>(a, s) : si_bwd_launch<2, false>(a, s);
}

static bool si_weight_ok(const lvae_conv_desc* d) {
  return d != nullptr && d->w != nullptr && d->KH == 3 && d->KW == 3 && d->C1 >= 1 && d->C1 <= 64 && d->C2 == 0 && d->Cout >= 1 && d->Cout <= 64;
}

}  // namespace lvae

using namespace lvae;

extern "C" int32_t lvae_stoch_block_ok(const lvae_stoch_block* b) {
  StochImgArgs a;
  int mi;
  return stoch_img_plan(b, a, mi) ? 1 : 0;
}

extern "C" size_t lvae_stoch_block_workspace(const lvae_conv_desc* d) { return si_weight_ok(d) ? conv3x3_bf16_workspace(d, 3) : 0; }

extern "C" int lvae_stoch_block_prepare_entry(const lvae_conv_desc* d, void* entry) {
  LVAE_REQUIRE(si_weight_ok(d) && entry, LVAE_EINVAL, "lvae_stoch_block_prepare_entry: needs a 3x3 descriptor with at most 64 -> 64 channels and an entry buffer");
  LVAE_REQUIRE(d->workspace && (size_t)d->workspace_bytes >= conv3x3_bf16_workspace(d, 3) && al16_or_null(d->workspace), LVAE_EINVAL,
               "lvae_stoch_block_prepare_entry: no scratch for the pre-split weights");
  conv3x3_bf16_prep_entry(d, 3, entry);
  return 0;
}

extern "C" int lvae_stoch_block_fwd_f32(const lvae_stoch_block* b, void* stream) {
  LVAE_REQUIRE(b != nullptr, LVAE_EINVAL, "lvae_stoch_block_fwd_f32: null descriptor");
  StochImgArgs a;
  int mi = 2;
  LVAE_REQUIRE(stoch_img_plan(b, a, mi), LVAE_EINVAL,
               "lvae_stoch_block_fwd_f32: shape not supported (lvae_stoch_block_ok(b) == 0: 3x3 / stride 1 / pad 1, 64 input channels, Z = 32, "
               "H*W a divisor of 64, fp32 NHWC tensors, 16-byte aligned operands and weight views, q present, mode 0..2)");
  const bool has_p = b->conv_p.w != nullptr;
  const lvae_conv_desc* cv[3] = {has_p ? &b->conv_p : nullptr, &b->conv_q, &b->conv_out};
  LVAE_REQUIRE(b->conv_q.x && b->conv_q.y && b->conv_out.x && b->conv_out.y && (!has_p || (b->conv_p.x && b->conv_p.y)) && b->logprob_p && b->logprob_q &&
                   b->kl_samplewise && (b->mode == 1 || b->eps),
               LVAE_EINVAL, "lvae_stoch_block_fwd_f32: null input / output tensor (eps may be null in mode 1 only)");
  hipStream_t s = (hipStream_t)stream;
  for (const lvae_conv_desc* d : cv) {
    if (d == nullptr) continue;
    LVAE_REQUIRE(d->workspace != nullptr && (size_t)d->workspace_bytes >= conv3x3_bf16_workspace(d, 3), LVAE_EWORKSPACE,
                 "lvae_stoch_block_fwd_f32: workspace (pre-split weights) missing or smaller than lvae_stoch_block_workspace(d)");
    if (!d->workspace_ready) {
      const int rc = conv3x3_bf16_prepare_single(d, 3, s);
      if (rc) return rc;
    }
  }
  if (has_p) {
    a.xp = b->conv_p.x;
    a.bias_p = b->conv_p.bias;
    a.Wp = static_cast<const __bf16*>(b->conv_p.workspace);
    a.p_out = b->conv_p.y;
  } else {
    a.p_in = b->p_given;
    a.p_bcast = b->p_bcast;
  }
  a.xq = b->conv_q.x;
  a.bias_q = b->conv_q.bias;
  a.Wq = static_cast<const __bf16*>(b->conv_q.workspace);
  a.q_out = b->conv_q.y;
  a.z = const_cast<float*>(b->conv_out.x);
  a.bias_o = b->conv_out.bias;
  a.Wo = static_cast<const __bf16*>(b->conv_out.workspace);
  a.out = b->conv_out.y;
  a.eps = b->eps;
  a.mode = b->mode;
  a.analytical = b->analytical_kl;
  a.lp = b->logprob_p;
  a.lq = b->logprob_q;
  a.kl = b->kl_samplewise;
  a.ks = b->kl_spatial;
  return stoch_img_fwd_launch(a, mi, has_p, s);
}

extern "C" int32_t lvae_stoch_block_bwd_ok(const lvae_stoch_block_bwd* b) {
  StochImgArgs a;
  int mi;
  return stoch_img_bwd_plan(b, a, mi) ? 1 : 0;
}

extern "C" int lvae_stoch_block_bwd_f32(const lvae_stoch_block_bwd* b, void* stream) {
  LVAE_REQUIRE(b != nullptr, LVAE_EINVAL, "lvae_stoch_block_bwd_f32: null descriptor");
  StochImgArgs a;
  int mi = 2;
  LVAE_REQUIRE(stoch_img_bwd_plan(b, a, mi), LVAE_EINVAL,
               "lvae_stoch_block_bwd_f32: shape not supported (lvae_stoch_block_bwd_ok(b) == 0: the dgrads of 3x3 / stride 1 / pad 1 convolutions, 64 input "
               "channels, Z = 32, H*W a divisor of 64, fp32 NHWC tensors, 16-byte aligned operands and weight views, mode 0..2)");
  const bool has_p = b->dgrad_p.w != nullptr;
  const lvae_conv_desc* cv[3] = {has_p ? &b->dgrad_p : nullptr, &b->dgrad_q, &b->dgrad_out};
  LVAE_REQUIRE(b->dgrad_out.x && b->dgrad_q.x && b->dgrad_q.y && b->dgrad_p.x && (!has_p || b->dgrad_p.y) && b->p && b->q && b->z && (b->mode != 0 || b->eps),
               LVAE_EINVAL, "lvae_stoch_block_bwd_f32: null input / output tensor (eps may be null unless mode 0)");
  hipStream_t s = (hipStream_t)stream;
  for (const lvae_conv_desc* d : cv) {
    if (d == nullptr) continue;
    LVAE_REQUIRE(d->workspace != nullptr && (size_t)d->workspace_bytes >= conv3x3_bf16_workspace(d, 3), LVAE_EWORKSPACE,
                 "lvae_stoch_block_bwd_f32: workspace (pre-split weights) missing or smaller than lvae_stoch_block_workspace(d)");
    if (!d->workspace_ready) {
      const int rc = conv3x3_bf16_prepare_single(d, 3, s);
      if (rc) return rc;
    }
  }
  a.d_out = b->dgrad_out.x;
  a.Wo = static_cast<const __bf16*>(b->dgrad_out.workspace);
  a.dq = const_cast<float*>(b->dgrad_q.x);
  a.dxq = b->dgrad_q.y;
  a.Wq = static_cast<const __bf16*>(b->dgrad_q.workspace);
  a.dp = const_cast<float*>(b->dgrad_p.x);
  if (has_p) {
    a.dxp = b->dgrad_p.y;
    a.Wp = static_cast<const __bf16*>(b->dgrad_p.workspace);
  }
  a.p_in = b->p;
  a.p_bcast = b->p_bcast;
  a.q_in = b->q;
  a.z_in = b->z;
  a.eps = b->eps;
  a.dz_ext = b->dz;
  a.g_lp = b->g_lp;
  a.g_lq = b->g_lq;
  a.g_kl = b->g_kl;
  a.g_ks = b->g_ks;
  a.mode = b->mode;
  a.analytical = b->analytical_kl;
  return stoch_img_bwd_launch(a, mi, has_p, s);
}
