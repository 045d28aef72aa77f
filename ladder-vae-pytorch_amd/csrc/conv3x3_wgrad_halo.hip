// Weight gradient of stride-1 "same" convolutions (3x3 pad 1, 1x1 pad 0): LDS-resident operands, wave-specialised.
//
//   dW[kh][kw][ci][co] = sum_pixels T(x)[pixel + (kh-p, kw-p)][ci] * dy[pixel][co]
//
// A workgroup owns ALL taps, one 64-wide co tile and a strided subset of the pixel tiles (so the x patch is fetched and
// transformed once, not once per kernel row); ONE workgroup per CU (the grid is sized to the CU count, which also bounds the split-K
// slab traffic). It has 8 waves with fixed roles:
//   * waves 4-7 (loaders): global -> registers -> LDS. They stage the (TH+2p) x (W+2p) x Cin patch of T(x)
//     (BatchNorm-apply + ELU recomputed once per element, channel-concat inputs read from two tensors, zero padding
//     materialised) and the dy tile of the NEXT tile into the idle LDS buffer;
//   * waves 0-3 (MFMA): one v_mfma_f32_32x32x2 chain per (kw, 64-channel ci block) over the CURRENT buffer. The A
//     fragment of tap kw is the same LDS image read kw pixels to the right, so x is fetched once per kernel row.
// One workgroup barrier per tile swaps the buffers, so a tile costs max(load, MFMA) instead of their sum (measured
// with phase-skip builds: in the single-role version the two phases added up, ~150 + ~175 us on a 32x32x64 layer).
// dy is stored with the row pitch of the x image (gap columns stay zero and contribute nothing), which makes the k-walk
// over an image linear and branch-free; the LDS reads of step s+1 are issued before the MFMAs of step s.
// Partials go to split-K slabs summed in a fixed order by wgrad_reduce_kernel (deterministic, no float atomics).
//
// Barrier protocol (T = tiles of this workgroup >= 1; both roles execute exactly T + 3 barriers):
//   all: B0 after zero-init | loaders: fill(i); bar  for i < T; bar; [bias partials]; bar
//                           | MFMA   : bar; compute(i); bar for i < T;       [slabs]; bar
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "lvae_host.h"

namespace lvae {

struct WTileArgs {
  lvae_conv_desc d;
  const float* dy;
  float* slab_w;  // [ksplit][KH*KW][Cin][Cout]
  float* slab_b;  // [ksplit][Cout] or null
  int TH, TW, NI, tiles_h, halo_w, halo_h, halo_px, ntiles, ksplit, Cin, ncot, pad, buf_floats;
  uint32_t m_thw, m_tw, m_per_img, m_halo_w, m_tiles_h;  // fastdiv magics
  int debug;  // profiling only: 1 = loaders idle, 2 = MFMA waves idle, 4 = loaders skip the x patch, 8 = loaders skip dy
};

template <int CIN_T, int NKW>
__global__ __launch_bounds__(512, 2) void conv_wgrad_ws_kernel(WTileArgs a) {
  kernarg_warmup<(sizeof(WTileArgs) < 1024 ? sizeof(WTileArgs) : 1024)>();
  const int grp = blockIdx.x;
#include "conv3x3_wgrad_halo_body.inc"
}

// Several independent weight gradients in one launch (blockIdx.y = problem): the low-resolution levels fill 16-64 CUs per
// problem, and their launches are independent of everything but their own inputs.
static_assert(kWgradTileGroup <= kMaxReduceGroup, "a group is reduced by one wgrad_reduce_grouped_launch");
struct WTileGroup {
  WTileArgs p[kWgradTileGroup];
};
static_assert(sizeof(WTileGroup) <= 4096, "kernel argument block");

template <int CIN_T, int NKW>
__global__ __launch_bounds__(512, 2) void conv_wgrad_ws_grouped_kernel(WTileGroup g) {
  kernarg_warmup<(sizeof(WTileGroup) < 1024 ? sizeof(WTileGroup) : 1024)>();
  const WTileArgs& a = g.p[blockIdx.y];
  if ((int)blockIdx.x >= a.ncot * a.ksplit) return;  // uniform per workgroup, before any barrier
  const int grp = blockIdx.x;
#include "conv3x3_wgrad_halo_body.inc"
}

static int cin_tile(int Cin) { return Cin <= 32 ? 32 : (Cin <= 64 ? 64 : 128); }

static bool wtile_plan(const lvae_conv_desc* d, WTileArgs& a) {
  const int Cin = d->C1 + d->C2;
  const bool k3 = d->KH == 3 && d->KW == 3 && d->pad == 1, k1 = d->KH == 1 && d->KW == 1 && d->pad == 0;
  if (!(k3 || k1) || d->stride != 1 || d->gather != LVAE_GATHER_CONV || d->OH != d->H || d->OW != d->W) return false;
  if ((int64_t)d->N * d->H * d->W * (Cin > d->Cout ? Cin : d->Cout) >= ((int64_t)1 << 31)) return false;  // 32-bit element offsets
  if (Cin > 128 || (k3 && Cin > 64) || d->C1 % 4 != 0 || d->C2 % 4 != 0 || d->Cout % 4 != 0 || d->W % 2 != 0) return false;
  if (!al16(d->x) || (d->x2 && !al16(d->x2)) || (d->in_scale && (!al16(d->in_scale) || !al16(d->in_shift)))) return false;
  const int cin_t = cin_tile(Cin), pad = k3 ? 1 : 0;
  // tile: as many pixels as two LDS buffers allow (at most 128), whole rows, whole images when several fit
  int BM = 128;
  for (;;) {
    if (d->W <= BM) {
      int TH = 1;
      for (int c = 1; c <= d->H; ++c)
        if (d->H % c == 0 && c * d->W <= BM) TH = c;
      int NI = BM / (TH * d->W);
      if (NI < 1) NI = 1;
      if (TH < d->H) NI = 1;
      if (NI > d->N) NI = d->N;
      a.TH = TH;
      a.TW = d->W;
      a.NI = NI;
      a.tiles_h = d->H / TH;
      a.halo_h = TH + 2 * pad;
      a.halo_w = d->W + 2 * pad;
      a.halo_px = NI * a.halo_h * a.halo_w;
      a.buf_floats = a.halo_px * cin_t + NI * TH * a.halo_w * 64 + 512;  // + look-ahead slack (dy side; the x side
                                                                            // look-ahead lands in the dy image)
      a.buf_floats = (a.buf_floats + 3) / 4 * 4;
      if ((size_t)2 * a.buf_floats * sizeof(float) <= 160 * 1024 && a.halo_px < 65536) break;
    }
    if (BM == 16) return false;
    BM /= 2;
  }
  a.pad = pad;
  a.Cin = Cin;
  a.m_thw = fastdiv_magic(a.TH * a.TW);
  a.m_tw = fastdiv_magic(a.TW);
  a.m_per_img = fastdiv_magic(a.halo_h * a.halo_w);
  a.m_halo_w = fastdiv_magic(a.halo_w);
  a.m_tiles_h = fastdiv_magic(a.tiles_h);
  a.ntiles = ((d->N + a.NI - 1) / a.NI) * a.tiles_h;
  a.ncot = (d->Cout + 63) / 64;
  int ks = 256 / a.ncot;  // one workgroup per CU: (co tiles) x ksplit ~ 256
  if (ks < 1) ks = 1;
  a.ksplit = a.ntiles < ks ? a.ntiles : ks;
  return a.ntiles < 65536;
}

// f(cin_t, nkw) with the values of a template pair <CIN_T, NKW> as compile-time constants: 0 <32,3>, 1 <64,3>, 2 <32,1>, 3 <64,1>, 4 <128,1>
template <typename F>
static int with_tile_pair(int pair, F f) {
  using std::integral_constant;
  switch (pair) {
    case 0: return f(integral_constant<int, 32>{}, integral_constant<int, 3>{});
    case 1: return f(integral_constant<int, 64>{}, integral_constant<int, 3>{});
    case 2: return f(integral_constant<int, 32>{}, integral_constant<int, 1>{});
    case 3: return f(integral_constant<int, 64>{}, integral_constant<int, 1>{});
    default: return f(integral_constant<int, 128>{}, integral_constant<int, 1>{});
  }
}

bool conv_wgrad_tile_plan(const lvae_conv_desc* d, WgradPlan& p) {
  WTileArgs a;
  if (!wtile_plan(d, a)) return false;
  const int cin_t = cin_tile(a.Cin);
  p.group = (d->KH == 3 ? 0 : 2) + (cin_t == 32 ? 0 : (cin_t == 64 ? 1 : 2));   // group key: the template pair of with_tile_pair
  p.set_slabs(a.ksplit, (size_t)d->KH * d->KW * a.Cin * d->Cout, d->Cout);
  return true;
}

// the kernel arguments and the slab reduce of one gradient; returns the kernel's workgroups
static int tile_fill(const WgradOp& o, WTileArgs& a, ReduceArgs& r) {
  static const int dbg = lvae::debug_phase_switch("LVAE_WG_DEBUG");  // phase-skip builds (-DLVAE_PHASE_DEBUG) only; 0 in the product
  const lvae_conv_desc* d = o.d;
  wtile_plan(d, a);
  a.d = *d;
  a.dy = o.dy;
  a.debug = dbg;
  a.slab_w = o.slab_w();
  a.slab_b = o.slab_b();
  r = ReduceArgs{a.slab_w, a.slab_b, a.ksplit, d->KH * d->KW, a.Cin, d->Cout, d->w_stap, d->w_sk, d->w_sn, o.dw, o.db};
  return a.ncot * a.ksplit;
}

static size_t tile_lds(const WTileArgs& a) { return (size_t)2 * a.buf_floats * sizeof(float); }

// n <= kWgradTileGroup gradients of one plan.group, each with its own workspace (16-byte aligned dy: the route checked it). One gradient
// runs the single kernel and its reduce, several the grouped kernel and one grouped reduce.
int conv_wgrad_tile_launch(const WgradOp* o, int n, hipStream_t s) {
  WTileGroup g;
  ReduceArgs r[kWgradTileGroup];
  int max_wgs = 0;
  size_t lds = 0;
  for (int i = 0; i < n; ++i) {
    max_wgs = std::max(max_wgs, tile_fill(o[i], g.p[i], r[i]));
    lds = std::max(lds, tile_lds(g.p[i]));
  }
  for (int i = n; i < kWgradTileGroup; ++i) g.p[i] = g.p[0];
  const int rc = with_tile_pair(o->plan.group, [&](auto cin_t, auto nkw) {
    constexpr int C = decltype(cin_t)::value, K = decltype(nkw)::value;
    if (n == 1) return launch_lds<conv_wgrad_ws_kernel<C, K>>("conv_wgrad_ws", dim3(max_wgs), dim3(512), lds, 160 * 1024, s, g.p[0]);
    return launch_lds<conv_wgrad_ws_grouped_kernel<C, K>>("conv_wgrad_ws_grouped", dim3(max_wgs, n), dim3(512), lds, 160 * 1024, s, g);
  });
  if (rc) return rc;
  if (n == 1) wgrad_reduce_launch(r->slab_w, r->slab_b, r->ksplit, r->ntaps, r->Cin, r->Cout, r->stap, r->sk, r->sn, r->dw, r->db, s);
  else wgrad_reduce_grouped_launch(r, n, s);
  LVAE_LAUNCH_CHECK(n == 1 ? "conv2d_wgrad_reduce" : "conv2d_wgrad_reduce_grouped");
  return 0;
}

}  // namespace lvae
