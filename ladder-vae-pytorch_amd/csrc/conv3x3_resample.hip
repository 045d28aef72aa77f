// 3x3 / stride 2 / pad 1 resampling convolutions, "position-major" like conv3x3_pos.hip: the strided convolution of a bottom-up
// `down` block (LVAE_GATHER_CONV), the transposed convolution of a top-down `up` block (LVAE_GATHER_TRANSPOSED), and the input
// gradient of each, which is the other gather.
//
// The GEMM rows of a workgroup are 32 IMAGES at ONE OUTPUT position (P = OH*OW positions), the columns 32 output channels. Which taps
// an output position has is then the same for all 32 rows (tap_coord of conv_igemm.hip, evaluated once per workgroup on scalars):
//  * conv gather:       i = 2*o - 1 + k, k = 0..2, valid inside the input: 9 taps, fewer on the top / left edge (and on the
//                       bottom / right edge of an odd-sized input);
//  * transposed gather: t = o + 1 - k must be even, i = t/2 < extent: an even o has k = 1 only, an odd o has k = 0 and 2, so a
//                       position has 1, 2 or 4 taps (2.25 on average) where the generic kernel walks all 9.
// Per axis the kernel enumerates the 3 (conv) or 2 (transposed) CANDIDATE taps, so registers and LDS are sized for 9 or 4 taps.
// As in conv3x3_pos.hip the launch is single shot: every global load (the input rows and the weight tile of every valid tap) is
// issued before the first use, ONE barrier, the 4 waves split the reduction channels and are summed through LDS in the epilogue
// (bias, per-(image, channel) scale, activation). No statistics epilogue and no folded BatchNorm finalize: the layers this runs
// have neither, and the plan says so (rows 0, folds false), which keeps the stride-1 kernel's emitted code as it was (the stride
// is not a template parameter of conv3x3_pos_kernel because that would rename its instantiations; profiles/resample_pos_isa.txt).
// The weight tap index is kh*3 + kw for both gathers, as in the generic kernel.
#include "lvae_host.h"

namespace lvae {

struct ResampleArgs {
  lvae_conv_desc d;
  int P, Cin, n_groups, ntn;
  uint32_t m_ow;  // fastdiv magic of OW
};

// candidate j of one axis for output coordinate o: weight tap k and input coordinate i; false when the tap does not exist
template <bool TRANSPOSED>
__device__ __forceinline__ bool resample_tap(int o, int j, int limit, int& k, int& i) {
  if (!TRANSPOSED) {
    k = j;
    i = 2 * o - 1 + j;
    return (unsigned)i < (unsigned)limit;
  }
  const bool odd = (o & 1) != 0;
  k = odd ? 2 * j : 1;
  i = (o + 1 - k) >> 1;  // o + 1 - k is even and >= 0 by the choice of k
  return (odd || j == 0) && i < limit;
}

template <int CIN_T, bool B_KCONTIG, bool TRANSPOSED>
__global__ __launch_bounds__(256) void conv3x3_resample_kernel(ResampleArgs a) {
  kernarg_warmup<(sizeof(ResampleArgs) < 1024 ? sizeof(ResampleArgs) : 1024)>();
  constexpr int NT = TRANSPOSED ? 2 : 3;     // candidate taps per axis
  constexpr int MAXT = NT * NT;
  constexpr int LDA = CIN_T + 4;             // A row pitch (floats): conflict-free ds_read_b128 (as conv3x3_pos.hip)
  constexpr int CIN4 = CIN_T / 4;            // float4 per A row
  constexpr int RPP = 256 / CIN4;            // A rows per pass of the 256 threads (16 at 64 channels, 32 at 32)
  constexpr int APT = 32 / RPP;              // passes per tap (2 / 1)
  constexpr int ASZ = 32 * LDA;              // floats per A tap slot
  constexpr int BSZ = B_KCONTIG ? 32 * LDA : CIN_T * 32;  // floats per B tap slot ([n][k] padded | [k][n])
  constexpr int BPT = CIN_T * 32 / 4 / 256;  // float4 of a weight tap per thread (2 / 1)
  constexpr int KW_ = CIN_T / 4;             // reduction channels per wave (16 / 8)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const lvae_conv_desc& d = a.d;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 31, lh = lane >> 5;

  const int bid = blockIdx.x;
  const int tile_n = bid % a.ntn, rest = bid / a.ntn;
  const int pos = rest % a.P, ig = rest / a.P;
  const int oy = fastdiv(pos, a.m_ow), ox = pos - oy * d.OW;
  const int n0 = ig * 32, co0 = tile_n * 32;
  const int Cin = a.Cin;
  const int nrows = min(32, d.N - n0);  // images of this group that exist

  // ---- valid taps (wave uniform) and ALL global loads: A rows and the weight tile of every valid tap
  f32x4 av[MAXT][APT], bv[MAXT][BPT];
  const int c4 = (t % CIN4) * 4, r0 = t / CIN4;
  const bool c_ok = c4 < Cin;
  unsigned valid = 0;
#pragma unroll
  for (int c = 0; c < MAXT; ++c) {
    int kh, kw, iy, ix;
    const bool vy = resample_tap<TRANSPOSED>(oy, c / NT, d.H, kh, iy);
    const bool vx = resample_tap<TRANSPOSED>(ox, c % NT, d.W, kw, ix);
    if (!(vy && vx)) continue;  // uniform
    valid |= 1u << c;
#pragma unroll
    for (int p = 0; p < APT; ++p) {
      const int r = r0 + p * RPP;
      const bool ok = (r < nrows) & c_ok;
      const size_t off = ok ? ((size_t)((n0 + r) * d.H + iy) * d.W + ix) * Cin + c4 : 0;
      av[c][p] = *reinterpret_cast<const f32x4*>(d.x + off);
    }
    const float* wt = d.w + (int64_t)(kh * 3 + kw) * d.w_stap;
#pragma unroll
    for (int p = 0; p < BPT; ++p) {
      const int idx = t + 256 * p;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (B_KCONTIG) {
        const int n = idx / CIN4, k = (idx - n * CIN4) * 4;
        if (co0 + n < d.Cout && k < Cin) v = *reinterpret_cast<const f32x4*>(wt + (int64_t)(co0 + n) * d.w_sn + k);
      } else {
        const int k = idx >> 3, n = (idx & 7) * 4;
        if (k < Cin && co0 + n < d.Cout) v = *reinterpret_cast<const f32x4*>(wt + (int64_t)k * d.w_sk + co0 + n);
      }
      bv[c][p] = v;
    }
  }

  f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
  const bool has_tf = d.in_scale != nullptr;
  if (has_tf && c_ok) {
    sc = *reinterpret_cast<const f32x4*>(d.in_scale + c4);
    sh = *reinterpret_cast<const f32x4*>(d.in_shift + c4);
  }

  // ---- registers -> LDS (input transform applied once per element; rows of images that do not exist are zero)
  const int ntaps = __popc(valid);
  float* As = smem;
  float* Bs = smem + (size_t)ntaps * ASZ;
  {
    int slot = 0;
#pragma unroll
    for (int c = 0; c < MAXT; ++c) {
      if (!((valid >> c) & 1u)) continue;
#pragma unroll
      for (int p = 0; p < APT; ++p) {
        const int r = r0 + p * RPP;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if ((r < nrows) & c_ok) {
          v = av[c][p];
          if (has_tf) v = act_fwd4(v * sc + sh, d.in_act);
        }
        *reinterpret_cast<f32x4*>(As + slot * ASZ + r * LDA + c4) = v;
      }
#pragma unroll
      for (int p = 0; p < BPT; ++p) {
        const int idx = t + 256 * p;
        if (B_KCONTIG) {
          const int n = idx / CIN4, k = (idx - n * CIN4) * 4;
          *reinterpret_cast<f32x4*>(Bs + slot * BSZ + n * LDA + k) = bv[c][p];
        } else {
          const int k = idx >> 3, n = (idx & 7) * 4;
          *reinterpret_cast<f32x4*>(Bs + slot * BSZ + k * 32 + n) = bv[c][p];
        }
      }
      ++slot;
    }
  }
  __syncthreads();

  // ---- MFMAs: wave w reduces channels [w*KW_, (w+1)*KW_) of every tap
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const int kb = wave * KW_;
  for (int slot = 0; slot < ntaps; ++slot) {
    const float* Ab = As + slot * ASZ + li * LDA + kb + 4 * lh;
    const float* Bb = Bs + slot * BSZ;
#pragma unroll
    for (int q = 0; q < KW_ / 8; ++q) {
      const f32x4 af = *reinterpret_cast<const f32x4*>(Ab + q * 8);
      f32x4 bf;
      if (B_KCONTIG) {
        bf = *reinterpret_cast<const f32x4*>(Bb + li * LDA + kb + q * 8 + 4 * lh);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) bf[j] = Bb[(kb + q * 8 + 4 * lh + j) * 32 + li];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[j], bf[j], acc, 0, 0, 0);
    }
  }
  __syncthreads();  // operands are dead: LDS becomes the 4 partial output tiles [wave][32 rows][36]

  constexpr int LDO = 36;
  float* Os = smem;
#pragma unroll
  for (int r = 0; r < 16; ++r) Os[wave * 32 * LDO + ((r & 3) + 8 * (r >> 2) + 4 * lh) * LDO + li] = acc[r];
  __syncthreads();

  // ---- epilogue: thread -> (row = image, 4 channels); 128-byte row segments
  const int row = t >> 3, oc4 = (t & 7) * 4, col = co0 + oc4;
  if (row < nrows && col < d.Cout) {
    f32x4 v = *reinterpret_cast<const f32x4*>(Os + row * LDO + oc4);
#pragma unroll
    for (int w = 1; w < 4; ++w) v += *reinterpret_cast<const f32x4*>(Os + w * 32 * LDO + row * LDO + oc4);
    if (d.bias) v += *reinterpret_cast<const f32x4*>(d.bias + col);
    const int n = n0 + row;
    if (d.out_scale) v = v * *reinterpret_cast<const f32x4*>(d.out_scale + (size_t)n * d.Cout + col);
    v = act_fwd4(v, d.out_act);
    const size_t o = ((size_t)(n * d.OH + oy) * d.OW + ox) * d.Cout + col;
    *reinterpret_cast<f32x4*>(d.y + o) = v;
  }
}

// eligibility: 3x3 / stride 2 / pad 1, one source of at most 64 channels, fp32 storage, vector-aligned operands
static bool resample_select(const lvae_conv_desc* d, bool& ncontig) {
  static const bool off = tune("LVAE_DISABLE_RESAMPLE", 0) != 0;  // A/B switch (tuning builds only)
  if (off) return false;
  const int Cin = d->C1;
  if (d->KH != 3 || d->KW != 3 || d->stride != 2 || d->pad != 1 || d->x2 != nullptr || d->C2 != 0) return false;
  if (d->gather != LVAE_GATHER_CONV && d->gather != LVAE_GATHER_TRANSPOSED) return false;
  if (d->x_dtype != LVAE_DT_F32 || d->y_dtype != LVAE_DT_F32) return false;
  if (Cin > 64 || Cin % 4 != 0 || d->Cout % 4 != 0 || d->w_stap % 4 != 0) return false;
  if (!al16_or_null(d->x) || !al16_or_null(d->w) || !al16_or_null(d->y) || !al16_or_null(d->bias) || !al16_or_null(d->out_scale) || !al16_or_null(d->in_scale) ||
      !al16_or_null(d->in_shift))
    return false;
  const bool kc = d->w_sk == 1 && d->w_sn % 4 == 0, nc = d->w_sn == 1 && d->w_sk % 4 == 0;
  if (!kc && !nc) return false;
  // The conv gather holds up to 9 taps in LDS (153 KB at 64 channels: one workgroup per CU), so a launch takes workgroups / CUs rounds of
  // one single-shot workgroup each. profiles/resample_pos_ab.txt, batch 256, 64 -> 64 channels: at 1,024 workgroups (8x8 outputs) it
  // beats the generic kernel, 29.6 against 35.4 us; at 4,096 (16x16 outputs, the 64x64 config) it loses, 108 against 76 us. Nothing in
  // between was measured, so it stays with the generic kernel. The transposed gather (<= 4 taps) won at every size up to 16,384 workgroups.
  if (d->gather == LVAE_GATHER_CONV && (int64_t)((d->N + 31) / 32) * d->OH * d->OW * ((d->Cout + 31) / 32) > 1024) return false;
  ncontig = nc;
  return true;
}

// plan: the direct fp32-MFMA arithmetic of the generic kernel (LVAE_VARIANT_DIRECT), no workspace, no statistics rows, no fold
bool conv3x3_resample_plan(const lvae_conv_desc* d, ConvPlan& p) {
  bool ncontig;
  if (!resample_select(d, ncontig)) return false;
  p = ConvPlan{};
  return true;
}

template <int CIN_T, bool KC, bool TR>
static int launch_resample(const ResampleArgs& a, hipStream_t s) {
  // taps a position can have at most, per axis: 3 (conv) or 2 (transposed), and never more than the input has rows / columns
  constexpr int nt = TR ? 2 : 3;
  const int th = a.d.H >= nt ? nt : a.d.H, tw = a.d.W >= nt ? nt : a.d.W;
  constexpr size_t asz = (size_t)32 * (CIN_T + 4), bsz = KC ? (size_t)32 * (CIN_T + 4) : (size_t)CIN_T * 32;
  size_t lds = (size_t)th * tw * (asz + bsz) * sizeof(float);
  const size_t lds_out = (size_t)4 * 32 * 36 * sizeof(float);
  if (lds < lds_out) lds = lds_out;
  return launch_lds<conv3x3_resample_kernel<CIN_T, KC, TR>>("conv3x3_resample", dim3(a.n_groups * a.P * a.ntn), dim3(256), lds, 157 * 1024, s, a);
}

template <int CIN_T, bool KC>
static int launch_resample_gather(const ResampleArgs& a, hipStream_t s) {
  return a.d.gather == LVAE_GATHER_TRANSPOSED ? launch_resample<CIN_T, KC, true>(a, s) : launch_resample<CIN_T, KC, false>(a, s);
}

int conv3x3_resample_launch(const lvae_conv_desc* d, hipStream_t s) {
  bool ncontig = false;
  resample_select(d, ncontig);  // (the plan accepted d)
  ResampleArgs a;
  a.d = *d;
  a.d.in_fold = nullptr;
  a.P = d->OH * d->OW;
  a.Cin = d->C1;
  a.n_groups = (d->N + 31) / 32;
  a.ntn = (d->Cout + 31) / 32;
  a.m_ow = fastdiv_magic(d->OW);
  const bool kc = !ncontig;
  if (d->C1 <= 32) return kc ? launch_resample_gather<32, true>(a, s) : launch_resample_gather<32, false>(a, s);
  return kc ? launch_resample_gather<64, true>(a, s) : launch_resample_gather<64, false>(a, s);
}

}  // namespace lvae
