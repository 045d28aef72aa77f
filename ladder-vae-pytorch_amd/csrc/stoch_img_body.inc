// Shared opening of stoch_img_fwd_kernel and stoch_img_bwd_kernel (stoch_img.hip), textually included at the top of both bodies (a call
// into a __device__ function with the argument block by reference cost resblock_img.hip's ancestors a 384-VGPR spill). Expects the template
// parameter MI and the argument block `a` (StochImgArgs); defines the tile's index maps and the LDS helpers:
//   zero_ring()            zero ring of the patch planes in As
//   put4(off, v)           four fp32 values -> the three bf16 piece planes at element offset `off`
//   conv(W, flip, tag)     one 3x3 convolution of the patch in As into the partial tiles Os (SiConv<shape> tag below)
//   os_sum4(p) / os_sum2(p)  this thread's four channels of tile row p, summed over the four / two partial tiles
//   pf_issue() / pf_drain()  L2 warm-up of the launch's three weight sets
constexpr int SPLIT = 3, BM = 32 * MI, LDK = SI_LDK, LDO = SI_LDO, NQ = BM / 16, Z = SI_Z;
constexpr int OSW = BM * LDO;
extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
kernarg_warmup<sizeof(StochImgArgs)>();
float* scr = reinterpret_cast<float*>(smem_raw);
unsigned char* mainr = smem_raw + SI_SCR_BYTES;
__bf16* As = reinterpret_cast<__bf16*>(mainr);   // [SPLIT][halo_px][LDK]; the partial output tiles alias it
float* Os = reinterpret_cast<float*>(mainr);     // [4][BM][LDO]
const int a_plane = a.halo_px * LDK;

const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 31, lh = lane >> 5;
const int bid = blockIdx.x, HW = a.HW;
const int n0 = bid * a.NI;
const int nvalid = min(BM, (a.N - n0) * HW);   // pixel rows of this tile that exist
const size_t row0 = (size_t)n0 * HW;           // global pixel row of tile row 0 (whole images: tile rows are consecutive pixels)
const int c4 = (t & 15) * 4, p0 = t >> 4;      // staging / store map: thread -> rows p0 + 16 q, channels c4 .. c4 + 3
const int ec = (t & 7) * 4, er0 = t >> 3;      // elementwise map: thread -> rows er0 + 32 u, latent channels ec .. ec + 3
const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

// ---- L2 warm-up. Every convolution of a step has weights of its own, so the 3 x 216 KB this launch streams are cold in its XCD's L2 when it
// starts, and a wave's three-deep weight ring does not cover a miss to memory (in the step the first form of this kernel ran 27-33 us where
// it ran 15-26 us back to back). As in resblock_img.hip the workgroups of an XCD (round-robin placement: speed only) touch one word of every
// 128-byte line of the ranges up front: plain loads the compiler tracks, consumed by an empty asm once the operand rows requested BEHIND them
// have been used (the memory counter retires in order: the drain costs no wait).
constexpr int PFN = 7, SI_W_LINES = 9 * SPLIT * 4096 * 2 / 128;   // touches per lane and range: 7 x 256 lanes cover the 1,728 lines of a range
unsigned pf_dump[3][PFN];
auto pf_issue = [&]() {
  const __bf16* rng[3] = {a.Wp, a.Wq, a.Wo};
  const int per_xcd = (a.nwg + 7) >> 3, part = bid >> 3, per = (SI_W_LINES + per_xcd - 1) / per_xcd;
  const int lo = part * per, hi = min(lo + per, SI_W_LINES);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const char* base = reinterpret_cast<const char*>(rng[k]) + (size_t)(lo + t) * 128;
#pragma unroll
    for (int i = 0; i < PFN; ++i) {
      pf_dump[k][i] = 0;
      if (rng[k] != nullptr && lo + t + 256 * i < hi) pf_dump[k][i] = *reinterpret_cast<const unsigned*>(base + i * 256 * 128);
    }
  }
};
auto pf_drain = [&]() {
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int i = 0; i < PFN; ++i) asm volatile("" ::"v"(pf_dump[k][i]));
};

// ---- this thread's rows in both maps: patch position, global row (rows past the batch read row 0 and are masked)
int hp[NQ], hz[MI], pr[NQ], epr[MI], eimg[MI];
size_t grow[NQ], erow[MI];
bool ok[NQ], eok[MI];
#pragma unroll
for (int q = 0; q < NQ; ++q) {
  const int p = p0 + 16 * q;
  const int img = fastdiv(p, a.m_hw), r = p - img * HW;
  const int y = fastdiv(r, a.m_w), x = r - y * a.W;
  hp[q] = ((img * a.halo_h + y + 1) * a.halo_w + x + 1) * LDK + c4;
  ok[q] = p < nvalid;
  grow[q] = row0 + (ok[q] ? p : 0);
  pr[q] = r;   // pixel inside its image: the row of a broadcast p_params
}
#pragma unroll
for (int u = 0; u < MI; ++u) {
  const int p = er0 + 32 * u;
  const int img = fastdiv(p, a.m_hw), r = p - img * HW;
  const int y = fastdiv(r, a.m_w), x = r - y * a.W;
  hz[u] = ((img * a.halo_h + y + 1) * a.halo_w + x + 1) * LDK + ec;
  eok[u] = p < nvalid;
  erow[u] = row0 + (eok[u] ? p : 0);
  epr[u] = r;
  eimg[u] = eok[u] ? n0 + img : n0;
}

auto zero_ring = [&]() {
  const int per_img = a.halo_h * a.halo_w;
  const bf16x8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int idx = t; idx < a.halo_px * 8; idx += 256) {
    const int px = idx >> 3, c8 = (idx & 7) * 8;
    const int img = fastdiv(px, a.m_per_img), r = px - img * per_img;
    const int hy = fastdiv(r, a.m_halo_w), hx = r - hy * a.halo_w;
    if (hy == 0 || hy == a.halo_h - 1 || hx == 0 || hx == a.halo_w - 1) {
#pragma unroll
      for (int k = 0; k < SPLIT; ++k) *reinterpret_cast<bf16x8*>(As + k * a_plane + px * LDK + c8) = z8;
    }
  }
};
auto put4 = [&](int off, f32x4 v) {
  bf16x4 pl[SPLIT];
  split4_packed<SPLIT>(v, pl);
#pragma unroll
  for (int k = 0; k < SPLIT; ++k) *reinterpret_cast<bf16x4*>(As + k * a_plane + off) = pl[k];
};

// ---- per-lane patch row of its A-fragment pixels (element offset inside a plane; tap (0, 0) = the pixel's upper-left neighbour)
int hbase[MI];
#pragma unroll
for (int mb = 0; mb < MI; ++mb) {
  const int p = mb * 32 + li;
  const int img = fastdiv(p, a.m_hw), r = p - img * HW;
  const int ty = fastdiv(r, a.m_w), tx = r - ty * a.W;
  hbase[mb] = ((img * a.halo_h + ty) * a.halo_w + tx) * LDK + 8 * lh;
}

// One 3x3 convolution of the patch in As: 9 k-steps per wave, no barrier inside, B three taps ahead from L2, A one tap ahead from LDS;
// then the waves' partial tiles go to Os (which aliases the patch). Shapes (reduction channels x output channels):
//   SI_K64_N64  k block = wave, both output halves, four partial tiles           (conv_in_p / conv_in_q and their dgrads)
//   SI_K32_N64  k block = wave & 1, output half = wave >> 1, two partial tiles   (conv_out)
//   SI_K64_N32  k block = wave, output half 0, four partial tiles of 32 columns  (dgrad of conv_out)
// flip: the taps mirrored (dgrad). The caller has staged the patch; the barrier that publishes it is here, behind the first weight requests.
auto conv = [&](const __bf16* Wt, const int flip, auto shape_tag) __attribute__((always_inline)) {
  constexpr int SHAPE = decltype(shape_tag)::value;
  constexpr int NH = SHAPE == SI_K64_N64 ? 2 : 1, RING = 3;
  const int kb = SHAPE == SI_K32_N64 ? (wave & 1) : wave, nh0 = SHAPE == SI_K32_N64 ? (wave >> 1) : 0;
  bf16x8 bq[RING][NH][SPLIT];
  const __bf16* wp_lane = Wt + (size_t)kb * SPLIT * 1024 + (size_t)nh0 * 512 + (size_t)lane * 8;
  auto load_b = [&](int tap, bf16x8 (&r)[NH][SPLIT]) {
    const __bf16* src = wp_lane + (size_t)tap * 4 * SPLIT * 1024;
#pragma unroll
    for (int p = 0; p < SPLIT; ++p)
#pragma unroll
      for (int nh = 0; nh < NH; ++nh) r[nh][p] = *reinterpret_cast<const bf16x8*>(src + p * 1024 + nh * 512);
  };
#pragma unroll
  for (int i = 0; i < RING; ++i) load_b(i, bq[i]);
  f32x16 acc[MI][NH];
#pragma unroll
  for (int mb = 0; mb < MI; ++mb)
#pragma unroll
    for (int nh = 0; nh < NH; ++nh)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mb][nh][r] = 0.f;
  lds_barrier();   // the patch is complete
  {
    bf16x8 af[2][MI][SPLIT];
    auto load_a = [&](int tap, bf16x8 (&fa)[MI][SPLIT]) {
      const int kh = tap / 3, kw = tap - kh * 3;
      const int dh = flip ? 2 - kh : kh, dw = flip ? 2 - kw : kw;
      const int off = (dh * a.halo_w + dw) * LDK + kb * 16;
#pragma unroll
      for (int p = 0; p < SPLIT; ++p)
#pragma unroll
        for (int mb = 0; mb < MI; ++mb) fa[mb][p] = *reinterpret_cast<const bf16x8*>(As + p * a_plane + hbase[mb] + off);
    };
    load_a(0, af[0]);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int cur = tap & 1;
      if (tap + 1 < 9) load_a(tap + 1, af[cur ^ 1]);
#pragma unroll
      for (int mb = 0; mb < MI; ++mb)
#pragma unroll
        for (int nh = 0; nh < NH; ++nh) acc[mb][nh] = mfma_pieces<SPLIT>(af[cur][mb], bq[tap % RING][nh], acc[mb][nh]);
      if (tap + RING < 9) load_b(tap + RING, bq[tap % RING]);
    }
  }
  lds_barrier();   // every wave is done with the patch: the region becomes the partial output tiles
#pragma unroll
  for (int mb = 0; mb < MI; ++mb)
#pragma unroll
    for (int nh = 0; nh < NH; ++nh)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        Os[kb * OSW + (mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * LDO + (nh0 + nh) * 32 + li] = acc[mb][nh][r];
  lds_barrier();
};
auto os_sum4_at = [&](int p, int c) {
  const float* o = Os + p * LDO + c;
  return (*reinterpret_cast<const f32x4*>(o) + *reinterpret_cast<const f32x4*>(o + OSW)) +
         (*reinterpret_cast<const f32x4*>(o + 2 * OSW) + *reinterpret_cast<const f32x4*>(o + 3 * OSW));
};
auto os_sum4 = [&](int p) { return os_sum4_at(p, c4); };
auto os_sum2 = [&](int p) {
  const float* o = Os + p * LDO + c4;
  return *reinterpret_cast<const f32x4*>(o) + *reinterpret_cast<const f32x4*>(o + OSW);
};
using K64N64 [[maybe_unused]] = std::integral_constant<int, SI_K64_N64>;
using K32N64 [[maybe_unused]] = std::integral_constant<int, SI_K32_N64>;
using K64N32 [[maybe_unused]] = std::integral_constant<int, SI_K64_N32>;
(void)os_sum2;   // (each kernel uses its own subset of the helpers)
(void)os_sum4;
