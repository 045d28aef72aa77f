// The training batch formed on the device: rows of an image table in HBM, chosen through an index table in HBM at a position read from
// a device step counter, written as the float32 NCHW batch LadderVAE.forward takes. One launch inside the captured step replaces the host
// collate, the pageable host-to-device copy and the copy into the graph's input buffer. Small (a CIFAR batch of 256 reads 0.8 MB and
// writes 3 MB) and launch-latency sized: one thread per four output floats, plain loads, one 16-byte store, no LDS.
#include "lvae_common.h"
#include "philox.h"

namespace lvae {

struct FeedArgs {
  static constexpr bool aug = false;
  const void* src;            // [N] images, uint8 or float32, each CHW or HWC contiguous
  const int32_t* index;       // [steps_per_epoch * B_global] image numbers, or null: images base, base + 1, ...
  const int64_t* cursor;      // [1] completed steps, or null: position 0
  float* out;                 // [n_rows][C][H][W]
  long long base;
  int N, C, HW, chw;
  int steps_per_epoch, B_global, lo, n_rows;
  int f32, hwc, vec;
};

// The augmenting gather (lvae_batch_gather_aug_f32): the same thread map, the noise of lvae_feed_aug on top.
struct AugFeedArgs : FeedArgs {
  static constexpr bool aug = true;
  unsigned long long seed, position;
  int mode, hflip, fixed, W;
};

// The position taken when there is no cursor.
__device__ __forceinline__ unsigned long long feed_position(const FeedArgs&) { return 0ull; }
__device__ __forceinline__ unsigned long long feed_position(const AugFeedArgs& a) { return a.position; }

// Element e (CHW order) of image `img`, from either layout and either storage type.
__device__ __forceinline__ float feed_elem(const FeedArgs& a, size_t img, int e) {
  const int c = e / a.HW, hw = e - c * a.HW;
  const size_t off = img * (size_t)a.chw + (a.hwc ? (size_t)hw * a.C + c : (size_t)e);
  return a.f32 ? static_cast<const float*>(a.src)[off] : byte_to_unit(static_cast<const unsigned char*>(a.src)[off]);
}

// What the augmenting gather writes for a byte b / a float v of the table and the uniform draw u of the output element.
__device__ __forceinline__ float aug_u8(const AugFeedArgs& a, unsigned b, float u) {
  if (a.mode == LVAE_AUG_DEQUANTIZE) return fminf(((float)b + u) * 0.00390625f, 0x1.fffffep-1f);
  const float v = byte_to_unit(b);
  return a.mode == LVAE_AUG_BINARIZE ? (u < v ? 1.f : 0.f) : v;
}
__device__ __forceinline__ float aug_f32(const AugFeedArgs& a, float v, float u) {
  return a.mode == LVAE_AUG_BINARIZE ? (u < v ? 1.f : 0.f) : v;
}

// Four outputs e .. e + 3 of one row of image `img`, augmented. P, g: the step and stream words of the noise (lvae_hip.h).
__device__ __forceinline__ void gather_aug(const AugFeedArgs& a, size_t img, int e, float* o, unsigned long long P, uint32_t g, bool fixed) {
  const unsigned long long key = a.seed ^ (P >> 32 << 32);
  bool flip = false;
  if (a.hflip && !fixed) {
    uint32_t f[4];
    philox4(0ull, g, (uint32_t)P, key ^ LVAE_AUG_TAG_FLIP, f);
    flip = (f[0] >> 31) != 0;
  }
  float u[4] = {0.f, 0.f, 0.f, 0.f};
  if (a.mode != LVAE_AUG_NONE) {   // one block per four outputs; the draw belongs to the output element, flipped or not
    uint32_t w[4];
    philox4((uint64_t)(e >> 2), g, (uint32_t)P, key ^ (fixed ? LVAE_AUG_TAG_FIXED : LVAE_AUG_TAG_PIXEL), w);
    for (int k = 0; k < 4; ++k) u[k] = u01(w[k]);
  }
  if (a.vec) {   // as the plain gather's, and W is a multiple of 4 when rows may flip: the four sources are one aligned group, read mirrored
    const int c = e / a.HW;
    int hw = e - c * a.HW;
    if (flip) {
      const int h = hw / a.W, w = hw - h * a.W;
      hw = h * a.W + (a.W - 4 - w);
    }
    f32x4 v;
    if (a.f32) {
      const f32x4 s = *reinterpret_cast<const f32x4*>(static_cast<const float*>(a.src) + img * a.chw + (size_t)c * a.HW + hw);
      v = flip ? f32x4{aug_f32(a, s.w, u[0]), aug_f32(a, s.z, u[1]), aug_f32(a, s.y, u[2]), aug_f32(a, s.x, u[3])}
               : f32x4{aug_f32(a, s.x, u[0]), aug_f32(a, s.y, u[1]), aug_f32(a, s.z, u[2]), aug_f32(a, s.w, u[3])};
    } else {
      uint32_t w;
      if (!a.hwc) {
        w = *reinterpret_cast<const uint32_t*>(static_cast<const unsigned char*>(a.src) + img * a.chw + (size_t)c * a.HW + hw);
      } else {
        const unsigned char* s = static_cast<const unsigned char*>(a.src) + img * a.chw + (size_t)hw * a.C + c;
        w = (uint32_t)s[0] | (uint32_t)s[a.C] << 8 | (uint32_t)s[2 * a.C] << 16 | (uint32_t)s[3 * a.C] << 24;
      }
      if (flip) w = __builtin_bswap32(w);
      v = f32x4{aug_u8(a, w & 255u, u[0]), aug_u8(a, (w >> 8) & 255u, u[1]), aug_u8(a, (w >> 16) & 255u, u[2]), aug_u8(a, w >> 24, u[3])};
    }
    *reinterpret_cast<f32x4*>(o) = v;
  } else {
    for (int k = 0; k < 4 && e + k < a.chw; ++k) {
      const int c = (e + k) / a.HW;
      int hw = (e + k) - c * a.HW;
      if (flip) {
        const int h = hw / a.W;
        hw = h * a.W + (a.W - 1 - (hw - h * a.W));
      }
      const size_t off = img * a.chw + (a.hwc ? (size_t)hw * a.C + c : (size_t)c * a.HW + hw);
      o[k] = a.f32 ? aug_f32(a, static_cast<const float*>(a.src)[off], u[k]) : aug_u8(a, static_cast<const unsigned char*>(a.src)[off], u[k]);
    }
  }
}

// A = FeedArgs: the plain gather. A = AugFeedArgs: the augmenting one.
template <class A>
__global__ __launch_bounds__(256) void batch_gather_kernel(A a) {
  const int qpr = (a.chw + 3) >> 2;   // threads per output row
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)a.n_rows * qpr) return;
  const int r = (int)(i / qpr), e = (int)(i - (long long)r * qpr) << 2;
  long long img;
  unsigned long long done = 0ull;
  if (a.index != nullptr) {
    done = a.cursor != nullptr ? (unsigned long long)a.cursor[0] : feed_position(a);
    const long long p = (long long)(done % (unsigned)a.steps_per_epoch) * a.B_global + a.lo + r;   // < steps_per_epoch * B_global
    img = a.index[p];
  } else {
    img = a.base + r;
  }
  float* o = a.out + (size_t)r * a.chw + e;
  if (img < 0 || img >= a.N) {
    // an index outside the table never becomes an address: the row is NaN, which no loss survives unnoticed
    const float nan = __int_as_float(0x7fc00000);
    for (int k = 0; k < 4 && e + k < a.chw; ++k) o[k] = nan;
    return;
  }
  if constexpr (A::aug) {
    const bool fixed = a.fixed != 0 || a.index == nullptr;
    gather_aug(a, (size_t)img, e, o, fixed ? 0ull : done, fixed ? (uint32_t)img : (uint32_t)(a.lo + r), fixed);
    return;
  }
  if (a.vec) {   // chw (and, for HWC, H*W) is a multiple of 4: the four elements share a channel, the store is 16-byte aligned
    f32x4 v;
    if (a.f32) {
      v = *reinterpret_cast<const f32x4*>(static_cast<const float*>(a.src) + (size_t)img * a.chw + e);
    } else if (!a.hwc) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(static_cast<const unsigned char*>(a.src) + (size_t)img * a.chw + e);
      v = f32x4{byte_to_unit(w & 255u), byte_to_unit((w >> 8) & 255u), byte_to_unit((w >> 16) & 255u), byte_to_unit(w >> 24)};
    } else {
      // four pixels of one channel, C bytes apart; the threads of the other channels read the same cache lines
      const int c = e / a.HW, hw = e - c * a.HW;
      const unsigned char* s = static_cast<const unsigned char*>(a.src) + (size_t)img * a.chw + (size_t)hw * a.C + c;
      v = f32x4{byte_to_unit(s[0]), byte_to_unit(s[a.C]), byte_to_unit(s[2 * a.C]), byte_to_unit(s[3 * a.C])};
    }
    *reinterpret_cast<f32x4*>(o) = v;
  } else {       // rows are not 16-byte aligned: element by element, the last thread of a row stops at its end
    for (int k = 0; k < 4 && e + k < a.chw; ++k) o[k] = feed_elem(a, (size_t)img, e + k);
  }
}

}  // namespace lvae

using namespace lvae;

// Checks the arguments both entry points share and fills `a` (`vec` as the plain gather takes it). `name`: the entry point, for messages.
static int feed_args(FeedArgs& a, const char* name, const void* src, int32_t src_kind, int32_t src_hwc, int32_t N, int32_t C, int32_t H,
                     int32_t W, const int32_t* index, const int64_t* cursor, int32_t steps_per_epoch, int32_t B_global, int32_t lo,
                     int64_t base, int32_t n_rows, float* out) {
  LVAE_REQUIRE(src && out && N > 0 && C > 0 && H > 0 && W > 0 && n_rows > 0, LVAE_EINVAL, "%s: bad args", name);
  LVAE_REQUIRE((src_kind == LVAE_FEED_U8 || src_kind == LVAE_FEED_F32) && (src_hwc == 0 || src_hwc == 1) &&
                   !(src_kind == LVAE_FEED_F32 && src_hwc),
               LVAE_EINVAL, "%s: source kind %d / layout %d not supported (uint8 CHW or HWC, float32 CHW)", name, (int)src_kind,
               (int)src_hwc);
  const long long chw = (long long)C * H * W;
  LVAE_REQUIRE(chw <= (1 << 28), LVAE_EINVAL, "%s: image of %lld values", name, chw);
  if (index != nullptr) {
    LVAE_REQUIRE(steps_per_epoch > 0 && B_global > 0 && lo >= 0 && (long long)lo + n_rows <= B_global && base == 0 &&
                     (long long)steps_per_epoch * B_global <= INT32_MAX,
                 LVAE_EINVAL, "%s: rows [%d, %lld) outside a global batch of %d, or no epoch length", name, (int)lo,
                 (long long)lo + n_rows, (int)B_global);
  } else {
    LVAE_REQUIRE(cursor == nullptr && base >= 0 && base + n_rows <= N, LVAE_EINVAL,
                 "%s: without an index table images [%lld, %lld) of %d are taken in order, and no cursor is read", name,
                 (long long)base, (long long)base + n_rows, (int)N);
  }
  LVAE_REQUIRE(al16(out) && (src_kind == LVAE_FEED_F32 ? al16(src) : (reinterpret_cast<uintptr_t>(src) & 3) == 0), LVAE_EINVAL,
               "%s: misaligned buffer", name);
  a.src = src, a.index = index, a.cursor = cursor, a.out = out, a.base = base;
  a.N = N, a.C = C, a.HW = H * W, a.chw = (int)chw;
  a.steps_per_epoch = steps_per_epoch, a.B_global = B_global, a.lo = lo, a.n_rows = n_rows;
  a.f32 = src_kind == LVAE_FEED_F32, a.hwc = src_hwc;
  a.vec = (chw % 4 == 0) && (!src_hwc || a.HW % 4 == 0);
  const long long threads = (long long)n_rows * ((chw + 3) / 4);
  LVAE_REQUIRE((threads + 255) / 256 <= INT32_MAX, LVAE_EINVAL, "%s: batch too large for one launch", name);
  return 0;
}

static unsigned feed_blocks(const FeedArgs& a) { return (unsigned)(((long long)a.n_rows * ((a.chw + 3) / 4) + 255) / 256); }

extern "C" int lvae_batch_gather_f32(const void* src, int32_t src_kind, int32_t src_hwc, int32_t N, int32_t C, int32_t H, int32_t W,
                                     const int32_t* index, const int64_t* cursor, int32_t steps_per_epoch, int32_t B_global, int32_t lo,
                                     int64_t base, int32_t n_rows, float* out, void* stream) {
  FeedArgs a;
  const int rc = feed_args(a, "lvae_batch_gather_f32", src, src_kind, src_hwc, N, C, H, W, index, cursor, steps_per_epoch, B_global, lo,
                           base, n_rows, out);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(batch_gather_kernel<FeedArgs>, dim3(feed_blocks(a)), dim3(256), 0, (hipStream_t)stream, a);
  LVAE_LAUNCH_CHECK("batch_gather");
  return 0;
}

extern "C" int lvae_batch_gather_aug_f32(const void* src, int32_t src_kind, int32_t src_hwc, int32_t N, int32_t C, int32_t H, int32_t W,
                                         const int32_t* index, const int64_t* cursor, int32_t steps_per_epoch, int32_t B_global,
                                         int32_t lo, int64_t base, int32_t n_rows, float* out, const lvae_feed_aug* aug, void* stream) {
  AugFeedArgs a;
  const int rc = feed_args(a, "lvae_batch_gather_aug_f32", src, src_kind, src_hwc, N, C, H, W, index, cursor, steps_per_epoch, B_global,
                           lo, base, n_rows, out);
  if (rc != 0) return rc;
  LVAE_REQUIRE(aug != nullptr && aug->position >= 0 &&
                   (aug->mode == LVAE_AUG_NONE || aug->mode == LVAE_AUG_BINARIZE || aug->mode == LVAE_AUG_DEQUANTIZE),
               LVAE_EINVAL, "lvae_batch_gather_aug_f32: no lvae_feed_aug, a negative position or an unknown mode");
  LVAE_REQUIRE(!(aug->mode == LVAE_AUG_DEQUANTIZE && src_kind == LVAE_FEED_F32), LVAE_EINVAL,
               "lvae_batch_gather_aug_f32: dequantization adds noise below one step of an 8-bit value: the table must be uint8");
  a.seed = aug->seed, a.position = (unsigned long long)aug->position;
  a.mode = aug->mode, a.hflip = aug->hflip != 0, a.fixed = aug->fixed != 0, a.W = W;
  const bool may_flip = a.hflip && !a.fixed && index != nullptr;
  a.vec = a.vec && (!may_flip || W % 4 == 0);   // a mirrored group of four must be one aligned group of the source row
  hipLaunchKernelGGL(batch_gather_kernel<AugFeedArgs>, dim3(feed_blocks(a)), dim3(256), 0, (hipStream_t)stream, a);
  LVAE_LAUNCH_CHECK("batch_gather_aug");
  return 0;
}
