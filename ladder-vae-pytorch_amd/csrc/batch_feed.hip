// The training batch formed on the device: rows of an image table in HBM, chosen through an index table in HBM at a position read from
// a device step counter, written as the float32 NCHW batch LadderVAE.forward takes. One launch inside the captured step replaces the host
// collate, the pageable host-to-device copy and the copy into the graph's input buffer. Small (a CIFAR batch of 256 reads 0.8 MB and
// writes 3 MB) and launch-latency sized: one thread per four output floats, plain loads, one 16-byte store, no LDS.
#include "lvae_common.h"

namespace lvae {

struct FeedArgs {
  const void* src;            // [N] images, uint8 or float32, each CHW or HWC contiguous
  const int32_t* index;       // [steps_per_epoch * B_global] image numbers, or null: images base, base + 1, ...
  const int64_t* cursor;      // [1] completed steps, or null: position 0
  float* out;                 // [n_rows][C][H][W]
  long long base;
  int N, C, HW, chw;
  int steps_per_epoch, B_global, lo, n_rows;
  int f32, hwc, vec;
};

// Element e (CHW order) of image `img`, from either layout and either storage type.
__device__ __forceinline__ float feed_elem(const FeedArgs& a, size_t img, int e) {
  const int c = e / a.HW, hw = e - c * a.HW;
  const size_t off = img * (size_t)a.chw + (a.hwc ? (size_t)hw * a.C + c : (size_t)e);
  return a.f32 ? static_cast<const float*>(a.src)[off] : byte_to_unit(static_cast<const unsigned char*>(a.src)[off]);
}

__global__ __launch_bounds__(256) void batch_gather_kernel(FeedArgs a) {
  const int qpr = (a.chw + 3) >> 2;   // threads per output row
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)a.n_rows * qpr) return;
  const int r = (int)(i / qpr), e = (int)(i - (long long)r * qpr) << 2;
  long long img;
  if (a.index != nullptr) {
    const unsigned long long done = a.cursor != nullptr ? (unsigned long long)a.cursor[0] : 0ull;
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

extern "C" int lvae_batch_gather_f32(const void* src, int32_t src_kind, int32_t src_hwc, int32_t N, int32_t C, int32_t H, int32_t W,
                                     const int32_t* index, const int64_t* cursor, int32_t steps_per_epoch, int32_t B_global, int32_t lo,
                                     int64_t base, int32_t n_rows, float* out, void* stream) {
  LVAE_REQUIRE(src && out && N > 0 && C > 0 && H > 0 && W > 0 && n_rows > 0, LVAE_EINVAL, "lvae_batch_gather_f32: bad args");
  LVAE_REQUIRE((src_kind == LVAE_FEED_U8 || src_kind == LVAE_FEED_F32) && (src_hwc == 0 || src_hwc == 1) &&
                   !(src_kind == LVAE_FEED_F32 && src_hwc),
               LVAE_EINVAL, "lvae_batch_gather_f32: source kind %d / layout %d not supported (uint8 CHW or HWC, float32 CHW)",
               (int)src_kind, (int)src_hwc);
  const long long chw = (long long)C * H * W;
  LVAE_REQUIRE(chw <= (1 << 28), LVAE_EINVAL, "lvae_batch_gather_f32: image of %lld values", chw);
  if (index != nullptr) {
    LVAE_REQUIRE(steps_per_epoch > 0 && B_global > 0 && lo >= 0 && (long long)lo + n_rows <= B_global && base == 0 &&
                     (long long)steps_per_epoch * B_global <= INT32_MAX,
                 LVAE_EINVAL, "lvae_batch_gather_f32: rows [%d, %lld) outside a global batch of %d, or no epoch length", (int)lo,
                 (long long)lo + n_rows, (int)B_global);
  } else {
    LVAE_REQUIRE(cursor == nullptr && base >= 0 && base + n_rows <= N, LVAE_EINVAL,
                 "lvae_batch_gather_f32: without an index table images [%lld, %lld) of %d are taken in order, and no cursor is read",
                 (long long)base, (long long)base + n_rows, (int)N);
  }
  LVAE_REQUIRE(al16(out) && (src_kind == LVAE_FEED_F32 ? al16(src) : (reinterpret_cast<uintptr_t>(src) & 3) == 0), LVAE_EINVAL,
               "lvae_batch_gather_f32: misaligned buffer");
  FeedArgs a;
  a.src = src, a.index = index, a.cursor = cursor, a.out = out, a.base = base;
  a.N = N, a.C = C, a.HW = H * W, a.chw = (int)chw;
  a.steps_per_epoch = steps_per_epoch, a.B_global = B_global, a.lo = lo, a.n_rows = n_rows;
  a.f32 = src_kind == LVAE_FEED_F32, a.hwc = src_hwc;
  a.vec = (chw % 4 == 0) && (!src_hwc || a.HW % 4 == 0);
  const long long threads = (long long)n_rows * ((chw + 3) / 4);
  LVAE_REQUIRE((threads + 255) / 256 <= INT32_MAX, LVAE_EINVAL, "lvae_batch_gather_f32: batch too large for one launch");
  hipLaunchKernelGGL(batch_gather_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  LVAE_LAUNCH_CHECK("batch_gather");
  return 0;
}
