// Training-log summaries (boilr's summarizer: the mean of every step's metrics since the last log line) kept on the device. Each step
// folds its fp32 scalars into a small double accumulator with ONE launch of one wave, inside the captured step; a log line takes the
// accumulator (copy out and clear) once. Every value is widened to double exactly and added to its own slot by the one thread that owns
// the slot, so a window's sum is the sequential float64 sum of the per-step float32 values in step order, whatever the launch mode.
// A step accumulated over M micro-passes keeps the means of its metrics the same way (micro_fold_kernel): one wave per micro-pass, the
// M-th of which writes the means and clears the accumulator.
#include "lvae_common.h"

namespace lvae {

constexpr int kSummaryFixed = 8;    // [steps folded, non-finite steps, loss, elbo, recons, kl, l2, grad]
constexpr int kSummaryMaxL = 64;

// acc (double) [8 + L]. Thread i owns slot i (with L > 56 also slot i + 64) and no other: plain loads, plain stores, nothing shared.
// A step whose loss or grad value is not finite is counted in slot 1 and adds to no other slot; every thread decides that from its own
// read of the two values.
__global__ __launch_bounds__(64) void summary_fold_kernel(const float* __restrict__ loss, const float* __restrict__ elbo,
                                                          const float* __restrict__ recons, const float* __restrict__ kl,
                                                          const float* __restrict__ l2, const float* __restrict__ grad_norm,
                                                          const float* __restrict__ gscale, const float* __restrict__ kl_layers, int L,
                                                          double* __restrict__ acc) {
  const float lv = loss[0];
  float gv = 0.f;
  if (grad_norm) gv = gscale ? grad_norm[0] * gscale[0] : grad_norm[0];   // fp32 product: the norm of the gradient Adamax applies
  const bool bad = !(isfinite(lv) && isfinite(gv));
  for (int s = threadIdx.x; s < kSummaryFixed + L; s += 64) {
    if (bad ? s != 1 : s == 1) continue;   // a bad step touches slot 1 alone; a good one every slot but slot 1
    double add;
    switch (s) {
      case 0: case 1: add = 1.0; break;
      case 2: add = (double)lv; break;
      case 3: add = (double)elbo[0]; break;
      case 4: add = (double)recons[0]; break;
      case 5: add = (double)kl[0]; break;
      case 6: add = (double)l2[0]; break;
      case 7: add = (double)gv; break;
      default: add = (double)kl_layers[s - kSummaryFixed]; break;
    }
    acc[s] = acc[s] + add;
  }
}

__global__ __launch_bounds__(64) void summary_take_kernel(double* __restrict__ acc, int n, double* __restrict__ out) {
  for (int s = threadIdx.x; s < n; s += 64) {
    out[s] = acc[s];
    acc[s] = 0.0;
  }
}

constexpr int kMicroFixed = 7;      // [loss, elbo, recons, kl, l2, iw, ess]

// One micro-pass of an accumulated step: acc (double) [7 + L] += this pass's fp32 scalars, count[0] += 1; on the M-th call
// out[s] = (float)(acc[s] / M), acc[s] = 0 and count[0] = 0. Thread i owns slot i (with L > 57 also slot i + 64) of acc and out and no
// other. Every thread reads the pass counter before the barrier and thread 0 alone writes it after, so all of them decide alike.
__global__ __launch_bounds__(64) void micro_fold_kernel(const float* __restrict__ loss, const float* __restrict__ elbo,
                                                        const float* __restrict__ recons, const float* __restrict__ kl,
                                                        const float* __restrict__ l2, const float* __restrict__ iw,
                                                        const float* __restrict__ ess, const float* __restrict__ kl_layers, int L, int M,
                                                        double* __restrict__ acc, long long* __restrict__ count, float* __restrict__ out) {
  const long long pass = count[0] + 1;
  const bool last = pass >= (long long)M;
  __syncthreads();
  for (int s = threadIdx.x; s < kMicroFixed + L; s += 64) {
    float v;
    switch (s) {
      case 0: v = loss[0]; break;
      case 1: v = elbo[0]; break;
      case 2: v = recons[0]; break;
      case 3: v = kl[0]; break;
      case 4: v = l2[0]; break;
      case 5: v = iw ? iw[0] : 0.f; break;
      case 6: v = ess ? ess[0] : 0.f; break;
      default: v = kl_layers[s - kMicroFixed]; break;
    }
    const double a = acc[s] + (double)v;
    if (last) {
      out[s] = (float)(a / (double)M);
      acc[s] = 0.0;
    } else {
      acc[s] = a;
    }
  }
  if (threadIdx.x == 0) count[0] = last ? 0 : pass;
}

inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
inline bool al8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace lvae

using namespace lvae;

extern "C" int lvae_summary_fold_f64(const float* loss, const float* elbo, const float* recons, const float* kl, const float* l2,
                                     const float* grad_norm, const float* gscale, const float* kl_layers, int32_t L, double* acc,
                                     void* stream) {
  LVAE_REQUIRE(loss && elbo && recons && kl && l2 && acc, LVAE_EINVAL, "lvae_summary_fold_f64: null scalar or accumulator");
  LVAE_REQUIRE(L >= 0 && L <= kSummaryMaxL, LVAE_EINVAL, "lvae_summary_fold_f64: L = %d outside [0, %d]", (int)L, kSummaryMaxL);
  LVAE_REQUIRE(L == 0 || kl_layers, LVAE_EINVAL, "lvae_summary_fold_f64: kl_layers missing for L = %d", (int)L);
  LVAE_REQUIRE(grad_norm || !gscale, LVAE_EINVAL, "lvae_summary_fold_f64: gscale without grad_norm");
  LVAE_REQUIRE(al4(loss) && al4(elbo) && al4(recons) && al4(kl) && al4(l2) && al4(grad_norm) && al4(gscale) && al4(kl_layers),
               LVAE_EALIGN, "lvae_summary_fold_f64: a float pointer is not 4-byte aligned");
  LVAE_REQUIRE(al8(acc), LVAE_EALIGN, "lvae_summary_fold_f64: the accumulator is not 8-byte aligned");
  hipLaunchKernelGGL(summary_fold_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, loss, elbo, recons, kl, l2, grad_norm, gscale,
                     kl_layers, (int)L, acc);
  LVAE_LAUNCH_CHECK("summary_fold");
  return 0;
}

extern "C" int lvae_summary_take_f64(double* acc, int32_t n, double* out, void* stream) {
  LVAE_REQUIRE(acc && out && acc != out, LVAE_EINVAL, "lvae_summary_take_f64: null or aliased buffers");
  LVAE_REQUIRE(n > 0 && n <= kSummaryFixed + kSummaryMaxL, LVAE_EINVAL, "lvae_summary_take_f64: n = %d outside [1, %d]", (int)n,
               kSummaryFixed + kSummaryMaxL);
  LVAE_REQUIRE(al8(acc) && al8(out), LVAE_EALIGN, "lvae_summary_take_f64: a buffer is not 8-byte aligned");
  hipLaunchKernelGGL(summary_take_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, acc, (int)n, out);
  LVAE_LAUNCH_CHECK("summary_take");
  return 0;
}

extern "C" int lvae_micro_fold_f64(const float* loss, const float* elbo, const float* recons, const float* kl, const float* l2,
                                   const float* iw, const float* ess, const float* kl_layers, int32_t L, int32_t M, double* acc,
                                   int64_t* count, float* out, void* stream) {
  LVAE_REQUIRE(M >= 1, LVAE_EINVAL, "lvae_micro_fold_f64: M = %d micro-passes per step (at least 1)", (int)M);
  LVAE_REQUIRE(L >= 0 && L <= kSummaryMaxL, LVAE_EINVAL, "lvae_micro_fold_f64: L = %d outside [0, %d]", (int)L, kSummaryMaxL);
  LVAE_REQUIRE(loss && elbo && recons && kl && l2 && acc && count && out, LVAE_EINVAL,
               "lvae_micro_fold_f64: null scalar, accumulator, counter or output");
  LVAE_REQUIRE(L == 0 || kl_layers, LVAE_EINVAL, "lvae_micro_fold_f64: kl_layers missing for L = %d", (int)L);
  LVAE_REQUIRE(al4(loss) && al4(elbo) && al4(recons) && al4(kl) && al4(l2) && al4(iw) && al4(ess) && al4(kl_layers) && al4(out),
               LVAE_EALIGN, "lvae_micro_fold_f64: a float pointer is not 4-byte aligned");
  LVAE_REQUIRE(al8(acc) && al8(count), LVAE_EALIGN, "lvae_micro_fold_f64: the accumulator or the counter is not 8-byte aligned");
  hipLaunchKernelGGL(micro_fold_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, loss, elbo, recons, kl, l2, iw, ess, kl_layers, (int)L,
                     (int)M, acc, reinterpret_cast<long long*>(count), out);
  LVAE_LAUNCH_CHECK("micro_fold");
  return 0;
}
