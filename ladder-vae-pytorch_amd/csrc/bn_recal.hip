// BatchNorm recalibration: running statistics that belong to the weights being evaluated (torch.optim.swa_utils.update_bn's
// momentum=None rule). With momentum 1 a train-mode forward leaves every BatchNorm's batch mean and unbiased batch variance in its running
// statistics (bn_update_running of bn_stats.h: 0 * r0 + 1 * s); after each forward ONE launch adds them, widened to double exactly, to an
// accumulator, and after the last forward ONE launch writes their equal-weight mean back. Every element of every entry is owned by one
// thread, which adds in launch order with plain loads and stores: the result is the sequential float64 sum of the per-batch float32
// values, whatever the grid, eager or replayed. A statistic that no forward rewrote adds the same float n times; the sum n * v and the
// quotient by n are exact in double, so it comes back bit for bit and the table may hold every BatchNorm of a model.
#include "lvae_common.h"

namespace lvae {

// workgroup e adds entry e; thread 0 of workgroup 0 counts the fold (nobody reads the count inside this launch)
__global__ __launch_bounds__(256) void bn_recal_fold_kernel(const lvae_bn_recal_entry* __restrict__ table, long long* __restrict__ count) {
  const lvae_bn_recal_entry en = table[blockIdx.x];
  for (int64_t i = threadIdx.x; i < en.n; i += 256) en.acc[i] = en.acc[i] + (double)en.stat[i];
  if (blockIdx.x == 0 && threadIdx.x == 0) count[0] = count[0] + 1;
}

// workgroup e finishes entry e with the number of folds read on the device. count[0] is cleared by the workgroup that arrives last at
// count[1] (an integer ticket, left at 0 again): every workgroup takes its ticket after its read of count[0] has returned (the value has
// gone through LDS by then), so the clearing store follows every read. Nothing waits on anything: no workgroup polls.
__global__ __launch_bounds__(256) void bn_recal_finish_kernel(const lvae_bn_recal_entry* __restrict__ table, long long* count,
                                                              int32_t* __restrict__ flag) {
  __shared__ long long folds;
  if (threadIdx.x == 0) folds = __hip_atomic_load(count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const long long n = folds;
  const lvae_bn_recal_entry en = table[blockIdx.x];
  if (n > 0) {   // without a fold there is no mean: the statistics stay as they are (the accumulators are zero already)
    bool bad = false;
    for (int64_t i = threadIdx.x; i < en.n; i += 256) {
      const float v = (float)(en.acc[i] / (double)n);
      en.stat[i] = v;
      en.acc[i] = 0.0;
      bad |= !isfinite(v);
    }
    if (bad) flag[0] = 1;   // (every writer stores the same value)
  }
  if (threadIdx.x == 0) {
    const long long ticket = __hip_atomic_fetch_add(count + 1, 1LL, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket == (long long)gridDim.x - 1) {
      __hip_atomic_store(count, 0LL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(count + 1, 0LL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

static inline bool recal_al8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace lvae

using namespace lvae;

extern "C" int lvae_bn_recal_fold_f64(const lvae_bn_recal_entry* table, int32_t n_entries, int64_t* count, void* stream) {
  LVAE_REQUIRE(table && count && n_entries > 0, LVAE_EINVAL, "lvae_bn_recal_fold_f64: bad args");
  LVAE_REQUIRE(recal_al8(table) && recal_al8(count), LVAE_EALIGN, "lvae_bn_recal_fold_f64: misaligned table or count");
  hipLaunchKernelGGL(bn_recal_fold_kernel, dim3(n_entries), dim3(256), 0, (hipStream_t)stream, table, reinterpret_cast<long long*>(count));
  LVAE_LAUNCH_CHECK("bn_recal_fold");
  return 0;
}

extern "C" int lvae_bn_recal_finish_f32(const lvae_bn_recal_entry* table, int32_t n_entries, int64_t* count, int32_t* flag, void* stream) {
  LVAE_REQUIRE(table && count && flag && n_entries > 0, LVAE_EINVAL, "lvae_bn_recal_finish_f32: bad args");
  LVAE_REQUIRE(recal_al8(table) && recal_al8(count) && (reinterpret_cast<uintptr_t>(flag) & 3) == 0, LVAE_EALIGN,
               "lvae_bn_recal_finish_f32: misaligned table, count or flag");
  hipLaunchKernelGGL(bn_recal_finish_kernel, dim3(n_entries), dim3(256), 0, (hipStream_t)stream, table, reinterpret_cast<long long*>(count),
                     flag);
  LVAE_LAUNCH_CHECK("bn_recal_finish");
  return 0;
}
