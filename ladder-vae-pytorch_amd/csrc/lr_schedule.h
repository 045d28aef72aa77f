// The learning-rate schedule of lvae_lr_schedule (include/lvae_hip.h), written once: lvae_lr_schedule_at evaluates it on the host and the
// scheduled Adamax kernel on the device, both from this text. Everything in double from the exact integer counter, rounded to float once
// (the idiom of anneal_beta in misc.hip; the library is built with -ffp-contract=off, so host and device round the same products).
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/lvae_hip.h"

namespace lvae {

// lr of the step that follows `n` completed ones. `s` has passed lr_schedule_valid: base_lr > 0, 0 <= min_lr <= base_lr, 0 < gamma <= 1,
// warmup_steps >= 0, decay_steps > 0 unless the kind is constant.
__host__ __device__ inline float lr_schedule_eval(const lvae_lr_schedule& s, uint64_t n) {
  const double base = (double)s.base_lr;
  const uint64_t W = (uint64_t)s.warmup_steps;
  if (n < W) return (float)(base * (double)(n + 1) / (double)W);   // the first step is not zero, step W - 1 reaches base
  if (s.kind == LVAE_LR_CONSTANT) return s.base_lr;
  const uint64_t t = n - W, T = (uint64_t)s.decay_steps;
  const double m = (double)s.min_lr / base;
  const double r = (double)(t < T ? t : T) / (double)T;            // min(t, T) / T
  double f;
  switch (s.kind) {
    case LVAE_LR_COSINE: f = m + (1.0 - m) * 0.5 * (1.0 + cos(M_PI * r)); break;
    case LVAE_LR_LINEAR: f = 1.0 - (1.0 - m) * r; break;
    case LVAE_LR_STEP:   f = fmax(m, pow((double)s.gamma, (double)(t / T))); break;
    default:             f = fmax(m, pow((double)s.gamma, (double)t / (double)T)); break;   // LVAE_LR_EXP
  }
  return (float)(base * f);
}

}  // namespace lvae
