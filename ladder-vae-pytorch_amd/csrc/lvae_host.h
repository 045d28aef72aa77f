// Host-side interface between the .hip files of liblvae_hip: every host function that one file defines and another calls, the structs
// that cross files, and the launcher of kernels with more than 64 KB of LDS. Declared here once; both the defining file and every
// caller include this header, so a changed signature is a compile error and a missing definition a link error (-Wl,--no-undefined).
#pragma once
#include "lvae_common.h"

namespace lvae {

// One forward / dgrad kernel family's accepted choice for a convolution descriptor. A family's *_plan() fills it and returns false
// when the family does not take the descriptor (every condition its launch depends on: buffer alignment, workspace, tile, LDS);
// its *_launch() runs exactly that choice and can no longer decline. The route of lvae_conv2d_* (conv_igemm.hip) walks the plans once;
// the 1x1 gate / concat-dgrad entry points (conv1x1.hip, conv1x1_gate_bwd_fused.hip) and their queries ask theirs the same way.
struct ConvPlan {
  int32_t variant = LVAE_VARIANT_DIRECT;  // LVAE_VARIANT_*
  int32_t rows = 0;                       // rows of statistics partials the launch writes (0: no statistics epilogue)
  bool folds = false;                     // folds the BatchNorm finalize of its input (lvae_bn_fold)
  size_t workspace = 0;                   // bytes of workspace the launch needs (pre-transformed weights, weight-gradient slabs)
};

// One problem of the grouped fixed-order slab reduce (wgrad_reduce_grouped_launch): ksplit slabs of [ntaps][Cin][Cout] (+ [Cout])
// summed into the strided dw (+ db).
struct ReduceArgs {
  const float* slab_w;
  const float* slab_b;
  int ksplit, ntaps, Cin, Cout;
  int64_t stap, sk, sn;
  float* dw;
  float* db;
};
constexpr int kMaxReduceGroup = 12;  // problems per wgrad_reduce_grouped_launch

// conv_igemm.hip
int conv_desc_check(const lvae_conv_desc* d, const char* who);

// conv3x3_halo.hip
bool conv3x3_halo_plan(const lvae_conv_desc* d, ConvPlan& p);
int conv3x3_halo_launch(const lvae_conv_desc* d, hipStream_t s);

// conv3x3_pos.hip
bool conv3x3_pos_plan(const lvae_conv_desc* d, ConvPlan& p);
int conv3x3_pos_launch(const lvae_conv_desc* d, hipStream_t s);

// conv3x3_wino.hip
bool conv3x3_wino_plan(const lvae_conv_desc* d, bool assume_ws, ConvPlan& p);
int conv3x3_wino_launch(const lvae_conv_desc* d, hipStream_t s);
int conv3x3_wino2_gate_rows(const lvae_conv_desc* d);
int conv3x3_wino2_gate_launch(const lvae_conv_desc* d, const lvae_rb_ext* gate, hipStream_t s);

// conv3x3_bf16.hip
int conv3x3_bf16_form(const lvae_conv_desc* d);
bool conv3x3_bf16_plan(const lvae_conv_desc* d, bool assume_ws, ConvPlan& p);
int conv3x3_bf16_launch(const lvae_conv_desc* d, const ConvPlan& p, hipStream_t s);
size_t conv3x3_bf16_workspace(const lvae_conv_desc* d, int split);
void conv3x3_bf16_prep_entry(const lvae_conv_desc* d, int split, void* entry);
int conv3x3_bf16_prepare_single(const lvae_conv_desc* d, int split, hipStream_t s);
int conv3x3_bf16_prepare_batched(const void* entries, int n, int npad, hipStream_t s);
size_t resblock_gate_ws_bytes(const lvae_conv_desc* d, int planes);
void resblock_gate_prep_entry(const lvae_conv_desc* d, int planes, void* entry);
int resblock_gate_prepare_single(const lvae_conv_desc* d, int planes, hipStream_t s);
size_t conv3x3_wgrad_bf16_workspace(const lvae_conv_desc* d);
int conv3x3_wgrad_bf16_launch(const lvae_conv_desc* d, const float* dy, float* dw, float* db, void* workspace, hipStream_t s);

// conv1x1.hip: the single-shot kernel. PwForm says which form of it a launch is and carries that form's operands outside the descriptor
// (the plan reads kind and split only: it assumes those operands 16-byte aligned, the entry points check them).
enum { PW_PLAIN, PW_GATE_FWD, PW_GATE_BWD, PW_DGRAD_CAT };
struct PwForm {
  int kind = PW_PLAIN;
  int act = 0;                               // PW_GATE_FWD / PW_GATE_BWD: LVAE_ACT_* of the gate
  const float* res = nullptr;                // PW_GATE_FWD: residual [M][C] or null, out [M][C]
  float* out = nullptr;
  const float* dout = nullptr;               // PW_GATE_BWD: dout [M][C], ab [M][2C], dab [M][2C] or null
  const float* ab = nullptr;
  float* dab = nullptr;
  float* y2 = nullptr;                       // PW_DGRAD_CAT: columns [split, Cout) go to y2
  int split = 0;
};
bool conv1x1_plan(const lvae_conv_desc* d, const PwForm& f, ConvPlan& p);  // p.rows: PW_GATE_FWD only
int conv1x1_launch(const lvae_conv_desc* d, const PwForm& f, hipStream_t s);

// conv1x1_gate_fwd.hip: the persistent gate forward of the 64-channel blocks (p.rows = its workgroups)
bool conv1x1_gate_fwd_plan(const lvae_conv_desc* d, ConvPlan& p);
int conv1x1_gate_fwd_launch(const lvae_conv_desc* d, const ConvPlan& p, const float* res, float* out, int act, hipStream_t s);

// conv1x1_gate_bwd_fused.hip: the persistent gate backward (p.workspace = its slabs); with_apply: with a deferred lvae_bn_apply
bool conv1x1_gate_bwd_fused_plan(const lvae_conv_desc* d, bool with_apply, ConvPlan& p);

// conv_wgrad.hip
void wgrad_reduce_launch(const float* slab_w, const float* slab_b, int ksplit, int ntaps, int Cin, int Cout, int64_t stap,
                         int64_t sk, int64_t sn, float* dw, float* db, hipStream_t s);
void wgrad_reduce_grouped_launch(const ReduceArgs* r, int n, hipStream_t s);

// conv_wgrad_img.hip: whole-image tiles of the <= 8x8 levels on the bf16 matrix pipe, up to 32 gradients per launch
size_t conv_wgrad_img_workspace(const lvae_conv_desc* d);
int conv_wgrad_img_kind(const lvae_conv_desc* d);
int conv_wgrad_img_grouped(const lvae_conv_desc* const* ds, const float* const* dy, float* const* dw, float* const* db,
                           void* const* workspace, int n, int kind, hipStream_t s);
int conv_wgrad_img_launch(const lvae_conv_desc* d, const float* dy, float* dw, float* db, void* workspace, hipStream_t s);

// conv3x3_wgrad_halo.hip
size_t conv_wgrad_tile_workspace(const lvae_conv_desc* d);
int conv_wgrad_tile_kind(const lvae_conv_desc* d);
int conv_wgrad_tile_grouped(const lvae_conv_desc* const* ds, const float* const* dy, float* const* dw, float* const* db,
                            void* const* workspace, int n, int kind, hipStream_t s);
int conv_wgrad_tile_launch(const lvae_conv_desc* d, const float* dy, float* dw, float* db, void* workspace, hipStream_t s);

// conv3x3_wgrad_wino.hip
size_t conv_wgrad_wino_workspace(const lvae_conv_desc* d);
int conv_wgrad_wino_grouped(const lvae_conv_desc* const* ds, const float* const* dy, float* const* dw, float* const* db,
                            void* const* workspace, int n, hipStream_t s);
int conv_wgrad_wino_launch(const lvae_conv_desc* d, const float* dy, float* dw, float* db, void* workspace, hipStream_t s);
bool conv_wgrad_wino_apply_ok(const lvae_conv_desc* d);
int conv_wgrad_wino_apply_launch(const lvae_conv_desc* d, const lvae_bn_apply* ap, float* dw, float* db, void* workspace, hipStream_t s);

// conv1x1_wgrad.hip
size_t conv1x1_wgrad_workspace(const lvae_conv_desc* d);
int conv1x1_wgrad_launch(const lvae_conv_desc* d, const float* dy, float* dw, float* db, void* workspace, hipStream_t s);

// Launch of a kernel whose dynamic LDS may exceed the 64 KB default: raises the kernel's limit to max_lds the first time THIS kernel is
// launched (one flag per kernel: the template argument), launches, checks. name: as it appears in lvae_last_error().
template <auto Kern, typename Args>
int launch_lds(const char* name, dim3 grid, dim3 block, size_t lds, int max_lds, hipStream_t s, const Args& a) {
  static std::atomic<bool> attr_set{false};  // idempotent attribute write; the flag itself is race-free
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
    if (e != hipSuccess) {
      set_error("%s: hipFuncSetAttribute failed: %s", name, hipGetErrorString(e));
      return (int)e;
    }
    attr_set = true;
  }
  hipLaunchKernelGGL(Kern, grid, block, lds, s, a);
  LVAE_LAUNCH_CHECK(name);
  return 0;
}

}  // namespace lvae
