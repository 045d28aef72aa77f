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

// One weight-gradient kernel family's accepted choice for a descriptor, by the rule of ConvPlan: <family>_plan() fills it and returns false
// when the family does not take the descriptor; the family's launches run that plan and cannot decline. The alignment a family needs from
// dy and the workspace stands in the table of the route (conv_wgrad.hip), which walks the plans once per gradient and sets `variant`.
struct WgradPlan {
  int32_t variant = LVAE_WGRAD_VARIANT_GENERIC;  // LVAE_WGRAD_VARIANT_*
  int32_t group = -1;                 // key inside the family: plans of equal (variant, group) may share one grouped launch; -1: never grouped
  int32_t slabs = 0;                  // partial slabs the launch writes (ksplit / workgroups / ranges)
  size_t w_floats = 0, b_floats = 0;  // one slab's weight part and its bias row: the workspace is [slabs][w_floats] then [slabs][b_floats]
  size_t workspace = 0;               // bytes
  bool takes_bf16_storage = false, apply_ok = false;  // bf16-stored x / dy accepted; deferred BatchNorm apply as dY accepted
  void set_slabs(int n, size_t w, size_t b) { slabs = n, w_floats = w, b_floats = b, workspace = (size_t)n * (w + b) * sizeof(float); }
};

// One gradient as a launch sees it: descriptor, routed plan, the operands outside the descriptor (db may be null)
struct WgradOp {
  const lvae_conv_desc* d;
  WgradPlan plan;
  const float* dy;
  float *dw, *db;
  void* workspace;
  float* slab_w() const { return static_cast<float*>(workspace); }
  float* slab_b() const { return db ? slab_w() + (size_t)plan.slabs * plan.w_floats : nullptr; }
};
// gradients per grouped launch of the families that have one: each sizes its family's p[] argument array and bounds the scheduler's groups
constexpr int kWgradTileGroup = 12, kWgradWinoGroup = 12, kWgradImgGroup = 32;

// conv_igemm.hip
int conv_desc_check(const lvae_conv_desc* d, const char* who);

// conv3x3_halo.hip
bool conv3x3_halo_plan(const lvae_conv_desc* d, ConvPlan& p);
int conv3x3_halo_launch(const lvae_conv_desc* d, hipStream_t s);

// conv3x3_pos.hip
bool conv3x3_pos_plan(const lvae_conv_desc* d, ConvPlan& p);
int conv3x3_pos_launch(const lvae_conv_desc* d, hipStream_t s);

// conv3x3_resample.hip: the stride-2 and transposed 3x3 convolutions, position-major (LVAE_VARIANT_DIRECT, no rows, no fold, no workspace)
bool conv3x3_resample_plan(const lvae_conv_desc* d, ConvPlan& p);
int conv3x3_resample_launch(const lvae_conv_desc* d, hipStream_t s);

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
bool conv3x3_wgrad_bf16_plan(const lvae_conv_desc* d, WgradPlan& p);
int conv3x3_wgrad_bf16_launch(const WgradOp& o, hipStream_t s);

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

// conv1x1_gate_bwd_fused.hip: the persistent gate backward (p.workspace = its slabs); with_apply: with a deferred lvae_bn_apply.
// (Its recompute form, lvae_conv1x1_gate_bwd_wgrad_recompute_*, adds conditions to this plan inside that file and fills the forward's gate
// planes through resblock_gate_prepare_single above: no declaration of its own here.)
bool conv1x1_gate_bwd_fused_plan(const lvae_conv_desc* d, bool with_apply, ConvPlan& p);

// conv_wgrad.hip
void wgrad_reduce_launch(const float* slab_w, const float* slab_b, int ksplit, int ntaps, int Cin, int Cout, int64_t stap,
                         int64_t sk, int64_t sn, float* dw, float* db, hipStream_t s);
void wgrad_reduce_grouped_launch(const ReduceArgs* r, int n, hipStream_t s);
int wgrad_op_reduce(const WgradOp& o, hipStream_t s);  // one gradient's slabs as its plan lays them out, launch checked

// conv_wgrad_img.hip: whole-image tiles of the <= 8x8 levels on the bf16 matrix pipe; a single gradient is a group of one
bool conv_wgrad_img_plan(const lvae_conv_desc* d, WgradPlan& p);
int conv_wgrad_img_grouped(const WgradOp* o, int n, hipStream_t s);

// conv3x3_wgrad_halo.hip
bool conv_wgrad_tile_plan(const lvae_conv_desc* d, WgradPlan& p);
int conv_wgrad_tile_launch(const WgradOp* o, int n, hipStream_t s);  // n = 1: the single kernel, else the grouped one

// conv3x3_wgrad_wino.hip (ap: the deferred BatchNorm-backward apply that forms dY, for a plan with apply_ok)
bool conv_wgrad_wino_plan(const lvae_conv_desc* d, WgradPlan& p);
int conv_wgrad_wino_launch(const WgradOp* o, int n, hipStream_t s);  // n = 1: the single kernel, else the grouped one
int conv_wgrad_wino_apply_launch(const WgradOp& o, const lvae_bn_apply* ap, hipStream_t s);
// The two gradients of a residual block as one launch pair (A: apply_ok, with ap in front; B: a real dy), for two routed Winograd plans of
// one geometry with 64 output channels: the plan re-splits the ranges between them (pa / pb: slabs and workspace of each; sched, if not
// null: ranges, chunks per range, workgroups of A, then of B), the launch runs that split.
bool conv_wgrad_wino_pair_plan(const lvae_conv_desc* da, const lvae_conv_desc* db, WgradPlan& pa, WgradPlan& pb, int32_t* sched);
int conv_wgrad_wino_pair_launch(const WgradOp& a, const lvae_bn_apply* ap, const WgradOp& b, hipStream_t s);
// n = 1 to 3 gradients with a real dy, shapes of the Winograd family of one image width with at most 64 output channels and 32 or 64 input
// channels (32: here only, conv_wgrad_wino_plan declines them), as one launch and one slab reduce: the plan splits the chip's workgroups between them (p[i]: slabs and workspace of each;
// sched, if not null: ranges, chunks per range, workgroups of each in turn), the launch runs that split.
constexpr int kWgradWinoShared = 3;
bool conv_wgrad_wino_shared_plan(const lvae_conv_desc* const* d, int n, WgradPlan* p, int32_t* sched);
int conv_wgrad_wino_shared_launch(const WgradOp* o, int n, hipStream_t s);

// conv1x1_wgrad.hip
bool conv1x1_wgrad_plan(const lvae_conv_desc* d, WgradPlan& p);
int conv1x1_wgrad_launch(const WgradOp& o, hipStream_t s);

// The one check of a lvae_bn_apply, for every entry point that takes one (`who`; resblock_img.hip passes views of its ap_* / bwd_* fields).
// M = N*H*W of the launch; `allows`: what this launch can do beside the plain apply. LVAE_EINVAL for what is missing or not allowed,
// then align_rc, naming the operand, for a pointer the kernels read or write 16 bytes at a time. Nothing is written. `name`: what the
// entry point's caller knows parts, coef, dh, x, add, out, drop as (resblock_img.hip's fields have names of their own).
enum { BN_AP_ADD = 1, BN_AP_DROP = 2, BN_AP_DH_BF16 = 4, BN_AP_OUT_OPTIONAL = 8 };
constexpr const char* kBnApplyNames[7] = {"ap->parts", "ap->coef", "ap->dh", "ap->x", "ap->add", "ap->out", "ap->drop"};
inline int bn_apply_check(const char* who, const lvae_bn_apply* ap, int64_t M, int allows, const char* const (&name)[7] = kBnApplyNames,
                          int align_rc = LVAE_EALIGN) {
  LVAE_REQUIRE(ap && ap->parts && ap->rows > 0 && ap->M == M && ap->coef && ap->dh && ap->x, LVAE_EINVAL,
               "%s: the BatchNorm-backward apply needs %s / rows, M = N*H*W, %s (the coefficient block), %s and %s", who, name[0], name[1], name[2], name[3]);
  LVAE_REQUIRE(ap->out || (allows & BN_AP_OUT_OPTIONAL), LVAE_EINVAL, "%s: the BatchNorm-backward apply needs %s", who, name[5]);
  LVAE_REQUIRE(!ap->add || (allows & BN_AP_ADD), LVAE_EINVAL, "%s: this launch takes no %s with the BatchNorm-backward apply", who, name[4]);
  LVAE_REQUIRE(!ap->drop || (allows & BN_AP_DROP), LVAE_EINVAL, "%s: this launch takes no %s with the BatchNorm-backward apply", who, name[6]);
  LVAE_REQUIRE(!ap->dh_bf16 || (allows & BN_AP_DH_BF16), LVAE_EINVAL, "%s: this launch takes an fp32 %s only", who, name[2]);
  const void* const operand[] = {ap->parts, ap->coef, ap->dh, ap->x, ap->add, ap->out, ap->drop};
  for (int i = 0; i < 7; ++i) LVAE_REQUIRE(al16_or_null(operand[i]), align_rc, "%s: %s must be 16-byte aligned", who, name[i]);
  return 0;
}

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
