/*
 * liblvae_hip.so — C ABI of the MI355X (gfx950) Ladder-VAE hot path.
 *
 * The reference (addtt/ladder-vae-pytorch) has no FFI/plugin boundary of its own: its hot path is stock torch
 * ops called from Python. Each entry point below therefore names the reference call site(s)
 * whose arithmetic it replaces (paths relative to the reference root), and INTEGRATION.md shows the ctypes
 * stub a maintainer of the reference would add.
 *
 * Conventions
 *  - activations are NHWC, contiguous, float32, device memory; `N` = batch.
 *  - the caller owns every buffer including workspaces; nothing here allocates, synchronises or touches the
 *    default stream. `stream` is a hipStream_t passed as void*.
 *  - every function returns 0 on success, a negative LVAE_E* code for a rejected argument, or the positive
 *    hipError_t of a failed launch. `lvae_last_error()` returns a static description of the last failure.
 *  - re-entrant. Mutable process state: the thread-local last-error string, and one atomic "dynamic-LDS attribute set" flag per
 *    kernel (an idempotent hipFuncSetAttribute on first use). The library reads NO environment variable: which kernel variant runs
 *    depends only on the descriptor — shape, alignment, `precision`, `workspace` and the `form` request below. Thresholds between
 *    variants are compile-time constants (csrc/lvae_common.h tune(); a -DLVAE_TUNING_ENV build, used by tools/ only, can sweep them
 *    through LVAE_* variables). Variants that were measured slower in round 2 (256-pixel Winograd workgroups, the persistent bf16 3x3
 *    kernel, the six-product weight gradient) are no longer compiled; phase-skip switches exist only in -DLVAE_PHASE_DEBUG builds.
 *  - the data-parallel gradient exchange is part of the library too (lvae_allreduce_*, at the end of this file): a private RCCL communicator
 *    whose ncclAllReduce runs on a side stream forked off / joined to the launch stream by the library; librccl is resolved at run time
 *    from the path the caller passes (this library has no link-time dependency on it).
 */
#ifndef LVAE_HIP_H
#define LVAE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LVAE_ABI_VERSION 17

#define LVAE_EINVAL (-1)   /* bad argument (null pointer, non-positive size, unsupported combination) */
#define LVAE_EALIGN (-2)   /* pointer / channel count not aligned as the vector path requires */
#define LVAE_EWORKSPACE (-3) /* workspace too small */

/* activation ids shared by every kernel (models/lvae.py:64-69 nonlin table) */
enum { LVAE_STATS_BN_FWD = 0, LVAE_STATS_BN_BWD = 1 };
enum { LVAE_PREC_F32 = 0, LVAE_PREC_BF16 = 1 };
/* Storage type of an activation tensor (lvae_conv_desc.x_dtype / y_dtype / stats_x_dtype and the `dtypes` masks below). bf16 storage exists
 * for the tensors INSIDE a residual block under precision = LVAE_PREC_BF16 (conv outputs y1 / y2, the gate pre-activations ab and their
 * gradients): what torch.autocast(bfloat16) stores for the reference's nn.Conv2d outputs (BASELINE configs[1], [3], [4]). The residual
 * stream, statistics, KL / likelihood terms, parameters and their gradients stay fp32. lvae_resblock_bf16_storage() says whether every kernel
 * of a block's forward and backward has the bf16-storage form for a shape; kernels without it reject bf16 tensors (LVAE_EINVAL). */
enum { LVAE_DT_F32 = 0, LVAE_DT_BF16 = 1 };
/* lvae_conv_desc.form: which arithmetic form an fp32 (LVAE_PREC_F32) descriptor asks for. All forms pass the same parity tests. */
enum {
  LVAE_FORM_AUTO = 0,               /* the library's choice for the shape (what the training step uses) */
  LVAE_FORM_F32_MFMA = 1,           /* every matrix product on v_mfma_f32_32x32x2_f32: Winograd / gate backward without the six-product form */
  LVAE_FORM_SIX_PRODUCT = 2,        /* six exact bf16-piece products per fp32 product wherever the selected kernel has that form (adds the
                                       GateLayer2d forward, which is HBM-bound and defaults to the fp32 MFMA) */
  LVAE_FORM_SIX_PRODUCT_DIRECT = 3  /* large 3x3 layers as a DIRECT six-product convolution instead of Winograd (measured: ties at 16x16, loses at 32x32) */
};
enum { LVAE_ACT_NONE = 0, LVAE_ACT_ELU = 1, LVAE_ACT_RELU = 2, LVAE_ACT_LEAKYRELU = 3, LVAE_ACT_SELU = 4 };

/* spatial gather of an implicit-GEMM convolution */
enum {
  LVAE_GATHER_CONV = 0,      /* ih = oh*stride - pad + kh           (nn.Conv2d forward; dgrad of ConvTranspose2d) */
  LVAE_GATHER_TRANSPOSED = 1 /* ih = (oh + pad - kh)/stride if exact (nn.ConvTranspose2d forward; dgrad of Conv2d) */
};

int lvae_abi_version(void);
const char* lvae_last_error(void);

/* ------------------------------------------------------------------------------------------------------------
 * Convolution as implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32).
 *
 *   y[n,oh,ow,co] = out_act( (bias[co] + sum_{kh,kw,ci} T(x)[n,ih,iw,ci] * w[kh,kw,ci,co]) * out_scale[n,co] )
 *   T(x)[..ci] = in_act(x[..ci]*in_scale[ci] + in_shift[ci])   (identity when in_scale == NULL), zero outside the image
 *
 * replaces: nn.Conv2d / nn.ConvTranspose2d call sites lib/nn.py:83-87,118 ; lib/stochastic.py:25-27 ;
 *           models/lvae.py:73-76 ; models/lvae_layers.py:263-276,347-356 ; lib/likelihoods.py:55-58,199-202
 *           with the BatchNorm-apply + activation of lib/nn.py:80-82 fused into T, the Dropout2d scaling of
 *           lib/nn.py:89 fused into out_scale, torch.cat of models/lvae_layers.py:359 fused as (x, x2), and the
 *           autograd dgrad of all of them (same kernel, transposed weight strides, other gather).
 * ---------------------------------------------------------------------------------------------------------- */
/* Folded BatchNorm finalize of a convolution INPUT (training mode, nn.BatchNorm2d of lib/nn.py:80-81): instead of in_scale /
 * in_shift the kernel gets the partial sums the producer's statistics epilogue wrote — parts [rows + 1][2][C1], whose LAST row
 * holds that producer's pivot (kernels for which lvae_conv2d_folds_bn_finalize != 0, and the gate kernel, store it) — computes
 * scale / shift in its prologue (M = N*H*W elements per channel; gamma / beta may be NULL = 1 / 0), publishes (scale, shift,
 * mean, rstd) to coef_out [4][C1] for the backward and applies the momentum update to running_mean / running_var (may be NULL).
 * Only for descriptors with lvae_conv2d_folds_bn_finalize(d) != 0 (asked on the descriptor WITHOUT in_fold): the position-major
 * kernel of the <= 4x4 levels and the Winograd kernels with at most 64 input channels and at most 512 workgroups. parts must be
 * 16-byte aligned, C1 % 4 == 0. A kernel with lvae_conv2d_folds_bn_finalize(d) != 0 also WRITES rows + 1 rows of statistics
 * (stats_out, LVAE_STATS_BN_FWD): size that buffer accordingly. */
typedef struct lvae_bn_fold {
  const float* parts;
  int32_t rows;
  int64_t M;
  const float* gamma;
  const float* beta;
  float eps, momentum;
  float* running_mean;
  float* running_var;
  float* coef_out;
} lvae_bn_fold;

typedef struct lvae_conv_desc {
  const float* x;        /* [N,H,W,C1] */
  const float* x2;       /* [N,H,W,C2] or NULL: channels C1..C1+C2 of the logical input */
  int32_t C1, C2;
  const float* w;        /* element (tap, k, n) at w[tap*w_stap + k*w_sk + n*w_sn]; k = GEMM reduction channel */
  int64_t w_stap, w_sk, w_sn;
  const float* bias;     /* [Cout] or NULL */
  const float* in_scale; /* [C1+C2] or NULL */
  const float* in_shift; /* [C1+C2] (required when in_scale != NULL) */
  int32_t in_act;
  const float* out_scale; /* [N,Cout] or NULL */
  int32_t out_act;
  float* y;              /* [N,OH,OW,Cout] */
  int32_t N, H, W, OH, OW, Cout;
  int32_t KH, KW, stride, pad;
  int32_t gather;        /* LVAE_GATHER_* */
  int32_t precision;     /* LVAE_PREC_F32 (0): results as an fp32 multiply-add chain (fp32 MFMA, Winograd, or six exact bf16-piece
                            products per fp32 product: finite inputs — of any magnitude up to FLT_MAX, denormals included — only differ from the
                            fp32 MFMA by terms below 2^-24 of a product; an infinite operand gives NaN there, where an fp32 multiply would give
                            +-inf. Winograd (either form) spreads a non-finite input to every output of the tiles whose 4x4 block contains
                            it and to no other; tests/test_forms_gpu.py pins all of this); LVAE_PREC_BF16: operands rounded to bf16 at the matrix-core input, fp32
                            accumulate (kernel variants that have no bf16 form run in fp32) */
  void* workspace;       /* scratch for lvae_conv2d_f32 (transformed weights of the Winograd path) or NULL */
  int64_t workspace_bytes; /* lvae_conv2d_workspace(d) bytes enable every kernel variant; fewer select a variant needing none */
  int32_t workspace_ready; /* non-zero: `workspace` already holds this descriptor's transformed weights (written by
                              lvae_conv2d_prepare_weights after the last change of w); the launch skips its own transform */
  float* stats_out;       /* NULL, or [lvae_conv2d_stats_buffer_rows(d)][2][Cout]: per-workgroup partial BatchNorm statistics of the
                              OUTPUT y: (sum(y - pivot), sum((y - pivot)^2)) per channel, for lvae_bn_finalize_parts_f32 */
  const float* stats_pivot; /* [Cout] pivot of those sums (e.g. the running mean of the BatchNorm that consumes y) */
  /* stats_mode = LVAE_STATS_BN_BWD: y is the gradient dh w.r.t. h = act(x*scale + shift) of a training-mode BatchNorm; the
   * epilogue writes the partials of that BatchNorm's backward, (sum g, sum g*xhat) with g = y * act'(x*scale+shift) and
   * xhat = (x - mean)*rstd, to stats_out for lvae_affine_act_bwd_parts_f32. stats_x = x [N,OH,OW,Cout]; stats_pivot then points to
   * the [4][Cout] coefficient block (scale, shift, mean, rstd) as written by lvae_bn_stats_f32 into consecutive arrays. */
  int32_t stats_mode;     /* LVAE_STATS_BN_FWD (0, the default) or LVAE_STATS_BN_BWD */
  int32_t stats_act;      /* activation of that BatchNorm block (mode LVAE_STATS_BN_BWD) */
  const float* stats_x;
  /* Folded BatchNorm finalize of the INPUT: NULL, or a HOST pointer to the block below (read by the launcher, not by the device) */
  const struct lvae_bn_fold* in_fold;
  int32_t form;           /* LVAE_FORM_* (0 = LVAE_FORM_AUTO) */
  /* one byte each (they share the 8 bytes `form` occupies: grouped launches pass twelve descriptors in one 4 KB kernel-argument block) */
  uint8_t x_dtype;        /* LVAE_DT_*: element type of x (and x2); the pointer fields keep their float* spelling */
  uint8_t y_dtype;        /* LVAE_DT_*: element type of y (lvae_conv2d_wgrad_*: of dy) */
  uint8_t stats_x_dtype;  /* LVAE_DT_*: element type of stats_x */
  uint8_t reserved_;      /* 0 */
} lvae_conv_desc;

/* Kernel choice: lvae_conv2d_f32 / _bf16 choose one kernel per descriptor (pos -> bf16 direct -> Winograd -> halo -> 1x1 -> stride-2 pos -> generic,
 * made on the descriptor without its in_fold), and every query below (_workspace, _variant, _stats_rows, _folds_bn_finalize,
 * _stats_buffer_rows, lvae_resblock_bf16_storage) answers for exactly the kernel the launch takes. A variant that reads a scratch buffer
 * needs d->workspace present, at least lvae_conv2d_workspace(d) bytes and 16-byte aligned; otherwise the choice (and every answer)
 * moves on to the next kernel of the order.
 *
 * Scratch bytes lvae_conv2d_f32 can use for `d` (0 when no variant needs any), answered for a sized, 16-byte aligned d->workspace.
 * Large 3x3 / stride-1 / 64-channel layers run as Winograd F(2x2,3x3) on the fp32 MFMA (2.25x fewer multiplies; coefficients 0, +-1,
 * +-1/2, result within a few ulp of the direct sum) when the scratch is supplied; without it the direct halo-tile kernel runs. */
size_t lvae_conv2d_workspace(const lvae_conv_desc* d);
int lvae_conv2d_f32(const lvae_conv_desc* d, void* stream);
/* dgrad of a 1x1 / stride-1 convolution whose INPUT was a channel concat (x, x2) — MergeLayer / SkipConnectionMerger,
 * models/lvae_layers.py:347-359 — in ONE launch (round 5): `d` describes the dgrad over all C1 + C2 input channels exactly as for lvae_conv2d_f32
 * (d->x = dy, d->Cout = C1 + C2, transposed weight strides); columns [0, split) are written to d->y [N,H,W,split], columns [split, Cout) to
 * dx2 [N,H,W,Cout - split]. At most 128 reduction and 128 output channels, multiples of 4; otherwise LVAE_EINVAL (use two launches with
 * a weight offset, as lvae_conv2d_f32 allows). */
int lvae_conv1x1_dgrad_cat_f32(const lvae_conv_desc* d, float* dx2, int32_t split, void* stream);
/* 1 when lvae_conv1x1_dgrad_cat_f32 takes `d` as given with this split (dx2 assumed 16-byte aligned), 0 when it would return
 * LVAE_EINVAL. Host only, no launch. */
int32_t lvae_conv1x1_dgrad_cat_ok(const lvae_conv_desc* d, int32_t split);
/* Which kernel family lvae_conv2d_f32 runs for `d` as given (workspace and form included): diagnostics for the parity tests and for
 * bench.py's roofline record (which matrix unit issues the FLOPs). */
enum {
  LVAE_VARIANT_DIRECT = 0,       /* fp32 MFMA, direct: halo-tile 3x3, single-shot 1x1 or the generic implicit GEMM */
  LVAE_VARIANT_POS = 2,          /* position-major 3x3 of the <= 4x4 levels (fp32 MFMA) */
  LVAE_VARIANT_WINO_F32 = 3,     /* Winograd F(2x2,3x3), position GEMMs on the fp32 MFMA */
  LVAE_VARIANT_WINO_SIX = 4,     /* Winograd F(2x2,3x3), position GEMMs as six bf16-piece products on the bf16 MFMA */
  LVAE_VARIANT_BF16_DIRECT = 5,  /* direct 3x3, bf16 operands on the bf16 MFMA (precision LVAE_PREC_BF16) */
  LVAE_VARIANT_SIX_DIRECT = 6    /* direct 3x3, six-product form (form LVAE_FORM_SIX_PRODUCT_DIRECT) */
};
int32_t lvae_conv2d_variant(const lvae_conv_desc* d);
/* 1 when lvae_conv2d_f32 runs `d` as given on a position-major kernel (GEMM rows = 32 images at one output position): the stride-1 one
 * of the <= 4x4 levels (LVAE_VARIANT_POS) or the stride-2 / transposed one (3x3, pad 1, one source of at most 64 channels, fp32 storage;
 * its variant is LVAE_VARIANT_DIRECT like the generic kernel's, which this query tells apart). 0 otherwise. Host only, no launch. */
int32_t lvae_conv2d_position_major(const lvae_conv_desc* d);
/* 1 when a residual block whose 3x3 convolutions look like `d` (a FORWARD descriptor: 64 -> 64 channels, precision LVAE_PREC_BF16, its
 * workspace attached) can keep its internal tensors in bf16: forward, dgrad and weight gradient of the convolution, the GateLayer2d
 * forward and its fused backward, and the BatchNorm-backward apply all have a bf16-storage form for N x H x W. 0 otherwise. */
int32_t lvae_resblock_bf16_storage(const lvae_conv_desc* d);
/* The same convolution with bf16 matrix-core operands (v_mfma_f32_32x32x16_bf16): activations (after the fused input transform)
 * and weights are rounded to bf16, products are exact, accumulation, bias, statistics and the stored result are fp32 — the
 * arithmetic of the reference's nn.Conv2d call sites under torch.autocast(bfloat16) (BASELINE configs[1], [3], [4]). Equivalent to
 * lvae_conv2d_f32 on a descriptor with precision = LVAE_PREC_BF16. Set precision before asking lvae_conv2d_stats_rows. */
int lvae_conv2d_bf16(const lvae_conv_desc* d, void* stream);
/* BatchNorm statistics of the convolution OUTPUT fused into the producing kernel's epilogue (saves the separate pass over y):
 * rows of d->stats_out the launch will write, or 0 when the kernel variant this descriptor selects cannot produce them (then
 * leave stats_out NULL and use lvae_bn_stats_f32 on y). Set workspace / workspace_bytes before asking: the answer depends on
 * the variant. */
int32_t lvae_conv2d_stats_rows(const lvae_conv_desc* d);
/* 1 when the variant selected for `d` also stores its pivot behind the partial rows (stats_out then needs rows + 1 rows) and can
 * itself consume such a buffer through d->in_parts (the position-major kernel of the <= 4x4 levels); 0 otherwise. */
int32_t lvae_conv2d_folds_bn_finalize(const lvae_conv_desc* d);
/* Rows to ALLOCATE for d->stats_out: lvae_conv2d_stats_rows(d), plus one when the selected variant stores its pivot row behind them
 * (stats_mode LVAE_STATS_BN_FWD and lvae_conv2d_folds_bn_finalize, asked on the descriptor without its in_fold); 0 when there is no
 * statistics epilogue. Size the buffer
 * from this, read the partial rows [0, lvae_conv2d_stats_rows(d)). */
int32_t lvae_conv2d_stats_buffer_rows(const lvae_conv_desc* d);

/* Batched weight pre-transform: one launch for every convolution of a training step instead of one per convolution call.
 * For each descriptor with lvae_conv2d_workspace(d) > 0 give it a PRIVATE scratch buffer in d->workspace (kept until the
 * weights change), let lvae_conv2d_prepare_entry write its lvae_conv2d_prepare_entry_bytes()-byte table entry, copy the
 * table to device memory once, and call lvae_conv2d_prepare_weights(table, n, largest Cout) after every optimizer step;
 * convolutions then run with d->workspace_ready = 1. */
size_t lvae_conv2d_prepare_entry_bytes(void);
int lvae_conv2d_prepare_entry(const lvae_conv_desc* d, void* entry);
int lvae_conv2d_prepare_weights(const void* entries, int32_t n, int32_t max_cout, void* stream);

/* GateLayer2d forward fused with its 1x1 convolution and the residual add — lib/nn.py:118-126 and lib/nn.py:99.
 * `d` describes the 1x1 conv C -> 2C (d->y receives the pre-activations ab [N,H,W,2C] when non-NULL: the backward
 * reads them); out[..., c] = act(ab[..., c]) * sigmoid(ab[..., C + c]) + res[..., c]  (res may be NULL).
 * Supported: Cin <= 128, 2C <= 128, channel counts multiples of 4; otherwise LVAE_EINVAL (compose lvae_conv2d_f32 +
 * lvae_gate_fwd_f32 instead). */
int lvae_conv1x1_gate_f32(const lvae_conv_desc* d, const float* res, int32_t act, float* out, void* stream);
/* With d->stats_out / d->stats_pivot ([C] pivot) set, lvae_conv1x1_gate_f32 also writes BatchNorm partials of `out` — the next
 * residual block's BatchNorm input — as [lvae_conv1x1_gate_stats_rows(d) + 1][2][C]: the partial rows for
 * lvae_bn_finalize_parts_f32 / lvae_bn_fold, then one row whose first C floats are the pivot (0 rows: not supported for this
 * shape, leave stats_out NULL). */
int32_t lvae_conv1x1_gate_stats_rows(const lvae_conv_desc* d);
/* Which kernel lvae_conv1x1_gate_f32 runs for `d` as given (the alignment of the pointers it carries included; res and out assumed
 * 16-byte aligned): 0 = none, the call would return LVAE_EINVAL — compose lvae_conv2d_f32 + lvae_gate_fwd_f32. Host only, no launch. */
enum {
  LVAE_GATE_PERSISTENT = 1, /* persistent kernel of the 64-channel blocks (the only one with bf16 storage) */
  LVAE_GATE_SINGLE_SHOT = 2 /* single-shot 1x1 kernel with the gate epilogue: Cin <= 128, 2C <= 128 */
};
int32_t lvae_conv1x1_gate_variant(const lvae_conv_desc* d);
/* GateLayer2d backward fused with the dgrad of its 1x1 convolution (autograd of lib/nn.py:118-126): forms
 *   dab[m,c] = dout*sigmoid(b)*act'(a) ; dab[m,C+c] = dout*act(a)*sigmoid(b)*(1-sigmoid(b))      (a, b = the halves of ab)
 * in the kernel's operand staging (also written to `dab` [M,2C] when non-NULL: the weight gradient of the gate convolution
 * reads it) and computes dx = dab . W^T with the descriptor's epilogue. `d` describes that dgrad exactly as for
 * lvae_conv2d_f32 (C1 = 2C, transposed weight strides, y = dx, out_scale = dropout mask); d->x is ignored.
 * Same shape limits as lvae_conv1x1_gate_f32, otherwise LVAE_EINVAL (compose lvae_gate_bwd_f32 + lvae_conv2d_f32). */
int lvae_conv1x1_gate_bwd_f32(const lvae_conv_desc* d, const float* dout, const float* ab, int32_t act, float* dab,
                              void* stream);
/* 1 when lvae_conv1x1_gate_bwd_f32 takes `d` as given (d->x ignored; dout, ab and dab assumed 16-byte aligned), 0 when it would
 * return LVAE_EINVAL. Host only, no launch. */
int32_t lvae_conv1x1_gate_bwd_ok(const lvae_conv_desc* d);

/* GateLayer2d backward of a 64-channel block as ONE persistent kernel: gate derivative + input gradient (exactly
 * lvae_conv1x1_gate_bwd_f32, same descriptor) AND the weight / bias gradient of the gate convolution, dw[ci*dw_sk + co*dw_sn] +=
 * sum_m y[m,ci] * dab[m,co], db[co] += sum_m dab[m,co] (autograd of lib/nn.py:118-126): dab is formed once per 64-pixel tile in LDS and
 * never written to memory; y [M,64] is the convolution input the forward saved. Deterministic (per-workgroup partial slabs in
 * `workspace`, summed in a fixed order). lvae_conv1x1_gate_bwd_wgrad_workspace(d) == 0: shape not supported (needs C = 64 and at
 * least 16384 pixels) — use lvae_conv1x1_gate_bwd_f32 + lvae_conv2d_wgrad_f32. */
/* Deferred BatchNorm-backward apply (round 5; `ap` NULL or ap->parts NULL: none). In a chain of residual blocks the block that ran just
 * before this one in the backward ends with dx = BN1'(dh; x) + add (lvae_affine_act_bwd_parts_f32), and that dx IS this call's dout. With
 * `ap` the kernel reduces the partial rows parts [rows][2][64] (written by the producer of dh, stats_mode LVAE_STATS_BN_BWD) itself, forms
 * dout on the fly from (dh — element type dh_bf16 —, x, add or NULL; coefficient block coef [4][64] = scale, shift, mean, rstd; M = N*H*W),
 * stores it to out [M][64] (fp32) and accumulates dgamma / dbeta; `dout` is not read. One launch, its finalize launch and one tensor pass
 * per gated block less. Not with form LVAE_FORM_F32_MFMA. */
typedef struct lvae_bn_apply {
  const float* parts;
  int32_t rows;
  int32_t act;
  int64_t M;
  const float* coef;
  const float* dh;
  const float* x;
  const float* add;
  float* dgamma;
  float* dbeta;
  float* out;
  int32_t dh_bf16;
  int32_t reserved_;
  const float* drop;   /* lvae_conv2d_wgrad_apply_f32 only: Dropout2d mask [N][C] multiplied into the result, or NULL */
} lvae_bn_apply;
size_t lvae_conv1x1_gate_bwd_wgrad_workspace(const lvae_conv_desc* d);
/* 1 when lvae_conv1x1_gate_bwd_wgrad_f32 takes `d` as given with a deferred apply (`ap`): lvae_conv1x1_gate_bwd_wgrad_workspace(d) != 0
 * and not form LVAE_FORM_F32_MFMA at precision LVAE_PREC_F32. Both queries ignore d->x and assume the operands outside the descriptor
 * 16-byte aligned. Host only, no launch. */
int32_t lvae_conv1x1_gate_bwd_wgrad_apply_ok(const lvae_conv_desc* d);
int lvae_conv1x1_gate_bwd_wgrad_f32(const lvae_conv_desc* d, const float* dout, const float* ab, const float* y, int32_t act,
                                    float* dw, int64_t dw_sk, int64_t dw_sn, float* db, void* workspace, size_t workspace_bytes,
                                    const lvae_bn_apply* ap, void* stream);
/* The same launch WITHOUT the saved pre-activations (fp32 six-product form only): where the forward was lvae_resblock_conv_f32 with the
 * gate epilogue of the 256-pixel Winograd kernel and ext->ab == NULL, ab = conv1x1(y) + gate_bias was never written. The kernel forms it
 * again per 64-pixel tile from y (which it stages anyway for the weight gradient) and the gate weights pre-split for the FORWARD direction:
 * gate_ws / gate_ws_bytes / gate_ws_ready exactly as in lvae_rb_ext for that forward call (lvae_resblock_gate_workspace() bytes of the
 * 64 -> 128 descriptor; not ready: written here first from gate_w, element (ci, co) at gate_w[ci*gate_w_sk + co*gate_w_sn]), in the
 * forward's accumulation order: the recomputed values are the forward's bit for bit, and so is every result. gate_bias [128] or NULL.
 * `d`, dout, y, act, dw .. ap as for lvae_conv1x1_gate_bwd_wgrad_f32 (same workspace). lvae_conv1x1_gate_bwd_wgrad_recompute_ok(d): 1
 * when it takes `d` (with or without `ap`): lvae_conv1x1_gate_bwd_wgrad_apply_ok(d), fp32-stored tensors, precision LVAE_PREC_F32, form
 * not LVAE_FORM_F32_MFMA. Host only, no launch. */
int32_t lvae_conv1x1_gate_bwd_wgrad_recompute_ok(const lvae_conv_desc* d);
int lvae_conv1x1_gate_bwd_wgrad_recompute_f32(const lvae_conv_desc* d, const float* dout, const float* y, int32_t act, void* gate_ws,
                                              int64_t gate_ws_bytes, int32_t gate_ws_ready, const float* gate_w, int64_t gate_w_sk,
                                              int64_t gate_w_sn, const float* gate_bias, float* dw, int64_t dw_sk, int64_t dw_sn,
                                              float* db, void* workspace, size_t workspace_bytes, const lvae_bn_apply* ap, void* stream);

/* The whole backward of a 1x1 / stride-1 convolution over a 64 + 64 channel concat with 64 output channels (MergeLayer /
 * SkipConnectionMerger) as ONE persistent kernel plus the fixed-order slab reduce: both halves of the input gradient (what
 * lvae_conv1x1_dgrad_cat_f32 writes) AND the weight / bias gradient (what lvae_conv2d_wgrad_f32 accumulates), fp32-equivalent (six bf16-piece
 * products per product). `d` describes the dgrad over the concat exactly as for lvae_conv1x1_dgrad_cat_f32 with split = 64: d->x = dy
 * [N,H,W,64], C1 = 64, Cout = 128, transposed weight strides with w_sk == 1; d->y is not used. x1, x2 [N,H,W,64]: the two inputs of the
 * forward; dx1, dx2 [N,H,W,64]: their gradients (overwritten); dweight: the weight's own layout, element (ci, co) at
 * dweight[ci*d->w_sn + co*d->w_sk], accumulated; dbias [64] or NULL, accumulated. `ap` (NULL or ap->parts NULL: none): dy does not exist
 * yet but is the deferred BatchNorm-backward apply of the residual block that read the convolution's output, as for
 * lvae_conv1x1_gate_bwd_wgrad_f32 (fp32 dh, no drop); d->x is then not read, and the formed dy is stored only where ap->out is not NULL.
 * max_workgroups: 0 = one per 64-pixel tile up to 256; a positive value caps the grid further (a workgroup then loops over several tiles).
 * lvae_conv1x1_cat_bwd_workspace(d, split): bytes of scratch the call needs at any max_workgroups, 0 when it does not take `d` (anything
 * but the shape above, split != 64, a dy or weight pointer off 16 bytes, bf16 storage, precision LVAE_PREC_BF16, form LVAE_FORM_F32_MFMA);
 * lvae_conv1x1_cat_bwd_apply_ok(d, split): 1 when it takes `d` with a deferred apply. Both assume the operands outside the descriptor
 * 16-byte aligned; host only, no launch. A call that is not taken launches and writes nothing: LVAE_EINVAL (shape), LVAE_EWORKSPACE
 * (workspace_bytes below the query), LVAE_EALIGN (an operand outside the descriptor off 16 bytes). */
size_t lvae_conv1x1_cat_bwd_workspace(const lvae_conv_desc* d, int32_t split);
int32_t lvae_conv1x1_cat_bwd_apply_ok(const lvae_conv_desc* d, int32_t split);
int lvae_conv1x1_cat_bwd_f32(const lvae_conv_desc* d, const float* x1, const float* x2, float* dx1, float* dx2, float* dweight, float* dbias,
                             const lvae_bn_apply* ap, void* workspace, size_t workspace_bytes, int32_t max_workgroups, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Fused residual-block kernels of the low-resolution levels (H*W a divisor of 64: 8x8, 4x4, 2x2 ...), "whole-image tiles"
 * (csrc/resblock_img.hip). A workgroup's 64 / 128 GEMM rows are whole images, so the 3x3 convolution of `d` (64 -> 64 channels,
 * stride 1, pad 1, fp32 tensors) can take its input from — and hand its output to — the neighbouring ops of a residual block
 * (lib/nn.py:78-99,118-126) through LDS instead of through memory and separate launches:
 *
 *   prologue  LVAE_RB_PRO_AFFINE    T(x) = in_act(x*in_scale + in_shift), exactly lvae_conv2d_f32's input transform; d->in_fold works too
 *             LVAE_RB_PRO_BN_APPLY  d->x = dh, the gradient w.r.t. h = act(BN(bwd_x)); the input of the convolution (a dgrad descriptor) is
 *                                   the training-mode BatchNorm backward of lvae_affine_act_bwd_parts_f32 — partial rows bwd_parts
 *                                   [bwd_rows][2][64] written by the producer of dh (stats_mode LVAE_STATS_BN_BWD), coefficient block
 *                                   bwd_coef [4][64], bwd_M = N*H*W, dgamma / dbeta accumulated by workgroup 0 — times the Dropout2d mask
 *                                   pro_drop [N][64]; also stored to xt_out [N,H,W,64] (the weight gradient of the producer reads it)
 *             LVAE_RB_PRO_GATE_BWD  the input of the convolution is the GateLayer2d backward of lvae_conv1x1_gate_bwd_f32: dab from
 *                                   (dout [M][64], ab_in [M][128]) — stored to dab when non-NULL — then (dab . gate_w^T) * pro_drop, stored to xt_out;
 *                                   with ap_parts != NULL dout itself is formed in the prologue (deferred BatchNorm-backward apply, see the struct)
 *   epilogue  LVAE_RB_EPI_PLAIN     y = (conv + bias) * out_scale and the statistics epilogue of lvae_conv2d_f32 (stats_out: lvae_resblock_conv_rows(d)
 *                                   rows, plus one pivot row behind them for LVAE_STATS_BN_FWD)
 *             LVAE_RB_EPI_GATE      (forward prologue only) y as above, then lvae_conv1x1_gate_f32 on it inside the same launch: ab [M][128]
 *                                   (optional), out = act(a) * sigmoid(b) + res, BatchNorm partials of out in out_stats [rows + 1][2][64]
 *
 * gate_w: element (reduction index k, output column n) at gate_w[k * gate_w_sk + n * gate_w_sn] — forward: k = input channel (64),
 * n = gate channel (128); backward: k = gate channel (128), n = input channel (64).
 * d->workspace: lvae_resblock_conv_workspace(d) bytes of pre-split weights, private to (w, orientation) like lvae_conv2d_f32's; filled by the
 * launch itself unless d->workspace_ready, or by lvae_conv2d_prepare_weights from a table entry written by lvae_resblock_conv_prepare_entry.
 * Arithmetic by d->precision: LVAE_PREC_F32 = six exact bf16-piece products per fp32 product (as LVAE_FORM_SIX_PRODUCT), LVAE_PREC_BF16 =
 * bf16 operands. lvae_resblock_conv_rows(d) == 0: shape not supported (use the one-kernel-per-op entry points).
 * replaces: lib/nn.py:80-89 (BatchNorm + activation + conv + Dropout2d), :118-126 + :99 (GateLayer2d + residual) and their autograd.
 * ---------------------------------------------------------------------------------------------------------- */
enum { LVAE_RB_PRO_AFFINE = 0, LVAE_RB_PRO_BN_APPLY = 1, LVAE_RB_PRO_GATE_BWD = 2 };
enum { LVAE_RB_EPI_PLAIN = 0, LVAE_RB_EPI_GATE = 1 };
typedef struct lvae_rb_ext {
  int32_t prologue, epilogue; /* LVAE_RB_PRO_*, LVAE_RB_EPI_* */
  const float* gate_w;    /* the 1x1 gate weight: only read when the pre-split copy below is not ready */
  int64_t gate_w_sk, gate_w_sn;
  void* gate_ws;          /* lvae_resblock_gate_workspace() bytes, private to (gate_w, direction): the pre-split gate weights */
  int64_t gate_ws_bytes;
  int32_t gate_ws_ready;  /* non-zero: gate_ws was written by lvae_conv2d_prepare_weights (table entry: lvae_resblock_gate_prepare_entry) after the last change of gate_w */
  const float* gate_bias; /* [128] or NULL (forward) */
  int32_t act;            /* activation of the gate (LVAE_ACT_*) */
  const float* res;       /* [M][64] or NULL */
  float* ab;              /* [M][128] or NULL */
  float* out;             /* [M][64] */
  float* out_stats;       /* NULL or [rows + 1][2][64] */
  const float* out_stats_pivot;
  const float* dout;      /* gate backward: [M][64] */
  const float* ab_in;     /* [M][128] */
  float* dab;             /* [M][128] or NULL */
  const float* bwd_parts; /* BatchNorm-apply prologue */
  int32_t bwd_rows;
  int32_t bwd_act;
  int64_t bwd_M;
  const float* bwd_coef;  /* [4][64]: scale, shift, mean, rstd */
  const float* bwd_x;     /* [M][64] */
  float* dgamma;          /* [64] accumulated, or NULL */
  float* dbeta;
  const float* pro_drop;  /* [N][64] or NULL */
  float* xt_out;          /* [M][64] or NULL */
  /* Optional L2 warm-up for the launch that FOLLOWS this one on the stream: up to two byte ranges (its pre-split weights — they are different
   * for every convolution of a step, i.e. cold in every XCD's L2 when their kernel starts) that this launch's workgroups touch once per
   * XCD while they wait for their own operands. Speed only: the ranges are read, never interpreted. */
  const void* pf_ptr[2];
  int64_t pf_bytes[2];
  /* Deferred BatchNorm-backward apply in front of LVAE_RB_PRO_GATE_BWD (round 5; ap_parts == NULL: none). In a chain of residual blocks the
   * block that ran just before this one in the backward ends with dx = BN1'(dh1; x) + dout (lvae_affine_act_bwd_parts_f32 with `add`), and
   * that dx IS this launch's dout. Instead of a launch of its own, this prologue forms it from (ap_parts [ap_rows][2][64] written by the
   * producer of ap_dh, coefficient block ap_coef [4][64], ap_M = N*H*W, ap_dh, ap_x, ap_add — all required), accumulates ap_dgamma / ap_dbeta
   * (workgroup 0) and stores it to ap_out [M][64]; `dout` is not read. */
  const float* ap_parts;
  int32_t ap_rows;
  int32_t ap_act;
  int64_t ap_M;
  const float* ap_coef;
  const float* ap_dh;
  const float* ap_x;
  const float* ap_add;
  float* ap_dgamma;
  float* ap_dbeta;
  float* ap_out;
  /* Workgroups per tile of an LVAE_RB_EPI_PLAIN launch: 0 = the library decides (two, each computing one 32-channel half of the tile's
   * output, where 32-pixel tiles in the six-product form leave at least half the CUs without a workgroup: the 4x4 and 2x2 levels at batch
   * 256), 1 = one, 2 = two wherever that kernel exists (32-pixel tiles, plain epilogue, LVAE_PREC_F32). Speed only: y, the statistics
   * rows and everything the prologue stores are bit for bit the same, and lvae_resblock_conv_rows(d) does not change.
   * lvae_resblock_conv_nsplit(d, ext) answers what a launch would use (0: shape not supported). */
  int32_t nsplit;
} lvae_rb_ext;
/* Pre-split copy of a gate weight for lvae_resblock_conv_f32: `g` describes the 1x1 convolution in the direction it is used (forward:
 * C1 = 64, Cout = 128, w_sk / w_sn = strides of the input / gate channel; backward: C1 = 128, Cout = 64, strides swapped); only C1, Cout, w,
 * w_sk, w_sn, precision and workspace are read. */
size_t lvae_resblock_gate_workspace(const lvae_conv_desc* g);
int lvae_resblock_gate_prepare_entry(const lvae_conv_desc* g, void* entry);
int32_t lvae_resblock_conv_rows(const lvae_conv_desc* d);
int32_t lvae_resblock_conv_nsplit(const lvae_conv_desc* d, const lvae_rb_ext* ext);
/* Rows of out_stats (= workgroups) of an LVAE_RB_EPI_GATE launch. Besides the whole-image shapes (= lvae_resblock_conv_rows) the forward
 * conv + gate fusion exists for the shapes of the 256-pixel six-product Winograd kernel (fp32, 64 -> 64 channels: the 16x16 and 32x32 levels at
 * batch 256; lvae_conv2d_variant(d) == LVAE_VARIANT_WINO_SIX with at least 256 workgroups): attach THAT kernel's workspace
 * (lvae_conv2d_workspace / lvae_conv2d_prepare_entry) to d before asking and before the launch. 0: use lvae_conv2d_f32 + lvae_conv1x1_gate_f32. */
int32_t lvae_resblock_conv_gate_rows(const lvae_conv_desc* d);
size_t lvae_resblock_conv_workspace(const lvae_conv_desc* d);
int lvae_resblock_conv_prepare_entry(const lvae_conv_desc* d, void* entry);
int lvae_resblock_conv_f32(const lvae_conv_desc* d, const lvae_rb_ext* ext, void* stream);

/* Weight / bias gradient of the convolution described by `d` (d->y is unused, d->w gives only the strides):
 *   dw[tap,k,n] += sum_{n,oh,ow} T(x)[n,ih,iw,k] * dy[n,oh,ow,n]     db[n] += sum dy[..,n]
 * written with the strides d->w_stap/w_sk/w_sn into `dw` (accumulating). Deterministic: split-K partial slabs
 * in `workspace` are summed in a fixed order by a second kernel. `dy` is [N,OH,OW,Cout].
 * Kernel choice: one ordered table of kernel families, img -> bf16 -> Winograd -> 1x1 -> tile -> thin -> generic; each row holds the family's
 * plan (every condition its launch depends on) and whether it needs 16-byte aligned dy and / or workspace, and the first row that takes `d`
 * is the choice, made once per call. lvae_conv2d_wgrad_workspace / _variant / _apply_ok and the grouped queries answer for that choice with
 * 16-byte aligned dy and workspace.
 * workspace bytes needed: lvae_conv2d_wgrad_workspace(d). With a dy or workspace that is not 16-byte aligned the launch may take a kernel
 * that needs more; it then returns LVAE_EWORKSPACE instead of writing past workspace_bytes.
 * replaces: autograd's convolution_backward (weight, bias) for every call site listed above. */
size_t lvae_conv2d_wgrad_workspace(const lvae_conv_desc* d);
int lvae_conv2d_wgrad_f32(const lvae_conv_desc* d, const float* dy, float* dw, float* db, void* workspace,
                          size_t workspace_bytes, void* stream);
/* The same gradient with bf16 matrix-core operands (transposed LDS reads feed v_mfma_f32_32x32x16_bf16; fp32 accumulation, fp32 bias
 * gradient, fp32 partial slabs): lvae_conv2d_wgrad_f32 on a descriptor with precision = LVAE_PREC_BF16. Shapes without a bf16
 * kernel (anything but 3x3 / stride 1 / <= 64 input channels / >= 16384 pixels) run in fp32. */
int lvae_conv2d_wgrad_bf16(const lvae_conv_desc* d, const float* dy, float* dw, float* db, void* workspace, size_t workspace_bytes,
                           void* stream);
/* Weight gradient whose dY operand is the result of a BatchNorm-backward apply that has not run (round 5): dy = BN'(ap->dh; ap->x) * ap->drop
 * — exactly lvae_affine_act_bwd_parts_f32(parts, dh, x, ..., drop) — is formed while the kernel stages its operand, stored to ap->out
 * [N,H,W,64] for the dgrad that follows, and used as dY; ap->dgamma / dbeta are accumulated. One launch, its finalize launch and one
 * tensor pass per BatchNorm less. lvae_conv2d_wgrad_apply_ok(d) != 0: the Winograd-domain fp32 weight gradient of a 64 -> 64 layer with
 * W = 16 or 32 (the >= 16x16 levels at batch 256). ap->add must be NULL, dh fp32. */
int32_t lvae_conv2d_wgrad_apply_ok(const lvae_conv_desc* d);
int lvae_conv2d_wgrad_apply_f32(const lvae_conv_desc* d, const lvae_bn_apply* ap, float* dw, float* db, void* workspace,
                                size_t workspace_bytes, void* stream);
/* Both weight gradients of a residual block in one launch and one slab reduce: A = the block's first convolution with the apply `ap` in
 * front, exactly as lvae_conv2d_wgrad_apply_f32(a, ap, dw_a, db_a, ...), B = its second convolution with a real dy, exactly as
 * lvae_conv2d_wgrad_f32(b, dy_b, dw_b, db_b, ...). The two share the chip: each gradient is summed over about half as many partial slabs as
 * alone (A gets the larger share, its chunks cost more), so results differ from the two single calls by the summation order only; they are
 * reproducible from run to run. lvae_conv2d_wgrad_pair_ok(a, b) != 0 exactly when both descriptors take the Winograd family, A has
 * lvae_conv2d_wgrad_apply_ok, both have the same geometry (N, H, W, kernel, channels) with Cout == 64, and both are fp32 in arithmetic and
 * storage. The queries read plans only: host only, no launch. lvae_conv2d_wgrad_pair_schedule writes sched[6] = ranges, chunks per range
 * and workgroups of A, then of B (a chunk = 16 Winograd tiles; range r of a problem takes chunks [r * cpr, min(total, (r + 1) * cpr)) of
 * its N * H * W / 64) and returns lvae_conv2d_wgrad_pair_ok. workspace: lvae_conv2d_wgrad_pair_workspace(a, b) bytes, 16-byte aligned like
 * dy_b and the operands of ap. */
int32_t lvae_conv2d_wgrad_pair_ok(const lvae_conv_desc* a, const lvae_conv_desc* b);
size_t lvae_conv2d_wgrad_pair_workspace(const lvae_conv_desc* a, const lvae_conv_desc* b);
int32_t lvae_conv2d_wgrad_pair_schedule(const lvae_conv_desc* a, const lvae_conv_desc* b, int32_t* sched);
int lvae_conv2d_wgrad_pair_f32(const lvae_conv_desc* a, const lvae_bn_apply* ap, const lvae_conv_desc* b, const float* dy_b, float* dw_a,
                               float* db_a, float* dw_b, float* db_b, void* workspace, size_t workspace_bytes, void* stream);
/* n = 1 to 3 independent weight gradients in the Winograd domain in one launch and one slab reduce (the convolutions of a stochastic
 * layer at the 16x16 level: conv_out 32 -> 64, conv_in_q and conv_in_p 64 -> 64): same results as n calls of lvae_conv2d_wgrad_f32 up to
 * the summation order and, for a gradient lvae_conv2d_wgrad_f32 runs in another family, the kernel's arithmetic; reproducible from run to
 * run. Here, and only here, the family also takes 32 input channels (one block of input channels, one workgroup per range):
 * lvae_conv2d_wgrad_f32, the grouped call and their queries keep the kernel they have always chosen for such a gradient. n = 1 runs one
 * gradient by itself on this family. lvae_conv2d_wgrad_shared_ok != 0
 * exactly when every descriptor has a shape of the Winograd family (3x3, stride 1, pad 1, 32 or 64 input channels), all have one N, H and W, at
 * most 64 output channels, fp32 arithmetic and storage, and no gradient has a deferred apply in front (aps: NULL, or n pointers that
 * are all NULL; a gradient whose dy lvae_bn_apply still has to form goes out with lvae_conv2d_wgrad_pair_f32 / _apply_f32). An explicit
 * request: the pixel limit of the grouped call's Winograd groups does not apply. The chip's 256 workgroups are split so that every problem
 * has ranges of the same number of chunks, a range taking two workgroups with 64 input channels and one with 32;
 * lvae_conv2d_wgrad_shared_schedule writes sched[3 * n] = ranges, chunks per range and workgroups of each problem in turn (chunks and
 * ranges as for the pair) and returns lvae_conv2d_wgrad_shared_ok. The queries read plans only: host only, no launch.
 * workspace: lvae_conv2d_wgrad_shared_workspace(descs, n) bytes, 16-byte aligned like every dy[i]. No two entries may share a dw. */
int32_t lvae_conv2d_wgrad_shared_ok(const lvae_conv_desc* descs, const lvae_bn_apply* const* aps, int32_t n);
size_t lvae_conv2d_wgrad_shared_workspace(const lvae_conv_desc* descs, int32_t n);
int32_t lvae_conv2d_wgrad_shared_schedule(const lvae_conv_desc* descs, const lvae_bn_apply* const* aps, int32_t n, int32_t* sched);
int lvae_conv2d_wgrad_shared_f32(const lvae_conv_desc* descs, const float* const* dy, float* const* dw, float* const* db, int32_t n,
                                 void* workspace, size_t workspace_bytes, void* stream);
/* Which kernel family lvae_conv2d_wgrad_f32 (and the grouped call) runs for `d` (d->x_dtype / y_dtype = the storage types of x / dy):
 * diagnostics for the parity tests and the profiles. */
enum {
  LVAE_WGRAD_VARIANT_GENERIC = 0,   /* fp32 MFMA, generic implicit GEMM (strided / transposed / odd channel counts) */
  LVAE_WGRAD_VARIANT_IMG = 1,       /* whole-image tiles of the H*W <= 64 levels on the bf16 matrix pipe: six exact bf16-piece products per fp32
                                       product (LVAE_PREC_F32) or bf16 operands (LVAE_PREC_BF16); 3x3 (<= 64 -> <= 64 channels) and 1x1
                                       (<= 64 -> <= 128), up to 32 gradients per launch (csrc/conv_wgrad_img.hip, round 5) */
  LVAE_WGRAD_VARIANT_BF16 = 2,      /* 3x3, bf16 operands, >= 16384 pixels (whole-slab or half-slab form) */
  LVAE_WGRAD_VARIANT_WINO = 3,      /* Winograd-domain fp32 MFMA (large 3x3 layers) */
  LVAE_WGRAD_VARIANT_DIRECT_1X1 = 4,/* 1x1 at >= 32 k pixels straight from memory */
  LVAE_WGRAD_VARIANT_TILE = 5,      /* stride-1 "same" 3x3 / 1x1 on LDS-resident tiles, fp32 MFMA, wave-specialised */
  LVAE_WGRAD_VARIANT_THIN = 6       /* stems: one workgroup per image, vector ALU */
};
int32_t lvae_conv2d_wgrad_variant(const lvae_conv_desc* d);
/* n independent weight gradients (descs[i], dy[i], dw[i], db[i]; db[i] may be NULL): same results as n calls of
 * lvae_conv2d_wgrad_f32 in index order. The low-resolution levels of the ladder fill 16-64 CUs per gradient and depend on
 * nothing but their own inputs, so gradients of one kernel family that share its kernel instantiation go out together: up to 12 per
 * launch in the tile family (by its template pair), up to 12 in the Winograd family (by image width, below 65536 pixels per gradient),
 * up to 32 in the whole-image family (by its kind), each with grouped slab reductions. Groups are issued first (tile, Winograd,
 * whole-image; entries in index order), then everything else one by one in index order, a tile or Winograd gradient alone in its group
 * among them. No two entries may accumulate into overlapping dw/db.
 * workspace: lvae_conv2d_wgrad_grouped_workspace(descs, n) bytes. */
size_t lvae_conv2d_wgrad_grouped_workspace(const lvae_conv_desc* descs, int32_t n);
int lvae_conv2d_wgrad_grouped_f32(const lvae_conv_desc* descs, const float* const* dy, float* const* dw, float* const* db,
                                  int32_t n, void* workspace, size_t workspace_bytes, void* stream);
/* Host only, no launch. How lvae_conv2d_wgrad_grouped_f32 issues descs[0..n) given 16-byte aligned dy and workspace:
 * launch_of[i] = index, in issue order, of the launch that computes entry i. Returns the number of launches. */
int32_t lvae_conv2d_wgrad_grouped_schedule(const lvae_conv_desc* descs, int32_t n, int32_t* launch_of);

/* ------------------------------------------------------------------------------------------------------------
 * BatchNorm2d (training statistics) — lib/nn.py:80-81 (nn.BatchNorm2d, momentum 0.1, eps 1e-5)
 * ---------------------------------------------------------------------------------------------------------- */
/* Per-channel batch statistics of x [M,C] (M = N*H*W): writes
 *   scale[c] = gamma[c]*rstd[c], shift[c] = beta[c] - mean[c]*scale[c], mean[c], rstd[c]
 * and, when running_mean != NULL, updates running_mean/var with `momentum` (unbiased variance).
 * Two launches (per-chunk partial sums, fixed-order finalize: bitwise reproducible, no float atomics). A single launch with a
 * last-workgroup-done hand-off was measured and rejected: on the 8-XCD part every workgroup's agent-scope release/acquire
 * writes back and invalidates its XCD's L2 (+20 us per launch).
 * workspace: lvae_bn_stats_workspace(M, C) bytes. */
size_t lvae_bn_stats_workspace(int64_t M, int32_t C);
int lvae_bn_stats_f32(const float* x, int64_t M, int32_t C, const float* gamma, const float* beta, float eps,
                      float momentum, float* running_mean, float* running_var, float* scale, float* shift,
                      float* mean, float* rstd, void* workspace, size_t workspace_bytes, void* stream);
/* Finalize from per-workgroup partials written by a convolution epilogue (lvae_conv_desc.stats_out): parts [rows][2][C] with
 * the pivot the producer used; same outputs and running-statistics update as lvae_bn_stats_f32 over M rows. `pivot` may alias
 * running_mean (each channel's pivot is read before its running mean is updated). */
int lvae_bn_finalize_parts_f32(const float* parts, int32_t rows, int64_t M, int32_t C, const float* pivot, const float* gamma,
                               const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                               float* scale, float* shift, float* mean, float* rstd, void* stream);
/* Inference form: scale/shift from the running statistics. */
int lvae_bn_eval_coeffs_f32(int32_t C, const float* gamma, const float* beta, const float* running_mean,
                            const float* running_var, float eps, float* scale, float* shift, void* stream);

/* y = act(x*scale[c] + shift[c]) materialised (used where no convolution consumes it: 'cabdcabd' blocks). */
int lvae_affine_act_f32(const float* x, int64_t M, int32_t C, const float* scale, const float* shift, int32_t act,
                        const float* row_scale, int64_t rows_per_n, float* y, void* stream);

/* Backward of h = act(x*scale + shift) with batch statistics (BatchNorm training) or fixed coefficients.
 *   g = dh * act'(u), u = x*scale+shift
 *   bn_train: dgamma += sum g*xhat, dbeta += sum g, dx = scale*(g - mean(g) - xhat*mean(g*xhat))
 *   else    : dx = scale*g
 * then dx *= drop[n,c] (optional Dropout2d mask of the producer) and dx += add (optional residual gradient).
 * Three launches (partial sums, finalize, apply); workspace lvae_bn_stats_workspace(M,C) bytes. */
int lvae_affine_act_bwd_f32(const float* dh, const float* x, int64_t M, int32_t C, const float* scale,
                            const float* shift, int32_t act, int32_t bn_train, const float* mean, const float* rstd,
                            float* dgamma, float* dbeta, const float* drop, int64_t rows_per_n, const float* add,
                            float* dx, void* workspace, size_t workspace_bytes, void* stream);
/* The training-mode case with the reduction already done by the epilogue of the convolution that produced dh
 * (lvae_conv_desc.stats_mode = LVAE_STATS_BN_BWD, parts [rows][2][C]): finalize + apply, two launches.
 * workspace: 2*C floats. */
int lvae_affine_act_bwd_parts_f32(const float* parts, int32_t rows, const float* dh, const float* x, int64_t M, int32_t C,
                                  const float* scale, const float* shift, int32_t act, const float* mean, const float* rstd,
                                  float* dgamma, float* dbeta, const float* drop, int64_t rows_per_n, const float* add,
                                  float* dx, void* workspace, size_t workspace_bytes, int32_t dtypes, void* stream);
/* dtypes: bit 0 dh, bit 1 x, bit 2 dx stored as bf16 (LVAE_DT_BF16), else fp32; `add` and everything else fp32. */

/* ------------------------------------------------------------------------------------------------------------
 * GateLayer2d epilogue + residual add — lib/nn.py:121-126 and lib/nn.py:99
 *   ab [M,2C] -> out[m,c] = act(ab[m,c]) * sigmoid(ab[m,C+c]) + res[m,c]      (res may be NULL)
 *   bwd: dab[m,c] = dout*sigmoid(b)*act'(a) ; dab[m,C+c] = dout*act(a)*sigmoid(b)*(1-sigmoid(b))
 * ---------------------------------------------------------------------------------------------------------- */
int lvae_gate_fwd_f32(const float* ab, const float* res, int64_t M, int32_t C, int32_t act, float* out, void* stream);
int lvae_gate_bwd_f32(const float* dout, const float* ab, int64_t M, int32_t C, int32_t act, float* dab, void* stream);

/* generic small elementwise helpers used by the host glue */
/* y = act(x) in place-capable; dact: dx = dy * act'(x) expressed from the OUTPUT y (elu/relu/leaky/selu allow it) */
int lvae_act_bwd_from_out_f32(const float* dy, const float* y, int64_t n, int32_t act, float* dx, void* stream);
int lvae_add_f32(const float* a, const float* b, int64_t n, float* out, void* stream);
/* out = (a + b) + c — the gradient of an activation with three consumers (TopDownLayer input: models/lvae_layers.py:134-160). */
int lvae_add3_f32(const float* a, const float* b, const float* c, int64_t n, float* out, void* stream);
/* out[0] = sum_l mean_n x[l][n] — `logp` of models/lvae.py:301 from the [L][N] matrix of per-layer, per-sample log p(z). */
int lvae_sum_of_row_means_f32(const float* x, int32_t L, int32_t N, float* out, void* stream);
/* residual without gate (lib/nn.py:99 when gated is falsy): out = (a*rowscale) + b */
int lvae_scale_rows_add_f32(const float* a, const float* row_scale, int64_t rows_per_n, int32_t C, const float* b,
                            int64_t M, float* out, void* stream);
/* out[p] (+)= sum_r x[r, p]  (batch reduction of a broadcast parameter's gradient, e.g. top_prior_params) */
int lvae_colsum_f32(const float* x, int64_t R, int64_t P, float* out, int32_t accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * NormalStochasticBlock2d elementwise core — lib/stochastic.py:45-99 and kl_normal_mc lib/stochastic.py:209-226
 * p, q: [N,HW,2Z] (mu = channels [0,Z), logvar = [Z,2Z)); p may be batch-broadcast (p_bcast=1: [1,HW,2Z]); q may be
 * NULL (sample from p). mode: 0 = z = mu + exp(lv/2)*eps, 1 = z = mu (use_mode), 2 = z given (forced_latent).
 * outputs: z [N,HW,Z]; logprob_p, logprob_q, kl_samplewise [N]; kl_spatial [N,HW] (analytical, sum over Z).
 * HW * Z * 2 > INT32_MAX: LVAE_EINVAL, forward and backward (a sample's elements are indexed with int).
 * ---------------------------------------------------------------------------------------------------------- */
int lvae_normal_stochastic_fwd_f32(const float* p, int32_t p_bcast, const float* q, const float* eps, int32_t N,
                                   int32_t HW, int32_t Z, int32_t mode, int32_t analytical_kl, float* z,
                                   float* logprob_p, float* logprob_q, float* kl_samplewise, float* kl_spatial,
                                   void* stream);
/* Backward. Upstream: dz [N,HW,Z] (may be NULL), g_lp, g_lq, g_kl [N] (may be NULL), g_ks [N,HW] (may be NULL).
 * Writes dp [N,HW,2Z] (caller sums over N when p was broadcast) and dq [N,HW,2Z] (NULL when q is NULL). */
int lvae_normal_stochastic_bwd_f32(const float* p, int32_t p_bcast, const float* q, const float* eps, const float* z,
                                   const float* dz, const float* g_lp, const float* g_lq, const float* g_kl,
                                   const float* g_ks, int32_t N, int32_t HW, int32_t Z, int32_t mode,
                                   int32_t analytical_kl, float* dp, float* dq, void* stream);

/* The same core with the posterior given RELATIVE to the prior (csrc/stochastic_residual.hip; the residual normal of NVAE, Vahdat & Kautz
 * 2020, section 3.2): d [N,HW,2Z] = (dmu | dlv) in the layout of q above, mu_q = mu_p + dmu, logvar_q = logvar_p + dlv. p, p_bcast, eps,
 * mode, z and the four reductions are as in lvae_normal_stochastic_fwd_f32 (d is required: there is no posterior-free form; kl_spatial may
 * be NULL). Every quantity is formed from the offset, never from the rounded sum: with s_q = exp(lv_p/2) exp(dlv/2), a = z - mu_p and
 * u = (z - mu_q) / s_q,
 *   mode 0: z = (mu_p + dmu) + s_q eps, a = dmu + s_q eps, u = eps;  mode 1: z = mu_p + dmu, a = dmu, u = 0;  mode 2: a = z - mu_p, u = (a - dmu) / s_q
 *   log p = -a^2 exp(-lv_p)/2 - lv_p/2 - log sqrt(2 pi);  log q = -u^2/2 - (lv_p + dlv)/2 - log sqrt(2 pi)
 *   analytical KL = (expm1(dlv) - dlv + dmu^2 exp(-lv_p)) / 2;  Monte-Carlo KL = (a^2 exp(-lv_p) - u^2)/2 - dlv/2
 * q_out [N,HW,2Z] (may be NULL: nothing is written for it) receives (mu_p + dmu | logvar_p + dlv), each rounded once, for the consumers of
 * absolute posterior parameters (lvae_latent_stats_fold_f32). Sums in a fixed order, no atomics: the same inputs give the same bits. */
int lvae_normal_stochastic_res_fwd_f32(const float* p, int32_t p_bcast, const float* d, const float* eps, int32_t N,
                                       int32_t HW, int32_t Z, int32_t mode, int32_t analytical_kl, float* z, float* q_out,
                                       float* logprob_p, float* logprob_q, float* kl_samplewise, float* kl_spatial,
                                       void* stream);
/* Backward of the above; upstream gradients as in lvae_normal_stochastic_bwd_f32 (each may be NULL). z is read in mode 2 only, eps in mode 0
 * only. Writes dd [N,HW,2Z], the gradient of the offset, and dp [N,HW,2Z], the TOTAL gradient of the prior parameters: their own terms plus
 * what flows through q = p + d, formed per term on paper (the caller sums dp over N when p was broadcast). */
int lvae_normal_stochastic_res_bwd_f32(const float* p, int32_t p_bcast, const float* d, const float* eps, const float* z,
                                       const float* dz, const float* g_lp, const float* g_lq, const float* g_kl,
                                       const float* g_ks, int32_t N, int32_t HW, int32_t Z, int32_t mode,
                                       int32_t analytical_kl, float* dp, float* dd, void* stream);

/* The whole block of the low-resolution levels in one launch (csrc/stoch_img.hip), forward: p_params = conv_in_p(x_p),
 * q_params = conv_in_q(x_q), the elementwise core above, out = conv_out(z). Every tensor the one-kernel-per-op form writes is written:
 *   conv_p   : x = x_p [N,H,W,64], y = p_params [N,H,W,2Z], w / bias of conv_in_p. conv_p.w == NULL: the block has no conv_in_p (top layer);
 *              p_params is then `p_given` ([N,H,W,2Z], or [1,H,W,2Z] with p_bcast = 1) and is only read
 *   conv_q   : x = x_q [N,H,W,64], y = q_params [N,H,W,2Z]
 *   conv_out : x = z [N,H,W,Z] (WRITTEN by this launch), y = out [N,H,W,64]
 * each a forward descriptor as lvae_conv2d_f32 takes it (LVAE_GATHER_CONV, 3x3, stride 1, pad 1, no input / output transform, no
 * statistics), with workspace = lvae_stoch_block_workspace(d) bytes of pre-split weights private to the weight view: filled by the launch
 * itself unless workspace_ready, or by lvae_conv2d_prepare_weights from a table entry written by lvae_stoch_block_prepare_entry.
 * eps, mode, analytical_kl and the four reductions as lvae_normal_stochastic_fwd_f32 (kl_spatial may be NULL; sums in a fixed order).
 * Arithmetic: six exact bf16-piece products per fp32 product (as LVAE_FORM_SIX_PRODUCT) whatever `precision` says.
 * lvae_stoch_block_ok(b) == 1 exactly when the launch takes b: 3x3 / stride 1 / pad 1, 64 input channels, Z = 32, H*W a divisor of 64 (and
 * the tile's patch within the LDS), fp32 tensors, 16-byte aligned operands and weight views, q present, mode 0..2. Otherwise compose lvae_conv2d_f32 and the core.
 * replaces: lib/stochastic.py:45-99 between the two residual chains of a top-down layer. */
typedef struct lvae_stoch_block {
  lvae_conv_desc conv_p, conv_q, conv_out;
  const float* p_given;
  int32_t p_bcast;
  int32_t mode, analytical_kl;
  const float* eps;
  float *logprob_p, *logprob_q, *kl_samplewise, *kl_spatial;
} lvae_stoch_block;
int32_t lvae_stoch_block_ok(const lvae_stoch_block* b);
size_t lvae_stoch_block_workspace(const lvae_conv_desc* d);
int lvae_stoch_block_prepare_entry(const lvae_conv_desc* d, void* entry);
int lvae_stoch_block_fwd_f32(const lvae_stoch_block* b, void* stream);
/* Its backward from d_out in one launch: dz = dgrad(conv_out)(d_out) (+ dz, the upstream gradient of z itself, or NULL) never reaches memory;
 * dp, dq by the formulas of lvae_normal_stochastic_bwd_f32 with its g_lp / g_lq / g_kl / g_ks (each may be NULL); then the two input gradients.
 *   dgrad_out : x = d_out [N,H,W,64]; y unused
 *   dgrad_q   : x = dq [N,H,W,2Z] (WRITTEN by this launch: the weight gradients read it), y = d x_q [N,H,W,64]
 *   dgrad_p   : x = dp [N,H,W,2Z] (WRITTEN), y = d x_p [N,H,W,64]. dgrad_p.w == NULL: no conv_in_p; only dp is written (the caller sums it
 *               over the batch where p was broadcast)
 * each a dgrad descriptor as lvae_conv2d_f32 takes it (LVAE_GATHER_TRANSPOSED, C1 = the convolution's output channels, Cout = its input
 * channels, w_sk / w_sn swapped), with workspace / workspace_ready as in the forward (lvae_stoch_block_workspace / _prepare_entry; private to
 * the weight view AND the direction). p (p_bcast), q, z, eps, mode, analytical_kl: what the forward used and wrote.
 * lvae_stoch_block_bwd_ok(b) == 1 exactly when the launch takes b (the forward's conditions). */
typedef struct lvae_stoch_block_bwd {
  lvae_conv_desc dgrad_out, dgrad_q, dgrad_p;
  const float* p;
  int32_t p_bcast;
  int32_t mode, analytical_kl;
  const float *q, *z, *eps, *dz, *g_lp, *g_lq, *g_kl, *g_ks;
} lvae_stoch_block_bwd;
int32_t lvae_stoch_block_bwd_ok(const lvae_stoch_block_bwd* b);
int lvae_stoch_block_bwd_f32(const lvae_stoch_block_bwd* b, void* stream);

/* Tempered draw from the prior (sampling only; no backward): for row n, t_n = row_temperature ? row_temperature[n] : temperature,
 * z = mu + (t_n * exp(lv/2)) * eps, and z = mu exactly where t_n == 0 (a branch: eps is not read, an infinite sigma gives no NaN).
 * logprob_p[n] = sum over the row of log N(z; mu, exp(lv)) under the UNTEMPERED prior, in a fixed order (deterministic).
 * p [N|1,HW,2Z] and p_bcast as above; eps, z [N,HW,Z]; row_temperature [N] on the device or NULL. eps may be NULL only when
 * row_temperature is NULL and temperature == 0. LVAE_EINVAL: a missing pointer, N, HW or Z <= 0 (or a row past 32-bit indexing), a
 * negative or non-finite `temperature`; per-row values are the caller's responsibility. 16-byte loads and stores when Z % 4 == 0 and
 * p, eps, z are 16-byte aligned, else a scalar map. */
int lvae_normal_prior_sample_f32(const float* p, int32_t p_bcast, const float* eps, float temperature,
                                 const float* row_temperature, int32_t N, int32_t HW, int32_t Z, float* z, float* logprob_p,
                                 void* stream);

/* Interpolation between two sets of latent rows (sampling only; no backward). za, zb [B,n] contiguous rows, t [T] on the device (any
 * finite value is legal, extrapolation uses the same formulas; the values are NOT validated: they are the caller's responsibility, like a
 * per-row temperature), out [T*B,n] step-major: row j*B + b = wa * za[b] + wc * zb[b] for step t[j].
 *   mode 0 (lerp):  wa = 1 - t, wc = t.
 *   mode 1 (slerp): wa = sin((1 - t) W) / sin W, wc = sin(t W) / sin W on the unnormalised rows, W = 2 atan2(|a^ - c^|, |a^ + c^|) the angle
 *                   between the rows (a^, c^ the rows over their norms), never acos of a cosine. FALLBACK: a pair with |a| == 0, |c| == 0 or
 *                   sin W < 1e-6 (a zero row, parallel rows, antipodal rows) takes the lerp coefficients at every step.
 * The row sums, W and both coefficients are evaluated in double in a fixed order (no float atomics: the result does not depend on launch
 * timing); each coefficient is rounded once to float and the two products and their sum are float. t == 0 writes za[b] and t == 1 writes
 * zb[b] bit for bit in both modes (a branch: the other row may hold Inf or NaN).
 * workspace: lvae_latent_interp_workspace(B, T) bytes (the [B][T][2] coefficients), owned by the caller. 16-byte loads and stores when
 * n % 4 == 0 and za, zb, out are 16-byte aligned, else a scalar map. Nothing is launched or written on an error: LVAE_EINVAL for a null za,
 * zb, t or out, B, n or T <= 0, T*B rows past 32-bit or T*B*n past 64-bit indexing, a mode outside {0, 1}; LVAE_EWORKSPACE for a workspace
 * that is missing or smaller than the query. */
size_t lvae_latent_interp_workspace(int32_t B, int32_t T);
int lvae_latent_interp_f32(const float* za, const float* zb, const float* t, int32_t B, int64_t n, int32_t T, int32_t mode, float* out,
                           void* workspace, size_t workspace_bytes, void* stream);

/* `kl_elementwise` of NormalStochasticBlock2d.forward (lib/stochastic.py:88-91,108) and kl_normal_mc (lib/stochastic.py:209-226):
 * out[n,pix,c] = log q(z) - log p(z)  (analytical_kl = 0)  or  KL(q || p)  (analytical_kl = 1).  p, q [N|1,HW,2Z] (mu | logvar on
 * the channel axis; *_bcast = 1: one row set shared by the batch), z, out [N,HW,Z]. The backward writes dp, dq [N,HW,2Z] (the
 * caller sums a broadcast operand over N) and, when dz != NULL, dz [N,HW,Z] (zero for the analytical form). */
int lvae_kl_elementwise_fwd_f32(const float* p, int32_t p_bcast, const float* q, int32_t q_bcast, const float* z, int32_t N,
                                int32_t HW, int32_t Z, int32_t analytical_kl, float* out, void* stream);
int lvae_kl_elementwise_bwd_f32(const float* p, int32_t p_bcast, const float* q, int32_t q_bcast, const float* z, const float* g,
                                int32_t N, int32_t HW, int32_t Z, int32_t analytical_kl, float* dp, float* dq, float* dz,
                                void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Likelihood heads (elementwise part; the 3x3 parameter conv is lvae_conv2d_f32)
 * ---------------------------------------------------------------------------------------------------------- */
/* Bernoulli — lib/likelihoods.py:60-78,385-388. logits [N,P] (P = H*W*C), x [N,P] or NULL, u [N,P] uniforms.
 * mean = sigmoid(logits), mode = round(mean), sample = u < mean, ll[n] = sum x*max(log m,-100)+(1-x)*max(log(1-m),-100)
 * dll_dlogits [N,P] (optional) = d ll[n] / d logits. */
int lvae_bernoulli_fwd_f32(const float* logits, const float* x, const float* u, int32_t N, int64_t P, float* mean,
                           float* mode, float* sample, float* ll, float* dll_dlogits, void* stream);
/* Discretized mixture of logistics — lib/likelihoods.py:291-382 (x given in [0,1]; the 2x-1 of :228 is applied here).
 * l [N,HW,10*nmix], x [N,HW,3]; ll [N]; dll_dl [N,HW,10*nmix] optional. */
size_t lvae_dmol_workspace(int32_t N, int32_t HW);
int lvae_dmol_ll_fwd_f32(const float* l, const float* x, int32_t N, int32_t HW, int32_t nmix, float* ll, float* dll_dl,
                         void* workspace, size_t workspace_bytes, void* stream);
/* lib/stochastic.py:141-206 + the (s+1)/2 clamp of lib/likelihoods.py:221-225.
 * u_mix [N,HW,nmix], u_log [N,HW,3] uniforms in (1e-5, 1-1e-5); sample [N,HW,3] in [0,1]. */
int lvae_dmol_sample_f32(const float* l, const float* u_mix, const float* u_log, int32_t N, int32_t HW, int32_t nmix,
                         float* sample, void* stream);
/* Gaussian head — lib/likelihoods.py:81-114 + log_normal :391-411. params [N,P,2C] (P = H*W; mean = channels [0,C),
 * logvar = [C,2C)), x / eps / sample [N,P,C]. sample = mean + exp(logvar/2)*eps; ll[n] = sum -0.5((x-mean)^2/var + logvar + log 2pi).
 * dll_dparams [N,P,2C] optional. */
int lvae_gaussian_fwd_f32(const float* params, const float* x, const float* eps, int32_t N, int64_t P, int32_t C,
                          float* sample, float* ll, float* dll_dparams, void* stream);
/* Discretized logistic head (256 bins) — lib/likelihoods.py:117-180 + log_discretized_logistic :233-288 and the sampler
 * logistic_rsample lib/stochastic.py:115-138. raw [N,P,2C] conv output; mean = raw_mean + 0.5, logscale = max(raw_ls - 1, -7)
 * (both [N,P,C], optional outputs); u uniforms in (1e-7, 1-1e-7); x is rescaled by 255/256 + 1/512 inside (:172).
 * dll_draw [N,P,2C] optional: gradient w.r.t. the RAW conv output. */
int lvae_discr_logistic_fwd_f32(const float* raw, const float* x, const float* u, int32_t N, int64_t P, int32_t C, float* mean,
                                float* logscale, float* sample, float* ll, float* dll_draw, void* stream);
/* Masked forms of the four heads above: score an image on the pixels it has, and complete it.
 * mask [N,HW] bytes, one flag per PIXEL shared by its colour channels (the DMoL colours of a pixel are coupled: a per-channel flag has no
 * meaning there); non-zero (any of 1..255) = observed. filled [N,HW,C] or NULL. Every other argument is that of the unmasked form; the
 * Bernoulli form also takes C, because its P = HW*C does not say where a pixel ends (LVAE_EINVAL unless C > 0 and P % C == 0), and the
 * DMoL form takes `sample`, the output of lvae_dmol_sample_f32 on the same l and uniforms (the draw of the unmasked path, made by the launch
 * the head issues anyway), from which it writes filled inside the ll launch; `sample` may be NULL when filled is.
 *   ll[n]   the sum of the unmasked kernel's per-element terms over the observed pixels of image n, in the same fixed order (the kernels
 *           are the unmasked ones instantiated with a mask: the thread map and the reduction order are theirs). No pixel observed: +0.0f.
 *   dll     exactly +0.0f at every parameter of a missing pixel: a branch, not a product. x is NOT READ at a missing pixel (it may hold
 *           NaN there), and parameters that are NaN or Inf at a missing pixel leave ll and every other dll element as they were.
 *   mean, mode, logscale, sample: written at every pixel as by the unmasked form, from the same noise.
 *   filled  x where observed, the head's sample where missing (from the same u / eps, so it needs them even when `sample` is NULL).
 *           filled MAY ALIAS x (in-place completion): each thread reads its element of x before it writes that element of filled, and no
 *           thread reads another's. It may not alias any other argument.
 * With every pixel observed ll, dll and the pictures are bit for bit those of the unmasked entry point, and filled == x.
 * Nothing is launched or written on an error: LVAE_EINVAL for a null mask, a null x or ll, and everything the unmasked form refuses;
 * LVAE_EWORKSPACE as in lvae_dmol_ll_fwd_f32 (workspace: lvae_dmol_workspace(N, HW) bytes). */
int lvae_bernoulli_masked_fwd_f32(const float* logits, const float* x, const float* u, int32_t N, int64_t P, int32_t C, float* mean,
                                  float* mode, float* sample, float* ll, float* dll_dlogits, const uint8_t* mask, float* filled,
                                  void* stream);
int lvae_dmol_ll_masked_fwd_f32(const float* l, const float* x, int32_t N, int32_t HW, int32_t nmix, float* ll, float* dll_dl,
                                void* workspace, size_t workspace_bytes, const uint8_t* mask, const float* sample, float* filled,
                                void* stream);
int lvae_gaussian_masked_fwd_f32(const float* params, const float* x, const float* eps, int32_t N, int64_t P, int32_t C, float* sample,
                                 float* ll, float* dll_dparams, const uint8_t* mask, float* filled, void* stream);
int lvae_discr_logistic_masked_fwd_f32(const float* raw, const float* x, const float* u, int32_t N, int64_t P, int32_t C, float* mean,
                                       float* logscale, float* sample, float* ll, float* dll_draw, const uint8_t* mask, float* filled,
                                       void* stream);
/* out = mask ? a : (b ? b : b_value), element by element, exactly (a select: the value not taken may be NaN). mask [N,HW] as above; a, b
 * (or NULL: the scalar b_value everywhere) and out are [N,C,HW] when nchw != 0, else [N,HW,C]. out MAY ALIAS a or b: each thread reads its
 * elements before it writes them. 16-byte loads and stores when a, b and out are 16-byte aligned and HW % 4 == 0 (nchw) or N*HW*C % 4 == 0
 * (channel-last), else a scalar map. Nothing is launched or written on an error: LVAE_EINVAL for a null a, mask or out, N, C or HW <= 0,
 * N*C*HW past 64-bit byte offsets. */
int lvae_mask_select_f32(const float* a, const float* b, float b_value, const uint8_t* mask, int32_t N, int32_t C, int64_t HW,
                         int32_t nchw, float* out, void* stream);
/* out[n, i] = g[n] * a[n, i]  (chain rule through a per-sample scalar; backward of the two heads above) */
int lvae_scale_per_sample_f32(const float* a, const float* g, int32_t N, int64_t P, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Resampling / geometry
 * ---------------------------------------------------------------------------------------------------------- */
/* bilinear x2, align_corners=False — boilr.nn.Interpolate(scale=2) at models/lvae.py:143-144 (restated, unpinned) */
int lvae_upsample2x_fwd_f32(const float* x, int32_t N, int32_t H, int32_t W, int32_t C, float* y, void* stream);
int lvae_upsample2x_bwd_f32(const float* dy, int32_t N, int32_t H, int32_t W, int32_t C, float* dx, void* stream);
/* centred zero pad (OH>=H) or centre crop (OH<=H) — boilr pad_img_tensor / crop_img_tensor, models/lvae.py:185,324.
 * Also converts layout: src_nchw / dst_nchw select NCHW vs NHWC on either side. */
int lvae_pad_crop_f32(const float* x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t src_nchw, float* y, int32_t OH,
                      int32_t OW, int32_t dst_nchw, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * KL bookkeeping + free bits — models/lvae.py:192-198 with boilr.nn.free_bits_kl (restated, parity unpinned):
 *   kl [L,N] (layer-major) -> kl_sep[n] = sum_l, kl_avg_layerwise[l] = mean_n,
 *   scalars[0] = kl_loss = sum_l mean_n max(kl, free_bits)   (plain mean when free_bits < 1e-6)
 *   scalars[1] = kl      = mean_n kl_sep
 * bwd: dkl from upstream g_sep [N], g_avg [L], g_scalars [2] (each may be NULL).
 * ---------------------------------------------------------------------------------------------------------- */
int lvae_kl_bookkeeping_fwd_f32(const float* kl, int32_t L, int32_t N, float free_bits, float* kl_sep,
                                float* kl_avg_layerwise, float* scalars, void* stream);
int lvae_kl_bookkeeping_bwd_f32(const float* kl, int32_t L, int32_t N, float free_bits, const float* g_sep,
                                const float* g_avg, const float* g_scalars, float* dkl, void* stream);
/* The same bookkeeping with the KL terms balanced over the layers during the KL warm-up (csrc/kl_balance.hip; NVAE, §3.2):
 *   m_l     = mean_n |kl[l][n]| + 0.01
 *   gamma_l = (m_l / alpha_l) / mean_j (m_j / alpha_j)   while beta < 1, else exactly 1.0f      -> coeff[l], written on every call
 *   scalars[0] = kl_loss = sum_l gamma_l * mean_n c(kl[l][n]),  c the free-bits clamp above; gamma is formed from the unclamped values
 * alpha: device float[L], positive and finite (the caller validates). beta: the step's own, `beta` when step is NULL, else
 * linear_anneal(step[0], 0, 1, anneal_steps) read on the device as lvae_elbo_loss_fwd_anneal_f32 reads it (`beta` is then ignored).
 * kl_sep, kl_avg_layerwise and scalars[1] are the plain numbers with the bits lvae_kl_bookkeeping_fwd_f32 gives them; with beta >= 1
 * scalars[0] has them too. The L-element part is formed in double and rounded once; one workgroup, no atomics: same inputs, same bits.
 * bwd: gamma is a constant of the gradient, read from coeff (never formed again, no beta):
 *   dkl[l][n] = g_sep[n] + g_avg[l]/N + g_scalars[1]/N + [clamp passes] * coeff[l] * g_scalars[0] / N      (each g may be NULL)
 * with coeff all 1.0f, the bits of lvae_kl_bookkeeping_bwd_f32. */
int lvae_kl_balance_fwd_f32(const float* kl, int32_t L, int32_t N, float free_bits, const float* alpha, float beta, const int64_t* step,
                            int64_t anneal_steps, float* kl_sep, float* kl_avg_layerwise, float* scalars, float* coeff, void* stream);
int lvae_kl_balance_bwd_f32(const float* kl, int32_t L, int32_t N, float free_bits, const float* coeff, const float* g_sep,
                            const float* g_avg, const float* g_scalars, float* dkl, void* stream);
/* ELBO / loss assembly — experiment/experiment_manager.py:329-344:
 *   elbo_sep[n] = ll[n] - kl_sep[n]; scalars[0] = loss = mean(-ll) + beta*kl_loss; [1] = elbo; [2] = recons
 * bwd (of `loss` only; elbo/recons are metrics): d_ll[n] = -g/N, d_kl_loss = g*beta, g = g_loss[0] on device. */
int lvae_elbo_loss_fwd_f32(const float* ll, const float* kl_sep, const float* kl_loss, float beta, int32_t N,
                           float* elbo_sep, float* scalars, void* stream);
int lvae_elbo_loss_bwd_f32(const float* g_loss, float beta, int32_t N, float* d_ll, float* d_kl_loss, void* stream);
/* The same pair with beta = linear_anneal(step[0], 0, 1, anneal_steps) read on the device (KL warm-up, experiment_manager.py:340-342):
 * min(max(step / anneal_steps, 0), 1) in double, rounded to float once; 1 when anneal_steps <= 0. step: device int64[1], the number of
 * completed training steps (advanced with lvae_counter_advance, so a captured step replays with a moving beta). */
int lvae_elbo_loss_fwd_anneal_f32(const float* ll, const float* kl_sep, const float* kl_loss, const int64_t* step, int64_t anneal_steps,
                                  int32_t N, float* elbo_sep, float* scalars, void* stream);
int lvae_elbo_loss_bwd_anneal_f32(const float* g_loss, const int64_t* step, int64_t anneal_steps, int32_t N, float* d_ll,
                                  float* d_kl_loss, void* stream);

/* Training on the K-sample importance-weighted bound (Burda et al.; the reference trains on the single-sample ELBO only, so
 * there is no call site to name). Rows are sample-major, row n = k*B + b for sample k of image b, the layout of lvae_iw_logmeanexp_f32.
 *   lw[k][b]   = ll - beta*kl_sep                                   log weight of a row
 *   bound[b]   = max_k lw + log sum_k exp(lw - max) - log K         [B]
 *   w[k][b]    = exp(lw - max) / sum_k exp(lw - max)                [K*B], the self-normalised weights the backward reads
 *   elbo_sep[n] = ll[n] - kl_sep[n]                                 [K*B], as lvae_elbo_loss_fwd_f32 writes it
 *   scalars[0] = loss = -mean_b bound[b]
 *          [1] = elbo = mean over the K*B rows of ll - kl_sep (the single-sample ELBO)     [2] = recons = mean of -ll
 *          [3] = iw = mean_b logmeanexp_k(ll - kl_sep), the bound at beta = 1              [4] = ess = mean_b 1 / sum_k w^2
 * One workgroup, one thread per image striding over k, double arithmetic, sums in a fixed order and no atomics: the same inputs give the
 * same bits, launched eagerly or replayed. A row with lw = -inf among finite ones gets weight exactly 0; an image whose rows are all
 * -inf (or hold +inf) gets torch.logsumexp's bound and torch.softmax's NaN weights. K, B <= 0 or K*B > INT32_MAX: LVAE_EINVAL.
 * bwd (of `loss` only; the other outputs are metrics): d_ll[n] = -g*w[n]/B, d_kl_sep[n] = g*beta*w[n]/B, g = g_loss[0] on device;
 * with K = 1 that is exactly -g/B and g*beta/B.
 * The *_anneal_* pair reads beta = linear_anneal(step[0], 0, 1, anneal_steps) on the device exactly as lvae_elbo_loss_fwd_anneal_f32 does. */
int lvae_iw_loss_fwd_f32(const float* ll, const float* kl_sep, float beta, int32_t K, int32_t B, float* elbo_sep, float* w, float* bound,
                         float* scalars, void* stream);
int lvae_iw_loss_bwd_f32(const float* g_loss, const float* w, float beta, int32_t K, int32_t B, float* d_ll, float* d_kl_sep,
                         void* stream);
int lvae_iw_loss_fwd_anneal_f32(const float* ll, const float* kl_sep, const int64_t* step, int64_t anneal_steps, int32_t K, int32_t B,
                                float* elbo_sep, float* w, float* bound, float* scalars, void* stream);
int lvae_iw_loss_bwd_anneal_f32(const float* g_loss, const float* w, const int64_t* step, int64_t anneal_steps, int32_t K, int32_t B,
                                float* d_ll, float* d_kl_sep, void* stream);
/* Broadcast over samples: the bottom-up pass is a deterministic function of the image, so it runs on B images and each level's output
 * (and the image the likelihood reads) is repeated for the K samples: out[k][i] = in[i], 0 <= k < K, i < n (n = elements of the B-image
 * tensor). bwd: din[i] = sum_k dout[k][i] accumulated in fp32 in ascending k, bit for bit the sequential float32 sum. 16-byte accesses
 * with a scalar tail of n % 4 elements; in / out / dout / din 16-byte aligned (LVAE_EALIGN otherwise). fp32 only: under LVAE_PREC_BF16
 * the block outputs that cross this point stay fp32 (LVAE_DT_* above). */
int lvae_repeat_samples_fwd_f32(const float* in, int64_t n, int32_t K, float* out, void* stream);
int lvae_repeat_samples_bwd_f32(const float* dout, int64_t n, int32_t K, float* din, void* stream);

/* Importance-weighted bound — evaluate.py:30,86-87 (the loop is boilr's test_procedure: S forward passes, then
 * logsumexp - log S). elbo [S,N] (sample-major) -> out[n] = log mean_s exp(elbo[s][n]). */
int lvae_iw_logmeanexp_f32(const float* elbo, int32_t S, int32_t N, float* out, void* stream);
/* The same bound accumulated one sample at a time (so that a captured top-down + likelihood graph can be replayed S times):
 * state [3][N] = running max, sum of exp(elbo - max), plain sum. mode 0: initialise; mode 1: fold in elbo [N]; mode 2: iw[n] = max +
 * log(sumexp) - log S and mean[n] = sum / S. */
int lvae_iw_online_f32(const float* elbo, float* state, int32_t N, int32_t mode, int32_t S, float* iw, float* mean, void* stream);
/* Test-pass metrics. lvae_eval_online_f32 keeps per-image double state [5*N + L] across the S samples of a batch: running max and
 * sum of exp of elbo_sep, sums of elbo_sep, -ll and kl_sep, and the per-layer KL summed over the batch (kl_avg_layerwise * N).
 * mode 0: initialise; mode 1: fold in one sample. lvae_eval_totals_f64 adds the finished batch to totals [5 + L] (double):
 * sum of IW bounds, ELBO, recons, KL (each image's mean over the samples), image count, per-layer KL; one workgroup in a fixed
 * order, so totals are reproducible bit for bit. */
int lvae_eval_online_f32(const float* elbo_sep, const float* ll, const float* kl_sep, const float* kl_avg_layerwise, double* state,
                         int32_t N, int32_t L, int32_t mode, void* stream);
int lvae_eval_totals_f64(const double* state, int32_t N, int32_t L, int32_t S, double* totals, void* stream);
/* Latent usage of a test pass: per latent unit (one (pixel, channel) position of a stochastic layer, U = HW * Z of them, in NHWC order
 * u = pixel * Z + channel) the sums over images of the posterior mean, of its square and of the analytical KL(q || p).
 * lvae_latent_stats_fold_f32 adds one batch to sums, device double [3][U] = sum mu_q, sum mu_q^2, sum KL. p and q are the fp32
 * (mu | logvar) tensors lvae_normal_stochastic_fwd_f32 reads: q [N][HW][2Z], p the same or, with p_bcast, [1][HW][2Z] read for every image.
 * The KL of an element is the fp32 expression that kernel sums into kl_spatial (analytical, whatever analytical_kl is); all sums are
 * double. Two launches: partial sums per batch slice into workspace (>= lvae_latent_stats_workspace(N, HW, Z) bytes, 8-byte aligned),
 * then the slices in slice order onto sums; no atomics, so the same inputs give the same bits, launched eagerly or replayed. Null
 * pointers, N, HW or Z <= 0 or a workspace that is too small: LVAE_EINVAL, nothing launched.
 * lvae_latent_stats_finalize_f64 (one workgroup, fixed order): unit_out, device double [3][U] = per unit the mean KL, the mean of mu_q and
 * its population variance sum mu^2 / n - (sum mu / n)^2 clamped at 0; layer_out, device double [4] = units with KL > kl_threshold, units
 * with variance > var_threshold, U, sum over units of the mean KL. n_images <= 0: LVAE_EINVAL. */
size_t lvae_latent_stats_workspace(int32_t N, int32_t HW, int32_t Z);
int lvae_latent_stats_fold_f32(const float* p, int32_t p_bcast, const float* q, int32_t N, int32_t HW, int32_t Z, double* sums,
                               void* workspace, size_t workspace_bytes, void* stream);
int lvae_latent_stats_finalize_f64(const double* sums, int64_t U, int64_t n_images, double kl_threshold, double var_threshold,
                                   double* unit_out, double* layer_out, void* stream);
/* Training-log summaries (boilr's summarizer: the mean of every step's metrics since the last train line), kept on the device.
 * acc: device double [2 + 6 + L], 8-byte aligned:
 *   [0] steps folded   [1] non-finite steps   [2] sum loss   [3] sum elbo   [4] sum recons   [5] sum kl   [6] sum l2   [7] sum grad
 *   [8 + l] sum kl_layers[l], 0 <= l < L <= 64
 * lvae_summary_fold_f64 folds one step: loss, elbo, recons, kl, l2 are device float[1]; kl_layers device float[L] (may be NULL when L = 0);
 * grad_norm device float[1] or NULL; gscale device float[1] or NULL (the 1/world factor lvae_adamax_step_f32 applies; needs grad_norm).
 * Every value is widened to double exactly and added to its slot, so a window's sum is the sequential double sum of the per-step floats in
 * step order, bit for bit, launched eagerly or replayed. The grad slot receives grad_norm[0] * gscale[0] formed in fp32 (grad_norm[0]
 * without gscale, 0 without grad_norm). A step whose loss or grad value is not finite adds 1 to slot [1] and nothing to any other slot; a
 * non-finite value elsewhere (a kl_layers entry, say) is added as it is and shows in that mean only. One launch of one wave: each slot
 * belongs to one thread (thread i owns slot i, with L > 56 also slot i + 64), plain loads and stores, no LDS, no atomics.
 * lvae_summary_take_f64: out[i] = acc[i]; acc[i] = 0 for i < n (1 <= n <= 72; out: device double [n], not acc). Stream-ordered between
 * two steps, so it cannot race a replayed step. */
int lvae_summary_fold_f64(const float* loss, const float* elbo, const float* recons, const float* kl, const float* l2,
                          const float* grad_norm, const float* gscale, const float* kl_layers, int32_t L, double* acc, void* stream);
int lvae_summary_take_f64(double* acc, int32_t n, double* out, void* stream);
/* Gradient accumulation: the mean of a step's metrics over its M micro-passes. One launch of one wave at the end of every micro-pass adds
 * that pass's fp32 scalars, widened to double exactly, into acc (device double [7 + L], 8-byte aligned, zero before the first pass):
 *   [0] loss   [1] elbo   [2] recons   [3] kl   [4] l2   [5] iw   [6] ess   [7 + l] kl_layers[l], 0 <= l < L <= 64
 * and advances count (device int64[1], zero before the first pass). iw and ess may be NULL (their slots then hold 0); kl_layers may be NULL
 * when L = 0. The M-th call writes out[s] = (float)(acc[s] / M) for every slot (out: device float [7 + L], untouched by the calls before
 * it) and clears acc and count, so the next step starts from zero without a launch of its own. A NaN or Inf of any pass reaches the mean
 * of its slot and no other. Each slot belongs to one thread, plain loads and stores, no atomics: the same passes give the same bits,
 * launched eagerly or replayed. M < 1, L outside [0, 64] or a null required pointer: LVAE_EINVAL; misaligned: LVAE_EALIGN; nothing
 * launched. No allocation, no synchronisation. */
int lvae_micro_fold_f64(const float* loss, const float* elbo, const float* recons, const float* kl, const float* l2, const float* iw,
                        const float* ess, const float* kl_layers, int32_t L, int32_t M, double* acc, int64_t* count, float* out,
                        void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Picture grids — torchvision's make_grid (padding 2) + save_image and boilr's img_grid_pad_value, restated from their published
 * behaviour (evaluate.py:33-45, 95-114 and boilr's save_images / generate_and_save_reconstructions write such grids; parity unpinned).
 * Sources are fp32 image sets with C = 1 or 3 (anything else: LVAE_EINVAL), each NCHW contiguous (`*_nhwc` = 0) or NHWC contiguous (1).
 * N is the number of grid images. With b == NULL grid image k is a[k]; with b given N is even, k even is a[k/2] and k odd is b[k/2]
 * (input, reconstruction, input, ...), so each source holds N/2 images.
 * ---------------------------------------------------------------------------------------------------------- */
/* count[0] = how many border values of all N images are < threshold, count[1] = how many are NaN (device int32[2], set here).
 * A border value: the pixel clamped to [0, 1], summed over channels in channel order, divided by C in fp32; taken for rows 0 and H-1 in
 * full and columns 0 and W-1 of rows 1 .. H-2 (n_b = N * (2W + 2 max(H-2, 0)) values). torch.median returns the lower middle element, so
 * "median < t" is "count[0] >= (n_b - 1)/2 + 1 and count[1] == 0" (a NaN makes the median NaN): integer counts, reproducible. */
int lvae_image_border_count_f32(const float* a, int32_t a_nhwc, const float* b, int32_t b_nhwc, int32_t N, int32_t C, int32_t H,
                                int32_t W, float threshold, int32_t* count, void* stream);
/* grid: uint8 [Hg][Wg][3], xmaps = min(nrow, N), ymaps = ceil(N / xmaps), Hg = (H+2)*ymaps + 2, Wg = (W+2)*xmaps + 2; grid_bytes must be
 * Hg*Wg*3 (else LVAE_EINVAL). Image k at row (k / xmaps)*(H+2) + 2, column (k % xmaps)*(W+2) + 2; all other pixels, unfilled cells
 * included, carry the padding value. One channel is replicated to three. byte = trunc(clamp(v*255 + 0.5, 0, 255)) with the product and
 * the sum rounded separately in fp32; NaN -> 0. Padding value: with border_count (the counts above, read on the device: the host never
 * waits for them) 1.0 when the median rule holds and 0.0 otherwise; with border_count == NULL, pad_value. */
int lvae_image_grid_u8(const float* a, int32_t a_nhwc, const float* b, int32_t b_nhwc, int32_t N, int32_t C, int32_t H, int32_t W,
                       int32_t nrow, const int32_t* border_count, float pad_value, uint8_t* grid, int64_t grid_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Device-resident training data (csrc/batch_feed.hip; data.DeviceDataset). The reference feeds each step from a shuffling DataLoader
 * (experiment/data.py:99-106); here the image table stays in HBM and the batch of a step is gathered by one launch inside the step.
 * ---------------------------------------------------------------------------------------------------------- */
#define LVAE_FEED_U8 0   /* src_kind: uint8 values, converted as (float)v / 255.0f (an IEEE division: torch's u8.float().div_(255.0)) */
#define LVAE_FEED_F32 1  /*           float32 values, copied */
/* out [n_rows][C][H][W] float32 (NCHW contiguous, 16-byte aligned): row r is image number
 *   index[(cursor[0] % steps_per_epoch) * B_global + lo + r]   with an index table (device int32 [steps_per_epoch * B_global]; base = 0), or
 *   base + r                                                   with index == NULL (cursor must be NULL too: storage order).
 * src: N images, each CHW contiguous (src_hwc = 0) or HWC contiguous (src_hwc = 1; uint8 only); uint8 tables 4-byte, float32 tables
 * 16-byte aligned. cursor: device int64[1], the number of COMPLETED steps, advanced with lvae_counter_advance as the last launch of a
 * step; NULL = position 0. [lo, lo + n_rows) is this rank's part of the global batch. An index outside [0, N) is never dereferenced: its
 * row comes out as NaN. One thread per four floats and one 16-byte store when C*H*W (for HWC also H*W) is a multiple of 4; element by
 * element otherwise. No allocation, no synchronisation. */
int lvae_batch_gather_f32(const void* src, int32_t src_kind, int32_t src_hwc, int32_t N, int32_t C, int32_t H, int32_t W,
                          const int32_t* index, const int64_t* cursor, int32_t steps_per_epoch, int32_t B_global, int32_t lo,
                          int64_t base, int32_t n_rows, float* out, void* stream);

/* The same gather with the batch augmented on the way (data.FeedAugment). The noise is stateless: Philox4x32-10 words (the generator of
 * lvae_rng_fill_f32; oracle/philox_ref.py restates it) that are a pure function of (seed, P, g, output element), so no counter advances
 * and nothing has to be saved for a resume to repeat them:
 *   P = cursor[0] (the count of completed micro-batches, NOT taken modulo the epoch), or `position` when cursor == NULL (the row of the
 *       index table is then position % steps_per_epoch); g = lo + r, the row's place in the GLOBAL batch; tag = LVAE_AUG_TAG_PIXEL.
 *   With fixed != 0, or with index == NULL: P = 0, g = the image number (base + r without an index table), tag = LVAE_AUG_TAG_FIXED,
 *       and no row is flipped: an image's noise then depends on the seed and its number alone.
 *   Output element e (CHW order) of the row draws word e & 3 of the block with counter e >> 2, stream word g, step word (uint32)P and
 *       key seed ^ (P >> 32 << 32) ^ tag; u = that word through the library's u01, in [2^-25, 1 - 2^-24].
 *   hflip: the row is mirrored in W when bit 31 of word 0 of the block (counter 0, g, (uint32)P, key seed ^ (P >> 32 << 32) ^
 *       LVAE_AUG_TAG_FLIP) is set. The draw belongs to the OUTPUT element: a flip changes only which source pixel is read.
 *   LVAE_AUG_BINARIZE:   out = u < v ? 1.0f : 0.0f, v being what lvae_batch_gather_f32 writes (v = 0 never gives 1, v = 1 always does).
 *   LVAE_AUG_DEQUANTIZE: out = fminf(((float)b + u) * 0.00390625f, 0x1.fffffep-1f) of the byte b, the sum and the product rounded
 *       separately; uint8 tables only (LVAE_EINVAL for float32). The bound is reached: 255 + (1 - 2^-24) rounds to 256 in fp32.
 * With mode = LVAE_AUG_NONE and hflip = 0 the output equals lvae_batch_gather_f32's bit for bit. A flipped row keeps the 16-byte store
 * path when W is a multiple of 4 as well. position >= 0. */
enum { LVAE_AUG_NONE = 0, LVAE_AUG_BINARIZE = 1, LVAE_AUG_DEQUANTIZE = 2 };
#define LVAE_AUG_TAG_PIXEL 0xA1
#define LVAE_AUG_TAG_FLIP 0xA2
#define LVAE_AUG_TAG_FIXED 0xA3
typedef struct lvae_feed_aug {
  uint64_t seed;
  int64_t position;
  int32_t mode;
  int32_t hflip;
  int32_t fixed;
} lvae_feed_aug;
int lvae_batch_gather_aug_f32(const void* src, int32_t src_kind, int32_t src_hwc, int32_t N, int32_t C, int32_t H, int32_t W,
                              const int32_t* index, const int64_t* cursor, int32_t steps_per_epoch, int32_t B_global, int32_t lo,
                              int64_t base, int32_t n_rows, float* out, const lvae_feed_aug* aug, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Nearest neighbours of samples in a table held in HBM (csrc/neighbours.hip; neighbours.NeighbourIndex). Evaluation only.
 * ---------------------------------------------------------------------------------------------------------- */
/* For each of the Q query rows (float32 [Q][D], contiguous) the k rows of `table` ([N][D] contiguous; table_kind LVAE_FEED_U8, an element
 * meaning (float)v / 255.0f as in lvae_batch_gather_f32, or LVAE_FEED_F32) of least squared L2 distance:
 *   dist = sum_i (q_i - t_i)^2, the difference taken first, accumulated in fp32 in one order per D (never |q|^2 + |t|^2 - 2 q.t), so a
 *   query equal to a row gives exactly 0.0f, and a pair's bits depend on the two rows, D and table_kind alone: not on Q, N, k, exclude,
 *   or the position and alignment of either row.
 * index_out / dist_out [Q][k]: ascending by (distance, row), so equal distances go to the lower row; a NaN distance ranks after +inf,
 * then by row. With fewer than k eligible rows the trailing slots hold (-1, +inf). exclude: NULL, or device int32 [Q], a row this query
 * skips (an entry outside [0, N), -1 by convention, skips nothing and is never used as an address). The element order inside a row is
 * the caller's business as long as queries and table agree. Limits: 1 <= k <= 32, Q >= 1, 1 <= N <= INT32_MAX, D >= 1, Q*k <= INT32_MAX.
 * workspace: lvae_nn_l2_workspace(Q, N, k) bytes (0 for sizes outside the limits), 8-byte aligned, owned by the caller; it holds the k
 * best of each group of table rows per query and stays far below Q*N floats. Two launches, no float atomics, no host wait. Nothing is
 * launched or written on an error: LVAE_EINVAL for a null queries, table, index_out or dist_out, a size outside the limits or an unknown
 * kind; LVAE_EWORKSPACE for a missing or short workspace; LVAE_EALIGN for a workspace off 8 bytes or a float32 / int32 buffer off 4. */
size_t lvae_nn_l2_workspace(int32_t Q, int64_t N, int32_t k);
int lvae_nn_l2_f32(const float* queries, int32_t Q, const void* table, int32_t table_kind, int64_t N, int64_t D, const int32_t* exclude,
                   int32_t k, int32_t* index_out, float* dist_out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Image quality of reconstructions: mean squared error, PSNR and SSIM per image (csrc/image_quality.hip; quality.ImageQuality).
 * Evaluation only. The reference has nothing comparable; the yardstick is the published SSIM definition (Wang, Bovik, Sheikh &
 * Simoncelli 2004) evaluated in float64 (tests/image_quality_ref.py).
 * ---------------------------------------------------------------------------------------------------------- */
/* a is the reference image set, b the one judged: fp32, N images of C channels (1 <= C <= 4) and H x W pixels (H, W >= 11), each NCHW
 * contiguous (`*_nhwc` = 0, `*_ld` ignored) or channel-last with a pixel stride of `*_ld` floats (`*_ld` = 0 means C; `*_ld` > C reads a
 * view such as the first C of 2C channels without a copy). Only 4-byte alignment is asked of a and b.
 * mask: NULL, or [N][H][W] bytes; a pixel is COUNTED when (mask != 0) == (count_where != 0). With mask == NULL every pixel is counted.
 * clamp != 0: both images are clamped to [0, data_range] before anything else (x < 0 ? 0 : x > R ? R : x, so a NaN stays a NaN).
 * out [N][3] per image:
 *   mse      the mean over counted pixels and all channels of (a - b)^2: the difference taken first, accumulated in fp32 in one fixed
 *            order per (C, H, W). Uncounted pixels do not enter, so a NaN under the mask changes no bit of it. NaN when nothing is counted.
 *   psnr_db  10 log10(data_range^2 / mse) (formed in double from the fp32 mse, rounded to fp32); +inf when mse == 0, NaN when mse is.
 *   ssim     11 x 11 Gaussian window, sigma 1.5, the 121 weights normalised in double on the host and rounded to fp32; "valid" positions
 *            only, (H - 10)(W - 10) per channel; C1 = (0.01 R)^2, C2 = (0.03 R)^2. Per position, with x_c the window's centre pixel,
 *              mu = x_c + sum w (x - x_c)     var = sum w (x - mu)^2     cov = sum w (a - mu_a)(b - mu_b)
 *              ssim = ((2 (mu_a mu_b) + C1)(2 cov + C2)) / (((mu_a^2 + mu_b^2) + C1)((var_a + var_b) + C2))
 *            every product and sum of the ratio rounded separately. The second moments are centred on the window's own means, never
 *            formed as E[x^2] - mu^2, and the mean is taken about the centre pixel, so a constant window has mu == x_c and variance 0.0f
 *            exactly, and a == b bit for bit gives ssim == 1.0f, mse == 0.0f, psnr == +inf. The mean runs over channels and over the
 *            positions whose CENTRE pixel is counted; the windows themselves read every pixel they cover, counted or not (a NaN under
 *            the mask reaches the windows that cover it). NaN when no centre is counted.
 * An image's three outputs depend on its own pixels, C, H, W, its mask and the flags alone: not on N, its place in the batch, the storage
 * order, ld or alignment. One workgroup per (32 x 32 tile of positions, channel, image) reads its 42 x 42 pixels into LDS; its partial
 * sums and counts go to workspace and a second launch adds them per image in (channel, tile) order. No atomics, no host wait.
 * workspace: lvae_image_quality_workspace(N, C, H, W) bytes (0 for sizes outside the limits), 8-byte aligned.
 * Nothing is launched or written on an error: LVAE_EINVAL for a null a, b or out, N <= 0, C outside [1, 4], H or W < 11 (or H, W > 32768),
 * a non-zero ld < C, a non-finite or non-positive data_range; LVAE_EWORKSPACE for a missing or short workspace; LVAE_EALIGN for a
 * workspace off 8 bytes.
 * lvae_image_quality_fold_f64 adds a batch's [N][3] rows to sums (device double [5], 8-byte aligned), in ascending image order, each fp32
 * value widened exactly: sums[0] += N, [1] += mse, [2] += psnr of the images whose psnr is not +inf, [3] += the count of images with
 * mse == 0, [4] += ssim. A NaN is added as it is: it shows in the mean. One workgroup, fixed order, so eager and replayed runs agree bit
 * for bit. Null pointer or N <= 0: LVAE_EINVAL; sums off 8 bytes: LVAE_EALIGN. */
size_t lvae_image_quality_workspace(int32_t N, int32_t C, int32_t H, int32_t W);
int lvae_image_quality_f32(const float* a, int32_t a_nhwc, int64_t a_ld, const float* b, int32_t b_nhwc, int64_t b_ld, const uint8_t* mask,
                           int32_t count_where, int32_t N, int32_t C, int32_t H, int32_t W, float data_range, int32_t clamp, float* out,
                           void* workspace, size_t workspace_bytes, void* stream);
int lvae_image_quality_fold_f64(const float* per_image, int32_t N, double* sums, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Optimiser and norms over the flat parameter arena — torch.optim.Adamax at experiment_manager.py:76-81 and the
 * L2 loop at experiment_manager.py:346-350.
 * ---------------------------------------------------------------------------------------------------------- */
/* step_count: device uint64[1] holding the number of COMPLETED steps (advance it with lvae_counter_advance after the
 * update; both are plain launches, so a captured graph replays them). mask [n] (optional, 0/1): elements with 0 are frozen (parameters that do not require grad). gscale: device float
 * pointer (optional) multiplied into the gradient (1/world_size after a sum all-reduce). */
int lvae_adamax_step_f32(float* p, const float* g, float* exp_avg, float* exp_inf, const float* mask, int64_t n,
                         float lr, float beta1, float beta2, float eps, float weight_decay, const float* gscale,
                         const uint64_t* step_count, void* stream);
/* The same update, and in the same pass an exponential moving average of the updated parameters: ema[i] += (p_new[i] - ema[i]) * (1 - d)
 * (the lerp form, three fp32 roundings) with d = min(decay, (1 + n) / (10 + n)) in fp32, n = step_count[0] = the steps completed BEFORE
 * this one, read on the device, so a captured step replays along the ramp (d = 0.1 at the first step: a young average follows the
 * weights; decay = 0 makes ema a copy of p). ema [n], 16-byte aligned; 0 <= decay < 1. p, exp_avg and exp_inf come out bit for bit as
 * from lvae_adamax_step_f32; elements frozen by `mask` keep their ema as well. One more 16-byte load and store per four elements. */
int lvae_adamax_ema_step_f32(float* p, const float* g, float* exp_avg, float* exp_inf, const float* mask, int64_t n,
                             float lr, float beta1, float beta2, float eps, float weight_decay, const float* gscale,
                             const uint64_t* step_count, float* ema, float decay, void* stream);
/* A learning-rate schedule as a function of the optimizer's own step counter, so that a captured step replays with the lr of the step it
 * runs. n = completed steps (step_count[0] before the update), W = warmup_steps, T = decay_steps, m = min_lr / base_lr, t = n - W:
 *   n <  W:  lr = base_lr * (n + 1) / W                    (linear warm-up: the first step is not zero, step W - 1 reaches base_lr)
 *   n >= W:  lr = base_lr * f, with f by `kind`:
 *     LVAE_LR_CONSTANT  1
 *     LVAE_LR_COSINE    m + (1 - m) * (1 + cos(pi * min(t, T) / T)) / 2
 *     LVAE_LR_LINEAR    1 - (1 - m) * min(t, T) / T
 *     LVAE_LR_STEP      max(m, gamma ^ floor(t / T))
 *     LVAE_LR_EXP       max(m, gamma ^ (t / T))
 * evaluated in double from the exact integer counter and rounded to float once. Valid: base_lr > 0, 0 <= min_lr <= base_lr,
 * 0 < gamma <= 1, warmup_steps >= 0, a known kind, and decay_steps > 0 unless the kind is LVAE_LR_CONSTANT; anything else: LVAE_EINVAL. */
enum { LVAE_LR_CONSTANT = 0, LVAE_LR_COSINE = 1, LVAE_LR_LINEAR = 2, LVAE_LR_STEP = 3, LVAE_LR_EXP = 4 };
typedef struct lvae_lr_schedule {
  float base_lr;
  float min_lr;
  float gamma;
  int32_t kind;
  int64_t warmup_steps;
  int64_t decay_steps;
} lvae_lr_schedule;
/* *lr = the schedule's value at n completed steps. Host only: no GPU, no stream; the function the kernel below runs on the device (host
 * and device libm may round a cos / pow differently: the two agree to one float spacing). */
int lvae_lr_schedule_at(const lvae_lr_schedule* schedule, uint64_t n, float* lr);
/* lvae_adamax_ema_step_f32 with lr = schedule(step_count[0]) computed inside the same kernel (no further launch). `schedule` is a host
 * pointer read at the call: its values travel as a kernel argument, so a captured launch keeps them. ema may be NULL (no average:
 * lvae_adamax_step_f32's update; `decay` is then ignored). lr_out: device float[1] or NULL, receives the lr this step applied. With a
 * LVAE_LR_CONSTANT schedule without warm-up every output is bit for bit that of the unscheduled entry points with lr = base_lr. */
int lvae_adamax_sched_step_f32(float* p, const float* g, float* exp_avg, float* exp_inf, const float* mask, int64_t n,
                               const lvae_lr_schedule* schedule, float beta1, float beta2, float eps, float weight_decay,
                               const float* gscale, const uint64_t* step_count, float* ema, float decay, float* lr_out, void* stream);
/* The gradient guard: clip the gradient by its global norm and / or leave a step out, decided on the device between the gradient exchange
 * and Adamax, so that a captured step replays the decision. lvae_grad_guard_f32 takes the arena's norm and writes this struct (device
 * memory, 8-byte aligned, 32 bytes); the guarded Adamax, lvae_counter_advance_unless and lvae_multi_copy_f32 read it.
 *   norm     sqrt(sum g^2), bit for bit lvae_l2norm_f32's value (before gscale_in)
 *   scale    what Adamax multiplies the gradient by: gscale_in * min(1, max_norm / (norm * gscale_in + 1e-6)), the quotient formed in double
 *            and the product rounded to float once; gscale_in itself without clipping; 0 on a skipped step
 *   skip     1: this step is left out, 0: it is applied
 *   clipped  applied steps with norm * gscale_in > max_norm since the struct was zeroed (cumulative)
 *   skipped  steps left out since then (cumulative) */
typedef struct lvae_grad_guard_state {
  float norm;
  float scale;
  int32_t skip;
  int32_t reserved_;
  uint64_t clipped;
  uint64_t skipped;
} lvae_grad_guard_state;
/* g [n]; gscale_in: device float[1] or NULL (= 1), the factor Adamax would apply; workspace as for lvae_l2norm_f32. With e = norm * gscale_in
 * (formed in fp32: the number lvae_summary_fold_f64 adds to its grad slot) the step is skipped when e is not finite (a NaN or Inf anywhere
 * in g, or a sum of squares beyond fp32) or when skip_threshold >= 0 and e > skip_threshold (0 skips every non-zero gradient, +Inf only
 * the non-finite ones; a negative threshold: non-finite ones only, too). max_norm <= 0, NaN or Inf: no clipping. A step is counted as
 * clipped when it is applied and e > max_norm (e == max_norm still gets the factor max_norm / (max_norm + 1e-6), as from
 * torch.nn.utils.clip_grad_norm_). Two launches: the partial sums of lvae_l2norm_f32, then one workgroup that adds them in the same order,
 * decides, and writes the struct with plain stores from one thread (no atomics). */
int lvae_grad_guard_f32(const float* g, int64_t n, const float* gscale_in, float max_norm, float skip_threshold,
                        lvae_grad_guard_state* state, void* workspace, size_t workspace_bytes, void* stream);
/* The Adamax step under a guard: with guard->skip set every thread returns before its first store (p, exp_avg, exp_inf, ema and lr_out
 * keep their bits); otherwise the gradient is multiplied by guard->scale and every output is bit for bit that of the unguarded entry point
 * of the same options called with gscale -> scale. schedule: NULL (the step runs at `lr`) or a schedule as for lvae_adamax_sched_step_f32
 * (`lr` is then ignored); ema and lr_out optional as there. There is no gscale argument: guard->scale holds it. Advance the step counter
 * with lvae_counter_advance_unless(step_count, 1, &guard->skip). */
int lvae_adamax_guarded_step_f32(float* p, const float* g, float* exp_avg, float* exp_inf, const float* mask, int64_t n, float lr,
                                 const lvae_lr_schedule* schedule, float beta1, float beta2, float eps, float weight_decay,
                                 const uint64_t* step_count, float* ema, float decay, float* lr_out,
                                 const lvae_grad_guard_state* guard, void* stream);
/* A second update rule over the same arena: torch.optim.Adam / torch.optim.AdamW in the single-tensor form (no amsgrad, no maximize), one
 * entry point for every combination the four Adamax entry points cover. exp_avg_sq [n] is the second moment. With n = step_count[0] and
 * t = n + 1 the step's scalars are formed in double from the exact integer counter and the double betas and rounded to float once:
 *   bc1 = 1 - beta1^t, bc2 = 1 - beta2^t, step_size = (float)(lr / bc1), rs = (float)sqrt(bc2)
 * (1 - 0.999f misses 1 - 0.999 by 1.3e-5, which an fp32 bias correction would carry straight into the first update), and so are the
 * element loop's constants (float)(1 - beta1), (float)beta2, (float)(1 - beta2), the floats torch's own scalars round to. lr is the
 * argument, or the schedule's value at n when `schedule` is given (NULL: none; `lr` is then used). Per element not frozen by `mask`:
 *   gg = g * gs;  if !decoupled: gg += weight_decay * p           (L2 decay, torch.optim.Adam)
 *   if decoupled: p *= (float)(1 - (double)lr * weight_decay)     (torch.optim.AdamW: not scaled by gs; a frozen element does not decay)
 *   m += (gg - m) * (1 - beta1);  v = v * beta2 + (1 - beta2) * gg * gg
 *   p -= step_size * m / (sqrt(v) / rs + eps)                     (IEEE sqrt and division)
 * and, with ema (NULL: none), the average's line and ramp of lvae_adamax_ema_step_f32; p, exp_avg and exp_avg_sq are bit for bit those
 * of the call without it. gs is gscale[0] (NULL: 1). guard (NULL: none) has the meaning it has in lvae_adamax_guarded_step_f32: with
 * guard->skip set every thread returns before its first store, lr_out included; otherwise gs is guard->scale. Giving both guard and gscale
 * is LVAE_EINVAL. lr_out: device float[1] or NULL, receives the rate applied, with a schedule or without. LVAE_EINVAL also for a beta
 * outside [0, 1), a negative eps or weight_decay, a decay outside [0, 1) with ema, an invalid schedule; LVAE_EALIGN for n % 4 != 0, an ema
 * off 16 bytes or a guard off 8. Advance the counter as after the Adamax entry points. */
int lvae_adam_step_f32(float* p, const float* g, float* exp_avg, float* exp_avg_sq, const float* mask, int64_t n, float lr,
                       const lvae_lr_schedule* schedule /* or NULL */, double beta1, double beta2, float eps, float weight_decay,
                       int32_t decoupled, const float* gscale /* or NULL */, const uint64_t* step_count, float* ema /* or NULL */,
                       float decay, float* lr_out /* or NULL */, const lvae_grad_guard_state* guard /* or NULL */, void* stream);
/* table: device array of n_entries {dst, src, n}; entry e is copied, dst[0:n] = src[0:n], by workgroup e, when flag == NULL or
 * flag[0] == want (flag: device int32[1], e.g. &guard->skip). The guarded step saves every BatchNorm running statistic into one shadow
 * buffer with it before the forward pass and puts them back after the guard on a skipped step. Entries must not overlap each other. */
typedef struct lvae_copy_entry {
  float* dst;
  const float* src;
  int64_t n;
} lvae_copy_entry;
int lvae_multi_copy_f32(const lvae_copy_entry* table, int32_t n_entries, const int32_t* flag, int32_t want, void* stream);
/* Spectral regularisation of the convolution weights (csrc/spectral.hip; NVAE, §3.2): the penalty lambda * sum_i sigma_i over a table of
 * matrices that lie in the parameter arena, sigma_i estimated by one power-iteration step per call from a persistent vector u_i, by the
 * rule of torch.nn.utils.spectral_norm. Entry i is the row-major matrix A of K rows and Cout contiguous columns at params + param_off
 * (a convolution weight as the arena stores it: K = KH*KW*Cin), its gradient slot of the same layout at grads + grad_off, its u (Cout
 * floats) at u_in / u_out + u_off and its v (K floats) at v_out + v_off. All offsets in elements. */
typedef struct lvae_spectral_entry {
  int64_t param_off;
  int64_t grad_off;
  int64_t K;
  int64_t Cout;
  int64_t u_off;
  int64_t v_off;
} lvae_spectral_entry;
/* For every entry, in one launch (table: device array, 8-byte aligned):
 *   s = A u,  v' = s / max(|s|, 1e-12);   t = A^T v',  u' = t / max(|t|, 1e-12);   sigma = |t|
 *   grads[k][c] += (lambda / gscale[0]) * v'[k] * u'[c]                        (grads NULL: iterate only, no gradient is touched)
 * v' -> v_out, u' -> u_out (u_out may be u_in), sigma -> sigma_out[i]. u' and v' are constants of the gradient, as in torch. gscale: device
 * float[1] or NULL (= 1), the factor the optimizer will multiply the arena by, so that the update sees lambda * v' u'^T. A zero matrix
 * gives v' = u' = 0, sigma = 0 and a zero increment. Sums are fp32 in one fixed order per entry (a workgroup owns an entry; no atomics),
 * the two norms are summed in double: the outputs do not depend on the grid (max_workgroups: 0 = one workgroup per entry). Nothing outside
 * the K * Cout elements of an entry's gradient slot is written. n_params, n_grads, n_u, n_v: the lengths of the four buffers; an entry
 * that does not lie inside them, or has K > 4096 or Cout > 1024, is not touched and gets sigma = NaN. */
int lvae_spectral_step_f32(const lvae_spectral_entry* table, int32_t n_entries, const float* params, int64_t n_params, float* grads,
                           int64_t n_grads, const float* u_in, float* u_out, int64_t n_u, float* v_out, int64_t n_v, float* sigma_out,
                           float lambda, const float* gscale, int32_t max_workgroups, void* stream);
/* out[0] = sum of sigma[0:n_entries] (added in double in a fixed order, rounded once), out[1] = their maximum; a NaN sigma makes both NaN. */
int lvae_spectral_reduce_f32(const float* sigma, int32_t n_entries, float* out, void* stream);
/* BatchNorm recalibration (csrc/bn_recal.hip): running statistics re-estimated for the weights a pass is about to evaluate, by the
 * momentum=None rule of torch.optim.swa_utils.update_bn. With momentum 1 a train-mode forward leaves each BatchNorm's batch mean and
 * unbiased batch variance in its running statistics; a fold after every forward and one finish give their equal-weight means.
 * table: device array of n_entries {stat, acc, n}, 8-byte aligned, laid out like lvae_copy_entry; entry e belongs to workgroup e and each
 * element to one thread of it, so no result depends on the grid and no atomics touch the data. Entries must not overlap each other.
 * count: device int64[2], zero before the first fold: count[0] is the number of folds since the last finish, count[1] belongs to finish
 * (the ticket by which the workgroup that arrives last clears count[0]; it is 0 again when the launch ends).
 *   lvae_bn_recal_fold_f64    acc[i] += (double)stat[i] for every element of every entry, then count[0] += 1: the sequential float64 sum
 *                             of the float32 values, in launch order. A statistic nobody rewrote between folds adds the same value n
 *                             times and comes back from finish bit for bit (n * v and its quotient by n are exact in double; only a
 *                             -0.0 returns as +0.0).
 *   lvae_bn_recal_finish_f32  stat[i] = (float)(acc[i] / count[0]) with count[0] read on the device, then acc[i] = 0 and count[0] = 0;
 *                             flag[0] = 1 (device int32[1], otherwise left alone: the caller clears it) when a value written is not
 *                             finite. With count[0] == 0 nothing is written. Both launches take their numbers from device memory, so
 *                             they can sit in a captured graph that is replayed any number of times. */
typedef struct lvae_bn_recal_entry {
  float* stat;
  double* acc;
  int64_t n;
} lvae_bn_recal_entry;
int lvae_bn_recal_fold_f64(const lvae_bn_recal_entry* table, int32_t n_entries, int64_t* count, void* stream);
int lvae_bn_recal_finish_f32(const lvae_bn_recal_entry* table, int32_t n_entries, int64_t* count, int32_t* flag, void* stream);
/* a[0:n] <-> b[0:n] in one pass (16-byte aligned, not overlapping): the averaged weights exchanged IN PLACE with the trainable prefix of
 * the parameter arena for a test pass and back, so captured graphs and parameter views keep their addresses. */
int lvae_swap_f32(float* a, float* b, int64_t n, void* stream);
/* out[0] = sqrt(sum x^2) ; workspace >= lvae_sumsq_workspace(n) bytes; deterministic two-pass */
size_t lvae_sumsq_workspace(int64_t n);
int lvae_l2norm_f32(const float* x, int64_t n, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * On-device noise (Philox4x32-10). `seed` is a host value; `offset` a device uint64[1] step counter advanced
 * with lvae_counter_advance (a plain launch, so graph replays draw fresh numbers); `stream_id` names the call site.
 * kind: 0 = standard normal, 1 = uniform(lo,hi), 2 = Bernoulli(p=lo) keep-mask scaled by `hi` (Dropout2d: hi=1/(1-p))
 * ---------------------------------------------------------------------------------------------------------- */
int lvae_rng_fill_f32(float* out, int64_t n, int32_t kind, float lo, float hi, uint64_t seed, const uint64_t* offset,
                      uint64_t stream_id, void* stream);
int lvae_counter_advance(uint64_t* counter, uint64_t by, void* stream);
/* counter[0] += by unless flag[0] != 0 (flag: device int32[1]): the Adamax step counter of a guarded step, which stands still on a skipped one. */
int lvae_counter_advance_unless(uint64_t* counter, uint64_t by, const int32_t* flag, void* stream);
/* out[0:n] = value (16-byte aligned out). replaces: optimizer.zero_grad() of boilr's training loop on the flat gradient arena. */
int lvae_fill_f32(float* out, int64_t n, float value, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Gradient exchange of the data-parallel step (the reference itself is single-process): SUM all-reduce of slices of
 * the flat fp32 gradient arena over the ranks of one node through a communicator of our own on librccl (RCCL over xGMI), each bucket on a
 * SIDE stream so that it overlaps the backward kernels still being issued. All calls enqueue work and return; nothing synchronises.
 * Inside a hipGraph capture the fork / join become graph edges and RCCL's kernels graph nodes.
 *   lvae_allreduce_unique_id  rank 0 only: a 128-byte communicator id, to be handed to every rank by the caller (e.g. an eager broadcast)
 *   lvae_allreduce_init       every rank (collective: ncclCommInitRank), with this rank's GPU current; *handle owns the communicator and
 *                             two events
 *   lvae_allreduce_enqueue    buf[0:n] = sum over ranks, enqueued on side_stream behind everything issued on launch_stream so far.
 *                             scratch (n floats) non-NULL: out of place into scratch + copy back — for one-rank rehearsals, where the
 *                             in-place form enqueues nothing; NULL: in place
 *   lvae_allreduce_wait       launch_stream waits for everything enqueued on side_stream so far (call before the optimizer step)
 *   lvae_allreduce_destroy    releases the communicator and the events (NULL is a no-op)
 * librccl_path: the librccl.so of the process (torch ships one: <torch>/lib/librccl.so). Errors: LVAE_E*, a hipError_t, or 1000 + the
 * ncclResult_t; lvae_last_error() has the text.
 * ---------------------------------------------------------------------------------------------------------- */
int lvae_allreduce_unique_id(const char* librccl_path, void* id128);
int lvae_allreduce_init(const char* librccl_path, const void* id128, int32_t world, int32_t rank, void** handle);
int lvae_allreduce_enqueue(void* handle, float* buf, int64_t n, float* scratch, void* launch_stream, void* side_stream);
int lvae_allreduce_wait(void* handle, void* launch_stream, void* side_stream);
int lvae_allreduce_destroy(void* handle);

#ifdef __cplusplus
}
#endif
#endif /* LVAE_HIP_H */
