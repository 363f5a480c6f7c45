/*
 * V-FloodNet on AMD -- C ABI of libvfn_hip.so, sixth part: fine-tuning the bootstrap LinkNet's decoder and head with the encoder
 * frozen (the training half of train_image_seg.py, vfloodnet_amd/linknet_train.py).
 *
 * Same conventions as vfn_hip.h (every entry point returns VFN_OK / VFN_ERR_*; `stream` is a hipStream_t; every pointer is a
 * device pointer); the binding derives its prototypes from this file by the same rule (v-floodnet_amd/_lib.py).  No structs:
 * VFN_ABI_VERSION of vfn_hip.h covers it.
 *
 * ---- what `freeze_encoder=True` means (the definition; torch terms)
 *     model.train(); model.encoder.eval()
 *     for p in model.encoder.parameters(): p.requires_grad_(False)
 *     optimizer = torch.optim.Adam([dict(params=[p for p in model.parameters() if p.requires_grad], lr=init_lr)])
 *     per batch:  pr = model(x); loss = DiceLoss()(pr, y); optimizer.zero_grad(); loss.backward(); optimizer.step()
 * The encoder runs the inference launch list (folded running statistics, no drop-connect) and receives no gradient.  The 52
 * tensors of decoder.* and segmentation_head.0.* are trained.  The 15 decoder BatchNorms run in training mode: batch mean and
 * biased variance over the M = N h w rows, eps 1e-5; running statistics updated with momentum 0.1, the running variance from
 * the unbiased estimate (M / (M - 1)); a layer with M < 2 is an error.  The loss is vfn_image_val.h's dice_loss over the whole
 * batch tensor, 1 - (2 S0 + 1) / (S1 + S2 + 1).  The optimizer is vfn_adamw_f32 with weight_decay = 0.
 *
 * ---- tensors
 * Activations and gradients are NHWC f32 seen as matrices [M][ld], M = N h w rows, C channels used, C a multiple of 4 (the
 * model pads to multiples of 32), C <= VFN_LNT_MAX_C, every leading dimension >= C and a multiple of 4, every pointer 16-byte
 * aligned.  Columns C .. ld-1 are neither read nor written.  A padded channel (gamma = beta = 0, x = 0) has mean 0 and variance
 * 0 and stays 0 through every kernel.  x below is a RAW convolution output (the convolution run with unit scale; the transposed
 * convolution's bias in its shift), y = BN(x) the normalised tensor.
 *
 * ---- determinism
 * No floating-point atomics.  A sum over the rows is cut into nb = ceil(M / r) chunks of r = ceil(M / min(VFN_LNT_MAX_BLOCKS,
 * ceil(M / 64))) consecutive rows, one workgroup each; inside a workgroup the row lanes are added in lane order; the chunks'
 * results go to `part` and a second launch combines them in a fixed order (8 runs of consecutive chunks, then the runs in
 * order).  Equal inputs give equal bits.  All sums are formed in float64.  No entry point synchronises, allocates or copies.
 *
 * vfn_lnt_bn_stats_f32      per channel c over x [M][ld], 2 <= M: mean and biased variance var by a Chan combination of
 *     (count, mean, M2) triples -- a chunk's triple from sums of (x - pivot) and (x - pivot)^2 in float64, pivot = the chunk's
 *     first row (no E[x^2] - mean^2 in f32 anywhere) -- then, all in float64 and rounded once,
 *         rstd = 1 / sqrt(var + eps)      scale = gamma rstd      shift = beta - mean scale
 *         running_mean = (1 - momentum) running_mean + momentum mean
 *         running_var  = (1 - momentum) running_var  + momentum var M / (M - 1)
 *     mean and rstd [C] are saved for the backward; running_mean / running_var [C] are updated in place (both may be null: no
 *     update).  part: scratch double [VFN_LNT_MAX_BLOCKS][2][C].  M < 2: VFN_ERR_ARG.  Two launches.
 * vfn_lnt_bn_apply_f32      y[m][c] = fma(x[m][c], scale[c], shift[c]), then max(., 0) when relu != 0 (a NaN stays a NaN).
 *     y == x is allowed when ld_y == ld_x.  One launch.
 * vfn_lnt_bn_bwd_reduce_f32 with g' = g [y > 0] (relu != 0; g' = g otherwise), y > 0 decided by re-evaluating
 *     fma(x, scale, shift) > 0 -- the bits of vfn_lnt_bn_apply_f32, so y need not be kept -- and xhat = (x - mean) rstd:
 *         dbeta[c] = sum_m g'[m][c]          dgamma[c] = sum_m g'[m][c] xhat[m][c]
 *     part: scratch double [VFN_LNT_MAX_BLOCKS][2][C].  Two launches.
 * vfn_lnt_bn_bwd_apply_f32  gx = scale (g' - dbeta / M - xhat dgamma / M)  (scale = gamma rstd), in f32.  gx == g is allowed
 *     when ld_gx == ld_g.  One launch.
 * vfn_lnt_head_bwd_f32      the 1x1 head convolution, the sigmoid and the Dice loss backwards in one pass: x [M][ld] the last
 *     decoder activation (32 channels), w [32] the head's weights, pr [M] the probabilities vfn_ln_head_f32 wrote for this x
 *     (the head's bias entered there; it is not needed again), gt [M] the labels, sums = S0 .. S2 as vfn_seg_scores_f64 left them
 *     on the device (no read-back).  With D = S1 + S2 + 1:
 *         dL/dpr_m = -(2 gt_m D - (2 S0 + 1)) / D^2          dz_m = dL/dpr_m pr_m (1 - pr_m)        (float64, rounded once)
 *         g_x[m][c] = dz_m w[c]  ([M][32], tight)     g_w[c] = sum_m dz_m x[m][c]      g_b = sum_m dz_m
 *     part: scratch double [VFN_LNT_MAX_BLOCKS][36].  Two launches.
 * Every entry returns VFN_ERR_ARG, and launches nothing, for a null pointer it needs, M < 1 (statistics: M < 2), C < 4, C % 4,
 * C > VFN_LNT_MAX_C, or a leading dimension below C or no multiple of 4.
 */
#ifndef VFN_IMAGE_TRAIN_H
#define VFN_IMAGE_TRAIN_H

#define VFN_LNT_MAX_BLOCKS 256
#define VFN_LNT_MAX_C 1024

#ifdef __cplusplus
extern "C" {
#endif

int vfn_lnt_bn_stats_f32(const float* x, int M, int C, int ld, const float* gamma, const float* beta, double eps, double momentum,
                         double* part, float* scale, float* shift, float* mean, float* rstd, float* running_mean,
                         float* running_var, void* stream);
int vfn_lnt_bn_apply_f32(const float* x, const float* scale, const float* shift, float* y, int M, int C, int ld_x, int ld_y,
                         int relu, void* stream);
int vfn_lnt_bn_bwd_reduce_f32(const float* g, const float* x, const float* scale, const float* shift, const float* mean,
                              const float* rstd, int M, int C, int ld_g, int ld_x, int relu, double* part, float* dgamma,
                              float* dbeta, void* stream);
int vfn_lnt_bn_bwd_apply_f32(const float* g, const float* x, const float* scale, const float* shift, const float* mean,
                             const float* rstd, const float* dgamma, const float* dbeta, float* gx, int M, int C, int ld_g,
                             int ld_x, int ld_gx, int relu, void* stream);
int vfn_lnt_head_bwd_f32(const float* x, const float* w, const float* pr, const float* gt, const double* sums, int M, int ld,
                         double* part, float* g_x, float* g_w, float* g_b, void* stream);

#ifdef __cplusplus
}
#endif

#endif
