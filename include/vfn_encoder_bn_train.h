/*
 * V-FloodNet on AMD -- C ABI of libvfn_hip.so, eighth part: the EfficientNet-B4 encoder of the bootstrap LinkNet in TRAIN mode:
 * batch-statistics BatchNorm and drop-connect (vfloodnet_amd/linknet_train.py, FullTrainer; train_image_seg.py,
 * freeze_encoder='train').  Everything else of the encoder's forward and backward is vfn_encoder_train.h's.
 *
 * Same conventions as vfn_hip.h (every entry point returns VFN_OK / VFN_ERR_*; `stream` is a hipStream_t; every pointer is a
 * device pointer); the binding derives its prototypes from this file by the same rule (v-floodnet_amd/_lib.py).  No structs:
 * VFN_ABI_VERSION of vfn_hip.h covers it.
 *
 * ---- what `freeze_encoder='train'` means (the definition; torch terms)
 *     model.train()                                   # encoder AND decoder BatchNorms on batch statistics, drop-connect on
 *     optimizer = torch.optim.Adam([dict(params=model.parameters(), lr=init_lr)])
 *     per batch:  pr = model(x); loss = DiceLoss()(pr, y); optimizer.zero_grad(); loss.backward(); optimizer.step()
 * The encoder's BatchNorms have eps 1e-3 and momentum 0.01 (efficientnet_pytorch: 1 - batch_norm_momentum, 0.99).  Per
 * BatchNorm over the M = N h w rows of a channel: mean and BIASED variance normalise; running_mean and running_var move by the
 * momentum, the variance as M / (M - 1) times the biased one; num_batches_tracked counts.  M < 2 is an error, as in torch.
 * Drop-connect: block i of 32 has rate p_i = 0.2 i / 32 and applies it only where the block is residual (stride 1, cin == cout)
 * and p_i > 0:  branch = branch / (1 - p_i) * floor(1 - p_i + u[n]),  one u[n] uniform in [0, 1) per image and block, then + x.
 * The table keep[block][n] (0 or 1 / (1 - p_i)) is drawn on the host and reaches the kernels as a device vector [B] per block.
 * The same 465 tensors as under 'statistics' receive a gradient; the encoder's 95 x 2 running statistics and 95 counters move.
 *
 * ---- one batch-statistics BatchNorm (z the raw convolution output, g = dL/dy)
 *     xh = (z - mean) rstd      y = gamma xh + beta      rstd = 1 / sqrt(var + eps)
 *     dbeta = sum g             dgamma = sum g xh        g_z = gamma rstd (g - dbeta / M - xh dgamma / M)
 * gamma rstd (`fold`) goes where vfn_encoder_train.h puts it: into the packed data-gradient filters, the depthwise data-gradient
 * filter and the rows of the weight gradients.  The activation-sized work that is new in the backward is the centring
 *     g' = g - dbeta / M - xh dgamma / M
 * between vfn_et_colsums_f32 and the weight and data gradients.  Under drop-connect the gradient that enters the project
 * convolution's BatchNorm is keep[n] g; the block's pass-through stays g.
 *
 * ---- tensors and determinism: those of vfn_encoder_train.h.  NHWC f32 matrices [M][ld], C >= 4 a multiple of 4 with NO upper
 * limit, ld >= C a multiple of 4, pointers 16-byte aligned, columns C .. ld-1 neither read nor written, a padded channel (z = 0,
 * gamma = beta = 0) stays 0.  No atomics; equal inputs give equal bits; no entry point synchronises, allocates or copies.
 *
 * vfn_et_bn_stats_f32     per channel c < C over the M rows of z: mean, the biased variance var, and
 *         rstd[c] = 1 / sqrt(var + eps)      nshift[c] = -mean rstd      fold[c] = gamma[c] rstd
 *     (computed in float64, stored as float32), and for c < c_run (0 <= c_run <= C; the unpadded channels) the momentum update
 *         running_mean[c] = (1 - momentum) running_mean[c] + momentum mean
 *         running_var[c]  = (1 - momentum) running_var[c]  + momentum var M / (M - 1)
 *     (running_mean / running_var may both be null: nothing moves).  The rows are cut into chunks by vfn_encoder_train.h's rule
 *     with nmax = VFN_ET_MAX_BLOCKS, one workgroup per chunk and group of 64 channels; a thread adds (z - pivot) and
 *     (z - pivot)^2 of its rows in float64, pivot the chunk's first row; the 16 row lanes are added in lane order; a chunk
 *     leaves its mean and its sum of squared deviations in `part`: scratch double [nb][2][C], at most VFN_ET_MAX_BLOCKS * 2 * C;
 *     the second launch combines the chunks by Chan's rule: eight runs of consecutive chunks, each in chunk order, then the runs
 *     in order.  Never E[x^2] - mean^2 in float32.  A channel that is constant over the batch gives var = 0 exactly and
 *     rstd = 1 / sqrt(eps).  M < 2 is VFN_ERR_ARG.  Two launches.
 * vfn_et_bn_norm_f32      one read of z:  xh[b][m][c] = fma(z, rstd[c], nshift[c])  and
 *         y[b][m][c] = act(fma(xh, gamma[c], beta[c])) keep[b] (+ res[b][m][c]),
 *     act = swish when swish != 0, keep [B] (null: 1), res nullable.  xh == z is allowed when ld_xh == ld_z.  One launch.
 * vfn_et_bn_sums_f32      dbeta[c] = sum_b keep[b] sum_g[b][c]  and  dgamma[c] = sum_b keep[b] sum_ga[b][c], in image order, in
 *     float64: the per-image sums of vfn_et_colsums_f32 ([B][C] each) finished under the per-image scale, so that the scale
 *     costs no activation pass.  keep [B] (null: 1).  One launch.
 * vfn_et_bn_center_f32    gp[b][m][c] = keep[b] g[b][m][c] - dbeta[c] / (B M) - xh[b][m][c] dgamma[c] / (B M); dbeta and dgamma
 *     the sums of keep[b] g and keep[b] g xh over all B M rows.  keep [B] (null: 1).  gp == g is allowed only when keep is null and
 *     ld_gp == ld_g: a residual block needs g untouched for its pass-through.  One launch.
 * Every entry returns VFN_ERR_ARG, and launches nothing, for a null pointer it needs, a size below 1 (more than 2^30 rows or
 * 2^31 - 1 elements), C < 4, C % 4, a leading dimension below C or no multiple of 4, c_run outside 0 .. C, one running pointer
 * without the other, eps <= 0, a momentum outside [0, 1], or an in-place call outside the rules above.
 */
#ifndef VFN_ENCODER_BN_TRAIN_H
#define VFN_ENCODER_BN_TRAIN_H

#ifdef __cplusplus
extern "C" {
#endif

int vfn_et_bn_stats_f32(const float* z, int M, int C, int ld, const float* gamma, double eps, double momentum, double* part, float* rstd,
                        float* nshift, float* fold, float* running_mean, float* running_var, int c_run, void* stream);
int vfn_et_bn_norm_f32(const float* z, const float* rstd, const float* nshift, const float* gamma, const float* beta, const float* keep,
                       const float* res, float* xh, float* y, int B, int M, int C, int ld_z, int ld_res, int ld_xh, int ld_y, int swish,
                       void* stream);
int vfn_et_bn_sums_f32(const float* sum_g, const float* sum_ga, const float* keep, float* dbeta, float* dgamma, int B, int C, void* stream);
int vfn_et_bn_center_f32(const float* g, const float* xh, const float* keep, const float* dbeta, const float* dgamma, float* gp, int B, int M,
                         int C, int ld_g, int ld_xh, int ld_gp, void* stream);

#ifdef __cplusplus
}
#endif

#endif
