/*
 * V-FloodNet on AMD -- C ABI of libvfn_hip.so, seventh part: the backward of the bootstrap LinkNet's EfficientNet-B4 encoder
 * with its BatchNorm statistics frozen (vfloodnet_amd/linknet_train.py, ModelTrainer; train_image_seg.py,
 * freeze_encoder='statistics').
 *
 * Same conventions as vfn_hip.h (every entry point returns VFN_OK / VFN_ERR_*; `stream` is a hipStream_t; every pointer is a
 * device pointer); the binding derives its prototypes from this file by the same rule (v-floodnet_amd/_lib.py).  No structs:
 * VFN_ABI_VERSION of vfn_hip.h covers it.
 *
 * ---- what `freeze_encoder='statistics'` means (the definition; torch terms)
 *     model.train(); model.encoder.eval()      # encoder: running statistics, no drop-connect; decoder BatchNorms: batch statistics
 *     for p in model.parameters(): p.requires_grad_(True)
 *     optimizer = torch.optim.Adam([dict(params=model.parameters(), lr=init_lr)])
 *     per batch:  pr = model(x); loss = DiceLoss()(pr, y); optimizer.zero_grad(); loss.backward(); optimizer.step()
 * 465 tensors receive a gradient: the 52 of vfn_image_train.h and 413 of encoder.*; encoder._conv_head.weight, encoder._bn1.weight
 * and encoder._bn1.bias are not part of smp's encoder and receive none (no optimizer state, they never move).  The encoder's
 * running statistics and num_batches_tracked do not change; the decoder's move as in vfn_image_train.h.
 *
 * ---- one MBConv block, forwards (x the block's input, every BatchNorm with its running statistics: rstd = 1 / sqrt(var + 1e-3))
 *     xh0 = (conv1x1(x, W_expand) - mean0) rstd0        y0 = gamma0 xh0 + beta0              (absent when expand == 1: y0 = x)
 *     xh1 = (dwconv(act(y0), W_dw) - mean1) rstd1       act = swish (identity when expand == 1: the stem applied it already)
 *     y1  = gamma1 xh1 + beta1                          a1 = swish(y1)
 *     p[n][c] = mean_hw a1      u = W1 p + b1      v = W2 swish(u) + b2      gate = sigmoid(v)      s = gate a1
 *     xh2 = (conv1x1(s, W_project) - mean2) rstd2       out = gamma2 xh2 + beta2 (+ x for a residual block)
 * xh0, xh1, xh2, y0, a1, s and the per-image pooled sums and gates [N][C] are kept for the backward; the squeezed vector swish(u)
 * is recomputed.
 * backwards, g the gradient of `out`:
 *     dbeta2 = sum g                 dgamma2 = sum g xh2                          (vfn_et_colsums_f32)
 *     dW_project = diag(gamma2 rstd2) wgrad(s, g)       g_s = conv1x1(g, (diag(gamma2 rstd2) W_project)^T)
 *     dgate[n][c] = sum_hw g_s a1                                                    (vfn_et_colsums_f32, per image)
 *     dv = dgate gate (1 - gate)     db2 = sum_n dv     dW2 = sum_n dv swish(u)^T
 *     du = (W2^T dv) swish'(u)       db1 = sum_n du     dW1 = sum_n du p^T     dp = W1^T du         (vfn_et_se_bwd_f32)
 *     g_y1 = (g_s gate + dp / (h w)) swish'(y1)         swish'(y) = sig(y) (1 + y (1 - sig(y)))     (vfn_et_swish_bwd_f32)
 *     dbeta1 = sum g_y1              dgamma1 = sum g_y1 xh1
 *     dW_dw = rstd1 gamma1 . vfn_et_dw_wgrad_f32(g_y1, y0)     g_y0 = vfn_et_dw_dgrad_f32(g_y1, gamma1 rstd1 W_dw, y0)
 *     dbeta0 = sum g_y0              dgamma0 = sum g_y0 xh0
 *     dW_expand = diag(gamma0 rstd0) wgrad(x, g_y0)     g_x = conv1x1(g_y0, (diag(gamma0 rstd0) W_expand)^T) (+ g for a residual block)
 * xhat is KEPT, never recovered as (y - beta) / gamma (gamma may be 0).  The per-channel factors gamma rstd are folded into the
 * packed data-gradient filters and into the rows of the weight-gradient results: parameter-sized work, no activation pass.
 * The 1x1 convolutions' data and weight gradients run through vfn_conv2d_nhwc_f32 and vfn_conv_wgrad_f32 of vfn_hip.h.
 *
 * ---- tensors
 * Activations and gradients are NHWC f32 seen as matrices [M][ld], C channels used, C >= 4 a multiple of 4 (the model pads to
 * multiples of 32; NO upper limit on C: the encoder is 2688 channels wide), every leading dimension >= C and a multiple of 4,
 * every pointer 16-byte aligned.  Columns C .. ld-1 are neither read nor written.  A padded channel (zero filter, gamma = beta
 * = 0, zero activations) stays 0 through every kernel.
 *
 * ---- determinism
 * No floating-point atomics.  A sum over M rows is cut into nb = ceil(M / r) chunks of r = ceil(M / min(nmax, ceil(M / 64)))
 * consecutive rows (nmax = VFN_ET_MAX_BLOCKS; vfn_et_colsums_f32 over B images: nmax = max(1, VFN_ET_MAX_BLOCKS / B) per image),
 * one workgroup per chunk and group of 64 channels; a thread adds its rows in float32 (at most ceil(r / 16) of them, in row
 * order), the 16 row lanes are added in lane order in float64, the chunks' float64 results go to `part` and a second launch adds
 * them in chunk order.  Equal inputs give equal bits.  No entry point synchronises, allocates or copies.
 *
 * ---- the depthwise geometry (vfn_ln_dwconv_f32's): input [N][H][W], output [N][Ho][Wo], k in {3, 5}, stride in {1, 2},
 * pad_before zeros in front of the image, output (yo, xo) reads input (yo stride - pad_before + ky, xo stride - pad_before + kx)
 * and whatever falls outside the image is zero.  Accepted: 0 <= pad_before < k and 1 <= Ho <= (H + pad_before - 1) / stride + 1
 * (likewise Wo): every window starts at or before the last input row, i.e. some non-negative padding behind the image produces
 * this Ho.  Anything else is VFN_ERR_ARG.  Maps smaller than the filter are fine (a 5x5 filter on a 2x2 map).
 *
 * vfn_et_affine_f32       y[m][c] = act(fma(x[m][c], scale[c], shift[c])) (+ res[m][c] when res != null), act = swish when
 *     swish != 0.  y == x is allowed when ld_y == ld_x.  One launch.
 * vfn_et_scale_rows_f32   y[b][m][c] = x[b][m][c] gate[b][c]: vfn_ln_scale_rows_f32 out of place (gate's stride is C).  One launch.
 * vfn_et_colsums_f32      per image b of B (M rows each) and channel c: sum_g[b][c] = sum_m g[b][m][c] and
 *     sum_ga[b][c] = sum_m g[b][m][c] a[b][m][c]; both [B][C].  sum_g may be null; a and sum_ga may both be null (plain column
 *     sums).  B <= VFN_ET_MAX_BLOCKS.  part: scratch double [B][nb][2][C], at most VFN_ET_MAX_BLOCKS * 2 * C.  Two launches.
 * vfn_et_se_bwd_f32       the squeeze-excite gate backwards (formulas above).  sum_px [B][Cpad] the per-image column sums of a1
 *     (the pooled vector is sum_px inv_hw, as vfn_ln_se_gate_batch_f32 forms it), dgate [B][Cpad], w1 [sq][C], b1 [sq], w2 [C][sq],
 *     b2 [C] over the UNPADDED channels; dpool [B][Cpad] (the gradient of the pooled MEAN; 0 in channels C .. Cpad-1), dw1 [sq][C],
 *     db1 [sq], dw2 [C][sq], db2 [C], summed over the images in image order.  tmp: scratch float [B][Cpad + 2 sq].
 *     1 <= sq <= VFN_ET_MAX_SQ, 1 <= C <= Cpad, 1 <= B.  Dot products in float64.  Two launches.
 * vfn_et_swish_bwd_f32    gy[b][m][c] = ga swish'(fma(xh[b][m][c], scale[c], shift[c])) with ga = g gate[b][c] + dpool[b][c] inv_hw
 *     (gate and dpool [B][C], both given) or ga = g (both null).  gy == g is allowed when ld_gy == ld_g.  One launch.
 * vfn_et_dwconv_f32       vfn_ln_dwconv_f32 without the swish behind the BatchNorm: out = fma(conv(act(x)), scale, shift), act =
 *     swish when swish_in != 0; run with scale = rstd, shift = -mean rstd it leaves xhat.  One launch.
 * vfn_et_dw_dgrad_f32     the adjoint of the depthwise convolution: gx[n][yi][xi][c] = sum over the taps (ky, kx) and outputs
 *     (yo, xo) with yo stride - pad_before + ky = yi, xo stride - pad_before + kx = xi of g[n][yo][xo][c] w[ky k + kx][c], a
 *     gather in tap order (no atomics); with swish_in != 0 multiplied by swish'(y[n][yi][xi][c]), y the tensor the forward
 *     kernel read (y may be null otherwise).  w [k k][C] tap-major.  Input pixels no window reaches get 0.  One launch.
 * vfn_et_dw_wgrad_f32     dw[ky k + kx][c] = sum_{n, yo, xo} g[n][yo][xo][c] act(a[n][yo stride - pad_before + ky][xo stride -
 *     pad_before + kx][c]), [k k][C] tap-major like the forward filter; act = swish when swish_in != 0 (evaluated once per
 *     input pixel: the sum walks the N H W INPUT rows in chunks).  part: scratch double [nb][k k][C], nb <= VFN_ET_MAX_BLOCKS
 *     the chunk count of M = N H W.  Two launches.
 * vfn_et_stem_f32         vfn_ln_stem_f32 without the swish: x [N][3][H][W] -> out [N][Ho][Wo][ld], channels 0 .. 47 =
 *     fma(conv 3x3 / stride 2, scale, shift), channels 48 .. Cp-1 = 0 (Cp a multiple of 16, 48 <= Cp <= ld).  Ho, Wo under the
 *     depthwise rule with k = 3, stride = 2.  One launch.
 * vfn_et_stem_wgrad_f32   dw[co][ci][ky][kx] = sum_{n, yo, xo} g[n][yo][xo][co] x[n][ci][2 yo - pad_before + ky][2 xo - pad_before
 *     + kx], [48][3][3][3]; g [N Ho Wo][ld_g], 48 channels read.  part: scratch double [nb][1296], nb the chunk count of
 *     M = N Ho Wo.  Rows are added in float32 over 64 rows at a time, then in float64.  Two launches.
 * Every entry returns VFN_ERR_ARG, and launches nothing, for a null pointer it needs, a size below 1 (more than 2^30 rows or
 * 2^31 - 1 elements), C < 4, C % 4, a leading dimension below C or no multiple of 4, k not in {3, 5}, stride not in {1, 2}, or
 * an Ho / Wo outside the rule above.
 */
#ifndef VFN_ENCODER_TRAIN_H
#define VFN_ENCODER_TRAIN_H

#define VFN_ET_MAX_BLOCKS 256
#define VFN_ET_MAX_SQ 256

#ifdef __cplusplus
extern "C" {
#endif

int vfn_et_affine_f32(const float* x, const float* scale, const float* shift, const float* res, float* y, int M, int C, int ld_x,
                      int ld_res, int ld_y, int swish, void* stream);
int vfn_et_scale_rows_f32(const float* x, const float* gate, float* y, int B, int M, int C, int ld_x, int ld_y, void* stream);
int vfn_et_colsums_f32(const float* g, const float* a, int B, int M, int C, int ld_g, int ld_a, double* part, float* sum_g,
                       float* sum_ga, void* stream);
int vfn_et_se_bwd_f32(const float* sum_px, float inv_hw, const float* dgate, const float* w1, const float* b1, const float* w2,
                      const float* b2, float* tmp, float* dpool, float* dw1, float* db1, float* dw2, float* db2, int B, int C, int sq,
                      int Cpad, void* stream);
int vfn_et_swish_bwd_f32(const float* g, const float* gate, const float* dpool, float inv_hw, const float* xh, const float* scale,
                         const float* shift, float* gy, int B, int M, int C, int ld_g, int ld_x, int ld_gy, void* stream);
int vfn_et_dwconv_f32(const float* x, const float* w, const float* scale, const float* shift, float* out, int N, int H, int W, int C,
                      int ld_x, int ld_out, int k, int stride, int pad_before, int Ho, int Wo, int swish_in, void* stream);
int vfn_et_dw_dgrad_f32(const float* g, const float* w, const float* y, float* gx, int N, int H, int W, int C, int ld_g, int ld_y,
                        int ld_gx, int k, int stride, int pad_before, int Ho, int Wo, int swish_in, void* stream);
int vfn_et_dw_wgrad_f32(const float* g, const float* a, double* part, float* dw, int N, int H, int W, int C, int ld_g, int ld_a, int k,
                        int stride, int pad_before, int Ho, int Wo, int swish_in, void* stream);
int vfn_et_stem_f32(const float* x, const float* w, const float* scale, const float* shift, float* out, int N, int H, int W, int Ho,
                    int Wo, int Cp, int ld, int pad_before, void* stream);
int vfn_et_stem_wgrad_f32(const float* g, const float* x, double* part, float* dw, int N, int H, int W, int Ho, int Wo, int ld_g,
                          int pad_before, void* stream);

#ifdef __cplusplus
}
#endif

#endif
