/*
 * V-FloodNet on AMD -- C ABI of libvfn_hip.so, third part: scoring LinkNet checkpoints on a labelled set (the validation half of
 * train_image_seg.py: WaterDataset_RGB's samples, smp's DiceLoss and IoU, one ValidEpoch).
 *
 * Same conventions as vfn_hip.h (every entry point returns VFN_OK / VFN_ERR_*; `stream` is a hipStream_t; device pointers
 * unless a parameter is called a host array below); the binding derives its prototypes from this file by the same rule
 * (v-floodnet_amd/_lib.py).  No structs: VFN_ABI_VERSION of vfn_hip.h covers it.  The size caps are vfn_hip.h's
 * VFN_TRAIN_AUG_MAX_SIDE (source sides) and VFN_TRAIN_AUG_MAX_OUT (S).
 *
 * ---- one sample of WaterDataset_RGB(mode='train_offline') (image_module/dataset_water.py:136-153, image_module/transforms.py)
 * from one decoded photograph src uint8 [H][W][3] and its palette-index plane label uint8 [H][W]; the photographs of a batch have
 * different sizes, so every entry takes one photograph.  The arithmetic is Pillow's (12.2.0), restated operation by operation
 * (the rules of the vfn_train_aug_* block of vfn_hip.h hold word for word where this block names them); no fused multiply-adds;
 * every byte equals Pillow's, every float the f32 expression given.  The host draws the parameters and builds the tables
 * (vfloodnet_amd/image_dataset.py).  The order is the image module's own: colour, affine, flip, crop.
 *
 * vfn_imgval_jitter   jit [H][W][3] = the colour step: brightness, then contrast, then hue, in that fixed order, each only when
 *     its switch is non-zero -- an operation that is off does not run at all (a hue round trip with shift 0 is no copy), and with
 *     all three off nothing is launched and jit is left alone (the caller goes on with src).  Brightness and contrast are
 *     vfn_train_aug_jitter's blends (ImageEnhance: degenerate = black / the constant int(sum L / N + 0.5) of the image as it
 *     stands after the brightness step; Blend.c's float arithmetic with its clamps outside 0 <= factor <= 1), hue its HSV round
 *     trip with H = (H + hue_shift) & 255, 0 <= hue_shift <= 255 (the reference's factor 0.1 is the shift int(0.1 * 255) = 25).
 *     lsum: one unsigned 64-bit scratch word for the sum of L (integer atomics), needed when contrast is on.  One launch, or a
 *     memset and two launches with contrast.
 * vfn_imgval_affine_window   win_img [win_h][win_w][3] and win_label [win_h][win_w] (tight rows) = the window rows win_i ..
 *     win_i+win_h-1, columns win_j .. win_j+win_w-1 of hflip(TF.affine(img)) and hflip(TF.affine(label)): the affine map when
 *     affine != 0 (bicubic for the image, nearest for the label: Pillow forces NEAREST on a mode-P image), THEN the horizontal
 *     flip when flip_after != 0.  Only the pixels of the window are evaluated, each exactly as the full transforms compute it.
 *     The flip is not folded into the matrix: window pixel (x, y) of the flipped result is output pixel (xs, y), xs = W - 1 - x,
 *     of the affine transform (xs = x without the flip), and Pillow's own formulas are evaluated at xs -- vfn_train_aug_affine's
 *     bicubic rule in double (xin = m0 (xs + 0.5) + m1 (y + 0.5) + m2, ...), its 16.16 fixed-point rule for the label (xx =
 *     FIX(m2 + m0 0.5 + m1 0.5) + FIX(m1) y + FIX(m0) xs), or, with nearest_tables != 0 (the caller sets it when m1 == m3 == 0,
 *     where Pillow takes ImagingScaleAffine), source column xtab[xs] and row ytab[y] of index tables int32 [W] / [H] (-1: outside,
 *     label 0).  affine == 0 copies pixel (xs, y).  m: host array of 6 doubles, the inverse matrix (output -> source pixel);
 *     every m finite, and on the fixed-point path every corner coordinate below 32768 in magnitude.  One launch.
 * vfn_imgval_resize_norm   Image.resize((S, S), BICUBIC) of a tight image window win_img [h][w][3], then ToTensor and Normalize
 *     into slot b of x float [B][3][S][S]: vfn_train_aug_resize's two 8-bit passes (out = clip8((2^21 + sum k p) >> 22) over the
 *     host's tables, bounds int32 [S][2] and coefficients int32 [S][ksize]; the horizontal result rounded to uint8 in hpass
 *     [h][S][3]), then per channel c x = (float(u8) / 255.0f - mean[c]) / std[c] in f32 -- vfn_imgseg_resize_norm's bits.  mean,
 *     std: host arrays of 3 floats, finite, std != 0.  Two launches.
 * vfn_imgval_label_gather   Image.resize((S, S)) of a tight mode-P plane [h][w] (Pillow: NEAREST, Geometry.c
 *     ImagingScaleAffine): y[b][0][oy][ox] = float(plane[ny[oy]][nx[ox]]) -- the index itself, not a one-hot -- from index
 *     tables int32 [S] the host accumulates (-1 or an index outside the plane: 0), into slot b of y float [B][1][S][S].  The
 *     window of a train_offline sample and the whole plane of a val_offline sample (the label of TF.resize) go the same way.  One
 *     launch.
 * The val_offline image is vfn_imgseg_resize_norm as it stands.
 * Every entry returns VFN_ERR_ARG, and launches nothing, for a null pointer it needs, H, W, h or w outside 1 ..
 * VFN_TRAIN_AUG_MAX_SIDE, S outside 1 .. VFN_TRAIN_AUG_MAX_OUT, b outside 0 .. B-1, a window outside the image, a non-finite
 * factor or matrix entry, or a corner coordinate of 32768 or more on the fixed-point path.
 *
 * ---- scores of a batch (smp 0.2.0's DiceLoss() and IoU(threshold=0.5) as train_image_seg.py:134-137 builds them, stated here
 * as the definition: the package is no dependency, and parity with its f32 summation is not pinned)
 * vfn_seg_scores_f64   pr, gt float [n] (the model's probabilities and the labels of a whole batch, n = B S S), all in float64:
 *         S0 = sum gt pr     S1 = sum pr     S2 = sum gt     S3 = sum gt b     S4 = sum b,     b = (pr > threshold) ? 1 : 0
 *     (the comparison strict and in f32; every product formed in float64, where an f32 x f32 product is exact), then
 *         dice_loss = 1 - (2 S0 + 1) / (S1 + S2 + 1)            iou_score = (S3 + 1e-7) / (S2 + S4 - S3 + 1e-7)
 *     stored as log[t][0] and log[t][1] of the device log double [rows][2]; sums double [5] (optional, may be null) receives S0 ..
 *     S4.  All-zero pr and gt give loss 0 and score 1.  The order of the additions is fixed, so equal inputs give equal bits:
 *     nb = min(ceil(n / VFN_SEG_SCORES_CHUNK), VFN_SEG_SCORES_MAX_BLOCKS) workgroups of 256; workgroup j owns elements j c ..
 *     min((j + 1) c, n) - 1, c = ceil(n / nb); thread i adds elements j c + i, j c + i + 256, ... to its five running sums in that
 *     order; the 64 lanes of a wavefront are added by a butterfly (lane ^ 32, 16, 8, 4, 2, 1), the four wavefronts in wavefront
 *     order; the workgroup's sums go to part[j][0..4] and a second launch adds part[0], part[1], ... in that order.  No
 *     floating-point atomics.  part: scratch double [VFN_SEG_SCORES_MAX_BLOCKS][5].  1 <= n < 2^31, threshold finite, 0 <= t <
 *     rows; else VFN_ERR_ARG and nothing is launched.  Two launches, no host synchronisation.
 */
#ifndef VFN_IMAGE_VAL_H
#define VFN_IMAGE_VAL_H

#define VFN_SEG_SCORES_CHUNK 2048
#define VFN_SEG_SCORES_MAX_BLOCKS 1024

#ifdef __cplusplus
extern "C" {
#endif

int vfn_imgval_jitter(const unsigned char* src, int H, int W, int brightness_on, float brightness, int contrast_on, float contrast,
                      int hue_on, int hue_shift, unsigned char* jit, unsigned long long* lsum, void* stream);
int vfn_imgval_affine_window(const unsigned char* img, const unsigned char* label, int H, int W, int affine, const double* m,
                             int nearest_tables, const int* xtab, const int* ytab, int flip_after, int win_i, int win_j, int win_h,
                             int win_w, unsigned char* win_img, unsigned char* win_label, void* stream);
int vfn_imgval_resize_norm(const unsigned char* win_img, int h, int w, unsigned char* hpass, const int* kx_bounds, const int* kx,
                           int ksize_x, const int* ky_bounds, const int* ky, int ksize_y, float* x, int B, int b, int S,
                           const float* mean, const float* std, void* stream);
int vfn_imgval_label_gather(const unsigned char* plane, int h, int w, const int* nx, const int* ny, float* y, int B, int b, int S,
                            void* stream);
int vfn_seg_scores_f64(const float* pr, const float* gt, int n, float threshold, double* part, double* sums, double* log, int rows,
                       int t, void* stream);

#ifdef __cplusplus
}
#endif

#endif
