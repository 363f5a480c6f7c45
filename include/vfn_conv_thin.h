/*
 * V-FloodNet on AMD -- C ABI of libvfn_hip.so, fifth part: the LDS-resident 3x3 convolution of the 32-filter layers.
 *
 * Same conventions as vfn_hip.h (every entry point returns VFN_OK / VFN_ERR_*; `stream` is a hipStream_t); the binding derives
 * its prototypes from this file by the same rule (v-floodnet_amd/_lib.py).  No new structs: the layer is a vfn_conv_desc of
 * vfn_hip.h, which must be included first; VFN_ABI_VERSION of vfn_hip.h covers it.
 *
 *   vfn_conv3x3_thin_f32   out = act((conv3x3(act_in(in)) * scale + shift) + res) for a layer with 32 filters: a workgroup keeps the
 *                          whole filter bank and the 10 x 18 input patch of an 8 x 16 block of output pixels in LDS and walks a list
 *                          of blocks (persistent grid); no split-K, no workspace, no counters (csrc/conv_thin3x3.hip).
 * cfg: workgroups of the persistent grid, 0 .. VFN_THIN3X3_MAX_WGS (0 = 256, one per CU; 8 and more are rounded down to a multiple
 * of 8; never more than there are blocks).  The same products as vfn_conv2d_nhwc_f32 without split-K, summed in the same order.
 *
 * VFN_ERR_ARG, and nothing launched, unless: f32 NHWC, 3x3 / stride 1 / pad 1, Cout = 32 (cout_pad >= 32), Cin 32 or 64; in_ld >= Cin
 * and a multiple of 4, `in` and `w` 16-byte aligned; out_ld >= 32; res (optional) with res_ld >= 32 and res_mod 0 or a multiple of
 * H * W (a residual that repeats every res_mod / (H * W) images); no mask, in_lp, out_lp, w_packed, w_batch_rows, ksplit > 1; every
 * operand below 2 GiB (32-bit buffer offsets).  Any N, H, W.
 */
#ifndef VFN_CONV_THIN_H
#define VFN_CONV_THIN_H

#define VFN_THIN3X3_MAX_WGS 2048

#ifdef __cplusplus
extern "C" {
#endif

int vfn_conv3x3_thin_f32(const vfn_conv_desc* d, int cfg, void* stream);

#ifdef __cplusplus
}
#endif

#endif
