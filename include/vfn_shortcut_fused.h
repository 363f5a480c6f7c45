/*
 * V-FloodNet on AMD -- C ABI of libvfn_hip.so, fourth part: a Bottleneck's shortcut convolution inside its conv3's launch.
 *
 * Same conventions as vfn_hip.h (every entry point returns VFN_OK / VFN_ERR_*; `stream` is a hipStream_t); the binding derives
 * its prototypes from this file by the same rule (v-floodnet_amd/_lib.py).  No new structs: both layers are vfn_conv_desc of
 * vfn_hip.h, which must be included first; VFN_ABI_VERSION of vfn_hip.h covers it.
 *
 *   vfn_conv1x1_shortcut_fused_f32   main.out = act(conv1x1(main.in) * main.scale + main.shift + r),
 *                                    r = act_sc(conv1x1(sc.in sampled at stride sc.stride) * sc.scale + sc.shift)
 * as ONE launch of the persistent 1x1 kernel (vfn_conv1x1_persistent_f32): a unit walks the shortcut's K range, keeps r in
 * registers, walks the main layer's K range from zero accumulators and adds r where the one-layer form loads its residual.  Each
 * output element is the same two fmaf chains and the same two epilogue expressions as the two layers run one after the other
 * WITHOUT split-K; sc.out is never written.  cfg: 0..3, the four tiles of vfn_conv1x1_persistent_f32 with operands requested one K tile
 * ahead (the deeper prefetch does not fit the registers next to the kept shortcut); wgs as there.
 *
 * VFN_ERR_ARG unless: both layers 1x1 / pad 0, main stride 1, shortcut stride 1 or 2; the same M and Cout; Cin a multiple of 32 and
 * in_ld a multiple of 4 (>= Cin) in both; no res, mask, in_lp, out_lp, w_packed, w_batch_rows, ksplit > 1 in either; cout_pad of both
 * covers the configuration's filter tile; every operand below 2 GiB (32-bit buffer offsets).
 */
#ifndef VFN_SHORTCUT_FUSED_H
#define VFN_SHORTCUT_FUSED_H

#ifdef __cplusplus
extern "C" {
#endif

int vfn_conv1x1_shortcut_fused_f32(const vfn_conv_desc* sc, const vfn_conv_desc* main_layer, int cfg, int wgs, void* stream);

#ifdef __cplusplus
}
#endif

#endif
