/*
 * V-FloodNet on AMD -- C ABI of libvfn_hip.so, second part: Winograd F(6x6, 3x3) for the f32 inference layers.
 *
 * Same conventions as vfn_hip.h (every entry point returns VFN_OK / VFN_ERR_*; `stream` is a hipStream_t); the binding derives
 * its prototypes from this file by the same rule (v-floodnet_amd/_lib.py).  No structs: VFN_ABI_VERSION of vfn_hip.h covers it.
 *
 * A 3x3 / stride-1 / pad-1 nn.Conv2d as 64 GEMMs in the transform domain -- 64 values per 6x6 output tile, 1.78 per output,
 * where F(4x4, 3x3) (vfn_winograd_input_f32 ...) spends 36 per 4x4 tile, 2.25 per output.  Points 0, +-1, +-2, +-1/2, inf:
 *   vfn_winograd6_input_f32   V [64][rows_pad][C] = B^T d B per tile (8x8 input patch at stride 6, zeros outside the image; relu:
 *                             max(d, 0) first); tiles in (n, ty, tx) order, N * ceil(H/6) * ceil(W/6) of them, rows_pad >= that;
 *                             rows past the tiles are written as zeros
 *   the GEMMs                 vfn_winograd_gemm_f32 with comps = 64 on U [64][cout_pad][C], U[8i+j] = (G g G^T)[i][j]
 *                             (refresh kind 6 of vfn_refresh_filters_f32 / ops.pack_winograd6_weight)
 *   vfn_winograd6_output_f32  out[n][y][x][co] = act((A^T M A) * scale + shift + res) -- the epilogue of vfn_winograd_output_f32
 * C, Cout multiples of 4; every tensor below 2 GiB.
 */
#ifndef VFN_WINOGRAD6_H
#define VFN_WINOGRAD6_H

#ifdef __cplusplus
extern "C" {
#endif

int vfn_winograd6_input_f32(const float* x, int N, int H, int W, int C, int ld_x, int relu, float* V, int rows_pad, void* stream);
int vfn_winograd6_output_f32(const float* Mb, int rows_pad, int N, int H, int W, int Cout, const float* scale, const float* shift,
                             const float* res, int res_ld, int res_mod, int relu_out, float* out, int out_ld, void* stream);
/* The two transforms exist in two forms that write the same bytes (csrc/conv_winograd.hip): 0 one thread per tile and channel pair,
 * 2 a tile and channel pair over 8 lanes through LDS (1 named a wave-uniform variant of 0 that was measured out and is not built).
 * vfn_winograd6_form: the form a call of that shape takes (C: the input transform's C or the output transform's Cout); -1 for a shape
 * the transforms refuse.  VFN_WINO6_XFORM, read once: 0 / 2 force a form everywhere (1: form 0), unset or "auto" the measured rule.
 * vfn_winograd6_force_form: the same override inside a process (0 / 1 / 2; 3: the measured rule; -1: back to the environment's
 * setting). */
int vfn_winograd6_form(int N, int H, int W, int C, int is_output, int has_res);
int vfn_winograd6_force_form(int form);

#ifdef __cplusplus
}
#endif

#endif
