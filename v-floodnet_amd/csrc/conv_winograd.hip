// Winograd F(4x4, 3x3) around the matrix kernels (round 4): the 3x3 / stride-1 / pad-1 convolutions of the decoder
// (AFB_URR.py:20-30,114-127,191-195: 256 -> 256 filters on 1/4- and 1/8-resolution feature maps, 2/3 of the frame's
// convolution FLOP) as 36 GEMMs in the transform domain -- 36 multiplies per 4x4 output tile and filter pair instead of 144:
//
//     Y = A^T [ (G g G^T) (.) (B^T d B) ] A          d: 6x6 input tile (pad 1), g: 3x3 filter, Y: 4x4 outputs
//
//   vfn_winograd_input_f32    V[xi][tile][c]  = (B^T d B)[xi]   (xi = 6 i + j; ReLU on d first for the pre-activation ResBlocks)
//   the 36 GEMMs              M[xi][tile][co] = sum_c V[xi][tile][c] U[xi][co][c]: ONE launch of the convolution kernels with
//                             batched filters (vfn_conv_desc.w_batch_rows = rows per component), U = G g G^T packed by the host
//   vfn_winograd_output_f32   Y = A^T M A per tile, then the convolution's epilogue: * scale + shift (+ residual) (ReLU)
//
// The same algebra cuDNN applies to the reference's convolutions on its own hardware; it is exact in real arithmetic, in f32
// the transforms add ~1e-6 relative rounding (tests/test_conv_gpu.py holds it against F.conv2d like every other configuration).
// Both transforms are HBM-bound: a thread owns 4 channels of one tile, so every load / store of a wave is a contiguous
// 256-byte to 1-KB row; V and M cost 36/16 of the tensor each way (119 MB each for 2 x 120 x 216 x 256).
#include <atomic>
#include <cstdlib>
#include <cstring>
#include "common.h"
#include "conv_internal.h"
#include "../../include/vfn_hip.h"
#include "../../include/vfn_winograd6.h"
#include "../../include/vfn_shortcut_fused.h"

namespace {

// t = B^T v (6 values)
__device__ __forceinline__ void bt6(const f32x4 (&v)[6], f32x4 (&t)[6]) {
    t[0] = 4.f * v[0] - 5.f * v[2] + v[4];
    t[1] = -4.f * (v[1] + v[2]) + v[3] + v[4];
    t[2] = 4.f * (v[1] - v[2]) - v[3] + v[4];
    t[3] = -2.f * v[1] - v[2] + 2.f * v[3] + v[4];
    t[4] = 2.f * v[1] - v[2] - 2.f * v[3] + v[4];
    t[5] = 4.f * v[1] - 5.f * v[3] + v[5];
}

// Branch-free (round 5): every tap of the 6x6 patch is a raw buffer load whose offset is out of range when the tap falls outside the
// image (the hardware returns zeros), so the 36 loads leave back to back and land together.  (The first form tested the bounds
// per tap: hipcc turned each test into an exec-masked branch with the ReLU behind it -- load, s_waitcnt vmcnt(0), next load: 36
// dependent round trips per thread, 3.6-4.5 TB/s on a kernel that only moves bytes.)
// LPOUT (round 5, the plain-bf16 mode): V is written as bf16 (RNE) -- the operand the reduced-precision GEMM multiplies -- half the bytes
template <bool LPOUT = false>
__global__ __launch_bounds__(256)
void winograd_input_kernel(const float* __restrict__ x, int N, int H, int W, int C, int ld_x, int relu, float* __restrict__ V,
                           int rows_pad) {
    const int th = (H + 3) / 4, tw = (W + 3) / 4;
    const int c4n = C / 4;
    const long long total = (long long)N * th * tw * c4n;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, (int)((size_t)N * H * W * ld_x * 4), 0x00020000);
    const float floor_ = relu ? 0.f : -INFINITY;
    for (long long i = vfn_xcd_block(blockIdx.x, gridDim.x) * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % c4n);
        const int tile = (int)(i / c4n);
        const int tx = tile % tw, ty = (tile / tw) % th, n = tile / (tw * th);
        f32x4 d[6][6];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const int yy = 4 * ty - 1 + a;
#pragma unroll
            for (int b = 0; b < 6; ++b) {
                const int xx = 4 * tx - 1 + b;
                const bool ok = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
                const int off = ok ? (((n * H + yy) * W + xx) * ld_x + c4 * 4) * 4 : 0x7ffffff0;
                d[a][b] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, off, 0, 0));
            }
        }
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = 0; b < 6; ++b)
#pragma unroll
                for (int e = 0; e < 4; ++e) d[a][b][e] = vfn_floor_nan(d[a][b][e], floor_);
        // columns: d <- B^T d, then rows: V = d B
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            f32x4 v[6], t[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) v[a] = d[a][b];
            bt6(v, t);
#pragma unroll
            for (int a = 0; a < 6; ++a) d[a][b] = t[a];
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            f32x4 t[6];
            bt6(d[a], t);
#pragma unroll
            for (int b = 0; b < 6; ++b) {
                if constexpr (LPOUT) {
                    const vfn_bf16x4 h = {(__bf16)t[b][0], (__bf16)t[b][1], (__bf16)t[b][2], (__bf16)t[b][3]};
                    *reinterpret_cast<vfn_bf16x4*>(reinterpret_cast<__bf16*>(V) + ((size_t)(a * 6 + b) * rows_pad + tile) * C + c4 * 4) = h;
                } else {
                    *reinterpret_cast<f32x4*>(V + ((size_t)(a * 6 + b) * rows_pad + tile) * C + c4 * 4) = t[b];
                }
            }
        }
    }
}

// y = A^T m (6 values -> 4)
__device__ __forceinline__ void at6(const f32x4 (&m)[6], f32x4 (&y)[4]) {
    const f32x4 s12 = m[1] + m[2], d12 = m[1] - m[2], s34 = m[3] + m[4], d34 = m[3] - m[4];
    y[0] = m[0] + s12 + s34;
    y[1] = d12 + 2.f * d34;
    y[2] = s12 + 4.f * s34;
    y[3] = d12 + 8.f * d34 + m[5];
}

// Branch-free (round 5): the 36 components are loaded back to back, the residual / mask taps of the 16 output pixels are raw buffer
// loads issued together behind the first transform stage, and the stores are buffer stores whose offset is out of range for pixels
// past the image edge (dropped by the hardware).  (The first form tested every pixel: 16 residual loads with a full wait each.)
template <bool MASK>
__global__ __launch_bounds__(256)
void winograd_output_kernel(const float* __restrict__ Mb, int rows_pad, int N, int H, int W, int Cout,
                            const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ res, int res_ld,
                            int res_mod, int relu_out, float* __restrict__ out, int out_ld, const float* __restrict__ mask, int mask_ld,
                            int mask_after) {
    const int th = (H + 3) / 4, tw = (W + 3) / 4;
    const int c4n = Cout / 4;
    const long long total = (long long)N * th * tw * c4n;
    const int npix = N * H * W;
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(out, 0, (int)((size_t)npix * out_ld * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(res ? res : Mb), 0,
                                                                        res ? (int)((size_t)(res_mod > 0 ? res_mod : npix) * res_ld * 4) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rm = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(MASK ? mask : Mb), 0,
                                                                        MASK ? (int)((size_t)npix * mask_ld * 4) : 0, 0x00020000);
    const float floor_ = relu_out ? 0.f : -INFINITY;
    for (long long i = vfn_xcd_block(blockIdx.x, gridDim.x) * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % c4n);
        const int tile = (int)(i / c4n);
        const int tx = tile % tw, ty = (tile / tw) % th, n = tile / (tw * th);
        f32x4 m[6][6];
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = 0; b < 6; ++b) m[a][b] = *reinterpret_cast<const f32x4*>(Mb + ((size_t)(a * 6 + b) * rows_pad + tile) * Cout + c4 * 4);
        f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
        if (scale) sc = *reinterpret_cast<const f32x4*>(scale + c4 * 4);
        if (shift) sh = *reinterpret_cast<const f32x4*>(shift + c4 * 4);
        f32x4 t[6][4];                            // t = M A  (rows of M through A^T)
#pragma unroll
        for (int a = 0; a < 6; ++a) at6(m[a], t[a]);
        // the 16 pixels of the tile: row index, or -1 past the image edge
        int rowi[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int yy = 4 * ty + a, xx = 4 * tx + b;
                rowi[a][b] = (yy < H && xx < W) ? (n * H + yy) * W + xx : -1;
            }
        f32x4 rv[4][4], mk[MASK ? 4 : 1][MASK ? 4 : 1];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int row = rowi[a][b];
                const int rrow = res_mod > 0 ? row % res_mod : row;
                rv[a][b] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rr, row >= 0 ? (rrow * res_ld + c4 * 4) * 4 : 0x7ffffff0, 0, 0));
                if constexpr (MASK)
                    mk[a][b] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rm, row >= 0 ? (row * mask_ld + c4 * 4) * 4 : 0x7ffffff0, 0, 0));
            }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            f32x4 col[6], y[4];
#pragma unroll
            for (int a = 0; a < 6; ++a) col[a] = t[a][b];
            at6(col, y);
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = y[a][e] * sc[e] + sh[e];
                if constexpr (MASK) {
                    if (!mask_after) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = mk[a][b][e] > 0.f ? v[e] : 0.f;
                    }
                }
                v += rv[a][b];                                     // (zeros without a residual: the resource is empty)
                if constexpr (MASK) {
                    if (mask_after) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = mk[a][b][e] > 0.f ? v[e] : 0.f;
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = vfn_floor_nan(v[e], floor_);
                const int row = rowi[a][b];
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, v), ro,
                                                       row >= 0 ? (row * out_ld + c4 * 4) * 4 : 0x7ffffff0, 0, 0);
            }
        }
    }
}

// ---- Winograd F(6x6, 3x3) for the f32 inference layers: 64 transform-domain values per 36 outputs (1.78 per output) instead of
// F(4x4)'s 36 per 16 (2.25): 21 % fewer rows of V and M, GEMM FLOP and transform bytes before tile rounding.  Points 0, +-1, +-2,
// +-1/2, inf; about twice F(4x4)'s rounding (tests/test_winograd6_gpu.py).  Same load / store form as the kernels above; a thread
// owns TWO channels of a tile (its 8x8 patch is 128 registers), so a wave's loads and stores are contiguous 512-byte rows.
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// t = B^T v (8 values)
__device__ __forceinline__ void bt8(const f32x2 (&v)[8], f32x2 (&t)[8]) {
    const f32x2 e1 = v[2] + v[6] - 4.25f * v[4], o1 = v[1] + v[5] - 4.25f * v[3];
    const f32x2 e2 = v[6] + 0.25f * v[2] - 1.25f * v[4], o2 = 0.5f * v[1] - 2.5f * v[3] + 2.f * v[5];
    const f32x2 e3 = v[6] + 4.f * v[2] - 5.f * v[4], o3 = 2.f * v[1] - 2.5f * v[3] + 0.5f * v[5];
    t[0] = v[0] - v[6] + 5.25f * (v[4] - v[2]);
    t[1] = e1 + o1;
    t[2] = e1 - o1;
    t[3] = e2 + o2;
    t[4] = e2 - o2;
    t[5] = e3 + o3;
    t[6] = e3 - o3;
    t[7] = v[7] - v[1] + 5.25f * (v[3] - v[5]);
}

inline int winograd6_tiles(int N, int H, int W) { return N * ((H + 5) / 6) * ((W + 5) / 6); }

// V [64][rows_pad][C]: rows >= the tile count are written as zeros (the scratch is shared between layers of different shapes).
// Addresses: one VGPR per tensor -- the tap (a, b) of the patch and the component xi are wave-uniform displacements ((a W + b) pixels,
// xi rows_pad C floats), so they ride in the scalar offset of the buffer instructions instead of 64 address registers.
__global__ __launch_bounds__(256, 2)
void winograd6_input_kernel(const float* __restrict__ x, int N, int H, int W, int C, int ld_x, int relu, float* __restrict__ V,
                            int rows_pad) {
    const int th = (H + 5) / 6, tw = (W + 5) / 6, tiles = N * th * tw;
    const int c2n = C / 2;
    const long long total = (long long)rows_pad * c2n;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, (int)((size_t)N * H * W * ld_x * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(V, 0, (int)((size_t)64 * rows_pad * C * 4), 0x00020000);
    const int comp4 = rows_pad * C * 4;                       // bytes per component
    const float floor_ = relu ? 0.f : -INFINITY;
    // (one pass: 64 rows_pad C floats stay below 2 GiB, so the grid always covers every thread's work item -- and a loop would make
    // the compiler keep all the scalar displacements below alive at once)
    const long long i = vfn_xcd_block(blockIdx.x, gridDim.x) * (long long)blockDim.x + threadIdx.x;
    if (i >= total) return;
    {
        const int c2 = (int)(i % c2n);
        const int tile = (int)(i / c2n);
        const int vo = (tile * C + c2 * 2) * 4;
        if (tile >= tiles) {
#pragma unroll
            for (int xi = 0; xi < 64; ++xi) __builtin_amdgcn_raw_buffer_store_b64(u32x2{0u, 0u}, rv, vo, xi * comp4, 0);
            return;
        }
        const int tx = tile % tw, ty = (tile / tw) % th, n = tile / (tw * th);
        const int y0 = 6 * ty - 1, x0 = 6 * tx - 1;
        const int base = (((n * H + y0) * W + x0) * ld_x + c2 * 2) * 4;      // (the patch's first tap; outside the image for edge tiles)
        f32x2 d[8][8];
#pragma unroll
        for (int a = 0; a < 8; ++a) {
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const bool ok = (unsigned)(y0 + a) < (unsigned)H && (unsigned)(x0 + b) < (unsigned)W;
                d[a][b] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rx, ok ? base + (a * W + b) * ld_x * 4 : 0x7ffffff0, 0, 0));
            }
        }
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int b = 0; b < 8; ++b)
#pragma unroll
                for (int e = 0; e < 2; ++e) d[a][b][e] = vfn_floor_nan(d[a][b][e], floor_);
        // columns: d <- B^T d, then rows: V = d B
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            f32x2 v[8], t[8];
#pragma unroll
            for (int a = 0; a < 8; ++a) v[a] = d[a][b];
            bt8(v, t);
#pragma unroll
            for (int a = 0; a < 8; ++a) d[a][b] = t[a];
        }
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            f32x2 t[8];
            bt8(d[a], t);
#pragma unroll
            for (int b = 0; b < 8; ++b) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, t[b]), rv, vo, (a * 8 + b) * comp4, 0);
        }
    }
}

// y = A^T m (8 values -> 6)
__device__ __forceinline__ void at8(const f32x2 (&m)[8], f32x2 (&y)[6]) {
    const f32x2 s12 = m[1] + m[2], d12 = m[1] - m[2], s34 = m[3] + m[4], d34 = m[3] - m[4], s56 = m[5] + m[6], d56 = m[5] - m[6];
    y[0] = m[0] + s12 + s34 + s56;
    y[1] = d12 + 2.f * d34 + 0.5f * d56;
    y[2] = s12 + 4.f * s34 + 0.25f * s56;
    y[3] = d12 + 8.f * d34 + 0.125f * d56;
    y[4] = s12 + 16.f * s34 + 0.0625f * s56;
    y[5] = d12 + 32.f * d34 + 0.03125f * d56 + m[7];
}

// the 64 components are loaded back to back (one address register: the component rides in the scalar offset), the residual taps of
// the 36 output pixels are raw buffer loads issued together behind the first transform stage, the stores are buffer stores whose
// offset is out of range for pixels past the image edge
// RES: with a residual (its 36 taps are 72 more registers: one workgroup per CU instead of two)
template <bool RES>
__global__ __launch_bounds__(256, RES ? 1 : 2)
void winograd6_output_kernel(const float* __restrict__ Mb, int rows_pad, int N, int H, int W, int Cout,
                             const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ res, int res_ld,
                             int res_mod, int relu_out, float* __restrict__ out, int out_ld) {
    const int th = (H + 5) / 6, tw = (W + 5) / 6;
    const int c2n = Cout / 2;
    const long long total = (long long)N * th * tw * c2n;
    const int npix = N * H * W;
    const __amdgpu_buffer_rsrc_t rm = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Mb), 0, (int)((size_t)64 * rows_pad * Cout * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(out, 0, (int)((size_t)npix * out_ld * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(res ? res : Mb), 0,
                                                                        res ? (int)((size_t)(res_mod > 0 ? res_mod : npix) * res_ld * 4) : 0, 0x00020000);
    const float floor_ = relu_out ? 0.f : -INFINITY;
    const int comp4 = rows_pad * Cout * 4;
    // (one pass: 64 rows_pad C floats stay below 2 GiB, so the grid always covers every thread's work item -- and a loop would make
    // the compiler keep all the scalar displacements below alive at once)
    const long long i = vfn_xcd_block(blockIdx.x, gridDim.x) * (long long)blockDim.x + threadIdx.x;
    if (i >= total) return;
    {
        int iw = (int)i;
        const int mo = ((iw / c2n) * Cout + (iw % c2n) * 2) * 4;
        f32x2 m[8][8];
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int b = 0; b < 8; ++b) m[a][b] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rm, mo, (a * 8 + b) * comp4, 0));
        f32x2 t[8][6];                            // t = M A  (rows of M through A^T)
#pragma unroll
        for (int a = 0; a < 8; ++a) at8(m[a], t[a]);
        __builtin_amdgcn_sched_barrier(0);        // (the 36 residual taps go out once M's 128 registers are free, not beside them)
        asm volatile("" : "+v"(iw));              // (... and the tile's coordinates are worked out here, not kept alive beside M)
        const int c2 = iw % c2n, tile = iw / c2n;
        const int tx = tile % tw, ty = (tile / tw) % th, n = tile / (tw * th);
        f32x2 sc = {1.f, 1.f}, sh = {0.f, 0.f};
        if (scale) sc = *reinterpret_cast<const f32x2*>(scale + c2 * 2);
        if (shift) sh = *reinterpret_cast<const f32x2*>(shift + c2 * 2);
        // the 36 pixels of the tile: row0 + a W + b, invalid past the image edge
        const int y0 = 6 * ty, x0 = 6 * tx, row0 = (n * H + y0) * W + x0;
        // (res_mod: the residual repeats every res_mod pixels, a whole number of images -- a tile never wraps)
        const int rb = ((row0 - (res_mod > 0 ? (n * H * W) / res_mod * res_mod : 0)) * res_ld + c2 * 2) * 4;
        f32x2 rv[RES ? 6 : 1][RES ? 6 : 1];
        if constexpr (RES) {
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = 0; b < 6; ++b) {
                    const bool ok = y0 + a < H && x0 + b < W;
                    rv[a][b] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rr, ok ? rb + (a * W + b) * res_ld * 4 : 0x7ffffff0, 0, 0));
                }
        }
        const int oo = (row0 * out_ld + c2 * 2) * 4;
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            f32x2 col[8], y[6];
#pragma unroll
            for (int a = 0; a < 8; ++a) col[a] = t[a][b];
            at8(col, y);
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                f32x2 v;
#pragma unroll
                for (int e = 0; e < 2; ++e) v[e] = vfn_floor_nan(y[a][e] * sc[e] + sh[e] + (RES ? rv[a][b][e] : 0.f), floor_);
                const bool ok = y0 + a < H && x0 + b < W;
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), ro, ok ? oo + (a * W + b) * out_ld * 4 : 0x7ffffff0, 0, 0);
            }
        }
    }
}

// ---- the lane-split form of the F(6x6) transforms ("form 2"; vfn_winograd6_form picks a form per call, the kernels above are form 0).
// Same helpers (bt8 / at8), same order of operations, same epilogue expression: it writes the bytes of form 0
// (tests/test_winograd6_forms_gpu.py).  A tile and 32 channel pairs per workgroup, a tile-and-pair over 8 lanes: lane j loads column j
// of the patch (row j of M) and transforms it, the 8x8 goes through LDS transposed (512 B per pair, 16 KB per workgroup), the lane
// transforms row j (output column j, lanes 0..5) and stores it.  8x the waves of form 0 -- a res4 map is 2000 waves, not 256 -- each
// with an eighth of the instruction stream (34-46 registers, 8 waves per SIMD); a half-wave's loads and stores are contiguous 256-byte
// rows.  Tile coordinates come from the workgroup index, so they are scalar; what is per lane is the column j and the channel pair.
// (Form 1 of the same round -- form 0's thread shape with the tile index through readfirstlane, scalar tap displacements, no per-tap
// test on inner tiles, 3 waves per SIMD -- was 2-8 % faster than form 0 and slower than this one at every shape but one tie: not kept,
// DESIGN.md 3.12.)
constexpr int kW6Oob = 0x7ffffff0;                 // a VGPR offset past every tensor (below 2 GiB): load gives zeros, store is dropped

__device__ __forceinline__ f32x2 w6_load(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
}
__device__ __forceinline__ void w6_store(f32x2 v, __amdgpu_buffer_rsrc_t r, int voff, int soff) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, voff, soff, 0);
}
// the epilogue of winograd6_output_kernel, one pixel of a channel pair
template <bool RES>
__device__ __forceinline__ f32x2 w6_epilogue(const f32x2& y, const f32x2& sc, const f32x2& sh, const f32x2& r, float floor_) {
    f32x2 v;
#pragma unroll
    for (int e = 0; e < 2; ++e) v[e] = vfn_floor_nan(y[e] * sc[e] + sh[e] + (RES ? r[e] : 0.f), floor_);
    return v;
}

// input.  Grid: rows_pad * ceil(C / 64) workgroups; thread = (j = threadIdx.x / 32: patch column, then V row; threadIdx.x % 32:
// channel pair of the group).  LDS image [8][8][32] pairs: a wave writes and reads 512 contiguous bytes per access.
template <bool RELU>
__global__ __launch_bounds__(256)
void winograd6_input_split_kernel(const float* __restrict__ x, int N, int H, int W, int C, int ld_x, float* __restrict__ V, int rows_pad) {
    __shared__ f32x2 lds[64 * 32];
    const int th = (H + 5) / 6, tw = (W + 5) / 6, tiles = N * th * tw;
    const int c2n = C / 2, groups = (c2n + 31) / 32;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, (int)((size_t)N * H * W * ld_x * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(V, 0, (int)((size_t)64 * rows_pad * C * 4), 0x00020000);
    const int comp4 = rows_pad * C * 4;
    const int blk = (int)vfn_xcd_block(blockIdx.x, gridDim.x);
    const int tile = blk / groups, cg = blk - tile * groups;
    const int cp = threadIdx.x & 31, j = threadIdx.x >> 5;
    const int c2 = cg * 32 + cp;
    const bool live = c2 < c2n;                               // (C / 2 no multiple of 32: the last group's spare lanes touch no memory)
    const int vo = live ? (tile * C + c2 * 2) * 4 + j * 8 * comp4 : kW6Oob;      // V: component 8 j of the lane's tile and pair
    if (tile >= tiles) {                                      // (the whole workgroup)
#pragma unroll
        for (int b = 0; b < 8; ++b) w6_store(f32x2{0.f, 0.f}, rv, live ? vo + b * comp4 : kW6Oob, 0);
        return;
    }
    const int tx = tile % tw, ty = (tile / tw) % th, n = tile / (tw * th);
    const int y0 = 6 * ty - 1, x0 = 6 * tx - 1;
    const bool colok = live && (unsigned)(x0 + j) < (unsigned)W;
    const int px4 = ld_x * 4;
    f32x2 v[8], t[8];
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        const bool ok = colok && (unsigned)(y0 + a) < (unsigned)H;
        v[a] = w6_load(rx, ok ? ((n * H + y0 + a) * W + x0 + j) * px4 + c2 * 8 : kW6Oob, 0);
    }
    if constexpr (RELU) {
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int e = 0; e < 2; ++e) v[a][e] = vfn_floor_nan(v[a][e], 0.f);
    }
    bt8(v, t);                                                // column j of B^T d
#pragma unroll
    for (int a = 0; a < 8; ++a) lds[(a * 8 + j) * 32 + cp] = t[a];
    __syncthreads();
#pragma unroll
    for (int b = 0; b < 8; ++b) v[b] = lds[(j * 8 + b) * 32 + cp];
    bt8(v, t);                                                // row j of (B^T d) B
#pragma unroll
    for (int b = 0; b < 8; ++b) w6_store(t[b], rv, live ? vo + b * comp4 : kW6Oob, 0);
}

// output.  Grid: tiles * ceil(Cout / 64) workgroups; lane j transforms row j of M, then (j < 6) output column j of the tile.
template <bool RES>
__global__ __launch_bounds__(256)
void winograd6_output_split_kernel(const float* __restrict__ Mb, int rows_pad, int N, int H, int W, int Cout,
                                   const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ res, int res_ld,
                                   int res_mod, int relu_out, float* __restrict__ out, int out_ld) {
    __shared__ f32x2 lds[64 * 32];
    const int th = (H + 5) / 6, tw = (W + 5) / 6;
    const int c2n = Cout / 2, groups = (c2n + 31) / 32;
    const int npix = N * H * W;
    const __amdgpu_buffer_rsrc_t rm = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Mb), 0, (int)((size_t)64 * rows_pad * Cout * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(out, 0, (int)((size_t)npix * out_ld * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(RES ? res : Mb), 0,
                                                                        RES ? (int)((size_t)(res_mod > 0 ? res_mod : npix) * res_ld * 4) : 0, 0x00020000);
    const float floor_ = relu_out ? 0.f : -INFINITY;
    const int comp4 = rows_pad * Cout * 4;
    const int blk = (int)vfn_xcd_block(blockIdx.x, gridDim.x);
    const int tile = blk / groups, cg = blk - tile * groups;
    const int cp = threadIdx.x & 31, j = threadIdx.x >> 5;
    const int c2 = cg * 32 + cp;
    const bool live = c2 < c2n;
    const int tx = tile % tw, ty = (tile / tw) % th, n = tile / (tw * th);
    const int y0 = 6 * ty, x0 = 6 * tx, row0 = (n * H + y0) * W + x0;
    const bool colok = live && j < 6 && x0 + j < W;           // the lane's output column
    f32x2 m[8], t[6];
    const int mo = (tile * Cout + c2 * 2) * 4 + j * 8 * comp4;
#pragma unroll
    for (int b = 0; b < 8; ++b) m[b] = w6_load(rm, live ? mo + b * comp4 : kW6Oob, 0);
    f32x2 rv[6];
    if constexpr (RES) {
        // (res_mod: the residual repeats every res_mod pixels, a whole number of images -- a tile never wraps)
        const int rb = ((row0 + j - (res_mod > 0 ? (n * H * W) / res_mod * res_mod : 0)) * res_ld + c2 * 2) * 4;
#pragma unroll
        for (int a = 0; a < 6; ++a) rv[a] = w6_load(rr, colok && y0 + a < H ? rb + a * W * res_ld * 4 : kW6Oob, 0);
    }
    f32x2 sc = {1.f, 1.f}, sh = {0.f, 0.f};
    if (scale && live) sc = *reinterpret_cast<const f32x2*>(scale + c2 * 2);
    if (shift && live) sh = *reinterpret_cast<const f32x2*>(shift + c2 * 2);
    at8(m, t);                                                // row j of M A
#pragma unroll
    for (int b = 0; b < 6; ++b) lds[(j * 8 + b) * 32 + cp] = t[b];
    __syncthreads();
    if (j >= 6) return;
#pragma unroll
    for (int a = 0; a < 8; ++a) m[a] = lds[(a * 8 + j) * 32 + cp];
    at8(m, t);                                                // column j of A^T (M A)
    const int oo = ((row0 + j) * out_ld + c2 * 2) * 4;
#pragma unroll
    for (int a = 0; a < 6; ++a)
        w6_store(w6_epilogue<RES>(t[a], sc, sh, rv[a], floor_), ro, colok && y0 + a < H ? oo + a * W * out_ld * 4 : kW6Oob, 0);
}

// ---- the weight gradient in the transform domain (round 4): dW = G^T [ sum_tiles (B^T d B) (.) (A dY A^T) ] G -- the transposition
// of the forward algorithm: 36 multiplies per (tile, filter, channel) instead of the direct form's 144.
//   vfn_winograd_input_f32   V[xi][tile][ci] = (B^T d B)[xi]           (the forward's input transform, ReLU included)
//   vfn_winograd_gy_f32      Z[xi][tile][co] = (A dY A^T)[xi]          dY: the 4x4 tile of dL/dy (zero outside the image)
//   vfn_conv_wgrad_f32       dU[xi][co][ci]  = sum_tile Z[xi][tile][co] V[xi][tile][ci]     (batch = 36 one-by-one problems)
//   vfn_winograd_dw_f32      dW[co][a][b][ci] (+)= rowscale[co] * sum_ij G[i][a] dU[6i+j][co][ci] G[j][b]
// z = A v (4 values -> 6), A = (A^T)^T
__device__ __forceinline__ void a6(const f32x4 (&v)[4], f32x4 (&z)[6]) {
    const f32x4 e = v[0] + v[2], o = v[1] + v[3];
    const f32x4 e4 = v[0] + 4.f * v[2], o8 = 2.f * v[1] + 8.f * v[3];
    z[0] = v[0];
    z[1] = e + o;
    z[2] = e - o;
    z[3] = e4 + o8;
    z[4] = e4 - o8;
    z[5] = v[3];
}

__global__ __launch_bounds__(256)
void winograd_gy_kernel(const float* __restrict__ gy, int N, int H, int W, int C, int ld, float* __restrict__ Z, int rows_pad) {
    const int th = (H + 3) / 4, tw = (W + 3) / 4;
    const int c4n = C / 4;
    const long long total = (long long)N * th * tw * c4n;
    for (long long i = vfn_xcd_block(blockIdx.x, gridDim.x) * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % c4n);
        const int tile = (int)(i / c4n);
        const int tx = tile % tw, ty = (tile / tw) % th, n = tile / (tw * th);
        f32x4 t[6][4];                               // t = A dY (columns of dY through A)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            f32x4 col[4], z[6];
            const int xx = 4 * tx + b;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int yy = 4 * ty + a;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (yy < H && xx < W) v = *reinterpret_cast<const f32x4*>(gy + ((size_t)(n * H + yy) * W + xx) * ld + c4 * 4);
                col[a] = v;
            }
            a6(col, z);
#pragma unroll
            for (int a = 0; a < 6; ++a) t[a][b] = z[a];
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            f32x4 z[6];
            a6(t[a], z);
#pragma unroll
            for (int b = 0; b < 6; ++b)
                *reinterpret_cast<f32x4*>(Z + ((size_t)(a * 6 + b) * rows_pad + tile) * C + c4 * 4) = z[b];
        }
    }
}

// w = G^T u (6 values -> 3)
__device__ __forceinline__ void gt3(const f32x4 (&u)[6], f32x4 (&w)[3]) {
    const f32x4 s12 = u[1] + u[2], d12 = u[2] - u[1], s34 = u[3] + u[4], d34 = u[3] - u[4];
    w[0] = 0.25f * u[0] - (1.f / 6.f) * s12 + (1.f / 24.f) * s34;
    w[1] = (1.f / 6.f) * d12 + (1.f / 12.f) * d34;
    w[2] = -(1.f / 6.f) * s12 + (1.f / 6.f) * s34 + u[5];
}

__global__ __launch_bounds__(256)
void winograd_dw_kernel(const float* __restrict__ dU, int Cout, int Cin, const float* __restrict__ rowscale, float* __restrict__ dw,
                        int accumulate) {
    const int c4n = Cin / 4;
    const long long total = (long long)Cout * c4n;
    const size_t bank = (size_t)Cout * Cin;
    for (long long i = vfn_xcd_block(blockIdx.x, gridDim.x) * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % c4n), co = (int)(i / c4n);
        f32x4 t[3][6];                               // t = G^T dU (columns through G^T)
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            f32x4 u[6], w[3];
#pragma unroll
            for (int a = 0; a < 6; ++a) u[a] = *reinterpret_cast<const f32x4*>(dU + (size_t)(a * 6 + j) * bank + (size_t)co * Cin + c4 * 4);
            gt3(u, w);
#pragma unroll
            for (int a = 0; a < 3; ++a) t[a][j] = w[a];
        }
        const float sc = rowscale ? rowscale[co] : 1.f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            f32x4 w[3];
            gt3(t[a], w);
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                f32x4* o = reinterpret_cast<f32x4*>(dw + ((size_t)co * 9 + a * 3 + b) * Cin + c4 * 4);
                f32x4 v = w[b] * sc;
                if (accumulate) v += *o;
                *o = v;
            }
        }
    }
}


// ---- the transform-domain GEMMs as ONE PERSISTENT launch (round 5) ------------------------------------------------------------
// M[xi][rows][Cout] = V[xi][rows][C] U[xi][cout][C]^T for the 36 components.  Each GEMM has K = C = 128 ... 1024 only, i.e. 4-32 K tiles:
// as separate workgroups (the batched-filter launch of conv_igemm_kernel) a 128 x 128 tile spends 8 K tiles of matrix work between a
// cold prologue (first operand tiles from HBM / L2: 2-14 us in the census, profiles/r05_census_wino_gemm.txt) and an epilogue through
// LDS, and rocprofv3 counts the matrix pipe busy 49 % of the launch.  Here a workgroup walks a LIST of (component, row tile, filter
// tile) units as one uninterrupted K loop: the operand tiles of the next unit are requested PD tiles ahead while the current unit is
// still multiplying, the accumulators leave through dword stores straight from the registers (a raw M tile has no epilogue
// arithmetic) and are zeroed in place -- no drain, no refill, no LDS transpose between units.  Same fragment layout, swizzle and
// k-order as conv_igemm_kernel: every output element is the same fmaf chain, bit for bit.
struct wino_gemm_args {
    const float* V;       // [comps][rows_pad][C]
    const float* U;       // [comps][cout_pad][C]
    float* Mb;            // [comps][rows_pad][Cout]
    int comps, rows_pad, C, Cout, cout_pad;
    int mtiles, ntiles;   // rows_pad / BM, ceil(Cout / BN)
    // CONV form (a 1x1 / stride-1 convolution as ONE such GEMM with the layer's epilogue): V = NHWC input with pixel stride a_ld
    // (rows_pad = M pixels: rows past M read zeros through the buffer resource), Mb = output with pixel stride out_ld
    int a_ld, out_ld, res_ld, res_mod, relu_in, relu_out;
    const float* scale;
    const float* shift;
    const float* res;
};

// DUAL form (CONV only: a block's shortcut 1x1 convolution inside conv3's launch, vfn_conv1x1_shortcut_fused_f32): a unit walks the K
// tiles of the shortcut source first -- input V [N][H][W][a_ld] sampled at (stride * yo, stride * xo) for output pixel (n, yo, xo) of
// an Ho x Wo map, filters U [cout_pad][C] -- turns its accumulators into r = acc * scale + shift (floored at 0 when relu_mid) in
// registers, and walks the main source from zero accumulators; the epilogue adds r where the one-source form loads `res`
struct wino_dual_args {
    const float* V;
    const float* U;
    const float* scale;
    const float* shift;
    int C, a_ld, cout_pad, relu_in, relu_mid, stride, H, W, Ho, Wo, pix;      // (pix = N * H * W input pixels)
};

// The two kernels share one body, wino_gemm_body.inc, as text: BM .. LP, DUAL, the arguments p and (DUAL) q2 are what it names.  The
// one-source kernel keeps its signature, its name and -- every DUAL statement being discarded -- its code.
// LP: both operands are bf16 in memory (V from winograd_input_kernel<true>, U packed by the host): a K tile is 64 channels -- the same
// 128-byte LDS rows, the same staging -- and a 16-byte fragment is one v_mfma_f32_32x32x16_bf16 (k = 16 kk + 8 h .. + 7), f32 accumulate
template <int BM, int BN, int WM, int WN, int PD, bool CONV = false, bool LP = false>
__global__ __launch_bounds__(WM * WN * 64)
void wino_gemm_kernel(const wino_gemm_args p) {
    constexpr bool DUAL = false;
    constexpr wino_dual_args q2{};
#include "wino_gemm_body.inc"
}

template <int BM, int BN, int WM, int WN, int PD>
__global__ __launch_bounds__(WM * WN * 64)
void wino_gemm_dual_kernel(const wino_gemm_args p, const wino_dual_args q2) {
    constexpr bool DUAL = true, CONV = true, LP = false;
#include "wino_gemm_body.inc"
}

template <int BM, int BN, int WM, int WN, int PD, bool CONV, bool LP, bool DUAL = false>
int launch_wino_gemm(const wino_gemm_args& a, int wgs, hipStream_t s, const wino_dual_args* dual = nullptr) {
    constexpr size_t lds = 2 * (size_t)(BM + BN) * 32 * sizeof(float);
    static const bool lds_ready = [] {
        if constexpr (DUAL) return vfn_allow_lds(&wino_gemm_dual_kernel<BM, BN, WM, WN, PD>, lds);
        else return vfn_allow_lds(&wino_gemm_kernel<BM, BN, WM, WN, PD, CONV, LP>, lds);
    }();
    (void)lds_ready;
    wino_gemm_args p = a;
    p.mtiles = (a.rows_pad + BM - 1) / BM;
    p.ntiles = (a.Cout + BN - 1) / BN;
    const int total = p.comps * p.mtiles * p.ntiles;
    int grid = wgs > 0 ? wgs : 512;
    if (grid > total) grid = total;
    grid = (grid + 7) / 8 * 8;                              // (the kernel deals units to blockIdx & 7 = XCD, blockIdx >> 3 = slot)
    if constexpr (DUAL)
        hipLaunchKernelGGL((wino_gemm_dual_kernel<BM, BN, WM, WN, PD>), dim3(grid), dim3(WM * WN * 64), lds, s, p, *dual);
    else
        hipLaunchKernelGGL((wino_gemm_kernel<BM, BN, WM, WN, PD, CONV, LP>), dim3(grid), dim3(WM * WN * 64), lds, s, p);
    return vfn_check_launch();
}

// Configurations of the persistent GEMM: cfg & 3 picks the tile {BM, BN, WM, WN}, cfg >> 2 the prefetch (operand tiles requested
// PD = 1 or 2 K tiles ahead).  CONV: the 1x1 convolution's addressing and epilogue; LP: bf16 operands.
constexpr int kWinoTile[4][4] = {{128, 128, 4, 2}, {64, 128, 2, 4}, {128, 64, 4, 2}, {64, 64, 2, 2}};
constexpr int kWinoCfgs = 8;

// (the two-source form: PD = 1 alone -- its PD = 2 instantiations keep 192-240 bytes per lane in scratch and measured 1.5-2x slower)
constexpr int kWinoDualCfgs = 4;

template <bool CONV, bool LP, bool DUAL = false>
int launch_wino_cfg(const wino_gemm_args& a, int cfg, int wgs, hipStream_t s, const wino_dual_args* dual = nullptr) {
    return vfn_dispatch<DUAL ? kWinoDualCfgs : kWinoCfgs>(cfg, [&](auto id) -> int {
        constexpr int c = decltype(id)::value;
        constexpr const int* t = kWinoTile[c & 3];
        return launch_wino_gemm<t[0], t[1], t[2], t[3], 1 + (c >> 2), CONV, LP, DUAL>(a, wgs, s, dual);
    });
}

// ... and the 32-row tiles of the f32 transform-domain GEMM alone (a 1/16-resolution F(6x6) map of two images is 90 tiles: 96 rows
// instead of 128): configurations kWinoCfgs + (cfg & 3 = tile, bit 2 = PD), one 32 x 32 MFMA tile per wave
constexpr int kWinoTile32[2][4] = {{32, 128, 1, 4}, {32, 64, 1, 2}};
constexpr int kWinoCfgs32 = 8;

inline const int* wino_tile_of(int cfg) { return cfg < kWinoCfgs ? kWinoTile[cfg & 3] : kWinoTile32[cfg & 1]; }
inline bool wino_cfg32_ok(int cfg) { return cfg >= kWinoCfgs && cfg < kWinoCfgs + kWinoCfgs32 && (cfg & 3) < 2; }

int launch_wino_cfg32(const wino_gemm_args& a, int cfg, int wgs, hipStream_t s) {
    switch (cfg - kWinoCfgs) {
        case 0: return launch_wino_gemm<32, 128, 1, 4, 1, false, false>(a, wgs, s);
        case 1: return launch_wino_gemm<32, 64, 1, 2, 1, false, false>(a, wgs, s);
        case 4: return launch_wino_gemm<32, 128, 1, 4, 2, false, false>(a, wgs, s);
        case 5: return launch_wino_gemm<32, 64, 1, 2, 2, false, false>(a, wgs, s);
    }
    return VFN_ERR_ARG;
}

// the transforms address activations through buffer resources with 32-bit byte offsets: every tensor must stay below 2 GiB
inline bool tensors_fit_32bit(int N, int H, int W, int ld, int res_ld, int mask_ld, int res_mod) {
    const long long px = (long long)N * H * W;
    return px * ld * 4 < 0x7fffff00LL && (res_mod > 0 ? (long long)res_mod : px) * res_ld * 4 < 0x7fffff00LL && px * mask_ld * 4 < 0x7fffff00LL;
}

inline int grid_of(long long total) {
    long long b = (total + 255) / 256;
    return (int)(b < 16384 ? (b ? b : 1) : 16384);
}

// VFN_WINO6_XFORM (read once): 0 = form 0 everywhere, 2 = the lane-split form everywhere (tests), unset or "auto" = the measured rule
// below; 1 is accepted and means form 0 (the wave-uniform form it named is not in the tree).  vfn_winograd6_force_form overrides it
// inside a process (tests, scripts/bench_wino6_transforms.py).
std::atomic<int> g_wino6_forced{-1};

int wino6_env_form() {
    static const int v = [] {
        const char* e = getenv("VFN_WINO6_XFORM");
        if (!e || !*e || !strcmp(e, "auto")) return -1;
        const int k = atoi(e);
        return k >= 0 && k <= 2 ? k : -1;
    }();
    return v;
}

// The measured rule (profiles/r11_tune_wino6_transforms.json: each form in isolation at the Winograd shapes of the 480x854 plan, a
// new form taken where it is >= 3 % faster).  The lane-split form won every input transform and every output transform with a
// residual; without a residual form 0 stays at the two shapes (tiles, Cout) where the margin was missed.
int wino6_auto_form(int tiles, int C, bool is_output, bool has_res) {
    static const int keep0_out[][2] = {{45, 640}, {1440, 256}};
    if (is_output && !has_res)
        for (const auto& k : keep0_out)
            if (tiles == k[0] && C == k[1]) return 0;
    return 2;
}

int wino6_form(int N, int H, int W, int C, int is_output, int has_res) {
    const int forced = g_wino6_forced.load(std::memory_order_relaxed);
    const int want = forced >= 0 ? forced : wino6_env_form();
    if (want == 0 || want == 1) return 0;
    if (want == 2) return 2;                                  // (3, forced: the rule whatever the environment says)
    return wino6_auto_form(winograd6_tiles(N, H, W), C, is_output != 0, has_res != 0);
}

}  // namespace

extern "C" int vfn_winograd_tiles(int N, int H, int W) { return N * ((H + 3) / 4) * ((W + 3) / 4); }

extern "C" int vfn_winograd_input_f32(const float* x, int N, int H, int W, int C, int ld_x, int relu, float* V, int rows_pad, void* stream) {
    if (!x || !V || N < 1 || H < 1 || W < 1 || C < 4 || C % 4 || ld_x < C || ld_x % 4 || rows_pad < vfn_winograd_tiles(N, H, W)) return VFN_ERR_ARG;
    const long long total = (long long)vfn_winograd_tiles(N, H, W) * (C / 4);
    if (!tensors_fit_32bit(N, H, W, ld_x, 0, 0, 0)) return VFN_ERR_ARG;
    hipLaunchKernelGGL(winograd_input_kernel<false>, dim3(grid_of(total)), dim3(256), 0, (hipStream_t)stream, x, N, H, W, C, ld_x, relu, V, rows_pad);
    return vfn_check_launch();
}

extern "C" int vfn_winograd_output_f32(const float* Mb, int rows_pad, int N, int H, int W, int Cout, const float* scale, const float* shift,
                                       const float* res, int res_ld, int res_mod, int relu_out, float* out, int out_ld, void* stream) {
    if (!Mb || !out || N < 1 || H < 1 || W < 1 || Cout < 4 || Cout % 4 || out_ld < Cout || out_ld % 4 || (res && res_ld % 4) ||
        rows_pad < vfn_winograd_tiles(N, H, W)) return VFN_ERR_ARG;
    const long long total = (long long)vfn_winograd_tiles(N, H, W) * (Cout / 4);
    if (!tensors_fit_32bit(N, H, W, out_ld, res ? res_ld : 0, 0, res_mod)) return VFN_ERR_ARG;
    hipLaunchKernelGGL(winograd_output_kernel<false>, dim3(grid_of(total)), dim3(256), 0, (hipStream_t)stream, Mb, rows_pad, N, H, W, Cout, scale, shift,
                       res, res_ld, res_mod, relu_out, out, out_ld, (const float*)nullptr, 0, 0);
    return vfn_check_launch();
}

// F(6x6, 3x3) (include/vfn_winograd6.h): V [64][rows_pad][C] of the 8x8 patches at stride 6, rows past the tiles zeroed; the GEMMs are
// vfn_winograd_gemm_f32 with comps = 64; the output transform carries the epilogue of vfn_winograd_output_f32
extern "C" int vfn_winograd6_input_f32(const float* x, int N, int H, int W, int C, int ld_x, int relu, float* V, int rows_pad, void* stream) {
    if (!x || !V || N < 1 || H < 1 || W < 1 || C < 4 || C % 4 || ld_x < C || ld_x % 4 || rows_pad < winograd6_tiles(N, H, W)) return VFN_ERR_ARG;
    if (!tensors_fit_32bit(N, H, W, ld_x, 0, 0, 0) || (long long)64 * rows_pad * C * 4 >= 0x7fffff00LL) return VFN_ERR_ARG;
    const hipStream_t s = (hipStream_t)stream;
    if (wino6_form(N, H, W, C, 0, 0) == 2) {
        const dim3 grid((long long)rows_pad * ((C / 2 + 31) / 32));
        if (relu) hipLaunchKernelGGL(winograd6_input_split_kernel<true>, grid, dim3(256), 0, s, x, N, H, W, C, ld_x, V, rows_pad);
        else hipLaunchKernelGGL(winograd6_input_split_kernel<false>, grid, dim3(256), 0, s, x, N, H, W, C, ld_x, V, rows_pad);
    } else {
        hipLaunchKernelGGL(winograd6_input_kernel, dim3(((long long)rows_pad * (C / 2) + 255) / 256), dim3(256), 0, s, x, N, H, W, C, ld_x, relu, V,
                           rows_pad);
    }
    return vfn_check_launch();
}

extern "C" int vfn_winograd6_form(int N, int H, int W, int C, int is_output, int has_res) {
    if (N < 1 || H < 1 || W < 1 || C < 4 || C % 4) return -1;          // (a form, not a status: 0 is a form)
    return wino6_form(N, H, W, C, is_output, has_res);
}

extern "C" int vfn_winograd6_force_form(int form) {
    if (form < -1 || form > 3) return VFN_ERR_ARG;
    g_wino6_forced.store(form, std::memory_order_relaxed);
    return VFN_OK;
}

extern "C" int vfn_winograd6_output_f32(const float* Mb, int rows_pad, int N, int H, int W, int Cout, const float* scale, const float* shift,
                                        const float* res, int res_ld, int res_mod, int relu_out, float* out, int out_ld, void* stream) {
    if (!Mb || !out || N < 1 || H < 1 || W < 1 || Cout < 4 || Cout % 4 || out_ld < Cout || out_ld % 4 || (res && res_ld % 4) ||
        rows_pad < winograd6_tiles(N, H, W) || res_mod < 0 || (res && res_mod % (H * W))) return VFN_ERR_ARG;
    if (!tensors_fit_32bit(N, H, W, out_ld, res ? res_ld : 0, 0, res_mod) || (long long)64 * rows_pad * Cout * 4 >= 0x7fffff00LL) return VFN_ERR_ARG;
    const long long tiles = winograd6_tiles(N, H, W);
    const int form = wino6_form(N, H, W, Cout, 1, res != nullptr);
    const dim3 grid(form == 2 ? tiles * ((Cout / 2 + 31) / 32) : (tiles * (Cout / 2) + 255) / 256);
    auto* kernel = form == 2 ? (res ? winograd6_output_split_kernel<true> : winograd6_output_split_kernel<false>)
                             : (res ? winograd6_output_kernel<true> : winograd6_output_kernel<false>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, Mb, rows_pad, N, H, W, Cout, scale, shift, res, res_ld, res_mod, relu_out, out,
                       out_ld);
    return vfn_check_launch();
}

// ... with the epilogue of a data-gradient convolution (vfn_conv_desc.mask / mask_after): the result is zeroed where mask <= 0,
// before (mask_after = 0) or after the residual is added
extern "C" int vfn_winograd_output_masked_f32(const float* Mb, int rows_pad, int N, int H, int W, int Cout, const float* res, int res_ld,
                                              const float* mask, int mask_ld, int mask_after, float* out, int out_ld, void* stream) {
    if (!Mb || !out || N < 1 || H < 1 || W < 1 || Cout < 4 || Cout % 4 || out_ld < Cout || out_ld % 4 || (res && res_ld % 4) ||
        (mask && mask_ld % 4) || rows_pad < vfn_winograd_tiles(N, H, W)) return VFN_ERR_ARG;
    const long long total = (long long)vfn_winograd_tiles(N, H, W) * (Cout / 4);
    if (!tensors_fit_32bit(N, H, W, out_ld, res ? res_ld : 0, mask ? mask_ld : 0, 0)) return VFN_ERR_ARG;
    if (mask)
        hipLaunchKernelGGL(winograd_output_kernel<true>, dim3(grid_of(total)), dim3(256), 0, (hipStream_t)stream, Mb, rows_pad, N, H, W, Cout,
                           (const float*)nullptr, (const float*)nullptr, res, res_ld, 0, 0, out, out_ld, mask, mask_ld, mask_after);
    else
        hipLaunchKernelGGL(winograd_output_kernel<false>, dim3(grid_of(total)), dim3(256), 0, (hipStream_t)stream, Mb, rows_pad, N, H, W, Cout,
                           (const float*)nullptr, (const float*)nullptr, res, res_ld, 0, 0, out, out_ld, (const float*)nullptr, 0, 0);
    return vfn_check_launch();
}

extern "C" int vfn_winograd_gy_f32(const float* gy, int N, int H, int W, int C, int ld, float* Z, int rows_pad, void* stream) {
    if (!gy || !Z || N < 1 || H < 1 || W < 1 || C < 4 || C % 4 || ld < C || ld % 4 || rows_pad < vfn_winograd_tiles(N, H, W)) return VFN_ERR_ARG;
    const long long total = (long long)vfn_winograd_tiles(N, H, W) * (C / 4);
    hipLaunchKernelGGL(winograd_gy_kernel, dim3(grid_of(total)), dim3(256), 0, (hipStream_t)stream, gy, N, H, W, C, ld, Z, rows_pad);
    return vfn_check_launch();
}

extern "C" int vfn_winograd_dw_f32(const float* dU, int Cout, int Cin, const float* rowscale, float* dw, int accumulate, void* stream) {
    if (!dU || !dw || Cout < 1 || Cin < 4 || Cin % 4) return VFN_ERR_ARG;
    hipLaunchKernelGGL(winograd_dw_kernel, dim3(grid_of((long long)Cout * (Cin / 4))), dim3(256), 0, (hipStream_t)stream, dU, Cout, Cin, rowscale,
                       dw, accumulate);
    return vfn_check_launch();
}

// (ABI 12) the 36 transform-domain GEMMs as one persistent launch: M [comps][rows_pad][Cout] = V [comps][rows_pad][C] x U [comps][cout_pad][C]^T.
// cfg: 0 = 128x128 tiles (8 waves), 1 = 64x128 (8 waves), 2 = 128x64 (8 waves), 3 = 64x64 (4 waves); + 4: operand tiles requested two K tiles
// ahead instead of one.  wgs: workgroups to launch (0 = 512, two per CU); rows_pad a multiple of the tile height, cout_pad >= the padded
// filter count, C a multiple of 32; every operand below 2 GiB (32-bit buffer offsets)
extern "C" int vfn_winograd_gemm_f32(const float* V, const float* U, float* Mb, int comps, int rows_pad, int C, int Cout, int cout_pad, int cfg,
                                     int wgs, void* stream) {
    if (!V || !U || !Mb || comps < 1 || rows_pad < 1 || C < 32 || C % 32 || Cout < 1 || cout_pad < Cout || cfg < 0 ||
        (cfg >= kWinoCfgs && !wino_cfg32_ok(cfg))) return VFN_ERR_ARG;
    const int bm = wino_tile_of(cfg)[0], bn = wino_tile_of(cfg)[1];
    if (rows_pad % bm || cout_pad < (Cout + bn - 1) / bn * bn) return VFN_ERR_ARG;
    if ((long long)comps * rows_pad * C * 4 >= 0x7fffff00LL || (long long)comps * cout_pad * C * 4 >= 0x7fffff00LL) return VFN_ERR_ARG;
    wino_gemm_args a{V, U, Mb, comps, rows_pad, C, Cout, cout_pad, 0, 0, 0, 0, 0, 0, 0, 0, nullptr, nullptr, nullptr};
    if (cfg >= kWinoCfgs) return launch_wino_cfg32(a, cfg, wgs, (hipStream_t)stream);
    return launch_wino_cfg<false, false>(a, cfg, wgs, (hipStream_t)stream);
}

// (ABI 12) a 1x1 / stride-1 convolution (+ eval BatchNorm / bias, residual, ReLU: the trunk's conv1 / conv3 / downsample, AFB_URR.py:59-61,
// 89-91 through torchvision's Bottleneck) through the same persistent kernel: ONE GEMM [M pixels x Cin] x [Cin x Cout] whose workgroups
// walk their list of output tiles as one uninterrupted K loop and apply the epilogue from the accumulator registers.  These layers
// have K = 64 ... 256 -- two to eight K tiles per output tile -- so as one workgroup per tile they are all prologue and epilogue
// (rocprofv3: matrix pipe busy 20-35 %, 3.8 TB/s on layers that only have to move their tensors once).  Same products in the same
// order as vfn_conv2d_nhwc_f32 without split-K.  cfg / wgs as vfn_winograd_gemm_f32.  Refuses what it does not implement (taps, strides,
// masks, operand images, split-K) with VFN_ERR_ARG.
extern "C" int vfn_conv1x1_persistent_f32(const vfn_conv_desc* d, int cfg, int wgs, void* stream) {
    if (!d || !d->in || !d->w || !d->out || cfg < 0 || cfg >= kWinoCfgs) return VFN_ERR_ARG;
    if (d->KH != 1 || d->KW != 1 || d->stride != 1 || d->pad != 0 || d->mask || d->in_lp || d->out_lp || d->w_packed || d->ksplit > 1 ||
        d->w_batch_rows || d->Cin % 32 || d->in_ld % 4 || d->M < 1 || d->M != d->N * d->H * d->W) return VFN_ERR_ARG;
    const int bn = kWinoTile[cfg & 3][1];
    if (d->cout_pad < (d->Cout + bn - 1) / bn * bn) return VFN_ERR_ARG;
    const long long lim = 0x7fffff00LL;
    if ((long long)d->M * d->in_ld * 4 >= lim || (long long)d->M * d->out_ld * 4 >= lim || (long long)d->cout_pad * d->Cin * 4 >= lim ||
        (d->res && (long long)(d->res_mod > 0 ? d->res_mod : d->M) * d->res_ld * 4 >= lim)) return VFN_ERR_ARG;
    wino_gemm_args a{d->in, d->w, d->out, 1, d->M, d->Cin, d->Cout, d->cout_pad, 0, 0,
                     d->in_ld, d->out_ld, d->res ? d->res_ld : 0, d->res_mod, d->relu_in, d->relu_out, d->scale, d->shift, d->res};
    return launch_wino_cfg<true, false>(a, cfg, wgs, (hipStream_t)stream);
}

// (include/vfn_shortcut_fused.h) a Bottleneck's shortcut convolution inside its conv3's launch: out = act(conv1x1(main) * scale + shift +
// r), r = conv1x1(sc, stride 1 or 2) * sc.scale + sc.shift, with r kept in the accumulator registers' twins instead of written and
// read back.  Every output element is the two fmaf chains and the two epilogue expressions of the two layers run one after the other
// through vfn_conv1x1_persistent_f32 (or vfn_conv2d_nhwc_f32 without split-K).  cfg: 0..3, the tiles of vfn_conv1x1_persistent_f32 with
// operands requested one K tile ahead; wgs as there.
extern "C" int vfn_conv1x1_shortcut_fused_f32(const vfn_conv_desc* sc, const vfn_conv_desc* d, int cfg, int wgs, void* stream) {
    if (!sc || !d || !sc->in || !sc->w || !d->in || !d->w || !d->out || cfg < 0 || cfg >= kWinoDualCfgs) return VFN_ERR_ARG;
    for (const vfn_conv_desc* l : {sc, d})
        if (l->KH != 1 || l->KW != 1 || l->pad != 0 || l->mask || l->in_lp || l->out_lp || l->w_packed || l->ksplit > 1 || l->w_batch_rows ||
            l->res || l->Cin < 32 || l->Cin % 32 || l->in_ld < l->Cin || l->in_ld % 4 || l->N < 1 || l->H < 1 || l->W < 1) return VFN_ERR_ARG;
    if (d->stride != 1 || (sc->stride != 1 && sc->stride != 2)) return VFN_ERR_ARG;
    if (d->M < 1 || d->M != d->N * d->H * d->W || sc->Ho != (sc->H - 1) / sc->stride + 1 || sc->Wo != (sc->W - 1) / sc->stride + 1 ||
        sc->M != sc->N * sc->Ho * sc->Wo || sc->M != d->M || sc->Cout != d->Cout || d->Cout < 1 || d->out_ld < d->Cout) return VFN_ERR_ARG;
    const int bn = kWinoTile[cfg & 3][1];
    const int need = (d->Cout + bn - 1) / bn * bn;
    if (d->cout_pad < need || sc->cout_pad < need) return VFN_ERR_ARG;
    const long long lim = 0x7fffff00LL, pix2 = (long long)sc->N * sc->H * sc->W;
    if (pix2 * sc->in_ld * 4 >= lim || (long long)d->M * d->in_ld * 4 >= lim || (long long)d->M * d->out_ld * 4 >= lim ||
        (long long)d->cout_pad * d->Cin * 4 >= lim || (long long)sc->cout_pad * sc->Cin * 4 >= lim) return VFN_ERR_ARG;
    wino_gemm_args a{d->in, d->w, d->out, 1, d->M, d->Cin, d->Cout, d->cout_pad, 0, 0,
                     d->in_ld, d->out_ld, 0, 0, d->relu_in, d->relu_out, d->scale, d->shift, nullptr};
    const wino_dual_args a2{sc->in, sc->w, sc->scale, sc->shift, sc->Cin, sc->in_ld, sc->cout_pad, sc->relu_in, sc->relu_out, sc->stride,
                            sc->H, sc->W, sc->Ho, sc->Wo, (int)pix2};
    return launch_wino_cfg<true, false, true>(a, cfg, wgs, (hipStream_t)stream, &a2);
}

// (ABI 12) the plain-bf16 mode's Winograd layers (BASELINE configs C3 / C5): the input transform writes V as bf16 (computed in f32, rounded to
// nearest-even once -- the rounding the bf16 convolution applies to its operands as it stages them), the filter banks U are bf16 (packed by
// the host from the float64 transform), the persistent GEMM multiplies them on v_mfma_f32_32x32x16_bf16 with f32 accumulation and writes M in
// f32 for vfn_winograd_output_f32.  C a multiple of 64.
extern "C" int vfn_winograd_input_bf16(const float* x, int N, int H, int W, int C, int ld_x, int relu, void* V, int rows_pad, void* stream) {
    if (!x || !V || N < 1 || H < 1 || W < 1 || C < 4 || C % 4 || ld_x < C || ld_x % 4 || rows_pad < vfn_winograd_tiles(N, H, W)) return VFN_ERR_ARG;
    const long long total = (long long)vfn_winograd_tiles(N, H, W) * (C / 4);
    if (!tensors_fit_32bit(N, H, W, ld_x, 0, 0, 0)) return VFN_ERR_ARG;
    hipLaunchKernelGGL(winograd_input_kernel<true>, dim3(grid_of(total)), dim3(256), 0, (hipStream_t)stream, x, N, H, W, C, ld_x, relu,
                       reinterpret_cast<float*>(V), rows_pad);
    return vfn_check_launch();
}

extern "C" int vfn_winograd_gemm_bf16(const void* V, const void* U, float* Mb, int comps, int rows_pad, int C, int Cout, int cout_pad, int cfg,
                                      int wgs, void* stream) {
    if (!V || !U || !Mb || comps < 1 || rows_pad < 1 || C < 64 || C % 64 || Cout < 1 || cout_pad < Cout || cfg < 0 || cfg >= kWinoCfgs) return VFN_ERR_ARG;
    const int bm = kWinoTile[cfg & 3][0], bn = kWinoTile[cfg & 3][1];
    if (rows_pad % bm || cout_pad < (Cout + bn - 1) / bn * bn) return VFN_ERR_ARG;
    if ((long long)comps * rows_pad * C * 2 >= 0x7fffff00LL || (long long)comps * cout_pad * C * 2 >= 0x7fffff00LL) return VFN_ERR_ARG;
    wino_gemm_args a{reinterpret_cast<const float*>(V), reinterpret_cast<const float*>(U), Mb, comps, rows_pad, C, Cout, cout_pad, 0, 0, 0, 0, 0, 0, 0, 0,
                     nullptr, nullptr, nullptr};
    return launch_wino_cfg<false, true>(a, cfg, wgs, (hipStream_t)stream);
}
