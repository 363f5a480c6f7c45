// Image segmentation on the device (test_image_seg.py:67-124 around model.predict), the pieces the video loop did not have:
//   resize + normalise   Image.resize((w, h), BILINEAR) of the decoded photograph + ToTensor + Normalize into slot b of the
//                        model's batch (libImaging/Resample.c's 8-bit passes over the host's tables; the passes of
//                        train_aug.hip restated for one image of any size, a skipped pass, and the normalising store)
//   upsample + round     F.interpolate(prob, (H, W), bilinear, align_corners=False).round() -> uint8 labels
//   batched squeeze-excite   per-image column sums, a gate per image, the gate applied to the image's rows
// Rules: include/vfn_hip.h.  Everything here is bandwidth- or latency-bound elementwise / reduction work.
#include "common.h"
#include "../../include/vfn_hip.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned char u8;

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

struct Norm { float mean[3], std[3]; };

// ImagingResampleHorizontal_8bpc: src [H][W][3] -> hpass [H][w][3]
__global__ void __launch_bounds__(256) imgseg_resize_h_kernel(const u8* __restrict__ src, u8* __restrict__ hpass,
                                                              const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                              int H, int W, int w) {
    const int ox = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (ox >= w || y >= H) return;
    const int lo = min(max(bounds[ox * 2], 0), W - 1), n = min(min(bounds[ox * 2 + 1], ksize), W - lo);
    const int* k = kk + (size_t)ox * ksize;
    const u8* in = src + ((size_t)y * W + lo) * 3;
    int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
    for (int q = 0; q < n; ++q) {
        const int c = k[q];
        s0 += c * in[q * 3], s1 += c * in[q * 3 + 1], s2 += c * in[q * 3 + 2];
    }
    u8* o = hpass + ((size_t)y * w + ox) * 3;
    o[0] = (u8)clip8(s0 >> 22), o[1] = (u8)clip8(s1 >> 22), o[2] = (u8)clip8(s2 >> 22);
}

// ImagingResampleVertical_8bpc over in [Hs][w][3] (VERT), or the image as it is (Hs == h: the pass Pillow skips), then
// ToTensor + Normalize into dst [3][h][w]
template <bool VERT>
__global__ void __launch_bounds__(256) imgseg_resize_v_kernel(const u8* __restrict__ in, float* __restrict__ dst,
                                                              const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                              int Hs, int h, int w, Norm nm) {
    const int ox = blockIdx.x * 64 + threadIdx.x, oy = blockIdx.y * 4 + threadIdx.y;
    if (ox >= w || oy >= h) return;
    int v0, v1, v2;
    if (VERT) {
        const int lo = min(max(bounds[oy * 2], 0), Hs - 1), n = min(min(bounds[oy * 2 + 1], ksize), Hs - lo);
        const int* k = kk + (size_t)oy * ksize;
        const u8* p0 = in + ((size_t)lo * w + ox) * 3;
        int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
        for (int q = 0; q < n; ++q) {
            const int c = k[q];
            const u8* p = p0 + (size_t)q * w * 3;
            s0 += c * p[0], s1 += c * p[1], s2 += c * p[2];
        }
        v0 = clip8(s0 >> 22), v1 = clip8(s1 >> 22), v2 = clip8(s2 >> 22);
    } else {
        const u8* p = in + ((size_t)oy * w + ox) * 3;
        v0 = p[0], v1 = p[1], v2 = p[2];
    }
    float* o = dst + (size_t)oy * w + ox;
    const size_t plane = (size_t)h * w;
    o[0] = ((float)v0 / 255.0f - nm.mean[0]) / nm.std[0];
    o[plane] = ((float)v1 / 255.0f - nm.mean[1]) / nm.std[1];
    o[2 * plane] = ((float)v2 / 255.0f - nm.mean[2]) / nm.std[2];
}

__global__ void __launch_bounds__(256) imgseg_upsample_round_kernel(const float* __restrict__ p, int h, int w, u8* __restrict__ labels,
                                                                    int H, int W) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    const float fy = fmaxf(sy * ((float)y + 0.5f) - 0.5f, 0.f), fx = fmaxf(sx * ((float)x + 0.5f) - 0.5f, 0.f);
    const int y0 = min((int)fy, h - 1), x0 = min((int)fx, w - 1);
    const int y1 = y0 + (y0 < h - 1), x1 = x0 + (x0 < w - 1);
    const float wy1 = fy - (float)y0, wx1 = fx - (float)x0;
    const float wy0 = 1.0f - wy1, wx0 = 1.0f - wx1;
    const float* r0 = p + (size_t)y0 * w;
    const float* r1 = p + (size_t)y1 * w;
    const float a = wx0 * r0[x0] + wx1 * r0[x1];
    const float b = wx0 * r1[x0] + wx1 * r1[x1];
    const float v = wy0 * a + wy1 * b;
    labels[(size_t)y * W + x] = (u8)(int)rintf(fminf(fmaxf(v, 0.f), 255.f));
}

// part[b][j][c]: 16 channel quads x 16 row lanes per workgroup; blockIdx = (64-channel group, chunk j, image b)
__global__ void __launch_bounds__(256) ln_colsum_batch_kernel(const float* __restrict__ x, int M, int C, int ld, float* __restrict__ part,
                                                              int nb) {
    __shared__ f32x4 red[16][16];
    const int q = threadIdx.x & 15, lane = threadIdx.x >> 4;
    const int c = blockIdx.x * 64 + q * 4, j = blockIdx.y, b = blockIdx.z;
    const int R = (M + nb - 1) / nb;
    const int r0 = j * R, r1 = min(r0 + R, M);
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    if (c < C) {
        const float* xb = x + (size_t)b * M * ld + c;
        for (int r = r0 + lane; r < r1; r += 16) a += *reinterpret_cast<const f32x4*>(xb + (size_t)r * ld);
    }
    red[lane][q] = a;
    __syncthreads();
#pragma unroll
    for (int s = 8; s > 0; s >>= 1) {
        if (lane < s) red[lane][q] += red[lane + s][q];
        __syncthreads();
    }
    if (lane == 0 && c < C) *reinterpret_cast<f32x4*>(part + ((size_t)b * nb + j) * C + c) = red[0][q];
}

__device__ __forceinline__ float swishf(float x) { return x / (1.f + __expf(-x)); }
__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + __expf(-x)); }

// one workgroup of 1024 per image: the chunk sums in order, then ln_se_gate_kernel's two layers (linknet_ops.hip)
__global__ void __launch_bounds__(1024) ln_se_gate_batch_kernel(const float* __restrict__ part, int nb, float inv_hw,
                                                                const float* __restrict__ w1, const float* __restrict__ b1,
                                                                const float* __restrict__ w2, const float* __restrict__ b2,
                                                                float* __restrict__ gate, int C, int sq, int Cpad) {
    __shared__ float mean[4096];
    __shared__ float s[256];
    const int b = blockIdx.x;
    const float* pb = part + (size_t)b * nb * Cpad;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float a = 0.f;
        for (int j = 0; j < nb; ++j) a += pb[(size_t)j * Cpad + c];
        mean[c] = a * inv_hw;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int j = wave; j < sq; j += nw) {
        float a = 0.f;
        for (int c = lane; c < C; c += 64) a = __fmaf_rn(w1[(size_t)j * C + c], mean[c], a);
        a = wave_sum(a);
        if (lane == 0) s[j] = swishf(a + b1[j]);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < Cpad; c += blockDim.x) {
        float g = 0.f;
        if (c < C) {
            float a = b2[c];
            for (int j = 0; j < sq; ++j) a = __fmaf_rn(w2[(size_t)c * sq + j], s[j], a);
            g = sigmoidf(a);
        }
        gate[(size_t)b * Cpad + c] = g;
    }
}

__global__ void __launch_bounds__(256) ln_scale_rows_kernel(float* __restrict__ x, const float* __restrict__ gate, int B, int M, int C,
                                                            int ld) {
    const int c4n = C / 4;
    const size_t total = (size_t)B * M * c4n;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % c4n);
        const size_t row = i / c4n;
        const int b = (int)(row / M);
        f32x4* px = reinterpret_cast<f32x4*>(x + row * ld + c4 * 4);
        const f32x4 g = *reinterpret_cast<const f32x4*>(gate + (size_t)b * C + c4 * 4);
        f32x4 v = *px;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] *= g[e];
        *px = v;
    }
}

}  // namespace

extern "C" int vfn_imgseg_resize_norm(const unsigned char* src, int H, int W, unsigned char* hpass, const int* kx_bounds, const int* kx,
                                      int ksize_x, const int* ky_bounds, const int* ky, int ksize_y, float* x, int B, int b, int h, int w,
                                      const float* mean, const float* std, void* stream) {
    if (!src || !x || !mean || !std || H < 1 || W < 1 || H > VFN_IMGSEG_MAX_SIDE || W > VFN_IMGSEG_MAX_SIDE || h < 1 || w < 1 ||
        h > VFN_IMGSEG_MAX_OUT || w > VFN_IMGSEG_MAX_OUT || B < 1 || b < 0 || b >= B)
        return VFN_ERR_ARG;
    const bool horiz = W != w, vert = H != h;
    if (horiz && (!hpass || !kx_bounds || !kx || ksize_x < 1)) return VFN_ERR_ARG;
    if (vert && (!ky_bounds || !ky || ksize_y < 1)) return VFN_ERR_ARG;
    Norm nm;
    for (int c = 0; c < 3; ++c) {
        nm.mean[c] = mean[c], nm.std[c] = std[c];
        if (!(fabsf(mean[c]) < 3.0e38f) || !(fabsf(std[c]) < 3.0e38f) || std[c] == 0.f) return VFN_ERR_ARG;
    }
    const dim3 block(64, 4);
    const u8* in = src;
    if (horiz) {
        hipLaunchKernelGGL(imgseg_resize_h_kernel, dim3(cdiv(w, 64), cdiv(H, 4)), block, 0, (hipStream_t)stream, src, hpass, kx_bounds, kx,
                           ksize_x, H, W, w);
        in = hpass;
    }
    float* dst = x + (size_t)b * 3 * h * w;
    const dim3 grid(cdiv(w, 64), cdiv(h, 4));
    if (vert)
        hipLaunchKernelGGL(imgseg_resize_v_kernel<true>, grid, block, 0, (hipStream_t)stream, in, dst, ky_bounds, ky, ksize_y, H, h, w, nm);
    else
        hipLaunchKernelGGL(imgseg_resize_v_kernel<false>, grid, block, 0, (hipStream_t)stream, in, dst, ky_bounds, ky, ksize_y, H, h, w, nm);
    return vfn_check_launch();
}

extern "C" int vfn_imgseg_upsample_round(const float* prob, int h, int w, unsigned char* labels, int H, int W, void* stream) {
    if (!prob || !labels || h < 1 || w < 1 || h > VFN_IMGSEG_MAX_OUT || w > VFN_IMGSEG_MAX_OUT || H < 1 || W < 1 ||
        H > VFN_IMGSEG_MAX_SIDE || W > VFN_IMGSEG_MAX_SIDE)
        return VFN_ERR_ARG;
    hipLaunchKernelGGL(imgseg_upsample_round_kernel, dim3(cdiv(W, 64), cdiv(H, 4)), dim3(64, 4), 0, (hipStream_t)stream, prob, h, w,
                       labels, H, W);
    return vfn_check_launch();
}

extern "C" int vfn_ln_colsum_batch_f32(const float* x, int B, int M, int C, int ld, float* part, int nb, void* stream) {
    if (!x || !part || B < 1 || B > 65535 || M < 1 || C < 4 || C % 4 || ld < C || ld % 4 || nb < 1 || nb > 1024) return VFN_ERR_ARG;
    hipLaunchKernelGGL(ln_colsum_batch_kernel, dim3(cdiv(C, 64), nb, B), dim3(256), 0, (hipStream_t)stream, x, M, C, ld, part, nb);
    return vfn_check_launch();
}

extern "C" int vfn_ln_se_gate_batch_f32(const float* part, int nb, float inv_hw, const float* w1, const float* b1, const float* w2,
                                        const float* b2, float* gate, int B, int C, int sq, int Cpad, void* stream) {
    if (!part || !w1 || !b1 || !w2 || !b2 || !gate || nb < 1 || nb > 1024 || B < 1 || C < 1 || sq < 1 || sq > 256 || Cpad < C ||
        Cpad > 4096)
        return VFN_ERR_ARG;
    hipLaunchKernelGGL(ln_se_gate_batch_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, part, nb, inv_hw, w1, b1, w2, b2, gate, C, sq,
                       Cpad);
    return vfn_check_launch();
}

extern "C" int vfn_ln_scale_rows_f32(float* x, const float* gate, int B, int M, int C, int ld, void* stream) {
    if (!x || !gate || B < 1 || M < 1 || C < 4 || C % 4 || ld < C || ld % 4) return VFN_ERR_ARG;
    const size_t total = (size_t)B * M * (C / 4);
    const size_t blocks = (total + 255) / 256;
    hipLaunchKernelGGL(ln_scale_rows_kernel, dim3((unsigned)(blocks < 65535 * 16 ? blocks : 65535 * 16)), dim3(256), 0, (hipStream_t)stream,
                       x, gate, B, M, C, ld);
    return vfn_check_launch();
}
