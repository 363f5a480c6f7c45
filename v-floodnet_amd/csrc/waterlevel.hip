// Water level by reference object (estimation/reference_tracking.py:116-218) on tensors the frame loop already holds:
//   vfn_warp_perspective_u8   cv2.warpPerspective(img, homo_mat, (W, H)) with its default flags (bilinear, constant border
//   vfn_warp_perspective_f32  0) as OpenCV's fixed-point remap, stated in integers (:169-170)
//   vfn_waterline_scan        the column scan below each reference's key point (:195-204)
//   vfn_waterlevel_draw_u8    the green boxes and red lines of the annotated overlay (:193, :203), by the project's own rule
//   vfn_waterline_scan_dev, vfn_waterlevel_draw_dev    the same two under boxes read from device memory (csrc/track.hip)
// All of them are bandwidth-trivial (about 3 MB per 480p frame); they exist so that the water-level series comes out of the
// pass that writes the masks, on the PNG sink's side stream, without a host synchronisation per frame.
#include "common.h"
#include "../../include/vfn_hip.h"
#include <limits.h>
#include <math.h>

namespace {

struct WarpMat { double m[9]; };                       // the INVERSE matrix (destination -> source), row-major
struct WlRefs { int n; int v[VFN_WL_MAX_REFS][4]; };   // key points use v[r][0..1], boxes v[r][0..3]

// destination pixel (x, y) -> source position in 1/32 pixel: integer part (sx, sy), 5-bit fraction (ax, ay)
__device__ __forceinline__ void warp_coord(const WarpMat& M, int x, int y, int& sx, int& sy, int& ax, int& ay) {
#pragma clang fp contract(off)                         // products and sums rounded one by one, as the definition states them
    const double X0 = M.m[0] * x + M.m[1] * y + M.m[2];
    const double Y0 = M.m[3] * x + M.m[4] * y + M.m[5];
    const double Wd = M.m[6] * x + M.m[7] * y + M.m[8];
    const double s = Wd != 0.0 ? 32.0 / Wd : 0.0;
    const int X = (int)rint(fmin(fmax(X0 * s, (double)INT_MIN), (double)INT_MAX));      // rint: round half to even
    const int Y = (int)rint(fmin(fmax(Y0 * s, (double)INT_MIN), (double)INT_MAX));
    sx = X >> 5, ax = X & 31, sy = Y >> 5, ay = Y & 31;
}

// (sum of wx * wy * tap + 512) >> 10 over the four taps; a tap outside the image counts as 0.  Tap(yy, xx) reads one sample.
template <typename Tap>
__device__ __forceinline__ int warp_sample(int sx, int sy, int ax, int ay, int H, int W, Tap tap) {
    const bool x0 = sx >= 0 && sx < W, x1 = sx >= -1 && sx < W - 1;
    const bool y0 = sy >= 0 && sy < H, y1 = sy >= -1 && sy < H - 1;
    const int p00 = (x0 && y0) ? tap(sy, sx) : 0, p01 = (x1 && y0) ? tap(sy, sx + 1) : 0;
    const int p10 = (x0 && y1) ? tap(sy + 1, sx) : 0, p11 = (x1 && y1) ? tap(sy + 1, sx + 1) : 0;
    return ((32 - ay) * ((32 - ax) * p00 + ax * p01) + ay * ((32 - ax) * p10 + ax * p11) + 512) >> 10;
}

// uint8 [H][W][C] -> uint8 [H][W][C]: one thread per destination pixel, its C bytes stored side by side
template <int C>
__global__ void warp_u8_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int H, int W, WarpMat M) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= H * W) return;
    const int y = i / W, x = i - y * W;
    int sx, sy, ax, ay;
    warp_coord(M, x, y, sx, sy, ax, ay);
#pragma unroll
    for (int c = 0; c < C; ++c)
        dst[(size_t)i * C + c] = (unsigned char)warp_sample(sx, sy, ax, ay, H, W, [&](int yy, int xx) {
            return (int)src[((size_t)yy * W + xx) * C + c];
        });
}

// the loop's frame, float [3][H][W] in [0,1]: every tap is first made uint8 the way vfn_overlay_u8 does it (truncation of the
// f32 product x * 255), interpolated as above, and leaves as float [3][H][W] = byte / 255 (vfn_to_tensor_u8's division, which
// that truncation undoes exactly for every byte) -- what vfn_overlay_u8 takes
__global__ void warp_f32_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int W, WarpMat M) {
    const int n = H * W;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int y = i / W, x = i - y * W;
    int sx, sy, ax, ay;
    warp_coord(M, x, y, sx, sy, ax, ay);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* plane = src + (size_t)c * n;
        const int v = warp_sample(sx, sy, ax, ay, H, W, [&](int yy, int xx) {
            return (int)(unsigned char)(plane[(size_t)yy * W + xx] * 255.0f);
        });
        dst[(size_t)c * n + i] = (float)v / 255.0f;
    }
}

// one wavefront per reference: lanes stride over the rows below the key point, a ballot picks the first water row
__device__ __forceinline__ void scan_column(const unsigned char* __restrict__ label, int H, int W, int kx, int ky, int water_label,
                                            int* __restrict__ out) {
    const int lane = threadIdx.x;
    int found = -1;
    for (int base = ky + 1; base < H; base += 64) {                 // (base is wave-uniform)
        const int row = base + lane;
        const bool hit = row < H && label[(size_t)row * W + kx] == water_label;
        const unsigned long long m = __ballot(hit);
        if (m) {
            found = base + __ffsll((long long)m) - 1 - ky;
            break;
        }
    }
    if (lane == 0) *out = found;
}

__global__ void __launch_bounds__(64) waterline_scan_kernel(const unsigned char* __restrict__ label, int H, int W, WlRefs K,
                                                            int water_label, int* __restrict__ log_row) {
    const int r = blockIdx.x;
    scan_column(label, H, W, K.v[r][0], K.v[r][1], water_label, log_row + r);
}

// the same under boxes that live on the device (the row the tracker just wrote): the key point is computed here, and one
// that does not have a row of the image below it logs -1 and reads nothing
__global__ void __launch_bounds__(64) waterline_scan_dev_kernel(const unsigned char* __restrict__ label, int H, int W,
                                                                const int* __restrict__ boxes, int water_label,
                                                                int* __restrict__ log_row) {
    const int r = blockIdx.x;
    const double kx = trunc(boxes[4 * r] + boxes[4 * r + 2] / 2.0);
    const long long ky = (long long)boxes[4 * r + 1] + boxes[4 * r + 3];
    if (!(kx >= 0 && kx < W) || ky < 0 || ky >= H - 1) {
        if (threadIdx.x == 0) log_row[r] = -1;
        return;
    }
    scan_column(label, H, W, (int)kx, (int)ky, water_label, log_row + r);
}

// in place on the RGB overlay.  Box r: the pixels of the closed rectangle [x, x+w] x [y, y+h] whose distance to its boundary
// is 0 or 1 pixel, (0, 200, 0).  Line r, when the scan found d > 1: columns kx, kx+1, rows ky .. ky+d, (200, 0, 0); lines
// after all boxes.  One thread per pixel, so clipping to the image is implicit; only covered pixels are written.
// box(r, v) fills v = (x, y, w, h) of reference r and says whether it is drawn
template <typename Box>
__device__ __forceinline__ void draw_pixel(unsigned char* __restrict__ img, int H, int W, int R, Box box,
                                           const int* __restrict__ log_row) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= H * W) return;
    const int py = i / W, px = i - py * W;
    int colour = 0;                                                 // 0 none, 1 box, 2 line
    int v[4];
    for (int r = 0; r < R; ++r) {
        if (!box(r, v)) continue;
        const int x = v[0], y = v[1], w = v[2], h = v[3];
        if (px >= x && px <= x + w && py >= y && py <= y + h &&
            min(min(px - x, x + w - px), min(py - y, y + h - py)) < 2) colour = 1;
    }
    for (int r = 0; r < R; ++r) {
        const int d = log_row[r];
        if (d <= 1 || !box(r, v)) continue;
        const int kx = (int)(v[0] + v[2] / 2.0), ky = v[1] + v[3];
        if ((px == kx || px == kx + 1) && py >= ky && py <= ky + d) colour = 2;
    }
    if (colour) {
        unsigned char* p = img + (size_t)i * 3;
        p[0] = colour == 2 ? 200 : 0;
        p[1] = colour == 1 ? 200 : 0;
        p[2] = 0;
    }
}

__global__ void waterlevel_draw_kernel(unsigned char* __restrict__ img, int H, int W, WlRefs B, const int* __restrict__ log_row) {
    draw_pixel(img, H, W, B.n, [&](int r, int* v) {
        for (int k = 0; k < 4; ++k) v[k] = B.v[r][k];
        return true;
    }, log_row);
}

// boxes int32 [R][4] on the device; a box the host entry point would refuse (w or h < 0, a value beyond +-2^24) is not drawn
__global__ void waterlevel_draw_dev_kernel(unsigned char* __restrict__ img, int H, int W, const int* __restrict__ boxes, int R,
                                           const int* __restrict__ log_row) {
    draw_pixel(img, H, W, R, [&](int r, int* v) {
        bool ok = true;
        for (int k = 0; k < 4; ++k) {
            v[k] = boxes[4 * r + k];
            ok = ok && v[k] >= (k < 2 ? -(1 << 24) : 0) && v[k] <= (1 << 24);
        }
        return ok;
    }, log_row);
}

bool warp_args(const void* src, const void* dst, int H, int W, const double* minv, WarpMat& M) {
    if (!src || !dst || src == dst || !minv || H < 1 || W < 1 || (long long)H * W > INT_MAX / 4) return false;
    for (int k = 0; k < 9; ++k) {
        if (!isfinite(minv[k])) return false;
        M.m[k] = minv[k];
    }
    return true;
}

}  // namespace

extern "C" int vfn_warp_perspective_u8(const unsigned char* src, unsigned char* dst, int H, int W, int C, const double* minv,
                                       void* stream) {
    WarpMat M;
    if (!warp_args(src, dst, H, W, minv, M) || (C != 1 && C != 3)) return VFN_ERR_ARG;
    const dim3 grid(cdiv(H * W, 256)), block(256);
    if (C == 1) hipLaunchKernelGGL(warp_u8_kernel<1>, grid, block, 0, (hipStream_t)stream, src, dst, H, W, M);
    else hipLaunchKernelGGL(warp_u8_kernel<3>, grid, block, 0, (hipStream_t)stream, src, dst, H, W, M);
    return vfn_check_launch();
}

extern "C" int vfn_warp_perspective_f32(const float* src, float* dst, int H, int W, const double* minv, void* stream) {
    WarpMat M;
    if (!warp_args(src, dst, H, W, minv, M)) return VFN_ERR_ARG;
    hipLaunchKernelGGL(warp_f32_kernel, dim3(cdiv(H * W, 256)), dim3(256), 0, (hipStream_t)stream, src, dst, H, W, M);
    return vfn_check_launch();
}

extern "C" int vfn_waterline_scan(const unsigned char* label, int H, int W, const int* keypoints, int R, int water_label,
                                  int* log, int T, int t, void* stream) {
    if (!label || !keypoints || !log || H < 1 || W < 1 || (long long)H * W > INT_MAX / 4 || R < 1 || R > VFN_WL_MAX_REFS ||
        water_label < 0 || water_label > 255 || t < 0 || t >= T) return VFN_ERR_ARG;
    WlRefs K;
    K.n = R;
    for (int r = 0; r < R; ++r) {
        const int kx = keypoints[2 * r], ky = keypoints[2 * r + 1];
        if (kx < 0 || kx >= W || ky < 0 || ky >= H) return VFN_ERR_ARG;      // never clamped (the reference: IndexError)
        K.v[r][0] = kx, K.v[r][1] = ky, K.v[r][2] = K.v[r][3] = 0;
    }
    hipLaunchKernelGGL(waterline_scan_kernel, dim3(R), dim3(64), 0, (hipStream_t)stream, label, H, W, K, water_label,
                       log + (size_t)t * R);
    return vfn_check_launch();
}

extern "C" int vfn_waterlevel_draw_u8(unsigned char* overlay, int H, int W, const int* boxes, int R, const int* log, int T,
                                      int t, void* stream) {
    if (!overlay || !boxes || !log || H < 1 || W < 1 || (long long)H * W > INT_MAX / 4 || R < 1 || R > VFN_WL_MAX_REFS ||
        t < 0 || t >= T) return VFN_ERR_ARG;
    WlRefs B;
    B.n = R;
    for (int r = 0; r < R; ++r) {
        for (int k = 0; k < 4; ++k) B.v[r][k] = boxes[4 * r + k];
        // (sums below stay far inside int: a box or a scan offset beyond +-2^24 is not an image coordinate)
        for (int k = 0; k < 4; ++k)
            if (B.v[r][k] < -(1 << 24) || B.v[r][k] > (1 << 24)) return VFN_ERR_ARG;
        if (B.v[r][2] < 0 || B.v[r][3] < 0) return VFN_ERR_ARG;
    }
    hipLaunchKernelGGL(waterlevel_draw_kernel, dim3(cdiv(H * W, 256)), dim3(256), 0, (hipStream_t)stream, overlay, H, W, B,
                       log + (size_t)t * R);
    return vfn_check_launch();
}

extern "C" int vfn_waterline_scan_dev(const unsigned char* label, int H, int W, const int* boxes, int R, int water_label, int* log,
                                      int T, int t, void* stream) {
    if (!label || !boxes || !log || H < 1 || W < 1 || (long long)H * W > INT_MAX / 4 || R < 1 || R > VFN_WL_MAX_REFS ||
        water_label < 0 || water_label > 255 || t < 0 || t >= T) return VFN_ERR_ARG;
    hipLaunchKernelGGL(waterline_scan_dev_kernel, dim3(R), dim3(64), 0, (hipStream_t)stream, label, H, W, boxes, water_label,
                       log + (size_t)t * R);
    return vfn_check_launch();
}

extern "C" int vfn_waterlevel_draw_dev(unsigned char* overlay, int H, int W, const int* boxes, int R, const int* log, int T, int t,
                                       void* stream) {
    if (!overlay || !boxes || !log || H < 1 || W < 1 || (long long)H * W > INT_MAX / 4 || R < 1 || R > VFN_WL_MAX_REFS ||
        t < 0 || t >= T) return VFN_ERR_ARG;
    hipLaunchKernelGGL(waterlevel_draw_dev_kernel, dim3(cdiv(H * W, 256)), dim3(256), 0, (hipStream_t)stream, overlay, H, W, boxes,
                       R, log + (size_t)t * R);
    return vfn_check_launch();
}
