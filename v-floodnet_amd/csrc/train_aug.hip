// The training clip of Water_Image_Train_DS (video_module/dataset/Water_DS.py:53-83) built on the device from one decoded
// photograph: every frame of the clip in one launch per stage (blockIdx.z = frame), driven by a per-frame record.
//   vfn_train_aug_jitter         torchvision ColorJitter on PIL images (ImageEnhance blends, the HSV round trip) with the
//                                horizontal flip folded into the read, uint8 RGB -> uint8 RGB at source resolution
//   vfn_train_aug_affine         Image.transform(AFFINE, BICUBIC | NEAREST, fillcolor=0), evaluated over the crop window only
//   vfn_train_aug_resize         crop().resize((S, S), BICUBIC | NEAREST), ToTensor and ToOnehot
//   vfn_train_aug_label_present  which labels frame 0's resized mask holds (ToOnehot builds its object list from them)
// Pillow's C code is integer, float and double arithmetic without fused multiply-adds; the kernels perform the same IEEE
// operations in the same order, so the output equals Pillow's in every byte (include/vfn_hip.h states each rule).
#include "common.h"
#include "../../include/vfn_hip.h"
#include "../../include/vfn_image_val.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

typedef unsigned char u8;

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// ------------------------------------------------------------------------------------------------ colour jitter
// Convert.c: L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16
__device__ __forceinline__ int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// Blend.c ImagingBlend(degenerate, image, alpha): float arithmetic; inside [0, 1] the sum is converted as it is, outside it
// is clamped first
__device__ __forceinline__ int blend(int deg, int img, float alpha) {
    if (alpha == 1.0f) return img;
    const float t = (float)deg + alpha * (float)(img - deg);
    if (alpha >= 0.0f && alpha <= 1.0f) return (int)(u8)(int)t;
    return t <= 0.0f ? 0 : t >= 255.0f ? 255 : (int)t;
}

// Convert.c rgb2hsv_row: float quotients, the hue sum in double rounded to float, fmod and the scaling by 255 in double
__device__ __forceinline__ void rgb2hsv(int r, int g, int b, int& H, int& S, int& V) {
    const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
    V = mx;
    if (mx == mn) {
        H = S = 0;
        return;
    }
    const float cr = (float)(mx - mn);
    const float s = cr / (float)mx;
    const float rc = (float)(mx - r) / cr, gc = (float)(mx - g) / cr, bc = (float)(mx - b) / cr;
    float h;
    if (r == mx) h = (float)((double)bc - (double)gc);
    else if (g == mx) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    h = (float)fmod((double)h / 6.0 + 1.0, 1.0);
    H = clip8((int)((double)h * 255.0));
    S = clip8((int)((double)s * 255.0));
}

// Convert.c hsv2rgb_row: f and fs are floats, everything else double; round() is half away from zero
__device__ __forceinline__ void hsv2rgb(int h, int s, int v, int& r, int& g, int& b) {
    if (s == 0) {
        r = g = b = v;
        return;
    }
    const double hd = (double)h * 6.0 / 255.0;
    const double i = floor(hd);
    const float f = (float)(hd - i);
    const float fs = (float)((double)s / 255.0);
    const int p = clip8((int)round((double)v * (1.0 - (double)fs)));
    const int q = clip8((int)round((double)v * (1.0 - (double)fs * (double)f)));
    const int t = clip8((int)round((double)v * (1.0 - (double)fs * (1.0 - (double)f))));
    switch ((int)i % 6) {
        case 0: r = v, g = t, b = p; break;
        case 1: r = q, g = v, b = p; break;
        case 2: r = p, g = v, b = t; break;
        case 3: r = p, g = q, b = v; break;
        case 4: r = t, g = p, b = v; break;
        default: r = v, g = p, b = q; break;
    }
}

struct JitFrame { int on, flip, hue; int order[4]; float f[3]; };
struct JitArgs { JitFrame f[VFN_TRAIN_AUG_MAX_T]; };

// FINAL = false: the operations before the contrast step, then the sum of L over the image (integer atomics: the order of
// the additions does not change the sum).  FINAL = true: all four with the mean that sum gives, written flipped or not.
template <bool FINAL>
__global__ void __launch_bounds__(256) jitter_kernel(const u8* __restrict__ src, u8* __restrict__ jit,
                                                     unsigned long long* __restrict__ lsum, int H, int W, JitArgs A) {
    const int t = blockIdx.z;
    const JitFrame& F = A.f[t];
    if (!F.on) return;                                                  // (uniform over the block)
    const int n = H * W;
    int mean = 0;
    if (FINAL) mean = (int)((double)lsum[t] / (double)n + 0.5);         // ImageEnhance.Contrast: int(mean + 0.5)
    u8* dst = jit + (size_t)t * n * 3;
    int acc = 0;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < n; p += gridDim.x * 256) {
        const int y = p / W, x = p - y * W;
        const u8* s = src + ((size_t)y * W + (F.flip ? W - 1 - x : x)) * 3;
        int r = s[0], g = s[1], b = s[2];
        bool stop = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int op = F.order[k];
            if (stop || (!FINAL && op == 1)) {
                stop = true;
                continue;
            }
            if (op == 0) {
                r = blend(0, r, F.f[0]), g = blend(0, g, F.f[0]), b = blend(0, b, F.f[0]);
            } else if (op == 1) {
                r = blend(mean, r, F.f[1]), g = blend(mean, g, F.f[1]), b = blend(mean, b, F.f[1]);
            } else if (op == 2) {
                const int l = luma(r, g, b);
                r = blend(l, r, F.f[2]), g = blend(l, g, F.f[2]), b = blend(l, b, F.f[2]);
            } else {
                int hh, ss, vv;
                rgb2hsv(r, g, b, hh, ss, vv);
                hsv2rgb((hh + F.hue) & 255, ss, vv, r, g, b);
            }
        }
        if (FINAL) {
            u8* d = dst + (size_t)p * 3;
            d[0] = (u8)r, d[1] = (u8)g, d[2] = (u8)b;
        } else {
            acc += luma(r, g, b);
        }
    }
    if (!FINAL) {
        acc = wave_sum_i(acc);
        if ((threadIdx.x & 63) == 0) atomicAdd(&lsum[t], (unsigned long long)acc);
    }
}

// ------------------------------------------------------------------------------------------------ affine over the window
struct AffFrame { double m[6]; long long fx[6]; int on, flip, jitter, tabs; int i, j, h, w; };
struct AffArgs { AffFrame f[VFN_TRAIN_AUG_MAX_T]; };

// Geometry.c BICUBIC: the a = -1 cubic in Horner form
__device__ __forceinline__ double cubic(double v1, double v2, double v3, double v4, double d) {
    const double p1 = v2;
    const double p2 = -v1 + v3;
    const double p3 = 2 * (v1 - v2) + v3 - v4;
    const double p4 = -v1 + v2 - v3 + v4;
    return p1 + d * (p2 + d * (p3 + d * p4));
}

__global__ void __launch_bounds__(256) affine_kernel(const u8* __restrict__ src, const u8* __restrict__ mask,
                                                     const u8* __restrict__ jit, const int* __restrict__ xtab,
                                                     const int* __restrict__ ytab, u8* __restrict__ win_img,
                                                     u8* __restrict__ win_mask, int H, int W, AffArgs A) {
    const int t = blockIdx.z;
    const AffFrame& F = A.f[t];
    const int wx = blockIdx.x * 64 + threadIdx.x, wy = blockIdx.y * 4 + threadIdx.y;
    if (wx >= F.w || wy >= F.h) return;
    const int x = F.j + wx, y = F.i + wy;                               // the output pixel of the full-size transform
    const size_t n = (size_t)H * W;
    const u8* img = F.jitter ? jit + (size_t)t * n * 3 : src;           // (the jittered frame is flipped already)
    const bool iflip = F.flip && !F.jitter;
    u8* oi = win_img + (size_t)t * n * 3 + ((size_t)wy * F.w + wx) * 3;
    u8* om = win_mask + (size_t)t * n + (size_t)wy * F.w + wx;
    auto px = [&](int yy, int xx, int c) { return (double)img[((size_t)yy * W + (iflip ? W - 1 - xx : xx)) * 3 + c]; };
    auto mk = [&](int yy, int xx) { return mask[(size_t)yy * W + (F.flip ? W - 1 - xx : xx)]; };
    if (!F.on) {
        oi[0] = (u8)px(y, x, 0), oi[1] = (u8)px(y, x, 1), oi[2] = (u8)px(y, x, 2);
        *om = mk(y, x);
        return;
    }
    // ---- mask: nearest.  Geometry.c affine_fixed (16.16) or, when m1 == m3 == 0, ImagingScaleAffine's index tables
    int sx, sy;
    if (F.tabs) {
        sx = xtab[(size_t)t * W + x], sy = ytab[(size_t)t * H + y];
    } else {
        sx = (int)((F.fx[2] + F.fx[1] * y + F.fx[0] * x) >> 16);
        sy = (int)((F.fx[5] + F.fx[4] * y + F.fx[3] * x) >> 16);
    }
    *om = (sx >= 0 && sx < W && sy >= 0 && sy < H) ? mk(sy, sx) : (u8)0;
    // ---- image: Geometry.c affine_transform + bicubic_filter8, in double
    const double xc = x + 0.5, yc = y + 0.5;
    double xin = F.m[0] * xc + F.m[1] * yc + F.m[2];
    double yin = F.m[3] * xc + F.m[4] * yc + F.m[5];
    if (xin < 0.0 || xin >= (double)W || yin < 0.0 || yin >= (double)H) {
        oi[0] = oi[1] = oi[2] = 0;
        return;
    }
    xin -= 0.5, yin -= 0.5;
    const int x0 = (int)floor(xin), y0 = (int)floor(yin);
    const double dx = xin - x0, dy = yin - y0;
    int cx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) cx[k] = min(max(x0 - 1 + k, 0), W - 1);
    double v[3][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int yy = y0 - 1 + r;
        // row y0 - 1 is clamped; a later row outside the image repeats the previous row's interpolated value
        const bool ok = r == 0 || (yy >= 0 && yy < H);
        const int yr = min(max(yy, 0), H - 1);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            v[c][r] = ok ? cubic(px(yr, cx[0], c), px(yr, cx[1], c), px(yr, cx[2], c), px(yr, cx[3], c), dx) : v[c][r - (r > 0)];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double o = cubic(v[c][0], v[c][1], v[c][2], v[c][3], dy);
        oi[c] = o <= 0.0 ? (u8)0 : o >= 255.0 ? (u8)255 : (u8)(int)o;          // truncated, not rounded
    }
}

// ------------------------------------------------------------------------------------------------ crop -> S x S
struct ResArgs { int h[VFN_TRAIN_AUG_MAX_T], w[VFN_TRAIN_AUG_MAX_T]; };

// Resample.c ImagingResampleHorizontal_8bpc over the window [h][w][3] -> hpass [h][S][3]
__global__ void __launch_bounds__(256) resize_h_kernel(const u8* __restrict__ win_img, u8* __restrict__ hpass,
                                                       const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                       int H, int W, int S, ResArgs A) {
    const int t = blockIdx.z, h = A.h[t], w = A.w[t];
    const int ox = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (ox >= S || y >= h) return;
    const int* bd = bounds + ((size_t)t * S + ox) * 2;
    const int lo = max(bd[0], 0), n = min(min(bd[1], ksize), w - lo);            // (the host's tables are inside the window)
    const int* k = kk + ((size_t)t * S + ox) * ksize;
    const u8* in = win_img + (size_t)t * H * W * 3 + ((size_t)y * w + lo) * 3;
    int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
    for (int q = 0; q < n; ++q) {
        const int c = k[q];
        s0 += c * in[q * 3], s1 += c * in[q * 3 + 1], s2 += c * in[q * 3 + 2];
    }
    u8* o = hpass + (size_t)t * H * S * 3 + ((size_t)y * S + ox) * 3;
    o[0] = (u8)clip8(s0 >> 22), o[1] = (u8)clip8(s1 >> 22), o[2] = (u8)clip8(s2 >> 22);
}

// ImagingResampleVertical_8bpc over hpass [h][S][3], then ToTensor: float(u8) / 255.0f into [T][3][S][S]
__global__ void __launch_bounds__(256) resize_v_kernel(const u8* __restrict__ hpass, float* __restrict__ frames,
                                                       const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                       int H, int S, ResArgs A) {
    const int t = blockIdx.z, h = A.h[t];
    const int ox = blockIdx.x * 64 + threadIdx.x, oy = blockIdx.y * 4 + threadIdx.y;
    if (ox >= S || oy >= S) return;
    const int* bd = bounds + ((size_t)t * S + oy) * 2;
    const int lo = max(bd[0], 0), n = min(min(bd[1], ksize), h - lo);
    const int* k = kk + ((size_t)t * S + oy) * ksize;
    const u8* in = hpass + (size_t)t * H * S * 3 + ((size_t)lo * S + ox) * 3;
    int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
    for (int q = 0; q < n; ++q) {
        const int c = k[q];
        const u8* p = in + (size_t)q * S * 3;
        s0 += c * p[0], s1 += c * p[1], s2 += c * p[2];
    }
    float* o = frames + (size_t)t * 3 * S * S + (size_t)oy * S + ox;
    o[0] = (float)clip8(s0 >> 22) / 255.0f;
    o[(size_t)S * S] = (float)clip8(s1 >> 22) / 255.0f;
    o[(size_t)2 * S * S] = (float)clip8(s2 >> 22) / 255.0f;
}

struct ObjArgs { int n; int label[VFN_TRAIN_AUG_MAX_OBJ - 1]; };

// Geometry.c ImagingScaleAffine through the host's index tables (-1: outside, the pixel stays 0), then ToOnehot
__global__ void __launch_bounds__(256) mask_onehot_kernel(const u8* __restrict__ win_mask, float* __restrict__ masks,
                                                          const int* __restrict__ nx, const int* __restrict__ ny, int H, int W,
                                                          int S, ResArgs A, ObjArgs O) {
    const int t = blockIdx.z, h = A.h[t], w = A.w[t];
    const int ox = blockIdx.x * 64 + threadIdx.x, oy = blockIdx.y * 4 + threadIdx.y;
    if (ox >= S || oy >= S) return;
    const int xi = nx[(size_t)t * S + ox], yi = ny[(size_t)t * S + oy];
    const int lab = (xi >= 0 && xi < w && yi >= 0 && yi < h) ? win_mask[(size_t)t * H * W + (size_t)yi * w + xi] : 0;
    float* o = masks + (size_t)t * O.n * S * S + (size_t)oy * S + ox;
    int sum = 0;
    for (int k = 1; k < O.n; ++k) {
        const int hit = lab == O.label[k - 1];
        sum += hit;
        o[(size_t)k * S * S] = (float)hit;
    }
    o[0] = (float)(1 - sum);
}

__global__ void __launch_bounds__(256) label_present_kernel(const u8* __restrict__ mask, const int* __restrict__ xtab,
                                                            const int* __restrict__ ytab, int H, int W, int S,
                                                            u8* __restrict__ present) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= S * S) return;
    const int oy = p / S, ox = p - oy * S;
    const int xi = xtab[ox], yi = ytab[oy];
    const int lab = (xi >= 0 && xi < W && yi >= 0 && yi < H) ? mask[(size_t)yi * W + xi] : 0;
    present[lab] = 1;                                                   // (every writer stores the same byte)
}

// ---- argument checks shared by the three clip stages
bool clip_args(const vfn_train_aug_desc* d) {
    if (!d || d->H < 1 || d->W < 1 || d->H > VFN_TRAIN_AUG_MAX_SIDE || d->W > VFN_TRAIN_AUG_MAX_SIDE || d->T < 1 ||
        d->T > VFN_TRAIN_AUG_MAX_T)
        return false;
    for (int t = 0; t < d->T; ++t) {
        const vfn_train_aug_frame& f = d->frame[t];
        if (f.win_i < 0 || f.win_j < 0 || f.win_h < 1 || f.win_w < 1 || f.win_i > d->H - f.win_h || f.win_j > d->W - f.win_w)
            return false;
        if (f.jitter) {
            int seen = 0;
            for (int k = 0; k < 4; ++k) {
                if (f.order[k] < 0 || f.order[k] > 3) return false;
                seen |= 1 << f.order[k];
            }
            if (seen != 15 || f.hue_shift < 0 || f.hue_shift > 255) return false;
            if (!isfinite(f.brightness) || !isfinite(f.contrast) || !isfinite(f.saturation)) return false;
        }
        if (f.affine)
            for (int k = 0; k < 6; ++k)
                if (!isfinite(f.m[k])) return false;
    }
    return true;
}

}  // namespace

extern "C" int vfn_train_aug_jitter(const vfn_train_aug_desc* d, void* stream) {
    if (!clip_args(d) || !d->src || !d->jit || !d->lsum) return VFN_ERR_ARG;
    JitArgs A;
    bool any = false;
    for (int t = 0; t < VFN_TRAIN_AUG_MAX_T; ++t) {
        JitFrame& F = A.f[t];
        F = JitFrame{};
        if (t >= d->T || !d->frame[t].jitter) continue;
        const vfn_train_aug_frame& f = d->frame[t];
        any = true;
        F.on = 1, F.flip = f.flip != 0, F.hue = f.hue_shift;
        for (int k = 0; k < 4; ++k) F.order[k] = f.order[k];
        F.f[0] = f.brightness, F.f[1] = f.contrast, F.f[2] = f.saturation;
    }
    if (!any) return VFN_OK;
    if (hipMemsetAsync(d->lsum, 0, sizeof(unsigned long long) * d->T, (hipStream_t)stream) != hipSuccess) return VFN_ERR_LAUNCH;
    const dim3 grid(min(cdiv(d->H * d->W, 256), 1024), 1, d->T), block(256);
    hipLaunchKernelGGL(jitter_kernel<false>, grid, block, 0, (hipStream_t)stream, d->src, d->jit, d->lsum, d->H, d->W, A);
    hipLaunchKernelGGL(jitter_kernel<true>, grid, block, 0, (hipStream_t)stream, d->src, d->jit, d->lsum, d->H, d->W, A);
    return vfn_check_launch();
}

extern "C" int vfn_train_aug_affine(const vfn_train_aug_desc* d, void* stream) {
    if (!clip_args(d) || !d->src || !d->mask || !d->win_img || !d->win_mask) return VFN_ERR_ARG;
    AffArgs A;
    int mh = 0, mw = 0;
    for (int t = 0; t < VFN_TRAIN_AUG_MAX_T; ++t) {
        AffFrame& F = A.f[t];
        F = AffFrame{};
        if (t >= d->T) continue;
        const vfn_train_aug_frame& f = d->frame[t];
        F.on = f.affine != 0, F.flip = f.flip != 0, F.jitter = f.jitter != 0, F.tabs = f.affine && f.nearest_tables;
        F.i = f.win_i, F.j = f.win_j, F.h = f.win_h, F.w = f.win_w;
        if (F.jitter && !d->jit) return VFN_ERR_ARG;
        if (F.tabs && (!d->aff_xtab || !d->aff_ytab)) return VFN_ERR_ARG;
        if (F.on) {
            const double* m = f.m;
            for (int k = 0; k < 6; ++k) F.m[k] = m[k];
            // Geometry.c check_fixed: the 16.16 path needs every corner coordinate below 32768
            const double xs[2] = {0.0, (double)d->W}, ys[2] = {0.0, (double)d->H};
            for (int a = 0; a < 2 && !F.tabs; ++a)
                for (int b = 0; b < 2; ++b)
                    if (!(fabs(m[0] * xs[a] + m[1] * ys[b] + m[2]) < 32768.0 && fabs(m[3] * xs[a] + m[4] * ys[b] + m[5]) < 32768.0))
                        return VFN_ERR_ARG;
            auto fix = [](double v) { return (long long)floor(v * 65536.0 + 0.5); };
            F.fx[0] = fix(m[0]), F.fx[1] = fix(m[1]), F.fx[3] = fix(m[3]), F.fx[4] = fix(m[4]);
            F.fx[2] = fix(m[2] + m[0] * 0.5 + m[1] * 0.5);
            F.fx[5] = fix(m[5] + m[3] * 0.5 + m[4] * 0.5);
        }
        mh = max(mh, F.h), mw = max(mw, F.w);
    }
    const dim3 grid(cdiv(mw, 64), cdiv(mh, 4), d->T), block(64, 4);
    hipLaunchKernelGGL(affine_kernel, grid, block, 0, (hipStream_t)stream, d->src, d->mask, d->jit, d->aff_xtab, d->aff_ytab,
                       d->win_img, d->win_mask, d->H, d->W, A);
    return vfn_check_launch();
}

extern "C" int vfn_train_aug_resize(const vfn_train_aug_desc* d, void* stream) {
    if (!clip_args(d) || !d->win_img || !d->win_mask || !d->hpass || !d->kx_bounds || !d->kx || !d->ky_bounds || !d->ky ||
        !d->nx || !d->ny || !d->frames || !d->masks || d->S < 1 || d->S > VFN_TRAIN_AUG_MAX_OUT || d->ksize_x < 1 ||
        d->ksize_y < 1 || d->obj_n < 1 || d->obj_n > VFN_TRAIN_AUG_MAX_OBJ)
        return VFN_ERR_ARG;
    ResArgs A = {};
    ObjArgs O = {};
    O.n = d->obj_n;
    for (int k = 0; k + 1 < d->obj_n; ++k) {
        if (d->obj_list[k] < 1 || d->obj_list[k] > 255) return VFN_ERR_ARG;
        O.label[k] = d->obj_list[k];
    }
    int mh = 0;
    for (int t = 0; t < d->T; ++t) {
        A.h[t] = d->frame[t].win_h, A.w[t] = d->frame[t].win_w;
        mh = max(mh, A.h[t]);
    }
    const int S = d->S;
    const dim3 block(64, 4);
    hipLaunchKernelGGL(resize_h_kernel, dim3(cdiv(S, 64), cdiv(mh, 4), d->T), block, 0, (hipStream_t)stream, d->win_img, d->hpass,
                       d->kx_bounds, d->kx, d->ksize_x, d->H, d->W, S, A);
    hipLaunchKernelGGL(resize_v_kernel, dim3(cdiv(S, 64), cdiv(S, 4), d->T), block, 0, (hipStream_t)stream, d->hpass, d->frames,
                       d->ky_bounds, d->ky, d->ksize_y, d->H, S, A);
    hipLaunchKernelGGL(mask_onehot_kernel, dim3(cdiv(S, 64), cdiv(S, 4), d->T), block, 0, (hipStream_t)stream, d->win_mask,
                       d->masks, d->nx, d->ny, d->H, d->W, S, A, O);
    return vfn_check_launch();
}

extern "C" int vfn_train_aug_label_present(const unsigned char* mask, int H, int W, const int* xtab, const int* ytab, int S,
                                           unsigned char* present, void* stream) {
    if (!mask || !xtab || !ytab || !present || H < 1 || W < 1 || H > VFN_TRAIN_AUG_MAX_SIDE || W > VFN_TRAIN_AUG_MAX_SIDE ||
        S < 1 || S > VFN_TRAIN_AUG_MAX_OUT)
        return VFN_ERR_ARG;
    if (hipMemsetAsync(present, 0, 256, (hipStream_t)stream) != hipSuccess) return VFN_ERR_LAUNCH;
    hipLaunchKernelGGL(label_present_kernel, dim3(cdiv(S * S, 256)), dim3(256), 0, (hipStream_t)stream, mask, xtab, ytab, H, W, S,
                       present);
    return vfn_check_launch();
}

// ================================================================================================ one sample of the image module
// WaterDataset_RGB(mode='train_offline') (image_module/dataset_water.py:136-153): the same Pillow arithmetic composed the image
// module's way -- colour operations in a fixed order, each optional; the flip AFTER the affine map; the label kept as an index;
// ImageNet normalisation into a slot of the model's batch.  One photograph per call.  Rules: include/vfn_image_val.h.
namespace {

struct SampleJit { int bri, con, hue_on, hue; float fb, fc; };

// FINAL = false: brightness (when on), then the sum of L for the contrast step's mean.  FINAL = true: every operation that is on.
template <bool FINAL>
__global__ void __launch_bounds__(256) sample_jitter_kernel(const u8* __restrict__ src, u8* __restrict__ jit,
                                                            unsigned long long* __restrict__ lsum, int n, SampleJit J) {
    int mean = 0;
    if (FINAL && J.con) mean = (int)((double)lsum[0] / (double)n + 0.5);
    int acc = 0;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < n; p += gridDim.x * 256) {
        const u8* s = src + (size_t)p * 3;
        int r = s[0], g = s[1], b = s[2];
        if (J.bri) r = blend(0, r, J.fb), g = blend(0, g, J.fb), b = blend(0, b, J.fb);
        if (!FINAL) {
            acc += luma(r, g, b);
            continue;
        }
        if (J.con) r = blend(mean, r, J.fc), g = blend(mean, g, J.fc), b = blend(mean, b, J.fc);
        if (J.hue_on) {
            int hh, ss, vv;
            rgb2hsv(r, g, b, hh, ss, vv);
            hsv2rgb((hh + J.hue) & 255, ss, vv, r, g, b);
        }
        u8* d = jit + (size_t)p * 3;
        d[0] = (u8)r, d[1] = (u8)g, d[2] = (u8)b;
    }
    if (!FINAL) {
        acc = wave_sum_i(acc);
        if ((threadIdx.x & 63) == 0) atomicAdd(lsum, (unsigned long long)acc);
    }
}

struct SampleAff { double m[6]; long long fx[6]; int on, flip, tabs; int i, j, h, w; };

// affine_kernel's arithmetic at output column xs = W - 1 - x (flip after the map) or x; the source is read as it lies
__global__ void __launch_bounds__(256) sample_affine_kernel(const u8* __restrict__ img, const u8* __restrict__ label,
                                                            const int* __restrict__ xtab, const int* __restrict__ ytab,
                                                            u8* __restrict__ win_img, u8* __restrict__ win_label, int H, int W,
                                                            SampleAff F) {
    const int wx = blockIdx.x * 64 + threadIdx.x, wy = blockIdx.y * 4 + threadIdx.y;
    if (wx >= F.w || wy >= F.h) return;
    const int x = F.j + wx, y = F.i + wy;                               // the pixel of the flipped result
    const int xs = F.flip ? W - 1 - x : x;                              // the output column of the transform under the flip
    u8* oi = win_img + ((size_t)wy * F.w + wx) * 3;
    u8* ol = win_label + (size_t)wy * F.w + wx;
    auto px = [&](int yy, int xx, int c) { return (double)img[((size_t)yy * W + xx) * 3 + c]; };
    if (!F.on) {
        const u8* s = img + ((size_t)y * W + xs) * 3;
        oi[0] = s[0], oi[1] = s[1], oi[2] = s[2];
        *ol = label[(size_t)y * W + xs];
        return;
    }
    // ---- label: nearest.  Geometry.c affine_fixed (16.16) or, when m1 == m3 == 0, ImagingScaleAffine's index tables
    int sx, sy;
    if (F.tabs) {
        sx = xtab[xs], sy = ytab[y];
    } else {
        sx = (int)((F.fx[2] + F.fx[1] * y + F.fx[0] * xs) >> 16);
        sy = (int)((F.fx[5] + F.fx[4] * y + F.fx[3] * xs) >> 16);
    }
    *ol = (sx >= 0 && sx < W && sy >= 0 && sy < H) ? label[(size_t)sy * W + sx] : (u8)0;
    // ---- image: Geometry.c affine_transform + bicubic_filter8, in double
    const double xc = xs + 0.5, yc = y + 0.5;
    double xin = F.m[0] * xc + F.m[1] * yc + F.m[2];
    double yin = F.m[3] * xc + F.m[4] * yc + F.m[5];
    if (xin < 0.0 || xin >= (double)W || yin < 0.0 || yin >= (double)H) {
        oi[0] = oi[1] = oi[2] = 0;
        return;
    }
    xin -= 0.5, yin -= 0.5;
    const int x0 = (int)floor(xin), y0 = (int)floor(yin);
    const double dx = xin - x0, dy = yin - y0;
    int cx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) cx[k] = min(max(x0 - 1 + k, 0), W - 1);
    double v[3][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int yy = y0 - 1 + r;
        // row y0 - 1 is clamped; a later row outside the image repeats the previous row's interpolated value
        const bool ok = r == 0 || (yy >= 0 && yy < H);
        const int yr = min(max(yy, 0), H - 1);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            v[c][r] = ok ? cubic(px(yr, cx[0], c), px(yr, cx[1], c), px(yr, cx[2], c), px(yr, cx[3], c), dx) : v[c][r - (r > 0)];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double o = cubic(v[c][0], v[c][1], v[c][2], v[c][3], dy);
        oi[c] = o <= 0.0 ? (u8)0 : o >= 255.0 ? (u8)255 : (u8)(int)o;          // truncated, not rounded
    }
}

struct SampleNorm { float mean[3], std[3]; };

// ImagingResampleVertical_8bpc over hpass [h][S][3], then ToTensor + Normalize into dst [3][S][S] (a slot of the batch)
__global__ void __launch_bounds__(256) sample_resize_v_norm_kernel(const u8* __restrict__ hpass, float* __restrict__ dst,
                                                                   const int* __restrict__ bounds, const int* __restrict__ kk,
                                                                   int ksize, int h, int S, SampleNorm nm) {
    const int ox = blockIdx.x * 64 + threadIdx.x, oy = blockIdx.y * 4 + threadIdx.y;
    if (ox >= S || oy >= S) return;
    const int lo = max(bounds[oy * 2], 0), n = min(min(bounds[oy * 2 + 1], ksize), h - lo);
    const int* k = kk + (size_t)oy * ksize;
    const u8* in = hpass + ((size_t)lo * S + ox) * 3;
    int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
    for (int q = 0; q < n; ++q) {
        const int c = k[q];
        const u8* p = in + (size_t)q * S * 3;
        s0 += c * p[0], s1 += c * p[1], s2 += c * p[2];
    }
    float* o = dst + (size_t)oy * S + ox;
    const size_t plane = (size_t)S * S;
    o[0] = ((float)clip8(s0 >> 22) / 255.0f - nm.mean[0]) / nm.std[0];
    o[plane] = ((float)clip8(s1 >> 22) / 255.0f - nm.mean[1]) / nm.std[1];
    o[2 * plane] = ((float)clip8(s2 >> 22) / 255.0f - nm.mean[2]) / nm.std[2];
}

// Geometry.c ImagingScaleAffine through the host's index tables (-1: outside, the pixel stays 0); the index as a float
__global__ void __launch_bounds__(256) sample_label_kernel(const u8* __restrict__ plane, float* __restrict__ dst,
                                                           const int* __restrict__ nx, const int* __restrict__ ny, int h, int w,
                                                           int S) {
    const int ox = blockIdx.x * 64 + threadIdx.x, oy = blockIdx.y * 4 + threadIdx.y;
    if (ox >= S || oy >= S) return;
    const int xi = nx[ox], yi = ny[oy];
    const int lab = (xi >= 0 && xi < w && yi >= 0 && yi < h) ? plane[(size_t)yi * w + xi] : 0;
    dst[(size_t)oy * S + ox] = (float)lab;
}

bool side_ok(int v) { return v >= 1 && v <= VFN_TRAIN_AUG_MAX_SIDE; }
bool slot_ok(int B, int b, int S) { return B >= 1 && b >= 0 && b < B && S >= 1 && S <= VFN_TRAIN_AUG_MAX_OUT; }

}  // namespace

extern "C" int vfn_imgval_jitter(const unsigned char* src, int H, int W, int brightness_on, float brightness, int contrast_on,
                                 float contrast, int hue_on, int hue_shift, unsigned char* jit, unsigned long long* lsum,
                                 void* stream) {
    if (!src || !jit || !side_ok(H) || !side_ok(W)) return VFN_ERR_ARG;
    if (brightness_on && !isfinite(brightness)) return VFN_ERR_ARG;
    if (contrast_on && (!isfinite(contrast) || !lsum)) return VFN_ERR_ARG;
    if (hue_on && (hue_shift < 0 || hue_shift > 255)) return VFN_ERR_ARG;
    if (!brightness_on && !contrast_on && !hue_on) return VFN_OK;
    SampleJit J = {};
    J.bri = brightness_on != 0, J.con = contrast_on != 0, J.hue_on = hue_on != 0, J.hue = hue_on ? hue_shift : 0;
    J.fb = brightness_on ? brightness : 1.0f, J.fc = contrast_on ? contrast : 1.0f;
    const int n = H * W;
    const dim3 grid(min(cdiv(n, 256), 1024)), block(256);
    if (J.con) {
        if (hipMemsetAsync(lsum, 0, sizeof(unsigned long long), (hipStream_t)stream) != hipSuccess) return VFN_ERR_LAUNCH;
        hipLaunchKernelGGL(sample_jitter_kernel<false>, grid, block, 0, (hipStream_t)stream, src, jit, lsum, n, J);
    }
    hipLaunchKernelGGL(sample_jitter_kernel<true>, grid, block, 0, (hipStream_t)stream, src, jit, lsum, n, J);
    return vfn_check_launch();
}

extern "C" int vfn_imgval_affine_window(const unsigned char* img, const unsigned char* label, int H, int W, int affine,
                                        const double* m, int nearest_tables, const int* xtab, const int* ytab, int flip_after,
                                        int win_i, int win_j, int win_h, int win_w, unsigned char* win_img,
                                        unsigned char* win_label, void* stream) {
    if (!img || !label || !win_img || !win_label || !side_ok(H) || !side_ok(W)) return VFN_ERR_ARG;
    if (win_i < 0 || win_j < 0 || win_h < 1 || win_w < 1 || win_i > H - win_h || win_j > W - win_w) return VFN_ERR_ARG;
    SampleAff F = {};
    F.on = affine != 0, F.flip = flip_after != 0, F.tabs = affine && nearest_tables;
    F.i = win_i, F.j = win_j, F.h = win_h, F.w = win_w;
    if (F.on) {
        if (!m) return VFN_ERR_ARG;
        for (int k = 0; k < 6; ++k) {
            if (!isfinite(m[k])) return VFN_ERR_ARG;
            F.m[k] = m[k];
        }
        if (F.tabs && (!xtab || !ytab)) return VFN_ERR_ARG;
        // Geometry.c check_fixed: the 16.16 path needs every corner coordinate below 32768
        const double xs[2] = {0.0, (double)W}, ys[2] = {0.0, (double)H};
        for (int a = 0; a < 2 && !F.tabs; ++a)
            for (int b = 0; b < 2; ++b)
                if (!(fabs(m[0] * xs[a] + m[1] * ys[b] + m[2]) < 32768.0 && fabs(m[3] * xs[a] + m[4] * ys[b] + m[5]) < 32768.0))
                    return VFN_ERR_ARG;
        auto fix = [](double v) { return (long long)floor(v * 65536.0 + 0.5); };
        F.fx[0] = fix(m[0]), F.fx[1] = fix(m[1]), F.fx[3] = fix(m[3]), F.fx[4] = fix(m[4]);
        F.fx[2] = fix(m[2] + m[0] * 0.5 + m[1] * 0.5);
        F.fx[5] = fix(m[5] + m[3] * 0.5 + m[4] * 0.5);
    }
    hipLaunchKernelGGL(sample_affine_kernel, dim3(cdiv(win_w, 64), cdiv(win_h, 4)), dim3(64, 4), 0, (hipStream_t)stream, img, label,
                       xtab, ytab, win_img, win_label, H, W, F);
    return vfn_check_launch();
}

extern "C" int vfn_imgval_resize_norm(const unsigned char* win_img, int h, int w, unsigned char* hpass, const int* kx_bounds,
                                      const int* kx, int ksize_x, const int* ky_bounds, const int* ky, int ksize_y, float* x, int B,
                                      int b, int S, const float* mean, const float* std, void* stream) {
    if (!win_img || !hpass || !kx_bounds || !kx || !ky_bounds || !ky || !x || !mean || !std || !side_ok(h) || !side_ok(w) ||
        !slot_ok(B, b, S) || ksize_x < 1 || ksize_y < 1)
        return VFN_ERR_ARG;
    SampleNorm nm;
    for (int c = 0; c < 3; ++c) {
        nm.mean[c] = mean[c], nm.std[c] = std[c];
        if (!isfinite(mean[c]) || !isfinite(std[c]) || std[c] == 0.f) return VFN_ERR_ARG;
    }
    ResArgs A = {};
    A.h[0] = h, A.w[0] = w;
    const dim3 block(64, 4);
    // (the clip's horizontal pass with T = 1: frame 0 starts at the buffer's first byte whatever H and W are)
    hipLaunchKernelGGL(resize_h_kernel, dim3(cdiv(S, 64), cdiv(h, 4), 1), block, 0, (hipStream_t)stream, win_img, hpass, kx_bounds, kx,
                       ksize_x, h, w, S, A);
    hipLaunchKernelGGL(sample_resize_v_norm_kernel, dim3(cdiv(S, 64), cdiv(S, 4)), block, 0, (hipStream_t)stream, hpass,
                       x + (size_t)b * 3 * S * S, ky_bounds, ky, ksize_y, h, S, nm);
    return vfn_check_launch();
}

extern "C" int vfn_imgval_label_gather(const unsigned char* plane, int h, int w, const int* nx, const int* ny, float* y, int B, int b,
                                       int S, void* stream) {
    if (!plane || !nx || !ny || !y || !side_ok(h) || !side_ok(w) || !slot_ok(B, b, S)) return VFN_ERR_ARG;
    hipLaunchKernelGGL(sample_label_kernel, dim3(cdiv(S, 64), cdiv(S, 4)), dim3(64, 4), 0, (hipStream_t)stream, plane,
                       y + (size_t)b * S * S, nx, ny, h, w, S);
    return vfn_check_launch();
}
