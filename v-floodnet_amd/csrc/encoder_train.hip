// The backward of the bootstrap LinkNet's EfficientNet-B4 encoder with frozen BatchNorm statistics (include/vfn_encoder_train.h):
// depthwise convolution (data and weight gradient), swish, squeeze-excite, the stem's weight gradient, and the element-wise
// and column-sum passes between them.  The 1x1 convolutions' gradients run through the implicit-GEMM and weight-gradient
// kernels; everything here is HBM- or latency-bound.  Matrices are [M][C] with 32 .. 2688 channels: float4 over the channel
// axis.  The reductions tile a workgroup as 16 column quads (64 channels, 256 contiguous bytes of a row) x 16 row lanes and
// own a run of consecutive rows; a thread adds its rows in float32, the lanes are added in lane order in float64 through LDS
// and a second launch adds the chunks in order.  No atomics.
#include "common.h"
#include "../../include/vfn_encoder_train.h"

namespace {

constexpr int NT = 256;             // threads per workgroup
constexpr int TQ = 16;              // column quads per workgroup
constexpr int TR = NT / TQ;         // row lanes
constexpr int MIN_ROWS = 64;        // rows per chunk at least

struct Chunks { int nb, rows; };
inline Chunks chunks_of(int M, int nmax) {
    int nb = cdiv(M, MIN_ROWS);
    if (nb > nmax) nb = nmax;
    const int rows = cdiv(M, nb);
    return {cdiv(M, rows), rows};
}

inline bool mat_ok(long long M, int C, int ld) {
    return M >= 1 && M <= (1ll << 30) && C >= 4 && C % 4 == 0 && ld >= C && ld % 4 == 0 && M * (long long)ld <= 0x7fffffffll;
}

// the depthwise geometry of the header
inline bool dw_ok(int N, int H, int W, int k, int stride, int pad_b, int Ho, int Wo) {
    if (N < 1 || H < 1 || W < 1 || (k != 3 && k != 5) || (stride != 1 && stride != 2) || pad_b < 0 || pad_b >= k || Ho < 1 || Wo < 1) return false;
    if (H > (1 << 20) || W > (1 << 20)) return false;
    if (Ho > (H + pad_b - 1) / stride + 1 || Wo > (W + pad_b - 1) / stride + 1) return false;
    return (long long)N * H * W <= (1ll << 30) && (long long)N * Ho * Wo <= (1ll << 30);
}

inline int grid_for4(long long total4) {
    const long long b = (total4 + NT - 1) / NT;
    return (int)(b < 4096 ? b : 4096);
}

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, const f32x4& v) { *reinterpret_cast<f32x4*>(p) = v; }
// (expf, not __expf: these passes wait for memory, and the gradients are held to a few float32 roundings)
__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float swishf(float x) { return x / (1.f + expf(-x)); }
__device__ __forceinline__ float dswishf(float x) {
    const float s = sigmoidf(x);
    return s * (1.f + x * (1.f - s));
}

// ------------------------------------------------------------------------------------------------------ element-wise
__global__ __launch_bounds__(NT) void affine_kernel(const float* x, const float* __restrict__ scale, const float* __restrict__ shift,
                                                    const float* __restrict__ res, float* y, int M, int C, int ld_x, int ld_res, int ld_y,
                                                    int swish) {
    const int cq = C >> 2;
    const long long total = (long long)M * cq;
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const long long m = i / cq;
        const int col = (int)(i - m * cq) * 4;
        const f32x4 v = ld4(x + (size_t)m * ld_x + col), sc = ld4(scale + col), sh = ld4(shift + col);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[e] = __fmaf_rn(v[e], sc[e], sh[e]);
            if (swish) o[e] = swishf(o[e]);
        }
        if (res) o += ld4(res + (size_t)m * ld_res + col);
        st4(y + (size_t)m * ld_y + col, o);
    }
}

__global__ __launch_bounds__(NT) void scale_rows_kernel(const float* __restrict__ x, const float* __restrict__ gate, float* __restrict__ y,
                                                        int B, int M, int C, int ld_x, int ld_y) {
    const int cq = C >> 2;
    const long long total = (long long)B * M * cq;
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const long long row = i / cq;
        const int col = (int)(i - row * cq) * 4, b = (int)(row / M);
        const f32x4 v = ld4(x + (size_t)row * ld_x + col), gg = ld4(gate + (size_t)b * C + col);
        st4(y + (size_t)row * ld_y + col, v * gg);
    }
}

__global__ __launch_bounds__(NT) void swish_bwd_kernel(const float* g, const float* __restrict__ gate, const float* __restrict__ dpool,
                                                       float inv_hw, const float* __restrict__ xh, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, float* gy, int B, int M, int C, int ld_g,
                                                       int ld_x, int ld_gy) {
    const int cq = C >> 2;
    const long long total = (long long)B * M * cq;
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const long long row = i / cq;
        const int col = (int)(i - row * cq) * 4, b = (int)(row / M);
        f32x4 gv = ld4(g + (size_t)row * ld_g + col);
        const f32x4 xv = ld4(xh + (size_t)row * ld_x + col), sc = ld4(scale + col), sh = ld4(shift + col);
        if (gate) {
            const f32x4 gg = ld4(gate + (size_t)b * C + col), dp = ld4(dpool + (size_t)b * C + col);
#pragma unroll
            for (int e = 0; e < 4; ++e) gv[e] = __fmaf_rn(gv[e], gg[e], dp[e] * inv_hw);
        }
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = gv[e] * dswishf(__fmaf_rn(xv[e], sc[e], sh[e]));
        st4(gy + (size_t)row * ld_gy + col, o);
    }
}

// ------------------------------------------------------------------------------------------------------- column sums
// grid (chunk, column tile, image).  part [B][nb][2][C].
__global__ __launch_bounds__(NT) void colsums_partial_kernel(const float* __restrict__ g, const float* __restrict__ a, int M, int C, int ld_g,
                                                             int ld_a, int rows, double* __restrict__ part) {
    __shared__ double sh[NT][8];
    const int q = threadIdx.x & (TQ - 1), r = threadIdx.x / TQ, cq = blockIdx.y * TQ + q;
    const int b = blockIdx.z, nb = gridDim.x;
    const int m0 = blockIdx.x * rows, m1 = min(M, m0 + rows);
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
    if (cq * 4 < C) {
        const float* gb = g + (size_t)b * M * ld_g + cq * 4;
        const float* ab = a ? a + (size_t)b * M * ld_a + cq * 4 : nullptr;
#pragma unroll 4
        for (int m = m0 + r; m < m1; m += TR) {
            const f32x4 gv = ld4(gb + (size_t)m * ld_g);
            s0 += gv;
            if (ab) {
                const f32x4 av = ld4(ab + (size_t)m * ld_a);
#pragma unroll
                for (int e = 0; e < 4; ++e) s1[e] = __fmaf_rn(gv[e], av[e], s1[e]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { sh[threadIdx.x][e] = (double)s0[e]; sh[threadIdx.x][4 + e] = (double)s1[e]; }
    __syncthreads();
    if (threadIdx.x < TQ * 8) {
        const int qq = threadIdx.x >> 3, k = threadIdx.x & 7, c = (blockIdx.y * TQ + qq) * 4 + (k & 3);
        if (c < C) {
            double s = sh[qq][k];
            for (int rr = 1; rr < TR; ++rr) s += sh[rr * TQ + qq][k];
            part[(((size_t)b * nb + blockIdx.x) * 2 + (k >> 2)) * C + c] = s;
        }
    }
}

__global__ __launch_bounds__(NT) void colsums_final_kernel(const double* __restrict__ part, int nb, int B, int C, float* __restrict__ sum_g,
                                                           float* __restrict__ sum_ga) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= B * C) return;
    const int b = i / C, c = i - b * C;
    double s0 = 0.0, s1 = 0.0;
    for (int j = 0; j < nb; ++j) {
        s0 += part[(((size_t)b * nb + j) * 2 + 0) * C + c];
        s1 += part[(((size_t)b * nb + j) * 2 + 1) * C + c];
    }
    if (sum_g) sum_g[i] = (float)s0;
    if (sum_ga) sum_ga[i] = (float)s1;
}

// ------------------------------------------------------------------------------------------------ squeeze-excite backward
// One workgroup per image: u, swish(u), dv, du and dpool.  tmp [B][Cpad + 2 sq]: dv [Cpad], swish(u) [sq], du [sq].
__global__ __launch_bounds__(1024) void se_bwd_image_kernel(const float* __restrict__ sum_px, float inv_hw, const float* __restrict__ dgate,
                                                            const float* __restrict__ w1, const float* __restrict__ b1,
                                                            const float* __restrict__ w2, const float* __restrict__ b2, float* tmp,
                                                            float* __restrict__ dpool, int C, int sq, int Cpad) {
    __shared__ float su[VFN_ET_MAX_SQ], shid[VFN_ET_MAX_SQ], sdu[VFN_ET_MAX_SQ];
    const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const float* px = sum_px + (size_t)n * Cpad;
    float* t_dv = tmp + (size_t)n * (Cpad + 2 * sq);
    float* t_hid = t_dv + Cpad;
    float* t_du = t_hid + sq;
    for (int j = wave; j < sq; j += nw) {
        double a = 0.0;
        for (int c = lane; c < C; c += 64) a = fma((double)w1[(size_t)j * C + c], (double)(px[c] * inv_hw), a);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        if (lane == 0) {
            const float u = (float)(a + (double)b1[j]);
            su[j] = u;
            shid[j] = swishf(u);
            t_hid[j] = shid[j];
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < Cpad; c += blockDim.x) {
        float dv = 0.f;
        if (c < C) {
            double a = (double)b2[c];
            for (int j = 0; j < sq; ++j) a = fma((double)w2[(size_t)c * sq + j], (double)shid[j], a);
            const float gt = sigmoidf((float)a);
            dv = dgate[(size_t)n * Cpad + c] * (gt * (1.f - gt));
        }
        t_dv[c] = dv;
    }
    __syncthreads();                                               // (the workgroup's own global writes are visible behind it)
    for (int j = wave; j < sq; j += nw) {
        double a = 0.0;
        for (int c = lane; c < C; c += 64) a = fma((double)w2[(size_t)c * sq + j], (double)t_dv[c], a);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        if (lane == 0) {
            const float du = (float)a * dswishf(su[j]);
            sdu[j] = du;
            t_du[j] = du;
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < Cpad; c += blockDim.x) {
        float dp = 0.f;
        if (c < C) {
            double a = 0.0;
            for (int j = 0; j < sq; ++j) a = fma((double)w1[(size_t)j * C + c], (double)sdu[j], a);
            dp = (float)a;
        }
        dpool[(size_t)n * Cpad + c] = dp;
    }
}

// the parameter gradients: sums over the images in image order, one thread per element of dw1 / dw2 (db1, db2: the first threads)
__global__ __launch_bounds__(NT) void se_bwd_params_kernel(const float* __restrict__ sum_px, float inv_hw, const float* __restrict__ tmp,
                                                           float* __restrict__ dw1, float* __restrict__ db1, float* __restrict__ dw2,
                                                           float* __restrict__ db2, int B, int C, int sq, int Cpad) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= C * sq) return;
    const int per = Cpad + 2 * sq;
    {   // dw2 [C][sq]
        const int c = i / sq, j = i - c * sq;
        double a = 0.0;
        for (int n = 0; n < B; ++n) a = fma((double)tmp[(size_t)n * per + c], (double)tmp[(size_t)n * per + Cpad + j], a);
        dw2[i] = (float)a;
    }
    {   // dw1 [sq][C]
        const int j = i / C, c = i - j * C;
        double a = 0.0;
        for (int n = 0; n < B; ++n)
            a = fma((double)tmp[(size_t)n * per + Cpad + sq + j], (double)(sum_px[(size_t)n * Cpad + c] * inv_hw), a);
        dw1[i] = (float)a;
    }
    if (i < C) {
        double a = 0.0;
        for (int n = 0; n < B; ++n) a += (double)tmp[(size_t)n * per + i];
        db2[i] = (float)a;
    }
    if (i < sq) {
        double a = 0.0;
        for (int n = 0; n < B; ++n) a += (double)tmp[(size_t)n * per + Cpad + sq + i];
        db1[i] = (float)a;
    }
}

// ------------------------------------------------------------------------------------------------ depthwise, forwards
// vfn_ln_dwconv_f32's kernel without the activation behind the BatchNorm: the backward wants xhat
template <int K>
__global__ __launch_bounds__(NT) void dwconv_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ scale,
                                                    const float* __restrict__ shift, float* __restrict__ out, int N, int H, int W, int C,
                                                    int ld_x, int ld_o, int stride, int pad_b, int Ho, int Wo, int swish_in) {
    const int cq = C >> 2;
    const long long total = (long long)N * Ho * Wo * cq;
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const long long pix = i / cq;
        const int col = (int)(i - pix * cq) * 4;
        const int xo = (int)(pix % Wo), yo = (int)((pix / Wo) % Ho), n = (int)(pix / ((long long)Wo * Ho));
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
            const int yi = yo * stride - pad_b + ky;
            if ((unsigned)yi >= (unsigned)H) continue;
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                const int xi = xo * stride - pad_b + kx;
                if ((unsigned)xi >= (unsigned)W) continue;
                f32x4 v = ld4(x + (((size_t)n * H + yi) * W + xi) * ld_x + col);
                if (swish_in) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = swishf(v[e]);
                }
                const f32x4 f = ld4(w + (size_t)(ky * K + kx) * C + col);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = __fmaf_rn(v[e], f[e], acc[e]);
            }
        }
        const f32x4 sc = ld4(scale + col), sh = ld4(shift + col);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = __fmaf_rn(acc[e], sc[e], sh[e]);
        st4(out + (size_t)pix * ld_o + col, o);
    }
}

// ------------------------------------------------------------------------------------------------ depthwise data gradient
// a thread per input pixel and column quad: a gather over the taps, in tap order
template <int K>
__global__ __launch_bounds__(NT) void dw_dgrad_kernel(const float* __restrict__ g, const float* __restrict__ w, const float* __restrict__ y,
                                                      float* __restrict__ gx, int N, int H, int W, int C, int ld_g, int ld_y, int ld_gx,
                                                      int stride, int pad_b, int Ho, int Wo, int swish_in) {
    const int cq = C >> 2, sm = stride - 1;                       // stride 1 / 2: t / stride = t >> sm, t % stride = t & sm
    const long long total = (long long)N * H * W * cq;
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const long long pix = i / cq;
        const int col = (int)(i - pix * cq) * 4;
        const int xi = (int)(pix % W), yi = (int)((pix / W) % H), n = (int)(pix / ((long long)W * H));
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
            const int ty = yi + pad_b - ky;
            if (ty < 0 || (ty & sm) || (ty >> sm) >= Ho) continue;
            const int yo = ty >> sm;
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                const int tx = xi + pad_b - kx;
                if (tx < 0 || (tx & sm) || (tx >> sm) >= Wo) continue;
                const int xo = tx >> sm;
                const f32x4 gv = ld4(g + (((size_t)n * Ho + yo) * Wo + xo) * ld_g + col), f = ld4(w + (size_t)(ky * K + kx) * C + col);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = __fmaf_rn(gv[e], f[e], acc[e]);
            }
        }
        if (swish_in) {
            const f32x4 yv = ld4(y + (size_t)pix * ld_y + col);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] *= dswishf(yv[e]);
        }
        st4(gx + (size_t)pix * ld_gx + col, acc);
    }
}

// ---------------------------------------------------------------------------------------------- depthwise weight gradient
// grid (chunk of input rows, column tile).  A thread: one column quad, every 16th input pixel of the chunk; act(a) once per
// pixel, then the k*k outputs that read it.  part [nb][K*K][C].
template <int K>
__global__ __launch_bounds__(NT) void dw_wgrad_partial_kernel(const float* __restrict__ g, const float* __restrict__ a, int M, int H, int W,
                                                              int C, int ld_g, int ld_a, int stride, int pad_b, int Ho, int Wo,
                                                              int swish_in, int rows, double* __restrict__ part) {
    __shared__ double sh[NT][4];
    const int q = threadIdx.x & (TQ - 1), r = threadIdx.x / TQ, col = (blockIdx.y * TQ + q) * 4, sm = stride - 1;
    const int m0 = blockIdx.x * rows, m1 = min(M, m0 + rows);
    f32x4 acc[K * K];
#pragma unroll
    for (int t = 0; t < K * K; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (col < C) {
        for (int m = m0 + r; m < m1; m += TR) {
            const int xi = m % W, yi = (m / W) % H, n = m / (W * H);
            f32x4 v = ld4(a + (size_t)m * ld_a + col);
            if (swish_in) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = swishf(v[e]);
            }
#pragma unroll
            for (int ky = 0; ky < K; ++ky) {
                const int ty = yi + pad_b - ky;
                if (ty < 0 || (ty & sm) || (ty >> sm) >= Ho) continue;
                const int yo = ty >> sm;
#pragma unroll
                for (int kx = 0; kx < K; ++kx) {
                    const int tx = xi + pad_b - kx;
                    if (tx < 0 || (tx & sm) || (tx >> sm) >= Wo) continue;
                    const f32x4 gv = ld4(g + (((size_t)n * Ho + yo) * Wo + (tx >> sm)) * ld_g + col);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[ky * K + kx][e] = __fmaf_rn(gv[e], v[e], acc[ky * K + kx][e]);
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < K * K; ++t) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) sh[threadIdx.x][e] = (double)acc[t][e];
        __syncthreads();
        if (threadIdx.x < TQ * 4) {
            const int qq = threadIdx.x >> 2, e = threadIdx.x & 3, c = (blockIdx.y * TQ + qq) * 4 + e;
            if (c < C) {
                double s = sh[qq][e];
                for (int rr = 1; rr < TR; ++rr) s += sh[rr * TQ + qq][e];
                part[((size_t)blockIdx.x * (K * K) + t) * C + c] = s;
            }
        }
    }
}

// out[i] = sum over the chunks, in chunk order, of part[j][i]; i < n
__global__ __launch_bounds__(NT) void chunks_final_kernel(const double* __restrict__ part, int nb, int n, float* __restrict__ out) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int j = 0; j < nb; ++j) s += part[(size_t)j * n + i];
    out[i] = (float)s;
}

// ------------------------------------------------------------------------------------------------------------- the stem
// vfn_ln_stem_f32's kernel without the swish: 16 output channels per thread
__global__ __launch_bounds__(NT) void stem_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ scale,
                                                  const float* __restrict__ shift, float* __restrict__ out, int N, int H, int W, int Ho,
                                                  int Wo, int Cp, int ld, int pad_b) {
    __shared__ float sw[48 * 27];
    for (int i = threadIdx.x; i < 48 * 27; i += NT) sw[i] = w[i];
    __syncthreads();
    const int groups = Cp / 16;
    const long long total = (long long)N * Ho * Wo * groups;
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const int gidx = (int)(i % groups);
        const long long pix = i / groups;
        const int xo = (int)(pix % Wo), yo = (int)((pix / Wo) % Ho), n = (int)(pix / ((long long)Wo * Ho));
        float v[27];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int yi = yo * 2 - pad_b + ky, xi = xo * 2 - pad_b + kx;
                    v[(c * 3 + ky) * 3 + kx] = ((unsigned)yi < (unsigned)H && (unsigned)xi < (unsigned)W)
                                                   ? x[(((size_t)n * 3 + c) * H + yi) * W + xi] : 0.f;
                }
        float* o = out + (size_t)pix * ld + gidx * 16;
#pragma unroll 4
        for (int cc = 0; cc < 16; ++cc) {
            const int co = gidx * 16 + cc;
            float rr = 0.f;
            if (co < 48) {
                float acc = 0.f;
#pragma unroll
                for (int t = 0; t < 27; ++t) acc = fmaf(v[t], sw[co * 27 + t], acc);
                rr = __fmaf_rn(acc, scale[co], shift[co]);
            }
            o[cc] = rr;
        }
    }
}

// A workgroup per chunk of output rows; 64 rows at a time through LDS (their 48 gradients and 27 input values); thread t: filter
// t % 48, taps 6 (t / 48) .. 6 (t / 48) + 5 of 27 (threads 240 .. 255 only help with the loads).  part [nb][48 * 27].
__global__ __launch_bounds__(NT) void stem_wgrad_partial_kernel(const float* __restrict__ g, const float* __restrict__ x, int M, int H, int W,
                                                                int Ho, int Wo, int ld_g, int pad_b, int rows, double* __restrict__ part) {
    __shared__ float sg[64][48];
    __shared__ float sv[64][32];
    const int co = threadIdx.x % 48, tg = threadIdx.x / 48;
    const int m0 = blockIdx.x * rows, m1 = min(M, m0 + rows);
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int base = m0; base < m1; base += 64) {
        const int cnt = min(64, m1 - base);
        __syncthreads();
        for (int i = threadIdx.x; i < 64 * 48; i += NT) {
            const int rr = i / 48, c = i - rr * 48;
            sg[rr][c] = rr < cnt ? g[(size_t)(base + rr) * ld_g + c] : 0.f;
        }
        for (int i = threadIdx.x; i < 64 * 32; i += NT) {
            const int rr = i >> 5, t = i & 31;
            float v = 0.f;
            if (rr < cnt && t < 27) {
                const int m = base + rr, xo = m % Wo, yo = (m / Wo) % Ho, n = m / (Wo * Ho);
                const int c = t / 9, ky = (t - c * 9) / 3, kx = t - c * 9 - ky * 3;
                const int yi = yo * 2 - pad_b + ky, xi = xo * 2 - pad_b + kx;
                if ((unsigned)yi < (unsigned)H && (unsigned)xi < (unsigned)W) v = x[(((size_t)n * 3 + c) * H + yi) * W + xi];
            }
            sv[rr][t] = v;
        }
        __syncthreads();
        if (tg < 5) {
            float a6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            for (int rr = 0; rr < 64; ++rr) {
                const float gv = sg[rr][co];
#pragma unroll
                for (int t = 0; t < 6; ++t) a6[t] = fmaf(gv, sv[rr][tg * 6 + t], a6[t]);
            }
#pragma unroll
            for (int t = 0; t < 6; ++t) acc[t] += (double)a6[t];
        }
    }
    if (tg < 5) {
#pragma unroll
        for (int t = 0; t < 6; ++t)
            if (tg * 6 + t < 27) part[(size_t)blockIdx.x * 1296 + co * 27 + tg * 6 + t] = acc[t];
    }
}

}  // namespace

extern "C" int vfn_et_affine_f32(const float* x, const float* scale, const float* shift, const float* res, float* y, int M, int C, int ld_x,
                                 int ld_res, int ld_y, int swish, void* stream) {
    if (!x || !scale || !shift || !y || !mat_ok(M, C, ld_x) || !mat_ok(M, C, ld_y) || (res && !mat_ok(M, C, ld_res))) return VFN_ERR_ARG;
    if (x == y && ld_x != ld_y) return VFN_ERR_ARG;
    hipLaunchKernelGGL(affine_kernel, dim3(grid_for4((long long)M * (C / 4))), dim3(NT), 0, (hipStream_t)stream, x, scale, shift, res, y, M, C,
                       ld_x, ld_res, ld_y, swish);
    return vfn_check_launch();
}

extern "C" int vfn_et_scale_rows_f32(const float* x, const float* gate, float* y, int B, int M, int C, int ld_x, int ld_y, void* stream) {
    if (!x || !gate || !y || B < 1 || M < 1 || !mat_ok((long long)B * M, C, ld_x) || !mat_ok((long long)B * M, C, ld_y)) return VFN_ERR_ARG;
    hipLaunchKernelGGL(scale_rows_kernel, dim3(grid_for4((long long)B * M * (C / 4))), dim3(NT), 0, (hipStream_t)stream, x, gate, y, B, M, C,
                       ld_x, ld_y);
    return vfn_check_launch();
}

extern "C" int vfn_et_colsums_f32(const float* g, const float* a, int B, int M, int C, int ld_g, int ld_a, double* part, float* sum_g,
                                  float* sum_ga, void* stream) {
    if (!g || !part || B < 1 || B > VFN_ET_MAX_BLOCKS || M < 1 || !mat_ok((long long)B * M, C, ld_g)) return VFN_ERR_ARG;
    if ((a != nullptr) != (sum_ga != nullptr) || (!sum_g && !sum_ga) || (a && !mat_ok((long long)B * M, C, ld_a))) return VFN_ERR_ARG;
    if ((long long)B * C > 0x7fffffffll) return VFN_ERR_ARG;
    const int nmax = VFN_ET_MAX_BLOCKS / B;
    const Chunks ch = chunks_of(M, nmax < 1 ? 1 : nmax);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(colsums_partial_kernel, dim3(ch.nb, cdiv(C / 4, TQ), B), dim3(NT), 0, s, g, a, M, C, ld_g, ld_a, ch.rows, part);
    hipLaunchKernelGGL(colsums_final_kernel, dim3(cdiv(B * C, NT)), dim3(NT), 0, s, (const double*)part, ch.nb, B, C, sum_g, sum_ga);
    return vfn_check_launch();
}

extern "C" int vfn_et_se_bwd_f32(const float* sum_px, float inv_hw, const float* dgate, const float* w1, const float* b1, const float* w2,
                                 const float* b2, float* tmp, float* dpool, float* dw1, float* db1, float* dw2, float* db2, int B, int C,
                                 int sq, int Cpad, void* stream) {
    if (!sum_px || !dgate || !w1 || !b1 || !w2 || !b2 || !tmp || !dpool || !dw1 || !db1 || !dw2 || !db2) return VFN_ERR_ARG;
    if (B < 1 || B > 65535 || C < 1 || Cpad < C || Cpad > (1 << 20) || sq < 1 || sq > VFN_ET_MAX_SQ) return VFN_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(se_bwd_image_kernel, dim3(B), dim3(1024), 0, s, sum_px, inv_hw, dgate, w1, b1, w2, b2, tmp, dpool, C, sq, Cpad);
    hipLaunchKernelGGL(se_bwd_params_kernel, dim3(cdiv(C * sq, NT)), dim3(NT), 0, s, sum_px, inv_hw, (const float*)tmp, dw1, db1, dw2, db2, B,
                       C, sq, Cpad);
    return vfn_check_launch();
}

extern "C" int vfn_et_swish_bwd_f32(const float* g, const float* gate, const float* dpool, float inv_hw, const float* xh, const float* scale,
                                    const float* shift, float* gy, int B, int M, int C, int ld_g, int ld_x, int ld_gy, void* stream) {
    if (!g || !xh || !scale || !shift || !gy || B < 1 || M < 1) return VFN_ERR_ARG;
    const long long rows = (long long)B * M;
    if (!mat_ok(rows, C, ld_g) || !mat_ok(rows, C, ld_x) || !mat_ok(rows, C, ld_gy)) return VFN_ERR_ARG;
    if ((gate != nullptr) != (dpool != nullptr) || (g == gy && ld_g != ld_gy)) return VFN_ERR_ARG;
    hipLaunchKernelGGL(swish_bwd_kernel, dim3(grid_for4(rows * (C / 4))), dim3(NT), 0, (hipStream_t)stream, g, gate, dpool, inv_hw, xh, scale,
                       shift, gy, B, M, C, ld_g, ld_x, ld_gy);
    return vfn_check_launch();
}

extern "C" int vfn_et_dwconv_f32(const float* x, const float* w, const float* scale, const float* shift, float* out, int N, int H, int W, int C,
                                 int ld_x, int ld_out, int k, int stride, int pad_before, int Ho, int Wo, int swish_in, void* stream) {
    if (!x || !w || !scale || !shift || !out || !dw_ok(N, H, W, k, stride, pad_before, Ho, Wo)) return VFN_ERR_ARG;
    const long long Mi = (long long)N * H * W, Mo = (long long)N * Ho * Wo;
    if (!mat_ok(Mi, C, ld_x) || !mat_ok(Mo, C, ld_out)) return VFN_ERR_ARG;
    const dim3 grid(grid_for4(Mo * (C / 4)));
    if (k == 3)
        hipLaunchKernelGGL(dwconv_kernel<3>, grid, dim3(NT), 0, (hipStream_t)stream, x, w, scale, shift, out, N, H, W, C, ld_x, ld_out, stride,
                           pad_before, Ho, Wo, swish_in);
    else
        hipLaunchKernelGGL(dwconv_kernel<5>, grid, dim3(NT), 0, (hipStream_t)stream, x, w, scale, shift, out, N, H, W, C, ld_x, ld_out, stride,
                           pad_before, Ho, Wo, swish_in);
    return vfn_check_launch();
}

extern "C" int vfn_et_dw_dgrad_f32(const float* g, const float* w, const float* y, float* gx, int N, int H, int W, int C, int ld_g, int ld_y,
                                   int ld_gx, int k, int stride, int pad_before, int Ho, int Wo, int swish_in, void* stream) {
    if (!g || !w || !gx || (swish_in && !y) || !dw_ok(N, H, W, k, stride, pad_before, Ho, Wo)) return VFN_ERR_ARG;
    const long long Mi = (long long)N * H * W, Mo = (long long)N * Ho * Wo;
    if (!mat_ok(Mo, C, ld_g) || !mat_ok(Mi, C, ld_gx) || (swish_in && !mat_ok(Mi, C, ld_y))) return VFN_ERR_ARG;
    const dim3 grid(grid_for4(Mi * (C / 4)));
    if (k == 3)
        hipLaunchKernelGGL(dw_dgrad_kernel<3>, grid, dim3(NT), 0, (hipStream_t)stream, g, w, y, gx, N, H, W, C, ld_g, ld_y, ld_gx, stride,
                           pad_before, Ho, Wo, swish_in);
    else
        hipLaunchKernelGGL(dw_dgrad_kernel<5>, grid, dim3(NT), 0, (hipStream_t)stream, g, w, y, gx, N, H, W, C, ld_g, ld_y, ld_gx, stride,
                           pad_before, Ho, Wo, swish_in);
    return vfn_check_launch();
}

extern "C" int vfn_et_dw_wgrad_f32(const float* g, const float* a, double* part, float* dw, int N, int H, int W, int C, int ld_g, int ld_a,
                                   int k, int stride, int pad_before, int Ho, int Wo, int swish_in, void* stream) {
    if (!g || !a || !part || !dw || !dw_ok(N, H, W, k, stride, pad_before, Ho, Wo)) return VFN_ERR_ARG;
    const long long Mi = (long long)N * H * W, Mo = (long long)N * Ho * Wo;
    if (!mat_ok(Mo, C, ld_g) || !mat_ok(Mi, C, ld_a) || (long long)k * k * C > 0x7fffffffll) return VFN_ERR_ARG;
    const Chunks ch = chunks_of((int)Mi, VFN_ET_MAX_BLOCKS);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(ch.nb, cdiv(C / 4, TQ));
    if (k == 3)
        hipLaunchKernelGGL(dw_wgrad_partial_kernel<3>, grid, dim3(NT), 0, s, g, a, (int)Mi, H, W, C, ld_g, ld_a, stride, pad_before, Ho, Wo,
                           swish_in, ch.rows, part);
    else
        hipLaunchKernelGGL(dw_wgrad_partial_kernel<5>, grid, dim3(NT), 0, s, g, a, (int)Mi, H, W, C, ld_g, ld_a, stride, pad_before, Ho, Wo,
                           swish_in, ch.rows, part);
    hipLaunchKernelGGL(chunks_final_kernel, dim3(cdiv(k * k * C, NT)), dim3(NT), 0, s, (const double*)part, ch.nb, k * k * C, dw);
    return vfn_check_launch();
}

extern "C" int vfn_et_stem_f32(const float* x, const float* w, const float* scale, const float* shift, float* out, int N, int H, int W, int Ho,
                               int Wo, int Cp, int ld, int pad_before, void* stream) {
    if (!x || !w || !scale || !shift || !out || !dw_ok(N, H, W, 3, 2, pad_before, Ho, Wo)) return VFN_ERR_ARG;
    if (Cp < 48 || Cp % 16 || !mat_ok((long long)N * Ho * Wo, Cp, ld) || (long long)N * 3 * H * W > 0x7fffffffll) return VFN_ERR_ARG;
    const long long total = (long long)N * Ho * Wo * (Cp / 16);
    hipLaunchKernelGGL(stem_kernel, dim3(grid_for4(total)), dim3(NT), 0, (hipStream_t)stream, x, w, scale, shift, out, N, H, W, Ho, Wo, Cp, ld,
                       pad_before);
    return vfn_check_launch();
}

extern "C" int vfn_et_stem_wgrad_f32(const float* g, const float* x, double* part, float* dw, int N, int H, int W, int Ho, int Wo, int ld_g,
                                     int pad_before, void* stream) {
    if (!g || !x || !part || !dw || !dw_ok(N, H, W, 3, 2, pad_before, Ho, Wo)) return VFN_ERR_ARG;
    const long long M = (long long)N * Ho * Wo;
    if (!mat_ok(M, 48, ld_g) || (long long)N * 3 * H * W > 0x7fffffffll) return VFN_ERR_ARG;
    const Chunks ch = chunks_of((int)M, VFN_ET_MAX_BLOCKS);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(stem_wgrad_partial_kernel, dim3(ch.nb), dim3(NT), 0, s, g, x, (int)M, H, W, Ho, Wo, ld_g, pad_before, ch.rows, part);
    hipLaunchKernelGGL(chunks_final_kernel, dim3(cdiv(1296, NT)), dim3(NT), 0, s, (const double*)part, ch.nb, 1296, dw);
    return vfn_check_launch();
}
