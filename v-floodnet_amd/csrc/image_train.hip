// Fine-tuning the bootstrap LinkNet's decoder and head (include/vfn_image_train.h): batch-statistics BatchNorm forward and
// backward, and the head convolution + sigmoid + Dice loss backwards.  All five are HBM-bound passes over [M][C] matrices with
// 32 .. 160 channels: float4 over the channel axis, a capped grid strided over the rows.  The reductions keep their sums in
// float64 (three f64 operations per element loaded: far below the memory time) and are deterministic: a workgroup owns a run
// of consecutive rows, its row lanes are added in lane order through LDS, and a second launch combines the workgroups' results
// in a fixed order.  No atomics.
#include "common.h"
#include "../../include/vfn_image_train.h"

namespace {

constexpr int NT = 256;             // threads per workgroup
constexpr int MIN_ROWS = 64;        // rows per chunk at least (header: "ceil(M / 64)")
constexpr int RUNS = 8;             // the second stage adds 8 runs of consecutive chunks, then the runs in order
constexpr int PER_MAX = VFN_LNT_MAX_BLOCKS / RUNS;      // chunks per run at most

struct Chunks { int nb, rows; };
inline Chunks chunks_of(int M) {
    int nb = cdiv(M, MIN_ROWS);
    if (nb > VFN_LNT_MAX_BLOCKS) nb = VFN_LNT_MAX_BLOCKS;
    const int rows = cdiv(M, nb);
    return {cdiv(M, rows), rows};
}

inline bool mat_ok(int M, int C, int ld) { return M >= 1 && M <= (1 << 30) && C >= 4 && C % 4 == 0 && C <= VFN_LNT_MAX_C && ld >= C && ld % 4 == 0; }

inline int grid_for4(long long total4) {
    const long long b = (total4 + NT - 1) / NT;
    return (int)(b < 2048 ? b : 2048);
}

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// sh[r * cq + q][k]: value k of column quad q as row lane r summed it.  Leaves in sh[q][k] the sum over the R lanes, added in lane
// order; one (q, k) per thread (up to four with many channels) instead of one quad per thread: the serial tail is K times shorter.
template <int K>
__device__ __forceinline__ void combine_lanes(double (*sh)[K], int cq, int R) {
    __syncthreads();
    if (R < 2) return;                                     // (uniform: one lane, nothing to add)
    double s[4] = {0, 0, 0, 0};
    const int total = cq * K;                              // R >= 2: cq <= 128, total <= 4 * NT
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int v = threadIdx.x + i * NT;
        if (v < total) {
            const int q = v / K, k = v - q * K;
            double a = sh[q][k];
            for (int rr = 1; rr < R; ++rr) a += sh[rr * cq + q][k];
            s[i] = a;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int v = threadIdx.x + i * NT;
        if (v < total) sh[v / K][v % K] = s[i];
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------- statistics
// Workgroup j: rows j * rows .. min(M, (j + 1) * rows) - 1.  Thread t: column quad t % cq, row lane t / cq of R = 256 / cq lanes.
__global__ __launch_bounds__(NT) void bn_stats_partial_kernel(const float* __restrict__ x, int M, int C, int ld, int rows,
                                                              double* __restrict__ part) {
    __shared__ double sh[NT][8];
    const int cq = C >> 2, R = NT / cq, q = threadIdx.x % cq, r = threadIdx.x / cq;
    const int m0 = blockIdx.x * rows, m1 = min(M, m0 + rows);
    double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0}, piv[4] = {0, 0, 0, 0};
    if (r < R) {
        const f32x4 p = ld4(x + (size_t)m0 * ld + q * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) piv[e] = (double)p[e];
#pragma unroll 4
        for (int m = m0 + r; m < m1; m += R) {
            const f32x4 v = ld4(x + (size_t)m * ld + q * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double d = (double)v[e] - piv[e];
                s1[e] += d;
                s2[e] = fma(d, d, s2[e]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { sh[threadIdx.x][e] = s1[e]; sh[threadIdx.x][4 + e] = s2[e]; }
    combine_lanes<8>(sh, cq, R);
    if (r == 0) {
        const double n = (double)(m1 - m0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double t1 = sh[q][e], m2 = sh[q][4 + e] - t1 * t1 / n;
            part[((size_t)blockIdx.x * 2 + 0) * C + q * 4 + e] = piv[e] + t1 / n;
            part[((size_t)blockIdx.x * 2 + 1) * C + q * 4 + e] = m2 > 0.0 ? m2 : 0.0;
        }
    }
}

struct Triple { double n, mean, m2; };
__device__ __forceinline__ Triple chan(const Triple& a, const Triple& b) {
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    const double n = a.n + b.n, d = b.mean - a.mean, f = b.n / n;
    return {n, a.mean + d * f, a.m2 + b.m2 + d * d * a.n * f};
}

// 32 channels per workgroup; run `by` of 8 combines its consecutive chunks, thread by = 0 then the runs in order
__global__ __launch_bounds__(NT) void bn_stats_final_kernel(const double* __restrict__ part, int nb, int rows, int M, int C,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, double eps,
                                                            double momentum, float* __restrict__ scale, float* __restrict__ shift,
                                                            float* __restrict__ mean, float* __restrict__ rstd, float* running_mean,
                                                            float* running_var) {
    __shared__ Triple red[RUNS][32];
    const int cx = threadIdx.x & 31, by = threadIdx.x >> 5, c = blockIdx.x * 32 + cx;
    const int per = (nb + RUNS - 1) / RUNS;
    Triple t = {0.0, 0.0, 0.0};
    if (c < C) {
        const int j0 = by * per, cnt = min(nb, j0 + per) - j0;
        double pm[PER_MAX], p2[PER_MAX];                       // every load issued before the serial combination starts
#pragma unroll
        for (int i = 0; i < PER_MAX; ++i) {
            const bool on = i < cnt;
            pm[i] = on ? part[((size_t)(j0 + i) * 2 + 0) * C + c] : 0.0;
            p2[i] = on ? part[((size_t)(j0 + i) * 2 + 1) * C + c] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < PER_MAX; ++i) {
            if (i < cnt) {
                const int j = j0 + i;
                t = chan(t, Triple{(double)(min(M, (j + 1) * rows) - j * rows), pm[i], p2[i]});
            }
        }
    }
    red[by][cx] = t;
    __syncthreads();
    if (by != 0 || c >= C) return;
    for (int b = 1; b < RUNS; ++b) t = chan(t, red[b][cx]);
    const double var = t.m2 / (double)M, rs = 1.0 / sqrt(var + eps), sc = (double)gamma[c] * rs;
    mean[c] = (float)t.mean;
    rstd[c] = (float)rs;
    scale[c] = (float)sc;
    shift[c] = (float)((double)beta[c] - t.mean * sc);
    if (running_mean) running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * t.mean);
    if (running_var) running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * (t.m2 / (double)(M - 1)));
}

// --------------------------------------------------------------------------------------------------------------- apply
__global__ __launch_bounds__(NT) void bn_apply_kernel(const float* x, const float* __restrict__ scale, const float* __restrict__ shift,
                                                      float* y, int M, int C, int ld_x, int ld_y, int relu) {
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
            if (relu) o[e] = vfn_relu_nan(o[e]);
        }
        *reinterpret_cast<f32x4*>(y + (size_t)m * ld_y + col) = o;
    }
}

// ----------------------------------------------------------------------------------------------------- backward reduce
__global__ __launch_bounds__(NT) void bn_bwd_partial_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                            const float* __restrict__ scale, const float* __restrict__ shift,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd, int M, int C,
                                                            int ld_g, int ld_x, int relu, int rows, double* __restrict__ part) {
    __shared__ double sh[NT][8];
    const int cq = C >> 2, R = NT / cq, q = threadIdx.x % cq, r = threadIdx.x / cq;
    const int m0 = blockIdx.x * rows, m1 = min(M, m0 + rows);
    double sb[4] = {0, 0, 0, 0}, sg[4] = {0, 0, 0, 0};
    if (r < R) {
        const f32x4 sc = ld4(scale + q * 4), sf = ld4(shift + q * 4), mu = ld4(mean + q * 4), rs = ld4(rstd + q * 4);
#pragma unroll 4
        for (int m = m0 + r; m < m1; m += R) {
            const f32x4 gv = ld4(g + (size_t)m * ld_g + q * 4), xv = ld4(x + (size_t)m * ld_x + q * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool on = !relu || __fmaf_rn(xv[e], sc[e], sf[e]) > 0.f;
                const double gp = on ? (double)gv[e] : 0.0;
                sb[e] += gp;
                sg[e] = fma(gp, ((double)xv[e] - (double)mu[e]) * (double)rs[e], sg[e]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { sh[threadIdx.x][e] = sb[e]; sh[threadIdx.x][4 + e] = sg[e]; }
    combine_lanes<8>(sh, cq, R);
    if (r == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            part[((size_t)blockIdx.x * 2 + 0) * C + q * 4 + e] = sh[q][e];
            part[((size_t)blockIdx.x * 2 + 1) * C + q * 4 + e] = sh[q][4 + e];
        }
    }
}

__global__ __launch_bounds__(NT) void bn_bwd_final_kernel(const double* __restrict__ part, int nb, int C, float* __restrict__ dgamma,
                                                          float* __restrict__ dbeta) {
    __shared__ double red[RUNS][32][2];
    const int cx = threadIdx.x & 31, by = threadIdx.x >> 5, c = blockIdx.x * 32 + cx;
    const int per = (nb + RUNS - 1) / RUNS;
    double sb = 0.0, sg = 0.0;
    if (c < C) {
        const int j0 = by * per, cnt = min(nb, j0 + per) - j0;
        double pb[PER_MAX], pg[PER_MAX];
#pragma unroll
        for (int i = 0; i < PER_MAX; ++i) {
            const bool on = i < cnt;
            pb[i] = on ? part[((size_t)(j0 + i) * 2 + 0) * C + c] : 0.0;
            pg[i] = on ? part[((size_t)(j0 + i) * 2 + 1) * C + c] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < PER_MAX; ++i) {
            if (i < cnt) { sb += pb[i]; sg += pg[i]; }
        }
    }
    red[by][cx][0] = sb;
    red[by][cx][1] = sg;
    __syncthreads();
    if (by != 0 || c >= C) return;
    for (int b = 1; b < RUNS; ++b) { sb += red[b][cx][0]; sg += red[b][cx][1]; }
    dbeta[c] = (float)sb;
    dgamma[c] = (float)sg;
}

// ------------------------------------------------------------------------------------------------------ backward apply
__global__ __launch_bounds__(NT) void bn_bwd_apply_kernel(const float* g, const float* __restrict__ x, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, const float* __restrict__ mean,
                                                          const float* __restrict__ rstd, const float* __restrict__ dgamma,
                                                          const float* __restrict__ dbeta, float* gx, int M, int C, int ld_g, int ld_x,
                                                          int ld_gx, int relu) {
    const int cq = C >> 2;
    const long long total = (long long)M * cq;
    const float inv_m = 1.f / (float)M;
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const long long m = i / cq;
        const int col = (int)(i - m * cq) * 4;
        const f32x4 gv = ld4(g + (size_t)m * ld_g + col), xv = ld4(x + (size_t)m * ld_x + col);
        const f32x4 sc = ld4(scale + col), sf = ld4(shift + col), mu = ld4(mean + col), rs = ld4(rstd + col);
        const f32x4 dg = ld4(dgamma + col), db = ld4(dbeta + col);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool on = !relu || __fmaf_rn(xv[e], sc[e], sf[e]) > 0.f;
            const float gp = on ? gv[e] : 0.f;
            const float xh = (xv[e] - mu[e]) * rs[e];
            o[e] = sc[e] * (gp - db[e] * inv_m - xh * (dg[e] * inv_m));
        }
        *reinterpret_cast<f32x4*>(gx + (size_t)m * ld_gx + col) = o;
    }
}

// -------------------------------------------------------------------------------------------------------- head backward
// Thread t: column quad t & 7 of the 32 channels, row lane t >> 3 of 32.
__global__ __launch_bounds__(NT) void head_bwd_partial_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ pr, const float* __restrict__ gt,
                                                              const double* __restrict__ sums, int M, int ld, int rows,
                                                              double* __restrict__ part, float* __restrict__ g_x) {
    __shared__ double sh[NT][5];
    const int q = threadIdx.x & 7, r = threadIdx.x >> 3;
    const int m0 = blockIdx.x * rows, m1 = min(M, m0 + rows);
    const double D = sums[1] + sums[2] + 1.0;
    const double c0 = (2.0 * sums[0] + 1.0) / (D * D), c1 = 2.0 / D;          // dL/dpr = c0 - gt c1
    const f32x4 wv = ld4(w + q * 4);
    double gw[4] = {0, 0, 0, 0}, gb = 0.0;
#pragma unroll 4
    for (int m = m0 + r; m < m1; m += 32) {
        const f32x4 xv = ld4(x + (size_t)m * ld + q * 4);
        const double p = (double)pr[m];
        const double dz = (c0 - (double)gt[m] * c1) * (p * (1.0 - p));
        const float dzf = (float)dz;
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[e] = dzf * wv[e];
            gw[e] = fma(dz, (double)xv[e], gw[e]);
        }
        gb += dz;
        *reinterpret_cast<f32x4*>(g_x + (size_t)m * 32 + q * 4) = o;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) sh[threadIdx.x][e] = gw[e];
    sh[threadIdx.x][4] = gb;
    combine_lanes<5>(sh, 8, 32);
    if (r == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) part[(size_t)blockIdx.x * 36 + q * 4 + e] = sh[q][e];
        if (q == 0) part[(size_t)blockIdx.x * 36 + 32] = sh[0][4];
    }
}

__global__ __launch_bounds__(NT) void head_bwd_final_kernel(const double* __restrict__ part, int nb, float* __restrict__ g_w,
                                                            float* __restrict__ g_b) {
    __shared__ double red[4][64];
    const int c = threadIdx.x & 63, by = threadIdx.x >> 6;
    const int per = (nb + 3) / 4;
    double s = 0.0;
    if (c < 33) {
        const int j0 = by * per, cnt = min(nb, j0 + per) - j0;
        double pv[VFN_LNT_MAX_BLOCKS / 4];
#pragma unroll
        for (int i = 0; i < VFN_LNT_MAX_BLOCKS / 4; ++i) pv[i] = i < cnt ? part[(size_t)(j0 + i) * 36 + c] : 0.0;
#pragma unroll
        for (int i = 0; i < VFN_LNT_MAX_BLOCKS / 4; ++i) {
            if (i < cnt) s += pv[i];
        }
    }
    red[by][c] = s;
    __syncthreads();
    if (by != 0 || c >= 33) return;
    s = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
    if (c < 32) g_w[c] = (float)s;
    else *g_b = (float)s;
}

}  // namespace

extern "C" int vfn_lnt_bn_stats_f32(const float* x, int M, int C, int ld, const float* gamma, const float* beta, double eps, double momentum,
                                    double* part, float* scale, float* shift, float* mean, float* rstd, float* running_mean,
                                    float* running_var, void* stream) {
    if (!x || !gamma || !beta || !part || !scale || !shift || !mean || !rstd) return VFN_ERR_ARG;
    if (M < 2 || !mat_ok(M, C, ld) || !(eps >= 0.0) || !(momentum >= 0.0 && momentum <= 1.0)) return VFN_ERR_ARG;
    const Chunks ch = chunks_of(M);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(ch.nb), dim3(NT), 0, s, x, M, C, ld, ch.rows, part);
    hipLaunchKernelGGL(bn_stats_final_kernel, dim3(cdiv(C, 32)), dim3(NT), 0, s, (const double*)part, ch.nb, ch.rows, M, C, gamma, beta, eps,
                       momentum, scale, shift, mean, rstd, running_mean, running_var);
    return vfn_check_launch();
}

extern "C" int vfn_lnt_bn_apply_f32(const float* x, const float* scale, const float* shift, float* y, int M, int C, int ld_x, int ld_y,
                                    int relu, void* stream) {
    if (!x || !scale || !shift || !y || !mat_ok(M, C, ld_x) || !mat_ok(M, C, ld_y)) return VFN_ERR_ARG;
    if (x == y && ld_x != ld_y) return VFN_ERR_ARG;
    hipLaunchKernelGGL(bn_apply_kernel, dim3(grid_for4((long long)M * (C / 4))), dim3(NT), 0, (hipStream_t)stream, x, scale, shift, y, M, C,
                       ld_x, ld_y, relu);
    return vfn_check_launch();
}

extern "C" int vfn_lnt_bn_bwd_reduce_f32(const float* g, const float* x, const float* scale, const float* shift, const float* mean,
                                         const float* rstd, int M, int C, int ld_g, int ld_x, int relu, double* part, float* dgamma,
                                         float* dbeta, void* stream) {
    if (!g || !x || !scale || !shift || !mean || !rstd || !part || !dgamma || !dbeta) return VFN_ERR_ARG;
    if (!mat_ok(M, C, ld_g) || !mat_ok(M, C, ld_x)) return VFN_ERR_ARG;
    const Chunks ch = chunks_of(M);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bn_bwd_partial_kernel, dim3(ch.nb), dim3(NT), 0, s, g, x, scale, shift, mean, rstd, M, C, ld_g, ld_x, relu, ch.rows, part);
    hipLaunchKernelGGL(bn_bwd_final_kernel, dim3(cdiv(C, 32)), dim3(NT), 0, s, (const double*)part, ch.nb, C, dgamma, dbeta);
    return vfn_check_launch();
}

extern "C" int vfn_lnt_bn_bwd_apply_f32(const float* g, const float* x, const float* scale, const float* shift, const float* mean,
                                        const float* rstd, const float* dgamma, const float* dbeta, float* gx, int M, int C, int ld_g,
                                        int ld_x, int ld_gx, int relu, void* stream) {
    if (!g || !x || !scale || !shift || !mean || !rstd || !dgamma || !dbeta || !gx) return VFN_ERR_ARG;
    if (!mat_ok(M, C, ld_g) || !mat_ok(M, C, ld_x) || !mat_ok(M, C, ld_gx)) return VFN_ERR_ARG;
    if (g == gx && ld_g != ld_gx) return VFN_ERR_ARG;
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(grid_for4((long long)M * (C / 4))), dim3(NT), 0, (hipStream_t)stream, g, x, scale, shift,
                       mean, rstd, dgamma, dbeta, gx, M, C, ld_g, ld_x, ld_gx, relu);
    return vfn_check_launch();
}

extern "C" int vfn_lnt_head_bwd_f32(const float* x, const float* w, const float* pr, const float* gt, const double* sums, int M, int ld,
                                    double* part, float* g_x, float* g_w, float* g_b, void* stream) {
    if (!x || !w || !pr || !gt || !sums || !part || !g_x || !g_w || !g_b || !mat_ok(M, 32, ld)) return VFN_ERR_ARG;
    const Chunks ch = chunks_of(M);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(head_bwd_partial_kernel, dim3(ch.nb), dim3(NT), 0, s, x, w, pr, gt, sums, M, ld, ch.rows, part, g_x);
    hipLaunchKernelGGL(head_bwd_final_kernel, dim3(1), dim3(NT), 0, s, (const double*)part, ch.nb, g_w, g_b);
    return vfn_check_launch();
}
