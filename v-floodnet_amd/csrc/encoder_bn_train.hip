// The bootstrap LinkNet's EfficientNet-B4 encoder in train mode (include/vfn_encoder_bn_train.h): batch statistics of a raw
// convolution output, the normalisation with the drop-connect scale and the residual, and the backward's centring term.  95
// BatchNorms per step, 32 .. 2688 channels wide: everything here waits for memory.  The statistics tile a workgroup as
// csrc/encoder_train.hip's column sums do (16 column quads x 16 row lanes over a run of consecutive rows) and add in float64
// around a pivot; a second launch combines the chunks by Chan's rule.  No atomics.
#include "common.h"
#include "../../include/vfn_encoder_train.h"
#include "../../include/vfn_encoder_bn_train.h"

namespace {

constexpr int NT = 256;             // threads per workgroup
constexpr int TQ = 16;              // column quads per workgroup
constexpr int TR = NT / TQ;         // row lanes
constexpr int MIN_ROWS = 64;        // rows per chunk at least
constexpr int RUNS = 8;             // runs of consecutive chunks the second launch combines side by side
constexpr int FC = NT / RUNS;       // channels per workgroup of the second launch

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

inline int grid_for4(long long total4) {
    const long long b = (total4 + NT - 1) / NT;
    return (int)(b < 4096 ? b : 4096);
}

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, const f32x4& v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ float swishf(float x) { return x / (1.f + expf(-x)); }

// ---------------------------------------------------------------------------------------------------------- statistics
// grid (chunk, column tile).  Chunk j: rows j * rows .. min(M, (j + 1) * rows) - 1.  part [nb][2][C]: the chunk's mean and its
// sum of squared deviations from it.
__global__ __launch_bounds__(NT) void bn_stats_partial_kernel(const float* __restrict__ z, int M, int C, int ld, int rows,
                                                              double* __restrict__ part) {
    __shared__ double sh[NT][8];
    const int q = threadIdx.x & (TQ - 1), r = threadIdx.x / TQ, col = (blockIdx.y * TQ + q) * 4;
    const int m0 = blockIdx.x * rows, m1 = min(M, m0 + rows);
    double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    if (col < C) {
        const float* zc = z + col;
        const f32x4 p = ld4(zc + (size_t)m0 * ld);
#pragma unroll 4
        for (int m = m0 + r; m < m1; m += TR) {
            const f32x4 v = ld4(zc + (size_t)m * ld);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double d = (double)v[e] - (double)p[e];
                s1[e] += d;
                s2[e] = fma(d, d, s2[e]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { sh[threadIdx.x][e] = s1[e]; sh[threadIdx.x][4 + e] = s2[e]; }
    __syncthreads();
    if (threadIdx.x < TQ * 4) {
        const int qq = threadIdx.x >> 2, e = threadIdx.x & 3, c = (blockIdx.y * TQ + qq) * 4 + e;
        if (c < C) {
            double t1 = sh[qq][e], t2 = sh[qq][4 + e];
            for (int rr = 1; rr < TR; ++rr) { t1 += sh[rr * TQ + qq][e]; t2 += sh[rr * TQ + qq][4 + e]; }
            const double n = (double)(m1 - m0), piv = (double)z[(size_t)m0 * ld + c], m2 = t2 - t1 * t1 / n;
            part[((size_t)blockIdx.x * 2 + 0) * C + c] = piv + t1 / n;
            part[((size_t)blockIdx.x * 2 + 1) * C + c] = m2 > 0.0 ? m2 : 0.0;
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

// FC channels per workgroup; run `by` of RUNS combines its consecutive chunks in order, thread by = 0 then the runs in order
__global__ __launch_bounds__(NT) void bn_stats_final_kernel(const double* __restrict__ part, int nb, int rows, int M, int C,
                                                            const float* __restrict__ gamma, double eps, double momentum,
                                                            float* __restrict__ rstd, float* __restrict__ nshift, float* __restrict__ fold,
                                                            float* running_mean, float* running_var, int c_run) {
    __shared__ Triple red[RUNS][FC];
    const int cx = threadIdx.x & (FC - 1), by = threadIdx.x / FC, c = blockIdx.x * FC + cx;
    const int per = (nb + RUNS - 1) / RUNS;
    Triple t = {0.0, 0.0, 0.0};
    if (c < C) {
        const int j0 = by * per, j1 = min(nb, j0 + per);
#pragma unroll 4
        for (int j = j0; j < j1; ++j)
            t = chan(t, Triple{(double)(min(M, (j + 1) * rows) - j * rows), part[((size_t)j * 2 + 0) * C + c], part[((size_t)j * 2 + 1) * C + c]});
    }
    red[by][cx] = t;
    __syncthreads();
    if (by != 0 || c >= C) return;
    for (int b = 1; b < RUNS; ++b) t = chan(t, red[b][cx]);
    const double var = t.m2 / (double)M, rs = 1.0 / sqrt(var + eps);
    rstd[c] = (float)rs;
    nshift[c] = (float)(-t.mean * rs);
    fold[c] = (float)((double)gamma[c] * rs);
    if (running_mean && c < c_run) {
        running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * t.mean);
        running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * (t.m2 / (double)(M - 1)));
    }
}

// ------------------------------------------------------------------------------------------------------- element-wise
// (at most 2^31 - 1 elements: the quad index and its divisions stay in 32 bits)
__global__ __launch_bounds__(NT) void bn_norm_kernel(const float* z, const float* __restrict__ rstd, const float* __restrict__ nshift,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     const float* __restrict__ keep, const float* __restrict__ res, float* xh,
                                                     float* __restrict__ y, int rows, int M, int C, int ld_z, int ld_res, int ld_xh, int ld_y,
                                                     int swish) {
    const int cq = C >> 2, total = rows * cq;
    for (int i = blockIdx.x * NT + threadIdx.x; i < total; i += gridDim.x * NT) {
        const int row = i / cq, col = (i - row * cq) * 4;
        const f32x4 v = ld4(z + (size_t)row * ld_z + col), rs = ld4(rstd + col), ns = ld4(nshift + col), ga = ld4(gamma + col),
                    be = ld4(beta + col);
        f32x4 h, o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            h[e] = __fmaf_rn(v[e], rs[e], ns[e]);
            o[e] = __fmaf_rn(h[e], ga[e], be[e]);
            if (swish) o[e] = swishf(o[e]);
        }
        if (keep) o *= keep[row / M];
        if (res) o += ld4(res + (size_t)row * ld_res + col);
        st4(xh + (size_t)row * ld_xh + col, h);
        st4(y + (size_t)row * ld_y + col, o);
    }
}

__global__ __launch_bounds__(NT) void bn_center_kernel(const float* g, const float* __restrict__ xh, const float* __restrict__ keep,
                                                       const float* __restrict__ dbeta, const float* __restrict__ dgamma, float* gp,
                                                       float inv_rows, int rows, int M, int C, int ld_g, int ld_xh, int ld_gp) {
    const int cq = C >> 2, total = rows * cq;
    for (int i = blockIdx.x * NT + threadIdx.x; i < total; i += gridDim.x * NT) {
        const int row = i / cq, col = (i - row * cq) * 4;
        const f32x4 gv = ld4(g + (size_t)row * ld_g + col), xv = ld4(xh + (size_t)row * ld_xh + col), db = ld4(dbeta + col),
                    dg = ld4(dgamma + col);
        const float k = keep ? keep[row / M] : 1.f;
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = __fmaf_rn(-xv[e], dg[e] * inv_rows, __fmaf_rn(gv[e], k, -(db[e] * inv_rows)));
        st4(gp + (size_t)row * ld_gp + col, o);
    }
}

// the per-image column sums under the per-image scale, in image order
__global__ __launch_bounds__(NT) void bn_sums_kernel(const float* __restrict__ sum_g, const float* __restrict__ sum_ga,
                                                     const float* __restrict__ keep, float* __restrict__ dbeta, float* __restrict__ dgamma,
                                                     int B, int C) {
    const int c = blockIdx.x * NT + threadIdx.x;
    if (c >= C) return;
    double s0 = 0.0, s1 = 0.0;
    for (int b = 0; b < B; ++b) {
        const double k = keep ? (double)keep[b] : 1.0;
        s0 = fma(k, (double)sum_g[(size_t)b * C + c], s0);
        s1 = fma(k, (double)sum_ga[(size_t)b * C + c], s1);
    }
    dbeta[c] = (float)s0;
    dgamma[c] = (float)s1;
}

}  // namespace

extern "C" int vfn_et_bn_stats_f32(const float* z, int M, int C, int ld, const float* gamma, double eps, double momentum, double* part,
                                   float* rstd, float* nshift, float* fold, float* running_mean, float* running_var, int c_run, void* stream) {
    if (!z || !gamma || !part || !rstd || !nshift || !fold || M < 2 || !mat_ok(M, C, ld)) return VFN_ERR_ARG;
    if ((running_mean != nullptr) != (running_var != nullptr) || c_run < 0 || c_run > C) return VFN_ERR_ARG;
    if (!(eps > 0.0) || !(momentum >= 0.0 && momentum <= 1.0)) return VFN_ERR_ARG;
    const Chunks ch = chunks_of(M, VFN_ET_MAX_BLOCKS);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(ch.nb, cdiv(C / 4, TQ)), dim3(NT), 0, s, z, M, C, ld, ch.rows, part);
    hipLaunchKernelGGL(bn_stats_final_kernel, dim3(cdiv(C, FC)), dim3(NT), 0, s, (const double*)part, ch.nb, ch.rows, M, C, gamma, eps, momentum,
                       rstd, nshift, fold, running_mean, running_var, c_run);
    return vfn_check_launch();
}

extern "C" int vfn_et_bn_norm_f32(const float* z, const float* rstd, const float* nshift, const float* gamma, const float* beta,
                                  const float* keep, const float* res, float* xh, float* y, int B, int M, int C, int ld_z, int ld_res,
                                  int ld_xh, int ld_y, int swish, void* stream) {
    if (!z || !rstd || !nshift || !gamma || !beta || !xh || !y || B < 1 || M < 1) return VFN_ERR_ARG;
    const long long rows = (long long)B * M;
    if (!mat_ok(rows, C, ld_z) || !mat_ok(rows, C, ld_xh) || !mat_ok(rows, C, ld_y) || (res && !mat_ok(rows, C, ld_res))) return VFN_ERR_ARG;
    if ((xh == z && ld_xh != ld_z) || y == z || y == xh) return VFN_ERR_ARG;
    hipLaunchKernelGGL(bn_norm_kernel, dim3(grid_for4(rows * (C / 4))), dim3(NT), 0, (hipStream_t)stream, z, rstd, nshift, gamma, beta, keep, res,
                       xh, y, (int)rows, M, C, ld_z, ld_res, ld_xh, ld_y, swish);
    return vfn_check_launch();
}

extern "C" int vfn_et_bn_sums_f32(const float* sum_g, const float* sum_ga, const float* keep, float* dbeta, float* dgamma, int B, int C,
                                  void* stream) {
    if (!sum_g || !sum_ga || !dbeta || !dgamma || B < 1 || C < 1 || (long long)B * C > 0x7fffffffll) return VFN_ERR_ARG;
    hipLaunchKernelGGL(bn_sums_kernel, dim3(cdiv(C, NT)), dim3(NT), 0, (hipStream_t)stream, sum_g, sum_ga, keep, dbeta, dgamma, B, C);
    return vfn_check_launch();
}

extern "C" int vfn_et_bn_center_f32(const float* g, const float* xh, const float* keep, const float* dbeta, const float* dgamma, float* gp,
                                    int B, int M, int C, int ld_g, int ld_xh, int ld_gp, void* stream) {
    if (!g || !xh || !dbeta || !dgamma || !gp || B < 1 || M < 1) return VFN_ERR_ARG;
    const long long rows = (long long)B * M;
    if (!mat_ok(rows, C, ld_g) || !mat_ok(rows, C, ld_xh) || !mat_ok(rows, C, ld_gp)) return VFN_ERR_ARG;
    if ((gp == g && (keep || ld_gp != ld_g)) || gp == xh) return VFN_ERR_ARG;
    hipLaunchKernelGGL(bn_center_kernel, dim3(grid_for4(rows * (C / 4))), dim3(NT), 0, (hipStream_t)stream, g, xh, keep, dbeta, dgamma, gp,
                       (float)(1.0 / (double)rows), (int)rows, M, C, ld_g, ld_xh, ld_gp);
    return vfn_check_launch();
}
