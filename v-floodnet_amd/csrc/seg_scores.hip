// Scores of a batch of the image model (train_image_seg.py:134-137: smp's DiceLoss() and IoU(threshold=0.5)): five sums over
// the probabilities and the labels in float64, in a fixed order, then loss and score into a row of a device log.  Rules:
// include/vfn_image_val.h.  Bandwidth-bound: 8 bytes read per element, a few hundred bytes written.
#include "common.h"
#include "../../include/vfn_image_val.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// workgroup j: elements j * chunk .. min((j + 1) * chunk, n) - 1, a strided walk per thread, butterfly per wavefront, the four
// wavefronts in order -> part[j][0..4]
__global__ void __launch_bounds__(256) seg_scores_part_kernel(const float* __restrict__ pr, const float* __restrict__ gt, int n,
                                                              int chunk, float threshold, double* __restrict__ part) {
    __shared__ double red[4][5];
    const long long first = (long long)blockIdx.x * chunk;
    const long long last = first + chunk < (long long)n ? first + chunk : (long long)n;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long i = first + threadIdx.x; i < last; i += 256) {
        const float p = pr[i];
        const double pd = (double)p, gd = (double)gt[i];
        const double b = p > threshold ? 1.0 : 0.0;
        s[0] += gd * pd, s[1] += pd, s[2] += gd, s[3] += gd * b, s[4] += b;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        s[k] = wave_sum_d(s[k]);
        if (lane == 0) red[wave][k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        const int k = threadIdx.x;
        part[(size_t)blockIdx.x * 5 + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    }
}

// one workgroup of 64: lane k < 5 adds part[0][k], part[1][k], ... in that order; lane 0 then forms loss and score
__global__ void __launch_bounds__(64) seg_scores_fold_kernel(const double* __restrict__ part, int nb, double* __restrict__ sums,
                                                             double* __restrict__ log_row) {
    __shared__ double S[5];
    if (threadIdx.x < 5) {
        double a = 0.0;
        for (int j = 0; j < nb; ++j) a += part[(size_t)j * 5 + threadIdx.x];
        S[threadIdx.x] = a;
        if (sums) sums[threadIdx.x] = a;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        log_row[0] = 1.0 - (2.0 * S[0] + 1.0) / (S[1] + S[2] + 1.0);
        log_row[1] = (S[3] + 1e-7) / (S[2] + S[4] - S[3] + 1e-7);
    }
}

}  // namespace

extern "C" int vfn_seg_scores_f64(const float* pr, const float* gt, int n, float threshold, double* part, double* sums, double* log,
                                  int rows, int t, void* stream) {
    if (!pr || !gt || !part || !log || n < 1 || !isfinite(threshold) || rows < 1 || t < 0 || t >= rows) return VFN_ERR_ARG;
    const long long want = ((long long)n + VFN_SEG_SCORES_CHUNK - 1) / VFN_SEG_SCORES_CHUNK;
    const int nb = (int)(want < VFN_SEG_SCORES_MAX_BLOCKS ? want : VFN_SEG_SCORES_MAX_BLOCKS);
    const int chunk = (int)(((long long)n + nb - 1) / nb);
    hipLaunchKernelGGL(seg_scores_part_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, pr, gt, n, chunk, threshold, part);
    hipLaunchKernelGGL(seg_scores_fold_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, part, nb, sums, log + (size_t)t * 2);
    return vfn_check_launch();
}
