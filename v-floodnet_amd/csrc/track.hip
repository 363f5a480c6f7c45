// Reference-box tracker of the water-level estimator: translation-only zero-mean normalised cross-correlation against a slowly
// adapting template, stated in integers in include/vfn_hip.h (NOT cv2.TrackerCSRT, which estimation/reference_tracking.py:104-107
// and :183-188 run: no scale or rotation adaptation, and no agreement with OpenCV's boxes is claimed).
//   vfn_track_luma_f32   the loop's frame float [3][H][W] -> luma uint8 [H][W]
//   vfn_track_init       boxes from the host, T16 = luma << 8 under each box
//   vfn_track_update     search (track_search_kernel), then arg-max, failure test, box move, template update and the three log
//                        rows (track_finish_kernel); the previous box is read on the device, nothing is reported to the host
// The search is the cost: (2S+1)^2 candidates x w h pixels x four sums.  A workgroup takes 256 candidates (one per lane) and one
// 64 x 32 tile of the template; the tile's T16, split into its high and low bytes, and the (64+2S) x (32+2S) luma window around
// it sit in the LDS, and v_dot4_u32_u8 carries the four sums (sum Th P, sum Tl P, sum P, sum P^2) four pixels at a time.  The
// sums are integers, so the per-tile partial sums are added with integer atomics: any order gives the same bits.
#include "common.h"
#include "../../include/vfn_hip.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int TW = 64, TH = 32;                        // template tile
constexpr int SMAX = VFN_TRACK_MAX_RADIUS;
constexpr int WIN_ROWS = TH + 2 * SMAX;                // 96
constexpr int WIN_PITCH = (TW + 2 * SMAX) / 4 + 1;     // 33 dwords: the dword behind the last pixel is read (and shifted out) by
                                                       // the unaligned fetch; an odd pitch puts the rows on different banks
constexpr int SEARCH_THREADS = 256, FINISH_THREADS = 1024;

struct TrackRefs {                                     // fixed for the clip, from the host
    int n;
    int w[VFN_WL_MAX_REFS], h[VFN_WL_MAX_REFS];
    long long t16_off[VFN_WL_MAX_REFS];                // element offset of reference r's template in the t16 buffer
};
struct TrackBoxes { int v[VFN_WL_MAX_REFS][4]; };

__global__ void track_luma_kernel(const float* __restrict__ frame, unsigned char* __restrict__ luma, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned r = (unsigned char)(frame[i] * 255.0f), g = (unsigned char)(frame[(size_t)n + i] * 255.0f),
                   b = (unsigned char)(frame[2 * (size_t)n + i] * 255.0f);
    luma[i] = (unsigned char)((19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16);
}

// grid (ceil(max w h / 256), R)
__global__ void track_init_kernel(const unsigned char* __restrict__ luma, int W, TrackRefs P, TrackBoxes B,
                                  int* __restrict__ box_state, unsigned short* __restrict__ t16) {
    const int r = blockIdx.y, w = P.w[r], h = P.h[r];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 4) box_state[4 * r + i] = B.v[r][i];
    if (i >= w * h) return;
    const int ty = i / w, tx = i - ty * w;
    t16[P.t16_off[r] + i] = (unsigned short)(luma[(size_t)(B.v[r][1] + ty) * W + B.v[r][0] + tx] << 8);
}

// grid (ceil((2S+1)^2 / 256), tiles of the largest template, R); acc [R][(2S+1)^2][3] += (sum P, sum P^2, sum T16 P) of the tile
__global__ void __launch_bounds__(SEARCH_THREADS)
track_search_kernel(const unsigned char* __restrict__ luma, int H, int W, TrackRefs P, int S, const int* __restrict__ box_state,
                    const unsigned short* __restrict__ t16, unsigned long long* __restrict__ acc) {
    __shared__ unsigned win[WIN_ROWS * WIN_PITCH];     // luma window, 4 pixels a dword; 0 outside the image
    __shared__ unsigned t_hi[TH * TW / 4], t_lo[TH * TW / 4];      // T16 >> 8 and T16 & 255 of the tile; 0 outside the template
    const int r = blockIdx.z, w = P.w[r], h = P.h[r];
    const int tiles_x = (w + TW - 1) / TW, tiles_y = (h + TH - 1) / TH;
    if ((int)blockIdx.y >= tiles_x * tiles_y) return;                        // (grid sized for the largest template)
    const int tx0 = ((int)blockIdx.y % tiles_x) * TW, ty0 = ((int)blockIdx.y / tiles_x) * TH;
    const int tw = min(TW, w - tx0), th = min(TH, h - ty0);
    const int x = box_state[4 * r], y = box_state[4 * r + 1];
    const int side = 2 * S + 1, ncand = side * side, tid = threadIdx.x;

    // window pixel (row i, column j) = luma(y + ty0 - S + i, x + tx0 - S + j), i < th + 2S, j < tw + 2S rounded up to dwords
    const int wrows = th + 2 * S, wcols4 = (tw + 2 * S + 3) / 4 + 1;
    const long long gx0 = (long long)x + tx0 - S, gy0 = (long long)y + ty0 - S;
    unsigned char* win8 = reinterpret_cast<unsigned char*>(win);
    for (int k = tid; k < wrows * wcols4 * 4; k += SEARCH_THREADS) {
        const int i = k / (wcols4 * 4), j = k - i * (wcols4 * 4);
        const long long gy = gy0 + i, gx = gx0 + j;
        win8[i * (WIN_PITCH * 4) + j] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? luma[(size_t)gy * W + gx] : 0;
    }
    unsigned char* hi8 = reinterpret_cast<unsigned char*>(t_hi);
    unsigned char* lo8 = reinterpret_cast<unsigned char*>(t_lo);
    const unsigned short* tpl = t16 + P.t16_off[r];
    const int tw4 = (tw + 3) / 4;
    for (int k = tid; k < th * tw4 * 4; k += SEARCH_THREADS) {
        const int i = k / (tw4 * 4), j = k - i * (tw4 * 4);
        const unsigned v = j < tw ? tpl[(size_t)(ty0 + i) * w + tx0 + j] : 0;
        hi8[i * TW + j] = (unsigned char)(v >> 8);
        lo8[i * TW + j] = (unsigned char)(v & 255);
    }
    __syncthreads();

    const int ci = blockIdx.x * SEARCH_THREADS + tid;
    const int cc = min(ci, ncand - 1);                                       // (lanes past the last candidate redo it and add nothing)
    const int c0 = cc % side, r0 = cc / side;                                // dx + S, dy + S
    const int base = c0 >> 2, sh = c0 & 3;
    const int full = tw / 4, rem = tw & 3;
    const unsigned tail_ones = (1u << (8 * rem)) - 1u & 0x01010101u, tail_mask = (1u << (8 * rem)) - 1u;
    unsigned long long sB = 0, sE = 0, sC = 0;
    // per row: at most 64 pixels, so 64 * 255 * 255 < 2^23 in 32 bits; the 64-bit totals take a row at a time
    for (int i = 0; i < th; ++i) {
        const unsigned* row = win + (r0 + i) * WIN_PITCH + base;
        const unsigned* hrow = t_hi + i * (TW / 4);
        const unsigned* lrow = t_lo + i * (TW / 4);
        unsigned b = 0, e = 0, ch = 0, cl = 0;
        unsigned lo = row[0];
        int j = 0;
        for (; j < full; ++j) {
            const unsigned hi = row[j + 1];
            const unsigned p = __builtin_amdgcn_alignbyte(hi, lo, sh);       // the four pixels from byte sh of (hi:lo)
            ch = __builtin_amdgcn_udot4(hrow[j], p, ch, false);
            cl = __builtin_amdgcn_udot4(lrow[j], p, cl, false);
            b = __builtin_amdgcn_udot4(0x01010101u, p, b, false);
            e = __builtin_amdgcn_udot4(p, p, e, false);
            lo = hi;
        }
        if (rem) {                                                           // a width that is no multiple of 4: the template's
            const unsigned hi = row[j + 1];                                  // bytes past it are 0, the pixels are masked
            const unsigned p = __builtin_amdgcn_alignbyte(hi, lo, sh) & tail_mask;
            ch = __builtin_amdgcn_udot4(hrow[j], p, ch, false);
            cl = __builtin_amdgcn_udot4(lrow[j], p, cl, false);
            b = __builtin_amdgcn_udot4(tail_ones, p, b, false);
            e = __builtin_amdgcn_udot4(p, p, e, false);
        }
        sB += b, sE += e, sC += ((unsigned long long)ch << 8) + cl;
    }
    if (ci < ncand) {
        unsigned long long* a = acc + ((size_t)r * ncand + ci) * 3;
        atomicAdd(a, sB), atomicAdd(a + 1, sE), atomicAdd(a + 2, sC);
    }
}

struct Best { double key; int idx; };
__device__ __forceinline__ bool better(const Best& a, const Best& b) {      // larger key; on a tie the earlier candidate
    return a.key > b.key || (a.key == b.key && a.idx < b.idx);
}

// one workgroup per reference; leaves acc zero for the next frame
__global__ void __launch_bounds__(FINISH_THREADS)
track_finish_kernel(const unsigned char* __restrict__ luma, int H, int W, TrackRefs P, int S, int* __restrict__ box_state,
                    unsigned short* __restrict__ t16, unsigned long long* __restrict__ acc, int* __restrict__ box_log,
                    int* __restrict__ ok_log, float* __restrict__ score_log) {
#pragma clang fp contract(off)
    __shared__ long long red_a[FINISH_THREADS], red_d[FINISH_THREADS];
    __shared__ Best red_b[FINISH_THREADS];
    __shared__ long long win_num, win_vp;
    __shared__ int moved[3];
    const int r = blockIdx.x, tid = threadIdx.x, w = P.w[r], h = P.h[r], n = w * h;
    const int x = box_state[4 * r], y = box_state[4 * r + 1];
    unsigned short* tpl = t16 + P.t16_off[r];

    long long a = 0, d = 0;
    for (int i = tid; i < n; i += FINISH_THREADS) {
        const long long v = tpl[i];
        a += v, d += v * v;
    }
    red_a[tid] = a, red_d[tid] = d;
    __syncthreads();
    for (int o = FINISH_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red_a[tid] += red_a[tid + o], red_d[tid] += red_d[tid + o];
        __syncthreads();
    }
    const long long A = red_a[0], D = red_d[0], N = n;

    const int side = 2 * S + 1, ncand = side * side;
    Best best = {-INFINITY, INT_MAX};
    long long best_num = 0, best_vp = 0;
    for (int ci = tid; ci < ncand; ci += FINISH_THREADS) {                   // ascending, so a strict > keeps the first
        unsigned long long* s = acc + ((size_t)r * ncand + ci) * 3;
        const long long B = (long long)s[0], E = (long long)s[1], C = (long long)s[2];
        s[0] = s[1] = s[2] = 0;
        const long long nx = (long long)x + ci % side - S, ny = (long long)y + ci / side - S;
        if (nx < 0 || ny < 0 || nx + w > W || ny + h > H) continue;
        const long long num = N * C - A * B, vp = N * E - B * B;
        if (vp == 0) continue;
        const double key = (double)num * fabs((double)num) / (double)vp;
        if (key > best.key) best = {key, ci}, best_num = num, best_vp = vp;
    }
    red_b[tid] = best;
    __syncthreads();
    for (int o = FINISH_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o && better(red_b[tid + o], red_b[tid])) red_b[tid] = red_b[tid + o];
        __syncthreads();
    }
    const Best winner = red_b[0];
    if (winner.idx != INT_MAX && winner.idx == best.idx) win_num = best_num, win_vp = best_vp;     // (its one owner)
    __syncthreads();
    if (tid == 0) {
        const double vt = (double)N * (double)D - (double)A * (double)A;
        bool ok = winner.idx != INT_MAX;
        float score = 0.f;
        int nx = x, ny = y;
        if (ok) {
            const double num = (double)win_num, vp = (double)win_vp;
            const double vv = vt * vp;
            score = (float)(num / sqrt(vv));
            ok = vt > 0.0 && win_num > 0 && !(num * num < 0.25 * vv);
            if (ok) nx = x + winner.idx % side - S, ny = y + winner.idx / side - S;
        }
        moved[0] = ok, moved[1] = nx, moved[2] = ny;
        box_state[4 * r] = nx, box_state[4 * r + 1] = ny, box_state[4 * r + 2] = w, box_state[4 * r + 3] = h;
        box_log[4 * r] = nx, box_log[4 * r + 1] = ny, box_log[4 * r + 2] = w, box_log[4 * r + 3] = h;
        ok_log[r] = ok;
        score_log[r] = score;
    }
    __syncthreads();
    if (!moved[0]) return;
    const int nx = moved[1], ny = moved[2];                                  // a valid candidate: the window lies inside the image
    for (int i = tid; i < n; i += FINISH_THREADS) {
        const int ty = i / w, tx = i - ty * w;
        const int t = tpl[i], p = luma[(size_t)(ny + ty) * W + nx + tx];
        tpl[i] = (unsigned short)(t + (((p << 8) - t + 8) >> 4));
    }
}

// sizes int32 [R][2] = (w, h) on the host -> the by-value table; false for anything outside the caps or the buffers
bool track_refs(const int* wh, int stride, int R, int S, long long t16_elems, long long acc_elems, TrackRefs& P) {
    if (!wh || R < 1 || R > VFN_WL_MAX_REFS || S < 1 || S > VFN_TRACK_MAX_RADIUS) return false;
    long long off = 0;
    P.n = R;
    for (int r = 0; r < R; ++r) {
        const int w = wh[stride * r], h = wh[stride * r + 1];
        if (w < 1 || h < 1 || w > VFN_TRACK_MAX_SIDE || h > VFN_TRACK_MAX_SIDE) return false;
        P.w[r] = w, P.h[r] = h, P.t16_off[r] = off;
        off += (long long)w * h;
    }
    const long long side = 2 * S + 1;
    return off <= t16_elems && (long long)R * side * side * 3 <= acc_elems;
}

bool image_args(const void* luma, int H, int W) { return luma && H >= 1 && W >= 1 && (long long)H * W <= INT_MAX / 4; }

}  // namespace

extern "C" int vfn_track_luma_f32(const float* frame, unsigned char* luma, int H, int W, void* stream) {
    if (!frame || !image_args(luma, H, W)) return VFN_ERR_ARG;
    hipLaunchKernelGGL(track_luma_kernel, dim3(cdiv(H * W, 256)), dim3(256), 0, (hipStream_t)stream, frame, luma, H * W);
    return vfn_check_launch();
}

extern "C" int vfn_track_init(const unsigned char* luma, int H, int W, const int* boxes, int R, int S, int* box_state,
                              unsigned short* t16, long long t16_elems, unsigned long long* acc, long long acc_elems,
                              void* stream) {
    TrackRefs P;
    if (!image_args(luma, H, W) || !box_state || !t16 || !acc || !track_refs(boxes ? boxes + 2 : nullptr, 4, R, S, t16_elems, acc_elems, P))
        return VFN_ERR_ARG;
    TrackBoxes B;
    int largest = 1;
    for (int r = 0; r < R; ++r) {
        const int x = boxes[4 * r], y = boxes[4 * r + 1];
        if (x < 0 || y < 0 || x > W - P.w[r] || y > H - P.h[r]) return VFN_ERR_ARG;      // the box lies inside the image
        B.v[r][0] = x, B.v[r][1] = y, B.v[r][2] = P.w[r], B.v[r][3] = P.h[r];
        largest = max(largest, P.w[r] * P.h[r]);
    }
    const long long side = 2 * S + 1;
    if (hipMemsetAsync(acc, 0, (size_t)R * side * side * 3 * sizeof(unsigned long long), (hipStream_t)stream) != hipSuccess)
        return VFN_ERR_LAUNCH;
    hipLaunchKernelGGL(track_init_kernel, dim3(cdiv(largest, 256), R), dim3(256), 0, (hipStream_t)stream, luma, W, P, B,
                       box_state, t16);
    return vfn_check_launch();
}

extern "C" int vfn_track_update(const unsigned char* luma, int H, int W, const int* sizes, int R, int S, int* box_state,
                                unsigned short* t16, long long t16_elems, unsigned long long* acc, long long acc_elems,
                                int* box_log, int* ok_log, float* score_log, int T, int t, void* stream) {
    TrackRefs P;
    if (!image_args(luma, H, W) || !box_state || !t16 || !acc || !box_log || !ok_log || !score_log || t < 0 || t >= T ||
        !track_refs(sizes, 2, R, S, t16_elems, acc_elems, P)) return VFN_ERR_ARG;
    int tiles = 1;
    for (int r = 0; r < R; ++r) tiles = max(tiles, cdiv(P.w[r], TW) * cdiv(P.h[r], TH));
    const int side = 2 * S + 1;
    hipLaunchKernelGGL(track_search_kernel, dim3(cdiv(side * side, SEARCH_THREADS), tiles, R), dim3(SEARCH_THREADS), 0,
                       (hipStream_t)stream, luma, H, W, P, S, box_state, t16, acc);
    hipLaunchKernelGGL(track_finish_kernel, dim3(R), dim3(FINISH_THREADS), 0, (hipStream_t)stream, luma, H, W, P, S, box_state,
                       t16, acc, box_log + (size_t)t * R * 4, ok_log + (size_t)t * R, score_log + (size_t)t * R);
    return vfn_check_launch();
}
