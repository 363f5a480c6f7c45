// 3x3 / stride-1 / pad-1 convolution with 32 filters and 32 or 64 input channels (the decoder's local refinement head at half
// resolution), f32, with the whole filter bank and the input patch of an output block resident in LDS (include/vfn_conv_thin.h).
//
// Why this exists.  As a tiled im2col GEMM such a layer is a 128 x 32 tile with a K loop of 9 or 18 K tiles: a barrier for every 32
// MFMAs of a wave, every input element staged nine times (once per tap), and split-K slabs where the tuner cut the last round of
// tiles.  Here a workgroup of 4 waves owns an 8 x 16 block of output pixels x all 32 filters:
//   - the filter bank [9][32][Cin] goes to LDS once per workgroup (73 KB at Cin 64, 37 KB at Cin 32);
//   - the block's 10 x 18 input patch goes to LDS once (ReLU on the input applied as it is stored, zeros outside the image) and every
//     tap reads it at an offset;
//   - a wave owns two output rows of the block (32 pixels): one 32 x 32 accumulator, 9 * Cin / 2 MFMAs with no barrier in between;
//   - the workgroup walks a list of blocks (persistent grid, one contiguous run of blocks per XCD) and requests the next block's
//     patch -- and this block's residual -- into registers from inside this block's MFMA loop.
// No split-K, no workspace, no counters; no dependency between workgroups.
//
// LDS images (bank of byte a for ds_read_b128: (a / 4) mod 64, 16 lanes per LDS cycle):
//   filters  sW[tap][filter][S], S = Cin + 4 floats: the 32 filters of a B fragment sit S / 4 = 17 (9) 16-byte chunks apart -- odd,
//            so the 16 lanes of a cycle cover the 64 banks once (a stride of exactly Cin floats would be a 32-way conflict);
//   patch    sP[row][RP] with pixel stride S and the row pitch RP rounded up to a multiple of 64 floats: the lanes of one cycle are
//            eight pixels of one patch row and the complementary eight of the next, which a pitch of 0 mod 64 keeps on disjoint banks.
//
// Summation order: taps (kh, kw), then channels in blocks of 8, per block four MFMAs on the channel pairs (c, c + 4) -- the order of
// conv_igemm_kernel without split-K.
#include "common.h"
#include "conv_internal.h"
#include "../../include/vfn_conv_thin.h"

template <int CIN>
struct thin_geom {
    static constexpr int TH = 8, TW = 16;                        // output block: 4 waves x (2 rows x 16 pixels)
    static constexpr int PH = TH + 2, PW = TW + 2;               // input patch
    static constexpr int S = CIN + 4;                            // pixel / filter stride in LDS, floats
    static constexpr int RP = (PW * S + 63) / 64 * 64;           // patch row pitch, floats
    static constexpr int CH = CIN / 4;                           // 16-byte chunks per pixel
    static constexpr int NCH = PH * PW * CH;                     // chunks per patch
    static constexpr int PC = (NCH + 255) / 256;                 // chunks per thread
    static constexpr int W_FLOATS = 9 * 32 * S;
    static constexpr int P_FLOATS = PH * RP;
    static constexpr size_t LDS_BYTES = (size_t)(W_FLOATS + P_FLOATS) * sizeof(float);
};

template <int CIN>
__global__ __launch_bounds__(256)
void conv_thin3x3_kernel(const vfn_conv_desc p, int tiles_x, int tiles_y, int total, int res_imgs) {
    using G = thin_geom<CIN>;
    constexpr int S = G::S, RP = G::RP, CH = G::CH, PC = G::PC;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sW = reinterpret_cast<float*>(smem);                  // [9][32][S]
    float* sP = sW + G::W_FLOATS;                                // [PH][RP]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;

    // blocks of this workgroup: XCD x (= blockIdx % 8) owns one contiguous run of the block list (x fastest, then y, then image:
    // neighbours share their halo through one L2), dealt round-robin to its workgroups; a grid that is no multiple of 8 strides plainly
    int first, step, n_my;
    if ((gridDim.x & 7) == 0) {
        const int gx = (int)gridDim.x >> 3, xcd = (int)blockIdx.x & 7, loc = (int)blockIdx.x >> 3;
        const int q = total >> 3, r8 = total & 7;
        const int u_begin = xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q;
        const int u_end = u_begin + q + (xcd < r8 ? 1 : 0);
        first = u_begin + loc;
        step = gx;
        n_my = first < u_end ? (u_end - first + gx - 1) / gx : 0;
    } else {
        first = blockIdx.x;
        step = gridDim.x;
        n_my = first < total ? (total - first + step - 1) / step : 0;
    }
    if (n_my == 0) return;

    constexpr int OOB = 0x7ffffff0;                              // an offset past every buffer: the load returns zeros
    const __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.in), 0, (int)((size_t)p.N * p.H * p.W * p.in_ld * sizeof(float)), 0x00020000);
    // (no residual: a buffer of no bytes, every load returns zero)
    const int res_rows = res_imgs > 0 ? res_imgs * p.H * p.W : p.M;
    const __amdgpu_buffer_rsrc_t rs_res = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.res), 0, p.res ? (int)((size_t)res_rows * p.res_ld * sizeof(float)) : 0, 0x00020000);

    // this thread's share of a patch, fixed for the kernel's life: chunk q = tid + 256 j is channels 4 (q % CH) .. + 3 of patch pixel
    // q / CH = (py, px); its place in LDS and its byte offset from the patch's first pixel in memory.  A chunk past the patch gets a
    // row no image has
    int c_py[PC], c_px[PC], c_lds[PC], c_off[PC];
#pragma unroll
    for (int j = 0; j < PC; ++j) {
        const int q = tid + j * 256;
        const int pix = q / CH, ch = q - pix * CH;
        const int py = pix / G::PW, px = pix - py * G::PW;
        c_py[j] = q < G::NCH ? py : (1 << 29);
        c_px[j] = px;
        c_lds[j] = py * RP + px * S + ch * 4;
        c_off[j] = ((py * p.W + px) * p.in_ld + ch * 4) * (int)sizeof(float);
    }
    struct blk { int n, y0, x0; };                               // image and first pixel of a block
    auto block_of = [&](int t) {
        const int tx = t % tiles_x, tyn = t / tiles_x;
        return blk{tyn / tiles_y, (tyn % tiles_y) * G::TH, tx * G::TW};
    };
    // one chunk of the patch of block b on its way into a register: outside the image (and `live` false: no block follows) zeros
    auto load_chunk = [&](const blk& b, bool live, int j, f32x4& r) {
        const int base = (((b.n * p.H + b.y0 - 1) * p.W + b.x0 - 1) * p.in_ld) * (int)sizeof(float);      // (wave-uniform)
        const bool ok = live && (unsigned)(b.y0 - 1 + c_py[j]) < (unsigned)p.H && (unsigned)(b.x0 - 1 + c_px[j]) < (unsigned)p.W;
        r = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_in, ok ? base + c_off[j] : OOB, 0, 0));
    };
    const float relu_floor = p.relu_in ? 0.f : -INFINITY;     // ReLU on the input: once, as the patch is stored
    auto store_patch = [&](const f32x4 (&r)[PC]) {
#pragma unroll
        for (int j = 0; j < PC; ++j) {
            if ((j + 1) * 256 <= G::NCH || tid + j * 256 < G::NCH) {      // (only the last chunk of a thread may lie past the patch)
                f32x4 v = r[j];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = vfn_floor_nan(v[e], relu_floor);
                *reinterpret_cast<f32x4*>(sP + c_lds[j]) = v;
            }
        }
    };

    f32x4 pre[PC];
    {
        const blk b0 = block_of(first);
#pragma unroll
        for (int j = 0; j < PC; ++j) load_chunk(b0, true, j, pre[j]);
    }

    // the filter bank: w [32][9 * CIN], K ordered (kh, kw, cin) -> sW[tap][filter][S]; every load issued before the first store
    {
        constexpr int WC = 32 * 9 * CH / 256;
        static_assert(WC * 256 == 32 * 9 * CH, "the filter bank is a whole number of chunks per thread");
        f32x4 wv[WC];
#pragma unroll
        for (int j = 0; j < WC; ++j) wv[j] = *reinterpret_cast<const f32x4*>(p.w + (size_t)(tid + j * 256) * 4);
#pragma unroll
        for (int j = 0; j < WC; ++j) {
            const int q = tid + j * 256;
            const int f = q / (9 * CH), k4 = q - f * (9 * CH);
            const int tap = k4 / CH, ch = k4 - tap * CH;
            *reinterpret_cast<f32x4*>(sW + (tap * 32 + f) * S + ch * 4) = wv[j];
        }
    }

    const float sc = p.scale ? p.scale[li] : 1.f;
    const float sh = p.shift ? p.shift[li] : 0.f;
    // MFMA row li of this wave is pixel (2 * wave + li / 16, li % 16) of the block; lane half lh holds channels 4 lh .. 4 lh + 3 of
    // every 8-channel block
    const float* aBase = sP + (2 * wave + (li >> 4)) * RP + (li & 15) * S + 4 * lh;
    const float* bBase = sW + li * S + 4 * lh;
    constexpr int KB = CIN / 8, STEPS = 9 * KB;
    // What else a block needs from memory is requested from inside its MFMA loop, one load per step, where the address arithmetic
    // issues in the shadow of the MFMAs: the block's residual in steps 0 .. 15, the next block's patch chunks after them
    constexpr int PSTEP = (STEPS - 1 - 16) / PC;                 // steps between two patch chunks
    static_assert(PSTEP >= 1, "more patch chunks than steps left");

    for (int i = 0; i < n_my; ++i) {
        const int t = first + i * step;
        store_patch(pre);                                        // (the patch is free: the barrier that ends the previous block)
        __syncthreads();
        const bool has_next = i + 1 < n_my;
        const blk b = block_of(t), bn = block_of(has_next ? t + step : t);
        // accumulator register r of a lane: pixel (r & 3) + 8 (r >> 2) + 4 lh of the wave's 32 = row r >> 3 of the wave's two, column
        // (r & 3) + 8 ((r >> 2) & 1) + 4 lh
        const int y_w = b.y0 + 2 * wave, x_l = b.x0 + 4 * lh;
        const int nr = res_imgs > 0 ? b.n % res_imgs : b.n;      // (res_mod: the residual repeats every res_imgs images)
        const int res_pix = (nr * p.H + y_w) * p.W + x_l, out_pix = (b.n * p.H + y_w) * p.W + x_l;
        float rv[16];

        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        // the fragments of step s + 1 are read before the MFMAs of step s are issued
        auto read_frags = [&](int s, f32x4& a, f32x4& bf) {
            const int tap = s / KB, kb = s - tap * KB;
            const int kh = tap / 3, kw = tap - kh * 3;
            a = *reinterpret_cast<const f32x4*>(aBase + kh * RP + kw * S + kb * 8);
            bf = *reinterpret_cast<const f32x4*>(bBase + tap * 32 * S + kb * 8);
        };
        f32x4 fa[2], fb[2];
        read_frags(0, fa[0], fb[0]);
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
            if (s + 1 < STEPS) read_frags(s + 1, fa[(s + 1) & 1], fb[(s + 1) & 1]);
            if (s < 16) {
                const int dy = s >> 3, dx = (s & 3) + 8 * ((s >> 2) & 1);
                const bool ok = y_w + dy < p.H && x_l + dx < p.W;
                rv[s] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                    rs_res, ok ? ((res_pix + dy * p.W + dx) * p.res_ld + li) * (int)sizeof(float) : OOB, 0, 0));
            } else if ((s - 16) % PSTEP == 0 && (s - 16) / PSTEP < PC) {
                load_chunk(bn, has_next, (s - 16) / PSTEP, pre[(s - 16) / PSTEP]);
            }
            __builtin_amdgcn_sched_barrier(0);                   // (pinned: left alone, the scheduler reads four fragments and waits)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s & 1][e], fb[s & 1][e], acc, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }

        // epilogue: lane holds filter li of its 16 pixels
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int dy = r >> 3, dx = (r & 3) + 8 * ((r >> 2) & 1);
            if (y_w + dy < p.H && x_l + dx < p.W) {
                float v = acc[r] * sc + sh;
                if (p.res) v += rv[r];
                if (p.relu_out) v = fmaxf(v, 0.f);
                p.out[(size_t)(out_pix + dy * p.W + dx) * p.out_ld + li] = v;
            }
        }
        __syncthreads();                                         // every wave is done with the patch
    }
}

template <int CIN>
static int launch_thin(const vfn_conv_desc& d, int wgs, hipStream_t s) {
    using G = thin_geom<CIN>;
    static const bool lds_ok = vfn_allow_lds(conv_thin3x3_kernel<CIN>, G::LDS_BYTES);
    (void)lds_ok;
    const int tiles_x = (d.W + G::TW - 1) / G::TW, tiles_y = (d.H + G::TH - 1) / G::TH;
    const long long total = (long long)d.N * tiles_y * tiles_x;
    if (total >= 0x7fffff00LL) return VFN_ERR_ARG;
    int grid = wgs > 0 ? wgs : 256;
    if (grid > total) grid = (int)total;
    if (grid >= 8) grid &= ~7;
    const int res_imgs = (d.res && d.res_mod > 0) ? d.res_mod / (d.H * d.W) : 0;
    hipLaunchKernelGGL(conv_thin3x3_kernel<CIN>, dim3(grid), dim3(256), G::LDS_BYTES, s, d, tiles_x, tiles_y, (int)total, res_imgs);
    return vfn_check_launch();
}

extern "C" int vfn_conv3x3_thin_f32(const vfn_conv_desc* d, int cfg, void* stream) {
    if (!d || !d->in || !d->w || !d->out || cfg < 0 || cfg > VFN_THIN3X3_MAX_WGS) return VFN_ERR_ARG;
    if (d->KH != 3 || d->KW != 3 || d->stride != 1 || d->pad != 1 || d->Cout != 32 || d->cout_pad < 32 || (d->Cin != 32 && d->Cin != 64))
        return VFN_ERR_ARG;
    if (d->N < 1 || d->H < 1 || d->W < 1 || d->Ho != d->H || d->Wo != d->W || d->M != d->N * d->H * d->W) return VFN_ERR_ARG;
    if (d->in_ld < d->Cin || d->in_ld % 4 || d->out_ld < 32) return VFN_ERR_ARG;
    if (d->mask || d->in_lp || d->out_lp || d->w_packed || d->w_batch_rows || d->ksplit > 1) return VFN_ERR_ARG;
    const long long hw = (long long)d->H * d->W, lim = 0x7fffff00LL;
    if (d->res && (d->res_ld < 32 || d->res_mod < 0 || (d->res_mod > 0 && d->res_mod % hw))) return VFN_ERR_ARG;
    if ((long long)d->M * d->in_ld * 4 >= lim || (long long)d->M * d->out_ld * 4 >= lim ||
        (d->res && (d->res_mod > 0 ? d->res_mod : (long long)d->M) * d->res_ld * 4 >= lim)) return VFN_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(d->in) | reinterpret_cast<uintptr_t>(d->w)) & 15) return VFN_ERR_ARG;
    return d->Cin == 64 ? launch_thin<64>(*d, cfg, (hipStream_t)stream) : launch_thin<32>(*d, cfg, (hipStream_t)stream);
}
