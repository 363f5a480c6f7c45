// Feature-bank contractions on the f32 matrix cores.
//
// (1) Memory read -- Matcher.forward, AFB_URR.py:136-178, per object:
//        p   = softmax_over_bank( keys^T q / sqrt(128) )          [B, HW]
//        mem = values p                                            [512, HW]
//        info[:,1] += log( sum_hw [p > 1e-3] + 1 )                 (update_bank side effect, :161-174)
//     The reference materialises p (648 MB at B = 100k) and makes >= 7 elementwise passes over it,
//     with an out-of-memory -> CPU fallback (:147-157).  Here p is never stored:
//        pass 1  vfn_bank_scan (mode 0) + _finish   per query column: running max m and sum l over the bank;
//                                    f32: the raw scores are also stored (score tiles, one write and one read per frame)
//        pass 2  vfn_memread_apply   scores read back (f32, memread_apply_ss_kernel) or recomputed (reduced precision,
//                                    or no score buffer), p = exp(s-m)/l in registers, hit counts by wave ballots,
//                                    O^T += P^T V on the MFMA
//        finish  vfn_memread_finish  reduce the bank-split partial O, write it (and the query
//                                    value) into the decoder input, apply the log(count+1) bump
//
// (2) Bank match -- FeatureBank.update, FeatureBank.py:63-68:
//        corr = normalize(keys)^T normalize(new_keys); argmax over the bank per new feature
//     Same GEMM with an arg-max epilogue (corr is never stored): vfn_bank_scan (mode 1) + vfn_bank_scan_finish.
//
// Layout: bank entry-major K [cap][128], V [cap][512]; queries / new keys [HW][ld]; reduced precision: the bank's
// split-bf16 image beside it (vfn_bank_refresh_lp).
// Tiling: the bank is walked in chunks of 64 entries.  Scans: persistent workgroups (two per CU) draw (bank slice, 128-query
// tile, object) items from a queue; a wave owns 32 query columns against all 64 rows of a chunk, key chunks arrive by
// LDS-DMA, double-buffered.  Apply: one workgroup = 128 query columns x one slice of the bank, 8 waves; P^T goes through
// LDS, wave w owns value channels 64w..64w+63 of all 128 queries and reads its value rows straight from global memory
// (buffer loads, two k-groups ahead).
#include "common.h"
#include "../../include/vfn_hip.h"
#include <type_traits>
#include <cstdlib>

namespace {

constexpr int DK = 128, DV = 512;
constexpr int CH = 64;      // bank entries per chunk

// [rows][128 floats] LDS image, 16-byte chunk index XOR (row & 15): conflict-free b128 fragment reads
__device__ __forceinline__ int swz(int row, int chunk) { return row * DK + ((chunk ^ (row & 15)) << 2); }

// [rows][64 floats] image (P^T): chunk index 0..15 XOR (row & 15)
__device__ __forceinline__ int swz64(int row, int chunk) { return row * CH + ((chunk ^ (row & 15)) << 2); }

// One 64 x 128 key chunk straight into its swizzled LDS image with LDS-DMA (no VGPRs): a wave
// instruction writes 1 KB = two image rows linearly, so the XOR swizzle goes on the per-lane SOURCE
// address.  Rows past `valid` re-read the last valid row (finite data; masked by the caller).
__device__ __forceinline__ void chunk_load_async(float* sK, const float* src, int valid, int wave, int lane) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int r = (wave * 8 + j) * 2 + (lane >> 5);
        const int pc = lane & 31;
        const int rr = min(r, valid - 1);
        const float* g = src + (size_t)rr * DK + ((pc ^ (r & 15)) << 2);
        __builtin_amdgcn_global_load_lds(g, sK + (wave * 8 + j) * 2 * DK, 16, 0, 0);
    }
}

// scores for this wave's 32 chunk rows (32*wr..) x 32 query columns (32*wq..): acc[r], row = (r&3)+8*(r>>2)+4*lh
__device__ __forceinline__ void score_tile(const float* sK, const float* sQ, int wr, int wq, int li, int lh, f32x16& acc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int ra = wr * 32 + li, rq = wq * 32 + li;
    f32x4 a[2], b[2];
    a[0] = *reinterpret_cast<const f32x4*>(sK + swz(ra, lh));
    b[0] = *reinterpret_cast<const f32x4*>(sQ + swz(rq, lh));
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
        const int cur = kk & 1;
        if (kk + 1 < 16) {
            a[cur ^ 1] = *reinterpret_cast<const f32x4*>(sK + swz(ra, 2 * (kk + 1) + lh));
            b[cur ^ 1] = *reinterpret_cast<const f32x4*>(sQ + swz(rq, 2 * (kk + 1) + lh));
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cur][t], b[cur][t], acc, 0, 0, 0);
    }
}

// ---- reduced-precision operands (BASELINE configs C3 / C5; precision 1 = bf16, 2 = bf16x3)
// 8 consecutive k of one operand row -> one v_mfma_f32_32x32x16_bf16 fragment.  bf16x3: x = hi + lo (two bf16,
// 16 significant bits); a product is hi*hi + hi*lo + lo*hi, the 2^-16 lo*lo term is dropped.
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

__device__ __forceinline__ bf16x8 cvt8(const f32x4& a, const f32x4& b) {
    bf16x8 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) { r[e] = (__bf16)a[e]; r[4 + e] = (__bf16)b[e]; }
    return r;
}
__device__ __forceinline__ void split8(const f32x4& a, const f32x4& b, bf16x8& h, bf16x8& l) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const __bf16 x = (__bf16)a[e], y = (__bf16)b[e];
        h[e] = x; h[4 + e] = y;
        l[e] = (__bf16)(a[e] - (float)x); l[4 + e] = (__bf16)(b[e] - (float)y);
    }
}
// A key chunk that has landed in LDS as f32 ([64 rows][128], 16-byte chunks XOR-swizzled by row & 15) is converted ONCE,
// in place, into the operand image the reduced-precision MFMAs read: per row 128 bf16 "hi" in the first 256 bytes and (bf16x3)
// 128 bf16 "lo" in the second, 16-byte chunks (8 consecutive k) again swizzled by row & 15.  Before, every wave split the
// fragments it read in registers -- the same key row was converted by every wave that used it (4x in the scan and in the
// 128-query apply kernel) and the conversion VALU equalled the MFMA time of the score GEMM.  NT threads, two barriers.
__device__ __forceinline__ int swzk(int row, int half, int chunk) { return row * 512 + half * 256 + ((chunk ^ (row & 15)) << 4); }   // bytes
// rows of 256 B (query image; hi plane of a key chunk): 16-byte chunk index XOR (row & 15)
__device__ __forceinline__ int swzq(int row, int chunk) { return row * 256 + ((chunk ^ (row & 15)) << 4); }          // bytes
// P^T rows of 128 B (reduced-precision apply kernels).  k is in natural order everywhere: step g of a 32x32x16 MFMA takes
// k = 16g + 8*(lane>>5) + j.
__device__ __forceinline__ int swzp(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }    // bytes

template <int NT, bool X3>
__device__ __forceinline__ void convert_chunk_inplace(float* sK, int tid) {
    constexpr int TPR = NT / CH;                   // threads per row (4 or 8)
    constexpr int F4 = 32 / TPR;                   // float4 per thread (8 or 4)
    const int r = tid / TPR, part = tid % TPR;
    f32x4 v[F4];
#pragma unroll
    for (int j = 0; j < F4; ++j) v[j] = *reinterpret_cast<const f32x4*>(sK + swz(r, part * F4 + j));
    __syncthreads();                               // every f32 value is in registers before the image is overwritten
    char* base = reinterpret_cast<char*>(sK);
#pragma unroll
    for (int j = 0; j < F4; j += 2) {
        bf16x8 h, l;
        split8(v[j], v[j + 1], h, l);
        const int chunk = (part * F4 + j) >> 1;    // 8 consecutive k = one 16-byte bf16 chunk
        *reinterpret_cast<bf16x8*>(base + swzk(r, 0, chunk)) = h;
        if constexpr (X3) *reinterpret_cast<bf16x8*>(base + swzk(r, 1, chunk)) = l;
    }
    __syncthreads();
}

template <bool X3>
__device__ __forceinline__ void mfma_lp(f32x16& acc, const bf16x8& ah, const bf16x8& al, const bf16x8& bh, const bf16x8& bl) {
    if constexpr (X3) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
}

// exp for the softmax inner loops: v_exp_f32 on x*log2(e) (1 ulp hardware exp2; the f32 product adds at most
// |x| * 6e-8 relative error, i.e. < 1e-6 where exp(x) still matters) -- the full-range expf is 10x the instructions
__device__ __forceinline__ float fast_exp(float x) { return __expf(x); }

__device__ __forceinline__ void chunk_range(int B, int nsplit, int split, int& c_lo, int& c_hi) {
    const int nchunks = (B + CH - 1) / CH;
    const int per = (nchunks + nsplit - 1) / nsplit;
    c_lo = split * per;
    c_hi = min(nchunks, c_lo + per);
}

// ------------------------------------------------------------------ pass 1: softmax statistics
// MODE 0: (max, sum exp) of scale*s per query.  MODE 1: arg-max of s*rowscale[b] per query.
// One workgroup = 128 query columns x one slice of the bank; wave w owns queries 32w..32w+31 against ALL 64 rows of
// every chunk (two 32x32 accumulator tiles), so a key fragment read from LDS feeds eight MFMAs, a key chunk is
// streamed once per 128 queries, and a query's statistics never leave its lane pair (no cross-wave reduction).
// Query fragments live in registers (64 VGPRs), key chunks are double-buffered in LDS by LDS-DMA:
// 64 KB of LDS -> two workgroups per CU, one barrier per chunk, the next chunk lands behind the MFMAs.
constexpr int QTS = 128;    // query columns per scan workgroup

#ifdef VFN_CENSUS
__device__ unsigned long long vfn_census_buf[4096 * 4];
#endif

// GATHER (MODE 1, f32): the query columns of an object are those listed in gather.list[obj][0 .. count[obj]) (the columns the
// certified match could not settle, vfn_bank_match_certified); part is written at the LIST position.  Same products in the same
// order per (entry, column) as the full scan.
struct scan_gather { const int* list; const int* count; };

template <int MODE, int PREC = 0, bool GATHER = false>
__global__ __launch_bounds__(256, 2)
void bank_scan_kernel(const vfn_bankscan_desc p, const scan_gather gather) {
#ifdef VFN_CENSUS
    const unsigned long long census_t0 = __builtin_amdgcn_s_memrealtime();
#endif
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sKb = reinterpret_cast<float*>(smem);     // [2][64][128]
    __shared__ int s_item;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    // Persistent workgroups (two per CU) pull work items from a queue: item = (bank slice, query tile, object), slice
    // slowest, so the workgroups that run at the same time walk the same part of the bank (L2).  A census of the former
    // one-workgroup-per-(tile, slice) grid showed why it ran at 0.63 MFMA utilisation: two workgroups sharing a CU keep
    // the matrix pipe 100 % busy, one alone only 71 %, and with 754 (or 494) equal workgroups on 512 slots the last
    // third of the kernel ran half-empty.  With ~2000 small items every slot stays paired until the queue is dry.
    // An item's result depends only on the item, so the output is bit-identical whichever workgroup computes it.
    const int qtiles = (p.HW + QTS - 1) / QTS;
    int total = p.nsplit * qtiles * p.obj_n;
    if constexpr (GATHER) {                            // per object: nsplit x ceil(count / 128) items, object by object
        total = 0;
        for (int o = 0; o < p.obj_n; ++o) total += p.nsplit * ((gather.count[o] + QTS - 1) / QTS);
    }
  for (;;) {
    if (tid == 0) s_item = atomicAdd(p.work_counter, 1);
    __syncthreads();
    int item = s_item;
    __syncthreads();                                   // (everyone has the item before thread 0 draws the next one)
    if (item >= total) break;
    int obj, qt, split;
    if constexpr (GATHER) {
        obj = 0;
        for (;;) {
            const int n = p.nsplit * ((gather.count[obj] + QTS - 1) / QTS);
            if (item < n) break;
            item -= n; ++obj;
        }
        const int qtl = (gather.count[obj] + QTS - 1) / QTS;
        qt = item % qtl;
        split = item / qtl;
    } else {
        obj = item % p.obj_n;
        qt = (item / p.obj_n) % qtiles;
        split = item / (p.obj_n * qtiles);
    }
    const int q0 = qt * QTS + wave * 32;             // first query of this wave (GATHER: first list position)
    const int ncol = GATHER ? gather.count[obj] : p.HW;
    const int B = p.bank_len[obj];
    // reduced precision with a kept split-bf16 image of the keys (vfn_bank_refresh_lp): same bytes per row as f32, the
    // chunk lands in LDS as the operand image itself (hi | lo halves, chunks swizzled like swzk)
    const bool lp_image = PREC != 0 && p.bank_k_lp != nullptr;
    const float* K = (lp_image ? reinterpret_cast<const float*>(p.bank_k_lp) : p.bank_k) + (size_t)obj * p.stride_k;
    const float* Q = p.q + (size_t)(p.q_per_obj ? obj : 0) * p.stride_q;

    int c_lo, c_hi;
    chunk_range(B, p.nsplit, split, c_lo, c_hi);
    if (c_lo < c_hi) chunk_load_async(sKb, K + (size_t)c_lo * CH * DK, min(CH, B - c_lo * CH), wave, lane);

    // B operand: this lane's query column, k = 8kk + 4lh + t (f32) / k = 16g + 8lh + j (bf16 fragments)
    f32x4 qf[PREC == 0 ? 16 : 1];
    bf16x8 qh[PREC == 0 ? 1 : 8], ql[PREC == 2 ? 8 : 1];
    {
        int q = min(q0 + li, ncol - 1);                          // columns past HW are never written out
        if constexpr (GATHER) q = gather.list[(size_t)obj * p.HW + q];
        if constexpr (PREC == 0) {
            const float* qrow = Q + (size_t)q * p.ldq + 4 * lh;
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) qf[kk] = *reinterpret_cast<const f32x4*>(qrow + 8 * kk);
        } else {
            const float* qrow = Q + (size_t)q * p.ldq + 8 * lh;
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const f32x4 x0 = *reinterpret_cast<const f32x4*>(qrow + 16 * g);
                const f32x4 x1 = *reinterpret_cast<const f32x4*>(qrow + 16 * g + 4);
                if constexpr (PREC == 2) split8(x0, x1, qh[g], ql[g]);
                else qh[g] = cvt8(x0, x1);
            }
        }
    }

    float run_m = -INFINITY, run_l = 0.f;
    int run_i = 0x7fffffff;
    float run_2 = -INFINITY;                           // MODE 2: runner-up score
    bool sick = false;                                 // MODE 2: a live entry of the slice has a zero / non-finite norm
    __syncthreads();                                   // chunk c_lo landed (the barrier drains the LDS-DMA)

    for (int c = c_lo; c < c_hi; ++c) {
        const int b0 = c * CH;
        const float* sK = sKb + ((c - c_lo) & 1) * CH * DK;
#ifndef VFN_ABLATE_KLOAD
        if (c + 1 < c_hi)
            chunk_load_async(sKb + ((c + 1 - c_lo) & 1) * CH * DK, K + (size_t)(b0 + CH) * DK, min(CH, B - b0 - CH), wave, lane);
#endif
        // MODE 1: the chunk's 32 row scales per lane (1 / |key|), requested BEFORE the score MFMAs (round 5: they were loaded behind
        // them, inside a range test per group, and used at once -- one exposed L2 round trip at the end of every chunk).  Rows past the
        // bank's end lie inside the slab (finite scratch) and are ignored by the comparison below.
        f32x4 scv[MODE >= 1 ? 2 : 1][MODE >= 1 ? 4 : 1];
        float rs_lane = 1.f;
        if constexpr (MODE >= 1) {
            const float* rs = p.rowscale + (size_t)obj * p.stride_rs;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) scv[i][g] = *reinterpret_cast<const f32x4*>(rs + b0 + 32 * i + 4 * lh + 8 * g);
            if constexpr (MODE == 2) rs_lane = rs[b0 + lane];     // entry b0 + lane: health check below
        }
        f32x16 acc[2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
        if constexpr (PREC == 0) {
            f32x4 a[2][2];
            a[0][0] = *reinterpret_cast<const f32x4*>(sK + swz(li, lh));
            a[0][1] = *reinterpret_cast<const f32x4*>(sK + swz(32 + li, lh));
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) {
                const int cur = kk & 1;
                if (kk + 1 < 16) {
                    a[cur ^ 1][0] = *reinterpret_cast<const f32x4*>(sK + swz(li, 2 * (kk + 1) + lh));
                    a[cur ^ 1][1] = *reinterpret_cast<const f32x4*>(sK + swz(32 + li, 2 * (kk + 1) + lh));
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cur][0][t], qf[kk][t], acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cur][1][t], qf[kk][t], acc[1], 0, 0, 0);
                }
            }
        } else if (PREC == 2 || lp_image) {
            // the chunk as hi | lo operand image: kept beside the bank, or split here ONCE (the four waves read the same
            // 64 rows; splitting in registers per wave cost as many VALU cycles as the score MFMAs).
            // k = 16g + 8h .. +7 is chunk 2g + h of a half.
            if (!lp_image) convert_chunk_inplace<256, true>(const_cast<float*>(sK), tid);
            const char* kb = reinterpret_cast<const char*>(sK);
#pragma unroll
            for (int g = 0; g < 8; ++g) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const bf16x8 ah = *reinterpret_cast<const bf16x8*>(kb + swzk(32 * i + li, 0, 2 * g + lh));
                    bf16x8 al = ah;
                    if constexpr (PREC == 2) al = *reinterpret_cast<const bf16x8*>(kb + swzk(32 * i + li, 1, 2 * g + lh));
                    mfma_lp<PREC == 2>(acc[i], ah, al, qh[g], ql[PREC == 2 ? g : 0]);
                }
            }
        } else {
            // bf16: two 16-byte reads (f32 chunks 4g+2h, 4g+2h+1 = k 16g+8h .. +7) per row tile, rounded in registers
            // (one cvt per pair; an in-LDS conversion pass measured slower here: 2 barriers for little VALU)
#pragma unroll
            for (int g = 0; g < 8; ++g) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const f32x4 x0 = *reinterpret_cast<const f32x4*>(sK + swz(32 * i + li, 4 * g + 2 * lh));
                    const f32x4 x1 = *reinterpret_cast<const f32x4*>(sK + swz(32 * i + li, 4 * g + 2 * lh + 1));
                    const bf16x8 ah = cvt8(x0, x1);
                    mfma_lp<false>(acc[i], ah, ah, qh[g], ql[0]);
                }
            }
        }
        if (MODE == 0 && p.scores) {
            // the raw scores of this (chunk, query tile), in accumulator order: [key half i][row group g][lane half][query][4
            // rows] -- each store instruction of a wave writes two 512-byte runs; the apply kernel reads them back the
            // same way instead of repeating the GEMM
            float* tile = p.scores + (size_t)obj * p.stride_scores + ((size_t)c * qtiles + qt) * (CH * QTS);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 v = {acc[i][4 * g], acc[i][4 * g + 1], acc[i][4 * g + 2], acc[i][4 * g + 3]};
                    __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(tile + ((((i * 4 + g) * 2 + lh) * QTS) + wave * 32 + li) * 4));
                }
        }
#ifdef VFN_ABLATE_SOFTMAX
        if (true) { run_m = fmaxf(run_m, acc[0][0] + acc[1][5]); } else
#endif
        if (MODE == 0) {
            if (b0 + CH <= B) {                          // whole chunk inside the bank (all but the last): no row checks
                float mx = acc[0][0];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, acc[i][r]);
                const float mn = fmaxf(run_m, mx * p.scale);     // scale > 0: max commutes with it
                float sum = 0.f;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) sum += fast_exp(acc[i][r] * p.scale - mn);
                run_l = run_l * expf(run_m - mn) + sum;       // exp(-inf)=0 on the first chunk
                run_m = mn;
            } else {
                float mx = -INFINITY;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = b0 + 32 * i + 4 * lh + (r & 3) + 8 * (r >> 2);
                        const float s_ = acc[i][r] * p.scale;
                        acc[i][r] = s_;
                        if (row < B) mx = fmaxf(mx, s_);
                    }
                const float mn = fmaxf(run_m, mx);
                if (mn > -INFINITY) {
                    float sum = 0.f;
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int row = b0 + 32 * i + 4 * lh + (r & 3) + 8 * (r >> 2);
                            if (row < B) sum += fast_exp(acc[i][r] - mn);
                        }
                    run_l = run_l * expf(run_m - mn) + sum;
                    run_m = mn;
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) {            // registers 4g..4g+3 = rows +8g .. +3: one 16-byte load
                    const int row0 = b0 + 32 * i + 4 * lh + 8 * g;
                    const f32x4 sc = scv[MODE >= 1 ? i : 0][MODE >= 1 ? g : 0];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int row = row0 + j;
                        if (row < B) {
                            const float s_ = acc[i][4 * g + j] * sc[j];
                            // MODE 2: runner-up = median(s, best, runner-up) before the best moves (best >= runner-up)
                            if constexpr (MODE == 2) run_2 = __builtin_amdgcn_fmed3f(s_, run_m, run_2);
                            if (s_ > run_m) { run_m = s_; run_i = row; }   // (ties: smaller row wins, below)
                        }
                    }
                }
            // rowscale = 1 / max(||key||, 1e-12): zero, tiny, NaN (fmaxf drops it: 1e12) and infinite (0) norms all fall outside
            if constexpr (MODE == 2) sick |= (b0 + lane < B) && !(rs_lane > 0.f && rs_lane < 1e12f);
        }
        __syncthreads();                               // next chunk landed; this buffer is free again
    }

    // combine the two lane halves of a query; lanes 0..31 write the slice result
    {
        const float om = __shfl_xor(run_m, 32, 64);
        if (MODE == 0) {
            const float ol = __shfl_xor(run_l, 32, 64);
            const float mn = fmaxf(run_m, om);
            float l = 0.f;
            if (mn > -INFINITY) l = run_l * expf(run_m - mn) + ol * expf(om - mn);
            run_m = mn; run_l = l;
        } else {
            const int oi = __shfl_xor(run_i, 32, 64);
            if constexpr (MODE == 2) {
                const float o2 = __shfl_xor(run_2, 32, 64);
                if (om > run_m || (om == run_m && oi < run_i)) run_2 = fmaxf(run_m, o2);
                else run_2 = fmaxf(run_2, om);
            }
            if (om > run_m || (om == run_m && oi < run_i)) { run_m = om; run_i = oi; }
        }
    }
    if constexpr (MODE == 2) {
        if (__ballot(sick) != 0) run_2 = INFINITY;    // (every wave of the workgroup saw the same entries)
    }
#ifdef VFN_CENSUS
    if (threadIdx.x == 0) {
        const int lin = blockIdx.y * gridDim.x + blockIdx.x;
        if (lin < 4096) {
            unsigned hw_id, xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            vfn_census_buf[lin * 4] = census_t0; vfn_census_buf[lin * 4 + 1] = __builtin_amdgcn_s_memrealtime();
            vfn_census_buf[lin * 4 + 2] = hw_id; vfn_census_buf[lin * 4 + 3] = xcc;
        }
    }
#endif
    const int q = q0 + li;
    if (lh == 0 && q < ncol) {
        if constexpr (MODE == 2) {
            float* dst = p.part + (((size_t)obj * p.nsplit + split) * p.HW + q) * 4;
            *reinterpret_cast<f32x4*>(dst) = f32x4{run_m, __int_as_float(run_i), run_2, 0.f};
        } else {
            float* dst = p.part + (((size_t)obj * p.nsplit + split) * p.HW + q) * 2;
            dst[0] = run_m;
            dst[1] = (MODE == 0) ? run_l : __int_as_float(run_i);
        }
    }
  }
}

// ------------------------------------------------------------------ pass 1, plain bf16 on the kept key image: register-staged keys (round 6)
// bank_scan_kernel<MODE, 1> brings every key chunk in by LDS-DMA ONE chunk ahead and ends every chunk on a barrier that drains the
// DMA: a chunk is 16 MFMAs + ~230 vector slots per wave (0.7 us), the DMA's round trip to L2 / HBM is longer, so the loop runs at
// the memory latency (rocprofv3, round 5: mfma_util 0.17-0.18 at C5 sizes, where the two scans are a quarter of the frame).
// Here the keys go through registers, requested TWO iterations before their chunk is multiplied: issued at the top of iteration
// c - 1, stored into the other LDS buffer at the end of iteration c, read in iteration c + 1 -- two register sets of 64 bytes per
// thread, no DMA (so hipcc's waits stay counted, also around the row-scale loads of MODE 1), and only the hi plane of the image is
// staged (256-byte rows: 16 KB per chunk instead of 32).  Same fragments, same products, same statistics in the same order as the
// image path of bank_scan_kernel<MODE, 1>: bit-identical.  LDS 32 KB; two workgroups per CU as before.
// (MODE 1: the chunk's 64 row scales travel with its keys -- one 16-byte load on 16 threads, through registers into 256 bytes of LDS
// beside the key buffer, read back as broadcast ds_read_b128.  As register loads of their own, issued behind the key requests, the
// in-order load counter made their wait a wait for the keys two chunks ahead: 0.76-1.04 x the DMA kernel instead of 1.4 x.)
constexpr size_t SCAN_PIPE_LDS = 2 * (size_t)CH * DK * 2 + 2 * CH * sizeof(float);
constexpr unsigned SCAN_PIPE_SC0 = 2 * CH * DK * 2;         // byte offset of the two row-scale buffers

template <int MODE>
__global__ __launch_bounds__(256, 2)
void bank_scan_pipe_kernel(const vfn_bankscan_desc p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];      // 2 x [64 rows][256 B] bf16 hi plane, swzq
    __shared__ int s_item;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int qtiles = (p.HW + QTS - 1) / QTS;
    const int total = p.nsplit * qtiles * p.obj_n;
    const int krow = tid >> 2, kc4 = (tid & 3) * 4;                   // key staging: row, first of four 16-byte chunks
    const unsigned klane_off = (unsigned)krow * 512u + (unsigned)kc4 * 16u;
  for (;;) {
    if (tid == 0) s_item = atomicAdd(p.work_counter, 1);
    __syncthreads();
    const int item = s_item;
    __syncthreads();                                   // (everyone has the item before thread 0 draws the next one)
    if (item >= total) break;
    const int obj = item % p.obj_n;
    const int qt = (item / p.obj_n) % qtiles;
    const int split = item / (p.obj_n * qtiles);
    const int q0 = qt * QTS + wave * 32;             // first query of this wave
    const int B = p.bank_len[obj];
    const char* Kimg = reinterpret_cast<const char*>(p.bank_k_lp) + (size_t)obj * p.stride_k * 4;    // image rows of 512 B: [128 hi | 128 lo]
    const float* Q = p.q + (size_t)(p.q_per_obj ? obj : 0) * p.stride_q;

    int c_lo, c_hi;
    chunk_range(B, p.nsplit, split, c_lo, c_hi);

    u32x4 kst[2][4];                                    // two chunks of keys in flight: 64 bytes per thread each
    f32x4 sst[2];                                       // (MODE 1) ... and their row scales: rows 4 tid .. + 3 on threads 0..15
    const float* rs = MODE == 1 ? p.rowscale + (size_t)obj * p.stride_rs : nullptr;
    auto load_k = [&](int c, auto SET_) {
        constexpr int set = decltype(SET_)::value;
        const int b0 = c * CH;
        const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(Kimg + (size_t)b0 * 512), 0, min(CH, B - b0) * 512, 0x00020000);
#pragma unroll
        for (int j = 0; j < 4; ++j) kst[set][j] = __builtin_amdgcn_raw_buffer_load_b128(r, klane_off, 16 * j, 0);
        // (rows past the bank's end lie inside the slab -- finite scratch -- and are ignored by the comparison below)
        if constexpr (MODE == 1) { if (tid < 16) sst[set] = *reinterpret_cast<const f32x4*>(rs + b0 + 4 * tid); }
    };
    auto store_k = [&](int buf, auto SET_) {
        constexpr int set = decltype(SET_)::value;
        char* d = smem + buf * (CH * DK * 2);
#pragma unroll
        for (int j = 0; j < 4; ++j) *reinterpret_cast<u32x4*>(d + swzq(krow, kc4 + j)) = kst[set][j];
        if constexpr (MODE == 1) { if (tid < 16) *reinterpret_cast<f32x4*>(smem + SCAN_PIPE_SC0 + buf * (CH * 4) + tid * 16) = sst[set]; }
    };
    using Z0 = std::integral_constant<int, 0>; using Z1 = std::integral_constant<int, 1>;
    if (c_lo < c_hi) load_k(c_lo, Z0{});
    if (c_lo + 1 < c_hi) load_k(c_lo + 1, Z1{});

    bf16x8 qh[8];                                      // B operand: this lane's query column, k = 16g + 8lh + j
    {
        const int q = min(q0 + li, p.HW - 1);                    // columns past HW are never written out
        const float* qrow = Q + (size_t)q * p.ldq + 8 * lh;
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const f32x4 x0 = *reinterpret_cast<const f32x4*>(qrow + 16 * g);
            const f32x4 x1 = *reinterpret_cast<const f32x4*>(qrow + 16 * g + 4);
            qh[g] = cvt8(x0, x1);
        }
    }

    float run_m = -INFINITY, run_l = 0.f;
    int run_i = 0x7fffffff;
    if (c_lo < c_hi) store_k(0, Z0{});
    __syncthreads();

    auto body = [&](auto PAR_, int c) {                 // PAR = (c - c_lo) & 1: LDS buffer of chunk c, register set of chunk c + 2
        constexpr int PAR = decltype(PAR_)::value;
        const int b0 = c * CH;
        const char* kb = smem + PAR * (CH * DK * 2);
        if (c + 2 < c_hi) load_k(c + 2, PAR_);          // (set PAR held chunk c: stored to LDS an iteration ago)
        f32x4 scv[MODE == 1 ? 2 : 1][MODE == 1 ? 4 : 1];
        if constexpr (MODE == 1) {
            const float* sS = reinterpret_cast<const float*>(smem + SCAN_PIPE_SC0 + PAR * (CH * 4));
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) scv[i][g] = *reinterpret_cast<const f32x4*>(sS + 32 * i + 4 * lh + 8 * g);
        }
        f32x16 acc[2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
#pragma unroll
        for (int g = 0; g < 8; ++g) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const bf16x8 ah = *reinterpret_cast<const bf16x8*>(kb + swzq(32 * i + li, 2 * g + lh));
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, qh[g], acc[i], 0, 0, 0);
            }
        }
        if (MODE == 0) {
            if (b0 + CH <= B) {                          // whole chunk inside the bank (all but the last): no row checks
                float mx = acc[0][0];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, acc[i][r]);
                const float mn = fmaxf(run_m, mx * p.scale);     // scale > 0: max commutes with it
                float sum = 0.f;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) sum += fast_exp(acc[i][r] * p.scale - mn);
                run_l = run_l * expf(run_m - mn) + sum;       // exp(-inf)=0 on the first chunk
                run_m = mn;
            } else {
                float mx = -INFINITY;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = b0 + 32 * i + 4 * lh + (r & 3) + 8 * (r >> 2);
                        const float s_ = acc[i][r] * p.scale;
                        acc[i][r] = s_;
                        if (row < B) mx = fmaxf(mx, s_);
                    }
                const float mn = fmaxf(run_m, mx);
                if (mn > -INFINITY) {
                    float sum = 0.f;
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int row = b0 + 32 * i + 4 * lh + (r & 3) + 8 * (r >> 2);
                            if (row < B) sum += fast_exp(acc[i][r] - mn);
                        }
                    run_l = run_l * expf(run_m - mn) + sum;
                    run_m = mn;
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) {            // registers 4g..4g+3 = rows +8g .. +3: one 16-byte load
                    const int row0 = b0 + 32 * i + 4 * lh + 8 * g;
                    const f32x4 sc = scv[MODE == 1 ? i : 0][MODE == 1 ? g : 0];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int row = row0 + j;
                        if (row < B) {
                            const float s_ = acc[i][4 * g + j] * sc[j];
                            if (s_ > run_m) { run_m = s_; run_i = row; }   // (ties: smaller row wins, below)
                        }
                    }
                }
        }
        if (c + 1 < c_hi) store_k(PAR ^ 1, std::integral_constant<int, PAR ^ 1>{});   // chunk c + 1 (requested an iteration ago) into the buffer chunk c - 1 has left
        __syncthreads();
    };
    for (int c = c_lo; c < c_hi; c += 2) {
        body(std::integral_constant<int, 0>{}, c);
        if (c + 1 < c_hi) body(std::integral_constant<int, 1>{}, c + 1);
    }

    // combine the two lane halves of a query; lanes 0..31 write the slice result
    {
        const float om = __shfl_xor(run_m, 32, 64);
        if (MODE == 0) {
            const float ol = __shfl_xor(run_l, 32, 64);
            const float mn = fmaxf(run_m, om);
            float l = 0.f;
            if (mn > -INFINITY) l = run_l * expf(run_m - mn) + ol * expf(om - mn);
            run_m = mn; run_l = l;
        } else {
            const int oi = __shfl_xor(run_i, 32, 64);
            if (om > run_m || (om == run_m && oi < run_i)) { run_m = om; run_i = oi; }
        }
    }
    const int q = q0 + li;
    if (lh == 0 && q < p.HW) {
        float* dst = p.part + (((size_t)obj * p.nsplit + split) * p.HW + q) * 2;
        dst[0] = run_m;
        dst[1] = (MODE == 0) ? run_l : __int_as_float(run_i);
    }
  }
}

// combine bank-split partials.  MODE 0 -> ml[obj][q] = (m, l); MODE 1 -> idx[obj][q], corr[obj][q]
// Eight lanes per query column: lane j folds the slices j, j + 8, ... (a fixed order), then the eight partial results are folded
// in lane order -- 8 + 7 steps instead of a 59-long chain on one thread (the kernel sits between the scan and the apply kernel of
// every frame: 18-22 us -> a few).  Deterministic: the order of the folds does not depend on the schedule.
template <int MODE>
__global__ void bank_scan_finish_kernel(const float* __restrict__ part, int nsplit, int HW, int obj_n,
                                        float* __restrict__ ml, int* __restrict__ idx, float* __restrict__ corr,
                                        const float* __restrict__ colscale) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = min(t >> 3, obj_n * HW - 1), j = t & 7;          // (surplus groups repeat the last column: whole waves shuffle)
    const bool live = (t >> 3) < obj_n * HW;
    const int obj = i / HW, q = i - obj * HW;
    float m = -INFINITY, x = (MODE == 0) ? 0.f : __int_as_float(0x7fffffff);
    auto fold = [&](float om, float ox) {
        if (MODE == 0) {
            const float mn = fmaxf(m, om);
            if (mn > -INFINITY) x = x * expf(m - mn) + ox * expf(om - mn);
            m = mn;
        } else {
            const int i0 = __float_as_int(x), i1 = __float_as_int(ox);
            if (om > m || (om == m && i1 < i0)) { m = om; x = ox; }
        }
    };
    for (int s = j; s < nsplit; s += 8) {
        const float* src = part + (((size_t)obj * nsplit + s) * HW + q) * 2;
        fold(src[0], src[1]);
    }
    const int base = (threadIdx.x & 63) & ~7;
#pragma unroll
    for (int o = 1; o < 8; ++o) {
        const float om = __shfl(m, base + o, 64), ox = __shfl(x, base + o, 64);
        if (j == 0) fold(om, ox);
    }
    if (j != 0 || !live) return;
    if (MODE == 0) { ml[(size_t)i * 2] = m; ml[(size_t)i * 2 + 1] = x; }
    else { idx[i] = __float_as_int(x); corr[i] = m * colscale[i]; }
}

// ------------------------------------------------------------------ certified bank match (f32 mode of FeatureBank.update)
// The update needs, per new key q, only the arg-max entry b* of  f(b) = fl(F(b) * rowscale[b])  (F = the f32 MFMA dot of
// bank_scan_kernel<1, 0>) and f(b*).  vfn_bank_match_certified gets both bit for bit at a fraction of the f32 matrix work:
//   1. bank_scan_kernel<2, 2>: a(b) = fl(A(b) * rowscale[b]) with A the bf16x3 dot (keys from the split image, q split in
//      registers); per (slice, column) the best a, its entry and the runner-up a (+inf when a live entry of the slice has a
//      zero or non-finite norm).
//   2. bank_match_certify_kernel: fold the slices; a column is CERTIFIED when  best - runner-up > margin(q).  Its winner's
//      f(b*) is recomputed with the f32 kernel's instruction sequence (one 32x32 tile, diagonal = 32 (entry, column) pairs) and
//      written with its index; any other column goes on a device list.
//   3. bank_scan_kernel<1, 0, GATHER> over the listed columns + bank_scan_finish_kernel<1, GATHER>: the f32 path itself.
//
// The bound.  Per column, with k = the 128 key channels, K = key, Q = q, |.| = 2-norm, u = 2^-23 (one f32 ulp: no rounding
// mode of the matrix cores is assumed beyond "each addition or product errs by at most u times the sum of the magnitudes it
// combines", which covers round-to-nearest, truncation and wide internal sums):
//   split   x = hi + lo + e,  hi = RNE_bf16(x), lo = RNE_bf16(x - hi) (x - hi is exact in f32): |lo| <= 2^-8 (1 + 2^-8) |x|,
//           |e| <= 2^-16 |x|.  The bf16x3 terms hiK hiQ + hiK loQ + loK hiQ miss  loK loQ + eK Q + (hiK + loK) eQ  per k:
//           <= (2^-16 (1 + 2^-7) + 2^-16 + 2^-16 (1 + 2^-16)) |K_k Q_k| <= 3.01 * 2^-16 |K_k Q_k|.
//   sums    bf16 x bf16 products are exact in f32; the 384 terms (sum of magnitudes <= 1.02 sum|K_k Q_k|) take <= 384
//           roundings: <= 384 u * 1.02 sum|K_k Q_k|.  The f32 kernel: 128 products and 128 additions, <= 256 u * sum|K_k Q_k|
//           from the exact dot.  Cauchy-Schwarz: sum|K_k Q_k| <= |K| |Q|.
//   so      |A - F| <= (3.01 * 2^-16 + 648 u) |K| |Q| = (4.593e-5 + 7.725e-5) |K| |Q| <= 1.232e-4 |K| |Q|.
//   scaling a and f are A and F times the same s = rowscale[b], each rounded once: |a - f| <= |A - F| s + u (|A| + |F|) s, and
//           |K| s <= 1 + 2^-16 (s = 1/|K| as vfn_row_norms computes it; smaller for |K| < 1e-12), |A|, |F| <= 1.03 |K| |Q|:
//           |a - f| <= (1.232e-4 + 2.5e-7) (1 + 2^-16) |Q| <= 1.24e-4 |Q|.
//   flushed subnormal operands or products add at most 3 * 128 * 2^-126 max|Q_k| per dot, times s <= 1e12: < 2^-77 |Q|.
//   |Q| is taken as qnorm * (1 + 2^-16) (the f32 norm of vfn_row_norms), so  E(q) = 1.25e-4 * qnorm + 2^-64  bounds |a - f|
//   for every entry of the column.
// Certification: if  a(b1) - a(b) > 2 E  for every b != b1, then  f(b1) >= a(b1) - E > a(b) + E >= f(b): b1 is the strict f32
// arg-max, so no tie rule is involved and f(b1) is the value the f32 path keeps.  The margin used is twice that, 4 E(q) (about
// 5e-4 in cosine units).  A column is never certified when qnorm is 0, above 2^60 (products could overflow) or not finite, when
// its best score is not finite, or when some live entry's norm is zero / non-finite (runner-up = +inf); equal best scores give a
// zero gap.  Every such column takes the f32 path.
constexpr float MATCH_EPS_REL = 1.25e-4f;
constexpr float MATCH_EPS_ABS = 5.421010862427522e-20f;    // 2^-64
constexpr float MATCH_QNORM_MAX = 1.152921504606846976e18f;  // 2^60

// One wave = 32 columns of one object: fold the bf16x3 slice partials (lane half lh takes the slices lh, lh + 2, ..., then the
// halves meet), certify, and for certified columns form f(b1) as bank_scan_kernel<1, 0> forms it: A row li = key b1 of column
// li, B column li = that column's query, k = 8kk + 4lh + t, 64 v_mfma_f32_32x32x2f32 from a zero accumulator; element (li, li)
// is then multiplied by rowscale[b1] and by colscale[q] as bank_scan_finish_kernel<1> does.  An MFMA output element depends only
// on its own A row and B column, so the diagonal is what the f32 scan computes for that (entry, column) pair.
__global__ __launch_bounds__(64)
void bank_match_certify_kernel(const vfn_bankmatch_desc p) {
    const int lane = threadIdx.x, li = lane & 31, lh = lane >> 5;
    const int obj = blockIdx.y, q0 = blockIdx.x * 32;
    const int q = q0 + li, qc = min(q, p.HW - 1);
    float m = -INFINITY, m2 = -INFINITY;
    int bi = 0x7fffffff;
    auto fold = [&](float om, int oi, float o2) {          // runner-up = the largest of the other three (+inf stays +inf)
        if (om > m || (om == m && oi < bi)) { m2 = fmaxf(fmaxf(m, m2), o2); m = om; bi = oi; }
        else m2 = fmaxf(fmaxf(m2, om), o2);
    };
    const float* part = p.part_x3 + ((size_t)obj * p.nsplit * p.HW + qc) * 4;
#pragma unroll 4
    for (int s = lh; s < p.nsplit; s += 2) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(part + (size_t)s * p.HW * 4);
        fold(v[0], __float_as_int(v[1]), v[2]);
    }
    fold(__shfl_xor(m, 32, 64), __shfl_xor(bi, 32, 64), __shfl_xor(m2, 32, 64));

    const size_t col = (size_t)obj * p.HW + qc;
    const float qn = p.qnorm[col];
    const float margin = 4.f * (MATCH_EPS_REL * qn + MATCH_EPS_ABS);
    const bool cert = q < p.HW && qn > 0.f && qn <= MATCH_QNORM_MAX && m > -INFINITY && m < INFINITY && (m - m2) > margin;

    // rescore (every lane takes part in the MFMAs; uncertain columns multiply zeros)
    const float* krow = p.bank_k + (size_t)obj * p.stride_k + (size_t)(cert ? bi : 0) * DK + 4 * lh;
    const float* qrow = p.q + (size_t)obj * p.stride_q + (size_t)qc * p.ldq + 4 * lh;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
        f32x4 a = *reinterpret_cast<const f32x4*>(krow + 8 * kk);
        const f32x4 b = *reinterpret_cast<const f32x4*>(qrow + 8 * kk);
        if (!cert) a = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b[t], acc, 0, 0, 0);
    }
    // element (row li, column li) sits in lane li + 32 * ((li >> 2) & 1), register (li & 3) + 4 * (li >> 3)
    const int rsel = (li & 3) + 4 * (li >> 3);
    float dot = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) dot = (r == rsel) ? acc[r] : dot;
    if (lh != ((li >> 2) & 1)) return;
    if (cert) {
        const float s_ = dot * p.rowscale[(size_t)obj * p.stride_rs + bi];
        p.match_idx[col] = bi;
        p.match_corr[col] = s_ * p.colscale[col];
    } else if (q < p.HW) {
        const int pos = atomicAdd(p.ucount + obj, 1);
        p.ulist[(size_t)obj * p.HW + pos] = q;
        if (p.utotal) atomicAdd(p.utotal + obj, 1);
    }
}

// bank_scan_finish_kernel<1> for the listed columns of bank_scan_kernel<1, 0, true> (partials at list positions)
__global__ void bank_match_finish_listed_kernel(const float* __restrict__ part, int nsplit, int HW, int obj_n,
                                                const int* __restrict__ ulist, const int* __restrict__ ucount,
                                                int* __restrict__ idx, float* __restrict__ corr, const float* __restrict__ colscale) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = min(t >> 3, obj_n * HW - 1), j = t & 7;
    const int obj = i / HW, pos = i - obj * HW;
    const bool live = (t >> 3) < obj_n * HW && pos < ucount[obj];
    float m = -INFINITY, x = __int_as_float(0x7fffffff);
    auto fold = [&](float om, float ox) {
        const int i0 = __float_as_int(x), i1 = __float_as_int(ox);
        if (om > m || (om == m && i1 < i0)) { m = om; x = ox; }
    };
    if (live)
        for (int s = j; s < nsplit; s += 8) {
            const float* src = part + (((size_t)obj * nsplit + s) * HW + pos) * 2;
            fold(src[0], src[1]);
        }
    const int base = (threadIdx.x & 63) & ~7;
#pragma unroll
    for (int o = 1; o < 8; ++o) {
        const float om = __shfl(m, base + o, 64), ox = __shfl(x, base + o, 64);
        if (j == 0) fold(om, ox);
    }
    if (j != 0 || !live) return;
    const size_t c = (size_t)obj * HW + ulist[(size_t)obj * HW + pos];
    idx[c] = __float_as_int(x);
    corr[c] = m * colscale[c];
}

// p = exp(scale*s - m) * (1/l) for the 16 scores of a lane (branch-free: an out-of-range query carries m = +big and
// 1/l = 0, rows past the bank end are masked only in the last chunk), and the hit counts of the wave's 32 bank rows:
// 16 ballots give 32 row masks (lanes 0-31: row (r&3)+8*(r>>2), lanes 32-63: that + 4); their popcounts are dropped
// into lane = row of `cnt` with v_writelane -- no divergent branch anywhere.
__device__ __forceinline__ int softmax_hits(f32x16& acc, float scale, float qm, float qinv, float thres, int nvalid, int rloc) {
    int cnt = 0;
#ifdef VFN_ABLATE_SOFTMAX
    for (int r = 0; r < 16; ++r) acc[r] *= qinv;
    return cnt;
#endif
    const float sm = -qm;
    if (nvalid >= CH) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = fast_exp(fmaf(acc[r], scale, sm)) * qinv;
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rr = rloc + (r & 3) + 8 * (r >> 2);
            const float pv = fast_exp(fmaf(acc[r], scale, sm)) * qinv;
            acc[r] = rr < nvalid ? pv : 0.f;
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const unsigned long long hit = __ballot(acc[r] > thres);
        const int rlo = (r & 3) + 8 * (r >> 2);
        const int c_lo = __popcll(hit & 0xffffffffull), c_hi = __popcll(hit >> 32);      // wave-uniform
        asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(cnt) : "s"(c_lo), "n"(rlo));
        asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(cnt) : "s"(c_hi), "n"(rlo + 4));
    }
    return cnt;                                       // lane i (0..31) holds the hits of chunk-local row 32*wr + i
}

// Workgroup -> (bank slice, query tile, object) of the apply kernels.  Workgroups are dealt round-robin over the 8 XCDs, each with
// a private L2: the query tiles of one (object, slice) pair stream the SAME value rows, so they are given to ONE XCD as a
// contiguous run of workgroup slots (they start together and advance in step: the first reader of a chunk brings it into that
// L2, the other tiles hit it).  With query tiles scattered over the XCDs (the linear order of rounds 1-2) every chunk was
// fetched from beyond L2 by up to 8 XCDs -- at C5 sizes (GBs of values per object) that is the kernel's bandwidth.  Bijective
// for any grid; affects speed only.  VFN_APPLY_XCD=0 (read once by the host) restores the linear order.
__device__ int vfn_apply_linear_order = 0;
__device__ __forceinline__ void apply_item(const vfn_memread_desc& p, int& split, int& qt, int& obj) {
    const int qtiles = (int)gridDim.x / p.nsplit;
    if (vfn_apply_linear_order) { split = blockIdx.x % p.nsplit; qt = blockIdx.x / p.nsplit; obj = blockIdx.y; return; }
    const int total = (int)(gridDim.x * gridDim.y);
    const int id = (int)(blockIdx.y * gridDim.x + blockIdx.x);
    const int q = total >> 3, r = total & 7;
    const int xcd = id & 7, slot = id >> 3;
    const int L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
    const int pair = L / qtiles;
    qt = L - pair * qtiles;
    obj = pair / p.nsplit;
    split = pair - obj * p.nsplit;
}

// ---- steps the apply kernels take the same way (128 query columns x one bank slice per workgroup, 8 waves)
// A step is shared only where the kernel's machine code comes out the same with the call as with the block written out: these
// kernels sit at 236-256 registers, and hipcc's register allocation follows the order in which the inliner leaves the
// instructions.  That holds for the three helpers below (load_qstats not in memread_apply_wide_kernel, zero_o only in the wide
// and shw kernels).  The query image, the P^T store, the hit-count bump and the o_part epilogue changed the instruction stream
// of every kernel they were shared between and stay written out; a change to one of those conventions goes to every apply kernel.
constexpr int QTW = 128;    // query columns per apply workgroup
// this workgroup's item: first query column and bank length
__device__ __forceinline__ void apply_slice(const vfn_memread_desc& p, int& split, int& qt, int& obj, int& q0, int& B) {
    apply_item(p, split, qt, obj);
    q0 = qt * QTW;
    B = p.bank_len[obj];
}

// softmax statistics of query column q0 + qcol: (m, 1/l); a column past HW carries m = +big, 1/l = 0 (p = 0 exactly)
__device__ __forceinline__ void load_qstats(const vfn_memread_desc& p, int obj, int q0, int qcol, float& qm, float& qinv) {
    qm = 1e30f; qinv = 0.f;
    if (q0 + qcol < p.HW) {
        qm = p.ml[((size_t)obj * p.HW + q0 + qcol) * 2];
        qinv = 1.f / p.ml[((size_t)obj * p.HW + q0 + qcol) * 2 + 1];
    }
}

// O^T accumulators of a wave: TQN query tiles x TCN channel tiles of 32 x 32
template <int TQN, int TCN>
__device__ __forceinline__ void zero_o(f32x16 (&o)[TQN][TCN]) {
#pragma unroll
    for (int a = 0; a < TQN; ++a)
#pragma unroll
        for (int b = 0; b < TCN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[a][b][r] = 0.f;
}

// ------------------------------------------------------------------ pass 2: P^T V and hit counts
// (The 64-query apply kernels of rounds 1-2 are gone: the 128-query kernels below measured faster at every bank size in
// every precision mode and were the only ones the default path had selected since.)
// ------------------------------------------------------------------ pass 2, bf16 / bf16x3, wide query tile
// For the bandwidth-bound regime (reduced-precision MFMAs are 5-16x faster than the f32 ones, so streaming the bank
// becomes the cost; at the C5 sizes every query tile re-reads a multi-GB bank): 128 query columns per workgroup,
// 8 waves.  A key chunk and a value row are fetched once per 128 queries (half the traffic of the 64-query kernel);
// wave w owns value channels 64w..64w+63 for all 128 queries, so no value row is loaded or converted twice.
// LDS: query image bf16 hi/lo [128][128] (32 + 32 KB), key chunk f32 [64][128] (32 KB), P^T bf16 hi/lo [128 q][64 b]
// (16 + 16 KB): 128 KB for bf16x3, one workgroup per CU (8 waves = two per SIMD, as the other kernels).
__device__ __forceinline__ void chunk_load_async8(float* sK, const float* src, int valid, int wave, int lane) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {                    // 8 waves x 4 instructions x 2 rows = 64 rows
        const int r = (wave * 4 + j) * 2 + (lane >> 5);
        const int pc = lane & 31;
        const int rr = min(r, valid - 1);
        const float* g = src + (size_t)rr * DK + ((pc ^ (r & 15)) << 2);
        __builtin_amdgcn_global_load_lds(g, sK + (wave * 4 + j) * 2 * DK, 16, 0, 0);
    }
}

template <bool X3>
__global__ __launch_bounds__(512, 1)
void memread_apply_lpw_kernel(const vfn_memread_desc p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sQh = smem;                                         // [128][128] bf16
    char* sQl = sQh + QTW * DK * 2;                           // (bf16x3 only)
    float* sK = reinterpret_cast<float*>(sQh + (X3 ? 2 : 1) * QTW * DK * 2);   // [64][128] f32
    char* sPh = reinterpret_cast<char*>(sK + CH * DK);        // [128 q][64 b] bf16
    char* sPl = sPh + QTW * CH * 2;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int wr = wave >> 2, wq = wave & 3;                  // score tile: key rows 32wr.., query columns 32wq..
    int split, qt, obj, q0, B;
    apply_slice(p, split, qt, obj, q0, B);
    const float* K = p.bank_k + (size_t)obj * p.stride_k;
    const float* V = p.bank_v + (size_t)obj * p.stride_v;

    {   // query image
        const int c = tid & 31;
        for (int r = tid >> 5; r < QTW; r += 16) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (q0 + r < p.HW) v = *reinterpret_cast<const f32x4*>(p.q + (size_t)(q0 + r) * p.ldq + c * 4);
            bf16x4 h, l;
#pragma unroll
            for (int e = 0; e < 4; ++e) { h[e] = (__bf16)v[e]; l[e] = (__bf16)(v[e] - (float)h[e]); }
            const int off = swzq(r, c >> 1) + (c & 1) * 8;
            *reinterpret_cast<bf16x4*>(sQh + off) = h;
            if constexpr (X3) *reinterpret_cast<bf16x4*>(sQl + off) = l;
        }
    }

    int c_lo, c_hi;
    chunk_range(B, p.nsplit, split, c_lo, c_hi);

    f32x16 o[4][2];                                           // O^T tiles: [query tile][channel tile]
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[a][b][r] = 0.f;

    // value channels of this wave: 64*wave .. +63; lane li owns channels 2*li, 2*li+1 (one per 32-wide tile tc)
    const unsigned vlane_off = (unsigned)((8 * lh) * DV + wave * 64 + li * 2) * 4u;   // bytes, per lane

    if (c_lo < c_hi) chunk_load_async8(sK, K + (size_t)c_lo * CH * DK, min(CH, B - c_lo * CH), wave, lane);
    __syncthreads();

    const int qcol = wq * 32 + li;
    float qm, qinv;
    load_qstats(p, obj, q0, qcol, qm, qinv);

    for (int c = c_lo; c < c_hi; ++c) {
        const int b0 = c * CH;
        const bool more = c + 1 < c_hi;

        // value rows of step 0 (16 bank rows; this lane half: rows 8*lh .. +7) -- they land behind the score GEMM
        f32x2 raw[8];
        // buffer descriptor over this chunk's value rows, ending at the bank's last row (rows past it read 0; P is exactly 0 there):
        // one load form for every chunk, no per-load address arithmetic beyond one vector add (round 5: the branch between this
        // form and a clamped plain-load form for the bank's last chunk cost hipcc's wait insertion the count of the loads in flight)
        const __amdgpu_buffer_rsrc_t vrsrc = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(V + (size_t)b0 * DV), 0, min(CH, B - b0) * DV * 4, 0x00020000);
        auto load_raw = [&](int st) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                raw[j] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(vrsrc, vlane_off + (unsigned)((16 * st + j) * DV * 4), 0, 0));
        };
        load_raw(0);

        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        {
            const int ra = wr * 32 + li, rq = wq * 32 + li;
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const f32x4 x0 = *reinterpret_cast<const f32x4*>(sK + swz(ra, 4 * g + 2 * lh));
                const f32x4 x1 = *reinterpret_cast<const f32x4*>(sK + swz(ra, 4 * g + 2 * lh + 1));
                const bf16x8 bh = *reinterpret_cast<const bf16x8*>(sQh + swzq(rq, 2 * g + lh));
                bf16x8 bl = bh;
                if constexpr (X3) bl = *reinterpret_cast<const bf16x8*>(sQl + swzq(rq, 2 * g + lh));
                bf16x8 ah, al;
                if constexpr (X3) split8(x0, x1, ah, al);
                else { ah = cvt8(x0, x1); al = ah; }
                mfma_lp<X3>(acc, ah, al, bh, bl);
            }
        }

        const int rloc = wr * 32 + 4 * lh;
        const int mycnt = softmax_hits(acc, p.scale, qm, qinv, p.thres, B - b0, rloc);
#pragma unroll
        for (int g = 0; g < 4; ++g) {                // registers 4g..4g+3 = 4 consecutive bank rows of query qcol
            const int brow = rloc + 8 * g;
            bf16x4 h, l;
#pragma unroll
            for (int e = 0; e < 4; ++e) { h[e] = (__bf16)acc[4 * g + e]; l[e] = (__bf16)(acc[4 * g + e] - (float)h[e]); }
            const int off = swzp(qcol, brow >> 3) + ((brow >> 2) & 1) * 8;
            *reinterpret_cast<bf16x4*>(sPh + off) = h;
            if constexpr (X3) *reinterpret_cast<bf16x4*>(sPl + off) = l;
        }
        // one wave per 32 x 32 score tile: the four query groups add their hits of the same bank rows
        if (p.cnt && lh == 0 && mycnt > 0) {
            const int row = b0 + wr * 32 + li;
            if (row < B) atomicAdd(p.cnt + (size_t)obj * p.stride_cnt + row, mycnt);
        }
        __syncthreads();                             // P^T visible; every wave is done reading sK
        if (more) chunk_load_async8(sK, K + (size_t)(b0 + CH) * DK, min(CH, B - b0 - CH), wave, lane);

        // O^T[q][ch] += sum_b P^T[q][b] V[b][ch]: A = P^T (rows q, 4 tiles), B = value rows (cols = channel 2li + tc)
#pragma unroll
        for (int st = 0; st < CH / 16; ++st) {
            bf16x8 vh[2], vl[2];
#pragma unroll
            for (int tc = 0; tc < 2; ++tc)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float x = raw[j][tc];
                    const __bf16 hx = (__bf16)x;
                    vh[tc][j] = hx;
                    if constexpr (X3) vl[tc][j] = (__bf16)(x - (float)hx); else vl[tc][j] = hx;
                }
            if (st + 1 < CH / 16) load_raw(st + 1);
#pragma unroll
            for (int tq = 0; tq < 4; ++tq) {
                const bf16x8 ph = *reinterpret_cast<const bf16x8*>(sPh + swzp(tq * 32 + li, 2 * st + lh));
                bf16x8 pl = ph;
                if constexpr (X3) pl = *reinterpret_cast<const bf16x8*>(sPl + swzp(tq * 32 + li, 2 * st + lh));
#pragma unroll
                for (int tc = 0; tc < 2; ++tc) mfma_lp<X3>(o[tq][tc], ph, pl, vh[tc], vl[tc]);
            }
        }
        __syncthreads();
    }

    float* dst = p.o_part + ((size_t)obj * p.nsplit + split) * p.HW * DV;
#pragma unroll
    for (int tq = 0; tq < 4; ++tq)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int q = q0 + tq * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (q < p.HW) {
                const f32x2 v = {o[tq][0][r], o[tq][1][r]};
                *reinterpret_cast<f32x2*>(dst + (size_t)q * DV + wave * 64 + li * 2) = v;
            }
        }
}


// ------------------------------------------------------------------ pass 2, bf16 / bf16x3, wide tile, kept split image
// As memread_apply_lpw_kernel, for a bank that carries its split-bf16 image (vfn_bank_refresh_lp): no operand is
// converted in the loop except P.  The key chunk lands in LDS as the hi | lo operand image; the value image is stored
// operand-ready (bank.hip: blocks of 8 rows, [hi | lo plane][channel][8 rows]): a lane's B operand of a 16-row step is one
// 16-byte buffer load per channel tile and plane, 32 lanes = 512 contiguous bytes -- no transposition in registers.
// P^T V mapping: wave = (query half qh, channel quarter cq): 2 query tiles x 4 channel tiles (channel = 128cq + 32tc + li),
// so P^T fragments are read from LDS half as often as with 4 query tiles x 2 channel tiles.
constexpr unsigned VBLK = 8 * DV * 4;       // bytes of one 8-row block of the value image

template <bool X3>
__global__ __launch_bounds__(512, 1)
void memread_apply_shw_kernel(const vfn_memread_desc p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sQh = smem;                                         // [128][128] bf16
    char* sQl = sQh + QTW * DK * 2;                           // (bf16x3 only)
    float* sK = reinterpret_cast<float*>(sQh + (X3 ? 2 : 1) * QTW * DK * 2);   // [64][hi 256 B | lo 256 B]
    char* sPh = reinterpret_cast<char*>(sK + CH * DK);        // [128 q][64 b] bf16
    char* sPl = sPh + QTW * CH * 2;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int wr = wave >> 2, wq = wave & 3;                  // score tile: key rows 32wr.., query columns 32wq..
    const int qhalf = wave >> 2, cq = wave & 3;               // P^T V: queries 64qhalf.., channels 128cq..
    int split, qt, obj, q0, B;
    apply_slice(p, split, qt, obj, q0, B);
    const float* K = reinterpret_cast<const float*>(p.bank_k_lp) + (size_t)obj * p.stride_k;     // image rows are 512 B too
    const char* V = reinterpret_cast<const char*>(p.bank_v_lp) + (size_t)obj * p.stride_v * 4;   // blocks of 8 rows, 16 KB

    {   // query image
        const int c = tid & 31;
        for (int r = tid >> 5; r < QTW; r += 16) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (q0 + r < p.HW) v = *reinterpret_cast<const f32x4*>(p.q + (size_t)(q0 + r) * p.ldq + c * 4);
            bf16x4 h, l;
#pragma unroll
            for (int e = 0; e < 4; ++e) { h[e] = (__bf16)v[e]; l[e] = (__bf16)(v[e] - (float)h[e]); }
            const int off = swzq(r, c >> 1) + (c & 1) * 8;
            *reinterpret_cast<bf16x4*>(sQh + off) = h;
            if constexpr (X3) *reinterpret_cast<bf16x4*>(sQl + off) = l;
        }
    }

    int c_lo, c_hi;
    chunk_range(B, p.nsplit, split, c_lo, c_hi);

    f32x16 o[2][4];                                           // O^T tiles: [query tile][channel tile]
    zero_o(o);

    const unsigned vlane_off = (unsigned)lh * VBLK + (unsigned)(cq * 128 + li) * 16u;   // bytes, per lane: row block lh of a step

    if (c_lo < c_hi) chunk_load_async8(sK, K + (size_t)c_lo * CH * DK, min(CH, B - c_lo * CH), wave, lane);
    __syncthreads();

    const int qcol = wq * 32 + li;
    float qm, qinv;
    load_qstats(p, obj, q0, qcol, qm, qinv);

    for (int c = c_lo; c < c_hi; ++c) {
        const int b0 = c * CH;
        const bool more = c + 1 < c_hi;
        // buffer descriptor over this chunk's live row blocks: blocks past the bank end read 0 through the range check; rows
        // past the end inside the last live block hold zeros or stale (finite) values -- their P is exactly 0
        const int live = min(CH, B - b0);
        const __amdgpu_buffer_rsrc_t vrsrc = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<char*>(V + (size_t)(b0 >> 3) * VBLK), 0, ((live + 7) >> 3) * VBLK, 0x00020000);

        // bf16x3: two steps of operands in flight, [tc][hi, lo].  Plain bf16 (round 5): its steps are 8 MFMAs = 256 cycles, one step of
        // lead left the kernel waiting on memory (PMC: 0.64 of the wave cycles, mfma_util 0.27) -- three of the chunk's four steps
        // are requested here, in front of the score GEMM, the fourth into step 0's slot behind step 0's MFMAs (a fourth slot spills:
        // 52 bytes of scratch at 256 registers)
        constexpr int NSLOT = X3 ? 2 : 3;
        u32x4 vop[NSLOT][8];
        auto load_v = [&](int st, u32x4 (&dst)[8]) {
#pragma unroll
            for (int tc = 0; tc < 4; ++tc) {
#ifdef VFN_ABLATE_V
                dst[2 * tc] = u32x4{(unsigned)lane, (unsigned)st, 0x3f803f80u, 0x3f803f80u};
                dst[2 * tc + 1] = u32x4{0x3f803f80u, (unsigned)tc, 0u, 0u};
#else
                dst[2 * tc] = __builtin_amdgcn_raw_buffer_load_b128(vrsrc, vlane_off, 2 * st * VBLK + tc * 512, 0);
                if constexpr (X3) dst[2 * tc + 1] = __builtin_amdgcn_raw_buffer_load_b128(vrsrc, vlane_off, 2 * st * VBLK + DV * 16 + tc * 512, 0);
#endif
            }
        };
        if constexpr (X3) load_v(0, vop[0]);         // lands behind the score GEMM
        else {
#pragma unroll
            for (int st = 0; st < 3; ++st) load_v(st, vop[st]);
        }

        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        {
            const int ra = wr * 32 + li, rq = wq * 32 + li;
            const char* kb = reinterpret_cast<const char*>(sK);
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const bf16x8 ah = *reinterpret_cast<const bf16x8*>(kb + swzk(ra, 0, 2 * g + lh));
                bf16x8 al = ah;
                if constexpr (X3) al = *reinterpret_cast<const bf16x8*>(kb + swzk(ra, 1, 2 * g + lh));
                const bf16x8 bh = *reinterpret_cast<const bf16x8*>(sQh + swzq(rq, 2 * g + lh));
                bf16x8 bl = bh;
                if constexpr (X3) bl = *reinterpret_cast<const bf16x8*>(sQl + swzq(rq, 2 * g + lh));
                mfma_lp<X3>(acc, ah, al, bh, bl);
            }
        }

        const int rloc = wr * 32 + 4 * lh;
        const int mycnt = softmax_hits(acc, p.scale, qm, qinv, p.thres, B - b0, rloc);
#pragma unroll
        for (int g = 0; g < 4; ++g) {                // registers 4g..4g+3 = 4 consecutive bank rows of query qcol
            const int brow = rloc + 8 * g;
            bf16x4 h, l;
#pragma unroll
            for (int e = 0; e < 4; ++e) { h[e] = (__bf16)acc[4 * g + e]; l[e] = (__bf16)(acc[4 * g + e] - (float)h[e]); }
            const int off = swzp(qcol, brow >> 3) + ((brow >> 2) & 1) * 8;
            *reinterpret_cast<bf16x4*>(sPh + off) = h;
            if constexpr (X3) *reinterpret_cast<bf16x4*>(sPl + off) = l;
        }
        if (p.cnt && lh == 0 && mycnt > 0) {
            const int row = b0 + wr * 32 + li;
            if (row < B) atomicAdd(p.cnt + (size_t)obj * p.stride_cnt + row, mycnt);
        }
        __syncthreads();                             // P^T visible; every wave is done reading sK
        if (more) chunk_load_async8(sK, K + (size_t)(b0 + CH) * DK, min(CH, B - b0 - CH), wave, lane);

        // O^T[q][ch] += sum_b P^T[q][b] V[b][ch]: A = P^T (2 query tiles), B = value rows (4 channel tiles)
#pragma unroll
        for (int st = 0; st < CH / 16; ++st) {
            if constexpr (X3) { if (st + 1 < CH / 16) load_v(st + 1, vop[(st + 1) & 1]); }
            const u32x4 (&vv)[8] = vop[X3 ? (st & 1) : st % 3];
#pragma unroll
            for (int tq = 0; tq < 2; ++tq) {
                const int prow = qhalf * 64 + tq * 32 + li;
                const bf16x8 ph = *reinterpret_cast<const bf16x8*>(sPh + swzp(prow, 2 * st + lh));
                bf16x8 pl = ph;
                if constexpr (X3) pl = *reinterpret_cast<const bf16x8*>(sPl + swzp(prow, 2 * st + lh));
#pragma unroll
                for (int tc = 0; tc < 4; ++tc) {
                    const bf16x8 vh = __builtin_bit_cast(bf16x8, vv[2 * tc]);
                    const bf16x8 vl = X3 ? __builtin_bit_cast(bf16x8, vv[2 * tc + 1]) : vh;
                    mfma_lp<X3>(o[tq][tc], ph, pl, vh, vl);
                }
            }
            if constexpr (!X3) {
                if (st == 0) { __builtin_amdgcn_sched_barrier(0); load_v(3, vop[0]); }
            }
        }
        __syncthreads();
    }

    float* dst = p.o_part + ((size_t)obj * p.nsplit + split) * p.HW * DV;
#pragma unroll
    for (int tq = 0; tq < 2; ++tq)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int q = q0 + qhalf * 64 + tq * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (q < p.HW) {
#pragma unroll
                for (int tc = 0; tc < 4; ++tc) dst[(size_t)q * DV + cq * 128 + tc * 32 + li] = o[tq][tc][r];
            }
        }
}

// ------------------------------------------------------------------ pass 2, plain bf16, software-pipelined (round 6)
// memread_apply_shw_kernel<false> walks a chunk as  [score GEMM -> softmax -> P^T to LDS] barrier [P^T V] barrier : all eight waves do
// the vector work (exp, threshold ballots, bf16 conversion: ~850 VALU cycles per wave and chunk, v_exp at quarter rate) TOGETHER
// between two barriers, with the matrix pipe idle, then the matrix work together with the vector pipe idle -- and its value rows are
// requested at most one chunk phase ahead (rocprofv3, round 5: mfma_util 0.27, 0.64 of the wave cycles waiting; 0.27 of the bf16 peak
// on the kernel that is 50-70 % of a C5 frame).  Here the loop is skewed by one chunk INSIDE every wave:
//
//     iteration c:   score GEMM of chunk c+1 (8 MFMAs)
//                    4 x { P^T V step of chunk c (8 MFMAs)  ||  a quarter of chunk c+1's softmax (VALU, in the MFMAs' shadow)
//                          -> its quarter of P^T(c+1) into the OTHER P^T buffer;  the value rows of (c+1, step) requested into the
//                          operand registers the step has just consumed: a whole chunk of lead }
//                    hit counts of chunk c+1; keys of chunk c+2: registers -> LDS        ONE barrier per chunk
//
// Keys go through registers (two 16-byte loads per thread at the top of an iteration, stored to LDS in front of its barrier), not by
// LDS-DMA: with a DMA in flight hipcc turns every wait for a register load into a full drain, which would
// put the value rows' latency back on the chain.  Only the hi plane of the key image is staged (256-byte rows: 16 KB per chunk).
// Registers are what the structure costs (128 accumulators + 64 value operands + 16 scores + 8 keys of 256): every LDS address is
// ONE xor away from a per-lane base (the swizzles are xors with lane constants), and the bases are made opaque once per iteration so
// that hipcc does not hoist the 30 derived addresses into registers of their own (a first form spilled 21 registers; each reload of a
// spilled ADDRESS was a scratch load with a full vmcnt(0) drain in front of the LDS access -- the value rows' lead thrown away).
// Same products in the same order as memread_apply_shw_kernel<false> (same fragments, same k order, same chunk order): bit-identical.
// LDS: query image 32 KB + 2 key chunks 32 KB + 2 P^T 32 KB = 96 KB; one workgroup of 8 waves per CU.
constexpr size_t APPLY_PIPE_LDS = (size_t)QTW * DK * 2 + 2 * (size_t)CH * DK * 2 + 2 * (size_t)QTW * CH * 2;
constexpr unsigned PIPE_K0 = QTW * DK * 2;                    // byte offsets inside the dynamic LDS: key buffers
constexpr unsigned PIPE_P0 = PIPE_K0 + 2 * CH * DK * 2;       // P^T buffers
constexpr unsigned PIPE_KB = CH * DK * 2, PIPE_PB = QTW * CH * 2;     // bytes of one key / P^T buffer

__global__ __launch_bounds__(512, 1)
void memread_apply_pipe_kernel(const vfn_memread_desc p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sQh = smem;                                         // [128 q][256 B] bf16, swzq

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int wr = wave >> 2, wq = wave & 3;                  // score tile: key rows 32wr.., query columns 32wq..
#ifdef PIPE_2X4
    constexpr int TQN = 2, TCN = 4;                           // P^T V tiles per wave: 2 query tiles x 4 channel tiles (memread_apply_shw_kernel's)
    const int qbase = (wave >> 2) * 64, cbase = (wave & 3) * 128;
#else
    // 4 query tiles x 2 channel tiles: every value row is requested by ONE wave of the workgroup.  With 2 x 4 the two waves that share
    // a channel quarter both request it -- 144 KB per chunk and CU through L1 / L2 instead of 80 KB, 15 TB/s chip-wide at the rate this
    // kernel runs: the L2's limit (an ablation with constant value operands ran 28 % faster).  P^T fragments are read from LDS twice as
    // often instead (128 KB per chunk: 1024 of ~5000 cycles), and the operand registers halve (32 instead of 64).
    constexpr int TQN = 4, TCN = 2;
    const int qbase = 0, cbase = wave * 64;
#endif
    int split, qt, obj, q0, B;
    apply_slice(p, split, qt, obj, q0, B);
    const char* Kimg = reinterpret_cast<const char*>(p.bank_k_lp) + (size_t)obj * p.stride_k * 4;   // image rows of 512 B: [128 hi | 128 lo]
    const char* V = reinterpret_cast<const char*>(p.bank_v_lp) + (size_t)obj * p.stride_v * 4;      // blocks of 8 rows, 16 KB

    {   // query image
        const int c = tid & 31;
        for (int r = tid >> 5; r < QTW; r += 16) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (q0 + r < p.HW) v = *reinterpret_cast<const f32x4*>(p.q + (size_t)(q0 + r) * p.ldq + c * 4);
            const bf16x4 h = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
            *reinterpret_cast<bf16x4*>(sQh + swzq(r, c >> 1) + (c & 1) * 8) = h;
        }
    }

    int c_lo, c_hi;
    chunk_range(B, p.nsplit, split, c_lo, c_hi);
    const int n = c_hi - c_lo;

    f32x16 o[TQN][TCN];                                       // O^T tiles: [query tile][channel tile]
#pragma unroll
    for (int a = 0; a < TQN; ++a)
#pragma unroll
        for (int b = 0; b < TCN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[a][b][r] = 0.f;

    const int qcol = wq * 32 + li;
    float qm, qinv;
    load_qstats(p, obj, q0, qcol, qm, qinv);
    const float sm = -qm;
    const int rloc = wr * 32 + 4 * lh;                        // this lane's first score row inside a chunk (+ (r & 3) + 8 (r >> 2))

    if (n > 0) {
        const unsigned vlane_off = (unsigned)lh * VBLK + (unsigned)(cbase + li) * 16u;         // bytes: row block lh of a step, channel
        const int krow = tid >> 3, kc2 = (tid & 7) * 2;                                        // key staging: row, first of two 16-byte chunks
        const unsigned klane_off = (unsigned)krow * 512u + (unsigned)kc2 * 16u;
        // LDS byte addresses, each ONE xor away from a per-lane base (swzq / swzp are xors of the 16-byte chunk index with lane constants):
        //   key fragment g of the score GEMM     bK ^ 32 g  (+ buffer)     bK = swzq(32 wr + li, lh)
        //   query fragment g                     bQ ^ 32 g                 bQ = swzq(32 wq + li, lh)
        //   P^T fragment of step st, tile tq     bR ^ 32 st + 4096 tq (+ buffer)      bR = swzp(qbase + li, lh)
        //   P^T store of softmax quarter g       bW ^ 16 g  (+ buffer)     bW = swzp(qcol, 4 wr) + 8 lh   (rows rloc + 8 g: chunk 4 wr + g, half lh)
        //   key staging store                    swzq(krow, kc2), swzq(krow, kc2 + 1)  (+ buffer)
        unsigned bK = PIPE_K0 + (unsigned)swzq(wr * 32 + li, lh);
        unsigned bQ = (unsigned)swzq(wq * 32 + li, lh);
        unsigned bR = PIPE_P0 + (unsigned)swzp(qbase + li, lh);
        unsigned bW = PIPE_P0 + (unsigned)swzp(qcol, 4 * wr) + 8u * lh;
        unsigned bS = PIPE_K0 + (unsigned)swzq(krow, kc2);
        const unsigned bS1 = (unsigned)(swzq(krow, kc2 + 1) - swzq(krow, kc2));                 // (+16 or -16: the pair's second chunk)
        auto lds = [&](unsigned a) { return smem + a; };
        u32x4 vop[4][TCN];                                    // value operands: [step][channel tile] (8 bank rows x 1 channel, bf16)
        u32x4 kreg[2];
        f32x16 acc;
        int mycnt = 0;

        // buffer descriptors over ONE chunk's live rows: key rows / value row blocks past the bank end read zeros through the range check
        auto vres = [&](int c) {
            const int b0 = c * CH;
            return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(V + (size_t)(b0 >> 3) * VBLK), 0, ((min(CH, B - b0) + 7) >> 3) * (int)VBLK, 0x00020000);
        };
        auto kres = [&](int c) {
            const int b0 = c * CH;
            return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(Kimg + (size_t)b0 * 512), 0, min(CH, B - b0) * 512, 0x00020000);
        };
        auto load_v = [&](const __amdgpu_buffer_rsrc_t& r, int st, auto SLOT_) {
            constexpr int slot = decltype(SLOT_)::value;
#ifdef PIPE_ABLATE_V
            for (int tc = 0; tc < TCN; ++tc) vop[slot][tc] = u32x4{0x3f803f80u + (unsigned)st, 0x3f803f80u, 0x3f803f80u + (unsigned)tc, 0x3f803f80u};
#else
#pragma unroll
            for (int tc = 0; tc < TCN; ++tc) vop[slot][tc] = __builtin_amdgcn_raw_buffer_load_b128(r, vlane_off, 2 * st * (int)VBLK + tc * 512, 0);
#endif
        };
        auto load_k = [&](int c) {
            const __amdgpu_buffer_rsrc_t r = kres(c);
            kreg[0] = __builtin_amdgcn_raw_buffer_load_b128(r, klane_off, 0, 0);
            kreg[1] = __builtin_amdgcn_raw_buffer_load_b128(r, klane_off, 16, 0);
        };
        auto store_k = [&](int buf) {
            const unsigned a = bS + buf * PIPE_KB;
            *reinterpret_cast<u32x4*>(lds(a)) = kreg[0];
            *reinterpret_cast<u32x4*>(lds(a + bS1)) = kreg[1];
        };
        auto score = [&](int buf) {
            const unsigned ak = bK + buf * PIPE_KB;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            // fragments of k-group g + 1 are requested in front of the MFMA of g (a first form read, waited, multiplied: eight exposed LDS
            // round trips with the matrix pipe idle -- both waves of a SIMD are in this section together)
            bf16x8 fa[2], fb[2];
            fa[0] = *reinterpret_cast<const bf16x8*>(lds(ak));
            fb[0] = *reinterpret_cast<const bf16x8*>(lds(bQ));
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                if (g + 1 < 8) {
                    fa[(g + 1) & 1] = *reinterpret_cast<const bf16x8*>(lds(ak ^ (32u * (g + 1))));
                    fb[(g + 1) & 1] = *reinterpret_cast<const bf16x8*>(lds(bQ ^ (32u * (g + 1))));
                }
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[g & 1], fb[g & 1], acc, 0, 0, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);      // 2 LDS reads, then 1 MFMA: keeps the requests one group ahead
                __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
            }
        };
        // a quarter of a chunk's softmax: score registers 4g .. 4g+3 = bank rows rloc + 8g + (0..3) of query qcol -> p, hit ballots, P^T
        auto softmax_quarter = [&](auto G_, int pbuf) {
            constexpr int g = decltype(G_)::value;
            float pv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) pv[e] = fast_exp(fmaf(acc[4 * g + e], p.scale, sm)) * qinv;
#ifndef PIPE_NO_HITS
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned long long hit = __ballot(pv[e] > p.thres);
                const int h_lo = __popcll(hit & 0xffffffffull), h_hi = __popcll(hit >> 32);      // wave-uniform
                asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(mycnt) : "s"(h_lo), "n"(e + 8 * g));
                asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(mycnt) : "s"(h_hi), "n"(e + 8 * g + 4));
            }
#endif
            const bf16x4 h = {(__bf16)pv[0], (__bf16)pv[1], (__bf16)pv[2], (__bf16)pv[3]};
            *reinterpret_cast<bf16x4*>(lds((bW + pbuf * PIPE_PB) ^ (16u * g))) = h;
        };
        // the bank's last chunk may be partial: its rows past the end got p = exp(0 - m) / l from the zero keys -- exactly 0 is required
        // (their value rows are stale).  Rare (one chunk per object): a fix-up of the lane's own P^T entries, outside the pipelined stream
        auto zero_dead_rows = [&](int pbuf, int nvalid) {
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (rloc + 8 * g + e >= nvalid) *reinterpret_cast<unsigned short*>(lds(((bW + pbuf * PIPE_PB) ^ (16u * g)) + e * 2)) = 0;
        };
        auto add_hits = [&](int c) {                          // one wave per 32 x 32 score tile: lane i (0..31) holds the hits of chunk row 32wr + i
            if (p.cnt && lh == 0 && mycnt > 0) {
                const int row = c * CH + wr * 32 + li;
                if (row < B) atomicAdd(p.cnt + (size_t)obj * p.stride_cnt + row, mycnt);
            }
            mycnt = 0;
        };
        auto pv_step = [&](auto ST_, auto SLOT_, int pbuf) {   // O^T[q][ch] += sum_b P^T[q][b] V[b][ch], 16 bank rows: TQN query tiles x TCN channel tiles
            constexpr int st = decltype(ST_)::value, slot = decltype(SLOT_)::value;
            const unsigned ar = (bR + pbuf * PIPE_PB) ^ (32u * st);
#pragma unroll
            for (int tq = 0; tq < TQN; ++tq) {
                const bf16x8 ph = *reinterpret_cast<const bf16x8*>(lds(ar + tq * 4096));
#ifdef PIPE_SETPRIO
                __builtin_amdgcn_s_setprio(1);
#endif
#pragma unroll
                for (int tc = 0; tc < TCN; ++tc)
                    o[tq][tc] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ph, __builtin_bit_cast(bf16x8, vop[slot][tc]), o[tq][tc], 0, 0, 0);
#ifdef PIPE_SETPRIO
                __builtin_amdgcn_s_setprio(0);
#endif
            }
        };
        using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>;
        using I2 = std::integral_constant<int, 2>; using I3 = std::integral_constant<int, 3>;
        auto opaque = [&]() {                                  // (keeps the derived LDS addresses out of loop-invariant registers)
            asm volatile("" : "+v"(bK), "+v"(bQ), "+v"(bR), "+v"(bW), "+v"(bS));
        };

        // ---- prologue: chunk c_lo's keys, value operands and P^T; chunk c_lo + 1's keys
        {
            const __amdgpu_buffer_rsrc_t vr = vres(c_lo);
            load_k(c_lo);
            load_v(vr, 0, I0{}); load_v(vr, 1, I1{}); load_v(vr, 2, I2{}); load_v(vr, 3, I3{});
            store_k(0);
            if (n > 1) load_k(c_lo + 1);
            __syncthreads();
            score(0);
            softmax_quarter(I0{}, 0); softmax_quarter(I1{}, 0); softmax_quarter(I2{}, 0); softmax_quarter(I3{}, 0);
            if (B - c_lo * CH < CH) zero_dead_rows(0, B - c_lo * CH);
            add_hits(c_lo);
            if (n > 1) store_k(1);
            __syncthreads();
        }

        // one iteration: chunk c = c_lo + i.  NEXT: chunk c + 1 exists (its scores / softmax / value requests ride along);
        // KNEXT: chunk c + 2 exists (its keys are staged)
        auto iter = [&](auto NEXT_, auto KNEXT_, int i) {
            constexpr bool NEXT = decltype(NEXT_)::value, KNEXT = decltype(KNEXT_)::value;
            const int c = c_lo + i;
            const int pc = i & 1, pn = pc ^ 1;
            opaque();
            if constexpr (KNEXT) load_k(c + 2);
            const __amdgpu_buffer_rsrc_t vr1 = vres(NEXT ? c + 1 : c);
#ifdef PIPE_NO_SCHEDBAR
#define PIPE_SB()
#else
#define PIPE_SB() __builtin_amdgcn_sched_barrier(0)
#endif
#ifdef PIPE_SCORE_LATE
            // (experiment) the score GEMM behind step 0's MFMAs, the softmax quarters one step later
            pv_step(I0{}, I0{}, pc);
            if constexpr (NEXT) { load_v(vr1, 0, I0{}); score(pn); }
            PIPE_SB();
            pv_step(I1{}, I1{}, pc);
            if constexpr (NEXT) { load_v(vr1, 1, I1{}); softmax_quarter(I0{}, pn); }
            PIPE_SB();
            pv_step(I2{}, I2{}, pc);
            if constexpr (NEXT) { load_v(vr1, 2, I2{}); softmax_quarter(I1{}, pn); }
            PIPE_SB();
            pv_step(I3{}, I3{}, pc);
            if constexpr (NEXT) { load_v(vr1, 3, I3{}); softmax_quarter(I2{}, pn); softmax_quarter(I3{}, pn); }
#else
            if constexpr (NEXT) score(pn);
            pv_step(I0{}, I0{}, pc);
            if constexpr (NEXT) { load_v(vr1, 0, I0{}); softmax_quarter(I0{}, pn); }
            PIPE_SB();
            pv_step(I1{}, I1{}, pc);
            if constexpr (NEXT) { load_v(vr1, 1, I1{}); softmax_quarter(I1{}, pn); }
            PIPE_SB();
            pv_step(I2{}, I2{}, pc);
            if constexpr (NEXT) { load_v(vr1, 2, I2{}); softmax_quarter(I2{}, pn); }
            PIPE_SB();
            pv_step(I3{}, I3{}, pc);
            if constexpr (NEXT) { load_v(vr1, 3, I3{}); softmax_quarter(I3{}, pn); }
#endif
            if constexpr (NEXT) {
                if (B - (c + 1) * CH < CH) zero_dead_rows(pn, B - (c + 1) * CH);
                add_hits(c + 1);
            }
            if constexpr (KNEXT) store_k(pc);                        // (chunk c's keys, read by the previous iteration's score GEMM, are dead)
            __syncthreads();
        };
        const std::true_type T{};
        const std::false_type F{};
        int i = 0;
        for (; i + 2 < n; ++i) iter(T, T, i);
        if (i + 1 < n) { iter(T, F, i); ++i; }
        iter(F, F, i);
    }

    float* dst = p.o_part + ((size_t)obj * p.nsplit + split) * p.HW * DV;
#pragma unroll
    for (int tq = 0; tq < TQN; ++tq)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int q = q0 + qbase + tq * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (q < p.HW) {
#pragma unroll
                for (int tc = 0; tc < TCN; ++tc) dst[(size_t)q * DV + cbase + tc * 32 + li] = o[tq][tc][r];
            }
        }
}

#ifdef VFN_CENSUS
#define PH_DECL unsigned long long ph_t = __builtin_amdgcn_s_memtime(), ph_acc[5] = {0, 0, 0, 0, 0}
#define PH_MARK(k) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); ph_acc[k] += t_ - ph_t; ph_t = t_; } while (0)
#else
#define PH_DECL
#define PH_MARK(k)
#endif
// ------------------------------------------------------------------ pass 2 (f32), wide query tile
// 128 query columns per workgroup, 8 waves: the score tile is 64 x 128 (one 32x32 tile per wave), wave w then owns
// value channels 64w..64w+63 for all 128 queries: a key chunk and a value row are fetched once per 128 queries and a
// chunk costs one barrier pair per 128 queries.
// LDS: queries [128][128] 64 KB + key chunk 32 KB + P^T [128 q][64 b] 32 KB = 128 KB, one workgroup per CU.
__global__ __launch_bounds__(512, 1)
void memread_apply_wide_kernel(const vfn_memread_desc p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sQ = reinterpret_cast<float*>(smem);      // [128][128]
    float* sK = sQ + QTW * DK;                       // [64][128]
    float* sP = sK + CH * DK;                        // [128 q][64 b]  (P^T)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int wr = wave >> 2, wq = wave & 3;
    int split, qt, obj, q0, B;
    apply_slice(p, split, qt, obj, q0, B);
    const float* K = p.bank_k + (size_t)obj * p.stride_k;
    const float* V = p.bank_v + (size_t)obj * p.stride_v;

    {   // query image (zero past HW): f32 rows under swz
        const int c = tid & 31;
        for (int r = tid >> 5; r < QTW; r += 16) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (q0 + r < p.HW) v = *reinterpret_cast<const f32x4*>(p.q + (size_t)(q0 + r) * p.ldq + c * 4);
            *reinterpret_cast<f32x4*>(sQ + swz(r, c)) = v;
        }
    }

    int c_lo, c_hi;
    chunk_range(B, p.nsplit, split, c_lo, c_hi);

    f32x16 o[4][2];                                  // O^T tiles: [query tile][channel tile]
    zero_o(o);

    // lane li owns channels 2*li, 2*li+1 (tile tc) of the wave's 64.  (vcol is unused, but the kernel's register allocation changes without it)
    const float* vcol = V + wave * 64 + li * 2;
    const unsigned vlane_off = (unsigned)((4 * lh) * DV + wave * 64 + li * 2) * 4u;   // bytes, per lane

    if (c_lo < c_hi) chunk_load_async8(sK, K + (size_t)c_lo * CH * DK, min(CH, B - c_lo * CH), wave, lane);
    __syncthreads();

    const int qcol = wq * 32 + li;
    // (written out: load_qstats changes this kernel's register allocation)
    const bool qok = (q0 + qcol) < p.HW;
    float qm = 1e30f, qinv = 0.f;
    if (qok) {
        qm = p.ml[((size_t)obj * p.HW + q0 + qcol) * 2];
        qinv = 1.f / p.ml[((size_t)obj * p.HW + q0 + qcol) * 2 + 1];
    }

    PH_DECL;
    for (int c = c_lo; c < c_hi; ++c) {
        const int b0 = c * CH;
        const bool more = c + 1 < c_hi;

        f32x16 acc;
        score_tile(sK, sQ, wr, wq, li, lh, acc);
        PH_MARK(0);

        const int rloc = wr * 32 + 4 * lh;
        const int mycnt = softmax_hits(acc, p.scale, qm, qinv, p.thres, B - b0, rloc);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int brow = rloc + 8 * g;
            const f32x4 v = {acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
            *reinterpret_cast<f32x4*>(sP + swz64(qcol, brow >> 2)) = v;
        }
        if (p.cnt && lh == 0 && mycnt > 0) {
            const int row = b0 + wr * 32 + li;
            if (row < B) atomicAdd(p.cnt + (size_t)obj * p.stride_cnt + row, mycnt);
        }
        PH_MARK(1);
        __syncthreads();                             // P^T visible; every wave is done reading sK
        PH_MARK(2);
        if (more) chunk_load_async8(sK, K + (size_t)(b0 + CH) * DK, min(CH, B - b0 - CH), wave, lane);

        f32x2 vb[3][4];                              // ring: value rows two k-groups ahead of their MFMAs
        // whole chunks read their value rows through a buffer descriptor (scalar base and row offset, one per-lane byte
        // offset): the 64-bit clamped addresses of the tail form cost ~7 vector-ALU instructions per load, and VALU
        // issue comes straight out of the MFMA pipe's time on this SIMD
        // (round 5: the resource ends at the bank's last row -- one load form for every chunk, see memread_apply_ss_kernel)
        const __amdgpu_buffer_rsrc_t vrsrc = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(V + (size_t)b0 * DV), 0, min(CH, B - b0) * DV * 4, 0x00020000);
        auto load_v = [&](int kk, int slot) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                vb[slot][t] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(vrsrc, vlane_off + (unsigned)((8 * kk + t) * DV * 4), 0, 0));
        };
        load_v(0, 0);
        load_v(1, 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = 0; kk < CH / 8; ++kk) {
            const int cur = kk % 3;
            if (kk + 2 < CH / 8) load_v(kk + 2, (kk + 2) % 3);
            __builtin_amdgcn_sched_barrier(0);
            const int lc = 2 * kk + lh;
            f32x4 a[4];
#pragma unroll
            for (int tq = 0; tq < 4; ++tq) a[tq] = *reinterpret_cast<const f32x4*>(sP + swz64(tq * 32 + li, lc));
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int tq = 0; tq < 4; ++tq) {
                    o[tq][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tq][t], vb[cur][t][0], o[tq][0], 0, 0, 0);
                    o[tq][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tq][t], vb[cur][t][1], o[tq][1], 0, 0, 0);
                }
        }
        PH_MARK(3);
        __syncthreads();                             // next chunk's keys visible; sP free again
        PH_MARK(4);
    }
#ifdef VFN_CENSUS
    if ((threadIdx.x & 63) == 0) {
        const int lin = (blockIdx.y * gridDim.x + blockIdx.x) * 8 + (threadIdx.x >> 6);
        if (lin < 2048) {
            for (int k = 0; k < 5; ++k) vfn_census_buf[lin * 8 + k] = ph_acc[k];
            vfn_census_buf[lin * 8 + 5] = c_hi - c_lo;
        }
    }
#endif

    float* dst = p.o_part + ((size_t)obj * p.nsplit + split) * p.HW * DV;
#pragma unroll
    for (int tq = 0; tq < 4; ++tq)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int q = q0 + tq * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (q < p.HW) {
                const f32x2 v = {o[tq][0][r], o[tq][1][r]};
                *reinterpret_cast<f32x2*>(dst + (size_t)q * DV + wave * 64 + li * 2) = v;
            }
        }
}

// ------------------------------------------------------------------ pass 2 (f32), wide tile, scores from the scan
// The statistics scan has already formed every score <key, query> of the frame; with vfn_bankscan_desc.scores it also
// stores them (HW x B floats per object: 363 MB at the C2 mean bank, written once and read once -- the bytes the key
// chunks cost before).  This kernel then has no score GEMM, no query image and no key chunks: it loads the 16 scores of
// its 32 x 32 tile position (a chunk ahead), runs the softmax, and goes on as memread_apply_wide_kernel.  The scan sums
// the same products in the same order, so O^T and the hit counts are bit-identical to the recomputing kernel; the frame
// executes F_min's 1280 B HW FLOP per object for the memory read instead of 1536.
// LDS: two P^T buffers [128 q][64 b], 64 KB.
// One (bank slice, query tile, object) item of memread_apply_ss_kernel.  LIVE = 32-column groups of the tile that hold query
// columns (4 except on a last tile cut into its own nsplit_tail slices): groups LIVE..3 get no MFMAs, no P^T fragment reads and
// no epilogue stores, and the waves that would run their softmax (wq >= LIVE) load no scores -- nobody reads those P^T columns,
// and their hit counts were 0 (p = 0 exactly past HW).  Per live group the products and their order do not depend on LIVE.
template <int LIVE>
__device__ __forceinline__ void apply_ss_item(const vfn_memread_desc& p, float* sP, int split, int nslices, int qt, int obj, int q0, int B) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int wr = wave >> 2, wq = wave & 3;
    const bool smx = LIVE == 4 || wq < LIVE;         // this wave's softmax column block holds query columns (wave-uniform)
    const int qtiles = (p.HW + QTW - 1) / QTW;
    const float* V = p.bank_v + (size_t)obj * p.stride_v;
    const float* S = p.scores + (size_t)obj * p.stride_scores;

    int c_lo, c_hi;
    chunk_range(B, nslices, split, c_lo, c_hi);

    f32x16 o[LIVE][2];                               // O^T tiles: [query tile][channel tile]
#pragma unroll
    for (int a = 0; a < LIVE; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[a][b][r] = 0.f;

    // lane li owns channels 2*li, 2*li+1 (tile tc) of the wave's 64
    const unsigned vlane_off = (unsigned)((4 * lh) * DV + wave * 64 + li * 2) * 4u;   // bytes, per lane
    // this lane's 16 scores of a chunk: key rows 32wr + (r&3) + 8(r>>2) + 4lh, query column 32wq + li
    const unsigned slane_off = (unsigned)(((wr * 4) * 2 + lh) * QTW + wq * 32 + li) * 16u;      // bytes; + g * 2 * QTW * 16
    f32x4 sv[4];
    auto load_scores = [&](int c) {
        const char* tile = reinterpret_cast<const char*>(S + ((size_t)c * qtiles + qt) * (CH * QTW));
#pragma unroll
        for (int g = 0; g < 4; ++g) sv[g] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(tile + slane_off + g * (2 * QTW * 16)));
    };
    const int qcol = wq * 32 + li;
    float qm, qinv;
    load_qstats(p, obj, q0, qcol, qm, qinv);
    const int rloc = wr * 32 + 4 * lh;
    // softmax of chunk c from the loaded scores -> P^T buffer `buf`, hit counts
    auto softmax_to = [&](int c, float* sPb) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = sv[r >> 2][r & 3];
        const int b0 = c * CH;
        const int mycnt = softmax_hits(acc, p.scale, qm, qinv, p.thres, B - b0, rloc);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int brow = rloc + 8 * g;
            const f32x4 v = {acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
            *reinterpret_cast<f32x4*>(sPb + swz64(qcol, brow >> 2)) = v;
        }
        if (p.cnt && lh == 0 && mycnt > 0) {
            const int row = b0 + wr * 32 + li;
            if (row < B) atomicAdd(p.cnt + (size_t)obj * p.stride_cnt + row, mycnt);
        }
    };

    // value rows: a ring of four k-groups that runs ACROSS the chunks (round 5).  Within a chunk a group is requested two groups ahead of
    // its MFMAs; the last two groups of a chunk request the first two of the NEXT chunk (8 groups per chunk, 8 % 4 = 0: the slots stay
    // compile-time constants), so a chunk no longer opens with the matrix pipe waiting a full memory latency for its first value rows --
    // both waves of a SIMD leave the chunk barrier together and used to wait there together.  A chunk's buffer resource ends at the
    // bank's last row (rows past it read 0; P is exactly 0 there); behind the slice's last chunk it is empty (loads return 0, no traffic).
    f32x2 vb[4][4];
    auto chunk_rsrc = [&](int c) {
        const int rows = c < c_hi ? min(CH, B - c * CH) : 0;
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(V + (size_t)min(c, max(c_hi - 1, 0)) * CH * DV), 0, rows * DV * 4, 0x00020000);
    };
    auto load_v = [&](const __amdgpu_buffer_rsrc_t& rs, int kk, int slot) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
            vb[slot][t] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs, vlane_off + (unsigned)((8 * kk + t) * DV * 4), 0, 0));
    };
    if (c_lo < c_hi) {
        const __amdgpu_buffer_rsrc_t rs0 = chunk_rsrc(c_lo);
        load_v(rs0, 0, 0);
        load_v(rs0, 1, 1);
        if (smx) {
            load_scores(c_lo);
            softmax_to(c_lo, sP);
            if (c_lo + 1 < c_hi) load_scores(c_lo + 1);
        }
    }
    __syncthreads();                                 // P^T of the first chunk visible

    // P^T is double-buffered: the softmax of chunk c+1 is issued in the middle of chunk c's P^T V loop (plain VALU work on
    // registers -- the scores were loaded a chunk ahead -- that runs under the queued MFMAs) and written to the other
    // buffer, so a chunk costs ONE barrier and the matrix pipe does not idle through the softmax
    for (int c = c_lo; c < c_hi; ++c) {
        const int b0 = c * CH;
        const int buf = (c - c_lo) & 1;
        const float* sPc = sP + buf * (QTW * CH);
        float* sPn = sP + (buf ^ 1) * (QTW * CH);
        const bool nxt = c + 1 < c_hi;

        const __amdgpu_buffer_rsrc_t vrsrc = chunk_rsrc(c), vrsrc_n = chunk_rsrc(c + 1);
        f32x4 a[2][LIVE];                            // P^T fragments, one k-group ahead of their MFMAs
#pragma unroll
        for (int tq = 0; tq < LIVE; ++tq) a[0][tq] = *reinterpret_cast<const f32x4*>(sPc + swz64(tq * 32 + li, lh));
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = 0; kk < CH / 8; ++kk) {
            const int cur = kk % 4;
            if (kk + 2 < CH / 8) load_v(vrsrc, kk + 2, (kk + 2) % 4);
            else load_v(vrsrc_n, kk + 2 - CH / 8, (kk + 2) % 4);
            if (kk + 1 < CH / 8) {
#pragma unroll
                for (int tq = 0; tq < LIVE; ++tq)
                    a[(kk + 1) & 1][tq] = *reinterpret_cast<const f32x4*>(sPc + swz64(tq * 32 + li, 2 * (kk + 1) + lh));
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int tq = 0; tq < LIVE; ++tq) {
                    o[tq][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk & 1][tq][t], vb[cur][t][0], o[tq][0], 0, 0, 0);
                    o[tq][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk & 1][tq][t], vb[cur][t][1], o[tq][1], 0, 0, 0);
                }
            if (kk == 2 && nxt && smx) {
                softmax_to(c + 1, sPn);
                if (c + 2 < c_hi) load_scores(c + 2);
            }
        }
        __syncthreads();                             // P^T of chunk c+1 visible; everyone is done with this buffer
    }

    float* dst = p.o_part + ((size_t)obj * p.nsplit + split) * p.HW * DV;
#pragma unroll
    for (int tq = 0; tq < LIVE; ++tq)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int q = q0 + tq * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (q < p.HW) {
                const f32x2 v = {o[tq][0][r], o[tq][1][r]};
                *reinterpret_cast<f32x2*>(dst + (size_t)q * DV + wave * 64 + li * 2) = v;
            }
        }
}

// Workgroup -> item when the last query tile has its own slice count (nsplit_tail > 0): per object nsplit x (qtiles - 1) items
// of the full tiles, slice-major, then the last tile's nsplit_tail items.  The XCD dealing is apply_item's: an XCD takes a
// contiguous run of items, so the full tiles of one (object, slice) -- the ones that stream the same value rows -- share an L2;
// a slice of the last tile covers other rows than any full-tile slice and has no partner to share with.  Bijective for any grid.
__device__ __forceinline__ void apply_tail_item(const vfn_memread_desc& p, int qtiles, int& split, int& qt, int& obj) {
    const int per_obj = (int)gridDim.x;              // (qtiles - 1) * nsplit + nsplit_tail
    int L = (int)blockIdx.x;
    obj = (int)blockIdx.y;
    if (!vfn_apply_linear_order) {
        const int total = (int)(gridDim.x * gridDim.y);
        const int id = (int)(blockIdx.y * gridDim.x + blockIdx.x);
        const int q = total >> 3, r = total & 7;
        const int xcd = id & 7, slot = id >> 3;
        L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
        obj = L / per_obj;
        L -= obj * per_obj;
    }
    const int full = (qtiles - 1) * p.nsplit;
    if (L < full) { split = L / (qtiles - 1); qt = L - split * (qtiles - 1); }
    else { split = L - full; qt = qtiles - 1; }
}

__global__ __launch_bounds__(512, 1)
void memread_apply_ss_kernel(const vfn_memread_desc p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sP = reinterpret_cast<float*>(smem);      // [128 q][64 b]  (P^T)
    int split, qt, obj, q0, B;
    if (p.nsplit_tail <= 0) {                        // every tile in nsplit slices, all four column groups computed
        apply_slice(p, split, qt, obj, q0, B);
        apply_ss_item<4>(p, sP, split, p.nsplit, qt, obj, q0, B);
        return;
    }
    const int qtiles = (p.HW + QTW - 1) / QTW;
    apply_tail_item(p, qtiles, split, qt, obj);
    q0 = qt * QTW;
    B = p.bank_len[obj];
    const int live = qt == qtiles - 1 ? (p.HW - q0 + 31) >> 5 : 4;      // workgroup-uniform
    if (live == 4) apply_ss_item<4>(p, sP, split, qt == qtiles - 1 ? p.nsplit_tail : p.nsplit, qt, obj, q0, B);
    else if (live == 3) apply_ss_item<3>(p, sP, split, p.nsplit_tail, qt, obj, q0, B);
    else if (live == 2) apply_ss_item<2>(p, sP, split, p.nsplit_tail, qt, obj, q0, B);
    else apply_ss_item<1>(p, sP, split, p.nsplit_tail, qt, obj, q0, B);
}

// out[obj][q][0:512] = sum_split o_part ; out[obj][q][512:1024] = query value; then the hit-count bump
__global__ void memread_finish_kernel(const vfn_memread_desc p) {
    const int obj = blockIdx.y;
    const size_t total = (size_t)p.HW * (DV / 4);
    const int last_q0 = (p.HW - 1) / QTW * QTW;      // first row of the last query tile of the apply kernels
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c4 = i % (DV / 4);
        const int q = i / (DV / 4);
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        const int ns = p.nsplit_tail > 0 && q >= last_q0 ? p.nsplit_tail : p.nsplit;      // slabs written for this row
        for (int sp = 0; sp < ns; ++sp)
            s += *reinterpret_cast<const f32x4*>(p.o_part + (((size_t)obj * p.nsplit + sp) * p.HW + q) * DV + c4 * 4);
        float* o = p.out + ((size_t)obj * p.HW + q) * p.ld_out;
        *reinterpret_cast<f32x4*>(o + c4 * 4) = s;
        if (p.qv) *reinterpret_cast<f32x4*>(o + DV + c4 * 4) = *reinterpret_cast<const f32x4*>(p.qv + (size_t)q * p.ldqv + c4 * 4);
    }
    if (p.cnt) {
        const int B = p.bank_len[obj];
        int* cnt = p.cnt + (size_t)obj * p.stride_cnt;
        float* info = p.info + (size_t)obj * p.stride_info;
        for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) {
            info[(size_t)b * 2 + 1] += logf((float)cnt[b] + 1.f);
            cnt[b] = 0;
        }
    }
}

constexpr size_t SCAN_LDS = (size_t)(2 * CH * DK) * sizeof(float);

// The score tiles of one object: one 8192-float tile per (64-entry chunk, 128-query tile); the capacity is what the key
// slab holds per object (stride_k / 128 entries).  An undersized buffer is refused here rather than overrun on the device.
bool scores_fit(long long stride_scores, long long stride_k, int HW) {
    const long long cap = stride_k / DK;
    return stride_scores >= ((cap + CH - 1) / CH) * (long long)((HW + 127) / 128) * 8192;
}

template <typename K>
void allow_lds(K kern, size_t bytes) {
    hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// an integer switch from the environment; unset -> dflt
int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}

}  // namespace

extern "C" int vfn_bank_scan(const vfn_bankscan_desc* d, void* stream) {
    if (!d || !d->q || !d->bank_k || !d->bank_len || !d->part) return VFN_ERR_ARG;
    if (d->nsplit < 1 || d->HW < 1 || d->obj_n < 1 || d->ldq % 4) return VFN_ERR_ARG;
    if (d->mode == 1 && (!d->rowscale || d->stride_rs % 4)) return VFN_ERR_ARG;
    if (d->precision < 0 || d->precision > 2) return VFN_ERR_ARG;
    if (d->scores && (d->mode != 0 || !scores_fit(d->stride_scores, d->stride_k, d->HW))) return VFN_ERR_ARG;
    // one-time set-up: LDS limits of every kernel this launcher can pick (the register-staged kernels fit the default limit), and
    // VFN_SCAN_WGS: 32 KB of LDS and <= 160 registers -- three register-staged workgroups fit a CU (the queue feeds any number)
    static const int pipe_wgs = [] {
        allow_lds(bank_scan_kernel<0, 0>, SCAN_LDS); allow_lds(bank_scan_kernel<1, 0>, SCAN_LDS);
        allow_lds(bank_scan_kernel<0, 1>, SCAN_LDS); allow_lds(bank_scan_kernel<1, 1>, SCAN_LDS);
        allow_lds(bank_scan_kernel<0, 2>, SCAN_LDS); allow_lds(bank_scan_kernel<1, 2>, SCAN_LDS);
        const int wgs = env_int("VFN_SCAN_WGS", 768);
        return wgs < 1 ? 768 : wgs;
    }();
    if (!d->work_counter) return VFN_ERR_ARG;
    const int items = cdiv(d->HW, QTS) * d->nsplit * d->obj_n;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(d->work_counter, 0, sizeof(int), s) != hipSuccess) return VFN_ERR_LAUNCH;
    // plain bf16 on the kept key image (round 6): keys through registers, two chunks ahead; VFN_SCAN_PIPE=0 (read at every
    // call: A/B in one process) restores bank_scan_kernel<MODE, 1>
    const bool pipe = d->precision == 1 && d->bank_k_lp && env_int("VFN_SCAN_PIPE", 1) != 0;
    // otherwise two resident workgroups per CU (64 KB of LDS each)
    const int wgs = pipe ? pipe_wgs : 512;
    const dim3 grid(items < wgs ? items : wgs), block(256);
    auto scan = [&](auto kern) { hipLaunchKernelGGL(kern, grid, block, SCAN_LDS, s, *d, scan_gather{}); };
    if (pipe) {
        if (d->mode == 0) hipLaunchKernelGGL((bank_scan_pipe_kernel<0>), grid, block, SCAN_PIPE_LDS, s, *d);
        else hipLaunchKernelGGL((bank_scan_pipe_kernel<1>), grid, block, SCAN_PIPE_LDS, s, *d);
    } else if (d->mode == 0) {
        if (d->precision == 0) scan(bank_scan_kernel<0, 0>);
        else if (d->precision == 1) scan(bank_scan_kernel<0, 1>);
        else scan(bank_scan_kernel<0, 2>);
    } else if (d->mode == 1) {
        if (d->precision == 0) scan(bank_scan_kernel<1, 0>);
        else if (d->precision == 1) scan(bank_scan_kernel<1, 1>);
        else scan(bank_scan_kernel<1, 2>);
    } else {
        return VFN_ERR_ARG;
    }
    return vfn_check_launch();
}

extern "C" int vfn_bank_scan_finish(const float* part, int nsplit, int HW, int obj_n, int mode, float* ml, int* idx,
                                    float* corr, const float* colscale, void* stream) {
    if (!part) return VFN_ERR_ARG;
    const int total = obj_n * HW;
    if (mode == 0) {
        if (!ml) return VFN_ERR_ARG;
        hipLaunchKernelGGL(bank_scan_finish_kernel<0>, dim3(cdiv(total * 8, 256)), dim3(256), 0, (hipStream_t)stream,
                           part, nsplit, HW, obj_n, ml, idx, corr, colscale);
    } else {
        if (!idx || !corr || !colscale) return VFN_ERR_ARG;
        hipLaunchKernelGGL(bank_scan_finish_kernel<1>, dim3(cdiv(total * 8, 256)), dim3(256), 0, (hipStream_t)stream,
                           part, nsplit, HW, obj_n, ml, idx, corr, colscale);
    }
    return vfn_check_launch();
}

extern "C" int vfn_bank_match_certified(const vfn_bankmatch_desc* d, void* stream) {
    if (!d || !d->q || !d->bank_k || !d->bank_k_lp || !d->bank_len || !d->rowscale || !d->qnorm || !d->colscale) return VFN_ERR_ARG;
    if (!d->part_x3 || !d->part_f32 || !d->ulist || !d->ucount || !d->work_counter || !d->match_idx || !d->match_corr) return VFN_ERR_ARG;
    if (d->nsplit < 1 || d->nsplit_fb < 1 || d->HW < 1 || d->obj_n < 1 || d->ldq % 4 || d->stride_rs % 4) return VFN_ERR_ARG;
    static const bool ready = [] {
        allow_lds(bank_scan_kernel<2, 2>, SCAN_LDS); allow_lds(bank_scan_kernel<1, 0, true>, SCAN_LDS);
        return true;
    }();
    (void)ready;
    hipStream_t s = (hipStream_t)stream;
    vfn_bankscan_desc sd = {};
    sd.q = d->q; sd.bank_k = d->bank_k; sd.bank_len = d->bank_len; sd.rowscale = d->rowscale;
    sd.stride_q = d->stride_q; sd.stride_k = d->stride_k; sd.stride_rs = d->stride_rs;
    sd.scale = 1.f; sd.ldq = d->ldq; sd.q_per_obj = 1; sd.HW = d->HW; sd.obj_n = d->obj_n;
    sd.work_counter = d->work_counter; sd.bank_k_lp = d->bank_k_lp;
    // 1. bf16x3 scores: best / entry / runner-up per (slice, column)
    sd.part = d->part_x3; sd.nsplit = d->nsplit; sd.mode = 2; sd.precision = 2;
    const int items = cdiv(d->HW, QTS) * d->nsplit * d->obj_n;
    if (hipMemsetAsync(d->work_counter, 0, sizeof(int), s) != hipSuccess) return VFN_ERR_LAUNCH;
    if (hipMemsetAsync(d->ucount, 0, sizeof(int) * d->obj_n, s) != hipSuccess) return VFN_ERR_LAUNCH;
    hipLaunchKernelGGL((bank_scan_kernel<2, 2>), dim3(items < 512 ? items : 512), dim3(256), SCAN_LDS, s, sd, scan_gather{});
    // 2. certify + exact rescore; the rest onto the list
    hipLaunchKernelGGL(bank_match_certify_kernel, dim3(cdiv(d->HW, 32), d->obj_n), dim3(64), 0, s, *d);
    // 3. the f32 scan over the listed columns (item count read on the device: an empty list is one near-empty launch)
    sd.part = d->part_f32; sd.nsplit = d->nsplit_fb; sd.mode = 1; sd.precision = 0; sd.bank_k_lp = nullptr;
    if (hipMemsetAsync(d->work_counter, 0, sizeof(int), s) != hipSuccess) return VFN_ERR_LAUNCH;
    hipLaunchKernelGGL((bank_scan_kernel<1, 0, true>), dim3(512), dim3(256), SCAN_LDS, s, sd, scan_gather{d->ulist, d->ucount});
    hipLaunchKernelGGL(bank_match_finish_listed_kernel, dim3(cdiv(d->obj_n * d->HW * 8, 256)), dim3(256), 0, s,
                       (const float*)d->part_f32, d->nsplit_fb, d->HW, d->obj_n, (const int*)d->ulist, (const int*)d->ucount,
                       d->match_idx, d->match_corr, d->colscale);
    return vfn_check_launch();
}

extern "C" int vfn_memread_apply(const vfn_memread_desc* d, void* stream) {
    if (!d || !d->q || !d->bank_k || !d->bank_v || !d->bank_len || !d->ml || !d->o_part) return VFN_ERR_ARG;
    if (d->nsplit < 1 || d->ldq % 4) return VFN_ERR_ARG;
    if (d->precision < 0 || d->precision > 2) return VFN_ERR_ARG;
    if (d->scores && !scores_fit(d->stride_scores, d->stride_k, d->HW)) return VFN_ERR_ARG;
    if (d->nsplit_tail < 0 || d->nsplit_tail > d->nsplit) return VFN_ERR_ARG;
    if (d->nsplit_tail && !(d->precision == 0 && d->scores)) return VFN_ERR_ARG;      // only the stored-scores f32 kernel knows it
    constexpr size_t LDS_WF = (size_t)(QTW * DK + CH * DK + QTW * CH) * sizeof(float);                       // 128 KB
    constexpr size_t LDS_SS = (size_t)2 * QTW * CH * sizeof(float);                                          // 64 KB
    constexpr size_t LDS_W1 = (size_t)QTW * DK * 2 + (size_t)CH * DK * 4 + 2 * (size_t)QTW * CH * 2;         // 80 KB
    constexpr size_t LDS_W2 = LDS_W1 + (size_t)QTW * DK * 2;                                                // 112 KB
    // one-time set-up: LDS limits of every kernel this launcher can pick (memread_apply_ss_kernel fits the default limit) and the
    // read-once switches.  VFN_APPLY_XCD=0: linear workgroup order (apply_item).  VFN_APPLY_IMG_BF16=0: plain bf16 reads the f32
    // rows although the bank carries its split image.
    struct setup_t { int status; bool img_bf16; };
    static const setup_t setup = [] {
        allow_lds(memread_apply_wide_kernel, LDS_WF);
        allow_lds(memread_apply_lpw_kernel<false>, LDS_W1); allow_lds(memread_apply_lpw_kernel<true>, LDS_W2);
        allow_lds(memread_apply_shw_kernel<false>, LDS_W1); allow_lds(memread_apply_shw_kernel<true>, LDS_W2);
        allow_lds(memread_apply_pipe_kernel, APPLY_PIPE_LDS);
        const int lin = env_int("VFN_APPLY_XCD", 1) == 0 ? 1 : 0;
        const bool ok = !lin || hipMemcpyToSymbol(HIP_SYMBOL(vfn_apply_linear_order), &lin, sizeof(int)) == hipSuccess;
        return setup_t{ok ? VFN_OK : VFN_ERR_LAUNCH, env_int("VFN_APPLY_IMG_BF16", 1) != 0};
    }();
    if (setup.status != VFN_OK) return setup.status;

    // precision, image present, pipe switch -> kernel, LDS bytes
    //   f32            scores stored by the scan ? ss : wide
    //   bf16x3         split image ? shw<true> : lpw<true>
    //   bf16           split image ? (VFN_APPLY_PIPE, read at every call: A/B in one process) ? pipe : shw<false>
    //                              : lpw<false>
    // The kept split image: keys land in LDS as the operand image, value operands come straight from the 8-row-blocked image
    // (bank.hip) -- in plain bf16 only its hi plane is read (2 bytes per element instead of the f32 rows' 4).
    const bool image = d->bank_k_lp && d->bank_v_lp && (d->precision == 2 || setup.img_bf16);
    void (*kern)(const vfn_memread_desc);
    size_t lds;
    if (d->precision == 0) {
        if (d->scores) { kern = memread_apply_ss_kernel; lds = LDS_SS; }
        else { kern = memread_apply_wide_kernel; lds = LDS_WF; }
    } else if (d->precision == 2) {
        kern = image ? memread_apply_shw_kernel<true> : memread_apply_lpw_kernel<true>; lds = LDS_W2;
    } else if (!image) {
        kern = memread_apply_lpw_kernel<false>; lds = LDS_W1;
    } else if (env_int("VFN_APPLY_PIPE", 1) != 0) {
        kern = memread_apply_pipe_kernel; lds = APPLY_PIPE_LDS;
    } else {
        kern = memread_apply_shw_kernel<false>; lds = LDS_W1;
    }
    // the last query tile in its own number of slices (memread_apply_ss_kernel only): (qtiles - 1) * nsplit + nsplit_tail items
    const int qtiles = cdiv(d->HW, QTW);
    const dim3 grid(d->nsplit_tail > 0 ? (qtiles - 1) * d->nsplit + d->nsplit_tail : qtiles * d->nsplit, d->obj_n);
    hipLaunchKernelGGL(kern, grid, dim3(512), lds, (hipStream_t)stream, *d);
    return vfn_check_launch();
}

extern "C" int vfn_memread_finish(const vfn_memread_desc* d, void* stream) {
    if (!d || !d->o_part || !d->out || !d->bank_len) return VFN_ERR_ARG;
    if (d->cnt && !d->info) return VFN_ERR_ARG;
    if (d->ld_out % 4 || d->ldqv % 4) return VFN_ERR_ARG;
    if (d->nsplit_tail < 0 || d->nsplit_tail > d->nsplit) return VFN_ERR_ARG;
    const dim3 grid(1024, d->obj_n);
    hipLaunchKernelGGL(memread_finish_kernel, grid, dim3(256), 0, (hipStream_t)stream, *d);
    return vfn_check_launch();
}

#ifdef VFN_CENSUS
extern "C" int vfn_debug_census(unsigned long long* host_out) {
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(vfn_census_buf), sizeof(unsigned long long) * 4096 * 4) == hipSuccess ? 0 : 1;
}
#endif
