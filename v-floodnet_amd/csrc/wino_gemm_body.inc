    // The body of wino_gemm_kernel and wino_gemm_dual_kernel (conv_winograd.hip includes it inside both): the persistent GEMM's unit walk.
    // It names the template parameters BM, BN, WM, WN, PD, the constants CONV, LP, DUAL and the arguments p (wino_gemm_args), q2 (wino_dual_args).
    static_assert(!(CONV && LP), "the reduced-precision form is the transform-domain GEMM only");
    static_assert(CONV || !DUAL, "two sources: the 1x1 convolution form only");
    constexpr int BK = 32;                               // floats per LDS row (128 bytes = 32 f32 / 64 bf16)
    constexpr int KT = LP ? 64 : 32;                     // K elements per tile
    constexpr int ES = LP ? 2 : 4;                       // bytes per operand element
    constexpr int NT = WM * WN * 64;
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int AC = BM * 8 / NT, BC = BN * 8 / NT, RSTEP = NT / 8;
    static_assert(AC >= 1 && BC >= 1, "tile too small for the thread count");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sA = reinterpret_cast<float*>(smem);          // [2][BM][32]
    float* sB = sA + 2 * BM * BK;                        // [2][BN][32]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int li = lane & 31, lh = lane >> 5;

    // units of this workgroup: XCD x (= blockIdx % 8) owns one contiguous run of the unit list (filter tile fastest, then row
    // tile, then component: the workgroups of one XCD share operand tiles through its L2), dealt round-robin to its workgroups
    const int per = p.mtiles * p.ntiles, total = p.comps * per;
    const int gx = (int)gridDim.x >> 3, xcd = (int)blockIdx.x & 7, loc = (int)blockIdx.x >> 3;
    const int q = total >> 3, r8 = total & 7;
    const int u_begin = xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q;
    const int u_end = u_begin + q + (xcd < r8 ? 1 : 0);
    const int first = u_begin + loc;
    const int n_units = first < u_end ? (u_end - first + gx - 1) / gx : 0;
    const int nkA = DUAL ? q2.C / KT : 0;                // (DUAL: K tiles 0 .. nkA - 1 of a unit come from the shortcut source)
    const int nk = p.C / KT + nkA;
    const int T = n_units * nk;
    if (T == 0) return;

    const int c16 = tid & 7, r0 = tid >> 3;
    const int a_ld = CONV ? p.a_ld : p.C;
    const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.V), 0, (int)((size_t)p.comps * p.rows_pad * a_ld * ES), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsU = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.U), 0, (int)((size_t)p.comps * p.cout_pad * p.C * ES), 0x00020000);
    int a_thr[AC], b_thr[BC];
#pragma unroll
    for (int j = 0; j < AC; ++j) a_thr[j] = (r0 + j * RSTEP) * a_ld * ES + c16 * 16;
#pragma unroll
    for (int j = 0; j < BC; ++j) b_thr[j] = (r0 + j * RSTEP) * p.C * ES + c16 * 16;

    // the tile being requested: (unit, K tile) and its operand bases (wave-uniform)
    int lu = 0, lkt = 0, la_base = 0, lb_base = 0;
    // DUAL: the shortcut source's descriptors, this thread's filter rows and -- per unit -- its input rows: output row -> (n, yo, xo)
    // -> pixel (n, stride yo, stride xo); rows at or past M keep an offset past every buffer, so they read zeros
    __amdgpu_buffer_rsrc_t rsV2 = rsV, rsU2 = rsU;
    int a_thr2[AC], b_thr2[BC], lb2_base = 0;
    float rfloor[PD];                                     // ReLU floor of the tile in each staging slot (the sources may differ)
    if constexpr (DUAL) {
        rsV2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(q2.V), 0, (int)((size_t)q2.pix * q2.a_ld * 4), 0x00020000);
        rsU2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(q2.U), 0, (int)((size_t)q2.cout_pad * q2.C * 4), 0x00020000);
#pragma unroll
        for (int j = 0; j < BC; ++j) b_thr2[j] = (r0 + j * RSTEP) * q2.C * 4 + c16 * 16;
    }
    auto unit_dual = [&](int ui) {
        if constexpr (DUAL) {
            const int u = first + ui * gx;
            const int mt = u / p.ntiles, nt = u - mt * p.ntiles;
            lb2_base = nt * BN * q2.C * 4;
            const int hw = q2.Ho * q2.Wo;
#pragma unroll
            for (int j = 0; j < AC; ++j) {
                const int row = mt * BM + r0 + j * RSTEP;
                const int n = row / hw, rem = row - n * hw;
                const int yo = rem / q2.Wo, xo = rem - yo * q2.Wo;
                a_thr2[j] = row < p.rows_pad ? ((n * q2.H + q2.stride * yo) * q2.W + q2.stride * xo) * q2.a_ld * 4 + c16 * 16 : 0x7fffff00;
            }
        }
    };
    int n0_cur = 0;
    auto unit_bases = [&](int ui, int& a_base, int& b_base, size_t& o_base, int* n0 = nullptr) {
        const int u = first + ui * gx;
        const int xi = u / per, rem = u - xi * per;
        const int mt = rem / p.ntiles, nt = rem - mt * p.ntiles;
        a_base = (xi * p.rows_pad + mt * BM) * a_ld * ES;
        b_base = (xi * p.cout_pad + nt * BN) * p.C * ES;
        o_base = CONV ? (size_t)mt * BM : ((size_t)xi * p.rows_pad + mt * BM) * p.Cout + nt * BN;      // (CONV: the first row of the tile)
        if (n0) *n0 = nt * BN;
    };
    size_t o_dummy;
    unit_bases(0, la_base, lb_base, o_dummy);
    if constexpr (DUAL) unit_dual(0);
    f32x4 ra[PD][AC], rb[PD][BC];
    auto request = [&](int slot) {                         // global loads of the next tile in line into staging slot `slot`
        if constexpr (DUAL) {
            // (the phase is wave-uniform: the prefetch runs straight through the phase seam and the unit seam)
            if (lkt < nkA) {
                const int koff = lkt * 128;
#pragma unroll
                for (int j = 0; j < AC; ++j)
                    ra[slot][j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsV2, a_thr2[j], koff, 0));
#pragma unroll
                for (int j = 0; j < BC; ++j)
                    rb[slot][j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsU2, b_thr2[j], lb2_base + koff, 0));
                rfloor[slot] = q2.relu_in ? 0.f : -INFINITY;
            } else {
                const int koff = (lkt - nkA) * 128;
#pragma unroll
                for (int j = 0; j < AC; ++j)
                    ra[slot][j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsV, a_thr[j], la_base + koff, 0));
#pragma unroll
                for (int j = 0; j < BC; ++j)
                    rb[slot][j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsU, b_thr[j], lb_base + koff, 0));
                rfloor[slot] = p.relu_in ? 0.f : -INFINITY;
            }
            if (++lkt == nk) {
                lkt = 0;
                if (++lu < n_units) {
                    unit_bases(lu, la_base, lb_base, o_dummy);
                    unit_dual(lu);
                }
            }
            return;
        }
        const int koff = lkt * 128;                        // (a K tile is 128 bytes of every operand row in either arithmetic)
#pragma unroll
        for (int j = 0; j < AC; ++j)
            ra[slot][j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsV, a_thr[j], la_base + koff, 0));
#pragma unroll
        for (int j = 0; j < BC; ++j)
            rb[slot][j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsU, b_thr[j], lb_base + koff, 0));
        if (++lkt == nk) {
            lkt = 0;
            if (++lu < n_units) unit_bases(lu, la_base, lb_base, o_dummy);
        }
    };
    const float relu_floor = (CONV && p.relu_in) ? 0.f : -INFINITY;
    auto stage = [&](int buf, int slot) {                  // staging slot -> LDS image (XOR-swizzled 16-byte chunks)
        float* dA = sA + buf * BM * BK;
        float* dB = sB + buf * BN * BK;
#pragma unroll
        for (int j = 0; j < AC; ++j) {
            const int r = r0 + j * RSTEP;
            f32x4 v = ra[slot][j];
            if constexpr (CONV) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], DUAL ? rfloor[slot] : relu_floor);
            }
            *reinterpret_cast<f32x4*>(dA + r * BK + ((c16 ^ ((r >> 1) & 7)) << 2)) = v;
        }
#pragma unroll
        for (int j = 0; j < BC; ++j) {
            const int r = r0 + j * RSTEP;
            *reinterpret_cast<f32x4*>(dB + r * BK + ((c16 ^ ((r >> 1) & 7)) << 2)) = rb[slot][j];
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    f32x16 keep[DUAL ? TM : 1][DUAL ? TN : 1];            // DUAL: the shortcut's output of this unit, from the phase seam to the epilogue
    // the unit being multiplied
    int cu = 0, ckt = 0, ca_dummy, cb_dummy;
    size_t o_base;
    unit_bases(0, ca_dummy, cb_dummy, o_base, &n0_cur);

#pragma unroll
    for (int d = 0; d < PD; ++d)
        if (d < T) request(d);
    stage(0, 0);
    __syncthreads();

    for (int t0 = 0; t0 < T; t0 += PD) {
#pragma unroll
        for (int uu = 0; uu < PD; ++uu) {
            const int t = t0 + uu;
            if (t >= T) break;
            const int buf = t & 1;
            const bool more = t + 1 < T;                   // tile t+1 goes to LDS during this tile (from slot (uu + 1) % PD)
            const bool more_req = t + PD < T;              // tile t+PD is requested during this tile (into slot uu, free by now)
            const float* cA = sA + buf * BM * BK + (wm * TM * 32) * BK;
            const float* cB = sB + buf * BN * BK + (wn * TN * 32) * BK;
            auto read_frags = [&](int kk, f32x4 (&a)[TM], f32x4 (&b)[TN]) {
                const int lc = 2 * kk + lh;
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int r = i * 32 + li;
                    a[i] = *reinterpret_cast<const f32x4*>(cA + r * BK + ((lc ^ ((r >> 1) & 7)) << 2));
                }
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int r = j * 32 + li;
                    b[j] = *reinterpret_cast<const f32x4*>(cB + r * BK + ((lc ^ ((r >> 1) & 7)) << 2));
                }
            };
            f32x4 fa[2][TM], fb[2][TN];
            read_frags(0, fa[0], fb[0]);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                if (PD > 1 && kk == 0 && more) stage(buf ^ 1, (uu + 1) % PD);       // (requested a whole tile ago: landed)
                if (kk == 1 && more_req) request(uu);
                if (PD == 1 && kk == 3 && more) stage(buf ^ 1, 0);
                if (kk + 1 < 4) read_frags(kk + 1, fa[(kk + 1) & 1], fb[(kk + 1) & 1]);
                if constexpr (LP) {
                    typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_;
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_, fa[kk & 1][i]), __builtin_bit_cast(bf16x8_, fb[kk & 1][j]),
                                                                                acc[i][j], 0, 0, 0);
                } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[kk & 1][i][e], fb[kk & 1][j][e], acc[i][j], 0, 0, 0);
                }
            }
            if constexpr (DUAL) {
                if (ckt + 1 == nkA) {
                    // the phase seam: the accumulators become the shortcut layer's output -- its epilogue's expression, per lane one
                    // channel -- and start again from zero for the main source
                    const float floor2 = q2.relu_mid ? 0.f : -INFINITY;
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        const int col = n0_cur + (wn * TN + j) * 32 + li;
                        const bool cok = col < p.Cout;
                        const float sc = (q2.scale && cok) ? q2.scale[col] : 1.f;
                        const float sh = (q2.shift && cok) ? q2.shift[col] : 0.f;
#pragma unroll
                        for (int i = 0; i < TM; ++i)
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                keep[i][j][r] = vfn_floor_nan(acc[i][j][r] * sc + sh, floor2);
                                acc[i][j][r] = 0.f;
                            }
                    }
                }
            }
            if (++ckt == nk) {
                // the unit is complete: lane = filter column (lane & 31), registers = rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
                if constexpr (CONV) {
                    // y = act(acc * scale[c] + shift[c] + res): lane = channel, so scale / shift are one value per lane and column tile;
                    // the residual taps of the whole tile are requested first (buffer loads: rows past M / columns past Cout return
                    // zeros), the stores of invalid positions are dropped by the hardware
                    const int m0 = (int)o_base;
                    const int npix = p.rows_pad;
                    const __amdgpu_buffer_rsrc_t rso = __builtin_amdgcn_make_buffer_rsrc(p.Mb, 0, (int)((size_t)npix * p.out_ld * 4), 0x00020000);
                    const __amdgpu_buffer_rsrc_t rsr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.res ? p.res : p.V), 0,
                        p.res ? (int)((size_t)(p.res_mod > 0 ? p.res_mod : npix) * p.res_ld * 4) : 0, 0x00020000);
                    const float floor_ = p.relu_out ? 0.f : -INFINITY;
                    float rv[TM][TN][16];
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        if constexpr (DUAL) break;         // (the residual is in `keep`)
                        const int col = n0_cur + (wn * TN + j) * 32 + li;
#pragma unroll
                        for (int i = 0; i < TM; ++i)
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                const int row = m0 + (wm * TM + i) * 32 + 4 * lh + (r & 3) + 8 * (r >> 2);
                                const int rrow = p.res_mod > 0 ? row % p.res_mod : row;
                                rv[i][j][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                    rsr, (row < npix && col < p.Cout) ? (rrow * p.res_ld + col) * 4 : 0x7ffffff0, 0, 0));
                            }
                    }
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        const int col = n0_cur + (wn * TN + j) * 32 + li;
                        const bool cok = col < p.Cout;
                        const float sc = (p.scale && cok) ? p.scale[col] : 1.f;
                        const float sh = (p.shift && cok) ? p.shift[col] : 0.f;
#pragma unroll
                        for (int i = 0; i < TM; ++i)
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                const int row = m0 + (wm * TM + i) * 32 + 4 * lh + (r & 3) + 8 * (r >> 2);
                                float res_v;
                                if constexpr (DUAL) res_v = keep[i][j][r]; else res_v = rv[i][j][r];
                                const float v = vfn_floor_nan(acc[i][j][r] * sc + sh + res_v, floor_);
                                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rso,
                                                                      (row < npix && cok) ? (row * p.out_ld + col) * 4 : 0x7ffffff0, 0, 0);
                                acc[i][j][r] = 0.f;
                            }
                    }
                } else {
                float* o = p.Mb + o_base;
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int col = (wn * TN + j) * 32 + li;
#pragma unroll
                    for (int i = 0; i < TM; ++i) {
                        const int rbase = (wm * TM + i) * 32 + 4 * lh;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            if (n0_cur + col < p.Cout)
                                o[(size_t)(rbase + (r & 3) + 8 * (r >> 2)) * p.Cout + col] = acc[i][j][r];
                            acc[i][j][r] = 0.f;
                        }
                    }
                }
                }
                ckt = 0;
                if (++cu < n_units) unit_bases(cu, ca_dummy, cb_dummy, o_base, &n0_cur);
            }
            __syncthreads();
        }
    }
