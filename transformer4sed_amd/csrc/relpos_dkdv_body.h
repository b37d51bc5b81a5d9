// Body of the score-recomputing dK / dV kernel (relpos_attention.hip, backward kernel 1), included once into the unbanded kernel --
// whose code and register allocation (at the 256-VGPR limit) thereby stay exactly what they were -- and once into the body template
// of the band kernel.  Expects in scope: the kernel parameters, the four workgroup arrays lds / lds_band / lds_g / lstat,
// `BAND` (compile-time bool) and `hw` (the head's half width; unused without BAND).
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, lg = lane >> 5;
    const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
    const int J0 = blockIdx.x * 128, key0 = J0 + wave * 32;
    const int R = 2 * T - 1;
    const size_t hb = (size_t)bh * T * HD, hbt = (size_t)bh * HD * Tpad;
    const bf16_t* Ph = P + (size_t)h * Rpad * HD;
    int krow = key0 + lr;
    const bool key_valid_lane = krow < T;
    krow = krow < T ? krow : T - 1;
    s16x8_t kf[4], vf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        kf[s] = *reinterpret_cast<const s16x8_t*>(K + hb + (size_t)krow * HD + 16 * s + 8 * lg);
        vf[s] = *reinterpret_cast<const s16x8_t*>(V + hb + (size_t)krow * HD + 16 * s + 8 * lg);
    }
    f32x16_t dk[2], dv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk[i][r] = 0.f; dv[i][r] = 0.f; }
    float* gs = lds_g[wave];
    const int ntiles = (T + 63) / 64;
    const int t_lo = BAND ? max(J0 - hw + 1, 0) >> 6 : 0;
    const int t_hi = BAND ? min(J0 + 127 + hw, T - 1) >> 6 : ntiles - 1;
    // next tile's operands travel HBM -> registers while the current tile is being consumed, registers -> LDS afterwards
    TileRegs r0, r1, r2, r3, r4;
    BandRegs rb;
    float rstat = 0.f;
    auto gload = [&](int t) {
        const int i0 = t * 64;
        tile_gload(r0, Qu + hb, i0, T, HD, 0, tid);
        tile_gload(r1, Qv + hb, i0, T, HD, 0, tid);
        tile_gload(r2, dOh + hb, i0, T, HD, 0, tid);
        tile_gload(r3, Qut + hbt, 0, HD, Tpad, i0, tid);
        tile_gload(r4, dOt + hbt, 0, HD, Tpad, i0, tid);
        band_gload(rb, Ph, J0 - (i0 + 63) + T - 1, R, tid);
        if (tid < 128) {
            const int qi = i0 + (tid & 63);
            const float* src = (tid < 64) ? LSE : Dv;
            rstat = qi < T ? src[(size_t)bh * T + qi] : (tid < 64 ? 1e30f : 0.f);  // L2 = +big -> P = 0 for padded queries
        }
    };
    auto lstore = [&]() {
        tile_lstore_rows(r0, lds[0], tid);
        tile_lstore_rows(r1, lds[1], tid);
        tile_lstore_rows(r2, lds[2], tid);
        tile_lstore_cols(r3, lds[3], tid);
        tile_lstore_cols(r4, lds[4], tid);
        band_lstore(rb, lds_band, tid);
        if (tid < 128) lstat[tid >> 6][tid & 63] = rstat;
    };
    gload(t_lo);
    lstore();
    __syncthreads();
    for (int t = t_lo; t <= t_hi; ++t) {
        if (t < t_hi) gload(t + 1);
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            const int rowoff = 32 * (wave - qb + 1);
            // BAND: does this (32-query x 32-key) block reach past the band (wave-uniform)?  A full window never does.
            const int dmin = key0 - (t * 64 + 32 * qb + 31);
            const bool edge = BAND && !(dmin >= -hw && dmin + 62 < hw);
            // band product G[i, rho] (rows = queries, column = rho): A = Qv rows, B = band rows
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) {
                f32x16_t g;
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    g = mfma32t<SF16>(lds_frag_rows(lds[1], 32 * qb + lr, 2 * s + lg),
                                      lds_frag_rows(lds_band, rowoff + 32 * blk + lr, 2 * s + lg), s == 0 ? zero16 : g);
#pragma unroll
                for (int r = 0; r < 16; ++r) gs[mfma32_row(r, lg) * 65 + 32 * blk + lr] = g[r];
            }
            f32x16_t s_, dp;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                s_ = mfma32t<SF16>(lds_frag_rows(lds[0], 32 * qb + lr, 2 * s + lg), kf[s], s == 0 ? zero16 : s_);
                dp = mfma32(lds_frag_rows(lds[2], 32 * qb + lr, 2 * s + lg), vf[s], s == 0 ? zero16 : dp);
            }
            __syncthreads();
            // (a lane whose key is >= T needs no masking: its columns only feed dK / dV rows that are never stored)
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {
                const int qq = 32 * qb + 8 * qd + 4 * lg;
                const f32x4_t l2 = *reinterpret_cast<const f32x4_t*>(&lstat[0][qq]);
                const f32x4_t dd = *reinterpret_cast<const f32x4_t*>(&lstat[1][qq]);
#pragma unroll
                for (int j = 0; j < 4; j += 2) {
                    const int r = 4 * qd + j, ii = mfma32_row(r, lg);
                    const f32x2_t bd = {gs[ii * 65 + lr - ii + 31], gs[(ii + 1) * 65 + lr - ii + 30]};
                    const f32x2_t c2 = {SCALE_LOG2E, SCALE_LOG2E}, nl = {-l2[j], -l2[j + 1]}, nd = {-dd[j], -dd[j + 1]};
                    f32x2_t x = {s_[r], s_[r + 1]}, d2 = {dp[r], dp[r + 1]};
                    x = __builtin_elementwise_fma(x + bd, c2, nl);
                    f32x2_t pv = {__builtin_amdgcn_exp2f(x.x), __builtin_amdgcn_exp2f(x.y)};
                    if (BAND && edge) {   // key - query of the pair (ii, lr); ii + 1 is the next query
                        const int dj = key0 + lr - (t * 64 + 32 * qb + ii);
                        pv.x = (dj >= -hw && dj < hw) ? pv.x : 0.f;
                        pv.y = (dj - 1 >= -hw && dj - 1 < hw) ? pv.y : 0.f;
                    }
                    d2 = pv * (d2 + nd);
                    s_[r] = pv.x; s_[r + 1] = pv.y;
                    dp[r] = d2.x; dp[r + 1] = d2.y;
                }
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const s16x8_t pf = pack_frag(s_, s), dsf = pack_frag(dp, s);
#pragma unroll
                for (int db = 0; db < 2; ++db) {
                    dv[db] = mfma32(pf, lds_frag_cols(lds[4], 32 * db + lr, 8 * qb + 4 * s + lg), dv[db]);
                    dk[db] = mfma32(dsf, lds_frag_cols(lds[3], 32 * db + lr, 8 * qb + 4 * s + lg), dk[db]);
                }
            }
            __syncthreads();
        }
        if (t < t_hi) {
            lstore();
            __syncthreads();
        }
    }
    const int ldq = 3 * H * HD;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = key0 + mfma32_row(r, lg);
            if (key < T) {
                bf16_t* row = dqkv + ((size_t)b * T + key) * ldq + h * HD + 32 * db + lr;
                row[H * HD] = f2bf(dk[db][r] * SCALE);
                row[2 * H * HD] = f2bf(dv[db][r]);
            }
        }
