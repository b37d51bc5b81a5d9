// Epilogues of the 256^2 NT kernel (gemm.hip: gemm_nt_pp_kernel), device code only: the column orders the B operand's DMA sets up for
// them, the 16-bit sinks and the one row walker (pp_rows16) behind every pp_stage16* form, the byte-plane helpers, the staged fp32
// path (V3Side, v3_side_load, v3_store_batch), the three epilogues that store straight from the accumulators (*_direct), the variant
// table (PP_* / PpTraits) and pp_epilogue, which picks among all of these at compile time.
#pragma once
#include "gemm_args.h"

// LDS row (within the B stage) -> weight row of the tile, PP_COL order (gemm_args.h)
__device__ __forceinline__ int pp_brow_src(int row) { return (row & ~0x1C) | ((row & 0x10) >> 2) | ((row & 0x0C) << 1); }
// Column order of the kernel variants whose epilogue stores fp32 straight from the accumulators (EPI_F32, the plain EPI_F32_RESID):
// block j, lane group lq -> columns 32 (j & 1) + 16 (j >> 1) + 4 lq .. + 3.  After the lane-pair swap (pp_pair_swap32) a lane holds, of
// one row, blocks 2 hk and 2 hk + 1 (hk = l15 >> 3): float4 number 4 hk + lq of the row's first and of its second 128 bytes -- each of the
// two 16-byte stores (or residual loads) per row is then 8 lanes x 16 B = 128 contiguous bytes, 8 rows per instruction.
__device__ __forceinline__ constexpr int PP_COL32(int j, int lq) { return 32 * (j & 1) + 16 * (j >> 1) + 4 * lq; }
__device__ __forceinline__ int pp_brow_src32(int row) { return (row & ~0x30) | ((row & 0x10) << 1) | ((row & 0x20) >> 1); }
// Per-lane column constants (bias, plus the rel-pos u / v vector for the q projection) for the 16 columns a lane owns: fetched ONCE,
// before any store -- the output pointers may alias them as far as the compiler knows, so a load placed between stores costs a full
// `s_waitcnt vmcnt(0)` round trip each time (measured: 8 us / tile).
__device__ __forceinline__ void pp_col_consts(float (&bv)[4][4], const float* bias_n, const float* extra, int lq) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = PP_COL(j, lq);
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (bias_n != nullptr) b = *reinterpret_cast<const float4*>(bias_n + col);
        if (extra != nullptr) {
            const float4 x = *reinterpret_cast<const float4*>(extra + col);
            b.x += x.x; b.y += x.y; b.z += x.z; b.w += x.w;
        }
        bv[j][0] = b.x; bv[j][1] = b.y; bv[j][2] = b.z; bv[j][3] = b.w;
    }
}

// Row-group bias of a wave's 128-row sub-tile (rows mb .. mb + 127): with gb_rows >= 128 it touches at most two groups; rows below
// `bnd` (relative to mb) belong to the first, the rest to the second.
__device__ __forceinline__ int gb_split(const GemmArgs& g, int mb, const float*& rowA, const float*& rowB) {
    const int last = g.M / g.gb_rows - 1;
    int gA = mb / g.gb_rows;
    gA = gA < last ? gA : last;
    const int gB = gA < last ? gA + 1 : last;
    rowA = g.gbias + (size_t)gA * g.N;
    rowB = g.gbias + (size_t)gB * g.N;
    return (gA + 1) * g.gb_rows - mb;
}
// ---- 16-bit epilogue sinks: where a lane's 8 consecutive 16-bit outputs of row block i, column half k (PP_COL order: columns
// 32 k + 8 lq .. + 7 of the wave's 64) go.  Global sinks store 16 bytes per lane straight from the accumulators; the LDS sink keeps
// the staged form for the head-split variants that also write transposed copies.
// A store instruction of 64 lanes x 16 B should cover 8 rows x 128 contiguous bytes (for the head-split q / k / v a wave's 128 token rows
// of one head are ONE contiguous 16 KB run), not 16 rows x 64: lanes l15 and l15 ^ 8 of a 16-lane DPP row swap one half each
// (`row_ror:8`), after which lanes l15 < 8 hold the low 64 bytes and lanes l15 >= 8 the high 64 bytes of rows 16 i + (l15 & 7)
// (first store) and 16 i + 8 + (l15 & 7) (second store).  12 VALU operations per 16-row block instead of the LDS round trip.
__device__ __forceinline__ unsigned pp_ror8(unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, true);      // row_ror:8
}
__device__ __forceinline__ void pp_pair_swap(uint4& a0, uint4& a1, bool lo) {
    // in: a0 / a1 = this lane's row, column halves 0 / 1.  out: a0 = (row l15 & 7, half l15 >> 3), a1 = (row 8 + (l15 & 7), half l15 >> 3)
    // (component-wise selects: a conditional between the two structs becomes a pointer select into scratch memory)
    const unsigned rx = pp_ror8(lo ? a1.x : a0.x), ry = pp_ror8(lo ? a1.y : a0.y), rz = pp_ror8(lo ? a1.z : a0.z), rw = pp_ror8(lo ? a1.w : a0.w);
    a0 = make_uint4(lo ? a0.x : rx, lo ? a0.y : ry, lo ? a0.z : rz, lo ? a0.w : rw);
    a1 = make_uint4(lo ? rx : a1.x, lo ? ry : a1.y, lo ? rz : a1.z, lo ? rw : a1.w);
}
struct PPSinkLds {
    unsigned char* wl; int l15, lq;
    __device__ __forceinline__ void half(int i, int k, const uint4& v) const {
        unsigned char* d = wl + (i * 16 + l15) * V3_RS16 + (32 * k + 8 * lq) * 2;      // (136-byte rows: two 8-byte writes)
        *reinterpret_cast<uint2*>(d) = make_uint2(v.x, v.y);
        *reinterpret_cast<uint2*>(d + 8) = make_uint2(v.z, v.w);
    }
    __device__ __forceinline__ void row(int i, const uint4& a0, const uint4& a1) const { half(i, 0, a0); half(i, 1, a1); }
};
template <bool TAIL = false>
struct PPSinkRowsT {         // row-major [M][ldc] output
    bf16_t* base;            // row mb + (l15 & 7), column nb + 32 (l15 >> 3) + 8 lq
    bf16_t* hbase;           // row mb + l15, column nb + 8 lq   (un-swapped halves)
    int ld8;                 // 8 * ldc
    int mrem, hrem;          // rows left from base's / hbase's row
    bool lo;
    // TAIL (F8 kernels): rows are [N f16 | N e4m3] and `tail` > 0 is the byte distance from a lane's 8 f16 outputs to their 8 e4m3 images
    // (GemmArgs.out_e4m3: the next GEMM's A operand with both halves written here); 0 = no image.  What the image costs is its bytes
    // (+50 % on the epilogue's writes: 70 us of 510 at M = 105 k, N = 3072), not its conversion: with MODE.FP16_OVFL = 1 the conversion
    // saturates by itself (tools/ablate/cvt_fp8_probe.hip) and the packed clamps can go -- 4 instructions instead of 12 per 8 values --
    // for no measurable change (726 vs 723 us).
    int tail;
    __device__ __forceinline__ void st16(bf16_t* p, const uint4& v) const {
        v3_st<uint4>(p, v);
        if constexpr (TAIL) {
#ifndef ABL_NO_TAIL      // (timing ablation, tools/ablate/build_variant.sh)
            if (tail > 0) v3_st<uint2>(reinterpret_cast<unsigned char*>(p) + tail, make_uint2(e4m3x4_of_h4(v.x, v.y), e4m3x4_of_h4(v.z, v.w)));
#endif
        }
    }
    __device__ __forceinline__ void half(int i, int k, const uint4& v) const {
        if (16 * i < hrem) v3_st<uint4>(hbase + (size_t)(2 * i) * ld8 + 32 * k, v);
    }
    __device__ __forceinline__ void row(int i, uint4 a0, uint4 a1) const {
        pp_pair_swap(a0, a1, lo);
        if (16 * i < mrem) st16(base + (size_t)(2 * i) * ld8, a0);
        if (16 * i + 8 < mrem) st16(base + (size_t)(2 * i + 1) * ld8, a1);
    }
};
typedef PPSinkRowsT<false> PPSinkRows;
struct PPSinkHeads {         // head-split q / k / v: [clip * heads + h][seq][64]
    bf16_t* dst;             // + h * seq * 64 + 32 (l15 >> 3) + 8 lq already applied
    int b0, t0, seq, hs, mrem;   // clip / token of row mb + (l15 & 7); hs = heads * seq; rows left from there
    bool lo;
    __device__ __forceinline__ void st(int r, const uint4& v) const {      // r = row offset from this lane's first row (a multiple of 8)
        if (r >= mrem) return;
        int t = t0 + r, b = b0;
        if (seq >= 128) { if (t >= seq) { t -= seq; ++b; } }
        else { const int q = t / seq; t -= q * seq; b += q; }
        v3_st<uint4>(dst + ((size_t)b * hs + t) * 64, v);
    }
    __device__ __forceinline__ void row(int i, uint4 a0, uint4 a1) const {
        pp_pair_swap(a0, a1, lo);
        st(16 * i, a0);
        st(16 * i + 8, a1);
    }
};
template <bool F16, int MODE>
__device__ __forceinline__ uint4 pp_pack8(f32x2v a0, f32x2v a1, f32x2v b0, f32x2v b1) {
    if (MODE == 1) { a0 = gelu_fast2(a0); a1 = gelu_fast2(a1); b0 = gelu_fast2(b0); b1 = gelu_fast2(b1); }
    return make_uint4(pack2<F16>(a0.x, a0.y), pack2<F16>(a1.x, a1.y), pack2<F16>(b0.x, b0.y), pack2<F16>(b1.x, b1.y));
}
// The row loop of the 16-bit epilogues: RB row blocks i x two column halves k x the two column blocks j = 2 k, 2 k + 1 of a half; a half is
// a lane's 8 consecutive 16-bit outputs and both halves of a row block go to the sink together.  pp_stage16, pp_stage16_gb and
// pp_stage16_ln differ only in the value they make of an accumulator: xf(i, j, c, acc) is the output for acc[i][j][c].  MODE 0: that
// value; 1: gelu_fast of it.  (One function on purpose: with the half as a helper of its own, shared with pp_stage16_gb_k, the compiler
// schedules the row-group-bias kernels differently -- same arithmetic, other instruction order.)
template <bool F16, int MODE, int RB, class Sink, class XF>
__device__ __forceinline__ void pp_rows16(const Sink& sink, const f32x4_t (&acc)[8][4], XF xf) {
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        uint4 o[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            f32x2v x[2][2];
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                const int j = 2 * k + jj;
                x[jj][0] = f32x2v{xf(i, j, 0, acc), xf(i, j, 1, acc)};
                x[jj][1] = f32x2v{xf(i, j, 2, acc), xf(i, j, 3, acc)};
            }
            o[k] = pp_pack8<F16, MODE>(x[0][0], x[0][1], x[1][0], x[1][1]);
        }
        sink.row(i, o[0], o[1]);
    }
}

// per-row choice between two sets of column constants (bv + group-bias row A for rows < bnd, + row B otherwise), kept as
// base = bv + A and delta = B - A (32 registers, as many as one 32-column half of both sets used to take): all four column blocks of a
// row block are then at hand together and the row leaves through the pair-swapped whole-row stores like every other 16-bit epilogue
template <bool F16, int MODE, class Sink>
__device__ __forceinline__ void pp_stage16_gb(const Sink& sink, const f32x4_t (&acc)[8][4], const float (&bv)[4][4], const float* rowA,
                                              const float* rowB, int bnd, int l15, int lq) {
    float base[4][4], delta[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4 a4 = *reinterpret_cast<const float4*>(rowA + PP_COL(j, lq)), b4 = *reinterpret_cast<const float4*>(rowB + PP_COL(j, lq));
        base[j][0] = bv[j][0] + a4.x; base[j][1] = bv[j][1] + a4.y; base[j][2] = bv[j][2] + a4.z; base[j][3] = bv[j][3] + a4.w;
        delta[j][0] = b4.x - a4.x; delta[j][1] = b4.y - a4.y; delta[j][2] = b4.z - a4.z; delta[j][3] = b4.w - a4.w;
    }
    pp_rows16<F16, MODE, 8>(sink, acc, [&](int i, int j, int c, const f32x4_t (&acc)[8][4]) {
        const bool second = i * 16 + l15 >= bnd;
        return acc[i][j][c] + base[j][c] + (second ? delta[j][c] : 0.f);
    });
}

// (the head-split epilogue's form: column constants per 32-column half -- 16 registers live at a time, it has none to spare -- halves
//  handed to the sink one at a time: k outside i, so it keeps a loop of its own beside pp_rows16)
template <bool F16, int MODE, class Sink>
__device__ __forceinline__ void pp_stage16_gb_k(const Sink& sink, const f32x4_t (&acc)[8][4], const float (&bv)[4][4], const float* rowA,
                                                const float* rowB, int bnd, int l15, int lq) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        float cA[2][4], cB[2][4];
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int j = 2 * k + jj;
            const float4 a4 = *reinterpret_cast<const float4*>(rowA + PP_COL(j, lq)), b4 = *reinterpret_cast<const float4*>(rowB + PP_COL(j, lq));
            cA[jj][0] = bv[j][0] + a4.x; cA[jj][1] = bv[j][1] + a4.y; cA[jj][2] = bv[j][2] + a4.z; cA[jj][3] = bv[j][3] + a4.w;
            cB[jj][0] = bv[j][0] + b4.x; cB[jj][1] = bv[j][1] + b4.y; cB[jj][2] = bv[j][2] + b4.z; cB[jj][3] = bv[j][3] + b4.w;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bool second = i * 16 + l15 >= bnd;
            f32x2v x[2][2];
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                const f32x4_t& a = acc[i][2 * k + jj];
                x[jj][0] = f32x2v{a[0] + (second ? cB[jj][0] : cA[jj][0]), a[1] + (second ? cB[jj][1] : cA[jj][1])};
                x[jj][1] = f32x2v{a[2] + (second ? cB[jj][2] : cA[jj][2]), a[3] + (second ? cB[jj][3] : cA[jj][3])};
            }
            sink.half(i, k, pp_pack8<F16, MODE>(x[0][0], x[0][1], x[1][0], x[1][1]));
        }
    }
}

// LayerNorm-folded form: x = rstd[row] * (acc - mean[row] * sv[col]) + bv[col]  (rows mb + 16 i + l15, statistics clipped to the last row)
// (BVP: the column constants are fetched per 32-column half from `bias_n` instead of living in 16 registers -- the head-split epilogue
//  has no room for them beside the accumulators)
template <bool F16, int MODE, bool BVP = false, int RB = 8, class Sink>
__device__ __forceinline__ void pp_stage16_ln(const Sink& sink, const f32x4_t (&acc)[8][4], const float (&bv)[4][4], const float* colS_n,
                                              const float* rowstat, int mb, int M, int l15, int lq, const float* bias_n = nullptr) {
    // every global load of the epilogue is issued up front (8 row statistics, the column vectors): one exposed round trip instead of
    // one per column block -- the K loop's fragment registers are free by now
    float2 st[8];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        const int m = mb + i * 16 + l15;
        st[i] = *reinterpret_cast<const float2*>(rowstat + 2 * (size_t)(m < M ? m : M - 1));
    }
    float sn[4][4], bn[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4 s = *reinterpret_cast<const float4*>(colS_n + PP_COL(j, lq));
        sn[j][0] = s.x; sn[j][1] = s.y; sn[j][2] = s.z; sn[j][3] = s.w;
        if constexpr (BVP) {
            const float4 b = *reinterpret_cast<const float4*>(bias_n + PP_COL(j, lq));
            bn[j][0] = b.x; bn[j][1] = b.y; bn[j][2] = b.z; bn[j][3] = b.w;
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) bn[j][c] = bv[j][c];
        }
    }
    pp_rows16<F16, MODE, RB>(sink, acc, [&](int i, int j, int c, const f32x4_t (&acc)[8][4]) {
        const float rs = st[i].y, tm = -st[i].x * st[i].y;
        return __builtin_fmaf(acc[i][j][c], rs, __builtin_fmaf(tm, sn[j][c], bn[j][c]));
    });
}

// mode 0: acc + column constant   1: gelu_fast(acc + column constant)
template <bool F16, int MODE, int RB = 8, class Sink>
__device__ __forceinline__ void pp_stage16(const Sink& sink, const f32x4_t (&acc)[8][4], const float (&bv)[4][4]) {
    pp_rows16<F16, MODE, RB>(sink, acc, [&](int i, int j, int c, const f32x4_t (&acc)[8][4]) { return acc[i][j][c] + bv[j][c]; });
}
// Byte plane layout: slab-major [N / 64][M][64] -- the 64 bytes of row m in 64-column slab s sit at (s * M + m) * 64, so a wave's
// 128 rows x 64 columns are ONE contiguous 8 KB run (row-major they are 128 pieces of 64 bytes, 768 bytes apart).  Only the producers
// touch this plane, so the layout is theirs to choose.
__device__ __forceinline__ size_t lo8_off(const GemmArgs& g, int m, int n) { return ((size_t)(n >> 6) * g.M + m) * 64 + (n & 63); }
// element offset of (m, n) in a plane of the producer: slab-major with the byte lo plane (GemmArgs.lo8), row-major otherwise
__device__ __forceinline__ size_t hi_off(const GemmArgs& g, int m, int n) { return g.lo8 ? lo8_off(g, m, n) : (size_t)m * g.ldc + n; }
// 8-bit lo plane of the split residual stream (GemmArgs.lo8): x = hi + (q - 128) * hi * 2^-18 = hi * (1 + (q - 128) 2^-18)
__device__ __forceinline__ float lo8_decode(float hf, unsigned q) {
    return __builtin_fmaf(__builtin_fmaf((float)q, 0x1p-18f, -0x1p-11f), hf, hf);
}
__device__ __forceinline__ unsigned lo8_encode4(float x0, float x1, float x2, float x3, unsigned pk0, unsigned pk1) {
    // (hi = 0: the quotient is inf / NaN and the byte arbitrary -- the decoder multiplies it by |hi| = 0)
    const float h0 = h2f((bf16_t)(pk0 & 0xFFFF)), h1 = h2f((bf16_t)(pk0 >> 16)), h2 = h2f((bf16_t)(pk1 & 0xFFFF)), h3 = h2f((bf16_t)(pk1 >> 16));
    const float q0 = __builtin_rintf(__builtin_fmaf((x0 - h0) * __builtin_amdgcn_rcpf(h0), 0x1p18f, 128.f));
    const float q1 = __builtin_rintf(__builtin_fmaf((x1 - h1) * __builtin_amdgcn_rcpf(h1), 0x1p18f, 128.f));
    const float q2 = __builtin_rintf(__builtin_fmaf((x2 - h2) * __builtin_amdgcn_rcpf(h2), 0x1p18f, 128.f));
    const float q3 = __builtin_rintf(__builtin_fmaf((x3 - h3) * __builtin_amdgcn_rcpf(h3), 0x1p18f, 128.f));
    unsigned r = __builtin_amdgcn_cvt_pk_u8_f32(q0, 0, 0);      // saturating float -> byte, inserted at byte 0..3
    r = __builtin_amdgcn_cvt_pk_u8_f32(q1, 1, r);
    r = __builtin_amdgcn_cvt_pk_u8_f32(q2, 2, r);
    return __builtin_amdgcn_cvt_pk_u8_f32(q3, 3, r);
}

// Side input of one batch (8 rows per lane, rows m0 + 4 u + lane/16): residual rows (fp32) or saved pre-activations (16-bit)
template <int EPI>
struct V3Side {
    float4 r[EPI == EPI_F32_RESID ? 8 : 1];
    uint2 a[EPI == EPI_DGELU ? 8 : 1];
};
// SM (side mode of the LayerNorm-fold producer): 0 = not a producer, 1 = fp32 residual, 2 = f16 hi + f16 lo planes, 3 = f16 hi + byte lo.
// A compile-time mode (part of the kernel variant, PpTraits::side_mode): with the three load forms as run-time branches of one function
// their results meet in register copies right behind the loads, and every batch waits for its own round trip.
template <int EPI, int SM = 0>
__device__ __forceinline__ void v3_side_load(V3Side<EPI>& sd, const GemmArgs& g, int m0, int n, int lane) {
#ifdef ABL_NO_SIDE
    if constexpr (SM >= 2) return;
#endif
    if constexpr (EPI == EPI_F32_RESID || EPI == EPI_DGELU) {
        if constexpr (SM >= 2) {
            // split-plane residual: the RAW plane words are parked in sd.r and decoded where they are used (v3_residual) -- arithmetic
            // on a loaded value right here makes the compiler wait for every row's loads before it issues the next row's (8 exposed
            // round trips per batch: what the "HBM-saturated" 30 us producer epilogue of rounds 3-4 really was)
            if constexpr (SM == 3) {      // f16 hi + byte lo
                const unsigned char* lo8p = reinterpret_cast<const unsigned char*>(g.res_lo);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int m = m0 + u * 4 + (lane >> 4);
                    const size_t o = (size_t)(m < g.M ? m : g.M - 1) * g.ldc + n;
                    const u32x2_t h = __builtin_nontemporal_load(reinterpret_cast<const u32x2_t*>(g.auxH + lo8_off(g, m < g.M ? m : g.M - 1, n)));
                    const unsigned l = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(lo8p + lo8_off(g, m < g.M ? m : g.M - 1, n)));
                    sd.r[u] = make_float4(__uint_as_float(h[0]), __uint_as_float(h[1]), __uint_as_float(l), 0.f);
                }
                return;
            }
            if constexpr (SM == 2) {      // f16 hi + f16 lo
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int m = m0 + u * 4 + (lane >> 4);
                    const size_t o = (size_t)(m < g.M ? m : g.M - 1) * g.ldc + n;
                    const u32x2_t h = __builtin_nontemporal_load(reinterpret_cast<const u32x2_t*>(g.auxH + o));
                    const u32x2_t l = __builtin_nontemporal_load(reinterpret_cast<const u32x2_t*>(g.res_lo + o));
                    sd.r[u] = make_float4(__uint_as_float(h[0]), __uint_as_float(h[1]), __uint_as_float(l[0]), __uint_as_float(l[1]));
                }
                return;
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int m = m0 + u * 4 + (lane >> 4);
            const size_t o = (size_t)(m < g.M ? m : g.M - 1) * g.ldc + n;
            // read-once side inputs: non-temporal, like the tile stores
            if constexpr (EPI == EPI_F32_RESID) {
                const f32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(g.resF + o));
                sd.r[u] = make_float4(v[0], v[1], v[2], v[3]);
            } else {
                const u32x2_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x2_t*>(g.auxH + o));
                sd.a[u] = make_uint2(v[0], v[1]);
            }
        }
    }
}
// rows m0 .. m0 + 31 of the output = staged rows srow0 .. srow0 + 31
// 16-lane (one staged row) sum through DPP: quad butterflies, then the two mirrors
__device__ __forceinline__ float row16_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));   // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));   // row_mirror
    return v;
}
template <int EPI, bool F16, int SM = 0>
__device__ __forceinline__ void v3_store_batch(const GemmArgs& g, const unsigned char* wl, const V3Side<EPI>& sd, const float4 b0,
                                               int m0, int srow0, int n, int c4, int lane, const float4 bB = make_float4(0.f, 0.f, 0.f, 0.f),
                                               int mbnd = 0x7fffffff, int mend = 0x7fffffff) {
    // (b0 already contains the first group's row-group bias; rows m >= mbnd take bB instead -- see pp_epilogue)
    float4 vv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) vv[u] = *reinterpret_cast<const float4*>(wl + (srow0 + u * 4 + (lane >> 4)) * V3_RS32 + c4 * 16);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int m = m0 + u * 4 + (lane >> 4);
        if (m >= g.M || m >= mend) continue;      // (mend: first row past a 112-row wave sub-tile)
        float4 v = vv[u];
        const float4 b = m >= mbnd ? bB : b0;
        const size_t o = (size_t)m * g.ldc + n;
        if constexpr (EPI == EPI_F32) {
            v3_st<float4>(g.outF + o, make_float4(v.x * g.alpha + b.x, v.y * g.alpha + b.y, v.z * g.alpha + b.z, v.w * g.alpha + b.w));
        } else if constexpr (EPI == EPI_F32_RESID) {
            float4 r = sd.r[u];
            if constexpr (SM >= 2) {      // split-plane residual: sd.r holds the raw plane words (v3_side_load)
                {
                    const unsigned h0 = __float_as_uint(r.x), h1 = __float_as_uint(r.y), l0 = __float_as_uint(r.z), l1 = __float_as_uint(r.w);
                    if constexpr (SM == 3)
                        r = make_float4(lo8_decode(h2f((bf16_t)(h0 & 0xFFFF)), l0 & 0xFF), lo8_decode(h2f((bf16_t)(h0 >> 16)), (l0 >> 8) & 0xFF),
                                        lo8_decode(h2f((bf16_t)(h1 & 0xFFFF)), (l0 >> 16) & 0xFF), lo8_decode(h2f((bf16_t)(h1 >> 16)), l0 >> 24));
                    else
                        r = make_float4(h2f((bf16_t)(h0 & 0xFFFF)) + h2f((bf16_t)(l0 & 0xFFFF)), h2f((bf16_t)(h0 >> 16)) + h2f((bf16_t)(l0 >> 16)),
                                        h2f((bf16_t)(h1 & 0xFFFF)) + h2f((bf16_t)(l1 & 0xFFFF)), h2f((bf16_t)(h1 >> 16)) + h2f((bf16_t)(l1 >> 16)));
                }
            }
            if constexpr (SM >= 2) asm volatile("" : "+v"(r.x), "+v"(r.y), "+v"(r.z), "+v"(r.w));      // (the decoded value is ONE operand: no re-association into it)
#ifdef ABL_NO_SIDE
            r = make_float4(0.f, 0.f, 0.f, 0.f);
#endif
            const float4 x = make_float4(r.x + v.x + b.x, r.y + v.y + b.y, r.z + v.z + b.z, r.w + v.w + b.w);
            if constexpr (SM == 0) v3_st<float4>(g.outF + o, x);
            if constexpr (SM >= 1) {      // LayerNorm-fold producer: f16 image of the stream + this 64-column slice's (sum, sum of squares) per row
                uint2 pk; pk.x = pack2<true>(x.x, x.y); pk.y = pack2<true>(x.z, x.w);
#ifdef ABL_NO_LO
                if (false) {
#else
                if (g.out_lo != nullptr && g.lo8) {
#endif
                    __builtin_nontemporal_store(lo8_encode4(x.x, x.y, x.z, x.w, pk.x, pk.y), reinterpret_cast<unsigned*>(reinterpret_cast<unsigned char*>(g.out_lo) + lo8_off(g, m, n)));
#ifdef ABL_NO_LO
                } else if (false) {
#else
                } else if (g.out_lo != nullptr) {      // split-plane stream: lo = f16(x - hi)
#endif
                    uint2 pl;
                    pl.x = pack2<true>(x.x - h2f((bf16_t)(pk.x & 0xFFFF)), x.y - h2f((bf16_t)(pk.x >> 16)));
                    pl.y = pack2<true>(x.z - h2f((bf16_t)(pk.y & 0xFFFF)), x.w - h2f((bf16_t)(pk.y >> 16)));
                    v3_st<uint2>(g.out_lo + o, pl);
                } else {
                    v3_st<float4>(g.outF + o, x);
                }
#ifndef ABL_NO_HI
                *reinterpret_cast<uint2*>(g.outH + hi_off(g, m, n)) = pk;      // (a plain store: the next GEMM reads this image right away)
#endif
                // (all 16 lanes of a row take this path together: m is uniform across them)
#ifndef ABL_NO_STATS
                const float s1 = row16_sum((x.x + x.y) + (x.z + x.w));
                const float s2 = row16_sum((x.x * x.x + x.y * x.y) + (x.z * x.z + x.w * x.w));
                if (c4 == 0) *reinterpret_cast<float2*>(g.rowpart + ((size_t)m * (g.N >> 6) + (n >> 6)) * 2) = make_float2(s1, s2);
#endif
            }
        } else if constexpr (EPI == EPI_F32_BF16) {
            v = make_float4(v.x + b.x, v.y + b.y, v.z + b.z, v.w + b.w);
            v3_st<float4>(g.outF + o, v);
            uint2 pk; pk.x = pack2<F16>(v.x, v.y); pk.y = pack2<F16>(v.z, v.w);
            v3_st<uint2>(g.outH + o, pk);
        } else if constexpr (EPI == EPI_GELU32) {
            v = make_float4(v.x + b.x, v.y + b.y, v.z + b.z, v.w + b.w);
            uint2 pk; pk.x = pack2_sel<F16>(v.x, v.y, g.bwd_bf16); pk.y = pack2_sel<F16>(v.z, v.w, g.bwd_bf16);
            v3_st<uint2>(g.outH + o, pk);
            v3_st<float4>(g.outF + o, make_float4(gelu_erf(v.x), gelu_erf(v.y), gelu_erf(v.z), gelu_erf(v.w)));
        } else if constexpr (EPI == EPI_DGELU) {
            const uint2 a = sd.a[u];
            const float h0 = to_f32<F16>((bf16_t)(a.x & 0xFFFF)), h1 = to_f32<F16>((bf16_t)(a.x >> 16));
            const float h2 = to_f32<F16>((bf16_t)(a.y & 0xFFFF)), h3 = to_f32<F16>((bf16_t)(a.y >> 16));
            uint2 pk;
            const f32x2v ga = gelu_fast_grad2(f32x2v{h0, h1}), gb = gelu_fast_grad2(f32x2v{h2, h3});
            pk.x = pack2<F16>(v.x * ga.x, v.y * ga.y);
            pk.y = pack2<F16>(v.z * gb.x, v.w * gb.y);
            v3_st<uint2>(g.outH + o, pk);
        }
    }
}

// LayerNorm-fold producer on the split-plane stream with the byte lo plane, planes in -> planes out (every proj / fc2 of a folded run
// except its first and last): straight from the accumulators, no LDS.  The staged form of this epilogue cost 33-40 us per 256^2 tile
// against a 14 us K = 768 main loop (tools/producer_ablate.sh: no single part -- residual loads, hi stores, row sums -- was worth more
// than 4 us of it): ~160 narrow memory instructions (4 / 8 bytes per lane) and ~80 vector instructions per lane and row.  Here a lane
// owns 16 values of a row (PP_COL order: two runs of 8 columns), so the planes move as 16-byte (hi) / 8-byte (lo) accesses -- 72 memory
// instructions per wave and tile --, every load is issued before the first store (a load behind a store waits for that store's
// acknowledgement: the counter retires in order), and the row sums are one 16-value sum per lane + two cross-lane steps.
template <int RB>
__device__ __forceinline__ void pp_epilogue_lo8_direct(const GemmArgs& g, f32x4_t (&acc)[8][4], int mb, int nb, int lane) {
    const int lq = lane >> 4;
    int lrow = lane & 15;
    asm volatile("" : "+v"(lrow));      // (see PPSinkRows: keeps the per-lane addresses out of the persistent loop's live registers)
    const unsigned char* lo_in = reinterpret_cast<const unsigned char*>(g.res_lo);
    unsigned char* lo_out = reinterpret_cast<unsigned char*>(g.out_lo);
    // row blocks in four groups of two: two groups are requested before any store, the next one each time a group has been computed --
    // its loads queue behind that group's stores, one group of arithmetic ahead of their use -- into the registers it vacated
    // (128 accumulators leave room for two groups in flight)
    constexpr int NG = (RB + 1) / 2;
    u32x4_t hw[NG][2][2];
    u32x2_t lw[NG][2][2];
    const int mfirst = mb + lrow;
    const bool lo = lrow < 8;
    const int r8 = lrow & 7;
    const size_t ocol = (size_t)nb + 32 * (lrow >> 3) + 8 * lq;
    // Loads in the pair-swapped layout too (rows 16 i + r8 and 16 i + 8 + r8, column half l15 >> 3): an instruction then covers 8 rows x
    // 128 B of the hi plane / 8 rows x 64 B of the byte plane -- whole lines.  With a lane reading its own row's two halves by two
    // instructions (16 rows x 64 / 32 B pieces) the launches fetched 1.5x their algorithmic bytes and the byte plane cost as many bytes
    // as the f16 one (FETCH_SIZE, profiles/r4_producer_epilogue.txt).  pp_pair_swap (an involution) brings a lane's own row back.
    auto side = [&](int i, u32x4_t (&hw)[2], u32x2_t (&lw)[2]) {
        const int mA = mb + 16 * i + r8, mB = mA + 8;
#ifdef ABL_NO_SIDE
        hw[0] = hw[1] = u32x4_t{0x3c003c00u, 0x3c003c00u, 0x3c003c00u, 0x3c003c00u}; lw[0] = lw[1] = u32x2_t{(unsigned)mA, 0x80808080u}; return;
#endif
        hw[0] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(g.auxH + lo8_off(g, mA < g.M ? mA : g.M - 1, (int)ocol)));
        hw[1] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(g.auxH + lo8_off(g, mB < g.M ? mB : g.M - 1, (int)ocol)));
        lw[0] = __builtin_nontemporal_load(reinterpret_cast<const u32x2_t*>(lo_in + lo8_off(g, mA < g.M ? mA : g.M - 1, (int)ocol)));
        lw[1] = __builtin_nontemporal_load(reinterpret_cast<const u32x2_t*>(lo_in + lo8_off(g, mB < g.M ? mB : g.M - 1, (int)ocol)));
    };
    float bv[4][4];
    pp_col_consts(bv, g.bias != nullptr ? g.bias + nb : nullptr, nullptr, lq);
#pragma unroll
    for (int i = 0; i < 2; ++i) side(i, hw[0][i], lw[0][i]);
    // bias into the accumulators while the first half's rows are in flight; its registers are free before the second half is requested
#pragma unroll
    for (int i = 0; i < RB; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{acc[i][j][0] + bv[j][0], acc[i][j][1] + bv[j][1], acc[i][j][2] + bv[j][2], acc[i][j][3] + bv[j][3]};
#pragma unroll
    for (int i = 0; i < 2; ++i) side(2 + i, hw[1][i], lw[1][i]);
    auto row_block = [&](int i, const u32x4_t (&hws)[2], const u32x2_t (&lws)[2]) {
        // un-swap the loaded words: this lane's own row, column halves 0 / 1
        uint4 hw[2] = {make_uint4(hws[0][0], hws[0][1], hws[0][2], hws[0][3]), make_uint4(hws[1][0], hws[1][1], hws[1][2], hws[1][3])};
        pp_pair_swap(hw[0], hw[1], lo);
        uint2 lw[2];
        {
            const unsigned rx = pp_ror8(lo ? lws[1][0] : lws[0][0]), ry = pp_ror8(lo ? lws[1][1] : lws[0][1]);
            lw[0] = make_uint2(lo ? lws[0][0] : rx, lo ? lws[0][1] : ry);
            lw[1] = make_uint2(lo ? rx : lws[1][0], lo ? ry : lws[1][1]);
        }
        uint4 oh[2];
        uint2 ol[2];
        f32x2v s1v = {0.f, 0.f}, s2v = {0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            float x[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const unsigned hword = (e >> 1) == 0 ? hw[k].x : ((e >> 1) == 1 ? hw[k].y : ((e >> 1) == 2 ? hw[k].z : hw[k].w));
                const unsigned lword = (e >> 2) == 0 ? lw[k].x : lw[k].y;
                const float hf = h2f((bf16_t)((e & 1) ? (hword >> 16) : (hword & 0xFFFF)));
                // residual = hi (1 + (q - 128) 2^-18) = hi * (q 2^-18 + (1 - 2^-11)), added to the accumulator by the same fma
                const float t = __builtin_fmaf((float)((lword >> (8 * (e & 3))) & 0xFF), 0x1p-18f, 1.0f - 0x1p-11f);
                x[e] = __builtin_fmaf(hf, t, acc[i][2 * k + (e >> 2)][e & 3]);
            }
#pragma unroll
            for (int e = 0; e < 8; e += 2) {
                const f32x2v xv = {x[e], x[e + 1]};
                s1v += xv;
                s2v = xv * xv + s2v;
            }
            oh[k] = make_uint4(pack2<true>(x[0], x[1]), pack2<true>(x[2], x[3]), pack2<true>(x[4], x[5]), pack2<true>(x[6], x[7]));
#ifdef ABL_NO_LO
            ol[k] = make_uint2(oh[k].x, oh[k].y);
#else
            // byte of the new value: (x / hi' - 1) 2^18 + 128, with 1 - hi' / x for x / hi' - 1 (they differ by the square of a number
            // below 2^-11: 1/16 of a step) -- one reciprocal of the fp32 value, one fma on the f16 hi' itself, one fma, round, convert
            unsigned ob[2] = {0u, 0u};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const unsigned hword = e < 2 ? oh[k].x : (e < 4 ? oh[k].y : (e < 6 ? oh[k].z : oh[k].w));
                const float hn = h2f((bf16_t)((e & 1) ? (hword >> 16) : (hword & 0xFFFF)));
                const float eps = __builtin_fmaf(-hn, __builtin_amdgcn_rcpf(x[e]), 1.0f);
                ob[e >> 2] = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_fmaf(eps, 0x1p18f, 128.f), e & 3, ob[e >> 2]);      // (rounds to nearest even, saturates: tools/ablate/cvt_u8_probe.hip)
            }
            ol[k] = make_uint2(ob[0], ob[1]);
#endif
        }
        float s1 = s1v.x + s1v.y, s2 = s2v.x + s2v.y;
        // this 64-column slice's (sum, sum of squares) of row 16 i + l15: the four lane groups hold 16 columns each
#ifndef ABL_NO_STATS
        s1 += __shfl_xor(s1, 16, 64); s2 += __shfl_xor(s2, 16, 64);
        s1 += __shfl_xor(s1, 32, 64); s2 += __shfl_xor(s2, 32, 64);
        const int mrow = mfirst + 16 * i;
        if (lq == 0 && mrow < g.M) *reinterpret_cast<float2*>(g.rowpart + ((size_t)mrow * (g.N >> 6) + (nb >> 6)) * 2) = make_float2(s1, s2);
#else
        if (s1 + s2 == 12345.678f) g.rowpart[0] = s1;
#endif
        // lane pairs swap one half each: stores of whole 128-byte (hi) / 64-byte (lo) row segments, rows 16 i + r8 and 16 i + 8 + r8
        pp_pair_swap(oh[0], oh[1], lo);
        {
            const unsigned rx = pp_ror8(lo ? ol[1].x : ol[0].x), ry = pp_ror8(lo ? ol[1].y : ol[0].y);
            ol[0] = make_uint2(lo ? ol[0].x : rx, lo ? ol[0].y : ry);
            ol[1] = make_uint2(lo ? rx : ol[1].x, lo ? ry : ol[1].y);
        }
#ifdef ABL_NO_ST
        const int mA = (oh[0].x ^ oh[1].y ^ ol[0].x ^ ol[1].y) == 0x12345u ? mb + 16 * i + r8 : g.M;
#else
        const int mA = mb + 16 * i + r8;
#endif
        if (mA < g.M) {
            *reinterpret_cast<uint4*>(g.outH + lo8_off(g, mA, (int)ocol)) = oh[0];      // (a plain store: the next GEMM reads this image right away)
#ifndef ABL_NO_LO
            v3_st<uint2>(lo_out + lo8_off(g, mA, (int)ocol), ol[0]);
#endif
        }
        if (mA + 8 < g.M) {
            *reinterpret_cast<uint4*>(g.outH + lo8_off(g, mA + 8, (int)ocol)) = oh[1];
#ifndef ABL_NO_LO
            v3_st<uint2>(lo_out + lo8_off(g, mA + 8, (int)ocol), ol[1]);
#endif
        }
    };
#pragma unroll
    for (int gi = 0; gi < NG; ++gi) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
            if (2 * gi + i < RB) row_block(2 * gi + i, hw[gi][i], lw[gi][i]);
        if (gi + 2 < NG) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
                if (2 * (gi + 2) + i < RB) side(2 * (gi + 2) + i, hw[gi + 2][i], lw[gi + 2][i]);
        }
    }
}

// GELU' epilogue (dX of fc2 times gelu'(saved pre-activation), student backward) straight from the accumulators: the pre-activation rows
// are fetched up front in the pair-swapped whole-line layout (16 bytes per lane, 8 rows x 128 bytes per instruction -- the staged form
// read and wrote 8 bytes per lane, 128 memory instructions per wave and tile instead of 32), un-swapped in registers, and the products
// leave the same way.  No LDS.
template <bool F16, int RB>
__device__ __forceinline__ void pp_epilogue_dgelu_direct(const GemmArgs& g, const f32x4_t (&acc)[8][4], int mb, int nb, int lane) {
    const int lq = lane >> 4;
    int lrow = lane & 15;
    asm volatile("" : "+v"(lrow));
    const bool lo = lrow < 8;
    const int r8 = lrow & 7;
    const size_t ocol = (size_t)nb + 32 * (lrow >> 3) + 8 * lq;
    u32x4_t hw[RB][2];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        const int mA = mb + 16 * i + r8, mB = mA + 8;
        hw[i][0] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(g.auxH + (size_t)(mA < g.M ? mA : g.M - 1) * g.ldc + ocol));
        hw[i][1] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(g.auxH + (size_t)(mB < g.M ? mB : g.M - 1) * g.ldc + ocol));
    }
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        uint4 h[2] = {make_uint4(hw[i][0][0], hw[i][0][1], hw[i][0][2], hw[i][0][3]), make_uint4(hw[i][1][0], hw[i][1][1], hw[i][1][2], hw[i][1][3])};
        pp_pair_swap(h[0], h[1], lo);      // -> this lane's own row, column halves 0 / 1
        uint4 o[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            unsigned ow[4];
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const unsigned hword = w == 0 ? h[k].x : (w == 1 ? h[k].y : (w == 2 ? h[k].z : h[k].w));
                const f32x2v ga = gelu_fast_grad2(f32x2v{to_f32<F16>((bf16_t)(hword & 0xFFFF)), to_f32<F16>((bf16_t)(hword >> 16))});
                const f32x4_t& a = acc[i][2 * k + (w >> 1)];
                ow[w] = pack2<F16>(a[2 * (w & 1)] * ga.x, a[2 * (w & 1) + 1] * ga.y);
            }
            o[k] = make_uint4(ow[0], ow[1], ow[2], ow[3]);
        }
        pp_pair_swap(o[0], o[1], lo);
        const int mA = mb + 16 * i + r8;
        if (mA < g.M) v3_st<uint4>(g.outH + (size_t)mA * g.ldc + ocol, o[0]);
        if (mA + 8 < g.M) v3_st<uint4>(g.outH + (size_t)(mA + 8) * g.ldc + ocol, o[1]);
    }
}

// fp32 pair swap: a0 / a1 = this lane's row, blocks (0, 1) / (2, 3) as 8 floats each -> (row l15 & 7, blocks 2 hk, 2 hk + 1), (row 8 + (l15 & 7), same blocks)
__device__ __forceinline__ void pp_pair_swap32(float (&a0)[8], float (&a1)[8], bool lo) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float r = __uint_as_float(pp_ror8(__float_as_uint(lo ? a1[e] : a0[e])));
        a0[e] = lo ? a0[e] : r;
        a1[e] = lo ? r : a1[e];
    }
}
// fp32 output (EPI_F32: acc * alpha + bias; plain EPI_F32_RESID: residual + acc + bias, in place or not) straight from the accumulators:
// residual rows requested two row-block groups ahead in the swapped layout, no LDS.  The staged form cost 18 (fp32 out) / 29 us (read-
// modify-write) per 256^2 tile.
template <int EPI, int RB>
__device__ __forceinline__ void pp_epilogue_f32_direct(const GemmArgs& g, const f32x4_t (&acc)[8][4], int mb, int nb, int lane) {
    constexpr bool RES = EPI == EPI_F32_RESID;
    const int lq = lane >> 4;
    int lrow = lane & 15;
    asm volatile("" : "+v"(lrow));
    const bool lo = lrow < 8;
    const int r8 = lrow & 7;
    const size_t ocol = (size_t)nb + 16 * (lrow >> 3) + 4 * lq;      // + 32 for the second float4
    constexpr int NG = (RB + 1) / 2;
    f32x4_t rw[RES ? NG : 1][2][4];      // [group][row block of the group][row A / row B x first / second float4]
    auto side = [&](int i, f32x4_t (&r)[4]) {
        const int mA = mb + 16 * i + r8, mB = mA + 8;
        const float* pA = g.resF + (size_t)(mA < g.M ? mA : g.M - 1) * g.ldc + ocol;
        const float* pB = g.resF + (size_t)(mB < g.M ? mB : g.M - 1) * g.ldc + ocol;
        r[0] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(pA));
        r[1] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(pA + 32));
        r[2] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(pB));
        r[3] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(pB + 32));
    };
    float bv[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (g.bias != nullptr) b = *reinterpret_cast<const float4*>(g.bias + nb + PP_COL32(j, lq));
        bv[j][0] = b.x; bv[j][1] = b.y; bv[j][2] = b.z; bv[j][3] = b.w;
    }
    if constexpr (RES) {
#pragma unroll
        for (int gi = 0; gi < 2 && gi < NG; ++gi)
#pragma unroll
            for (int i = 0; i < 2; ++i)
                if (2 * gi + i < RB) side(2 * gi + i, rw[gi][i]);
    }
    const float alpha = RES ? 1.f : g.alpha;
#pragma unroll
    for (int gi = 0; gi < NG; ++gi) {
#pragma unroll
        for (int ii = 0; ii < 2; ++ii) {
            const int i = 2 * gi + ii;
            if (i >= RB) continue;
            float a0[8], a1[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                a0[e] = __builtin_fmaf(acc[i][e >> 2][e & 3], alpha, bv[e >> 2][e & 3]);
                a1[e] = __builtin_fmaf(acc[i][2 + (e >> 2)][e & 3], alpha, bv[2 + (e >> 2)][e & 3]);
            }
            pp_pair_swap32(a0, a1, lo);
            if constexpr (RES) {      // ((product + bias) + residual: the variants that still stage add in another order -- last-bit differences)
                const f32x4_t (&r)[4] = rw[gi][ii];
#pragma unroll
                for (int e = 0; e < 8; ++e) { a0[e] += r[e >> 2][e & 3]; a1[e] += r[2 + (e >> 2)][e & 3]; }
            }
            const int mA = mb + 16 * i + r8;
            if (mA < g.M) {
                float* p = g.outF + (size_t)mA * g.ldc + ocol;
                v3_st<float4>(p, make_float4(a0[0], a0[1], a0[2], a0[3]));
                v3_st<float4>(p + 32, make_float4(a0[4], a0[5], a0[6], a0[7]));
            }
            if (mA + 8 < g.M) {
                float* p = g.outF + (size_t)(mA + 8) * g.ldc + ocol;
                v3_st<float4>(p, make_float4(a1[0], a1[1], a1[2], a1[3]));
                v3_st<float4>(p + 32, make_float4(a1[4], a1[5], a1[6], a1[7]));
            }
        }
        if constexpr (RES) {
            if (gi + 2 < NG) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    if (2 * (gi + 2) + i < RB) side(2 * (gi + 2) + i, rw[gi + 2][i]);
            }
        }
    }
}

template <int EPI>
struct V3Consts {  // per-lane bias values, fetched before the K loop so their latency is off the epilogue's critical path
    static constexpr bool kStaged16 = (EPI == EPI_BF16 || EPI == EPI_GELU);
    float bv[kStaged16 ? 4 : 1][4];
};
template <int EPI>
__device__ __forceinline__ void v3_load_consts(V3Consts<EPI>& c, const GemmArgs& g, int nb, int lane) {
    if constexpr (EPI == EPI_QKV) {
        c.bv[0][0] = 0.f;
    } else if constexpr (V3Consts<EPI>::kStaged16) {
        pp_col_consts(c.bv, g.bias != nullptr ? g.bias + nb : nullptr, nullptr, lane >> 4);
    } else {
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (g.bias != nullptr) b = *reinterpret_cast<const float4*>(g.bias + nb + (lane & 15) * 4);
        c.bv[0][0] = b.x; c.bv[0][1] = b.y; c.bv[0][2] = b.z; c.bv[0][3] = b.w;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Variants of the 256^2 kernel: the third template argument of gemm_nt_pp_kernel / pp_epilogue (an int: the kernels' symbol names carry
// the number).  pp_select<EPI> (host) is the only place that picks one, PpTraits the only place that says what one means.  All but
// PP_PLAIN and PP_QKV_ROWS take f16 operands only and exist for the encoder epilogues EPI_F32_RESID / EPI_GELU / EPI_QKV; the folded-
// LayerNorm producer is EPI_F32_RESID, its consumers EPI_GELU / EPI_QKV (GemmArgs.rowpart ..).  RB = 7: 224-row tiles; F8: fp8 K tiles.
//   PP_PLAIN              every EPI but EPI_ATOMIC, RB 7 / 8.  A [M, K], B [N, K]; EPI_F32 / EPI_F32_RESID / EPI_DGELU store straight from
//                         the accumulators, EPI_QKV writes every requested output (row-major, transposed, biased second q)
//   PP_GROUP_BIAS         + gbias[m / gb_rows][n].  With F8 (EPI_GELU only): outH2 rows carry their e4m3 image; no fp8 K tile is walked
//   PP_TWO_TERM           B = [hi | lo] ([hi | hi | lo] with b_skip), the A panel walked twice (k_wrap).  With F8 (EPI_F32_RESID / EPI_GELU):
//                         A and B rows [f16 | e4m3], K / 64 f16 tiles then k8 fp8 tiles, no wrap
//   PP_LN                 RB 7 / 8.  Producer: fp32 residual in; fp32 stream + f16 image + rowpart out.  Consumer: rstd (acc - mean colS) + bias
//                         from rowstat / colS; EPI_QKV: q / k / v row-major only
//   PP_QKV_ROWS           EPI_QKV, RB 7 / 8.  PP_PLAIN's operands; q / k / v row-major only (no transposed copies, second q or pos_u), stored
//                         straight from the accumulators
//   PP_LN_PLANES16        producer, RB 7 / 8: residual in as f16 hi + f16 lo planes; fp32 + f16 image or the planes out
//   PP_LN_PLANES8         producer, RB 7 / 8: f16 hi (slab-major) + byte lo planes in and out, stored straight from the accumulators
//   PP_LN_PLANES8_F32OUT  producer, RB 7 / 8: f16 hi + byte lo planes in; fp32 stream + f16 image out
//   PP_TWO_TERM_QKV_ROWS  EPI_QKV: PP_TWO_TERM's operands and K walk (f16 or F8) with PP_QKV_ROWS' epilogue
// ---------------------------------------------------------------------------------------------------------------------
enum { PP_PLAIN = 0, PP_GROUP_BIAS = 1, PP_TWO_TERM = 2, PP_LN = 3, PP_QKV_ROWS = 4, PP_LN_PLANES16 = 5, PP_LN_PLANES8 = 6,
       PP_LN_PLANES8_F32OUT = 7, PP_TWO_TERM_QKV_ROWS = 8 };
template <int V, bool F8 = false>
struct PpTraits {
    static constexpr bool plain = V == PP_PLAIN;
    static constexpr bool group_bias = V == PP_GROUP_BIAS;
    static constexpr bool two_term = V == PP_TWO_TERM || V == PP_TWO_TERM_QKV_ROWS;
    static constexpr bool two_term_walk = two_term && !F8;      // the A panel wraps at k_wrap (the F8 forms walk their [f16 | e4m3] rows once)
    static constexpr bool ln = V == PP_LN || V == PP_LN_PLANES16 || V == PP_LN_PLANES8 || V == PP_LN_PLANES8_F32OUT;
    static constexpr bool planes8_out = V == PP_LN_PLANES8;
    static constexpr bool rows_only = ln || V == PP_QKV_ROWS || V == PP_TWO_TERM_QKV_ROWS;      // head split: row-major q / k / v only
    static constexpr bool slab_a = !group_bias && !two_term;      // (the evaluation-mode variants have no register to spare for slab-major A)
    // SM of v3_side_load / v3_store_batch, the producer's residual form: 0 = not a producer, 1 = fp32, 2 = f16 + f16 planes, 3 = f16 + byte planes
    static constexpr int side_mode(int epi) { return !(ln && epi == EPI_F32_RESID) ? 0 : (V == PP_LN ? 1 : (V == PP_LN_PLANES16 ? 2 : 3)); }
    // epilogues that store straight from the accumulators and leave the LDS alone
    static constexpr bool direct_epi(int epi) { return epi == EPI_BF16 || epi == EPI_GELU || (epi == EPI_QKV && rows_only); }
    // fp32 straight from the accumulators (B rows in PP_COL32 column order)
    static constexpr bool f32_direct(int epi) { return plain && (epi == EPI_F32 || epi == EPI_F32_RESID); }
};

template <int EPI, bool F16, int V, int RB = 8, bool F8 = false>
__device__ __forceinline__ void pp_epilogue(const GemmArgs& g, const f32x4_t (&acc)[8][4], const V3Consts<EPI>& cc,
                                            unsigned char* wl, int mb, int nb, int lane, unsigned long long* gxt = nullptr) {
    // mb = first row of this wave's 128 x 64 sub-tile, nb = its first column
    using T = PpTraits<V, F8>;
    const int l15 = lane & 15, lq = lane >> 4;
    if constexpr (EPI == EPI_BF16 || EPI == EPI_GELU) {
        // 16-byte stores straight from the accumulators (PP_COL column order): no staging, no wave barrier
#pragma unroll
        for (int pass = 0; pass < (EPI == EPI_GELU ? 2 : 1); ++pass) {
            bf16_t* out = (EPI == EPI_GELU && pass == 1) ? g.outH2 : g.outH;
            if (out == nullptr) continue;
            // (opaque to the optimiser: otherwise the per-lane output address is hoisted out of the persistent tile loop as a 64-bit value,
            //  spilled around it in the register-tight variants and reloaded -- behind a vmcnt(0) -- at every tile's store phase)
            int lrow = l15;
            asm volatile("" : "+v"(lrow));
            const int r8 = lrow & 7, hk = lrow >> 3;
            // (slab-major output: the wave's 64 columns are slab nb / 64, rows 128 bytes apart)
            const int ldo = g.c_slab ? 64 : g.ldc;
            bf16_t* const ob = g.c_slab ? out + (size_t)(nb >> 6) * g.M * 64 : out + nb;
            const PPSinkRowsT<F8> sink{ob + (size_t)(mb + r8) * ldo + 32 * hk + 8 * lq, ob + (size_t)(mb + lrow) * ldo + 8 * lq,
                                       8 * ldo, g.M - mb - r8, g.M - mb - lrow, lrow < 8,
                                       (F8 && g.out_e4m3) ? 2 * g.N - (nb + 32 * hk + 8 * lq) : 0};
            if constexpr (T::group_bias) {      // evaluation-mode encoder only (no saved pre-activation: one pass)
                const float *rA, *rB;
                const int bnd = gb_split(g, mb, rA, rB);
                if (EPI == EPI_GELU && pass == 1) pp_stage16_gb<F16, 1>(sink, acc, cc.bv, rA + nb, rB + nb, bnd, l15, lq);
                else pp_stage16_gb<F16, 0>(sink, acc, cc.bv, rA + nb, rB + nb, bnd, l15, lq);
            } else if constexpr (T::ln) {      // consumer: Linear(LayerNorm(x)) from the raw stream's product (no saved pre-activation either)
                if (EPI == EPI_GELU && pass == 1) pp_stage16_ln<F16, 1, false, RB>(sink, acc, cc.bv, g.colS + nb, g.rowstat, mb, g.M, l15, lq);
                else pp_stage16_ln<F16, 0, false, RB>(sink, acc, cc.bv, g.colS + nb, g.rowstat, mb, g.M, l15, lq);
            } else
            if (EPI == EPI_GELU && pass == 1) pp_stage16<F16, 1, RB>(sink, acc, cc.bv);
            else if (EPI == EPI_GELU && F16 && g.bwd_bf16) pp_stage16<false, 0, RB>(sink, acc, cc.bv);  // pre-activation for the bf16 backward
            else pp_stage16<F16, 0, RB>(sink, acc, cc.bv);
#ifdef GX_TRACE
            if (gxt != nullptr) gxt[4] = __builtin_amdgcn_s_memrealtime();
#endif
        }
        return;
    }
    if constexpr (EPI == EPI_QKV) {
        const int D = g.heads * 64;
        const int which = nb / D, h = (nb - which * D) >> 6;
        bf16_t* row_dst = which == 0 ? g.q : (which == 1 ? g.k : g.v);
        if constexpr (T::rows_only) {
            // (folded-LayerNorm consumer / plain encoder form: row-major q / k / v only -- no second biased q, no transposed copies.)
            // Stored straight from the accumulators: a lane's 8 columns of a half are 16 contiguous bytes of one head row.
            if (row_dst == nullptr) return;      // (the row-major V is only needed by the backward: inference passes v = NULL)
            int lrow = l15;
            asm volatile("" : "+v"(lrow));
            const int m_first = mb + (lrow & 7), b0 = m_first / g.seq;
            const PPSinkHeads sink{row_dst + (size_t)h * g.seq * 64 + 32 * (lrow >> 3) + 8 * lq, b0, m_first - b0 * g.seq, g.seq, g.heads * g.seq,
                                   g.M - m_first, lrow < 8};
            if constexpr (T::ln) {
                float bv[4][4];
                pp_stage16_ln<F16, 0, true, RB>(sink, acc, bv, g.colS + nb, g.rowstat, mb, g.M, l15, lq, g.bias + nb);
            } else {
                float bv[4][4];
                pp_col_consts(bv, g.bias != nullptr ? g.bias + nb : nullptr, (which == 0 && g.pu != nullptr) ? g.pu + h * 64 : nullptr, lq);
                pp_stage16<F16, 0, RB>(sink, acc, bv);
            }
            return;
        }
        bf16_t* tr_dst = which == 0 ? g.qt : (which == 1 ? g.kt : g.vt);
        const PPSinkLds lsink{wl, l15, lq};
        const int npass = (which == 0 && g.q2 != nullptr) ? 2 : 1;
        for (int pass = 0; pass < npass; ++pass) {
            const float* extra = nullptr;
            if (which == 0 && g.pu != nullptr) extra = (pass == 0 ? g.pu : g.pv) + h * 64;
            bf16_t* rd = pass == 0 ? row_dst : g.q2;
            bf16_t* td = pass == 0 ? tr_dst : g.q2t;
            float bv[4][4];
            pp_col_consts(bv, g.bias != nullptr ? g.bias + nb : nullptr, extra, lq);
            if constexpr (T::group_bias) {
                const float *rA, *rB;
                const int bnd = gb_split(g, mb, rA, rB);
                pp_stage16_gb_k<F16, 0>(lsink, acc, bv, rA + nb, rB + nb, bnd, l15, lq);
            } else {
                pp_stage16<F16, 0, RB>(lsink, acc, bv);
            }
            // Tensors that only the bf16 backward reads (row-major V; Q^T, K^T, (q+v)^T) are emitted as bf16 when g.bwd_bf16 is
            // set: converted from the staged f16 tile on the way out (same double rounding as a later in-place conversion,
            // without the extra pass over HBM); V^T and the row-major q / k stay f16.
            // (a row-major V that the forward itself consumes -- no V^T requested: the encoder's attention transposes it in LDS -- stays f16)
            const bool row_bf = F16 && g.bwd_bf16 && which == 2 && pass == 0 && g.vt != nullptr;
            const bool tr_bf = F16 && g.bwd_bf16 && !(which == 2 && pass == 0);
            __builtin_amdgcn_wave_barrier();
            if (rd != nullptr) {  // (the row-major V is only needed by the backward: inference passes v = NULL)
#pragma unroll
                for (int rb = 0; rb < 16; rb += 8) {
                    uint4 v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const uint4*>(wl + ((rb + u) * 8 + (lane >> 3)) * V3_RS16 + (lane & 7) * 16);
                    if (row_bf) {
#pragma unroll
                        for (int u = 0; u < 8; ++u) v[u] = make_uint4(h2x2_to_bf(v[u].x), h2x2_to_bf(v[u].y), h2x2_to_bf(v[u].z), h2x2_to_bf(v[u].w));
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int m = mb + (rb + u) * 8 + (lane >> 3);
                        if (m < g.M && (rb + u) * 8 + (lane >> 3) < 16 * RB) {
                            const int bidx = m / g.seq, t = m - bidx * g.seq;
                            v3_st<uint4>(rd + ((size_t)(bidx * g.heads + h) * g.seq + t) * 64 + (lane & 7) * 8, v[u]);
                        }
                    }
                }
            }
            if (td != nullptr && (g.seq & 1) == 0) {
                // transposed copy [bh][d][seq_pad]: a lane owns a PAIR of consecutive tokens (same clip: seq is even and
                // the pair starts on an even row) and one of two interleaved d columns -> 4-byte stores, 32 lanes = 128 B
                const int pr = (lane & 31) * 2, dsel = lane >> 5;
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const int row = half * 64 + pr, m = mb + row;
                    if (m < g.M && row < 16 * RB) {
                        const int bidx = m / g.seq, t = m - bidx * g.seq;
                        bf16_t* base = td + (size_t)(bidx * g.heads + h) * 64 * g.seq_pad + t;
                        const unsigned short* s0 = reinterpret_cast<const unsigned short*>(wl + row * V3_RS16);
                        const unsigned short* s1 = reinterpret_cast<const unsigned short*>(wl + (row + 1) * V3_RS16);
#pragma unroll 8
                        for (int dd = 0; dd < 32; ++dd) {
                            const int d = dd * 2 + dsel;
                            unsigned pk = (unsigned)s0[d] | ((unsigned)s1[d] << 16);
                            if (tr_bf) pk = h2x2_to_bf(pk);
                            *reinterpret_cast<unsigned*>(base + (size_t)d * g.seq_pad) = pk;
                        }
                    }
                }
            } else if (td != nullptr) {
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const int row = half * 64 + lane, m = mb + row;
                    if (m < g.M && row < 16 * RB) {
                        const int bidx = m / g.seq, t = m - bidx * g.seq;
                        bf16_t* base = td + (size_t)(bidx * g.heads + h) * 64 * g.seq_pad + t;
                        const unsigned short* src = reinterpret_cast<const unsigned short*>(wl + row * V3_RS16);
#pragma unroll 8
                        for (int d = 0; d < 64; ++d) base[(size_t)d * g.seq_pad] = tr_bf ? f2bf(h2f(src[d])) : src[d];
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        return;
    }
    if constexpr (T::f32_direct(EPI)) {
        pp_epilogue_f32_direct<EPI, RB>(g, acc, mb, nb, lane);
        return;
    }
    if constexpr (EPI == EPI_DGELU && T::plain) {
        pp_epilogue_dgelu_direct<F16, RB>(g, acc, mb, nb, lane);
        return;
    }
    if constexpr (EPI == EPI_F32_RESID && T::planes8_out) {      // byte planes in -> byte planes out: straight from the accumulators
        pp_epilogue_lo8_direct<RB>(g, const_cast<f32x4_t (&)[8][4]>(acc), mb, nb, lane);
        return;
    }
    // fp32-staged epilogues (two passes of 64 rows): EPI_F32, EPI_F32_RESID, EPI_F32_BF16, EPI_GELU32, EPI_DGELU
    // 16 lanes x 16 B = one 256-B fp32 row; the lane's 4 columns (and so its bias) are the same for every row.  Four batches
    // of 8 rows-per-lane; the residual / saved pre-activation of batch k+1 is requested before batch k is stored, so its
    // latency hides under the stores (loads placed between stores would each cost a full wait, see pp_col_consts).
    const int c4 = lane & 15, n = nb + c4 * 4;
    float4 b = make_float4(cc.bv[0][0], cc.bv[0][1], cc.bv[0][2], cc.bv[0][3]);
    float4 bB = b;
    int mbnd = 0x7fffffff;
    if constexpr (T::group_bias) {
        const float *rA, *rB;
        mbnd = mb + gb_split(g, mb, rA, rB);
        const float4 xa = *reinterpret_cast<const float4*>(rA + n), xb = *reinterpret_cast<const float4*>(rB + n);
        bB = make_float4(b.x + xb.x, b.y + xb.y, b.z + xb.z, b.w + xb.w);
        b = make_float4(b.x + xa.x, b.y + xa.y, b.z + xa.z, b.w + xa.w);
    }
    const int mend = mb + 16 * RB;
    constexpr int SM = T::side_mode(EPI);      // (the producer's residual form is part of the kernel variant -- see v3_side_load)
#ifdef ABL_NO_EPI
    if constexpr (SM >= 2) return;
#endif
    V3Side<EPI> s0, s1;
    v3_side_load<EPI, SM>(s0, g, mb, n, lane);
    pp_stage32<RB, true>(wl, acc, 0, l15, lq);
    __builtin_amdgcn_wave_barrier();
    v3_side_load<EPI, SM>(s1, g, mb + 32, n, lane);
    v3_store_batch<EPI, F16, SM>(g, wl, s0, b, mb, 0, n, c4, lane, bB, mbnd, mend);
    v3_side_load<EPI, SM>(s0, g, mb + 64, n, lane);
    v3_store_batch<EPI, F16, SM>(g, wl, s1, b, mb + 32, 32, n, c4, lane, bB, mbnd, mend);
    __builtin_amdgcn_wave_barrier();
    pp_stage32<RB, true>(wl, acc, 1, l15, lq);
    __builtin_amdgcn_wave_barrier();
    v3_side_load<EPI, SM>(s1, g, mb + 96, n, lane);
    v3_store_batch<EPI, F16, SM>(g, wl, s0, b, mb + 64, 0, n, c4, lane, bB, mbnd, mend);
    v3_store_batch<EPI, F16, SM>(g, wl, s1, b, mb + 96, 32, n, c4, lane, bB, mbnd, mend);
    __builtin_amdgcn_wave_barrier();
}
