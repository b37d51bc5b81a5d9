// Weight-gradient GEMM in TN form for gfx950 (sed_gemm_dw_tn): the 256^2 ping-pong kernel on transposing LDS reads, its two split-K
// reduce kernels and the host entry point.  Shares the tile constants, mfma16, pp_stage32 / v3_st and the CU budget with the NT
// GEMMs (gemm_args.h); nothing else.
#include "gemm_args.h"
#include "../../include/sed_hip.h"

// ---------------------------------------------------------------------------------------------------------------------
// Weight-gradient GEMM in TN form: dW[m, n] += sum_t dY[t, m] * X[t, n] with BOTH operands read in their natural row-major
// [token][feature] layout -- no transposed operand copies in HBM (the NT kernels need dY^T and X^T: 6.4 ms/step of transposes).
// The contraction index is the slow dimension of both tiles, so the MFMA fragments (8 consecutive tokens per lane) are columns of
// the LDS image: read with `ds_read_b64_tr_b16`.  Semantics measured on gfx950 (tools/ablate/trread.hip): the 16 lanes of a group
// supply 16 addresses of 8-byte chunks, taken as a [4 rows r = a>>2][4 chunks c = a&3] grid = a 4 x 16 halfword matrix M;
// lane i of the group receives column i: {M[0][i], M[1][i], M[2][i], M[3][i]}.  With rows = 4 consecutive tokens and columns =
// 16 consecutive features, two such reads give the 8-token slice of one feature per lane -- exactly the v_mfma_f32_16x16x32
// operand (lane & 15 = feature, lane >> 4 = token group of 8): lane group G reads tokens 8 G .. 8 G + 7 of the 32-token k-step.
// LDS stage = [64 tokens][256 features] per operand (512-B rows), filled by DMA; the 64-B unit u of token row k is stored at unit
// u ^ (k & 3) and its 32-B halves are swapped when (k >> 3) & 1, so that the 32 lanes of a read cycle (groups G, G + 1: token rows
// 8 G + r and 8 G + 8 + r, r = 0..3, 32 bytes each) cover four whole 64-B units = all 64 banks.
// Same 256 x 256 x 64 tiling / 8 waves (128 x 64 per wave) / two stages as the NT kernel; split-K over the tokens.
// X may be IEEE half (saved forward activation): converted to bf16 in registers (the gradient-side MFMA is bf16).
// ---------------------------------------------------------------------------------------------------------------------
struct TnArgs {
    const bf16_t* A;  // dY [T, lda]  bf16
    const bf16_t* B;  // X  [T, ldb]  bf16 or f16
    float* C;         // dW [M, ldc]  fp32 (accumulated)
    float* ws;        // optional split-K workspace [ksplit][M][N] fp32 (plain stores + a reduce pass instead of atomics)
    float* dbias;     // optional: dbias[m] += sum_t dY[t, m] (the bias gradient of the same linear), taken from the dY fragments
    int M, N, T, lda, ldb, ldc, ksplit, b_f16;
};
template <int OFF>
__device__ __forceinline__ unsigned long long lds_tr(unsigned addr) {
    unsigned long long v;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
    return v;
}
__device__ __forceinline__ s16x8_t tn_frag(unsigned long long lo, unsigned long long hi, bool cvt_f16) {
    unsigned w[4] = {(unsigned)lo, (unsigned)(lo >> 32), (unsigned)hi, (unsigned)(hi >> 32)};
    if (cvt_f16) {
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = h2x2_to_bf(w[e]);
    }
    s16x8_t f;
    __builtin_memcpy(&f, w, 16);
    return f;
}
// LDS stage: per operand four PANELS of [64 tokens][64 features] (128-byte rows, 8 KiB each) -- a DMA piece is 8 token rows of one
// panel, so pieces (and the DMA slots built from them) follow the feature halves the ping-pong phases consume, exactly like the row
// halves of the NT kernel.  Inside a row the 32-byte block b (16 features) of token row r sits at block b ^ (r & 3) ^ ((r >> 3) & 1):
// the 32 lanes of one transposing-read cycle (two 16-lane groups: token rows 8 G + r and 8 G + 8 + r, r = 0..3, 32 bytes each) then
// cover all 64 banks.  A stage s at s * 32 KiB, B stage s at 64 KiB + s * 32 KiB.
// K loop: the ping-pong schedule of gemm_nt_pp_kernel (two wave rows half a phase apart, four 64 x 32 quadrant phases per 64-token
// K tile, B half 0 of the next tile read in P4).  DMA slots (2 pieces per wave each): A0 = A panels {0, 2}, A1 = {1, 3}, B01, B23.
// A piece spans both feature halves of the waves that read it, so a B slot is free only after P2 and the issue order differs from the
// NT kernel: P1(t): B23(t+1), P2(t): A1(t+1), P3(t): A0(t+2), P4(t): B01(t+2); `vmcnt(4)` at P3(t) retires A0 / B01 / B23 of tile
// t+1 one phase ahead of their first read (B half 0 in P4(t)), `vmcnt(6)` at P1(t) retires A1(t) two phases ahead of its read.
template <bool BF16_B>
__global__ __launch_bounds__(512) void gemm_tn_dw_kernel(const TnArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds3[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    // One linear workgroup index, split-major and XCD-contiguous: the tiles of one token split run side by side on ONE XCD, so the
    // split's dY / X rows go through that L2 once for all of them (9 x 3 tiles: fabric reads 663 -> ~250 MB per launch; with the tile
    // index spread over the XCDs every dY panel was fetched by three L2s and every X panel by up to nine).
    // M, N multiples of 64: the last tile of a dimension may be partly valid.  Its out-of-range operand columns are whatever lies behind
    // them in memory (the next token's row; nothing past the buffer end) -- an output element depends on its own operand columns only,
    // and the out-of-range rows / columns of the tile are not stored.
    const int ntn = (g.N + V3_T - 1) / V3_T, ntm = (g.M + V3_T - 1) / V3_T, ntiles = ntm * ntn;
    const int L = xcd_remap(blockIdx.x, ntiles * g.ksplit);
    const int split = L / ntiles, t = L - split * ntiles;
    const int m0 = (t % ntm) * V3_T, n0 = (t / ntm) * V3_T;
    const int ktiles = (g.T + BK - 1) / BK;
    const int kt_begin = (int)(((long long)split * ktiles) / g.ksplit);
    const int kt_end = (int)(((long long)(split + 1) * ktiles) / g.ksplit);
    const int nk = kt_end - kt_begin;
    const int mw = (g.M - m0) < V3_T ? (g.M - m0) : V3_T, nw = (g.N - n0) < V3_T ? (g.N - n0) : V3_T;     // valid tile extent
    // token rows of this split; a ragged last K tile (T not a multiple of 64) ends the buffer descriptors at the last real token, the
    // rows behind it read as zeros and add nothing to dW or to the bias sums (round 4: the tail used to be two transposes + an NT GEMM)
    const int trows = (g.T - kt_begin * BK) < nk * BK ? (g.T - kt_begin * BK) : nk * BK;
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)(g.A + (size_t)kt_begin * BK * g.lda + m0), 0,
                                                                        (trows - 1) * g.lda * 2 + mw * 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)(g.B + (size_t)kt_begin * BK * g.ldb + n0), 0,
                                                                        (trows - 1) * g.ldb * 2 + nw * 2, 0x00020000);
    // DMA pieces of this wave: slot piece index pi = 2 wave + e -> panel list[pi >> 3], token rows 8 (pi & 7) .. + 7
    const int prow = lane >> 3, pc = lane & 7;
    int vo[4][2], ld_[4][2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int pi = 2 * wave + e, q = pi & 7, hi = pi >> 3;
        const int panels[4] = {2 * hi, hi, 2 + hi, 2 * hi + 1};      // slots: A0 {0,2}, B01 {0,1}, B23 {2,3}, A1 {1,3}
        const int r = 8 * q + prow;
        const int lc = ((((pc >> 1) ^ (r & 3) ^ ((r >> 3) & 1)) & 3) << 1) | (pc & 1);      // logical 16-B chunk held by physical chunk pc
#pragma unroll
        for (int sl = 0; sl < 4; ++sl) {
            const bool is_b = (sl == 1 || sl == 2);
            vo[sl][e] = r * (is_b ? g.ldb : g.lda) * 2 + (panels[sl] * 64 + lc * 8) * 2;
            ld_[sl][e] = (is_b ? 65536 : 0) + panels[sl] * 8192 + q * 1024;
        }
    }
    const int kstride_a = BK * g.lda * 2, kstride_b = BK * g.ldb * 2;
#define TN_DMA(SL, KT)                                                                                                    \
    {                                                                                                                     \
        const bool b_ = ((SL) == 1 || (SL) == 2);                                                                         \
        const int so_ = (KT) * (b_ ? kstride_b : kstride_a), st_ = ((KT) & 1) << 15;                                      \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(b_ ? rb : ra, (lds_ptr_t)(lds3 + st_ + ld_[SL][0]), 16, vo[SL][0], so_, 0, 0); \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(b_ ? rb : ra, (lds_ptr_t)(lds3 + st_ + ld_[SL][1]), 16, vo[SL][1], so_, 0, 0); \
    }
    f32x4_t acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // transposing-read lane addresses: group G = lane >> 4 reads token rows 8 G + (a >> 2) (+ 4 for the second read), a = lane & 15
    const int a = lane & 15, G = lane >> 4;
    const unsigned lbase = (unsigned)(size_t)lds3;
    const unsigned rowb = (unsigned)((8 * G + (a >> 2)) * 128 + 8 * (a & 3));
    const int sx = ((a >> 2) & 3) ^ (G & 1);
    unsigned aaddr[4], baddr[4];        // one per 32-byte block (16 features) of a 64-feature panel
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        aaddr[u] = lbase + (2 * wm) * 8192 + rowb + ((u ^ sx) << 5);
        baddr[u] = lbase + 65536 + wn * 8192 + rowb + ((u ^ sx) << 5);
    }
    const bool do_bias = g.dbias != nullptr && n0 == 0;
    float colacc[2] = {0.f, 0.f};
    unsigned long long al[4][2], ah[4][2], bl[2][2][2], bh[2][2][2];   // A half: [ii][ks]; B: [set][jj][ks]; lo / hi = tokens +0..3 / +4..7
#define TN_RD_A(H)                                                                                                        \
    _Pragma("unroll") for (int ii = 0; ii < 4; ++ii) {                                                                    \
        al[ii][0] = lds_tr<(H) * 8192>(aaddr[ii]); ah[ii][0] = lds_tr<(H) * 8192 + 512>(aaddr[ii]);                       \
        al[ii][1] = lds_tr<(H) * 8192 + 4096>(aaddr[ii]); ah[ii][1] = lds_tr<(H) * 8192 + 4608>(aaddr[ii]);               \
    }
#define TN_RD_B(SET, JH, XOR)                                                                                             \
    _Pragma("unroll") for (int jj = 0; jj < 2; ++jj) {                                                                    \
        bl[SET][jj][0] = lds_tr<0>(baddr[2 * (JH) + jj] ^ (XOR)); bh[SET][jj][0] = lds_tr<512>(baddr[2 * (JH) + jj] ^ (XOR)); \
        bl[SET][jj][1] = lds_tr<4096>(baddr[2 * (JH) + jj] ^ (XOR)); bh[SET][jj][1] = lds_tr<4608>(baddr[2 * (JH) + jj] ^ (XOR)); \
    }
    // the compiler does not know the asm read results are in flight: the fragments are tied to the wait that retires them
#define TN_TIE_A() asm volatile("" : "+v"(al[0][0]), "+v"(al[0][1]), "+v"(al[1][0]), "+v"(al[1][1]), "+v"(al[2][0]), "+v"(al[2][1]), "+v"(al[3][0]), "+v"(al[3][1]), \
                                   "+v"(ah[0][0]), "+v"(ah[0][1]), "+v"(ah[1][0]), "+v"(ah[1][1]), "+v"(ah[2][0]), "+v"(ah[2][1]), "+v"(ah[3][0]), "+v"(ah[3][1]) :: "memory");
#define TN_TIE_B(SET) asm volatile("" : "+v"(bl[SET][0][0]), "+v"(bl[SET][0][1]), "+v"(bl[SET][1][0]), "+v"(bl[SET][1][1]), \
                                        "+v"(bh[SET][0][0]), "+v"(bh[SET][0][1]), "+v"(bh[SET][1][0]), "+v"(bh[SET][1][1]) :: "memory");
#define TN_SYNC_IN()                                                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                                                    \
    __builtin_amdgcn_s_barrier();                                                                                         \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#define TN_MFMA(IH, JH, SET, BIAS)                                                                                        \
    __builtin_amdgcn_sched_barrier(0);                                                                                    \
    {                                                                                                                     \
        s16x8_t bf_[2][2];                                                                                                \
        _Pragma("unroll") for (int jj = 0; jj < 2; ++jj)                                                                  \
            _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) bf_[jj][ks] = tn_frag(bl[SET][jj][ks], bh[SET][jj][ks], !BF16_B); \
        _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                                  \
            _Pragma("unroll") for (int ii = 0; ii < 4; ++ii) {                                                            \
                const s16x8_t af = tn_frag(al[ii][ks], ah[ii][ks], false);                                                \
                _Pragma("unroll") for (int jj = 0; jj < 2; ++jj)                                                          \
                    acc[4 * (IH) + ii][2 * (JH) + jj] = mfma16<false>(bf_[jj][ks], af, acc[4 * (IH) + ii][2 * (JH) + jj]); \
                if ((BIAS) && do_bias && ((4 * (IH) + ii) >> 1) == wn) {                                                  \
                    unsigned w4[4];                                                                                       \
                    __builtin_memcpy(w4, &af, 16);                                                                        \
                    _Pragma("unroll") for (int e = 0; e < 4; ++e)                                                         \
                        colacc[ii & 1] += __uint_as_float(w4[e] << 16) + __uint_as_float(w4[e] & 0xffff0000u);            \
                }                                                                                                         \
            }                                                                                                             \
    }                                                                                                                     \
    __builtin_amdgcn_sched_barrier(0);                                                                                    \
    __builtin_amdgcn_s_barrier();                                                                                         \
    __builtin_amdgcn_sched_barrier(0);
    // one K tile; X = B register set holding this tile's half 0, Y = the other set
#define TN_TILE(T_, X, Y)                                                                                                 \
    if ((T_) + 1 < nk) { TN_DMA(2, (T_) + 1) asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); }                           \
    else { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }                                                             \
    TN_RD_A(0)                                                                                                            \
    TN_SYNC_IN() TN_TIE_A() TN_TIE_B(X)                                                                                   \
    TN_MFMA(0, 0, X, true)                                                                                                \
    if ((T_) + 1 < nk) TN_DMA(3, (T_) + 1)                                                                                \
    TN_RD_B(Y, 1, 0)                                                                                                      \
    TN_SYNC_IN() TN_TIE_B(Y)                                                                                              \
    TN_MFMA(0, 1, Y, false)                                                                                               \
    if ((T_) + 2 < nk) { TN_DMA(0, (T_) + 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); }                           \
    else if ((T_) + 1 < nk) { asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); }                                          \
    TN_RD_A(1)                                                                                                            \
    TN_SYNC_IN() TN_TIE_A()                                                                                               \
    TN_MFMA(1, 1, Y, true)                                                                                                \
    if ((T_) + 2 < nk) TN_DMA(1, (T_) + 2)                                                                                \
    if ((T_) + 1 < nk) { TN_RD_B(Y, 0, 0x8000) }                                                                          \
    TN_SYNC_IN() TN_TIE_B(Y)                                                                                              \
    TN_MFMA(1, 0, X, false)                                                                                               \
    _Pragma("unroll") for (int u = 0; u < 4; ++u) { aaddr[u] ^= 0x8000; baddr[u] ^= 0x8000; }

    if (nk > 0) {
        TN_DMA(0, 0) TN_DMA(1, 0) TN_DMA(2, 0) TN_DMA(3, 0)
        if (nk > 1) { TN_DMA(0, 1) TN_DMA(1, 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); }
        else { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
    }
    __builtin_amdgcn_s_barrier();
    if (wm == 1) __builtin_amdgcn_s_barrier();   // second wave row: half a phase behind
    if (nk > 0) { TN_RD_B(0, 0, 0) }
    int it = 0;
    for (; it + 1 < nk; it += 2) {
        TN_TILE(it, 0, 1)
        TN_TILE(it + 1, 1, 0)
    }
    if (it < nk) { TN_TILE(it, 0, 1) }
    if (wm == 0) __builtin_amdgcn_s_barrier();   // pairs with the last barrier of waves 4-7
#undef TN_DMA
#undef TN_RD_A
#undef TN_RD_B
#undef TN_TIE_A
#undef TN_TIE_B
#undef TN_SYNC_IN
#undef TN_MFMA
#undef TN_TILE
    if (do_bias) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            float c = colacc[e];
            c += __shfl_xor(c, 16, 64);      // the four 8-token groups of the fragment
            c += __shfl_xor(c, 32, 64);
            if (lane < 16 && wm * 128 + (2 * wn + e) * 16 + lane < mw) unsafeAtomicAdd(&g.dbias[m0 + wm * 128 + (2 * wn + e) * 16 + lane], c);
        }
    }
    __builtin_amdgcn_s_barrier();    // both wave rows are past their last operand read: LDS becomes the per-wave staging area
    // Split-K partial sums.  With a workspace: plain coalesced stores of the tile into ws[split] (a reduce pass adds the splits
    // into dW) -- one workgroup per CU cannot hide 64 Ki device-scope atomics behind anything (measured ~150-200 us per GEMM,
    // as long as the whole K loop).  Without: atomics straight into dW.
    unsigned char* wl = lds3 + wave * V3_WLDS;
    const int l15 = lane & 15, lq = lane >> 4;
    const int mb = m0 + wm * 128, nb = n0 + wn * 64;
    if (mb >= g.M || nb >= g.N) return;      // (64-granular validity: each 64 x 64 pass of a wave's sub-tile is entirely in or entirely out)
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        if (mb + pass * 64 >= g.M) break;
        pp_stage32(wl, acc, pass, l15, lq);
        __builtin_amdgcn_wave_barrier();
        if (g.ws != nullptr) {
            float* dstp = g.ws + ((size_t)split * g.M + mb + pass * 64) * g.N + nb + (lane & 15) * 4;
#pragma unroll
            for (int rb2 = 0; rb2 < 16; rb2 += 8) {
                float4 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4*>(wl + ((rb2 + u) * 4 + (lane >> 4)) * V3_RS32 + (lane & 15) * 16);
#pragma unroll
                for (int u = 0; u < 8; ++u) v3_st<float4>(dstp + (size_t)((rb2 + u) * 4 + (lane >> 4)) * g.N, v[u]);
            }
        } else {
#pragma unroll 8
            for (int row = 0; row < 64; ++row) {
                const float v = *reinterpret_cast<const float*>(wl + row * V3_RS32 + lane * 4);
                unsafeAtomicAdd(&g.C[(size_t)(mb + pass * 64 + row) * g.ldc + nb + lane], v);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// dW[m, n] += sum_s ws[s][m][n]
__global__ __launch_bounds__(256) void tn_reduce_kernel(const float* __restrict__ ws, int ks, int M, int N, float* __restrict__ C,
                                                        int ldc) {
    const size_t total4 = (size_t)M * N / 4, plane4 = total4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
        float4 a = reinterpret_cast<const float4*>(ws)[i];
        for (int s2 = 1; s2 < ks; ++s2) {
            const float4 b = reinterpret_cast<const float4*>(ws)[(size_t)s2 * plane4 + i];
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        }
        const size_t e = i * 4, m = e / N, n = e - m * N;
        float4* dst = reinterpret_cast<float4*>(C + m * ldc + n);
        float4 c = *dst;
        c.x += a.x; c.y += a.y; c.z += a.z; c.w += a.w;
        *dst = c;
    }
}

// ... for small outputs (a few thousand float4s: the [64, k] gradient images of the PMAM CNN reduce up to 256 splits with 16 blocks' worth of
// threads, each walking all splits one dependent load after the other -- 64 us): 32 float4s per block, the splits dealt to 8 thread groups
__global__ __launch_bounds__(256) void tn_reduce_small_kernel(const float* __restrict__ ws, int ks, int M, int N, float* __restrict__ C,
                                                              int ldc) {
    __shared__ float4 red[8][32];
    const size_t total4 = (size_t)M * N / 4;
    const size_t i = (size_t)blockIdx.x * 32 + (threadIdx.x & 31);
    const int grp = threadIdx.x >> 5;
    float4 a = {0.f, 0.f, 0.f, 0.f};
    if (i < total4)
        for (int s2 = grp; s2 < ks; s2 += 8) {
            const float4 b = reinterpret_cast<const float4*>(ws)[(size_t)s2 * total4 + i];
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        }
    red[grp][threadIdx.x & 31] = a;
    __syncthreads();
    if (grp == 0 && i < total4) {
#pragma unroll
        for (int g2 = 1; g2 < 8; ++g2) { const float4 b = red[g2][threadIdx.x]; a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
        const size_t e = i * 4, m = e / N, n = e - m * N;
        float4* dst = reinterpret_cast<float4*>(C + m * ldc + n);
        float4 c = *dst;
        c.x += a.x; c.y += a.y; c.z += a.z; c.w += a.w;
        *dst = c;
    }
}

extern "C" int sed_gemm_dw_tn(const void* dY, const void* X, int x_f16, int T, int M, int N, int ldy, int ldx, float* dW,
                              int ldc, float* dbias, float* workspace, int64_t workspace_bytes, hipStream_t stream) {
    (void)hipGetLastError();
    if (T <= 0 || (M % 64) || (N % 64) || (ldy % 8) || (ldx % 8) || (ldc % 4) || M <= 0 || N <= 0) return SED_ERR_ARG;
    TnArgs g;
    g.A = (const bf16_t*)dY; g.B = (const bf16_t*)X; g.C = dW; g.dbias = dbias;
    g.M = M; g.N = N; g.T = T; g.lda = ldy; g.ldb = ldx; g.ldc = ldc; g.b_f16 = x_f16;
    const int tiles = cdiv(M, V3_T) * cdiv(N, V3_T), ktiles = cdiv(T, BK);
    // one workgroup per CU and ONE round: tiles * ks <= 256 (rounding the split count up instead costs a second, nearly empty
    // round -- 36 tiles x 8 splits = 288 workgroups took twice the time of 36 x 7)
    int ks = gemm_cu_budget() / tiles;      // (the CUs a data-parallel job leaves to the GEMMs)
    if (ks >= 8) ks &= ~7;        // whole splits per XCD (the kernel lays the splits out XCD-contiguously)
    if (ks > ktiles / 16) ks = ktiles / 16;
    if (ks < 1) ks = 1;
    g.ksplit = ks;
    g.ws = (workspace != nullptr && workspace_bytes >= (int64_t)ks * M * N * 4) ? workspace : nullptr;
    static bool attr[2] = {false, false};
    dim3 grid(tiles * ks);
    if (x_f16) launch_big_lds(attr[1], gemm_tn_dw_kernel<false>, grid, dim3(512), V3_LDS, stream, g);
    else launch_big_lds(attr[0], gemm_tn_dw_kernel<true>, grid, dim3(512), V3_LDS, stream, g);
    if (g.ws != nullptr) {
        const size_t total4 = (size_t)M * N / 4;
        if (total4 < 32768 && ks >= 16) {
            hipLaunchKernelGGL(tn_reduce_small_kernel, dim3((unsigned)((total4 + 31) / 32)), dim3(256), 0, stream, g.ws, ks, M, N, dW, ldc);
        } else {
            int blocks = (int)((total4 + 255) / 256);
            if (blocks > 2048) blocks = 2048;
            hipLaunchKernelGGL(tn_reduce_kernel, dim3(blocks), dim3(256), 0, stream, g.ws, ks, M, N, dW, ldc);
        }
    }
    return sed_check_launch();
}
