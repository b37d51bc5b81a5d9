// bf16 MFMA GEMM (NT form) with fused epilogues, for gfx950.
//
//   C[M,N] = A[M,K] . B[N,K]^T        A, B bf16 row-major with K contiguous (nn.Linear weight layout for B)
//
// 128x128x64 workgroup tile, 4 waves (2x2), each wave a 64x64 sub-tile = 2x2 v_mfma_f32_32x32x16_bf16 blocks,
// fp32 accumulation.  Operand tiles are register-staged (global_load_dwordx4 issued before the MFMA phase,
// ds_write_b128 after it) into double-buffered, XOR-swizzled LDS so that the fragment ds_read_b128s are
// bank-conflict free (128-byte rows: 16-B chunk index ^= (row >> 1) & 7).  One barrier per K tile.
// Workgroup ids are remapped XCD-aware so that neighbouring tiles (which share A rows / B columns) hit the
// same per-XCD L2.
//
// Replaces (reference, all relative to /root/reference): F.linear / nn.Linear calls at
// src/models/passt/passt.py:271,274,332,342; src/models/transformer/transformerXL.py:382,493,584;
// timm Mlp fc1/fc2 in the context blocks; the conv2d of passt.py:307 (as im2col GEMM);
// src/models/passt/passt_sed.py:196 (mlm_mlp) and their autograd backward GEMMs.
//
// This file, top to bottom: the 128^2 kernel described above, the K loop of the 256^2 ping-pong kernel, the host side (tile-counter ring, CU
// budget, pp_geometry / pp_select / launch_gemm, the sed_gemm_nt* / sed_gemm_qkv* entry points).  Arguments and shared helpers:
// gemm_args.h; the 256^2 kernel's epilogues: gemm_epilogue.h; the weight-gradient (TN) GEMM: gemm_tn.hip; casts, transposes and
// operand images: layout.hip.
#include <stdlib.h>
#include <atomic>

#include "gemm_epilogue.h"
#include "../../include/sed_hip.h"

// Epilogue for one accumulator quad.  The MFMA operands are issued swapped (B fragment as the row operand), so the
// accumulator block holds C^T: a lane owns ONE output row m and a register quad holds 4 CONSECUTIVE columns n..n+3 ->
// 16-byte fp32 / 8-byte 16-bit vector stores instead of 4 scalar ones per quad.
template <int EPI, bool F16>
__device__ __forceinline__ void epilogue_quad(const GemmArgs& g, int m, int n, const float v4[4]) {
    float b[4] = {0.f, 0.f, 0.f, 0.f};
    if (g.bias != nullptr) {
        const float4 bb = *reinterpret_cast<const float4*>(g.bias + n);
        b[0] = bb.x; b[1] = bb.y; b[2] = bb.z; b[3] = bb.w;
    }
    if (g.gbias != nullptr) {
        const float4 bb = *reinterpret_cast<const float4*>(g.gbias + (size_t)(m / g.gb_rows) * g.N + n);
        b[0] += bb.x; b[1] += bb.y; b[2] += bb.z; b[3] += bb.w;
    }
    if (EPI == EPI_QKV) {
        const int D = g.heads * 64;
        const int which = n / D, hn = n - which * D, h = hn >> 6, d = hn & 63;
        const int bidx = m / g.seq, t = m - bidx * g.seq;
        const int bh = bidx * g.heads + h;
        bf16_t* row_dst = which == 0 ? g.q : (which == 1 ? g.k : g.v);
        bf16_t* tr_dst = which == 0 ? g.qt : (which == 1 ? g.kt : g.vt);
        float e1[4] = {0.f, 0.f, 0.f, 0.f}, e2[4] = {0.f, 0.f, 0.f, 0.f};
        if (which == 0 && g.pu != nullptr) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { e1[j] = g.pu[h * 64 + d + j]; e2[j] = g.pv[h * 64 + d + j]; }
        }
        float val[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) val[j] = v4[j] + b[j];
        // backward-only tensors (row-major V, every transposed copy except V^T) may be requested as bf16 (g.bwd_bf16)
        const int row_bf = g.bwd_bf16 && which == 2, tr_bf = g.bwd_bf16 && which != 2;
        uint2 pk;
        pk.x = pack2_sel<F16>(val[0] + e1[0], val[1] + e1[1], row_bf);
        pk.y = pack2_sel<F16>(val[2] + e1[2], val[3] + e1[3], row_bf);
        if (row_dst != nullptr) *reinterpret_cast<uint2*>(&row_dst[((size_t)bh * g.seq + t) * 64 + d]) = pk;
        if (tr_dst != nullptr) {
#pragma unroll
            for (int j = 0; j < 4; ++j) tr_dst[((size_t)bh * 64 + d + j) * g.seq_pad + t] = to16_sel<F16>(val[j] + e1[j], tr_bf);
        }
        if (which == 0 && g.q2 != nullptr) {
            pk.x = pack2<F16>(val[0] + e2[0], val[1] + e2[1]);
            pk.y = pack2<F16>(val[2] + e2[2], val[3] + e2[3]);
            *reinterpret_cast<uint2*>(&g.q2[((size_t)bh * g.seq + t) * 64 + d]) = pk;
            if (g.q2t != nullptr) {
#pragma unroll
                for (int j = 0; j < 4; ++j) g.q2t[((size_t)bh * 64 + d + j) * g.seq_pad + t] = to16_sel<F16>(val[j] + e2[j], g.bwd_bf16);
            }
        }
        return;
    }
    const size_t o = (size_t)m * g.ldc + n;
    if (EPI == EPI_F32) {
        *reinterpret_cast<float4*>(g.outF + o) =
            make_float4(v4[0] * g.alpha + b[0], v4[1] * g.alpha + b[1], v4[2] * g.alpha + b[2], v4[3] * g.alpha + b[3]);
    } else if (EPI == EPI_F32_RESID) {
        const float4 r = *reinterpret_cast<const float4*>(g.resF + o);
        *reinterpret_cast<float4*>(g.outF + o) = make_float4(r.x + v4[0] + b[0], r.y + v4[1] + b[1], r.z + v4[2] + b[2], r.w + v4[3] + b[3]);
    } else if (EPI == EPI_BF16) {
        uint2 pk;
        pk.x = pack2<F16>(v4[0] + b[0], v4[1] + b[1]);
        pk.y = pack2<F16>(v4[2] + b[2], v4[3] + b[3]);
        *reinterpret_cast<uint2*>(g.outH + o) = pk;
    } else if (EPI == EPI_GELU) {
        float h[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) h[j] = v4[j] + b[j];
        uint2 pk;
        if (g.outH != nullptr) {  // pre-activation is only kept when a backward will need it
            pk.x = pack2_sel<F16>(h[0], h[1], g.bwd_bf16);
            pk.y = pack2_sel<F16>(h[2], h[3], g.bwd_bf16);
            *reinterpret_cast<uint2*>(g.outH + o) = pk;
        }
        pk.x = pack2<F16>(gelu_fast(h[0]), gelu_fast(h[1]));
        pk.y = pack2<F16>(gelu_fast(h[2]), gelu_fast(h[3]));
        *reinterpret_cast<uint2*>(g.outH2 + o) = pk;
    } else if (EPI == EPI_DGELU) {
        const uint2 a = *reinterpret_cast<const uint2*>(g.auxH + o);
        const float h0 = to_f32<F16>((bf16_t)(a.x & 0xFFFF)), h1 = to_f32<F16>((bf16_t)(a.x >> 16));
        const float h2 = to_f32<F16>((bf16_t)(a.y & 0xFFFF)), h3 = to_f32<F16>((bf16_t)(a.y >> 16));
        uint2 pk;
        pk.x = pack2<F16>(v4[0] * gelu_fast_grad(h0), v4[1] * gelu_fast_grad(h1));
        pk.y = pack2<F16>(v4[2] * gelu_fast_grad(h2), v4[3] * gelu_fast_grad(h3));
        *reinterpret_cast<uint2*>(g.outH + o) = pk;
    } else if (EPI == EPI_ATOMIC) {
#pragma unroll
        for (int j = 0; j < 4; ++j) unsafeAtomicAdd(&g.outF[o + j], v4[j] * g.alpha);
    } else if (EPI == EPI_F32_BF16) {
        *reinterpret_cast<float4*>(g.outF + o) = make_float4(v4[0] + b[0], v4[1] + b[1], v4[2] + b[2], v4[3] + b[3]);
        uint2 pk;
        pk.x = pack2<F16>(v4[0] + b[0], v4[1] + b[1]);
        pk.y = pack2<F16>(v4[2] + b[2], v4[3] + b[3]);
        *reinterpret_cast<uint2*>(g.outH + o) = pk;
    } else if (EPI == EPI_GELU32) {
        float h[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) h[j] = v4[j] + b[j];
        uint2 pk;
        pk.x = pack2_sel<F16>(h[0], h[1], g.bwd_bf16);
        pk.y = pack2_sel<F16>(h[2], h[3], g.bwd_bf16);
        *reinterpret_cast<uint2*>(g.outH + o) = pk;
        *reinterpret_cast<float4*>(g.outF + o) = make_float4(gelu_erf(h[0]), gelu_erf(h[1]), gelu_erf(h[2]), gelu_erf(h[3]));
    }
}

// MFMA phase over one 64-deep K tile for a wave's 2x2 accumulator blocks, with the LDS->register fragment loads of
// k-step s+1 issued BEFORE the four MFMAs of k-step s (register double buffering), so ds_read latency hides under MFMA
// issue instead of serialising "4 reads - wait - 4 MFMAs" per k-step.
template <bool F16, bool SWAP>
__device__ __forceinline__ void mfma_tile(const unsigned char* la, const unsigned char* lb, const int (&arow)[2],
                                          const int (&brow)[2], int lg, f32x16_t (&acc)[2][2]) {
    s16x8_t af[2][2], bfr[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        af[0][i] = *reinterpret_cast<const s16x8_t*>(la + arow[i] * 128 + ((lg ^ ((arow[i] >> 1) & 7)) << 4));
        bfr[0][i] = *reinterpret_cast<const s16x8_t*>(lb + brow[i] * 128 + ((lg ^ ((brow[i] >> 1) & 7)) << 4));
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int cur = s & 1, nxt = cur ^ 1;
        if (s < 3) {
            const int ch = 2 * (s + 1) + lg;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                af[nxt][i] = *reinterpret_cast<const s16x8_t*>(la + arow[i] * 128 + ((ch ^ ((arow[i] >> 1) & 7)) << 4));
                bfr[nxt][i] = *reinterpret_cast<const s16x8_t*>(lb + brow[i] * 128 + ((ch ^ ((brow[i] >> 1) & 7)) << 4));
            }
        }
        __builtin_amdgcn_sched_barrier(0);  // keep the prefetch ahead of the MFMAs (else the reads are sunk onto reused VGPRs)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = SWAP ? mfma32t<F16>(bfr[cur][j], af[cur][i], acc[i][j]) : mfma32t<F16>(af[cur][i], bfr[cur][j], acc[i][j]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <int EPI, bool F16>
__global__ __launch_bounds__(256) void gemm_nt_kernel(const GemmArgs g) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[2][2][TILE * BK * 2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int ntn = g.N / TILE, ntm = (g.M + TILE - 1) / TILE, nwg = ntm * ntn;
    // XCD-contiguous linear tile id, then "grouped" order inside it: 8 tile-rows x all tile-columns form a group whose
    // A panel (8 x 192 KB at K = 768) and B panel stay resident in the XCD's 4 MB L2 while its ~64 concurrent
    // workgroups sweep it (otherwise every tile-row re-streams the whole weight matrix: ~64 FLOP/B, bandwidth-bound).
    const int t = xcd_remap(blockIdx.x, nwg);
    const int group_size = 8 * ntn, gid = t / group_size, first_m = gid * 8;
    const int gm = (ntm - first_m) < 8 ? (ntm - first_m) : 8;
    const int tin = t - gid * group_size;
    const int m0 = (first_m + tin % gm) * TILE, n0 = (tin / gm) * TILE;
    const int ktiles = g.K / BK;
    const int kt_begin = (int)(((long long)blockIdx.y * ktiles) / g.ksplit);
    const int kt_end = (int)(((long long)(blockIdx.y + 1) * ktiles) / g.ksplit);

    f32x16_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // fragment read offsets (row part), chunk part depends on the k-step
    const int lr = lane & 31, lg = lane >> 5;
    int arow[2], brow[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        arow[i] = wm * 64 + i * 32 + lr;
        brow[i] = wn * 64 + i * 32 + lr;
    }

// split-K weight gradients keep the un-swapped accumulator layout (lane = output column): their atomics then hit 2 cache
// lines per instruction instead of 64
#define GEMM_COMPUTE(buf) mfma_tile<F16, EPI != EPI_ATOMIC>(lds[buf][0], lds[buf][1], arow, brow, lg, acc)
    // Direct-to-LDS staging (global_load_lds_dwordx4): each wave-instruction DMAs 64 x 16 B = 8 tile rows straight into LDS
    // (lane-linear destination), no VGPR round trip and no ds_write pass.  The XOR swizzle therefore sits on the per-lane SOURCE
    // address: lane l fills physical chunk l & 7 of row 8 p + (l >> 3) with logical chunk (l & 7) ^ ((row >> 1) & 7) -- the same
    // involution the fragment reads apply.  Wave w owns pieces 4 w .. 4 w + 3.
    const int prow = lane >> 3, pch = lane & 7;
    const bf16_t* asrc[4];
    const bf16_t* bsrc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = (wave * 4 + i) * 8 + prow;
        const int cl = pch ^ ((row >> 1) & 7);
        int am = m0 + row;
        am = am < g.M ? am : g.M - 1;
        asrc[i] = g.A + (size_t)am * g.lda + cl * 8;
        bsrc[i] = g.B + (size_t)(n0 + row) * g.ldb + cl * 8;
    }
#define GEMM_DMA(kt, buf)                                                                                                \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                      \
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(asrc[i] + (size_t)(kt) * BK),   \
                                         (__attribute__((address_space(3))) void*)(&lds[buf][0][(wave * 4 + i) * 1024]), \
                                         16, 0, 0);                                                                      \
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(bsrc[i] + (size_t)(kt) * BK),   \
                                         (__attribute__((address_space(3))) void*)(&lds[buf][1][(wave * 4 + i) * 1024]), \
                                         16, 0, 0);                                                                      \
    }
    if (kt_begin < kt_end) GEMM_DMA(kt_begin, 0);
    __syncthreads();  // (drains the LDS-DMA: hipcc emits vmcnt(0) before a barrier while one is in flight)
    for (int kt = kt_begin; kt < kt_end; ++kt) {
        const int buf = (kt - kt_begin) & 1;
        if (kt + 1 < kt_end) GEMM_DMA(kt + 1, buf ^ 1);
        GEMM_COMPUTE(buf);
        __syncthreads();
    }
    if (EPI == EPI_ATOMIC) {  // un-swapped: column = lane & 31, rows from the register index
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int n = n0 + wn * 64 + j * 32 + lr;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + wm * 64 + i * 32 + mfma32_row(r, lg);
                    if (m < g.M) unsafeAtomicAdd(&g.outF[(size_t)m * g.ldc + n], acc[i][j][r] * g.alpha);
                }
            }
        return;
    }
    // accumulator block (i, j) holds C^T: column index (lane & 31) = row m of C, register rows = columns n of C
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + wm * 64 + i * 32 + lr;
        if (m >= g.M) continue;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = n0 + wn * 64 + j * 32 + 8 * q + 4 * lg;
                if (n >= g.ncols) continue;
                const float v4[4] = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
                epilogue_quad<EPI, F16>(g, m, n, v4);
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// 256 x 256 x 64 workgroup tile, 8 waves (2 x 4), 128 x 64 per wave, "ping-pong" K loop on v_mfma_f32_16x16x32.
//
// Why this shape of loop (measured on MI355X, tools/ablate/pp_lab.hip, mfma_bench.hip, dma_bench.hip):
//  * The chip is POWER-limited in a dense GEMM on real data: the clock settles at 1.35-1.65 GHz (2.4 GHz on all-zero
//    operands), so TFLOP/s is set by energy per FLOP, not by issue slots.  v_mfma_f32_16x16x32 sustains ~1800 TFLOP/s on
//    random operands, v_mfma_f32_32x32x16 ~1550 (twice the accumulator read/write traffic per FLOP): the whole kernel moved
//    from 1270 to 1440 TFLOP/s at 8192^3 by changing the MFMA shape alone.  Fragment reads cost ~6 %, the DMA ~13 % of the energy.
//  * The two wave rows run half a phase apart.  A K tile is four phases; in each, a wave computes one 64 x 32 quadrant of its
//    sub-tile (4 x 2 blocks x 2 k-steps = 16 back-to-back MFMAs) between two workgroup barriers, and before the first of them
//    does its memory work: 2 direct-to-LDS DMA pieces of a later K tile and the fragment reads the coming quadrant needs (A half:
//    8 ds_read_b128, B half: 4).  Waves 4-7 execute one extra barrier up front, so on every SIMD one wave is in its MFMA section
//    while its partner issues DMA / LDS reads: 92 % MFMA-pipe occupancy in cycles, against two waves that stall on the same
//    `s_waitcnt lgkmcnt(0)` at the same time in a lock-step loop.
//  * Reads per phase are balanced 8/4/8/4: the next tile's B half 0 is read in P4 into the registers that B half 1 vacated after
//    P3, so the two B register sets swap roles every K tile (two tiles per loop trip).
// DMA plan for K tile t+1 (16 pieces of 8 rows x 128 B per slot, 2 per wave): B half-0 rows at P2(t-1), A half-0 rows at P3(t-1),
// B half-1 rows at P4(t-1), A half-1 rows at P1(t) -- each at least two barriers after the last read of the region it overwrites --
// retired by ONE counted `s_waitcnt vmcnt(4)` at P3(t) ahead of that phase's first barrier (the 4 youngest pieces belong to tile
// t+2); the first read of tile t+1 (its B half 0) is a phase later, in P4(t).
// Operands come through buffer descriptors: rows past M read as zeros, 32-bit lane offsets + an SGPR K offset.
// LDS: A stage s at s * 32 KiB, B stage s at 64 KiB + s * 32 KiB -> every fragment read is `vaddr + imm16`; the address registers
// flip bit 15 per K tile.  128-byte rows, 16-B chunk c of row r stored at chunk c ^ ((r >> 1) & 7) (applied on the DMA source
// address): conflict-free for the 16 x 32 fragment reads (lane & 15 = row, lane >> 4 = chunk inside the k-step).
// Accumulators: acc[i][j], i = 0..7 (16-row blocks), j = 0..3 (16-column blocks); the MFMA operands are issued swapped (B fragment
// first), so a block holds C^T: lane & 15 = row, register r = column 4 (lane >> 4) + r of the block's 16 weight rows -> a lane owns 4
// CONSECUTIVE columns of one row per block.  Which 16 output columns a block's weight rows are is the DMA's choice (round 4): PP_COL /
// PP_COL32 (gemm_args.h, gemm_epilogue.h) place them so that a lane's blocks form 16-byte runs that the epilogues store straight from the registers.
// ---------------------------------------------------------------------------------------------------------------------
// RB = 16-row blocks per wave row: 8 -> 256-row tiles; 7 -> 224-row tiles (the eighth block's reads, MFMAs and stores are skipped; its
// LDS rows are still filled so that every wave keeps the same DMA count for the counted waits).  With M = 38080 tokens on 256 CUs the
// N = 768 / 2304 GEMMs are 447 / 1341 tiles of 256 rows = 1.75 / 5.24 rounds, i.e. 2 / 6 rounds with 13 % of the last ones empty; as
// 510 / 1530 tiles of 224 rows they are 1.99 / 5.98 rounds of tiles that are 12.5 % shorter -- pp_geometry picks the cheaper height.
typedef int i32x8_t __attribute__((ext_vector_type(8)));
__device__ __forceinline__ i32x8_t cat32(s16x8_t a, s16x8_t b) {
    typedef int i32x4_t __attribute__((ext_vector_type(4)));
    const i32x4_t x = __builtin_bit_cast(i32x4_t, a), y = __builtin_bit_cast(i32x4_t, b);
    return i32x8_t{x[0], x[1], x[2], x[3], y[0], y[1], y[2], y[3]};
}
// The F8 variants pin their accumulators: with the compiler's untied MFMA forms (vdst != srcC allowed) and 250 of 256 registers in use
// the allocator moved accumulator tuples between K tiles and spilled some (scratch reloads behind s_waitcnt vmcnt(0): the end of the DMA
// pipeline).  Tied inline-asm forms leave it nothing to move.  Back-to-back accumulation into the same vdst needs no wait states; the
// epilogue's first VALU read of an accumulator is kept >= 18 cycles behind the last MFMA by hand (pp kernel, after the K loop).
__device__ __forceinline__ void mfma16_f16_tied(f32x4_t& c, s16x8_t a, s16x8_t b) {
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}
__device__ __forceinline__ void mfma128_e4m3_tied(f32x4_t& c, i32x8_t a, i32x8_t b, int sc) {
    asm volatile("v_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, %0, %3, %3 op_sel_hi:[0,0,0]" : "+v"(c) : "v"(a), "v"(b), "v"(sc));
}
template <int EPI, bool F16, int V = PP_PLAIN, int RB = 8, bool F8 = false>
__global__ __launch_bounds__(512) void gemm_nt_pp_kernel(const GemmArgs g) {
    using T = PpTraits<V, F8>;
    constexpr int TM = 32 * RB;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds3[];
#ifdef GX_TRACE
    const unsigned long long gx_top = __builtin_amdgcn_s_memrealtime();
#endif
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int ntn = g.N / V3_T, ntm = (g.M + TM - 1) / TM, nwg = ntm * ntn;
    // Persistent form: gridDim.x = number of CUs, every workgroup walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ... (gridDim.x is
    // a multiple of 8, so a workgroup's tiles stay on its XCD and the L2 grouping below is unchanged).  Measured per 256^2 tile with
    // one launch per tile: 1.6 us between the last store of a workgroup and the first instruction of the next one on that CU plus
    // 0.5 us of kernel-argument / address setup (tools/epi_gaps.py) against a 17 us K = 768 main loop.
    const int tstep = g.persist ? (int)gridDim.x : nwg;
    if (g.stagger > 0) {
        // (stagger >> 16 = number of phase groups P, default 2; workgroup i of an XCD starts (i mod P) / P * ticks late)
        const int P = (g.stagger >> 16) ? (g.stagger >> 16) : 2, ticks = g.stagger & 0xFFFF;
        const unsigned long long dly = (unsigned long long)(((blockIdx.x >> 3) % P) * ticks / P) * (P == 2 ? 2 : 1);
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        while (__builtin_amdgcn_s_memrealtime() - t0 < dly) __builtin_amdgcn_s_sleep(16);
    }
    // Dynamic walk (g.tile_ctr): the logical tiles tl with tl & 7 == x are XCD x's contiguous range (xcd_remap); index k of that range
    // comes from the per-XCD counter.  The counter for tile i + 1 is read at the top of tile i (one lane) and handed to the other waves
    // through one LDS word after the prologue barrier, so the ~1 us of a device-scope atomic is never waited for.
    __shared__ int s_next_tile;
    int* const dyn_ctr = g.tile_ctr != nullptr ? g.tile_ctr + 16 * (blockIdx.x & 7) : nullptr;
    int tl = blockIdx.x;
    if (dyn_ctr != nullptr) {
        if (tid == 0) s_next_tile = atomicAdd(dyn_ctr, 1);
        __syncthreads();
        tl = __builtin_amdgcn_readfirstlane(s_next_tile) * 8 + (blockIdx.x & 7);
    }
    // Epilogues that store straight from the accumulators leave the LDS alone: the next tile's first operand stage is requested BEFORE
    // the epilogue (its DMA lands under the stores) and the end-of-tile workgroup barrier goes away.
    constexpr bool DIRECT_EPI = T::direct_epi(EPI);
    constexpr bool F32L = T::f32_direct(EPI);      // PP_COL32 column order
    auto tile_mn = [&](int tl_, int& m0_, int& n0_) {
        const int t = xcd_remap(tl_, nwg);
        const int GM = g.group_m;
        const int group_size = GM * ntn, gid = t / group_size, first_m = gid * GM;
        const int gm = (ntm - first_m) < GM ? (ntm - first_m) : GM;
        const int tin = t - gid * group_size;
        m0_ = (first_m + tin % gm) * TM;
        n0_ = (tin / gm) * V3_T;
    };
    bool primed = false;      // this tile's K-tile-0 DMA was issued by the previous tile
    int m0n = 0, n0n = 0;
    while (tl < nwg) {
    int m0, n0;
    if (primed) { m0 = m0n; n0 = n0n; } else tile_mn(tl, m0, n0);
    const int nk = g.K / BK;

    const int rows_a = (g.M - m0) < TM ? (g.M - m0) : TM;
    // (slab-major A, GemmArgs.a_slab: row pitch 128 bytes, K tile kt at kt * M * 128; rows past M read the next slab -- they only reach
    //  accumulator rows that are never stored -- and nothing is read past the last slab's end)
    const bool a_slab = T::slab_a ? g.a_slab != 0 : false;
    const int a_ld2 = a_slab ? 128 : g.lda * 2, a_kst = a_slab ? g.M * 128 : BK * 2;
    const __amdgpu_buffer_rsrc_t ra = a_slab
        ? __builtin_amdgcn_make_buffer_rsrc((void*)(g.A + (size_t)m0 * 64), 0, (unsigned)((size_t)(g.K / BK) * g.M * 128 - (size_t)m0 * 128), 0x00020000)
#ifdef ABL_A_ALIAS   /* experiment (tools/ablate): every row panel reads the first 1024 rows of A -- the operand then lives in L2, results are wrong */
        : __builtin_amdgcn_make_buffer_rsrc((void*)(g.A + (size_t)(m0 % 1024) * g.lda), 0, rows_a * g.lda * 2, 0x00020000);
#else
        : __builtin_amdgcn_make_buffer_rsrc((void*)(g.A + (size_t)m0 * g.lda), 0, rows_a * g.lda * 2, 0x00020000);
#endif
    const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)(g.B + (size_t)n0 * g.ldb), 0, V3_T * g.ldb * 2, 0x00020000);
    // DMA pieces of this wave: slot piece index p = 2 wave + e.  Slot 0 = A rows of half 0 (wave-row * 128 + 0..63), slot 3 = A rows
    // of half 1, slot 1 = B rows of half 0 (wave-column * 64 + 0..31), slot 2 = B rows of half 1
    const int prow = lane >> 3, pch = lane & 7;
    int vo[4][2];      // lane byte offsets into the A / B row panels, [slot][e]
    int ld_[4][2];     // LDS byte offsets (stage bit 15 added at issue)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int p = 2 * wave + e;
        const int ra0 = (p >> 3) * 128 + (p & 7) * 8, ra1 = ra0 + 64;
        const int rb0 = (p >> 2) * 64 + (p & 3) * 8, rb1 = rb0 + 32;
        const int rows[4] = {ra0, rb0, rb1, ra1};
#pragma unroll
        for (int sl = 0; sl < 4; ++sl) {
            const int row = rows[sl] + prow;
            const int cl = pch ^ ((row >> 1) & 7);
            const bool is_b = (sl == 1 || sl == 2);
            // LDS row wm * 128 + r of the A stage holds tile row wm * 16 RB + r (r >= 16 RB: a row nobody reads)
            const int grow = is_b ? (F32L ? pp_brow_src32(row) : pp_brow_src(row)) : (row >> 7) * (16 * RB) + (row & 127);
            vo[sl][e] = grow * (is_b ? g.ldb * 2 : a_ld2) + cl * 16;
            ld_[sl][e] = (is_b ? 65536 : 0) + rows[sl] * 128;
        }
    }
#define PP_DMA_R(RA_, RB_, SL, KT)                                                                                        \
    {                                                                                                                     \
        const int kt_ = (T::two_term_walk && (KT) >= g.k_wrap) ? (((SL) == 0 || (SL) == 3) ? (KT) - g.k_wrap : (KT) + g.b_skip) : (KT);              \
        const int so_ = kt_ * (((SL) == 1 || (SL) == 2) ? BK * 2 : a_kst), st_ = ((KT) & 1) << 15;                        \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(((SL) == 1 || (SL) == 2) ? RB_ : RA_, (lds_ptr_t)(lds3 + st_ + ld_[SL][0]), 16, vo[SL][0], so_, 0, 0); \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(((SL) == 1 || (SL) == 2) ? RB_ : RA_, (lds_ptr_t)(lds3 + st_ + ld_[SL][1]), 16, vo[SL][1], so_, 0, 0); \
    }
#define PP_DMA(SL, KT) PP_DMA_R(ra, rb, SL, KT)
    f32x4_t acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // fragment addresses: every block's rows are (lane & 15) + a multiple of 16, so one swizzle serves all of them
    const int l15 = lane & 15, lq = lane >> 4, sw = (l15 >> 1) & 7;
    int aaddr[2], baddr[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const int c = ((4 * ks + lq) ^ sw) << 4;
        aaddr[ks] = wm * 16384 + l15 * 128 + c;
        baddr[ks] = 65536 + wn * 8192 + l15 * 128 + c;
    }
    V3Consts<EPI> cc;
    v3_load_consts<EPI>(cc, g, n0 + wn * 64, lane);

    s16x8_t fa[4][2], fb[2][2][2];   // fa[ii][ks]: 4 row blocks of the current A half; fb[set][jj][ks]: 2 column blocks of a B half
#define PP_RD_A(IH)                                                                                                       \
    _Pragma("unroll") for (int ii = 0; ii < ((IH) == 1 ? RB - 4 : 4); ++ii)                                               \
        _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                                  \
            fa[ii][ks] = *reinterpret_cast<const s16x8_t*>(lds3 + aaddr[ks] + (4 * (IH) + ii) * 2048);
#define PP_RD_B(SET, JH, XOR)                                                                                             \
    _Pragma("unroll") for (int jj = 0; jj < 2; ++jj)                                                                      \
        _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                                  \
            fb[SET][jj][ks] = *reinterpret_cast<const s16x8_t*>(lds3 + (baddr[ks] ^ (XOR)) + (2 * (JH) + jj) * 2048);
#define PP_MFMA(IH, JH, SET)                                                                                              \
    __builtin_amdgcn_sched_barrier(0);                                                                                    \
    __builtin_amdgcn_s_barrier();                                                                                         \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                                                    \
    _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                                      \
        _Pragma("unroll") for (int ii = 0; ii < ((IH) == 1 ? RB - 4 : 4); ++ii)                                           \
            _Pragma("unroll") for (int jj = 0; jj < 2; ++jj) {                                                            \
                if constexpr (F8) mfma16_f16_tied(acc[4 * (IH) + ii][2 * (JH) + jj], fb[SET][jj][ks], fa[ii][ks]);           \
                else acc[4 * (IH) + ii][2 * (JH) + jj] = mfma16<F16>(fb[SET][jj][ks], fa[ii][ks], acc[4 * (IH) + ii][2 * (JH) + jj]); \
            }                                                                                                             \
    __builtin_amdgcn_sched_barrier(0);                                                                                    \
    __builtin_amdgcn_s_barrier();                                                                                         \
    __builtin_amdgcn_sched_barrier(0);
    // fp8 K tile (F8): the two 16-byte fragments of a row block are one 32-byte e4m3 operand
#define PP_MFMA8(IH, JH, SET)                                                                                             \
    __builtin_amdgcn_sched_barrier(0);                                                                                    \
    __builtin_amdgcn_s_barrier();                                                                                         \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                                                    \
    _Pragma("unroll") for (int ii = 0; ii < ((IH) == 1 ? RB - 4 : 4); ++ii)                                               \
        _Pragma("unroll") for (int jj = 0; jj < 2; ++jj)                                                                  \
            mfma128_e4m3_tied(acc[4 * (IH) + ii][2 * (JH) + jj], cat32(fb[SET][jj][0], fb[SET][jj][1]), cat32(fa[ii][0], fa[ii][1]), f8s); \
    __builtin_amdgcn_sched_barrier(0);                                                                                    \
    __builtin_amdgcn_s_barrier();                                                                                         \
    __builtin_amdgcn_sched_barrier(0);
    // one K tile; X = B register set holding this tile's half 0, Y = the other set
#define PP_TILE_(MF, T_, X, Y)                                                                                            \
    if ((T_) + 1 < nk) PP_DMA(3, (T_) + 1)                                                                                \
    PP_RD_A(0)                                                                                                            \
    MF(0, 0, X)                                                                                                           \
    if ((T_) + 2 < nk) PP_DMA(1, (T_) + 2)                                                                                \
    PP_RD_B(Y, 1, 0)                                                                                                      \
    MF(0, 1, Y)                                                                                                           \
    if ((T_) + 2 < nk) { PP_DMA(0, (T_) + 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); }                           \
    else { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }                                                             \
    PP_RD_A(1)                                                                                                            \
    MF(1, 1, Y)                                                                                                           \
    if ((T_) + 2 < nk) PP_DMA(2, (T_) + 2)                                                                                \
    if ((T_) + 1 < nk) { PP_RD_B(Y, 0, 0x8000) }                                                                          \
    MF(1, 0, X)                                                                                                           \
    _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) { aaddr[ks] ^= 0x8000; baddr[ks] ^= 0x8000; }
#define PP_TILE(T_, X, Y) PP_TILE_(PP_MFMA, T_, X, Y)
#define PP_TILE8(T_, X, Y) PP_TILE_(PP_MFMA8, T_, X, Y)

#ifdef GX_TRACE
    unsigned long long gx_t[8];
    gx_t[0] = __builtin_amdgcn_s_memrealtime();
#define GX_STAMP(i) gx_t[i] = __builtin_amdgcn_s_memrealtime();
#else
#define GX_STAMP(i)
#endif
    // prologue: all of tile 0; then the three slots of tile 1 that the steady state would have issued during tile -1
    int dyn_nxt = 0;
    if (dyn_ctr != nullptr && tid == 0) dyn_nxt = atomicAdd(dyn_ctr, 1);     // next tile's index: returns under the prologue's DMA
    if (!primed) { PP_DMA(1, 0) PP_DMA(0, 0) PP_DMA(2, 0) PP_DMA(3, 0) }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (dyn_ctr != nullptr && tid == 0) s_next_tile = dyn_nxt;     // (everybody read the previous value before this barrier; read again after the tile's last one)
    GX_STAMP(1)
    if (nk > 1) { PP_DMA(1, 1) PP_DMA(0, 1) PP_DMA(2, 1) }
    if (wm == 1) __builtin_amdgcn_s_barrier();   // second wave row: half a phase behind
    PP_RD_B(0, 0, 0)
    int it = 0;
    if constexpr (F8) {
        const int f8s = g.f8_scale;
        const int nk16 = nk - g.k8;          // even (K % 128 == 0)
        for (; it < nk16; it += 2) {
            PP_TILE(it, 0, 1)
            PP_TILE(it + 1, 1, 0)
        }
        for (; it + 1 < nk; it += 2) {
            PP_TILE8(it, 0, 1)
            PP_TILE8(it + 1, 1, 0)
        }
        if (it < nk) { PP_TILE8(it, 0, 1) }
        asm volatile("s_nop 15\n\ts_nop 3" ::: "memory");      // last (16-pass) MFMA -> the epilogue's accumulator reads
    } else {
    for (; it + 1 < nk; it += 2) {
        PP_TILE(it, 0, 1)
        PP_TILE(it + 1, 1, 0)
    }
    if (it < nk) { PP_TILE(it, 0, 1) }
    }
    GX_STAMP(2)
    if (wm == 0) __builtin_amdgcn_s_barrier();   // pairs with the last barrier of waves 4-7: nobody reads the stages any more
    GX_STAMP(3)
    // next tile (the K loop's last barrier is behind every wave: the operand stages are free and s_next_tile holds the next index)
    int tl_next = tl + tstep;
    primed = false;
    if constexpr (DIRECT_EPI) {
        if (dyn_ctr != nullptr) tl_next = __builtin_amdgcn_readfirstlane(s_next_tile) * 8 + (blockIdx.x & 7);
        if (tl_next < nwg) {
            tile_mn(tl_next, m0n, n0n);
            const int rows_n = (g.M - m0n) < TM ? (g.M - m0n) : TM;
            const __amdgpu_buffer_rsrc_t ran = a_slab
                ? __builtin_amdgcn_make_buffer_rsrc((void*)(g.A + (size_t)m0n * 64), 0, (unsigned)((size_t)(g.K / BK) * g.M * 128 - (size_t)m0n * 128), 0x00020000)
                : __builtin_amdgcn_make_buffer_rsrc((void*)(g.A + (size_t)m0n * g.lda), 0, rows_n * g.lda * 2, 0x00020000);
            const __amdgpu_buffer_rsrc_t rbn = __builtin_amdgcn_make_buffer_rsrc((void*)(g.B + (size_t)n0n * g.ldb), 0, V3_T * g.ldb * 2, 0x00020000);
            PP_DMA_R(ran, rbn, 1, 0) PP_DMA_R(ran, rbn, 0, 0) PP_DMA_R(ran, rbn, 2, 0) PP_DMA_R(ran, rbn, 3, 0)
            primed = true;
        }
    }
#undef PP_DMA
#undef PP_DMA_R
#undef PP_RD_A
#undef PP_RD_B
#undef PP_MFMA
#undef PP_MFMA8
#undef PP_TILE
#undef PP_TILE8
#undef PP_TILE_
#ifdef GX_TRACE
    pp_epilogue<EPI, F16, V, RB, F8>(g, acc, cc, lds3 + wave * V3_WLDS, m0 + wm * (16 * RB), n0 + wn * 64, lane, gx_t);
    GX_STAMP(5)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    GX_STAMP(6)
    if constexpr (EPI == EPI_BF16 || EPI == EPI_GELU) {
        // developer trace: stamps of every wave of workgroups 0, 100 and 300 behind the output matrix (tools/epi_trace.py)
        const int slot = blockIdx.x == 0 ? 0 : (blockIdx.x == 100 ? 1 : (blockIdx.x == 300 ? 2 : -1));
        if (slot >= 0 && lane == 0) {
            unsigned long long* tr = reinterpret_cast<unsigned long long*>((EPI == EPI_GELU ? g.outH2 : g.outH) + (size_t)g.M * g.ldc) + (slot * 8 + wave) * 8;
#pragma unroll
            for (int i = 0; i < 7; ++i) tr[i] = gx_t[i];
        }
        // every workgroup: (hardware id, first instruction, entry stamp, last store acknowledged) of wave 0 -> occupancy gaps per CU
        if (wave == 0 && lane == 0) {
            unsigned long long* wr = reinterpret_cast<unsigned long long*>((EPI == EPI_GELU ? g.outH2 : g.outH) + (size_t)g.M * g.ldc) + 256 + 4 * blockIdx.x;
            unsigned hw, xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            wr[0] = ((unsigned long long)xcc << 32) | hw;
            wr[1] = gx_top; wr[2] = gx_t[0]; wr[3] = gx_t[6];
        }
    }
#else
    pp_epilogue<EPI, F16, V, RB, F8>(g, acc, cc, lds3 + wave * V3_WLDS, m0 + wm * (16 * RB), n0 + wn * 64, lane);
#endif
    if constexpr (DIRECT_EPI) {
        tl = tl_next;                        // (no barrier: nothing of this tile is left in the LDS)
    } else if (dyn_ctr != nullptr) {
        __syncthreads();                     // (also orders the epilogue's staging reads before the next tile's DMA)
        tl = __builtin_amdgcn_readfirstlane(s_next_tile) * 8 + (blockIdx.x & 7);
    } else {
        tl += tstep;
        if (tl < nwg) __syncthreads();       // the staging areas overlap the operand stages the next tile's DMA is about to fill
    }
    }
    if (dyn_ctr != nullptr && tid == 0) {
        // last workgroup out re-arms the slot for its next user (every tile-counter atomic of a workgroup has returned before its exit atomic)
        int* const base = g.tile_ctr;
        if (atomicAdd(base + 16 * 8, 1) == (int)gridDim.x - 1) {
#pragma unroll
            for (int x = 0; x <= 8; ++x) atomicExch(base + 16 * x, 0);
        }
    }
}

// Counter slots of the dynamic tile walk: a ring in device memory (zero at module load, every launch leaves its slot zeroed again), one
// slot per launch so that GEMMs running concurrently on different streams never share counters.  A slot comes round again after
// DYN_SLOTS launches -- far more than a stream queue holds.
#define DYN_SLOTS 2048
#define DYN_SLOT_INTS (16 * 9)
__device__ int g_tile_counters[DYN_SLOTS * DYN_SLOT_INTS];
static int* dyn_counter_slot() {
    static int* base[64] = {};
    static std::atomic<unsigned> next{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    if (base[dev] == nullptr) {
        void* p = nullptr;
        if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_tile_counters)) != hipSuccess) return nullptr;
        base[dev] = (int*)p;
    }
    return base[dev] + (size_t)(next.fetch_add(1) % DYN_SLOTS) * DYN_SLOT_INTS;
}
// Number of CUs the persistent GEMM kernels size their grids for.  Default: all of them.  A data-parallel job whose collectives run
// beside the backward (ddp.py) reserves the communication kernels' CUs by lowering it (sed_gemm_set_cu_budget / SED_GEMM_CUS): a
// persistent workgroup that cannot become resident beside a communication kernel would otherwise start only after another one has exited.
static std::atomic<int> g_cu_budget{0};
int gemm_cu_budget() {
    static int ncu_device = 0;      // (each process owns one device)
    if (ncu_device == 0) {
        int dev = 0, n = 0;
        (void)hipGetDevice(&dev);
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        ncu_device = n;
    }
    int b = g_cu_budget.load();
    if (b <= 0) {
        const char* e = getenv("SED_GEMM_CUS");
        b = e ? atoi(e) : 0;
    }
    if (b <= 0 || b > ncu_device) b = ncu_device;
    return b < 8 ? 8 : b;
}
// Measurement aid (tools/cu_steal.py): `n` single-wave workgroups, one per CU (81 KiB of LDS each: two cannot share a CU), that hold their
// CUs for `usec` microseconds doing nothing -- a stand-in for the RCCL kernels of a data-parallel step, whose workgroups keep a persistent
// GEMM workgroup (the whole register file of a CU) from becoming resident next to them.
__global__ __launch_bounds__(64) void hold_cus_kernel(unsigned long long ticks, int* sink) {
    extern __shared__ unsigned char hold_lds[];
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
    if (sink != nullptr && threadIdx.x == 1000) sink[0] = hold_lds[0];
}
extern "C" int sed_debug_hold_cus(int n_cus, int usec, hipStream_t stream) {
    (void)hipGetLastError();
    if (n_cus <= 0 || usec <= 0) return SED_ERR_ARG;
    static bool attr = false;
    launch_big_lds(attr, hold_cus_kernel, dim3(n_cus), dim3(64), 81 * 1024, stream, (unsigned long long)usec * 100ull, (int*)nullptr);
    return sed_check_launch();
}
// Test aid: number of non-zero words in the counter ring of the current device after a device synchronisation (must be 0 whenever no GEMM
// is in flight: every launch re-arms its slot).  Returns the count (>= 0) or a negative error code.
extern "C" int sed_debug_tile_counters_dirty(int reserved) {
    (void)reserved;
    if (hipDeviceSynchronize() != hipSuccess) return SED_ERR_LAUNCH;
    static int host[DYN_SLOTS * DYN_SLOT_INTS];
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_tile_counters), sizeof(host)) != hipSuccess) return SED_ERR_LAUNCH;
    int dirty = 0;
    for (int i = 0; i < DYN_SLOTS * DYN_SLOT_INTS; ++i) dirty += host[i] != 0;
    return dirty;
}
extern "C" int sed_gemm_set_cu_budget(int n_cus) {
    g_cu_budget.store(n_cus > 0 ? n_cus : 0);
    return SED_OK;
}

// ---- host side of the 256^2 kernel: geometry (pp_geometry), kernel selection (pp_select<EPI>), launch (pp_launch<...>) ----
// Fills the launch-geometry fields of g (group_m, persist, tile_ctr) and returns the grid; use7 = 224-row tiles.
static unsigned pp_geometry(GemmArgs& g, bool& use7) {
    // L2 grouping: 4 tile rows x all tile columns per group, groups XCD-contiguous.  Swept 2..32 on the model's shapes
    // (tools/gemm_l2.py): fabric reads stay at 1.4-2.3x (N = 768) / ~5x (N = 3072) of the algorithmic operand bytes for every
    // height -- column tiles of one row panel drift apart by more than the ~2 K-steps a line survives in the 4 MB L2 and re-read it
    // from the Infinity Cache -- while the time is best at 4 (fc2 1186 vs 998 TFLOP/s at 2): the counter does not track the time.
    g.group_m = 4;
    // SED_GEMM_RB (read per launch): 7 / 8 force a tile height (A/B and the bit-exactness test), 0 = choose by the round count below.
    // Default 8: alone on the GPU the 224-row form wins 3-4 % on the N = 768 shapes, but inside the train step the teacher's and the
    // weight-gradient streams fill the last round's idle CUs anyway and the shorter tiles cost 0.25 % (104.03 vs 103.77 ms, 3 A/B pairs).
    const char* rb_s = getenv("SED_GEMM_RB");
    const int rb_env = rb_s ? atoi(rb_s) : 8;
    const int ncu = gemm_cu_budget() & ~7;   // whole XCD rounds: blockIdx.x & 7 must stay the XCD of every tile a workgroup walks
    // Tile height: rounds of workgroups x rows per tile is what the launch costs; 224-row tiles win when they fill the last round
    // that 256-row tiles leave mostly empty (M = 38080: 2 x 256 vs 2 x 224 for N = 768, 6 x 256 vs 6 x 224 for N = 2304).
    // (the row-group-bias and two-term variants exist with 256-row tiles only)
    const int ntn = g.N / V3_T;
    const long long t8 = (long long)cdiv(g.M, 256) * ntn, t7 = (long long)cdiv(g.M, 224) * ntn;
    const long long c8 = ((t8 + ncu - 1) / ncu) * 256, c7 = ((t7 + ncu - 1) / ncu) * 224;
    use7 = g.gbias == nullptr && g.k_wrap == 0 && g.k8 == 0 && (rb_env == 7 || (rb_env == 0 && c7 * 100 < c8 * 97));
    // Persistent form whenever there are more tiles than CUs (one workgroup per tile lost its A/B in round 3 and has no switch any more)
    const unsigned tiles = (unsigned)(use7 ? t7 : t8);
    g.persist = (int)tiles > ncu ? 1 : 0;
    // SED_GEMM_DYN (read per launch; default 1): dynamic tile walk of the persistent form, 0 = the static walk (bit-identical results)
    const char* dy = getenv("SED_GEMM_DYN");
    g.tile_ctr = (g.persist && !(dy && atoi(dy) == 0)) ? dyn_counter_slot() : nullptr;
    return g.persist ? (unsigned)ncu : tiles;
}

// Launch of one instantiation (launch_big_lds: gemm_args.h).
typedef void (*PpLaunch)(const GemmArgs&, unsigned, hipStream_t);
template <int EPI, bool F16, int V, int RB = 8, bool F8 = false>
static void pp_launch(const GemmArgs& g, unsigned grid, hipStream_t s) {
    static bool attr = false;
    launch_big_lds(attr, gemm_nt_pp_kernel<EPI, F16, V, RB, F8>, dim3(grid, 1), dim3(512), V3_LDS, s, g);
}
template <int EPI, bool F16, int V>
static PpLaunch pp_tile_height(bool use7) { return use7 ? &pp_launch<EPI, F16, V, 7> : &pp_launch<EPI, F16, V, 8>; }
template <int EPI, int V>
static PpLaunch pp_type_and_height(int f16, bool use7) { return f16 ? pp_tile_height<EPI, true, V>(use7) : pp_tile_height<EPI, false, V>(use7); }

// The kernel a 256^2 launch goes to, or nullptr for an argument set no variant serves.  A pure function of its arguments; the variant
// table is beside PP_PLAIN.  (use7 is false whenever gbias, k_wrap or k8 is set: pp_geometry.)
template <int EPI>
static PpLaunch pp_select(const GemmArgs& g, int f16, bool use7) {
    constexpr bool ENC = EPI == EPI_F32_RESID || EPI == EPI_GELU || EPI == EPI_QKV;      // the epilogues the special variants exist for
    if ((long long)g.lda * 2 * V3_T >= (1LL << 31) || (long long)g.ldb * 2 * V3_T >= (1LL << 31)) return nullptr;  // 32-bit panel offsets
    // head split with row-major q / k / v only: no transposed copies, no biased second q, no pos_u
    const bool rows_only = g.qt == nullptr && g.kt == nullptr && g.vt == nullptr && g.q2 == nullptr && g.q2t == nullptr && g.pu == nullptr;
    const int nk = g.K / BK;
    if (g.rowpart != nullptr || g.rowstat != nullptr) {
        // folded LayerNorm: producer (residual epilogue) or consumer (head-split / fused-GELU epilogue); f16, no other special mode
        if constexpr (ENC) {
            if (!f16 || g.gbias != nullptr || g.k_wrap != 0 || (g.N & 63)) return nullptr;
            if constexpr (EPI == EPI_F32_RESID) {
                if (g.rowpart == nullptr || g.outH == nullptr || g.rowstat != nullptr) return nullptr;
                if (g.res_lo != nullptr && g.lo8) return g.out_lo != nullptr ? pp_tile_height<EPI, true, PP_LN_PLANES8>(use7) : pp_tile_height<EPI, true, PP_LN_PLANES8_F32OUT>(use7);
                if (g.res_lo != nullptr) return pp_tile_height<EPI, true, PP_LN_PLANES16>(use7);
            } else {
                if (g.rowstat == nullptr || g.colS == nullptr || g.rowpart != nullptr) return nullptr;
            }
            return pp_tile_height<EPI, true, PP_LN>(use7);
        }
        return nullptr;
    }
    if (g.k8 != 0) {
        // two-term weights, lo product on the fp8 matrix path: the two-term variants' epilogues behind a K walk of f16 tiles followed by
        // e4m3 tiles (an even number of f16 tiles, at least one)
        if constexpr (ENC) {
            if (!f16 || g.gbias != nullptr || g.k_wrap != 0 || g.a_slab || ((nk - g.k8) & 1) || g.k8 >= nk) return nullptr;
            if constexpr (EPI == EPI_QKV) return rows_only ? &pp_launch<EPI, true, PP_TWO_TERM_QKV_ROWS, 8, true> : nullptr;
            else return &pp_launch<EPI, true, PP_TWO_TERM, 8, true>;
        }
        return nullptr;
    }
    if (g.gbias != nullptr || g.k_wrap != 0) {
        // row-group bias / two-term weights: evaluation-mode encoder GEMMs only (f16 operands)
        if constexpr (ENC) {
            if (!f16 || (g.gbias != nullptr && g.k_wrap != 0)) return nullptr;
            if constexpr (EPI == EPI_QKV) if (g.k_wrap != 0 && rows_only) return &pp_launch<EPI, true, PP_TWO_TERM_QKV_ROWS>;
            if constexpr (EPI == EPI_GELU) if (g.out_e4m3) {
                // row-group bias + the e4m3 image of the output (fc1 of the evaluation-mode encoder in its fp8 form: f16 weights + mean
                // correction, the activation leaves as fc2's two-image A operand): the F8 kernel with no fp8 K tiles
                return (g.k_wrap != 0 || (nk & 1)) ? nullptr : &pp_launch<EPI, true, PP_GROUP_BIAS, 8, true>;
            }
            return g.k_wrap != 0 ? &pp_launch<EPI, true, PP_TWO_TERM> : &pp_launch<EPI, true, PP_GROUP_BIAS>;
        }
        return nullptr;
    }
    // the encoder's form of the head split (its attention kernels transpose in LDS): a kernel without the other outputs' paths, 3 % faster
    // than carrying them as run-time branches
    if constexpr (EPI == EPI_QKV) if (rows_only) return pp_type_and_height<EPI, PP_QKV_ROWS>(f16, use7);
    return pp_type_and_height<EPI, PP_PLAIN>(f16, use7);
}

template <int EPI>
static int launch_gemm(const GemmArgs& g, int f16, hipStream_t s) {
    if (g.M <= 0 || g.N % TILE != 0 || g.K % BK != 0 || g.ksplit < 1) return SED_ERR_ARG;
    if ((g.lda % 8) || (g.ldb % 8) || (g.ldc % 4)) return SED_ERR_ARG;
    // 256^2 kernel: every forward / dX GEMM of the model (N % 256 == 0, M >= 1024).  The split-K weight-gradient GEMMs of the NT
    // form stay on the 128^2 kernel (two workgroups per CU cover its atomic epilogue).
    if constexpr (EPI != EPI_ATOMIC) if (g.N % V3_T == 0 && g.M >= 1024 && g.ksplit == 1) {
        GemmArgs gg = g;
        bool use7 = false;
        const unsigned grid = pp_geometry(gg, use7);
        const PpLaunch launch = pp_select<EPI>(gg, f16, use7);
        if (launch == nullptr) return SED_ERR_ARG;
        launch(gg, grid, s);
        return sed_check_launch();
    }
    if (g.k_wrap != 0 || g.k8 != 0 || g.rowpart != nullptr || g.rowstat != nullptr) return SED_ERR_ARG;   // 256^2-kernel-only modes (N % 256 == 0, M >= 1024)
    dim3 grid(cdiv(g.M, TILE) * (g.N / TILE), g.ksplit);
    if (f16) hipLaunchKernelGGL((gemm_nt_kernel<EPI, true>), grid, dim3(256), 0, s, g);
    else hipLaunchKernelGGL((gemm_nt_kernel<EPI, false>), grid, dim3(256), 0, s, g);
    return sed_check_launch();
}

// The fields every builder below sets the same way: operands, extents and pitches; one K split, alpha 1, every output column written
static GemmArgs gemm_args(const void* A, const void* B, int M, int N, int K, int lda, int ldb, int ldc) {
    GemmArgs g = {};
    g.A = (const bf16_t*)A; g.B = (const bf16_t*)B;
    g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc;
    g.ksplit = 1; g.alpha = 1.f; g.ncols = N;
    return g;
}
static int gemm_nt_impl(const void* A, const void* B, int M, int N, int K, int lda, int ldb, int epi, const float* bias,
                        const float* resF, float* outF, void* outH, void* outH2, const void* auxH, int ldc, float alpha,
                        int ksplit, int f16, int ncols, hipStream_t stream, const float* gbias = nullptr, int gb_rows = 0, int two_term = 0,
                        int f8_scale = 0, int out_e4m3 = 0) {
    (void)hipGetLastError();
    if (out_e4m3 && ((two_term != 3 && gbias == nullptr) || epi != EPI_GELU || outH != nullptr || ldc < N + N / 2)) return SED_ERR_ARG;
    if (two_term && (K % (two_term == 3 ? 128 : BK) || epi == EPI_ATOMIC || epi == EPI_DGELU || gbias != nullptr || ksplit > 1)) return SED_ERR_ARG;
    if (gbias != nullptr && (gb_rows < 128 || M % gb_rows || epi == EPI_ATOMIC || epi == EPI_DGELU)) return SED_ERR_ARG;
    // two_term 3: A [M, K f16 | K e4m3] against B [N, K f16 | K e4m3], K / 64 f16 tiles + K / 128 fp8 tiles; else: A [M, K] against B [N, 2K]
    GemmArgs g = gemm_args(A, B, M, N, two_term == 3 ? K + K / 2 : (two_term ? 2 * K : K), lda, ldb, ldc);
    if (two_term == 3) { g.k8 = K / 128; g.f8_scale = f8_scale; }
    else if (two_term) g.k_wrap = K / BK;
    g.out_e4m3 = out_e4m3;
    g.gbias = gbias; g.gb_rows = gb_rows;
    g.ncols = ncols; g.ksplit = ksplit > 0 ? ksplit : 1;
    g.alpha = alpha; g.bias = bias; g.resF = resF; g.outF = outF; g.outH = (bf16_t*)outH; g.outH2 = (bf16_t*)outH2;
    g.auxH = (const bf16_t*)auxH;
    g.bwd_bf16 = (f16 & 2) ? 1 : 0;
    f16 &= 1;
    if (g.bwd_bf16 && !f16) return SED_ERR_ARG;
    switch (epi) {
        case EPI_F32: return launch_gemm<EPI_F32>(g, f16, stream);
        case EPI_F32_RESID: return launch_gemm<EPI_F32_RESID>(g, f16, stream);
        case EPI_BF16: return launch_gemm<EPI_BF16>(g, f16, stream);
        case EPI_GELU: return launch_gemm<EPI_GELU>(g, f16, stream);
        case EPI_DGELU: return launch_gemm<EPI_DGELU>(g, f16, stream);
        case EPI_ATOMIC: return launch_gemm<EPI_ATOMIC>(g, f16, stream);
        case EPI_F32_BF16: return launch_gemm<EPI_F32_BF16>(g, f16, stream);
        case EPI_GELU32: return launch_gemm<EPI_GELU32>(g, f16, stream);
        default: return SED_ERR_ARG;
    }
}
extern "C" int sed_gemm_nt(const void* A, const void* B, int M, int N, int K, int lda, int ldb, int epi,
                           const float* bias, const float* resF, float* outF, void* outH, void* outH2,
                           const void* auxH, int ldc, float alpha, int ksplit, int f16, hipStream_t stream) {
    return gemm_nt_impl(A, B, M, N, K, lda, ldb, epi, bias, resF, outF, outH, outH2, auxH, ldc, alpha, ksplit, f16, N, stream);
}
extern "C" int sed_gemm_nt_gb(const void* A, const void* B, int M, int N, int K, int lda, int ldb, int epi,
                              const float* bias, const float* resF, float* outF, void* outH, void* outH2,
                              const void* auxH, int ldc, float alpha, int f16, const float* gbias, int gb_rows, hipStream_t stream) {
    return gemm_nt_impl(A, B, M, N, K, lda, ldb, epi, bias, resF, outF, outH, outH2, auxH, ldc, alpha, 1, f16, N, stream, gbias, gb_rows);
}
// ... fused GELU with the e4m3 image of the result in the same rows (outH2 [M][N f16 | N e4m3], ldc >= 3N / 2): the A operand of a following
// sed_gemm_nt_w2f8
extern "C" int sed_gemm_nt_gb_e4m3(const void* A, const void* B, int M, int N, int K, int lda, int ldb, const float* bias, void* outH2,
                                   int ldc, const float* gbias, int gb_rows, hipStream_t stream) {
    if (gbias == nullptr || N % 256 || M < 1024) return SED_ERR_ARG;
    return gemm_nt_impl(A, B, M, N, K, lda, ldb, EPI_GELU, bias, nullptr, nullptr, nullptr, outH2, nullptr, ldc, 1.f, 1, 1, N, stream, gbias, gb_rows,
                        0, 0, 1);
}
// Two-term weights: A [M, K] (f16) against B [N, 2K] = [f16(W) | f16(W - f16(W))] (sed_weight_two_term_f16); A is read twice, the
// result is A . W^T with W good to ~2^-19 relative.  256^2 kernel only (N % 256 == 0, M >= 1024), epilogues EPI_F32_RESID / EPI_GELU.
extern "C" int sed_gemm_nt_w2(const void* A, const void* B, int M, int N, int K, int lda, int ldb, int epi,
                              const float* bias, const float* resF, float* outF, void* outH, void* outH2,
                              int ldc, int f16, hipStream_t stream) {
    if (!(f16 & 1) || N % 256 || M < 1024) return SED_ERR_ARG;
    return gemm_nt_impl(A, B, M, N, K, lda, ldb, epi, bias, resF, outF, outH, outH2, nullptr, ldc, 1.f, 1, f16, N, stream, nullptr, 0, 1);
}
// ... with the lo product on the fp8 matrix path: A [M][K f16 | K e4m3] (row pitch lda halfs >= 3K / 2; the e4m3 half is the activation
// times 2^-2: sed_fp8_tail), B [N][K f16 | K e4m3] = sed_weight_two_term_f8's image with its scale exponent s; f8_exp = s.  K % 128 == 0.
static int f8_scale_word(int s) {       // both operands' scale registers are the same one: e8m0 byte of 2^-(s - 2) / 2, replicated; s even
    const int e = 128 - s / 2;
    return (s & 1) || e < 1 || e > 254 ? -1 : e * 0x01010101;
}
// out_e4m3 != 0 (epi 3, outH NULL): outH2 rows are [N f16 | N e4m3] (ldc >= 3N / 2) -- the activation and its e4m3 image, the A operand
// of the next sed_gemm_nt_w2f8
extern "C" int sed_gemm_nt_w2f8(const void* A, const void* B, int M, int N, int K, int lda, int ldb, int epi,
                                const float* bias, const float* resF, float* outF, void* outH, void* outH2,
                                int ldc, int out_e4m3, int f8_exp, hipStream_t stream) {
    if (N % 256 || M < 1024 || f8_scale_word(f8_exp) < 0) return SED_ERR_ARG;
    return gemm_nt_impl(A, B, M, N, K, lda, ldb, epi, bias, resF, outF, outH, outH2, nullptr, ldc, 1.f, 1, 1, N, stream, nullptr, 0, 3,
                        f8_scale_word(f8_exp), out_e4m3);
}
// LayerNorm folded into the two GEMMs around it (no-grad f16 passes; 256^2 kernel only: N % 256 == 0, M >= 1024).
// producer = sed_gemm_nt with EPI_F32_RESID that ALSO writes x16 [M, N] (f16 image of the new residual stream) and rowpart [M][N / 64][2]
// (per-row partial sum / sum of squares of each 64-column slice); sed_ln_fold_stats turns rowpart into rowstat [M][2] = (mean, rstd);
// consumer = EPI_GELU GEMM whose A operand is x16 (the RAW stream), B the f16 image of gamma (.) W (sed_ln_fold_weight), with
// out[m, n] = act(rstd[m] * (acc - mean[m] * colS[n]) + colC[n]).
static int gemm_nt_lnp_impl(const void* A, const void* B, int M, int N, int K, int lda, int ldb, const float* bias, const float* resF,
                            const void* res_hi, const void* res_lo, float* outF, void* x16, void* out_lo, float* rowpart, int ldc, int lo8,
                            hipStream_t stream) {
    (void)hipGetLastError();
    if (N % 256 || M < 1024 || K % BK || x16 == nullptr || rowpart == nullptr || ldc != N) return SED_ERR_ARG;
    // residual: fp32 resF, or the planes res_hi + res_lo; result: fp32 outF + f16 image x16, or the planes x16 (hi) + out_lo
    if ((res_lo != nullptr) != (res_hi != nullptr) || (res_lo == nullptr && resF == nullptr) || (out_lo == nullptr && outF == nullptr)) return SED_ERR_ARG;
    GemmArgs g = gemm_args(A, B, M, N, K, lda, ldb, ldc);
    g.bias = bias; g.resF = resF; g.outF = outF; g.outH = (bf16_t*)x16; g.rowpart = rowpart;
    g.auxH = (const bf16_t*)res_hi; g.res_lo = (const bf16_t*)res_lo; g.out_lo = (bf16_t*)out_lo; g.lo8 = lo8;
    if (lo8 && lda == 64 && K > 64) { g.a_slab = 1; g.lda = K; }      // A as [K / 64][M][64] (what sed_gemm_nt_lnc8 writes with ldc = 64)
    // (slab-major operands are addressed through one 32-bit buffer range / K-tile offset: the whole plane has to stay below 2 GiB)
    if (g.a_slab && (size_t)M * K * 2 >= (1ull << 31)) return SED_ERR_ARG;
    return launch_gemm<EPI_F32_RESID>(g, 1, stream);
}
extern "C" int sed_gemm_nt_lnp(const void* A, const void* B, int M, int N, int K, int lda, int ldb, const float* bias, const float* resF,
                               const void* res_hi, const void* res_lo, float* outF, void* x16, void* out_lo, float* rowpart, int ldc,
                               hipStream_t stream) {
    return gemm_nt_lnp_impl(A, B, M, N, K, lda, ldb, bias, resF, res_hi, res_lo, outF, x16, out_lo, rowpart, ldc, 0, stream);
}
// ... with the lo plane as bytes (GemmArgs.lo8): res_lo / out_lo are [M][ldc] uint8
extern "C" int sed_gemm_nt_lnp8(const void* A, const void* B, int M, int N, int K, int lda, int ldb, const float* bias, const float* resF,
                                const void* res_hi, const void* res_lo8, float* outF, void* x16, void* out_lo8, float* rowpart, int ldc,
                                hipStream_t stream) {
    return gemm_nt_lnp_impl(A, B, M, N, K, lda, ldb, bias, resF, res_hi, res_lo8, outF, x16, out_lo8, rowpart, ldc, 1, stream);
}
static int gemm_nt_lnc_impl(const void* A, const void* B, int M, int N, int K, int lda, int ldb, const float* colC, const float* colS,
                            const float* rowstat, void* outH2, int ldc, int a_slab, hipStream_t stream) {
    (void)hipGetLastError();
    if (N % 256 || M < 1024 || K % BK || colS == nullptr || rowstat == nullptr || outH2 == nullptr) return SED_ERR_ARG;
    GemmArgs g = gemm_args(A, B, M, N, K, lda, ldb, ldc);
    g.bias = colC; g.outH2 = (bf16_t*)outH2; g.colS = colS; g.rowstat = rowstat; g.a_slab = a_slab;
    if (a_slab && (lda != K || (size_t)M * K * 2 >= (1ull << 31))) return SED_ERR_ARG;
    if (a_slab && ldc == 64 && N > 64) { g.c_slab = 1; g.ldc = N; }      // output as [N / 64][M][64]
    return launch_gemm<EPI_GELU>(g, 1, stream);
}
extern "C" int sed_gemm_nt_lnc(const void* A, const void* B, int M, int N, int K, int lda, int ldb, const float* colC, const float* colS,
                               const float* rowstat, void* outH2, int ldc, hipStream_t stream) {
    return gemm_nt_lnc_impl(A, B, M, N, K, lda, ldb, colC, colS, rowstat, outH2, ldc, 0, stream);
}
// ... fed with the slab-major hi plane sed_gemm_nt_lnp8 writes ([K / 64][M][64] f16)
extern "C" int sed_gemm_nt_lnc8(const void* A, const void* B, int M, int N, int K, int lda, int ldb, const float* colC, const float* colS,
                                const float* rowstat, void* outH2, int ldc, hipStream_t stream) {
    return gemm_nt_lnc_impl(A, B, M, N, K, lda, ldb, colC, colS, rowstat, outH2, ldc, 1, stream);
}
// same GEMM with a narrow result: the operands are padded to N (multiple of 128) but only the first ncols (multiple of 4) output
// columns exist in memory (row stride ldc >= ncols); bias / residual / outputs are indexed like the narrow matrix.  128^2 kernel only.
extern "C" int sed_gemm_nt_cols(const void* A, const void* B, int M, int N, int K, int lda, int ldb, int epi,
                                const float* bias, const float* resF, float* outF, void* outH, void* outH2,
                                const void* auxH, int ldc, float alpha, int f16, int ncols, hipStream_t stream) {
    if (ncols <= 0 || ncols > N || (ncols % 4) || N % 256 == 0 || epi == EPI_ATOMIC) return SED_ERR_ARG;
    return gemm_nt_impl(A, B, M, N, K, lda, ldb, epi, bias, resF, outF, outH, outH2, auxH, ldc, alpha, 1, f16, ncols, stream);
}

static int gemm_qkv_impl(const void* A, const void* W, const float* bias, int M, int K, int heads, int seq,
                         int seq_pad, void* q, void* k, void* v, void* qt, void* kt, void* vt, void* q2,
                         void* q2t, const float* pos_u, const float* pos_v, int f16, const float* gbias, int gb_rows, hipStream_t stream, int two_term = 0,
                         int f8_scale = 0);
// the context network's in_proj on TWO of the three split-precision terms: A = plain f16 activations [M, K], W = the split weight image
// [N, 3K] = [hi | hi | lo] (sed_weight_images); computes A . (hi + lo)^T -- the weight to ~2^-22, the activation rounded once.  Which terms
// the posteriors need per GEMM: tools/err_sim.py (SIM_DEC_TERMS=1): in_proj is insensitive to the activation's lo part (logit error
// 3.96e-4 -> 5.4e-4) and sensitive to the weight's (1.9e-3).  All outputs of sed_gemm_qkv.
extern "C" int sed_gemm_qkv_w2s(const void* A, const void* Wsplit, const float* bias, int M, int K, int heads, int seq, int seq_pad, void* q,
                                void* k, void* v, void* qt, void* kt, void* vt, void* q2, void* q2t, const float* pos_u, const float* pos_v,
                                int f16, hipStream_t stream) {
    if (!(f16 & 1) || M < 1024) return SED_ERR_ARG;
    return gemm_qkv_impl(A, Wsplit, bias, M, K, heads, seq, seq_pad, q, k, v, qt, kt, vt, q2, q2t, pos_u, pos_v, f16, nullptr, 0, stream, 2);
}
extern "C" int sed_gemm_qkv(const void* A, const void* W, const float* bias, int M, int K, int heads, int seq,
                            int seq_pad, void* q, void* k, void* v, void* qt, void* kt, void* vt, void* q2,
                            void* q2t, const float* pos_u, const float* pos_v, int f16, hipStream_t stream) {
    return gemm_qkv_impl(A, W, bias, M, K, heads, seq, seq_pad, q, k, v, qt, kt, vt, q2, q2t, pos_u, pos_v, f16, nullptr, 0, stream);
}
extern "C" int sed_gemm_qkv_gb(const void* A, const void* W, const float* bias, int M, int K, int heads, int seq,
                               int seq_pad, void* q, void* k, void* v, int f16, const float* gbias, int gb_rows, hipStream_t stream) {
    return gemm_qkv_impl(A, W, bias, M, K, heads, seq, seq_pad, q, k, v, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, f16,
                         gbias, gb_rows, stream);
}
// folded-LayerNorm consumer (see sed_gemm_nt_lnc): A = f16 image of the raw stream, W = f16 image of gamma (.) W_qkv; inference outputs only
static int gemm_qkv_lnc_impl(const void* A, const void* W, const float* colC, const float* colS, const float* rowstat, int M, int K,
                             int heads, int seq, int seq_pad, void* q, void* k, void* v, int a_slab, hipStream_t stream) {
    (void)hipGetLastError();
    if (M < 1024 || K % BK || colS == nullptr || rowstat == nullptr || seq <= 0 || (seq_pad % 64) || M % seq) return SED_ERR_ARG;
    GemmArgs g = gemm_args(A, W, M, 3 * heads * 64, K, K, K, 3 * heads * 64);
    g.bias = colC; g.colS = colS; g.rowstat = rowstat;
    g.q = (bf16_t*)q; g.k = (bf16_t*)k; g.v = (bf16_t*)v;
    g.seq = seq; g.seq_pad = seq_pad; g.heads = heads; g.a_slab = a_slab;
    if (a_slab && (size_t)M * K * 2 >= (1ull << 31)) return SED_ERR_ARG;
    return launch_gemm<EPI_QKV>(g, 1, stream);
}
extern "C" int sed_gemm_qkv_lnc(const void* A, const void* W, const float* colC, const float* colS, const float* rowstat, int M, int K,
                                int heads, int seq, int seq_pad, void* q, void* k, void* v, hipStream_t stream) {
    return gemm_qkv_lnc_impl(A, W, colC, colS, rowstat, M, K, heads, seq, seq_pad, q, k, v, 0, stream);
}
extern "C" int sed_gemm_qkv_lnc8(const void* A, const void* W, const float* colC, const float* colS, const float* rowstat, int M, int K,
                                 int heads, int seq, int seq_pad, void* q, void* k, void* v, hipStream_t stream) {
    return gemm_qkv_lnc_impl(A, W, colC, colS, rowstat, M, K, heads, seq, seq_pad, q, k, v, 1, stream);
}
// two-term weights (see sed_gemm_nt_w2): W is [3 * heads * 64, 2K]; inference outputs only
extern "C" int sed_gemm_qkv_w2(const void* A, const void* W, const float* bias, int M, int K, int heads, int seq,
                               int seq_pad, void* q, void* k, void* v, int f16, hipStream_t stream) {
    if (!(f16 & 1) || M < 1024) return SED_ERR_ARG;
    return gemm_qkv_impl(A, W, bias, M, K, heads, seq, seq_pad, q, k, v, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, f16,
                         nullptr, 0, stream, 1);
}
// ... lo product on the fp8 matrix path (see sed_gemm_nt_w2f8): A [M][K f16 | K e4m3], W [3 * heads * 64][K f16 | K e4m3], both with
// a row pitch of 3K / 2 halfs
extern "C" int sed_gemm_qkv_w2f8(const void* A, const void* W, const float* bias, int M, int K, int heads, int seq,
                                 int seq_pad, void* q, void* k, void* v, int f8_exp, hipStream_t stream) {
    if (M < 1024 || K % 128 || f8_scale_word(f8_exp) < 0) return SED_ERR_ARG;
    return gemm_qkv_impl(A, W, bias, M, K, heads, seq, seq_pad, q, k, v, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1,
                         nullptr, 0, stream, 3, f8_scale_word(f8_exp));
}
static int gemm_qkv_impl(const void* A, const void* W, const float* bias, int M, int K, int heads, int seq,
                         int seq_pad, void* q, void* k, void* v, void* qt, void* kt, void* vt, void* q2,
                         void* q2t, const float* pos_u, const float* pos_v, int f16, const float* gbias, int gb_rows, hipStream_t stream, int two_term,
                         int f8_scale) {
    (void)hipGetLastError();
    if (gbias != nullptr && (gb_rows < 128 || M % gb_rows)) return SED_ERR_ARG;
    GemmArgs g = gemm_args(A, W, M, 3 * heads * 64, K, K, K, 3 * heads * 64);
    g.gbias = gbias; g.gb_rows = gb_rows;
    if (two_term == 3) {
        if (K % 128 || gbias != nullptr) return SED_ERR_ARG;
        g.k8 = K / 128; g.f8_scale = f8_scale; g.K = K + K / 2; g.lda = g.K; g.ldb = g.K;
    } else if (two_term) {
        if (K % BK || gbias != nullptr) return SED_ERR_ARG;
        g.k_wrap = K / BK; g.K = 2 * K; g.ldb = 2 * K;
        if (two_term == 2) { g.ldb = 3 * K; g.b_skip = K / BK; }      // W = [hi | hi | lo]: walk hi, then lo
    }
    g.bias = bias;
    g.q = (bf16_t*)q; g.k = (bf16_t*)k; g.v = (bf16_t*)v; g.qt = (bf16_t*)qt; g.kt = (bf16_t*)kt; g.vt = (bf16_t*)vt;
    g.q2 = (bf16_t*)q2; g.q2t = (bf16_t*)q2t; g.pu = pos_u; g.pv = pos_v;
    g.seq = seq; g.seq_pad = seq_pad; g.heads = heads;
    if (seq <= 0 || (seq_pad % 64) || M % seq) return SED_ERR_ARG;
    g.bwd_bf16 = (f16 & 2) ? 1 : 0;
    f16 &= 1;
    if (g.bwd_bf16 && !f16) return SED_ERR_ARG;
    return launch_gemm<EPI_QKV>(g, f16, stream);
}
