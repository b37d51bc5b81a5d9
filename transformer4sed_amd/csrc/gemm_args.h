// What the GEMM translation units share: the epilogue kinds (EPI_*), the argument block of the NT kernels (GemmArgs), the tile
// constants, and the few device helpers that more than one of gemm.hip (NT GEMMs), gemm_epilogue.h (the 256^2 kernel's epilogues)
// and gemm_tn.hip (weight-gradient GEMM) use.  Host side: the CU budget (one instance, in gemm.hip) and the launch helper for
// kernels that need more than the default dynamic-LDS limit.
#pragma once
#include "common.h"

enum {
    EPI_F32 = 0,          // outF = acc*alpha + bias
    EPI_F32_RESID = 1,    // outF = resF + acc + bias                (residual stream; resF may alias outF)
    EPI_BF16 = 2,         // outH = bf16(acc + bias)
    EPI_GELU = 3,         // outH = bf16(h = acc + bias), outH2 = bf16(gelu(h))
    EPI_DGELU = 4,        // outH = bf16(acc * gelu'(auxH))
    EPI_ATOMIC = 5,       // atomicAdd(outF, acc*alpha)               (split-K weight gradients)
    EPI_QKV = 6,          // head-split q/k/v (+ transposed copies, + rel-pos biased queries)
    EPI_F32_BF16 = 7,     // outF = acc + bias and outH = bf16(same)
    EPI_GELU32 = 8,       // outH = 16-bit(h = acc + bias) (kept for backward), outF = fp32 gelu(h) (split-precision consumers)
};

struct GemmArgs {
    const bf16_t* A;
    const bf16_t* B;
    int M, N, K, lda, ldb, ldc, ksplit;
    float alpha;
    const float* bias;
    const float* resF;
    float* outF;
    bf16_t* outH;
    bf16_t* outH2;
    const bf16_t* auxH;
    // EPI_QKV
    bf16_t *q, *k, *v, *qt, *kt, *vt, *q2, *q2t;
    const float *pu, *pv;
    int seq, seq_pad, heads;
    int bwd_bf16; // f16 runs only: tensors that only the (bf16) backward consumes are written as bf16 straight away
    int group_m;  // 256^2 kernel: tile rows per L2 group (see gemm_nt_pp_kernel)
    int persist;  // 256^2 kernel: one workgroup per CU walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ...
    int ncols;    // 128^2 kernel: output columns >= ncols are computed but not written (operands padded to the tile width)
    // Row-group bias (nullable): row m additionally gets gbias[(m / gb_rows) * N + n] -- one bias row per clip (gb_rows = tokens per
    // clip, M % gb_rows == 0, gb_rows >= 128).  Carries the weight-rounding correction of the evaluation-mode encoder (engine.py
    // `_wcorr_bias`): mean activation of the clip x the part of the fp32 weight its f16 image dropped.
    const float* gbias;
    int gb_rows;
    // Two-term weights (256^2 kernel, evaluation-mode encoder): B rows are [f16(W) | f16(W - f16(W))] over K = 2 * k_wrap * 64 and the
    // A panel (k_wrap K tiles wide) is walked twice -- the fp32 weight to ~2^-19 against the same f16 activations.  0 = off.
    int k_wrap;
    // ... and, when the B rows are a split-precision weight image [hi | hi | lo] over 3 * k_wrap K tiles (context network), the number of B
    // K tiles to skip once the A panel has wrapped: the walk then multiplies A . hi^T and A . lo^T (b_skip = k_wrap), dropping the a_lo
    // term of the three-term product.
    int b_skip;
    // Two-term weights with the lo product on the fp8 matrix path (256^2 kernel, evaluation-mode encoder; k8 != 0): A rows are
    // [K f16 | K e4m3] (the activation and its OCP-e4m3 image, scaled by 2^-2: sed_fp8_tail or the producing kernels), B rows
    // [f16(W) | e4m3(2^s (W - f16(W)))] (sed_weight_two_term_f8); both with a row pitch of 3 K bytes.  The K walk is K / 64 f16 tiles followed
    // by k8 = K / 128 fp8 tiles of the same 128 bytes per row: same DMA, same LDS image, same fragment reads -- the 32 bytes a lane holds
    // of a row are the operand of ONE v_mfma_scale_f32_16x16x128_f8f6f4 instead of two v_mfma_f32_16x16x32_f16 (the k order inside a
    // tile is the same permutation for both operands).  f8_scale = the e8m0 byte 128 - s / 2 replicated four times, used as BOTH operands' block
    // scale (s even): the hardware scales the lo product back by 2^-(s - 2).  W_lo is 2^-12 of the result and e4m3 keeps 2^-4 of either factor: the lo product to ~2^-15 of the
    // result for half of an f16 pass (`profiles/r4_fp8_mfma_probe.txt`).
    int k8;
    int f8_scale;
    // ... and the 16-bit output of such a GEMM (EPI_GELU's outH2: the fc1 activation, fc2's A operand) can carry its own e4m3 image:
    // rows [N f16 | N e4m3], ldc >= 3N / 2 halfs
    int out_e4m3;
    // Persistent 256^2 kernel: workgroups with an odd (blockIdx.x >> 3) start `stagger` ticks of the 100 MHz real-time counter late, so
    // that their store phases fall into the other half's main loops instead of all 256 CUs hitting HBM in lock-step.  0 = off.
    int stagger;
    // LayerNorm folded into the GEMMs around it (256^2 kernel, no-grad f16 passes; engine.py `_encoder_fwd`):
    //   producer (EPI_F32_RESID): besides the fp32 residual stream it writes the f16 image of the new stream to outH and, per row and
    //     64-column slice, the partial sums (sum x, sum x^2) to rowpart [M][N / 64][2];
    //   consumer (EPI_QKV / EPI_GELU): A is that f16 image of the RAW stream, B the f16 image of gamma (.) W; row m of the result is
    //     rstd[m] * (acc - mean[m] * colS[n]) + bias[n] with rowstat [M][2] = (mean, rstd), colS[n] = sum_k B[n, k], and `bias` already
    //     holding beta . W^T + b  ->  exactly Linear(LayerNorm(x)) without the normalised tensor ever existing.
    float* rowpart;
    const float* rowstat;
    const float* colS;
    // producer, split-plane residual stream: the stream lives as two f16 planes hi + lo (~22 significand bits) instead of fp32 -- the hi
    // plane IS the next GEMM's A operand, so the producer moves 8 bytes per element (read hi, lo; write hi, lo) instead of 10 (fp32
    // read-modify-write + the f16 image).  res_lo != NULL: the residual comes as auxH (hi) + res_lo; out_lo != NULL: the result leaves as
    // outH (hi) + out_lo and outF is not written.
    const bf16_t* res_lo;
    bf16_t* out_lo;
    // ... with an 8-bit lo plane (lo8 != 0; res_lo / out_lo then point at [M][ldc] BYTES): the stream value is hi * (1 + (q - 128) * 2^-18),
    // q = the byte -- the f16 rounding residual |x - hi| <= ulp(hi) / 2 <= |hi| 2^-11 in steps of |hi| 2^-18, i.e. the stream to ~2^-19
    // relative (the f16 lo plane: ~2^-22; an f16 stream: 2^-12) for 6 instead of 8 bytes per element through a producer.
    int lo8;
    // ... and with lo8 the hi plane (outH / auxH of the producer) is slab-major as well: [ldc / 64][M][64] f16 -- a wave's 128 rows x 64
    // columns are one contiguous 16 KB run, and for the consumer GEMMs (a_slab != 0: A is such a plane with K / 64 slabs) a K tile of
    // 256 rows is one contiguous 32 KB run instead of 256 pieces of 128 bytes, 1536 bytes apart.
    int a_slab;
    // ... and the 16-bit output of the fused-GELU consumer (outH2) can leave slab-major as well (c_slab != 0: [N / 64][M][64]) -- the fc1
    // activation of a folded block is read by nobody but the fc2 producer, as its slab-major A operand.
    int c_slab;
    // Persistent 256^2 kernel, dynamic tile walk: 8 per-XCD tile counters + 1 exit counter, one 64-byte line each (int index 16 x).  A
    // workgroup takes the next tile of ITS XCD's contiguous tile range from counter blockIdx.x & 7 (so the L2 grouping of the static walk
    // is kept) instead of the fixed blockIdx.x + k gridDim.x: a workgroup that becomes resident late -- or only after the others have
    // drained the range, when communication kernels hold CUs -- costs nothing instead of a whole column of tiles.  NULL = static walk.
    int* tile_ctr;
};

#define TILE 128
#define BK 64

// two packed IEEE halves -> two packed bf16
__device__ __forceinline__ unsigned h2x2_to_bf(unsigned p) { return pack2bf(h2f((bf16_t)(p & 0xFFFF)), h2f((bf16_t)(p >> 16))); }
template <bool F16>
__device__ __forceinline__ unsigned pack2_sel(float a, float b, int as_bf16) { return (F16 && !as_bf16) ? pack2<true>(a, b) : pack2<false>(a, b); }
template <bool F16>
__device__ __forceinline__ bf16_t to16_sel(float a, int as_bf16) { return (F16 && !as_bf16) ? to_16<true>(a) : to_16<false>(a); }

// 256^2 tiles (NT ping-pong kernel and TN kernel): LDS budget and the staging area of the epilogues that still stage (NT: the fp32 +
// 16-bit outputs, the head split with transposed copies, the LayerNorm-fold producers at the ends of a folded run, the evaluation-mode
// residual GEMMs -- everything else is LDS-free; TN: the split-K partial sums).
// After the K loop each wave owns a private 17 KiB LDS region.  The accumulators are written there as a row-major [rows][64]
// sub-tile (padded row stride), then read back so that 8 (16-bit) or 16 (fp32) consecutive lanes cover one full output row: every
// global store / residual load is a run of whole 128- / 256-byte rows instead of 64 different cache lines per instruction.
#define V3_WLDS 17408          // per-wave bytes: 128 rows x 136 B (16-bit) or 64 rows x 264 B (fp32, two passes)
#define V3_RS16 136
#define V3_RS32 264
#define V3_T 256
#define V3_STAGE (64 * 1024)
#define V3_LDS (8 * V3_WLDS > 2 * V3_STAGE ? 8 * V3_WLDS : 2 * V3_STAGE)

// Column order of a wave's 128 x 64 sub-tile (round 4).  MFMA block j, lane group lq = lane >> 4, register r used to be column
// 16 j + 4 lq + r: a lane's 16 values of a row were four separate 8-byte runs, and the tile had to go through LDS to become whole rows.
// The B operand's DMA now places weight row PP_COL(j, lq) + r at LDS row 16 j + 4 lq + r of its 64-row group (a permutation of address
// bits 2..4 on the DMA SOURCE side; fragment reads and swizzle unchanged), so the lane holds columns 8 lq .. 8 lq + 7 (blocks 0, 1)
// and 32 + 8 lq .. 32 + 8 lq + 7 (blocks 2, 3): two 16-byte runs of 16-bit outputs, and the four lane groups of a row make 64
// contiguous bytes per store instruction -- the 16-bit epilogues store straight from the accumulators, no LDS round trip.
__device__ __forceinline__ constexpr int PP_COL(int j, int lq) { return 8 * lq + 32 * (j >> 1) + 4 * (j & 1); }
// C-tile stores of the 256^2 kernels are non-temporal: the tile is not re-read by this kernel, and write-allocating it evicts
// the A/B panels that the neighbouring column tiles still need from the 4 MB L2 (+2..4 % on the model's shapes).
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
template <class T>
__device__ __forceinline__ void v3_st(void* p, const T& v) {
    if constexpr (sizeof(T) == 16) {
        u32x4_t t;
        __builtin_memcpy(&t, &v, 16);
        __builtin_nontemporal_store(t, reinterpret_cast<u32x4_t*>(p));
    } else {
        u32x2_t t;
        __builtin_memcpy(&t, &v, 8);
        __builtin_nontemporal_store(t, reinterpret_cast<u32x2_t*>(p));
    }
}

// 64 staged rows (accumulator blocks 4 p .. 4 p + 3) as fp32
// (PERM: the accumulators are in PP_COL column order -- the NT ping-pong kernel; the TN kernel's are in plain order)
template <int RB = 8, bool PERM = false>
__device__ __forceinline__ void pp_stage32(unsigned char* wl, const f32x4_t (&acc)[8][4], int p, int l15, int lq) {
#pragma unroll
    for (int ii = 0; ii < 4; ++ii)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (4 * p + ii >= RB) continue;
            const f32x4_t& a = acc[4 * p + ii][j];
            *reinterpret_cast<float4*>(wl + (ii * 16 + l15) * V3_RS32 + (PERM ? PP_COL(j, lq) : j * 16 + 4 * lq) * 4) = make_float4(a[0], a[1], a[2], a[3]);
        }
}
// the LDS pointer type of the direct-to-LDS loads of both 256^2 K loops (their MFMA is common.h's mfma16)
typedef __attribute__((address_space(3))) void* lds_ptr_t;

// ---- host ----
// Number of CUs the persistent GEMM kernels (NT and TN) size their grids for: the device's CU count, lowered by
// sed_gemm_set_cu_budget / SED_GEMM_CUS.  Process-wide state; defined in gemm.hip.
__attribute__((visibility("hidden"))) int gemm_cu_budget();
// Launch of a kernel that needs `lds_bytes` of dynamic LDS: its limit is raised once per process (each process owns one device), then
// it is launched.  `raised` is the caller's per-kernel flag.
template <class... P, class... A>
inline void launch_big_lds(bool& raised, void (*kernel)(P...), dim3 grid, dim3 block, int lds_bytes, hipStream_t s, const A&... args) {
    if (!raised) { (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes); raised = true; }
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, s, args...);
}
