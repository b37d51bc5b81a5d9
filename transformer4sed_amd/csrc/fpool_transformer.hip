// Frequency-wise transformer pooling, PaSST_SED(f_pool="frequency_wise_tranformer_encoder") (src/models/pooling.py:18-34,
// src/models/passt/passt_sed.py:199-218): the pieces around the GEMMs and LayerNorms of its two timm blocks.
//   * sequence build: out_norm over the patch tokens of the tapped layer [Bx, 2 + F tp, 768], regrouped from (f, t) order into one
//     sequence per time column [Bx tp, 1 + F, 768] behind the tag row linear_emb(1) = weight[:, 0] + bias; and its backward;
//   * short attention: softmax(q k^T 192^-0.5) v for sequences of N <= 16 tokens, H heads of 192, straight from the packed qkv GEMM
//     output [S N, 3 H 192]; the backward recomputes the probabilities (N^2 dot products of 192 terms: nothing next to reading qkv,
//     and no [S, H, N, N] tensor to write and read back);
//   * the final LayerNorm of row 0 of every sequence -> pooled [S, 768], and its backward (rows 1 .. N-1 get zero gradient).
// All fp32 math with IEEE semantics (built like norm_elem.hip, no fast-math); 16-bit only as GEMM operand storage.  No atomics:
// parameter gradients are reduced in two stages of fixed order, sequences never share a reduction, so every result is bit-reproducible.
// No kernel waits on another workgroup.
#include "common.h"
#include "rows768.h"
#include "../../include/sed_hip.h"

#define HD 192                  // head width
#define NMAX 16                 // longest sequence of the short attention
#define LD (HD + 1)             // LDS row pitch of a head slice: rows one bank apart
#define RED_MAX_WG 256          // workgroups of a backward that reduces parameter gradients: each leaves ONE partial of every gradient
#define ROW_WAVES 4             // waves per workgroup of the row kernels, one 768-wide row per wave at a time

// mean and 1 / sqrt(var + eps) of a row held by one wave (two passes over the registers)
__device__ __forceinline__ void row_stats(const float4* v, float eps, float& mu, float& rs) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    mu = wave_sum(s) * (1.0f / DM);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float d = f4(v[i], e) - mu; q = fmaf(d, d, q); }
    rs = 1.0f / sqrtf(wave_sum(q) * (1.0f / DM) + eps);
}
__device__ __forceinline__ void normalise_row(float4* v, float mu, float rs, const float4* g, const float4* b) {
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) f4(v[i], e) = (f4(v[i], e) - mu) * rs * f4(g[i], e) + f4(b[i], e);
}
// LayerNorm backward of one row: dy -> dx (in place in dy), dgamma += dy xhat, dbeta += dy
__device__ __forceinline__ void ln_bwd_row(float4* dy, const float4* x, float mu, float rs, const float4* g, float4* dg, float4* db) {
    float4 xh[NV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float h = (f4(x[i], e) - mu) * rs;
            const float d = f4(dy[i], e);
            f4(xh[i], e) = h;
            f4(dg[i], e) = fmaf(d, h, f4(dg[i], e));
            f4(db[i], e) += d;
            const float gd = d * f4(g[i], e);
            f4(dy[i], e) = gd;
            s1 += gd;
            s2 = fmaf(gd, h, s2);
        }
    const float c1 = wave_sum(s1) * (1.0f / DM), c2 = wave_sum(s2) * (1.0f / DM);
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) f4(dy[i], e) = rs * (f4(dy[i], e) - c1 - f4(xh[i], e) * c2);
}

// ---------------------------------------------------------------------------------------------------
// two-stage reduction of the parameter gradients: every workgroup adds its waves' register partials through LDS in wave order and
// leaves partials[wg][q][768]; reduce_partials_kernel adds the workgroups in index order into the (accumulating) destinations
// ---------------------------------------------------------------------------------------------------
template <int NQ>
__device__ __forceinline__ void block_partials(float (*red)[DM], const Row* acc, float* __restrict__ partials, int lane, int wave) {
    for (int q = 0; q < NQ; ++q) {
        __syncthreads();
        row_store(acc[q], red[wave], lane);
        __syncthreads();
        for (int c = threadIdx.x; c < DM; c += 64 * ROW_WAVES) {
            float s = red[0][c];
#pragma unroll
            for (int w = 1; w < ROW_WAVES; ++w) s += red[w][c];
            partials[((size_t)blockIdx.x * NQ + q) * DM + c] = s;
        }
    }
}

__global__ __launch_bounds__(256) void reduce_partials_kernel(const float* __restrict__ partials, int nparts, int nq, float* o0, float* o1,
                                                              float* o2) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= nq * DM) return;
    const int q = idx / DM, c = idx % DM;
    float* out = q == 0 ? o0 : (q == 1 ? o1 : o2);
    if (out == nullptr) return;
    float s = 0.f;
    for (int p = 0; p < nparts; ++p) s += partials[((size_t)p * nq + q) * DM + c];
    out[c] += s;
}

// ---------------------------------------------------------------------------------------------------
// sequence build
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * ROW_WAVES) void seq_build_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                      const float* __restrict__ beta, float eps,
                                                                      const float* __restrict__ tag_w, const float* __restrict__ tag_b,
                                                                      float* __restrict__ xs, float* __restrict__ mean,
                                                                      float* __restrict__ rstd, int tp, int F, int64_t R) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * ROW_WAVES + wave;
    if (row >= R) return;
    const int N = 1 + F;
    const int64_t s = row / N;
    const int j = (int)(row % N);
    Row v;
    float mu = 0.f, rs = 0.f;
    if (j == 0) {       // the tag row: linear_emb(1) = weight[:, 0] + bias, the same for every sequence
        Row b;
        row_load(v, tag_w, lane);
        row_load(b, tag_b, lane);
#pragma unroll
        for (int i = 0; i < NV; ++i) { v.v[i].x += b.v[i].x; v.v[i].y += b.v[i].y; v.v[i].z += b.v[i].z; v.v[i].w += b.v[i].w; }
    } else {
        const int64_t b = s / tp, t = s % tp;
        Row g, bt;
        row_load(v, x + ((size_t)b * (2 + (size_t)F * tp) + 2 + (size_t)(j - 1) * tp + t) * DM, lane);
        row_load(g, gamma, lane);
        row_load(bt, beta, lane);
        row_stats(v.v, eps, mu, rs);
        normalise_row(v.v, mu, rs, g.v, bt.v);
    }
    row_store(v, xs + (size_t)row * DM, lane);
    if (mean != nullptr && lane == 0) { mean[row] = mu; rstd[row] = rs; }
}

__global__ __launch_bounds__(64 * ROW_WAVES) void seq_build_bwd_kernel(const float* __restrict__ dxs, const float* __restrict__ x,
                                                                      const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                      const float* __restrict__ gamma, float* __restrict__ dx,
                                                                      float* __restrict__ partials, int tp, int F, int64_t R) {
    __shared__ float red[ROW_WAVES][DM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int N = 1 + F;
    const size_t Ntok = 2 + (size_t)F * tp;
    Row g, acc[3];       // dgamma, dbeta, dtag
    row_load(g, gamma, lane);
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int i = 0; i < NV; ++i) acc[q].v[i] = float4{0.f, 0.f, 0.f, 0.f};
    for (int64_t row = (int64_t)blockIdx.x * ROW_WAVES + wave; row < R; row += (int64_t)gridDim.x * ROW_WAVES) {
        const int64_t s = row / N;
        const int j = (int)(row % N);
        const int64_t b = s / tp, t = s % tp;
        Row d;
        row_load(d, dxs + (size_t)row * DM, lane);
        if (j == 0) {
#pragma unroll
            for (int i = 0; i < NV; ++i) { acc[2].v[i].x += d.v[i].x; acc[2].v[i].y += d.v[i].y; acc[2].v[i].z += d.v[i].z; acc[2].v[i].w += d.v[i].w; }
            if (t == 0 && dx != nullptr) {      // cls / dist rows of this clip: nothing of the pooling reads them
                row_zero(dx + (size_t)b * Ntok * DM, lane);
                row_zero(dx + ((size_t)b * Ntok + 1) * DM, lane);
            }
            continue;
        }
        const size_t tok = (size_t)b * Ntok + 2 + (size_t)(j - 1) * tp + t;
        Row xv;
        row_load(xv, x + tok * DM, lane);
        ln_bwd_row(d.v, xv.v, mean[row], rstd[row], g.v, acc[0].v, acc[1].v);
        if (dx != nullptr) row_store(d, dx + tok * DM, lane);
    }
    block_partials<3>(red, acc, partials, lane, wave);
}

// ---------------------------------------------------------------------------------------------------
// final LayerNorm of row 0 of every sequence
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * ROW_WAVES) void rownorm_fwd_kernel(const float* __restrict__ xs, const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, float eps, float* __restrict__ pooled,
                                                                    float* __restrict__ mean, float* __restrict__ rstd, int N, int64_t S) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t s = (int64_t)blockIdx.x * ROW_WAVES + wave;
    if (s >= S) return;
    Row v, g, bt;
    row_load(v, xs + (size_t)s * N * DM, lane);
    row_load(g, gamma, lane);
    row_load(bt, beta, lane);
    float mu, rs;
    row_stats(v.v, eps, mu, rs);
    normalise_row(v.v, mu, rs, g.v, bt.v);
    row_store(v, pooled + (size_t)s * DM, lane);
    if (mean != nullptr && lane == 0) { mean[s] = mu; rstd[s] = rs; }
}

__global__ __launch_bounds__(64 * ROW_WAVES) void rownorm_bwd_kernel(const float* __restrict__ dpooled, const float* __restrict__ xs,
                                                                    const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                    const float* __restrict__ gamma, float* __restrict__ dxs,
                                                                    float* __restrict__ partials, int N, int64_t S) {
    __shared__ float red[ROW_WAVES][DM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Row g, acc[2];
    row_load(g, gamma, lane);
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int i = 0; i < NV; ++i) acc[q].v[i] = float4{0.f, 0.f, 0.f, 0.f};
    for (int64_t s = (int64_t)blockIdx.x * ROW_WAVES + wave; s < S; s += (int64_t)gridDim.x * ROW_WAVES) {
        Row d, xv;
        row_load(d, dpooled + (size_t)s * DM, lane);
        row_load(xv, xs + (size_t)s * N * DM, lane);
        ln_bwd_row(d.v, xv.v, mean[s], rstd[s], g.v, acc[0].v, acc[1].v);
        row_store(d, dxs + (size_t)s * N * DM, lane);
        for (int j = 1; j < N; ++j) row_zero(dxs + ((size_t)s * N + j) * DM, lane);
    }
    block_partials<2>(red, acc, partials, lane, wave);
}

// ---------------------------------------------------------------------------------------------------
// short attention: one wave owns a (sequence, head)
// ---------------------------------------------------------------------------------------------------
// N rows of 192 values starting at `src` (row pitch `ld` elements; kind 0 bf16, 1 f16, 2 f32) -> fp32 dst[N][LD] in LDS, 16 bytes a load
__device__ __forceinline__ void load_slice(const void* src, int kind, size_t ld, int N, float (*dst)[LD], int lane) {
    if (kind == 2) {
        const float* p = static_cast<const float*>(src);
        for (int idx = lane; idx < N * (HD / 4); idx += 64) {
            const int tok = idx / (HD / 4), ch = idx % (HD / 4);
            const float4 v = *reinterpret_cast<const float4*>(p + tok * ld + ch * 4);
            dst[tok][ch * 4 + 0] = v.x; dst[tok][ch * 4 + 1] = v.y; dst[tok][ch * 4 + 2] = v.z; dst[tok][ch * 4 + 3] = v.w;
        }
        return;
    }
    const bf16_t* p = static_cast<const bf16_t*>(src);
    for (int idx = lane; idx < N * (HD / 8); idx += 64) {
        const int tok = idx / (HD / 8), ch = idx % (HD / 8);
        const uint4 v = *reinterpret_cast<const uint4*>(p + tok * ld + ch * 8);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bf16_t lo = (bf16_t)(w[e] & 0xffffu), hi = (bf16_t)(w[e] >> 16);
            dst[tok][ch * 8 + 2 * e] = kind ? h2f(lo) : bf2f(lo);
            dst[tok][ch * 8 + 2 * e + 1] = kind ? h2f(hi) : bf2f(hi);
        }
    }
}

// a[i] . b[j] over the 192 columns for the pairs of this lane: row i = lane >> 2, columns j = (lane & 3) + 4 c
__device__ __forceinline__ void pair_dots(const float (*a)[LD], const float (*b)[LD], int N, int lane, float* out) {
    const int i = lane >> 2, j0 = lane & 3;
    out[0] = out[1] = out[2] = out[3] = 0.f;
    if (i >= N) return;
    for (int d = 0; d < HD; ++d) {
        const float av = a[i][d];
#pragma unroll
        for (int c = 0; c < 4; ++c) out[c] = fmaf(av, b[j0 + 4 * c][d], out[c]);      // (rows >= N of b: never loaded, never used below)
    }
}
__device__ __forceinline__ float quad_sum(float v) { v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); return v; }
__device__ __forceinline__ float quad_max(float v) { v = fmaxf(v, __shfl_xor(v, 1, 64)); v = fmaxf(v, __shfl_xor(v, 2, 64)); return v; }

// softmax over the valid columns of row i of the scores this lane holds (the four lanes of a row cooperate); p = 0 outside the sequence
__device__ __forceinline__ void row_softmax(const float* sc, float scale, int N, int lane, float* p) {
    const int i = lane >> 2, j0 = lane & 3;
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < 4; ++c) if (i < N && j0 + 4 * c < N) m = fmaxf(m, sc[c] * scale);
    m = quad_max(m);
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        p[c] = (i < N && j0 + 4 * c < N) ? expf(sc[c] * scale - m) : 0.f;
        sum += p[c];
    }
    sum = quad_sum(sum);
    const float inv = (i < N) ? 1.0f / sum : 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) p[c] *= inv;
}

__global__ __launch_bounds__(64) void attn_short_fwd_kernel(const void* __restrict__ qkv, bf16_t* __restrict__ out, int N, int H, int in_kind,
                                                           int mode) {
    __shared__ float qs[NMAX][LD], ks[NMAX][LD], vs[NMAX][LD];
    __shared__ float ps[NMAX][NMAX + 1];
    const int lane = threadIdx.x;
    const size_t s = blockIdx.x / H;
    const int h = blockIdx.x % H;
    const size_t ld = 3 * (size_t)H * HD, esz = in_kind == 2 ? 4 : 2;
    const char* base = static_cast<const char*>(qkv) + (s * N * ld + (size_t)h * HD) * esz;
    // (rows N .. 15 of ks are read by pair_dots for lanes whose columns lie outside the sequence: keep them finite)
    for (int idx = lane; idx < (NMAX - N) * LD; idx += 64) ks[N + idx / LD][idx % LD] = 0.f;
    load_slice(base, in_kind, ld, N, qs, lane);
    load_slice(base + (size_t)H * HD * esz, in_kind, ld, N, ks, lane);
    load_slice(base + 2 * (size_t)H * HD * esz, in_kind, ld, N, vs, lane);
    __syncthreads();
    float sc[4], p[4];
    pair_dots(qs, ks, N, lane, sc);
    row_softmax(sc, 0.07216878364870322f, N, lane, p);       // 192^-0.5
#pragma unroll
    for (int c = 0; c < 4; ++c) ps[lane >> 2][(lane & 3) + 4 * c] = p[c];
    __syncthreads();
    for (int i = 0; i < N; ++i) {
        float o[3] = {0.f, 0.f, 0.f};
        for (int j = 0; j < N; ++j) {
            const float pij = ps[i][j];
#pragma unroll
            for (int e = 0; e < 3; ++e) o[e] = fmaf(pij, vs[j][lane + 64 * e], o[e]);
        }
        const size_t W = (size_t)H * HD;
        if (mode == 4) {        // split precision [hi | lo | hi], as sed_layernorm_fwd writes it
            bf16_t* dst = out + (s * N + i) * 3 * W + (size_t)h * HD;
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const bf16_t hi = f2h(o[e]);
                dst[lane + 64 * e] = hi;
                dst[W + lane + 64 * e] = f2h(o[e] - h2f(hi));
                dst[2 * W + lane + 64 * e] = hi;
            }
        } else {
            bf16_t* dst = out + (s * N + i) * W + (size_t)h * HD;
#pragma unroll
            for (int e = 0; e < 3; ++e) dst[lane + 64 * e] = mode ? f2h(o[e]) : f2bf(o[e]);
        }
    }
}

__global__ __launch_bounds__(64) void attn_short_bwd_kernel(const void* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                           bf16_t* __restrict__ dqkv, int N, int H, int in_kind) {
    __shared__ float qs[NMAX][LD], ks[NMAX][LD], vs[NMAX][LD], gs[NMAX][LD];
    __shared__ float ps[NMAX][NMAX + 1], ds[NMAX][NMAX + 1];
    const int lane = threadIdx.x;
    const size_t s = blockIdx.x / H;
    const int h = blockIdx.x % H;
    const size_t W = (size_t)H * HD, ld = 3 * W, esz = in_kind == 2 ? 4 : 2;
    const float scale = 0.07216878364870322f;
    const char* base = static_cast<const char*>(qkv) + (s * N * ld + (size_t)h * HD) * esz;
    for (int idx = lane; idx < (NMAX - N) * LD; idx += 64) { ks[N + idx / LD][idx % LD] = 0.f; vs[N + idx / LD][idx % LD] = 0.f; }
    load_slice(base, in_kind, ld, N, qs, lane);
    load_slice(base + W * esz, in_kind, ld, N, ks, lane);
    load_slice(base + 2 * W * esz, in_kind, ld, N, vs, lane);
    load_slice(dout + s * N * W + (size_t)h * HD, 0, W, N, gs, lane);
    __syncthreads();
    float sc[4], p[4], dp[4];
    pair_dots(qs, ks, N, lane, sc);
    row_softmax(sc, scale, N, lane, p);
    pair_dots(gs, vs, N, lane, dp);            // dP[i][j] = dO[i] . v[j]
    float rsum = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) rsum = fmaf(p[c], dp[c], rsum);
    rsum = quad_sum(rsum);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        ps[lane >> 2][(lane & 3) + 4 * c] = p[c];
        ds[lane >> 2][(lane & 3) + 4 * c] = scale * p[c] * (dp[c] - rsum);     // d(q . k): the scale folded in
    }
    __syncthreads();
    // dq[i] = sum_j dS[i][j] k[j],  dk[j] = sum_i dS[i][j] q[i],  dv[j] = sum_i P[i][j] dO[i]; a lane owns columns lane, +64, +128
    for (int r = 0; r < N; ++r) {
        float dq[3] = {0.f, 0.f, 0.f}, dk[3] = {0.f, 0.f, 0.f}, dv[3] = {0.f, 0.f, 0.f};
        for (int o = 0; o < N; ++o) {
            const float a = ds[r][o], bT = ds[o][r], pT = ps[o][r];
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                dq[e] = fmaf(a, ks[o][lane + 64 * e], dq[e]);
                dk[e] = fmaf(bT, qs[o][lane + 64 * e], dk[e]);
                dv[e] = fmaf(pT, gs[o][lane + 64 * e], dv[e]);
            }
        }
        bf16_t* dst = dqkv + (s * N + r) * ld + (size_t)h * HD;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            dst[lane + 64 * e] = f2bf(dq[e]);
            dst[W + lane + 64 * e] = f2bf(dk[e]);
            dst[2 * W + lane + 64 * e] = f2bf(dv[e]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------
static inline int red_grid(int64_t rows) { return (int)((rows + ROW_WAVES - 1) / ROW_WAVES < RED_MAX_WG ? (rows + ROW_WAVES - 1) / ROW_WAVES : RED_MAX_WG); }

extern "C" int sed_fpool_seq_build_fwd(const float* x, const float* gamma, const float* beta, float eps, const float* tag_w,
                                       const float* tag_b, float* xs, float* mean, float* rstd, int Bx, int tp, int F,
                                       hipStream_t stream) {
    if (Bx < 1 || tp < 1 || F < 1 || F > 12 || (mean == nullptr) != (rstd == nullptr)) return SED_ERR_ARG;
    const int64_t R = (int64_t)Bx * tp * (1 + F);
    seq_build_fwd_kernel<<<cdiv(R, ROW_WAVES), 64 * ROW_WAVES, 0, stream>>>(x, gamma, beta, eps, tag_w, tag_b, xs, mean, rstd, tp, F, R);
    return sed_check_launch();
}

extern "C" int sed_fpool_seq_build_bwd(const float* dxs, const float* x, const float* mean, const float* rstd, const float* gamma,
                                       float* dx, float* dgamma, float* dbeta, float* dtag, float* partials, int64_t partial_floats,
                                       int Bx, int tp, int F, hipStream_t stream) {
    if (Bx < 1 || tp < 1 || F < 1 || F > 12) return SED_ERR_ARG;
    const int64_t R = (int64_t)Bx * tp * (1 + F);
    const int grid = red_grid(R);
    if (partials == nullptr || partial_floats < (int64_t)grid * 3 * DM) return SED_ERR_ARG;
    seq_build_bwd_kernel<<<grid, 64 * ROW_WAVES, 0, stream>>>(dxs, x, mean, rstd, gamma, dx, partials, tp, F, R);
    reduce_partials_kernel<<<cdiv(3 * DM, 256), 256, 0, stream>>>(partials, grid, 3, dgamma, dbeta, dtag);
    return sed_check_launch();
}

extern "C" int sed_fpool_rownorm_fwd(const float* xs, const float* gamma, const float* beta, float eps, float* pooled, float* mean,
                                     float* rstd, int S, int N, hipStream_t stream) {
    if (S < 1 || N < 1 || (mean == nullptr) != (rstd == nullptr)) return SED_ERR_ARG;
    rownorm_fwd_kernel<<<cdiv(S, ROW_WAVES), 64 * ROW_WAVES, 0, stream>>>(xs, gamma, beta, eps, pooled, mean, rstd, N, S);
    return sed_check_launch();
}

extern "C" int sed_fpool_rownorm_bwd(const float* dpooled, const float* xs, const float* mean, const float* rstd, const float* gamma,
                                     float* dxs, float* dgamma, float* dbeta, float* partials, int64_t partial_floats, int S, int N,
                                     hipStream_t stream) {
    if (S < 1 || N < 1) return SED_ERR_ARG;
    const int grid = red_grid(S);
    if (partials == nullptr || partial_floats < (int64_t)grid * 2 * DM) return SED_ERR_ARG;
    rownorm_bwd_kernel<<<grid, 64 * ROW_WAVES, 0, stream>>>(dpooled, xs, mean, rstd, gamma, dxs, partials, N, S);
    reduce_partials_kernel<<<cdiv(2 * DM, 256), 256, 0, stream>>>(partials, grid, 2, dgamma, dbeta, nullptr);
    return sed_check_launch();
}

extern "C" int sed_attn_short_fwd(const void* qkv, void* out, int S, int N, int H, int in_kind, int mode, hipStream_t stream) {
    if (S < 1 || N < 2 || N > NMAX || H < 1 || in_kind < 0 || in_kind > 2 || (int64_t)S * H > 0x7fffffff) return SED_ERR_ARG;
    if (mode != 0 && mode != 1 && mode != 4) return SED_ERR_ARG;
    attn_short_fwd_kernel<<<S * H, 64, 0, stream>>>(qkv, static_cast<bf16_t*>(out), N, H, in_kind, mode);
    return sed_check_launch();
}

extern "C" int sed_attn_short_bwd(const void* qkv, const void* dout, void* dqkv, int S, int N, int H, int in_kind, hipStream_t stream) {
    if (S < 1 || N < 2 || N > NMAX || H < 1 || in_kind < 0 || in_kind > 2 || (int64_t)S * H > 0x7fffffff) return SED_ERR_ARG;
    attn_short_bwd_kernel<<<S * H, 64, 0, stream>>>(qkv, static_cast<const bf16_t*>(dout), static_cast<bf16_t*>(dqkv), N, H, in_kind);
    return sed_check_launch();
}
