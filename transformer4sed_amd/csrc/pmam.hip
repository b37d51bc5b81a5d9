// Width-generic and PMAM-specific HBM-bound kernels, every forward followed by its backward: LayerNorm and MLM masking of any width
// (the 384-wide context network; the masking pair is SedEngine's, engine.py), the per-frame attention pooling over the 12 frequency
// tokens, the projector merge (two linear interpolations + learned mixing weight), the prototype loss and the batched small-tensor
// gather / scatter.  Called by PmamEngine (pmam_engine.py).  The CNN branch is cnn_branch.hip, LoRA lora.hip, the narrow weight
// gradients dw_narrow.hip.  All fp32 math; 16-bit only as GEMM-operand outputs.
#include "common.h"
#include "../../include/sed_hip.h"

// ---------------------------------------------------------------------------------------------------
// LayerNorm of any width D (multiple of 128, <= 1024):  y = LN(in_scale * x) * gamma + beta.  One wave per row, float2 per
// lane per 128-column group, two-pass statistics in registers.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ln_fwd_any_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float eps, float in_scale,
                                                         bf16_t* __restrict__ y16, float* __restrict__ y32, float* __restrict__ mean,
                                                         float* __restrict__ rstd, int M, int D, int f16) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int G = D / 128;
    float2 v[8];
    float s = 0.f;
#pragma unroll
    for (int g = 0; g < 8; ++g)
        if (g < G) {
            v[g] = reinterpret_cast<const float2*>(x + (size_t)row * D)[lane + 64 * g];
            v[g].x *= in_scale; v[g].y *= in_scale;
            s += v[g].x + v[g].y;
        }
    const float mu = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int g = 0; g < 8; ++g)
        if (g < G) { v[g].x -= mu; v[g].y -= mu; q += v[g].x * v[g].x + v[g].y * v[g].y; }
    const float rs = rsqrtf(wave_sum(q) / (float)D + eps);
    if (lane == 0) {
        if (mean != nullptr) mean[row] = mu;
        if (rstd != nullptr) rstd[row] = rs;
    }
#pragma unroll
    for (int g = 0; g < 8; ++g)
        if (g < G) {
            const float2 ga = reinterpret_cast<const float2*>(gamma)[lane + 64 * g], be = reinterpret_cast<const float2*>(beta)[lane + 64 * g];
            const float a = v[g].x * rs * ga.x + be.x, b = v[g].y * rs * ga.y + be.y;
            if (y32 != nullptr) reinterpret_cast<float2*>(y32 + (size_t)row * D)[lane + 64 * g] = make_float2(a, b);
            if (y16 != nullptr)
                reinterpret_cast<unsigned*>(y16 + (size_t)row * D)[lane + 64 * g] = (unsigned)cvt16(a, f16) | ((unsigned)cvt16(b, f16) << 16);
        }
}
extern "C" int sed_ln_fwd_any(const float* x, const float* gamma, const float* beta, float eps, float in_scale, void* y16,
                              float* y32, float* mean, float* rstd, int M, int D, int f16, hipStream_t stream) {
    (void)hipGetLastError();
    if (M <= 0 || D <= 0 || (D % 128) || D > 1024) return SED_ERR_ARG;
    hipLaunchKernelGGL(ln_fwd_any_kernel, dim3(cdiv(M, 4)), dim3(256), 0, stream, x, gamma, beta, eps, in_scale, (bf16_t*)y16, y32, mean,
                       rstd, M, D, f16);
    return sed_check_launch();
}

// LayerNorm backward of any width (see layernorm_bwd_kernel): dx = in_scale * rstd * (dyg - mean(dyg) - xhat * mean(dyg * xhat)),
// dyg = dy * gamma; dx is ADDED into dx_acc when accumulate != 0; dgamma / dbeta (+=, nullable).
__global__ __launch_bounds__(256) void ln_bwd_any_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         const float* __restrict__ gamma, float in_scale, float* __restrict__ dx_acc,
                                                         int accumulate, float* __restrict__ dgamma, float* __restrict__ dbeta, int M,
                                                         int D) {
    __shared__ float red[4][1024];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, G = D / 128;
    float2 g[8], pg[8], pb[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        pg[k] = make_float2(0.f, 0.f); pb[k] = make_float2(0.f, 0.f);
        if (k < G) g[k] = reinterpret_cast<const float2*>(gamma)[lane + 64 * k];
    }
    for (int row = blockIdx.x * 4 + wave; row < M; row += gridDim.x * 4) {
        const float mu = mean[row], rs = rstd[row];
        float2 d[8], xh[8];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < G) {
                const float2 dv = reinterpret_cast<const float2*>(dy + (size_t)row * D)[lane + 64 * k];
                const float2 xv = reinterpret_cast<const float2*>(x + (size_t)row * D)[lane + 64 * k];
                xh[k] = make_float2((xv.x * in_scale - mu) * rs, (xv.y * in_scale - mu) * rs);
                pg[k].x += dv.x * xh[k].x; pg[k].y += dv.y * xh[k].y;
                pb[k].x += dv.x; pb[k].y += dv.y;
                d[k] = make_float2(dv.x * g[k].x, dv.y * g[k].y);
                s1 += d[k].x + d[k].y;
                s2 += d[k].x * xh[k].x + d[k].y * xh[k].y;
            }
        s1 = wave_sum(s1) / (float)D;
        s2 = wave_sum(s2) / (float)D;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < G) {
                float2* o = reinterpret_cast<float2*>(dx_acc + (size_t)row * D) + lane + 64 * k;
                float2 v = make_float2(in_scale * rs * (d[k].x - s1 - xh[k].x * s2), in_scale * rs * (d[k].y - s1 - xh[k].y * s2));
                if (accumulate) { const float2 old = *o; v.x += old.x; v.y += old.y; }
                *o = v;
            }
    }
    if (dgamma == nullptr) return;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < G) reinterpret_cast<float2*>(red[wave])[lane + 64 * k] = pass == 0 ? pg[k] : pb[k];
        __syncthreads();
        for (int c = threadIdx.x; c < D; c += 256)
            unsafeAtomicAdd(pass == 0 ? &dgamma[c] : &dbeta[c], red[0][c] + red[1][c] + red[2][c] + red[3][c]);
        __syncthreads();
    }
}
extern "C" int sed_ln_bwd_any(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                              float in_scale, float* dx, int accumulate, float* dgamma, float* dbeta, int M, int D,
                              hipStream_t stream) {
    (void)hipGetLastError();
    if (M <= 0 || D <= 0 || (D % 128) || D > 1024 || (dgamma == nullptr) != (dbeta == nullptr)) return SED_ERR_ARG;
    int blocks = cdiv(M, 4);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(ln_bwd_any_kernel, dim3(blocks), dim3(256), 0, stream, dy, x, mean, rstd, gamma, in_scale, dx, accumulate, dgamma,
                       dbeta, M, D);
    return sed_check_launch();
}

// MlmModule.setence_mask application for rows of any width C (multiple of 4); see sed_mlm_apply.
__global__ void mlm_apply_c_kernel(const float* __restrict__ x, const float* __restrict__ mask_token,
                                   const unsigned char* __restrict__ action, const int* __restrict__ src_idx,
                                   float* __restrict__ out, int rows, int C4) {
    const size_t total = (size_t)rows * C4;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int d4 = (int)(idx % C4);
        const int row = (int)(idx / C4);
        const unsigned char a = action[row];
        float4 v;
        if (a == 1) v = reinterpret_cast<const float4*>(mask_token)[d4];
        else if (a == 2) v = reinterpret_cast<const float4*>(x)[(size_t)src_idx[row] * C4 + d4];
        else v = reinterpret_cast<const float4*>(x)[idx];
        reinterpret_cast<float4*>(out)[idx] = v;
    }
}
extern "C" int sed_mlm_apply_c(const float* x, const float* mask_token, const uint8_t* action, const int* src_idx, float* out,
                               int rows, int C, hipStream_t stream) {
    (void)hipGetLastError();
    if (rows <= 0 || C <= 0 || (C % 4)) return SED_ERR_ARG;
    hipLaunchKernelGGL(mlm_apply_c_kernel, dim3(grid_for((size_t)rows * (C / 4))), dim3(256), 0, stream, x, mask_token, action, src_idx,
                       out, rows, C / 4);
    return sed_check_launch();
}

// backward of sed_mlm_apply_c: dx (zero-initialised) receives kept rows and the scatter of 'copy' rows, dtoken the 'mask' rows
__global__ __launch_bounds__(256) void mlm_apply_bwd_c_kernel(const float* __restrict__ dout, const unsigned char* __restrict__ action,
                                                              const int* __restrict__ src_idx, float* __restrict__ dx,
                                                              float* __restrict__ dtoken, int rows, int C) {
    // a workgroup walks a slab of rows with one thread per column (C <= 1024): the 'mask' rows (most of the masked frames) are summed
    // in registers and leave as ONE atomic per column and workgroup instead of one per element on the same C addresses
    float tok[4] = {0.f, 0.f, 0.f, 0.f};
    const int per = (rows + gridDim.x - 1) / gridDim.x, r0 = blockIdx.x * per, r1 = r0 + per < rows ? r0 + per : rows;
    for (int row = r0; row < r1; ++row) {
        const unsigned char a = action[row];
        const int src = a == 2 ? src_idx[row] : row;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int d = threadIdx.x + 256 * u;
            if (d >= C) break;
            const float g = dout[(size_t)row * C + d];
            if (a == 1) tok[u] += g;
            else unsafeAtomicAdd(&dx[(size_t)src * C + d], g);   // 'copy' rows scatter onto rows that also keep their own gradient
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int d = threadIdx.x + 256 * u;
        if (d < C && tok[u] != 0.f) unsafeAtomicAdd(&dtoken[d], tok[u]);
    }
}
extern "C" int sed_mlm_apply_bwd_c(const float* dout, const uint8_t* action, const int* src_idx, float* dx_zeroed, float* dtoken,
                                   int rows, int C, hipStream_t stream) {
    (void)hipGetLastError();
    if (rows <= 0 || C <= 0 || C > 1024) return SED_ERR_ARG;
    int blocks = rows < 2048 ? rows : 2048;
    hipLaunchKernelGGL(mlm_apply_bwd_c_kernel, dim3(blocks), dim3(256), 0, stream, dout, action, src_idx, dx_zeroed, dtoken, rows, C);
    return sed_check_launch();
}

// ---------------------------------------------------------------------------------------------------
// `attention` frequency pooling (src/models/pooling.py:37-51 with 6 heads of 128, passt_sed.py:211-215): for every (clip, time
// column) one learned query attends over the 12 frequency tokens.  kv [B*N, 1536] = (k | v) projections of the out_norm'ed tokens
// (rows b*N + 2 + f*tp + t), q [768] the projected query.  One wave per head, six waves per (b, t).
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(384) void fpool_attn_fwd_kernel(const bf16_t* __restrict__ kv, const float* __restrict__ q,
                                                             bf16_t* __restrict__ out16, float* __restrict__ out32,
                                                             float* __restrict__ probs, int N, int tp, int f16) {
    const int lane = threadIdx.x & 63, h = threadIdx.x >> 6;
    const int b = blockIdx.x / tp, t = blockIdx.x % tp;
    const float2 qq = reinterpret_cast<const float2*>(q + h * 128)[lane];
    float s[12];
    float mx = -3.0e38f;
#pragma unroll
    for (int f = 0; f < 12; ++f) {
        const bf16_t* row = kv + ((size_t)b * N + 2 + (size_t)f * tp + t) * 1536 + h * 128;
        const unsigned kk = reinterpret_cast<const unsigned*>(row)[lane];
        const float d = qq.x * ld16((bf16_t)(kk & 0xffff), f16) + qq.y * ld16((bf16_t)(kk >> 16), f16);
        s[f] = wave_sum(d) * 0.08838834764831845f;   // 1 / sqrt(128)
        mx = fmaxf(mx, s[f]);
    }
    float den = 0.f;
#pragma unroll
    for (int f = 0; f < 12; ++f) { s[f] = __expf(s[f] - mx); den += s[f]; }
    const float inv = 1.0f / den;
    float ox = 0.f, oy = 0.f;
#pragma unroll
    for (int f = 0; f < 12; ++f) {
        const float p = s[f] * inv;
        const bf16_t* row = kv + ((size_t)b * N + 2 + (size_t)f * tp + t) * 1536 + 768 + h * 128;
        const unsigned vv = reinterpret_cast<const unsigned*>(row)[lane];
        ox = fmaf(p, ld16((bf16_t)(vv & 0xffff), f16), ox);
        oy = fmaf(p, ld16((bf16_t)(vv >> 16), f16), oy);
        if (probs != nullptr && lane == 0) probs[((size_t)blockIdx.x * 6 + h) * 12 + f] = p;
    }
    const size_t o = (size_t)blockIdx.x * 768 + h * 128;
    if (out16 != nullptr) reinterpret_cast<unsigned*>(out16 + o)[lane] = (unsigned)cvt16(ox, f16) | ((unsigned)cvt16(oy, f16) << 16);
    if (out32 != nullptr) reinterpret_cast<float2*>(out32 + o)[lane] = make_float2(ox, oy);
}
extern "C" int sed_fpool_attn_fwd(const void* kv, const float* q, void* out16, float* out32, float* probs, int B, int N, int tp,
                                  int f16, hipStream_t stream) {
    (void)hipGetLastError();
    if (B <= 0 || tp <= 0 || N != 2 + 12 * tp) return SED_ERR_ARG;
    hipLaunchKernelGGL(fpool_attn_fwd_kernel, dim3(B * tp), dim3(384), 0, stream, (const bf16_t*)kv, q, (bf16_t*)out16, out32, probs, N,
                       tp, f16);
    return sed_check_launch();
}

// backward of sed_fpool_attn_fwd: dout [B*tp, 768] fp32 -> dkv bf16 [B*N, 1536] (the 12 token rows of the column; cls / dist rows
// of each clip zeroed by the t == 0 workgroups), dq [768] (+=).
__global__ __launch_bounds__(384) void fpool_attn_bwd_kernel(const bf16_t* __restrict__ kv, const float* __restrict__ q,
                                                             const float* __restrict__ probs, const float* __restrict__ dout,
                                                             bf16_t* __restrict__ dkv, float* __restrict__ dq, int N, int tp, int f16) {
    const int lane = threadIdx.x & 63, h = threadIdx.x >> 6;
    const int b = blockIdx.x / tp, t = blockIdx.x % tp;
    const float2 qq = reinterpret_cast<const float2*>(q + h * 128)[lane];
    const float2 go = reinterpret_cast<const float2*>(dout + (size_t)blockIdx.x * 768 + h * 128)[lane];
    float p[12], dp[12];
    float dot = 0.f;
#pragma unroll
    for (int f = 0; f < 12; ++f) {
        p[f] = probs[((size_t)blockIdx.x * 6 + h) * 12 + f];
        const bf16_t* row = kv + ((size_t)b * N + 2 + (size_t)f * tp + t) * 1536 + 768 + h * 128;
        const unsigned vv = reinterpret_cast<const unsigned*>(row)[lane];
        dp[f] = wave_sum(go.x * ld16((bf16_t)(vv & 0xffff), f16) + go.y * ld16((bf16_t)(vv >> 16), f16));
        dot += p[f] * dp[f];
    }
    float dqx = 0.f, dqy = 0.f;
#pragma unroll
    for (int f = 0; f < 12; ++f) {
        const float ds = p[f] * (dp[f] - dot) * 0.08838834764831845f;
        const size_t r = ((size_t)b * N + 2 + (size_t)f * tp + t) * 1536 + h * 128;
        const unsigned kk = reinterpret_cast<const unsigned*>(kv + r)[lane];
        dqx = fmaf(ds, ld16((bf16_t)(kk & 0xffff), f16), dqx);
        dqy = fmaf(ds, ld16((bf16_t)(kk >> 16), f16), dqy);
        reinterpret_cast<unsigned*>(dkv + r)[lane] = pack2bf(ds * qq.x, ds * qq.y);
        reinterpret_cast<unsigned*>(dkv + r + 768)[lane] = pack2bf(p[f] * go.x, p[f] * go.y);
    }
    unsafeAtomicAdd(&dq[h * 128 + 2 * lane], dqx);
    unsafeAtomicAdd(&dq[h * 128 + 2 * lane + 1], dqy);
    if (t == 0)
        for (int i = threadIdx.x; i < 2 * 1536 / 2; i += 384) reinterpret_cast<unsigned*>(dkv + (size_t)b * N * 1536)[i] = 0;
}
extern "C" int sed_fpool_attn_bwd(const void* kv, const float* q, const float* probs, const float* dout, void* dkv, float* dq,
                                  int B, int N, int tp, int f16, hipStream_t stream) {
    (void)hipGetLastError();
    if (B <= 0 || tp <= 0 || N != 2 + 12 * tp) return SED_ERR_ARG;
    hipLaunchKernelGGL(fpool_attn_bwd_kernel, dim3(B * tp), dim3(384), 0, stream, (const bf16_t*)kv, q, probs, dout, (bf16_t*)dkv, dq, N, tp,
                       f16);
    return sed_check_launch();
}

// ---------------------------------------------------------------------------------------------------
// Projector merge (passt_cnn.py:48-62, with both projections applied BEFORE the interpolations -- linear maps commute with the
// interpolation weights, which sum to one): out[b, j] = lerp_r1(pad(P1))[j] + mw * lerp_r2(P2)[j];  F.interpolate(mode='linear',
// align_corners=False) index arithmetic as in sed_interp_fwd.  P1 [B, tp1, C] is extended by `pad1` copies of its last frame.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void lerp_idx(int j, int ratio, int tin, int& i0, int& i1, float& lam) {
    float src = (float)(1.0 / (double)ratio) * ((float)j + 0.5f) - 0.5f;   // torch: scale * (dst + 0.5) - 0.5, scale = (float)(1 / scale_factor)
    src = src < 0.f ? 0.f : src;
    i0 = (int)src;
    i1 = i0 + 1 < tin ? i0 + 1 : tin - 1;
    lam = src - (float)i0;
}
__global__ void pmam_merge_kernel(const float* __restrict__ P1, const float* __restrict__ P2, const float* __restrict__ mw,
                                  float* __restrict__ out, int B, int tp1, int pad1, int r1, int tp2, int r2, int C4) {
    const int T = (tp1 + pad1) * r1;
    const size_t total = (size_t)B * T * C4;
    const float w = mw[0];
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int d4 = (int)(idx % C4);
        const int j = (int)((idx / C4) % T);
        const size_t b = idx / ((size_t)C4 * T);
        int a0, a1, c0, c1;
        float la, lc;
        lerp_idx(j, r1, tp1 + pad1, a0, a1, la);
        a0 = a0 < tp1 ? a0 : tp1 - 1;
        a1 = a1 < tp1 ? a1 : tp1 - 1;
        lerp_idx(j, r2, tp2, c0, c1, lc);
        const float4 x0 = reinterpret_cast<const float4*>(P1)[(b * tp1 + a0) * C4 + d4], x1 = reinterpret_cast<const float4*>(P1)[(b * tp1 + a1) * C4 + d4];
        const float4 y0 = reinterpret_cast<const float4*>(P2)[(b * tp2 + c0) * C4 + d4], y1 = reinterpret_cast<const float4*>(P2)[(b * tp2 + c1) * C4 + d4];
        float4 o;
        o.x = ((1.f - la) * x0.x + la * x1.x) + w * ((1.f - lc) * y0.x + lc * y1.x);
        o.y = ((1.f - la) * x0.y + la * x1.y) + w * ((1.f - lc) * y0.y + lc * y1.y);
        o.z = ((1.f - la) * x0.z + la * x1.z) + w * ((1.f - lc) * y0.z + lc * y1.z);
        o.w = ((1.f - la) * x0.w + la * x1.w) + w * ((1.f - lc) * y0.w + lc * y1.w);
        reinterpret_cast<float4*>(out)[idx] = o;
    }
}
extern "C" int sed_pmam_merge(const float* P1, const float* P2, const float* mw, float* out, int B, int tp1, int pad1, int r1,
                              int tp2, int r2, int C, hipStream_t stream) {
    (void)hipGetLastError();
    if (B <= 0 || (C % 4) || (tp1 + pad1) * r1 != tp2 * r2) return SED_ERR_ARG;
    hipLaunchKernelGGL(pmam_merge_kernel, dim3(grid_for((size_t)B * tp2 * r2 * (C / 4))), dim3(256), 0, stream, P1, P2, mw, out, B, tp1,
                       pad1, r1, tp2, r2, C / 4);
    return sed_check_launch();
}

// backward of sed_pmam_merge: dP1 [B, tp1, C], dP2 [B, tp2, C] (gather over the output frames each input frame feeds) and
// dmw[0] += sum(g * lerp_r2(P2)).  grid.y: 0 -> dP1, 1 -> dP2 (+ dmw).
__global__ void pmam_merge_bwd_kernel(const float* __restrict__ g, const float* __restrict__ P2, const float* __restrict__ mw,
                                      float* __restrict__ dP1, float* __restrict__ dP2, float* __restrict__ dmw, int B, int tp1,
                                      int pad1, int r1, int tp2, int r2, int C4) {
    const int T = (tp1 + pad1) * r1;
    const bool second = blockIdx.y == 1;
    const int tin = second ? tp2 : tp1, ratio = second ? r2 : r1, tlen = second ? tp2 : tp1 + pad1;
    const size_t total = (size_t)B * tin * C4;
    const float w = mw[0];
    double dw_part = 0.0;      // (the merge weight's gradient is a sum of ~10^6 products that cancel to ~10^-5 of their size: fp64 partials)
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int d4 = (int)(idx % C4);
        const int i = (int)((idx / C4) % tin);
        const size_t b = idx / ((size_t)C4 * tin);
        int jlo = (i - 2) * ratio, jhi = (i == tin - 1) ? T - 1 : (i + 2) * ratio;
        jlo = jlo < 0 ? 0 : jlo;
        jhi = jhi > T - 1 ? T - 1 : jhi;
        float4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int j = jlo; j <= jhi; ++j) {
            int i0, i1;
            float lam;
            lerp_idx(j, ratio, tlen, i0, i1, lam);
            i0 = i0 < tin ? i0 : tin - 1;
            i1 = i1 < tin ? i1 : tin - 1;
            float wt = 0.f;
            if (i0 == i) wt += 1.f - lam;
            if (i1 == i) wt += lam;
            if (wt != 0.f) {
                const float4 gv = reinterpret_cast<const float4*>(g)[(b * T + j) * C4 + d4];
                acc.x += wt * gv.x; acc.y += wt * gv.y; acc.z += wt * gv.z; acc.w += wt * gv.w;
            }
        }
        if (second) {
            const float4 p = reinterpret_cast<const float4*>(P2)[idx];
            dw_part += ((double)acc.x * p.x + (double)acc.y * p.y) + ((double)acc.z * p.z + (double)acc.w * p.w);    // sum_j g lerp(P2) = sum_i (lerp^T g)_i P2_i
            acc.x *= w; acc.y *= w; acc.z *= w; acc.w *= w;
            reinterpret_cast<float4*>(dP2)[idx] = acc;
        } else {
            reinterpret_cast<float4*>(dP1)[idx] = acc;
        }
    }
    if (second && dmw != nullptr) {
        __shared__ double wsum[4];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) dw_part += __shfl_xor(dw_part, o, 64);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = dw_part;
        __syncthreads();
        if (threadIdx.x == 0) unsafeAtomicAdd(dmw, (float)((wsum[0] + wsum[1]) + (wsum[2] + wsum[3])));
    }
}
extern "C" int sed_pmam_merge_bwd(const float* g, const float* P2, const float* mw, float* dP1, float* dP2, float* dmw, int B,
                                  int tp1, int pad1, int r1, int tp2, int r2, int C, hipStream_t stream) {
    (void)hipGetLastError();
    if (B <= 0 || (C % 4) || (tp1 + pad1) * r1 != tp2 * r2) return SED_ERR_ARG;
    hipLaunchKernelGGL(pmam_merge_bwd_kernel, dim3(grid_for((size_t)B * tp2 * (C / 4), 256, 2048), 2), dim3(256), 0, stream, g, P2, mw,
                       dP1, dP2, dmw, B, tp1, pad1, r1, tp2, r2, C / 4);
    return sed_check_launch();
}

// ---------------------------------------------------------------------------------------------------
// Prototype-similarity loss of the PMAM trainer (recipes/desed/pmam/train.py:82-87, 100-106): for every selected frame
//   z_c = 2 leaky_relu_0.2(cos(logit, proto_c)) - 1,  p_c = sigmoid(z_c / T),  loss = mean over (selected frames x classes) BCE(p, y)
// protos [C, 768] row-normalised by the caller side (F.normalize of the GMM means, train.py:31), labels [B, C, T], sel [B*T] bytes.
// One wave per frame; dlogit (nullable) receives d loss / d logit for selected rows, zeros elsewhere.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void proto_bce_kernel(const float* __restrict__ logit, const float* __restrict__ protos,
                                                        const float* __restrict__ labels, const unsigned char* __restrict__ sel,
                                                        float inv_count, const int* __restrict__ n_dev, float inv_temp,
                                                        float* __restrict__ loss, float* __restrict__ dlogit, float* __restrict__ post,
                                                        int rows, int T, int C) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (n_dev != nullptr) inv_count = 1.0f / (fmaxf((float)n_dev[0], 1.0f) * (float)C);   // count produced on the device: no host sync
    float lsum = 0.f;
    for (int row = blockIdx.x * 4 + wave; row < rows; row += gridDim.x * 4) {
        float4 x[3], gacc[3];
        if (!sel[row]) {
            if (dlogit != nullptr)
                for (int i = 0; i < 3; ++i) reinterpret_cast<float4*>(dlogit + (size_t)row * 768)[lane + 64 * i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (post != nullptr && lane < C) post[(size_t)row * C + lane] = 0.f;
            continue;
        }
        float nn = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            x[i] = reinterpret_cast<const float4*>(logit + (size_t)row * 768)[lane + 64 * i];
            nn += x[i].x * x[i].x + x[i].y * x[i].y + x[i].z * x[i].z + x[i].w * x[i].w;
            gacc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const float nrm = fmaxf(sqrtf(wave_sum(nn)), 1e-12f), rn = 1.0f / nrm;
        const int b = row / T, t = row - b * T;
        float sum_gc_cos = 0.f;
        for (int c = 0; c < C; ++c) {
            float4 pr[3];
            float d = 0.f;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                pr[i] = reinterpret_cast<const float4*>(protos + (size_t)c * 768)[lane + 64 * i];
                d += x[i].x * pr[i].x + x[i].y * pr[i].y + x[i].z * pr[i].z + x[i].w * pr[i].w;
            }
            const float cs = wave_sum(d) * rn;
            const float slope = cs > 0.f ? 2.f : 0.4f;
            const float z = (cs > 0.f ? cs : 0.2f * cs) * 2.f - 1.f;
            const float p = sigmoidf_(z * inv_temp);
            const float y = labels[((size_t)b * C + c) * T + t];
            if (post != nullptr && lane == 0) post[(size_t)row * C + c] = p;
            // torch BCELoss clamps each log at -100
            const float lp = fmaxf(__logf(p), -100.f), lq = fmaxf(__logf(1.f - p), -100.f);
            lsum += -(y * lp + (1.f - y) * lq);
            const float gc = (p - y) * inv_temp * slope * inv_count;      // d loss / d cos_c
            sum_gc_cos += gc * cs;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                gacc[i].x = fmaf(gc, pr[i].x, gacc[i].x); gacc[i].y = fmaf(gc, pr[i].y, gacc[i].y);
                gacc[i].z = fmaf(gc, pr[i].z, gacc[i].z); gacc[i].w = fmaf(gc, pr[i].w, gacc[i].w);
            }
        }
        if (dlogit != nullptr) {
            // d cos_c / d x = (proto_c - cos_c * xhat) / |x|
            const float k = sum_gc_cos * rn;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                float4 o;
                o.x = (gacc[i].x - k * x[i].x) * rn; o.y = (gacc[i].y - k * x[i].y) * rn;
                o.z = (gacc[i].z - k * x[i].z) * rn; o.w = (gacc[i].w - k * x[i].w) * rn;
                reinterpret_cast<float4*>(dlogit + (size_t)row * 768)[lane + 64 * i] = o;
            }
        }
    }
    if (lane == 0 && lsum != 0.f) unsafeAtomicAdd(loss, lsum * inv_count);
}
extern "C" int sed_proto_bce(const float* logit, const float* protos, const float* labels, const uint8_t* sel, int n_selected,
                             const int* n_selected_dev, float temperature, float* loss, float* dlogit, float* post, int B, int T,
                             int C, int D, hipStream_t stream) {
    (void)hipGetLastError();
    if (B <= 0 || T <= 0 || C <= 0 || C > 64 || D != 768 || (n_selected <= 0 && n_selected_dev == nullptr) || temperature <= 0.f)
        return SED_ERR_ARG;
    const int rows = B * T;
    int blocks = cdiv(rows, 4);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(proto_bce_kernel, dim3(blocks), dim3(256), 0, stream, logit, protos, labels, sel,
                       n_selected > 0 ? 1.0f / ((float)n_selected * (float)C) : 0.f, n_selected_dev, 1.0f / temperature, loss, dlogit, post,
                       rows, T, C);
    return sed_check_launch();
}

// ---------------------------------------------------------------------------------------------------
// Batched small-tensor plumbing of the PMAM step (round 4).  The padded fp32 vectors the kernels read (in_proj bias / pos_bias_u / v with
// 32-wide heads sitting in 64-wide slots, convolution and gate biases in 128-wide tiles) are gathers of the masters, and the gradients of
// every padded image go back to the masters through the same plan: ~230 torch index_select / mul / add_ launches per step as one launch
// each way.  desc: n_desc x 8 int64.
//   sed_gather_f32      {src fp32, plan int32 [n] (image element -> source element), scale fp32 [n] or 0, dst fp32 [n], n, first block, 0, 0}
//                       dst[e] = src[plan[e]] * scale[e]
//   sed_scatter_add_f32 {gimg fp32, plan int32 [n] or 0 (identity), scale fp32 [n] or 0, gmaster fp32, n, first block, C | ld_i << 32, ld_j}
//                       image element e = (i, j) = (e / C, e % C) read at gimg[i ld_i + j ld_j];  gmaster[plan[e]] += scale[e] * value
//                       for every e with scale[e] != 0 (the padding has scale 0; a plan is injective on the rest: no atomics)
// one workgroup per 256 elements.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ const long long* small_desc(const long long* desc, int n_desc) {
    int lo = 0, hi = n_desc - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[(size_t)mid * 8 + 5] <= (long long)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    return desc + (size_t)lo * 8;
}
__global__ __launch_bounds__(256) void gather_f32_kernel(const long long* __restrict__ desc, int n_desc) {
    const long long* d = small_desc(desc, n_desc);
    const float* src = reinterpret_cast<const float*>(d[0]);
    const int* plan = reinterpret_cast<const int*>(d[1]);
    const float* scale = reinterpret_cast<const float*>(d[2]);
    float* dst = reinterpret_cast<float*>(d[3]);
    const long long e = (long long)(blockIdx.x - (int)d[5]) * 256 + threadIdx.x;
    if (e >= d[4]) return;
    const float v = src[plan[e]];
    dst[e] = scale != nullptr ? v * scale[e] : v;
}
extern "C" int sed_gather_f32(const int64_t* desc, int n_desc, int total_blocks, hipStream_t stream) {
    (void)hipGetLastError();
    if (n_desc <= 0 || total_blocks <= 0) return SED_ERR_ARG;
    hipLaunchKernelGGL(gather_f32_kernel, dim3(total_blocks), dim3(256), 0, stream, (const long long*)desc, n_desc);
    return sed_check_launch();
}
__global__ __launch_bounds__(256) void scatter_add_f32_kernel(const long long* __restrict__ desc, int n_desc) {
    const long long* d = small_desc(desc, n_desc);
    const float* gimg = reinterpret_cast<const float*>(d[0]);
    const int* plan = reinterpret_cast<const int*>(d[1]);
    const float* scale = reinterpret_cast<const float*>(d[2]);
    float* gm = reinterpret_cast<float*>(d[3]);
    const long long e = (long long)(blockIdx.x - (int)d[5]) * 256 + threadIdx.x;
    if (e >= d[4]) return;
    float sc = 1.0f;
    if (scale != nullptr) {
        sc = scale[e];
        if (sc == 0.0f) return;
    }
    const int C = (int)(d[6] & 0xffffffffll);
    const long long ld_i = d[6] >> 32, ld_j = d[7];
    const long long i = e / C, j = e - i * C;
    gm[plan != nullptr ? (long long)plan[e] : e] += sc * gimg[i * ld_i + j * ld_j];
}
extern "C" int sed_scatter_add_f32(const int64_t* desc, int n_desc, int total_blocks, hipStream_t stream) {
    (void)hipGetLastError();
    if (n_desc <= 0 || total_blocks <= 0) return SED_ERR_ARG;
    hipLaunchKernelGGL(scatter_add_f32_kernel, dim3(total_blocks), dim3(256), 0, stream, (const long long*)desc, n_desc);
    return sed_check_launch();
}
