// Conformer context network (src/models/transformer/conformer.py): the middle of the convolution module as one kernel per direction,
//   x [B T, 2 C] --GLU--> u --depthwise conv along time (31 taps, zero "same" padding inside a clip)--> c --LayerNorm--> n --Swish--> y,
// the Swish of the two feed-forwards, and the scaling of the residual stream.  All fp32 math, IEEE semantics (no fast-math: this file
// is built like norm_elem.hip); 16-bit only as GEMM-operand outputs.
//
// Tiling.  C = 768 is fixed, a workgroup has 768 threads (12 waves).  It owns TT = 20 consecutive frames of one clip.
//   * depthwise phase: thread = channel.  The convolution of a channel touches that channel only, so the 50 GLU values a thread needs
//     (20 frames + 15 halo frames on each side, zero outside the clip) stay in ITS registers; each is used by up to 31 outputs.  Neither
//     u nor c goes to memory on the way.
//   * LayerNorm phase: wave = frame, 12 channels per lane.  The frame's 768 convolution outputs cross from the channel-owning threads to
//     the frame-owning wave through LDS ([20][768] fp32 forward; the backward keeps d c for 50 frames there, 150 KB of the 160 KB).
#include "common.h"
#include "rows768.h"
#include "../../include/sed_hip.h"

#define KW 31
#define HALO 15
#define TT 20
#define TR (TT + 2 * HALO)
#define NWAVE (DM / 64)
#define BWD_MAX_WG 256          // workgroups of the backward: each leaves ONE partial of every parameter gradient
#define BWD_SLOTS (KW + 3)      // per channel: 31 taps, depthwise bias, LayerNorm weight, LayerNorm bias

__device__ __forceinline__ float sigmoid_acc(float x) { return 1.0f / (1.0f + expf(-x)); }

// 16-bit operand row of 768 values held 4 per lane per float4 (lane + 64 i): mode 0 bf16, 1 f16, 4 split precision [hi | lo | hi] f16
__device__ __forceinline__ void store_operand_row(const float4* v, bf16_t* y16, size_t row, int lane, int mode) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const float4 q = v[i];
        if (mode == 4) {
            const bf16_t h0 = f2h(q.x), h1 = f2h(q.y), h2 = f2h(q.z), h3 = f2h(q.w);
            uint2 hi, lo;
            hi.x = (unsigned)h0 | ((unsigned)h1 << 16); hi.y = (unsigned)h2 | ((unsigned)h3 << 16);
            lo.x = pack2h(q.x - h2f(h0), q.y - h2f(h1)); lo.y = pack2h(q.z - h2f(h2), q.w - h2f(h3));
            uint2* p = reinterpret_cast<uint2*>(y16 + row * 3 * DM) + lane + 64 * i;
            p[0] = hi; p[DM / 4] = lo; p[2 * (DM / 4)] = hi;
        } else {
            uint2 pk;
            pk.x = mode ? pack2h(q.x, q.y) : pack2bf(q.x, q.y);
            pk.y = mode ? pack2h(q.z, q.w) : pack2bf(q.z, q.w);
            reinterpret_cast<uint2*>(y16 + row * DM)[lane + 64 * i] = pk;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DM) void conv_glu_dw_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ bias, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float eps, bf16_t* __restrict__ y16,
                                                            float* __restrict__ y32, float* __restrict__ conv, float* __restrict__ mean,
                                                            float* __restrict__ rstd, int T, int tiles_per_clip, int mode) {
    __shared__ float cs[TT][DM];
    const int c = threadIdx.x;
    const int b = blockIdx.x / tiles_per_clip, t0 = (blockIdx.x % tiles_per_clip) * TT;
    const float* xb = x + (size_t)b * T * (2 * DM);
    float wk[KW];
#pragma unroll
    for (int k = 0; k < KW; ++k) wk[k] = w[c * KW + k];
    // GLU of the tile and its halo: u = a * sigmoid(g), zero outside the clip (the convolution's padding)
    float u[TR];
#pragma unroll
    for (int r = 0; r < TR; ++r) {
        const int t = t0 - HALO + r;
        float v = 0.f;
        if (t >= 0 && t < T) {
            const float a = xb[(size_t)t * (2 * DM) + c];
            const float g = xb[(size_t)t * (2 * DM) + DM + c];
            v = a * sigmoid_acc(g);
        }
        u[r] = v;
    }
    const float bc = bias[c];
#pragma unroll
    for (int i = 0; i < TT; ++i) {
        float acc = bc;
#pragma unroll
        for (int k = 0; k < KW; ++k) acc = fmaf(wk[k], u[i + k], acc);      // c[t] = bias + sum_k w[k] u[t + k - 15]
        cs[i][c] = acc;
    }
    __syncthreads();
    // LayerNorm over the channels + Swish, one wave per frame
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float4 g4[NV], b4[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        g4[i] = reinterpret_cast<const float4*>(gamma)[lane + 64 * i];
        b4[i] = reinterpret_cast<const float4*>(beta)[lane + 64 * i];
    }
    for (int i = wave; i < TT; i += NWAVE) {
        const int t = t0 + i;
        if (t >= T) break;
        const size_t row = (size_t)b * T + t;
        float4 v[NV];
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            v[j] = reinterpret_cast<const float4*>(cs[i])[lane + 64 * j];
            s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
        }
        const float mu = wave_sum(s) * (1.0f / DM);
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float d = f4(v[j], e) - mu; q = fmaf(d, d, q); }
        const float rs = rsqrtf(wave_sum(q) * (1.0f / DM) + eps);
        if (conv != nullptr) {      // training: what the backward reads (u is recomputed from x there, n from c and the statistics)
#pragma unroll
            for (int j = 0; j < NV; ++j) reinterpret_cast<float4*>(conv + row * DM)[lane + 64 * j] = v[j];
            if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
        }
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float n = (f4(v[j], e) - mu) * rs * f4(g4[j], e) + f4(b4[j], e);
                f4(v[j], e) = n * sigmoid_acc(n);
            }
        if (y16 != nullptr) store_operand_row(v, y16, row, lane, mode);
        if (y32 != nullptr) {
#pragma unroll
            for (int j = 0; j < NV; ++j) reinterpret_cast<float4*>(y32 + row * DM)[lane + 64 * j] = v[j];
        }
    }
}

extern "C" int sed_conv_glu_dw_fwd(const float* x, const float* w, const float* bias, const float* gamma, const float* beta, float eps,
                                   void* y16, float* y32, float* conv, float* mean, float* rstd, int B, int T, int C, int mode,
                                   hipStream_t stream) {
    (void)hipGetLastError();
    if (C != DM || B <= 0 || T <= 0 || (mode != 0 && mode != 1 && mode != 4) || (y16 == nullptr && y32 == nullptr)) return SED_ERR_ARG;
    if (conv != nullptr && (mean == nullptr || rstd == nullptr)) return SED_ERR_ARG;
    const int tiles = cdiv(T, TT);
    if ((int64_t)B * tiles > 0x7fffffff) return SED_ERR_ARG;
    hipLaunchKernelGGL(conv_glu_dw_fwd_kernel, dim3(B * tiles), dim3(DM), 0, stream, x, w, bias, gamma, beta, eps, (bf16_t*)y16, y32, conv,
                       mean, rstd, T, tiles, mode);
    return sed_check_launch();
}

// ---------------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------------
// Phase A (wave = frame, the tile and its halo): Swish' and the LayerNorm backward give d c of 50 frames in LDS (zero outside the clip).
// Phase B (thread = channel), per owned frame, from the channel's column of d c in LDS:
//     d u[t]  = sum_k w[k] d c[t - k + 15]                (correlation with the flipped taps, same zero padding)
//     d w[k] += u[t] d c[t - k + 15]                      (each (frame of u, tap) pair is visited by exactly one workgroup)
//     d a = d u sigmoid(g),  d g = d u a sigmoid(g) (1 - sigmoid(g))
// The parameter gradients (taps, depthwise bias, LayerNorm weight and bias) are sums over all B T frames: every thread keeps its
// channel's partial sums in registers over the tiles its workgroup walks (a fixed assignment: tile = workgroup + i * grid) and stores
// them once; conv_bwd_reduce_kernel adds the <= 256 partials of a value in workgroup order.  No atomics: the result is the same bits
// in every run.
__global__ __launch_bounds__(DM) void conv_glu_dw_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                            const float* __restrict__ conv, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, const float* __restrict__ w,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            bf16_t* __restrict__ dx16, float* __restrict__ part, int T,
                                                            int tiles_per_clip, int ntiles) {
    extern __shared__ float dc[];       // [TR][DM]
    const int c = threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float wk[KW], dwk[KW];
#pragma unroll
    for (int k = 0; k < KW; ++k) { wk[k] = w[c * KW + k]; dwk[k] = 0.f; }
    float dbs = 0.f, dgm = 0.f, dbt = 0.f;
    const float gc = gamma[c], btc = beta[c];
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int b = tile / tiles_per_clip, t0 = (tile % tiles_per_clip) * TT;
        {
            float4 g4[NV], b4[NV];
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                g4[j] = reinterpret_cast<const float4*>(gamma)[lane + 64 * j];
                b4[j] = reinterpret_cast<const float4*>(beta)[lane + 64 * j];
            }
            for (int r = wave; r < TR; r += NWAVE) {
                const int t = t0 - HALO + r;
                float4 d[NV], xh[NV];
                if (t < 0 || t >= T) {
#pragma unroll
                    for (int j = 0; j < NV; ++j) reinterpret_cast<float4*>(dc + r * DM)[lane + 64 * j] = make_float4(0.f, 0.f, 0.f, 0.f);
                    continue;
                }
                const size_t row = (size_t)b * T + t;
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    d[j] = reinterpret_cast<const float4*>(dy + row * DM)[lane + 64 * j];
                    xh[j] = reinterpret_cast<const float4*>(conv + row * DM)[lane + 64 * j];
                }
                const float mu = mean[row], rs = rstd[row];
                float s1 = 0.f, s2 = 0.f;
#pragma unroll
                for (int j = 0; j < NV; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float h = (f4(xh[j], e) - mu) * rs;
                        const float n = h * f4(g4[j], e) + f4(b4[j], e);
                        const float s = sigmoid_acc(n);
                        const float dn = f4(d[j], e) * (s + n * s * (1.0f - s));       // Swish'(n)
                        const float dg = dn * f4(g4[j], e);
                        f4(d[j], e) = dg;
                        f4(xh[j], e) = h;
                        s1 += dg;
                        s2 = fmaf(dg, h, s2);
                    }
                s1 = wave_sum(s1) * (1.0f / DM);
                s2 = wave_sum(s2) * (1.0f / DM);
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    float4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) f4(o, e) = rs * (f4(d[j], e) - s1 - f4(xh[j], e) * s2);
                    reinterpret_cast<float4*>(dc + r * DM)[lane + 64 * j] = o;
                }
            }
        }
        __syncthreads();
        // (the channel's d c column is read from LDS per use, consecutive lanes on consecutive words: holding its 50 values in registers
        //  beside the 31 taps and their 31 gradient sums spilled)
#pragma unroll 2
        for (int i = 0; i < TT; ++i) {
            const int t = t0 + i;
            if (t >= T) break;
            const size_t row = (size_t)b * T + t;
            const float* dcp = dc + (i + 2 * HALO) * DM + c;        // d c of frame t + 15; frame t - k + 15 is k rows back
            const float a = x[row * (2 * DM) + c], g = x[row * (2 * DM) + DM + c];
            const float cv = conv[row * DM + c], dyv = dy[row * DM + c];
            const float sg = sigmoid_acc(g);
            const float u = a * sg;
            float du = 0.f;
#pragma unroll
            for (int k = 0; k < KW; ++k) {
                const float v = dcp[-k * DM];
                du = fmaf(wk[k], v, du);
                dwk[k] = fmaf(u, v, dwk[k]);
            }
            dbs += dcp[-HALO * DM];
            // LayerNorm weight / bias gradients of this frame and channel: d n recomputed from the (cached) rows phase A just read
            const float h = (cv - mean[row]) * rstd[row];
            const float n = h * gc + btc;
            const float s = sigmoid_acc(n);
            const float dn = dyv * (s + n * s * (1.0f - s));
            dgm = fmaf(dn, h, dgm);
            dbt += dn;
            dx16[row * (2 * DM) + c] = f2bf(du * sg);
            dx16[row * (2 * DM) + DM + c] = f2bf(du * a * sg * (1.0f - sg));
        }
        __syncthreads();        // the next tile overwrites d c
    }
    float* p = part + (size_t)blockIdx.x * BWD_SLOTS * DM + c;
#pragma unroll
    for (int k = 0; k < KW; ++k) p[k * DM] = dwk[k];
    p[KW * DM] = dbs;
    p[(KW + 1) * DM] = dgm;
    p[(KW + 2) * DM] = dbt;
}

// out += sum over the workgroups' partials, in workgroup order (one thread per value)
__global__ __launch_bounds__(256) void conv_bwd_reduce_kernel(const float* __restrict__ part, int nwg, float* __restrict__ dw,
                                                              float* __restrict__ dbias, float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= BWD_SLOTS * DM) return;
    const int slot = idx / DM, c = idx % DM;
    float* out = slot < KW ? (dw != nullptr ? dw + c * KW + slot : nullptr)
                           : (slot == KW ? dbias : (slot == KW + 1 ? dgamma : dbeta));
    if (out == nullptr) return;
    if (slot >= KW) out += c;
    float s = 0.f;
    for (int g = 0; g < nwg; ++g) s += part[(size_t)g * BWD_SLOTS * DM + idx];
    *out += s;
}

extern "C" int sed_conv_glu_dw_bwd(const float* dy, const float* x, const float* conv, const float* mean, const float* rstd,
                                   const float* w, const float* gamma, const float* beta, void* dx16, float* dw, float* dbias,
                                   float* dgamma, float* dbeta, float* partials, int64_t partial_floats, int B, int T, int C,
                                   hipStream_t stream) {
    (void)hipGetLastError();
    if (C != DM || B <= 0 || T <= 0 || dx16 == nullptr || partials == nullptr) return SED_ERR_ARG;
    const int tiles = cdiv(T, TT);
    if ((int64_t)B * tiles > 0x7fffffff) return SED_ERR_ARG;
    const int ntiles = B * tiles;
    const int nwg = ntiles < BWD_MAX_WG ? ntiles : BWD_MAX_WG;
    if (partial_floats < (int64_t)nwg * BWD_SLOTS * DM) return SED_ERR_ARG;
    const int lds = TR * DM * (int)sizeof(float);
    static bool attr = false;
    if (!attr) { (void)hipFuncSetAttribute((const void*)conv_glu_dw_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds); attr = true; }
    hipLaunchKernelGGL(conv_glu_dw_bwd_kernel, dim3(nwg), dim3(DM), lds, stream, dy, x, conv, mean, rstd, w, gamma, beta, (bf16_t*)dx16,
                       partials, T, tiles, ntiles);
    int rc = sed_check_launch();
    if (rc != SED_OK) return rc;
    hipLaunchKernelGGL(conv_bwd_reduce_kernel, dim3(cdiv(BWD_SLOTS * DM, 256)), dim3(256), 0, stream, partials, nwg, dw, dbias, dgamma,
                       dbeta);
    return sed_check_launch();
}

// ---------------------------------------------------------------------------------------------------
// Swish of the feed-forwards (Linear -> x sigmoid(x) -> Linear), elementwise between the two GEMMs
// ---------------------------------------------------------------------------------------------------
// h fp32 [M, 768] -> 16-bit operand image of h sigmoid(h) (mode as above) and / or the fp32 value
__global__ __launch_bounds__(256) void swish_fwd_kernel(const float* __restrict__ h, bf16_t* __restrict__ y16, float* __restrict__ y32,
                                                        int M, int mode) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    Row v;
#pragma unroll
    for (int j = 0; j < NV; ++j) {      // (load and Swish per float4: a row_load in front of the loop costs a register)
        v.v[j] = reinterpret_cast<const float4*>(h + (size_t)row * DM)[lane + 64 * j];
#pragma unroll
        for (int e = 0; e < 4; ++e) f4(v.v[j], e) = f4(v.v[j], e) * sigmoid_acc(f4(v.v[j], e));
    }
    if (y16 != nullptr) store_operand_row(v.v, y16, (size_t)row, lane, mode);
    if (y32 != nullptr) row_store(v, y32 + (size_t)row * DM, lane);
}

extern "C" int sed_swish_fwd(const float* h, void* y16, float* y32, int M, int C, int mode, hipStream_t stream) {
    (void)hipGetLastError();
    if (C != DM || M <= 0 || (mode != 0 && mode != 1 && mode != 4) || (y16 == nullptr && y32 == nullptr)) return SED_ERR_ARG;
    hipLaunchKernelGGL(swish_fwd_kernel, dim3(cdiv(M, 4)), dim3(256), 0, stream, h, (bf16_t*)y16, y32, M, mode);
    return sed_check_launch();
}

// dh16 = bf16(dy * Swish'(h)): the dY operand of the first Linear's weight-gradient and dX GEMMs
__global__ __launch_bounds__(256) void swish_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ h,
                                                        bf16_t* __restrict__ dh16, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 d = reinterpret_cast<const float4*>(dy)[i];
        float4 v = reinterpret_cast<const float4*>(h)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float xv = f4(v, e), s = sigmoid_acc(xv);
            f4(v, e) = reinterpret_cast<const float*>(&d)[e] * (s + xv * s * (1.0f - s));
        }
        uint2 pk;
        pk.x = pack2bf(v.x, v.y); pk.y = pack2bf(v.z, v.w);
        reinterpret_cast<uint2*>(dh16)[i] = pk;
    }
}

extern "C" int sed_swish_bwd(const float* dy, const float* h, void* dh16, int64_t n, hipStream_t stream) {
    (void)hipGetLastError();
    if (n <= 0 || n % 4 || dh16 == nullptr) return SED_ERR_ARG;
    int64_t blocks = (n / 4 + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(swish_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, dy, h, (bf16_t*)dh16, n / 4);
    return sed_check_launch();
}

// out = res + scale * in (res nullable: out = scale * in), optionally also out16 = bf16(out): the sqrt(d) scaling of the
// relative positional encoding (whose result IS the residual stream here), the half-step feed-forward residuals, and the halved
// gradient operand of their backward.  In place allowed (out == in or out == res).
__global__ __launch_bounds__(256) void scale_add_kernel(const float* in, const float* res, float* out, bf16_t* __restrict__ out16,
                                                        int64_t n4, float scale) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 v = reinterpret_cast<const float4*>(in)[i];
        v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
        if (res != nullptr) {
            const float4 r = reinterpret_cast<const float4*>(res)[i];
            v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
        }
        if (out != nullptr) reinterpret_cast<float4*>(out)[i] = v;
        if (out16 != nullptr) {
            uint2 pk;
            pk.x = pack2bf(v.x, v.y); pk.y = pack2bf(v.z, v.w);
            reinterpret_cast<uint2*>(out16)[i] = pk;
        }
    }
}

extern "C" int sed_scale_add_f32(const float* in, const float* res, float* out, void* out16, int64_t n, float scale,
                                 hipStream_t stream) {
    (void)hipGetLastError();
    if (n <= 0 || n % 4 || (out == nullptr && out16 == nullptr)) return SED_ERR_ARG;
    int64_t blocks = (n / 4 + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(scale_add_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, in, res, out, (bf16_t*)out16, n / 4, scale);
    return sed_check_launch();
}
