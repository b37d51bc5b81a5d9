// Frequency-dynamic convolution (FDY-CNN) of the PaSST_CNN branch: what a dynamic layer needs beyond the base branch's patch matrix, GEMMs,
// BatchNorm2d, ContextGating and pooling kernels (cnn_branch.hip).  Reference: src/models/cnn/FDY_cnn.py:7-116 (pool_dim 'freq', 4 basis kernels).
//
// A dynamic 3x3 layer is  y[b, o, h, w] = sum_k a[b, k, h] conv3x3(x; weight[k])[b, o, h, w]:  the four convolutions are ONE GEMM of the
// patch matrix against the [4 co, 9 cin] weight image (Y4, fp32 [pixels, 4 co]); the per-frame mixing weights a come from a small attention
// head on the mean of x over the mel bins.  Everything here works on R = B H frame rows of cin / hid / 4 values -- thousands of times
// fewer elements than the activations -- except the two mixing passes and the frequency mean, which stream the activations once.
//
// Every reduction is ordered (wave shuffles, LDS, per-block partials summed by one thread each): no float atomics, results are
// reproducible run to run.  The small dot products and all sums over the rows accumulate in double.
#include "common.h"
#include "../../include/sed_hip.h"

#define FDY_TR 16          // frame rows per workgroup of the attention-head kernels
#define FDY_K 4            // basis kernels (FDY_cnn.py:130)

// ---------------------------------------------------------------------------------------------------
// pm[r, c] = mean over the W mel bins of X[r, w, c]     (FDY_cnn.py:97; X 16-bit NHWC [R, W, Cp], channels C.. are padding)
// one workgroup per frame row; a thread owns 8 channels (one 16-byte load per bin) of every (256 / (C / 8))-th bin
// ---------------------------------------------------------------------------------------------------
template <bool F16>
__global__ __launch_bounds__(256) void fdy_freq_mean_kernel(const bf16_t* __restrict__ X, float* __restrict__ pm, int W, int C, int Cp) {
    extern __shared__ float red[];      // [wl][C]
    const int nv = C / 8, wl = 256 / nv;
    const int v = threadIdx.x % nv, l = threadIdx.x / nv;
    const size_t r = blockIdx.x;
    if (l < wl) {
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int w = l; w < W; w += wl) {
            const uint4 q = *reinterpret_cast<const uint4*>(X + (r * W + w) * Cp + v * 8);
            const unsigned qq[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                acc[2 * i] += to_f32<F16>((bf16_t)(qq[i] & 0xffff));
                acc[2 * i + 1] += to_f32<F16>((bf16_t)(qq[i] >> 16));
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) red[l * C + v * 8 + i] = acc[i];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float s = 0.f;
        for (int j = 0; j < wl; ++j) s += red[j * C + c];
        pm[r * C + c] = s / (float)W;
    }
}
extern "C" int sed_fdy_freq_mean(const void* X, int f16, float* pm, int64_t R, int W, int C, int Cp, hipStream_t stream) {
    (void)hipGetLastError();
    if (R <= 0 || R > 0x7fffffff || W <= 0 || C <= 0 || (C % 8) || C > 2048 || (Cp % 8) || Cp < C) return SED_ERR_ARG;
    const size_t lds = (size_t)(256 / (C / 8)) * C * sizeof(float);
    if (f16)
        hipLaunchKernelGGL(fdy_freq_mean_kernel<true>, dim3((unsigned)R), dim3(256), lds, stream, (const bf16_t*)X, pm, W, C, Cp);
    else
        hipLaunchKernelGGL(fdy_freq_mean_kernel<false>, dim3((unsigned)R), dim3(256), lds, stream, (const bf16_t*)X, pm, W, C, Cp);
    return sed_check_launch();
}

// ---------------------------------------------------------------------------------------------------
// Attention head, first launch: u[r, j] = sum_{t, c} W1[j, c, t] pm[(b, h + t - 1), c]   (Conv1d(cin -> hid, 3, padding 1, no bias) along
// the frames, FDY_cnn.py:78,107) and, for the batch statistics of the BatchNorm1d behind it, the per-workgroup sums of u and u^2
// (part [blocks, 2, hid] double).  A workgroup stages its 16 frame rows and their two neighbours in LDS.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fdy_taps_kernel(const float* __restrict__ pm, const float* __restrict__ W1, float* __restrict__ u,
                                                       double* __restrict__ part, int R, int H, int cin, int hid) {
    extern __shared__ float sm[];
    float* p = sm;                                  // [(FDY_TR + 2)][cin]: rows r0 - 1 .. r0 + FDY_TR
    float* uo = sm + (FDY_TR + 2) * cin;            // [FDY_TR][hid]
    const int r0 = blockIdx.x * FDY_TR;
    for (int i = threadIdx.x; i < (FDY_TR + 2) * cin; i += 256) {
        const int r = r0 - 1 + i / cin;
        p[i] = (r >= 0 && r < R) ? pm[(size_t)r * cin + i % cin] : 0.f;
    }
    __syncthreads();
    for (int o = threadIdx.x; o < FDY_TR * hid; o += 256) {
        const int rl = o / hid, j = o % hid, r = r0 + rl;
        float res = 0.f;
        if (r < R) {
            const int h = r % H;
            const bool v0 = h > 0, v2 = h < H - 1;        // the outer taps of a clip's first / last frame read the zero padding
            const float* w = W1 + (size_t)j * cin * 3;
            const float* pr = p + rl * cin;
            double acc = 0.0;
            for (int c = 0; c < cin; ++c) {
                const float a0 = v0 ? pr[c] : 0.f, a1 = pr[cin + c], a2 = v2 ? pr[2 * cin + c] : 0.f;
                acc += (double)w[3 * c] * a0 + (double)w[3 * c + 1] * a1 + (double)w[3 * c + 2] * a2;
            }
            res = (float)acc;
            u[(size_t)r * hid + j] = res;
        }
        uo[o] = res;
    }
    __syncthreads();
    if (part != nullptr) {
        for (int j = threadIdx.x; j < hid; j += 256) {
            double s1 = 0.0, s2 = 0.0;
            for (int rl = 0; rl < FDY_TR; ++rl) {
                const double v = uo[rl * hid + j];
                s1 += v;
                s2 += v * v;
            }
            part[((size_t)blockIdx.x * 2) * hid + j] = s1;
            part[((size_t)blockIdx.x * 2 + 1) * hid + j] = s2;
        }
    }
}
extern "C" int sed_fdy_attn_taps(const float* pm, const float* W1, float* u, double* part, int B, int H, int cin, int hid, hipStream_t stream) {
    (void)hipGetLastError();
    if (B <= 0 || H <= 0 || cin <= 0 || hid <= 0 || (int64_t)B * H > 0x7fffffff) return SED_ERR_ARG;
    const size_t lds = ((size_t)(FDY_TR + 2) * cin + (size_t)FDY_TR * hid) * sizeof(float);
    if (lds > 64 * 1024) return SED_ERR_ARG;
    const int R = B * H;
    hipLaunchKernelGGL(fdy_taps_kernel, dim3(cdiv(R, FDY_TR)), dim3(256), lds, stream, pm, W1, u, part, R, H, cin, hid);
    return sed_check_launch();
}

// ---------------------------------------------------------------------------------------------------
// Attention head, second launch: BatchNorm1d statistics (batch: from the partial sums, running statistics updated with torch's rule --
// momentum, unbiased variance; eval: the running statistics), then per frame row  n = relu((u - mean) rstd gamma + beta),
// a = softmax_k((W2 n + b2) / temperature)   (FDY_cnn.py:108-116).  aff [3, hid] = mean | rstd | gamma rstd is kept for the backward.
// ---------------------------------------------------------------------------------------------------
__global__ void fdy_bn1d_finalize_kernel(const double* __restrict__ part, int nblk, const float* __restrict__ gamma, float* __restrict__ run_mean,
                                         float* __restrict__ run_var, int R, int hid, float mom, float eps, float* __restrict__ aff) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= hid) return;
    double mean, var;
    if (part != nullptr) {
        double s1 = 0.0, s2 = 0.0;
        for (int b = 0; b < nblk; ++b) {
            s1 += part[((size_t)b * 2) * hid + j];
            s2 += part[((size_t)b * 2 + 1) * hid + j];
        }
        mean = s1 / (double)R;
        var = s2 / (double)R - mean * mean;
        if (var < 0.0) var = 0.0;
        run_mean[j] = (1.0f - mom) * run_mean[j] + mom * (float)mean;
        run_var[j] = (1.0f - mom) * run_var[j] + mom * (float)(var * (double)R / (double)(R - 1));
    } else {
        mean = run_mean[j];
        var = run_var[j];
    }
    const double rstd = 1.0 / sqrt(var + (double)eps);
    aff[j] = (float)mean;
    aff[hid + j] = (float)rstd;
    aff[2 * hid + j] = (float)((double)gamma[j] * rstd);
}
__global__ __launch_bounds__(256) void fdy_attn_softmax_kernel(const float* __restrict__ u, const float* __restrict__ aff,
                                                               const float* __restrict__ beta, const float* __restrict__ W2,
                                                               const float* __restrict__ b2, float inv_temp, float* __restrict__ att, int R,
                                                               int hid) {
    extern __shared__ float sm[];       // mean | a | beta | W2 [4, hid]
    for (int i = threadIdx.x; i < hid; i += 256) {
        sm[i] = aff[i];
        sm[hid + i] = aff[2 * hid + i];
        sm[2 * hid + i] = beta[i];
    }
    for (int i = threadIdx.x; i < FDY_K * hid; i += 256) sm[3 * hid + i] = W2[i];
    __syncthreads();
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    double l[FDY_K] = {b2[0], b2[1], b2[2], b2[3]};
    const float* ur = u + (size_t)r * hid;
    for (int j = 0; j < hid; ++j) {
        const float n = fmaxf(fmaf(ur[j] - sm[j], sm[hid + j], sm[2 * hid + j]), 0.f);
#pragma unroll
        for (int k = 0; k < FDY_K; ++k) l[k] += (double)sm[(3 + k) * hid + j] * n;
    }
    float z[FDY_K], mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < FDY_K; ++k) {
        z[k] = (float)l[k] * inv_temp;
        mx = fmaxf(mx, z[k]);
    }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < FDY_K; ++k) {
        z[k] = expf(z[k] - mx);
        s += z[k];
    }
    const float is = 1.0f / s;
    *reinterpret_cast<float4*>(att + (size_t)r * FDY_K) = make_float4(z[0] * is, z[1] * is, z[2] * is, z[3] * is);
}
extern "C" int sed_fdy_attn_softmax(const float* u, const double* part, const float* gamma, const float* beta, float* run_mean, float* run_var,
                                    const float* W2, const float* b2, float temperature, double momentum, double eps, float* aff, float* att,
                                    int R, int hid, hipStream_t stream) {
    (void)hipGetLastError();
    if (R <= 0 || hid <= 0 || !(temperature > 0.f) || (part != nullptr && R < 2)) return SED_ERR_ARG;
    const size_t lds = (size_t)(3 + FDY_K) * hid * sizeof(float);
    if (lds > 64 * 1024) return SED_ERR_ARG;
    hipLaunchKernelGGL(fdy_bn1d_finalize_kernel, dim3(cdiv(hid, 64)), dim3(64), 0, stream, part, cdiv(R, FDY_TR), gamma, run_mean, run_var, R, hid,
                       (float)momentum, (float)eps, aff);
    hipLaunchKernelGGL(fdy_attn_softmax_kernel, dim3(cdiv(R, 256)), dim3(256), lds, stream, u, aff, beta, W2, b2, 1.0f / temperature, att, R,
                       hid);
    return sed_check_launch();
}

// ---------------------------------------------------------------------------------------------------
// Mixing: Y[m, o] = sum_k a[m / W, k] Y4[m, k co + o]   (FDY_cnn.py:53-61).  Y4 fp32 [M, ld4] is the GEMM's output, Y fp32 [M, ldy] what
// the BatchNorm2d path reads (columns co.. zero).
// ---------------------------------------------------------------------------------------------------
__global__ void fdy_mix_fwd_kernel(const float* __restrict__ Y4, int ld4, const float* __restrict__ att, float* __restrict__ Y, int ldy,
                                   size_t M, int W, int co) {
    const int c4n = ldy / 4;
    const size_t total = M * c4n;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx % c4n) * 4;
        const size_t m = idx / c4n;
        float4 y = {0.f, 0.f, 0.f, 0.f};
        if (c < co) {
            const float4 a = *reinterpret_cast<const float4*>(att + (m / W) * FDY_K);
            const float* src = Y4 + m * ld4 + c;
            const float4 y0 = *reinterpret_cast<const float4*>(src), y1 = *reinterpret_cast<const float4*>(src + co);
            const float4 y2 = *reinterpret_cast<const float4*>(src + 2 * co), y3 = *reinterpret_cast<const float4*>(src + 3 * co);
            y.x = fmaf(a.w, y3.x, fmaf(a.z, y2.x, fmaf(a.y, y1.x, a.x * y0.x)));
            y.y = fmaf(a.w, y3.y, fmaf(a.z, y2.y, fmaf(a.y, y1.y, a.x * y0.y)));
            y.z = fmaf(a.w, y3.z, fmaf(a.z, y2.z, fmaf(a.y, y1.z, a.x * y0.z)));
            y.w = fmaf(a.w, y3.w, fmaf(a.z, y2.w, fmaf(a.y, y1.w, a.x * y0.w)));
        }
        *reinterpret_cast<float4*>(Y + m * ldy + c) = y;
    }
}
extern "C" int sed_fdy_mix_fwd(const float* Y4, int ld4, const float* att, float* Y, int ldy, int64_t M, int W, int co, hipStream_t stream) {
    (void)hipGetLastError();
    if (M <= 0 || W <= 0 || (M % W) || co <= 0 || (co % 4) || (ld4 % 4) || ld4 < FDY_K * co || (ldy % 4) || ldy < co) return SED_ERR_ARG;
    hipLaunchKernelGGL(fdy_mix_fwd_kernel, dim3(grid_for((size_t)M * (ldy / 4), 256, 16384)), dim3(256), 0, stream, Y4, ld4, att, Y, ldy, (size_t)M, W, co);
    return sed_check_launch();
}

// ---------------------------------------------------------------------------------------------------
// Mixing backward, one workgroup per frame row r = (b, h):  dY4[m, k co + o] = a[r, k] dY[m, o]  (bf16 [M, ldg4], the operand of the
// weight-gradient and input-gradient GEMMs; columns 4 co.. zero)  and  da[r, k] = sum_{w, o} dY[m, o] Y4[m, k co + o].
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fdy_mix_bwd_kernel(const bf16_t* __restrict__ dY, int ldo, const float* __restrict__ Y4, int ld4,
                                                          const float* __restrict__ att, bf16_t* __restrict__ dY4, int ldg4,
                                                          float* __restrict__ da, int W, int co) {
    const size_t r = blockIdx.x;
    const float4 a4 = *reinterpret_cast<const float4*>(att + r * FDY_K);
    const float a[FDY_K] = {a4.x, a4.y, a4.z, a4.w};
    const int c4n = co / 4, n = W * c4n;
    float s[FDY_K] = {0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < n; i += 256) {
        const int c = (i % c4n) * 4;
        const size_t m = r * W + i / c4n;
        const uint2 gq = *reinterpret_cast<const uint2*>(dY + m * ldo + c);
        const float g0 = bf2f((bf16_t)(gq.x & 0xffff)), g1 = bf2f((bf16_t)(gq.x >> 16));
        const float g2 = bf2f((bf16_t)(gq.y & 0xffff)), g3 = bf2f((bf16_t)(gq.y >> 16));
#pragma unroll
        for (int k = 0; k < FDY_K; ++k) {
            const float4 y = *reinterpret_cast<const float4*>(Y4 + m * ld4 + k * co + c);
            s[k] += g0 * y.x + g1 * y.y + g2 * y.z + g3 * y.w;
            uint2 o;
            o.x = pack2bf(a[k] * g0, a[k] * g1);
            o.y = pack2bf(a[k] * g2, a[k] * g3);
            *reinterpret_cast<uint2*>(dY4 + m * ldg4 + k * co + c) = o;
        }
    }
    const int p4n = (ldg4 - FDY_K * co) / 4;
    for (int i = threadIdx.x; i < W * p4n; i += 256)
        *reinterpret_cast<uint2*>(dY4 + (r * W + i / p4n) * ldg4 + FDY_K * co + (i % p4n) * 4) = make_uint2(0u, 0u);
    __shared__ float red[4][FDY_K];
#pragma unroll
    for (int k = 0; k < FDY_K; ++k) {
        const float t = wave_sum(s[k]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < FDY_K) da[r * FDY_K + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}
extern "C" int sed_fdy_mix_bwd(const void* dY, int ldo, const float* Y4, int ld4, const float* att, void* dY4, int ldg4, float* da, int64_t R,
                               int W, int co, hipStream_t stream) {
    (void)hipGetLastError();
    if (R <= 0 || R > 0x7fffffff || W <= 0 || co <= 0 || (co % 4) || (ldo % 4) || ldo < co || (ld4 % 4) || ld4 < FDY_K * co || (ldg4 % 4) ||
        ldg4 < FDY_K * co)
        return SED_ERR_ARG;
    hipLaunchKernelGGL(fdy_mix_bwd_kernel, dim3((unsigned)R), dim3(256), 0, stream, (const bf16_t*)dY, ldo, Y4, ld4, att, (bf16_t*)dY4, ldg4, da,
                       W, co);
    return sed_check_launch();
}

// ---------------------------------------------------------------------------------------------------
// Attention head backward: da [R, 4] -> d(pm) [R, cin] and the gradients of conv1d2 (W2, b2), the BatchNorm1d affine and conv1d1 (W1),
// added to the gradient views (any may be null: frozen).  batch_stats: the BatchNorm1d ran on batch statistics (training mode).
//   a   softmax / temperature, 1x1, ReLU per frame row -> dz (gradient of the BatchNorm1d output) and per-workgroup partial sums of
//       dW2 [4, hid] | db2 [4] | sum dz [hid] | sum dz xhat [hid]                                        (part [blocks, 6 hid + 4] double)
//   b   the partial sums in block order -> red (fp32) and the four small gradients
//   c   BatchNorm1d backward in place: dz -> du
//   d   dW1 [hid, cin, 3] = sum_r du[r, j] pm[(b, h + t - 1), c] over row slabs (wsW [slabs, hid 3 cin]), e: summed in slab order
//   f   d(pm)[r, c] = sum_{t, j} du[(b, h - t + 1), j] W1[j, c, t]
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fdy_attn_bwd_a_kernel(const float* __restrict__ da, const float* __restrict__ att,
                                                             const float* __restrict__ u, const float* __restrict__ aff,
                                                             const float* __restrict__ beta, const float* __restrict__ W2, float inv_temp,
                                                             float* __restrict__ dz, double* __restrict__ part, int R, int hid) {
    extern __shared__ float sm[];
    float* dl = sm;                             // [FDY_TR][4]   gradient of the 1x1 convolution's output
    float* nn = sm + FDY_TR * FDY_K;            // [FDY_TR][hid] ReLU output
    float* zz = nn + FDY_TR * hid;              // dz
    float* xh = zz + FDY_TR * hid;              // xhat
    const int r0 = blockIdx.x * FDY_TR;
    if (threadIdx.x < FDY_TR) {
        const int r = r0 + threadIdx.x;
        float d[FDY_K] = {0.f, 0.f, 0.f, 0.f};
        if (r < R) {
            const float4 a = *reinterpret_cast<const float4*>(att + (size_t)r * FDY_K), g = *reinterpret_cast<const float4*>(da + (size_t)r * FDY_K);
            const float dot = (a.x * g.x + a.y * g.y) + (a.z * g.z + a.w * g.w);
            d[0] = a.x * (g.x - dot) * inv_temp; d[1] = a.y * (g.y - dot) * inv_temp;
            d[2] = a.z * (g.z - dot) * inv_temp; d[3] = a.w * (g.w - dot) * inv_temp;
        }
#pragma unroll
        for (int k = 0; k < FDY_K; ++k) dl[threadIdx.x * FDY_K + k] = d[k];
    }
    __syncthreads();
    for (int o = threadIdx.x; o < FDY_TR * hid; o += 256) {
        const int rl = o / hid, j = o % hid, r = r0 + rl;
        float n = 0.f, z = 0.f, x = 0.f;
        if (r < R) {
            const float d = u[(size_t)r * hid + j] - aff[j];
            x = d * aff[hid + j];
            const float pre = fmaf(d, aff[2 * hid + j], beta[j]);
            n = fmaxf(pre, 0.f);
            if (pre > 0.f)
                z = (dl[rl * FDY_K] * W2[j] + dl[rl * FDY_K + 1] * W2[hid + j]) + (dl[rl * FDY_K + 2] * W2[2 * hid + j] + dl[rl * FDY_K + 3] * W2[3 * hid + j]);
            dz[(size_t)r * hid + j] = z;
        }
        nn[o] = n; zz[o] = z; xh[o] = x;
    }
    __syncthreads();
    const int P = 6 * hid + FDY_K;
    for (int e = threadIdx.x; e < P; e += 256) {
        double s = 0.0;
        if (e < FDY_K * hid) {
            const int k = e / hid, j = e % hid;
            for (int rl = 0; rl < FDY_TR; ++rl) s += (double)dl[rl * FDY_K + k] * nn[rl * hid + j];
        } else if (e < FDY_K * hid + FDY_K) {
            for (int rl = 0; rl < FDY_TR; ++rl) s += dl[rl * FDY_K + (e - FDY_K * hid)];
        } else if (e < 5 * hid + FDY_K) {
            const int j = e - FDY_K * hid - FDY_K;
            for (int rl = 0; rl < FDY_TR; ++rl) s += zz[rl * hid + j];
        } else {
            const int j = e - 5 * hid - FDY_K;
            for (int rl = 0; rl < FDY_TR; ++rl) s += (double)zz[rl * hid + j] * xh[rl * hid + j];
        }
        part[(size_t)blockIdx.x * P + e] = s;
    }
}
__global__ void fdy_attn_bwd_b_kernel(const double* __restrict__ part, int nblk, int hid, float* __restrict__ red, float* __restrict__ gW2,
                                      float* __restrict__ gb2, float* __restrict__ ggamma, float* __restrict__ gbeta) {
    const int P = 6 * hid + FDY_K;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= P) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += part[(size_t)b * P + e];
    const float v = (float)s;
    red[e] = v;
    if (e < FDY_K * hid) { if (gW2 != nullptr) gW2[e] += v; }
    else if (e < FDY_K * hid + FDY_K) { if (gb2 != nullptr) gb2[e - FDY_K * hid] += v; }
    else if (e < 5 * hid + FDY_K) { if (gbeta != nullptr) gbeta[e - FDY_K * hid - FDY_K] += v; }
    else if (ggamma != nullptr) ggamma[e - 5 * hid - FDY_K] += v;
}
__global__ void fdy_attn_bwd_c_kernel(float* __restrict__ dz, const float* __restrict__ u, const float* __restrict__ aff,
                                      const float* __restrict__ red, int R, int hid, int batch_stats) {
    const size_t total = (size_t)R * hid;
    const float invR = 1.0f / (float)R;
    const float* s1 = red + FDY_K * hid + FDY_K;
    const float* s2 = s1 + hid;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(idx % hid);
        float z = dz[idx];
        if (batch_stats) {
            const float x = (u[idx] - aff[j]) * aff[hid + j];
            z = z - s1[j] * invR - x * (s2[j] * invR);
        }
        dz[idx] = aff[2 * hid + j] * z;
    }
}
__global__ __launch_bounds__(256) void fdy_attn_bwd_d_kernel(const float* __restrict__ du, const float* __restrict__ pm, float* __restrict__ wsW,
                                                             int R, int H, int cin, int hid, int rows_per) {
    const int n = hid * 3 * cin;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int j = e / (3 * cin), t = (e % (3 * cin)) / cin, c = e % cin;     // c fastest: the pm reads of a wave are contiguous
    const int r_beg = blockIdx.y * rows_per, r_end = min(R, r_beg + rows_per);
    double acc = 0.0;
    for (int r = r_beg; r < r_end; ++r) {
        const int hh = r % H + t - 1;
        if (hh < 0 || hh >= H) continue;
        acc += (double)du[(size_t)r * hid + j] * pm[(size_t)(r + t - 1) * cin + c];
    }
    wsW[(size_t)blockIdx.y * n + ((size_t)j * cin + c) * 3 + t] = (float)acc;      // W1's own layout [hid, cin, 3]
}
__global__ void fdy_attn_bwd_e_kernel(const float* __restrict__ wsW, int nslab, int n, float* __restrict__ gW1) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    double s = 0.0;
    for (int b = 0; b < nslab; ++b) s += wsW[(size_t)b * n + e];
    gW1[e] += (float)s;
}
__global__ void fdy_attn_bwd_f_kernel(const float* __restrict__ du, const float* __restrict__ W1, float* __restrict__ dpm, int R, int H, int cin,
                                      int hid) {
    const size_t total = (size_t)R * cin;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx % cin), r = (int)(idx / cin), h = r % H;
        double acc = 0.0;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int hs = h - t + 1;          // the frame whose tap t read frame h
            if (hs < 0 || hs >= H) continue;
            const float* d = du + (size_t)(r - t + 1) * hid;
            for (int j = 0; j < hid; ++j) acc += (double)d[j] * W1[((size_t)j * cin + c) * 3 + t];
        }
        dpm[idx] = (float)acc;
    }
}
static inline int fdy_slabs(int R) {
    const int s = R / 128;
    return s < 1 ? 1 : (s > 32 ? 32 : s);
}
extern "C" int sed_fdy_attn_bwd(const float* da, const float* att, const float* u, const float* aff, const float* pm, const float* W1,
                                const float* beta, const float* W2, float temperature, int batch_stats, float* dz, double* part, float* ws,
                                int64_t ws_floats, float* dpm, float* gW1, float* ggamma, float* gbeta, float* gW2, float* gb2, int B, int H,
                                int cin, int hid, hipStream_t stream) {
    (void)hipGetLastError();
    if (B <= 0 || H <= 0 || cin <= 0 || hid <= 0 || (int64_t)B * H > 0x7fffffff || !(temperature > 0.f)) return SED_ERR_ARG;
    const int R = B * H, nblk = cdiv(R, FDY_TR), P = 6 * hid + FDY_K, nslab = fdy_slabs(R), n1 = hid * 3 * cin;
    const int Pe = (P + 3) / 4 * 4;
    if (ws_floats < (int64_t)Pe + (int64_t)nslab * n1) return SED_ERR_ARG;
    const size_t lds = ((size_t)FDY_TR * FDY_K + 3 * (size_t)FDY_TR * hid) * sizeof(float);
    if (lds > 64 * 1024) return SED_ERR_ARG;
    float* red = ws;
    float* wsW = ws + Pe;
    hipLaunchKernelGGL(fdy_attn_bwd_a_kernel, dim3(nblk), dim3(256), lds, stream, da, att, u, aff, beta, W2, 1.0f / temperature, dz, part, R, hid);
    hipLaunchKernelGGL(fdy_attn_bwd_b_kernel, dim3(cdiv(P, 64)), dim3(64), 0, stream, part, nblk, hid, red, gW2, gb2, ggamma, gbeta);
    hipLaunchKernelGGL(fdy_attn_bwd_c_kernel, dim3(grid_for((size_t)R * hid, 256, 16384)), dim3(256), 0, stream, dz, u, aff, red, R, hid, batch_stats);
    if (gW1 != nullptr) {
        const int rows_per = cdiv(R, nslab);
        hipLaunchKernelGGL(fdy_attn_bwd_d_kernel, dim3(cdiv(n1, 256), nslab), dim3(256), 0, stream, dz, pm, wsW, R, H, cin, hid, rows_per);
        hipLaunchKernelGGL(fdy_attn_bwd_e_kernel, dim3(cdiv(n1, 256)), dim3(256), 0, stream, wsW, nslab, n1, gW1);
    }
    hipLaunchKernelGGL(fdy_attn_bwd_f_kernel, dim3(grid_for((size_t)R * cin, 256, 16384)), dim3(256), 0, stream, dz, W1, dpm, R, H, cin, hid);
    return sed_check_launch();
}

// dX[r, w, c] += dpm[r, c] / W: the frequency mean's backward, added to the input gradient sed_col2im3x3 produced (fp32 [R, W, C])
__global__ void fdy_mean_bwd_add_kernel(float* __restrict__ dX, const float* __restrict__ dpm, size_t R, int W, int C) {
    const int c4n = C / 4;
    const size_t total = R * W * c4n;
    const float inv = 1.0f / (float)W;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx % c4n) * 4;
        const size_t m = idx / c4n;
        const float4 d = *reinterpret_cast<const float4*>(dpm + (m / W) * C + c);
        float4 x = *reinterpret_cast<float4*>(dX + m * C + c);
        x.x = fmaf(d.x, inv, x.x); x.y = fmaf(d.y, inv, x.y); x.z = fmaf(d.z, inv, x.z); x.w = fmaf(d.w, inv, x.w);
        *reinterpret_cast<float4*>(dX + m * C + c) = x;
    }
}
extern "C" int sed_fdy_mean_bwd_add(float* dX, const float* dpm, int64_t R, int W, int C, hipStream_t stream) {
    (void)hipGetLastError();
    if (R <= 0 || W <= 0 || C <= 0 || (C % 4)) return SED_ERR_ARG;
    hipLaunchKernelGGL(fdy_mean_bwd_add_kernel, dim3(grid_for((size_t)R * W * (C / 4), 256, 16384)), dim3(256), 0, stream, dX, dpm, (size_t)R, W, C);
    return sed_check_launch();
}
