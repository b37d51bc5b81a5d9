// The CNN branch of PaSST_CNN around its im2col GEMMs, in the order of a layer and every forward followed by its backward: patch gather
// and its transpose (layer 0 direct), column statistics, BatchNorm2d (finalize, affine, backward), ContextGating + dropout + average
// pooling, the dropout keep-masks.  Called by PmamEngine (pmam_engine.py) for the base branch and for the FDY-CNN branch, which adds
// fdy_cnn.hip.  fp32 math, 16-bit only as GEMM-operand outputs; built with the flags of pmam.hip, the file they came from.
#include "common.h"
#include "../../include/sed_hip.h"

// ---------------------------------------------------------------------------------------------------
// CNN branch (src/models/cnn/base.py:62-113).  Activations are NHWC 16-bit [B, H = time, W = freq, Cp] with the channel
// count padded to a multiple of 64 (zeros), so that every convolution is one im2col gather + one NT GEMM.
// ---------------------------------------------------------------------------------------------------
// layer 0: mel [B, 128, T] fp32 -> col [B*T*128, 64]: 9 taps (time-major: tap = 3 * (dt + 1) + (df + 1)) + 55 zero columns
__global__ void conv0_im2col_kernel(const float* __restrict__ mel, bf16_t* __restrict__ col, int B, int T, int f16) {
    const size_t total = (size_t)B * T * 128;
    for (size_t m = (size_t)blockIdx.x * blockDim.x + threadIdx.x; m < total; m += (size_t)gridDim.x * blockDim.x) {
        const int f = (int)(m % 128);
        const int t = (int)((m / 128) % T);
        const int b = (int)(m / ((size_t)128 * T));
        bf16_t v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = 0;
#pragma unroll
        for (int dt = -1; dt <= 1; ++dt)
#pragma unroll
            for (int df = -1; df <= 1; ++df) {
                const int tt = t + dt, ff = f + df;
                float x = 0.f;
                if (tt >= 0 && tt < T && ff >= 0 && ff < 128) x = mel[((size_t)b * 128 + ff) * T + tt];
                v[3 * (dt + 1) + (df + 1)] = cvt16(x, f16);
            }
        uint4* dst = reinterpret_cast<uint4*>(col + m * 64);
        uint4 p0, p1;
        p0.x = (unsigned)v[0] | ((unsigned)v[1] << 16); p0.y = (unsigned)v[2] | ((unsigned)v[3] << 16);
        p0.z = (unsigned)v[4] | ((unsigned)v[5] << 16); p0.w = (unsigned)v[6] | ((unsigned)v[7] << 16);
        p1.x = v[8]; p1.y = 0; p1.z = 0; p1.w = 0;
        const uint4 z = {0, 0, 0, 0};
        dst[0] = p0; dst[1] = p1;
#pragma unroll
        for (int i = 2; i < 8; ++i) dst[i] = z;
    }
}
extern "C" int sed_conv0_im2col(const float* mel, void* col, int B, int T, int f16, hipStream_t stream) {
    (void)hipGetLastError();
    if (B <= 0 || T <= 0) return SED_ERR_ARG;
    hipLaunchKernelGGL(conv0_im2col_kernel, dim3(grid_for((size_t)B * T * 128)), dim3(256), 0, stream, mel, (bf16_t*)col, B, T, f16);
    return sed_check_launch();
}
// layer 0 with 16 filters, direct (round 4): Y[m, c] = bias[c] + sum_tap Wc[c, tap] patch(m, tap) on the fp32 spectrogram -- 144 FMAs per
// pixel instead of a [pixels, 64] 16-bit patch matrix (393 MB at batch 24) and a [pixels x 64] . [64 -> 128] GEMM over it.  Pixel m =
// (b, t, f), tap = 3 (dt + 1) + (df + 1) as above; Wc = conv0.weight [16, 1, 3, 3] as it lies.
__global__ __launch_bounds__(256) void conv0_fwd16_kernel(const float* __restrict__ mel, const float* __restrict__ Wc,
                                                          const float* __restrict__ bias, float* __restrict__ Y, int B, int T,
                                                          float* __restrict__ s1, float* __restrict__ s2) {
    __shared__ float wl[9][16], bl[16];
    __shared__ float sred[4][32];
    if (threadIdx.x < 144) wl[threadIdx.x % 9][threadIdx.x / 9] = Wc[threadIdx.x];
    if (threadIdx.x < 16) bl[threadIdx.x] = bias[threadIdx.x];
    __syncthreads();
    float t1[16], t2[16];      // (s1 != nullptr: the BatchNorm batch statistics sums, sed_colstats mode 0, from the values in registers)
#pragma unroll
    for (int c = 0; c < 16; ++c) { t1[c] = 0.f; t2[c] = 0.f; }
    const size_t total = (size_t)B * T * 128;
    for (size_t m = (size_t)blockIdx.x * blockDim.x + threadIdx.x; m < total; m += (size_t)gridDim.x * blockDim.x) {
        const int f = (int)(m % 128);
        const int t = (int)((m / 128) % T);
        const size_t b = m / ((size_t)128 * T);
        float acc[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) acc[c] = bl[c];
#pragma unroll
        for (int dt = -1; dt <= 1; ++dt)
#pragma unroll
            for (int df = -1; df <= 1; ++df) {
                const int tt = t + dt, ff = f + df;
                float x = 0.f;
                if (tt >= 0 && tt < T && ff >= 0 && ff < 128) x = mel[(b * 128 + ff) * T + tt];
                const int tap = 3 * (dt + 1) + (df + 1);
#pragma unroll
                for (int c = 0; c < 16; ++c) acc[c] = fmaf(wl[tap][c], x, acc[c]);
            }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *reinterpret_cast<float4*>(Y + m * 16 + 4 * q) = make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
        if (s1 != nullptr) {
#pragma unroll
            for (int c = 0; c < 16; ++c) { t1[c] += acc[c]; t2[c] = fmaf(acc[c], acc[c], t2[c]); }
        }
    }
    if (s1 != nullptr) {
#pragma unroll
        for (int c = 0; c < 16; ++c) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { t1[c] += __shfl_xor(t1[c], o, 64); t2[c] += __shfl_xor(t2[c], o, 64); }
        }
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int c = 0; c < 16; ++c) { sred[threadIdx.x >> 6][c] = t1[c]; sred[threadIdx.x >> 6][16 + c] = t2[c]; }
        }
        __syncthreads();
        if (threadIdx.x < 32) {
            const float v = (sred[0][threadIdx.x] + sred[1][threadIdx.x]) + (sred[2][threadIdx.x] + sred[3][threadIdx.x]);
            unsafeAtomicAdd((threadIdx.x < 16 ? s1 : s2) + (threadIdx.x & 15), v);
        }
    }
}
extern "C" int sed_conv0_fwd16(const float* mel, const float* Wc, const float* bias, float* Y, int B, int T, float* s1, float* s2,
                               hipStream_t stream) {
    (void)hipGetLastError();
    if (B <= 0 || T <= 0 || (s1 == nullptr) != (s2 == nullptr)) return SED_ERR_ARG;
    hipLaunchKernelGGL(conv0_fwd16_kernel, dim3(grid_for((size_t)B * T * 128, 256, 4096)), dim3(256), 0, stream, mel, Wc, bias, Y, B, T, s1, s2);
    return sed_check_launch();
}
// ... and its weight / bias gradient: dW[c, tap] += sum_m dY[m, c] patch(m, tap), dbias[c] += sum_m dY[m, c], as the streaming reduction of
// sed_small_dw with the patches gathered from the spectrogram (lane = (pixel slot, 4 taps): four lanes per pixel, 16 pixels per wave trip).
__global__ __launch_bounds__(256) void conv0_dw16_kernel(const bf16_t* __restrict__ dY, int ldy, const float* __restrict__ mel,
                                                         float* __restrict__ dW, int ldw, float* __restrict__ dbias, int B, int T,
                                                         int rows_per_wg) {
    __shared__ float red[4][16][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cg = lane & 3, rs = lane >> 2;
    const long long M = (long long)B * T * 128;
    const long long m_begin = (long long)blockIdx.x * rows_per_wg, m_end = (m_begin + rows_per_wg) < M ? (m_begin + rows_per_wg) : M;
    float acc[16][4], bacc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        bacc[i] = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][e] = 0.f;
    }
    for (long long m0 = m_begin + (long long)wave * 32; m0 < m_end; m0 += 128) {      // two pixels per lane and trip
        float xv[2][4];
        uint4 dr[2][2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const long long m = m0 + 16 * u + rs;
            const bool ok = m < m_end;
            const int f = (int)(m % 128), t = (int)((m / 128) % T);
            const long long b = m / ((long long)128 * T);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int tap = 4 * cg + e, tt = t + tap / 3 - 1, ff = f + tap % 3 - 1;
                xv[u][e] = (ok && tap < 9 && tt >= 0 && tt < T && ff >= 0 && ff < 128) ? mel[(b * 128 + ff) * T + tt] : 0.f;
            }
            dr[u][0] = ok ? reinterpret_cast<const uint4*>(dY + m * ldy)[0] : make_uint4(0u, 0u, 0u, 0u);
            dr[u][1] = ok ? reinterpret_cast<const uint4*>(dY + m * ldy)[1] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const unsigned w[4] = {dr[u][q].x, dr[u][q].y, dr[u][q].z, dr[u][q].w};
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const float d0 = __uint_as_float(w[p] << 16), d1 = __uint_as_float(w[p] & 0xffff0000u);
                    const int i = 8 * q + 2 * p;
                    bacc[i] += d0; bacc[i + 1] += d1;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        acc[i][e] = fmaf(d0, xv[u][e], acc[i][e]);
                        acc[i + 1][e] = fmaf(d1, xv[u][e], acc[i + 1][e]);
                    }
                }
            }
    }
    for (int off = 4; off < 64; off <<= 1) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            bacc[i] += __shfl_xor(bacc[i], off, 64);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[i][e] += __shfl_xor(acc[i][e], off, 64);
        }
    }
    if (rs == 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) red[wave][i][4 * cg + e] = acc[i][e];
    }
    __syncthreads();
    {
        const int i = threadIdx.x >> 4, j = threadIdx.x & 15;
        if (j < 9) unsafeAtomicAdd(dW + (size_t)i * ldw + j, (red[0][i][j] + red[1][i][j]) + (red[2][i][j] + red[3][i][j]));
    }
    if (dbias != nullptr) {
        __syncthreads();
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 16; ++i) red[wave][0][i] = bacc[i];
        }
        __syncthreads();
        if (threadIdx.x < 16) unsafeAtomicAdd(dbias + threadIdx.x, (red[0][0][threadIdx.x] + red[1][0][threadIdx.x]) + (red[2][0][threadIdx.x] + red[3][0][threadIdx.x]));
    }
}
extern "C" int sed_conv0_dw16(const void* dY, int ldy, const float* mel, float* dW, int ldw, float* dbias, int B, int T, hipStream_t stream) {
    (void)hipGetLastError();
    if (B <= 0 || T <= 0 || (ldy % 8) || ldy < 16 || ldw < 9) return SED_ERR_ARG;
    const long long M = (long long)B * T * 128;
    long long rows = (M + 1023) / 1024;
    rows = (rows + 127) / 128 * 128;
    const int slabs = (int)((M + rows - 1) / rows);
    hipLaunchKernelGGL(conv0_dw16_kernel, dim3(slabs), dim3(256), 0, stream, (const bf16_t*)dY, ldy, mel, dW, ldw, dbias, B, T, (int)rows);
    return sed_check_launch();
}
// generic layer: X [B, H, W, Cp] -> col [B*H*W, Kp], column tap * C + c (tap as above, c < C), zeros up to Kp; 16-byte chunks
__global__ void conv3x3_im2col_kernel(const bf16_t* __restrict__ X, bf16_t* __restrict__ col, int B, int H, int W, int C, int Cp,
                                      int Kp) {
    const int chunks = Kp / 8;
    const size_t total = (size_t)B * H * W * chunks;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(idx % chunks);
        const size_t m = idx / chunks;
        const int k0 = j * 8;
        uint4 v = {0, 0, 0, 0};
        if (k0 < 9 * C) {
            const int tap = k0 / C, c = k0 - tap * C;
            const int w = (int)(m % W), h = (int)((m / W) % H);
            const int hh = h + tap / 3 - 1, ww = w + tap % 3 - 1;
            if (hh >= 0 && hh < H && ww >= 0 && ww < W) {
                const size_t b = m / ((size_t)W * H);
                v = *reinterpret_cast<const uint4*>(X + ((b * H + hh) * W + ww) * Cp + c);
            }
        }
        reinterpret_cast<uint4*>(col)[idx] = v;
    }
}
extern "C" int sed_conv3x3_im2col(const void* X, void* col, int B, int H, int W, int C, int Cp, int Kp, hipStream_t stream) {
    (void)hipGetLastError();
    if (B <= 0 || H <= 0 || W <= 0 || (C % 8) || (Cp % 8) || (Kp % 8) || Kp < 9 * C || Cp < C) return SED_ERR_ARG;
    hipLaunchKernelGGL(conv3x3_im2col_kernel, dim3(grid_for((size_t)B * H * W * (Kp / 8), 256, 16384)), dim3(256), 0, stream,
                       (const bf16_t*)X, (bf16_t*)col, B, H, W, C, Cp, Kp);
    return sed_check_launch();
}
// col2im: dX[b, h, w, c] = sum over the 9 taps of dcol[(b, h - dh, w - dw), tap * C + c]  (gather form of the im2col transpose)
__global__ void col2im3x3_kernel(const bf16_t* __restrict__ dcol, int Kp, float* __restrict__ dX, int B, int H, int W, int C) {
    const int c4n = C / 4;
    const size_t total = (size_t)B * H * W * c4n;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx % c4n) * 4;
        const size_t m = idx / c4n;
        const int w = (int)(m % W), h = (int)((m / W) % H);
        const size_t b = m / ((size_t)W * H);
        float4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int hh = h - (tap / 3 - 1), ww = w - (tap % 3 - 1);   // the output pixel whose tap `tap` reads (h, w)
            if (hh < 0 || hh >= H || ww < 0 || ww >= W) continue;
            const uint2 v = *reinterpret_cast<const uint2*>(dcol + ((b * H + hh) * W + ww) * Kp + tap * C + c);
            acc.x += bf2f((bf16_t)(v.x & 0xffff)); acc.y += bf2f((bf16_t)(v.x >> 16));
            acc.z += bf2f((bf16_t)(v.y & 0xffff)); acc.w += bf2f((bf16_t)(v.y >> 16));
        }
        *reinterpret_cast<float4*>(dX + m * C + c) = acc;
    }
}
extern "C" int sed_col2im3x3(const void* dcol, int Kp, float* dX, int B, int H, int W, int C, hipStream_t stream) {
    (void)hipGetLastError();
    if (B <= 0 || (C % 4) || Kp < 9 * C) return SED_ERR_ARG;
    hipLaunchKernelGGL(col2im3x3_kernel, dim3(grid_for((size_t)B * H * W * (C / 4), 256, 16384)), dim3(256), 0, stream, (const bf16_t*)dcol,
                       Kp, dX, B, H, W, C);
    return sed_check_launch();
}

// ---------------------------------------------------------------------------------------------------
// Column statistics over the rows of fp32 matrices: s1[c] += sum_m A[m, c] (* B[m, c] when B != NULL ... ) -- the BatchNorm
// batch statistics and its backward sums.  mode 0: s1 = sum A, s2 = sum A^2.  mode 1: s1 = sum A, s2 = sum A * (B * a + b)
// (A = dZ, B = Y: the BatchNorm backward sums with xhat folded into the affine a, b).
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void colstats_kernel(const float* __restrict__ A, int lda, const float* __restrict__ Bm, int ldb,
                                                       const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ s1,
                                                       float* __restrict__ s2, size_t M, int C, int mode) {
    // a block covers Cw = min(C, 64) columns (grid.x column groups) and 256 / Cw rows per iteration (grid.y row slabs), so that
    // narrow matrices (16 / 32 channels) still use every lane; partials are combined through LDS before the atomics
    const int Cw = C < 64 ? C : 64, rpi = 256 / Cw;
    const int cl = threadIdx.x % Cw, rsub = threadIdx.x / Cw;
    const int c = blockIdx.x * 64 + cl;
    __shared__ float r1[256], r2[256];
    float t1 = 0.f, t2 = 0.f;
    if (c < C && rsub < rpi) {
        const float aa = mode ? a[c] : 0.f, bb = mode ? b[c] : 0.f;
        for (size_t m = (size_t)blockIdx.y * rpi + rsub; m < M; m += (size_t)gridDim.y * rpi) {
            const float v = A[m * lda + c];
            t1 += v;
            t2 += mode ? v * fmaf(Bm[m * ldb + c], aa, bb) : v * v;
        }
    }
    r1[threadIdx.x] = t1; r2[threadIdx.x] = t2;
    __syncthreads();
    if (rsub == 0 && c < C) {
        float u1 = 0.f, u2 = 0.f;
        for (int j = 0; j < rpi; ++j) { u1 += r1[j * Cw + cl]; u2 += r2[j * Cw + cl]; }
        unsafeAtomicAdd(&s1[c], u1);
        unsafeAtomicAdd(&s2[c], u2);
    }
}
extern "C" int sed_colstats(const float* A, int lda, const float* Bm, int ldb, const float* a, const float* b, float* s1,
                            float* s2, int64_t M, int C, int mode, hipStream_t stream) {
    (void)hipGetLastError();
    if (M <= 0 || C <= 0 || (C < 64 && (256 % C)) || (mode && (Bm == nullptr || a == nullptr || b == nullptr))) return SED_ERR_ARG;
    const int rpi = 256 / (C < 64 ? C : 64);
    int slabs = (int)((M + (size_t)rpi * 16 - 1) / ((size_t)rpi * 16));
    if (slabs > 2048) slabs = 2048;
    if (slabs < 1) slabs = 1;
    hipLaunchKernelGGL(colstats_kernel, dim3(cdiv(C, 64), slabs), dim3(256), 0, stream, A, lda, Bm, ldb, a, b, s1, s2, (size_t)M, C, mode);
    return sed_check_launch();
}

// ---------------------------------------------------------------------------------------------------
// BatchNorm2d statistics -> the per-channel affines the CNN kernels use (src/models/cnn/base.py:72-75; torch BatchNorm semantics).
//   train (s1 / s2 = column sums of Y and Y^2 over the M rows, sed_colstats mode 0):  mean = s1 / M, var = max(s2 / M - mean^2, 0);
//         running_mean = (1 - mom) running_mean + mom mean,  running_var = (1 - mom) running_var + mom var M / (M - 1)
//   eval  (s1 == nullptr): mean / var = the running statistics, left untouched
//   a = gamma rstd, b = beta - mean a   (Z = Y a + b);   ah = rstd, bh = -mean rstd   (xhat = Y ah + bh, backward)
// replaces eleven single-purpose torch launches per layer.
// ---------------------------------------------------------------------------------------------------
__global__ void bn_finalize_kernel(const float* __restrict__ s1, const float* __restrict__ s2, const float* __restrict__ gamma,
                                   const float* __restrict__ beta, float* __restrict__ run_mean, float* __restrict__ run_var, float inv_m,
                                   float unbias, float mom, float keep, float eps, float* __restrict__ a, float* __restrict__ b, float* __restrict__ ah,
                                   float* __restrict__ bh, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float mean, var;
    if (s1 != nullptr) {
        mean = s1[c] * inv_m;
        var = fmaxf(s2[c] * inv_m - mean * mean, 0.f);
        run_mean[c] = run_mean[c] * keep + mom * mean;
        run_var[c] = run_var[c] * keep + mom * (var * unbias);
    } else {
        mean = run_mean[c];
        var = run_var[c];
    }
    const float rstd = 1.0f / sqrtf(var + eps);
    const float av = gamma[c] * rstd;
    a[c] = av;
    b[c] = beta[c] - mean * av;
    ah[c] = rstd;
    bh[c] = -mean * rstd;
}
extern "C" int sed_bn_finalize(const float* s1, const float* s2, const float* gamma, const float* beta, float* run_mean, float* run_var,
                               int64_t M, int C, double momentum, double eps, float* a, float* b, float* ah, float* bh, hipStream_t stream) {
    (void)hipGetLastError();
    if (C <= 0 || M <= 1 || (s1 == nullptr) != (s2 == nullptr)) return SED_ERR_ARG;
    hipLaunchKernelGGL(bn_finalize_kernel, dim3(cdiv(C, 128)), dim3(128), 0, stream, s1, s2, gamma, beta, run_mean, run_var,
                       (float)(1.0 / (double)M), (float)((double)M / (double)(M - 1)), (float)momentum, (float)(1.0 - momentum), (float)eps, a, b,
                       ah, bh, C);
    return sed_check_launch();
}
// BatchNorm as a per-channel affine (eval: running statistics; train: the batch statistics folded by the host into a, b):
// Z16[m, c] = Y[m, c] * a[c] + b[c] for c < C, zero for C <= c < Cp.  Operand of the ContextGating GEMM.
__global__ void bn_act_kernel(const float* __restrict__ Y, int ldy, const float* __restrict__ a, const float* __restrict__ b,
                              bf16_t* __restrict__ Z, size_t M, int C, int Cp, int f16) {
    const int c4n = Cp / 4;
    const size_t total = M * c4n;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx % c4n) * 4;
        const size_t m = idx / c4n;
        uint2 p = {0, 0};
        if (c < C) {
            const float4 y = *reinterpret_cast<const float4*>(Y + m * ldy + c);
            const float4 aa = *reinterpret_cast<const float4*>(a + c), bb = *reinterpret_cast<const float4*>(b + c);
            p.x = (unsigned)cvt16(fmaf(y.x, aa.x, bb.x), f16) | ((unsigned)cvt16(fmaf(y.y, aa.y, bb.y), f16) << 16);
            p.y = (unsigned)cvt16(fmaf(y.z, aa.z, bb.z), f16) | ((unsigned)cvt16(fmaf(y.w, aa.w, bb.w), f16) << 16);
        }
        *reinterpret_cast<uint2*>(Z + m * Cp + c) = p;
    }
}
extern "C" int sed_bn_act(const float* Y, int ldy, const float* a, const float* b, void* Z, int64_t M, int C, int Cp, int f16,
                          hipStream_t stream) {
    (void)hipGetLastError();
    if (M <= 0 || (C % 4) || (Cp % 4) || Cp < C || (ldy % 4)) return SED_ERR_ARG;
    hipLaunchKernelGGL(bn_act_kernel, dim3(grid_for((size_t)M * (Cp / 4), 256, 16384)), dim3(256), 0, stream, Y, ldy, a, b, (bf16_t*)Z,
                       (size_t)M, C, Cp, f16);
    return sed_check_launch();
}
// BatchNorm backward (batch statistics), given the column sums s1 = sum dz, s2 = sum dz * xhat (xhat = Y * ah + bh with
// ah = rstd, bh = -mean * rstd):  dY = gamma * rstd * (dz - s1 / M - xhat * s2 / M) -> bf16 [M, ldo] (columns C.. zero).
__global__ void bn_bwd_kernel(const float* __restrict__ dz, int ldz, const float* __restrict__ Y, int ldy, const float* __restrict__ ah,
                              const float* __restrict__ bh, const float* __restrict__ gamma, const float* __restrict__ s1,
                              const float* __restrict__ s2, bf16_t* __restrict__ dY, int ldo, size_t M, int C) {
    const int c4n = ldo / 4;
    const size_t total = M * c4n;
    const float invM = 1.0f / (float)M;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx % c4n) * 4;
        const size_t m = idx / c4n;
        uint2 p = {0, 0};
        if (c < C) {
            float o[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float xh = fmaf(Y[m * ldy + c + u], ah[c + u], bh[c + u]);
                o[u] = gamma[c + u] * ah[c + u] * (dz[m * ldz + c + u] - s1[c + u] * invM - xh * s2[c + u] * invM);
            }
            p.x = pack2bf(o[0], o[1]);
            p.y = pack2bf(o[2], o[3]);
        }
        *reinterpret_cast<uint2*>(dY + m * ldo + c) = p;
    }
}
extern "C" int sed_bn_bwd(const float* dz, int ldz, const float* Y, int ldy, const float* ah, const float* bh, const float* gamma,
                          const float* s1, const float* s2, void* dY, int ldo, int64_t M, int C, hipStream_t stream) {
    (void)hipGetLastError();
    if (M <= 0 || (C % 4) || (ldo % 4) || ldo < C) return SED_ERR_ARG;
    hipLaunchKernelGGL(bn_bwd_kernel, dim3(grid_for((size_t)M * (ldo / 4), 256, 16384)), dim3(256), 0, stream, dz, ldz, Y, ldy, ah, bh, gamma,
                       s1, s2, (bf16_t*)dY, ldo, (size_t)M, C);
    return sed_check_launch();
}
// ContextGating + dropout + average pooling:  out[b, ho, wo, c] = mean over the (ph x pw) window of z * sigmoid(l) * keep,
// z = Y * a + b (BatchNorm output, fp32), l = L (gate logits), keep = mask * drop_scale (mask NULL: 1).  16-bit NHWC output with
// channel pad Cpo (zeros) and/or fp32 [rows, C].
__global__ void cg_pool_kernel(const float* __restrict__ Y, int ldy, const float* __restrict__ a, const float* __restrict__ b,
                               const float* __restrict__ L, int ldl, const unsigned char* __restrict__ mask, float drop_scale,
                               bf16_t* __restrict__ out16, float* __restrict__ out32, int B, int H, int W, int C, int Cpo, int ph,
                               int pw, int f16) {
    const int Ho = H / ph, Wo = W / pw, c4n = Cpo / 4;
    const size_t total = (size_t)B * Ho * Wo * c4n;
    const float inv = 1.0f / (float)(ph * pw);
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx % c4n) * 4;
        const size_t mo = idx / c4n;
        float4 acc = {0.f, 0.f, 0.f, 0.f};
        if (c < C) {
            const int wo = (int)(mo % Wo), ho = (int)((mo / Wo) % Ho);
            const size_t bi = mo / ((size_t)Wo * Ho);
            const float4 aa = *reinterpret_cast<const float4*>(a + c), bb = *reinterpret_cast<const float4*>(b + c);
            for (int i = 0; i < ph; ++i)
                for (int j = 0; j < pw; ++j) {
                    const size_t m = (bi * H + (size_t)ho * ph + i) * W + (size_t)wo * pw + j;
                    const float4 y = *reinterpret_cast<const float4*>(Y + m * ldy + c);
                    const float4 l = *reinterpret_cast<const float4*>(L + m * ldl + c);
                    float4 k = {1.f, 1.f, 1.f, 1.f};
                    if (mask != nullptr) {
                        const uchar4 mk = *reinterpret_cast<const uchar4*>(mask + m * C + c);
                        k.x = mk.x ? drop_scale : 0.f; k.y = mk.y ? drop_scale : 0.f; k.z = mk.z ? drop_scale : 0.f; k.w = mk.w ? drop_scale : 0.f;
                    }
                    acc.x += fmaf(y.x, aa.x, bb.x) * sigmoidf_(l.x) * k.x;
                    acc.y += fmaf(y.y, aa.y, bb.y) * sigmoidf_(l.y) * k.y;
                    acc.z += fmaf(y.z, aa.z, bb.z) * sigmoidf_(l.z) * k.z;
                    acc.w += fmaf(y.w, aa.w, bb.w) * sigmoidf_(l.w) * k.w;
                }
            acc.x *= inv; acc.y *= inv; acc.z *= inv; acc.w *= inv;
            if (out32 != nullptr) *reinterpret_cast<float4*>(out32 + mo * C + c) = acc;
        }
        if (out16 != nullptr) {
            uint2 p;
            p.x = (unsigned)cvt16(acc.x, f16) | ((unsigned)cvt16(acc.y, f16) << 16);
            p.y = (unsigned)cvt16(acc.z, f16) | ((unsigned)cvt16(acc.w, f16) << 16);
            *reinterpret_cast<uint2*>(out16 + mo * Cpo + c) = p;
        }
    }
}
extern "C" int sed_cg_pool(const float* Y, int ldy, const float* a, const float* b, const float* L, int ldl,
                           const uint8_t* mask, float drop_scale, void* out16, float* out32, int B, int H, int W, int C,
                           int Cpo, int ph, int pw, int f16, hipStream_t stream) {
    (void)hipGetLastError();
    if (B <= 0 || ph <= 0 || pw <= 0 || (H % ph) || (W % pw) || (C % 4) || (Cpo % 4) || Cpo < C || (ldy % 4) || (ldl % 4))
        return SED_ERR_ARG;
    hipLaunchKernelGGL(cg_pool_kernel, dim3(grid_for((size_t)B * (H / ph) * (W / pw) * (Cpo / 4), 256, 16384)), dim3(256), 0, stream, Y,
                       ldy, a, b, L, ldl, mask, drop_scale, (bf16_t*)out16, out32, B, H, W, C, Cpo, ph, pw, f16);
    return sed_check_launch();
}

// backward of sed_cg_pool: dout (fp32 [B, Ho, Wo, C]) -> dzd [M, C] fp32 = up * sigmoid(l)  (direct path of z) and
// dL16 [M, ldl16] bf16 = up * z * s * (1 - s)  (gate logits; columns C..ldl16-1 zero), up = dout / (ph pw) * keep.
__global__ void cg_pool_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ Y, int ldy, const float* __restrict__ a,
                                   const float* __restrict__ b, const float* __restrict__ L, int ldl,
                                   const unsigned char* __restrict__ mask, float drop_scale, float* __restrict__ dzd, int ldz,
                                   bf16_t* __restrict__ dL16, int ldl16, int B, int H, int W, int C, int ph, int pw) {
    const int Ho = H / ph, Wo = W / pw, c4n = ldl16 / 4;
    const size_t total = (size_t)B * H * W * c4n;
    const float inv = 1.0f / (float)(ph * pw);
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx % c4n) * 4;
        const size_t m = idx / c4n;
        uint2 p = {0, 0};
        if (c < C) {
            const int w = (int)(m % W), h = (int)((m / W) % H);
            const size_t bi = m / ((size_t)W * H);
            const size_t mo = (bi * Ho + h / ph) * Wo + w / pw;
            const float4 g = *reinterpret_cast<const float4*>(dout + mo * C + c);
            const float4 y = *reinterpret_cast<const float4*>(Y + m * ldy + c), l = *reinterpret_cast<const float4*>(L + m * ldl + c);
            const float4 aa = *reinterpret_cast<const float4*>(a + c), bb = *reinterpret_cast<const float4*>(b + c);
            float4 k = {inv, inv, inv, inv};
            if (mask != nullptr) {
                const uchar4 mk = *reinterpret_cast<const uchar4*>(mask + m * C + c);
                k.x = mk.x ? inv * drop_scale : 0.f; k.y = mk.y ? inv * drop_scale : 0.f;
                k.z = mk.z ? inv * drop_scale : 0.f; k.w = mk.w ? inv * drop_scale : 0.f;
            }
            const float sx = sigmoidf_(l.x), sy = sigmoidf_(l.y), sz = sigmoidf_(l.z), sw = sigmoidf_(l.w);
            const float ux = g.x * k.x, uy = g.y * k.y, uz = g.z * k.z, uw = g.w * k.w;
            *reinterpret_cast<float4*>(dzd + m * ldz + c) = make_float4(ux * sx, uy * sy, uz * sz, uw * sw);
            p.x = pack2bf(ux * fmaf(y.x, aa.x, bb.x) * sx * (1.f - sx), uy * fmaf(y.y, aa.y, bb.y) * sy * (1.f - sy));
            p.y = pack2bf(uz * fmaf(y.z, aa.z, bb.z) * sz * (1.f - sz), uw * fmaf(y.w, aa.w, bb.w) * sw * (1.f - sw));
        }
        else if (c < ldz) *reinterpret_cast<float4*>(dzd + m * ldz + c) = make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<uint2*>(dL16 + m * ldl16 + c) = p;
    }
}
extern "C" int sed_cg_pool_bwd(const float* dout, const float* Y, int ldy, const float* a, const float* b, const float* L, int ldl,
                               const uint8_t* mask, float drop_scale, float* dzd, int ldz, void* dL16, int ldl16, int B, int H,
                               int W, int C, int ph, int pw, hipStream_t stream) {
    (void)hipGetLastError();
    if (B <= 0 || ph <= 0 || pw <= 0 || (H % ph) || (W % pw) || (C % 4) || (ldl16 % 4) || ldl16 < C || (ldy % 4) || (ldl % 4) || (ldz % 4) || ldz < C || ldz > ldl16)
        return SED_ERR_ARG;
    hipLaunchKernelGGL(cg_pool_bwd_kernel, dim3(grid_for((size_t)B * H * W * (ldl16 / 4), 256, 16384)), dim3(256), 0, stream, dout, Y, ldy, a,
                       b, L, ldl, mask, drop_scale, dzd, ldz, (bf16_t*)dL16, ldl16, B, H, W, C, ph, pw);
    return sed_check_launch();
}
// The same for a 16-filter layer with the gate Linear inside (round 4): l = W_g z + b_g by 256 FMAs per pixel on the fp32 BatchNorm output --
// no 64-column 16-bit image of z, no [pixels x 64] . [64 -> 128] gate GEMM, no fp32 logits round trip.  One thread per OUTPUT pixel, the 16 x 16
// weight from LDS (every lane reads the same words: broadcasts).  Optional side outputs for the backward: the logits L [pixels, 16] fp32 and
// the 16-bit image Z [pixels, 16] of z (operand of the gate's weight gradient).
__global__ __launch_bounds__(256) void cg_gate16_pool_kernel(const float* __restrict__ Y, int ldy, const float* __restrict__ a,
                                                             const float* __restrict__ b, const float* __restrict__ Wg,
                                                             const float* __restrict__ bg, const unsigned char* __restrict__ mask,
                                                             float drop_scale, float* __restrict__ Lout, bf16_t* __restrict__ Zout,
                                                             bf16_t* __restrict__ out16, float* __restrict__ out32, int B, int H, int W,
                                                             int Cpo, int ph, int pw, int f16) {
    __shared__ __attribute__((aligned(16))) float wg[16][16];
    __shared__ float ab[3][16];
    wg[threadIdx.x >> 4][threadIdx.x & 15] = Wg[threadIdx.x];
    if (threadIdx.x < 16) { ab[0][threadIdx.x] = a[threadIdx.x]; ab[1][threadIdx.x] = b[threadIdx.x]; ab[2][threadIdx.x] = bg[threadIdx.x]; }
    __syncthreads();
    const int Ho = H / ph, Wo = W / pw;
    const size_t total = (size_t)B * Ho * Wo;
    const float inv = 1.0f / (float)(ph * pw);
    for (size_t mo = (size_t)blockIdx.x * blockDim.x + threadIdx.x; mo < total; mo += (size_t)gridDim.x * blockDim.x) {
        const int wo = (int)(mo % Wo), ho = (int)((mo / Wo) % Ho);
        const size_t bi = mo / ((size_t)Wo * Ho);
        float acc[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) acc[c] = 0.f;
        for (int i = 0; i < ph; ++i)
            for (int j = 0; j < pw; ++j) {
                const size_t m = (bi * H + (size_t)ho * ph + i) * W + (size_t)wo * pw + j;
                float z[16], l[16];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 y = *reinterpret_cast<const float4*>(Y + m * ldy + 4 * q);
                    z[4 * q] = fmaf(y.x, ab[0][4 * q], ab[1][4 * q]); z[4 * q + 1] = fmaf(y.y, ab[0][4 * q + 1], ab[1][4 * q + 1]);
                    z[4 * q + 2] = fmaf(y.z, ab[0][4 * q + 2], ab[1][4 * q + 2]); z[4 * q + 3] = fmaf(y.w, ab[0][4 * q + 3], ab[1][4 * q + 3]);
                }
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    float s = ab[2][c];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 w = *reinterpret_cast<const float4*>(&wg[c][4 * q]);
                        s = fmaf(w.x, z[4 * q], s); s = fmaf(w.y, z[4 * q + 1], s); s = fmaf(w.z, z[4 * q + 2], s); s = fmaf(w.w, z[4 * q + 3], s);
                    }
                    l[c] = s;
                }
                if (Lout != nullptr) {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        *reinterpret_cast<float4*>(Lout + m * 16 + 4 * q) = make_float4(l[4 * q], l[4 * q + 1], l[4 * q + 2], l[4 * q + 3]);
                }
                if (Zout != nullptr) {
                    unsigned pk[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) pk[e] = (unsigned)cvt16(z[2 * e], f16) | ((unsigned)cvt16(z[2 * e + 1], f16) << 16);
                    uint4* zd = reinterpret_cast<uint4*>(Zout + m * 16);
                    zd[0] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
                    zd[1] = make_uint4(pk[4], pk[5], pk[6], pk[7]);
                }
                uint4 mk4 = make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u);
                if (mask != nullptr) mk4 = *reinterpret_cast<const uint4*>(mask + m * 16);
                const unsigned mw[4] = {mk4.x, mk4.y, mk4.z, mk4.w};
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const float keep = ((mw[c >> 2] >> (8 * (c & 3))) & 0xffu) ? (mask != nullptr ? drop_scale : 1.0f) : 0.f;
                    acc[c] += z[c] * sigmoidf_(l[c]) * keep;
                }
            }
        if (out32 != nullptr) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                *reinterpret_cast<float4*>(out32 + mo * 16 + 4 * q) = make_float4(acc[4 * q] * inv, acc[4 * q + 1] * inv, acc[4 * q + 2] * inv, acc[4 * q + 3] * inv);
        }
        if (out16 != nullptr) {
            unsigned pk[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) pk[e] = (unsigned)cvt16(acc[2 * e] * inv, f16) | ((unsigned)cvt16(acc[2 * e + 1] * inv, f16) << 16);
            uint4* od = reinterpret_cast<uint4*>(out16 + mo * Cpo);
            od[0] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
            od[1] = make_uint4(pk[4], pk[5], pk[6], pk[7]);
            for (int c8 = 2; c8 < Cpo / 8; ++c8) od[c8] = make_uint4(0u, 0u, 0u, 0u);       // channel padding of the NHWC operand
        }
    }
}
extern "C" int sed_cg_gate16_pool(const float* Y, int ldy, const float* a, const float* b, const float* Wg, const float* bg,
                                  const uint8_t* mask, float drop_scale, float* Lout, void* Zout, void* out16, float* out32, int B, int H,
                                  int W, int Cpo, int ph, int pw, int f16, hipStream_t stream) {
    (void)hipGetLastError();
    if (B <= 0 || ph <= 0 || pw <= 0 || (H % ph) || (W % pw) || (Cpo % 8) || Cpo < 16 || (ldy % 4) || ldy < 16) return SED_ERR_ARG;
    hipLaunchKernelGGL(cg_gate16_pool_kernel, dim3(grid_for((size_t)B * (H / ph) * (W / pw), 256, 16384)), dim3(256), 0, stream, Y, ldy, a, b,
                       Wg, bg, mask, drop_scale, Lout, (bf16_t*)Zout, (bf16_t*)out16, out32, B, H, W, Cpo, ph, pw, f16);
    return sed_check_launch();
}

// backward of sed_cg_gate16_pool (16 filters): as sed_cg_pool_bwd, with the gate Linear's input gradient added in the same pass --
// dz[m, c] = up * sigmoid(l) + sum_i dl[m, i] Wg[i, c] (fp32 dl; the NT GEMM dz += dL16 . Wg it replaces read a bf16 dl) -- and dL16 as a
// 16-column bf16 image (operand of the gate's weight gradient, sed_small_dw).  One thread per input pixel.
__global__ __launch_bounds__(256) void cg_gate16_pool_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ Y, int ldy,
                                                                 const float* __restrict__ a, const float* __restrict__ b,
                                                                 const float* __restrict__ L, const float* __restrict__ Wg,
                                                                 const unsigned char* __restrict__ mask, float drop_scale,
                                                                 float* __restrict__ dz, bf16_t* __restrict__ dL16, int B, int H, int W,
                                                                 int ph, int pw, const float* __restrict__ ah, const float* __restrict__ bh,
                                                                 float* __restrict__ s1, float* __restrict__ s2) {
    __shared__ __attribute__((aligned(16))) float wg[16][16];
    __shared__ float ab[4][16];
    __shared__ float sred[4][32];
    wg[threadIdx.x >> 4][threadIdx.x & 15] = Wg[threadIdx.x];
    if (threadIdx.x < 16) {
        ab[0][threadIdx.x] = a[threadIdx.x]; ab[1][threadIdx.x] = b[threadIdx.x];
        ab[2][threadIdx.x] = s1 != nullptr ? ah[threadIdx.x] : 0.f; ab[3][threadIdx.x] = s1 != nullptr ? bh[threadIdx.x] : 0.f;
    }
    __syncthreads();
    // (s1 != nullptr: also the BatchNorm backward sums of this layer, s1[c] += sum dz, s2[c] += sum dz * xhat with xhat = Y ah + bh --
    //  sed_colstats mode 1 -- from the values in registers)
    float t1[16], t2[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) { t1[c] = 0.f; t2[c] = 0.f; }
    const int Ho = H / ph, Wo = W / pw;
    const size_t total = (size_t)B * H * W;
    const float inv = 1.0f / (float)(ph * pw);
    for (size_t m = (size_t)blockIdx.x * blockDim.x + threadIdx.x; m < total; m += (size_t)gridDim.x * blockDim.x) {
        const int w = (int)(m % W), h = (int)((m / W) % H);
        const size_t bi = m / ((size_t)W * H);
        const size_t mo = (bi * Ho + h / ph) * Wo + w / pw;
        uint4 mk4 = make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u);
        if (mask != nullptr) mk4 = *reinterpret_cast<const uint4*>(mask + m * 16);
        const unsigned mw[4] = {mk4.x, mk4.y, mk4.z, mk4.w};
        const float kscale = mask != nullptr ? inv * drop_scale : inv;
        float dzv[16], dl[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 g = *reinterpret_cast<const float4*>(dout + mo * 16 + 4 * q);
            const float4 y = *reinterpret_cast<const float4*>(Y + m * ldy + 4 * q);
            const float4 l = *reinterpret_cast<const float4*>(L + m * 16 + 4 * q);
            const float gg[4] = {g.x, g.y, g.z, g.w}, yy[4] = {y.x, y.y, y.z, y.w}, ll[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = 4 * q + e;
                const float keep = ((mw[q] >> (8 * e)) & 0xffu) ? kscale : 0.f;
                const float sg = sigmoidf_(ll[e]), up = gg[e] * keep;
                dzv[c] = up * sg;
                dl[c] = up * fmaf(yy[e], ab[0][c], ab[1][c]) * sg * (1.f - sg);
            }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 wv = *reinterpret_cast<const float4*>(&wg[i][4 * q]);
                dzv[4 * q] = fmaf(dl[i], wv.x, dzv[4 * q]); dzv[4 * q + 1] = fmaf(dl[i], wv.y, dzv[4 * q + 1]);
                dzv[4 * q + 2] = fmaf(dl[i], wv.z, dzv[4 * q + 2]); dzv[4 * q + 3] = fmaf(dl[i], wv.w, dzv[4 * q + 3]);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *reinterpret_cast<float4*>(dz + m * 16 + 4 * q) = make_float4(dzv[4 * q], dzv[4 * q + 1], dzv[4 * q + 2], dzv[4 * q + 3]);
        if (s1 != nullptr) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 y = *reinterpret_cast<const float4*>(Y + m * ldy + 4 * q);      // (L1 hit: read above)
                const float yy[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int c = 4 * q + e;
                    t1[c] += dzv[c];
                    t2[c] = fmaf(dzv[c], fmaf(yy[e], ab[2][c], ab[3][c]), t2[c]);
                }
            }
        }
        unsigned pk[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) pk[e] = pack2bf(dl[2 * e], dl[2 * e + 1]);
        uint4* dd = reinterpret_cast<uint4*>(dL16 + m * 16);
        dd[0] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
        dd[1] = make_uint4(pk[4], pk[5], pk[6], pk[7]);
    }
    if (s1 != nullptr) {
#pragma unroll
        for (int c = 0; c < 16; ++c) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { t1[c] += __shfl_xor(t1[c], o, 64); t2[c] += __shfl_xor(t2[c], o, 64); }
        }
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int c = 0; c < 16; ++c) { sred[threadIdx.x >> 6][c] = t1[c]; sred[threadIdx.x >> 6][16 + c] = t2[c]; }
        }
        __syncthreads();
        if (threadIdx.x < 32) {
            const float v = (sred[0][threadIdx.x] + sred[1][threadIdx.x]) + (sred[2][threadIdx.x] + sred[3][threadIdx.x]);
            unsafeAtomicAdd((threadIdx.x < 16 ? s1 : s2) + (threadIdx.x & 15), v);
        }
    }
}
extern "C" int sed_cg_gate16_pool_bwd(const float* dout, const float* Y, int ldy, const float* a, const float* b, const float* L,
                                      const float* Wg, const uint8_t* mask, float drop_scale, float* dz, void* dL16, int B, int H, int W,
                                      int ph, int pw, const float* ah, const float* bh, float* s1, float* s2, hipStream_t stream) {
    (void)hipGetLastError();
    if (B <= 0 || ph <= 0 || pw <= 0 || (H % ph) || (W % pw) || (ldy % 4) || ldy < 16) return SED_ERR_ARG;
    if ((s1 == nullptr) != (s2 == nullptr) || (s1 != nullptr && (ah == nullptr || bh == nullptr))) return SED_ERR_ARG;
    hipLaunchKernelGGL(cg_gate16_pool_bwd_kernel, dim3(grid_for((size_t)B * H * W, 256, 4096)), dim3(256), 0, stream, dout, Y, ldy, a, b, L, Wg,
                       mask, drop_scale, dz, (bf16_t*)dL16, B, H, W, ph, pw, ah, bh, s1, s2);
    return sed_check_launch();
}

// ---------------------------------------------------------------------------------------------------
// Dropout keep-masks of the CNN branch (nn.Dropout(conv_dropout) after every ContextGating, src/models/cnn/base.py:88-89), all layers in one
// launch: mask[e] = 1 with probability 1 - p.  Counter-based generator (splitmix64 finaliser of seed + 4-element group index, 16 bits per
// element: p is resolved to 1 / 65536) -- torch's Philox stream cannot be reproduced from outside torch, and only the distribution is part
// of the model.  Replaces rand -> compare -> byte cast (three launches and 9 bytes of traffic per element, per layer).
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dropout_mask_kernel(unsigned char* __restrict__ mask, long long n4, unsigned thr, unsigned long long seed) {
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < n4; g += (long long)gridDim.x * 256) {
        unsigned long long z = seed + (unsigned long long)(g + 1) * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        const unsigned lo = (unsigned)z, hi = (unsigned)(z >> 32);
        const unsigned m = ((lo & 0xffffu) >= thr ? 1u : 0u) | ((lo >> 16) >= thr ? 0x100u : 0u) | ((hi & 0xffffu) >= thr ? 0x10000u : 0u) |
                           ((hi >> 16) >= thr ? 0x1000000u : 0u);
        reinterpret_cast<unsigned*>(mask)[g] = m;
    }
}
extern "C" int sed_dropout_mask(uint8_t* mask, int64_t n, float p, int64_t seed, hipStream_t stream) {
    (void)hipGetLastError();
    if (n <= 0 || (n % 4) || p < 0.f || p >= 1.f) return SED_ERR_ARG;
    const unsigned thr = (unsigned)(p * 65536.0f + 0.5f);
    hipLaunchKernelGGL(dropout_mask_kernel, dim3(grid_for((size_t)(n / 4))), dim3(256), 0, stream, mask, (long long)(n / 4), thr,
                       (unsigned long long)seed);
    return sed_check_launch();
}
