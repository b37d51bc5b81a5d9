// Memory-layout kernels around the GEMMs, for gfx950: casts, transposes, the operand images of the weights (straight, transposed,
// split-precision, two-term, e4m3, LayerNorm-folded), the per-clip column means and row statistics that feed the GEMM epilogues, and
// the small fp32 linear.  None of them shares code with the GEMM kernels: common.h only.
#include <algorithm>

#include "common.h"
#include "../../include/sed_hip.h"

// ---------------------------------------------------------------------------------------------------
// Layout helpers around the GEMM: casts, transposes (with zero padding of the reduction dim), column sums.
// ---------------------------------------------------------------------------------------------------
// in fp32 [R, C] -> out bf16 [R, C]  (grid-stride, float4 in / 8 B out)
template <bool F16>
__global__ void cast_f32_bf16_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, size_t n4) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n4; i += stride) {
        const float4 v = reinterpret_cast<const float4*>(in)[i];
        uint2 p;
        p.x = pack2<F16>(v.x, v.y);
        p.y = pack2<F16>(v.z, v.w);
        reinterpret_cast<uint2*>(out)[i] = p;
    }
}

extern "C" int sed_cast_f32_bf16(const float* in, void* out, int64_t n, int f16, hipStream_t stream) {
    (void)hipGetLastError();
    if (n % 4) return SED_ERR_ARG;
    const size_t n4 = n / 4;
    int blocks = (int)((n4 + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    if (f16) hipLaunchKernelGGL(cast_f32_bf16_kernel<true>, dim3(blocks), dim3(256), 0, stream, in, (bf16_t*)out, n4);
    else hipLaunchKernelGGL(cast_f32_bf16_kernel<false>, dim3(blocks), dim3(256), 0, stream, in, (bf16_t*)out, n4);
    return sed_check_launch();
}

// Transpose [R, C] (fp32 or bf16 in) -> bf16 out^T [C, Rpad] (rows R..Rpad-1 written as zeros), optionally also
// the straight bf16 copy [R, C] and the fp32 column sums (atomicAdd into colsum[C]) -- one pass over the input.
// 64x64 tiles through LDS; 256 threads.
// kinds: 0 = bf16, 1 = f32 (input only), 2 = f16
__device__ __forceinline__ float load_kind(const void* p, size_t i, int kind) {
    if (kind == 1) return ((const float*)p)[i];
    const bf16_t h = ((const bf16_t*)p)[i];
    return kind == 2 ? h2f(h) : bf2f(h);
}
__device__ __forceinline__ bf16_t store_kind(float v, int kind) { return kind == 2 ? f2h(v) : f2bf(v); }

// 64 x 64 tiles through an fp32 LDS tile; 16-byte global loads along input rows and 16-byte stores along output rows
// (requires C % 64 == 0, which holds for every feature width on this path; R is arbitrary, rows R..Rpad-1 become zeros).
__global__ __launch_bounds__(256) void transpose_kernel(const void* __restrict__ in, int in_kind, int R, int C, int ldin,
                                                        bf16_t* __restrict__ outT, int Rpad, int outT_kind,
                                                        bf16_t* __restrict__ outS, int outS_kind,
                                                        float* __restrict__ colsum) {
    __shared__ float tile[64][65];
    const int c0 = blockIdx.x * 64, r0 = blockIdx.y * 64;
    const int t = threadIdx.x;
    {
        const int row = t >> 2, cg = (t & 3) * 16, r = r0 + row;
        float v[16];
        if (r < R) {
            if (in_kind == 1) {
                const float4* src = reinterpret_cast<const float4*>((const float*)in + (size_t)r * ldin + c0 + cg);
#pragma unroll
                for (int k = 0; k < 4; ++k) { const float4 f = src[k]; v[4 * k] = f.x; v[4 * k + 1] = f.y; v[4 * k + 2] = f.z; v[4 * k + 3] = f.w; }
            } else {
                const uint4* src = reinterpret_cast<const uint4*>((const bf16_t*)in + (size_t)r * ldin + c0 + cg);
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const uint4 u = src[k];
                    const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const bf16_t lo = (bf16_t)(w[e] & 0xFFFF), hi = (bf16_t)(w[e] >> 16);
                        v[8 * k + 2 * e] = in_kind == 2 ? h2f(lo) : bf2f(lo);
                        v[8 * k + 2 * e + 1] = in_kind == 2 ? h2f(hi) : bf2f(hi);
                    }
                }
            }
            if (outS != nullptr) {
                unsigned pk[8];
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    pk[e] = (unsigned)store_kind(v[2 * e], outS_kind) | ((unsigned)store_kind(v[2 * e + 1], outS_kind) << 16);
                uint4* dst = reinterpret_cast<uint4*>(outS + (size_t)r * C + c0 + cg);
                dst[0] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
                dst[1] = make_uint4(pk[4], pk[5], pk[6], pk[7]);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) v[e] = 0.f;
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) tile[row][cg + e] = v[e];
    }
    __syncthreads();
    if (colsum != nullptr && t < 64) {
        float s = 0.f;
#pragma unroll 8
        for (int i = 0; i < 64; ++i) s += tile[i][t];
        unsafeAtomicAdd(&colsum[c0 + t], s);
    }
    if (outT == nullptr) return;
    {
        const int oc = t >> 2, seg = (t & 3) * 16;
        if (r0 + seg < Rpad) {
            unsigned pk[8];
#pragma unroll
            for (int e = 0; e < 8; ++e)
                pk[e] = (unsigned)store_kind(tile[seg + 2 * e][oc], outT_kind) |
                        ((unsigned)store_kind(tile[seg + 2 * e + 1][oc], outT_kind) << 16);
            uint4* dst = reinterpret_cast<uint4*>(outT + (size_t)(c0 + oc) * Rpad + r0 + seg);
            dst[0] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
            dst[1] = make_uint4(pk[4], pk[5], pk[6], pk[7]);
        }
    }
}

extern "C" int sed_transpose_to_bf16(const void* in, int in_kind, int R, int C, int ldin, void* outT, int Rpad,
                                     int outT_kind, void* outS, int outS_kind, float* colsum, hipStream_t stream) {
    (void)hipGetLastError();
    if (Rpad < R || in_kind < 0 || in_kind > 2 || (C % 64) || (Rpad % 16) || (ldin % 8)) return SED_ERR_ARG;
    dim3 grid(cdiv(C, 64), cdiv(Rpad, 64));
    hipLaunchKernelGGL(transpose_kernel, grid, dim3(256), 0, stream, in, in_kind, R, C, ldin, (bf16_t*)outT, Rpad,
                       outT_kind, (bf16_t*)outS, outS_kind, colsum);
    return sed_check_launch();
}

// All weight images of a model in ONE launch.  Per step the engine rebuilds, from the fp32 masters, the straight 16-bit image of
// every GEMM weight, its transposed bf16 image (backward operand) and, for the split-precision layers, the [hi | hi | lo] f16
// image: ~130 launches of 5-20 us for student + teacher.  desc: n_desc x 16 int64 {in fp32, outT bf16 [C, R] or 0,
// outS [R, C] or 0, split f16 [R, 3C] or 0, R, C, outS kind (0 bf16 / 2 f16), first tile index, gather plan int32 [R, C] or 0,
// scale plan fp32 [R, C] or 0, LoRA A fp32 [r, C] or 0, LoRA B fp32 [R, r], r, LoRA scaling (float bits), 0, 0}; one workgroup per
// 64 x 64 tile.  Image element (i, j) = in[plan ? plan[i C + j] : i C + j] * (scale ? scale[i C + j] : 1) + s sum_k B[i, k] A[k, j]:
// the PMAM model's padded context-network / CNN images (a gather of the master with zeros on the padding, round 4) and its merged
// LoRA weights W + s B A (src/models/lora/layers.py:148-151) without an fp32 copy of either.
#define WIMG_DESC 16
__global__ __launch_bounds__(256) void weight_images_kernel(const long long* __restrict__ desc, int n_desc) {
    __shared__ float tile[64][65];
    int lo = 0, hi = n_desc - 1;
    while (lo < hi) {   // last descriptor whose first tile <= blockIdx.x
        const int mid = (lo + hi + 1) >> 1;
        if (desc[(size_t)mid * WIMG_DESC + 7] <= (long long)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const long long* d = desc + (size_t)lo * WIMG_DESC;
    const float* in = reinterpret_cast<const float*>(d[0]);
    bf16_t* outT = reinterpret_cast<bf16_t*>(d[1]);
    bf16_t* outS = reinterpret_cast<bf16_t*>(d[2]);
    bf16_t* outP = reinterpret_cast<bf16_t*>(d[3]);
    const int R = (int)d[4], C = (int)d[5], skind = (int)d[6];
    const int tl = blockIdx.x - (int)d[7], tx = C / 64;
    const int c0 = (tl % tx) * 64, r0 = (tl / tx) * 64;
    const int* gplan = reinterpret_cast<const int*>(d[8]);
    const float* gscale = reinterpret_cast<const float*>(d[9]);
    const float* la = reinterpret_cast<const float*>(d[10]);
    const float* lb = reinterpret_cast<const float*>(d[11]);
    const int lr = (int)d[12];
    const float ls = __int_as_float((int)d[13]);
    const int t = threadIdx.x;
    {
        const int row = t >> 2, cg = (t & 3) * 16, r = r0 + row;
        float v[16];
        if (r < R) {
            const size_t e0 = (size_t)r * C + c0 + cg;
            if (gplan != nullptr) {      // (uniform per workgroup)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int4 ix = reinterpret_cast<const int4*>(gplan + e0)[k];
                    v[4 * k] = in[ix.x]; v[4 * k + 1] = in[ix.y]; v[4 * k + 2] = in[ix.z]; v[4 * k + 3] = in[ix.w];
                }
            } else {
                const float4* src = reinterpret_cast<const float4*>(in + e0);
#pragma unroll
                for (int k = 0; k < 4; ++k) { const float4 f = src[k]; v[4 * k] = f.x; v[4 * k + 1] = f.y; v[4 * k + 2] = f.z; v[4 * k + 3] = f.w; }
            }
            if (gscale != nullptr) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float4 f = reinterpret_cast<const float4*>(gscale + e0)[k];
                    v[4 * k] *= f.x; v[4 * k + 1] *= f.y; v[4 * k + 2] *= f.z; v[4 * k + 3] *= f.w;
                }
            }
            if (la != nullptr) {         // + s B A, accumulated as sed_lora_merge does (k ascending, one fma with s at the end)
                float acc[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[e] = 0.f;
                for (int k = 0; k < lr; ++k) {
                    const float bv = lb[(size_t)r * lr + k];
                    const float4* arow = reinterpret_cast<const float4*>(la + (size_t)k * C + c0 + cg);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 a = arow[q];
                        acc[4 * q] = fmaf(bv, a.x, acc[4 * q]); acc[4 * q + 1] = fmaf(bv, a.y, acc[4 * q + 1]);
                        acc[4 * q + 2] = fmaf(bv, a.z, acc[4 * q + 2]); acc[4 * q + 3] = fmaf(bv, a.w, acc[4 * q + 3]);
                    }
                }
#pragma unroll
                for (int e = 0; e < 16; ++e) v[e] = fmaf(ls, acc[e], v[e]);
            }
            if (outS != nullptr) {
                unsigned pk[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) pk[e] = (unsigned)store_kind(v[2 * e], skind) | ((unsigned)store_kind(v[2 * e + 1], skind) << 16);
                uint4* dst = reinterpret_cast<uint4*>(outS + (size_t)r * C + c0 + cg);
                dst[0] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
                dst[1] = make_uint4(pk[4], pk[5], pk[6], pk[7]);
            }
            if (outP != nullptr) {
                unsigned ph[8], pl[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const bf16_t h0 = f2h(v[2 * e]), h1 = f2h(v[2 * e + 1]);
                    ph[e] = (unsigned)h0 | ((unsigned)h1 << 16);
                    pl[e] = (unsigned)f2h(v[2 * e] - h2f(h0)) | ((unsigned)f2h(v[2 * e + 1] - h2f(h1)) << 16);
                }
                bf16_t* prow = outP + (size_t)r * 3 * C + c0 + cg;
                uint4* d0 = reinterpret_cast<uint4*>(prow);
                uint4* d1 = reinterpret_cast<uint4*>(prow + C);
                uint4* d2 = reinterpret_cast<uint4*>(prow + 2 * C);
                d0[0] = make_uint4(ph[0], ph[1], ph[2], ph[3]); d0[1] = make_uint4(ph[4], ph[5], ph[6], ph[7]);
                d1[0] = make_uint4(ph[0], ph[1], ph[2], ph[3]); d1[1] = make_uint4(ph[4], ph[5], ph[6], ph[7]);
                d2[0] = make_uint4(pl[0], pl[1], pl[2], pl[3]); d2[1] = make_uint4(pl[4], pl[5], pl[6], pl[7]);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) v[e] = 0.f;
        }
        if (outT != nullptr) {
#pragma unroll
            for (int e = 0; e < 16; ++e) tile[row][cg + e] = v[e];
        }
    }
    if (outT == nullptr) return;    // uniform per workgroup
    __syncthreads();
    {
        const int oc = t >> 2, seg = (t & 3) * 16;
        if (r0 + seg < R) {
            unsigned pk[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) pk[e] = pack2bf(tile[seg + 2 * e][oc], tile[seg + 2 * e + 1][oc]);
            uint4* dst = reinterpret_cast<uint4*>(outT + (size_t)(c0 + oc) * R + r0 + seg);
            dst[0] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
            dst[1] = make_uint4(pk[4], pk[5], pk[6], pk[7]);
        }
    }
}
extern "C" int sed_weight_images(const int64_t* desc, int n_desc, int total_tiles, hipStream_t stream) {
    (void)hipGetLastError();
    if (n_desc <= 0 || total_tiles <= 0) return SED_ERR_ARG;
    hipLaunchKernelGGL(weight_images_kernel, dim3(total_tiles), dim3(256), 0, stream, (const long long*)desc, n_desc);
    return sed_check_launch();
}

// ---------------------------------------------------------------------------------------------------------------------
// Weight-rounding correction of the evaluation-mode encoder (engine.py `_wcorr_bias`).  The f16 image of an fp32 weight drops
// W_lo = W - f16(W); the dropped product x . W_lo^T has a part that is the SAME for every token of a clip -- mean_t(x) . W_lo^T -- which
// no later averaging (frequency pooling, attention) reduces, and which is most of the posterior error the image costs (measured
// with tools/err_sim.py: logit error of the f16 weight images 1.6e-3 -> 0.7e-3).  It is a [clips, K] x [K, N] product: the two kernels
// below make its operands (per-clip token means of the 16-bit activation; f16 image of 2^11 W_lo), the ordinary GEMM forms it and
// the main GEMM adds it as a row-group bias.
// x [groups * rows, K] 16-bit -> mean [groups, K] 16-bit (same kind); one workgroup per (group, 256-column chunk), fp32 sums
// `step` > 1: every step-th token only -- an estimate of the mean (the correction needs it to a few per cent; the part of the dropped
// product that varies from token to token is left uncorrected anyway), for 1 / step of the extra pass over the activation
template <bool F16>
__global__ __launch_bounds__(256) void group_colmean_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ out, int rows, int K, int ld, int step) {
    __shared__ float part[8][256];
    const int grp = blockIdx.x, c0 = blockIdx.y * 256;
    // thread = (row slice of 8, 32 column groups of 8 columns = 16 bytes)
    const int cg = threadIdx.x & 31, sl = threadIdx.x >> 5;
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const bf16_t* base = x + (size_t)grp * rows * ld + c0 + cg * 8;
    const int nvis = (rows + step - 1) / step;
    for (int r = sl * step; r < rows; r += 8 * step) {
        const uint4 u = *reinterpret_cast<const uint4*>(base + (size_t)r * ld);
        const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            a[2 * e] += to_f32<F16>((bf16_t)(w[e] & 0xFFFF));
            a[2 * e + 1] += to_f32<F16>((bf16_t)(w[e] >> 16));
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) part[sl][cg * 8 + e] = a[e];
    __syncthreads();
    const int c = threadIdx.x;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += part[i][c];
    out[(size_t)grp * K + c0 + c] = to_16<F16>(s / (float)nvis);
}
extern "C" int sed_group_colmean_ld(const void* x, void* out, int groups, int rows, int K, int ld, int step, int f16, hipStream_t stream) {
    (void)hipGetLastError();
    if (groups <= 0 || rows <= 0 || K % 256 || step < 1 || ld < K || ld % 8) return SED_ERR_ARG;
    if (f16) hipLaunchKernelGGL(group_colmean_kernel<true>, dim3(groups, K / 256), dim3(256), 0, stream, (const bf16_t*)x, (bf16_t*)out, rows, K, ld, step);
    else hipLaunchKernelGGL(group_colmean_kernel<false>, dim3(groups, K / 256), dim3(256), 0, stream, (const bf16_t*)x, (bf16_t*)out, rows, K, ld, step);
    return sed_check_launch();
}
extern "C" int sed_group_colmean(const void* x, void* out, int groups, int rows, int K, int step, int f16, hipStream_t stream) {
    return sed_group_colmean_ld(x, out, groups, rows, K, K, step, f16, stream);
}
// out = f16(scale * (w - f16(w)))  -- what the straight f16 image of an fp32 weight dropped (scale 2^11 keeps it a normal number)
__global__ void weight_residual_kernel(const float* __restrict__ w, bf16_t* __restrict__ out, size_t n4, float scale) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const float4 v = reinterpret_cast<const float4*>(w)[i];
        uint2 p;
        p.x = (unsigned)f2h(scale * (v.x - h2f(f2h(v.x)))) | ((unsigned)f2h(scale * (v.y - h2f(f2h(v.y)))) << 16);
        p.y = (unsigned)f2h(scale * (v.z - h2f(f2h(v.z)))) | ((unsigned)f2h(scale * (v.w - h2f(f2h(v.w)))) << 16);
        reinterpret_cast<uint2*>(out)[i] = p;
    }
}
// e4m3 (OCP) images for the fp8 lo product (GemmArgs.k8); pack4_e4m3: common.h
// rows of [K f16 | K e4m3] (pitch ld halfs): the e4m3 half = 2^-2 x the f16 half
__global__ __launch_bounds__(256) void fp8_tail_kernel(bf16_t* __restrict__ x, int M, int K, int ld) {
    const int per_row = K / 8;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)M * per_row; i += (size_t)gridDim.x * 256) {
        const size_t m = i / per_row;
        const int c = (int)(i - m * per_row);
        bf16_t* row = x + m * ld;
        const uint4 v = *reinterpret_cast<const uint4*>(row + 8 * c);
        uint2 o;
        o.x = e4m3x4_of_h4(v.x, v.y);
        o.y = e4m3x4_of_h4(v.z, v.w);
        *reinterpret_cast<uint2*>(reinterpret_cast<unsigned char*>(row + K) + 8 * c) = o;
    }
}
extern "C" int sed_fp8_tail(void* x, int M, int K, int ld, hipStream_t stream) {
    (void)hipGetLastError();
    if (M <= 0 || K % 8 || ld % 8 || ld < K + K / 2) return SED_ERR_ARG;
    const size_t n = (size_t)M * (K / 8);
    hipLaunchKernelGGL(fp8_tail_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 8192)), dim3(256), 0, stream, (bf16_t*)x, M, K, ld);
    return sed_check_launch();
}
// fp32 weight [N, K] -> rows [f16(W) | e4m3(2^s (W - f16(W)))] (3 K bytes per row)
__global__ __launch_bounds__(256) void weight_two_term_f8_kernel(const float* __restrict__ w, unsigned char* __restrict__ out, size_t N, int K, float scale) {
    const int per_row = K / 4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N * per_row; i += (size_t)gridDim.x * 256) {
        const size_t n = i / per_row;
        const int c = (int)(i - n * per_row);
        const float4 v = *reinterpret_cast<const float4*>(w + n * K + 4 * c);
        const _Float16 h0 = (_Float16)v.x, h1 = (_Float16)v.y, h2 = (_Float16)v.z, h3 = (_Float16)v.w;
        unsigned char* row = out + n * (size_t)(3 * K);
        typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));
        *reinterpret_cast<f16x4_t*>(row + 8 * c) = f16x4_t{h0, h1, h2, h3};
        *reinterpret_cast<unsigned*>(row + 2 * K + 4 * c) =
            pack4_e4m3(scale * (v.x - (float)h0), scale * (v.y - (float)h1), scale * (v.z - (float)h2), scale * (v.w - (float)h3));
    }
}
extern "C" int sed_weight_two_term_f8(const float* w, void* out, int64_t N, int K, int s, hipStream_t stream) {
    (void)hipGetLastError();
    if (N <= 0 || K % 8 || s < -100 || s > 100) return SED_ERR_ARG;
    const size_t n = (size_t)N * (K / 4);
    hipLaunchKernelGGL(weight_two_term_f8_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 8192)), dim3(256), 0, stream, w,
                       (unsigned char*)out, (size_t)N, K, ldexpf(1.f, s));
    return sed_check_launch();
}
extern "C" int sed_weight_residual_f16(const float* w, void* out, int64_t n, float scale, hipStream_t stream) {
    (void)hipGetLastError();
    if (n <= 0 || n % 4) return SED_ERR_ARG;
    const size_t n4 = n / 4;
    int blocks = (int)((n4 + 255) / 256);
    blocks = blocks > 4096 ? 4096 : blocks;
    hipLaunchKernelGGL(weight_residual_kernel, dim3(blocks), dim3(256), 0, stream, w, (bf16_t*)out, n4, scale);
    return sed_check_launch();
}

// rowpart [M][S][2] (per-row partial sums of S column slices) -> rowstat [M][2] = (mean, 1 / sqrt(var + eps)) over D columns
__global__ void ln_fold_stats_kernel(const float* __restrict__ rowpart, float* __restrict__ rowstat, int M, int S, float invD, float eps) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    float s1 = 0.f, s2 = 0.f;
    for (int i = 0; i < S; ++i) {
        const float2 p = *reinterpret_cast<const float2*>(rowpart + ((size_t)m * S + i) * 2);
        s1 += p.x; s2 += p.y;
    }
    const float mean = s1 * invD;
    float var = s2 * invD - mean * mean;
    var = var > 0.f ? var : 0.f;
    *reinterpret_cast<float2*>(rowstat + 2 * (size_t)m) = make_float2(mean, 1.0f / sqrtf(var + eps));
}
extern "C" int sed_ln_fold_stats(const float* rowpart, float* rowstat, int M, int S, int D, float eps, hipStream_t stream) {
    (void)hipGetLastError();
    if (M <= 0 || S <= 0 || D <= 0) return SED_ERR_ARG;
    hipLaunchKernelGGL(ln_fold_stats_kernel, dim3((M + 255) / 256), dim3(256), 0, stream, rowpart, rowstat, M, S, 1.0f / (float)D, eps);
    return sed_check_launch();
}
// Weight side of the fold: W16[n, k] = f16(gamma[k] W[n, k]); colS[n] = sum_k W16[n, k] (of the ROUNDED values: the mean component the
// GEMM accumulates is then cancelled exactly); colC[n] = sum_k beta[k] W[n, k] + bias[n].  One wave per output row.
__global__ __launch_bounds__(256) void ln_fold_weight_kernel(const float* __restrict__ W, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, const float* __restrict__ bias,
                                                             bf16_t* __restrict__ W16, float* __restrict__ colS, float* __restrict__ colC,
                                                             int N, int K) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (n >= N) return;
    float s = 0.f, c = 0.f;
    for (int k = lane * 4; k < K; k += 256) {
        const float4 w = *reinterpret_cast<const float4*>(W + (size_t)n * K + k), gm = *reinterpret_cast<const float4*>(gamma + k),
                     bt = *reinterpret_cast<const float4*>(beta + k);
        const bf16_t h0 = f2h(w.x * gm.x), h1 = f2h(w.y * gm.y), h2 = f2h(w.z * gm.z), h3 = f2h(w.w * gm.w);
        uint2 pk;
        pk.x = (unsigned)h0 | ((unsigned)h1 << 16);
        pk.y = (unsigned)h2 | ((unsigned)h3 << 16);
        *reinterpret_cast<uint2*>(W16 + (size_t)n * K + k) = pk;
        s += (h2f(h0) + h2f(h1)) + (h2f(h2) + h2f(h3));
        c += (bt.x * w.x + bt.y * w.y) + (bt.z * w.z + bt.w * w.w);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); c += __shfl_xor(c, o, 64); }
    if (lane == 0) { colS[n] = s; colC[n] = c + (bias != nullptr ? bias[n] : 0.f); }
}
extern "C" int sed_ln_fold_weight(const float* W, const float* gamma, const float* beta, const float* bias, void* W16, float* colS,
                                  float* colC, int N, int K, hipStream_t stream) {
    (void)hipGetLastError();
    if (N <= 0 || K <= 0 || (K % 4)) return SED_ERR_ARG;
    hipLaunchKernelGGL(ln_fold_weight_kernel, dim3((N + 3) / 4), dim3(256), 0, stream, W, gamma, beta, bias, (bf16_t*)W16, colS, colC, N, K);
    return sed_check_launch();
}

// Split-precision operand images (f16 hi + f16 lo carries ~22 significand bits): a GEMM over the concatenated reduction
// dimension [A_hi | A_lo | A_hi] . [W_hi | W_hi | W_lo]^T accumulates A_hi W_hi + A_lo W_hi + A_hi W_lo in fp32 inside the
// ordinary MFMA kernel.  Used for the context-network GEMMs, whose operand rounding dominates the posterior error.
// in fp32 [M, K] -> out f16 [M, 3K]; mode 0: [hi | lo | hi] (activations), mode 1: [hi | hi | lo] (weights);
// mode 2: out f16 [M, 2K] = [hi | lo], the two-term weight image of sed_gemm_nt_w2 / sed_gemm_qkv_w2
__global__ void split3_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, size_t M, int K, int mode) {
    const size_t total = M * (size_t)(K / 2);
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const size_t m = idx / (K / 2);
        const int k = (int)(idx - m * (K / 2)) * 2;
        const float2 v = *reinterpret_cast<const float2*>(in + m * K + k);
        const bf16_t h0 = f2h(v.x), h1 = f2h(v.y);
        const bf16_t l0 = f2h(v.x - h2f(h0)), l1 = f2h(v.y - h2f(h1));
        const unsigned hi = (unsigned)h0 | ((unsigned)h1 << 16), lo = (unsigned)l0 | ((unsigned)l1 << 16);
        unsigned* row = reinterpret_cast<unsigned*>(out + m * (size_t)((mode == 2 ? 2 : 3) * K));
        row[k / 2] = hi;
        row[(K + k) / 2] = mode == 1 ? hi : lo;
        if (mode != 2) row[(2 * K + k) / 2] = mode == 0 ? hi : lo;
    }
}
extern "C" int sed_split3_f16(const float* in, void* out, int64_t M, int K, int mode, hipStream_t stream) {
    (void)hipGetLastError();
    if (K % 2 || M <= 0 || mode < 0 || mode > 2) return SED_ERR_ARG;
    size_t total = (size_t)M * (K / 2);
    int blocks = (int)((total + 255) / 256);
    blocks = blocks > 4096 ? 4096 : blocks;
    hipLaunchKernelGGL(split3_kernel, dim3(blocks), dim3(256), 0, stream, in, (bf16_t*)out, (size_t)M, K, mode);
    return sed_check_launch();
}

// in-place f16 -> bf16 conversion of saved forward operands that the backward consumes as bf16 MFMA operands
__global__ void f16_to_bf16_kernel(bf16_t* __restrict__ p, size_t n8) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
        uint4 v = reinterpret_cast<uint4*>(p)[i];
        unsigned* w = reinterpret_cast<unsigned*>(&v);
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = pack2bf(h2f((bf16_t)(w[k] & 0xFFFF)), h2f((bf16_t)(w[k] >> 16)));
        reinterpret_cast<uint4*>(p)[i] = v;
    }
}
extern "C" int sed_f16_to_bf16_inplace(void* p, int64_t n, hipStream_t stream) {
    (void)hipGetLastError();
    if (n % 8) return SED_ERR_ARG;
    size_t n8 = n / 8;
    int blocks = (int)((n8 + 255) / 256);
    blocks = blocks > 4096 ? 4096 : (blocks < 1 ? 1 : blocks);
    hipLaunchKernelGGL(f16_to_bf16_kernel, dim3(blocks), dim3(256), 0, stream, (bf16_t*)p, n8);
    return sed_check_launch();
}

// Small-M fp32 linear: out[m, n] = sum_k a[m, k] w[n, k] + b[n]   (one wave per output element row-chunk).
// Used for the batch-independent / per-clip tiny projections (AT-head query, out_proj, 768->10 classifier).
__global__ void small_linear_kernel(const float* __restrict__ a, const float* __restrict__ w,
                                    const float* __restrict__ b, float* __restrict__ out, int M, int N, int K,
                                    int act) {
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (wave >= M * N) return;
    const int m = wave / N, n = wave - m * N;
    float s = 0.f;
    for (int k = lane; k < K; k += 64) s += a[(size_t)m * K + k] * w[(size_t)n * K + k];
    s = wave_sum(s);
    if (lane == 0) {
        s += (b != nullptr ? b[n] : 0.f);
        if (act == 1) s = sigmoidf_(s);
        out[(size_t)m * N + n] = s;
    }
}

extern "C" int sed_small_linear(const float* a, const float* w, const float* b, float* out, int M, int N, int K,
                                int act, hipStream_t stream) {
    (void)hipGetLastError();
    const int64_t waves = (int64_t)M * N;
    hipLaunchKernelGGL(small_linear_kernel, dim3(cdiv(waves * 64, 256)), dim3(256), 0, stream, a, w, b, out, M, N,
                       K, act);
    return sed_check_launch();
}
