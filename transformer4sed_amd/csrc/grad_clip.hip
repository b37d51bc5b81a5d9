// Gradient-norm clipping on the flat fp32 gradient arena (torch.nn.utils.clip_grad_norm_ semantics, norm_type 2): three plain launches,
// no host synchronisation, no float atomics -- every sum runs in a fixed order, so the norms are bit-reproducible run to run.
//
//   sed_grad_sumsq_chunks   one workgroup per chunk (a run of at most SED_GRAD_CHUNK floats inside ONE tensor's arena slice) -> partial[chunk]
//   sed_grad_norm_finalize  one workgroup: per-tensor and global sums of the partials in fp64, norms, total, clip scale
//   sed_scale_by_dev        g *= scale with the scale read from device memory; a scale >= 1 returns before touching g
//
// Chunk length: 16384 floats = 64 KiB per workgroup = 16 independent 16-byte loads per lane, all issued before the first use (enough bytes
// in flight per CU to cover the HBM latency at a few resident workgroups); a 1e8-float arena gives ~6e3 workgroups (several rounds of the
// 256 CUs) and a partial table of ~24 KB, which one workgroup sums in microseconds.  The host table (grad_clip.grad_chunk_table) never
// emits a longer chunk; the kernel itself takes any length.
#include "common.h"
#include "../../include/sed_hip.h"

#define GC_THREADS 256
#define GC_CHUNK 16384
#define GC_ITERS (GC_CHUNK / 4 / GC_THREADS)

// chunk_tab: int32 [n_chunks, 2] = {arena offset (multiple of 4 floats), length in floats}.  Per lane: four accumulators (the components
// of its 16-byte loads) take one square each per load in load order, then (x + y) + (z + w); the < 4 floats behind the last whole 16 bytes
// go to lanes 0..2 afterwards.  Wave: xor butterfly; workgroup: the four wave sums from LDS in wave order.
__global__ __launch_bounds__(GC_THREADS) void grad_sumsq_chunks_kernel(const float* __restrict__ g, const int2* __restrict__ tab,
                                                                       float* __restrict__ partial) {
    __shared__ float s_wave[GC_THREADS / 64];
    const int2 c = tab[blockIdx.x];
    const float* __restrict__ p = g + c.x;
    const float4* __restrict__ p4 = reinterpret_cast<const float4*>(p);
    const int n4 = c.y >> 2, tid = threadIdx.x;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c.y == GC_CHUNK) {      // (uniform) the whole-chunk case: every load independent of the sums
        float4 v[GC_ITERS];
#pragma unroll
        for (int k = 0; k < GC_ITERS; ++k) v[k] = p4[tid + k * GC_THREADS];
#pragma unroll
        for (int k = 0; k < GC_ITERS; ++k) {
            a.x = fmaf(v[k].x, v[k].x, a.x); a.y = fmaf(v[k].y, v[k].y, a.y);
            a.z = fmaf(v[k].z, v[k].z, a.z); a.w = fmaf(v[k].w, v[k].w, a.w);
        }
    } else {
        for (int i = tid; i < n4; i += GC_THREADS) {
            const float4 v = p4[i];
            a.x = fmaf(v.x, v.x, a.x); a.y = fmaf(v.y, v.y, a.y);
            a.z = fmaf(v.z, v.z, a.z); a.w = fmaf(v.w, v.w, a.w);
        }
        const int t = (n4 << 2) + tid;
        if (t < c.y) {
            const float v = p[t];
            a.x = fmaf(v, v, a.x);
        }
    }
    float s = (a.x + a.y) + (a.z + a.w);
    s = wave_sum(s);
    if ((tid & 63) == 0) s_wave[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) partial[blockIdx.x] = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
}

extern "C" int sed_grad_sumsq_chunks(const float* g, const int32_t* chunk_tab, int n_chunks, float* partial, hipStream_t stream) {
    (void)hipGetLastError();
    if (n_chunks < 0 || (n_chunks > 0 && (g == nullptr || chunk_tab == nullptr || partial == nullptr))) return SED_ERR_ARG;
    if (n_chunks == 0) return SED_OK;
    hipLaunchKernelGGL(grad_sumsq_chunks_kernel, dim3(n_chunks), dim3(GC_THREADS), 0, stream, g, reinterpret_cast<const int2*>(chunk_tab),
                       partial);
    return sed_check_launch();
}

// One workgroup.  Tensors are taken 256 at a time: lane t sums the partials of its tensor in chunk order (fp64), writes the tensor's norm and
// leaves the sum in LDS; lane 0 then adds the batch's sums to the running total in layout order.  Nothing is special-cased for non-finite
// values: an inf / NaN partial gives an inf / NaN norm and total, and the scale is whatever torch's formula gives for it
// (max_norm / inf = 0; NaN stays NaN through the clamp, like torch.clamp).
__global__ __launch_bounds__(GC_THREADS) void grad_norm_finalize_kernel(const float* __restrict__ partial, const int* __restrict__ first,
                                                                        int n_tensors, float max_norm, float* __restrict__ norms,
                                                                        float* __restrict__ total_and_scale) {
    __shared__ double s_sum[GC_THREADS];
    const int tid = threadIdx.x;
    double total = 0.0;
    for (int base = 0; base < n_tensors; base += GC_THREADS) {
        const int t = base + tid;
        double acc = 0.0;
        if (t < n_tensors) {
            const int c0 = first[t], c1 = first[t + 1];
            for (int c = c0; c < c1; ++c) acc += (double)partial[c];
            norms[t] = (float)sqrt(acc);
        }
        s_sum[tid] = acc;
        __syncthreads();
        if (tid == 0) {
            const int cnt = min(GC_THREADS, n_tensors - base);
            for (int j = 0; j < cnt; ++j) total += s_sum[j];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const float tn = (float)sqrt(total);
        float scale = 1.0f;
        if (max_norm > 0.0f) {
            const float coef = max_norm / (tn + 1e-6f);
            scale = coef > 1.0f ? 1.0f : coef;      // (a NaN coef fails the comparison and stays NaN)
        }
        total_and_scale[0] = tn;
        total_and_scale[1] = scale;
    }
}

extern "C" int sed_grad_norm_finalize(const float* partial, const int32_t* tensor_first_chunk, int n_tensors, float max_norm, float* norms,
                                      float* total_and_scale, hipStream_t stream) {
    (void)hipGetLastError();
    if (n_tensors < 0 || total_and_scale == nullptr || (n_tensors > 0 && (partial == nullptr || tensor_first_chunk == nullptr || norms == nullptr)))
        return SED_ERR_ARG;
    hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(GC_THREADS), 0, stream, partial, tensor_first_chunk, n_tensors, max_norm,
                       norms, total_and_scale);
    return sed_check_launch();
}

// g[i] = g[i] * scale (one fp32 rounding), 16-byte accesses, four per lane and pass.  The scale is the first thing every workgroup reads; the
// comparison is uniform, and a step that does not clip (scale >= 1) moves no gradient bytes.  A NaN scale fails the comparison and scales.
__global__ __launch_bounds__(GC_THREADS) void scale_by_dev_kernel(float* __restrict__ g, size_t n4, const float* __restrict__ scale) {
    const float s = scale[0];
    if (s >= 1.0f) return;
    float4* __restrict__ g4 = reinterpret_cast<float4*>(g);
    const size_t stride = (size_t)gridDim.x * GC_THREADS;
    for (size_t i = (size_t)blockIdx.x * GC_THREADS + threadIdx.x; i < n4; i += 4 * stride) {
        float4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i + k * stride < n4) v[k] = g4[i + k * stride];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i + k * stride < n4) {
                v[k].x *= s; v[k].y *= s; v[k].z *= s; v[k].w *= s;
                g4[i + k * stride] = v[k];
            }
    }
}

extern "C" int sed_scale_by_dev(float* g, int64_t n, const float* scale, hipStream_t stream) {
    (void)hipGetLastError();
    if (n < 0 || n % 4 || scale == nullptr || (n > 0 && g == nullptr)) return SED_ERR_ARG;
    if (n == 0) return SED_OK;
    const size_t n4 = (size_t)n / 4;
    size_t blocks = (n4 + 4 * GC_THREADS - 1) / (4 * GC_THREADS);
    blocks = blocks > 8192 ? 8192 : blocks;
    hipLaunchKernelGGL(scale_by_dev_kernel, dim3((unsigned)blocks), dim3(GC_THREADS), 0, stream, g, n4, scale);
    return sed_check_launch();
}
