// Long-form detection on the device (transformer4sed_amd/longform.py; DESIGN.md section 7d holds the definitions): a recording of any
// length is cut into overlapping 10 s chunks, the chunks' frame posteriors are stitched into one timeline, the timeline is median / max
// filtered and thresholded into events.  The reference has only an unused stub for this (`get_segment_scores_and_overlap_add`,
// src/codec/decoder.py), so the definitions are this project's.
//
//   sed_longform_gather        wav [L] -> chunks [nk, Lc], chunk j from sample (k0 + j) hop on, zeros from L on
//   sed_longform_stitch        strong [K, C, Tc] (x weak [K, C]) -> timeline [Tt, C]: triangular-capped weighted mean of the covering chunks
//   sed_longform_filter        timeline [T, C] -> [T, C]: the filters of median_filter.hip (same three modes, same element selected) on a
//                              timeline of any length, tiled along T with a halo of real neighbours
//   sed_longform_event_count / sed_longform_event_write     timeline [T, C] > th [C] -> the maximal runs as (class, onset, offset) rows,
//                              class-major, onsets ascending; two passes so the list is allocated at its exact size
//
// Every loop is bounded by its sizes; no kernel waits for another workgroup, none uses a floating-point atomic: every output element is
// computed by one thread from its sources in a fixed order, so results do not change from run to run.
#include "common.h"
#include "median_select.h"

// --------------------------------------------------------------------------------------------------- chunk gather
// One thread per four output samples.  VEC: wav, out, hop and Lc are all 16-byte multiples, so source and destination of a float4 are
// aligned; the float4 that straddles L, and everything without VEC, goes sample by sample.
template <bool VEC>
__global__ __launch_bounds__(256) void lf_gather_kernel(const float* __restrict__ wav, float* __restrict__ out, long long L, long long hop,
                                                        int Lc, int k0) {
    const int j = blockIdx.y;
    const long long base = (long long)(k0 + j) * hop;
    float* dst = out + (size_t)j * Lc;
    const int n4 = (Lc + 3) / 4;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < n4; q += gridDim.x * 256) {
        const int i = 4 * q;
        const long long s = base + i;
        if (VEC && s + 4 <= L) {
            *reinterpret_cast<float4*>(dst + i) = *reinterpret_cast<const float4*>(wav + s);
        } else if (VEC && s >= L) {
            *reinterpret_cast<float4*>(dst + i) = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            for (int e = 0; e < 4 && i + e < Lc; ++e) dst[i + e] = s + e < L ? wav[s + e] : 0.f;
        }
    }
}
extern "C" int sed_longform_gather(const float* wav, float* out, int64_t L, int64_t hop, int Lc, int k0, int nk, hipStream_t stream) {
    (void)hipGetLastError();
    if (L < 1 || hop < 1 || Lc < 1 || k0 < 0 || nk < 1 || nk > 65535) return SED_ERR_ARG;
    const bool vec = hop % 4 == 0 && Lc % 4 == 0 && ((uintptr_t)wav % 16) == 0 && ((uintptr_t)out % 16) == 0;
    const dim3 grid(grid_for((size_t)(Lc + 3) / 4, 256, 512), nk);
    if (vec) hipLaunchKernelGGL(lf_gather_kernel<true>, grid, dim3(256), 0, stream, wav, out, (long long)L, (long long)hop, Lc, k0);
    else hipLaunchKernelGGL(lf_gather_kernel<false>, grid, dim3(256), 0, stream, wav, out, (long long)L, (long long)hop, Lc, k0);
    return sed_check_launch();
}

// --------------------------------------------------------------------------------------------------- stitch
// out[t, c] = sum_k w(t - k Hf) v_k / sum_k w(t - k Hf) over the chunks k that cover frame t, ascending; v_k = strong[k, c, t - k Hf]
// (x weak[k, c]); w(i) = min(i + 1, Tc - i, R), R = max(1, Tc - Hf).  Where one chunk covers t the value is COPIED (x weak: one fp32
// multiply), so a recording of one chunk reproduces the model output bit for bit.  Gather form: a 32 x 32 (frame x class) tile per
// workgroup, read along Tc (contiguous in `strong`), turned in LDS, written along C (contiguous in `out`).
#define LF_ST 32
__global__ __launch_bounds__(256) void lf_stitch_kernel(const float* __restrict__ strong, const float* __restrict__ weak,
                                                        float* __restrict__ out, int K, int C, int Tc, int Hf, long long Tt) {
    __shared__ float tile[LF_ST][LF_ST + 1];          // [class][frame], odd row stride: the turned read is conflict-free
    const long long t0 = (long long)blockIdx.x * LF_ST;
    const int c0 = blockIdx.y * LF_ST;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int R = Tc - Hf > 1 ? Tc - Hf : 1;
    const long long t = t0 + tx;
    if (t < Tt) {
        const long long kh = t / Hf;
        const int khi = kh < K - 1 ? (int)kh : K - 1;
        const int klo = t < Tc ? 0 : (int)((t - Tc) / Hf + 1);
#pragma unroll
        for (int j = 0; j < LF_ST / 8; ++j) {
            const int cl = ty + 8 * j, c = c0 + cl;
            if (c >= C) continue;
            float res;
            if (klo == khi) {
                res = strong[((size_t)klo * C + c) * Tc + (int)(t - (long long)klo * Hf)];
                if (weak != nullptr) res = res * weak[(size_t)klo * C + c];
            } else {
                float num = 0.f;
                int den = 0;
                for (int k = klo; k <= khi; ++k) {
                    const int i = (int)(t - (long long)k * Hf);
                    int w = i + 1 < Tc - i ? i + 1 : Tc - i;
                    w = w < R ? w : R;
                    float v = strong[((size_t)k * C + c) * Tc + i];
                    if (weak != nullptr) v = v * weak[(size_t)k * C + c];
                    num += (float)w * v;
                    den += w;
                }
                res = num / (float)den;
            }
            tile[cl][tx] = res;
        }
    }
    __syncthreads();
    const int c = c0 + tx;
#pragma unroll
    for (int j = 0; j < LF_ST / 8; ++j) {
        const int tl = ty + 8 * j;
        if (t0 + tl < Tt && c < C) out[(size_t)(t0 + tl) * C + c] = tile[tx][tl];
    }
}
extern "C" int sed_longform_stitch(const float* strong, const float* weak, float* out, int K, int C, int Tc, int Hf, int64_t Tt,
                                   hipStream_t stream) {
    (void)hipGetLastError();
    if (K < 1 || C < 1 || Tc < 1 || Hf < 1 || Hf > Tc || Tt < 1 || Tt > (int64_t)(K - 1) * Hf + Tc) return SED_ERR_ARG;
    const int64_t gx = (Tt + LF_ST - 1) / LF_ST;
    const int gy = (C + LF_ST - 1) / LF_ST;
    if (gx > 0x7fffffffLL || gy > 65535) return SED_ERR_ARG;
    hipLaunchKernelGGL(lf_stitch_kernel, dim3((unsigned)gx, gy), dim3(256), 0, stream, strong, weak, out, K, C, Tc, Hf, (long long)Tt);
    return sed_check_launch();
}

// --------------------------------------------------------------------------------------------------- long filter
// The three filters of median_filter.hip (mode 0: median_filter_torch, even size -> size + 1, replicate padding; mode 1 / 2: scipy median /
// maximum filter, window [i - k/2, i - k/2 + k), edge-inclusive reflection) on in / out [T, C] with any T.  One workgroup per (tile of
// LF_TILE frames, class): the tile with k - 1 halo frames goes to LDS as the PADDED segment vp[0 .. n), n = frames + k - 1, where
// vp[p] is frame t0 + p - k/2 -- a real neighbour wherever one exists; the boundary rule applies at frames < 0 and >= T only, the two
// true ends of the timeline.  The window of local output i is then vp[i .. i + k).  Selection by median_select.h, as in median_filter.hip
// and therefore bit-identical to it: windows below 24 frames by rank search in window order, longer ones by global ranks of the segment
// (ties by position) and a per-thread bitmap over ranks that slides with the window; the maximum by fmaxf in window order.
#define LF_TILE 1024
#define LF_MAXN 2048                     // frames + halo of one tile: windows up to LF_MAXN - LF_TILE + 1 = 1025 frames
__global__ __launch_bounds__(256) void lf_filter_kernel(const float* __restrict__ in, float* __restrict__ out, const int* __restrict__ sizes,
                                                        long long T, int C, int mode, int max_k, int W) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lf_lds[];
    const MedselLds s = medsel_carve(lf_lds, LF_MAXN);                               // (byrank, rk, bm: launches with long windows only; W odd)
    const int tid = threadIdx.x;
    const int c = blockIdx.x % C;                     // class fastest: the workgroups in flight together share the lines they read
    const long long t0 = (long long)(blockIdx.x / C) * LF_TILE;
    const int len = T - t0 < LF_TILE ? (int)(T - t0) : LF_TILE;
    int k = sizes[c];
    k = k < 1 ? 1 : k;
    if (mode == 0 && (k & 1) == 0) k += 1;
    if (k > max_k) {                                  // a window beyond the caller's bound: loud in the data, never a read past LDS
        for (int i = tid; i < len; i += 256) out[(size_t)(t0 + i) * C + c] = __builtin_nanf("");
        return;
    }
    const int lo = k / 2, n = len + k - 1;
    for (int p = tid; p < n; p += 256) {
        long long f = medsel_src(t0 + p - lo, T, mode);
        f = f < 0 ? 0 : (f >= T ? T - 1 : f);         // (reflection is single for k <= T, which the caller checks; this keeps any k in bounds)
        s.vp[p] = in[(size_t)f * C + c];
    }
    __syncthreads();
    float* o = out + (size_t)t0 * C + c;
    if (mode == 2) {
        for (int i = tid; i < len; i += 256) o[(size_t)i * C] = medsel_window_max([&](int j) { return s.vp[i + j]; }, k);
        return;
    }
    if (k < MEDSEL_RANK_MIN) {
        for (int i = tid; i < len; i += 256) o[(size_t)i * C] = medsel_rank_search([&](int j) { return s.vp[i + j]; }, k);
        return;
    }
    medsel_rank_column(s.vp, n, s.rk, s.byrank);
    __syncthreads();
    const int chunk = (len + 255) / 256, i0 = tid * chunk;
    if (i0 >= len) return;
    medsel_slide(s.rk, s.byrank, s.bm + tid * W, W, k, i0, i0 + chunk < len ? i0 + chunk : len, o, C);
}
extern "C" int sed_longform_filter(const float* in, float* out, const int* sizes, int64_t T, int C, int mode, int max_size,
                                   hipStream_t stream) {
    (void)hipGetLastError();
    if (mode < 0 || mode > 2 || T < 1 || T > 0x7fffffffLL || C < 1 || max_size < 1) return SED_ERR_ARG;
    const int max_k = (mode == 0 && (max_size & 1) == 0) ? max_size + 1 : max_size;
    if (LF_TILE + max_k - 1 > LF_MAXN) return SED_ERR_ARG;
    if (mode != 0 && max_size > T) return SED_ERR_ARG;           // scipy's extension of a line shorter than the window is not reproduced
    const int64_t nwg = (T + LF_TILE - 1) / LF_TILE * C;
    if (nwg > 0x7fffffffLL) return SED_ERR_ARG;
    const int n_max = (T < LF_TILE ? (int)T : LF_TILE) + max_k - 1;
    const int W = medsel_bitmap_stride(n_max);
    const bool ranks = mode != 2 && max_k >= MEDSEL_RANK_MIN;      // (the kernel chooses per class: k >= MEDSEL_RANK_MIN)
    const size_t lds = ranks ? medsel_rank_lds(LF_MAXN, W) : (size_t)LF_MAXN * 4;
    static size_t attr = 0;
    if (lds > attr) { (void)hipFuncSetAttribute((const void*)lf_filter_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); attr = lds; }
    hipLaunchKernelGGL(lf_filter_kernel, dim3((unsigned)nwg), dim3(256), lds, stream, in, out, sizes, (long long)T, C, mode, max_k, W);
    return sed_check_launch();
}

// --------------------------------------------------------------------------------------------------- events
// Frame t of class c is active iff post[t, c] > th[c] (strict; NaN is inactive).  A run starts at t where t is active and t - 1 is not
// (or t = 0) and ends at t where t is active and t + 1 is not (or t = T - 1): the j-th start and the j-th end of a class are the same
// run.  The timeline is cut into segments of `seg` frames; one workgroup per (class, segment).
//   count:  starts per (class, segment), then one workgroup scans them class-major into seg_offs [C nseg + 1] and cls_offs [C + 1]
//           (row of each class's first event; cls_offs[C] = number of events) -- what the host reads to allocate.
//   write:  a workgroup walks its segment 256 frames at a time, positions from a block scan of the start flags (and one of the end
//           flags) plus the running offset; starts write (class, onset), ends write offset = t + 1 into rows [n, 3].  The ends before
//           a segment number the starts before it, less one if a run crosses its first frame.
__device__ __forceinline__ int lf_block_excl(bool flag, int* total, int* wsum) {      // wsum: 4 ints of LDS
    const unsigned long long b = __ballot(flag);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pre = __popcll(b & ((1ull << lane) - 1ull));
    __syncthreads();                                  // (the previous call's readers are done with wsum)
    if (lane == 0) wsum[wave] = __popcll(b);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const int s = wsum[w]; off += w < wave ? s : 0; tot += s; }
    *total = tot;
    return off + pre;
}
__device__ __forceinline__ bool lf_active(const float* __restrict__ post, long long t, long long T, int C, int c, float th) {
    return t >= 0 && t < T && post[(size_t)t * C + c] > th;
}
__global__ __launch_bounds__(256) void lf_event_count_kernel(const float* __restrict__ post, const float* __restrict__ th, long long T,
                                                             int C, int seg, int* __restrict__ seg_counts) {
    __shared__ int wsum[4];
    const int c = blockIdx.x, s = blockIdx.y, nseg = gridDim.y;
    const float thr = th[c];
    const long long t0 = (long long)s * seg, t1 = t0 + seg < T ? t0 + seg : T;
    int cnt = 0;
    for (long long t = t0 + threadIdx.x; t < t1; t += 256)
        cnt += lf_active(post, t, T, C, c, thr) && !lf_active(post, t - 1, T, C, c, thr);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) seg_counts[(size_t)c * nseg + s] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}
__global__ __launch_bounds__(256) void lf_event_scan_kernel(const int* __restrict__ seg_counts, int n, int nseg, int* __restrict__ seg_offs,
                                                            int* __restrict__ cls_offs) {
    __shared__ int wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + threadIdx.x;
        const int v = i < n ? seg_counts[i] : 0;
        int inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(inc, o, 64); inc += lane >= o ? u : 0; }
        __syncthreads();
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int off = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { const int s = wsum[w]; off += w < wave ? s : 0; tot += s; }
        if (i < n) {
            const int ex = carry + off + inc - v;
            seg_offs[i] = ex;
            if (i % nseg == 0) cls_offs[i / nseg] = ex;
        }
        carry += tot;
    }
    if (threadIdx.x == 0) { seg_offs[n] = carry; cls_offs[n / nseg] = carry; }
}
__global__ __launch_bounds__(256) void lf_event_write_kernel(const float* __restrict__ post, const float* __restrict__ th, long long T,
                                                             int C, int seg, const int* __restrict__ seg_offs, int* __restrict__ events) {
    __shared__ int wsum[4];
    const int c = blockIdx.x, s = blockIdx.y, nseg = gridDim.y;
    const float thr = th[c];
    const long long t0 = (long long)s * seg, t1 = t0 + seg < T ? t0 + seg : T;
    int sbase = seg_offs[(size_t)c * nseg + s];
    int ebase = sbase - (lf_active(post, t0 - 1, T, C, c, thr) && lf_active(post, t0, T, C, c, thr) ? 1 : 0);
    for (long long tb = t0; tb < t1; tb += 256) {                // (uniform trip count: every thread reaches the barriers of the scans)
        const long long t = tb + threadIdx.x;
        const bool in = t < t1;
        const bool a = in && lf_active(post, t, T, C, c, thr);
        const bool st = a && !lf_active(post, t - 1, T, C, c, thr);
        const bool en = a && !lf_active(post, t + 1, T, C, c, thr);
        int ns, ne;
        const int ps = lf_block_excl(st, &ns, wsum);
        const int pe = lf_block_excl(en, &ne, wsum);
        if (st) {
            int* row = events + (size_t)(sbase + ps) * 3;
            row[0] = c;
            row[1] = (int)t;
        }
        if (en) events[(size_t)(ebase + pe) * 3 + 2] = (int)(t + 1);
        sbase += ns;
        ebase += ne;
    }
}
static int lf_event_args(int64_t T, int C, int seg) {
    if (T < 1 || T >= 0x7fffffffLL || C < 1 || C > 0x7fffffff / 2 || seg < 1) return SED_ERR_ARG;
    const int64_t nseg = (T + seg - 1) / seg;
    if (nseg > 65535 || nseg * C >= 0x7fffffffLL || (T + 1) / 2 * C >= 0x7fffffffLL / 3) return SED_ERR_ARG;
    return (int)nseg;
}
extern "C" int sed_longform_event_count(const float* post, const float* th, int64_t T, int C, int seg, int* seg_counts, int* seg_offs,
                                        int* cls_offs, hipStream_t stream) {
    (void)hipGetLastError();
    const int nseg = lf_event_args(T, C, seg);
    if (nseg < 0) return SED_ERR_ARG;
    hipLaunchKernelGGL(lf_event_count_kernel, dim3(C, nseg), dim3(256), 0, stream, post, th, (long long)T, C, seg, seg_counts);
    hipLaunchKernelGGL(lf_event_scan_kernel, dim3(1), dim3(256), 0, stream, seg_counts, C * nseg, nseg, seg_offs, cls_offs);
    return sed_check_launch();
}
extern "C" int sed_longform_event_write(const float* post, const float* th, int64_t T, int C, int seg, const int* seg_offs, int* events,
                                        hipStream_t stream) {
    (void)hipGetLastError();
    const int nseg = lf_event_args(T, C, seg);
    if (nseg < 0) return SED_ERR_ARG;
    hipLaunchKernelGGL(lf_event_write_kernel, dim3(C, nseg), dim3(256), 0, stream, post, th, (long long)T, C, seg, seg_offs, events);
    return sed_check_launch();
}
