// Segment scores for the segment-based ROC area: what get_segment_scores and
// get_segment_scores_and_overlap_add (src/codec/decoder.py:138-230) compute on the host from score DataFrames, from the frame scores
// [n, T, C] the forward pass leaves on the device.
//
// sed_segment_pool: segment k of a clip is [k Ls, (k + 1) Ls) for k < ceil(Lc / Ls), not cut at Lc.  Frame f weighs
// w_f = max(0, min(ts[f + 1], end) - max(ts[f], start)) integer microseconds, and
//     pooled = float32( (sum_f double(w_f) * double(y_f)) / double(sum_f w_f) )
// over the frames with w_f > 0 in increasing f, every product and every addition rounded to double once (__dmul_rn / __dadd_rn: the
// compiler must not contract them into fused multiply-adds, which a host restatement cannot follow).  One lane per (clip, segment, class),
// neighbouring lanes on neighbouring classes; a lane walks its own frames only, the first one found by a bounded search in ts.
//
// sed_segment_gather: file segment s and class c average the pooled rows rows[ptr[s] .. ptr[s + 1]) in the order given (the host lists
// them by clip onset): float32( (sum double(pooled)) / count ), 0 without a row, written class-major [C][ld] as sed_roc_compute reads it.
//
// Plain launches on the caller's stream; no workgroup waits for another; every loop is bounded by an argument; plain vector stores; no
// atomics.  status (int [SED_SEG_STATUS_WORDS], sticky, zeroed once by the caller; every writer stores the same 1): [0] a segment
// without weight, [1] a NaN score, [2] a row outside the storage, [3] a row list longer than max_rows.  A NaN is only ever a value.
#include "common.h"
#include "../../include/sed_hip.h"

#define SEG_THREADS 256

// grid (cdiv(max_seg * C, SEG_THREADS), n)
__global__ __launch_bounds__(SEG_THREADS) void segment_pool_kernel(const float* __restrict__ scores, const long long* __restrict__ ts_us,
                                                                  const long long* __restrict__ clip_len_us,
                                                                  const int* __restrict__ row_off, long long seg_us, int T, int C,
                                                                  int max_seg, int cap_rows, float* __restrict__ pooled,
                                                                  int* __restrict__ status) {
    const int clip = blockIdx.y;
    const long long idx = (long long)blockIdx.x * SEG_THREADS + threadIdx.x;
    const int seg = (int)(idx / C), cls = (int)(idx - (long long)seg * C);
    if (seg >= max_seg) return;
    const long long Lc = clip_len_us[clip];
    if (Lc <= 0 || (long long)seg * seg_us >= Lc) return;          // seg >= ceil(Lc / Ls)
    const long long row = (long long)row_off[clip] + seg;
    if (row_off[clip] < 0 || row >= cap_rows) {
        status[SED_SEG_BAD_ROW] = 1;
        return;
    }
    const long long start = (long long)seg * seg_us, end = start + seg_us;
    int lo = 0, hi = T;                                              // first frame with ts[f + 1] > start
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const int mid = (lo + hi) >> 1;
        if (ts_us[mid + 1] <= start) lo = mid + 1; else hi = mid;
    }
    const float* y = scores + (size_t)clip * T * C + cls;
    double num = 0.0;
    long long den = 0;
    bool nan = false;
    for (int f = lo; f < T; ++f) {
        const long long t0 = ts_us[f], t1 = ts_us[f + 1];
        if (t0 >= end) break;
        const long long w = min(t1, end) - max(t0, start);
        if (w <= 0) continue;
        const float v = y[(size_t)f * C];
        nan |= v != v;
        num = __dadd_rn(num, __dmul_rn((double)w, (double)v));
        den += w;
    }
    if (nan) status[SED_SEG_NAN] = 1;
    if (den <= 0) status[SED_SEG_ZERO_WEIGHT] = 1;
    pooled[(size_t)row * C + cls] = den > 0 ? __double2float_rn(__ddiv_rn(num, (double)den)) : 0.0f;
}

extern "C" int sed_segment_pool(const float* scores, const int64_t* ts_us, const int64_t* clip_len_us, const int* row_off, int64_t seg_us,
                                int n, int T, int C, int max_seg, int cap_rows, float* pooled, int* status, hipStream_t stream) {
    (void)hipGetLastError();
    if (n < 0 || T <= 0 || C <= 0 || seg_us <= 0 || max_seg <= 0 || cap_rows < 0 || !status) return SED_ERR_ARG;
    if (n == 0) return SED_OK;
    if (!scores || !ts_us || !clip_len_us || !row_off || !pooled || n > 65535) return SED_ERR_ARG;
    const int64_t lanes = (int64_t)max_seg * C;
    if (lanes > (int64_t)SEG_THREADS * 0x7fffffff) return SED_ERR_ARG;
    hipLaunchKernelGGL(segment_pool_kernel, dim3((unsigned)((lanes + SEG_THREADS - 1) / SEG_THREADS), n), dim3(SEG_THREADS), 0, stream, scores,
                       (const long long*)ts_us, (const long long*)clip_len_us, row_off, (long long)seg_us, T, C, max_seg, cap_rows, pooled,
                       status);
    return sed_check_launch();
}

// grid (cdiv(S * C, SEG_THREADS))
__global__ __launch_bounds__(SEG_THREADS) void segment_gather_kernel(const float* __restrict__ pooled, const int* __restrict__ ptr,
                                                                    const int* __restrict__ rows, int S, int C, int n_rows, int nnz,
                                                                    int max_rows, int ld, float* __restrict__ out,
                                                                    int* __restrict__ status) {
    const long long idx = (long long)blockIdx.x * SEG_THREADS + threadIdx.x;
    if (idx >= (long long)S * C) return;
    const int s = (int)(idx / C), cls = (int)(idx - (long long)s * C);
    const int p0 = ptr[s], p1 = ptr[s + 1];
    float res = 0.0f;
    if (p0 < 0 || p1 < p0 || p1 > nnz) {
        status[SED_SEG_BAD_ROW] = 1;
    } else if (p1 - p0 > max_rows) {
        status[SED_SEG_LONG_LIST] = 1;
    } else if (p1 > p0) {
        double sum = 0.0;
        bool bad = false;
        for (int j = 0; j < max_rows && p0 + j < p1; ++j) {
            const int r = rows[p0 + j];
            if (r < 0 || r >= n_rows) {
                bad = true;
                continue;
            }
            sum = __dadd_rn(sum, (double)pooled[(size_t)r * C + cls]);
        }
        if (bad) status[SED_SEG_BAD_ROW] = 1;
        else res = __double2float_rn(__ddiv_rn(sum, (double)(p1 - p0)));
    }
    out[(size_t)cls * ld + s] = res;
}

extern "C" int sed_segment_gather(const float* pooled, const int* ptr, const int* rows, int S, int C, int n_rows, int nnz, int max_rows,
                                  int ld, float* out, int* status, hipStream_t stream) {
    (void)hipGetLastError();
    if (S <= 0 || C <= 0 || n_rows < 0 || nnz < 0 || max_rows < 0 || ld < S || !ptr || !out || !status) return SED_ERR_ARG;
    if (nnz > 0 && (!pooled || !rows || n_rows == 0)) return SED_ERR_ARG;
    const int64_t lanes = (int64_t)S * C;
    if (lanes > (int64_t)SEG_THREADS * 0x7fffffff) return SED_ERR_ARG;
    hipLaunchKernelGGL(segment_gather_kernel, dim3((unsigned)((lanes + SEG_THREADS - 1) / SEG_THREADS)), dim3(SEG_THREADS), 0, stream, pooled,
                       ptr, rows, S, C, n_rows, nnz, max_rows, ld, out, status);
    return sed_check_launch();
}
