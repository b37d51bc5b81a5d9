// Multilabel average precision on the device: the validation metric of the three AudioSet-Strong loops
// (recipes/audioset_strong/base/passt_cnn/train.py:239-314, detect_any_sound/passt/train.py:134-211, open_vocabulary.py:146-227:
// torchmetrics 0.11 MultilabelAveragePrecision(average="macro"), thresholds=None).
//
// Accumulation (sed_ap_append): each update's [B, C] batch goes into class-major storage, scores [C][cap] fp32 and labels [C][cap] uint8.
// torchmetrics' input formatting runs per batch on the device: if any score of the batch lies outside [0, 1] (NaN included) the whole
// batch goes through a sigmoid.  A small reduction (at most 64 workgroups) takes that flag and the error bits compute() reports, a tiled
// transpose appends.  Nothing is read back by the host.
//
// AP (sed_ap_compute): with s_i the score of clip i, P the positives of a class and `>=` on scores,
//     AP = (1/P) * sum over positives i of  pos_ge(s_i) / all_ge(s_i)
// which is torchmetrics' -sum((r[1:] - r[:-1]) * p[:-1]) over the distinct-threshold curve of _binary_clf_curve: all clips tied at one
// value form one step, and every positive of that step sees the step's precision.  Scores become order-preserving uint32 keys (-0.0
// canonicalised to +0.0), a class is cut into chunks of at most `chunk` clips, and a workgroup sorts a chunk's keys and, separately, its
// positives' keys in LDS (bitonic network in its all-ascending form, so a non-power-of-two length needs no padding slots).  The counts
// are sums over chunks of binary searches; with one chunk (the validation split, N = 16 901) everything stays in LDS and one launch does
// a class.  Each term pos_ge / all_ge is rounded to a 2^-40 fixed-point integer and the terms are summed as integers: the sum does not
// depend on the order of the clips, the chunking or the reduction tree (error <= 2^-41 per term, far below the fp32 result's rounding).
#include "metric_common.h"
#include "../../include/sed_hip.h"

#define AP_THREADS 1024
#define AP_MAX_CHUNK 20000               // 2 x 20000 keys = 160 000 B of LDS: the whole 160 KiB of a CU, less the static reduction slots
#define AP_FIX 1099511627776.0           // 2^40

// first index of a sorted [n] array whose key is >= k
__device__ __forceinline__ int ap_lower_bound(const uint32_t* a, int n, uint32_t k) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ unsigned long long ap_term(int pos_ge, int all_ge) {
    return __double2ull_rn((double)pos_ge / (double)all_ge * AP_FIX);
}

__device__ unsigned long long ap_block_sum(unsigned long long v, unsigned long long* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    unsigned long long s = 0;
    if (threadIdx.x == 0)
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += red[i];
    return s;                            // (valid in thread 0)
}

// Loads chunk `ch` of class `c` into LDS and sorts its keys (`all`) and its positives' keys (`pos`); `npos` is a shared counter.
// -> the chunk's positives.  (Shared by the AP and the ROC kernels.)
__device__ int ap_load_sort(const float* __restrict__ scores, const uint8_t* __restrict__ labels, int cap, int base, int len, int c,
                            uint32_t* all, uint32_t* pos, int* npos) {
    if (threadIdx.x == 0) *npos = 0;
    __syncthreads();
    const float* sc = scores + (size_t)c * cap + base;
    const uint8_t* lb = labels + (size_t)c * cap + base;
    const int lane = threadIdx.x & 63;
    for (int i0 = 0; i0 < len; i0 += blockDim.x) {
        const int i = i0 + threadIdx.x;
        uint32_t k = 0;
        bool p = false;
        if (i < len) {
            k = score_key(sc[i]);
            all[i] = k;
            p = lb[i] != 0;
        }
        // wave-compacted append of the positives (their order is irrelevant: they are sorted next)
        const unsigned long long m = __ballot(p);
        int wbase = 0;
        if (lane == 0 && m) wbase = atomicAdd(npos, __popcll(m));
        wbase = __shfl(wbase, 0, 64);
        if (p) pos[wbase + __popcll(m & ((1ull << lane) - 1ull))] = k;
    }
    __syncthreads();
    const int P = *npos;
    lds_sort(all, len);
    lds_sort(pos, P);
    return P;
}

// grid (nchunks, C).  Loads chunk `ch` of class `c`, sorts its keys and its positives' keys in LDS.  One chunk: counts and sums the
// class right here.  Several: writes both sorted arrays and the positive count to scratch for ap_count_kernel (`partial` may then be
// null: sed_roc_compute sorts its chunks with this kernel too).
__global__ __launch_bounds__(AP_THREADS) void ap_sort_kernel(const float* __restrict__ scores, const uint8_t* __restrict__ labels, int N,
                                                            int cap, int chunk, uint32_t* __restrict__ all_sorted,
                                                            uint32_t* __restrict__ pos_sorted, int* __restrict__ pos_cnt,
                                                            unsigned long long* __restrict__ partial) {
    extern __shared__ uint32_t ap_lds[];
    __shared__ unsigned long long red[AP_THREADS / 64];
    __shared__ int npos;
    const int nch = gridDim.x, ch = blockIdx.x, c = blockIdx.y;
    const int L = chunk < N ? chunk : N;                 // LDS slots per array
    const int base = ch * chunk;
    const int len = min(chunk, N - base);
    uint32_t* all = ap_lds;
    uint32_t* pos = ap_lds + L;
    const int P = ap_load_sort(scores, labels, cap, base, len, c, all, pos, &npos);
    if (nch == 1) {
        unsigned long long acc = 0;
        for (int j = threadIdx.x; j < P; j += blockDim.x) {
            const uint32_t k = pos[j];
            acc += ap_term(P - ap_lower_bound(pos, P, k), len - ap_lower_bound(all, len, k));
        }
        const unsigned long long s = ap_block_sum(acc, red);
        if (threadIdx.x == 0) {
            partial[c] = s;
            pos_cnt[c] = P;
        }
        return;
    }
    uint32_t* ga = all_sorted + (size_t)c * nch * chunk + base;
    uint32_t* gp = pos_sorted + (size_t)c * nch * chunk + base;
    for (int i = threadIdx.x; i < len; i += blockDim.x) ga[i] = all[i];
    for (int i = threadIdx.x; i < P; i += blockDim.x) gp[i] = pos[i];
    if (threadIdx.x == 0) pos_cnt[(size_t)c * nch + ch] = P;
}

// grid (nchunks, C), several chunks only: the positives of chunk `ch`, counted against every chunk's sorted arrays (L2-resident).
__global__ __launch_bounds__(AP_THREADS) void ap_count_kernel(int N, int chunk, const uint32_t* __restrict__ all_sorted,
                                                             const uint32_t* __restrict__ pos_sorted, const int* __restrict__ pos_cnt,
                                                             unsigned long long* __restrict__ partial) {
    __shared__ unsigned long long red[AP_THREADS / 64];
    const int nch = gridDim.x, ch = blockIdx.x, c = blockIdx.y;
    const uint32_t* ga = all_sorted + (size_t)c * nch * chunk;
    const uint32_t* gp = pos_sorted + (size_t)c * nch * chunk;
    const int* pc = pos_cnt + (size_t)c * nch;
    const int P_here = pc[ch];
    unsigned long long acc = 0;
    for (int j = threadIdx.x; j < P_here; j += blockDim.x) {
        const uint32_t k = gp[(size_t)ch * chunk + j];
        int all_ge = 0, pos_ge = 0;
        for (int d = 0; d < nch; ++d) {
            const int len = min(chunk, N - d * chunk), pd = pc[d];
            all_ge += len - ap_lower_bound(ga + (size_t)d * chunk, len, k);
            pos_ge += pd - ap_lower_bound(gp + (size_t)d * chunk, pd, k);
        }
        acc += ap_term(pos_ge, all_ge);
    }
    const unsigned long long s = ap_block_sum(acc, red);
    if (threadIdx.x == 0) partial[(size_t)c * nch + ch] = s;
}

// one thread per class: AP = sum of terms / P (NaN without a positive, torchmetrics' recall = tps / tps[-1] = 0 / 0), positive count.
__global__ void ap_reduce_kernel(const int* __restrict__ pos_cnt, const unsigned long long* __restrict__ partial, int C, int nch,
                                 double* __restrict__ ap, int* __restrict__ npos) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    long long P = 0;
    unsigned long long s = 0;
    for (int d = 0; d < nch; ++d) {
        P += pos_cnt[(size_t)c * nch + d];
        s += partial[(size_t)c * nch + d];
    }
    ap[c] = P > 0 ? (double)s / AP_FIX / (double)P : __longlong_as_double(0x7ff8000000000000ll);
    npos[c] = (int)P;
}

// ap_sort_kernel's dynamic LDS of `lds` bytes (a launch attribute of the kernel, not state of a computation)
static void ap_sort_lds(size_t lds) {
    static size_t attr = 0;
    if (lds > attr) {
        (void)hipFuncSetAttribute((const void*)ap_sort_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr = lds;
    }
}

extern "C" int sed_ap_compute(const float* scores, const uint8_t* labels, int C, int N, int cap, int chunk, uint32_t* all_sorted,
                              uint32_t* pos_sorted, int* pos_cnt, unsigned long long* partial, double* ap, int* npos,
                              hipStream_t stream) {
    (void)hipGetLastError();
    if (C <= 0 || N <= 0 || cap < N || chunk <= 0 || chunk > AP_MAX_CHUNK || !scores || !labels || !pos_cnt || !partial || !ap || !npos)
        return SED_ERR_ARG;
    const int nch = cdiv(N, chunk);
    if (nch > 1 && (!all_sorted || !pos_sorted)) return SED_ERR_ARG;
    if (nch > 65535 || C > 65535) return SED_ERR_ARG;
    const int L = chunk < N ? chunk : N;
    const size_t lds = (size_t)2 * L * sizeof(uint32_t);
    ap_sort_lds(lds);
    hipLaunchKernelGGL(ap_sort_kernel, dim3(nch, C), dim3(AP_THREADS), lds, stream, scores, labels, N, cap, chunk, all_sorted, pos_sorted,
                       pos_cnt, partial);
    int rc = sed_check_launch();
    if (rc) return rc;
    if (nch > 1) {
        hipLaunchKernelGGL(ap_count_kernel, dim3(nch, C), dim3(AP_THREADS), 0, stream, N, chunk, all_sorted, pos_sorted, pos_cnt, partial);
        if ((rc = sed_check_launch())) return rc;
    }
    hipLaunchKernelGGL(ap_reduce_kernel, dim3(cdiv(C, 256)), dim3(256), 0, stream, pos_cnt, partial, C, nch, ap, npos);
    return sed_check_launch();
}

// ---------------------------------------------------------------------------------------------------
// ROC area (sed_roc_compute).  Same storage, chunks and sorted arrays as the AP.  Per class, with neg_lt(k) /
// neg_le(k) the negatives whose key is below / not above k (differences of binary searches in the sorted keys and the sorted positives'
// keys, summed over chunks), every positive i contributes A_i = neg_lt(k_i) + neg_le(k_i) = 2 #neg{key < k_i} + #neg{key = k_i}:
//     auc2  = sum over positives of A_i
//     area2 = sum over positives with key >= k_a of A_i  -  2 tp_a (Nn - fp_a)
// (the trapezoids left of ROC point a, seen from the positives: sum_j dfp_j (tp_j + tp_j-1) + sum_j dtp_j (fp_j + fp_j-1) telescopes
// to 2 fp_a tp_a, and a positive of group j sees fp_j + fp_j-1 = 2 Nn - A_i).  k_a, the key of the last ROC point with
// fp <= F = floor(max_fpr Nn), comes from a bisection on the 32-bit key value (#neg{key >= v} does not grow with v), done by one wave
// whose lanes take a chunk each.  All sums are integers: nothing depends on the order of the items or on the chunking.
// ---------------------------------------------------------------------------------------------------
static_assert(SED_ROC_MAX_CHUNK == AP_MAX_CHUNK && SED_ROC_OUT == 8, "include/sed_hip.h states the chunk rule and the output row");

__device__ __forceinline__ int ap_upper_bound(const uint32_t* a, int n, uint32_t k) {        // first index whose key is > k
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] <= k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The sorted chunks of one class: in scratch (nch chunks, `chunk` slots apart), or the one chunk still in LDS (nch = 1).
struct RocChunks {
    const uint32_t* all;
    const uint32_t* pos;
    const int* pc;              // positives per chunk
    int nch, chunk, N;
    __device__ __forceinline__ int len(int d) const { return min(chunk, N - d * chunk); }
};

struct RocCut {                 // ROC points a and b (section 7g); has_a = 0: a is point 0
    uint32_t k_a;
    int has_a;
    long long fp_a, tp_a, fp_b, tp_b;
};

__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One whole wave: (negatives, positives) with key >= v, v in [0, 2^32]; every lane gets both.
__device__ void roc_ge(const RocChunks& s, unsigned long long v, long long& neg_ge, long long& pos_ge) {
    long long a = 0, p = 0;
    if (v <= 0xffffffffull)
        for (int d = threadIdx.x & 63; d < s.nch; d += 64) {
            const int len = s.len(d), pd = s.pc[d];
            a += len - ap_lower_bound(s.all + (size_t)d * s.chunk, len, (uint32_t)v);
            p += pd - ap_lower_bound(s.pos + (size_t)d * s.chunk, pd, (uint32_t)v);
        }
    a = wave_sum_ll(a);
    pos_ge = wave_sum_ll(p);
    neg_ge = a - pos_ge;
}

// One whole wave: the cut at F = floor(max_fpr Nn).  Every lane returns the same RocCut.
__device__ RocCut roc_cut(const RocChunks& s, long long Nn, double max_fpr) {
    const long long F = (long long)floor(__dmul_rn(max_fpr, (double)Nn));
    unsigned long long lo = 0, hi = 1ull << 32;          // the smallest v with #neg{key >= v} <= F (v = 2^32: none is left)
    for (int it = 0; it < 33 && lo < hi; ++it) {
        const unsigned long long mid = (lo + hi) >> 1;
        long long ng, pg;
        roc_ge(s, mid, ng, pg);
        if (ng <= F) hi = mid; else lo = mid + 1;
    }
    // k_a: the smallest key present that is >= lo; k_b: the largest one below lo (the next ROC point)
    long long ka = 1ll << 32, kb = -1;
    for (int d = threadIdx.x & 63; d < s.nch; d += 64) {
        const int len = s.len(d);
        const uint32_t* a = s.all + (size_t)d * s.chunk;
        const int i = lo <= 0xffffffffull ? ap_lower_bound(a, len, (uint32_t)lo) : len;
        if (i < len) ka = min(ka, (long long)a[i]);
        if (i > 0) kb = max(kb, (long long)a[i - 1]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ka = min(ka, __shfl_xor(ka, o, 64));
        kb = max(kb, __shfl_xor(kb, o, 64));
    }
    RocCut r;
    r.has_a = ka < (1ll << 32);
    r.k_a = r.has_a ? (uint32_t)ka : 0u;
    r.fp_a = r.tp_a = 0;
    if (r.has_a) roc_ge(s, (unsigned long long)ka, r.fp_a, r.tp_a);
    r.fp_b = r.fp_a;
    r.tp_b = r.tp_a;
    if (kb >= 0) roc_ge(s, (unsigned long long)kb, r.fp_b, r.tp_b);
    return r;
}

// A_i of a positive with key k
__device__ __forceinline__ unsigned long long roc_term(const RocChunks& s, uint32_t k) {
    long long a = 0;
    for (int d = 0; d < s.nch; ++d) {
        const int len = s.len(d), pd = s.pc[d];
        const uint32_t* ga = s.all + (size_t)d * s.chunk;
        const uint32_t* gp = s.pos + (size_t)d * s.chunk;
        a += ap_lower_bound(ga, len, k) + ap_upper_bound(ga, len, k) - ap_lower_bound(gp, pd, k) - ap_upper_bound(gp, pd, k);
    }
    return (unsigned long long)a;
}

__device__ __forceinline__ void roc_write(long long* __restrict__ o, long long P, long long Nn, unsigned long long s_all,
                                          unsigned long long s_a, int has_a, long long fp_a, long long tp_a, long long fp_b,
                                          long long tp_b) {
    o[0] = P;
    o[1] = Nn;
    o[2] = (long long)s_all;
    o[3] = has_a ? (long long)s_a - 2 * tp_a * (Nn - fp_a) : 0;
    o[4] = fp_a;
    o[5] = tp_a;
    o[6] = fp_b;
    o[7] = tp_b;
}

// grid (1, C), N <= chunk: sorts a class in LDS, cuts and sums it right there.
__global__ __launch_bounds__(AP_THREADS) void roc_one_kernel(const float* __restrict__ scores, const uint8_t* __restrict__ labels, int N,
                                                            int cap, double max_fpr, long long* __restrict__ out) {
    extern __shared__ uint32_t ap_lds[];
    __shared__ unsigned long long red[AP_THREADS / 64];
    __shared__ int npos;
    __shared__ RocCut cut_s;
    const int c = blockIdx.y;
    uint32_t* all = ap_lds;
    uint32_t* pos = ap_lds + N;
    const int P = ap_load_sort(scores, labels, cap, 0, N, c, all, pos, &npos);
    const RocChunks s = {all, pos, &npos, 1, N, N};
    if (threadIdx.x < 64) {
        const RocCut r = roc_cut(s, (long long)N - P, max_fpr);
        if (threadIdx.x == 0) cut_s = r;
    }
    __syncthreads();
    const RocCut cut = cut_s;
    unsigned long long acc = 0, acc_a = 0;
    for (int j = threadIdx.x; j < P; j += blockDim.x) {
        const uint32_t k = pos[j];
        const unsigned long long a = roc_term(s, k);
        acc += a;
        if (cut.has_a && k >= cut.k_a) acc_a += a;
    }
    const unsigned long long s_all = ap_block_sum(acc, red);
    __syncthreads();                                     // (red is reused)
    const unsigned long long s_a = ap_block_sum(acc_a, red);
    if (threadIdx.x == 0)
        roc_write(out + (size_t)c * 8, P, (long long)N - P, s_all, s_a, cut.has_a, cut.fp_a, cut.tp_a, cut.fp_b, cut.tp_b);
}

// Several chunks.  scratch (uint64): cut word [C] = k_a | has_a << 32, then the partial sums [C][nch][2].
// grid (C), one wave: P, Nn and the cut of a class into out[c][0, 1, 4..7] and the cut word.
__global__ __launch_bounds__(64) void roc_cut_kernel(int N, int chunk, int nch, double max_fpr, const uint32_t* __restrict__ all_sorted,
                                                    const uint32_t* __restrict__ pos_sorted, const int* __restrict__ pos_cnt,
                                                    unsigned long long* __restrict__ scratch, long long* __restrict__ out) {
    const int c = blockIdx.x;
    const RocChunks s = {all_sorted + (size_t)c * nch * chunk, pos_sorted + (size_t)c * nch * chunk, pos_cnt + (size_t)c * nch, nch, chunk, N};
    long long P = 0;
    for (int d = threadIdx.x; d < nch; d += 64) P += s.pc[d];
    P = wave_sum_ll(P);
    const RocCut r = roc_cut(s, (long long)N - P, max_fpr);
    if (threadIdx.x == 0) {
        scratch[c] = (unsigned long long)r.k_a | ((unsigned long long)r.has_a << 32);
        roc_write(out + (size_t)c * 8, P, (long long)N - P, 0, 0, 0, r.fp_a, r.tp_a, r.fp_b, r.tp_b);
    }
}

// grid (nch, C): the positives of chunk `ch` against every chunk's sorted arrays.
__global__ __launch_bounds__(AP_THREADS) void roc_count_kernel(int N, int chunk, int C, const uint32_t* __restrict__ all_sorted,
                                                              const uint32_t* __restrict__ pos_sorted, const int* __restrict__ pos_cnt,
                                                              unsigned long long* __restrict__ scratch) {
    __shared__ unsigned long long red[AP_THREADS / 64];
    const int nch = gridDim.x, ch = blockIdx.x, c = blockIdx.y;
    const RocChunks s = {all_sorted + (size_t)c * nch * chunk, pos_sorted + (size_t)c * nch * chunk, pos_cnt + (size_t)c * nch, nch, chunk, N};
    const unsigned long long word = scratch[c];
    const uint32_t k_a = (uint32_t)word;
    const bool has_a = (word >> 32) != 0;
    const int P_here = s.pc[ch];
    unsigned long long acc = 0, acc_a = 0;
    for (int j = threadIdx.x; j < P_here; j += blockDim.x) {
        const uint32_t k = s.pos[(size_t)ch * chunk + j];
        const unsigned long long a = roc_term(s, k);
        acc += a;
        if (has_a && k >= k_a) acc_a += a;
    }
    const unsigned long long s_all = ap_block_sum(acc, red);
    __syncthreads();
    const unsigned long long s_a = ap_block_sum(acc_a, red);
    if (threadIdx.x == 0) {
        unsigned long long* part = scratch + C + ((size_t)c * nch + ch) * 2;
        part[0] = s_all;
        part[1] = s_a;
    }
}

// one thread per class: the sums over chunks into out[c][2, 3].
__global__ void roc_reduce_kernel(const unsigned long long* __restrict__ scratch, int C, int nch, long long* __restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    unsigned long long s_all = 0, s_a = 0;
    for (int d = 0; d < nch; ++d) {
        s_all += scratch[C + ((size_t)c * nch + d) * 2];
        s_a += scratch[C + ((size_t)c * nch + d) * 2 + 1];
    }
    long long* o = out + (size_t)c * 8;
    roc_write(o, o[0], o[1], s_all, s_a, (int)(scratch[c] >> 32), o[4], o[5], o[6], o[7]);
}

extern "C" int sed_roc_compute(const float* scores, const uint8_t* labels, int C, int N, int cap, int chunk, double max_fpr,
                               uint32_t* all_sorted, uint32_t* pos_sorted, int* pos_cnt, unsigned long long* scratch, long long* out,
                               hipStream_t stream) {
    (void)hipGetLastError();
    if (C <= 0 || N <= 0 || cap < N || chunk <= 0 || chunk > AP_MAX_CHUNK || !scores || !labels || !out) return SED_ERR_ARG;
    if (!(max_fpr > 0.0 && max_fpr <= 1.0)) return SED_ERR_ARG;
    const int nch = cdiv(N, chunk);
    if (nch > 1 && (!all_sorted || !pos_sorted || !pos_cnt || !scratch)) return SED_ERR_ARG;
    if (nch > 65535 || C > 65535) return SED_ERR_ARG;
    const int L = chunk < N ? chunk : N;
    const size_t lds = (size_t)2 * L * sizeof(uint32_t);
    if (nch == 1) {
        static size_t attr = 0;
        if (lds > attr) {
            (void)hipFuncSetAttribute((const void*)roc_one_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            attr = lds;
        }
        hipLaunchKernelGGL(roc_one_kernel, dim3(1, C), dim3(AP_THREADS), lds, stream, scores, labels, N, cap, max_fpr, out);
        return sed_check_launch();
    }
    ap_sort_lds(lds);
    hipLaunchKernelGGL(ap_sort_kernel, dim3(nch, C), dim3(AP_THREADS), lds, stream, scores, labels, N, cap, chunk, all_sorted, pos_sorted,
                       pos_cnt, (unsigned long long*)nullptr);
    int rc = sed_check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(roc_cut_kernel, dim3(C), dim3(64), 0, stream, N, chunk, nch, max_fpr, all_sorted, pos_sorted, pos_cnt, scratch, out);
    if ((rc = sed_check_launch())) return rc;
    hipLaunchKernelGGL(roc_count_kernel, dim3(nch, C), dim3(AP_THREADS), 0, stream, N, chunk, C, all_sorted, pos_sorted, pos_cnt, scratch);
    if ((rc = sed_check_launch())) return rc;
    hipLaunchKernelGGL(roc_reduce_kernel, dim3(cdiv(C, 256)), dim3(256), 0, stream, scratch, C, nch, out);
    return sed_check_launch();
}

// ---------------------------------------------------------------------------------------------------
// Append.  Per batch, torchmetrics 0.11 _multilabel_precision_recall_curve_format: `if not torch.all((preds >= 0) * (preds <= 1)):
// preds = preds.sigmoid()` (NaN counts as outside).  ap_flag_kernel: up to AP_FLAG_BLOCKS workgroups, each ORs the bits of its share
// (1 score outside [0, 1] or NaN, 2 NaN score, 4 target outside {0, 1}) into flags[blockIdx.x] -- one writer per word, no atomics on
// global memory, no clearing between batches.  ap_append_kernel ORs the `nflag` words; its workgroup (0, 0) also folds bits 2 | 4 into
// the sticky status[0] (compute() raises on them; the caller clears it once).
// ---------------------------------------------------------------------------------------------------
#define AP_FLAG_BLOCKS 64

__global__ __launch_bounds__(1024) void ap_flag_kernel(const float* __restrict__ preds, const float* __restrict__ target, int64_t n,
                                                      int* __restrict__ flags) {
    __shared__ int bits;
    if (threadIdx.x == 0) bits = 0;
    __syncthreads();
    int b = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float x = preds[i], t = target[i];
        if (!(x >= 0.f && x <= 1.f)) b |= 1;
        if (x != x) b |= 2;
        if (t != 0.f && t != 1.f) b |= 4;
    }
    for (int o = 32; o > 0; o >>= 1) b |= __shfl_xor(b, o, 64);
    if ((threadIdx.x & 63) == 0 && b) atomicOr(&bits, b);
    __syncthreads();
    if (threadIdx.x == 0) flags[blockIdx.x] = bits;
}

// 32 x 32 tiles: reads along classes, writes along clips (class-major storage).
__global__ __launch_bounds__(256) void ap_append_kernel(const float* __restrict__ preds, const float* __restrict__ target, int B, int C,
                                                       int n0, int cap, const int* __restrict__ flags, int nflag, int* __restrict__ status,
                                                       float* __restrict__ scores, uint8_t* __restrict__ labels) {
    __shared__ float ts[32][33];
    __shared__ uint8_t tl[32][33];
    const int b0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;          // ty 0..7
    int bits = 0;
    for (int i = 0; i < nflag; ++i) bits |= flags[i];
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) status[0] |= bits & 6;
    const bool sig = (bits & 1) != 0;
    for (int r = ty; r < 32; r += 8) {
        const int b = b0 + r, c = c0 + tx;
        if (b < B && c < C) {
            float x = preds[(size_t)b * C + c];
            if (sig) x = 1.0f / (1.0f + expf(-x));
            ts[r][tx] = x;
            tl[r][tx] = target[(size_t)b * C + c] == 1.f ? 1 : 0;
        }
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int c = c0 + r, b = b0 + tx;
        if (b < B && c < C) {
            scores[(size_t)c * cap + n0 + b] = ts[tx][r];
            labels[(size_t)c * cap + n0 + b] = tl[tx][r];
        }
    }
}

extern "C" int sed_ap_append(const float* preds, const float* target, int B, int C, int n0, int cap, int* flags, int* status, float* scores,
                             uint8_t* labels, hipStream_t stream) {
    (void)hipGetLastError();
    if (B < 0 || C <= 0 || n0 < 0 || (int64_t)n0 + B > cap || !flags || !status || !scores || !labels) return SED_ERR_ARG;
    if (B == 0) return SED_OK;
    if (!preds || !target || cdiv(C, 32) > 65535) return SED_ERR_ARG;
    const int64_t n = (int64_t)B * C;
    const int nflag = (int)(n / (1024 * 16) < AP_FLAG_BLOCKS - 1 ? n / (1024 * 16) + 1 : AP_FLAG_BLOCKS);   // >= 16 values per thread
    hipLaunchKernelGGL(ap_flag_kernel, dim3(nflag), dim3(1024), 0, stream, preds, target, n, flags);
    int rc = sed_check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(ap_append_kernel, dim3(cdiv(B, 32), cdiv(C, 32)), dim3(256), 0, stream, preds, target, B, C, n0, cap, flags, nflag,
                       status, scores, labels);
    return sed_check_launch();
}

// Capacity growth: rows [C][n] of the old storage into the new [C][new_cap] (device-to-device, stream-ordered).
extern "C" int sed_ap_grow(const float* old_scores, const uint8_t* old_labels, int C, int n, int old_cap, float* new_scores,
                           uint8_t* new_labels, int new_cap, hipStream_t stream) {
    (void)hipGetLastError();
    if (C <= 0 || n < 0 || n > old_cap || n > new_cap || !new_scores || !new_labels) return SED_ERR_ARG;
    if (n == 0) return SED_OK;
    if (!old_scores || !old_labels) return SED_ERR_ARG;
    hipError_t e = hipMemcpy2DAsync(new_scores, (size_t)new_cap * 4, old_scores, (size_t)old_cap * 4, (size_t)n * 4, C,
                                    hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess)
        e = hipMemcpy2DAsync(new_labels, (size_t)new_cap, old_labels, (size_t)old_cap, (size_t)n, C, hipMemcpyDeviceToDevice, stream);
    return e == hipSuccess ? SED_OK : -(1000 + (int)e);
}
