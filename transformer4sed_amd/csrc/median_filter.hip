// Median / max filter along time per class, both reference semantics, bit-exact (compare / select only; median_select.h holds the
// selection the rank kernel and the bank here and lf_filter_kernel of longform.hip share):
//   mode 0: src/postprocess/filter.py:4-36   even size -> size+1, replicate padding, true median
//   mode 1: scipy.ndimage.median_filter as called at src/codec/decoder.py:91: window [i - k/2, i - k/2 + k),
//           symmetric (edge-inclusive reflect) padding, element of rank k/2
//   mode 2: scipy.ndimage.maximum_filter (decoder.py:94), same window/padding
//
//   sed_median_filter{,_k}     the clip filter: in / out [B, T, C], one window per class; every score table and event list of validation
//   sed_median_filter_bank     in [B, T, C] -> out [W, B, T, C], out[w] = the clip filter with the window row sizes[w, :], for W candidate
//                              rows at once (transformer4sed_amd/postproc_search.py)
//
// Optional per-(b,c) multiplier applied first (soft weak mask, decoder.py:80) or hard zeroing (decoder.py:22-23) via `scale` [B, C].
// Which selection runs is a function of (mode, T, max_size) alone (medsel_use_ranks), the same for the clip filter and the bank.
//
// Every loop is bounded by T, W or max_size; no workgroup waits for another; there is no atomic; every output element is written by one
// thread: the same bits in every run.  A window outside its bound comes out as a NaN plane: loud in the data, never a read past LDS.
#include "median_select.h"

// ---------------------------------------------------------------------------------------------------  the clip filter
// One workgroup per (b, c).  The rank-search kernel keeps the column UNPADDED and maps window positions to frames on the fly: it serves
// sed_median_filter, whose windows live on the device, so the host cannot size a padded column for it.  It restates the boundary
// rule, the rank search and the maximum of median_select.h in place: written over a load functor the same steps compiled to other
// loop counters and one more register here, 1 % slower at [32, 1000, 407] (profiles/median_filter_core_ab.txt).
__global__ __launch_bounds__(256) void median_filter_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                            const int* __restrict__ sizes, const float* __restrict__ scale,
                                                            int T, int C, int mode) {
    extern __shared__ float col[];  // [T]
    const int b = blockIdx.x / C, c = blockIdx.x - b * C;
    const float sc = scale != nullptr ? scale[b * C + c] : 1.0f;
    for (int t = threadIdx.x; t < T; t += 256) {
        const float v = in[((size_t)b * T + t) * C + c];
        col[t] = scale != nullptr ? v * sc : v;
    }
    __syncthreads();
    int k = sizes[c];
    if (mode == 0 && (k & 1) == 0) k += 1;
    const int lo = k / 2, rank = k / 2;
    for (int i = threadIdx.x; i < T; i += 256) {
        float res = 0.f;
        if (mode == 2) {
            float m = -INFINITY;
            for (int j = 0; j < k; ++j) {
                int idx = i - lo + j;
                idx = idx < 0 ? -idx - 1 : (idx >= T ? 2 * T - idx - 1 : idx);
                m = fmaxf(m, col[idx]);
            }
            res = m;
        } else {
            for (int a = 0; a < k; ++a) {
                int ia = i - lo + a;
                if (mode == 0) ia = ia < 0 ? 0 : (ia >= T ? T - 1 : ia);
                else ia = ia < 0 ? -ia - 1 : (ia >= T ? 2 * T - ia - 1 : ia);
                const float va = col[ia];
                int lt = 0, le = 0;
                for (int j = 0; j < k; ++j) {
                    int ij = i - lo + j;
                    if (mode == 0) ij = ij < 0 ? 0 : (ij >= T ? T - 1 : ij);
                    else ij = ij < 0 ? -ij - 1 : (ij >= T ? 2 * T - ij - 1 : ij);
                    const float vj = col[ij];
                    lt += vj < va;
                    le += vj <= va;
                }
                if (lt <= rank && rank < le) { res = va; break; }
            }
        }
        out[((size_t)b * T + i) * C + c] = res;
    }
}
// The same median (modes 0 and 1) for long windows -- the evaluation path filters with 32 / 128 frames (train.py:221-227: median_window
// / 156 * 1000), where the rank search above is O(k^2) per output (4.5 ms per launch, 7 % of a validation batch): global ranks of the
// column padded for the class's own window (T + k - 1 entries), every thread a chunk of consecutive outputs.  A window above the
// caller's bound, beyond the bitmaps sized from it, or below 1 after mode 0's even -> odd step (a 0 there is the window 1, as in the
// kernel above) is a NaN plane.
__global__ __launch_bounds__(256) void median_filter_rank_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                 const int* __restrict__ sizes, const float* __restrict__ scale,
                                                                 int T, int C, int mode, int max_size, int W) {
    extern __shared__ unsigned char medr_lds[];
    const MedselLds s = medsel_carve(medr_lds, MEDSEL_MAXN);                        // (W odd)
    const int b = blockIdx.x / C, c = blockIdx.x - b * C, tid = threadIdx.x;
    const float sc = scale != nullptr ? scale[b * C + c] : 1.0f;
    int k = sizes[c];
    const bool ok = k <= max_size;
    if (mode == 0 && (k & 1) == 0) k += 1;
    const int lo = k / 2, n = T + k - 1;
    float* o = out + (size_t)b * T * C + c;
    if (!ok || k < 1 || n > MEDSEL_MAXN || n > 32 * W) {  // (uniform over the workgroup)
        for (int i = tid; i < T; i += 256) o[(size_t)i * C] = __builtin_nanf("");
        return;
    }
    for (int p = tid; p < n; p += 256) {
        const float v = in[((size_t)b * T + medsel_src(p - lo, T, mode)) * C + c];
        s.vp[p] = scale != nullptr ? v * sc : v;
    }
    __syncthreads();
    medsel_rank_column(s.vp, n, s.rk, s.byrank);
    __syncthreads();
    const int chunk = (T + 255) / 256, i0 = tid * chunk;
    if (i0 >= T) return;
    medsel_slide(s.rk, s.byrank, s.bm + tid * W, W, k, i0, i0 + chunk < T ? i0 + chunk : T, o, C);
}
static int median_filter_impl(const float* in, float* out, const int* sizes, const float* scale, int B, int T, int C, int mode,
                              int max_size, hipStream_t stream) {
    (void)hipGetLastError();
    if (mode < 0 || mode > 2 || T > 12288 || max_size < 0) return SED_ERR_ARG;
    // max_size: the caller's bound on the window sizes (they live on the device); 0 = unknown -> the rank-search kernel
    if (medsel_use_ranks(mode, T, max_size)) {
        const int W = medsel_bitmap_stride(T + max_size + 1);
        const size_t lds = medsel_rank_lds(MEDSEL_MAXN, W);
        static size_t attr = 0;
        if (lds > attr) { (void)hipFuncSetAttribute((const void*)median_filter_rank_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); attr = lds; }
        hipLaunchKernelGGL(median_filter_rank_kernel, dim3(B * C), dim3(256), lds, stream, in, out, sizes, scale, T, C, mode, max_size, W);
        return sed_check_launch();
    }
    hipLaunchKernelGGL(median_filter_kernel, dim3(B * C), dim3(256), T * sizeof(float), stream, in, out, sizes, scale, T,
                       C, mode);
    return sed_check_launch();
}
extern "C" int sed_median_filter(const float* in, float* out, const int* sizes, const float* scale, int B, int T, int C,
                                 int mode, hipStream_t stream) {
    return median_filter_impl(in, out, sizes, scale, B, T, C, mode, 0, stream);
}
// the same filter with the caller's bound on the (device-resident) window sizes: long windows take the rank kernel
extern "C" int sed_median_filter_k(const float* in, float* out, const int* sizes, const float* scale, int B, int T, int C,
                                   int mode, int max_size, hipStream_t stream) {
    return median_filter_impl(in, out, sizes, scale, B, T, C, mode, max_size, stream);
}

// ---------------------------------------------------------------------------------------------------  the bank
// out[w] holds the bits sed_median_filter_k(in, ., sizes[w], scale, B, T, C, mode, max_size) writes, because the same ELEMENT of the input
// is selected -- the result is always an input value (x scale: one fp32 multiply, done once while staging), never an arithmetic combination.
//   * global ranks: a (clip, class) column is staged ONCE with the padding of the class's widest window (K - 1 entries, K/2 in front),
//     and its n = T + K - 1 entries are ranked ONCE -- the n^2 / 256 compares per thread that bound the clip kernel, which it repeats on
//     every call.  Every window k <= K of the W rows is a contiguous run of that one padded column, starting (K/2 - k/2) entries later
//     than the widest; the order of a run's entries by (value, position) is the same in the shared column as in the column padded for
//     k alone, so the (k/2 + 1)-th set bit of the run's bitmap over ranks is the element the clip kernel returns.
//   * otherwise: the clip kernel's rank search (or fmaxf) in window order, over the same staged column.
// Work split: one workgroup per (clip, class), every window row inside it.  The shared arrays hold one column whatever W is, and the
// bitmaps belong to threads, not to windows (256 threads x ceil(n / 32) words): at T = 1000, max_size = 1024 that is 20 KB + 65 KB = 85 KB
// of the CU's 160 KB, so all W <= 64 rows are served from one residency and W needs no grouping; at the search's own sizes (windows up
// to 179 frames) it is 50 KB and three workgroups share a CU.  The 256 threads are dealt to (row, chunk of frames) pairs, 256 / W chunks
// per row, so a thread builds its bitmap once per chunk of about T W / 256 outputs.
// A (row, class) whose window is below 1, above max_size or (modes 1 / 2) above T comes out as NaN.
#define FB_MAX_W 64
#define FB_SEARCH_MAXN 16384             // padded column of the rank-search form: 64 KB

template <bool RANKS>
__global__ __launch_bounds__(256) void filter_bank_kernel(const float* __restrict__ in, float* __restrict__ out, const int* __restrict__ sizes,
                                                          const float* __restrict__ scale, int B, int T, int C, int W, int mode, int max_size,
                                                          int n_cap, int Wb) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fb_lds[];
    __shared__ int ks[FB_MAX_W];                                                     // effective window of row w, 0 = out of range
    const MedselLds s = medsel_carve(fb_lds, n_cap);                                 // (byrank, rk, bm: RANKS only; Wb odd)
    const int b = blockIdx.x / C, c = blockIdx.x - b * C, tid = threadIdx.x;
    const float sc = scale != nullptr ? scale[b * C + c] : 1.0f;
    if (tid < W) {
        int k = sizes[tid * C + c];
        const bool ok = k >= 1 && k <= max_size && (mode == 0 || k <= T);
        if (mode == 0 && (k & 1) == 0) k += 1;
        ks[tid] = ok ? k : 0;
    }
    __syncthreads();
    int K = 0;
    for (int w = 0; w < W; ++w) K = ks[w] > K ? ks[w] : K;
    for (int w = 0; w < W; ++w) {
        if (ks[w] != 0) continue;
        float* o = out + ((size_t)w * B + b) * T * C + c;
        for (int i = tid; i < T; i += 256) o[(size_t)i * C] = __builtin_nanf("");
    }
    const int LO = K / 2, n = T + K - 1;
    if (K == 0 || n > n_cap) return;                  // (n <= n_cap by the host's sizing; uniform over the workgroup)
    for (int p = tid; p < n; p += 256) {
        const float v = in[((size_t)b * T + medsel_src(p - LO, T, mode)) * C + c];
        s.vp[p] = scale != nullptr ? v * sc : v;
    }
    __syncthreads();
    if (!RANKS) {
        for (int idx = tid; idx < W * T; idx += 256) {                  // frames fastest: a wave reads consecutive LDS words
            const int w = idx / T, i = idx - w * T, k = ks[w];
            if (k == 0) continue;
            const float* run = s.vp + i + LO - k / 2;
            const auto win = [&](int j) { return run[j]; };
            out[(((size_t)w * B + b) * T + i) * C + c] = mode == 2 ? medsel_window_max(win, k) : medsel_rank_search(win, k);
        }
        return;
    }
    medsel_rank_column(s.vp, n, s.rk, s.byrank);
    __syncthreads();
    const int nch = 256 / W, w = tid / nch, ch = tid - w * nch;        // (row, chunk) of this thread
    if (w >= W) return;
    const int k = ks[w];
    const int chunk = (T + nch - 1) / nch, i0 = ch * chunk;
    if (k == 0 || i0 >= T) return;
    medsel_slide(s.rk + LO - k / 2, s.byrank, s.bm + tid * Wb, Wb, k, i0, i0 + chunk < T ? i0 + chunk : T,
                 out + ((size_t)w * B + b) * T * C + c, C);
}

extern "C" int sed_median_filter_bank(const float* in, float* out, const int* sizes, const float* scale, int B, int T, int C, int W, int mode,
                                      int max_size, hipStream_t stream) {
    (void)hipGetLastError();
    if (in == nullptr || out == nullptr || sizes == nullptr) return SED_ERR_ARG;
    if (mode < 0 || mode > 2 || B < 1 || T < 1 || T > 12288 || C < 1 || W < 1 || W > FB_MAX_W || max_size < 1) return SED_ERR_ARG;
    if ((int64_t)B * C > 0x7fffffffLL) return SED_ERR_ARG;
    int max_k = (mode == 0 && (max_size & 1) == 0) ? max_size + 1 : max_size;
    if (mode != 0 && max_k > T) max_k = T;                                 // longer windows come out as NaN and are not staged
    const int n_cap = (T + max_k - 1 + 3) & ~3;
    if (medsel_use_ranks(mode, T, max_size)) {
        const int Wb = medsel_bitmap_stride(n_cap);
        const size_t lds = medsel_rank_lds(n_cap, Wb);
        static size_t attr = 0;
        if (lds > attr) { (void)hipFuncSetAttribute((const void*)filter_bank_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); attr = lds; }
        hipLaunchKernelGGL(filter_bank_kernel<true>, dim3((unsigned)(B * C)), dim3(256), lds, stream, in, out, sizes, scale, B, T, C, W, mode,
                           max_size, n_cap, Wb);
    } else {
        if (n_cap > FB_SEARCH_MAXN) return SED_ERR_ARG;
        hipLaunchKernelGGL(filter_bank_kernel<false>, dim3((unsigned)(B * C)), dim3(256), (size_t)n_cap * 4, stream, in, out, sizes, scale, B, T, C,
                           W, mode, max_size, n_cap, 0);
    }
    return sed_check_launch();
}
