// A bank of median / max filters for the post-processing search (transformer4sed_amd/postproc_search.py):
//
//   sed_median_filter_bank     in [B, T, C] -> out [W, B, T, C], out[w] = the filter of frontend.hip (sed_median_filter_k, same three modes)
//                              with the window row sizes[w, :], for W candidate rows at once
//
// out[w] holds the bits sed_median_filter_k(in, ., sizes[w], scale, B, T, C, mode, max_size) writes, because the same ELEMENT of the input
// is selected -- the result is always an input value (x scale: one fp32 multiply, done once while staging), never an arithmetic combination.
// Which selection that kernel uses is a function of (mode, T, max_size) alone, and this one follows it:
//   * mode 0 / 1, max_size >= 24, T >= 256, T + max_size + 1 <= 2048: order statistics on GLOBAL ranks (ties by position).  A (clip,
//     class) column is staged ONCE with the padding of the class's widest window (K - 1 entries, K/2 in front), and its n = T + K - 1
//     entries are ranked ONCE -- the n^2 / 256 compares per thread that bound the clip kernel, which it repeats on every call.  Every
//     window k <= K of the W rows is a contiguous run of that one padded column, starting (K/2 - k/2) entries later than the widest; the
//     order of a run's entries by (value, position) is the same in the shared column as in the column padded for k alone, so the
//     (k/2 + 1)-th set bit of the run's bitmap over ranks is the element the clip kernel returns.
//   * otherwise: the clip kernel's rank search (or fmaxf) in window order, over the same staged column.
// Work split: one workgroup per (clip, class), every window row inside it.  The shared arrays hold one column whatever W is, and the
// bitmaps belong to threads, not to windows (256 threads x ceil(n / 32) words): at T = 1000, max_size = 1024 that is 20 KB + 65 KB = 85 KB
// of the CU's 160 KB, so all W <= 64 rows are served from one residency and W needs no grouping; at the search's own sizes (windows up
// to 179 frames) it is 50 KB and three workgroups share a CU.  The 256 threads are dealt to (row, chunk of frames) pairs, 256 / W chunks
// per row, so a thread builds its bitmap once per chunk of about T W / 256 outputs.
//
// Every loop is bounded by T, W or max_size; no workgroup waits for another; there is no atomic; every output element is written by one
// thread: the same bits in every run.  A (row, class) whose window is below 1, above max_size or (modes 1 / 2) above T comes out as NaN:
// loud in the data, never a read past LDS.
#include "common.h"

#define FB_MAX_W 64
#define FB_RANK_MIN 24                   // frontend.hip's dispatch: the rank kernel from this bound on ...
#define FB_RANK_MIN_T 256                // ... and this many frames ...
#define FB_RANK_MAXN 2048                // ... while T + max_size + 1 fits (MEDR_MAXN)
#define FB_SEARCH_MAXN 16384             // padded column of the rank-search form: 64 KB

template <bool RANKS>
__global__ __launch_bounds__(256) void filter_bank_kernel(const float* __restrict__ in, float* __restrict__ out, const int* __restrict__ sizes,
                                                          const float* __restrict__ scale, int B, int T, int C, int W, int mode, int max_size,
                                                          int n_cap, int Wb) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fb_lds[];
    __shared__ int ks[FB_MAX_W];                                                     // effective window of row w, 0 = out of range
    float* vp = reinterpret_cast<float*>(fb_lds);                                    // [n_cap] padded column
    float* byrank = vp + n_cap;                                                       // [n_cap] value of rank r          (RANKS only)
    unsigned short* rk = reinterpret_cast<unsigned short*>(byrank + n_cap);          // [n_cap] rank of padded entry p   (n_cap % 4 == 0)
    unsigned* bm = reinterpret_cast<unsigned*>(rk + n_cap);                          // [256][Wb] per-thread window bitmaps (Wb odd)
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
        int s = p - LO;
        if (mode == 0) s = s < 0 ? 0 : (s >= T ? T - 1 : s);
        else s = s < 0 ? -s - 1 : (s >= T ? 2 * T - s - 1 : s);         // (single reflection: K <= T in these modes)
        const float v = in[((size_t)b * T + s) * C + c];
        vp[p] = scale != nullptr ? v * sc : v;
    }
    __syncthreads();
    if (!RANKS) {
        for (int idx = tid; idx < W * T; idx += 256) {                  // frames fastest: a wave reads consecutive LDS words
            const int w = idx / T, i = idx - w * T, k = ks[w];
            if (k == 0) continue;
            const float* win = vp + i + LO - k / 2;
            const int rank = k / 2;
            float res = 0.f;
            if (mode == 2) {
                float m = -INFINITY;
                for (int j = 0; j < k; ++j) m = fmaxf(m, win[j]);
                res = m;
            } else {
                for (int a = 0; a < k; ++a) {
                    const float va = win[a];
                    int lt = 0, le = 0;
                    for (int j = 0; j < k; ++j) {
                        const float vj = win[j];
                        lt += vj < va;
                        le += vj <= va;
                    }
                    if (lt <= rank && rank < le) { res = va; break; }
                }
            }
            out[(((size_t)w * B + b) * T + i) * C + c] = res;
        }
        return;
    }
    for (int p = tid; p < n; p += 256) {
        const float v = vp[p];
        int r = 0;
        for (int q = 0; q < n; ++q) {
            const float u = vp[q];
            r += (u < v) || (u == v && q < p);
        }
        rk[p] = (unsigned short)r;
        byrank[r] = v;
    }
    __syncthreads();
    const int nch = 256 / W, w = tid / nch, ch = tid - w * nch;        // (row, chunk) of this thread
    if (w >= W) return;
    const int k = ks[w];
    const int chunk = (T + nch - 1) / nch, i0 = ch * chunk;
    if (k == 0 || i0 >= T) return;
    const int rank = k / 2;
    const unsigned short* wr = rk + LO - k / 2;                         // window of output i: wr[i .. i + k)
    unsigned* my = bm + tid * Wb;
    for (int x = 0; x < Wb; ++x) my[x] = 0u;
    for (int j = 0; j < k; ++j) { const int r = wr[i0 + j]; my[r >> 5] |= 1u << (r & 31); }
    const int i1 = i0 + chunk < T ? i0 + chunk : T;
    float* o = out + ((size_t)w * B + b) * T * C + c;
    for (int i = i0; i < i1; ++i) {
        int cum = 0, x = 0;
        unsigned word = my[0];
        int cnt = __popc(word);
        while (x + 1 < Wb && cum + cnt <= rank) { cum += cnt; word = my[++x]; cnt = __popc(word); }
        for (int q = rank - cum; q > 0; --q) word &= word - 1;         // drop the lower set bits: the wanted one becomes the lowest
        o[(size_t)i * C] = word != 0u ? byrank[32 * x + __ffs(word) - 1] : __builtin_nanf("");   // (no bit left: unordered input, NaN)
        if (i + 1 < i1) {
            const int r0 = wr[i], r1 = wr[i + k];
            my[r0 >> 5] &= ~(1u << (r0 & 31));
            my[r1 >> 5] |= 1u << (r1 & 31);
        }
    }
}

extern "C" int sed_median_filter_bank(const float* in, float* out, const int* sizes, const float* scale, int B, int T, int C, int W, int mode,
                                      int max_size, hipStream_t stream) {
    (void)hipGetLastError();
    if (in == nullptr || out == nullptr || sizes == nullptr) return SED_ERR_ARG;
    if (mode < 0 || mode > 2 || B < 1 || T < 1 || T > 12288 || C < 1 || W < 1 || W > FB_MAX_W || max_size < 1) return SED_ERR_ARG;
    if ((int64_t)B * C > 0x7fffffffLL) return SED_ERR_ARG;
    int max_k = (mode == 0 && (max_size & 1) == 0) ? max_size + 1 : max_size;
    if (mode != 0 && max_k > T) max_k = T;                                 // longer windows come out as NaN and are not staged
    const bool ranks = mode != 2 && max_size >= FB_RANK_MIN && T >= FB_RANK_MIN_T && T + max_size + 1 <= FB_RANK_MAXN;
    const int n_cap = (T + max_k - 1 + 3) & ~3;
    if (!ranks && n_cap > FB_SEARCH_MAXN) return SED_ERR_ARG;
    if (ranks) {
        const int Wb = ((n_cap + 31) / 32) | 1;        // odd row stride: the 64 lanes' bitmap words fall into different banks
        const size_t lds = (size_t)n_cap * (4 + 4 + 2) + (size_t)256 * Wb * 4;
        static size_t attr = 0;
        if (lds > attr) { (void)hipFuncSetAttribute((const void*)filter_bank_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); attr = lds; }
        hipLaunchKernelGGL(filter_bank_kernel<true>, dim3((unsigned)(B * C)), dim3(256), lds, stream, in, out, sizes, scale, B, T, C, W, mode,
                           max_size, n_cap, Wb);
    } else {
        hipLaunchKernelGGL(filter_bank_kernel<false>, dim3((unsigned)(B * C)), dim3(256), (size_t)n_cap * 4, stream, in, out, sizes, scale, B, T, C,
                           W, mode, max_size, n_cap, 0);
    }
    return sed_check_launch();
}
