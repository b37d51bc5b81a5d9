// Order-statistic selection shared by the three median / max filters ("The shared selection core"):
//   median_filter_rank_kernel, filter_bank_kernel   (median_filter.hip; its median_filter_kernel restates the rank search in place)
//   lf_filter_kernel                                (longform.hip)
// Every filter returns an ELEMENT of its window (compare / select only, never an arithmetic combination), so two kernels that select
// through the functions below write the same bits.  Two forms:
//   * rank search in window order (medsel_rank_search): the first element a of the window with lt <= k/2 < le, lt / le = the window's
//     entries below / not above a.  O(k^2) per output; short windows.  An unordered window (NaN) satisfies no element: the answer is 0.
//   * global ranks (medsel_rank_column + medsel_slide): the padded column (padding entries kept as entries of their own, so every
//     window is a contiguous run of distinct entries) gets a total order once (rank = entries smaller, ties by position); a window is
//     then a bitmap over ranks, its median the (k/2 + 1)-th set bit, and sliding the window by one output clears one bit and sets one.
//     NaN entries compare false both ways and collide on a rank, so the bitmap of a window that holds one has fewer than k bits: the
//     walk stops at the thread's last word and a window with no bit left answers NaN.
#pragma once
#include "common.h"

#define MEDSEL_RANK_MIN 24               // global ranks from this window bound on ...
#define MEDSEL_RANK_MIN_T 256            // ... and this many frames ...
#define MEDSEL_MAXN 2048                 // ... while the padded column (T + max_size + 1 entries at most) fits

// which form a launch over windows up to max_size takes (0 = unknown): the clip filter and the bank follow the same predicate
static inline bool medsel_use_ranks(int mode, int T, int max_size) {
    return mode != 2 && max_size >= MEDSEL_RANK_MIN && T >= MEDSEL_RANK_MIN_T && T + max_size + 1 <= MEDSEL_MAXN;
}
// words per thread bitmap over n ranks; odd, so the 64 lanes' words fall into different banks
static inline int medsel_bitmap_stride(int n) { return ((n + 31) / 32) | 1; }
// LDS of the global-rank form: [vp | byrank | rk | bm] for a column of n_cap entries (n_cap % 4 == 0) and 256 thread bitmaps
static inline size_t medsel_rank_lds(int n_cap, int stride) { return (size_t)n_cap * (4 + 4 + 2) + (size_t)256 * stride * 4; }

struct MedselLds {
    float* vp;                           // [n_cap] padded column
    float* byrank;                       // [n_cap] value of rank r
    unsigned short* rk;                  // [n_cap] rank of padded entry p
    unsigned* bm;                        // [256][stride] per-thread window bitmaps
};
__device__ __forceinline__ MedselLds medsel_carve(unsigned char* lds, int n_cap) {
    MedselLds s;
    s.vp = reinterpret_cast<float*>(lds);
    s.byrank = s.vp + n_cap;
    s.rk = reinterpret_cast<unsigned short*>(s.byrank + n_cap);
    s.bm = reinterpret_cast<unsigned*>(s.rk + n_cap);
    return s;
}

// Source frame of position s of the extended sequence: replicate (mode 0) or edge-inclusive reflection (modes 1 / 2; single, k <= T).
template <typename I>
__device__ __forceinline__ I medsel_src(I s, I T, int mode) {
    return mode == 0 ? (s < 0 ? 0 : (s >= T ? T - 1 : s)) : (s < 0 ? -s - 1 : (s >= T ? 2 * T - s - 1 : s));
}

// The window is win(0 .. k): a load functor, so a caller may map indices on the fly or pass a staged run of LDS.
template <typename Load>
__device__ __forceinline__ float medsel_rank_search(Load win, int k) {
    const int rank = k / 2;
    float res = 0.f;
    for (int a = 0; a < k; ++a) {
        const float va = win(a);
        int lt = 0, le = 0;
        for (int j = 0; j < k; ++j) {
            const float vj = win(j);
            lt += vj < va;
            le += vj <= va;
        }
        if (lt <= rank && rank < le) { res = va; break; }
    }
    return res;
}
template <typename Load>
__device__ __forceinline__ float medsel_window_max(Load win, int k) {
    float m = -INFINITY;
    for (int j = 0; j < k; ++j) m = fmaxf(m, win(j));
    return m;
}

// vp[0, n) -> rk, byrank, by the whole workgroup of 256 threads (n^2 / 256 compares per thread); barriers are the caller's.
__device__ __forceinline__ void medsel_rank_column(const float* vp, int n, unsigned short* rk, float* byrank) {
    for (int p = threadIdx.x; p < n; p += 256) {
        const float v = vp[p];
        int r = 0;
        for (int q = 0; q < n; ++q) {
            const float u = vp[q];
            r += (u < v) || (u == v && q < p);
        }
        rk[p] = (unsigned short)r;
        byrank[r] = v;
    }
}

// One thread's outputs [i0, i1): the window of output i is the ranks wr[i .. i + k); o[i * C] receives its (k/2 + 1)-th smallest.
// `my` are the thread's `stride` bitmap words (32 * stride covers every rank of the column).
__device__ __forceinline__ void medsel_slide(const unsigned short* wr, const float* byrank, unsigned* my, int stride, int k, int i0, int i1,
                                             float* o, int C) {
    const int rank = k / 2;
    for (int x = 0; x < stride; ++x) my[x] = 0u;
    for (int j = 0; j < k; ++j) { const int r = wr[i0 + j]; my[r >> 5] |= 1u << (r & 31); }
    for (int i = i0; i < i1; ++i) {
        int cum = 0, x = 0;
        unsigned word = my[0];
        int cnt = __popc(word);
        // (x + 1 < stride && cum + cnt <= rank, with the bound carried in the limit: cum + cnt >= 0 > -1 ends the walk at the last word.  x
        // is the same in every lane still walking, so the limit is scalar work beside the load: profiles/median_filter_core_ab.txt)
        while (cum + cnt <= (x + 1 < stride ? rank : -1)) { cum += cnt; word = my[++x]; cnt = __popc(word); }
        for (int q = rank - cum; q > 0; --q) word &= word - 1;         // drop the lower set bits: the wanted one becomes the lowest
        o[(size_t)i * C] = word != 0u ? byrank[32 * x + __ffs(word) - 1] : __builtin_nanf("");   // (no bit left: unordered input, NaN)
        if (i + 1 < i1) {
            const int r0 = wr[i], r1 = wr[i + k];
            my[r0 >> 5] &= ~(1u << (r0 & 31));
            my[r1 >> 5] |= 1u << (r1 & 31);
        }
    }
}
