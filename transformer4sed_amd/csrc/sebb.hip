// Change-detection sound event bounding boxes for a bank of parameter rows (transformer4sed_amd/sebb.py):
//
//   sed_sebb_bank     in [B, T, C] -> out [K, B, T, C] frame scores, boxes [K, B, C, cap, 2], conf [K, B, C, cap], counts [K, B, C]
//
// The definition is exact in integers, so that this kernel and the host references agree bit for bit:
//   1. q[t] = rint(y[t] 2^24) (y = in x scale: one fp32 multiply, as the filter kernels do), P its exclusive prefix sum in int64
//   2. D[t] = sum q[t .. t+L) - sum q[t-L .. t) at the boundaries t = 0 .. T, frames outside the clip 0
//   3. onset candidates: D[t] > 0, > every D in [t-L, t), >= every D in (t, t+L]; offset candidates the mirror rule
//   4. the left-to-right walk off -> on -> off gives the candidate events [a_i, b_i)
//   5. one greedy merge pass with the two integer inequalities of (tau_q, rho_q)
//   6. c = float(double(S) / double(n << 24)) on the frames of a box, 0 elsewhere
// Work split: one workgroup of 256 threads per (clip, class).  The column is staged and its prefix sum made ONCE.  Steps 2-4 depend on L
// alone, so they run once per DISTINCT L of that class (L >= T is L = T exactly: both windows cover the clip) -- D and the candidate flags
// by all threads (a +-L window scan with early exit), the walk by one lane: it is a two-state machine over T + 1 bytes of LDS.  Step 5
// is serial per row and rows are independent, so every row of the bank with this L merges in a lane of its own, all at once; the lane
// writes its boxes and, walking the frames once, the T scores of its plane (exactly one store per frame: zeros up to the next box,
// c inside).  The LDS holds one column (P, D, flags, events: 24 KB) whatever K is.
//
// Every loop is bounded by T, L or K; no workgroup waits for another; there is no atomic; every output element is written by one
// thread with a plain store: the same bits in every run.  A row with more boxes than `cap` keeps its first `cap`, counts holds the true
// number, and status[0] is set (every writer stores the same 1); status[1] is set where a score was NaN or outside [0, 1] (it is then
// clamped: the host refuses such input first).  The launcher clears both words.
#include "common.h"

#define SEBB_MAX_K 64
#define SEBB_MAX_T 1024
#define SEBB_MAX_EV ((SEBB_MAX_T + 1) / 2 + 1)        // events are disjoint, at least one frame long and one frame apart

__global__ __launch_bounds__(256) void sebb_bank_kernel(const float* __restrict__ in, const float* __restrict__ scale,
                                                        const int* __restrict__ params, float* __restrict__ out, int* __restrict__ boxes,
                                                        float* __restrict__ conf, int* __restrict__ counts, int* __restrict__ status, int B,
                                                        int T, int C, int K, int cap) {
    __shared__ long long P[SEBB_MAX_T + 1];            // P[t] = sum q[0 .. t)
    __shared__ long long D[SEBB_MAX_T + 1];
    __shared__ long long part[2][256];
    __shared__ unsigned char flag[SEBB_MAX_T + 1];     // 1 onset candidate, 2 offset candidate
    __shared__ short ev_a[SEBB_MAX_EV], ev_b[SEBB_MAX_EV];
    __shared__ int Ls[SEBB_MAX_K], taus[SEBB_MAX_K], rhos[SEBB_MAX_K];
    __shared__ int n_ev;
    const int b = blockIdx.x / C, c = blockIdx.x - b * C, tid = threadIdx.x;
    if (tid < K) {
        const int* p = params + ((size_t)tid * C + c) * 3;
        const int L = p[0];
        Ls[tid] = L < 1 ? 1 : (L > T ? T : L);
        taus[tid] = p[1];
        rhos[tid] = p[2];
    }
    // ---- 1. quantise four consecutive frames per thread, prefix sum over the 256 partial sums
    const float sc = scale != nullptr ? scale[(size_t)b * C + c] : 1.0f;
    int q[4];
    long long mine = 0;
    bool bad = false;
    for (int j = 0; j < 4; ++j) {
        const int t = tid * 4 + j;
        q[j] = 0;
        if (t < T) {
            float y = in[((size_t)b * T + t) * C + c];
            if (scale != nullptr) y = y * sc;
            if (!(y >= 0.0f)) { y = 0.0f; bad = true; }
            if (y > 1.0f) { y = 1.0f; bad = true; }
            q[j] = (int)rintf(y * 16777216.0f);
        }
        mine += q[j];
    }
    if (bad) status[1] = 1;
    part[0][tid] = mine;
    __syncthreads();
    int cur = 0;
    for (int s = 1; s < 256; s <<= 1) {
        part[cur ^ 1][tid] = part[cur][tid] + (tid >= s ? part[cur][tid - s] : 0);
        cur ^= 1;
        __syncthreads();
    }
    long long run = part[cur][tid] - mine;
    for (int j = 0; j < 4; ++j) {
        const int t = tid * 4 + j;
        if (t <= T) P[t] = run;
        run += q[j];
    }
    if (tid == 255 && T == SEBB_MAX_T) P[T] = run;     // (the one boundary past the last thread's four frames)
    __syncthreads();
    for (int k0 = 0; k0 < K; ++k0) {
        const int L = Ls[k0];
        bool first = true;
        for (int j = 0; j < k0; ++j) first = first && Ls[j] != L;
        if (!first) continue;                          // (uniform over the workgroup: the rows with this L went with its first one)
        // ---- 2. step response
        for (int t = tid; t <= T; t += 256) {
            const int hi = t + L < T ? t + L : T, lo = t - L > 0 ? t - L : 0;
            D[t] = (P[hi] - P[t]) - (P[t] - P[lo]);
        }
        __syncthreads();
        // ---- 3. change points
        for (int t = tid; t <= T; t += 256) {
            const long long d = D[t];
            const int u0 = t - L > 0 ? t - L : 0, u1 = t + L < T ? t + L : T;
            unsigned char f = 0;
            if (d > 0) {
                bool ok = true;
                for (int u = t - 1; ok && u >= u0; --u) ok = d > D[u];
                for (int u = t + 1; ok && u <= u1; ++u) ok = d >= D[u];
                f = ok ? 1 : 0;
            } else if (d < 0) {
                bool ok = true;
                for (int u = t - 1; ok && u >= u0; --u) ok = d < D[u];
                for (int u = t + 1; ok && u <= u1; ++u) ok = d <= D[u];
                f = ok ? 2 : 0;
            }
            flag[t] = f;
        }
        __syncthreads();
        // ---- 4. candidate events
        if (tid == 0) {
            int n = 0, a = 0;
            bool on = false;
            for (int t = 0; t <= T; ++t) {
                const int f = flag[t];
                if (!on && f == 1) { on = true; a = t; }
                else if (on && f == 2) {
                    if (n < SEBB_MAX_EV) { ev_a[n] = (short)a; ev_b[n] = (short)t; ++n; }
                    on = false;
                }
            }
            if (on && n < SEBB_MAX_EV) { ev_a[n] = (short)a; ev_b[n] = (short)T; ++n; }
            n_ev = n;
        }
        __syncthreads();
        // ---- 5 / 6. merge and write, one lane per row with this L
        if (tid < K && Ls[tid] == L) {
            const int n = n_ev;
            const long long tau_q = taus[tid], rho_q = rhos[tid];
            const size_t row = ((size_t)tid * B + b) * C + c;
            float* o = out + ((size_t)tid * B + b) * T * C + c;
            int* bx = boxes + row * cap * 2;
            float* cf = conf + row * cap;
            int cnt = 0, done = 0;                     // boxes emitted, frames written
            int aE = 0, bE = 0;
            for (int i = 0; i <= n; ++i) {
                bool emit = i == n && n > 0;
                int aK = 0, bK = 0;
                if (i < n) {
                    aK = ev_a[i]; bK = ev_b[i];
                    if (i == 0) { aE = aK; bE = bK; continue; }
                    const long long SE = P[bE] - P[aE], SK = P[bK] - P[aK], SG = P[aK] - P[bE];
                    const long long nE = bE - aE, nK = bK - aK, nG = aK - bE;
                    const bool e_lo = SE * nK <= SK * nE;
                    const long long Sl = e_lo ? SE : SK, nl = e_lo ? nE : nK;
                    const bool merge = SG * nl + tau_q * nl * nG > Sl * nG && rho_q * SG * nl > 256 * Sl * nG;
                    if (merge) { bE = bK; continue; }
                    emit = true;
                }
                if (emit) {
                    const long long S = P[bE] - P[aE], nE = bE - aE;
                    const float cv = (float)((double)S / (double)(nE << 24));
                    if (cnt < cap) { bx[2 * cnt] = aE; bx[2 * cnt + 1] = bE; cf[cnt] = cv; }
                    ++cnt;
                    for (; done < aE; ++done) o[(size_t)done * C] = 0.0f;
                    for (; done < bE; ++done) o[(size_t)done * C] = cv;
                    aE = aK; bE = bK;
                }
            }
            for (; done < T; ++done) o[(size_t)done * C] = 0.0f;
            counts[row] = cnt;
            if (cnt > cap) status[0] = 1;
        }
        __syncthreads();                               // (D, flag and the events are rewritten for the next L)
    }
}

extern "C" int sed_sebb_bank(const float* in, const float* scale, const int* params, float* out, int* boxes, float* conf, int* counts,
                             int* status, int B, int T, int C, int K, int cap, hipStream_t stream) {
    (void)hipGetLastError();
    if (in == nullptr || params == nullptr || out == nullptr || boxes == nullptr || conf == nullptr || counts == nullptr || status == nullptr)
        return SED_ERR_ARG;
    if (B < 1 || T < 1 || T > SEBB_MAX_T || C < 1 || K < 1 || K > SEBB_MAX_K || cap < 1 || cap > SEBB_MAX_T) return SED_ERR_ARG;
    if ((int64_t)B * C > 0x7fffffffLL) return SED_ERR_ARG;
    if (hipMemsetAsync(status, 0, 2 * sizeof(int), stream) != hipSuccess) return sed_check_launch();
    hipLaunchKernelGGL(sebb_bank_kernel, dim3((unsigned)(B * C)), dim3(256), 0, stream, in, scale, params, out, boxes, conf, counts, status, B,
                       T, C, K, cap);
    return sed_check_launch();
}
