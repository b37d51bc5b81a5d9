// Event-based (collar) and segment-based F1 counts on the device: what `log_sedeval_metrics` (src/evaluation_measures.py:52-152, 256-295)
// gets from sed_eval's EventBasedMetrics / SegmentBasedMetrics on the event lists of `decode_pred_batch_fast`
// (recipes/desed/finetune/train.py:370-398, 481-517).  DESIGN.md section 7c is the definition this file implements.
//
// sed_event_f1_counts: one wave per (clip, class), state in LDS.
//   1. The estimated events of the class in the clip, in onset order, into an LDS list: from the binarised frame matrix (maximal runs of
//      non-zero frames a..b, spanning ts[a]..ts[b + 1]) or from the wave's slice of a CSR event list.
//   2. Estimates of one class in one clip are disjoint, so their onsets AND offsets ascend: the estimates a reference event hits form one
//      index interval [lo, hi].  Each lane evaluates the hit predicate of its reference events (j = lane, lane + 64, ..) over all
//      estimates and keeps lo and hi; a non-hit between two hits sets status bit 1 -- the invariant the next stage rests on.
//   3. Maximum matching of that convex bipartite graph by Glover's rule: estimates in order, each to the unmatched reference event whose
//      interval holds it and ends first (a wave-wide minimum over (hi, j)).
//   4. Segment masks (64 segments of res_us) of reference and estimates, OR-reduced over the wave; the counts are popcounts.
//   5. Lane 0 adds n_ref, n_sys, tp, seg_tp, seg_fp, seg_fn to counts[class][6] with integer atomics: the sums do not depend on the order
//      of clips, batches or workgroups.
//
// Times are int64 microseconds.  Hit: |ron - eon| <= collar and (double)|roff - eoff| <= max((double)collar, p * (double)(roff - ron)),
// one IEEE product, the expression a host evaluates; ties are hits.
//
// Every loop is bounded by T, the clip's event count or F1_MAX_EST; there is no waiting between workgroups.
#include "metric_common.h"

#define F1_MAX_T 1024                    // frames per clip
#define F1_MAX_EST 512                   // estimated events of one class in one clip (1024 alternating frames make 512)
#define F1_MAX_EV 256                    // ground-truth events of one clip
#define F1_MAX_SEG 64                    // segments per clip: one bit each

// Bits of the segments on / res .. ceil(off / res) - 1 (none for a zero-length event); *over: a segment past the mask.
__device__ __forceinline__ unsigned long long f1_segments(long long on, long long off, long long res, bool* over) {
    if (on < 0) on = 0;
    if (off <= on) return 0ull;
    long long s0 = on / res, s1 = (off + res - 1) / res;
    if (s1 > F1_MAX_SEG) {
        *over = true;
        s1 = F1_MAX_SEG;
    }
    if (s0 >= s1) return 0ull;
    const unsigned long long upto = s1 >= 64 ? ~0ull : ((1ull << s1) - 1ull);
    return upto & ~((1ull << s0) - 1ull);
}

__device__ __forceinline__ bool f1_hit(long long ron, long long roff, long long eon, long long eoff, long long collar, double p) {
    const long long d_on = ron > eon ? ron - eon : eon - ron;
    const long long d_off = roff > eoff ? roff - eoff : eoff - roff;
    const double tol = fmax((double)collar, p * (double)(roff - ron));
    return d_on <= collar && (double)d_off <= tol;
}

__global__ __launch_bounds__(64) void event_f1_kernel(const uint8_t* __restrict__ active, const int* __restrict__ est_ptr,
                                                     const int* __restrict__ est_cls, const long long* __restrict__ est_on_g,
                                                     const long long* __restrict__ est_off_g, const int* __restrict__ clip_id,
                                                     const long long* __restrict__ ts_us, const int* __restrict__ gt_ptr,
                                                     const int* __restrict__ gt_cls, const long long* __restrict__ gt_on,
                                                     const long long* __restrict__ gt_off, long long collar, double p, long long res,
                                                     int T, int C, unsigned long long* __restrict__ counts, int* __restrict__ status) {
    __shared__ long long e_on[F1_MAX_EST], e_off[F1_MAX_EST];
    __shared__ long long r_on[F1_MAX_EV], r_off[F1_MAX_EV];
    __shared__ short r_lo[F1_MAX_EV], r_hi[F1_MAX_EV];
    __shared__ uint8_t r_used[F1_MAX_EV];
    __shared__ uint8_t act[F1_MAX_T + 2];                // act[t + 1] = frame t; act[0] = act[T + 1] = 0
    const int b = blockIdx.x / C, c = blockIdx.x - b * C;
    const int lane = threadIdx.x;
    int bits = 0;                                        // status bits of this lane

    // ---- reference events of the class (the clip's events are sorted by class)
    const int clip = clip_id[b];
    const int g0 = gt_ptr[clip];
    int ne = gt_ptr[clip + 1] - g0;
    if (ne > F1_MAX_EV) {                                // (the host that built the lists refuses such a clip; never index past LDS)
        bits |= 8;
        ne = F1_MAX_EV;
    }
    int below = 0, mine = 0;
    for (int i = lane; i < ne; i += 64) {
        const int k = gt_cls[g0 + i];
        below += k < c;
        mine += k == c;
    }
    const int c_lo = wave_sum_i(below), n_ref = wave_sum_i(mine);
    for (int j = lane; j < n_ref; j += 64) {
        r_on[j] = gt_on[g0 + c_lo + j];
        r_off[j] = gt_off[g0 + c_lo + j];
        r_used[j] = 0;
    }

    // ---- stage 1: the estimated events, in order
    int n_sys = 0;
    if (active != nullptr) {
        for (int t = lane; t < T + 2; t += 64)
            act[t] = (t >= 1 && t <= T) ? (uint8_t)(active[((size_t)b * T + (t - 1)) * C + c] != 0) : (uint8_t)0;
        __syncthreads();
        int n_end = 0;                                   // the k-th start and the k-th end are one run
        for (int t0 = 0; t0 < T; t0 += 64) {
            const int t = min(t0 + lane, T - 1);         // (lanes past T repeat the last frame and are masked out)
            const bool on = t0 + lane < T && act[t + 1];
            const bool starts = on && !act[t], ends = on && !act[t + 2];
            const unsigned long long sm = __ballot(starts), em = __ballot(ends);
            const unsigned long long before = (1ull << lane) - 1ull;
            if (starts) {
                const int i = n_sys + __popcll(sm & before);
                if (i < F1_MAX_EST) e_on[i] = ts_us[t];
            }
            if (ends) {
                const int i = n_end + __popcll(em & before);
                if (i < F1_MAX_EST) e_off[i] = ts_us[t + 1];
            }
            n_sys += __popcll(sm);
            n_end += __popcll(em);
        }
    } else {
        const int s0 = est_ptr[b], s1 = est_ptr[b + 1];
        int lower = 0, own = 0;
        for (int i = s0 + lane; i < s1; i += 64) {       // (bounded by the clip's event count)
            const int k = est_cls[i];
            lower += k < c;
            own += k == c;
        }
        const int first = s0 + wave_sum_i(lower);
        n_sys = wave_sum_i(own);
        for (int i = lane; i < min(n_sys, F1_MAX_EST); i += 64) {
            e_on[i] = est_on_g[first + i];
            e_off[i] = est_off_g[first + i];
        }
    }
    if (n_sys > F1_MAX_EST) {                            // (T <= 1024 cannot make more; the host refuses a longer list)
        bits |= 4;
        n_sys = F1_MAX_EST;
    }
    __syncthreads();

    // ---- stage 2: the interval of estimates each reference event hits
    for (int j = lane; j < n_ref; j += 64) {
        const long long ron = r_on[j], roff = r_off[j];
        int lo = 1, hi = 0, hits = 0;
        for (int i = 0; i < n_sys; ++i) {
            if (f1_hit(ron, roff, e_on[i], e_off[i], collar, p)) {
                if (hits == 0) lo = i;
                hi = i;
                ++hits;
            }
        }
        if (hits > 0 && hits != hi - lo + 1) bits |= 1;  // a non-hit between two hits
        r_lo[j] = (short)lo;
        r_hi[j] = (short)hi;
    }

    // ---- stage 3: Glover's rule.  A lane reads and writes the state of its own reference events only.
    int tp = 0;
    if (n_ref > 0) {
        for (int i = 0; i < n_sys; ++i) {
            int best = 0x7fffffff;
            for (int j = lane; j < n_ref; j += 64)
                if (!r_used[j] && r_lo[j] <= i && i <= r_hi[j]) best = min(best, ((int)r_hi[j] << 16) | j);
            const int win = wave_min_i(best);
            if (win != 0x7fffffff) {
                const int j = win & 0xffff;
                if ((j & 63) == lane) r_used[j] = 1;
                ++tp;
            }
        }
    }

    // ---- stage 4: segments
    bool over = false;
    unsigned long long ref_m = 0ull, sys_m = 0ull;
    for (int j = lane; j < n_ref; j += 64) ref_m |= f1_segments(r_on[j], r_off[j], res, &over);
    for (int i = lane; i < n_sys; i += 64) sys_m |= f1_segments(e_on[i], e_off[i], res, &over);
    if (over) bits |= 16;
    ref_m = wave_or_u64(ref_m);
    sys_m = wave_or_u64(sys_m);
    if (bits) atomicOr(status, bits);

    // ---- stage 5
    if (lane == 0) {
        unsigned long long* out = counts + (size_t)c * 6;
        const int v[6] = {n_ref, n_sys, tp, (int)__popcll(ref_m & sys_m), (int)__popcll(sys_m & ~ref_m), (int)__popcll(ref_m & ~sys_m)};
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (v[k]) atomicAdd(out + k, (unsigned long long)v[k]);
    }
}

extern "C" int sed_event_f1_counts(const uint8_t* active, const int* est_ptr, const int* est_cls, const int64_t* est_on,
                                   const int64_t* est_off, const int* clip_id, const int64_t* ts_us, const int* gt_ptr,
                                   const int* gt_cls, const int64_t* gt_on, const int64_t* gt_off, int64_t collar_us, double p,
                                   int64_t res_us, int B, int T, int C, int64_t* counts, int* status, hipStream_t stream) {
    (void)hipGetLastError();
    if (B < 0 || C <= 0 || collar_us < 0 || !(p >= 0.0) || res_us <= 0 || !gt_ptr || !counts || !status) return SED_ERR_ARG;
    if (active != nullptr) {
        if (T <= 0 || T > F1_MAX_T || !ts_us) return SED_ERR_ARG;
    } else if (!est_ptr) {
        return SED_ERR_ARG;
    }
    if (B == 0) return SED_OK;
    if (!clip_id || (int64_t)B * C > 0x7fffffff) return SED_ERR_ARG;
    hipLaunchKernelGGL(event_f1_kernel, dim3(B * C), dim3(64), 0, stream, active, est_ptr, est_cls, (const long long*)est_on,
                       (const long long*)est_off, clip_id, (const long long*)ts_us, gt_ptr, gt_cls, (const long long*)gt_on,
                       (const long long*)gt_off, (long long)collar_us, p, (long long)res_us, T, C, (unsigned long long*)counts, status);
    return sed_check_launch();
}
