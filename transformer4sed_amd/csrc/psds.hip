// Intersection-based PSDS on the device (Bilen et al. 2020, threshold-free over all score values as in Ebbers et al. 2022): the model
// selection metric of every validation loop of the reference (recipes/desed/finetune/train.py:229-253, 370-398: psds1 / psds2;
// recipes/audioset_strong/base/passt_cnn/train.py:174-186).  DESIGN.md section 7b is the definition this file implements.
//
// sed_psds_sweep: one wave per (clip, class).  The clip's frame scores of the class become order-preserving keys packed with the frame
// index and are sorted in LDS (descending score).  Lane 0 then inserts the frames in that order into a set of contiguous segments --
// boundary arrays: each end of a segment stores the other end, an insertion touches at most its two neighbours -- and keeps the running
// TP / FP / cross-trigger counts of the clip and class current: every segment that disappears is taken out of the counts and the merged
// one is put in, its overlaps recomputed from the clip's ground-truth intervals (held in LDS).  After each group of equal scores the
// change of the three counts is one threshold event.  The counts are NOT monotone in the threshold (a detection that passed the DTC can
// fail after growing), so nothing here assumes they are.
//
// Times are int64 microseconds; every criterion is `(double)intersection >= threshold * (double)length`, one IEEE product, the same
// expression a host evaluates.  The cross-trigger term is carried as one integer per event: sum over classes k of dCT_k * ct_q[k], with
// ct_q the caller's fixed-point image of 1 / (T_k (C - 1)) -- integer sums do not depend on the order of clips, batches or reductions.
//
// Every loop is bounded by T or by the clip's event count; there is no waiting between workgroups.
#include "metric_common.h"

#define PSDS_MAX_T 1024                  // frames per clip (the score tables have 156 .. 1000)
#define PSDS_MAX_EV 256                  // ground-truth events of one clip held in LDS
#define PSDS_MAX_CT_CLASSES 32           // classes with a cross-trigger threshold

struct PsdsState {
    int tp, fp;
    long long ct;
};

// [lo, hi): hull of a set of ground-truth events.  A detection outside it overlaps none of them, and every criterion with a zero
// intersection fails (thresholds and lengths are positive): the event loops are skipped for it.
struct PsdsHull {
    long long lo, hi;
};

__device__ __forceinline__ long long psds_overlap(long long s, long long e, long long on, long long off) {
    const long long lo = s > on ? s : on, hi = e < off ? e : off;
    return hi > lo ? hi - lo : 0;
}

// Puts the detection [s, e) into the counts (sign +1) or takes it out (sign -1).  ev_*: the clip's events, sorted by class; [c_lo, c_hi)
// those of the swept class.
__device__ void psds_apply(PsdsState& st, long long s, long long e, int sign, const long long* ev_on, const long long* ev_off,
                           const int* ev_cls, int ne, int c_lo, int c_hi, int c, long long* cov, double dtc, double gtc, double cttc,
                           const long long* __restrict__ ct_q, PsdsHull own, PsdsHull all) {
    const double len = (double)(e - s);
    long long inter = 0;
    if (s < own.hi && e > own.lo)
        for (int i = c_lo; i < c_hi; ++i) inter += psds_overlap(s, e, ev_on[i], ev_off[i]);
    if ((double)inter >= dtc * len) {
        for (int i = c_lo; i < c_hi; ++i) {
            const long long ov = psds_overlap(s, e, ev_on[i], ev_off[i]);
            if (ov == 0) continue;
            const double need = gtc * (double)(ev_off[i] - ev_on[i]);
            const long long before = cov[i - c_lo], after = before + sign * ov;
            cov[i - c_lo] = after;
            st.tp += (int)((double)after >= need) - (int)((double)before >= need);
        }
        return;
    }
    st.fp += sign;
    if (ct_q == nullptr || !(s < all.hi && e > all.lo)) return;
    int k = -1;
    long long sum = 0;
    for (int i = 0; i <= ne; ++i) {                      // (one pass past the end flushes the last class)
        const int ki = i < ne ? ev_cls[i] : -1;
        if (ki != k) {
            if (k >= 0 && k != c && (double)sum >= cttc * len) st.ct += sign * ct_q[k];
            k = ki;
            sum = 0;
        }
        if (i < ne) sum += psds_overlap(s, e, ev_on[i], ev_off[i]);
    }
}

__global__ __launch_bounds__(64) void psds_sweep_kernel(const float* __restrict__ scores, const int* __restrict__ clip_id,
                                                       const int* __restrict__ n_frames, const long long* __restrict__ ts_us, int t_pos,
                                                       const int* __restrict__ gt_ptr, const int* __restrict__ gt_cls,
                                                       const long long* __restrict__ gt_on, const long long* __restrict__ gt_off,
                                                       const long long* __restrict__ ct_q, double dtc, double gtc, double cttc, int T,
                                                       int C, float* __restrict__ ev_val, short* __restrict__ ev_dtp,
                                                       short* __restrict__ ev_dfp, long long* __restrict__ ev_dct,
                                                       int* __restrict__ status) {
    __shared__ unsigned long long srt[PSDS_MAX_T];       // (~key << 32) | frame: ascending order = descending score
    __shared__ long long ts[PSDS_MAX_T + 1];
    __shared__ short other[PSDS_MAX_T];                  // other end of the segment a frame is an end of; -1: frame not inserted yet
    __shared__ long long ev_on[PSDS_MAX_EV], ev_off[PSDS_MAX_EV], cov[PSDS_MAX_EV];
    __shared__ int ev_cls[PSDS_MAX_EV];
    const int b = blockIdx.x / C, c = blockIdx.x - b * C;
    const int lane = threadIdx.x;
    int tv = t_pos;                                      // frames that take part: leading frames of positive duration inside n_frames
    if (n_frames != nullptr) tv = min(tv, max(n_frames[b], 0));
    const int clip = clip_id[b];
    const int e0 = gt_ptr[clip];
    int ne = gt_ptr[clip + 1] - e0;
    if (ne > PSDS_MAX_EV) {                              // (the host that built the lists refuses such a clip; never index past LDS)
        if (lane == 0) atomicOr(status, 8);
        ne = PSDS_MAX_EV;
    }
    bool nan = false;
    for (int t = lane; t < tv; t += 64) {
        const float x = scores[((size_t)b * T + t) * C + c];
        nan |= x != x;
        srt[t] = ((unsigned long long)(~score_key(x)) << 32) | (unsigned)t;
        other[t] = -1;
    }
    for (int t = lane; t <= tv; t += 64) ts[t] = ts_us[t];
    for (int i = lane; i < ne; i += 64) {
        ev_on[i] = gt_on[e0 + i];
        ev_off[i] = gt_off[e0 + i];
        ev_cls[i] = gt_cls[e0 + i];
        cov[i] = 0;
    }
    if (nan) atomicOr(status, 2);
    __syncthreads();
    lds_sort(srt, tv);
    const size_t out = ((size_t)b * C + c) * T;
    __shared__ int n_groups;
    if (lane == 0) {
        int c_lo = 0;
        while (c_lo < ne && ev_cls[c_lo] < c) ++c_lo;
        int c_hi = c_lo;
        while (c_hi < ne && ev_cls[c_hi] == c) ++c_hi;
        PsdsState st = {0, 0, 0}, prev = {0, 0, 0};
        PsdsHull own = {0, 0}, all = {0, 0};             // (empty: lo == hi, nothing lies inside)
        for (int i = 0; i < ne; ++i) {
            if (i == 0 || ev_on[i] < all.lo) all.lo = ev_on[i];
            if (i == 0 || ev_off[i] > all.hi) all.hi = ev_off[i];
            if (i >= c_lo && i < c_hi) {
                if (i == c_lo || ev_on[i] < own.lo) own.lo = ev_on[i];
                if (i == c_lo || ev_off[i] > own.hi) own.hi = ev_off[i];
            }
        }
        int ng = 0;
        for (int j = 0; j < tv; ++j) {
            const unsigned long long cur = srt[j];
            const int t = (int)(cur & 0xffffffffu);
            int a = t, z = t;
            if (t > 0 && other[t - 1] >= 0) {
                a = other[t - 1];
                psds_apply(st, ts[a], ts[t], -1, ev_on, ev_off, ev_cls, ne, c_lo, c_hi, c, cov, dtc, gtc, cttc, ct_q, own, all);
            }
            if (t + 1 < tv && other[t + 1] >= 0) {
                z = other[t + 1];
                psds_apply(st, ts[t + 1], ts[z + 1], -1, ev_on, ev_off, ev_cls, ne, c_lo, c_hi, c, cov, dtc, gtc, cttc, ct_q, own, all);
            }
            other[t] = (short)t;
            other[a] = (short)z;
            other[z] = (short)a;
            psds_apply(st, ts[a], ts[z + 1], +1, ev_on, ev_off, ev_cls, ne, c_lo, c_hi, c, cov, dtc, gtc, cttc, ct_q, own, all);
            if (j + 1 == tv || (srt[j + 1] >> 32) != (cur >> 32)) {
                ev_val[out + ng] = scores[((size_t)b * T + t) * C + c];
                ev_dtp[out + ng] = (short)(st.tp - prev.tp);
                ev_dfp[out + ng] = (short)(st.fp - prev.fp);
                if (ev_dct != nullptr) ev_dct[out + ng] = st.ct - prev.ct;
                prev = st;
                ++ng;
            }
        }
        n_groups = ng;
    }
    __syncthreads();
    for (int j = n_groups + lane; j < T; j += 64) {      // unused slots: events that change nothing
        ev_val[out + j] = 0.f;
        ev_dtp[out + j] = 0;
        ev_dfp[out + j] = 0;
        if (ev_dct != nullptr) ev_dct[out + j] = 0;
    }
}

extern "C" int sed_psds_sweep(const float* scores, const int* clip_id, const int* n_frames, const int64_t* ts_us, int t_pos,
                              const int* gt_ptr, const int* gt_cls, const int64_t* gt_on, const int64_t* gt_off, const int64_t* ct_q,
                              double dtc, double gtc, double cttc, int B, int T, int C, float* ev_val, int16_t* ev_dtp, int16_t* ev_dfp,
                              int64_t* ev_dct, int* status, hipStream_t stream) {
    (void)hipGetLastError();
    if (B < 0 || T <= 0 || T > PSDS_MAX_T || C <= 0 || t_pos < 0 || t_pos > T || !ts_us || !gt_ptr || !status) return SED_ERR_ARG;
    if (!(dtc > 0.0 && dtc <= 1.0) || !(gtc > 0.0 && gtc <= 1.0)) return SED_ERR_ARG;
    if ((ct_q != nullptr) != (ev_dct != nullptr)) return SED_ERR_ARG;
    if (ct_q != nullptr && (C > PSDS_MAX_CT_CLASSES || !(cttc > 0.0 && cttc <= 1.0))) return SED_ERR_ARG;
    if (B == 0) return SED_OK;
    if (!scores || !clip_id || !ev_val || !ev_dtp || !ev_dfp || (int64_t)B * C > 0x7fffffff) return SED_ERR_ARG;
    hipLaunchKernelGGL(psds_sweep_kernel, dim3(B * C), dim3(64), 0, stream, scores, clip_id, n_frames, (const long long*)ts_us, t_pos,
                       gt_ptr, gt_cls, (const long long*)gt_on, (const long long*)gt_off, (const long long*)ct_q, dtc, gtc, cttc, T, C,
                       ev_val, (short*)ev_dtp, (short*)ev_dfp, (long long*)ev_dct, status);
    return sed_check_launch();
}
