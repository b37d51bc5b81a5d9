"""Seeded cases and two host references for the intersection-based PSDS, in float64 and Python integers.

  * `brute`      as literal as the definition: per class and distinct score value threshold every clip, find the runs, intersect them with
                 the ground-truth events, count.  Times are the definition's: rounded to 6 decimals, integer microseconds.
  * `sweep_ref`  a plain restatement of the kernel's method (descending insertion into segments, one event per group of equal scores),
                 used where `brute` is too slow, and -- through `cpu_sweep` -- as the sweep of an `IntersectionPSDS` in tests without a GPU.

Both give, per class, the operating points in descending score order as (value, TP, FP, CT[k] for every class k): cumulative integers.
`psds_from_points` turns them into the PSD-ROC, the PSDS and the single-class values; `canonical` brings them into the form
`IntersectionPSDS.counts()` reports (points that change no count left out, cross-triggers folded with the accumulator's weights).
No test reads anything outside the repository."""
from collections import namedtuple

import numpy as np
import pandas as pd

Case = namedtuple("Case", "scores ts n_frames gt durations names classes")     # gt: [(clip, class, onset_s, offset_s)]
Args = namedtuple("Args", "dtc gtc cttc alpha_ct alpha_st")
PSDS1 = Args(0.7, 0.7, None, 0.0, 1.0)          # recipes/desed/finetune/train.py:229-253
PSDS2 = Args(0.1, 0.1, 0.3, 0.5, 1.0)
ARG_SETS = {"psds1": PSDS1, "psds2": PSDS2}
MAX_EFPR = 3600.0                               # the cases hold seconds of audio: one FP is already ~100 per hour


def us(x):
    return [int(v) for v in np.rint(np.round(np.asarray(x, dtype=np.float64), 6) * 1e6).astype(np.int64).reshape(-1)]


def _events(rng, n, c, dur):
    gt = []
    for clip in range(n):
        for k in range(c):
            for _ in range(rng.randint(0, 3)):
                on = round(float(rng.uniform(0, dur - 0.6)), 3)
                gt.append((clip, k, on, round(min(on + float(rng.uniform(0.2, 0.45 * dur)), dur), 3)))
    for k in range(c):                          # at least one event per class
        if not any(g[1] == k for g in gt):
            gt.append((int(rng.randint(n)), k, 1.0, round(0.5 * dur, 3)))
    return gt


def _case(scores, ts, n_frames, gt, dur):
    n, _, c = scores.shape
    return Case(np.ascontiguousarray(scores, dtype=np.float32), np.asarray(ts, dtype=np.float64), n_frames, gt, [dur] * n,
                [f"clip{i}" for i in range(n)], [f"class{k}" for k in range(c)])


def _inside(gt, ts, n, c):
    """[n, T, c] bool: the frame's centre lies in an event of the class."""
    mid = 0.5 * (ts[:-1] + ts[1:])
    m = np.zeros((n, len(mid), c), dtype=bool)
    for clip, k, on, off in gt:
        m[clip, :, k] |= (mid >= on) & (mid < off)
    return m


def case_a(seed=0):
    """4 clips, 24 frames, 3 classes; ts = min(0.4 t, 9.5); half the scores from {0, 1/8, .., 1} (ties within and across clips), half
    3-decimal values, high inside the events and low outside with 15 % of the frames flipped.  Planted, so that a wrong reading shows
    (at the lowest score value, 0, every clip is one detection of 9.5 s, and that LAST group of values carries the best operating point):
      * class 2 has one long event per clip, at least 70 % of the clip, and scores 0 on frames 3-9 (1.2 .. 4.0 s) only: above 0 the
        detection 4.0 .. 9.5 passes dtc = 0.7 but covers less than 70 % of the event, at 0 the whole clip passes and covers it;
      * clip 3, class 2: the event 1.0 .. 7.65 is 6.65 s = 0.7 * 9.5 s, an exact tie of the DTC at 0.7;
      * clip 3, class 1: one event 2.0 .. 2.95, 0.95 s = 0.1 * 9.5 s, an exact tie of the DTC at 0.1."""
    rng = np.random.RandomState(1000 + seed)
    n, t, c = 4, 24, 3
    ts = np.minimum(0.4 * np.arange(t + 1), 9.5)
    gt = [g for g in _events(rng, n, 2, 9.5) if (g[0], g[1]) != (3, 1)] + [(3, 1, 2.0, 2.95)]
    gt += [(clip, 2, round(float(rng.uniform(0.5, 1.5)), 3), round(float(rng.uniform(8.2, 9.0)), 3)) for clip in range(3)] + [(3, 2, 1.0, 7.65)]
    high = _inside(gt, ts, n, c) ^ (rng.rand(n, t, c) < 0.15)
    coarse = np.where(high, rng.randint(5, 9, size=(n, t, c)), rng.randint(0, 5, size=(n, t, c))) / 8.0
    fine = np.round(np.where(high, 0.6 + 0.4 * rng.rand(n, t, c), 0.5 * rng.rand(n, t, c)), 3)
    scores = np.where(rng.rand(n, t, c) < 0.5, coarse, fine)
    scores[:, :, 2] = np.maximum(scores[:, :, 2], 0.125)
    scores[:, 3:10, 2] = 0.0
    return _case(scores, ts, None, sorted(gt), 9.5)


def _smooth(rng, n, t, c, width):
    x = rng.rand(n, t + width - 1, c)
    k = np.ones(width) / width
    return np.stack([np.stack([np.convolve(x[i, :, j], k, mode="valid") for j in range(c)], axis=1) for i in range(n)])


def case_b(seed=0):
    """5 clips, 157 frames (the last one clipped at 10 s), 10 classes, ragged n_frames; smooth scores rounded to 2 decimals."""
    rng = np.random.RandomState(2000 + seed)
    n, t, c = 5, 157, 10
    scores = np.round(_smooth(rng, n, t, c, 9) * 1.6 - 0.3, 2).clip(0, 1)
    n_frames = [157, 120, 156, 97, 140]
    return _case(scores, np.minimum(0.064 * np.arange(t + 1), 10.0), n_frames, _events(rng, n, c, 10.0), 10.0)


def case_c(seed=0):
    """3 clips, 1000 frames, 10 classes: a median-filtered random walk quantised to 64 levels -- long equal-valued runs."""
    rng = np.random.RandomState(3000 + seed)
    n, t, c = 3, 1000, 10
    walk = np.cumsum(rng.randn(n, t + 6, c) * 0.05, axis=1)
    walk = (walk - walk.min(1, keepdims=True)) / (walk.max(1, keepdims=True) - walk.min(1, keepdims=True))
    med = np.median(np.stack([walk[:, i:i + t] for i in range(7)]), axis=0)
    return _case(np.floor(med * 63.999) / 64.0, 0.01 * np.arange(t + 1), None, _events(rng, n, c, 10.0), 10.0)


def case_d(seed=0):
    """3 clips, 64 frames, 40 classes: the many-class path (no cross-trigger threshold)."""
    rng = np.random.RandomState(4000 + seed)
    n, t, c = 3, 64, 40
    scores = np.round(_smooth(rng, n, t, c, 5), 2)
    return _case(scores, 0.15 * np.arange(t + 1), [64, 50, 64], _events(rng, n, c, 9.6), 9.6)


def frames(case):
    gt = pd.DataFrame([(case.names[g[0]] + ".wav", g[2], g[3], case.classes[g[1]]) for g in case.gt],
                      columns=["filename", "onset", "offset", "event_label"])
    dur = pd.DataFrame({"filename": [n + ".wav" for n in case.names], "duration": case.durations})
    return gt, dur


def score_tables(case):
    """The case as the dict of score DataFrames `batched_decode_preds` returns (needs n_frames None)."""
    assert case.n_frames is None
    return {n: pd.DataFrame(np.concatenate((case.ts[:-1, None], case.ts[1:, None], case.scores[i].astype(np.float64)), axis=1),
                            columns=["onset", "offset", *case.classes]) for i, n in enumerate(case.names)}


# ------------------------------------------------------------------------------------------------ shared integer pieces
def _overlap(s, e, on, off):
    return max(0, min(e, off) - max(s, on))


def _valid(case, clip):
    """Frames of the clip that take part: inside n_frames, of positive duration."""
    ts = us(case.ts)
    nf = len(ts) - 1 if case.n_frames is None else case.n_frames[clip]
    return [t for t in range(len(ts) - 1) if t < nf and ts[t + 1] > ts[t]]


def _clip_events(case, clip):
    return [(g[1], us(g[2])[0], us(g[3])[0]) for g in case.gt if g[0] == clip]


def _count(dets, events, c, n_class, a, strict=False):
    """Detections [(s, e)] of class c in one clip against its events [(class, on, off)] -> (TP, FP, CT[k])."""
    ge = (lambda x, y: x > y) if strict else (lambda x, y: x >= y)
    own = [(on, off) for k, on, off in events if k == c]
    passing, fp, ct = [], 0, [0] * n_class
    for s, e in dets:
        inter = sum(_overlap(s, e, on, off) for on, off in own)
        if ge(float(inter), a.dtc * float(e - s)):
            passing.append((s, e))
            continue
        fp += 1
        if a.cttc is not None:
            for k in range(n_class):
                if k != c and any(ev[0] == k for ev in events):
                    inter_k = sum(_overlap(s, e, on, off) for kk, on, off in events if kk == k)
                    if ge(float(inter_k), a.cttc * float(e - s)):
                        ct[k] += 1
    tp = sum(1 for on, off in own if ge(float(sum(_overlap(s, e, on, off) for s, e in passing)), a.gtc * float(off - on)))
    return tp, fp, ct


# ------------------------------------------------------------------------------------------------ (a) brute
def brute(case, a, clips=None, strict=False):
    """-> per class [(value, TP, FP, [CT_k])] over the distinct values of the class, descending."""
    n, _, n_class = case.scores.shape
    clips = range(n) if clips is None else clips
    ts = us(case.ts)
    out = []
    for c in range(n_class):
        values = sorted({float(case.scores[b, t, c]) for b in clips for t in _valid(case, b)}, reverse=True)
        pts = []
        for v in values:
            tp = fp = 0
            ct = [0] * n_class
            for b in clips:
                valid = _valid(case, b)
                on = [float(case.scores[b, t, c]) >= v for t in valid]
                dets, start = [], None
                for i, flag in enumerate(on + [False]):
                    if flag and start is None:
                        start = i
                    if not flag and start is not None:
                        dets.append((ts[valid[start]], ts[valid[i - 1] + 1]))
                        start = None
                r = _count(dets, _clip_events(case, b), c, n_class, a, strict)
                tp, fp, ct = tp + r[0], fp + r[1], [x + y for x, y in zip(ct, r[2])]
            pts.append((v, tp, fp, ct))
        out.append(pts)
    return out


# ------------------------------------------------------------------------------------------------ (b) sweep
def sweep_clip_class(col, valid, ts, events, c, n_class, a):
    """One clip, one class: scores `col` [T], participating frames `valid` (a prefix), boundaries `ts` (us) -> the threshold events
    [(value, dTP, dFP, [dCT_k])] in descending value order, one per distinct value.  Frames are inserted in descending score order into
    a set of segments; whatever segment an insertion changes is re-counted from the ground truth."""
    order = sorted(valid, key=lambda t: -float(col[t]))
    inside, segs = set(), set()                     # segs: (first, last) frame of every current segment
    prev = (0, 0, [0] * n_class)
    out = []
    for j, t in enumerate(order):
        first, last = t, t
        for s in list(segs):
            if s[1] == t - 1:
                first = s[0]
                segs.remove(s)
            elif s[0] == t + 1:
                last = s[1]
                segs.remove(s)
        inside.add(t)
        segs.add((first, last))
        if j + 1 == len(order) or float(col[order[j + 1]]) != float(col[t]):
            cur = _count([(ts[s[0]], ts[s[1] + 1]) for s in sorted(segs)], events, c, n_class, a)
            out.append((float(col[t]), cur[0] - prev[0], cur[1] - prev[1], [x - y for x, y in zip(cur[2], prev[2])]))
            prev = cur
    return out


def merge(events, merge_equal=True):
    """Threshold events of one class from all clips -> cumulative points in descending value order.  Events at one value form ONE point:
    their deltas are summed before the point exists.  merge_equal=False is the mistake the tie test is aimed at: a running sum that
    exposes the state between two equal-valued events."""
    events = sorted(events, key=lambda e: -e[0])
    pts, tp, fp, ct = [], 0, 0, None
    for i, (v, dtp, dfp, dct) in enumerate(events):
        tp, fp = tp + dtp, fp + dfp
        ct = list(dct) if ct is None else [x + y for x, y in zip(ct, dct)]
        if merge_equal and i + 1 < len(events) and events[i + 1][0] == v:
            continue
        pts.append((v, tp, fp, list(ct)))
    return pts


def sweep_ref(case, a, clips=None, merge_equal=True):
    n, _, n_class = case.scores.shape
    clips = range(n) if clips is None else clips
    ts = us(case.ts)
    out = []
    for c in range(n_class):
        ev = []
        for b in clips:
            ev += sweep_clip_class(case.scores[b, :, c], _valid(case, b), ts, _clip_events(case, b), c, n_class, a)
        out.append(merge(ev, merge_equal))
    return out


# ------------------------------------------------------------------------------------------------ points -> PSDS
def psds_from_points(case, a, points, max_efpr=MAX_EFPR, clips=None):
    """-> (psds, [single-class psds], (grid, effective tpr), [(efpr, tpr) per class]); eFPR per hour."""
    n, _, n_class = case.scores.shape
    clips = list(range(n) if clips is None else clips)
    t_data = sum(us([case.durations[b] for b in clips])) / 1e6
    n_ref = [sum(1 for g in case.gt if g[1] == k and g[0] in clips) for k in range(n_class)]
    t_k = [sum(us(g[3])[0] - us(g[2])[0] for g in case.gt if g[1] == k and g[0] in clips) / 1e6 for k in range(n_class)]
    rocs = []
    for c, pts in enumerate(points):
        raw = [(0.0, 0.0)]
        for _, tp, fp, ct in pts:
            cts = [ct[k] / t_k[k] for k in range(n_class) if k != c]
            raw.append(((fp / t_data + a.alpha_ct * (sum(cts) / len(cts) if cts else 0.0)) * 3600.0, tp / n_ref[c]))
        raw.sort(key=lambda p: (p[0], -p[1]))
        e, y, best = [], [], 0.0
        for ef, tpr in raw:
            best = max(best, tpr)
            e.append(ef)
            y.append(best)
        rocs.append((np.array(e), np.array(y)))

    def area(e, y):
        e = np.minimum(np.append(e, max_efpr), max_efpr)
        return float(np.sum(y * (e[1:] - e[:-1]))) / max_efpr

    def at(e, y, g):
        return y[np.searchsorted(e, g, side="right") - 1]

    grid = np.unique(np.concatenate([e[e <= max_efpr] for e, _ in rocs]))
    ys = np.stack([at(e, y, grid) for e, y in rocs])
    eff = np.maximum(ys.mean(0) - a.alpha_st * ys.std(0), 0.0)
    return area(grid, eff), [area(e, y) for e, y in rocs], (grid, eff), rocs


def canonical(points, ct_q=None):
    """Per class (value [n] f32, tp, fp, ct) with the points that repeat the counts before them left out -- `IntersectionPSDS.counts()`'s
    form.  ct = sum_k CT_k ct_q[k] in Python integers (0 without weights)."""
    out = []
    for pts in points:
        rows, last = [], (0, 0, 0)
        for v, tp, fp, ct in pts:
            w = sum(int(x) * int(q) for x, q in zip(ct, ct_q)) if ct_q is not None else 0
            if (tp, fp, w) != last:
                rows.append((np.float32(v), tp, fp, w))
                last = (tp, fp, w)
        out.append(rows)
    return out


def counts_as_rows(acc):
    return [[(np.float32(v), int(tp), int(fp), int(ct)) for v, tp, fp, ct in zip(p["value"], p["tp"], p["fp"], p["ct"])]
            for p in acc.counts()]


def has_decreasing_tp(points):
    return [any(b[1] < a[1] for a, b in zip(pts[:-1], pts[1:])) for pts in points]


# ------------------------------------------------------------------------------------------------ the class without a GPU
def cpu_sweep(acc):
    """A stand-in for `IntersectionPSDS._sweep` that runs `sweep_clip_class` on the accumulator's own ground-truth lists and fills the
    sweep's slots [n, C, T] (value f32, dTP int16, dFP int16, dCT int64 | None) on the host."""
    import torch

    def run(scores, clip_index, n_frames):
        n, t_all, n_class = scores.shape
        a = Args(acc.dtc, acc.gtc, acc.cttc, acc.alpha_ct, acc.alpha_st)
        x = scores.numpy()
        if np.isnan(x).any():
            raise ValueError("Detected NaN values in the scores")
        val = np.zeros((n, n_class, t_all), np.float32)
        dtp, dfp = np.zeros((n, n_class, t_all), np.int16), np.zeros((n, n_class, t_all), np.int16)
        dct = np.zeros((n, n_class, t_all), np.int64) if acc.ct_q is not None else None
        ts = [int(v) for v in acc.ts_us]
        for i, row in enumerate(clip_index):
            tv = acc.t_pos if n_frames is None else min(acc.t_pos, max(int(n_frames[i]), 0))
            ev = [tuple(int(v) for v in e) for e in acc.gt[acc.gt_ptr[row]:acc.gt_ptr[row + 1]]]
            for c in range(n_class):
                for j, (v, a_tp, a_fp, a_ct) in enumerate(sweep_clip_class(x[i, :, c], list(range(tv)), ts, ev, c, n_class, a)):
                    val[i, c, j], dtp[i, c, j], dfp[i, c, j] = v, a_tp, a_fp
                    if dct is not None:
                        dct[i, c, j] = sum(int(d) * int(q) for d, q in zip(a_ct, acc.ct_q))
        return (torch.from_numpy(val), torch.from_numpy(dtp), torch.from_numpy(dfp), torch.from_numpy(dct) if dct is not None else None)

    return run
