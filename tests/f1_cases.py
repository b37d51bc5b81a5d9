"""Seeded cases and two host references for the event-based and segment-based F1 counts, in Python integers.

  * `brute`       as literal as the definition: per clip and class the runs of the frame column, the full hit matrix, an augmenting-path
                  maximum matching, segment index sets.  `mode` and `matching` switch in the mistakes the cases are aimed at.
  * `greedy_ref`  a plain restatement of the kernel's method (interval of hits per reference event, Glover's rule, segment bit masks),
                  and -- through `cpu_counts` -- the counting of an `EventSegmentF1` in tests without a GPU.

Both give {"n_ref", "n_sys", "tp", "seg_tp", "seg_fp", "seg_fn"}: lists of C Python integers.  No test reads anything outside the
repository."""
from collections import namedtuple

import numpy as np
import pandas as pd

Case = namedtuple("Case", "active ts gt names classes")     # active [n, T, C] bool; gt: [(clip, class, onset_s, offset_s)]
COLLAR, P, RES = 0.2, 0.2, 1.0                              # src/evaluation_measures.py:137-152
NAMES = ("n_ref", "n_sys", "tp", "seg_tp", "seg_fp", "seg_fn")


def us(x):
    return [int(v) for v in np.rint(np.round(np.asarray(x, dtype=np.float64), 6) * 1e6).astype(np.int64).reshape(-1)]


def _case(active, ts, gt):
    n, _, c = active.shape
    return Case(np.ascontiguousarray(active, dtype=bool), np.asarray(ts, dtype=np.float64), sorted(gt), [f"clip{i}" for i in range(n)],
                [f"class{k}" for k in range(c)])


def frames(case):
    """The ground truth as the DataFrame a TSV holds; a clip without events is one row with a NaN label (DESED's validation TSV)."""
    rows = [(case.names[g[0]] + ".wav", g[2], g[3], case.classes[g[1]]) for g in case.gt]
    rows += [(n + ".wav", np.nan, np.nan, np.nan) for i, n in enumerate(case.names) if not any(g[0] == i for g in case.gt)]
    return pd.DataFrame(rows, columns=["filename", "onset", "offset", "event_label"])


# ------------------------------------------------------------------------------------------------ lists: {(clip, class): [(on_us, off_us)]}
def runs(col):
    """Maximal runs of true frames [(first, last)]."""
    out, start = [], None
    for t, v in enumerate(list(col) + [False]):
        if v and start is None:
            start = t
        if not v and start is not None:
            out.append((start, t - 1))
            start = None
    return out


def lists_of_case(case):
    n, _, n_class = case.active.shape
    ts = us(case.ts)
    refs = {(b, c): [] for b in range(n) for c in range(n_class)}
    for b, c, on, off in case.gt:
        refs[(b, c)].append((us(on)[0], us(off)[0]))
    ests = {(b, c): [(ts[a], ts[z + 1]) for a, z in runs(case.active[b, :, c])] for b in range(n) for c in range(n_class)}
    return refs, ests


def lists_of_frames(gt, pred, names, classes):
    """The same from two DataFrames(filename, onset, offset, event_label); NaN labels are clips without events."""
    clip = {n: i for i, n in enumerate(names)}
    cls = {c: i for i, c in enumerate(classes)}
    out = []
    for df in (gt, pred):
        d = {(b, c): [] for b in range(len(names)) for c in range(len(classes))}
        for f, on, off, label in zip(df["filename"], df["onset"], df["offset"], df["event_label"]):
            if not pd.isna(label):
                d[(clip[f.rsplit(".", 1)[0].rsplit("/", 1)[-1]], cls[label])].append((us(on)[0], us(off)[0]))
        out.append({k: sorted(v) for k, v in d.items()})
    return out


def events_frame(case):
    """The estimated events of a case as `decode_pred_batch_fast` lists them."""
    _, ests = lists_of_case(case)
    rows = [(case.classes[c], on / 1e6, off / 1e6, case.names[b] + ".wav") for (b, c), ev in sorted(ests.items()) for on, off in ev]
    return pd.DataFrame(rows, columns=["event_label", "onset", "offset", "filename"])


# ------------------------------------------------------------------------------------------------ (a) brute
def hit(ref, est, collar, p, mode="ok"):
    """mode: "ok" the definition; "no_offset" drops the offset condition; "strict" reads < for <=; "no_max" uses p * length alone."""
    (ron, roff), (eon, eoff) = ref, est
    le = (lambda a, b: a < b) if mode == "strict" else (lambda a, b: a <= b)
    if not le(abs(ron - eon), collar):
        return False
    if mode == "no_offset":
        return True
    tol = p * float(roff - ron) if mode == "no_max" else max(float(collar), p * float(roff - ron))
    return le(float(abs(roff - eoff)), tol)


def max_matching(adj, n_est):
    """Size of a maximum matching; adj[j]: the estimates reference j hits (augmenting paths)."""
    owner = [-1] * n_est

    def augment(j, seen):
        for i in adj[j]:
            if i not in seen:
                seen.add(i)
                if owner[i] < 0 or augment(owner[i], seen):
                    owner[i] = j
                    return True
        return False

    return sum(1 for j in range(len(adj)) if augment(j, set()))


def first_fit(adj, n_est):
    """The mistake: every reference event, in order, takes the first free estimate it hits."""
    taken, tp = set(), 0
    for row in adj:
        for i in row:
            if i not in taken:
                taken.add(i)
                tp += 1
                break
    return tp


def _segments(ev, res):
    out = set()
    for on, off in ev:
        if off > on:
            out |= set(range(on // res, -(-off // res)))
    return out


def pair_brute(refs, ests, collar=COLLAR, p=P, res=RES, mode="ok", matching="max"):
    """One clip, one class -> (n_ref, n_sys, tp, seg_tp, seg_fp, seg_fn)."""
    collar_us, res_us = us(collar)[0], us(res)[0]
    adj = [[i for i, e in enumerate(ests) if hit(r, e, collar_us, p, mode)] for r in refs]
    tp = (max_matching if matching == "max" else first_fit)(adj, len(ests))
    rs, es = _segments(refs, res_us), _segments(ests, res_us)
    return len(refs), len(ests), tp, len(rs & es), len(es - rs), len(rs - es)


def count_lists(refs, ests, n_class, pair=pair_brute, **kw):
    out = {k: [0] * n_class for k in NAMES}
    for (b, c) in sorted(refs):
        for k, v in zip(NAMES, pair(refs[(b, c)], ests[(b, c)], **kw)[:6]):
            out[k][c] += v
    return out


def brute(case, **kw):
    refs, ests = lists_of_case(case)
    return count_lists(refs, ests, case.active.shape[2], **kw)


def pair_tp(case, **kw):
    """{(clip, class): tp} -- for counting the pairs a mistake changes."""
    refs, ests = lists_of_case(case)
    return {k: pair_brute(refs[k], ests[k], **kw)[2] for k in refs}


# ------------------------------------------------------------------------------------------------ (b) the kernel's method
def pair_greedy(refs, ests, collar=COLLAR, p=P, res=RES):
    """-> (n_ref, n_sys, tp, seg_tp, seg_fp, seg_fn, status): status 1 if a non-hit lies between two hits."""
    collar_us, res_us = us(collar)[0], us(res)[0]
    lo, hi, status = [], [], 0
    for r in refs:
        hits = [i for i, e in enumerate(ests) if hit(r, e, collar_us, p)]
        lo.append(hits[0] if hits else 1)
        hi.append(hits[-1] if hits else 0)
        if hits and len(hits) != hits[-1] - hits[0] + 1:
            status |= 1
    used, tp = [False] * len(refs), 0
    for i in range(len(ests)):
        cand = [(hi[j], j) for j in range(len(refs)) if not used[j] and lo[j] <= i <= hi[j]]
        if cand:
            used[min(cand)[1]] = True
            tp += 1
    masks = []
    for ev in (refs, ests):
        m = 0
        for on, off in ev:
            if off > on:
                m |= ((1 << -(-off // res_us)) - 1) & ~((1 << (on // res_us)) - 1)
        masks.append(m)
    r, e = masks
    return len(refs), len(ests), tp, bin(r & e).count("1"), bin(e & ~r).count("1"), bin(r & ~e).count("1"), status


def greedy_ref(case):
    """-> (counts, status)."""
    refs, ests = lists_of_case(case)
    status = 0
    for k in refs:
        status |= pair_greedy(refs[k], ests[k])[6]
    return count_lists(refs, ests, case.active.shape[2], pair=pair_greedy), status


def cpu_counts(acc):
    """A stand-in for `EventSegmentF1._run`: `pair_greedy` on the accumulator's own ground-truth lists, added to its counts on the host."""
    import torch

    def run(rows, active=None, est=None):
        acc._state(torch.device("cpu"))
        n_class = acc.num_classes
        a = None if active is None else active.numpy()
        ts = None if acc.ts_us is None else [int(v) for v in acc.ts_us]
        for i, row in enumerate(rows):
            ev = [tuple(int(v) for v in e) for e in acc.gt[acc.gt_ptr[row]:acc.gt_ptr[row + 1]]]
            for c in range(n_class):
                refs = [(on, off) for k, on, off in ev if k == c]
                if a is not None:
                    ests = [(ts[s], ts[z + 1]) for s, z in runs(a[i, :, c] != 0)]
                else:
                    ptr, cls, on, off = est
                    ests = [(int(on[j]), int(off[j])) for j in range(ptr[i], ptr[i + 1]) if cls[j] == c]
                *cnt, status = pair_greedy(refs, ests, acc.collar_us / 1e6, acc.p, acc.res_us / 1e6)
                acc._counts[c] += torch.tensor(cnt, dtype=torch.int64)
                acc._status |= status

    return run


def counts_of(acc):
    return {k: [int(x) for x in v] for k, v in acc.counts().items()}


# ------------------------------------------------------------------------------------------------ case builders
GRID = 0.02            # 50 frames per second: collar = 10 frames, times on the grid are exact in microseconds


def _paint(active, b, c, first, last):
    t = active.shape[1]
    if last >= first and last >= 0 and first < t:
        active[b, max(first, 0):min(last, t - 1) + 1, c] = True


def _random_gt(rng, n, c, dur, per_class, short):
    gt = []
    for b in range(n):
        for k in range(c):
            for _ in range(rng.randint(0, per_class + 1)):
                length = float(rng.uniform(0.08, 0.5)) if short or rng.rand() < 0.4 else float(rng.uniform(0.5, 0.45 * dur))
                on = round(float(rng.uniform(0, max(dur - length, 0.1))), 3)
                gt.append((b, k, on, round(min(on + length, dur), 3)))
    return gt


def _active_near(rng, gt, n, t, c, ts, spurious):
    """Runs near the reference events: boundaries moved by up to one and a half collars (some exactly one collar), some events missed,
    some split, plus runs that belong to nothing."""
    active = np.zeros((n, t, c), dtype=bool)
    step = float(ts[1] - ts[0])
    shift = lambda: int(rng.choice([0, 0, 1, -1, 3, -3, int(round(0.2 / step)), -int(round(0.2 / step)), int(0.3 / step), -int(0.3 / step)]))
    for b, k, on, off in gt:
        if rng.rand() < 0.2:
            continue
        a, z = int(round(on / step)) + shift(), int(round(off / step)) - 1 + shift()
        _paint(active, b, k, a, max(a, z))
        if z - a > 4 and rng.rand() < 0.3:
            active[b, min(max((a + z) // 2, 0), t - 1), k] = False
    for _ in range(spurious):
        a = rng.randint(0, t)
        _paint(active, rng.randint(n), rng.randint(c), a, a + rng.randint(0, 12))
    return active


def case_random(seed=0, n=4, t=157, c=3, step=0.064, dur=10.0):
    """Random clips on the recipe's 64 ms grid with the last frame clipped at 10 s; the last clip and the last class stay empty when
    there are enough of them (a clip without events, a class without events)."""
    rng = np.random.RandomState(100 + seed)
    ts = np.minimum(step * np.arange(t + 1), dur)
    gt = [g for g in _random_gt(rng, n, c, min(dur, step * t), 2, False) if not (n > 2 and g[0] == n - 1) and not (c > 2 and g[1] == c - 1)]
    return _case(_active_near(rng, gt, n, t, c, ts, spurious=n * c // 2 + 1), ts, gt)


def case_dense(seed=0, n=3, t=250, c=2):
    """Short, overlapping reference events of one class (up to 8) on a 16 ms grid and many short estimates: where first-fit matching
    goes wrong."""
    rng = np.random.RandomState(200 + seed)
    ts = 0.016 * np.arange(t + 1)
    gt = _random_gt(rng, n, c, 0.016 * t, 8, True)
    active = _active_near(rng, gt, n, t, c, ts, spurious=6)
    active[:, rng.randint(0, t, size=t // 6), :] = False           # more, shorter runs
    return _case(active, ts, gt)


def case_first_fit(n=12):
    """Planted, one pair per clip, shifted by half a second from clip to clip.  Reference A = 0.99 .. 1.34 and B = 1.02 .. 1.15 (sorted by
    onset: A first); estimates e0 = frames 50-57 = 1.00 .. 1.16 and e1 = frames 59-69 = 1.18 .. 1.40.
      A-e0: |d on| 0.01, |d off| 0.18 <= max(0.2, 0.07): hit.    A-e1: 0.19, 0.06: hit.
      B-e0: 0.02, 0.01: hit.                                      B-e1: 0.16, |1.15 - 1.40| = 0.25 > 0.2: no hit.
    First-fit gives A e0 and leaves B empty: tp 1.  The maximum is A-e1, B-e0: tp 2."""
    t = 50 * (n // 2 + 2)
    active = np.zeros((n, t, 1), dtype=bool)
    gt = []
    for b in range(n):
        s = b // 2
        _paint(active, b, 0, 50 + 25 * s, 57 + 25 * s)
        _paint(active, b, 0, 59 + 25 * s, 69 + 25 * s)
        gt += [(b, 0, round(0.99 + 0.5 * s, 3), round(1.34 + 0.5 * s, 3)), (b, 0, round(1.02 + 0.5 * s, 3), round(1.15 + 0.5 * s, 3))]
    return _case(active, GRID * np.arange(t + 1), gt)


TIE_KINDS = ("onset == collar", "offset == 0.2 length", "offset == collar, short event", "offset inside the collar, short event",
             "offset far off")


def case_ties(n=12):
    """Planted, class k of every clip holds kind k (TIE_KINDS), one reference event and one estimate; the clip index moves the pair along
    the grid and alternates the side of the deviation.  With s = +-1:
      0  ref 2.0 .. 4.0, est onset 2.0 + 0.2 s, same offset                  -> |d on| = collar exactly: hit, no hit with <
      1  ref 2.0 .. 4.0, est offset 4.0 + 0.4 s                              -> |d off| = 0.2 * 2.0 exactly: hit, no hit with <
      2  ref 2.0 .. 2.5, est offset 2.5 + 0.2 s                              -> |d off| = collar > 0.2 * 0.5: hit; no hit with < or without max
      3  ref 2.0 .. 2.5, est offset 2.5 + 0.14 s                             -> inside the collar, outside 0.1: hit; no hit without max
      4  ref 2.0 .. 4.0, est offset 4.0 + 1.0 s                              -> no hit; a hit without the offset condition."""
    t = 500
    active = np.zeros((n, t, len(TIE_KINDS)), dtype=bool)
    gt = []
    for b in range(n):
        s, base = (1 if b % 2 == 0 else -1), 100 + 10 * (b // 2)            # frame of the reference onset (2.0 s + 0.2 s per pair of clips)
        for k in range(len(TIE_KINDS)):
            length = 25 if k in (2, 3) else 100
            on, off = base, base + length                                    # frames: the event spans ts[on] .. ts[off]
            gt.append((b, k, round(GRID * on, 3), round(GRID * off, 3)))
            d_on = 10 * s if k == 0 else 0
            d_off = {0: 0, 1: 20 * s, 2: 10 * s, 3: 7 * s, 4: 50 * s}[k]
            _paint(active, b, k, on + d_on, off + d_off - 1)
    return _case(active, GRID * np.arange(t + 1), gt)


def case_trailing(seed=0):
    """Frames past the audio's end have zero duration (ts clipped at 10 s): runs there are zero-length events at 10.0 s, listed by
    `Encoder.decode_strong` and counted as estimates.  A short reference event that ends at 10.0 is hit by one of them."""
    rng = np.random.RandomState(300 + seed)
    n, t, c = 3, 164, 2
    ts = np.minimum(0.064 * np.arange(t + 1), 10.0)                         # frames 157 .. 163 have zero duration
    active = np.zeros((n, t, c), dtype=bool)
    active[:, 150:164:2, :] = True                                         # 150, 152, .., 162: three of them zero-length
    active[1, 140:160, 1] = True
    active[2, :, 0] = rng.rand(t) < 0.5
    gt = [(0, 0, 9.85, 10.0), (0, 1, 9.5, 10.0), (1, 0, 9.6, 9.7), (1, 1, 8.9, 10.0), (2, 0, 1.0, 3.0), (2, 0, 9.9, 10.0)]
    return _case(active, ts, gt)


def case_shape(n, t, c, seed=0, step=GRID, per_class=2, fill=None):
    """A random case of a given shape; fill = "on" / "off" / "alternate" sets every frame instead."""
    rng = np.random.RandomState(400 + seed + 7 * n + 13 * t + 17 * c)
    ts = step * np.arange(t + 1)
    dur = step * t
    gt = [(b, k, round(float(on), 6), round(float(min(on + rng.uniform(0.3, 1.0) * dur, dur)), 6))
          for b in range(n) for k in range(c) for _ in range(rng.randint(0, per_class + 1)) for on in [rng.uniform(0, 0.6) * dur]]
    gt = [g for g in gt if us(g[3])[0] > us(g[2])[0]]
    if fill is None:
        active = _active_near(rng, gt, n, t, c, ts, spurious=n * c // 2 + 1)
    else:
        active = np.zeros((n, t, c), dtype=bool)
        active[:, ::2 if fill == "alternate" else 1, :] = fill != "off"
    return _case(active, ts, gt)


def case_many_refs(seed=0):
    """One clip with 256 reference events, 130 of them in class 0 (a lane holds up to three of its class), short and overlapping, on
    1000 frames of 10 ms; many short estimates."""
    rng = np.random.RandomState(500 + seed)
    t, c = 1000, 4
    ts = 0.01 * np.arange(t + 1)
    cls = [0] * 130 + [1 + i % 3 for i in range(126)]
    gt = []
    for k in cls:
        on = round(float(rng.uniform(0, 9.5)), 2)
        gt.append((0, k, on, round(on + float(rng.uniform(0.05, 0.45)), 2)))
    active = _active_near(rng, gt, 1, t, c, ts, spurious=10)
    active[:, rng.randint(0, t, size=150), :] = False
    return _case(active, ts, gt)


def cpu_cases():
    """The set the CPU tests count on (name, case)."""
    out = [(f"random{s}", case_random(s)) for s in range(6)] + [(f"dense{s}", case_dense(s)) for s in range(12)]
    return out + [("first_fit", case_first_fit()), ("ties", case_ties()), ("trailing", case_trailing())]
