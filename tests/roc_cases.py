"""Cases and host references of the ROC-area tests (tests/test_roc_cpu.py, tests/test_gpu_roc.py).

Two readings of the ROC integers, written apart from each other and from the product: `ref_points` walks the ROC points and finishes
in `fractions.Fraction`, `ref_items` sums per item with numpy integers.  `pool_ref` / `overlap_add_ref` restate the segment pooling."""
from fractions import Fraction

import numpy as np

INTS = ("P", "Nn", "auc2", "area2", "fp_a", "tp_a", "fp_b", "tp_b")


def score_key(scores):
    """csrc/metric_common.h: float32 -> uint32 whose unsigned order is the float order, -0.0 and +0.0 one value."""
    u = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = np.where(u == 0x80000000, 0, u)
    return np.where(u & 0x80000000, ~u & 0xffffffff, u | 0x80000000).astype(np.int64)


def _cut_rank(max_fpr, Nn):
    return int(np.floor(np.float64(max_fpr) * np.float64(Nn)))          # one IEEE-double multiply, then a floor


def ref_points(scores, labels, max_fpr):
    """One class, from the ROC points -> the eight integers (python ints)."""
    key, y = score_key(scores), np.asarray(labels).astype(bool)
    P, Nn = int(y.sum()), int((~y).sum())
    pts = [(0, 0)]
    for k in sorted(set(key.tolist()), reverse=True):
        pts.append((int((~y & (key >= k)).sum()), int((y & (key >= k)).sum())))
    m = len(pts) - 1
    trap = lambda j: (pts[j][0] - pts[j - 1][0]) * (pts[j][1] + pts[j - 1][1])
    F = _cut_rank(max_fpr, Nn)
    a = max(j for j in range(m + 1) if pts[j][0] <= F)
    b = min(a + 1, m)
    return (P, Nn, sum(trap(j) for j in range(1, m + 1)), sum(trap(j) for j in range(1, a + 1)), *pts[a], *pts[b])


def ref_items(scores, labels, max_fpr):
    """One class, from the per-item sums (numpy integers) -> the eight integers."""
    key, y = score_key(scores), np.asarray(labels).astype(bool)
    pos, neg = np.sort(key[y]), np.sort(key[~y])
    P, Nn = pos.size, neg.size
    lt = lambda arr, k: np.searchsorted(arr, k, side="left")            # items of arr with key < k
    le = lambda arr, k: np.searchsorted(arr, k, side="right")           # ... <= k
    auc2 = int((2 * lt(neg, pos) + (le(neg, pos) - lt(neg, pos))).sum())
    F = _cut_rank(max_fpr, Nn)
    distinct = np.unique(key)
    within = distinct[Nn - lt(neg, distinct) <= F]                      # keys whose ROC point has fp <= F
    ge = lambda arr, k: int(arr.size - lt(arr, k))
    if within.size == 0:
        area2, fp_a, tp_a, below = 0, 0, 0, distinct
    else:
        k_a = within.min()
        side = neg[neg >= k_a]
        area2 = int((2 * (P - le(pos, side)) + (le(pos, side) - lt(pos, side))).sum())
        fp_a, tp_a, below = ge(neg, k_a), ge(pos, k_a), distinct[distinct < k_a]
    fp_b, tp_b = (ge(neg, below.max()), ge(pos, below.max())) if below.size else (fp_a, tp_a)
    return (int(P), int(Nn), auc2, area2, fp_a, tp_a, fp_b, tp_b)


def finish_fraction(ints, max_fpr=None, normalize="mcclish"):
    """Section 7g's finish in exact arithmetic -> (AUROC, partial area) as Fractions, None for a class without both kinds."""
    P, Nn, auc2, area2, fp_a, tp_a, fp_b, tp_b = (int(v) for v in ints)
    if P == 0 or Nn == 0:
        return None, None
    auroc = Fraction(auc2, 2 * P * Nn)
    if max_fpr is None:
        return auroc, auroc
    x = Fraction(float(np.float64(max_fpr) * np.float64(Nn)))
    tp_x = tp_a + (Fraction(tp_b - tp_a) * (x - fp_a) / (fp_b - fp_a) if fp_b != fp_a else 0)
    raw = (Fraction(area2, 2) + (x - fp_a) * (tp_a + tp_x) / 2) / (P * Nn)
    f = Fraction(float(max_fpr))
    if normalize == "max_fpr":
        return auroc, raw / f
    return auroc, (raw if f == 1 else (1 + (raw - f * f / 2) / (f - f * f / 2)) / 2)


def auc2_strict(scores, labels):
    """auc2 if ties were read as a strict order (earlier items first): what a sort without tie groups would give."""
    key, y = score_key(scores), np.asarray(labels).astype(bool)
    order = np.argsort(-key, kind="stable")
    neg_after = np.cumsum((~y[order])[::-1])[::-1] - (~y[order])
    return int(2 * neg_after[y[order]].sum())


# ---------------------------------------------------------------------------------------------------- cases
def case(name, scores, labels, max_fpr, nan_classes=()):
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    labels = np.ascontiguousarray(labels, dtype=np.uint8)
    assert scores.shape == labels.shape and scores.ndim == 2
    return dict(name=name, scores=scores, labels=labels, max_fpr=float(max_fpr), nan_classes=frozenset(nan_classes))


def random_case(N, levels, max_fpr, seed, C=3):
    """[C][N]: `levels` score levels (None: continuous), labels correlated with the score; class 1 carries +-0.0."""
    rng = np.random.RandomState(seed)
    s = rng.rand(C, N)
    if levels:
        s = np.floor(s * levels) / levels
    s = s.astype(np.float32)
    y = (rng.rand(C, N) < 0.15 + 0.5 * s).astype(np.uint8)
    if N >= 4:
        s[1, :: max(N // 8, 2)] = 0.0
        s[1, 1:: max(N // 8, 2)] = -0.0
        for c in range(C):                                              # both kinds present
            y[c, c % N], y[c, (c + 1) % N] = 1, 0
    nan = [c for c in range(C) if y[c].all() or not y[c].any()]
    return case(f"random N={N} levels={levels} fpr={max_fpr}", s, y, max_fpr, nan)


def designated_cases():
    """The cases the issue names, built so: see tests/test_roc_cpu.py::test_case_set_holds_every_designated_property."""
    out = []
    out.append(case("tie between a positive and a negative", [[0.5, 0.5, 0.2, 0.9]], [[1, 0, 0, 1]], 1.0))
    # 20 negatives, max_fpr 0.25: x = 5.  Negatives: 3 at 0.9, 6 tied at 0.5 (fp 3 -> 9: the cut lies inside the group), 11 below.
    neg = [0.9] * 3 + [0.5] * 6 + list(np.linspace(0.05, 0.4, 11))
    pos = [0.95, 0.9, 0.5, 0.5, 0.3, 0.1]
    out.append(case("cut inside a tie group", [neg + pos], [[0] * 20 + [1] * 6], 0.25))
    # 20 negatives, x = 5 exactly; the five best negatives are distinct, a positive shares the fifth's score: the point (5, tp) exists.
    neg = [0.9, 0.85, 0.8, 0.75, 0.7] + list(np.linspace(0.05, 0.6, 15))
    pos = [0.95, 0.7, 0.65, 0.2]
    out.append(case("cut on a point", [neg + pos], [[0] * 20 + [1] * 4], 0.25))
    out.append(case("max_fpr 1", random_case(50, 8, 1.0, 11)["scores"], random_case(50, 8, 1.0, 11)["labels"], 1.0))
    s = np.linspace(0, 1, 30)
    out.append(case("one positive / none / all", [s, s, s], [[0] * 12 + [1] + [0] * 17, [0] * 30, [1] * 30], 0.1, nan_classes=(1, 2)))
    out.append(case("signed zeros", [[0.0, -0.0, -0.0, 0.0, 0.3, -0.2, 0.0, -0.0]], [[1, 0, 1, 0, 1, 0, 0, 1]], 0.5))
    out.append(case("all tied", [[0.25] * 17], [[1, 0, 0, 1, 0, 1, 1, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0]], 0.1))
    return out


def cpu_cases():
    out = designated_cases()
    for i, (N, levels) in enumerate([(1, 8), (2, 8), (63, 8), (64, None), (65, 8), (1000, 8), (1000, None), (200, 8)]):
        for max_fpr in (0.1, 0.25, 1.0):
            out.append(random_case(N, levels, max_fpr, 100 + i))
    return out


def reference(c, which=ref_points):
    """int64 [C][8] of a case."""
    return np.array([which(c["scores"][k], c["labels"][k], c["max_fpr"]) for k in range(c["scores"].shape[0])], dtype=np.int64)


# ---------------------------------------------------------------------------------------------------- segment pooling
def microseconds(x):
    return np.rint(np.round(np.asarray(x, dtype=np.float64), 6) * 1e6).astype(np.int64)


GEOMETRIES = {                                      # name: (frames, frame seconds, clip seconds)
    "156x64ms": (156, 0.064, 10.0),                 # (the reference docstring's)
    "1000x10ms": (1000, 0.010, 10.0),
    "9.5s": (1000, 0.010, 9.5),
}


def geometry(name):
    """-> (ts_us int64 [T + 1], clip_us)."""
    T, hop, clip = GEOMETRIES[name]
    return microseconds(np.arange(T + 1) * hop), int(microseconds(clip))


def frame_scores(T, C, seed):
    return np.random.RandomState(seed).rand(T, C).astype(np.float32)


def pool_ref(scores, ts_us, clip_us, seg_us):
    """scores [T, C] f32 -> pooled f32 [ceil(clip / seg), C]: section 7g, one rounding per product, per addition, one division."""
    scores = np.asarray(scores, dtype=np.float32)
    n_seg = -(-int(clip_us) // int(seg_us))
    out = np.zeros((n_seg, scores.shape[1]), dtype=np.float32)
    for k in range(n_seg):
        start, end = k * seg_us, (k + 1) * seg_us
        num, den = np.zeros(scores.shape[1], dtype=np.float64), 0
        first = int(np.searchsorted(ts_us[1:], start, side="right"))     # frames ending at or before `start` weigh nothing
        for f in range(first, scores.shape[0]):
            if ts_us[f] >= end:
                break
            w = min(int(ts_us[f + 1]), end) - max(int(ts_us[f]), start)
            if w <= 0:
                continue
            num = num + np.float64(w) * scores[f].astype(np.float64)
            den += w
        if den <= 0:
            raise ValueError("a segment without weight")
        out[k] = (num / np.float64(den)).astype(np.float32)
    return out


def overlap_add_ref(clips, n_seg, seg_us):
    """clips: [(onset_us, pooled f32 [k, C])] of one file, in arrival order -> f32 [n_seg, C]: the mean over the contributing clips in
    increasing onset (arrival order among equal onsets), 0 where no clip reaches."""
    C = clips[0][1].shape[1]
    total, count = np.zeros((n_seg, C), dtype=np.float64), np.zeros(n_seg, dtype=np.int64)
    for onset, pooled in sorted(clips, key=lambda c: c[0]):
        first = onset // seg_us
        for k in range(pooled.shape[0]):
            total[first + k] = total[first + k] + pooled[k].astype(np.float64)
            count[first + k] += 1
    return (total / np.maximum(count, 1)[:, None]).astype(np.float32)


def sliding_file(duration=23.4, n_clips=14, clip=10.0):
    """The 23.4 s file under 14 sliding clips of 10 s, one per second -> (clip ids, onsets_us, duration)."""
    ids = [f"long-{100 * o}-{100 * o + int(100 * clip)}" for o in range(n_clips)]
    return ids, [o * 1000000 for o in range(n_clips)], duration
