"""Host references and seeded inputs for the post-processing search, pure numpy / scipy.

  * `bank_ref`      the filter bank as W calls of the `scipy.ndimage` filters (modes 1 / 2) and of the numpy restatement of
                    `median_filter_torch` (mode 0) in `longform_cases.filter_ref`, clip by clip.
  * `planted`       8 clips of 160 frames at 0.05 s, 3 classes whose best windows differ: long noisy events, pairs of short clean
                    events, medium events with a little noise; scores on a 1/64 grid.
  * `search_ref`    the search as a literal loop over filter types and candidates through `psds_cases.sweep_ref` / `psds_from_points`
                    and `f1_cases.brute`, the per-class choice, the composition and the fresh run on the mixed windows.  Its keyword
                    switches make the three WRONG searches the CPU tests show to be visible.

Everything is generated from seeds; no test reads anything outside the repository."""
import numpy as np

import f1_cases as FC
import longform_cases as LC
import psds_cases as PC

MODES = {"torch": 0, "median": 1, "max": 2}
MAX_EFPR = 100.0                               # `IntersectionPSDS`'s default, which the search keeps


# ------------------------------------------------------------------------------------------------ the bank
def bank_input(B, T, C, seed=0, ties=False):
    """[B, T, C] fp32 in [0, 1): distinct values, or values on a 1/8 grid (many ties)."""
    x = np.random.RandomState(5000 + seed + 3 * B + 7 * T + 11 * C).rand(B, T, C).astype(np.float32)
    return (np.floor(x * 8) / 8).astype(np.float32) if ties else x


def bank_ref(x, rows, mode, scale=None):
    """x [B, T, C] fp32, rows [W][C] -> [W, B, T, C] fp32; `scale` [B, C] multiplies in fp32 first, as the kernel does."""
    x = np.asarray(x, dtype=np.float32)
    if scale is not None:
        x = x * np.asarray(scale, dtype=np.float32)[:, None, :]
    return np.stack([np.stack([LC.filter_ref(x[b], row, mode) for b in range(x.shape[0])]) for row in rows])


# ------------------------------------------------------------------------------------------------ the planted case
FRAME = 0.05
PLANTED_WINDOWS = (1, 3, 7, 15, 31)            # in the YAML's unit; at 160 frames int(u / 156 * 160) = u
PLANTED_CONFIG = (15, 7, 15)                   # a hand-tuned list that is good, not best


def planted(seed=3, n=8, t=160):
    """-> psds_cases.Case.  Class 0: one event of 3 .. 4.5 s per clip, 25 % of the clip's frames flipped (only a long window mends it).
    Class 1: two events of 0.3 s per clip, clean scores (a window beyond 7 frames wipes them out).  Class 2: one event of 1 .. 2.5 s per
    clip, 8 % of the clip's frames flipped.  Inside an event the scores lie in [40, 63] / 64, outside in [0, 23] / 64; a flipped frame
    takes a value of the other range.  Events start and end on frame boundaries.  With the default seed, psds1 and the median, the
    single-class values are 1.0 at the windows {31}, {1, 3, 7} and {7, 15, 31} frames of the three classes and no single window does
    better than 0.195 overall; the event-based F1 at 0.5 prefers 15 frames for class 2."""
    rng = np.random.RandomState(seed)
    ts = FRAME * np.arange(t + 1)
    gt, flip = [], np.zeros((n, t, 3), dtype=bool)
    for b in range(n):
        length = rng.randint(60, 91)
        on = rng.randint(5, t - length - 5)
        gt.append((b, 0, round(on * FRAME, 3), round((on + length) * FRAME, 3)))
        flip[b, :, 0] = rng.rand(t) < 0.25
        first = rng.randint(5, 60)
        second = rng.randint(first + 30, t - 12)
        gt += [(b, 1, round(first * FRAME, 3), round((first + 6) * FRAME, 3)), (b, 1, round(second * FRAME, 3), round((second + 6) * FRAME, 3))]
        length = rng.randint(20, 51)
        on = rng.randint(5, t - length - 5)
        gt.append((b, 2, round(on * FRAME, 3), round((on + length) * FRAME, 3)))
        flip[b, :, 2] = rng.rand(t) < 0.08
    inside = np.zeros((n, t, 3), dtype=bool)
    for b, k, on, off in gt:
        inside[b, int(round(on / FRAME)):int(round(off / FRAME)), k] = True
    high = inside ^ flip
    scores = np.where(high, rng.randint(40, 64, size=(n, t, 3)), rng.randint(0, 24, size=(n, t, 3))) / 64.0
    return PC.Case(np.ascontiguousarray(scores, dtype=np.float32), ts, None, sorted(gt), [t * FRAME] * n, [f"clip{i}" for i in range(n)],
                   [f"class{k}" for k in range(3)])


def planted_weak(case):
    """[n, C] fp32 clip-level scores on a 1/64 grid: high where the clip holds the class (every clip holds every class here)."""
    n, _, c = case.scores.shape
    return (np.random.RandomState(11).randint(45, 64, size=(n, c)) / 64.0).astype(np.float32)


def planted_encoder(case):
    """The `Encoder` whose frame clock is the case's: t frames of 0.05 s (sr 16000, hop 800)."""
    from transformer4sed_amd.evaluation import Encoder
    t = case.scores.shape[1]
    return Encoder(case.classes, audio_len=t * FRAME, frame_len=1600, frame_hop=800, net_pooling=1, sr=16000)


def host_search(case, **kw):
    """A `PostprocSearch` on the case's ground truth whose device steps are the host references: `bank_ref` for the bank,
    `psds_cases.cpu_sweep` for the sweep, `f1_cases.cpu_counts` for the counting kernel.  Everything behind them is the product's."""
    import torch
    from transformer4sed_amd.postproc_search import PostprocSearch

    class HostSearch(PostprocSearch):
        def _bank(self, x, rows, mode, scale):
            return torch.from_numpy(bank_ref(x.cpu().numpy(), rows, mode, None if scale is None else scale.cpu().numpy()))

        def _psds_accumulator(self, timestamps, args):
            acc = super()._psds_accumulator(timestamps, args)
            acc._sweep = PC.cpu_sweep(acc)
            return acc

        def _f1_accumulator(self, timestamps):
            acc = super()._f1_accumulator(timestamps)
            acc._run = FC.cpu_counts(acc)
            return acc

    gt, dur = PC.frames(case)
    return HostSearch(planted_encoder(case), gt, dur, **kw)


def frames_of(units, t):
    """`scaled_median_window`'s rule at t frames."""
    return [int(u / 156 * t) for u in units]


def candidate_rows(windows, t, c, config=None):
    """-> [(name, frames [C])]: one uniform row per distinct frame count (the first unit that maps to it names it), then "config"."""
    rows, seen = [], set()
    for u, f in zip(windows, frames_of(windows, t)):
        if f not in seen:
            seen.add(f)
            rows.append((u, [f] * c))
    if config is not None:
        rows.append(("config", frames_of(config, t)))
    return rows


# ------------------------------------------------------------------------------------------------ the search, literally
def _first_greatest(values, last_on_ties=False):
    best = 0
    for i, v in enumerate(values):
        if v > values[best] or (last_on_ties and v == values[best]):
            best = i
    return best


def psds_table(case, rows, a, filter_type, weak=None, ignore_filter_type=False):
    """-> (single [n_rows][C] float64, overall [n_rows], points [n_rows] per class) of the literal loop."""
    mode = MODES["median" if ignore_filter_type else filter_type]
    bank = bank_ref(case.scores, [r for _, r in rows], mode, weak)
    single, overall, points = [], [], []
    for w in range(len(rows)):
        filtered = case._replace(scores=bank[w])
        pts = PC.sweep_ref(filtered, a)
        psds, one, _, _ = PC.psds_from_points(filtered, a, pts, max_efpr=MAX_EFPR)
        single.append(one)
        overall.append(psds)
        points.append(pts)
    return single, overall, points


def psds_search_ref(case, rows, a, filter_type, weak=None, *, ignore_filter_type=False, last_on_ties=False, wrong_class=False):
    """-> dict(single, overall, choice [C] = row index per class, composed, fresh): the per-class choice (greatest single-class value, the
    first row on ties), the overall value composed from the chosen rows' operating points, and the fresh run on scores filtered with the
    mixed windows.  The switches are the faults: a search that filters with the median whatever the type, one that takes the last
    candidate on ties, one that composes class c from the row chosen for class c + 1."""
    n_class = case.scores.shape[2]
    single, overall, points = psds_table(case, rows, a, filter_type, weak, ignore_filter_type)
    choice = [_first_greatest([single[w][c] for w in range(len(rows))], last_on_ties) for c in range(n_class)]
    src = [choice[(c + 1) % n_class] if wrong_class else choice[c] for c in range(n_class)]
    composed = PC.psds_from_points(case, a, [points[src[c]][c] for c in range(n_class)], max_efpr=MAX_EFPR)[0]
    mixed = [rows[choice[c]][1][c] for c in range(n_class)]
    filtered = case._replace(scores=bank_ref(case.scores, [mixed], MODES[filter_type], weak)[0])
    fresh = PC.psds_from_points(filtered, a, PC.sweep_ref(filtered, a), max_efpr=MAX_EFPR)[0]
    return dict(single=single, overall=overall, choice=choice, composed=composed, fresh=fresh, mixed=mixed)


def f1_counts_ref(case, row, theta, weak):
    """The six integer counts per class of the event path: hard mask weak >= theta, torch-semantics median, > theta."""
    keep = (np.asarray(weak, dtype=np.float32) >= np.float32(theta)).astype(np.float32)
    active = bank_ref(case.scores, [row], MODES["torch"], keep)[0] > np.float32(theta)
    fcase = FC.Case(active, case.ts, sorted(case.gt), case.names, case.classes)
    return FC.brute(fcase)


def f1_scores(counts, kind):
    """Class-wise F1 [C] (float64; 0.0 where the denominator is zero) from integer counts, `kind` "event_f1" or "segment_f1"."""
    out = []
    for c in range(len(counts["tp"])):
        if kind == "event_f1":
            num, den = 2.0 * counts["tp"][c], counts["n_ref"][c] + counts["n_sys"][c]
        else:
            num, den = 2.0 * counts["seg_tp"][c], 2 * counts["seg_tp"][c] + counts["seg_fp"][c] + counts["seg_fn"][c]
        out.append(num / den if den > 0 else 0.0)
    return out


def f1_search_ref(case, rows, thetas, weak, kind):
    """-> dict(values [n_rows][n_theta][C], choice [C] = (row, theta index), counts of the composition, mixed windows / thresholds):
    candidates outer, thresholds inner, the first greatest wins."""
    n_class = case.scores.shape[2]
    counts = [[f1_counts_ref(case, r, th, weak) for th in thetas] for _, r in rows]
    values = [[f1_scores(cn, kind) for cn in per] for per in counts]
    choice = []
    for c in range(n_class):
        flat = [values[w][j][c] for w in range(len(rows)) for j in range(len(thetas))]
        choice.append(divmod(_first_greatest(flat), len(thetas)))
    composed = {k: [counts[choice[c][0]][choice[c][1]][k][c] for c in range(n_class)] for k in FC.NAMES}
    return dict(values=values, choice=choice, composed=composed, counts=counts)
