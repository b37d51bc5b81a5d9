"""Host references and seeded inputs for the change-detection sound event bounding boxes, pure numpy.

The definition is stated twice:
  * `row_loop`      a plain Python loop over one row, written straight from steps 1-6 with Python integers.
  * `row_numpy`     vectorised numpy: prefix sums, windowed extrema by sliding windows over a padded D, the walk by alternation of the
                    candidate list; only the greedy merge stays a loop (it is serial by definition).
Both return (boxes [(onset, offset)], conf [float32], scores [T] float32).  `bank_ref` applies one of them to every (row, clip, class) of
a bank; `quantise` is step 1 alone.  Generators: smooth random rows, rows on the grid {0, 0.25, 0.5, 1} (ties in D and in the means
everywhere), plateaus.  Everything is generated from seeds; no test reads anything outside the repository."""
import numpy as np

Q = 1 << 24


def quantise(y):
    """Step 1: q = rint(y 2^24), round half to even; the product is exact in fp32."""
    y = np.asarray(y, dtype=np.float32)
    return np.rint(y * np.float32(Q)).astype(np.int64)


def quantise_params(tau, rho):
    return int(np.rint(np.float64(tau) * Q)), int(np.rint(np.float64(rho) * 256))


def confidence(S, n):
    return np.float32(np.float64(int(S)) / np.float64(int(n) << 24))


# ------------------------------------------------------------------------------------------------ the literal loop
def row_loop(y, L, tau, rho):
    q = [int(v) for v in quantise(y)]
    T = len(q)
    tau_q, rho_q = quantise_params(tau, rho)

    def s(a, b):                                # sum of q[a .. b), frames outside the clip count as 0
        return sum(q[max(a, 0):max(min(b, T), 0)])

    D = [s(t, t + L) - s(t - L, t) for t in range(T + 1)]
    onset, offset = [], []
    for t in range(T + 1):
        left = [D[u] for u in range(max(0, t - L), t)]
        right = [D[u] for u in range(t + 1, min(T, t + L) + 1)]
        onset.append(D[t] > 0 and all(D[t] > d for d in left) and all(D[t] >= d for d in right))
        offset.append(D[t] < 0 and all(D[t] < d for d in left) and all(D[t] <= d for d in right))
    events, on, a = [], False, 0
    for t in range(T + 1):
        if not on and onset[t]:
            on, a = True, t
        elif on and offset[t]:
            events.append((a, t))
            on = False
    if on:
        events.append((a, T))
    boxes = []
    if events:
        aE, bE = events[0]
        for aK, bK in events[1:]:
            SE, nE, SK, nK, SG, nG = s(aE, bE), bE - aE, s(aK, bK), bK - aK, s(bE, aK), aK - bE
            Sl, nl = (SE, nE) if SE * nK <= SK * nE else (SK, nK)
            if SG * nl + tau_q * nl * nG > Sl * nG and rho_q * SG * nl > 256 * Sl * nG:
                bE = bK
            else:
                boxes.append((aE, bE))
                aE, bE = aK, bK
        boxes.append((aE, bE))
    conf = [confidence(s(a, b), b - a) for a, b in boxes]
    scores = np.zeros(T, dtype=np.float32)
    for (a, b), c in zip(boxes, conf):
        scores[a:b] = c
    return boxes, conf, scores


# ------------------------------------------------------------------------------------------------ vectorised
def candidates_numpy(q, L):
    """Steps 2-4 -> (P [T + 1] int64 prefix sums, events [n, 2])."""
    T = len(q)
    P = np.concatenate(([0], np.cumsum(q, dtype=np.int64)))
    t = np.arange(T + 1)
    D = (P[np.minimum(t + L, T)] - P[t]) - (P[t] - P[np.maximum(t - L, 0)])
    Lw = min(L, T + 1)                          # windows beyond the clip hold nothing more
    big = np.int64(1) << 62
    view = np.lib.stride_tricks.sliding_window_view

    def extrema(pad):                           # (over the Lw boundaries left of t, over the Lw right of t) of D padded with `pad`
        Dp = np.concatenate((np.full(Lw, pad, dtype=np.int64), D, np.full(Lw, pad, dtype=np.int64)))
        w = view(Dp, Lw)                        # w[i] covers Dp[i .. i + Lw) = D[i - Lw .. i)
        return w[:T + 1], w[Lw + 1:Lw + T + 2]
    left, right = extrema(-big)
    onset = (D > 0) & (D > left.max(axis=1)) & (D >= right.max(axis=1))
    left, right = extrema(big)
    offset = (D < 0) & (D < left.min(axis=1)) & (D <= right.min(axis=1))
    # the walk: a candidate counts when it differs in kind from the last one that counted, starting from "off"
    idx = np.flatnonzero(onset | offset)
    kinds = onset[idx]                          # True onset, False offset
    if len(idx):
        keep = np.concatenate(([True], kinds[1:] != kinds[:-1]))
        idx, kinds = idx[keep], kinds[keep]
        if not kinds[0]:
            idx, kinds = idx[1:], kinds[1:]
    if len(idx) % 2:
        idx = np.concatenate((idx, [T]))
    return P, idx.reshape(-1, 2)


def row_numpy(y, L, tau, rho):
    q = quantise(y)
    T = len(q)
    tau_q, rho_q = quantise_params(tau, rho)
    P, events = candidates_numpy(q, L)
    P = [int(p) for p in P]
    boxes = []
    if len(events):
        aE, bE = (int(v) for v in events[0])
        for aK, bK in events[1:].tolist():
            SE, nE, SK, nK, SG, nG = P[bE] - P[aE], bE - aE, P[bK] - P[aK], bK - aK, P[aK] - P[bE], aK - bE
            Sl, nl = (SE, nE) if SE * nK <= SK * nE else (SK, nK)
            if SG * nl + tau_q * nl * nG > Sl * nG and rho_q * SG * nl > 256 * Sl * nG:
                bE = bK
            else:
                boxes.append((aE, bE))
                aE, bE = aK, bK
        boxes.append((aE, bE))
    conf = [confidence(P[b] - P[a], b - a) for a, b in boxes]
    scores = np.zeros(T, dtype=np.float32)
    if boxes:
        ab = np.asarray(boxes)
        inside = np.zeros(T + 1, dtype=np.int64)
        np.add.at(inside, ab[:, 0], 1)
        np.add.at(inside, ab[:, 1], -1)
        which = np.cumsum(inside[:T]) > 0
        owner = np.searchsorted(ab[:, 0], np.arange(T), side="right") - 1
        scores[which] = np.asarray(conf, dtype=np.float32)[owner[which]]
    return boxes, conf, scores


# ------------------------------------------------------------------------------------------------ banks
def bank_ref(x, rows, scale=None, fn=row_numpy):
    """x [B, T, C] fp32, rows [K] of (L [C], tau [C], rho [C]) -> (scores [K, B, T, C] fp32, boxes {(k, b, c): ([(a, b)], [conf])});
    `scale` [B, C] multiplies in fp32 first, as the kernel does."""
    x = np.asarray(x, dtype=np.float32)
    if scale is not None:
        x = x * np.asarray(scale, dtype=np.float32)[:, None, :]
    B, T, C = x.shape
    scores = np.zeros((len(rows), B, T, C), dtype=np.float32)
    boxes, memo = {}, {}
    for k, (Ls, taus, rhos) in enumerate(rows):
        for b in range(B):
            for c in range(C):
                key = (b, c, int(Ls[c]), float(taus[c]), float(rhos[c]))
                if key not in memo:
                    memo[key] = fn(x[b, :, c], int(Ls[c]), taus[c], rhos[c])
                bx, cf, sc = memo[key]
                scores[k, b, :, c] = sc
                boxes[(k, b, c)] = (bx, cf)
    return scores, boxes


def uniform_row(C, L, tau, rho):
    return ([L] * C, [tau] * C, [rho] * C)


# ------------------------------------------------------------------------------------------------ generators
def smooth(B, T, C, seed=0):
    """[B, T, C] fp32 in [0, 1]: random events on a noisy floor, smoothed over a few frames."""
    rng = np.random.RandomState(7100 + seed + 3 * B + 7 * T + 11 * C)
    x = rng.rand(B, T, C) * 0.3
    for b in range(B):
        for c in range(C):
            for _ in range(rng.randint(0, 4)):
                a = rng.randint(0, T)
                x[b, a:a + rng.randint(1, max(2, T // 3)), c] += 0.4 + 0.3 * rng.rand()
    k = min(5, T)
    ker = np.ones(k) / k
    x = np.apply_along_axis(lambda v: np.convolve(v, ker, mode="same"), 1, x)
    return np.clip(x, 0, 1).astype(np.float32)


def grid(B, T, C, seed=0):
    """[B, T, C] fp32 drawn from {0, 0.25, 0.5, 1} in runs of random length: ties in D and in the means are everywhere."""
    rng = np.random.RandomState(7200 + seed + 3 * B + 7 * T + 11 * C)
    levels = np.asarray([0, 0.25, 0.5, 1], dtype=np.float32)
    x = np.zeros((B, T, C), dtype=np.float32)
    for b in range(B):
        for c in range(C):
            t = 0
            while t < T:
                n = rng.randint(1, 9)
                x[b, t:t + n, c] = levels[rng.randint(0, 4)]
                t += n
    return x


def plateau(T, a, b, high=1.0, low=0.0):
    y = np.full(T, low, dtype=np.float32)
    y[a:b] = high
    return y


# ------------------------------------------------------------------------------------------------ the search, literally
SEARCH_GRID = dict(step_filter_lengths=(0.3, 0.7, 1.5), merge_thresholds_abs=(0.1, 0.3), merge_thresholds_rel=(1.5, 3.0))


def grid_rows(C, period, step_filter_lengths, merge_thresholds_abs, merge_thresholds_rel):
    """-> [(name, (L [C], tau [C], rho [C]))] in grid order: step filter length outermost, then tau, then rho."""
    out = []
    for s in step_filter_lengths:
        L = max(1, int(np.floor(s / (2 * period) + 0.5)))
        for tau in merge_thresholds_abs:
            for rho in merge_thresholds_rel:
                out.append((f"{s:g}/{tau:g}/{rho:g}", uniform_row(C, L, tau, rho)))
    return out


def host_search(case, **kw):
    """A `SebbSearch` on the case's ground truth whose device steps are the host references: `bank_ref` for the bank,
    `psds_cases.cpu_sweep` for the sweep, `f1_cases.cpu_counts` for the counting kernel.  Everything behind them is the product's."""
    import torch
    import f1_cases as FC
    import psds_cases as PC
    import search_cases as SC
    from transformer4sed_amd.sebb import SebbSearch

    class HostSearch(SebbSearch):
        def _bank(self, x, rows, mode, scale):
            return torch.from_numpy(bank_ref(x.cpu().numpy(), self._rows, None if scale is None else scale.cpu().numpy())[0])

        def _psds_accumulator(self, timestamps, args):
            acc = super()._psds_accumulator(timestamps, args)
            acc._sweep = PC.cpu_sweep(acc)
            return acc

        def _f1_accumulator(self, timestamps):
            acc = super()._f1_accumulator(timestamps)
            acc._run = FC.cpu_counts(acc)
            return acc

    gt, dur = PC.frames(case)
    return HostSearch(SC.planted_encoder(case), gt, dur, **kw)


def _first_greatest(values):
    best = 0
    for i, v in enumerate(values):
        if v > values[best]:
            best = i
    return best


def psds_search_ref(case, rows, a, weak=None, max_efpr=100.0):
    """The brute force: every row through `bank_ref`, `psds_cases.sweep_ref` and `psds_from_points`; per class the first greatest
    single-class value; the overall value composed from the chosen rows' operating points and a fresh run on the mixed parameters."""
    import psds_cases as PC
    C = case.scores.shape[2]
    bank = bank_ref(case.scores, [r for _, r in rows], weak)[0]
    single, overall, points = [], [], []
    for k in range(len(rows)):
        boxed = case._replace(scores=bank[k])
        pts = PC.sweep_ref(boxed, a)
        psds, one, _, _ = PC.psds_from_points(boxed, a, pts, max_efpr=max_efpr)
        single.append(one)
        overall.append(psds)
        points.append(pts)
    choice = [_first_greatest([single[k][c] for k in range(len(rows))]) for c in range(C)]
    composed = PC.psds_from_points(case, a, [points[choice[c]][c] for c in range(C)], max_efpr=max_efpr)[0]
    mixed = tuple([rows[choice[c]][1][j][c] for c in range(C)] for j in range(3))
    boxed = case._replace(scores=bank_ref(case.scores, [mixed], weak)[0][0])
    fresh = PC.psds_from_points(boxed, a, PC.sweep_ref(boxed, a), max_efpr=max_efpr)[0]
    return dict(single=single, overall=overall, choice=choice, composed=composed, fresh=fresh, mixed=mixed)


def f1_counts_ref(case, row, theta, weak):
    """The six integer counts per class of the event path: hard mask weak >= theta, boxes with confidence > theta."""
    import f1_cases as FC
    keep = (np.asarray(weak, dtype=np.float32) >= np.float32(theta)).astype(np.float32)
    active = bank_ref(case.scores, [row], keep)[0][0] > np.float32(theta)
    return FC.brute(FC.Case(active, case.ts, sorted(case.gt), case.names, case.classes))


def f1_search_ref(case, rows, thetas, weak, kind):
    import f1_cases as FC
    import search_cases as SC
    C = case.scores.shape[2]
    counts = [[f1_counts_ref(case, r, th, weak) for th in thetas] for _, r in rows]
    values = [[SC.f1_scores(cn, kind) for cn in per] for per in counts]
    choice = [divmod(_first_greatest([values[k][j][c] for k in range(len(rows)) for j in range(len(thetas))]), len(thetas)) for c in range(C)]
    composed = {n: [counts[choice[c][0]][choice[c][1]][n][c] for c in range(C)] for n in FC.NAMES}
    return dict(values=values, choice=choice, composed=composed, counts=counts)
