"""Host restatements and seeded inputs for score-level ensembling (csrc/ensemble.hip), pure numpy.

  * `coords`      the integer source coordinate of the linear half-pixel rule: i0, i1, rem with lambda = rem / (2 T).
  * `combine32`   (a) the kernel's mode 0 in ITS operation order, every operation one numpy float32 operation: the bits the kernel writes.
                  Its `fault` switch makes the five wrong kernels the CPU test shows the bound to catch.
  * `combine64`   (b) the definition in float64 (both modes).
  * `bound`       the error model of (a) against (b), from the count of fp32 roundings per output.

Everything is generated from seeds; no test reads anything outside the repository."""
import numpy as np

U = 2.0 ** -24                                  # one fp32 rounding of a quantity of magnitude <= 1 (half an ulp of [1, 2))
LO, HI = np.float32(1e-7), np.float32(1.0) - np.float32(1e-7)      # mode 1's clamp: the fp32 numbers
SENTINEL = np.float32(-12345.0)
FAULTS = ("wrong_neighbour", "dropped_member", "row_shift", "class_shift", "missing_pass")


def bound(M):
    """|(a) - (b)| for scores in [0, 1] and normalised weights (w >= 0, sum_m w = 1; the SAME fp32 weights on both sides, so their own
    rounding does not enter).  Per member: lambda = float(rem) / float(2 T) is one rounding, |d lambda| <= U, times |x1 - x0| <= 1: U; the
    difference x1 - x0: U; the product lambda d: U; the sum x0 + .: U -- v_m is within 4 U.  The product w_m v_m adds U w_m (relative), so
    the members' errors weigh (4 U + U) sum_m w_m = 5 U; the M - 1 additions of partial sums <= 1 add U each.  (4 + M) U in all; the
    float64 side's own error is 1e-16."""
    return (4 + M) * U


def coords(T, Tm):
    """-> (i0, i1, rem) int64 [T]: num = max((2 t + 1) Tm - T, 0), i0 = num // (2 T), i1 = min(i0 + 1, Tm - 1), rem = num - 2 T i0."""
    t = np.arange(T, dtype=np.int64)
    num = np.maximum((2 * t + 1) * Tm - T, 0)
    i0 = num // (2 * T)
    i1 = np.minimum(i0 + 1, Tm - 1)
    return i0, i1, num - 2 * T * i0


def resample32(x, T, wrong_neighbour=False):
    """x [n, Tm, C] fp32 -> [n, T, C] fp32: x[i0] where rem == 0 or i1 == i0, else x0 + lambda (x1 - x0), three fp32 operations."""
    x = np.asarray(x, dtype=np.float32)
    i0, i1, rem = coords(T, x.shape[1])
    if wrong_neighbour:
        i1 = i0
    lam = (rem.astype(np.float32) / np.float32(2 * T))[None, :, None]
    x0, x1 = x[:, i0], x[:, i1]
    v = x0 + lam * (x1 - x0)
    return np.where(((rem == 0) | (i1 == i0))[None, :, None], x0, v).astype(np.float32)


def resample64(x, T):
    x = np.asarray(x, dtype=np.float64)
    i0, i1, rem = coords(T, x.shape[1])
    lam = (rem.astype(np.float64) / np.float64(2 * T))[None, :, None]
    return x[:, i0] + lam * (x[:, i1] - x[:, i0])


def round32(y, decimals):
    """y = rintf(y 10^d) / 10^d in fp32."""
    if decimals is None:
        return y
    s = np.float32(10.0 ** decimals)
    return (np.rint(y * s) / s).astype(np.float32)


def combine64(members, w, T, mode=0):
    """(b): members [n, Tm, C], w [W, M, C] (normalised fp32) -> float64 [W, n, T, C], no rounding to decimals."""
    w = np.asarray(w, dtype=np.float64)
    acc = 0.0
    for m, x in enumerate(members):
        v = resample64(x, T)
        if mode == 1:
            q = np.clip(v, np.float64(LO), np.float64(HI))
            v = np.log(q) - np.log1p(-q)
        acc = acc + w[:, m][:, None, None, :] * v[None]
    return 1.0 / (1.0 + np.exp(-acc)) if mode == 1 else acc


def combine32(members, w, T, mode=0, decimals=None, fault=None, grid_pass=None):
    """(a): -> fp32 [W, n, T, C], the kernel's bits in mode 0: y = w_0 v_0, then y = y + w_m v_m, m ascending, every product and sum a
    float32 operation; then the rounding.  Mode 1 is the float64 definition rounded to fp32 (the kernel is not pinned there).
    `fault`: one of FAULTS ("missing_pass": the elements of the last grid pass of `grid_pass` elements keep SENTINEL)."""
    assert fault is None or fault in FAULTS
    w = np.ascontiguousarray(w, dtype=np.float32)
    W, M, C = w.shape
    assert len(members) == M
    if fault == "row_shift":
        w = np.roll(w, 1, axis=0)
    if fault == "class_shift":
        w = np.roll(w, 1, axis=2)
    if mode == 1:
        y = combine64(members, w, T, 1).astype(np.float32)
    else:
        use = M - 1 if (fault == "dropped_member" and M > 1) else M
        y = None
        for m in range(use):
            v = resample32(members[m], T, fault == "wrong_neighbour")
            term = w[:, m][:, None, None, :] * v[None]
            y = term if y is None else y + term
    y = np.ascontiguousarray(round32(y, decimals))
    if fault == "missing_pass":
        N = int(np.prod(y.shape[1:]))
        flat = y.reshape(W, N)
        flat[:, (N - 1) // grid_pass * grid_pass:] = SENTINEL
    return y


# ------------------------------------------------------------------------------------------------ inputs
def members(n, Tms, C, seed=0):
    """One fp32 array [n, Tm, C] in [0, 1) per entry of Tms."""
    rng = np.random.RandomState(7000 + seed + 3 * n + 11 * C)
    return [rng.rand(n, int(tm), C).astype(np.float32) for tm in Tms]


def weights(W, M, C=None, seed=0, rows_only=False):
    """Raw (not normalised) non-negative weights [W, M] (C None) or [W, M, C], or [M] with `rows_only`; a few exact zeros."""
    rng = np.random.RandomState(8000 + seed + 5 * W + 13 * M)
    shape = (M,) if rows_only else ((W, M) if C is None else (W, M, C))
    w = rng.randint(0, 9, size=shape).astype(np.float64) / 4.0
    s = w.sum(axis=0 if rows_only else 1, keepdims=True)
    return w + (s == 0)                          # (a row of zeros becomes a row of ones)


def mode1_fixture():
    """3 clips, 4 members of 40 / 20 / 10 / 1 frames, 10 classes, uniform scores with exact 0 and 1 among them, 7 per-class weight rows
    -> (members, normalised weights [7, 4, 10], the raw weights `combine` normalises to them), at T = 40: the fixture mode 1's error is
    measured and asserted on."""
    from transformer4sed_amd.ensemble import normalise_weights
    ms = members(3, (40, 20, 10, 1), 10, seed=5)
    ms[0][0, :4, 0] = (0.0, 1.0, 0.0, 1.0)
    ms[1][1, :2, 3] = (1.0, 0.0)
    raw = weights(7, 4, 10, seed=5)
    return ms, normalise_weights(raw, 4, 10), raw


def near_tie(y64, decimals=4, margin=1e-6):
    """Entries of the float64 definition within `margin` of a rounding tie (k + 1/2) 10^-decimals."""
    s = 10.0 ** decimals
    frac = y64 * s - np.floor(y64 * s)
    return np.abs(frac - 0.5) <= margin * s


# ------------------------------------------------------------------------------------------------ host stand-ins for the device steps
def host_combine(members, weights, T, mode, decimals):
    """`ensemble._combine_host` on the host: numpy members -> numpy [W, n, T, C] through `combine32`, after the product's own checks."""
    import torch
    from transformer4sed_amd import ensemble as E
    members = [np.ascontiguousarray(x, dtype=np.float32) for x in members]
    n, C, _, T = E.check_members([torch.from_numpy(x) for x in members], T)
    return combine32(members, E.normalise_weights(weights, len(members), C), T, E.check_mode(mode), decimals)


def search_case(seed=3, n=6, t=200):
    """-> (psds_cases.Case, strongs [[n, C, t], [n, C, t / 2]], weaks [[n, C]] * 2): `search_cases.planted` ground truth seen by two
    members with independent noise -- member 0 at the full frame rate, noisy on class 0 and clean on class 1; member 1 at half the rate
    (means of frame pairs), clean on class 0 and noisy on class 1; both noisy on class 2."""
    import search_cases as SC
    case = SC.planted(seed=seed, n=n, t=t)
    rng = np.random.RandomState(40 + seed)
    sigma = np.asarray([[0.35, 0.05, 0.25], [0.05, 0.35, 0.25]])
    views = [np.clip(case.scores + rng.randn(n, t, 3) * sigma[m], 0.0, 1.0).astype(np.float32) for m in range(2)]
    views[1] = (0.5 * (views[1][:, 0::2] + views[1][:, 1::2])).astype(np.float32)
    strongs = [np.ascontiguousarray(v.transpose(0, 2, 1)) for v in views]
    weaks = [np.clip(SC.planted_weak(case) + rng.randn(n, 3).astype(np.float32) * 0.1, 0.0, 1.0).astype(np.float32) for _ in range(2)]
    return case, strongs, weaks


def host_search(case, n_members, **kw):
    """An `EnsembleSearch` on the case's ground truth whose device steps are host code: `combine32` for the bank, the scipy / numpy
    filters of `search_cases.bank_ref` for the score and event paths, `psds_cases.cpu_sweep` and `f1_cases.cpu_counts` for the
    accumulators' kernels.  Everything behind them is the product's."""
    import torch
    import f1_cases as FC
    import psds_cases as PC
    import search_cases as SC
    from transformer4sed_amd import ensemble as E

    class HostSearch(E.EnsembleSearch):
        def _bank(self, members, weights, T):
            members = [x.cpu().numpy() for x in members]
            w = E.normalise_weights(weights, len(members), members[0].shape[2])
            return torch.from_numpy(combine32(members, w, T, E.MODES[self.mode]))

        def _scores(self, strong, weak):
            x = np.ascontiguousarray(strong.cpu().numpy().transpose(0, 2, 1))
            scale = weak.cpu().numpy() if self.weak_mask else None
            if self.median_filter is None:
                return torch.from_numpy(x if scale is None else x * scale[:, None, :])
            return torch.from_numpy(SC.bank_ref(x, [self.median_filter], SC.MODES[self.filter_type], scale)[0])

        def _events(self, strong, weak, threshold):
            x = np.ascontiguousarray(strong.cpu().numpy().transpose(0, 2, 1))
            keep = (weak.cpu().numpy() >= np.float32(threshold)).astype(np.float32)
            rows = [self.median_filter or [1] * x.shape[2]]
            return torch.from_numpy(SC.bank_ref(x, rows, SC.MODES["torch"], keep)[0] > np.float32(threshold))

        def _psds_accumulator(self, timestamps, args):
            acc = super()._psds_accumulator(timestamps, args)
            acc._sweep = PC.cpu_sweep(acc)
            return acc

        def _f1_accumulator(self, timestamps):
            acc = super()._f1_accumulator(timestamps)
            acc._run = FC.cpu_counts(acc)
            return acc

    gt, dur = PC.frames(case)
    return HostSearch(SC.planted_encoder(case), gt, dur, n_members, **kw)


def feed(search, case, strongs, weaks, batches=None, dev="cpu"):
    import torch
    n = len(case.names)
    for lo, hi in batches or [(0, n)]:
        search.update([torch.from_numpy(s[lo:hi]).to(dev) for s in strongs], [torch.from_numpy(w[lo:hi]).to(dev) for w in weaks],
                      [case.names[i] + ".wav" for i in range(lo, hi)])
    return search


def write_score_folders(root, case, strongs, names=("full", "half")):
    """The members' strong posteriors as score-TSV folders root/<name>/<clip>.tsv (onset, offset, classes), 6 decimals."""
    import os
    import pandas as pd
    dur = case.durations[0]
    for name, s in zip(names, strongs):
        os.makedirs(os.path.join(root, name), exist_ok=True)
        T = s.shape[2]
        ts = np.round(dur / T * np.arange(T + 1), 6)
        for j, clip in enumerate(case.names):
            df = pd.DataFrame(np.concatenate([ts[:-1, None], ts[1:, None], s[j].T.astype(np.float64)], axis=1),
                              columns=["onset", "offset", *case.classes])
            df.to_csv(os.path.join(root, name, clip + ".tsv"), sep="\t", index=False)
    return [os.path.join(root, name) for name in names]
