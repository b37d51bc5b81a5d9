"""Score-level ensembling on the device with a weight-bank search (csrc/ensemble.hip).

The reference averages the frame scores of several systems with hand-typed weights (src/postprocess/ensemble.py: `cnn-trans` and
`atst-cnn` at 0.7 / 0.3, at different frame rates) and averages chosen classes of score containers (src/postprocess/score.py).  Here:

  * `combine`                  members [n, T_m, C] on the device -> [W, n, T, C] for W weight rows from ONE launch per 64 rows: every member
                               is resampled to T frames (linear, half-pixel, the coordinate in integers) and read once for the whole bank.
  * `weighted_average_ensemble`, `load_predictions`, `save_predictions`, `ensemble` and `Score`, `ScoreContainer`, `score_average`: the
                               reference's functions on score-TSV folders and DataFrames, on `combine`.
  * `EnsembleSearch`           which weights: every row of a simplex grid feeds accumulators of its own (`IntersectionPSDS`,
                               `EventSegmentF1`), the choice is made per class and composed from integers, as `PostprocSearch` does.

There is no CPU path: `combine` refuses host tensors.  `_combine_host`, and the search's `_bank`, `_scores`, `_events`, `_psds_accumulator`
and `_f1_accumulator`, are the device steps; a test without a GPU replaces them with host restatements."""
import copy
import json
import os
from collections import namedtuple
from dataclasses import asdict, dataclass
from itertools import combinations
from pathlib import Path
from typing import Optional

import numpy as np
import pandas as pd
import torch

from .evaluation.codec import _events_device, _scores_device, check_filter_type, frame_boundaries
from .evaluation.evaluator import Evaluator
from .evaluation.event_f1 import F1_COUNTS, EventSegmentF1
from .evaluation.ground_truth import _table
from .evaluation.psds import IntersectionPSDS
from .ops import call, h2d
from .postproc_search import F1_OBJECTIVES, _first_greatest, window_frames

MAX_MEMBERS = 8                 # csrc/ensemble.hip: ENS_MAX_M
MAX_ROWS = 64                   # ENS_MAX_W: weight rows of one launch
MAX_WEIGHTS = 32768             # ENS_MAX_WEIGHTS: W * M * C floats of LDS
GRID_THREADS = 256              # ENS_THREADS
MAX_GRID = 1024                 # ENS_MAX_GRID: workgroups of one launch
GRID_PASS = MAX_GRID * GRID_THREADS             # elements (n T C) of one pass of the kernel's grid-stride loop
MODES = {"mean": 0, "logit": 1}
REFERENCE_DECIMALS = 4          # src/postprocess/ensemble.py:51


# ------------------------------------------------------------------------------------------------ the bank
def check_mode(mode):
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
    return MODES[mode]


def check_decimals(decimals):
    if decimals is None:
        return -1
    if int(decimals) != decimals or not 0 <= int(decimals) <= 9:
        raise ValueError("decimals must be None or an integer in 0 .. 9")
    return int(decimals)


def normalise_weights(weights, M, C):
    """[M], [W, M] or [W, M, C] non-negative weights -> float32 [W, M, C] with every (row, class) divided by its sum over the members (in
    float64, rounded to fp32 once): what the kernel is given."""
    w = np.asarray(weights, dtype=np.float64)
    if w.ndim == 1:
        w = w[None, :, None]
    elif w.ndim == 2:
        w = w[:, :, None]
    elif w.ndim != 3:
        raise ValueError("weights must be [M], [W, M] or [W, M, C]")
    if w.shape[0] < 1:
        raise ValueError("no weight row")
    if w.shape[1] != M:
        raise ValueError(f"the weights name {w.shape[1]} members, {M} were given")
    if w.shape[2] not in (1, C):
        raise ValueError(f"per-class weights must hold {C} classes, got {w.shape[2]}")
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError("weights must be finite and not negative")
    s = w.sum(axis=1, keepdims=True)
    if (s <= 0).any():
        raise ValueError("a weight row sums to 0")
    return np.ascontiguousarray(np.broadcast_to(w / s, (w.shape[0], M, C)), dtype=np.float32)


def check_members(members, T=None):
    """-> (n, C, [T_m], T) after the refusals: 1 .. 8 members, each [n, T_m, C] fp32 contiguous with n, T_m, C >= 1, one n and one C, and
    no T_m above T (default: the largest T_m) -- the bank raises the frame rate, it does not lower it."""
    members = list(members)
    if not 1 <= len(members) <= MAX_MEMBERS:
        raise ValueError(f"combine takes 1 .. {MAX_MEMBERS} members, got {len(members)}")
    for x in members:
        if not isinstance(x, torch.Tensor) or x.dim() != 3:
            raise ValueError("every member must be a tensor [n, T_m, C]")
        if x.dtype != torch.float32:
            raise ValueError(f"members must be float32, got {x.dtype}")
        if not x.is_contiguous():
            raise ValueError("members must be contiguous")
        if min(x.shape) < 1:
            raise ValueError(f"empty member {tuple(x.shape)}")
    n, C = members[0].shape[0], members[0].shape[2]
    if any(x.shape[0] != n for x in members):
        raise ValueError(f"members differ in the number of clips: {[x.shape[0] for x in members]}")
    if any(x.shape[2] != C for x in members):
        raise ValueError(f"members differ in the number of classes: {[x.shape[2] for x in members]}")
    Tms = [int(x.shape[1]) for x in members]
    T = max(Tms) if T is None else int(T)
    if T < 1 or any(tm > T for tm in Tms):
        raise ValueError(f"members of {Tms} frames cannot be combined at {T} frames: a member is never resampled to fewer frames")
    return int(n), int(C), Tms, T


def rows_per_launch(M, C):
    rows = min(MAX_ROWS, MAX_WEIGHTS // (M * C))
    if rows < 1:
        raise ValueError(f"{M} members x {C} classes: one weight row exceeds the {MAX_WEIGHTS} weights a launch holds")
    return rows


def combine(members, weights, *, T=None, mode="mean", decimals=None):
    """members: 1 .. 8 device tensors [n, T_m, C] fp32; weights [M], [W, M] or [W, M, C] (not negative; divided by their sum over the
    members) -> [W, n, T, C] fp32, T defaulting to the largest T_m.  mode "mean": y = sum_m w_m v_m (the reference's); "logit":
    y = sigmoid(sum_m w_m logit(v_m)).  decimals: None, or y rounded to that many decimals (the reference: 4).  Banks above 64 rows are
    split into launches."""
    code, dec = check_mode(mode), check_decimals(decimals)
    members = list(members)
    n, C, Tms, T = check_members(members, T)
    w = normalise_weights(weights, len(members), C)
    per = rows_per_launch(len(members), C)
    if not all(x.is_cuda for x in members):
        raise NotImplementedError("combine runs on the device only: the members must be HIP tensors (there is no CPU path)")
    dev = members[0].device
    if any(x.device != dev for x in members):
        raise ValueError("the members lie on different devices")
    M, W = len(members), w.shape[0]
    out = torch.empty((W, n, T, C), dtype=torch.float32, device=dev)
    table = h2d([x.data_ptr() for x in members], torch.int64, dev)
    tms = h2d(Tms, torch.int32, dev)
    w_d = h2d(w, torch.float32, dev)
    for lo in range(0, W, per):
        hi = min(lo + per, W)
        call("sed_ensemble_bank", table, tms, w_d[lo:hi], out[lo:hi], M, hi - lo, n, T, C, code, dec)
    return out


def _combine_host(members, weights, T, mode, decimals):
    """numpy members [n, T_m, C] -> numpy [W, n, T, C] through `combine` on the current device (the step a test without a GPU replaces)."""
    dev = torch.device("cuda")
    return combine([h2d(np.ascontiguousarray(x, dtype=np.float32), torch.float32, dev) for x in members], weights, T=T, mode=mode,
                   decimals=decimals).cpu().numpy()


# ------------------------------------------------------------------------------------------------ src/postprocess/ensemble.py
def load_predictions(subfolders):
    """{file: [(model name, score DataFrame), ...]} in the order of `subfolders`; every folder must hold the same set of .tsv files."""
    all_files = None
    for subfolder in subfolders:
        files = {f for f in os.listdir(subfolder) if f.endswith(".tsv")}
        if all_files is None:
            all_files = files
        elif files != all_files:
            raise ValueError(f"Subfolder {subfolder} contains different set of files.")
    predictions = {}
    for subfolder in subfolders:
        model_name = os.path.basename(subfolder)
        for file in sorted(all_files or ()):
            predictions.setdefault(file, []).append((model_name, pd.read_csv(os.path.join(subfolder, file), sep="\t")))
    return predictions


def _groups(keys, shape_of):
    """{shape signature: [key, ...]}: the files one launch serves."""
    groups = {}
    for k in keys:
        groups.setdefault(shape_of(k), []).append(k)
    return groups


def weighted_average_ensemble(predictions, weights, mode="mean"):
    """src/postprocess/ensemble.py:33.  predictions {file: [(model, DataFrame onset, offset, classes...)]}, weights [M] (divided by their
    sum) -> {file: DataFrame}: the weighted mean of the members' scores at the frame rate of the longest member, rounded to 4 decimals;
    `onset` / `offset` are the longest member's (the first of that length).  Shorter members are resampled to the OUTPUT SIZE, so every
    ratio of lengths works (the reference asks for a scale factor, which yields one frame too few at some ratios, such as 122 -> 1000)."""
    weights = np.asarray(weights, dtype=np.float64).reshape(-1)
    tables = {f: [df for _, df in models] for f, models in predictions.items()}
    for f, dfs in tables.items():
        if len(dfs) != len(weights):
            raise ValueError(f"{f}: {len(dfs)} members, {len(weights)} weights")
        if any(list(df.columns) != list(dfs[0].columns) for df in dfs):
            raise ValueError(f"{f}: the members' tables differ in their columns")
    out = {}
    for _, files in _groups(tables, lambda f: (tuple(len(df) for df in tables[f]), tables[f][0].shape[1])).items():
        M = len(weights)
        members = [np.stack([tables[f][m].values[:, 2:] for f in files]).astype(np.float32) for m in range(M)]
        y = _combine_host(members, weights, None, mode, REFERENCE_DECIMALS)[0]
        for j, f in enumerate(files):
            dfs = tables[f]
            longest = max(range(M), key=lambda m: (len(dfs[m]), -m))
            times = np.round(dfs[longest].values[:, :2].astype(np.float64), REFERENCE_DECIMALS)
            values = np.round(y[j].astype(np.float64), REFERENCE_DECIMALS)           # (the fp32 number nearest k 1e-4 -> the double)
            out[f] = pd.DataFrame(np.concatenate([times, values], axis=1), columns=dfs[0].columns)
    return {f: out[f] for f in predictions}


def save_predictions(predictions, output_folder):
    os.makedirs(output_folder, exist_ok=True)
    for file, df in predictions.items():
        df.to_csv(os.path.join(output_folder, file), sep="\t", index=False)


def ensemble(root, output_dir, model_list, weights):
    """src/postprocess/ensemble.py:67: the folders root/<model> combined into output_dir."""
    if len(weights) != len(model_list):
        raise ValueError("The number of weights must match the number of models.")
    predictions = load_predictions([os.path.join(root, m) for m in model_list])
    save_predictions(weighted_average_ensemble(predictions, weights), output_dir)


# ------------------------------------------------------------------------------------------------ src/postprocess/score.py
class Score:
    """One file's score table with the events it must hold (src/postprocess/score.py:7)."""

    def __init__(self, events, df=None) -> None:
        self.events = events
        self.df = None
        if df is not None:
            self.load(df)

    def load(self, df: pd.DataFrame):
        for event in self.events:
            if event not in list(df.columns):
                raise Exception("Don't find event \"{0}\" in table".format(event))
        self.df = df

    def reload_events(self, reload_events, reload_df: pd.DataFrame):
        if len(self.df) != len(reload_df):
            raise Exception("Input table must have the same length with Score")
        for event in reload_events:
            if (event not in self.events) or (event not in reload_df.columns):
                raise Exception("Event \"{0}\" misses in table".format(event))
            self.df[event] = reload_df[event].values

    def average_events(self, reload_events, reload_df_list: list):
        """In place: every event of `reload_events` becomes the mean over this table and the tables of the list."""
        assert type(reload_df_list) == list
        _average_tables(self.events, reload_events, [[self.df] + reload_df_list])

    def __len__(self):
        return len(self.df) if self.df is not None else 0


def _average_tables(events, reload_events, table_lists):
    """table_lists: per file [own df, other dfs...]; the own df is changed in place.  One `combine` per group of files of one length, with
    per-class weights: 1 / M on every member for a class of `reload_events`, 1 on the own table for every other class."""
    events = list(events)
    for dfs in table_lists:
        for event in reload_events:
            for df in dfs[1:]:
                if (event not in events) or (event not in df.columns):
                    raise Exception("Event \"{0}\" misses in table".format(event))
        if any(len(df) != len(dfs[0]) for df in dfs):
            raise Exception("Input table must have the same length with Score")
    cols = [e for e in events if e in set(reload_events)]
    if not cols or not table_lists:
        return
    M = len(table_lists[0])
    if M == 1:
        return
    for _, idx in _groups(range(len(table_lists)), lambda i: len(table_lists[i][0])).items():
        members = [np.stack([table_lists[i][m][cols].values for i in idx]).astype(np.float32) for m in range(M)]
        y = _combine_host(members, np.ones((1, M, len(cols))), None, "mean", None)[0]
        for j, i in enumerate(idx):
            for k, event in enumerate(cols):
                table_lists[i][0][event] = y[j, :, k].astype(np.float64)


class ScoreContainer:
    """{file: Score} (src/postprocess/score.py:46)."""

    def __init__(self, events, score_buffer: dict = None) -> None:
        self.events = events
        self.score_dict = dict()
        if score_buffer is not None:
            self.load(events, score_buffer)

    def load(self, events, score_buffer: dict):
        for file in score_buffer.keys():
            self.score_dict[file] = Score(events, score_buffer[file])

    def reload_events(self, reload_events, reload_container: "ScoreContainer"):
        for file, score in reload_container.score_dict.items():
            self.score_dict[file].reload_events(reload_events, score.df)

    def average_events(self, reload_events, reload_container_list: list) -> "ScoreContainer":
        """-> a copy whose events of `reload_events` are the mean over this container and those of the list; a class outside
        `reload_events` keeps this container's scores (weight 1 on the first container)."""
        assert type(reload_container_list) == list
        res = copy.deepcopy(self)
        _average_tables(self.events, reload_events,
                        [[res.score_dict[f].df] + [c.score_dict[f].df for c in reload_container_list] for f in res.files])
        return res

    def get_score_buffer(self):
        return {file: score.df for file, score in self.score_dict.items()}

    @property
    def files(self):
        return list(self.score_dict.keys())

    def __len__(self):
        return len(self.score_dict)


def score_average(reload_events, reload_container_list: list) -> "ScoreContainer":
    assert type(reload_container_list) == list
    if len(reload_container_list) == 1:
        return copy.deepcopy(reload_container_list[0])
    return reload_container_list[0].average_events(reload_events, reload_container_list[1:])


# ------------------------------------------------------------------------------------------------ the search
Row = namedtuple("Row", "name weights")         # one candidate: name, raw weights [M] (float64; divided by their sum in the bank)


def simplex_grid(M, step):
    """Every weight vector {k step} with sum 1 over M members: C(K + M - 1, M - 1) rows for K = 1 / step, as integer tuples k (sum K), in
    descending lexicographic order (member 0's weight falls first)."""
    K = int(round(1.0 / step)) if 0.0 < step <= 1.0 else 0
    if K < 1 or abs(K * step - 1.0) > 1e-9:
        raise ValueError(f"step {step!r} does not divide 1")
    if M < 1:
        raise ValueError("no member")
    rows = []
    for bars in combinations(range(K + M - 1), M - 1):                                # stars and bars
        edges = (-1,) + bars + (K + M - 1,)
        rows.append(tuple(edges[i + 1] - edges[i] - 1 for i in range(M)))
    return K, sorted(rows, reverse=True)


def make_rows(M, step=0.1, weights=None):
    """-> [Row]: the simplex grid, then the M single-member rows where the grid does not hold them already (it does for every step that
    divides 1), then the explicit rows of `weights` [R, M]; a row equal to an earlier one after normalisation is left out."""
    K, grid = simplex_grid(M, step)
    rows, seen = [], set()

    def add(name, w):
        w = np.asarray(w, dtype=np.float64)
        key = tuple(normalise_weights(w, M, 1).reshape(-1).tolist())
        if key not in seen:
            seen.add(key)
            rows.append(Row(name, [float(v) for v in w]))

    for k in grid:
        add("/".join(f"{v / K:.6g}" for v in k), [v / K for v in k])
    for m in range(M):
        add("/".join("1" if j == m else "0" for j in range(M)), [1.0 if j == m else 0.0 for j in range(M)])
    if weights is not None:
        extra = np.asarray(weights, dtype=np.float64)
        if extra.ndim != 2 or extra.shape[1] != M:
            raise ValueError(f"weights must be rows of {M} member weights")
        for w in extra:
            add("/".join(f"{v:.6g}" for v in w), w)
    return rows


@dataclass
class EnsembleChoice:
    """What `EnsembleSearch.best` returns: per class the member weights (normalised, [C][M]) and, for the F1 objectives, the threshold;
    `per_class` the class's value under its row, `overall` the value of the mixed choice (PSDS; macro F1, with `overall_micro`),
    `member_overall` the overall value of each member alone."""
    objective: str
    mode: str
    labels: list
    rows: list
    weights: list
    thresholds: Optional[list]
    per_class: list
    overall: float
    overall_micro: Optional[float] = None
    member_overall: Optional[list] = None

    def to_config(self):
        """What `combine` needs: the mode and the per-class weights as one row [1, M, C]."""
        return {"mode": self.mode, "weights": [[[self.weights[c][m] for c in range(len(self.labels))] for m in range(len(self.weights[0]))]]}

    def save(self, path):
        with open(path, "w") as f:
            json.dump(asdict(self), f, indent=1)

    @classmethod
    def load(cls, path):
        with open(path) as f:
            return cls(**json.load(f))


class EnsembleSearch:
    """`update(strongs, weaks, paths)` per validation batch -- lists of the members' [n, C, T_m] and [n, C] posteriors, as
    `Evaluator.step` returns the student's and the teacher's -- then `results()` / `overall(objective)` / `best(objective)`.

    Candidate rows: `make_rows(n_members, step, weights)`.  One bank launch (per 64 rows) combines the strong posteriors at
    T = `encoder.n_frames`, one the weak ones; every row then goes through the score-table path (`_scores_device`: soft weak scale with
    `weak_mask`, scipy median or max with the per-class `median_window`, given in the YAML's unit for 156 frames; None: no filter) into
    its `IntersectionPSDS` per PSDS objective, and through the event path (`_events_device` per threshold) into its `EventSegmentF1`.
    A class's points depend on that class's scores alone, so the per-class choice is exact and the mixed choice's value is composed
    from the chosen accumulators' integers.

    Memory: one padded PSDS accumulator per row and PSDS objective -- n_members = 3 at step = 0.1 is 66 rows, 132 accumulators for
    psds1 + psds2 -- and the bank itself, rows x n x T x C floats per batch.

    The device steps are `_bank`, `_scores`, `_events`, `_psds_accumulator` and `_f1_accumulator`; a subclass may replace them."""

    def __init__(self, encoder, ground_truth, audio_durations, n_members, *, step=0.1, weights=None, mode="mean",
                 objectives=("psds1", "psds2"), thresholds=(0.5,), median_window=None, filter_type="median", weak_mask=False,
                 psds_args=None):
        self.encoder = encoder
        self.labels = list(encoder.labels)
        self.num_frames = int(encoder.n_frames)
        self.n_members = int(n_members)
        if not 1 <= self.n_members <= MAX_MEMBERS:
            raise ValueError(f"n_members must be 1 .. {MAX_MEMBERS}")
        check_mode(mode)
        self.mode = mode
        args = {k: dict(v) for k, v in Evaluator.PSDS_ARGS.items()}
        args.update({k: dict(v) for k, v in (psds_args or {}).items()})
        self.objectives = list(objectives)
        if not self.objectives:
            raise ValueError("no objective")
        for name in self.objectives:
            if name not in args and name not in F1_OBJECTIVES:
                raise ValueError(f"objective {name!r}: not one of {sorted(args)} or {list(F1_OBJECTIVES)}")
        self.psds_objectives = [o for o in self.objectives if o not in F1_OBJECTIVES]
        self.f1_objectives = [o for o in self.objectives if o in F1_OBJECTIVES]
        self.filter_type = check_filter_type(filter_type)
        self.thresholds = [float(t) for t in thresholds]
        if self.f1_objectives and not self.thresholds:
            raise ValueError("the F1 objectives need at least one threshold")
        self.weak_mask = bool(weak_mask)
        C = len(self.labels)
        self.median_filter = None
        if median_window is not None:
            if len(median_window) != C:
                raise ValueError(f"median_window must hold one window per class ({C})")
            self.median_filter = window_frames(median_window, self.num_frames)
            if min(self.median_filter) < 1:
                raise ValueError("a window needs at least 1 frame")
        self.rows = make_rows(self.n_members, step, weights)
        self._w = np.stack([np.asarray(r.weights, dtype=np.float64) for r in self.rows])          # [W, M], raw
        self._gt, self._dur = _table(ground_truth), _table(audio_durations)
        ts = frame_boundaries(encoder, self.num_frames)
        self._psds = {name: [self._psds_accumulator(ts, args[name]) for _ in self.rows] for name in self.psds_objectives}
        self._f1 = [[self._f1_accumulator(ts) for _ in self.rows] for _ in self.thresholds] if self.f1_objectives else []
        self._cache = {}

    # ---- the device steps
    def _bank(self, members, weights, T):
        """members [n, T_m, C] each, weights [W, M] -> [W, n, T, C]."""
        return combine(members, weights, T=T, mode=self.mode)

    def _scores(self, strong, weak):
        """One row's [n, C, T] / [n, C] -> the post-processed frame scores [n, T, C] of the score-table path."""
        raw, post = _scores_device(strong, strong.shape[0], self.median_filter, self.filter_type, weak, self.weak_mask)
        return raw if post is None else post

    def _events(self, strong, weak, threshold):
        """One row's [n, C, T] / [n, C] -> bool [n, T, C] of the event path at one threshold."""
        return _events_device(strong, weak, [threshold], self.median_filter or [1] * len(self.labels))[0]

    def _psds_accumulator(self, timestamps, args):
        return IntersectionPSDS(self._gt, self._dur, self.labels, timestamps, **args)

    def _f1_accumulator(self, timestamps):
        return EventSegmentF1(self._gt, self.labels, timestamps)

    @torch.no_grad()
    def update(self, strongs, weaks, paths):
        strongs, weaks = list(strongs), list(weaks)
        M, C, T = self.n_members, len(self.labels), self.num_frames
        if len(strongs) != M or len(weaks) != M:
            raise ValueError(f"update takes the posteriors of {M} members, got {len(strongs)} strong and {len(weaks)} weak")
        n = strongs[0].shape[0]
        if n > len(paths):
            raise IndexError("list index out of range")     # (batched_decode_preds' contract)
        for s, w in zip(strongs, weaks):
            if s.dim() != 3 or s.shape[0] != n or s.shape[1] != C or s.shape[2] > T:
                raise ValueError(f"every strong must be [{n}, {C}, T_m <= {T}], got {tuple(s.shape)}")
            if w is None or tuple(w.shape) != (n, C):
                raise ValueError(f"every weak must be [{n}, {C}]")
        if n == 0:
            return
        paths = list(paths[:n])
        self._cache = {}
        xs = [s.detach().transpose(1, 2).contiguous().float() for s in strongs]                  # [n, T_m, C]
        ws = [w.detach().float().reshape(n, 1, C).contiguous() for w in weaks]                   # [n, 1, C]: T_m = 1 broadcasts
        strong = self._bank(xs, self._w, T).transpose(2, 3)                                       # [W, n, C, T] (a view)
        weak = self._bank(ws, self._w, 1).reshape(len(self.rows), n, C)
        for name in self.psds_objectives:
            for ri, acc in enumerate(self._psds[name]):
                acc.update(self._scores(strong[ri], weak[ri]), paths)
        if self._f1:
            known = self._f1[0][0]._clip_index
            keep = [i for i, f in enumerate(paths) if Path(f).stem in known]
            if not keep:
                return
            kept = [paths[i] for i in keep]
            for ti, th in enumerate(self.thresholds):
                for ri, acc in enumerate(self._f1[ti]):
                    active = self._events(strong[ri], weak[ri], th)
                    if len(keep) != n:
                        idx = h2d(keep, torch.int64, active.device) if active.is_cuda else torch.as_tensor(keep, dtype=torch.int64)
                        active = active.index_select(0, idx)
                    acc.update(active, kept)

    # ---- finish: host arithmetic on the accumulators' integers
    def _psds_values(self, name):
        key = ("psds", name)
        if key not in self._cache:
            out = []
            for acc in self._psds[name]:
                overall, single = acc.compute()
                out.append((overall, [np.float64(single[c]) for c in self.labels]))
            self._cache[key] = out
        return self._cache[key]

    def _f1_counts(self):
        if "f1" not in self._cache:
            self._cache["f1"] = [[acc.counts() for acc in per] for per in self._f1]
        return self._cache["f1"]

    def normalised(self, ri):
        """Row ri's weights as the bank applies them: float32 [M], as floats."""
        return [float(v) for v in normalise_weights(self._w[ri], self.n_members, 1).reshape(-1)]

    def results(self):
        """One line per (objective, row[, threshold], class): DataFrame(objective, row, threshold, class, value) -- the single-class PSDS,
        or the class-wise F1."""
        lines = []
        for name in self.psds_objectives:
            for row, (_, single) in zip(self.rows, self._psds_values(name)):
                lines += [(name, row.name, None, label, float(single[c])) for c, label in enumerate(self.labels)]
        for name in self.f1_objectives:
            counts = self._f1_counts()
            for ri, row in enumerate(self.rows):
                for ti, th in enumerate(self.thresholds):
                    f1 = EventSegmentF1.scores(counts[ti][ri])[name]
                    lines += [(name, row.name, th, label, float(f1[c])) for c, label in enumerate(self.labels)]
        return pd.DataFrame(lines, columns=["objective", "row", "threshold", "class", "value"])

    def overall(self, objective, threshold=None):
        """{row name: overall value} of every single row: the PSDS, or the macro F1 at `threshold` (default: the first)."""
        if objective not in self.objectives:
            raise ValueError(f"objective {objective!r} was not searched ({self.objectives})")
        if objective in F1_OBJECTIVES:
            ti = 0 if threshold is None else self.thresholds.index(float(threshold))
            key = objective.replace("_f1", "_macro")
            return {r.name: EventSegmentF1.scores(cn)[key] for r, cn in zip(self.rows, self._f1_counts()[ti])}
        return {r.name: v[0] for r, v in zip(self.rows, self._psds_values(objective))}

    def _member_rows(self):
        """Index of each member's single row."""
        unit = np.eye(self.n_members)
        norm = self._w / self._w.sum(axis=1, keepdims=True)
        return [int(np.flatnonzero((norm == unit[m]).all(axis=1))[0]) for m in range(self.n_members)]

    def best(self, objective):
        """Per class the row -- for the F1 objectives the (row, threshold) pair -- with the greatest value; the first in row order wins a
        tie (thresholds inner, as given)."""
        if objective not in self.objectives:
            raise ValueError(f"objective {objective!r} was not searched ({self.objectives})")
        C = len(self.labels)
        if objective in F1_OBJECTIVES:
            counts = self._f1_counts()
            n_th = len(self.thresholds)
            f1 = [[EventSegmentF1.scores(counts[ti][ri])[objective] for ti in range(n_th)] for ri in range(len(self.rows))]
            pick = [divmod(_first_greatest([f1[ri][ti][c] for ri in range(len(self.rows)) for ti in range(n_th)]), n_th) for c in range(C)]
            mixed = {k: np.asarray([counts[ti][ri][k][c] for c, (ri, ti) in enumerate(pick)], dtype=np.int64) for k in F1_COUNTS}
            s = EventSegmentF1.scores(mixed)
            kind = objective.replace("_f1", "")
            return EnsembleChoice(objective=objective, mode=self.mode, labels=list(self.labels), rows=[self.rows[ri].name for ri, _ in pick],
                                  weights=[self.normalised(ri) for ri, _ in pick], thresholds=[self.thresholds[ti] for _, ti in pick],
                                  per_class=[float(f1[ri][ti][c]) for c, (ri, ti) in enumerate(pick)], overall=float(s[kind + "_macro"]),
                                  overall_micro=float(s[kind + "_micro"]),
                                  member_overall=[float(EventSegmentF1.scores(counts[0][ri])[kind + "_macro"]) for ri in self._member_rows()])
        values = self._psds_values(objective)
        pick = [_first_greatest([v[1][c] for v in values]) for c in range(C)]
        accs = self._psds[objective]
        points = [accs[pick[c]].counts()[c] for c in range(C)]                          # class c's operating points under ITS row
        overall = accs[0].compute_points(points)[0]
        return EnsembleChoice(objective=objective, mode=self.mode, labels=list(self.labels), rows=[self.rows[p].name for p in pick],
                              weights=[self.normalised(p) for p in pick], thresholds=None,
                              per_class=[float(values[p][1][c]) for c, p in enumerate(pick)], overall=float(overall),
                              member_overall=[float(values[ri][0]) for ri in self._member_rows()])
