"""Class-wise search of the post-processing parameters on the device: which median / max window, and for the event
lists which threshold, gives each class its best PSDS or F1 on a validation set.

The reference ships its per-class windows (`median_window: [5,20,5,5,5,20,20,20,5,20]`, `filter_type`) tuned by hand; here they are searched:
every batch of validation posteriors is filtered with ALL candidate windows by one launch per filter type (`filter.filter_bank`,
csrc/median_filter.hip: a column is staged and ranked once for the whole bank), each candidate's slice feeds an accumulator of its own
(`IntersectionPSDS` per filter type, candidate and argument set; `EventSegmentF1` per threshold and candidate), and the choice is made per
class at the end.  A class's single-class PSDS and its class-wise F1 depend on that class's scores alone -- the cross-trigger term of psds2
counts that class's detections against the other classes' GROUND TRUTH -- so the per-class choice is exact, and the value of the mixed choice
is composed from the chosen accumulators' integers instead of being run again."""
import json
from collections import namedtuple
from dataclasses import asdict, dataclass
from pathlib import Path
from typing import Optional

import numpy as np
import pandas as pd
import torch

from . import filter as dev_filter
from .evaluation.codec import check_filter_type, frame_boundaries
from .evaluation.evaluator import Evaluator
from .evaluation.event_f1 import F1_COUNTS, EventSegmentF1
from .evaluation.ground_truth import _table
from .evaluation.psds import IntersectionPSDS
from .ops import h2d

FILTER_MODES = {"median": 1, "max": 2}          # the score tables' filters (scipy semantics); the event path's is mode 0 (torch semantics)
F1_OBJECTIVES = ("event_f1", "segment_f1")
DEFAULT_WINDOWS = (1, 2, 3, 5, 7, 10, 14, 20, 28)
CONFIG = "config"

Candidate = namedtuple("Candidate", "name units frames")        # one window row: name, windows in the YAML's unit [C], in frames [C]


def window_frames(units, T):
    """`scaled_median_window`'s rule at T frames: the YAML's windows are given for 156 frames."""
    return [int(u / 156 * T) for u in units]


def make_candidates(windows, T, C, config_windows=None, scipy=True):
    """-> [Candidate]: one uniform row per window unit, units that map to the same frame count merged (the first is kept), then the
    YAML's own per-class list as the row "config".  Refused: a frame count below 1, and with `scipy` (the score tables' filters) above T."""
    def check(f, u):
        if f < 1:
            raise ValueError(f"window {u!r} is {f} frames at {T} frames per clip: a window needs at least 1 frame")
        if scipy and f > T:
            raise ValueError(f"window {u!r} is {f} frames, longer than the clip's {T}: outside the scipy filters' reproduced domain")
    out, seen = [], set()
    for u, f in zip(windows, window_frames(windows, T)):
        check(f, u)
        if f not in seen:
            seen.add(f)
            out.append(Candidate(str(u), [u] * C, [f] * C))
    if config_windows is not None:
        config_windows = list(config_windows)
        if len(config_windows) != C:
            raise ValueError(f"config_windows must hold one window per class ({C}), got {len(config_windows)}")
        frames = window_frames(config_windows, T)
        for u, f in zip(config_windows, frames):
            check(f, u)
        out.append(Candidate(CONFIG, config_windows, frames))
    if not out:
        raise ValueError("no candidate windows")
    if len(out) > dev_filter.FILTER_BANK_MAX_ROWS:
        raise ValueError(f"{len(out)} candidate rows, one bank launch takes {dev_filter.FILTER_BANK_MAX_ROWS}")
    return out


def _first_greatest(values):
    """Index of the greatest value, the first one on ties (float64, compared with >)."""
    best = 0
    for i in range(1, len(values)):
        if np.float64(values[i]) > np.float64(values[best]):
            best = i
    return best


@dataclass
class PostprocChoice:
    """What `PostprocSearch.best` returns: per class the window (in the YAML's unit and in frames) and, for the F1 objectives, the
    threshold; `per_class` the class's value under its choice, `overall` the value of the mixed choice (PSDS; macro F1, with
    `overall_micro`), `config_overall` the same for the "config" row when one was given (F1: at the first threshold)."""
    objective: str
    filter_type: str
    labels: list
    candidates: list
    windows_units: list
    windows_frames: list
    thresholds: Optional[list]
    per_class: list
    overall: float
    overall_micro: Optional[float] = None
    config_overall: Optional[float] = None

    def to_config(self):
        """The fragment of the recipe's `training:` section."""
        return {"median_window": list(self.windows_units), "filter_type": self.filter_type}

    def to_yaml(self):
        c = self.to_config()
        return f"training:\n  median_window: [{', '.join(str(u) for u in c['median_window'])}]\n  filter_type: {c['filter_type']}\n"

    def save(self, path):
        with open(path, "w") as f:
            json.dump(asdict(self), f, indent=1)

    @classmethod
    def load(cls, path):
        with open(path) as f:
            return cls(**json.load(f))


class PostprocSearch:
    """`update(strong [n, C, T], weak [n, C], paths)` per validation batch, then `results()` / `best(objective)`.

    `windows`: candidate windows in the YAML's unit (frames = int(u / 156 * T), T = `encoder.n_frames`); `config_windows`: the YAML's own
    list, searched as the row "config".  `objectives`: names of PSDS argument sets (`Evaluator.PSDS_ARGS`, replaced or extended by
    `psds_args` {name: IntersectionPSDS keywords}) and / or "event_f1", "segment_f1".  PSDS objectives follow the score-table path
    (`_scores_device`: soft weak scale with `weak_mask`, scipy median or max per `filter_types`); F1 objectives follow the event path
    (`_events_device`: hard mask weak >= theta, torch median, > theta) for every theta of `thresholds`, so their filter type is "median".
    Clips the ground truth does not list are left out of the F1 counts, as `Evaluator` leaves them out.

    The device steps are `_bank`, `_psds_accumulator` and `_f1_accumulator`: a subclass may replace them (a test without a GPU puts the
    scipy filters and the host sweeps there); everything else is host bookkeeping on their integers."""

    def __init__(self, encoder, ground_truth, audio_durations, *, windows=DEFAULT_WINDOWS, filter_types=("median", "max"),
                 objectives=("psds1", "psds2"), thresholds=(0.5,), weak_mask=False, config_windows=None, psds_args=None):
        self.encoder = encoder
        self.labels = list(encoder.labels)
        self.num_frames = int(encoder.n_frames)
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
        self.filter_types = [check_filter_type(f) for f in filter_types]
        if self.psds_objectives and not self.filter_types:
            raise ValueError("no filter type")
        self.thresholds = [float(t) for t in thresholds]
        if self.f1_objectives and not self.thresholds:
            raise ValueError("the F1 objectives need at least one threshold")
        self.weak_mask = bool(weak_mask)
        self.candidates = make_candidates(windows, self.num_frames, len(self.labels), config_windows, scipy=bool(self.psds_objectives))
        self._gt, self._dur = _table(ground_truth), _table(audio_durations)
        ts = frame_boundaries(encoder, self.num_frames)
        n_cand = len(self.candidates)
        self._psds = {(name, ft): [self._psds_accumulator(ts, args[name]) for _ in range(n_cand)]
                      for name in self.psds_objectives for ft in self.filter_types}
        self._f1 = [[self._f1_accumulator(ts) for _ in range(n_cand)] for _ in self.thresholds] if self.f1_objectives else []
        self._cache = {}

    # ---- the device steps
    def _bank(self, x, rows, mode, scale):
        """x [n, T, C] -> [W, n, T, C]: every candidate row's filter."""
        return dev_filter.filter_bank(x, rows, mode, scale)

    def _psds_accumulator(self, timestamps, args):
        return IntersectionPSDS(self._gt, self._dur, self.labels, timestamps, **args)

    def _f1_accumulator(self, timestamps):
        return EventSegmentF1(self._gt, self.labels, timestamps)

    @torch.no_grad()
    def update(self, strong, weak, paths):
        n, T, C = strong.shape[0], self.num_frames, len(self.labels)
        if n > len(paths):
            raise IndexError("list index out of range")     # (batched_decode_preds' contract)
        if strong.dim() != 3 or tuple(strong.shape[1:]) != (C, T):
            raise ValueError(f"strong must be [n, {C}, {T}]")
        if n == 0:
            return
        paths = list(paths[:n])
        self._cache = {}
        x = strong.detach().transpose(1, 2).contiguous().float()                    # [n, frames, n_class]
        rows = [c.frames for c in self.candidates]
        if self._psds:
            scale = weak[:n].detach().float() if (self.weak_mask and weak is not None) else None
            for ft in self.filter_types:
                bank = self._bank(x, rows, FILTER_MODES[ft], scale)
                for name in self.psds_objectives:
                    for ci, acc in enumerate(self._psds[(name, ft)]):
                        acc.update(bank[ci], paths)
        if self._f1:
            if weak is None:
                raise ValueError("the F1 objectives need the weak predictions (the event path masks with weak >= threshold)")
            known = self._f1[0][0]._clip_index
            keep = [i for i, f in enumerate(paths) if Path(f).stem in known]
            if not keep:
                return
            kept = [paths[i] for i in keep]
            for ti, th in enumerate(self.thresholds):
                mask = (weak[:n].detach() >= th).float()                            # output[b, :, c] = 0 where weak[b, c] < th
                active = self._bank(x, rows, 0, mask) > th
                if len(keep) != n:
                    idx = h2d(keep, torch.int64, active.device) if active.is_cuda else torch.as_tensor(keep, dtype=torch.int64)
                    active = active.index_select(1, idx)
                for ci, acc in enumerate(self._f1[ti]):
                    acc.update(active[ci], kept)

    # ---- finish: host arithmetic on the accumulators' integers
    def _psds_values(self, name, ft):
        """-> [(overall, [single-class value per class])] per candidate."""
        key = ("psds", name, ft)
        if key not in self._cache:
            out = []
            for acc in self._psds[(name, ft)]:
                overall, single = acc.compute()
                out.append((overall, [np.float64(single[c]) for c in self.labels]))
            self._cache[key] = out
        return self._cache[key]

    def _f1_counts(self):
        """-> [threshold][candidate] {count name: int64 [C]}."""
        if "f1" not in self._cache:
            self._cache["f1"] = [[acc.counts() for acc in per] for per in self._f1]
        return self._cache["f1"]

    def results(self):
        """One row per (objective, filter type, candidate[, threshold], class): DataFrame(objective, filter_type, candidate, frames,
        threshold, class, value) -- the single-class PSDS, or the class-wise F1."""
        rows = []
        for name in self.psds_objectives:
            for ft in self.filter_types:
                for cand, (_, single) in zip(self.candidates, self._psds_values(name, ft)):
                    rows += [(name, ft, cand.name, cand.frames[c], None, label, float(single[c])) for c, label in enumerate(self.labels)]
        for name in self.f1_objectives:
            counts = self._f1_counts()
            for ci, cand in enumerate(self.candidates):
                for ti, th in enumerate(self.thresholds):
                    f1 = EventSegmentF1.scores(counts[ti][ci])[name]
                    rows += [(name, "median", cand.name, cand.frames[c], th, label, float(f1[c])) for c, label in enumerate(self.labels)]
        return pd.DataFrame(rows, columns=["objective", "filter_type", "candidate", "frames", "threshold", "class", "value"])

    def overall(self, objective, filter_type="median", threshold=None):
        """{candidate name: overall value} of every single candidate row: the PSDS, or the macro F1 at `threshold` (default: the first)."""
        if objective in F1_OBJECTIVES:
            ti = 0 if threshold is None else self.thresholds.index(float(threshold))
            key = objective.replace("_f1", "_macro")
            return {c.name: EventSegmentF1.scores(cn)[key] for c, cn in zip(self.candidates, self._f1_counts()[ti])}
        return {c.name: v[0] for c, v in zip(self.candidates, self._psds_values(objective, filter_type))}

    def _config_index(self):
        return len(self.candidates) - 1 if self.candidates[-1].name == CONFIG else None

    def _best_psds(self, name, ft):
        values = self._psds_values(name, ft)
        C = len(self.labels)
        pick = [_first_greatest([v[1][c] for v in values]) for c in range(C)]
        accs = self._psds[(name, ft)]
        points = [accs[pick[c]].counts()[c] for c in range(C)]                      # class c's operating points under ITS window
        overall = accs[0].compute_points(points)[0]
        cfg = self._config_index()
        return PostprocChoice(objective=name, filter_type=ft, labels=list(self.labels), candidates=[self.candidates[p].name for p in pick],
                              windows_units=[self.candidates[p].units[c] for c, p in enumerate(pick)],
                              windows_frames=[self.candidates[p].frames[c] for c, p in enumerate(pick)], thresholds=None,
                              per_class=[float(values[p][1][c]) for c, p in enumerate(pick)], overall=float(overall),
                              config_overall=None if cfg is None else float(values[cfg][0]))

    def _best_f1(self, name):
        counts = self._f1_counts()
        C, n_th = len(self.labels), len(self.thresholds)
        f1 = [[EventSegmentF1.scores(counts[ti][ci])[name] for ti in range(n_th)] for ci in range(len(self.candidates))]
        pick = [divmod(_first_greatest([f1[ci][ti][c] for ci in range(len(self.candidates)) for ti in range(n_th)]), n_th)
                for c in range(C)]                                                  # candidates outer, thresholds inner
        mixed = {k: np.asarray([counts[ti][ci][k][c] for c, (ci, ti) in enumerate(pick)], dtype=np.int64) for k in F1_COUNTS}
        s = EventSegmentF1.scores(mixed)
        kind = name.replace("_f1", "")
        cfg = self._config_index()
        return PostprocChoice(objective=name, filter_type="median", labels=list(self.labels),
                              candidates=[self.candidates[ci].name for ci, _ in pick],
                              windows_units=[self.candidates[ci].units[c] for c, (ci, _) in enumerate(pick)],
                              windows_frames=[self.candidates[ci].frames[c] for c, (ci, _) in enumerate(pick)],
                              thresholds=[self.thresholds[ti] for _, ti in pick],
                              per_class=[float(f1[ci][ti][c]) for c, (ci, ti) in enumerate(pick)], overall=float(s[kind + "_macro"]),
                              overall_micro=float(s[kind + "_micro"]),
                              config_overall=None if cfg is None else float(EventSegmentF1.scores(counts[0][cfg])[kind + "_macro"]))

    def best(self, objective, filter_type=None):
        """Per class the candidate -- for the F1 objectives the (candidate, threshold) pair -- with the greatest value; the first in
        candidate order wins a tie (windows as given, "config" last, thresholds as given).  `filter_type=None`: the filter type whose
        composed overall value is greater, "median" on a tie."""
        if objective not in self.objectives:
            raise ValueError(f"objective {objective!r} was not searched ({self.objectives})")
        if objective in F1_OBJECTIVES:
            if filter_type not in (None, "median"):
                raise ValueError("the F1 objectives follow the event path: torch-semantics median only")
            return self._best_f1(objective)
        if filter_type is not None:
            if filter_type not in self.filter_types:
                raise ValueError(f"filter type {filter_type!r} was not searched ({self.filter_types})")
            return self._best_psds(objective, filter_type)
        order = sorted(self.filter_types, key=lambda f: f != "median")              # (stable: "median" first)
        choices = [self._best_psds(objective, ft) for ft in order]
        return choices[_first_greatest([c.overall for c in choices])]
