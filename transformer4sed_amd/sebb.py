"""Sound event bounding boxes by change detection (cSEBBs, after Ebbers et al. 2024) on the device: DESIGN.md section 7f.

Event extents are fixed once, by a step filter's change points and a greedy merge of neighbouring segments, and each box carries ONE
confidence (the mean score over its extent); sweeping the decision threshold then switches whole events on and off instead of moving
their edges.  The output is again a frame-score tensor [n, T, C] (a box's confidence on its frames, 0 elsewhere), so everything behind it
(`IntersectionPSDS`, `EventSegmentF1`, the score tables) takes it unchanged.  The definition is this project's own, exact in integers
(scores quantised to 2^-24), so the kernel (csrc/sebb.hip) and the host references of tests/sebb_cases.py agree bit for bit; parity with
the `sebbs` package is not pinned.  Timelines beyond 1024 frames (the long-form path) are out of scope.

  * `sebb_bank(x, rows, weak_scale=None)`     K parameter rows in one launch -> frame scores and boxes of every row
  * `SebbPostprocessor`                       one per-class parameter set: `scores`, `boxes`, `events`, `to_config`, `save` / `load`
  * `SebbSearch`                              `PostprocSearch` with the bank of a (step_filter_length, merge_threshold_abs,
                                              merge_threshold_rel) grid in place of the filter bank -> `SebbChoice`"""
import json
from collections import namedtuple
from dataclasses import asdict, dataclass
from typing import Optional

import numpy as np
import torch

from .evaluation.evaluator import Evaluator
from .ops import call, h2d
from .postproc_search import Candidate, PostprocSearch

SEBB_MAX_ROWS = 64             # csrc/sebb.hip: parameter rows of one launch
SEBB_MAX_FRAMES = 1024         # frames of a clip
Q = 1 << 24                    # the score quantum's reciprocal
RHO_Q = 256                    # merge_threshold_rel is quantised to 1 / 256, 1 .. 16
DEFAULT_STEP_FILTER_LENGTHS = (0.32, 0.48, 0.64)
DEFAULT_MERGE_THRESHOLDS_ABS = (0.15, 0.2, 0.3)
DEFAULT_MERGE_THRESHOLDS_REL = (1.5, 2.0, 3.0)

SebbBank = namedtuple("SebbBank", "scores boxes conf counts status")
"""scores [K, B, T, C] fp32; boxes [K, B, C, cap, 2] int32 (onset frame, offset frame); conf [K, B, C, cap] fp32; counts [K, B, C] int32, the
true number of boxes; status [2] int32: [0] some row had more than cap boxes (its first cap are there), [1] a score was clamped.  Box
slots from the count on are not initialised."""


def half_length(step_filter_length, frame_period):
    """Seconds of the whole step filter -> L, its half length in frames: max(1, floor(s / (2 p) + 0.5))."""
    return max(1, int(np.floor(float(step_filter_length) / (2.0 * float(frame_period)) + 0.5)))


def check_rows(rows, T, C):
    """The parameter rows of a bank [(L [C], tau [C], rho [C])] -> int32 array [K, C, 3] of (L, tau_q, rho_q), after the bounds: ValueError."""
    rows = list(rows)
    if not 1 <= len(rows) <= SEBB_MAX_ROWS:
        raise ValueError(f"sebb_bank takes 1 .. {SEBB_MAX_ROWS} parameter rows, got {len(rows)}")
    if not 1 <= T <= SEBB_MAX_FRAMES:
        raise ValueError(f"sebb_bank takes clips of 1 .. {SEBB_MAX_FRAMES} frames, got {T}: long-form timelines are out of scope")
    out = np.zeros((len(rows), C, 3), dtype=np.int32)
    for k, row in enumerate(rows):
        if len(row) != 3:
            raise ValueError("a parameter row is (L [C], tau [C], rho [C])")
        Ls, taus, rhos = (list(v) for v in row)
        if not len(Ls) == len(taus) == len(rhos) == C:
            raise ValueError(f"every list of a parameter row must hold one value per class ({C})")
        for c in range(C):
            L, tau, rho = Ls[c], float(taus[c]), float(rhos[c])
            if int(L) != L or not 1 <= int(L) <= (1 << 20):
                raise ValueError(f"step filter half length {L!r}: an integer number of frames, at least 1")
            if not 0.0 <= tau <= 1.0:
                raise ValueError(f"merge_threshold_abs {tau!r} must lie in [0, 1]")
            if not 1.0 <= rho <= 16.0:
                raise ValueError(f"merge_threshold_rel {rho!r} must lie in [1, 16]")
            out[k, c] = (int(L), int(np.rint(np.float64(tau) * Q)), int(np.rint(np.float64(rho) * RHO_Q)))
    return out


def check_scores(x, weak_scale=None):
    """NaN or out-of-range scores (after the weak scale) are refused: the integer definition covers [0, 1].  One read from the device."""
    bad = ~((x >= 0) & (x <= 1)).all()
    if weak_scale is not None:
        bad = bad | ~((weak_scale >= 0) & (weak_scale <= 1)).all()
    if bool(bad):
        raise ValueError("sebb: scores (and the weak scale) must lie in [0, 1] and hold no NaN")


def sebb_bank(x, rows, weak_scale=None, capacity=None, check=True):
    """x [B, T, C] fp32 in [0, 1], rows [K] of (L [C] frames, tau [C], rho [C]), weak_scale [B, C] or None (multiplied in, one fp32
    multiply, as the filter kernels do) -> `SebbBank`, every row from one launch that stages a (clip, class) column once and finds the
    candidate events once per distinct L (csrc/sebb.hip).  `capacity`: box slots per (row, clip, class); the default (T + 1) // 2 cannot
    overflow.  `check=False` skips the host's range check (the kernel then clamps and sets status[1])."""
    if x.dim() != 3:
        raise ValueError("input_tensor must have shape (Batch, Length, Classes)")
    B, T, C = x.shape
    params = check_rows(rows, T, C)
    cap = (T + 1) // 2 if capacity is None else int(capacity)
    if not 1 <= cap <= SEBB_MAX_FRAMES:
        raise ValueError(f"capacity must lie in [1, {SEBB_MAX_FRAMES}]")
    if weak_scale is not None and tuple(weak_scale.shape) != (B, C):
        raise ValueError(f"weak_scale must be [{B}, {C}]")
    x = x.contiguous().float()
    sc = None if weak_scale is None else weak_scale.contiguous().float()
    if check and B > 0:
        check_scores(x, sc)
    K, dev = len(params), x.device
    out = SebbBank(torch.empty((K, B, T, C), dtype=torch.float32, device=dev), torch.empty((K, B, C, cap, 2), dtype=torch.int32, device=dev),
                   torch.empty((K, B, C, cap), dtype=torch.float32, device=dev), torch.zeros((K, B, C), dtype=torch.int32, device=dev),
                   torch.zeros(2, dtype=torch.int32, device=dev))
    if B == 0:
        return out
    if not x.is_cuda:
        raise RuntimeError("sebb_bank needs tensors on an MI355X (HIP) device; there is no CPU path")
    call("sed_sebb_bank", x, sc, h2d(params, torch.int32, dev), out.scores, out.boxes, out.conf, out.counts, out.status, B, T, C, K, cap)
    return out


def box_lists(bank):
    """`SebbBank` -> [K][B][C] lists of (onset frame, offset frame, confidence) on the host; RuntimeError if a row overflowed its slots."""
    status = bank.status.cpu().numpy()
    if status[0]:
        raise RuntimeError("sebb_bank: more boxes than the capacity holds")
    boxes, conf, counts = bank.boxes.cpu().numpy(), bank.conf.cpu().numpy(), bank.counts.cpu().numpy()
    K, B, C = counts.shape
    return [[[[(int(boxes[k, b, c, i, 0]), int(boxes[k, b, c, i, 1]), float(conf[k, b, c, i])) for i in range(counts[k, b, c])]
              for c in range(C)] for b in range(B)] for k in range(K)]


def _per_class(value, C, what):
    v = list(value) if np.ndim(value) else [value] * C
    if len(v) != C:
        raise ValueError(f"{what}: one value or one per class ({C}), got {len(v)}")
    return [float(u) for u in v]


class SebbPostprocessor:
    """One SEBB parameter set, scalars or per-class lists: `step_filter_length` in seconds (the whole filter; the half length in frames
    follows from the encoder's frame period), `merge_threshold_abs` (tau), `merge_threshold_rel` (rho).  `Evaluator(..., sebb=this)` and
    `batched_decode_preds(..., sebb=this)` take it in place of the median / max filter."""

    KIND = "sebb"

    def __init__(self, encoder, step_filter_length=0.48, merge_threshold_abs=0.2, merge_threshold_rel=2.0):
        self.encoder = encoder
        self.labels = list(encoder.labels)
        C = len(self.labels)
        self.frame_period = float(encoder.net_pooling * encoder.frame_hop / encoder.sr)
        self.step_filter_length = _per_class(step_filter_length, C, "step_filter_length")
        self.merge_threshold_abs = _per_class(merge_threshold_abs, C, "merge_threshold_abs")
        self.merge_threshold_rel = _per_class(merge_threshold_rel, C, "merge_threshold_rel")
        if min(self.step_filter_length) <= 0:
            raise ValueError("step_filter_length must be positive")
        self.half_lengths = [half_length(s, self.frame_period) for s in self.step_filter_length]
        self.row = (self.half_lengths, self.merge_threshold_abs, self.merge_threshold_rel)
        check_rows([self.row], 1, C)

    # ---- device
    def scores_btc(self, x, scale=None, check=True):
        """x [n, T, C] (the score tables' layout), scale [n, C] or None -> [n, T, C]."""
        if x.shape[0] == 0:
            return x.contiguous().float()
        return sebb_bank(x, [self.row], scale, capacity=1, check=check).scores[0]     # (the scores do not depend on the box slots)

    @staticmethod
    def _btc(strong):
        if strong.dim() != 3:
            raise ValueError("strong must be [n, n_class, frames]")
        return strong.detach().transpose(1, 2).contiguous().float()

    def scores(self, strong, weak=None):
        """strong [n, C, T] (the model's layout), weak [n, C] or None (the soft weak mask) -> frame scores [n, T, C]."""
        return self.scores_btc(self._btc(strong), None if weak is None else weak.detach().float())

    def boxes(self, strong, weak=None):
        """-> [n][C] lists of (onset frame, offset frame, confidence)."""
        if strong.shape[0] == 0:
            return []
        return box_lists(sebb_bank(self._btc(strong), [self.row], None if weak is None else weak.detach().float()))[0]

    def events(self, strong, weak=None, threshold=0.5):
        """-> per clip an int32 array [m, 3] of (class, onset frame, offset frame), class-major, onsets ascending -- the rows
        `decode_events` gives for `scores(...)[i]` at `threshold` (one float or one per class): the boxes with confidence > threshold."""
        from .longform import _thresholds
        th = _thresholds(threshold, len(self.labels))
        return [np.asarray([(c, a, b) for c, per in enumerate(clip) for a, b, cf in per if np.float32(cf) > th[c]],
                           dtype=np.int32).reshape(-1, 3) for clip in self.boxes(strong, weak)]

    # ---- configuration
    def to_config(self):
        """The fragment of the recipe's `training:` section."""
        return {"sebb": {"step_filter_length": list(self.step_filter_length), "merge_threshold_abs": list(self.merge_threshold_abs),
                         "merge_threshold_rel": list(self.merge_threshold_rel)}}

    def save(self, path):
        with open(path, "w") as f:
            json.dump({"kind": self.KIND, "labels": self.labels, **self.to_config()["sebb"]}, f, indent=1)

    @classmethod
    def load(cls, path, encoder):
        """From what `save` or `SebbChoice.save` wrote; the classes must be the encoder's."""
        with open(path) as f:
            d = json.load(f)
        if d.get("kind") != cls.KIND:
            raise ValueError(f"{path} holds no SEBB parameters")
        if list(d["labels"]) != list(encoder.labels):
            raise ValueError(f"{path} was made for the classes {d['labels']}, the encoder's are {list(encoder.labels)}")
        return cls(encoder, d["step_filter_length"], d["merge_threshold_abs"], d["merge_threshold_rel"])


def is_sebb_file(path):
    with open(path) as f:
        return json.load(f).get("kind") == SebbPostprocessor.KIND


@dataclass
class SebbChoice:
    """What `SebbSearch.best` returns: per class the grid point and, for the F1 objectives, the threshold; `per_class` the class's value
    under its choice, `overall` the value of the mixed choice (PSDS; macro F1, with `overall_micro`)."""
    objective: str
    labels: list
    candidates: list
    step_filter_length: list
    merge_threshold_abs: list
    merge_threshold_rel: list
    half_lengths: list
    thresholds: Optional[list]
    per_class: list
    overall: float
    overall_micro: Optional[float] = None
    kind: str = SebbPostprocessor.KIND

    def to_config(self):
        return {"sebb": {"step_filter_length": list(self.step_filter_length), "merge_threshold_abs": list(self.merge_threshold_abs),
                         "merge_threshold_rel": list(self.merge_threshold_rel)}}

    def to_yaml(self):
        return "training:\n  sebb:\n" + "".join(f"    {k}: [{', '.join(str(u) for u in v)}]\n" for k, v in self.to_config()["sebb"].items())

    def postprocessor(self, encoder):
        return SebbPostprocessor(encoder, self.step_filter_length, self.merge_threshold_abs, self.merge_threshold_rel)

    def save(self, path):
        with open(path, "w") as f:
            json.dump(asdict(self), f, indent=1)

    @classmethod
    def load(cls, path):
        with open(path) as f:
            return cls(**json.load(f))


class SebbSearch(PostprocSearch):
    """`PostprocSearch` over a grid of SEBB parameters: the candidates are the points of `step_filter_lengths` x `merge_thresholds_abs` x
    `merge_thresholds_rel` (step filter length outermost; the default grid is 27 rows, one launch), the same for every class, and `_bank`
    is `sebb_bank`.  Objectives, accumulators, the per-class choice (the first greatest in grid order) and the composition of the mixed
    choice from integer counts are the parent's.  PSDS objectives take the scores with the soft weak scale (`weak_mask`), F1 objectives the
    hard mask weak >= theta and the boxes with confidence > theta.  The parent's one filter-type slot (`SLOT`) holds the SEBB tables;
    `results()` names it "sebb"."""

    SLOT = "median"

    def __init__(self, encoder, ground_truth, audio_durations, *, step_filter_lengths=DEFAULT_STEP_FILTER_LENGTHS,
                 merge_thresholds_abs=DEFAULT_MERGE_THRESHOLDS_ABS, merge_thresholds_rel=DEFAULT_MERGE_THRESHOLDS_REL,
                 objectives=("psds1", "psds2"), thresholds=(0.5,), weak_mask=False, psds_args=None):
        from .evaluation.codec import frame_boundaries
        from .evaluation.ground_truth import _table
        from .postproc_search import F1_OBJECTIVES
        self.encoder = encoder
        self.labels = list(encoder.labels)
        self.num_frames = int(encoder.n_frames)
        C = len(self.labels)
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
        self.filter_types = [self.SLOT]
        self.thresholds = [float(t) for t in thresholds]
        if self.f1_objectives and not self.thresholds:
            raise ValueError("the F1 objectives need at least one threshold")
        self.weak_mask = bool(weak_mask)
        period = float(encoder.net_pooling * encoder.frame_hop / encoder.sr)
        self.candidates = [Candidate(f"{s:g}/{tau:g}/{rho:g}", [(float(s), float(tau), float(rho))] * C, [half_length(s, period)] * C)
                           for s in step_filter_lengths for tau in merge_thresholds_abs for rho in merge_thresholds_rel]
        if not self.candidates:
            raise ValueError("no candidate parameters")
        if min(float(s) for s in step_filter_lengths) <= 0:
            raise ValueError("step_filter_length must be positive")
        self._rows = [(c.frames, [u[1] for u in c.units], [u[2] for u in c.units]) for c in self.candidates]
        check_rows(self._rows, self.num_frames, C)
        self._gt, self._dur = _table(ground_truth), _table(audio_durations)
        ts = frame_boundaries(encoder, self.num_frames)
        n_cand = len(self.candidates)
        self._psds = {(name, self.SLOT): [self._psds_accumulator(ts, args[name]) for _ in range(n_cand)] for name in self.psds_objectives}
        self._f1 = [[self._f1_accumulator(ts) for _ in range(n_cand)] for _ in self.thresholds] if self.f1_objectives else []
        self._cache = {}

    def _bank(self, x, rows, mode, scale):
        """x [n, T, C] -> [K, n, T, C]: every grid point's frame scores (`rows`, the half lengths alone, and the filter `mode` play no part)."""
        return sebb_bank(x, self._rows, scale, capacity=1).scores

    def results(self):
        table = super().results()
        table["filter_type"] = SebbPostprocessor.KIND
        return table

    def _choice(self, ch):
        return SebbChoice(objective=ch.objective, labels=ch.labels, candidates=ch.candidates,
                          step_filter_length=[u[0] for u in ch.windows_units], merge_threshold_abs=[u[1] for u in ch.windows_units],
                          merge_threshold_rel=[u[2] for u in ch.windows_units], half_lengths=ch.windows_frames, thresholds=ch.thresholds,
                          per_class=ch.per_class, overall=ch.overall, overall_micro=ch.overall_micro)

    def _best_psds(self, name, ft):
        return self._choice(super()._best_psds(name, ft))

    def _best_f1(self, name):
        return self._choice(super()._best_f1(name))
