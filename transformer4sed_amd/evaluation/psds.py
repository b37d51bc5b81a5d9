"""Intersection-based PSDS on the device (csrc/psds.hip), and the reference's entry points on top of it."""
import os
from pathlib import Path

import numpy as np
import torch

from ..ops import call
from .codec import write_sed_scores
from .ground_truth import ClipAccumulator, _microseconds, _table, build_ground_truth

PSDS_MAX_FRAMES = 1024         # csrc/psds.hip: frames per clip the sweep holds in LDS
PSDS_MAX_CLIP_EVENTS = 256     # ... and ground-truth events of one clip
PSDS_MAX_CT_CLASSES = 32       # ... and classes together with a cross-trigger threshold
PSDS_PADDED_CLASSES = 16       # up to here `update` keeps the sweep's padded event slots and reads nothing back
PSDS_BLOCK_CLIPS = 2048        # ... in storage allocated for this many clips at a time (the whole split, if it is smaller)
_PSDS_UNITS = {"second": 1.0, "minute": 60.0, "hour": 3600.0}


class IntersectionPSDS(ClipAccumulator):
    """Intersection-based polyphonic sound detection score (Bilen et al. 2020) over all score values (Ebbers et al. 2022), accumulated
    batch by batch from the post-processed frame scores the evaluation path leaves on the device.  DESIGN.md section 7b is the
    definition; parity with sed_scores_eval's own output is not pinned (the package is not available to compare with).

    `ground_truth` / `audio_durations`: TSV path or DataFrame (filename, onset, offset, event_label / filename, duration); clips are
    keyed by the filename's stem.  `timestamps` [T + 1]: the frame boundaries shared by all clips (`encoder._frame_to_time(arange(T + 1))`).
    `update(scores [n, T, C] fp32 device tensor, filenames, n_frames=None)` runs `sed_psds_sweep` (one wave per clip and class) and keeps
    the threshold events, never the scores.  With C <= 16 the events stay in the sweep's padded slots -- 8 bytes per frame and class, 16
    with a cross-trigger threshold -- and `update` never waits for the device; with more classes the slots that change no count are
    dropped right away, which costs one small count read-back per update.  `compute()` -> (psds, {class: single-class psds}),
    `roc()` -> the PSD-ROC and the per-class ROCs, `counts()` -> the cumulative integer counts behind them.

    Refused: T > 1024, a cross-trigger threshold together with more than 32 classes, a clip with more than 256 events
    (NotImplementedError); thresholds outside (0, 1], a class without a ground-truth event, a clip scored twice or unknown to
    `audio_durations`, NaN scores (at `compute`), ground-truth clips without scores (at `compute`) (ValueError)."""

    _unknown_clip = "audio_durations"

    def __init__(self, ground_truth, audio_durations, event_classes, timestamps, dtc_threshold, gtc_threshold, cttc_threshold=None,
                 alpha_ct=0, alpha_st=0, max_efpr=100, unit_of_time="hour"):
        C = self._set_classes(event_classes)
        for name, v in (("dtc_threshold", dtc_threshold), ("gtc_threshold", gtc_threshold), ("cttc_threshold", cttc_threshold)):
            if v is None and name == "cttc_threshold":
                continue
            if v is None or not 0.0 < float(v) <= 1.0:
                raise ValueError(f"{name} must lie in (0, 1], got {v!r}")
        if unit_of_time not in _PSDS_UNITS:
            raise ValueError(f"unit_of_time must be one of {sorted(_PSDS_UNITS)}")
        if not float(max_efpr) > 0:
            raise ValueError("max_efpr must be positive")
        d = self._set_timestamps(timestamps, PSDS_MAX_FRAMES, "HIP sweep")
        T = self.num_frames
        if cttc_threshold is not None and C > PSDS_MAX_CT_CLASSES:
            raise NotImplementedError(f"IntersectionPSDS: cttc_threshold with {C} classes (at most {PSDS_MAX_CT_CLASSES}; the "
                                      "AudioSet recipes pass None)")
        self.dtc, self.gtc = float(dtc_threshold), float(gtc_threshold)
        self.cttc = None if cttc_threshold is None else float(cttc_threshold)
        self.alpha_ct, self.alpha_st, self.max_efpr = float(alpha_ct), float(alpha_st), float(max_efpr)
        self.unit = _PSDS_UNITS[unit_of_time]
        if (d < 0).any():
            raise ValueError("timestamps must not decrease")
        self.t_pos = int(T if (d > 0).all() else np.argmin(d > 0))      # leading frames of positive duration: the ones that take part
        if (d[self.t_pos:] > 0).any():
            raise ValueError("a frame of zero duration lies before frames of positive duration")

        dur = _table(audio_durations)
        ids = [Path(f).stem for f in dur["filename"]]
        if len(set(ids)) != len(ids):
            raise ValueError("audio_durations lists a clip twice")
        self.data_us = int(_microseconds(dur["duration"].to_numpy()).sum())
        if self.data_us <= 0:
            raise ValueError("audio_durations sums to nothing")
        self._set_ground_truth(build_ground_truth(ground_truth, self.event_classes, ids, PSDS_MAX_CLIP_EVENTS, "IntersectionPSDS"))
        self.n_ref = np.bincount(self.gt[:, 0], minlength=C).astype(np.int64)
        self.class_us = np.bincount(self.gt[:, 0], weights=(self.gt[:, 2] - self.gt[:, 1]).astype(np.float64), minlength=C).astype(np.int64)
        if (self.n_ref == 0).any():
            raise ValueError("event classes without a ground-truth event (pass the classes of the ground truth only): "
                             f"{[c for c, n in zip(self.event_classes, self.n_ref) if n == 0]}")
        # cross-trigger term as ONE integer: sum_k CT_k ct_q[k], ct_q[k] = round(w_k / ct_unit), w_k = 1 / (T_k [s] (C - 1)).  The scale
        # leaves room for every detection of every clip (at most ceil(T / 2) per clip and class) cross-triggering every other class.
        self.ct_q, self.ct_unit = None, 0.0
        if self.cttc is not None:
            w = 1e6 / self.class_us.astype(np.float64) / max(C - 1, 1) if C > 1 else np.zeros(C)
            bound = len(ids) * ((T + 1) // 2) * max(C - 1, 1)
            self.ct_unit = float(w.max()) / 2.0 ** (62 - int(bound).bit_length()) if C > 1 else 1.0
            self.ct_q = np.rint(w / self.ct_unit).astype(np.int64)
        self._blocks = []                               # slot storage of the padded form: dict(cap, used, slots)
        self.reset()

    def reset(self):
        super().reset()
        self._chunks = []           # compacted events: (class int64, value f32, dTP int64, dFP int64, dCT int64 | None)
        self._padded = []           # the sweep's slots as they are: (value [n, C, T] f32, dTP int16, dFP int16, dCT int64 | None)
        self._points = None
        self._blocks = self._blocks[:1]
        for blk in self._blocks:
            blk["used"] = 0

    # ---- device half
    def _constants(self, dev):
        k, fresh = self._device_state(dev)
        if fresh:
            k["q"] = torch.from_numpy(self.ct_q).to(dev) if self.ct_q is not None else None
        return k

    def _sweep(self, scores, clip_index, n_frames):
        """scores [n, T, C] fp32 on the device -> the sweep's event slots (value f32, dTP int16, dFP int16, dCT int64 | None), each
        [n, C, T].  Stream-ordered: the clip rows travel through pinned memory, nothing is read back."""
        if not scores.is_cuda:
            raise RuntimeError("IntersectionPSDS needs scores on an MI355X (HIP) device; the sweep has no CPU path")
        k = self._constants(scores.device)
        n, T, C = scores.shape
        host = torch.tensor([clip_index] if n_frames is None or isinstance(n_frames, torch.Tensor)
                            else [clip_index, [int(v) for v in n_frames]], dtype=torch.int32)
        side = host.pin_memory().to(scores.device, non_blocking=True)
        nf = side[1] if side.shape[0] == 2 else n_frames
        if isinstance(nf, torch.Tensor):
            nf = nf.to(device=scores.device, dtype=torch.int32).contiguous()
        val, dtp, dfp, dct = self._slots(n, scores.device)
        call("sed_psds_sweep", scores, side[0], nf, k["ts"], self.t_pos, k["ptr"], k["cls"], k["on"], k["off"], k["q"], self.dtc, self.gtc,
             self.cttc if self.cttc is not None else -1.0, n, T, C, val, dtp, dfp, dct, self._status)
        return val, dtp, dfp, dct

    def _slots(self, n, dev):
        """Event slots for n more clips.  The padded form is kept until `compute`, so it lives in storage allocated once for the whole
        split and reused after `reset` (no trip to the device allocator per validation step); the many-class form is compacted and
        released right away."""
        T, C = self.num_frames, self.num_classes
        new = lambda rows: (torch.empty(rows, C, T, dtype=torch.float32, device=dev), torch.empty(rows, C, T, dtype=torch.int16, device=dev),
                            torch.empty(rows, C, T, dtype=torch.int16, device=dev),
                            torch.empty(rows, C, T, dtype=torch.int64, device=dev) if self.ct_q is not None else None)
        if C > PSDS_PADDED_CLASSES:
            return new(n)
        blk = self._blocks[-1] if self._blocks else None
        if blk is None or blk["used"] + n > blk["cap"]:
            cap = max(n, min(len(self.clip_ids), PSDS_BLOCK_CLIPS))
            blk = dict(cap=cap, used=0, slots=new(cap))
            self._blocks.append(blk)
        lo = blk["used"]
        blk["used"] += n
        return tuple(None if t is None else t[lo:lo + n] for t in blk["slots"])

    @staticmethod
    def _compact(val, dtp, dfp, dct):
        keep = (dtp != 0) | (dfp != 0)
        if dct is not None:
            keep |= dct != 0
        b, c, t = torch.nonzero(keep, as_tuple=True)
        return c, val[b, c, t], dtp[b, c, t].long(), dfp[b, c, t].long(), dct[b, c, t] if dct is not None else None

    def update(self, scores, filenames, n_frames=None):
        T, C = self.num_frames, self.num_classes
        if not isinstance(scores, torch.Tensor) or scores.dim() != 3 or tuple(scores.shape[1:]) != (T, C):
            raise ValueError(f"scores must be a [n, {T}, {C}] tensor")
        if scores.dtype != torch.float32:
            raise ValueError("scores must be fp32")
        n = scores.shape[0]
        if len(filenames) != n or (n_frames is not None and len(n_frames) != n):
            raise ValueError("one filename (and one n_frames entry) per clip")
        rows, batch = self._rows(filenames)
        if n == 0:
            return
        slots = self._sweep(scores.detach().contiguous(), rows, n_frames)
        self._seen |= batch
        self._points = None
        if C <= PSDS_PADDED_CLASSES:
            self._padded.append(slots)
        else:
            self._chunks.append(self._compact(*slots))

    # ---- finish: exact integer curves, then float64 rates
    def _check(self):
        missing = sorted(self._gt_clips - self._seen)
        if missing:
            raise ValueError(f"ground-truth clips without scores: {missing}")
        if self._status is not None:
            status = int(self._status.item())
            if status & 2:
                raise ValueError("Detected NaN values in the scores")
            if status & 8:
                raise ValueError("a clip's ground truth exceeds the sweep's event list")

    def counts(self):
        """Per class (in event_classes order) the operating points in descending score order, cumulative and exact: dict(value f32,
        tp, fp int64, ct int64 = sum_k CT_k ct_q[k]); events at one score value, from whatever clip or batch, are summed BEFORE the
        point exists.  Points that change no count are left out, the empty point (nothing detected) is implied."""
        if self._points is not None:
            return self._points
        self._check()
        self._chunks += [self._compact(*s) for s in self._padded]
        self._padded = []
        C = self.num_classes
        if not self._chunks or sum(ch[0].numel() for ch in self._chunks) == 0:
            z = np.zeros(0, dtype=np.int64)
            self._points = [dict(value=np.zeros(0, dtype=np.float32), tp=z, fp=z, ct=z) for _ in range(C)]
            return self._points
        has_ct = self.ct_q is not None
        cls, val, dtp, dfp = (torch.cat([ch[i] for ch in self._chunks]) for i in range(4))
        dct = torch.cat([ch[4] for ch in self._chunks]) if has_ct else torch.zeros_like(dtp)
        self._chunks = [(cls, val, dtp, dfp, dct if has_ct else None)]
        val = val + 0.0                                                     # -0.0 and +0.0 are one score value
        order = torch.sort(val, descending=True, stable=True).indices
        order = order[torch.sort(cls[order], stable=True).indices]        # by class, inside a class by descending value
        cls, val, dtp, dfp, dct = cls[order], val[order], dtp[order], dfp[order], dct[order]
        first = torch.ones_like(cls, dtype=torch.bool)
        first[1:] = (cls[1:] != cls[:-1]) | (val[1:] != val[:-1])
        seg = torch.cumsum(first, 0) - 1
        n_pts = int(seg[-1]) + 1
        pcls, pval = cls[first], val[first]
        out = []
        for d in (dtp, dfp, dct):
            s = torch.zeros(n_pts, dtype=torch.int64, device=d.device).index_add_(0, seg, d)       # equal values merge here
            tot = torch.zeros(C, dtype=torch.int64, device=d.device).index_add_(0, pcls, s)
            out.append(torch.cumsum(s, 0) - (torch.cumsum(tot, 0) - tot)[pcls])
        n_c = torch.bincount(pcls, minlength=C).cpu().tolist()
        host = [x.cpu().numpy() for x in (pval, *out)]
        self._points, lo = [], 0
        for n in n_c:
            v, tp, fp, ct = (x[lo:lo + n] for x in host)
            keep = np.ones(n, dtype=bool)
            keep[1:] = (tp[1:] != tp[:-1]) | (fp[1:] != fp[:-1]) | (ct[1:] != ct[:-1])          # merged deltas that cancelled
            if n:
                keep[0] = bool(tp[0] or fp[0] or ct[0])
            self._points.append(dict(value=v[keep], tp=tp[keep], fp=fp[keep], ct=ct[keep]))
            lo += n
        return self._points

    def _class_rocs(self, points=None):
        """Per class the staircase (eFPR ascending, running-maximum TPR), float64, with the empty point first; `points`: operating
        points in `counts()`'s form instead of this accumulator's own."""
        rocs = []
        for c, p in enumerate(self.counts() if points is None else points):
            tpr = np.concatenate(([0.0], p["tp"].astype(np.float64) / float(self.n_ref[c])))
            efpr = np.concatenate(([0.0], (p["fp"].astype(np.float64) / (self.data_us / 1e6)
                                           + self.alpha_ct * (p["ct"].astype(np.float64) * self.ct_unit)) * self.unit))
            order = np.lexsort((-tpr, efpr))                    # by eFPR; at equal eFPR the larger TPR first
            rocs.append((efpr[order], np.maximum.accumulate(tpr[order])))
        return rocs

    @staticmethod
    def _area(e, y, m):
        e = np.minimum(e, m)
        return float(np.sum(y * np.diff(np.concatenate((e, [m]))))) / m

    def _psd_roc(self, rocs):
        m = self.max_efpr
        grid = np.unique(np.concatenate([e[e <= m] for e, _ in rocs]))
        eff = np.empty_like(grid)
        for lo in range(0, grid.size, 1 << 14):                 # (a [C, grid] slab at a time: 407 classes meet a long grid)
            g = grid[lo:lo + (1 << 14)]
            ys = np.stack([y[np.searchsorted(e, g, side="right") - 1] for e, y in rocs])
            eff[lo:lo + g.size] = np.maximum(ys.mean(0) - self.alpha_st * ys.std(0), 0.0)
        return grid, eff

    def compute(self):
        return self.compute_points(None)

    def compute_points(self, points):
        """`compute()` on operating points given per class in `counts()`'s form (None: this accumulator's own) -- class c's points may
        come from another accumulator of the same ground truth and arguments that was fed other scores (a class's points depend on that
        class's scores alone: `PostprocSearch` composes a per-class choice this way instead of running the sweep again)."""
        rocs = self._class_rocs(points)
        grid, eff = self._psd_roc(rocs)
        single = {c: self._area(e, y, self.max_efpr) for c, (e, y) in zip(self.event_classes, rocs)}
        return self._area(grid, eff, self.max_efpr), single

    def roc(self):
        """-> ((efpr, effective tpr) of the PSD-ROC, {class: (efpr, tpr)}): staircases, each value holding up to the next eFPR."""
        rocs = self._class_rocs()
        grid, eff = self._psd_roc(rocs)
        return (grid, eff), {c: r for c, r in zip(self.event_classes, rocs)}


def compute_psds_from_scores(scores, ground_truth_file, durations_file, dtc_threshold=0.5, gtc_threshold=0.5, cttc_threshold=0.3,
                             alpha_ct=0, alpha_st=0, max_efpr=100, num_jobs=4, save_dir=None):
    """src/evaluation_measures.py:299-341 on `IntersectionPSDS`: `scores` is a dict audio_id -> score DataFrame as `batched_decode_preds`
    returns them (all with the same frames and classes); they are uploaded and swept on the device.  -> (psds, single_class_psds).
    `save_dir` writes the score tables (`write_sed_scores`); the reference's ROC plot is left out.  `num_jobs` is accepted and ignored."""
    if not scores:
        raise ValueError("no scores")
    keys = list(scores)
    first = scores[keys[0]]
    classes = list(first.columns[2:])
    ts = np.concatenate((first["onset"].to_numpy(), first["offset"].to_numpy()[-1:]))
    for k in keys:
        df = scores[k]
        if list(df.columns[2:]) != classes or len(df) != len(first) or not np.array_equal(df["onset"].to_numpy(), ts[:-1]):
            raise ValueError(f"score table {k!r} differs from {keys[0]!r} in classes or frames")
    acc = IntersectionPSDS(ground_truth_file, durations_file, classes, ts, dtc_threshold, gtc_threshold, cttc_threshold, alpha_ct,
                           alpha_st, max_efpr)
    x = torch.from_numpy(np.stack([scores[k][classes].to_numpy(dtype=np.float32) for k in keys]))
    dev = torch.device("cuda") if torch.cuda.is_available() else x.device     # (without a HIP device the sweep itself refuses)
    for s in range(0, len(keys), 64):
        acc.update(x[s:s + 64].to(dev), keys[s:s + 64])
    res = acc.compute()
    if save_dir is not None:
        write_sed_scores(scores, os.path.join(save_dir, "scores"))
    return res


def mean_psds_per_type(single_psds, type_dict):
    """passt_cnn/train.py:223-237: mean of the per-class PSDS of each class type ({"common": .., "rare": ..}) -- of the single-class
    dict `IntersectionPSDS.compute` / `AudiosetStrongEvaluator.psds` return."""
    ret = {category: [] for category in set(type_dict.values())}
    for event, psds in single_psds.items():
        ret[type_dict[event]].append(psds)
    return {category: sum(v) / len(v) for category, v in ret.items()}
