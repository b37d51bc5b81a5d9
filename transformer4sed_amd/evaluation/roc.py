"""ROC area on the device: the multilabel AUROC / d' beside the mAP (csrc/metrics.hip: sed_roc_compute) and the
segment-based partial AUROC of DCASE 2024 Task 4's MAESTRO half (csrc/segment_pool.hip), with the reference's segment functions
(src/codec/decoder.py:106-230) on top.  The device returns integers; the scores are finished here in float64."""
import math
import warnings
from collections import defaultdict
from pathlib import Path

import numpy as np
import torch

from ..ops import call, h2d
from .codec import create_score_dataframe
from .ground_truth import ClipAccumulator, _microseconds, _table, build_ground_truth
from .metrics import AP_CHUNK, ClassMajorScores

# include/sed_hip.h (tests/test_roc_cpu.py compares)
SED_ROC_OUT = 8
SED_ROC_MAX_CHUNK = 20000
SED_SEG_STATUS_WORDS = 4
SED_SEG_ZERO_WEIGHT, SED_SEG_NAN, SED_SEG_BAD_ROW, SED_SEG_LONG_LIST = range(4)

ROC_INTS = ("P", "Nn", "auc2", "area2", "fp_a", "tp_a", "fp_b", "tp_b")
NORMALIZE = ("max_fpr", "mcclish")


def _check_fpr(max_fpr, normalize):
    if max_fpr is not None and not 0.0 < float(max_fpr) <= 1.0:
        raise ValueError(f"max_fpr must lie in (0, 1], got {max_fpr!r}")
    if normalize not in NORMALIZE:
        raise ValueError(f"normalize must be one of {NORMALIZE}, got {normalize!r}")
    return None if max_fpr is None else float(max_fpr)


def roc_integers(scores, labels, N, max_fpr=None, chunk=AP_CHUNK):
    """`sed_roc_compute` on class-major storage: scores [C][cap] fp32, labels [C][cap] uint8 (device), items 0 .. N-1
    -> int64 [C][8] = P, Nn, auc2, area2, fp_a, tp_a, fp_b, tp_b on the device."""
    C, cap = scores.shape
    dev = scores.device
    nch = (N + chunk - 1) // max(chunk, 1)
    a_sorted = p_sorted = pos_cnt = scratch = None
    if nch > 1:
        a_sorted = torch.empty(C * nch * chunk, dtype=torch.int32, device=dev)
        p_sorted = torch.empty(C * nch * chunk, dtype=torch.int32, device=dev)
        pos_cnt = torch.empty(C * nch, dtype=torch.int32, device=dev)
        scratch = torch.empty(C * (2 * nch + 1), dtype=torch.int64, device=dev)
    out = torch.empty(C, SED_ROC_OUT, dtype=torch.int64, device=dev)
    call("sed_roc_compute", scores, labels, C, N, cap, chunk, 1.0 if max_fpr is None else float(max_fpr), a_sorted, p_sorted, pos_cnt,
         scratch, out)
    return out


def roc_scores(ints, max_fpr=None, normalize="mcclish"):
    """The float64 finish of section 7g.  ints: int64 [C][8] -> (auroc [C], pauc [C]); pauc is the area left of max_fpr normalised as
    `normalize` says (the AUROC itself without max_fpr); NaN for a class without a positive or without a negative."""
    v = np.asarray(ints, dtype=np.int64).astype(np.float64)
    P, Nn, auc2, area2, fp_a, tp_a, fp_b, tp_b = v.T
    with np.errstate(invalid="ignore", divide="ignore"):
        den = P * Nn
        auroc = np.where(den > 0, auc2 / (2.0 * den), np.nan)
        if max_fpr is None:
            return auroc, auroc.copy()
        x = max_fpr * Nn
        dfp = fp_b - fp_a
        tp_x = tp_a + np.where(dfp > 0, (tp_b - tp_a) * (x - fp_a) / np.where(dfp > 0, dfp, 1.0), 0.0)
        raw = (area2 / 2.0 + (x - fp_a) * (tp_a + tp_x) / 2.0) / den
        if normalize == "max_fpr":
            pauc = raw / max_fpr
        else:
            lo = max_fpr * max_fpr / 2.0
            pauc = 0.5 * (1.0 + (raw - lo) / (max_fpr - lo)) if max_fpr < 1.0 else raw
        return auroc, np.where(den > 0, pauc, np.nan)


def _mean(values, weights, what, average):
    """Macro / weighted mean over the classes that have a value, with torchmetrics' warning for the others."""
    nan = np.isnan(values)
    if nan.any():
        warnings.warn(f"{what} for one or more classes was `nan`. Ignoring these classes in {average}-average", UserWarning)
    ok = ~nan
    if not ok.any():
        return float("nan")
    if average == "weighted":
        w = weights[ok].astype(np.float64)
        return float((values[ok] * w).sum() / w.sum()) if w.sum() > 0 else 0.0
    return float(values[ok].mean())


def d_prime(auroc):
    """d' = sqrt(2) * ndtri(AUROC), float64."""
    return math.sqrt(2.0) * torch.special.ndtri(torch.as_tensor(auroc, dtype=torch.float64))


class MultilabelAUROC(ClassMajorScores):
    """torchmetrics' `MultilabelAUROC(num_labels, average, thresholds=None)` on HIP kernels, with a partial area: `update` / `__call__` /
    `reset` / `to` and the storage are `MultilabelAveragePrecision`'s (one stream-ordered append per batch, the per-batch sigmoid rule,
    no wait for the device), `compute()` sorts it with `sed_roc_compute` and finishes in float64.

    `max_fpr`: None for the whole area, or the false-positive rate in (0, 1] the area stops at; `normalize`: "mcclish" (what
    `sklearn.metrics.roc_auc_score(max_fpr=)` returns) or "max_fpr" (area / max_fpr).  `average`: "macro", "weighted" (weights = positives
    per class), None / "none"; a class without a positive or without a negative scores NaN and is left out of both averages with a
    warning.  `compute()` -> float64 tensor on the storage's device; `per_class()` -> the int64 [C][8] integers of section 7g (device);
    `d_prime()` -> sqrt(2) ndtri(AUROC) of the whole area, averaged as `average` says before the transform.

    Refused: average="micro", thresholds (a binned curve), ignore_index (NotImplementedError); what torchmetrics' validation rejects, at
    `compute` (RuntimeError)."""

    def __init__(self, num_labels, average="macro", thresholds=None, ignore_index=None, validate_args=True, *, max_fpr=None,
                 normalize="mcclish", chunk=AP_CHUNK):
        if average == "micro":
            raise NotImplementedError("MultilabelAUROC: average='micro' is not implemented on the HIP path")
        if average not in ("macro", "weighted", "none", None):
            raise ValueError(f"Expected argument `average` to be one of ('macro', 'weighted', 'none', None), but got {average}")
        if thresholds is not None or ignore_index is not None:
            raise NotImplementedError("MultilabelAUROC: thresholds and ignore_index are not implemented on the HIP path")
        self.max_fpr = _check_fpr(max_fpr, normalize)
        self.normalize = normalize
        self.num_labels, self.average, self.chunk = int(num_labels), average, int(chunk)
        self.device = None
        self.reset()

    def per_class(self):
        self._checked()
        return roc_integers(self.scores, self.labels, self.n, self.max_fpr, self.chunk)

    def _finish(self, values, positives):
        if self.average in (None, "none"):
            return torch.from_numpy(values).to(self.device)
        return torch.tensor(_mean(values, positives, "AUROC score", self.average), dtype=torch.float64, device=self.device)

    def compute(self):
        ints = self.per_class().cpu().numpy()
        return self._finish(roc_scores(ints, self.max_fpr, self.normalize)[1], ints[:, 0])

    def d_prime(self):
        ints = self.per_class().cpu().numpy()
        return d_prime(self._finish(roc_scores(ints)[0], ints[:, 0]))


def storage_auroc(store, max_fpr=None):
    """`AudiosetStrongEvaluator.compute_auroc`: the macro AUROC (standardised partial area with `max_fpr`), d' of the macro whole-area
    AUROC and the integers, from a `ClassMajorScores` as it stands -- no copy of it is made."""
    max_fpr = _check_fpr(max_fpr, "mcclish")
    store._checked()
    ints = roc_integers(store.scores, store.labels, store.n, max_fpr, store.chunk).cpu().numpy()
    auroc, pauc = roc_scores(ints, max_fpr, "mcclish")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        whole = _mean(auroc, ints[:, 0], "AUROC score", "macro")
    return {"auroc": _mean(pauc, ints[:, 0], "AUROC score", "macro"), "d_prime": float(d_prime(whole)), "per_class": ints}


# ---------------------------------------------------------------------------------------------------- segments
def segment_weights(ts_us, clip_us, seg_us):
    """int64 [n_seg][T]: w_f of every frame in every segment of a clip of `clip_us` microseconds (section 7g)."""
    ts = np.asarray(ts_us, dtype=np.int64)
    n_seg = -(-int(clip_us) // int(seg_us))
    start = np.arange(n_seg, dtype=np.int64)[:, None] * int(seg_us)
    return np.maximum(0, np.minimum(ts[None, 1:], start + int(seg_us)) - np.maximum(ts[None, :-1], start))


def segment_targets(gt, gt_ptr, dur_us, seg_us, num_classes):
    """File segment k is positive for class c iff an event of c has onset < min((k + 1) Ls, d) and offset > k Ls (integer us).
    gt / gt_ptr: `build_ground_truth`'s arrays over the files of `dur_us`.  -> (uint8 [C][S_total], seg_ptr int64 [n_files + 1])."""
    n_seg = -(-np.asarray(dur_us, dtype=np.int64) // int(seg_us))
    seg_ptr = np.concatenate(([0], np.cumsum(n_seg))).astype(np.int64)
    target = np.zeros((num_classes, int(seg_ptr[-1])), dtype=np.uint8)
    for i, d in enumerate(np.asarray(dur_us, dtype=np.int64).tolist()):
        for c, on, off in gt[gt_ptr[i]:gt_ptr[i + 1]].tolist():
            k0 = max(on, 0) // seg_us                                    # segments k with onset < (k + 1) Ls
            k1 = min(-(-min(off, d) // seg_us), int(n_seg[i]))          # segments k with k Ls < offset (and below the file's end)
            if on < d and k1 > k0:
                target[c, seg_ptr[i] + k0:seg_ptr[i] + k1] = 1
    return target, seg_ptr


def _durations(audio_durations):
    if isinstance(audio_durations, dict):
        return [Path(str(f)).stem for f in audio_durations], _microseconds(list(audio_durations.values()))
    dur = _table(audio_durations)
    return [Path(f).stem for f in dur["filename"]], _microseconds(dur["duration"].to_numpy())


class SegmentAUROC(ClipAccumulator):
    """Segment-based partial AUROC (the mpAUC that src/utils/validate_submissions.py:111 asks for on MAESTRO) from frame scores on the
    device: duration-weighted pooling of a clip's frames into segments of `segment_length`, overlap-add of sliding clips into their file
    (src/codec/decoder.py:138-230), a segment ground truth, and `sed_roc_compute` over the file segments.  DESIGN.md section 7g is the
    definition.

    `ground_truth` / `audio_durations`: TSV path or DataFrame (filename, onset, offset, event_label / filename, duration), files keyed by
    the filename's stem; `audio_durations` may be a dict {file: seconds}.  `timestamps` [T + 1]: the frame boundaries every clip shares.
    `clip_ids`: "file" (a clip is a whole file) or "sliding" (a clip is named "{file}-{100 onset}-{100 offset}", decoder.py:109,169).
    `update(scores [n, T, C] device tensor, filenames)` pools on the current stream and never waits for the device.
    `segment_scores()` -> {file: DataFrame} in `create_score_dataframe`'s layout for the files scored so far; `counts()` -> int64 [C][8];
    `compute()` -> {"mpauc", "auroc", "per_class"}: the macro means of the partial area (normalised as `normalize` says) and of the whole
    area over the classes that have both a positive and a negative segment.

    Refused (ValueError): a clip of a file `audio_durations` does not list, a clip id seen twice, a clip whose segments run past its
    file's, a geometry in which some segment overlaps no frame, timestamps that decrease, files without a clip (at `counts`), NaN scores
    (at `counts` / `segment_scores`)."""

    _unknown_clip = "audio_durations"

    def __init__(self, ground_truth, audio_durations, event_classes, timestamps, segment_length=1.0, max_fpr=0.1, normalize="max_fpr",
                 clip_ids="file", chunk=AP_CHUNK):
        C = self._set_classes(event_classes)
        if clip_ids not in ("file", "sliding"):
            raise ValueError("clip_ids must be 'file' or 'sliding'")
        self.mode, self.chunk = clip_ids, int(chunk)
        self.max_fpr = _check_fpr(max_fpr, normalize)
        self.normalize = normalize
        self.seg_us = int(_microseconds(segment_length))
        if self.seg_us <= 0:
            raise ValueError("segment_length must be a positive number of microseconds")
        if (self._set_timestamps(timestamps, 1 << 24, "pooling kernel") < 0).any():
            raise ValueError("timestamps must not decrease")
        ids, self.dur_us = _durations(audio_durations)
        if len(set(ids)) != len(ids):
            raise ValueError("audio_durations lists a file twice")
        if (self.dur_us <= 0).any():
            raise ValueError("audio_durations holds a file without a duration")
        self._set_ground_truth(build_ground_truth(ground_truth, self.event_classes, ids, None, "SegmentAUROC"))
        self.target, self.seg_ptr = segment_targets(self.gt, self.gt_ptr, self.dur_us, self.seg_us, C)
        self._good_len = set()          # clip lengths whose every segment overlaps a frame
        self._pooled, self._cap = None, 0
        self.reset()

    def reset(self):
        super().reset()
        self._clips = []                # (file row, onset_us, first pooled row, segments), in arrival order
        self._used = 0

    # ---- device half
    def _parse(self, name):
        """-> (clip id, file row, onset_us, length_us)."""
        a = Path(name).stem
        if self.mode == "file":
            file, onset, length = a, 0, None
        else:
            try:
                file, on, off = a.rsplit("-", 2)
                onset, length = int(on) * 10000, (int(off) - int(on)) * 10000
            except ValueError:
                raise ValueError(f"clip id {a!r} is not '{{file}}-{{100 onset}}-{{100 offset}}'") from None
            if length <= 0 or onset < 0:
                raise ValueError(f"clip {a!r} has no length or a negative onset")
        if file not in self._clip_index:
            raise ValueError(f"clip {a!r} is missing from {self._unknown_clip}")
        row = self._clip_index[file]
        return a, row, onset, int(self.dur_us[row]) if length is None else length

    def _check_geometry(self, length):
        if length not in self._good_len:
            if (segment_weights(self.ts_us, length, self.seg_us).sum(1) <= 0).any():
                raise ValueError(f"a clip of {length} us has a segment of {self.seg_us} us that overlaps no frame")
            self._good_len.add(length)

    def _grow(self, need, dev):
        cap = max(need, 2 * self._cap, 256)
        pooled = torch.empty(cap, self.num_classes, dtype=torch.float32, device=dev)
        if self._pooled is not None and self._used:
            pooled[:self._used].copy_(self._pooled[:self._used])
        self._pooled, self._cap = pooled, cap

    def update(self, scores, filenames):
        T, C = self.num_frames, self.num_classes
        if not isinstance(scores, torch.Tensor) or scores.dim() != 3 or tuple(scores.shape[1:]) != (T, C):
            raise ValueError(f"scores must be a [n, {T}, {C}] tensor")
        if len(filenames) != scores.shape[0]:
            raise ValueError("one filename per clip")
        clips, batch, used = [], set(), self._used
        for f in filenames:
            a, row, onset, length = self._parse(f)
            if a in self._seen or a in batch:
                raise ValueError(f"clip {a!r} was scored twice")
            batch.add(a)
            self._check_geometry(length)
            n_seg = -(-length // self.seg_us)
            first = onset // self.seg_us
            if first + n_seg > self.seg_ptr[row + 1] - self.seg_ptr[row]:
                raise ValueError(f"clip {a!r} runs past the {int(self.seg_ptr[row + 1] - self.seg_ptr[row])} segments of its file")
            clips.append((row, onset, used, n_seg, length))
            used += n_seg
        if not scores.is_cuda:
            raise RuntimeError("SegmentAUROC needs scores on an MI355X (HIP) device; the pooling has no CPU path")
        if not clips:
            return
        dev = scores.device
        if self._status is None:
            self._dev = dict(device=dev, ts=h2d(self.ts_us, torch.int64, dev))
            self._status = torch.zeros(SED_SEG_STATUS_WORDS, dtype=torch.int32, device=dev)
        elif self._dev["device"] != dev:
            raise ValueError(f"batches on different devices ({self._dev['device']}, {dev})")
        if used > self._cap:
            self._grow(used, dev)
        side = h2d(np.array([[c[4] for c in clips], [c[2] for c in clips]], dtype=np.int64), torch.int64, dev)
        call("sed_segment_pool", scores.detach().to(torch.float32).contiguous(), self._dev["ts"], side[0], side[1].to(torch.int32),
             self.seg_us, len(clips), T, C, max(c[3] for c in clips), self._cap, self._pooled, self._status)
        self._clips += [c[:4] for c in clips]
        self._used = used
        self._seen |= batch

    def _file_scores(self):
        """-> scores [C][S_total] fp32 on the device (files without a clip score 0)."""
        if not self._clips:
            raise RuntimeError(f"{type(self).__name__}: no clip was scored")
        dev = self._dev["device"]
        S = int(self.seg_ptr[-1])
        entries = sorted((int(self.seg_ptr[row]) + onset // self.seg_us + k, onset, i, first + k)
                         for i, (row, onset, first, n_seg) in enumerate(self._clips) for k in range(n_seg))
        seg = np.array([e[0] for e in entries], dtype=np.int64)
        ptr = np.searchsorted(seg, np.arange(S + 1)).astype(np.int32)
        rows = np.array([e[3] for e in entries], dtype=np.int32)
        out = torch.empty(self.num_classes, S, dtype=torch.float32, device=dev)
        call("sed_segment_gather", self._pooled, h2d(ptr, torch.int32, dev), h2d(rows, torch.int32, dev), S, self.num_classes, self._used,
             len(rows), int(np.diff(ptr).max()), S, out, self._status)
        status = self._status.cpu().numpy()
        if status[SED_SEG_NAN]:
            raise ValueError(f"{type(self).__name__}: NaN scores")
        if status.any():
            raise RuntimeError(f"{type(self).__name__}: the pooling kernels report {status.tolist()} (include/sed_hip.h: SED_SEG_*)")
        return out

    def segment_scores(self):
        host = self._file_scores().cpu().numpy()
        out = {}
        for row in sorted({c[0] for c in self._clips}):
            lo, hi = int(self.seg_ptr[row]), int(self.seg_ptr[row + 1])
            d = self.dur_us[row] / 1e6
            ts = np.minimum(np.arange(hi - lo + 1) * (self.seg_us / 1e6), d)
            out[self.clip_ids[row]] = create_score_dataframe(host[:, lo:hi].T.astype(np.float64), ts, self.event_classes)
        return out

    def counts(self):
        """int64 [C][8] = P, Nn, auc2, area2, fp_a, tp_a, fp_b, tp_b over the segments of every file."""
        missing = sorted(set(self.clip_ids) - {self.clip_ids[c[0]] for c in self._clips})
        if missing:
            raise ValueError(f"files without scores: {missing}")
        scores = self._file_scores()
        labels = torch.from_numpy(self.target).to(scores.device)
        return roc_integers(scores, labels, scores.shape[1], self.max_fpr, self.chunk).cpu().numpy()

    def compute(self):
        ints = self.counts()
        auroc, pauc = roc_scores(ints, self.max_fpr, self.normalize)
        return {"mpauc": _mean(pauc, ints[:, 0], "Partial AUROC", "macro"), "auroc": _mean(auroc, ints[:, 0], "AUROC", "macro"),
                "per_class": {name: {"pauc": float(pauc[i]), "auroc": float(auroc[i]), **{k: int(ints[i, j]) for j, k in enumerate(ROC_INTS)}}
                              for i, name in enumerate(self.event_classes)}}


# ---------------------------------------------------------------------------------------------------- the reference's functions
def _frame_table(scores_df):
    """-> (timestamps [T + 1], event classes, scores [T, C]) of a score DataFrame (onset, offset, classes)."""
    cols = list(scores_df.columns)
    if cols[:2] != ["onset", "offset"] or len(cols) < 3 or len(scores_df) == 0:
        raise ValueError("a score DataFrame has the columns onset, offset and one per event class, and a row per frame")
    on, off = scores_df["onset"].to_numpy(dtype=np.float64), scores_df["offset"].to_numpy(dtype=np.float64)
    if not np.array_equal(on[1:], off[:-1]):
        raise ValueError("the frames of a score DataFrame must follow each other")
    return np.concatenate((on, off[-1:])), cols[2:], scores_df[cols[2:]].to_numpy(dtype=np.float32)


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("segment pooling needs an MI355X (HIP) device; it has no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def get_segment_scores(scores_df, clip_length, segment_length=1.):
    """src/codec/decoder.py:193-230: the frame scores of one clip pooled into segments (upload, `sed_segment_pool`, download)."""
    ts, classes, arr = _frame_table(scores_df)
    acc = SegmentAUROC(_empty_ground_truth(), {"clip": float(clip_length)}, classes, ts, segment_length)
    acc.update(torch.from_numpy(arr[None]).to(_device()), ["clip"])
    df = acc.segment_scores()["clip"]
    df.loc[df.index[-1], "offset"] = float(clip_length)
    return df


def get_segment_scores_and_overlap_add(frame_scores, audio_durations, event_classes, segment_length=1.):
    """src/codec/decoder.py:138-190: {"{file}-{100 onset}-{100 offset}": score DataFrame} -> {file: segment score DataFrame}.  The
    reference pools with a hard-coded segment_length of 1 whatever it is given (decoder.py:178); `segment_length` is used throughout here."""
    event_classes = list(event_classes)
    ts, arrs = None, []
    for clip_id, df in frame_scores.items():
        t, _, _ = _frame_table(df[["onset", "offset"] + event_classes])
        if ts is not None and not np.array_equal(t, ts):
            raise ValueError("the clips must share their frame boundaries")
        ts = t
        arrs.append(df[event_classes].to_numpy(dtype=np.float32))
    if ts is None:
        return {}
    acc = SegmentAUROC(_empty_ground_truth(), dict(audio_durations), event_classes, ts, segment_length, clip_ids="sliding")
    acc.update(torch.from_numpy(np.stack(arrs)).to(_device()), list(frame_scores))
    return acc.segment_scores()


def _empty_ground_truth():
    import pandas as pd
    return pd.DataFrame({"filename": [], "onset": [], "offset": [], "event_label": []})


def merge_overlapping_events(ground_truth_events):
    """src/codec/decoder.py:118-135 (host only): per file and class, events that overlap or touch become one.  {file: [(onset, offset,
    class), ...]} -> the same dict with [onset, offset, class] lists, classes in order of first appearance."""
    for file_id, events in ground_truth_events.items():
        by_class = defaultdict(list)
        for ev in events:
            by_class[ev[2]].append(ev)
        merged = []
        for evs in by_class.values():
            last = None
            for ev in sorted(evs):
                if last is not None and ev[0] <= last[1]:
                    last[1] = max(last[1], ev[1])
                else:
                    last = list(ev)
                    merged.append(last)
        ground_truth_events[file_id] = merged
    return ground_truth_events


def merge_maestro_ground_truth(clip_ground_truth):
    """src/codec/decoder.py:106-115 (host only): the events of "{file}-{100 onset}-{100 offset}" clips shifted by the clip's onset in
    whole seconds (`int(onset) // 100`, as the reference has it), gathered per file and merged."""
    files = defaultdict(list)
    for clip_id, events in clip_ground_truth.items():
        file_id, on, _ = clip_id.rsplit("-", 2)
        shift = int(on) // 100
        files[file_id].extend((shift + a, shift + b, c) for a, b, c in events)
    return merge_overlapping_events(files)
