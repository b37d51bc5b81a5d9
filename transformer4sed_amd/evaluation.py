"""Evaluation path right behind the model: score tables and event decoding with the reference's
call contracts, the per-frame work done on the device.

Mirrors (same names, argument meaning, return types):
  * `Encoder`                         src/codec/encoder.py:7-84   (frame<->time mapping, decode_strong, find_contiguous_regions)
  * `batched_decode_preds`            src/codec/decoder.py:38-103 (soft weak mask, scipy median / max filter, score DataFrames)
  * `decode_pred_batch_fast`          src/codec/decoder.py:15-35  (hard weak mask, median_filter_torch, threshold, events)
  * `create_score_dataframe` / `write_sed_scores`  the sed_scores_eval table layout the reference hands to its metric code
    (recipes/desed/finetune/train.py:470-478; third-party package, restated from its public layout: parity unpinned)
  * `WeakF1Macro`                     torchmetrics MultilabelF1Score(average="macro") as used at train.py:277-287,324-327
  * `log_sedeval_metrics` / `EventSegmentF1`  src/evaluation_measures.py:52-152, 256-295 (sed_eval's event-based and segment-based F1,
    restated in DESIGN.md section 7c and counted on the device: parity with the package unpinned)
  * `Evaluator.step`                  the per-batch body of Trainer.validation / Trainer.test (train.py:296-366, 427-466)

Masking, both median filters and the thresholding run in `sed_median_filter` launches over the whole batch (bit-exact with the
reference's per-clip, per-class scipy / torch loops, tests/test_gpu_eval.py); the host only slices the result into tables."""
import math
import os
from collections import namedtuple
from pathlib import Path

import numpy as np
import pandas as pd
import torch

from . import filter as dev_filter
from .ops import call, h2d


class Encoder:
    """src/codec/encoder.py:7-84."""

    def __init__(self, labels, audio_len, frame_len, frame_hop, net_pooling=1, sr=16000):
        if isinstance(labels, np.ndarray):
            labels = labels.tolist()
        self.labels = list(labels)
        self.audio_len, self.frame_len, self.frame_hop, self.sr, self.net_pooling = audio_len, frame_len, frame_hop, sr, net_pooling
        n_samples = self.audio_len * self.sr
        self.n_frames = int(math.ceil(n_samples / 2 / self.frame_hop) * 2 / self.net_pooling)

    def _time_to_frame(self, time):
        return np.clip(time * self.sr / self.frame_hop / self.net_pooling, a_min=0, a_max=self.n_frames)

    def _frame_to_time(self, frame):
        return np.clip(frame * self.net_pooling * self.frame_hop / self.sr, a_min=0, a_max=self.audio_len)

    def encode_strong_df(self, events_df):
        true_labels = np.zeros((self.n_frames, len(self.labels)))
        for _, row in events_df.iterrows():
            if not pd.isna(row["event_label"]):
                onset = round(self._time_to_frame(row["onset"]))
                offset = round(np.ceil(self._time_to_frame(row["offset"])))
                true_labels[onset:offset, self.labels.index(row["event_label"])] = 1
        return true_labels

    def encode_weak(self, events):
        labels = np.zeros((len(self.labels)))
        for event in events:
            labels[self.labels.index(event)] = 1
        return labels

    def find_contiguous_regions(self, array):
        change = np.logical_xor(array[1:], array[:-1]).nonzero()[0] + 1
        if array[0]:
            change = np.r_[0, change]
        if array[-1]:
            change = np.r_[change, array.size]
        return change.reshape((-1, 2))

    def decode_strong(self, outputs):
        """outputs [n_frame, n_class] {0,1} -> [[label, onset_s, offset_s], ...] (class-major order like the reference)."""
        pred = []
        for i, col in enumerate(outputs.T):
            for on, off in self.find_contiguous_regions(col):
                pred.append([self.labels[i], float(self._frame_to_time(on)), float(self._frame_to_time(off))])
        return pred

    def decode_weak(self, outputs):
        return [self.labels[i] for i, v in enumerate(outputs) if v == 1]


def create_score_dataframe(scores, timestamps, event_classes):
    """sed_scores_eval layout: columns onset, offset, then one column per event class; one row per frame."""
    scores, timestamps = np.asarray(scores), np.asarray(timestamps)
    if timestamps.shape != (scores.shape[0] + 1,) or scores.shape[1] != len(event_classes):
        raise ValueError("scores [T, C] need T + 1 timestamps and C event classes")
    return pd.DataFrame(np.concatenate((timestamps[:-1, None], timestamps[1:, None], scores), axis=1),
                        columns=["onset", "offset", *event_classes])


def write_sed_scores(scores, dirpath):
    """One `<audio_id>.tsv` per clip (tab separated, header onset/offset/classes) -- what sed_scores_eval.io.read_sed_scores and
    the DCASE evaluation tooling read (train.py:470-478 writes the four score buffers this way)."""
    os.makedirs(dirpath, exist_ok=True)
    for audio_id, df in scores.items():
        df.to_csv(os.path.join(dirpath, f"{audio_id}.tsv"), sep="\t", index=False)


def read_sed_scores(dirpath):
    return {p.stem: pd.read_csv(p, sep="\t") for p in sorted(Path(dirpath).glob("*.tsv"))}


def _scores_device(strong_preds, n, filter, filter_type, weak_preds, need_weak_mask):
    """Device half of `batched_decode_preds`: (raw, post) [n, frames, n_class] fp32 device tensors (post None without a filter)."""
    x = strong_preds[:n].detach().transpose(1, 2).contiguous().float()          # [bs, frames, n_class]
    scale = weak_preds[:n].detach().float() if (need_weak_mask and weak_preds is not None) else None
    raw = x if scale is None else x * scale.unsqueeze(1)
    post = None
    if filter:
        run = dev_filter.median_filter_scipy if filter_type == "median" else dev_filter.max_filter_scipy
        post = run(x, list(filter), weak_scale=scale)
    return raw, post


def _scores_tables(raw_h, post_h, filenames, encoder, pad_indx, n_frames):
    """Host half of `batched_decode_preds`: numpy score arrays -> dicts audio_id -> score DataFrame."""
    scores_raw, scores_post = {}, {}
    for j in range(raw_h.shape[0]):
        audio_id = Path(filenames[j]).stem
        r, p = raw_h[j], (post_h[j] if post_h is not None else None)
        if pad_indx is not None:
            # reference quirk (decoder.py:70-72): the cut is applied to the [n_class, frame] tensor BEFORE the transpose,
            # i.e. it truncates classes, not frames.  Reproduced literally (no recipe passes pad_indx).
            true_len = int(n_frames * float(pad_indx[j]))
            r = r[:, :true_len]
            p = p[:, :true_len] if p is not None else None
        ts = encoder._frame_to_time(np.arange(len(r) + 1))
        classes = encoder.labels[:r.shape[1]]
        scores_raw[audio_id] = create_score_dataframe(r, ts, classes)
        scores_post[audio_id] = create_score_dataframe(p, ts, classes) if p is not None else scores_raw[audio_id]
    return scores_raw, scores_post


def batched_decode_preds(strong_preds, filenames, encoder, filter=7, filter_type="median", pad_indx=None, weak_preds=None,
                         need_weak_mask=None):
    """src/codec/decoder.py:38-103.  strong_preds [bs, n_class, frames] (device tensor), weak_preds [bs, n_class].
    Returns (scores_raw, scores_postprocessed): dicts audio_id -> score DataFrame.  `filter`: per-class window list."""
    if filter_type not in ("median", "max"):
        raise ValueError("filter_type must be 'median' or 'max'")
    n = min(strong_preds.shape[0], len(filenames))      # the reference loops over strong_preds and indexes filenames[j]
    if strong_preds.shape[0] > len(filenames):
        raise IndexError("list index out of range")     # same failure as the reference's filenames[j]
    if n == 0:
        return {}, {}
    raw, post = _scores_device(strong_preds, n, filter, filter_type, weak_preds, need_weak_mask)
    return _scores_tables(raw.cpu().numpy(), post.cpu().numpy() if post is not None else None, filenames, encoder, pad_indx,
                          strong_preds.shape[-1])


def _events_device(outputs, weak_preds, thresholds, median_filter):
    """Device half of `decode_pred_batch_fast`: one bool tensor [batch, frames, n_class] per threshold."""
    x = outputs.detach().transpose(1, 2).contiguous().float()
    out = []
    for c_th in thresholds:
        keep = (weak_preds.detach() >= c_th).float()              # output[b, :, c] = 0 where weak_preds[b, c] < c_th
        out.append(dev_filter._run(x, list(median_filter), 0, keep) > c_th)
    return out


def _events_frames(binms, filenames, encoder, thresholds):
    """Host half of `decode_pred_batch_fast`: numpy bool arrays -> {threshold: DataFrame(event_label, onset, offset, filename)}."""
    pred_dfs = {}
    for c_th, binm in zip(thresholds, binms):
        frames = []
        for b in range(binm.shape[0]):
            ev = encoder.decode_strong(binm[b])
            if not ev:
                continue
            pred = pd.DataFrame(ev, columns=["event_label", "onset", "offset"])
            pred["filename"] = Path(filenames[b]).stem + ".wav"
            frames.append(pred)
        pred_dfs[c_th] = (pd.concat(frames, ignore_index=True) if frames
                          else pd.DataFrame(columns=["event_label", "onset", "offset", "filename"]))
    return pred_dfs


def decode_pred_batch_fast(outputs, weak_preds, filenames, encoder, thresholds, median_filter):
    """src/codec/decoder.py:15-35.  outputs [batch, n_class, frames]; per threshold: zero the classes whose weak prediction is
    below it, median_filter_torch, binarise, decode events.  Returns {threshold: DataFrame(event_label, onset, offset, filename)}."""
    thresholds = list(thresholds)
    return _events_frames([b.cpu().numpy() for b in _events_device(outputs, weak_preds, thresholds, median_filter)], filenames, encoder,
                          thresholds)


class WeakF1Macro:
    """Macro-averaged multilabel F1 at threshold 0.5 accumulated over batches (train.py:277-287: torchmetrics
    MultilabelF1Score(num_labels, average="macro"); a class without positives or predictions scores 0).  The counts accumulate on the
    device of the predictions (no host synchronisation per batch); `compute` fetches them."""

    def __init__(self, num_labels, threshold=0.5):
        self.num_labels = num_labels
        self.counts = None          # [3, num_labels] float64: tp, fp, fn
        self.threshold = threshold

    def update(self, preds, target):
        p = (preds.detach() > self.threshold)
        t = target.detach().bool()
        c = torch.stack([(p & t).sum(0), (p & ~t).sum(0), (~p & t).sum(0)]).double()
        self.counts = c if self.counts is None else self.counts + c.to(self.counts.device)

    @property
    def tp(self):
        return self._host()[0]

    @property
    def fp(self):
        return self._host()[1]

    @property
    def fn(self):
        return self._host()[2]

    def _host(self):
        return torch.zeros(3, self.num_labels, dtype=torch.float64) if self.counts is None else self.counts.cpu()

    def compute(self):
        tp, fp, fn = self._host()
        den = 2 * tp + fp + fn
        f1 = torch.where(den > 0, 2 * tp / den.clamp(min=1), torch.zeros_like(den))
        return float(f1.mean())


AP_CHUNK = 20000        # clips per LDS sort of sed_ap_compute (its maximum): the validation split (16 891 clips) is one chunk


class MultilabelAveragePrecision:
    """torchmetrics 0.11 `MultilabelAveragePrecision(num_labels, average, thresholds=None)` as the AudioSet-Strong recipes construct it
    (passt_cnn/train.py:239-314, detect_any_sound/passt/train.py:134-211, open_vocabulary.py:146-227), on HIP kernels (csrc/metrics.hip).

    `update(preds [B, C], target [B, C])` appends the batch to class-major device storage in one stream-ordered call and never waits for the
    device.  Like torchmetrics, a batch with any score outside [0, 1] is stored as its sigmoid (decided per batch, on the device).  The
    target may be integer, bool or a {0, 1}-valued float: the passt_cnn loop hands over a float target (train.py:267); whether 0.11 itself
    accepts one is not checked here.  Scores are kept as fp32.  `compute()` raises on what torchmetrics' argument validation rejects: no
    update, a target outside {0, 1}, a NaN score.  `compute_on_step` is accepted and ignored (calling the object updates and returns None).
    `average`: "macro" (mean over classes with a positive), "weighted" (weights = positives per class), None / "none" ([C]); a class without
    a positive scores NaN and is left out of both averages with torchmetrics' warning.  "micro" is not implemented."""

    def __init__(self, num_labels, average="macro", compute_on_step=None, chunk=AP_CHUNK, **kwargs):
        if average == "micro":
            raise NotImplementedError("MultilabelAveragePrecision: average='micro' is not implemented on the HIP path")
        if average not in ("macro", "weighted", "none", None):
            raise ValueError(f"Expected argument `average` to be one of ('macro', 'weighted', 'none', None), but got {average}")
        for k, v in kwargs.items():
            if k == "thresholds" and v is None or k == "validate_args" or k == "ignore_index" and v is None:
                continue
            raise NotImplementedError(f"MultilabelAveragePrecision: unsupported argument {k}={v!r}")
        self.num_labels, self.average, self.chunk = int(num_labels), average, int(chunk)
        self.device = None
        self.reset()

    def reset(self):
        self.n = 0
        self.cap = 0
        self.scores = self.labels = None
        self._flag = self._status = None

    def to(self, device):
        return self         # (storage lives on the device of the first batch)

    def __call__(self, preds, target):
        self.update(preds, target)

    def _grow(self, need, dev):
        cap = max(need, 2 * self.cap, 64)
        C = self.num_labels
        scores = torch.empty(C, cap, dtype=torch.float32, device=dev)
        labels = torch.empty(C, cap, dtype=torch.uint8, device=dev)
        if self.scores is not None:
            call("sed_ap_grow", self.scores, self.labels, C, self.n, self.cap, scores, labels, cap)
        self.scores, self.labels, self.cap = scores, labels, cap

    def update(self, preds, target):
        if preds.dim() != 2 or preds.shape[1] != self.num_labels or tuple(target.shape) != tuple(preds.shape):
            raise ValueError(f"preds and target must both be [batch, {self.num_labels}], got {tuple(preds.shape)} and {tuple(target.shape)}")
        if preds.is_floating_point() is False:
            raise ValueError("Expected argument `preds` to be a floating tensor")
        dev = preds.device
        if self.device is not None and dev != self.device:
            raise ValueError(f"batches on different devices ({self.device}, {dev})")
        self.device = dev
        p = preds.detach().to(torch.float32).contiguous()
        t = target.detach().to(device=dev, dtype=torch.float32).contiguous()
        B = p.shape[0]
        if self._status is None:
            self._flag = torch.zeros(64, dtype=torch.int32, device=dev)     # (sed_ap_append's per-workgroup flag words)
            self._status = torch.zeros(1, dtype=torch.int32, device=dev)
        if self.n + B > self.cap:
            self._grow(self.n + B, dev)
        call("sed_ap_append", p, t, B, self.num_labels, self.n, self.cap, self._flag, self._status, self.scores, self.labels)
        self.n += B

    def per_class(self):
        """-> (ap [C] float64, positives [C] int32), device tensors."""
        if self.n == 0:
            raise RuntimeError("MultilabelAveragePrecision.compute() called before any update")
        status = int(self._status.item())
        if status & 4:
            raise RuntimeError("Detected the following values in `target`: values outside {0, 1}; expected only 0 and 1")
        if status & 2:
            raise RuntimeError("Detected NaN values in `preds`")
        C, N, ch = self.num_labels, self.n, self.chunk
        nch = (N + ch - 1) // ch
        dev = self.device
        a_sorted = p_sorted = None
        if nch > 1:
            a_sorted = torch.empty(C * nch * ch, dtype=torch.int32, device=dev)
            p_sorted = torch.empty(C * nch * ch, dtype=torch.int32, device=dev)
        pos_cnt = torch.empty(C * nch, dtype=torch.int32, device=dev)
        partial = torch.empty(C * nch, dtype=torch.int64, device=dev)
        ap = torch.empty(C, dtype=torch.float64, device=dev)
        npos = torch.empty(C, dtype=torch.int32, device=dev)
        call("sed_ap_compute", self.scores, self.labels, C, N, self.cap, ch, a_sorted, p_sorted, pos_cnt, partial, ap, npos)
        return ap, npos

    def compute(self):
        ap, npos = self.per_class()
        res = ap.float()
        if self.average in (None, "none"):
            return res
        nan = torch.isnan(res)
        if bool(nan.any()):
            import warnings
            warnings.warn(f"Average precision score for one or more classes was `nan`. Ignoring these classes in {self.average}-average",
                          UserWarning)
        idx = ~nan
        if self.average == "macro":
            return res[idx].mean()
        w = npos.float()[idx]
        s = w.sum()
        w = w / s if float(s) != 0 else torch.zeros_like(w)
        return (res[idx] * w).sum()


PSDS_MAX_FRAMES = 1024         # csrc/psds.hip: frames per clip the sweep holds in LDS
PSDS_MAX_CLIP_EVENTS = 256     # ... and ground-truth events of one clip
PSDS_MAX_CT_CLASSES = 32       # ... and classes together with a cross-trigger threshold
PSDS_PADDED_CLASSES = 16       # up to here `update` keeps the sweep's padded event slots and reads nothing back
PSDS_BLOCK_CLIPS = 2048        # ... in storage allocated for this many clips at a time (the whole split, if it is smaller)
_PSDS_UNITS = {"second": 1.0, "minute": 60.0, "hour": 3600.0}


def _microseconds(x):
    """Times rounded to 6 decimals (sed_scores_eval's time_decimals), as int64 microseconds."""
    return np.rint(np.round(np.asarray(x, dtype=np.float64), 6) * 1e6).astype(np.int64)


def _table(x):
    return x if isinstance(x, pd.DataFrame) else pd.read_csv(x, sep="\t")


class IntersectionPSDS:
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

    def __init__(self, ground_truth, audio_durations, event_classes, timestamps, dtc_threshold, gtc_threshold, cttc_threshold=None,
                 alpha_ct=0, alpha_st=0, max_efpr=100, unit_of_time="hour"):
        self.event_classes = list(event_classes)
        C = self.num_classes = len(self.event_classes)
        if C == 0 or len(set(self.event_classes)) != C:
            raise ValueError("event_classes must be a non-empty list of distinct names")
        for name, v in (("dtc_threshold", dtc_threshold), ("gtc_threshold", gtc_threshold), ("cttc_threshold", cttc_threshold)):
            if v is None and name == "cttc_threshold":
                continue
            if v is None or not 0.0 < float(v) <= 1.0:
                raise ValueError(f"{name} must lie in (0, 1], got {v!r}")
        if unit_of_time not in _PSDS_UNITS:
            raise ValueError(f"unit_of_time must be one of {sorted(_PSDS_UNITS)}")
        if not float(max_efpr) > 0:
            raise ValueError("max_efpr must be positive")
        ts = np.asarray(timestamps, dtype=np.float64)
        if ts.ndim != 1 or ts.size < 2:
            raise ValueError("timestamps must be [T + 1] frame boundaries")
        T = self.num_frames = ts.size - 1
        if T > PSDS_MAX_FRAMES:
            raise NotImplementedError(f"IntersectionPSDS: {T} frames per clip, the HIP sweep holds at most {PSDS_MAX_FRAMES}")
        if cttc_threshold is not None and C > PSDS_MAX_CT_CLASSES:
            raise NotImplementedError(f"IntersectionPSDS: cttc_threshold with {C} classes (at most {PSDS_MAX_CT_CLASSES}; the "
                                      "AudioSet recipes pass None)")
        self.dtc, self.gtc = float(dtc_threshold), float(gtc_threshold)
        self.cttc = None if cttc_threshold is None else float(cttc_threshold)
        self.alpha_ct, self.alpha_st, self.max_efpr = float(alpha_ct), float(alpha_st), float(max_efpr)
        self.unit = _PSDS_UNITS[unit_of_time]
        self.ts_us = _microseconds(ts)
        d = np.diff(self.ts_us)
        if (d < 0).any():
            raise ValueError("timestamps must not decrease")
        self.t_pos = int(T if (d > 0).all() else np.argmin(d > 0))      # leading frames of positive duration: the ones that take part
        if (d[self.t_pos:] > 0).any():
            raise ValueError("a frame of zero duration lies before frames of positive duration")

        dur = _table(audio_durations)
        ids = [Path(f).stem for f in dur["filename"]]
        if len(set(ids)) != len(ids):
            raise ValueError("audio_durations lists a clip twice")
        self.clip_ids = ids
        self._clip_index = {a: i for i, a in enumerate(ids)}
        self.data_us = int(_microseconds(dur["duration"].to_numpy()).sum())
        if self.data_us <= 0:
            raise ValueError("audio_durations sums to nothing")
        gt = _table(ground_truth)
        cls_index = {c: i for i, c in enumerate(self.event_classes)}
        per_clip = [[] for _ in ids]
        self._gt_clips = set()
        on_us, off_us = _microseconds(gt["onset"].to_numpy()), _microseconds(gt["offset"].to_numpy())
        for f, label, on, off in zip(gt["filename"], gt["event_label"], on_us.tolist(), off_us.tolist()):
            a = Path(f).stem
            if a not in self._clip_index:
                raise ValueError(f"ground-truth clip {a!r} is missing from audio_durations")
            self._gt_clips.add(a)
            if pd.isna(label):
                continue                                # (a clip without events)
            if label not in cls_index:
                raise ValueError(f"ground-truth label {label!r} is not one of event_classes")
            if off <= on:
                raise ValueError(f"ground-truth event of {a!r} with offset <= onset")
            per_clip[self._clip_index[a]].append((cls_index[label], on, off))
        ptr, flat = [0], []
        for a, ev in zip(ids, per_clip):
            if len(ev) > PSDS_MAX_CLIP_EVENTS:
                raise NotImplementedError(f"IntersectionPSDS: clip {a!r} has {len(ev)} events (at most {PSDS_MAX_CLIP_EVENTS})")
            flat += sorted(ev)
            ptr.append(len(flat))
        self.gt_ptr = np.asarray(ptr, dtype=np.int32)
        self.gt = np.asarray(flat, dtype=np.int64).reshape(-1, 3)        # class, onset_us, offset_us; CSR by clip, sorted by (clip, class)
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
        self._dev = self._status = None                 # ground truth on the device and the sweep's status word: made at the first update
        self._blocks = []                               # slot storage of the padded form: dict(cap, used, slots)
        self.reset()

    def reset(self):
        """Forgets every scored clip (a new validation epoch); the ground truth stays where it is."""
        self._seen = set()
        self._chunks = []           # compacted events: (class int64, value f32, dTP int64, dFP int64, dCT int64 | None)
        self._padded = []           # the sweep's slots as they are: (value [n, C, T] f32, dTP int16, dFP int16, dCT int64 | None)
        self._points = None
        self._blocks = self._blocks[:1]
        for blk in self._blocks:
            blk["used"] = 0
        if self._status is not None:
            self._status.zero_()

    # ---- device half
    def _constants(self, dev):
        if self._dev is None:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            self._dev = dict(device=dev, ts=up(self.ts_us), ptr=up(self.gt_ptr), cls=up(self.gt[:, 0].astype(np.int32)),
                             on=up(self.gt[:, 1]), off=up(self.gt[:, 2]), q=up(self.ct_q) if self.ct_q is not None else None)
            self._status = torch.zeros(1, dtype=torch.int32, device=dev)
        elif self._dev["device"] != dev:
            raise ValueError(f"batches on different devices ({self._dev['device']}, {dev})")
        return self._dev

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
        rows, batch = [], set()
        for f in filenames:
            a = Path(f).stem
            if a not in self._clip_index:
                raise ValueError(f"clip {a!r} is missing from audio_durations")
            if a in self._seen or a in batch:
                raise ValueError(f"clip {a!r} was scored twice")
            batch.add(a)
            rows.append(self._clip_index[a])
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

    def _class_rocs(self):
        """Per class the staircase (eFPR ascending, running-maximum TPR), float64, with the empty point first."""
        rocs = []
        for c, p in enumerate(self.counts()):
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
        rocs = self._class_rocs()
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


F1_MAX_FRAMES = 1024           # csrc/event_f1.hip: frames per clip
F1_MAX_CLIP_EVENTS = 256       # ... ground-truth events of one clip
F1_MAX_ESTIMATES = 512         # ... estimated events of one class in one clip
F1_MAX_SEGMENTS = 64           # ... segments per clip (one bit each)
F1_COUNTS = ("n_ref", "n_sys", "tp", "seg_tp", "seg_fp", "seg_fn")


class EventSegmentF1:
    """Event-based (collar) and segment-based F1 as `log_sedeval_metrics` takes them from sed_eval (src/evaluation_measures.py:52-152:
    t_collar 0.2, percentage_of_length 0.2, time_resolution 1.0, onset and offset evaluated, optimal matching), accumulated batch by
    batch as six integers per class on the device.  DESIGN.md section 7c is the definition and names its open points; parity with
    sed_eval's own output is not pinned (the package is not available to compare with).

    `ground_truth`: TSV path or DataFrame (filename, onset, offset, event_label); a row with a NaN label is a clip without events; clips
    are keyed by the filename's stem.  `timestamps` [T + 1]: the frame boundaries shared by all clips
    (`encoder._frame_to_time(arange(T + 1))`), or None for an accumulator that only takes event lists.
    `update(active [n, T, C] bool / uint8 device tensor, filenames)`: the binarised frame matrix `decode_pred_batch_fast` decodes; the
    estimated events are its maximal runs, exactly `Encoder.decode_strong`'s list.  `update_events(DataFrame, filenames=None)`: the same
    from an event list; `filenames` names the clips it scores (a clip without a row has no output), by default the clips of the frame.
    Both run `sed_event_f1_counts` (one wave per clip and class) on the current stream and read nothing back.
    `counts()` -> {name: int64 [C]} for n_ref, n_sys, tp, seg_tp, seg_fp, seg_fn; `compute()` -> event_macro, event_micro,
    segment_macro, segment_micro (fractions in [0, 1]) and "class_wise".  A class without reference events (segments) is left out of the
    macro mean; a class-wise F1 whose denominator is zero is reported as 0.0.

    Refused: T > 1024, a clip with more than 256 ground-truth events, more than 64 segments per clip, more than 512 estimated events of
    one class in one clip (NotImplementedError); a ground-truth event with offset <= onset, a label outside event_classes, a clip scored
    twice or missing from the ground truth, overlapping estimates of one class in one clip, ground-truth clips without a score (at
    `compute`) (ValueError)."""

    def __init__(self, ground_truth, event_classes, timestamps, t_collar=0.2, percentage_of_length=0.2, time_resolution=1.0):
        self.event_classes = list(event_classes)
        C = self.num_classes = len(self.event_classes)
        if C == 0 or len(set(self.event_classes)) != C:
            raise ValueError("event_classes must be a non-empty list of distinct names")
        if not float(t_collar) >= 0 or not 0.0 <= float(percentage_of_length) <= 1.0:
            raise ValueError("t_collar must not be negative and percentage_of_length must lie in [0, 1]")
        self.collar_us = int(_microseconds(t_collar))
        self.p = float(percentage_of_length)
        self.res_us = int(_microseconds(time_resolution))
        if self.res_us <= 0:
            raise ValueError("time_resolution must be a positive number of microseconds")
        self.ts_us, self.num_frames = None, None
        if timestamps is not None:
            ts = np.asarray(timestamps, dtype=np.float64)
            if ts.ndim != 1 or ts.size < 2:
                raise ValueError("timestamps must be [T + 1] frame boundaries")
            self.num_frames = ts.size - 1
            if self.num_frames > F1_MAX_FRAMES:
                raise NotImplementedError(f"EventSegmentF1: {self.num_frames} frames per clip, the HIP kernel holds at most {F1_MAX_FRAMES}")
            self.ts_us = _microseconds(ts)
            if (np.diff(self.ts_us) < 0).any() or self.ts_us[0] < 0:
                raise ValueError("timestamps must not decrease or be negative")
        gt = _table(ground_truth)
        cls_index = {c: i for i, c in enumerate(self.event_classes)}
        self._cls_index = cls_index
        self.clip_ids, self._clip_index, per_clip = [], {}, []
        on_us, off_us = (_microseconds(np.nan_to_num(gt[k].to_numpy(dtype=np.float64))) for k in ("onset", "offset"))     # (NaN: rows without a label)
        for f, label, on, off in zip(gt["filename"], gt["event_label"], on_us.tolist(), off_us.tolist()):
            a = Path(f).stem
            if a not in self._clip_index:
                self._clip_index[a] = len(self.clip_ids)
                self.clip_ids.append(a)
                per_clip.append([])
            if pd.isna(label):
                continue                                # (a clip without events)
            if label not in cls_index:
                raise ValueError(f"ground-truth label {label!r} is not one of event_classes")
            if off <= on:
                raise ValueError(f"ground-truth event of {a!r} with offset <= onset")
            if on < 0:
                raise ValueError(f"ground-truth event of {a!r} with a negative onset")
            per_clip[self._clip_index[a]].append((cls_index[label], on, off))
        ptr, flat = [0], []
        end_us = int(self.ts_us[-1]) if self.ts_us is not None else 0
        for a, ev in zip(self.clip_ids, per_clip):
            if len(ev) > F1_MAX_CLIP_EVENTS:
                raise NotImplementedError(f"EventSegmentF1: clip {a!r} has {len(ev)} events (at most {F1_MAX_CLIP_EVENTS})")
            flat += sorted(ev)
            ptr.append(len(flat))
            end_us = max([end_us] + [e[2] for e in ev])
        self._check_segments(end_us)
        self.gt_ptr = np.asarray(ptr, dtype=np.int32)
        self.gt = np.asarray(flat, dtype=np.int64).reshape(-1, 3)        # class, onset_us, offset_us; CSR by clip, sorted by (clip, class)
        self._dev = self._counts = self._status = None                   # made at the first update, on its device
        self.reset()

    def _check_segments(self, end_us):
        n_seg = -(-int(end_us) // self.res_us)
        if n_seg > F1_MAX_SEGMENTS:
            raise NotImplementedError(f"EventSegmentF1: {n_seg} segments of {self.res_us} us per clip (at most {F1_MAX_SEGMENTS})")

    def reset(self):
        """Forgets every scored clip (a new validation epoch); the ground truth stays where it is."""
        self._seen = set()
        if self._counts is not None:
            self._counts.zero_()
            self._status.zero_()

    # ---- device half
    def _state(self, dev):
        """The ground truth, the counts [C, 6] and the status word on `dev`, made once."""
        if self._dev is None:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            pad = lambda a: a if a.size else np.zeros(1, dtype=a.dtype)      # (no null pointer for a ground truth without events)
            self._dev = dict(device=dev, ts=up(self.ts_us) if self.ts_us is not None else None, ptr=up(self.gt_ptr),
                             cls=up(pad(self.gt[:, 0].astype(np.int32))), on=up(pad(self.gt[:, 1])), off=up(pad(self.gt[:, 2])))
            self._counts = torch.zeros(self.num_classes, len(F1_COUNTS), dtype=torch.int64, device=dev)
            self._status = torch.zeros(1, dtype=torch.int32, device=dev)
        elif self._dev["device"] != dev:
            raise ValueError(f"batches on different devices ({self._dev['device']}, {dev})")
        return self._dev

    def _run(self, rows, active=None, est=None):
        """Adds the counts of the clips `rows` (ground-truth rows) to the device counts.  `active` [n, T, C] uint8 on the device, or
        `est` = (ptr int32 [n + 1], class int32, onset_us int64, offset_us int64) host arrays.  Stream-ordered: the small host arrays
        travel through pinned memory, nothing is read back."""
        if active is not None and not active.is_cuda or active is None and not torch.cuda.is_available():
            raise RuntimeError("EventSegmentF1 needs an MI355X (HIP) device; the counting kernel has no CPU path")
        dev = active.device if active is not None else (self._dev["device"] if self._dev is not None
                                                              else torch.device("cuda", torch.cuda.current_device()))
        k = self._state(dev)
        n = len(rows)
        side = lambda a, dt: h2d(np.ascontiguousarray(a), dt, dev)      # (pinned staging ring: no allocation, no wait)
        clip = side(np.asarray(rows, dtype=np.int32), torch.int32)
        if active is not None:
            T = active.shape[1]
            call("sed_event_f1_counts", active, None, None, None, None, clip, k["ts"], k["ptr"], k["cls"], k["on"], k["off"],
                 self.collar_us, self.p, self.res_us, n, T, self.num_classes, self._counts, self._status)
            return
        ptr, cls, on, off = est
        pad = lambda a: a if a.size else np.zeros(1, dtype=a.dtype)
        call("sed_event_f1_counts", None, side(ptr, torch.int32), side(pad(cls), torch.int32), side(pad(on), torch.int64),
             side(pad(off), torch.int64), clip, None, k["ptr"], k["cls"], k["on"], k["off"], self.collar_us, self.p, self.res_us, n, 0,
             self.num_classes, self._counts, self._status)

    def _rows(self, filenames):
        rows, batch = [], set()
        for f in filenames:
            a = Path(f).stem
            if a not in self._clip_index:
                raise ValueError(f"clip {a!r} is missing from the ground truth")
            if a in self._seen or a in batch:
                raise ValueError(f"clip {a!r} was scored twice")
            batch.add(a)
            rows.append(self._clip_index[a])
        return rows, batch

    def update(self, active, filenames):
        T, C = self.num_frames, self.num_classes
        if T is None:
            raise ValueError("EventSegmentF1 was made without timestamps: it takes event lists only (update_events)")
        if not isinstance(active, torch.Tensor) or active.dim() != 3 or tuple(active.shape[1:]) != (T, C):
            raise ValueError(f"active must be a [n, {T}, {C}] tensor")
        if active.dtype not in (torch.bool, torch.uint8):
            raise ValueError("active must be bool or uint8")
        if len(filenames) != active.shape[0]:
            raise ValueError("one filename per clip")
        rows, batch = self._rows(filenames)
        if not rows:
            return
        a = active.detach().contiguous()
        self._run(rows, active=a.view(torch.uint8) if a.dtype == torch.bool else a)
        self._seen |= batch

    def update_events(self, events, filenames=None):
        """`events`: DataFrame(event_label, onset, offset, filename), as `decode_pred_batch_fast` returns it; rows with a NaN label are
        skipped."""
        names = list(events["filename"]) if len(events) else []
        rows, batch = self._rows(list(dict.fromkeys(Path(f).stem for f in names)) if filenames is None else filenames)
        slot = {r: i for i, r in enumerate(rows)}
        per_clip = [[] for _ in rows]
        if len(events):
            on_us, off_us = (_microseconds(np.nan_to_num(events[k].to_numpy(dtype=np.float64))) for k in ("onset", "offset"))
            for f, label, on, off in zip(names, events["event_label"], on_us.tolist(), off_us.tolist()):
                a = Path(f).stem
                if self._clip_index.get(a) not in slot:
                    raise ValueError(f"event of clip {a!r}, which is not among the clips this call scores")
                if pd.isna(label):
                    continue
                if label not in self._cls_index:
                    raise ValueError(f"label {label!r} is not one of event_classes")
                if off < on or on < 0:
                    raise ValueError(f"estimated event of {a!r} with offset < onset or a negative onset")
                per_clip[slot[self._clip_index[a]]].append((self._cls_index[label], on, off))
        ptr, flat, end_us = [0], [], 0
        for r, ev in zip(rows, per_clip):
            ev.sort()
            for c in range(self.num_classes):
                of_c = [e for e in ev if e[0] == c]
                if len(of_c) > F1_MAX_ESTIMATES:
                    raise NotImplementedError(f"EventSegmentF1: {len(of_c)} estimated events of {self.event_classes[c]!r} in clip "
                                              f"{self.clip_ids[r]!r} (at most {F1_MAX_ESTIMATES})")
                if any(nxt[1] < cur[2] for cur, nxt in zip(of_c[:-1], of_c[1:])):
                    raise ValueError(f"overlapping estimated events of {self.event_classes[c]!r} in clip {self.clip_ids[r]!r}: the "
                                     "matching needs the estimates of one class disjoint")
            flat += ev
            ptr.append(len(flat))
            end_us = max([end_us] + [e[2] for e in ev])
        self._check_segments(end_us)
        if not rows:
            return
        flat = np.asarray(flat, dtype=np.int64).reshape(-1, 3)
        self._run(rows, est=(np.asarray(ptr, dtype=np.int32), flat[:, 0].astype(np.int32), flat[:, 1], flat[:, 2]))
        self._seen |= batch

    # ---- finish: integer counts, then float64 scores
    def counts(self):
        """{"n_ref", "n_sys", "tp", "seg_tp", "seg_fp", "seg_fn"}: int64 [C] in event_classes order, summed over the scored clips."""
        missing = sorted(set(self.clip_ids) - self._seen)
        if missing:
            raise ValueError(f"ground-truth clips without scores: {missing}")
        if self._counts is None:
            host = np.zeros((self.num_classes, len(F1_COUNTS)), dtype=np.int64)
        else:
            status = int(self._status.item())
            if status & 1:
                raise RuntimeError("EventSegmentF1: the estimates a reference event hits were not one index interval; the greedy "
                                   "matching is not known to be maximal (DESIGN.md section 7c)")
            if status & (4 | 8 | 16):
                raise RuntimeError(f"EventSegmentF1: a list exceeded the kernel's limits (status {status})")
            host = self._counts.cpu().numpy()
        return {name: host[:, i].copy() for i, name in enumerate(F1_COUNTS)}

    @staticmethod
    def scores(counts):
        """The four numbers and the class-wise F1 arrays from integer counts [C] (float64)."""
        c = {k: np.asarray(v, dtype=np.int64) for k, v in counts.items()}
        ratio = lambda num, den: np.where(den > 0, num / np.maximum(den, 1), 0.0).astype(np.float64)
        ev_den = c["n_ref"] + c["n_sys"]
        ev_f1 = ratio(2.0 * c["tp"], ev_den)
        seg_den = 2 * c["seg_tp"] + c["seg_fp"] + c["seg_fn"]
        seg_f1 = ratio(2.0 * c["seg_tp"], seg_den)
        has_ev, has_seg = c["n_ref"] > 0, (c["seg_tp"] + c["seg_fn"]) > 0
        return dict(event_macro=float(ev_f1[has_ev].mean()) if has_ev.any() else 0.0,
                    event_micro=float(ratio(2.0 * c["tp"].sum(), ev_den.sum())),
                    segment_macro=float(seg_f1[has_seg].mean()) if has_seg.any() else 0.0,
                    segment_micro=float(ratio(2.0 * c["seg_tp"].sum(), seg_den.sum())), event_f1=ev_f1, segment_f1=seg_f1)

    def compute(self):
        c = self.counts()
        s = self.scores(c)
        out = {k: s[k] for k in ("event_macro", "event_micro", "segment_macro", "segment_micro")}
        out["class_wise"] = {name: {"event_f1": float(s["event_f1"][i]), "segment_f1": float(s["segment_f1"][i]),
                                    **{k: int(c[k][i]) for k in F1_COUNTS}} for i, name in enumerate(self.event_classes)}
        return out


def log_sedeval_metrics(predictions, ground_truth, save_dir=None, return_class_wise=False):
    """src/evaluation_measures.py:256-295 on `EventSegmentF1`: `predictions` is the DataFrame(event_label, onset, offset, filename) of
    `decode_pred_batch_fast`, `ground_truth` a TSV path (or DataFrame).  -> (event macro F1, event micro F1, segment macro F1, segment
    micro F1), with `return_class_wise` the class-wise dict after the second entry; (0.0, 0.0, 0.0, 0.0) for an empty prediction frame.
    Like the reference's loops it scores every file of the ground truth and ignores predictions for other files; the classes are those
    of either table.  `save_dir` gets `event_f1.txt` and `segment_f1.txt` with the counts and scores as plain text: sed_eval's report
    layout (error rates, substitutions, its tables) is not reproduced."""
    if predictions.empty:
        return 0.0, 0.0, 0.0, 0.0
    gt = _table(ground_truth)
    classes = sorted(set(gt["event_label"].dropna()) | set(predictions["event_label"].dropna()))
    if not classes:
        return 0.0, 0.0, 0.0, 0.0
    acc = EventSegmentF1(gt, classes, None)
    known = [Path(f).stem in acc._clip_index for f in predictions["filename"]]
    acc.update_events(predictions[known], acc.clip_ids)
    res = acc.compute()
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
        for stem, kind, keys in (("event_f1", "event", ("n_ref", "n_sys", "tp")), ("segment_f1", "segment", ("seg_tp", "seg_fp", "seg_fn"))):
            with open(os.path.join(save_dir, stem + ".txt"), "w") as f:
                f.write(f"{kind}-based F1 (t_collar 0.2 s, percentage_of_length 0.2, time_resolution 1.0 s)\n")
                f.write(f"micro {res[kind + '_micro']:.6f}\nmacro {res[kind + '_macro']:.6f}\n")
                f.write("\t".join(("class", "f1") + keys) + "\n")
                for name, row in res["class_wise"].items():
                    f.write("\t".join([name, f"{row[kind + '_f1']:.6f}"] + [str(row[k]) for k in keys]) + "\n")
    if return_class_wise:
        return res["event_macro"], res["event_micro"], res["class_wise"], res["segment_macro"], res["segment_micro"]
    return res["event_macro"], res["event_micro"], res["segment_macro"], res["segment_micro"]


ScoreBufferTuple = namedtuple("ScoreBufferTuple", ["raw_student", "raw_teacher", "post_student", "post_teacher"])


class _HostStage:
    """Pinned staging buffers + one event: device results travel to the host without the host waiting for the stream -- it waits for
    THIS copy (the event) only, after it has queued whatever the GPU is to do next."""

    def __init__(self):
        self.bufs, self.event = {}, None

    def put(self, key, t):
        if not t.is_cuda:
            return t
        t = t.contiguous()
        b = self.bufs.get(key)
        if b is None or b.shape != t.shape or b.dtype != t.dtype:
            b = self.bufs[key] = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        b.copy_(t, non_blocking=True)
        return b

    def mark(self):
        if torch.cuda.is_available():
            self.event = torch.cuda.Event()
            self.event.record()

    def wait(self):
        if self.event is not None:
            self.event.synchronize()
            self.event = None


class Evaluator:
    """Per-batch body of Trainer.validation / Trainer.test (recipes/desed/finetune/train.py:296-366, 427-466): eval-mode frontend,
    student + EMA-teacher forward with `val_kwargs` (17 sliding windows, temperature 0.5, pad mask), weak-F1 accumulation, score
    tables (soft weak mask + per-class scipy median) and half-point event lists (hard mask + torch median).

    The host half of a model's decode (DataFrames, event lists: ~7 ms per model and batch of 32) runs while the GPU is busy with the NEXT
    forward: `step` queues the student's forward, filters and device-to-host copies, finishes the previous batch's teacher tables, queues
    the teacher, finishes the student's tables and returns with the teacher's still pending.  `scores`, `events`, `event_frame`,
    `write` and `flush` complete whatever is pending first, so what a caller reads is always whole.  (The synchronous form -- decode
    right behind each forward with `.cpu()` -- left the GPU idle for 14 of a 212 ms validation step, tools/ablate/step_gaps.sh.)

    With `ground_truth=` / `audio_durations=` the post-processed scores and the binarised frames also feed, still on the device, the
    PSDS accumulators (`psds()`) and one `EventSegmentF1` per model (`f1()`)."""

    PSDS_ARGS = {"psds1": dict(dtc_threshold=0.7, gtc_threshold=0.7, cttc_threshold=None, alpha_ct=0, alpha_st=1),      # train.py:229-253
                 "psds2": dict(dtc_threshold=0.1, gtc_threshold=0.1, cttc_threshold=0.3, alpha_ct=0.5, alpha_st=1)}

    def __init__(self, net, ema_net, encoder, config, ground_truth=None, audio_durations=None):
        self.net, self.ema_net, self.encoder, self.config = net, ema_net, encoder, config
        if (ground_truth is None) != (audio_durations is None):
            raise ValueError("ground_truth and audio_durations go together")
        self._psds_tables = None if ground_truth is None else (_table(ground_truth), _table(audio_durations))
        self._psds = None           # who -> {"psds1": IntersectionPSDS, "psds2": ...}, made at the first batch (it brings the frame count)
        self._f1 = None             # who -> EventSegmentF1, likewise
        tr = config["training"]
        self.median_filter = [int(i / 156 * 1000) for i in tr["median_window"]]          # train.py:221-227
        self.filter_type = tr.get("filter_type", "median")
        self.weak_mask = tr.get("weak_mask", False)
        if self.filter_type not in ("median", "max"):
            raise ValueError("filter_type must be 'median' or 'max'")
        self._scores = ScoreBufferTuple(dict(), dict(), dict(), dict())
        self._events = {"student": [], "teacher": []}
        self.weak_f1 = {"student": WeakF1Macro(len(encoder.labels)), "teacher": WeakF1Macro(len(encoder.labels))}
        self._stage = {"student": _HostStage(), "teacher": _HostStage()}
        self._pending = {}

    # ---- device half of one model's decode: filters, thresholds, device-to-host copies into pinned buffers, one event
    def _enqueue(self, who, strong, weak, paths):
        if strong.shape[0] > len(paths):
            raise IndexError("list index out of range")     # (batched_decode_preds' contract)
        n = min(strong.shape[0], len(paths))
        st = self._stage[who]
        job = {"who": who, "paths": list(paths), "n": n, "frames": strong.shape[-1], "raw": None, "post": None, "bin": None}
        if n > 0:
            raw, post = _scores_device(strong, n, self.median_filter, self.filter_type, weak, self.weak_mask)
            job["raw"] = st.put("raw", raw)
            job["post"] = st.put("post", post) if post is not None else None
            if self._psds_tables is not None:
                self._psds_update(who, post if post is not None else raw, paths[:n])
        binm = _events_device(strong, weak, [0.5], self.median_filter)[0]
        if self._psds_tables is not None and n > 0:
            self._f1_update(who, binm, paths[:n])
        job["bin"] = st.put("bin", binm)
        st.mark()
        return job

    def _psds_update(self, who, scores, paths):
        """Feeds the post-processed scores [n, frames, n_class] to the model's psds1 / psds2 accumulators: stream-ordered sweeps, the
        host waits for nothing (10 classes: the accumulators keep the sweep's padded event slots)."""
        if self._psds is None:
            ts = self.encoder._frame_to_time(np.arange(scores.shape[1] + 1))
            self._psds = {w: {k: IntersectionPSDS(*self._psds_tables, self.encoder.labels, ts, **a) for k, a in self.PSDS_ARGS.items()}
                          for w in ("student", "teacher")}
        for acc in self._psds[who].values():
            acc.update(scores, paths)

    def _f1_update(self, who, binm, paths):
        """Feeds the binarised, median-filtered frames [n, frames, n_class] (bool, still on the device) to the model's `EventSegmentF1`:
        one stream-ordered launch, the host waits for nothing.  Like the reference's loops over the files of the ground truth, clips
        the ground truth does not list are left out."""
        if self._f1 is None:
            ts = self.encoder._frame_to_time(np.arange(binm.shape[1] + 1))
            self._f1 = {w: EventSegmentF1(self._psds_tables[0], self.encoder.labels, ts) for w in ("student", "teacher")}
        acc = self._f1[who]
        keep = [i for i, f in enumerate(paths) if Path(f).stem in acc._clip_index]
        if len(keep) != len(paths):
            if not keep:
                return
            binm = binm.index_select(0, h2d(keep, torch.int64, binm.device))
        acc.update(binm, [paths[i] for i in keep])

    def f1(self):
        """The validation's event-based and segment-based F1 (train.py:370-398: `log_sedeval_metrics` on the half-point event lists):
        {"event_macro/s", "event_micro/s", "segment_macro/s", "segment_micro/s", the same with "/t", "class_wise": {"s": ..., "t": ...}}."""
        if self._psds_tables is None:
            raise RuntimeError("Evaluator.f1() needs ground_truth= and audio_durations= at construction")
        if self._f1 is None:
            raise RuntimeError("Evaluator.f1() called before any step")
        out = {"class_wise": {}}
        for who, tag in (("student", "s"), ("teacher", "t")):
            res = self._f1[who].compute()
            out["class_wise"][tag] = res.pop("class_wise")
            out.update({f"{k}/{tag}": v for k, v in res.items()})
        return out

    def psds(self):
        """The validation's four PSDS numbers (train.py:370-398) under the reference's log keys, and the single-class dicts under
        "single": {"psds1/s": ..., "psds2/s": ..., "psds1/t": ..., "psds2/t": ..., "single": {same keys: {class: psds}}}."""
        if self._psds_tables is None:
            raise RuntimeError("Evaluator.psds() needs ground_truth= and audio_durations= at construction")
        if self._psds is None:
            raise RuntimeError("Evaluator.psds() called before any step")
        out = {"single": {}}
        for who, tag in (("student", "s"), ("teacher", "t")):
            for k, acc in self._psds[who].items():
                out[f"{k}/{tag}"], out["single"][f"{k}/{tag}"] = acc.compute()
        return out

    # ---- host half
    def _finish(self, job):
        if job is None:
            return
        who = job["who"]
        self._stage[who].wait()
        raw_buf, post_buf = ((self._scores.raw_student, self._scores.post_student) if who == "student"
                             else (self._scores.raw_teacher, self._scores.post_teacher))
        if job["n"] > 0:
            raw, post = _scores_tables(job["raw"].numpy(), job["post"].numpy() if job["post"] is not None else None, job["paths"],
                                       self.encoder, None, job["frames"])
            raw_buf.update(raw); post_buf.update(post)
        self._events[who].append(_events_frames([job["bin"].numpy()], job["paths"], self.encoder, [0.5])[0.5])

    def flush(self):
        """Completes the tables / event lists of every batch handed to `step` so far."""
        for who in ("student", "teacher"):
            self._finish(self._pending.pop(who, None))

    @property
    def scores(self):
        self.flush()
        return self._scores

    @property
    def events(self):
        self.flush()
        return self._events

    @torch.no_grad()
    def step(self, wav, labels, pad_mask, paths):
        self.net.eval(); self.ema_net.eval()
        ext = self.net.get_feature_extractor()
        ext.eval()
        feat = ext.logmel(wav)                                                           # preprocess_eval (train.py:216-219)
        kw = self.config[self.net.get_model_name()]["val_kwargs"]
        labels_weak = (labels.sum(-1) >= 1)
        out = {}
        strong, weak, other = self.net(feat, pad_mask=pad_mask, **kw)
        self.weak_f1["student"].update(other["at_out"], labels_weak)
        job_s = self._enqueue("student", strong, weak, paths)
        out["student"] = (strong, weak, other["at_out"])
        self._finish(self._pending.pop("teacher", None))        # the previous batch's teacher, under the student's forward
        strong, weak, other = self.ema_net(feat, pad_mask=pad_mask, **kw)
        self.weak_f1["teacher"].update(other["at_out"], labels_weak)
        self._pending["teacher"] = self._enqueue("teacher", strong, weak, paths)
        out["teacher"] = (strong, weak, other["at_out"])
        self._finish(job_s)                                     # the student's tables, under the teacher's forward
        return out

    def event_frame(self, who):
        ev = self.events[who]
        return pd.concat(ev, ignore_index=True) if ev else pd.DataFrame()

    def write(self, save_folder):
        """train.py:470-478."""
        for name in ScoreBufferTuple._fields:
            write_sed_scores(getattr(self.scores, name), os.path.join(save_folder, name))


def mean_psds_per_type(single_psds, type_dict):
    """passt_cnn/train.py:223-237: mean of the per-class PSDS of each class type ({"common": .., "rare": ..}) -- of the single-class
    dict `IntersectionPSDS.compute` / `AudiosetStrongEvaluator.psds` return."""
    ret = {category: [] for category in set(type_dict.values())}
    for event, psds in single_psds.items():
        ret[type_dict[event]].append(psds)
    return {category: sum(v) / len(v) for category, v in ret.items()}


def remove_extra_events(scores_buffer, events):
    """passt_cnn/train.py:169-172 (`_remove_extra_events`): drops the columns of `events` from every score table, in place."""
    events = list(events)
    for audio_id, df in scores_buffer.items():
        scores_buffer[audio_id] = df.drop(events, axis=1)
    return scores_buffer


class AudiosetStrongEvaluator:
    """Per-batch body of the AudioSet-Strong validation / test loops:
      mode "closed"           passt_cnn/train.py:239-314 / 323-370 (PaSST_CNN, 407 classes): mAP of the weak output
      mode "dasm"             detect_any_sound/passt/train.py:134-211 / 213-269 (DASM, out_type 'sigmoid'): mAP of the tagging output at_out
      mode "open_vocabulary"  open_vocabulary.py:146-227 / 229-301: DASM queried common classes first with the decoder's attention mask
                              (get_common_first_query / get_att_mask), every output put back into class order (reorder_pred)
    Eval-mode forward with `val_kwargs` (`test_kwargs` when test=True), mAP through `MultilabelAveragePrecision` on
    labels_weak = labels.sum(-1) >= 1, score tables of the post-processed posteriors with the device median filter (no weak mask).  A
    batch's tables are built on the host while the GPU runs the next batch's forward (`_HostStage`, like `Evaluator`); `scores` waits for
    whatever is pending.

    Median window: the reference computes `int(median_window / 156 * pred_len)`, ONE int, and hands it to batched_decode_preds, which
    needs a per-class list -- its validation fails with a nonzero window.  Here the int is expanded to [w] * C.
    `events_set`: the classes of the ground truth; the other columns are dropped from the post-processed tables (`psds` does that before
    computing, train.py:174-175).  The 'logit' tagging output of DASM is out of scope, as in dasm_trainer."""

    MODES = ("closed", "dasm", "open_vocabulary")

    PSDS_ARGS = dict(dtc_threshold=0.7, gtc_threshold=0.7, cttc_threshold=None, alpha_ct=0, alpha_st=0)       # passt_cnn/train.py:174-186

    def __init__(self, net, encoder, config, mode, type_dict=None, events_set=None, test=False, ground_truth=None, audio_durations=None):
        if mode not in self.MODES:
            raise ValueError(f"mode must be one of {self.MODES}")
        self.net, self.encoder, self.config, self.mode, self.test = net, encoder, config, mode, test
        name = net.get_model_name()
        if mode != "closed":
            out_type = config[name].get("init_kwargs", {}).get("at_param", {}).get("out_type", "sigmoid")
            if out_type != "sigmoid":
                raise NotImplementedError("AudiosetStrongEvaluator: the 'logit' tagging output is out of scope on the HIP path")
        self.kwargs = config[name]["test_kwargs" if test else "val_kwargs"]
        tr = config["training"]
        w = int(tr["median_window"] / 156 * config["feature"]["pred_len"])                 # train.py:156-160
        self.median_filter = [w] * len(encoder.labels) if w else None
        self.filter_type = tr.get("filter_type", "median") if test else "median"
        self.events_set = events_set
        self.type_dict = None
        self.mask = None
        if mode == "open_vocabulary":
            from .dasm_trainer import common_type_mask, load_type_dict
            self.type_dict = load_type_dict(type_dict if type_dict is not None else config["dataset"]["event_state"])
            self.mask = common_type_mask(encoder.labels, self.type_dict, next(net.parameters()).device)
            # the common-first permutation, its inverse and the attention mask, once: per batch only index_select runs (the reference's
            # boolean-mask forms, dasm_trainer.get_common_first_query / reorder_pred, wait for the device on every call)
            from .dasm_trainer import get_att_mask
            self._first = torch.cat([torch.nonzero(self.mask).reshape(-1), torch.nonzero(~self.mask).reshape(-1)])
            self._inv = torch.argsort(self._first)
            self._att = get_att_mask(self.mask)
        elif type_dict is not None:
            from .dasm_trainer import load_type_dict
            self.type_dict = load_type_dict(type_dict)
        self.map = MultilabelAveragePrecision(len(encoder.labels), average="macro", compute_on_step=False)
        self._post, self._raw = {}, {}
        self._stage = [_HostStage(), _HostStage()]
        self._n = 0
        self._pending = None
        if (ground_truth is None) != (audio_durations is None):
            raise ValueError("ground_truth and audio_durations go together")
        self._psds_tables = None if ground_truth is None else (_table(ground_truth), _table(audio_durations))
        self._psds = None           # IntersectionPSDS over the classes of events_set, made at the first batch
        self._psds_cols = None

    def _psds_update(self, scores, paths):
        """Post-processed scores [n, frames, n_class] -> the PSDS accumulator, the classes outside `events_set` dropped first like
        train.py:174-175.  With more than 16 classes each update reads one small count back (IntersectionPSDS)."""
        if self._psds is None:
            labels = list(self.encoder.labels)
            keep = [i for i, l in enumerate(labels) if self.events_set is None or l in self.events_set]
            ts = self.encoder._frame_to_time(np.arange(scores.shape[1] + 1))
            self._psds = IntersectionPSDS(*self._psds_tables, [labels[i] for i in keep], ts, **self.PSDS_ARGS)
            self._psds_cols = None if len(keep) == len(labels) else torch.tensor(keep, device=scores.device)
        if self._psds_cols is not None:
            scores = scores.index_select(2, self._psds_cols)
        self._psds.update(scores, paths)

    def psds(self):
        """-> (psds, {class: single-class psds}) with the arguments of passt_cnn/train.py:174-186."""
        if self._psds_tables is None:
            raise RuntimeError("AudiosetStrongEvaluator.psds() needs ground_truth= and audio_durations= at construction")
        if self._psds is None:
            raise RuntimeError("AudiosetStrongEvaluator.psds() called before any step")
        return self._psds.compute()

    def forward(self, feat, pad_mask):
        """-> strong [B, C, T], weak [B, C], at_out [B, C] (None for the closed set) in the encoder's class order."""
        if self.mode == "open_vocabulary":
            q = self.net.at_query
            q = ([t.detach().index_select(0, self._first) for t in q] if isinstance(q, (list, tuple, torch.nn.ParameterList))
                 else q.detach().index_select(0, self._first))                              # get_common_first_query
            strong, weak, other = self.net(feat, pad_mask=pad_mask, query=q, tgt_mask=self._att, **self.kwargs)
            back = lambda x: x.index_select(1, self._inv)                                    # reorder_pred
            return back(strong), back(weak), back(other["at_out"])
        strong, weak, other = self.net(feat, pad_mask=pad_mask, **self.kwargs)
        return strong, weak, other.get("at_out")

    def _enqueue(self, strong, paths):
        if strong.shape[0] > len(paths):
            raise IndexError("list index out of range")     # (batched_decode_preds' contract)
        n = strong.shape[0]
        st = self._stage[self._n % 2]
        self._n += 1
        raw, post = _scores_device(strong, n, self.median_filter, self.filter_type, None, False)
        job = {"paths": list(paths), "frames": strong.shape[-1], "stage": st, "raw": st.put("raw", raw),
               "post": st.put("post", post) if post is not None else None}
        if self._psds_tables is not None:
            self._psds_update(post if post is not None else raw, paths[:n])
        st.mark()
        return job

    def _finish(self, job):
        if job is None:
            return
        job["stage"].wait()
        raw, post = _scores_tables(job["raw"].numpy(), job["post"].numpy() if job["post"] is not None else None, job["paths"],
                                   self.encoder, None, job["frames"])
        if self.events_set is not None:
            extra = set(self.encoder.labels) - set(self.events_set)
            post = remove_extra_events(post, extra)
        self._raw.update(raw)
        self._post.update(post)

    def flush(self):
        job, self._pending = self._pending, None
        self._finish(job)

    @property
    def scores(self):
        """audio_id -> post-processed score DataFrame of every batch so far."""
        self.flush()
        return self._post

    @property
    def raw_scores(self):
        self.flush()
        return self._raw

    def compute_map(self):
        return self.map.compute()

    def mean_psds_per_type(self, single_psds):
        return mean_psds_per_type(single_psds, self.type_dict)

    @torch.no_grad()
    def step(self, wav, labels, pad_mask, paths):
        self.net.eval()
        ext = self.net.get_feature_extractor()
        ext.eval()
        feat = ext.logmel(wav)                                        # preprocess_eval (passt_cnn/train.py:150-153)
        strong, weak, at_out = self.forward(feat, pad_mask)
        self.map.update(weak if self.mode == "closed" else at_out, labels.sum(-1) >= 1)
        job = self._enqueue(strong, paths)
        self._finish(self._pending)                                   # the previous batch's tables, under this batch's filters
        self._pending = job
        return strong, weak, at_out
