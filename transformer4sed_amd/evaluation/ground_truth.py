"""The ground truth of the clip-wise accumulators (`IntersectionPSDS`, `EventSegmentF1`): one parser from the event table to CSR arrays
in integer microseconds, and the state both keep around it (device copy made at the first update, status word, clips scored so far)."""
from collections import namedtuple
from pathlib import Path

import numpy as np
import pandas as pd
import torch


def _microseconds(x):
    """Times rounded to 6 decimals (sed_scores_eval's time_decimals), as int64 microseconds."""
    return np.rint(np.round(np.asarray(x, dtype=np.float64), 6) * 1e6).astype(np.int64)


def _table(x):
    return x if isinstance(x, pd.DataFrame) else pd.read_csv(x, sep="\t")


GroundTruth = namedtuple("GroundTruth", "clip_ids clip_index gt_ptr gt gt_clips")


def build_ground_truth(ground_truth, event_classes, clip_ids=None, max_clip_events=None, owner="", nan_to_num=False,
                       refuse_negative_onset=False):
    """`ground_truth`: TSV path or DataFrame (filename, onset, offset, event_label); clips are keyed by the filename's stem, a row with a
    NaN label is a clip without events.  `clip_ids`: the fixed clip order (a clip outside it is an error), or None to number the clips
    by first appearance.  `max_clip_events`: the per-clip cap, refused in `owner`'s name.  `nan_to_num`: NaN times (rows without a
    label) become 0.  -> GroundTruth(clip_ids, clip_index {stem: row}, gt_ptr int32 [n_clips + 1], gt int64 [n, 3] = class, onset_us,
    offset_us sorted by (clip, class, onset, offset), gt_clips = the clips of the table)."""
    gt = _table(ground_truth)
    cls_index = {c: i for i, c in enumerate(event_classes)}
    fixed = clip_ids is not None
    clip_ids = list(clip_ids) if fixed else []
    clip_index = {a: i for i, a in enumerate(clip_ids)}
    per_clip = [[] for _ in clip_ids]
    gt_clips = set()
    clean = np.nan_to_num if nan_to_num else (lambda a: a)
    on_us, off_us = (_microseconds(clean(gt[k].to_numpy(dtype=np.float64))) for k in ("onset", "offset"))
    for f, label, on, off in zip(gt["filename"], gt["event_label"], on_us.tolist(), off_us.tolist()):
        a = Path(f).stem
        if a not in clip_index:
            if fixed:
                raise ValueError(f"ground-truth clip {a!r} is missing from audio_durations")
            clip_index[a] = len(clip_ids)
            clip_ids.append(a)
            per_clip.append([])
        gt_clips.add(a)
        if pd.isna(label):
            continue                                # (a clip without events)
        if label not in cls_index:
            raise ValueError(f"ground-truth label {label!r} is not one of event_classes")
        if off <= on:
            raise ValueError(f"ground-truth event of {a!r} with offset <= onset")
        if refuse_negative_onset and on < 0:
            raise ValueError(f"ground-truth event of {a!r} with a negative onset")
        per_clip[clip_index[a]].append((cls_index[label], on, off))
    ptr, flat = [0], []
    for a, ev in zip(clip_ids, per_clip):
        if max_clip_events is not None and len(ev) > max_clip_events:
            raise NotImplementedError(f"{owner}: clip {a!r} has {len(ev)} events (at most {max_clip_events})")
        flat += sorted(ev)
        ptr.append(len(flat))
    return GroundTruth(clip_ids, clip_index, np.asarray(ptr, dtype=np.int32), np.asarray(flat, dtype=np.int64).reshape(-1, 3), gt_clips)


class ClipAccumulator:
    """What `IntersectionPSDS` and `EventSegmentF1` share: classes, frame boundaries `ts_us`, the parsed ground truth (`clip_ids`,
    `_clip_index`, `gt_ptr`, `gt`, `_gt_clips`), its copy on the device of the first update with the status word `_status`, and `_seen`."""

    _unknown_clip = "the ground truth"              # the table a clip is missing from, in `_rows`' message

    def _set_classes(self, event_classes):
        self.event_classes = list(event_classes)
        C = self.num_classes = len(self.event_classes)
        if C == 0 or len(set(self.event_classes)) != C:
            raise ValueError("event_classes must be a non-empty list of distinct names")
        return C

    def _set_timestamps(self, timestamps, max_frames, holder):
        """-> the frame durations in microseconds."""
        ts = np.asarray(timestamps, dtype=np.float64)
        if ts.ndim != 1 or ts.size < 2:
            raise ValueError("timestamps must be [T + 1] frame boundaries")
        self.num_frames = ts.size - 1
        if self.num_frames > max_frames:
            raise NotImplementedError(f"{type(self).__name__}: {self.num_frames} frames per clip, the {holder} holds at most {max_frames}")
        self.ts_us = _microseconds(ts)
        return np.diff(self.ts_us)

    def _set_ground_truth(self, parsed):
        self.clip_ids, self._clip_index, self.gt_ptr, self.gt, self._gt_clips = parsed
        self._dev = self._status = None             # made at the first update, on its device

    def reset(self):
        """Forgets every scored clip (a new validation epoch); the ground truth stays where it is."""
        self._seen = set()
        if self._status is not None:
            self._status.zero_()

    def _device_state(self, dev):
        """-> (dict(device, ts, ptr, cls, on, off) on `dev`, made just now?): uploaded once, with the status word."""
        if self._dev is None:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            pad = lambda a: a if a.size else np.zeros(1, dtype=a.dtype)      # (no null pointer for a ground truth without events)
            self._dev = dict(device=dev, ts=up(self.ts_us) if self.ts_us is not None else None, ptr=up(self.gt_ptr),
                             cls=up(pad(self.gt[:, 0].astype(np.int32))), on=up(pad(self.gt[:, 1])), off=up(pad(self.gt[:, 2])))
            self._status = torch.zeros(1, dtype=torch.int32, device=dev)
            return self._dev, True
        if self._dev["device"] != dev:
            raise ValueError(f"batches on different devices ({self._dev['device']}, {dev})")
        return self._dev, False

    def _rows(self, filenames):
        """-> (ground-truth rows of the clips, their stems); refuses a clip it does not know or has scored."""
        rows, batch = [], set()
        for f in filenames:
            a = Path(f).stem
            if a not in self._clip_index:
                raise ValueError(f"clip {a!r} is missing from {self._unknown_clip}")
            if a in self._seen or a in batch:
                raise ValueError(f"clip {a!r} was scored twice")
            batch.add(a)
            rows.append(self._clip_index[a])
        return rows, batch
