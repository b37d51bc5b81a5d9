"""Event-based and segment-based F1 on the device (csrc/event_f1.hip), and the reference's entry point on top."""
import os
from pathlib import Path

import numpy as np
import pandas as pd
import torch

from ..ops import call, h2d
from .ground_truth import ClipAccumulator, _microseconds, _table, build_ground_truth

F1_MAX_FRAMES = 1024           # csrc/event_f1.hip: frames per clip
F1_MAX_CLIP_EVENTS = 256       # ... ground-truth events of one clip
F1_MAX_ESTIMATES = 512         # ... estimated events of one class in one clip
F1_MAX_SEGMENTS = 64           # ... segments per clip (one bit each)
F1_COUNTS = ("n_ref", "n_sys", "tp", "seg_tp", "seg_fp", "seg_fn")


class EventSegmentF1(ClipAccumulator):
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
        self._set_classes(event_classes)
        if not float(t_collar) >= 0 or not 0.0 <= float(percentage_of_length) <= 1.0:
            raise ValueError("t_collar must not be negative and percentage_of_length must lie in [0, 1]")
        self.collar_us = int(_microseconds(t_collar))
        self.p = float(percentage_of_length)
        self.res_us = int(_microseconds(time_resolution))
        if self.res_us <= 0:
            raise ValueError("time_resolution must be a positive number of microseconds")
        self.ts_us, self.num_frames = None, None
        if timestamps is not None:
            if (self._set_timestamps(timestamps, F1_MAX_FRAMES, "HIP kernel") < 0).any() or self.ts_us[0] < 0:
                raise ValueError("timestamps must not decrease or be negative")
        self._cls_index = {c: i for i, c in enumerate(self.event_classes)}
        self._set_ground_truth(build_ground_truth(ground_truth, self.event_classes, None, F1_MAX_CLIP_EVENTS, "EventSegmentF1",
                                                  nan_to_num=True, refuse_negative_onset=True))     # (NaN: rows without a label)
        self._check_segments(max([int(self.ts_us[-1]) if self.ts_us is not None else 0] + self.gt[:, 2].tolist()))
        self._counts = None                                              # [C, 6], made at the first update, on its device
        self.reset()

    def _check_segments(self, end_us):
        n_seg = -(-int(end_us) // self.res_us)
        if n_seg > F1_MAX_SEGMENTS:
            raise NotImplementedError(f"EventSegmentF1: {n_seg} segments of {self.res_us} us per clip (at most {F1_MAX_SEGMENTS})")

    def reset(self):
        super().reset()
        if self._counts is not None:
            self._counts.zero_()

    # ---- device half
    def _state(self, dev):
        """The ground truth, the counts [C, 6] and the status word on `dev`, made once."""
        k, fresh = self._device_state(dev)
        if fresh:
            self._counts = torch.zeros(self.num_classes, len(F1_COUNTS), dtype=torch.int64, device=dev)
        return k

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
