"""Score tables and event decoding with the reference's call contracts, the per-frame work done on the device.

Mirrors (same names, argument meaning, return types):
  * `Encoder`                         src/codec/encoder.py:7-84   (frame<->time mapping, decode_strong, find_contiguous_regions)
  * `batched_decode_preds`            src/codec/decoder.py:38-103 (soft weak mask, scipy median / max filter, score DataFrames)
  * `decode_pred_batch_fast`          src/codec/decoder.py:15-35  (hard weak mask, median_filter_torch, threshold, events)
  * `create_score_dataframe` / `write_sed_scores`  the sed_scores_eval table layout the reference hands to its metric code
    (recipes/desed/finetune/train.py:470-478; third-party package, restated from its public layout: parity unpinned)

Masking, both median filters and the thresholding run in `sed_median_filter` launches over the whole batch (bit-exact with the
reference's per-clip, per-class scipy / torch loops, tests/test_gpu_eval.py); the host only slices the result into tables."""
import math
import os
from pathlib import Path

import numpy as np
import pandas as pd

from .. import filter as dev_filter


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


def frame_boundaries(encoder, T):
    """The T + 1 frame boundaries in seconds that all clips of T frames share."""
    return encoder._frame_to_time(np.arange(T + 1))


def scaled_median_window(windows):
    """recipes/desed/finetune/train.py:221-227: the per-class windows, given for 156 frames, at the 1000 frames of a clip."""
    return [int(i / 156 * 1000) for i in windows]


def check_filter_type(filter_type):
    if filter_type not in ("median", "max"):
        raise ValueError("filter_type must be 'median' or 'max'")
    return filter_type


def _scores_device(strong_preds, n, filter, filter_type, weak_preds, need_weak_mask, sebb=None):
    """Device half of `batched_decode_preds`: (raw, post) [n, frames, n_class] fp32 device tensors (post None without a filter).  `sebb`:
    a `sebb.SebbPostprocessor` whose frame scores take the filter's place."""
    x = strong_preds[:n].detach().transpose(1, 2).contiguous().float()          # [bs, frames, n_class]
    scale = weak_preds[:n].detach().float() if (need_weak_mask and weak_preds is not None) else None
    raw = x if scale is None else x * scale.unsqueeze(1)
    post = None
    if sebb is not None:
        post = sebb.scores_btc(x, scale, check=False)         # (no read from the device here: the kernel clamps what the check refuses)
    elif filter:
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
        ts = frame_boundaries(encoder, len(r))
        classes = encoder.labels[:r.shape[1]]
        scores_raw[audio_id] = create_score_dataframe(r, ts, classes)
        scores_post[audio_id] = create_score_dataframe(p, ts, classes) if p is not None else scores_raw[audio_id]
    return scores_raw, scores_post


def batched_decode_preds(strong_preds, filenames, encoder, filter=7, filter_type="median", pad_indx=None, weak_preds=None,
                         need_weak_mask=None, sebb=None):
    """src/codec/decoder.py:38-103.  strong_preds [bs, n_class, frames] (device tensor), weak_preds [bs, n_class].
    Returns (scores_raw, scores_postprocessed): dicts audio_id -> score DataFrame.  `filter`: per-class window list.  `sebb` (not in the
    reference): a `SebbPostprocessor` that post-processes in place of `filter` / `filter_type`."""
    check_filter_type(filter_type)
    n = min(strong_preds.shape[0], len(filenames))      # the reference loops over strong_preds and indexes filenames[j]
    if strong_preds.shape[0] > len(filenames):
        raise IndexError("list index out of range")     # same failure as the reference's filenames[j]
    if n == 0:
        return {}, {}
    raw, post = _scores_device(strong_preds, n, filter, filter_type, weak_preds, need_weak_mask, sebb)
    return _scores_tables(raw.cpu().numpy(), post.cpu().numpy() if post is not None else None, filenames, encoder, pad_indx,
                          strong_preds.shape[-1])


def _events_device(outputs, weak_preds, thresholds, median_filter, sebb=None):
    """Device half of `decode_pred_batch_fast`: one bool tensor [batch, frames, n_class] per threshold.  With `sebb` the frames of the
    boxes whose confidence exceeds the threshold, in place of the median-filtered frames above it."""
    x = outputs.detach().transpose(1, 2).contiguous().float()
    out = []
    for c_th in thresholds:
        keep = (weak_preds.detach() >= c_th).float()              # output[b, :, c] = 0 where weak_preds[b, c] < c_th
        post = dev_filter._run(x, list(median_filter), 0, keep) if sebb is None else sebb.scores_btc(x, keep, check=False)
        out.append(post > c_th)
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
