"""The per-batch bodies of the validation / test loops, `Evaluator` (DESED) and `AudiosetStrongEvaluator`: both queue a batch's filters and
device-to-host copies, feed the metric accumulators on the device and build its score tables while the GPU runs the next forward."""
import os
from collections import namedtuple
from pathlib import Path

import pandas as pd
import torch

from ..ops import h2d
from .codec import (_events_device, _events_frames, _scores_device, _scores_tables, check_filter_type, frame_boundaries,
                    scaled_median_window, write_sed_scores)
from .event_f1 import EventSegmentF1
from .ground_truth import _table
from .metrics import MultilabelAveragePrecision, WeakF1Macro
from .psds import IntersectionPSDS, mean_psds_per_type

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


def _enqueue_scores(stage, strong, weak, paths, median_filter, filter_type, weak_mask, sebb=None):
    """Device half of one model's score tables: filters, raw and post-processed scores on their way into `stage`'s pinned buffers.
    -> (job for `_finish_scores`, the scores the metrics take, still on the device; None for an empty batch).  `stage.mark()` is the caller's."""
    if strong.shape[0] > len(paths):
        raise IndexError("list index out of range")     # (batched_decode_preds' contract)
    job = {"paths": list(paths), "n": strong.shape[0], "frames": strong.shape[-1], "stage": stage, "raw": None, "post": None}
    if job["n"] == 0:
        return job, None
    raw, post = _scores_device(strong, job["n"], median_filter, filter_type, weak, weak_mask, sebb)
    job["raw"] = stage.put("raw", raw)
    job["post"] = stage.put("post", post) if post is not None else None
    return job, post if post is not None else raw


def _finish_scores(job, encoder):
    """Host half: waits for the job's copies (its stage's event, nothing else) -> (scores_raw, scores_post) of the batch."""
    job["stage"].wait()
    if job["n"] == 0:
        return {}, {}
    return _scores_tables(job["raw"].numpy(), job["post"].numpy() if job["post"] is not None else None, job["paths"], encoder, None,
                          job["frames"])


class _GroundTruthMetrics:
    """The ground truth both evaluators may be given: two tables that go together; a result asked for without them or a batch is refused."""

    def _pair_tables(self, ground_truth, audio_durations):
        if (ground_truth is None) != (audio_durations is None):
            raise ValueError("ground_truth and audio_durations go together")
        self._psds_tables = None if ground_truth is None else (_table(ground_truth), _table(audio_durations))

    def _made(self, acc, method):
        if self._psds_tables is None:
            raise RuntimeError(f"{type(self).__name__}.{method}() needs ground_truth= and audio_durations= at construction")
        if acc is None:
            raise RuntimeError(f"{type(self).__name__}.{method}() called before any step")
        return acc


class Evaluator(_GroundTruthMetrics):
    """Per-batch body of Trainer.validation / Trainer.test (recipes/desed/finetune/train.py:296-366, 427-466): eval-mode frontend,
    student + EMA-teacher forward with `val_kwargs` (17 sliding windows, temperature 0.5, pad mask), weak-F1 accumulation, score
    tables (soft weak mask + per-class scipy median) and half-point event lists (hard mask + torch median).

    The host half of a model's decode (DataFrames, event lists: ~7 ms per model and batch of 32) runs while the GPU is busy with the NEXT
    forward: `step` queues the student's forward, filters and device-to-host copies, finishes the previous batch's teacher tables, queues
    the teacher, finishes the student's tables and returns with the teacher's still pending.  `scores`, `events`, `event_frame`,
    `write` and `flush` complete whatever is pending first, so what a caller reads is always whole.  (The synchronous form -- decode
    right behind each forward with `.cpu()` -- left the GPU idle for 14 of a 212 ms validation step, tools/ablate/step_gaps.sh.)

    With `ground_truth=` / `audio_durations=` the post-processed scores and the binarised frames also feed, still on the device, the
    PSDS accumulators (`psds()`) and one `EventSegmentF1` per model (`f1()`).

    `sebb=`: a `sebb.SebbPostprocessor`; its bounding-box scores take the place of both filters -- of the scipy filter behind the
    post-processed tables and the PSDS, and of the torch median behind the half-point events and the F1."""

    PSDS_ARGS = {"psds1": dict(dtc_threshold=0.7, gtc_threshold=0.7, cttc_threshold=None, alpha_ct=0, alpha_st=1),      # train.py:229-253
                 "psds2": dict(dtc_threshold=0.1, gtc_threshold=0.1, cttc_threshold=0.3, alpha_ct=0.5, alpha_st=1)}

    def __init__(self, net, ema_net, encoder, config, ground_truth=None, audio_durations=None, sebb=None):
        self.net, self.ema_net, self.encoder, self.config, self.sebb = net, ema_net, encoder, config, sebb
        self._pair_tables(ground_truth, audio_durations)
        self._psds = None           # who -> {"psds1": IntersectionPSDS, "psds2": ...}, made at the first batch (it brings the frame count)
        self._f1 = None             # who -> EventSegmentF1, likewise
        tr = config["training"]
        self.median_filter = scaled_median_window(tr["median_window"])
        self.filter_type = check_filter_type(tr.get("filter_type", "median"))
        self.weak_mask = tr.get("weak_mask", False)
        self._scores = ScoreBufferTuple(dict(), dict(), dict(), dict())
        self._events = {"student": [], "teacher": []}
        self.weak_f1 = {"student": WeakF1Macro(len(encoder.labels)), "teacher": WeakF1Macro(len(encoder.labels))}
        self._stage = {"student": _HostStage(), "teacher": _HostStage()}
        self._pending = {}

    # ---- device half of one model's decode: filters, thresholds, device-to-host copies into pinned buffers, one event
    def _enqueue(self, who, strong, weak, paths):
        st = self._stage[who]
        job, scores = _enqueue_scores(st, strong, weak, paths, self.median_filter, self.filter_type, self.weak_mask, self.sebb)
        job["who"], n = who, job["n"]
        if self._psds_tables is not None and n > 0:
            self._psds_update(who, scores, paths[:n])
        binm = _events_device(strong, weak, [0.5], self.median_filter, self.sebb)[0]
        if self._psds_tables is not None and n > 0:
            self._f1_update(who, binm, paths[:n])
        job["bin"] = st.put("bin", binm)
        st.mark()
        return job

    def _psds_update(self, who, scores, paths):
        """Feeds the post-processed scores [n, frames, n_class] to the model's psds1 / psds2 accumulators: stream-ordered sweeps, the
        host waits for nothing (10 classes: the accumulators keep the sweep's padded event slots)."""
        if self._psds is None:
            ts = frame_boundaries(self.encoder, scores.shape[1])
            self._psds = {w: {k: IntersectionPSDS(*self._psds_tables, self.encoder.labels, ts, **a) for k, a in self.PSDS_ARGS.items()}
                          for w in ("student", "teacher")}
        for acc in self._psds[who].values():
            acc.update(scores, paths)

    def _f1_update(self, who, binm, paths):
        """Feeds the binarised, median-filtered frames [n, frames, n_class] (bool, still on the device) to the model's `EventSegmentF1`:
        one stream-ordered launch, the host waits for nothing.  Like the reference's loops over the files of the ground truth, clips
        the ground truth does not list are left out."""
        if self._f1 is None:
            ts = frame_boundaries(self.encoder, binm.shape[1])
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
        f1 = self._made(self._f1, "f1")
        out = {"class_wise": {}}
        for who, tag in (("student", "s"), ("teacher", "t")):
            res = f1[who].compute()
            out["class_wise"][tag] = res.pop("class_wise")
            out.update({f"{k}/{tag}": v for k, v in res.items()})
        return out

    def psds(self):
        """The validation's four PSDS numbers (train.py:370-398) under the reference's log keys, and the single-class dicts under
        "single": {"psds1/s": ..., "psds2/s": ..., "psds1/t": ..., "psds2/t": ..., "single": {same keys: {class: psds}}}."""
        psds = self._made(self._psds, "psds")
        out = {"single": {}}
        for who, tag in (("student", "s"), ("teacher", "t")):
            for k, acc in psds[who].items():
                out[f"{k}/{tag}"], out["single"][f"{k}/{tag}"] = acc.compute()
        return out

    # ---- host half
    def _finish(self, job):
        if job is None:
            return
        who = job["who"]
        raw, post = _finish_scores(job, self.encoder)
        getattr(self._scores, "raw_" + who).update(raw)
        getattr(self._scores, "post_" + who).update(post)
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


def remove_extra_events(scores_buffer, events):
    """passt_cnn/train.py:169-172 (`_remove_extra_events`): drops the columns of `events` from every score table, in place."""
    events = list(events)
    for audio_id, df in scores_buffer.items():
        scores_buffer[audio_id] = df.drop(events, axis=1)
    return scores_buffer


class AudiosetStrongEvaluator(_GroundTruthMetrics):
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
            from ..dasm_trainer import common_type_mask, get_att_mask, load_type_dict
            self.type_dict = load_type_dict(type_dict if type_dict is not None else config["dataset"]["event_state"])
            self.mask = common_type_mask(encoder.labels, self.type_dict, next(net.parameters()).device)
            # the common-first permutation, its inverse and the attention mask, once: per batch only index_select runs (the reference's
            # boolean-mask forms, dasm_trainer.get_common_first_query / reorder_pred, wait for the device on every call)
            self._first = torch.cat([torch.nonzero(self.mask).reshape(-1), torch.nonzero(~self.mask).reshape(-1)])
            self._inv = torch.argsort(self._first)
            self._att = get_att_mask(self.mask)
        elif type_dict is not None:
            from ..dasm_trainer import load_type_dict
            self.type_dict = load_type_dict(type_dict)
        self.map = MultilabelAveragePrecision(len(encoder.labels), average="macro", compute_on_step=False)
        self._post, self._raw = {}, {}
        self._stage = [_HostStage(), _HostStage()]
        self._n = 0
        self._pending = None
        self._pair_tables(ground_truth, audio_durations)
        self._psds = None           # IntersectionPSDS over the classes of events_set, made at the first batch
        self._psds_cols = None

    def _psds_update(self, scores, paths):
        """Post-processed scores [n, frames, n_class] -> the PSDS accumulator, the classes outside `events_set` dropped first like
        train.py:174-175.  With more than 16 classes each update reads one small count back (IntersectionPSDS)."""
        if self._psds is None:
            labels = list(self.encoder.labels)
            keep = [i for i, l in enumerate(labels) if self.events_set is None or l in self.events_set]
            ts = frame_boundaries(self.encoder, scores.shape[1])
            self._psds = IntersectionPSDS(*self._psds_tables, [labels[i] for i in keep], ts, **self.PSDS_ARGS)
            self._psds_cols = None if len(keep) == len(labels) else torch.tensor(keep, device=scores.device)
        if self._psds_cols is not None:
            scores = scores.index_select(2, self._psds_cols)
        self._psds.update(scores, paths)

    def psds(self):
        """-> (psds, {class: single-class psds}) with the arguments of passt_cnn/train.py:174-186."""
        return self._made(self._psds, "psds").compute()

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
        st = self._stage[self._n % 2]
        self._n += 1
        job, scores = _enqueue_scores(st, strong, None, paths, self.median_filter, self.filter_type, False)
        if self._psds_tables is not None and scores is not None:
            self._psds_update(scores, paths[:job["n"]])
        st.mark()
        return job

    def _finish(self, job):
        if job is None:
            return
        raw, post = _finish_scores(job, self.encoder)
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

    def compute_auroc(self, max_fpr=None):
        """The AUC and d' AudioSet systems report beside the mAP, from the storage `compute_map` sorts:
        {"auroc": macro AUROC (sklearn's standardised partial area with `max_fpr`), "d_prime": sqrt(2) ndtri(macro AUROC),
        "per_class": int64 [C][8]}."""
        from .roc import storage_auroc
        return storage_auroc(self.map, max_fpr)

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
