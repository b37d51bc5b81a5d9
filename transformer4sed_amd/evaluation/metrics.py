"""Clip-level validation metrics: weak F1 (torchmetrics MultilabelF1Score as train.py:277-287 uses it) and multilabel average
precision on HIP kernels (csrc/metrics.hip), with the class-major score storage that `roc.MultilabelAUROC` shares."""
import torch

from ..ops import call

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


class ClassMajorScores:
    """The append / grow / status storage `MultilabelAveragePrecision` and `roc.MultilabelAUROC` share (csrc/metrics.hip): class-major
    `scores` [C][cap] fp32 and `labels` [C][cap] uint8 on the device of the first batch, `n` items so far, torchmetrics' per-batch
    sigmoid rule applied on the device by `sed_ap_append`, and the sticky status word `_checked` reads."""

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

    def _checked(self):
        """Raises on what torchmetrics' argument validation rejects; reads the status word (the one wait for the device)."""
        if self.n == 0:
            raise RuntimeError(f"{type(self).__name__}.compute() called before any update")
        status = int(self._status.item())
        if status & 4:
            raise RuntimeError("Detected the following values in `target`: values outside {0, 1}; expected only 0 and 1")
        if status & 2:
            raise RuntimeError("Detected NaN values in `preds`")


AP_CHUNK = 20000        # clips per LDS sort of sed_ap_compute (its maximum): the validation split (16 891 clips) is one chunk


class MultilabelAveragePrecision(ClassMajorScores):
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

    def per_class(self):
        """-> (ap [C] float64, positives [C] int32), device tensors."""
        self._checked()
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
