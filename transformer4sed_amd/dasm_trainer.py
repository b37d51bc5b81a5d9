"""AudioSet-Strong training steps on the HIP path (BASELINE.json config #5; north_star: "recipes/audioset_strong training loops ... a drop-in"):

`AudiosetStrongTrainer`  the closed-set loop of recipes/audioset_strong/base/passt_cnn/train.py:103-140 (`Trainer.train`): PaSST_CNN with the
                         407-class head, one supervised loss on the frame posteriors.
`DasmTrainer`            recipes/audioset_strong/detect_any_sound/passt/train.py:66-120 (`DASMTrainer.train`): DASM, supervised loss on the
                         frame posteriors + w_AT x supervised loss on the clip-level tagging probabilities of the query decoder.
`OvDasmTrainer`          recipes/audioset_strong/detect_any_sound/passt/open_vocabulary.py:34-96 (`OV_DASM_Trainer.train`): the same step on
                         the "common" classes only, with the common rows of `at_query` handed to the model as external queries.

Both keep the reference's call order per batch -- zero_grad, preprocess (frontend, normalisation, frame_shift with max_shift_frame
2 x sr, mixup with c ~ Beta(10, 0.5) under a coin flip, feature_transformation, pooled weak labels), forward with the config's
train_kwargs, losses, (clip_grad_norm before backward: acts on cleared gradients, a no-op -- kept as one), backward, optimizer step,
scheduler step -- and its RNG consumption (python `random`, numpy, torch CPU generator).  Parameter groups: the closed-set main.py uses
recipes/desed/finetune/cnn_trans/setting.py:get_param_lr = `pmam_trainer.get_param_lr`; the DASM main.py imports a module that does not
exist in the reference (recipes.desed.detect_any_sound...), so the same grouping function is what this package offers for it.

Supervised losses: `loss_function_factory` mirrors src/functional/loss/__init__.py:18-22 for the classes the recipes can name through
`config['class_loss']` -- BCELoss, MSELoss, AsymmetricalFocalLoss, AslLoss -- on one fused HIP kernel (`sed_sup_loss`: value and gradient
in one pass over the [B, 407, 1000] posteriors).  Out of scope: the 'logit' tagging output with its CrossEntropy branch
(train.py:91-96) -- the reference's own DASM.forward cannot produce it (dasm.py, DASM docstring)."""
import json
import os
import random

import numpy as np
import torch

from . import data_aug
from .grad_clip import clip_grad_norm_, max_grad_norm_of
from .ops import call
from .trainer import pool_strong_labels


class SupervisedLoss(torch.autograd.Function):
    """mean-reduced elementwise loss between a prediction and a target of the same shape, value + d loss / d pred from one launch."""

    @staticmethod
    def forward(ctx, pred, target, kind, gamma_pos, gamma_neg, margin):
        # (pred arrives contiguous fp32: `_Loss.__call__` makes it so outside this Function, where autograd records the cast and the copy;
        #  grad mode is off in here, so `requires_grad` of a tensor made here says nothing -- `needs_input_grad` does)
        if pred.dtype != torch.float32 or not pred.is_contiguous():
            raise ValueError("SupervisedLoss: the prediction must be a contiguous float32 tensor")
        target = target.contiguous().float()
        if pred.shape != target.shape:
            raise ValueError(f"prediction {tuple(pred.shape)} and target {tuple(target.shape)} differ in shape")
        loss = torch.zeros(1, dtype=torch.float32, device=pred.device)
        grad = torch.empty_like(pred) if ctx.needs_input_grad[0] else None
        call("sed_sup_loss", pred, target, loss, grad, pred.numel(), int(kind), float(gamma_pos), float(gamma_neg), float(margin))
        ctx.save_for_backward(grad)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None, None, None, None


class _Loss:
    def __init__(self, kind=0, gamma_pos=0.0, gamma_neg=0.0, margin=0.0):
        self.args = (kind, gamma_pos, gamma_neg, margin)

    def __call__(self, input=None, target=None, **kw):
        pred = input if input is not None else kw.get("pred")
        return SupervisedLoss.apply(pred.float().contiguous(), target, *self.args)

    def to(self, device):       # (the recipes call `.to(device)` on the loss module)
        return self


def loss_function_factory(name, kwargs=None):
    """src/functional/loss/__init__.py:18-22 for the elementwise losses of that module.  Keyword arguments the kernel does not implement
    raise instead of being dropped: torch's BCELoss / MSELoss take only their defaults (mean reduction, no weight), the two asymmetric
    losses exactly their constructor arguments (the reference raises a TypeError on any other key too)."""
    kw = dict(kwargs or {})
    if name in ("BCELoss", "MSELoss"):
        defaults = dict(weight=None, size_average=None, reduce=None, reduction="mean")
        bad = {k: v for k, v in kw.items() if k not in defaults or not (v == defaults[k] or (k in ("size_average", "reduce") and v is True))}
        if bad:
            raise NotImplementedError(f"class_loss {name}: the HIP loss is the unweighted mean; unsupported kwargs {bad}")
        return _Loss(kind=0 if name == "BCELoss" else 1)
    allowed = {"AsymmetricalFocalLoss": ("gamma", "zeta"), "AslLoss": ("rp", "rn", "margin")}.get(name)
    if allowed is not None and set(kw) - set(allowed):
        raise TypeError(f"class_loss {name}: unexpected kwargs {sorted(set(kw) - set(allowed))}")
    if name == "AsymmetricalFocalLoss":      # :59-68
        return _Loss(0, kw.get("gamma", 0), kw.get("zeta", 0), 0.0)
    if name == "AslLoss":                    # :25-37
        return _Loss(0, kw["rp"], kw["rn"], kw["margin"])
    raise NotImplementedError(f"class_loss {name!r}: the HIP path offers BCELoss, MSELoss, AsymmetricalFocalLoss and AslLoss")


class AudiosetStrongTrainer:
    """`Trainer` of recipes/audioset_strong/base/passt_cnn/train.py (training step; the validation / test side is evaluation/evaluator.py's)."""

    def __init__(self, net, optimizer, scheduler, config, sr=16000, ddp=None):
        self.net, self.optimizer, self.scheduler, self.config, self.sr, self.ddp = net, optimizer, scheduler, config, sr, ddp
        self.supervised_loss = loss_function_factory(config["class_loss"]["loss_name"], config["class_loss"].get("kwargs"))
        self.max_grad_norm = max_grad_norm_of(config.get("training") or {})     # optional; not the reference's `clip_grad` (see `_finish`)
        from .hostcpu import cap_torch_threads
        cap_torch_threads()

    def preprocess(self, wav, label):
        """train.py:62-83."""
        ext = self.net.get_feature_extractor()
        mel = ext.logmel(wav)                                                   # extractor(wav) + extractor.normalize, one kernel
        mel, label = data_aug.frame_shift(mel, label, net_pooling=mel.shape[-1] / label.shape[-1], max_shift_frame=2 * self.sr)
        if random.random() < 0.5:
            mel, label = data_aug.mixup(mel, label, c=np.random.beta(10, 0.5))
        mel = data_aug.feature_transformation(mel, log=True, norm_std=5.0, **self.config["training"]["transform"])
        return mel, label, pool_strong_labels(label)

    def _forward(self, feat):
        pred = self.net(feat, **self.config[self.net.get_model_name()]["train_kwargs"])
        # (train.py:119-120 raises on a NaN posterior with a host-side .any(): the HIP path leaves the check to the loss value the caller
        #  reads -- a NaN posterior makes it NaN -- instead of stalling the stream every step)
        return pred

    def losses(self, pred, labels, labels_weak):
        strong = self.supervised_loss(pred[0], labels)
        return dict(loss_class_strong=strong, loss_total=strong)

    def _finish(self, terms):
        if self.config["training"].get("clip_grad"):
            pass      # train.py:128-129: clip_grad_norm BEFORE backward, on gradients zero_grad() just cleared: no effect on the step
        terms["loss_total"].backward()
        self._after_backward()
        if self.ddp is not None:
            self.ddp.allreduce_grads(self.net)
        out = {k: v.detach() for k, v in terms.items()}
        if self.max_grad_norm is not None:
            # training["max_grad_norm"] (grad_clip.py): the arena is final here -- `_after_backward` has moved the open-vocabulary queries'
            # gradient into it and the all-reduce has run.  The gradient of an external query INPUT is no parameter's and is not clipped
            out["grad_norm"] = clip_grad_norm_(self.net, self.max_grad_norm)
        self.optimizer.step(None)
        self.scheduler.step()
        return out

    def _after_backward(self):
        pass

    def step(self, wav, labels):
        self.net.train()
        self.optimizer.zero_grad()
        feat, labels, labels_weak = self.preprocess(wav, labels)
        pred = self._forward(feat)
        return self._finish(self.losses(pred, labels, labels_weak))


class DasmTrainer(AudiosetStrongTrainer):
    """`DASMTrainer.train` (recipes/audioset_strong/detect_any_sound/passt/train.py:66-120), out_type 'sigmoid'."""

    def losses(self, pred, labels, labels_weak):
        at = self.supervised_loss(input=pred[2]["at_out"], target=labels_weak)                # :97-101
        strong = self.supervised_loss(pred[0], labels)                                         # :106
        total = strong + at * self.config["training"]["w_AT"]                                  # :108
        return dict(loss_total=total, loss_class_strong=strong, loss_class_at_specific=at)


# ------------------------------------------------------------------------------------------------------------- open vocabulary
def load_type_dict(src):
    """label -> "common" / "rare" (config['dataset']['event_state'], a JSON file, passt_cnn/train.py:215-220), from a path or a dict."""
    if isinstance(src, (str, os.PathLike)):
        with open(src) as f:
            return json.load(f)
    return dict(src)


def common_type_mask(labels, type_dict, device=None):
    """passt_cnn/train.py:206-213: bool [C], True where the label's type is "common"."""
    return torch.tensor([type_dict[l] == "common" for l in labels], dtype=torch.bool, device=device)


def _expand(x, num_gpu):
    # open_vocabulary.py:27-28, 109-111, 124-125: one copy per DataParallel replica; DASM.forward takes [0] of a 3-D query / mask
    return x.unsqueeze(0).expand(num_gpu, *x.shape) if num_gpu > 1 else x


def get_att_mask(mask, num_gpu=1):
    """open_vocabulary.py:98-112: [C, C] bool self-attention mask of the query decoder for common-first queries (True = masked): every
    query sees the common queries and itself, no rare query sees another."""
    common = int(mask.sum())
    n = mask.numel()
    att = torch.ones(n, n, dtype=torch.bool, device=mask.device)
    att[:, :common] = False
    att.fill_diagonal_(False)
    return _expand(att, num_gpu)


def get_common_first_query(at_query, mask, num_gpu=1):
    """open_vocabulary.py:114-133: the query rows reordered common classes first (a list of tables: each one).  Evaluation input: detached."""
    def one(q):
        q = q.detach()
        return _expand(torch.cat([q[mask, :], q[~mask, :]]), num_gpu)
    if isinstance(at_query, (list, tuple, torch.nn.ParameterList)):
        out = [one(q) for q in at_query]
        return out[0] if len(out) == 1 else out
    return one(at_query)


def reorder_pred(pred, mask):
    """open_vocabulary.py:135-145: [batch, C, ...] in common-first order -> the original class order."""
    common = int(mask.sum())
    ret = torch.zeros_like(pred)
    ret[:, mask, ...] = pred[:, :common, ...]
    ret[:, ~mask, ...] = pred[:, common:, ...]
    return ret


class OvDasmTrainer(DasmTrainer):
    """`OV_DASM_Trainer.train` (open_vocabulary.py:34-96): DasmTrainer's step on the common classes only.  Per batch: labels restricted to
    the common classes, zero_grad, preprocess, forward with `query` = the common rows of `at_query` (an autograd-connected slice, so those
    rows train through the external-query path of DASM.forward), losses, backward, optimizer, scheduler -- the reference's order and RNG
    consumption.  The reference slices the queries once per epoch (:45) and reuses that graph for every batch, so its second backward in an
    epoch fails; here every step slices afresh, which is what each of its one-batch epochs computes.

    The slice's gradient is dense: the rows of the rare classes receive zeros, so AdamW still decays them (weight decay and moment decay)
    like the reference's torch AdamW.  The model's backward fills the fused optimiser's gradient arena for the parameters it owns; the
    queries' gradient arrives through autograd instead and `_after_backward` moves it into the arena slot the optimiser and the all-reduce
    read (without that the optimiser would step `at_query` with the arena's zeros).  Under data parallelism the reducer is told to leave
    those slices to `allreduce_grads` (`GradBucketReducer.defer`), which runs after the move: a stage hook would exchange them while they
    still hold zeros."""

    def __init__(self, net, optimizer, scheduler, config, labels, type_dict=None, sr=16000, ddp=None, num_gpu=1):
        super().__init__(net, optimizer, scheduler, config, sr=sr, ddp=ddp)
        self.labels = list(labels)
        self.type_dict = load_type_dict(type_dict if type_dict is not None else config["dataset"]["event_state"])
        self.num_gpu = num_gpu
        if ddp is not None:
            # the queries' gradient enters the arena in `_after_backward`, after the model's stage hooks have fired: reduce it there
            ddp.defer(n for n, _ in net.named_parameters() if n.startswith("at_query"))

    @property
    def device(self):
        return next(self.net.parameters()).device

    @property
    def common_type_mask(self):
        if not hasattr(self, "_common_type_mask"):
            self._common_type_mask = common_type_mask(self.labels, self.type_dict, self.device)
        return self._common_type_mask

    def _common_index(self):
        m = self.common_type_mask
        if getattr(self, "_idx_of", None) is not m:          # (the reference lets a caller set `_common_type_mask` directly)
            self._idx = torch.nonzero(m).reshape(-1).to(self.device)
            self._idx_of = m
        return self._idx

    def get_common_query(self):
        """open_vocabulary.py:20-31, an index_select (no host synchronisation) of the live parameter."""
        idx = self._common_index()
        qs = [self.net.at_query] if isinstance(self.net.at_query, torch.Tensor) else list(self.net.at_query)
        out = [_expand(q.index_select(0, idx), self.num_gpu) for q in qs]
        return out[0] if len(out) == 1 else out

    def get_att_mask(self):
        return get_att_mask(self.common_type_mask, self.num_gpu)

    def get_common_first_query(self):
        return get_common_first_query(self.net.at_query, self.common_type_mask, self.num_gpu)

    def reorder_pred(self, pred):
        return reorder_pred(pred, self.common_type_mask)

    def _after_backward(self):
        arena, flat = getattr(self.net, "_last_grad_arena", None), getattr(self.net, "_flat_layout", None)
        if arena is None or flat is None:
            return
        for n, p in self.net.named_parameters():
            if not n.startswith("at_query") or p.grad is None or n not in flat.offset:
                continue
            o, k = flat.offset[n]
            view = arena[o:o + k].view(p.shape)
            if p.grad.data_ptr() != view.data_ptr():
                view.copy_(p.grad)
                p.grad = view

    def step(self, wav, labels):
        self.net.train()
        query = self.get_common_query()                                                           # :45
        labels = labels.index_select(1, self._common_index().to(labels.device))                   # :49
        self.optimizer.zero_grad()
        feat, labels, labels_weak = self.preprocess(wav, labels)
        pred = self.net(feat, query=query, **self.config[self.net.get_model_name()]["train_kwargs"])
        return self._finish(self.losses(pred, labels, labels_weak))
