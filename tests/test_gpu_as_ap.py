"""Multilabel average precision on the device (csrc/metrics.hip, evaluation.MultilabelAveragePrecision) against a float64 numpy
restatement of torchmetrics 0.11's binary_average_precision with thresholds=None, as the AudioSet-Strong validation loops use it."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu
DEV = "cuda"

from transformer4sed_amd.evaluation import AP_CHUNK, MultilabelAveragePrecision  # noqa: E402

C = 407


def tm_binary_ap(preds, target):
    """torchmetrics 0.11 _binary_clf_curve + _binary_precision_recall_curve_compute + _reduce_average_precision, one class, float64."""
    preds, target = np.asarray(preds, np.float64), np.asarray(target, np.float64)
    order = np.argsort(-preds, kind="stable")
    p, t = preds[order], target[order]
    distinct = np.where(np.diff(p))[0]
    thr = np.r_[distinct, t.size - 1]
    tps = np.cumsum(t)[thr]
    fps = 1 + thr - tps
    with np.errstate(invalid="ignore", divide="ignore"):
        precision = tps / (tps + fps)
        recall = tps / tps[-1]
    precision = np.r_[precision[::-1], 1.0]
    recall = np.r_[recall[::-1], 0.0]
    return -np.sum((recall[1:] - recall[:-1]) * precision[:-1])


def tm_format(preds):
    """per-batch formatting rule of torchmetrics 0.11: any score outside [0, 1] -> sigmoid of the whole batch."""
    if not ((preds >= 0) & (preds <= 1)).all():
        return torch.sigmoid(preds)
    return preds


def ref_per_class(preds, target):
    preds, target = np.asarray(preds), np.asarray(target)
    return np.array([tm_binary_ap(preds[:, c], target[:, c]) for c in range(preds.shape[1])])


def synth(N, seed, special=True):
    """scores on 256 levels (heavy ties, +-0.0 among them), sparse positives; class 0 no positive, 1 one, 2 all."""
    rng = np.random.RandomState(seed)
    preds = (np.round(rng.rand(N, C) * 255) / 255).astype(np.float32)
    zero = preds == 0
    preds[zero & (rng.rand(N, C) < 0.5)] = -0.0
    preds[rng.rand(N, C) < 0.01] = -0.0
    rate = rng.uniform(0.005, 0.3, size=C)
    target = (rng.rand(N, C) < rate).astype(np.int64)
    # correlate the target with the score so the AP is not ~ the prevalence
    target |= (rng.rand(N, C) < preds * 0.2).astype(np.int64)
    if special:
        target[:, 0] = 0
        target[:, 1] = 0
        target[rng.randint(N), 1] = 1
        target[:, 2] = 1
    return preds, target


@pytest.mark.parametrize("N", [1, 63, 64, 1000, 16901, 2 * AP_CHUNK + 1])
def test_ap_vs_torchmetrics_restatement(N):
    preds, target = synth(N, seed=N)
    assert (np.signbit(preds) & (preds == 0)).any() or N < 64
    m = MultilabelAveragePrecision(C, average=None)
    m.update(torch.from_numpy(preds).to(DEV), torch.from_numpy(target).to(DEV))
    got = m.compute().cpu().numpy().astype(np.float64)
    ref = ref_per_class(preds, target)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert np.isnan(got[0])
    err = np.abs(got[ok] - ref[ok]).max()
    assert err <= 2e-6, err
    if N > 1:
        assert got[2] == 1.0 and 0 < got[1] <= 1.0
    ap, npos = m.per_class()
    assert np.array_equal(npos.cpu().numpy(), target.sum(0))
    # macro / weighted exclude the NaN classes, with torchmetrics' warning
    for avg in ("macro", "weighted"):
        m.average = avg
        with pytest.warns(UserWarning, match="Ignoring these classes in " + avg):
            val = float(m.compute())
        w = target.sum(0)[ok].astype(np.float64)
        want = ref[ok].mean() if avg == "macro" else (ref[ok] * w / w.sum()).sum()
        assert abs(val - want) <= 2e-6, (avg, val, want)
    if N >= 64:
        sk = pytest.importorskip("sklearn.metrics")
        for c in np.nonzero(ok)[0][:40]:
            assert abs(got[c] - sk.average_precision_score(target[:, c], preds[:, c])) <= 2e-6


def test_ap_chunked_path_is_bit_identical():
    preds, target = synth(16901, seed=3)
    p, t = torch.from_numpy(preds).to(DEV), torch.from_numpy(target).to(DEV)
    outs = []
    for chunk in (AP_CHUNK, 1000, 777):
        m = MultilabelAveragePrecision(C, average=None, chunk=chunk)
        m.update(p, t)
        outs.append(m.per_class()[0].cpu().numpy())
    assert np.array_equal(outs[0], outs[1], equal_nan=True) and np.array_equal(outs[0], outs[2], equal_nan=True)


def test_accumulation_formatting_and_determinism():
    preds, target = synth(3000, seed=7)
    p, t = torch.from_numpy(preds).to(DEV), torch.from_numpy(target).to(DEV)
    one = MultilabelAveragePrecision(C, average=None)
    one.update(p, t)
    ref = one.per_class()[0].cpu().numpy()
    # uneven updates (capacity grows several times): bit-identical
    many = MultilabelAveragePrecision(C, average=None)
    cuts = [0, 1, 33, 34, 500, 1777, 2999, 3000]
    torch.cuda.set_sync_debug_mode("error")         # update() never waits for the device
    try:
        for a, b in zip(cuts[:-1], cuts[1:]):
            many.update(p[a:b], t[a:b].float())      # (a {0, 1}-valued float target, as passt_cnn/train.py:267 passes)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert many.cap >= 3000 and many.n == 3000
    assert np.array_equal(many.per_class()[0].cpu().numpy(), ref, equal_nan=True)
    # clip permutation: bit-identical
    perm = torch.from_numpy(np.random.RandomState(1).permutation(3000)).to(DEV)
    pm = MultilabelAveragePrecision(C, average=None)
    pm.update(p[perm], t[perm])
    assert np.array_equal(pm.per_class()[0].cpu().numpy(), ref, equal_nan=True)
    # two computes: identical
    one.average = "macro"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a, b = one.compute(), one.compute()
    assert a.dim() == 0 and a.dtype == torch.float32 and torch.equal(a, b)
    # a logit batch is sigmoid-ed, a probability batch is not, in the same run
    rng = np.random.RandomState(5)
    logits = torch.from_numpy((rng.randn(200, C) * 3).astype(np.float32)).to(DEV)
    probs = torch.from_numpy(rng.rand(300, C).astype(np.float32)).to(DEV)
    tg = torch.from_numpy((rng.rand(500, C) < 0.2).astype(np.int64)).to(DEV)
    mix = MultilabelAveragePrecision(C, average=None)
    mix.update(logits, tg[:200])
    mix.update(probs, tg[200:])
    stored = mix.scores[:, :500].t()
    assert torch.allclose(stored[:200], torch.sigmoid(logits), rtol=0, atol=1e-7)
    assert torch.equal(stored[200:], probs)
    allp = torch.cat([tm_format(logits), tm_format(probs)]).cpu().numpy()
    want = ref_per_class(allp, tg.cpu().numpy())
    got = mix.per_class()[0].cpu().numpy()
    assert np.abs(got - want).max() <= 2e-6


def test_compute_errors_and_options():
    with pytest.raises(NotImplementedError):
        MultilabelAveragePrecision(C, average="micro")
    m = MultilabelAveragePrecision(4, average="macro", compute_on_step=False)
    with pytest.raises(RuntimeError):
        m.compute()
    x = torch.rand(5, 4, device=DEV)
    m(x, torch.full((5, 4), 2, device=DEV))           # update accepts it; compute raises
    with pytest.raises(RuntimeError, match="target"):
        m.compute()
    m.reset()
    x[0, 0] = float("nan")
    m.update(x, torch.ones(5, 4, device=DEV, dtype=torch.long))
    with pytest.raises(RuntimeError, match="NaN"):
        m.compute()
    m.reset()
    m.update(torch.rand(5, 4, device=DEV), torch.ones(5, 4, device=DEV, dtype=torch.long))
    assert float(m.compute()) == 1.0


def test_large_batch_formatting_flag_spans_workgroups():
    """One update of a whole split (the flag reduction then runs on several workgroups): a single score outside [0, 1] at the END of the
    batch still sends the whole batch through the sigmoid; a NaN or a bad target there is still reported at compute()."""
    rng = np.random.RandomState(9)
    N = 16901
    x = torch.from_numpy(rng.rand(N, C).astype(np.float32)).to(DEV)
    t = torch.from_numpy((rng.rand(N, C) < 0.1).astype(np.int64)).to(DEV)
    m = MultilabelAveragePrecision(C, average=None)
    m.update(x, t)
    assert torch.equal(m.scores[:, :N].t(), x)                        # in range: stored as given
    y = x.clone()
    y[-1, -1] = 1.5
    m2 = MultilabelAveragePrecision(C, average=None)
    m2.update(y, t)
    assert torch.allclose(m2.scores[:, :N].t(), torch.sigmoid(y), rtol=0, atol=1e-7)
    y[-1, -1] = float("nan")
    t2 = t.clone()
    t2[-1, 0] = 3
    m3 = MultilabelAveragePrecision(C, average=None)
    m3.update(y, t)
    with pytest.raises(RuntimeError, match="NaN"):
        m3.compute()
    m4 = MultilabelAveragePrecision(C, average=None)
    m4.update(x, t2)
    with pytest.raises(RuntimeError, match="target"):
        m4.compute()
