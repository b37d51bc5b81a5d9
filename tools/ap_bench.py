#!/usr/bin/env python
"""AudioSet-Strong validation timing, HIP events:
  * MultilabelAveragePrecision.compute() at the validation split's size (N = 16 901 clips, C = 407 classes) against the per-class torch loop
    torchmetrics 0.11 runs for thresholds=None (argsort + cumsum + curve per class), on the same GPU;
  * one AudiosetStrongEvaluator batch (DASM depth 2, 407 queries, batch 4) in dasm and open-vocabulary mode, and its mAP update.

    python tools/ap_bench.py [--reps 20] [--out profiles/as_eval_timing.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def torch_loop_ap(preds, target):
    """torchmetrics 0.11 _multilabel_precision_recall_curve_compute (thresholds=None) + _reduce_average_precision, in torch on the device."""
    res = []
    for c in range(preds.shape[1]):
        p, t = preds[:, c], target[:, c]
        idx = torch.argsort(p, descending=True, stable=True)
        p, t = p[idx], t[idx].float()
        distinct = torch.nonzero(p[1:] - p[:-1], as_tuple=False).squeeze(1)
        thr = torch.cat([distinct, torch.tensor([t.numel() - 1], device=p.device)])
        tps = torch.cumsum(t, 0)[thr]
        fps = 1 + thr - tps
        precision = tps / (tps + fps)
        recall = tps / tps[-1]
        precision = torch.cat([precision.flip(0), torch.ones(1, device=p.device)])
        recall = torch.cat([recall.flip(0), torch.zeros(1, device=p.device)])
        res.append(-torch.sum((recall[1:] - recall[:-1]) * precision[:-1]))
    res = torch.stack(res)
    return res[~torch.isnan(res)].mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from transformer4sed_amd.evaluation import MultilabelAveragePrecision
    lines = [f"device: {torch.cuda.get_device_name(0)}"]
    N, C = 16901, 407
    rng = np.random.RandomState(0)
    preds = torch.from_numpy(rng.rand(N, C).astype(np.float32)).cuda()
    target = torch.from_numpy((rng.rand(N, C) < 0.05).astype(np.int64)).cuda()
    m = MultilabelAveragePrecision(C)
    for s in range(0, N, 64):
        m.update(preds[s:s + 64], target[s:s + 64])
    med, lo = timed(lambda: m.per_class(), args.reps)
    lines.append(f"AP compute (HIP sort + count + reduce) N={N} C={C}: median {med:.3f} ms, min {lo:.3f} ms")
    got = float(m.compute())
    medt, lot = timed(lambda: torch_loop_ap(preds, target), max(3, args.reps // 4), warm=1)
    ref = float(torch_loop_ap(preds, target))
    lines.append(f"per-class torch argsort loop, same data:  median {medt:.3f} ms, min {lot:.3f} ms  (x{medt / med:.1f})")
    lines.append(f"macro mAP: HIP {got:.7f}, torch loop {ref:.7f}")
    b = torch.from_numpy(rng.rand(32, C).astype(np.float32)).cuda()
    tb = torch.from_numpy((rng.rand(32, C) < 0.05).astype(np.int64)).cuda()
    mu = MultilabelAveragePrecision(C)
    mu.update(b, tb)
    med, lo = timed(lambda: (mu.reset(), mu.update(b, tb)), args.reps)
    lines.append(f"update() of one [32, {C}] batch (fresh storage): median {med:.3f} ms")

    from test_gpu_as_eval import build_dasm, _encoder
    from transformer4sed_amd import synth
    from transformer4sed_amd.evaluation import AudiosetStrongEvaluator
    net = build_dasm(2, nb=C)
    enc = _encoder()
    cfg = {"DASM": dict(val_kwargs=dict(encoder_win=False, temp_w=0.5), init_kwargs=dict(at_param=dict(out_type="sigmoid"))),
           "training": dict(median_window=7), "feature": dict(pred_len=1000)}
    td = {l: ("common" if i % 3 else "rare") for i, l in enumerate(enc.labels)}
    B = 4
    wav = torch.from_numpy(synth.synth_wav(B, seed=5100)).cuda()
    labels = torch.from_numpy(synth.synth_strong_labels(B, n_classes=C, seed=950)).cuda()
    pad = torch.zeros(B, 1000, dtype=torch.bool, device="cuda")
    paths = [f"clip_{j}.wav" for j in range(B)]
    for mode in ("dasm", "open_vocabulary"):
        ev = AudiosetStrongEvaluator(net, enc, cfg, mode, type_dict=td)
        med, lo = timed(lambda: (ev.step(wav, labels, pad, paths), ev.flush()), max(5, args.reps // 2))
        lines.append(f"evaluator batch ({mode}, DASM depth 2, {C} queries, B={B}, incl. host tables): median {med:.2f} ms, min {lo:.2f} ms")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
