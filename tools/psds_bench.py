#!/usr/bin/env python
"""PSDS timing on the device (IntersectionPSDS / csrc/psds.hip), HIP events and wall clock, everything alternating in one process:
  * `update` of one [32, 1000, 10] batch with both DESED accumulators (psds1: no cross-trigger threshold, psds2: with one);
  * `update` of one [32, 1000, 407] batch without a cross-trigger threshold (the AudioSet-Strong arguments; includes the compaction
    and its count read-back);
  * `compute` after 1168 clips (the DESED validation split) of 10 classes;
  * an `Evaluator` validation step (depth-2 model, batch 32) with the accumulators on and off, alternating: wall time per step of a
    pipelined run of steps behind the epoch's first batch -- whatever the accumulators add that the host or the device can see.

    python tools/psds_bench.py [--reps 10] [--out profiles/psds_timing.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import pandas as pd
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

PSDS1 = dict(dtc_threshold=0.7, gtc_threshold=0.7, cttc_threshold=None, alpha_ct=0, alpha_st=1)
PSDS2 = dict(dtc_threshold=0.1, gtc_threshold=0.1, cttc_threshold=0.3, alpha_ct=0.5, alpha_st=1)


def ground_truth(names, classes, rng, per_clip=5):
    rows = []
    for i, n in enumerate(names):
        for j in range(per_clip):
            on = round(float(rng.uniform(0, 8.5)), 3)
            rows.append((n + ".wav", on, round(min(on + float(rng.uniform(0.3, 4.0)), 10.0), 3), classes[(i * per_clip + j) % len(classes)]))
    return (pd.DataFrame(rows, columns=["filename", "onset", "offset", "event_label"]),
            pd.DataFrame({"filename": [n + ".wav" for n in names], "duration": 10.0}))


def scores_like_posteriors(rng, n, t, c, levels=None):
    """A smoothed random walk per clip and class in [0, 1]; `levels` quantises it (long equal-valued runs, what median-filtered
    posteriors look like), None leaves every value distinct (the most threshold events a clip can have)."""
    x = np.cumsum(rng.randn(n, t, c).astype(np.float32) * 0.05, axis=1)
    x = (x - x.min(1, keepdims=True)) / (x.max(1, keepdims=True) - x.min(1, keepdims=True) + 1e-9)
    return (np.floor(x * (levels - 1e-3)) / levels if levels else x).astype(np.float32)


def device_ms(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    dev, wall = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        wall.append((time.perf_counter() - t0) * 1e3)       # host time until the calls returned
        b.synchronize()
        dev.append(a.elapsed_time(b))
    return float(np.median(dev)), float(np.min(dev)), float(np.median(wall))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from transformer4sed_amd.evaluation import Encoder, Evaluator, IntersectionPSDS
    lines = [f"device: {torch.cuda.get_device_name(0)}"]
    rng = np.random.RandomState(0)
    ts = np.minimum(np.arange(1001) * 0.01, 10.0)

    # ---- update, 10 classes, both accumulators
    B, T = 32, 1000
    classes = [f"class{k}" for k in range(10)]
    names = [f"clip{i}" for i in range(B)]
    gt, dur = ground_truth(names, classes, rng)
    for tag, levels in (("64 score levels", 64), ("all values distinct", None)):
        x = torch.from_numpy(scores_like_posteriors(rng, B, T, 10, levels)).cuda()
        accs = [IntersectionPSDS(gt, dur, classes, ts, **PSDS1), IntersectionPSDS(gt, dur, classes, ts, **PSDS2)]

        def both():
            for acc in accs:
                acc.reset()
                acc.update(x, names)
        med, lo, wall = device_ms(both, args.reps)
        lines.append(f"update B=32 T=1000 C=10, psds1 + psds2 accumulators ({tag}): device median {med:.3f} ms, min {lo:.3f} ms; "
                     f"host time in the two calls {wall:.3f} ms")

    # ---- update, 407 classes, no cross-trigger threshold
    many = [f"class{k}" for k in range(407)]
    gt_m, dur_m = ground_truth(names, many, rng, per_clip=13)
    x = torch.from_numpy(scores_like_posteriors(rng, B, T, 407, 64)).cuda()
    acc = IntersectionPSDS(gt_m, dur_m, many, ts, dtc_threshold=0.7, gtc_threshold=0.7)
    med, lo, wall = device_ms(lambda: (acc.reset(), acc.update(x, names)), args.reps)
    lines.append(f"update B=32 T=1000 C=407, cttc None (64 score levels; sweep + compaction, one count read-back): device median "
                 f"{med:.3f} ms, min {lo:.3f} ms; host time in the call {wall:.3f} ms")

    # ---- compute after the DESED validation split
    N = 1168
    names_v = [f"val{i}" for i in range(N)]
    gt_v, dur_v = ground_truth(names_v, classes, rng)
    xs = torch.from_numpy(scores_like_posteriors(rng, N, T, 10, 64)).cuda()
    for tag, kw in (("psds1", PSDS1), ("psds2", PSDS2)):
        t_all = []
        for _ in range(3):
            acc = IntersectionPSDS(gt_v, dur_v, classes, ts, **kw)
            for s in range(0, N, 32):
                acc.update(xs[s:s + 32], names_v[s:s + 32])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            value, _ = acc.compute()
            t_all.append((time.perf_counter() - t0) * 1e3)
        pts = sum(len(p["tp"]) for p in acc.counts())
        lines.append(f"compute after {N} clips C=10 ({tag}, 64 score levels, {pts} operating points, psds {value:.4f}): wall median "
                     f"{np.median(t_all):.1f} ms, min {np.min(t_all):.1f} ms (first call of a fresh accumulator: compaction, sort, merge, rates)")

    # ---- Evaluator step with and without the accumulators
    from test_gpu_model import _build
    from transformer4sed_amd import synth
    net, _ = _build(False, 2, 2)
    labels_d = ["Alarm_bell_ringing", "Blender", "Cat", "Dishes", "Dog", "Electric_shaver_toothbrush", "Frying", "Running_water", "Speech",
                "Vacuum_cleaner"]
    enc = Encoder(labels_d, audio_len=10, frame_len=1024, frame_hop=320, net_pooling=1, sr=32000)
    cfg = {"training": {"median_window": [5, 20, 5, 5, 5, 20, 20, 20, 5, 20], "filter_type": "median", "weak_mask": True},
           "PaSST_SED": {"val_kwargs": {"encoder_win": True, "win_param": [512, 31], "mix_rate": 0.5, "temp_w": 0.5}}}
    steps = 4
    wav = torch.from_numpy(synth.synth_wav(B, seed=1000)).cuda()
    lab = torch.from_numpy(synth.synth_batch_labels(B, 0, 0, seed=1000)).cuda()
    pad = torch.zeros(B, 1000, dtype=torch.bool)
    paths = [[f"/v/s{s}_{i}.wav" for i in range(B)] for s in range(steps + 1)]
    gt_e, dur_e = ground_truth([f"s{s}_{i}" for s in range(steps + 1) for i in range(B)], labels_d, rng)

    def run(on):
        ev = Evaluator(net, net, enc, cfg, **(dict(ground_truth=gt_e, audio_durations=dur_e) if on else {}))
        ev.step(wav, lab, pad, paths[steps])        # (the first batch of an epoch makes the accumulators and uploads the ground truth)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(steps):
            ev.step(wav, lab, pad, paths[s])
        ev.flush()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    run(True), run(False)
    on, off = [], []
    for _ in range(max(3, args.reps // 2)):
        off.append(run(False))
        on.append(run(True))
    lines.append(f"Evaluator step (depth-2 model, B=32, {steps} pipelined steps + flush), alternating: accumulators off median "
                 f"{np.median(off):.2f} ms (min {np.min(off):.2f}, max {np.max(off):.2f}), on median {np.median(on):.2f} ms "
                 f"(min {np.min(on):.2f}, max {np.max(on):.2f}) per step")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
