#!/usr/bin/env python
"""ROC-area timing (transformer4sed_amd/evaluation/roc.py, csrc/metrics.hip, csrc/segment_pool.hip); developer tool, needs a GPU.

  1. `sed_roc_compute` at the AudioSet-Strong validation size (C = 407, N = 16 901: one chunk) and at C = 10, N = 200 000 (ten chunks),
     through `roc_integers` with the read-back of the [C][8] integers, beside the path it replaces: device-to-host copy of the scores
     and labels plus a `sklearn.metrics.roc_auc_score(max_fpr=0.1)` loop over the classes.
  2. Pooling plus gather for 1 168 clips of [1000, 10] (`SegmentAUROC.update` in batches of 24, then the file scores; 1 168 files of
     10 s, one clip each) beside the numpy definition of tests/roc_cases.py on downloaded scores.
Both sides of a pair run in this one process on the same data; wall clock to a device synchronise, medians of `--reps` runs after a
warm-up run.  The host sides are slow, so they run `--host-reps` times.

    python tools/roc_bench.py [--reps 10] [--host-reps 2] [--out profiles/roc_timing.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import roc_cases as RC  # noqa: E402
from transformer4sed_amd.evaluation import SegmentAUROC, roc  # noqa: E402

DEV = "cuda"


def wall(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def roc_pair(lines, C, N, args):
    from sklearn.metrics import roc_auc_score
    rng = np.random.RandomState(C)
    scores = torch.from_numpy(rng.rand(C, N).astype(np.float32)).to(DEV)
    labels = torch.from_numpy((rng.rand(C, N) < 0.05).astype(np.uint8)).to(DEV)
    ints = [None]

    def device():
        ints[0] = roc.roc_integers(scores, labels, N, 0.1).cpu().numpy()

    def host():
        s, y = scores.cpu().numpy(), labels.cpu().numpy()
        return [roc_auc_score(y[c], s[c], max_fpr=0.1) for c in range(C)]

    d = wall(device, args.reps)
    h = wall(host, args.host_reps, warm=0)
    err = np.abs(roc.roc_scores(ints[0], 0.1, "mcclish")[1] - np.array(host())).max()
    fmt = lambda r: f"median {r[0]:9.3f} ms (min {r[1]:.3f}, max {r[2]:.3f})"
    lines += [f"  C = {C}, N = {N} ({-(-N // roc.AP_CHUNK)} chunk(s)), max_fpr 0.1:",
              f"    sed_roc_compute + read-back of the integers:        {fmt(d)}",
              f"    device-to-host copy + sklearn roc_auc_score loop:   {fmt(h)}: x{h[0] / d[0]:.1f}; largest difference {err:.1e}"]


def pool_pair(lines, args):
    n, T, C, B = 1168, 1000, 10, 24
    ts = np.arange(T + 1) * 0.01
    names = [f"clip{j}" for j in range(n)]
    x = torch.rand(n, T, C, device=DEV)
    acc = SegmentAUROC(roc._empty_ground_truth(), {f: 10.0 for f in names}, [f"c{k}" for k in range(C)], ts)
    got = [None]

    def device():
        acc.reset()
        for lo in range(0, n, B):
            acc.update(x[lo:lo + B], names[lo:lo + B])
        got[0] = acc._file_scores()

    def host():
        xs, ts_us = x.cpu().numpy(), RC.microseconds(ts)
        return np.concatenate([RC.pool_ref(xs[j], ts_us, 10000000, 1000000) for j in range(n)])

    d = wall(device, args.reps)
    h = wall(host, args.host_reps, warm=0)
    same = np.array_equal(got[0].cpu().numpy().T, host())
    fmt = lambda r: f"median {r[0]:9.3f} ms (min {r[1]:.3f}, max {r[2]:.3f})"
    lines += [f"  {n} clips of [{T}, {C}], segments of 1 s, updates of {B} clips:",
              f"    sed_segment_pool per update + sed_segment_gather:    {fmt(d)}",
              f"    device-to-host copy + the numpy definition:          {fmt(h)}: x{h[0] / d[0]:.1f}; bit-equal: {same}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"device {torch.cuda.get_device_name(0)}; tools/roc_bench.py; wall clock to a synchronise, {args.reps} device runs, "
             f"{args.host_reps} host runs"]
    roc_pair(lines, 407, 16901, args)
    roc_pair(lines, 10, 200000, args)
    pool_pair(lines, args)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
