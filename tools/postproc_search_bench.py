#!/usr/bin/env python
"""Post-processing search timing (transformer4sed_amd/postproc_search.py, csrc/median_filter.hip); developer tool, needs a GPU.

  1. The filter bank against one `sed_median_filter_k` launch per candidate row (each under its own bound, as `filter._run` calls it: what a
     loop over candidates costs without the bank), on [32, 1000, C] posteriors: the search's nine default windows (6 .. 179 frames) with
     the median and the max, nine windows below 24 frames (the rank-search form), C = 10 and C = 407.  HIP events, warm-up, ROUNDS rounds of
     REPS launches, bank and loop taking turns inside every round; medians and the max - min spread over the rounds.  Before timing, the
     two outputs are compared at the timed size.
  2. One `PostprocSearch.update` of the default search (nine windows + the config row, median and max, psds1 and psds2) on a batch of 32:
     wall clock to a device synchronise.
  3. A whole search over a synthetic validation set of DESED's size (1168 clips of 10 s, 10 classes): 37 updates, `results()` and
     `best()` for both objectives, wall clock.
The clock and power the device showed during the run (gpumon) are printed with the numbers.

    python tools/postproc_search_bench.py [--clips 1168] [--out profiles/postproc_search_timing.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import pandas as pd
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from transformer4sed_amd import filter as dev_filter  # noqa: E402
from transformer4sed_amd.evaluation import Encoder  # noqa: E402
from transformer4sed_amd.gpumon import GpuSampler  # noqa: E402
from transformer4sed_amd.postproc_search import DEFAULT_WINDOWS, PostprocSearch, window_frames  # noqa: E402

ROUNDS, REPS = 5, 5
DEV = "cuda"
LABELS = ["Alarm_bell_ringing", "Blender", "Cat", "Dishes", "Dog", "Electric_shaver_toothbrush", "Frying", "Running_water", "Speech",
          "Vacuum_cleaner"]
CONFIG = [5, 20, 5, 5, 5, 20, 20, 20, 5, 20]
SHORT = [3, 5, 7, 9, 11, 15, 19, 21, 23]


def timed(f, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(variants, reps=REPS, warm=2):
    """{name: fn} -> {name: (median ms, relative spread)}; the variants take turns inside every round."""
    for f in variants.values():
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, f in variants.items():
            ts[k].append(timed(f, reps))
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for k, v in ts.items()}


def posteriors(n, T, C, seed):
    """[n, T, C] fp32 that vary slowly along time, like a model's: runs of tens of frames plus a little noise."""
    rng = np.random.RandomState(seed)
    base = rng.rand(n, T // 50 + 2, C).astype(np.float32)
    return np.repeat(base, 50, axis=1)[:, :T] * 0.9 + rng.rand(n, T, C).astype(np.float32) * 0.1


def bank_vs_loop(lines):
    B, T = 32, 1000
    for C in (10, 407):
        x = torch.from_numpy(posteriors(B, T, C, seed=C)).to(DEV)
        scale = torch.rand(B, C, device=DEV)
        for tag, frames, mode in (("nine default windows (6 .. 179 frames), median", window_frames(DEFAULT_WINDOWS, T), 1),
                                  ("nine default windows (6 .. 179 frames), max", window_frames(DEFAULT_WINDOWS, T), 2),
                                  ("nine windows below 24 frames (3 .. 23), median", SHORT, 1)):
            rows = [[f] * C for f in frames]
            bank = lambda: dev_filter.filter_bank(x, rows, mode, scale)
            loop = lambda: [dev_filter._run(x, r, mode, scale) for r in rows]
            same = all(torch.equal(a, b) for a, b in zip(bank(), loop()))
            r = alternate({"bank": bank, "loop": loop})
            (mb, sb), (ml, sl) = r["bank"], r["loop"]
            lines.append(f"  [{B}, {T}, {C}] {tag}: bank {mb * 1e3:9.1f} us (spread {100 * sb:4.1f} %), {len(rows)} clip-kernel launches "
                         f"{ml * 1e3:9.1f} us (spread {100 * sl:4.1f} %): x{ml / mb:.2f}; outputs equal: {same}")


def synthetic_validation(n_clips, T=1000, seed=0):
    """-> (ground truth, durations, [(strong [n, C, T], weak [n, C], names)] batches of 32 on the host): random events, posteriors high
    inside them with flipped frames and slow drift, on a 1/256 grid."""
    rng = np.random.RandomState(seed)
    C = len(LABELS)
    names = [f"clip{i:04d}" for i in range(n_clips)]
    rows, inside = [], np.zeros((n_clips, T, C), dtype=bool)
    for i in range(n_clips):
        for c in range(C):
            if i >= C and rng.rand() < 0.7:        # (the first clips hold every class: no class without a ground-truth event)
                continue
            for _ in range(rng.randint(1, 3)):
                length = rng.randint(20, 120) if c % 2 == 0 else rng.randint(150, 600)
                on = rng.randint(0, T - length)
                rows.append((names[i] + ".wav", on * 0.01, (on + length) * 0.01, LABELS[c]))
                inside[i, on:on + length, c] = True
    gt = pd.DataFrame(rows, columns=["filename", "onset", "offset", "event_label"])
    dur = pd.DataFrame({"filename": [n + ".wav" for n in names], "duration": [10.0] * n_clips})
    noise = 0.25 * posteriors(n_clips, T, C, seed + 1)
    flip = rng.rand(n_clips, T, C) < 0.1
    scores = np.round(np.where(inside ^ flip, 0.7 + noise, 0.05 + noise) * 256) / 256
    weak = np.where(inside.any(1), 0.9, 0.2).astype(np.float32)
    strong = np.ascontiguousarray(scores.transpose(0, 2, 1), dtype=np.float32)
    batches = [(strong[a:a + 32], weak[a:a + 32], [n + ".wav" for n in names[a:a + 32]]) for a in range(0, n_clips, 32)]
    return gt, dur, batches


def search(lines, n_clips):
    enc = Encoder(LABELS, audio_len=10, frame_len=1024, frame_hop=320, net_pooling=1, sr=32000)
    gt, dur, batches = synthetic_validation(n_clips)
    dev_batches = [(torch.from_numpy(s).to(DEV), torch.from_numpy(w).to(DEV), n) for s, w, n in batches]
    make = lambda: PostprocSearch(enc, gt, dur, config_windows=CONFIG, weak_mask=True)
    walls = []
    for _ in range(2 + ROUNDS):                    # (two warm-up searches of one batch each, then timed ones: an update scores a clip once)
        s = make()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.update(*dev_batches[0])
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    walls = walls[2:]
    lines.append(f"  one update, batch of 32, {len(s.candidates)} candidate rows x (median, max) x (psds1, psds2) = "
                 f"{2 * 2 * len(s.candidates)} accumulators, 2 bank launches: median {statistics.median(walls) * 1e3:.1f} ms wall to a synchronise "
                 f"(min {min(walls) * 1e3:.1f}, max {max(walls) * 1e3:.1f}, {ROUNDS} runs after 2 warm-up runs)")
    del s
    whole = []
    for _ in range(2):
        s = make()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in dev_batches:
            s.update(*b)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        table = s.results()
        best = {name: s.best(name) for name in ("psds1", "psds2")}
        t2 = time.perf_counter()
        whole.append((t1 - t0, t2 - t1))
        del s
    lines.append(f"  whole search, {n_clips} clips in {len(dev_batches)} updates: updates {whole[-1][0]:.2f} s, results() + best() of both objectives "
                 f"{whole[-1][1]:.2f} s (second of two runs; the first: {whole[0][0]:.2f} s + {whole[0][1]:.2f} s); table of {len(table)} rows")
    for name, b in best.items():
        lines.append(f"    {name}: {b.filter_type}, windows {b.windows_units}, composed {b.overall:.4f}, config row {b.config_overall:.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1168)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"device {torch.cuda.get_device_name(0)}; tools/postproc_search_bench.py --clips {args.clips}",
             f"filter bank vs one sed_median_filter_k launch per row; {ROUNDS} rounds x {REPS} launches, alternating"]
    mon = GpuSampler(0)
    mon.start()
    bank_vs_loop(lines)
    lines.append("search, default settings (nine windows + the config row, median and max, psds1 and psds2, soft weak mask)")
    search(lines, args.clips)
    mon.stop()
    lines.append(f"gpumon: {mon.summary()}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
