#!/usr/bin/env python
"""Sound event bounding box timing (transformer4sed_amd/sebb.py, csrc/sebb.hip); developer tool, needs a GPU.

  1. One validation batch [24, 1000, 10] in three forms: a single parameter row, the 27-row bank of the default grid (three distinct
     half lengths), and the 27 single-row launches the bank replaces.  The yardstick is `sed_median_filter_bank` with the nine default
     windows (median) on the same batch.  HIP events, warm-up, ROUNDS rounds of REPS calls, all four taking turns inside every round;
     medians and the max - min spread over the rounds.  Before timing, the bank is compared with its single-row launches.  The calls
     go through `sebb_bank(..., check=False)`: the host's range check reads from the device and is timed on its own line.
  2. One `SebbSearch.update` of the default search (27 rows, psds1 and psds2, soft weak mask) on a batch of 24: wall clock to a
     device synchronise.
The clock and power the device showed during the run (gpumon) are printed with the numbers.

    python tools/sebb_bench.py [--out profiles/sebb_timing.txt]"""
import argparse
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from postproc_search_bench import DEV, LABELS, REPS, ROUNDS, alternate, posteriors, synthetic_validation  # noqa: E402
from transformer4sed_amd import filter as dev_filter  # noqa: E402
from transformer4sed_amd.evaluation import Encoder  # noqa: E402
from transformer4sed_amd.gpumon import GpuSampler  # noqa: E402
from transformer4sed_amd.postproc_search import DEFAULT_WINDOWS, window_frames  # noqa: E402
from transformer4sed_amd.sebb import SebbSearch, check_scores, sebb_bank  # noqa: E402

B, T, C = 24, 1000, 10


def kernel_forms(lines):
    enc = Encoder(LABELS, audio_len=10, frame_len=1024, frame_hop=320, net_pooling=1, sr=32000)
    rows = SebbSearch(enc, *synthetic_validation(C)[:2])._rows
    x = torch.from_numpy(posteriors(B, T, C, seed=1)).to(DEV)
    scale = torch.rand(B, C, device=DEV)
    windows = [[f] * C for f in window_frames(DEFAULT_WINDOWS, T)]
    one = lambda: sebb_bank(x, rows[13:14], scale, capacity=1, check=False)
    bank = lambda: sebb_bank(x, rows, scale, capacity=1, check=False)
    loop = lambda: [sebb_bank(x, [r], scale, capacity=1, check=False) for r in rows]
    same = all(torch.equal(bank().scores[k], o.scores[0]) for k, o in enumerate(loop()))
    r = alternate({"one": one, "bank": bank, "loop": loop, "filters": lambda: dev_filter.filter_bank(x, windows, 1, scale),
                   "check": lambda: check_scores(x, scale)})
    fmt = lambda k: f"{r[k][0] * 1e3:9.1f} us (spread {100 * r[k][1]:4.1f} %)"
    lines += [f"  [{B}, {T}, {C}], HIP events around the calls (allocation of the outputs included):",
              f"    a single parameter row:                              {fmt('one')}",
              f"    the {len(rows)}-row bank, half lengths {sorted({q[0][0] for q in rows})}:                {fmt('bank')}",
              f"    the {len(rows)} single-row launches it replaces:                {fmt('loop')}: x{r['loop'][0] / r['bank'][0]:.2f}; outputs equal: {same}",
              f"    yardstick sed_median_filter_bank, nine windows, median: {fmt('filters')}",
              f"    the host's range check (two reductions and one read): {fmt('check')}"]


def search_update(lines):
    enc = Encoder(LABELS, audio_len=10, frame_len=1024, frame_hop=320, net_pooling=1, sr=32000)
    gt, dur, batches = synthetic_validation(B)
    strong, weak, names = batches[0]
    strong, weak = torch.from_numpy(strong).to(DEV), torch.from_numpy(weak).to(DEV)
    walls = []
    for _ in range(2 + ROUNDS):                    # (two warm-up searches, then timed ones: an update scores a clip once)
        s = SebbSearch(enc, gt, dur, weak_mask=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.update(strong, weak, names)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    walls = walls[2:]
    lines.append(f"  one SebbSearch.update, batch of {B}, {len(s.candidates)} rows x (psds1, psds2) = {2 * len(s.candidates)} accumulators, 1 bank "
                 f"launch: median {statistics.median(walls) * 1e3:.1f} ms wall to a synchronise (min {min(walls) * 1e3:.1f}, max "
                 f"{max(walls) * 1e3:.1f}, {ROUNDS} runs after 2 warm-up runs)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"device {torch.cuda.get_device_name(0)}; tools/sebb_bench.py", f"{ROUNDS} rounds x {REPS} calls, alternating"]
    mon = GpuSampler(0)
    mon.start()
    kernel_forms(lines)
    search_update(lines)
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
