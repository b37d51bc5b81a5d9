#!/usr/bin/env python
"""Ensemble bank timing (transformer4sed_amd/ensemble.py, csrc/ensemble.hip); developer tool, needs a GPU.

  1. `combine` (one `sed_ensemble_bank` launch per 64 rows) against the plain torch expression per weight row,
     sum_m w_m F.interpolate(x_m, size=T, mode="linear"), at DESED validation's shape: n = 32 clips, T = 1000 frames, C = 10 classes,
     M = 2 (1000 and 500 frames) and M = 3 (1000, 500, 250), W = 11 and W = 64 rows.  Two torch baselines: the expression as written, which
     resamples every member again for every row, and the same with the members resampled once before the rows.  HIP events, warm-up,
     ROUNDS rounds of REPS calls, the variants taking turns inside every round; medians and the max - min spread over the rounds.  Next to
     each time the bytes the algorithm has to move (every member once, the weights, every output element once) per second of the bank.
     Before timing, the outputs are compared at the timed size (torch finds the coordinate in floating point and may fuse: close, not
     equal).
  2. Mode "logit" at the same shapes (no torch baseline: the time only).
  3. The largest |device - float64 definition| of mode "logit" on the fixture tests/test_gpu_ensemble.py asserts on
     (tests/ensemble_cases.py `mode1_fixture`).
The clock and power the device showed during the run (gpumon) are printed with the numbers.

    python tools/ensemble_bench.py [--out profiles/ensemble_timing.txt]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from transformer4sed_amd import ensemble as E  # noqa: E402
from transformer4sed_amd.gpumon import GpuSampler  # noqa: E402

ROUNDS, REPS = 7, 20
DEV = "cuda"


def timed(f, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(variants, reps=REPS, warm=3):
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


def interp(x, T):
    """[n, T_m, C] -> [n, T, C] as the reference resamples: F.interpolate over time."""
    if x.shape[1] == T:
        return x
    return torch.nn.functional.interpolate(x.transpose(1, 2), size=T, mode="linear", align_corners=False).transpose(1, 2)


def torch_rows(xs, w, T, once):
    """w [W, M] (normalised) -> [W, n, T, C], one torch expression per row."""
    if once:
        vs = [interp(x, T) for x in xs]
        return torch.stack([sum(float(w[r, m]) * vs[m] for m in range(len(xs))) for r in range(len(w))])
    return torch.stack([sum(float(w[r, m]) * interp(xs[m], T) for m in range(len(xs))) for r in range(len(w))])


def bank_vs_torch(lines):
    n, T, C = 32, 1000, 10
    rng = np.random.RandomState(0)
    for M in (2, 3):
        Tms = (1000, 500, 250)[:M]
        xs = [torch.from_numpy(rng.rand(n, tm, C).astype(np.float32)).to(DEV) for tm in Tms]
        for W in (11, 64):
            raw = rng.rand(W, M) + 0.05
            w = E.normalise_weights(raw, M, C)[:, :, 0]
            bank = lambda: E.combine(xs, raw)
            rows = lambda: torch_rows(xs, w, T, False)
            once = lambda: torch_rows(xs, w, T, True)
            diff = float((bank() - rows()).abs().max())
            r = alternate({"bank": bank, "rows": rows, "once": once})
            (mb, sb), (mr, sr), (mo, so) = r["bank"], r["rows"], r["once"]
            moved = 4.0 * (n * C * sum(Tms) + W * M * C + W * n * T * C)
            lines.append(f"  M = {M} {Tms}, W = {W:2d}: bank {mb * 1e3:8.1f} us (spread {100 * sb:4.1f} %), {moved / 1e6:6.2f} MB = "
                         f"{moved / (mb * 1e-3) / 1e9:7.1f} GB/s; torch per row {mr * 1e3:8.1f} us (spread {100 * sr:4.1f} %): x{mr / mb:.2f}; "
                         f"torch, members resampled once {mo * 1e3:8.1f} us (spread {100 * so:4.1f} %): x{mo / mb:.2f}; "
                         f"max |bank - torch| {diff:.2e}")
            logit = lambda: E.combine(xs, raw, mode="logit")
            ml, sl = alternate({"logit": logit})["logit"]
            lines.append(f"      mode logit: bank {ml * 1e3:8.1f} us (spread {100 * sl:4.1f} %), {moved / (ml * 1e-3) / 1e9:7.1f} GB/s")


def mode1_error(lines):
    import ensemble_cases as EC
    members, w, raw = EC.mode1_fixture()
    xs = [torch.from_numpy(x).to(DEV) for x in members]
    got = E.combine(xs, raw, mode="logit").cpu().numpy().astype(np.float64)
    err = float(np.abs(got - EC.combine64(members, w, 40, 1)).max())
    lines.append(f"mode logit against the float64 definition on tests/ensemble_cases.py mode1_fixture (3 x 40 x 10, 4 members, 7 rows): "
                 f"max |difference| = {err:.3e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"device {torch.cuda.get_device_name(0)}; tools/ensemble_bench.py",
             f"ensemble bank vs torch expressions per weight row at [32, 1000, 10]; {ROUNDS} rounds x {REPS} calls, alternating; each call "
             "includes the wrapper's host work (weight normalisation, three small uploads)"]
    mon = GpuSampler(0)
    mon.start()
    bank_vs_torch(lines)
    mon.stop()
    mode1_error(lines)
    lines.append(f"gpumon: {mon.summary()}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
