#!/usr/bin/env python
"""Long-form detection timing (transformer4sed_amd/longform.py, csrc/longform.hip); developer tool, needs a GPU.

  1. A synthetic 10-minute recording through `LongFormDetector` on the depth-12 model with synthetic weights and the recipe's validation
     settings (17 encoder windows, weak mask, median windows 32 / 128 frames, hop 500 frames, batches of 32 chunks): wall time of
     `posteriors` + `decode_events` ending in a device synchronise -> seconds of audio per second; and, from HIP events around their
     launches in a separate run (ops.KernelTimer), the share of the new kernels (gather, stitch, filter, the two event passes) in it.
  2. Each new kernel alone at T = 60 000 and 360 000 timeline frames (10 min / 1 h at a hop of 500) with C = 10 and 407 classes: HIP
     events, warm-up, ROUNDS rounds of REPS launches, all kernels of a shape taking turns inside every round; medians, the max - min
     spread over the rounds, and the bytes each has to move over its time.
The clock and power the device showed during the run (gpumon) are printed with the numbers.

    python tools/longform_bench.py [--minutes 10] [--depth 12] [--out profiles/longform_timing.txt]"""
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

from transformer4sed_amd import longform as LF, ops, synth  # noqa: E402
from transformer4sed_amd.evaluation import Encoder  # noqa: E402
from transformer4sed_amd.gpumon import GpuSampler  # noqa: E402
from transformer4sed_amd.ops import call, h2d  # noqa: E402

ROUNDS, REPS = 5, 5
DEV = "cuda"
LABELS = ["Alarm_bell_ringing", "Blender", "Cat", "Dishes", "Dog", "Electric_shaver_toothbrush", "Frying", "Running_water", "Speech",
          "Vacuum_cleaner"]
CFG = {"training": {"median_window": [5, 20, 5, 5, 5, 20, 20, 20, 5, 20], "filter_type": "median", "weak_mask": True},
       "PaSST_SED": {"val_kwargs": {"encoder_win": True, "win_param": [512, 31], "mix_rate": 0.5, "temp_w": 0.5}}}
NEW = ("sed_longform_gather", "sed_longform_stitch", "sed_longform_filter", "sed_longform_event_count", "sed_longform_event_write")


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


def end_to_end(minutes, depth, lines):
    from test_gpu_model import _build
    net, _ = _build(False, depth, 10 if depth == 12 else depth)
    enc = Encoder(LABELS, audio_len=10, frame_len=1024, frame_hop=320, net_pooling=1, sr=32000)
    clips = -(-int(minutes * 60) // 10)
    wav = torch.from_numpy(np.concatenate([synth.synth_wav(6, seed=2000 + i).reshape(-1) for i in range(-(-clips // 6))])
                           [:int(minutes * 60 * 32000)].copy()).to(DEV)
    seconds = wav.numel() / 32000
    det = LF.LongFormDetector(net, enc, CFG)

    def run():
        out = det.posteriors(wav)
        return out, LF.decode_events(out["post"], 0.5)

    for _ in range(2):
        out, ev = run()
    torch.cuda.synchronize()
    walls = []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        out, ev = run()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    plan = out["plan"]
    med = statistics.median(walls)
    lines.append(f"end to end: {seconds:.0f} s of audio, depth-{depth} PaSST_SED (synthetic weights), validation kwargs (17 encoder windows), "
                 f"hop {plan.hop_frames} frames, {plan.n_chunks} chunks in batches of {det.batch_size}, {plan.n_frames} timeline frames, "
                 f"{ev.shape[0]} events")
    lines.append(f"  posteriors + decode_events, wall clock to a device synchronise, {ROUNDS} runs after 2 warm-up runs: median {med * 1e3:.1f} ms "
                 f"(min {min(walls) * 1e3:.1f}, max {max(walls) * 1e3:.1f}) = {seconds / med:.0f} s of audio per second")
    # a run of its own with HIP events around the new launches (the events cost host time: not the run timed above)
    ops.TIMER = ops.KernelTimer(NEW)
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    summ = ops.TIMER.summarize()
    ops.TIMER = None
    total = sum(d["ms"] for d in summ.values())
    for name in NEW:
        d = summ.get(name, dict(launches=0, ms=0.0))
        lines.append(f"  {name:26s} {d['launches']:3d} launches {d['ms'] * 1e3:9.1f} us")
    lines.append(f"  the new kernels together: {total:.3f} ms of device time = {100 * total / (wall * 1e3):.2f} % of that run's {wall * 1e3:.1f} ms")


def kernels_alone(lines):
    rng = np.random.RandomState(0)
    Tc, Hf, S = 1000, 500, 320
    for T in (60000, 360000):
        for C in (10, 407):
            K = 1 + -(-(T - Tc) // Hf)
            # posteriors that vary slowly along time, like a model's: runs of tens of frames
            base = rng.rand(T // 50 + 2, C).astype(np.float32)
            post_h = np.repeat(base, 50, axis=0)[:T] * 0.9 + rng.rand(T, C).astype(np.float32) * 0.1
            post = torch.from_numpy(post_h).to(DEV)
            strong = torch.rand(K, C, Tc, device=DEV)
            weak = torch.rand(K, C, device=DEV)
            sizes = ([32, 128, 32, 32, 32, 128, 128, 128, 32, 128] * (C // 10 + 1))[:C]
            sz = h2d(sizes, torch.int32, DEV)
            sz7 = h2d([7] * C, torch.int32, DEV)
            th = torch.full((C,), 0.5, device=DEV)
            out = torch.empty(T, C, device=DEV)
            wav = torch.rand(T * S, device=DEV)
            nk = min(32, K)
            chunks = torch.empty(nk, Tc * S, device=DEV)
            seg = LF.EVENT_SEGMENT
            nseg = -(-T // seg)
            cnt, offs, cls = (torch.empty(C * nseg, dtype=torch.int32, device=DEV), torch.empty(C * nseg + 1, dtype=torch.int32, device=DEV),
                              torch.empty(C + 1, dtype=torch.int32, device=DEV))
            call("sed_longform_event_count", post, th, T, C, seg, cnt, offs, cls)
            n_ev = int(cls.cpu()[-1])
            events = torch.empty(max(n_ev, 1), 3, dtype=torch.int32, device=DEV)
            kinds = {
                f"gather ({nk} chunks)": (lambda: call("sed_longform_gather", wav, chunks, T * S, Hf * S, Tc * S, 0, nk), 8.0 * nk * Tc * S),
                "stitch (weak mask)": (lambda: call("sed_longform_stitch", strong, weak, out, K, C, Tc, Hf, T), 4.0 * (K * C * Tc + T * C)),
                "filter median 32/128": (lambda: call("sed_longform_filter", post, out, sz, T, C, 1, 128), 8.0 * T * C),
                "filter max 32/128": (lambda: call("sed_longform_filter", post, out, sz, T, C, 2, 128), 8.0 * T * C),
                "filter median 7": (lambda: call("sed_longform_filter", post, out, sz7, T, C, 1, 7), 8.0 * T * C),
                "event count + scan": (lambda: call("sed_longform_event_count", post, th, T, C, seg, cnt, offs, cls), 4.0 * T * C),
                f"event write ({n_ev} events)": (lambda: call("sed_longform_event_write", post, th, T, C, seg, offs, events), 4.0 * T * C + 12.0 * n_ev),
            }
            r = alternate({k: f for k, (f, _) in kinds.items()})
            lines.append(f"kernels alone, T = {T} frames, C = {C} ({K} chunks behind the stitch); {ROUNDS} rounds x {REPS} launches, alternating")
            for k, (m, sp) in r.items():
                lines.append(f"  {k:34s} {m * 1e3:10.1f} us  {kinds[k][1] / m / 1e6:8.1f} GB/s of the bytes it has to move  (spread {100 * sp:4.1f} %)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"device {torch.cuda.get_device_name(0)}; tools/longform_bench.py --minutes {args.minutes:g} --depth {args.depth}"]
    mon = GpuSampler(0)
    mon.start()
    end_to_end(args.minutes, args.depth, lines)
    kernels_alone(lines)
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
