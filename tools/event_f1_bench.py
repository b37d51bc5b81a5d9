#!/usr/bin/env python
"""Event-based / segment-based F1 timing on the device (EventSegmentF1 / csrc/event_f1.hip), HIP events and wall clock, everything
alternating in one process:
  * `update` of one [32, 1000, 10] batch, frame form, and `update_events` of the same batch's decoded event list (list form);
  * the host route it replaces, on the same batch: `_events_frames` (DataFrames from the bin matrix) plus the host reference of the
    tests (`f1_cases.brute` on the lists) -- a stand-in for sed_eval, which walks Python lists the same way;
  * an `Evaluator` validation step (depth-2 model, batch 32), three forms taking turns: without ground truth, with ground truth but the
    F1 feed switched off, and with it on.  `--parent-evaluation FILE` loads the parent commit's evaluation.py (e.g.
    `git show HEAD~1:transformer4sed_amd/evaluation.py > FILE`) and times ITS Evaluator with ground truth in the same alternation.

    python tools/event_f1_bench.py [--reps 10] [--parent-evaluation FILE] [--out profiles/event_f1_timing.txt]
"""
import argparse
import importlib.util
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from psds_bench import device_ms, ground_truth, scores_like_posteriors  # noqa: E402  (tools/ is on sys.path: this script's directory)


def stats(x):
    return f"median {np.median(x):.2f} ms (min {np.min(x):.2f}, max {np.max(x):.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--parent-evaluation", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import f1_cases as FC
    from transformer4sed_amd import evaluation as EV
    lines = [f"device: {torch.cuda.get_device_name(0)}"]
    rng = np.random.RandomState(0)
    ts = np.minimum(np.arange(1001) * 0.01, 10.0)

    # ---- update, frame form and list form, against the host route
    B, T = 32, 1000
    classes = [f"class{k}" for k in range(10)]
    names = [f"clip{i}" for i in range(B)]
    gt, _ = ground_truth(names, classes, rng)
    active_h = scores_like_posteriors(rng, B, T, 10, 64) > 0.5
    active = torch.from_numpy(active_h).cuda()
    enc = EV.Encoder(classes, audio_len=10, frame_len=1024, frame_hop=320, net_pooling=1, sr=32000)
    acc = EV.EventSegmentF1(gt, classes, ts)
    med, lo, wall = device_ms(lambda: (acc.reset(), acc.update(active, names)), args.reps)
    n_sys = int(acc.counts()["n_sys"].sum())
    lines.append(f"update B=32 T=1000 C=10, frame form ({len(gt)} reference events, {n_sys} estimated): device median {med:.3f} ms, min "
                 f"{lo:.3f} ms (reset's two memsets included); host time in the call {wall:.3f} ms")
    pred = EV._events_frames([active_h], names, enc, [0.5])[0.5]
    med, lo, wall = device_ms(lambda: (acc.reset(), acc.update_events(pred, names)), args.reps)
    lines.append(f"update_events of the same batch's event list, list form: device median {med:.3f} ms, min {lo:.3f} ms; host time in "
                 f"the call {wall:.3f} ms (sorting and checking the list in Python)")
    decode, count = [], []
    for _ in range(max(3, args.reps // 2)):
        t0 = time.perf_counter()
        frame = EV._events_frames([active.cpu().numpy()], names, enc, [0.5])[0.5]
        t1 = time.perf_counter()
        refs, ests = FC.lists_of_frames(gt, frame, names, classes)
        host = FC.count_lists(refs, ests, len(classes))
        t2 = time.perf_counter()
        decode.append((t1 - t0) * 1e3)
        count.append((t2 - t1) * 1e3)
    same = {k: [int(v) for v in acc.counts()[k]] for k in FC.NAMES} == host
    lines.append(f"host route on the same batch: bin matrix to the host + _events_frames {stats(decode)}; lists + brute-force counts "
                 f"(tests/f1_cases.py) {stats(count)}; counts equal to the device's: {same}")

    # ---- Evaluator step: no ground truth / ground truth with the F1 feed off / on (/ the parent's evaluation.py)
    from test_gpu_model import _build
    from transformer4sed_amd import synth
    net, _ = _build(False, 2, 2)
    labels_d = ["Alarm_bell_ringing", "Blender", "Cat", "Dishes", "Dog", "Electric_shaver_toothbrush", "Frying", "Running_water", "Speech",
                "Vacuum_cleaner"]
    enc = EV.Encoder(labels_d, audio_len=10, frame_len=1024, frame_hop=320, net_pooling=1, sr=32000)
    cfg = {"training": {"median_window": [5, 20, 5, 5, 5, 20, 20, 20, 5, 20], "filter_type": "median", "weak_mask": True},
           "PaSST_SED": {"val_kwargs": {"encoder_win": True, "win_param": [512, 31], "mix_rate": 0.5, "temp_w": 0.5}}}
    steps = 4
    wav = torch.from_numpy(synth.synth_wav(B, seed=1000)).cuda()
    lab = torch.from_numpy(synth.synth_batch_labels(B, 0, 0, seed=1000)).cuda()
    pad = torch.zeros(B, 1000, dtype=torch.bool)
    paths = [[f"/v/s{s}_{i}.wav" for i in range(B)] for s in range(steps + 1)]
    gt_e, dur_e = ground_truth([f"s{s}_{i}" for s in range(steps + 1) for i in range(B)], labels_d, rng)
    forms = {"no ground truth": (EV, False, False), "ground truth, F1 feed off": (EV, True, False), "ground truth, F1 on": (EV, True, True)}
    if args.parent_evaluation:
        spec = importlib.util.spec_from_file_location("transformer4sed_amd.evaluation_parent", args.parent_evaluation)
        parent = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = parent
        spec.loader.exec_module(parent)
        assert not hasattr(parent, "EventSegmentF1"), "--parent-evaluation must be the evaluation.py of the commit before the F1"
        forms["ground truth, parent commit's evaluation.py"] = (parent, True, None)

    def run(form):
        mod, with_gt, feed = forms[form]
        ev = mod.Evaluator(net, net, enc, cfg, **(dict(ground_truth=gt_e, audio_durations=dur_e) if with_gt else {}))
        if feed is False and with_gt:
            ev._f1_update = lambda who, binm, p: None
        ev.step(wav, lab, pad, paths[steps])        # (the first batch of an epoch makes the accumulators and uploads the ground truth)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(steps):
            ev.step(wav, lab, pad, paths[s])
        ev.flush()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    for form in forms:
        run(form)
    times = {form: [] for form in forms}
    for _ in range(max(3, args.reps // 2)):
        for form in forms:
            times[form].append(run(form))
    lines.append(f"Evaluator step (depth-2 model, B=32, {steps} pipelined steps + flush), {len(forms)} forms taking turns, per step:")
    lines += [f"  {form}: {stats(t)}" for form, t in times.items()]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
