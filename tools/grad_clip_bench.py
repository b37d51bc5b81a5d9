"""Gradient-norm clipping (`training["max_grad_norm"]`, transformer4sed_amd/grad_clip.py) at the bench shape: finetune2, B = 32, depth 12
(developer tool; needs a GPU).

  1. the finetune2 train step (`bench.FINETUNE2`) with the key unset, set so high that the scale is 1 (norms measured, nothing scaled) and
     set so low that every step scales -- three trainers taking turns inside every round of one process;
  2. the three kernels alone on the gradient arena of that model -- `sed_grad_sumsq_chunks`, `sed_grad_norm_finalize`, `sed_scale_by_dev`
     with a scale below 1 (read + write) and with scale 1 (returns at once) -- beside the yardstick, `sed_adamw_ema` over the same arena
     (AdamW + EMA sweep, 36 B per element), taking turns as well; achieved GB/s from the bytes each kernel has to move.
Warm-up, device events, ROUNDS rounds of REPS steps (launches) per variant, medians and the max - min spread over the rounds; the clock and
power the device showed during the run (gpumon) and the commit are printed with the numbers.  python tools/grad_clip_bench.py [--b B]
[--depth D]"""
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from transformer4sed_amd import synth
from transformer4sed_amd.gpumon import GpuSampler
from transformer4sed_amd.grad_clip import _plan_of
from transformer4sed_amd.ops import call
from transformer4sed_amd.trainer import MatSedTrainer

B = int(sys.argv[sys.argv.index("--b") + 1]) if "--b" in sys.argv else 32
DEPTH = int(sys.argv[sys.argv.index("--depth") + 1]) if "--depth" in sys.argv else 12
ROUNDS, REPS = 5, 3
HIGH, LOW = 1e9, 1e-3
dev = "cuda"


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


def step_level():
    sn = wn = (B * 4 + 11) // 12
    un = B - sn - wn
    wav = torch.from_numpy(synth.synth_wav(B, seed=1000)).to(dev)
    labels = torch.from_numpy(synth.synth_batch_labels(sn, wn, un, seed=1000)).to(dev)
    variants, trainers = {}, {}
    for name, m in (("key unset", None), (f"max_grad_norm={HIGH:g} (scale 1)", HIGH), (f"max_grad_norm={LOW:g} (scales)", LOW)):
        net, ema_net, opt, built, _ = bench.build(B, DEPTH, dev, "finetune2")
        cfg = json.loads(json.dumps(bench.FINETUNE2))
        cfg["training"]["batch_size"] = [sn, 0, wn, un]
        if m is not None:
            cfg["training"]["max_grad_norm"] = m
        t = MatSedTrainer(net, ema_net, opt, built.scheduler, cfg, built.epoch_len)
        trainers[name] = t
        variants[name] = lambda t=t: t.finetune_step(wav, labels.clone())
    r = alternate(variants)
    print(f"finetune2 step, B={B} depth {DEPTH}; {ROUNDS} rounds x {REPS} steps, alternating")
    base = r["key unset"][0]
    for k, (m, sp) in r.items():
        print(f"  {k:34s} {m:8.2f} ms/step  {B / m * 1e3:7.1f} clips/s  (spread {100 * sp:4.1f} %)  {m - base:+6.2f} ms vs key unset")
    for name, t in trainers.items():
        if t.max_grad_norm is not None:
            out = t.finetune_step(wav, labels.clone())
            print(f"  {name}: grad_norm of one more step {float(out['grad_norm']):.4f}, clip scale {float(t.net._last_clip_scale):.3e}")
    return trainers["key unset"]


def kernel_level(tr):
    net, opt = tr.net, tr.optimizer
    arena = net._last_grad_arena          # the gradients of the last step (finetune_step clears them at the start of the next one)
    plan = _plan_of(net, arena.device)
    n = arena.numel()
    covered = sum(k for _, _, k in opt.layout)
    out = torch.empty(plan.n_tensors + 2, device=dev)
    below, one = torch.full((1,), 1.0 - 2.0 ** -12, device=dev), torch.ones(1, device=dev)
    kinds = {
        "sed_grad_sumsq_chunks": (lambda: call("sed_grad_sumsq_chunks", arena, plan.tab, plan.n_chunks, plan.partial), 4.0 * covered + 12.0 * plan.n_chunks),
        "sed_grad_norm_finalize": (lambda: call("sed_grad_norm_finalize", plan.partial, plan.first, plan.n_tensors, 20.0, out, out[plan.n_tensors:]),
                                   4.0 * plan.n_chunks + 8.0 * plan.n_tensors),
        "sed_scale_by_dev scale<1": (lambda: call("sed_scale_by_dev", arena, n, below), 8.0 * n),
        "sed_scale_by_dev scale=1": (lambda: call("sed_scale_by_dev", arena, n, one), 0.0),
        # the yardstick: AdamW (lr 0, no decay: the parameters stay) + EMA sweep over the same arena
        "sed_adamw_ema (AdamW + EMA)": (lambda: call("sed_adamw_ema", opt.arena, arena, opt.m, opt.v, opt.ema_arena, n, 0.0, 0.0, 0.9, 0.999, 1e-8, 2, 0.999, 1), 36.0 * n),
    }
    r = alternate({k: f for k, (f, _) in kinds.items()}, reps=10, warm=3)
    print(f"kernels alone on the gradient arena of that model: {n} floats ({4 * n / 2 ** 20:.1f} MiB), {plan.n_tensors} tensors, "
          f"{plan.n_chunks} chunks; {ROUNDS} rounds x 10 launches, alternating")
    for k, (m, sp) in r.items():
        by = kinds[k][1]
        rate = f"{by / m / 1e6:8.1f} GB/s" if by else "       (no traffic)"
        print(f"  {k:30s} {m * 1e3:9.1f} us  {rate}  (spread {100 * sp:4.1f} %)")
    a, y = kinds["sed_grad_sumsq_chunks"][1] / r["sed_grad_sumsq_chunks"][0], kinds["sed_adamw_ema (AdamW + EMA)"][1] / r["sed_adamw_ema (AdamW + EMA)"][0]
    print(f"  sed_grad_sumsq_chunks reaches {a / y:.2f} x the GB/s of sed_adamw_ema in this run")
    clip = r["sed_grad_sumsq_chunks"][0] + r["sed_grad_norm_finalize"][0]
    print(f"  a step that measures: {clip * 1e3:.1f} us of kernels; a step that also scales: {(clip + r['sed_scale_by_dev scale<1'][0]) * 1e3:.1f} us")


if __name__ == "__main__":
    try:
        commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=os.path.dirname(os.path.abspath(__file__)),
                                         stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = "unknown"
    print(f"commit {commit} (+ working tree), device {torch.cuda.get_device_name(0)}")
    mon = GpuSampler(0)
    mon.start()
    tr = step_level()
    kernel_level(tr)
    mon.stop()
    print("gpumon:", mon.summary())
