"""Structured frequency patchout (`PaSST_SED(s_patchout_f=4)`) beside the un-patched model at the bench shape, B = 32, depth 12
(developer tool; needs a GPU).

  1. the finetune2 train step (`bench.FINETUNE2`: global student, windowed EMA teacher in train mode -- both patched out) and the
     pretrain step (frozen, patched-out encoder), ms per step and clips/s, two trainers per stage with `s_patchout_f` 0 and 4 taking
     turns inside every round of one process;
  2. HIP-event times of `sed_mhsa_fwd` / `sed_mhsa_bwd` at the sequence lengths of the global pass (N = 1190 -> 794) and of a window
     (N = 602 -> 402).
The FLOP ratios the shapes predict (per token 14.156 MFLOP of GEMMs per layer, attention 4 N^2 768) are printed beside the measured
ratios.  Warm-up, device events, ROUNDS rounds of REPS steps per variant, medians and the max - min spread over the rounds; the clock
and power the device showed during the run (gpumon) and the commit are printed with the numbers.  python tools/patchout_bench.py [--b B]

`--trace S`: nothing is timed; two warm-up and four further finetune2 steps with `s_patchout_f = S` run and the process ends -- the
form to put behind `rocprofv3 --kernel-trace --stats --` (with SED_OVERLAP_TEACHER=0 SED_DW_STREAM=0: one stream) to see where the
step's time goes with and without patchout."""
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
from transformer4sed_amd.ops import call, pad64

B = int(sys.argv[sys.argv.index("--b") + 1]) if "--b" in sys.argv else 32
DEPTH = int(sys.argv[sys.argv.index("--depth") + 1]) if "--depth" in sys.argv else 12
ROUNDS, REPS = 5, 3
S_F = 4
dev = "cuda"


def timed(f, reps=REPS):
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


def layer_gflop(n):
    return (14.156e6 * n + 4.0 * n * n * 768) / 1e9


def step_level(mode, only=None):
    sn = wn = (B * 4 + 11) // 12
    un = B - sn - wn
    wav = torch.from_numpy(synth.synth_wav(B, seed=1000)).to(dev)
    labels = torch.from_numpy(synth.synth_batch_labels(sn, wn, un, seed=1000)).to(dev)
    variants = {}
    for s in ((0, S_F) if only is None else (only,)):
        net, ema_net, opt, trainer, _ = bench.build(B, DEPTH, dev, mode)
        trainer.cfg = json.loads(json.dumps(bench.MODE_CFG[mode]))
        net.backbone.s_patchout_f = s
        if ema_net is not None:
            ema_net.backbone.s_patchout_f = s
        if mode == "pretrain":
            variants[f"s_patchout_f={s}"] = lambda t=trainer: t.pretrain_step(wav)
        else:
            trainer.cfg["training"]["batch_size"] = [sn, 0, wn, un]
            variants[f"s_patchout_f={s}"] = lambda t=trainer: t.finetune_step(wav, labels.clone())
    if only is not None:
        for _ in range(6):
            variants[f"s_patchout_f={only}"]()
        torch.cuda.synchronize()
        return None
    r = alternate(variants)
    print(f"{mode} step, B={B} depth {DEPTH}; {ROUNDS} rounds x {REPS} steps, alternating")
    for k, (m, sp) in r.items():
        print(f"  {k:18s} {m:8.2f} ms/step  {B / m * 1e3:7.1f} clips/s  (spread {100 * sp:4.1f} %)")
    print(f"  measured ratio s={S_F} / s=0: {r[f's_patchout_f={S_F}'][0] / r['s_patchout_f=0'][0]:.3f}")
    return r


def attention_level():
    Hh = 12
    variants, shapes = {}, {}
    for N in (1190, 794, 602, 402):
        Bx = B if N in (1190, 794) else 2 * B       # (a window group folds several windows into the batch; two of them here)
        Npad = pad64(N)
        q, k, v = [torch.randn(Bx * Hh, N, 64, device=dev).to(torch.float16) for _ in range(3)]
        O = torch.empty(Bx, N, 768, dtype=torch.float16, device=dev)
        lse = torch.empty(Bx * Hh, N, device=dev)
        dO = torch.randn(Bx, N, 768, device=dev).to(torch.bfloat16)
        dqkv = torch.empty(Bx * N, 2304, dtype=torch.bfloat16, device=dev)
        Dt = torch.empty(Bx * Hh, N, device=dev)
        variants[f"sed_mhsa_fwd N={N} B={Bx}"] = lambda a=(q, k, v, O, lse, Bx, Hh, N, Npad, 1): call("sed_mhsa_fwd", *a)
        variants[f"sed_mhsa_bwd N={N} B={Bx}"] = lambda a=(q, k, v, O, dO, lse, Dt, None, dqkv, Bx, Hh, N, Npad, 1, 1): call("sed_mhsa_bwd", *a)
        shapes[N] = Bx
    r = alternate(variants, reps=10)
    print(f"encoder attention kernels, f16, 12 heads; {ROUNDS} rounds x 10 launches, alternating; us")
    for k, (m, sp) in r.items():
        print(f"  {k:30s} {m * 1e3:9.1f} (spread {100 * sp:4.1f} %)")
    for full, cut in ((1190, 794), (602, 402)):
        for kind in ("fwd", "bwd"):
            a, b = r[f"sed_mhsa_{kind} N={cut} B={shapes[cut]}"][0], r[f"sed_mhsa_{kind} N={full} B={shapes[full]}"][0]
            print(f"  {kind} N={cut} / N={full}: measured {a / b:.3f}, 4 N^2 768 predicts {(cut / full) ** 2:.3f}")


if __name__ == "__main__":
    if "--trace" in sys.argv:
        step_level("finetune2", only=int(sys.argv[sys.argv.index("--trace") + 1]))
        sys.exit(0)
    try:
        commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=os.path.dirname(os.path.abspath(__file__)),
                                         stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = "unknown"
    print(f"commit {commit} (+ working tree), device {torch.cuda.get_device_name(0)}")
    print("work per encoder layer and clip, GFLOP (GEMMs 14.156 MFLOP per token + attention 4 N^2 768): "
          + ", ".join(f"N={n}: {layer_gflop(n):.2f}" for n in (1190, 794, 602, 402)))
    print(f"predicted whole-layer ratio s={S_F} / s=0: global pass {layer_gflop(794) / layer_gflop(1190):.3f}, "
          f"window {layer_gflop(402) / layer_gflop(602):.3f}")
    mon = GpuSampler(0)
    mon.start()
    step_level("finetune2")
    step_level("pretrain")
    attention_level()
    mon.stop()
    print("gpumon:", mon.summary())
