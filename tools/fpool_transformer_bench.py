"""Frequency-wise transformer pooling (`PaSST_SED(f_pool="frequency_wise_tranformer_encoder")`) beside mean pooling at the bench
shape, depth 12 (developer tool; needs a GPU).

  1. the finetune2 train step (`bench.FINETUNE2`: global student, windowed EMA teacher in train mode) and the pretrain step (frozen
     encoder), ms per step and clips/s, two trainers per stage -- `mean_pool` and the transformer pooling -- taking turns inside every
     round of one process;
  2. the pooling stage alone (`SedEngine._fpool_fwd`, nothing saved, training-mode operands) on a [B, 1190, 768] token stream beside
     two encoder blocks on the same clips (`_encoder_fwd` of a depth-2 model without the final norm): the derivation expects the two to
     cost about the same (2 x 7.08 M GEMM weights per token either way; 1287 against 1190 tokens per clip);
  3. HIP-event times of the new kernels alone at the student's shape (S = B 99 sequences of 13) and at a window group of the teacher
     (S = 10 B 49), with the bytes they move (qkv / dout / dqkv in 16 bits, fp32 streams) over the time.
Warm-up, device events, ROUNDS rounds per variant, medians and the max - min spread over the rounds; the clock and power the device
showed during the run (gpumon) and the commit are printed with the numbers.  python tools/fpool_transformer_bench.py [--b B]"""
import contextlib
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
from transformer4sed_amd.ops import call

B = int(sys.argv[sys.argv.index("--b") + 1]) if "--b" in sys.argv else 12
DEPTH = int(sys.argv[sys.argv.index("--depth") + 1]) if "--depth" in sys.argv else 12
ROUNDS, REPS = 5, 3
FPOOL = "frequency_wise_tranformer_encoder"
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


@contextlib.contextmanager
def pooling(f_pool, mode):
    """bench.build with another `f_pool` (and the synth weights that go with it); bench.py itself stays as it is."""
    kw = bench.MODE_CFG[mode]["PaSST_SED"]["init_kwargs"]
    old_kw, old_sd = kw.get("f_pool", "mean_pool"), synth.matsed_state_dict_np
    kw["f_pool"] = f_pool
    if f_pool == FPOOL:
        extra = {n: v for n, v in synth.fpool_transformer_state_dict_np(tag="w768", dec_layers=0, depth=0).items() if n.startswith("f_pool_module.")}
        synth.matsed_state_dict_np = lambda **k: {**old_sd(**k), **extra}
    try:
        yield
    finally:
        kw["f_pool"], synth.matsed_state_dict_np = old_kw, old_sd


def step_level(mode):
    sn = wn = (B * 4 + 11) // 12
    un = B - sn - wn
    wav = torch.from_numpy(synth.synth_wav(B, seed=1000)).to(dev)
    labels = torch.from_numpy(synth.synth_batch_labels(sn, wn, un, seed=1000)).to(dev)
    variants = {}
    for f_pool in ("mean_pool", FPOOL):
        with pooling(f_pool, mode):
            net, ema_net, opt, trainer, _ = bench.build(B, DEPTH, dev, mode)
        assert net.f_pool_name == f_pool
        trainer.cfg = json.loads(json.dumps(bench.MODE_CFG[mode]))
        if mode == "pretrain":
            variants[f_pool] = lambda t=trainer: t.pretrain_step(wav)
        else:
            trainer.cfg["training"]["batch_size"] = [sn, 0, wn, un]
            variants[f_pool] = lambda t=trainer: t.finetune_step(wav, labels.clone())
    r = alternate(variants)
    print(f"{mode} step, B={B} depth {DEPTH}; {ROUNDS} rounds x {REPS} steps, alternating")
    for k, (m, sp) in r.items():
        print(f"  {k:36s} {m:8.2f} ms/step  {B / m * 1e3:7.1f} clips/s  (spread {100 * sp:4.1f} %)")
    print(f"  measured ratio transformer pooling / mean_pool: {r[FPOOL][0] / r['mean_pool'][0]:.3f}")


def stage_level():
    from transformer4sed_amd.passt_sed import PaSST_SED
    net = PaSST_SED(load_pretrained_model=False, encoder_depth=2, passt_feature_layer=2, f_pool=FPOOL, decoder="transformerXL", decoder_layer_num=2)
    sd = synth.fpool_transformer_state_dict_np(tag="w768", dec_layers=2, depth=12)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items() if k in net.state_dict()}, strict=True)
    net = net.to(dev).train()
    eng = net._make_engine()
    mel = torch.from_numpy(synth.det_uniform("fpoolbench/mel", (B, 128, 1000), -1.2, 1.2)).to(dev)
    x = torch.randn(B, 2 + 12 * 99, 768, device=dev)
    with torch.no_grad():
        W = eng._weights(need_t=False)

        def two_blocks():       # patch embedding + two encoder blocks + the pooling stage they feed
            eng._encoder_fwd(W, mel, [0], 99, [0], False, want_frame=False)

        def stage():
            eng._fpool_fwd(W, x, B, 99, False, dict(F=12))
        r = alternate({"two encoder blocks + pooling stage": two_blocks, "pooling stage": stage}, reps=5)
    a, b = r["two encoder blocks + pooling stage"][0], r["pooling stage"][0]
    print(f"forward, nothing saved, training-mode operands, B={B}: patch embedding + two encoder blocks + pooling stage {a:.3f} ms "
          f"(spread {100 * r['two encoder blocks + pooling stage'][1]:.1f} %), pooling stage alone {b:.3f} ms (spread {100 * r['pooling stage'][1]:.1f} %)")
    print(f"  pooling stage / (two encoder blocks + patch embedding) = {b / (a - b):.3f}; tokens per clip 1287 / 1190 = {1287 / 1190:.3f}")


def kernel_level():
    variants, bytes_of = {}, {}
    for label, S in ((f"student S={B * 99}", B * 99), (f"teacher window group S={10 * B * 49}", 10 * B * 49)):
        N, M = 13, S * 13
        qkv = torch.randn(M, 2304, device=dev).to(torch.float16)
        out = torch.empty(M, 768, dtype=torch.float16, device=dev)
        dout = torch.randn(M, 768, device=dev).to(torch.bfloat16)
        dqkv = torch.empty(M, 2304, dtype=torch.bfloat16, device=dev)
        Bx, tp = S // 49 if "window" in label else B, 49 if "window" in label else 99
        x = torch.randn(Bx, 2 + 12 * tp, 768, device=dev)
        g, bt, tw, tb = [torch.randn(768, device=dev) for _ in range(4)]
        xs, dxs = torch.empty(M, 768, device=dev), torch.randn(M, 768, device=dev)
        mean, rstd = torch.empty(M, device=dev), torch.empty(M, device=dev)
        dx, part = torch.empty_like(x), torch.empty(256 * 3 * 768, device=dev)
        sinks = [torch.zeros(768, device=dev) for _ in range(3)]
        variants[f"sed_attn_short_fwd {label}"] = lambda a=(qkv, out, S, N, 4, 1, 1): call("sed_attn_short_fwd", *a)
        bytes_of[f"sed_attn_short_fwd {label}"] = M * (2304 + 768) * 2
        variants[f"sed_attn_short_bwd {label}"] = lambda a=(qkv, dout, dqkv, S, N, 4, 1): call("sed_attn_short_bwd", *a)
        bytes_of[f"sed_attn_short_bwd {label}"] = M * (2304 + 768 + 2304) * 2
        variants[f"sed_fpool_seq_build_fwd {label}"] = lambda a=(x, g, bt, 1e-5, tw, tb, xs, mean, rstd, Bx, tp, 12): call("sed_fpool_seq_build_fwd", *a)
        bytes_of[f"sed_fpool_seq_build_fwd {label}"] = (x.numel() + xs.numel()) * 4
        variants[f"sed_fpool_seq_build_bwd {label}"] = lambda a=(dxs, x, mean, rstd, g, dx, *sinks, part, part.numel(), Bx, tp, 12): call("sed_fpool_seq_build_bwd", *a)
        bytes_of[f"sed_fpool_seq_build_bwd {label}"] = (dxs.numel() + 2 * x.numel()) * 4
        call("sed_fpool_seq_build_fwd", x, g, bt, 1e-5, tw, tb, xs, mean, rstd, Bx, tp, 12)
    r = alternate(variants, reps=10)
    print(f"new kernels alone, N = 13, 4 heads; {ROUNDS} rounds x 10 launches, alternating")
    for k, (m, sp) in r.items():
        print(f"  {k:62s} {m * 1e3:9.1f} us (spread {100 * sp:4.1f} %)  {bytes_of[k] / 1e6:8.1f} MB  {bytes_of[k] / m / 1e6:7.0f} GB/s")


if __name__ == "__main__":
    try:
        commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=os.path.dirname(os.path.abspath(__file__)),
                                         stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = "unknown"
    print(f"commit {commit} (+ working tree), device {torch.cuda.get_device_name(0)}")
    print("derivation: the module runs 99 x 13 = 1287 tokens per clip through 2 blocks of 7.08 M GEMM weights, 36 GFLOP forward against "
          "202 GFLOP for the 12 encoder blocks on 1190 tokens: +18 % GEMM work per backbone pass")
    mon = GpuSampler(0)
    mon.start()
    step_level("finetune2")
    step_level("pretrain")
    stage_level()
    kernel_level()
    mon.stop()
    print("gpumon:", mon.summary())
