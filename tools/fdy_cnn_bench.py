"""The frequency-dynamic CNN branch (`cnn_param["cnn_name"] = "FDY-CNN"`) beside the base branch at the bench shape (developer tool;
needs a GPU).

  1. the PMAM post-pretrain step (`bench.PMAM`, depth 12) at batch B with the base branch and with the FDY branch -- the 10-layer PMAM
     stack with DY_layers = [0] + [1] * 9 -- two trainers taking turns inside every round of one process; ms per step, clips/s and
     `torch.cuda.max_memory_allocated` of a step of each;
  2. the CNN branch alone (`PmamEngine._cnn_fwd` without saving, and `_cnn_fwd` + `_cnn_bwd`) for both, and the share of the FDY branch's
     time that is spent outside the GEMMs (HIP events around every GEMM launch of one instrumented pass);
  3. HIP-event times of the new kernels alone at the shapes of the stack's layers 1 (500 x 64 bins, 16 -> 16 filters) and 8 (250 x 2 bins,
     128 -> 256), with the bytes they move over the time, beside the project's LayerNorm kernels on a [B 1190, 768] stream in the same run.
Warm-up, device events, ROUNDS rounds per variant, medians and the max - min spread over the rounds; the clock and power the device
showed during the run (gpumon) and the commit are printed with the numbers.  python tools/fdy_cnn_bench.py [--b B] [--depth D]"""
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from transformer4sed_amd import ops, synth
from transformer4sed_amd.gpumon import GpuSampler
from transformer4sed_amd.ops import call

B = int(sys.argv[sys.argv.index("--b") + 1]) if "--b" in sys.argv else 24
DEPTH = int(sys.argv[sys.argv.index("--depth") + 1]) if "--depth" in sys.argv else 12
ROUNDS, REPS = 5, 3
DY = [0] + [1] * 9
dev = "cuda"
GEMMS = ("sed_gemm_nt", "sed_gemm_nt_cols", "sed_gemm_dw_tn")


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


def build(fdy):
    """bench.build_pmam with the branch swapped (bench.py itself stays as it is)."""
    from transformer4sed_amd.passt_cnn import PaSST_CNN
    from transformer4sed_amd.pmam_trainer import PmamTrainer, get_param_lr, mark_only_lora_as_trainable
    from transformer4sed_amd.scheduler import ExponentialDown
    from transformer4sed_amd.trainer import FusedAdamWEMA
    if not fdy:
        return bench.build_pmam(DEPTH, torch.device(dev))
    cfg = json.loads(json.dumps(bench.PMAM))
    kw = cfg["PaSST_CNN"]["init_kwargs"]
    ps = dict(kw["passt_sed_param"], load_pretrained_model=False, encoder_depth=DEPTH)
    ps["passt_feature_layer"] = min(ps["passt_feature_layer"], DEPTH)
    base = kw["cnn_param"]
    cnn = dict(cnn_name="FDY-CNN", n_input_ch=1, activation="cg", conv_dropout=base["conv_dropout"], kernel=[3] * 10, pad=[1] * 10, stride=[1] * 10,
               nb_filters=list(synth.PMAM_FILTERS), pooling=[list(p) for p in synth.PMAM_POOLING], normalization="batch", n_basis_kernels=4,
               DY_layers=DY, temperature=31, pool_dim="freq")
    net = PaSST_CNN(passt_sed_param=ps, cnn_param=cnn)
    sd = synth.fdy_cnn_state_dict_np(tag="pmam0", nb_filters=synth.PMAM_FILTERS, dy_layers=DY, depth=12)
    net.load_state_dict({k: torch.from_numpy(np.asarray(sd[k])) for k in net.state_dict()}, strict=True)
    net = net.to(dev)
    mark_only_lora_as_trainable(net.backbone)
    opt = FusedAdamWEMA(net, get_param_lr(net, cfg["opt"]["param_groups"]), ema_net=None, betas=(0.9, 0.999), eps=1e-8)
    sc = cfg["training"]["scheduler"]
    sched = ExponentialDown(opt, start_iter=sc["n_epochs_cut"] * 1000, total_iter=sc["n_epochs"] * 1000, exponent=sc["exponent"],
                            warmup_iter=sc["lr_warmup_epochs"] * 1000, warmup_rate=sc["lr_warmup_rate"])
    net.train()
    return net, opt, PmamTrainer(net, opt, sched, torch.from_numpy(synth.det_normal("pmam/gmm_means", (30, 768))), cfg)


def step_level(nets):
    wav = torch.from_numpy(synth.synth_wav(B, seed=1000)).to(dev)
    labels = torch.from_numpy(synth.synth_strong_labels(B, n_classes=30, seed=1000)).to(dev)
    variants = {k: (lambda t=t: t.step(wav, labels.clone())) for k, (_, _, t) in nets.items()}
    r = alternate(variants)
    print(f"PMAM post-pretrain step, B={B} depth {DEPTH}; {ROUNDS} rounds x {REPS} steps, alternating")
    for k, (m, sp) in r.items():
        torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
        variants[k]()
        torch.cuda.synchronize()
        print(f"  {k:12s} {m:8.2f} ms/step  {B / m * 1e3:7.1f} clips/s  (spread {100 * sp:4.1f} %)  peak memory of a step "
              f"{torch.cuda.max_memory_allocated() / 2 ** 30:6.2f} GiB")
    print(f"  measured ratio FDY-CNN / base: {r['FDY-CNN'][0] / r['base'][0]:.3f}")


def branch_level(nets):
    mel = torch.from_numpy(synth.det_uniform("fdybench/mel", (B, 128, 1000), -1.2, 1.2)).to(dev)
    variants, runs = {}, {}
    for k, (net, _, _) in nets.items():
        eng = net.engine
        net.train()
        with torch.no_grad():
            W = eng._weights(True)
        views = {n: torch.zeros_like(p) for n, p in net.named_parameters() if n.startswith("cnn.")}
        dfeat = torch.randn(B * 250, 384, device=dev)

        def fwd(eng=eng, W=W):
            with torch.no_grad():
                eng._cnn_fwd(W, mel, train=True, save=False)

        def fwd_bwd(eng=eng, W=W, views=views):
            with torch.no_grad():
                _, cctx = eng._cnn_fwd(W, mel, train=True, save=True)
                slots, scatter = eng._grad_slots(B, mel.device, views.get, False, True, T=mel.shape[2])
                eng._cnn_bwd(W, cctx, dfeat, B, views.get, slots)
                eng._join_dw()
                call("sed_scatter_add_f32", *scatter["cnn"])
        variants[k + " forward"], variants[k + " forward + backward"] = fwd, fwd_bwd
        runs[k] = fwd_bwd
    r = alternate(variants)
    print(f"CNN branch alone (10 layers, training mode, dropout 0.5), B={B}; {ROUNDS} rounds x {REPS} passes, alternating")
    for k, (m, sp) in r.items():
        print(f"  {k:30s} {m:8.2f} ms  (spread {100 * sp:4.1f} %)")
    for k, f in runs.items():      # one instrumented pass: HIP events around every GEMM launch
        ops.TIMER = ops.KernelTimer(GEMMS)
        try:
            t = timed(f, 1)
            g = sum(v["ms"] for v in ops.TIMER.summarize().values())
        finally:
            ops.TIMER = None
        print(f"  {k:12s} instrumented forward + backward {t:8.2f} ms, of which GEMM launches {g:8.2f} ms: {100 * (1 - g / t):4.1f} % outside the GEMMs")


def kernel_level():
    variants, bytes_of = {}, {}
    for label, (H, W, cin, co) in (("layer 1", (500, 64, 16, 16)), ("layer 8", (250, 2, 128, 256))):
        R, M, hid, Cp = B * H, B * H * W, max(cin // 4, 4), max(64, cin)
        ld4, ldg4 = (64, 64) if 4 * co == 64 else (4 * co, 4 * co)
        ldy, ldo = co, (64 if co <= 64 else co)
        X = torch.randn(B, H, W, Cp, device=dev).half()
        pm, u, aff, att = torch.empty(R, cin, device=dev), torch.empty(R, hid, device=dev), torch.empty(3, hid, device=dev), torch.empty(R, 4, device=dev)
        part = torch.empty((R + 15) // 16 * 2 * hid, dtype=torch.float64, device=dev)
        w1, w2, b2 = torch.randn(hid, cin, 3, device=dev), torch.randn(4, hid, device=dev), torch.randn(4, device=dev)
        g, bt, rm, rv = torch.ones(hid, device=dev), torch.zeros(hid, device=dev), torch.zeros(hid, device=dev), torch.ones(hid, device=dev)
        Y4, Y = torch.randn(M, ld4, device=dev), torch.empty(M, ldy, device=dev)
        dY, dY4, da = torch.randn(M, ldo, device=dev).bfloat16(), torch.empty(M, ldg4, dtype=torch.bfloat16, device=dev), torch.empty(R, 4, device=dev)
        P6 = 6 * hid + 4
        ws = torch.empty((P6 + 3) // 4 * 4 + max(1, min(32, R // 128)) * 3 * hid * cin, device=dev)
        bpart = torch.empty((R + 15) // 16 * P6, dtype=torch.float64, device=dev)
        dz, dpm, dX = torch.empty(R, hid, device=dev), torch.empty(R, cin, device=dev), torch.zeros(B, H, W, cin, device=dev)
        gs = [torch.zeros_like(t) for t in (w1, g, bt, w2, b2)]
        call("sed_fdy_freq_mean", X, 1, pm, R, W, cin, Cp)
        call("sed_fdy_attn_taps", pm, w1, u, part, B, H, cin, hid)
        call("sed_fdy_attn_softmax", u, part, g, bt, rm, rv, w2, b2, 31.0, 0.1, 1e-5, aff, att, R, hid)
        add = lambda name, a, nbytes: (variants.__setitem__(f"{name} {label}", lambda: call(name, *a)), bytes_of.__setitem__(f"{name} {label}", nbytes))
        add("sed_fdy_freq_mean", (X, 1, pm, R, W, cin, Cp), X.numel() * 2 + pm.numel() * 4)
        add("sed_fdy_attn_taps", (pm, w1, u, part, B, H, cin, hid), (pm.numel() + u.numel()) * 4)
        add("sed_fdy_attn_softmax", (u, part, g, bt, rm, rv, w2, b2, 31.0, 0.1, 1e-5, aff, att, R, hid), (u.numel() + att.numel()) * 4)
        add("sed_fdy_mix_fwd", (Y4, ld4, att, Y, ldy, M, W, co), (Y4.numel() + Y.numel()) * 4)
        add("sed_fdy_mix_bwd", (dY, ldo, Y4, ld4, att, dY4, ldg4, da, R, W, co), Y4.numel() * 4 + (dY.numel() + dY4.numel()) * 2)
        add("sed_fdy_attn_bwd", (da, att, u, aff, pm, w1, bt, w2, 31.0, 1, dz, bpart, ws, ws.numel(), dpm, *gs, B, H, cin, hid),
            (3 * u.numel() + 2 * pm.numel()) * 4)
        add("sed_fdy_mean_bwd_add", (dX, dpm, R, W, cin), 2 * dX.numel() * 4)
    Mt = B * 1190
    x, gam, bet = torch.randn(Mt, 768, device=dev), torch.ones(768, device=dev), torch.zeros(768, device=dev)
    y16, mean, rstd = torch.empty(Mt, 768, dtype=torch.float16, device=dev), torch.empty(Mt, device=dev), torch.empty(Mt, device=dev)
    dx, dg, db = torch.empty_like(x), torch.zeros(768, device=dev), torch.zeros(768, device=dev)
    call("sed_layernorm_fwd", x, gam, bet, 1e-5, 1.0, y16, None, mean, rstd, Mt, 768, 1)
    for name, a in (("sed_layernorm_fwd", (x, gam, bet, 1e-5, 1.0, y16, None, mean, rstd, Mt, 768, 1)),
                    ("sed_layernorm_bwd", (x, x, mean, rstd, gam, 1.0, dx, 0, dg, db, Mt, 768))):
        variants[name] = lambda name=name, a=a: call(name, *a)
        bytes_of[name] = ops._hbm_bytes_of(name, a)
    r = alternate(variants, reps=10)
    print(f"new kernels alone, B={B}; {ROUNDS} rounds x 10 launches, alternating; bytes = operands once + outputs once")
    for k, (m, sp) in r.items():
        print(f"  {k:34s} {m * 1e3:9.1f} us (spread {100 * sp:4.1f} %)  {bytes_of[k] / 1e6:8.1f} MB  {bytes_of[k] / m / 1e6:7.0f} GB/s")


if __name__ == "__main__":
    try:
        commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=os.path.dirname(os.path.abspath(__file__)),
                                         stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = "unknown"
    print(f"commit {commit} (+ working tree), device {torch.cuda.get_device_name(0)}")
    mon = GpuSampler(0)
    mon.start()
    nets = {"base": build(False), "FDY-CNN": build(True)}
    step_level(nets)
    branch_level(nets)
    kernel_level()
    mon.stop()
    print("gpumon:", mon.summary())
