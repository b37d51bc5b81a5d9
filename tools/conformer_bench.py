"""Conformer context network microbenchmark at the model's shape, B = 32, T = 1000 (developer tool; needs a GPU).

  1. the fused convolution-module kernels (sed_conv_glu_dw_fwd / _bwd, csrc/conformer.hip) against the same chain as separate
     torch-ROCm ops (F.glu -> F.conv1d(groups=768) -> F.layer_norm -> silu, and their autograd) on the same device, alternating in one
     process, with the achieved bytes/s against the bytes each form must move;
  2. the whole conformer decoder (two layers), forward + backward through the engine, beside the Transformer-XL decoder (three layers).

Warm-up, device events, ROUNDS rounds of REPS launches per variant, medians and the max - min spread over the rounds; the clock and
power the device showed during the run (gpumon) and the commit are printed with the numbers.  python tools/conformer_bench.py [--b B]"""
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from transformer4sed_amd import synth
from transformer4sed_amd.gpumon import GpuSampler
from transformer4sed_amd.ops import call
from transformer4sed_amd.passt_sed import PaSST_SED

B = int(sys.argv[sys.argv.index("--b") + 1]) if "--b" in sys.argv else 32
T, C, KW = 1000, 768, 31
M = B * T
ROUNDS, REPS = 7, 5
dev = "cuda"


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3


def alternate(variants):
    """{name: fn} -> {name: (median us, relative spread)}; the variants take turns inside every round."""
    for f in variants.values():
        f()
    torch.cuda.synchronize()
    ts = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, f in variants.items():
            ts[k].append(timed(f))
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for k, v in ts.items()}


def kernel_level():
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(M, 2 * C, device=dev, generator=g) * 1.5
    w = (torch.rand(C, KW, device=dev, generator=g) - 0.5) * 0.7
    b, gamma, beta = torch.randn(C, device=dev, generator=g) * 0.1, 1 + 0.1 * torch.randn(C, device=dev, generator=g), torch.randn(C, device=dev, generator=g) * 0.1
    dy = torch.randn(M, C, device=dev, generator=g)
    y16 = torch.empty(M, 3 * C, dtype=torch.float16, device=dev)
    conv, mean, rstd = torch.empty(M, C, device=dev), torch.empty(M, device=dev), torch.empty(M, device=dev)
    dx16 = torch.empty(M, 2 * C, dtype=torch.bfloat16, device=dev)
    dw, db, dg, dbt = torch.zeros(C, KW, device=dev), torch.zeros(C, device=dev), torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    part = torch.empty(min(B * ((T + 19) // 20), 256) * 34 * C, device=dev)

    def chain(xx, ww, bb, gg, bt):
        u = F.glu(xx.view(B, T, 2 * C).transpose(1, 2), dim=1)
        c = F.conv1d(u, ww.view(C, 1, KW), bb, padding=KW // 2, groups=C).transpose(1, 2)
        return F.silu(F.layer_norm(c, (C,), gg, bt, 1e-5))

    leaves = [t.clone().requires_grad_(True) for t in (x, w, b, gamma, beta)]
    dy3 = dy.view(B, T, C)

    def torch_fwd():
        with torch.no_grad():
            return chain(x, w, b, gamma, beta).to(torch.float16)

    def torch_fwd_bwd():
        for t in leaves:
            t.grad = None
        chain(*leaves).backward(dy3)

    def torch_fwd_graph():
        chain(*leaves)

    fwd_eval = lambda: call("sed_conv_glu_dw_fwd", x, w, b, gamma, beta, 1e-5, y16, None, None, None, None, B, T, C, 4)
    fwd_train = lambda: call("sed_conv_glu_dw_fwd", x, w, b, gamma, beta, 1e-5, y16, None, conv, mean, rstd, B, T, C, 4)
    bwd = lambda: call("sed_conv_glu_dw_bwd", dy, x, conv, mean, rstd, w, gamma, beta, dx16, dw, db, dg, dbt, part, part.numel(), B, T, C)
    r = alternate({"fused fwd (eval)": fwd_eval, "fused fwd (train: + conv, mean, rstd)": fwd_train, "torch fwd (no grad, + f16 cast)": torch_fwd,
                   "fused bwd": bwd, "torch fwd with graph": torch_fwd_graph, "torch fwd + bwd (autograd)": torch_fwd_bwd})
    must = {"fused fwd (eval)": M * (2 * C * 4 + 3 * C * 2), "fused fwd (train: + conv, mean, rstd)": M * (2 * C * 4 + 3 * C * 2 + C * 4 + 8),
            "fused bwd": M * (C * 4 + 2 * C * 4 + C * 4 + 8 + 2 * C * 2)}
    print(f"convolution-module middle (GLU -> depthwise 31 -> LayerNorm -> Swish), B={B} T={T} C={C}; {ROUNDS} rounds x {REPS} launches, alternating; us")
    for k, (m, s) in r.items():
        extra = f"   must move {must[k] / 1e6:7.1f} MB -> {must[k] / m / 1e6:5.2f} TB/s" if k in must else ""
        print(f"  {k:42s} {m:9.0f} (spread {100 * s:4.1f} %){extra}")
    tb = r["torch fwd + bwd (autograd)"][0] - r["torch fwd with graph"][0]
    print(f"  torch bwd alone (fwd + bwd minus fwd with graph) {tb:9.0f}")
    print(f"  fused / torch: fwd eval {r['fused fwd (eval)'][0] / r['torch fwd (no grad, + f16 cast)'][0]:.3f}, "
          f"fwd train {r['fused fwd (train: + conv, mean, rstd)'][0] / r['torch fwd with graph'][0]:.3f}, bwd {r['fused bwd'][0] / tb:.3f}")


def decoder_level():
    def model(decoder, layers):
        net = PaSST_SED(passt_feature_layer=2, f_pool="mean_pool", decode_ratio=10, at_adapter=True, decoder=decoder, decoder_layer_num=layers,
                        decoder_pos_emd_len=1000, load_pretrained_model=False, encoder_depth=2)
        sd = (synth.conformer_state_dict_np(dec_layers=layers, depth=2) if decoder == "conformer"
              else synth.matsed_state_dict_np(depth=2, dec_layers=layers))
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        net = net.to(dev).train()
        net.engine = net._make_engine()
        return net

    x = torch.randn(B, T, C, device=dev)
    gout = torch.randn(B, T, C, device=dev)
    variants = {}
    for name, decoder, layers in (("conformer, 2 layers", "conformer", 2), ("transformerXL, 3 layers", "transformerXL", 3)):
        net = model(decoder, layers)
        eng = net.engine
        grads = {n: torch.zeros_like(p) for n, p in net.named_parameters() if n.startswith("decoder.")}
        fwd = eng._conformer_fwd if decoder == "conformer" else eng._decoder_fwd
        bwd = eng._conformer_bwd if decoder == "conformer" else eng._decoder_bwd

        def step(eng=eng, fwd=fwd, bwd=bwd, grads=grads):
            W = eng._weights(need_t=True)
            _, dctx = fwd(W, x, True)
            bwd(W, dctx, gout.clone(), grads.get, True)
            eng._join_dw()

        def fwd_only(eng=eng, fwd=fwd):
            fwd(eng._weights(need_t=False), x, False)
        variants[name + " fwd + bwd"] = step
        variants[name + " fwd (no grad)"] = fwd_only
    r = alternate(variants)
    print(f"context network through the engine, B={B} T={T}; us")
    for k, (m, s) in r.items():
        print(f"  {k:42s} {m:9.0f} (spread {100 * s:4.1f} %)")


if __name__ == "__main__":
    try:
        commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=os.path.dirname(os.path.abspath(__file__)),
                                         stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = "unknown"
    print(f"commit {commit} (+ working tree), device {torch.cuda.get_device_name(0)}")
    mon = GpuSampler(0)
    mon.start()
    kernel_level()
    decoder_level()
    mon.stop()
    print("gpumon:", mon.summary())
