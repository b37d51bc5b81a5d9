"""Conformer context network, `PaSST_SED(decoder="conformer")` (needs an MI355X).

Kernel level: `sed_conv_glu_dw_fwd` / `sed_conv_glu_dw_bwd` (csrc/conformer.hip) against a float64 torch restatement of the middle of
ConvolutionModule.forward (conformer.py:242-270: F.glu, F.conv1d(groups=768, padding=15), F.layer_norm, x sigmoid(x); autograd for the
backward).  The bound of every output is taken from the SAME restatement evaluated in float32 torch on the CPU: the kernel may have
8 x that error (a different summation order over 31 taps / 768 channels / B T frames) plus half a unit in the last place of the
output's storage format at the output's magnitude, taken per element: 2^(floor(log2 |x|) - 8) for bf16, 2^(floor(log2 |x|) - 11) for
f16 (between 2^-9 and 2^-8, 2^-12 and 2^-11 of |x|: what a correctly rounded store of the exact value may err by), nothing for fp32.

Model level: the depth-2 synth-weight model against the reference goldens of tools/gen_conformer_golden.py, with the bounds of
tests/test_gpu_band_attention.py (posteriors within 1e-3: the project's contract)."""
import os
from copy import deepcopy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from transformer4sed_amd import synth  # noqa: E402
from transformer4sed_amd.ops import call, BF16, F16  # noqa: E402
from transformer4sed_amd.passt_sed import PaSST_SED  # noqa: E402

# the pure-torch half of this file (the restatement, its inputs and references, the storage term of the bound) lives in tests/walk_cases.py,
# where tests/test_walk_cases_cpu.py can import it without a GPU
from walk_cases import C, KW, SIG_BITS, chain, half_ulp, inputs, maxerr, reference  # noqa: E402,F401

DEV = "cuda"
LOGDIR = os.environ.get("SED_TEST_LOG_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_logs")
LOG = os.path.join(LOGDIR, "conformer_kernel_errors.log")
MLOG = os.path.join(LOGDIR, "conformer_model_errors.log")
SHAPES = [(1, 8), (3, 31), (2, 65), (3, 100), (2, 1000)]


def check(name, got, ref64, ref32, storage="f32"):
    """Logs and asserts, per element,  |got - ref64| <= 8 max|ref32 - ref64| + half_ulp(storage) at |ref64|."""
    got, ref64 = got.detach().double().cpu(), ref64.detach().double().cpu()
    yard = maxerr(ref32, ref64)
    diff, tol = (got - ref64).abs(), 8 * yard + half_ulp(ref64, storage)
    err, worst = float(diff.max()), float((diff / tol.clamp_min(1e-300)).max())
    os.makedirs(LOGDIR, exist_ok=True)
    with open(LOG, "a") as f:
        f.write(f"{name}: max_abs_err={err:.4e} yardstick_f32_vs_f64={yard:.4e} magnitude={float(ref64.abs().max()):.3e} storage={storage} "
                f"worst_err_over_bound={worst:.3f}\n")
    print(f"{name}: err {err:.3e} yardstick {yard:.3e} worst err / bound {worst:.3f}")
    assert bool((diff <= tol).all()), (name, err, yard, worst)


def run_fwd(t, B, T, mode=4, save=True, y32=True):
    M = B * T
    y16 = torch.empty(M, 3 * C if mode == 4 else C, dtype=BF16 if mode == 0 else F16, device=DEV)
    o32 = torch.empty(M, C, device=DEV) if y32 else None
    conv, mean, rstd = (torch.empty(M, C, device=DEV), torch.empty(M, device=DEV), torch.empty(M, device=DEV)) if save else (None, None, None)
    call("sed_conv_glu_dw_fwd", t["x"], t["w"], t["b"], t["gamma"], t["beta"], 1e-5, y16, o32, conv, mean, rstd, B, T, C, mode)
    return y16, o32, conv, mean, rstd


def run_bwd(t, B, T, conv, mean, rstd):
    M = B * T
    dx = torch.empty(M, 2 * C, dtype=BF16, device=DEV)
    dw, db, dg, dbt = torch.zeros(C, KW, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    part = torch.empty(min(B * ((T + 19) // 20), 256) * 34 * C, device=DEV)
    call("sed_conv_glu_dw_bwd", t["dy"], t["x"], conv, mean, rstd, t["w"], t["gamma"], t["beta"], dx, dw, db, dg, dbt, part, part.numel(), B, T, C)
    return dx, dw, db, dg, dbt


def on_dev(t):
    return {k: v.to(DEV).contiguous() for k, v in t.items()}


# ------------------------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("B,T", SHAPES)
def test_conv_glu_dw_fwd_vs_float64(B, T):
    r64, r32 = reference(B, T)
    t = on_dev(inputs(B, T))
    y16, y32, conv, mean, rstd = run_fwd(t, B, T)
    tag = f"fwd B={B} T={T}"
    # measured at (2, 1000), error / yardstick (the bound is 8 x the yardstick): y 1.87e-6 / 1.87e-6, conv 1.33e-6 / 1.33e-6,
    # mean 2.5e-8 / 1.9e-8, rstd 1.52e-7 / 1.44e-7; worst error / bound over the five shapes 0.17
    check(f"{tag} y (fp32)", y32, r64["y"], r32["y"])
    check(f"{tag} conv (fp32)", conv, r64["c"], r32["c"])
    check(f"{tag} mean", mean, r64["mean"], r32["mean"])
    check(f"{tag} rstd", rstd, r64["rstd"], r32["rstd"])
    # the operand images are roundings of the fp32 result, exactly: [hi | lo | hi] with hi = f16(y), lo = f16(y - hi)
    hi = y32.to(F16)
    assert torch.equal(y16[:, :C], hi) and torch.equal(y16[:, 2 * C:], hi)
    assert torch.equal(y16[:, C:2 * C], (y32 - hi.float()).to(F16))
    check(f"{tag} y (f16 hi third)", y16[:, :C].float(), r64["y"], r32["y"], "f16")      # measured at (2, 1000): 1.95e-3 on values up to 5.8, 0.992 of the bound (the rounding itself)
    for mode, dt, st in ((1, F16, "f16"), (0, BF16, "bf16")):
        p16, _, _, _, _ = run_fwd(t, B, T, mode=mode, save=False, y32=False)        # evaluation form: one output, nothing saved
        assert torch.equal(p16, y32.to(dt))
        check(f"{tag} y ({st})", p16.float(), r64["y"], r32["y"], st)      # measured at (2, 1000): f16 1.95e-3 (0.992 of the bound), bf16 1.56e-2 (0.998)


@pytest.mark.parametrize("B,T", SHAPES)
def test_conv_glu_dw_bwd_vs_float64(B, T):
    r64, r32 = reference(B, T)
    t = on_dev(inputs(B, T))
    _, _, conv, mean, rstd = run_fwd(t, B, T)
    dx, dw, db, dg, dbt = run_bwd(t, B, T, conv, mean, rstd)
    tag = f"bwd B={B} T={T}"
    # measured at (2, 1000), error / yardstick: dx 5.4e-3 on values up to 2.2 (bf16 rounding, 0.999 of the bound; yardstick 5.8e-7),
    # dw 2.47e-5 / 1.77e-5, dbias 2.16e-5 / 6.05e-5, dgamma 2.49e-5 / 1.63e-5, dbeta 1.55e-5 / 1.30e-5 (0.05 .. 0.19 of the bound)
    check(f"{tag} dx (bf16)", dx.float(), r64["dx"], r32["dx"], "bf16")
    check(f"{tag} dw", dw, r64["dw"], r32["dw"])
    check(f"{tag} dbias", db, r64["db"], r32["db"])
    check(f"{tag} dgamma", dg, r64["dgamma"], r32["dgamma"])
    check(f"{tag} dbeta", dbt, r64["dbeta"], r32["dbeta"])
    # determinism: fixed-order two-stage reduction, no atomics -- a second run gives the same bits
    again = run_bwd(t, B, T, conv, mean, rstd)
    for nm, a, b in zip(("dx", "dw", "dbias", "dgamma", "dbeta"), (dx, dw, db, dg, dbt), again):
        assert torch.equal(a, b), (tag, nm)


def test_conv_glu_dw_clip_isolation():
    """B = 3, T = 31: replacing clip 1's input (and its incoming gradient) changes no bit of clips 0 and 2, forward and backward."""
    B, T = 3, 31
    t = on_dev(inputs(B, T))
    y16, y32, conv, mean, rstd = run_fwd(t, B, T)
    dx = run_bwd(t, B, T, conv, mean, rstd)[0]
    t2 = dict(t)
    other = on_dev(inputs(B, T, tag="iso"))
    t2["x"], t2["dy"] = t["x"].clone(), t["dy"].clone()
    t2["x"][T:2 * T] = 3.0 * other["x"][T:2 * T]
    t2["dy"][T:2 * T] = other["dy"][T:2 * T]
    z16, z32, conv2, mean2, rstd2 = run_fwd(t2, B, T)
    dz = run_bwd(t2, B, T, conv2, mean2, rstd2)[0]
    keep = torch.cat([torch.arange(0, T), torch.arange(2 * T, 3 * T)]).to(DEV)
    for a, b in ((y16, z16), (y32, z32), (conv, conv2), (mean, mean2), (rstd, rstd2), (dx, dz)):
        assert torch.equal(a[keep], b[keep])
    assert not torch.equal(y32[T:2 * T], z32[T:2 * T]) and not torch.equal(dx[T:2 * T], dz[T:2 * T])


@pytest.mark.parametrize("B,T", [(3, 31), (2, 65)])
def test_conv_glu_dw_centre_tap_is_identity(B, T):
    """Taps zero except tap 15 = 1, bias 0: the kernel gives Swish(LayerNorm(GLU(x))), the restatement with the convolution removed."""
    t = inputs(B, T)
    t["w"] = torch.zeros(C, KW)
    t["w"][:, KW // 2] = 1.0
    t["b"] = torch.zeros(C)
    ref = {}
    for dt in (torch.float64, torch.float32):
        ref[dt] = chain(t["x"].to(dt), t["w"].to(dt), t["b"].to(dt), t["gamma"].to(dt), t["beta"].to(dt), B, T, conv=False)
    _, y32, conv, _, _ = run_fwd(on_dev(t), B, T)
    check(f"centre tap B={B} T={T} conv = GLU output (fp32)", conv, ref[torch.float64][1], ref[torch.float32][1])
    check(f"centre tap B={B} T={T} y (fp32)", y32, ref[torch.float64][0], ref[torch.float32][0])      # measured: conv 3.9e-7 / 3.5e-7, y 9.5e-7 / 1.06e-6 at (3, 31)


def test_swish_and_scale_kernels():
    """The feed-forwards' elementwise kernels: Swish forward (fp32 and split image), Swish' backward (bf16), out = res + s * in."""
    M = 130
    h = torch.from_numpy(synth.det_normal("conf/swish/h", (M, C), 2.0))
    dy = torch.from_numpy(synth.det_uniform("conf/swish/dy", (M, C)))
    ref = {}
    for dt in (torch.float64, torch.float32):
        hh = h.to(dt).requires_grad_(True)
        y = hh * torch.sigmoid(hh)
        (y * dy.to(dt)).sum().backward()
        ref[dt] = (y.detach(), hh.grad)
    hd, dyd = h.to(DEV), dy.to(DEV)
    y16, y32 = torch.empty(M, 3 * C, dtype=F16, device=DEV), torch.empty(M, C, device=DEV)
    call("sed_swish_fwd", hd, y16, y32, M, C, 4)
    check("swish fwd (fp32)", y32, ref[torch.float64][0], ref[torch.float32][0])
    hi = y32.to(F16)
    assert torch.equal(y16[:, :C], hi) and torch.equal(y16[:, 2 * C:], hi) and torch.equal(y16[:, C:2 * C], (y32 - hi.float()).to(F16))
    dh = torch.empty(M, C, dtype=BF16, device=DEV)
    call("sed_swish_bwd", dyd, hd, dh, M * C)
    check("swish bwd (bf16)", dh.float(), ref[torch.float64][1], ref[torch.float32][1], "bf16")
    out, out16 = torch.empty(M, C, device=DEV), torch.empty(M, C, dtype=BF16, device=DEV)
    call("sed_scale_add_f32", hd, dyd, out, out16, M * C, 0.5)
    assert torch.equal(out, dyd + 0.5 * hd) and torch.equal(out16, out.to(BF16))
    call("sed_scale_add_f32", hd, None, out, None, M * C, float(np.sqrt(768.0)))
    assert torch.equal(out, hd * float(np.float32(np.sqrt(768.0))))


# ------------------------------------------------------------------------------------------------ model level
GOLD_TAGS = [("model_d768_l2_conformer", None), ("model_d768_l2_conformer_win100", 100)]


def mreport(name, err, extra=""):
    os.makedirs(LOGDIR, exist_ok=True)
    with open(MLOG, "a") as f:
        f.write(f"{name}: {err:.4e} {extra}\n")


def build_model(mlm, win, depth=2, feature_layer=2):
    kw = dict(mlm_dict=dict(strategy="block", block_width=10, mask_rate=0.75, out_dim=768)) if mlm else {}
    net = PaSST_SED(passt_feature_layer=feature_layer, f_pool="mean_pool", decode_ratio=10, at_adapter=True, decoder="conformer",
                    decoder_layer_num=2, decoder_pos_emd_len=1000, mlm=mlm, load_pretrained_model=False, encoder_depth=depth,
                    decoder_win_len=win, **kw)
    sd = synth.conformer_state_dict_np(tag="wc768", dec_layers=2, depth=12, mlm=mlm)
    own = net.state_dict()
    load = {k: torch.from_numpy(v) for k, v in sd.items() if k in own}
    if win is not None:
        load["decoder.att_mask"] = own["decoder.att_mask"]
    net.load_state_dict(load, strict=True)
    return net.to(DEV)


def grad_tol(name, base):
    """tests/test_gpu_model.py `_grad_tol`, unchanged."""
    if "pos_bias_u" in name:
        return 0.1
    if "pos_bias_v" in name or "linear_pos" in name:
        return 1e-2
    return base


def _mel(tag, B=2):
    return torch.from_numpy(synth.det_uniform(f"{tag}/mel", (B, 128, 1000), -1.2, 1.2)).to(DEV)


@pytest.mark.parametrize("tag,win", GOLD_TAGS)
def test_conformer_model_vs_reference_golden(golden, tag, win):
    """Finetune-mode outputs, loss and every gradient norm against the reference's (bounds: test_band_model_vs_reference_golden)."""
    g = golden(tag)
    assert float(g["strong_vs_centre_tap_max"]) >= 20 * 1e-3 and (win is None or float(g["strong_vs_full_max"]) >= 20 * 1e-3)
    mel = _mel(tag)
    net = build_model(False, win)
    net.eval()
    with torch.no_grad():
        strong, weak, other = net(mel, encoder_win=False, temp_w=1)
        pm = torch.zeros(2, 1000, dtype=torch.bool)
        pm[0, 900:] = True
        s2, w2, _ = net(mel, encoder_win=False, temp_w=0.5, pad_mask=pm.to(DEV))
    for nm, got, ref in (("strong", strong, g["strong"]), ("weak", weak, g["weak"]), ("at_out", other["at_out"], g["at_out"]),
                         ("strong_t05_pad", s2, g["strong_t05_pad"]), ("weak_t05_pad", w2, g["weak_t05_pad"])):
        e = maxerr(got, torch.from_numpy(ref)); mreport(f"{tag} {nm} vs reference", e); print(f"{tag} {nm}: {e:.3e}")
        assert e < 1e-3, (nm, e)          # measured: strong 3.0e-4 / 3.5e-4 (win100), weak 8.3e-5 / 6.0e-5, at_out 1.3e-4 / 1.0e-4, strong_t05_pad 5.7e-4 / 6.9e-4
    S = lambda t: t[:, ::25, ::16]
    assert maxerr(S(other["frame_before_mask"]), torch.from_numpy(g["interp_s"])) < 2e-2
    net.train()
    strong, weak, other = net(mel, encoder_win=False, temp_w=1)
    gs = torch.from_numpy(synth.det_uniform(f"{tag}/gs", tuple(strong.shape))).to(DEV)
    gw = torch.from_numpy(synth.det_uniform(f"{tag}/gw", tuple(weak.shape))).to(DEV)
    ga = torch.from_numpy(synth.det_uniform(f"{tag}/ga", tuple(other["at_out"].shape))).to(DEV)
    loss = (strong * gs).sum() + (weak * gw).sum() + (other["at_out"] * ga).sum()
    loss.backward()
    rel = abs(float(loss.detach()) - float(g["ft_loss"])) / abs(float(g["ft_loss"])); mreport(f"{tag} loss rel", rel); print(f"{tag} loss rel: {rel:.3e}")
    assert rel < 2e-3          # measured: 7.5e-4, win100 6.1e-4
    names = [str(n) for n in g["ft_grad_names"]]
    params = dict(net.named_parameters())
    got_names = {n for n, p in params.items() if p.grad is not None}
    assert got_names == set(names), (got_names ^ set(names))
    worst, fails = 0.0, []
    for n, norm in zip(names, g["ft_grad_norms"]):
        r = abs(float(params[n].grad.double().norm()) - norm) / (norm + 1e-12)
        mreport(f"{tag} grad {n}", r)
        worst = max(worst, r)
        if not r < grad_tol(n, 3e-3):
            fails.append((n, r))
    mreport(f"{tag} worst grad-norm rel err", worst); print(f"{tag} worst grad-norm rel err: {worst:.3e}")
    assert not fails, fails          # measured worst over all 200+ tensors, the 66 new ones included: 7.8e-4, win100 5.5e-4 (bound 3e-3)


@pytest.mark.parametrize("tag,win", GOLD_TAGS)
def test_conformer_model_mlm_vs_reference_golden(golden, tag, win):
    """MLM-mode prediction, loss and gradient norms (bounds: test_band_model_mlm_vs_reference_golden)."""
    g = golden(tag)
    mel = _mel(tag)
    net = build_model(True, win)
    net.train()
    for p in net.backbone.parameters():
        p.requires_grad_(False)
    net._mlm_draws = dict(noise=torch.from_numpy(g["mlm_noise"]), probs=torch.from_numpy(g["mlm_probs"]), rand_idx=torch.from_numpy(g["mlm_rand_idx"]))
    pred, other = net(mel, encoder_win=False)
    assert np.array_equal(other["mask_id_seq"].cpu().numpy(), g["mlm_mask_ids"])
    S = lambda t: t[:, ::25, ::16]
    e = maxerr(S(pred), torch.from_numpy(g["mlm_pred_s"])); sc = float(np.abs(g["mlm_pred_s"]).max()); mreport(f"{tag} mlm pred", e, f"scale={sc:.2f}")
    print(f"{tag} mlm pred: {e:.3e} scale {sc:.2f}")
    assert e < 1e-3 * sc          # measured: 1.14e-3 on values up to 2.05 (5.6e-4 of scale), win100 1.44e-3 on 1.90 (7.6e-4)
    loss = torch.nn.functional.mse_loss(other["frame_before_mask"][other["mask_id_seq"]], pred[other["mask_id_seq"]])
    rel = abs(float(loss.detach()) - float(g["mlm_loss"])) / float(g["mlm_loss"]); mreport(f"{tag} mlm loss rel", rel); print(f"{tag} mlm loss rel: {rel:.3e}")
    assert rel < 1e-4          # measured: 2.9e-5, win100 8.3e-6
    loss.backward()
    names = [str(n) for n in g["mlm_grad_names"]]
    params = dict(net.named_parameters())
    got_names = {n for n, p in params.items() if p.grad is not None}
    assert got_names == set(names), (got_names ^ set(names))
    worst, fails = 0.0, []
    for n, norm in zip(names, g["mlm_grad_norms"]):
        r = abs(float(params[n].grad.double().norm()) - norm) / (norm + 1e-12)
        mreport(f"{tag} mlm grad {n}", r); worst = max(worst, r)
        if not r < grad_tol(n, 3e-3):
            fails.append((n, r))
    print(f"{tag} mlm worst grad-norm rel err: {worst:.3e}")
    assert not fails, fails          # measured worst: 5.6e-4, win100 5.0e-4


# ------------------------------------------------------------------------------------------------ behaviour
def test_conformer_wide_window_matches_windowless_and_backward_repeats():
    """A window >= 2 T is the windowless model (2e-4, as the band test); two backwards of one model agree (the band test's run-to-run
    bound: the attention and GEMM weight gradients use atomics; the convolution module's own reductions are bit-stable, kernel test)."""
    mel = _mel("conformer/behaviour")
    plain, wide = build_model(False, None), build_model(False, 2000)
    plain.eval(); wide.eval()
    with torch.no_grad():
        s0, w0, _ = plain(mel, encoder_win=False)
        s1, w1, _ = wide(mel, encoder_win=False)
    d = maxerr(s0, s1); mreport("conformer window >= 2T vs windowless: strong", d); assert d < 2e-4
    assert maxerr(w0, w1) < 2e-4
    net = build_model(False, 100)
    net.train()
    w = torch.from_numpy(synth.det_uniform("conformer/w", (2, 10, 1000))).to(DEV)
    names = ["backbone.blocks.0.attn.qkv.weight", "decoder.blocks.1.self_attn.in_proj.weight", "decoder.blocks.0.self_attn.linear_pos.weight",
             "decoder.blocks.0.conv_module.depthwise_conv.weight", "decoder.blocks.1.conv_module.pointwise_conv1.weight",
             "decoder.blocks.0.conv_module.norm.weight", "decoder.blocks.1.feed_forward_macaron.0.weight", "decoder.blocks.0.norm_final.bias",
             "classifier.weight"]
    pn = dict(net.named_parameters())
    runs = []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        s, _, _ = net(mel, encoder_win=False)
        (s * w).sum().backward()
        runs.append([pn[n].grad.detach().clone() for n in names])
    for n, a, b in zip(names, *runs):
        assert float(a.abs().max()) > 0 and maxerr(a, b) <= 2e-3 * float(a.abs().max()) + 1e-7, n
    assert float((s - s0).abs().max()) > 20e-3          # and the window is not ignored


def _fwd_eval(net, mel):
    net.eval()
    with torch.no_grad():
        s, w, o = net(mel, encoder_win=False, temp_w=0.5)
    return torch.cat([s.reshape(-1), w.reshape(-1), o["at_out"].reshape(-1)]).clone()


DW, PW1 = "decoder.blocks.0.conv_module.depthwise_conv.weight", "decoder.blocks.0.conv_module.pointwise_conv1.weight"


@pytest.mark.parametrize("how", ["mul_", "fused_adamw_ema"])
def test_conformer_weight_writes_show_in_next_forward(how):
    """In-place writes to the depthwise and pointwise_conv1 weights between two evaluations (plain `p.data.mul_(1.5)`; one FusedAdamWEMA
    step): the next forward equals a fresh model loaded with the written weights and differs from the first (tests/test_gpu_param_writes.py)."""
    from transformer4sed_amd.trainer import FusedAdamWEMA, get_params
    mel = _mel("conformer/writes")
    net = build_model(False, None)
    opt = None
    if how == "fused_adamw_ema":
        groups = get_params(net, {"encoder": {"lr": 5e-6, "weight_decay": 1e-4, "freeze_layer": 1, "step_lr": 4},
                                  "decoder": {"lr": 1e-3, "weight_decay": 1e-4}, "head": {"lr": 1e-4, "weight_decay": 1e-4}})
        opt = FusedAdamWEMA(net, groups)
    _fwd_eval(net, mel)
    before = _fwd_eval(net, mel)
    pn = dict(net.named_parameters())
    old = {n: pn[n].detach().clone() for n in (DW, PW1)}
    if how == "mul_":
        for n in (DW, PW1):
            pn[n].data.mul_(1.5)
    else:
        g = torch.Generator(device=DEV).manual_seed(3)
        arena = torch.zeros(opt.total, dtype=torch.float32, device=DEV)
        for n in (DW, PW1):
            o, k = opt.offset[n]
            arena[o:o + k].copy_(torch.randn(k, generator=g, device=DEV))
            pn[n].grad = arena[o:o + k].view(pn[n].shape)
        net._last_grad_arena = arena
        opt.step(None)
        opt.zero_grad()
    assert all(not torch.equal(old[n], pn[n].detach()) for n in (DW, PW1))
    after = _fwd_eval(net, mel)
    fresh = build_model(False, None)
    fresh.load_state_dict({k: v.detach().clone() for k, v in net.state_dict().items()}, strict=True)
    want = _fwd_eval(fresh, mel)
    moved, err = maxerr(after, before), maxerr(after, want)
    mreport(f"conformer weight write ({how})", err, f"moved={moved:.3e}")
    assert moved > 1e-4, moved
    assert err < 1e-6, err


def test_conformer_trainer_step_and_checkpoint(tmp_path):
    """One optimisation step of the mean-teacher trainer with a conformer student and EMA teacher at depth 2: every `decoder.blocks.*`
    parameter moves, the teacher's copy is the EMA of the student's; a checkpoint of the model loads back strictly and reproduces
    `strong` bit for bit."""
    import json
    import bench
    from transformer4sed_amd.scheduler import ExponentialDown, ema_alpha
    from transformer4sed_amd.trainer import FusedAdamWEMA, MatSedTrainer, get_params
    net = build_model(False, None)
    ema = deepcopy(net)
    for p in ema.parameters():
        p.detach_()
    cfg = json.loads(json.dumps(bench.FINETUNE2))
    cfg["training"]["batch_size"] = [2, 0, 2, 2]
    groups = get_params(net, {"encoder": {"lr": 5e-6, "weight_decay": 1e-4, "freeze_layer": 1, "step_lr": 4},
                              "decoder": {"lr": 1e-3, "weight_decay": 1e-4}, "head": {"lr": 1e-3, "weight_decay": 1e-4}})
    opt = FusedAdamWEMA(net, groups, ema_net=ema)
    sched = ExponentialDown(opt, start_iter=100, total_iter=200, exponent=-1, warmup_iter=0, warmup_rate=0.1)
    net.train(); ema.train()
    tr = MatSedTrainer(net, ema, opt, sched, cfg, epoch_len=10)
    wav = torch.from_numpy(synth.synth_wav(6, seed=5)).to(DEV)
    labels = torch.from_numpy(synth.synth_batch_labels(2, 2, 2, seed=5)).to(DEV)
    dec = [n for n, _ in net.named_parameters() if n.startswith("decoder.blocks.")]
    assert len(dec) == 66
    tr.finetune_step(wav, labels.clone())        # (the first step's EMA factor is 0: the teacher becomes the student; check the second)
    s0 = {n: p.detach().clone() for n, p in net.named_parameters() if n in dec}
    e0 = {n: p.detach().clone() for n, p in ema.named_parameters() if n in dec}
    out = tr.finetune_step(wav, labels.clone())
    assert np.isfinite(float(out["loss_total"]))
    alpha = ema_alpha(sched.step_num, cfg["training"]["ema_factor"])
    assert 0 < alpha < 1
    sp, ep = dict(net.named_parameters()), dict(ema.named_parameters())
    for n in dec:
        assert not torch.equal(s0[n], sp[n].detach()), f"{n} did not move"
        want = alpha * e0[n] + (1 - alpha) * sp[n].detach()
        assert maxerr(ep[n], want) <= 1e-6 * max(1.0, float(want.abs().max())), n
    # checkpoint round trip
    net.eval()
    mel = _mel("conformer/ckpt")
    with torch.no_grad():
        a, _, _ = net(mel, encoder_win=False)
    path = tmp_path / "conformer.pt"
    torch.save(net.state_dict(), path)
    fresh = build_model(False, None)
    fresh.load_state_dict(torch.load(path, map_location="cpu"), strict=True)
    fresh.eval()
    with torch.no_grad():
        b, _, _ = fresh(mel, encoder_win=False)
    assert torch.equal(a, b)
