"""The frequency-dynamic CNN branch (`cnn_name="FDY-CNN"`, csrc/fdy_cnn.hip) on the GPU.

Kernel level: every new entry point against the restatement of tests/fdy_cases.py (which tests/test_fdy_cnn_cpu.py checks against the
reference module's recorded outputs), per element  |got - ref64| <= 8 max|ref32 - ref64| + half an ulp of the output's storage format
(the rule of tests/test_gpu_conformer.py), logged to test_logs/fdy_cnn_kernel_errors.log.
Branch level: `_cnn_fwd` / `_cnn_bwd` of the 7-layer stack against the float64 restatement.  The branch stores activations and GEMM
operands in 16 bits, so its bound is twice the error of the restatement evaluated on the CPU with those tensors rounded to IEEE half
(forward); the gradients get the rule of tests/test_gpu_pmam.py -- every gradient norm within 3 % -- and, for the attention heads'
parameters, whose gradients pass through the softmax's Jacobian and the BatchNorm1d backward (both differences of nearly equal terms),
the larger of 3 % and twice the relative L2 error of the same gradient in the restatement evaluated on the CPU with the engine's 16-bit
storage emulated (`emulated_grad_errors`: IEEE half for the stored activations and GEMM weights, bfloat16 for the gradients of the
convolution outputs and the gate logits).  |norm deviation| <= |L2 error|, so the emulated L2 error bounds what storage rounding alone
can do to a norm.  Both numbers, and the L2 error of every gradient, go to the log.
Model level: tests/golden/pmam_fdy_d2.npz / pmam_fdy_ft_d2.npz with the bounds tests/test_gpu_pmam.py uses for the base branch."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fdy_cases as FC
from fdy_cases import head_inputs, head_ref  # noqa: F401  (pure torch: shared with tests/walk_cases.py)

pytestmark = pytest.mark.gpu

from transformer4sed_amd import synth  # noqa: E402
from transformer4sed_amd.ops import call, BF16, F16  # noqa: E402
from test_gpu_conformer import half_ulp, maxerr  # noqa: E402

DEV = "cuda"
LOGDIR = os.environ.get("SED_TEST_LOG_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_logs")
LOG = os.path.join(LOGDIR, "fdy_cnn_kernel_errors.log")
MLOG = os.path.join(LOGDIR, "fdy_cnn_model_errors.log")
S = (slice(None), slice(None, None, 25), slice(None, None, 16))
DYN = [i for i, d in enumerate(synth.FDY_DY_LAYERS) if d]

PASST = dict(class_num=30, f_pool="attention", decode_ratio=10, at_adapter=True, decoder="transformerXL", decoder_layer_num=3,
             decoder_pos_emd_len=1000, decoder_dim=384, mlm=True, lora_config=dict(r=8, lora_alpha=1, requires_grad_pretrain=False),
             mlm_dict=dict(strategy="block", block_width=10, mask_rate=0.8, out_dim=768, mask_style=[0.9, 0.05, 0.05]),
             load_pretrained_model=False)


def log(path, line):
    os.makedirs(LOGDIR, exist_ok=True)
    with open(path, "a") as f:
        f.write(line + "\n")
    print(line)


def check(name, got, ref64, ref32, storage="f32"):
    """Logs and asserts, per element,  |got - ref64| <= 8 max|ref32 - ref64| + half_ulp(storage) at |ref64|."""
    got, ref64 = got.detach().double().cpu(), ref64.detach().double().cpu()
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    yard = maxerr(ref32, ref64)
    diff, tol = (got - ref64).abs(), 8 * yard + half_ulp(ref64, storage)
    err, worst = float(diff.max()), float((diff / tol.clamp_min(1e-300)).max())
    log(LOG, f"{name}: max_abs_err={err:.4e} yardstick_f32_vs_f64={yard:.4e} magnitude={float(ref64.abs().max()):.3e} storage={storage} "
             f"worst_err_over_bound={worst:.3f}")
    assert bool((diff <= tol).all()), (name, err, yard, worst)


def close(a, b, atol, rtol=0.0, what=""):
    a = np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    b = np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b)
    log(MLOG, f"{what}: max err {err.max():.3e} (tol {atol:g}+{rtol:g}*|ref|, |ref| max {np.abs(b).max():.3e})")
    assert (err <= atol + rtol * np.abs(b)).all(), f"{what}: max err {err.max():.3e} (tol {atol:g}+{rtol:g}*|ref|)"


# ================================================================================================ kernel level: mixing
def mix_inputs(B, H, W, co):
    M = B * H * W
    tag = f"fdy/mix/{B}x{H}x{W}x{co}"
    y4 = torch.from_numpy(synth.det_normal(tag + "/y4", (M, 4 * co), 1.0))
    att = torch.softmax(torch.from_numpy(synth.det_normal(tag + "/a", (B * H, 4), 1.5)).double(), -1).float()
    dy = torch.from_numpy(FC.exact16(tag + "/dy", (M, co), 0.25))
    return y4, att, dy


def mix_ref(y4, att, dy, B, H, W, co, dt):
    """-> (Y [M, co], dY4 [M, 4 co], da [B H, 4]) in dtype dt through autograd of fdy_cases.mix."""
    y4n = y4.to(dt).view(B, H, W, 4 * co).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    an = att.to(dt).view(B, H, 4).permute(0, 2, 1).contiguous().requires_grad_(True)
    y = FC.mix(y4n, an)
    y.backward(dy.to(dt).view(B, H, W, co).permute(0, 3, 1, 2))
    return (y.detach().permute(0, 2, 3, 1).reshape(-1, co), y4n.grad.permute(0, 2, 3, 1).reshape(-1, 4 * co),
            an.grad.permute(0, 2, 1).reshape(-1, 4))


@pytest.mark.parametrize("B,H,W,co", FC.MIX_CASES)
def test_mix_forward_and_backward(B, H, W, co):
    y4, att, dy = mix_inputs(B, H, W, co)
    M, R = B * H * W, B * H
    r64, r32 = mix_ref(y4, att, dy, B, H, W, co, torch.float64), mix_ref(y4, att, dy, B, H, W, co, torch.float32)
    # layouts of the engine: Y4 with its row pitch, Y with the BatchNorm path's, dY / dY4 bf16 with the gradient operands'
    Nc = (4 * co + 127) // 128 * 128
    ld4 = 64 if 4 * co == 64 else Nc
    ldy = co if co < 128 else (co + 127) // 128 * 128
    ldo = 64 if co <= 64 else (co + 127) // 128 * 128
    ldg4 = 64 if 4 * co <= 64 else Nc
    Y4 = torch.full((M, ld4), float("nan"), device=DEV); Y4[:, :4 * co] = y4.to(DEV)
    A = att.to(DEV).contiguous()
    Y = torch.full((M, ldy), float("nan"), device=DEV)
    call("sed_fdy_mix_fwd", Y4, ld4, A, Y, ldy, M, W, co)
    name = f"mix B{B} H{H} W{W} co{co}"
    check(name + " fwd Y", Y[:, :co], r64[0], r32[0])
    assert ldy == co or float(Y[:, co:].abs().max()) == 0.0
    dY = torch.full((M, ldo), float("nan"), dtype=BF16, device=DEV); dY[:, :co] = dy.to(DEV).to(BF16)
    assert torch.equal(dY[:, :co].float().cpu(), dy), "the upstream gradient is exact in bf16"
    dY4 = torch.full((M, ldg4), float("nan"), dtype=BF16, device=DEV)
    da = torch.full((R, 4), float("nan"), device=DEV)
    call("sed_fdy_mix_bwd", dY, ldo, Y4, ld4, A, dY4, ldg4, da, R, W, co)
    check(name + " bwd dY4", dY4[:, :4 * co].float(), r64[1], r32[1], "bf16")
    check(name + " bwd da", da, r64[2], r32[2])
    assert ldg4 == 4 * co or float(dY4[:, 4 * co:].float().abs().max()) == 0.0
    da2 = torch.empty_like(da)
    call("sed_fdy_mix_bwd", dY, ldo, Y4, ld4, A, dY4, ldg4, da2, R, W, co)
    assert torch.equal(da, da2), "ordered reduction: the same bits in every run"


# ================================================================================================ kernel level: frequency mean + attention head
@pytest.mark.parametrize("temperature", FC.TEMPERATURES)
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("B,H,W,cin", FC.HEAD_CASES)
def test_frequency_mean_and_attention_head(B, H, W, cin, train, temperature):
    inp = head_inputs(B, H, W, cin, temperature)
    r64, r32 = head_ref(inp, temperature, train, torch.float64), head_ref(inp, temperature, train, torch.float32)
    hid, R, Cp = FC.hid_of(cin), B * H, max(64, cin)
    name = f"head B{B} H{H} W{W} cin{cin} {'train' if train else 'eval'} T{temperature:g}"
    d = {k: v.to(DEV).contiguous() for k, v in inp.items()}
    for dt16 in (F16, BF16):
        X = torch.full((B, H, W, Cp), float("nan"), dtype=dt16, device=DEV); X[..., :cin] = d["x"].to(dt16)
        assert torch.equal(X[..., :cin].float(), d["x"]), "the activation is exact in its 16-bit format"
        pm = torch.full((R, cin), float("nan"), device=DEV)
        call("sed_fdy_freq_mean", X, 1 if dt16 == F16 else 0, pm, R, W, cin, Cp)
        check(name + f" pm ({'f16' if dt16 == F16 else 'bf16'} input)", pm, r64["pm"], r32["pm"])
    u, aff, att = torch.empty(R, hid, device=DEV), torch.empty(3, hid, device=DEV), torch.full((R, 4), float("nan"), device=DEV)
    part = torch.empty((R + 15) // 16 * 2 * hid, dtype=torch.float64, device=DEV) if train else None
    rm, rv = d["bn_rm"].clone(), d["bn_rv"].clone()
    call("sed_fdy_attn_taps", pm, d["c1w"], u, part, B, H, cin, hid)
    call("sed_fdy_attn_softmax", u, part, d["bn_w"], d["bn_b"], rm, rv, d["c2w"], d["c2b"], float(temperature), 0.1, 1e-5, aff, att, R, hid)
    check(name + " att", att, r64["att"], r32["att"])
    assert float(att.min()) < 0.2 and float(att.max()) > 0.3, "the case exercises the softmax"
    if train:      # torch's rule: momentum 0.1, unbiased variance (bound of tests/test_gpu_pmam_kernels.py:338)
        want_m = 0.9 * inp["bn_rm"].double() + 0.1 * r64["mean"]
        want_v = 0.9 * inp["bn_rv"].double() + 0.1 * r64["var"] * R / (R - 1)
        log(LOG, f"{name} running statistics: mean err {maxerr(rm, want_m):.3e} var err {maxerr(rv, want_v):.3e}")
        assert maxerr(rm, want_m) < 1e-6 and maxerr(rv, want_v) < 1e-5
    else:
        assert torch.equal(rm, d["bn_rm"]) and torch.equal(rv, d["bn_rv"])
    # backward
    P6 = 6 * hid + 4
    ws = torch.empty((P6 + 3) // 4 * 4 + max(1, min(32, R // 128)) * 3 * hid * cin, device=DEV)
    bpart = torch.empty((R + 15) // 16 * P6, dtype=torch.float64, device=DEV)
    dz, dpm = torch.empty(R, hid, device=DEV), torch.full((R, cin), float("nan"), device=DEV)
    g = {k: torch.zeros_like(d[k]) for k in ("c1w", "bn_w", "bn_b", "c2w", "c2b")}
    call("sed_fdy_attn_bwd", d["da"], att, u, aff, pm, d["c1w"], d["bn_b"], d["c2w"], float(temperature), 1 if train else 0, dz, bpart, ws, ws.numel(),
         dpm, g["c1w"], g["bn_w"], g["bn_b"], g["c2w"], g["c2b"], B, H, cin, hid)
    dX = d["dx0"].clone()
    call("sed_fdy_mean_bwd_add", dX, dpm, R, W, cin)
    check(name + " dX", dX, r64["dX"], r32["dX"])
    for k in g:
        check(name + " grad " + k, g[k], r64["g_" + k], r32["g_" + k])
    # a second backward accumulates on top of what the gradient views hold, in the same order: exactly twice
    call("sed_fdy_attn_bwd", d["da"], att, u, aff, pm, d["c1w"], d["bn_b"], d["c2w"], float(temperature), 1 if train else 0, dz, bpart, ws, ws.numel(),
         dpm, g["c1w"], g["bn_w"], g["bn_b"], g["c2w"], g["c2b"], B, H, cin, hid)
    for k in g:
        check(name + " grad " + k + " accumulated", g[k], 2 * r64["g_" + k], 2 * r32["g_" + k])
    # frozen parameters: null gradient views
    dpm2 = torch.empty_like(dpm)
    call("sed_fdy_attn_bwd", d["da"], att, u, aff, pm, d["c1w"], d["bn_b"], d["c2w"], float(temperature), 1 if train else 0, dz, bpart, ws, ws.numel(),
         dpm2, None, None, None, None, None, B, H, cin, hid)
    assert torch.equal(dpm, dpm2)


# ================================================================================================ branch level
def build(depth=2, fl=2, dropout=0.5, ft=False, cnn=None, state=None):
    from transformer4sed_amd.passt_cnn import PaSST_CNN
    ps = dict(PASST, passt_feature_layer=fl, encoder_depth=depth)
    if ft:
        ps = {k: v for k, v in ps.items() if k not in ("lora_config", "mlm_dict")}
        ps.update(mlm=False, class_num=10)
    net = PaSST_CNN(passt_sed_param=ps, cnn_param=dict(cnn or FC.FDY_CNN_PARAM, conv_dropout=dropout))
    sd = state or (synth.fdy_cnn_state_dict_np(depth=12, mlm=False, lora_r=0, class_num=10) if ft else synth.fdy_cnn_state_dict_np(depth=12))
    own = net.state_dict()
    net.load_state_dict({k: torch.from_numpy(np.asarray(sd[k])) for k in own}, strict=True)
    return net.cuda()


@pytest.fixture(scope="module")
def net7():
    return build()


def run_branch(net, mel, train, masks=None, dfeat=None):
    """`_cnn_fwd` (and, with dfeat, `_cnn_bwd` + the scatter of the gradient images) -> (features [B T', C], {name: gradient})."""
    if net.engine is None:
        net.engine = net._make_engine()
    eng = net.engine
    net.train(train)
    W = eng._weights(dfeat is not None)
    B, _, T = mel.shape
    dm = None if masks is None else [torch.from_numpy(m.reshape(-1, m.shape[-1]).astype(np.uint8)).cuda() for m in masks]
    feat, cctx = eng._cnn_fwd(W, mel, train=train, save=dfeat is not None, drop_masks=dm)
    if dfeat is None:
        return feat, None
    views = {n: torch.zeros_like(p) for n, p in net.named_parameters() if n.startswith("cnn.")}
    slots, scatter = eng._grad_slots(B, mel.device, views.get, False, True, T=T)
    eng._cnn_bwd(W, cctx, dfeat, B, views.get, slots)
    eng._join_dw()
    call("sed_scatter_add_f32", *scatter["cnn"])
    return feat, views


def branch_ref(sd_np, mel, pooling, dy, train, masks, dfeat, dt, q=None, qb=None, drop_p=0.5):
    sd = FC.cnn_tensors(sd_np, dt)
    if dfeat is not None:
        sd = {k: (v.requires_grad_(True) if "running" not in k else v) for k, v in sd.items()}
    mk = None if masks is None else [torch.from_numpy(m.transpose(0, 3, 1, 2).copy()) for m in masks]
    feat, rec = FC.branch(sd, mel.to(dt), pooling, dy, 31.0, train, drop_masks=mk, drop_p=drop_p, q=q, qb=qb)
    f2 = feat.squeeze(-1).transpose(1, 2).reshape(-1, feat.shape[1])
    grads = None
    if dfeat is not None:
        (f2 * dfeat.to(dt)).sum().backward()
        grads = {"cnn.cnn." + k: v.grad for k, v in sd.items() if v.requires_grad}
    return f2.detach(), rec, grads


def half(t):
    return t.half().to(t.dtype)


def bf16r(t):
    return t.bfloat16().to(t.dtype)


def emulated_grad_errors(sd_np, mel, masks, dfeat, drop_p=0.5):
    """{parameter: relative L2 error of its gradient} of the 7-layer stack's training-mode restatement with the engine's 16-bit storage
    emulated on the CPU (forward: IEEE half; backward: bfloat16) against the float64 restatement, for the upstream gradient dfeat."""
    args = (sd_np, mel, synth.FDY_POOLING, synth.FDY_DY_LAYERS, True, masks)
    _, _, g64 = branch_ref(*args, dfeat, torch.float64, drop_p=drop_p)
    _, _, ge = branch_ref(*args, dfeat, torch.float32, q=half, qb=bf16r, drop_p=drop_p)
    return {k: float((ge[k].double() - g64[k]).norm() / g64[k].norm().clamp_min(1e-30)) for k in g64}, g64


def record_dfeat(net):
    """After a forward: have the engine's CNN backward keep the upstream gradient it receives (the gradient of the CNN features, fp32
    [B T', C], produced by the projector / context-network backward that the base branch shares) -> dict that will hold it as "dfeat"."""
    rec, orig = {}, net.engine._cnn_bwd

    def spy(W, cctx, dfeat, *a, **k):
        rec["dfeat"] = dfeat.detach().clone()
        return orig(W, cctx, dfeat, *a, **k)
    net.engine._cnn_bwd = spy
    return rec


def grad_bound(name, emu):
    """3 % on a gradient norm; an attention-head parameter: the larger of 3 % and twice its emulated relative L2 error."""
    return max(0.03, 2 * emu[name]) if ".attention." in name else 0.03


@pytest.mark.parametrize("T", [8, 1000])
@pytest.mark.parametrize("train", [False, True])
def test_branch_forward_and_backward_vs_restatement(net7, T, train):
    B = 2
    sd_np = synth.fdy_cnn_state_dict_np(depth=12)
    net7.load_state_dict({k: torch.from_numpy(np.asarray(sd_np[k])) for k in net7.state_dict()}, strict=True)       # (running statistics back to the synthetic ones)
    mel = torch.from_numpy(synth.det_uniform(f"fdy/branch/mel{T}", (B, 128, T), -1.2, 1.2))
    masks = FC.drop_masks_np(f"fdy/branch{T}", B, synth.FDY_FILTERS, synth.FDY_POOLING, 0.5, T=T) if train else None
    Tc = T // 4
    dfeat = torch.from_numpy(synth.det_normal(f"fdy/branch/dfeat{T}", (B * Tc, 128), 1.0))
    args = (sd_np, mel, synth.FDY_POOLING, synth.FDY_DY_LAYERS, train, masks)
    r64, rec, _ = branch_ref(*args, None, torch.float64)
    emu, _, _ = branch_ref(*args, None, torch.float32, q=half)
    feat, grads = run_branch(net7, mel.cuda(), train, masks, dfeat.cuda() if train else None)
    assert tuple(feat.shape) == (B * Tc, 128)
    name = f"branch T{T} {'train' if train else 'eval'}"
    e_emu, e_got = maxerr(emu, r64), maxerr(feat, r64)
    log(LOG, f"{name}: features max err {e_got:.3e}, restatement with 16-bit storage emulated on the CPU {e_emu:.3e} (bound: twice that), "
             f"|feat| max {float(r64.abs().max()):.3e}")
    assert e_got <= 2 * e_emu
    if train:      # running statistics of both kinds of BatchNorm (bound of tests/test_gpu_pmam.py for the model: 3e-3 + 1e-2 |ref|)
        own = net7.state_dict()
        for i, r in enumerate(rec):
            n = r["count2"]
            close(own[f"cnn.cnn.batchnorm{i}.running_mean"], 0.01 * sd_np[f"cnn.cnn.batchnorm{i}.running_mean"] + 0.99 * r["mean2"].detach().numpy(), 3e-3, 1e-2,
                  what=f"{name} BatchNorm2d {i} running_mean")
            close(own[f"cnn.cnn.batchnorm{i}.running_var"], 0.01 * sd_np[f"cnn.cnn.batchnorm{i}.running_var"] + 0.99 * r["var2"].detach().numpy() * n / (n - 1), 3e-3, 1e-2,
                  what=f"{name} BatchNorm2d {i} running_var")
            if "att" in r:
                pre, n1 = f"cnn.cnn.conv{i}.attention.bn.", r["rows"]
                close(own[pre + "running_mean"], 0.9 * sd_np[pre + "running_mean"] + 0.1 * r["mean"].detach().numpy(), 3e-3, 1e-2, what=f"{name} BatchNorm1d {i} running_mean")
                close(own[pre + "running_var"], 0.9 * sd_np[pre + "running_var"] + 0.1 * r["var"].detach().numpy() * n1 / (n1 - 1), 3e-3, 1e-2,
                      what=f"{name} BatchNorm1d {i} running_var")
                assert int(own[pre + "num_batches_tracked"]) == 4
    else:
        return     # (the backward of this branch runs on batch statistics only, as the base branch's)
    emu_g, g64 = emulated_grad_errors(sd_np, mel, masks, dfeat)
    bad = []
    for n_, ref in g64.items():
        got = grads[n_].double().cpu()
        if re.fullmatch(r"cnn\.cnn\.conv\d\.bias", n_):
            # BatchNorm removes the batch mean, so the true gradient of a conv bias is zero: both sides hold rounding noise only
            assert float(got.norm()) < 2e-2 * float(grads[n_.replace(".bias", ".weight")].double().norm()), n_
            continue
        rel, l2 = abs(float(got.norm() / ref.norm().clamp_min(1e-30)) - 1.0), float((got - ref).norm() / ref.norm().clamp_min(1e-30))
        bound = grad_bound(n_, emu_g)
        log(LOG, f"{name}: gradient {n_} norm off by {rel:.4f} (bound {bound:.4f}), relative L2 error {l2:.4f}, emulated on the CPU {emu_g[n_]:.4f}")
        if rel >= bound:
            bad.append((n_, rel, bound))
    assert not bad, bad


def test_pmam10_stack_eval_vs_fixture(golden):
    """The 10-layer PMAM stack with nine dynamic layers (widths up to 384, 256 -> 384 channels with one mel bin left) in evaluation mode against
    the reference module's recorded features."""
    g = golden("pmam_fdy_d2")
    sd = synth.fdy_cnn_state_dict_np(tag="fdy10", nb_filters=synth.PMAM_FILTERS, dy_layers=FC.PMAM10_DY, depth=12)
    net = build(cnn=FC.FDY10_CNN_PARAM, state=sd)
    mel = torch.from_numpy(synth.det_uniform("pmam_fdy_d2/mel", (2, 128, 1000), -1.2, 1.2))
    feat, _ = run_branch(net, mel.cuda(), False)
    got = feat.view(2, 250, 384).transpose(1, 2)[:, ::16, ::10]
    emu, _, _ = branch_ref(sd, mel, synth.PMAM_POOLING, FC.PMAM10_DY, False, None, None, torch.float32, q=half)
    e_emu = float(np.abs(emu.view(2, 250, 384).transpose(1, 2)[:, ::16, ::10].numpy() - g["pm10_cnn_s"]).max())
    e_got = float(np.abs(got.cpu().numpy() - g["pm10_cnn_s"]).max())
    log(LOG, f"10-layer stack eval: features max err {e_got:.3e}, 16-bit storage emulated on the CPU {e_emu:.3e} (bound: twice that), "
             f"|feat| max {np.abs(g['pm10_cnn_s']).max():.3e}")
    assert e_got <= 2 * e_emu


# ================================================================================================ model level
def draws(g, pre):
    return dict(noise=torch.from_numpy(g[pre + "_noise"]), probs=torch.from_numpy(g[pre + "_probs"]), rand_idx=torch.from_numpy(g[pre + "_rand_idx"]))


def test_post_pretrain_eval_vs_reference(golden):
    from transformer4sed_amd.pmam_trainer import prototype_posteriors
    g = golden("pmam_fdy_d2")
    net = build().eval()
    mel = torch.from_numpy(synth.det_uniform("pmam_fdy_d2/mel", (2, 128, 1000), -1.2, 1.2)).cuda()
    net._mlm_draws = draws(g, "ev")
    with torch.no_grad():
        pred, other = net(mel, encoder_win=False)
    assert (other["mask_id_seq"].cpu().numpy() == g["ev_mask_ids"]).all()
    close(other["frame_before_mask"][S], g["ev_fbm_s"], 6e-3, 2e-3, what="eval merged projector sequence")
    close(other["at_out"], g["ev_at_out"], 1e-3, what="eval AT head")
    close(pred[S], g["ev_pred_s"], 8e-3, 2e-3, what="eval MLM logits")
    protos = F.normalize(torch.from_numpy(synth.det_normal("pmam/gmm_means", (30, 768))), dim=-1).cuda()
    strong = prototype_posteriors(pred, protos)
    strong = strong if strong.shape[1] == 1000 else strong.transpose(1, 2)
    close(strong[:, ::25], g["ev_strong_s"], 1e-3, what="eval prototype posteriors")


def test_post_pretrain_train_step_vs_reference(golden):
    """Train mode: unmerged LoRA, batch statistics in both kinds of BatchNorm, dropout 0.5 under the recorded keep-masks; the loss,
    every gradient norm and the running statistics after the forward."""
    from transformer4sed_amd.pmam_trainer import mark_only_lora_as_trainable, ProtoBCE
    g = golden("pmam_fdy_d2")
    B = 2
    net = build(dropout=float(g["drop_p"]))
    mark_only_lora_as_trainable(net.backbone)
    net.backbone.norm.weight.requires_grad_(True)
    net.backbone.norm.bias.requires_grad_(True)
    net.train()
    net._mlm_draws = draws(g, "tr")
    masks = FC.drop_masks_np("pmam_fdy_d2", B, synth.FDY_FILTERS, synth.FDY_POOLING, float(g["drop_p"]))
    net._drop_masks = [torch.from_numpy(m.reshape(-1, m.shape[-1]).astype(np.uint8)).cuda() for m in masks]
    mel = torch.from_numpy(synth.det_uniform("pmam_fdy_d2/mel", (B, 128, 1000), -1.2, 1.2)).cuda()
    gmm = torch.from_numpy(synth.det_normal("pmam/gmm_means", (30, 768))).cuda()
    labels = torch.from_numpy(synth.synth_strong_labels(B, n_classes=30, seed=500)).cuda()
    pred, other = net(mel, encoder_win=False)
    close(other["frame_before_mask"][S], g["tr_fbm_s"], 6e-3, 2e-3, what="train merged sequence")
    close(pred[S], g["tr_pred_s"], 8e-3, 2e-3, what="train MLM logits")
    close(other["at_out"], g["tr_at_out"], 1e-3, what="train AT head")
    sd_after = net.state_dict()
    for i in range(len(synth.FDY_FILTERS)):
        for st in ("running_mean", "running_var"):
            close(sd_after[f"cnn.cnn.batchnorm{i}.{st}"], g[f"tr_bn{i}_{st}"], 3e-3, 1e-2, what=f"BatchNorm2d {i} {st}")
            if i in DYN:
                close(sd_after[f"cnn.cnn.conv{i}.attention.bn.{st}"], g[f"tr_abn{i}_{st}"], 3e-3, 1e-2, what=f"BatchNorm1d {i} {st}")
    assert int(sd_after["cnn.cnn.conv1.attention.bn.num_batches_tracked"]) == 4 == int(sd_after["cnn.cnn.batchnorm0.num_batches_tracked"])
    protos = F.normalize(gmm, dim=-1)
    loss_strong = ProtoBCE.apply(pred, protos, labels, other["mask_id_seq"].reshape(-1), 0.1)
    loss_weak = F.binary_cross_entropy(other["at_out"], (labels.sum(-1) >= 1).float())
    loss = loss_strong + 0.1 * loss_weak
    close(loss, g["tr_loss"], 0, 2e-3, what="loss")
    rec = record_dfeat(net)
    loss.backward()
    emu_g, _ = emulated_grad_errors(synth.fdy_cnn_state_dict_np(depth=12), mel.cpu(), masks, rec["dfeat"].cpu(), drop_p=float(g["drop_p"]))
    grad_norms(net, g, "post-pretrain", emu_g)


def grad_norms(net, g, what, emu_g):
    """Every gradient norm within 3 % of the reference's (the rule of tests/test_gpu_pmam.py, with its rule for the conv biases); an
    attention-head parameter: `grad_bound` with the branch's emulated error under the same spectrograms, weights, dropout masks and the
    upstream gradient the branch's backward received in this run (`record_dfeat`; the CPU has no restatement of the rest of the model)."""
    names = [str(n) for n in g["tr_grad_names"]]
    got = {n for n, p in net.named_parameters() if p.grad is not None}
    assert got == set(names), (sorted(got - set(names))[:5], sorted(set(names) - got)[:5])
    pn = dict(net.named_parameters())
    bad = []
    for n, norm in zip(names, g["tr_grad_norms"]):
        gn = float(pn[n].grad.double().norm())
        if re.fullmatch(r"cnn\.cnn\.conv\d\.bias", n):      # true gradient zero behind a BatchNorm: rounding noise on both sides
            assert gn < 2e-2 * float(pn[n.replace(".bias", ".weight")].grad.double().norm()), n
            continue
        rel = abs(gn - norm) / max(norm, 1e-12)
        bound = grad_bound(n, emu_g) if n.startswith("cnn.cnn.") else 0.03
        log(MLOG, f"{what}: |grad {n}| {gn:.4e} ref {norm:.4e} off by {rel:.4f} (bound {bound:.4f}"
                  + (f", emulated relative L2 error {emu_g[n]:.4f})" if ".attention." in n else ")"))
        if rel >= bound:
            bad.append((n, rel, bound))
    assert not bad, bad


def test_finetune_stage_vs_reference(golden):
    g = golden("pmam_fdy_ft_d2")
    B = 2
    mel = torch.from_numpy(synth.det_uniform("pmam_fdy_ft_d2/mel", (B, 128, 1000), -1.2, 1.2)).cuda()
    net = build(ft=True).eval()
    pm = torch.zeros(B, 1000, dtype=torch.bool)
    pm[0, 900:] = True
    with torch.no_grad():
        s1, w1, o1 = net(mel, encoder_win=False, temp_w=1)
        s2, w2, _ = net(mel, encoder_win=False, temp_w=0.5, pad_mask=pm.cuda())
        s3, w3, o3 = net(mel, encoder_win=True, mix_rate=0.5, win_param=[512, 49], temp_w=0.5)
    close(s1, g["strong"], 1e-3, what="strong")
    close(w1, g["weak"], 1e-3, what="weak")
    close(o1["at_out"], g["at_out"], 1e-3, what="at_out")
    close(s2, g["strong_t05_pad"], 1e-3, what="strong temp_w 0.5 + pad mask")
    close(w2, g["weak_t05_pad"], 1e-3, what="weak temp_w 0.5 + pad mask")
    assert float(s2[0, :, 900:].abs().max()) == 0.0
    close(s3, g["strong_win49"], 1e-3, what="strong encoder_win")
    close(w3, g["weak_win49"], 1e-3, what="weak encoder_win")
    close(o3["frame_before_mask"][:, ::25, ::16], g["fbm_win49_s"], 8e-3, 2e-3, what="windowed merged sequence")
    net = build(ft=True, dropout=0.0).train()
    strong, weak, other = net(mel, encoder_win=False, temp_w=1)
    loss = (strong * torch.from_numpy(synth.det_uniform("pmam_fdy_ft_d2/gs", tuple(strong.shape))).cuda()).sum() + \
           (weak * torch.from_numpy(synth.det_uniform("pmam_fdy_ft_d2/gw", tuple(weak.shape))).cuda()).sum() + \
           (other["at_out"] * torch.from_numpy(synth.det_uniform("pmam_fdy_ft_d2/ga", tuple(other["at_out"].shape))).cuda()).sum()
    close(loss, g["tr_loss"], 0, 2e-3, what="fine-tune loss")
    rec = record_dfeat(net)
    loss.backward()
    emu_g, _ = emulated_grad_errors(synth.fdy_cnn_state_dict_np(depth=12, mlm=False, lora_r=0, class_num=10), mel.cpu(), None, rec["dfeat"].cpu())
    grad_norms(net, g, "fine-tune", emu_g)


# ================================================================================================ trainer, cache rule, base branch
ATT_NAMES = ["cnn.cnn.conv2.weight", "cnn.cnn.conv2.attention.conv1d1.weight", "cnn.cnn.conv2.attention.bn.weight", "cnn.cnn.conv2.attention.bn.bias",
             "cnn.cnn.conv2.attention.conv1d2.weight", "cnn.cnn.conv2.attention.conv1d2.bias"]


def test_pmam_trainer_two_steps():
    """Two steps of PmamTrainer (frontend, augmentation, dropout 0.5, prototype loss, backward, fused AdamW) on a fixed batch, wired as
    bench.build_pmam wires the base branch: the loss is finite and decreases, the basis kernels and the attention head move."""
    import json
    import random
    import bench
    from transformer4sed_amd.passt_cnn import PaSST_CNN
    from transformer4sed_amd.pmam_trainer import PmamTrainer, get_param_lr, mark_only_lora_as_trainable
    from transformer4sed_amd.scheduler import ExponentialDown
    from transformer4sed_amd.trainer import FusedAdamWEMA
    cfg = json.loads(json.dumps(bench.PMAM))
    ps = dict(cfg["PaSST_CNN"]["init_kwargs"]["passt_sed_param"], load_pretrained_model=False, encoder_depth=2, passt_feature_layer=2)
    net = PaSST_CNN(passt_sed_param=ps, cnn_param=dict(FC.FDY_CNN_PARAM))
    sd = synth.fdy_cnn_state_dict_np(depth=12)
    net.load_state_dict({k: torch.from_numpy(np.asarray(sd[k])) for k in net.state_dict()}, strict=True)
    net = net.cuda()
    mark_only_lora_as_trainable(net.backbone)
    groups = get_param_lr(net, cfg["opt"]["param_groups"])
    for gr in groups:      # a fixed batch and a larger step: the loss has to move at once
        gr["lr"] *= 20
    opt = FusedAdamWEMA(net, groups, ema_net=None, betas=(0.9, 0.999), eps=1e-8)
    sched = ExponentialDown(opt, start_iter=10000, total_iter=20000, exponent=-1.5, warmup_iter=0, warmup_rate=0.1)
    trainer = PmamTrainer(net, opt, sched, torch.from_numpy(synth.det_normal("pmam/gmm_means", (30, 768))), cfg)
    net.train()
    wav = torch.from_numpy(synth.synth_wav(4, seed=77)).cuda()
    labels = torch.from_numpy(synth.synth_strong_labels(4, n_classes=30, seed=77)).cuda()
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    losses = []
    for _ in range(2):      # the same augmentation and masking draws in both steps
        random.seed(3); np.random.seed(3); torch.manual_seed(3)
        losses.append(float(trainer.step(wav, labels.clone())["loss_total"]))
    log(MLOG, f"FDY PmamTrainer losses: {losses}")
    assert all(np.isfinite(losses)) and losses[1] < losses[0]
    for n in ATT_NAMES:
        assert not torch.equal(before[n], dict(net.named_parameters())[n].detach()), n
    assert int(net.state_dict()["cnn.cnn.conv2.attention.bn.num_batches_tracked"]) == 3 + 2


def test_mean_teacher_steps_move_the_ema_copies():
    """The fine-tune stage's mean-teacher trainer (FusedAdamWEMA with an EMA teacher, sliding windows): the new parameters and their EMA
    copies move, the teacher's BatchNorm1d counters advance."""
    import json
    from copy import deepcopy
    import bench
    from transformer4sed_amd.pmam_trainer import get_param_lr
    from transformer4sed_amd.scheduler import ExponentialDown
    from transformer4sed_amd.trainer import FusedAdamWEMA, MatSedTrainer
    net = build(ft=True, dropout=0.5)
    ema = deepcopy(net)
    for p in ema.parameters():
        p.detach_()
    cfg = json.loads(json.dumps(bench.FINETUNE2))
    cfg["PaSST_CNN"] = cfg.pop("PaSST_SED")
    cfg["training"]["batch_size"] = [2, 0, 2, 2]
    lr = dict(cnn=dict(lr=1e-3, weight_decay=1e-4), passt=dict(lr=1e-4, weight_decay=1e-4, freeze_layer=0, step_lr=1),
              decoder=dict(lr=1e-3, weight_decay=1e-4), head=dict(lr=1e-3, weight_decay=1e-4))
    opt = FusedAdamWEMA(net, get_param_lr(net, lr), ema_net=ema)
    sched = ExponentialDown(opt, start_iter=100, total_iter=200, exponent=-1, warmup_iter=0, warmup_rate=0.1)
    net.train(); ema.train()
    tr = MatSedTrainer(net, ema, opt, sched, cfg, epoch_len=10)
    wav = torch.from_numpy(synth.synth_wav(6, seed=5)).cuda()
    labels = torch.from_numpy(synth.synth_batch_labels(2, 2, 2, seed=5)).cuda()
    before = {n: (dict(net.named_parameters())[n].detach().clone(), dict(ema.named_parameters())[n].detach().clone()) for n in ATT_NAMES}
    losses = [float(tr.finetune_step(wav, labels.clone())["loss_total"]) for _ in range(2)]
    log(MLOG, f"FDY fine-tune trainer losses: {losses}")
    assert all(np.isfinite(losses))
    for n in ATT_NAMES:
        assert not torch.equal(before[n][0], dict(net.named_parameters())[n].detach()), n
        assert not torch.equal(before[n][1], dict(ema.named_parameters())[n].detach()), n
    assert int(ema.state_dict()["cnn.cnn.conv2.attention.bn.num_batches_tracked"]) == 3 + 2, "the teacher runs in train mode"


def test_in_place_parameter_writes_reach_the_next_forward(net7):
    """The cached weight image of `conv{i}.weight` is rebuilt iff its master moved; the attention parameters are read from the masters."""
    sd_np = synth.fdy_cnn_state_dict_np(depth=12)
    net7.load_state_dict({k: torch.from_numpy(np.asarray(sd_np[k])) for k in net7.state_dict()}, strict=True)
    mel = torch.from_numpy(synth.det_uniform("fdy/writes/mel", (2, 128, 1000), -1.2, 1.2)).cuda()
    f0, _ = run_branch(net7, mel, False)
    f0b, _ = run_branch(net7, mel, False)
    assert torch.equal(f0, f0b)
    pn = dict(net7.named_parameters())
    with torch.no_grad():
        pn["cnn.cnn.conv3.weight"][2].mul_(1.5)
    f1, _ = run_branch(net7, mel, False)
    assert not torch.equal(f0, f1)
    with torch.no_grad():
        pn["cnn.cnn.conv3.attention.conv1d2.bias"][1].add_(40.0)
    f2, _ = run_branch(net7, mel, False)
    assert not torch.equal(f1, f2)
    r64, _, _ = branch_ref({k: v.detach().cpu().numpy() for k, v in net7.state_dict().items()}, mel.cpu(), synth.FDY_POOLING, synth.FDY_DY_LAYERS, False, None,
                           None, torch.float64)
    assert maxerr(f2, r64) < 0.05 * float(r64.abs().max()), "and it is the written values that are used"


def test_base_branch_posteriors_are_bit_equal_to_the_parent_commits(golden):
    """`cnn_name="base"` (and the key absent) runs what it ran before the FDY branch existed: the evaluation-mode posteriors of the
    fine-tune-stage model on the PMAM synthetic weights equal, bit for bit, what the parent commit's build produced on an MI355X
    (tests/golden/pmam_ft_base_parent.npz; the same dump came out of two processes there)."""
    from transformer4sed_amd.passt_cnn import PaSST_CNN
    g = golden("pmam_ft_base_parent")
    ps = {k: v for k, v in PASST.items() if k not in ("lora_config", "mlm_dict")}
    ps.update(mlm=False, class_num=10, passt_feature_layer=2, encoder_depth=2)
    base = dict(n_in_channel=1, activation="cg", conv_dropout=0.5, kernel_size=[3] * 10, padding=[1] * 10, stride=[1] * 10,
                nb_filters=list(synth.PMAM_FILTERS), pooling=[list(p) for p in synth.PMAM_POOLING])
    mel = torch.from_numpy(synth.det_uniform("pmam_ft_d2/mel", (2, 128, 1000), -1.2, 1.2)).cuda()
    sd = synth.pmam_state_dict_np(depth=12, mlm=False, lora_r=0, class_num=10)
    for cnn in (dict(base), dict(base, cnn_name="base")):
        net = PaSST_CNN(passt_sed_param=dict(ps), cnn_param=cnn)
        net.load_state_dict({k: torch.from_numpy(np.asarray(sd[k])) for k in net.state_dict()}, strict=True)
        net = net.cuda().eval()
        with torch.no_grad():
            s, w, o = net(mel, encoder_win=False, temp_w=1)
        assert np.array_equal(s.cpu().numpy(), g["strong"]) and np.array_equal(w.cpu().numpy(), g["weak"])
        assert np.array_equal(o["at_out"].cpu().numpy(), g["at_out"])
