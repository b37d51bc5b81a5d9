"""Local-window attention of the context network (`PaSST_SED(decoder_win_len=...)`; needs an MI355X).

Kernel level: `sed_relpos_attn_band_fwd` / `sed_relpos_attn_band_bwd` against an fp32 torch restatement of transformerXL.py:510-576 with
the mask of mask.py:7-23 applied as `masked_fill(-inf)` (transformerXL.py:530-532), the way tests/test_gpu_kernels.py tests the unbanded
entry points and with its tolerances.  Model level: the depth-2 synth-weight model against reference goldens made with a window
(tools/gen_band_golden.py), with the bounds of tests/test_gpu_model.py."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from transformer4sed_amd import ops  # noqa: E402
from transformer4sed_amd.ops import call, pad64, BF16, F16  # noqa: E402

DEV = "cuda"
HH = 12
# measured errors: SED_TEST_LOG_DIR, else test_logs/ at the repository root (kept out of git), as tests/test_gpu_batch_scale.py
LOGDIR = os.environ.get("SED_TEST_LOG_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_logs")
LOG = os.path.join(LOGDIR, "band_kernel_errors.log")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MIXED = [2, 3, 16, 64, 100, 130, 2, 3, 16, 64, 100, 130]      # one width per head; head 5 / 11 also cover "hw >= T" at the short lengths


def report(name, err, scale=None):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(f"{name}: max_abs_err={err:.4e}" + (f" ref_scale={scale:.3e}" if scale is not None else "") + "\n")


def maxerr(a, b):
    return float((a.double() - b.double()).abs().max())


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def r16(x):
    return x.to(BF16).float()


def widths_of(w, T):
    """The parametrised width -> 12 widths ('full': hw >= T on every head; 'mixed': all of the widths, one per head, the widest
    replaced by a full window on the last head)."""
    if w == "full":
        return [2 * T + 2] * HH
    if w == "mixed":
        return MIXED[:-1] + [2 * T + 2]
    return [w] * HH


def band_masks(T, widths):
    """[H, T(query), T(key)] bool, True = masked: the closed form of mask.py:7-23 for each head."""
    i = torch.arange(T, device=DEV).view(1, T, 1)
    j = torch.arange(T, device=DEV).view(1, 1, T)
    hw = torch.tensor([w // 2 for w in widths], device=DEV).view(-1, 1, 1)
    return ~((j >= i - hw) & (j < i + hw))


def hw_tensor(widths):
    return torch.tensor([w // 2 for w in widths], dtype=torch.int32, device=DEV)


def relpos_ref(qu, qv, k, v, P, T, mask):
    """qu, qv, k, v [BH, T, 64] fp32; P [H, R, 64]; mask [H, T, T] bool (True = masked) -> out [BH, T, 64], masked scores."""
    BH = qu.shape[0]
    B = BH // HH
    ac = qu @ k.transpose(1, 2)
    bd_full = qv.view(B, HH, T, 64) @ P.transpose(1, 2).unsqueeze(0)
    i = torch.arange(T, device=qu.device).unsqueeze(1)
    j = torch.arange(T, device=qu.device).unsqueeze(0)
    idx = (j - i + T - 1).expand(B, HH, T, T)
    bd = torch.gather(bd_full, 3, idx).reshape(BH, T, T)
    s = ((ac + bd) * 0.125).masked_fill(mask.repeat(B, 1, 1), float("-inf"))      # index b H + h, like the reference's repeat / view
    return torch.softmax(s, dim=-1) @ v, s


class Case:
    """Operands of one (B, T, DT) in every layout the entry points take (as tests/test_gpu_kernels.py:789-794 makes them)."""

    def __init__(self, B, T, DT, seed=40):
        self.B, self.T, self.DT = B, T, DT
        self.f16 = 1 if DT == F16 else 0
        self.Tpad, self.R = pad64(T), 2 * T - 1
        self.Rpad = pad64(self.R)
        Tpad, R, Rpad = self.Tpad, self.R, self.Rpad
        self.qu, self.k, self.v = [r16(rnd(B * HH, T, 64, scale=1.2, seed=seed + i)) for i in range(3)]
        self.qv = r16(rnd(B * HH, T, 64, scale=1.2, seed=47))
        self.P = r16(rnd(HH, R, 64, scale=0.7, seed=48))
        self.Pp = torch.zeros(HH, Rpad, 64, dtype=DT, device=DEV); self.Pp[:, :R] = self.P.to(DT)
        self.Pt = torch.zeros(HH, 64, Rpad, dtype=BF16, device=DEV); self.Pt[:, :, :R] = self.P.to(BF16).transpose(1, 2)
        self.dO = r16(rnd(B, T, 768, seed=53))

    def tr(self, t, d):
        return torch.nn.functional.pad(t.transpose(1, 2), (0, self.Tpad - self.T)).to(d).contiguous()

    def fwd(self, hw, k=None, v=None, o_f32=False):
        """hw: int32 [H] device tensor -> band entry point; None -> the unbanded one."""
        B, T, DT = self.B, self.T, self.DT
        k = self.k if k is None else k
        v = self.v if v is None else v
        O = torch.empty(B, T, 768, dtype=torch.float32 if o_f32 else DT, device=DEV)
        Osp = torch.empty(B * T, 3 * 768, dtype=F16, device=DEV) if o_f32 else None
        lse = torch.empty(B * HH, T, device=DEV)
        a = (self.qu.to(DT), self.qv.to(DT), k.to(DT), self.tr(v, DT), self.Pp, O, Osp, lse, B, HH, T, self.Tpad, self.Rpad, self.f16,
             1 if o_f32 else 0)
        if hw is None:
            call("sed_relpos_attn_fwd", *a)
        else:
            call("sed_relpos_attn_band_fwd", *a, hw)
        return O, lse, Osp

    def bwd(self, hw, O, lse, stream=True, dSt=None, Pst=None):
        B, T, DT, Tpad, Rpad = self.B, self.T, self.DT, self.Tpad, self.Rpad
        dqkv = torch.empty(B * T, 2304, dtype=BF16, device=DEV)
        Dt = torch.empty(B * HH, T, device=DEV)
        dOh = torch.empty(B * HH, T, 64, dtype=BF16, device=DEV)
        dOt = torch.empty(B * HH, 64, Tpad, dtype=BF16, device=DEV)
        dSt = torch.zeros(B * HH, Tpad, Tpad, dtype=BF16, device=DEV) if dSt is None else dSt
        if stream and Pst is None:
            Pst = torch.zeros(B * HH, Tpad, Tpad, dtype=BF16, device=DEV)
        dP = torch.zeros(Rpad, 768, device=DEV)
        du = torch.zeros(HH, 64, device=DEV); dv = torch.zeros(HH, 64, device=DEV)
        a = (self.qu.to(DT), self.tr(self.qu, BF16), self.qv.to(DT), self.tr(self.qv, BF16), self.k.to(DT), self.tr(self.k, BF16),
             self.v.to(BF16), self.Pp, self.Pt, O, self.dO.to(BF16), lse, Dt, dOh, dOt, dqkv, dSt, Pst if stream else None, dP, du, dv,
             B, HH, T, Tpad, Rpad, 1, self.f16, self.f16)
        if hw is None:
            call("sed_relpos_attn_bwd", *a)
        else:
            call("sed_relpos_attn_band_bwd", *a, hw)
        return dict(dqkv=dqkv, dSt=dSt, Pst=Pst, dP=dP, du=du, dv=dv)


@pytest.mark.parametrize("DT", [BF16, F16])
@pytest.mark.parametrize("w", [2, 3, 16, 64, 100, 130, "full", "mixed"])
@pytest.mark.parametrize("B,T", [(1, 8), (1, 72), (1, 136), (1, 200), (2, 1000)])
def test_band_fwd_bwd(B, T, w, DT):
    c = Case(B, T, DT)
    f16, R = c.f16, c.R
    widths = widths_of(w, T)
    mask = band_masks(T, widths)
    hw = hw_tensor(widths)
    O, lse, _ = c.fwd(hw)
    O32, _, Osp = c.fwd(hw, o_f32=True)
    assert maxerr(O32.to(DT).float(), O.float()) == 0
    assert torch.equal(Osp, ops.split3(O32.view(B * T, 768), B * T, 768))     # the [hi | lo | hi] split-precision image of the fp32 output
    leaves = [t.clone().requires_grad_(True) for t in (c.qu, c.qv, c.k, c.v, c.P)]
    o, s = relpos_ref(*leaves, T, mask)
    oref = o.view(B, HH, T, 64).permute(0, 2, 1, 3).reshape(B, T, 768)
    e = maxerr(O.float(), oref); report(f"band fwd T={T} w={w} {DT}", e); assert e < (4e-3 if f16 else 2e-2)
    e = maxerr(lse, torch.logsumexp(s, -1) / math.log(2.0)); report(f"band lse T={T} w={w} {DT}", e); assert e < 3e-3
    oref.backward(c.dO)
    g1 = c.bwd(hw, O, lse, stream=True)
    g2 = c.bwd(hw, O, lse, stream=False)
    dqkv, dSt, Pst, dP = g1["dqkv"], g1["dSt"], g1["Pst"], g1["dP"]
    # dK / dV from the score-recomputing kernel (no P^T slab): same dQ bits, dK / dV to bf16 rounding (test_gpu_kernels.py:825-827)
    assert torch.equal(g2["dqkv"][:, :768], dqkv[:, :768])
    e = maxerr(g2["dqkv"][:, 768:].float(), dqkv[:, 768:].float()); report(f"band bwd dk|dv stream vs recompute T={T} w={w}", e)
    assert e < 0.02 * float(dqkv[:, 768:].float().abs().max()) + 2e-3
    # the slabs (rows = keys, columns = queries): exact zeros at every out-of-band pair, nothing outside [T, T]; P^T columns sum to 1
    mT = mask.transpose(1, 2).repeat(B, 1, 1)
    for slab in (Pst, dSt, g2["dSt"]):
        assert float(slab[:, T:, :].float().abs().max()) == 0 and float(slab[:, :, T:].float().abs().max()) == 0
        assert float(slab[:, :T, :T].float().masked_fill(~mT, 0.0).abs().max()) == 0
    assert maxerr(Pst[:, :T, :T].float().sum(1), torch.ones(B * HH, T, device=DEV)) < 2e-2
    g = dqkv.float().view(B, T, 3, HH, 64).permute(2, 0, 3, 1, 4).reshape(3, B * HH, T, 64)
    dq_ref = leaves[0].grad + leaves[1].grad
    for got, ref, nm in ((g[0], dq_ref, "dq"), (g[1], leaves[2].grad, "dk"), (g[2], leaves[3].grad, "dv")):
        e = maxerr(got, ref); sc = float(ref.abs().max()); report(f"band bwd {nm} T={T} w={w}", e, sc)
        assert e < 0.03 * sc + 5e-3
    du_ref = leaves[0].grad.view(B, HH, T, 64).sum((0, 2)); dv_ref = leaves[1].grad.view(B, HH, T, 64).sum((0, 2))
    for got, ref, nm in ((g1["du"], du_ref, "du"), (g1["dv"], dv_ref, "dv_bias")):
        e = maxerr(got, ref); sc = float(ref.abs().max()); report(f"band bwd {nm} T={T} w={w}", e, sc); assert e < 0.03 * sc + 2e-2
    dP_ref = leaves[4].grad.permute(1, 0, 2).reshape(R, 768)
    for dPx in (dP, g2["dP"]):
        e = maxerr(dPx[:R], dP_ref); sc = float(dP_ref.abs().max()); report(f"band bwd dP T={T} w={w}", e, sc)
        assert e < 0.03 * sc + 2e-2
        # rows r = j - i + T - 1 outside -hw <= j - i < hw: exact zeros
        d = torch.arange(R, device=DEV) - (T - 1)
        for h in range(HH):
            out = (d < -(widths[h] // 2)) | (d >= widths[h] // 2)
            assert float(dPx[:R, 64 * h:64 * h + 64][out].abs().sum()) == 0


@pytest.mark.parametrize("i0", [300, 320])      # inside a 64-key tile; on a tile boundary
def test_band_locality(i0):
    """Keys past the right edge of a query's window (and before its left edge) do not reach its output: O and LSE bit for bit."""
    T, hw = 1000, 50
    c = Case(1, T, F16)
    hwt = hw_tensor([2 * hw] * HH)
    O, lse, _ = c.fwd(hwt)
    k2, v2 = c.k.clone(), c.v.clone()
    k2[:, i0 + hw:] = r16(rnd(HH, T - i0 - hw, 64, scale=1.2, seed=91))
    v2[:, i0 + hw:] = r16(rnd(HH, T - i0 - hw, 64, scale=1.2, seed=92))
    O2, lse2, _ = c.fwd(hwt, k=k2, v=v2)
    assert torch.equal(O2[:, :i0 + 1], O[:, :i0 + 1]) and torch.equal(lse2[:, :i0 + 1], lse[:, :i0 + 1])
    assert not torch.equal(O2[:, i0 + 1], O[:, i0 + 1])       # the next query sees key i0 + hw
    k3, v3 = c.k.clone(), c.v.clone()
    k3[:, :i0 - hw] = r16(rnd(HH, i0 - hw, 64, scale=1.2, seed=93))
    v3[:, :i0 - hw] = r16(rnd(HH, i0 - hw, 64, scale=1.2, seed=94))
    O3, lse3, _ = c.fwd(hwt, k=k3, v=v3)
    assert torch.equal(O3[:, i0:], O[:, i0:]) and torch.equal(lse3[:, i0:], lse[:, i0:])
    assert not torch.equal(O3[:, i0 - 1], O[:, i0 - 1])       # the previous query sees key i0 - 1 - hw


@pytest.mark.parametrize("DT", [BF16, F16])
@pytest.mark.parametrize("B,T", [(1, 136), (2, 1000)])
def test_band_full_window_equals_unbanded(B, T, DT):
    """hw >= T on every head: the band kernels walk every tile in the order of the unbanded ones and no score is masked.  Forward (O,
    LSE), dq | dk | dv and both slabs are bit-identical; du, dv and dP are sums of atomics in both forms and agree within the tolerances
    of the parity test."""
    c = Case(B, T, DT)
    hw = hw_tensor([2 * T + 2] * HH)
    O, lse, _ = c.fwd(None)
    Ob, lseb, _ = c.fwd(hw)
    assert torch.equal(Ob, O) and torch.equal(lseb, lse)
    for stream in (True, False):
        a, b = c.bwd(None, O, lse, stream=stream), c.bwd(hw, O, lse, stream=stream)
        assert torch.equal(a["dqkv"], b["dqkv"]) and torch.equal(a["dSt"], b["dSt"])
        if stream:
            assert torch.equal(a["Pst"], b["Pst"])
        for nm in ("du", "dv", "dP"):
            sc = float(a[nm].abs().max())
            assert maxerr(a[nm], b[nm]) < 0.03 * sc + 2e-2, nm


@pytest.mark.parametrize("w", [100, "mixed"])
def test_band_on_slabs_of_an_unbanded_call(w):
    """The engine's slab pool: a banded backward on slabs that still hold the full-window content of an unbanded backward (tiles the
    band never visits stay stale) gives the dqkv and dP of freshly zeroed slabs (bound: tests/test_gpu_model.py:1025, run to run)."""
    B, T = 2, 1000
    c = Case(B, T, F16)
    O, lse, _ = c.fwd(None)
    full = c.bwd(None, O, lse)
    stale_d, stale_p = full["dSt"], full["Pst"]
    widths = widths_of(w, T)
    hw = hw_tensor(widths)
    Ob, lseb, _ = c.fwd(hw)
    fresh = c.bwd(hw, Ob, lseb)
    before = stale_d.clone()
    dirty = c.bwd(hw, Ob, lseb, dSt=stale_d, Pst=stale_p)
    if w == 100:       # the hazard is real: most of the slab still holds the unbanded call's values
        far = torch.zeros(T, T, dtype=torch.bool, device=DEV)
        far[:256, 512:] = True
        assert torch.equal(dirty["dSt"][:, :T, :T][:, far], before[:, :T, :T][:, far]) and float(before[:, :T, :T][:, far].float().abs().max()) > 0
    for nm in ("dqkv", "dP"):
        a, b = fresh[nm].float(), dirty[nm].float()
        assert maxerr(a, b) <= 2e-3 * float(a.abs().max()) + 1e-7, nm


# ------------------------------------------------------------------------------------------------ model level
from transformer4sed_amd import synth  # noqa: E402
from transformer4sed_amd.passt_sed import PaSST_SED  # noqa: E402

MLOG = os.path.join(LOGDIR, "band_model_errors.log")
HEAD_WIDTHS = [8, 16, 32, 64, 100, 128, 200, 256, 400, 600, 1000, 2000]


def mreport(name, err, extra=""):
    os.makedirs(os.path.dirname(MLOG), exist_ok=True)
    with open(MLOG, "a") as f:
        f.write(f"{name}: max_abs_err={err:.4e} {extra}\n")


def nerr(a, b):
    a = torch.as_tensor(np.asarray(a)) if not isinstance(a, torch.Tensor) else a
    b = torch.as_tensor(np.asarray(b)) if not isinstance(b, torch.Tensor) else b
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def build_model(mlm, win, depth=2, feature_layer=2):
    """tests/test_gpu_model.py `_build` with a window: the synth weights carry no mask, the model's own buffer is the constructor's."""
    kw = dict(mlm_dict=dict(strategy="block", block_width=10, mask_rate=0.75, out_dim=768)) if mlm else {}
    net = PaSST_SED(passt_feature_layer=feature_layer, f_pool="mean_pool", decode_ratio=10, at_adapter=True, decoder="transformerXL",
                    decoder_layer_num=3, decoder_pos_emd_len=1000, mlm=mlm, load_pretrained_model=False, encoder_depth=depth,
                    decoder_win_len=win, **kw)
    sd = synth.matsed_state_dict_np(tag="w768", depth=12, mlm=mlm)
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


@pytest.mark.parametrize("tag,win", [("model_d768_l2_win100", 100), ("model_d768_l2_winheads", HEAD_WIDTHS)])
def test_band_model_vs_reference_golden(golden, tag, win):
    """Finetune-mode outputs, loss and every gradient norm of the depth-2 model with a window against the reference's
    (bounds: test_model_depth2_vs_reference_golden).  The fixture records that `strong` lies >= 0.47 from the full-window model."""
    g = golden(tag)
    assert float(g["strong_vs_full_max"]) >= 20 * 1e-3
    B = 2
    mel = torch.from_numpy(synth.det_uniform(f"{tag}/mel", (B, 128, 1000), -1.2, 1.2)).to(DEV)
    net = build_model(False, win)
    net.eval()
    with torch.no_grad():
        strong, weak, other = net(mel, encoder_win=False, temp_w=1)
    for nm, got in (("strong", strong), ("weak", weak), ("at_out", other["at_out"])):
        e = nerr(got, g[nm]); mreport(f"{tag} {nm} vs reference", e); print(f"{tag} {nm}: {e:.3e}"); assert e < 1e-3, (nm, e)
        # measured: win100 strong 5.3e-4, weak 9.0e-5, at_out 1.1e-4; winheads strong 5.4e-4, weak 1.4e-4, at_out 6.8e-5
    S = lambda t: t[:, ::25, ::16]
    e = nerr(S(other["frame_before_mask"]), g["interp_s"]); assert e < 2e-2
    strong, weak, other = net(mel, encoder_win=False, temp_w=1)
    gs = torch.from_numpy(synth.det_uniform(f"{tag}/gs", tuple(strong.shape))).to(DEV)
    gw = torch.from_numpy(synth.det_uniform(f"{tag}/gw", tuple(weak.shape))).to(DEV)
    ga = torch.from_numpy(synth.det_uniform(f"{tag}/ga", tuple(other["at_out"].shape))).to(DEV)
    loss = (strong * gs).sum() + (weak * gw).sum() + (other["at_out"] * ga).sum()
    loss.backward()
    rel = abs(float(loss) - float(g["ft_loss"])) / abs(float(g["ft_loss"])); mreport(f"{tag} loss rel", rel); print(f"{tag} loss rel: {rel:.3e}")
    assert rel < 2e-3          # measured: win100 4.4e-4, winheads 1.0e-5
    names = [str(n) for n in g["ft_grad_names"]]
    params = dict(net.named_parameters())
    got_names = {n for n, p in params.items() if p.grad is not None}
    assert got_names == set(names), (got_names ^ set(names))
    worst = 0.0
    for n, norm in zip(names, g["ft_grad_norms"]):
        r = abs(float(params[n].grad.double().norm()) - norm) / (norm + 1e-12)
        mreport(f"{tag} grad {n}", r)
        worst = max(worst, r)
        assert r < grad_tol(n, 3e-3), (n, r)          # measured worst: win100 1.4e-3, winheads 6.9e-4
    mreport(f"{tag} worst grad-norm rel err", worst); print(f"{tag} worst grad-norm rel err: {worst:.3e}")


@pytest.mark.parametrize("tag,win", [("model_d768_l2_win100", 100), ("model_d768_l2_winheads", HEAD_WIDTHS)])
def test_band_model_mlm_vs_reference_golden(golden, tag, win):
    """MLM-mode prediction, loss and gradient norms with a window (bounds: test_model_mlm_vs_reference_golden)."""
    g = golden(tag)
    B = 2
    mel = torch.from_numpy(synth.det_uniform(f"{tag}/mel", (B, 128, 1000), -1.2, 1.2)).to(DEV)
    net = build_model(True, win)
    net.train()
    for p in net.backbone.parameters():
        p.requires_grad_(False)
    net._mlm_draws = dict(noise=torch.from_numpy(g["mlm_noise"]), probs=torch.from_numpy(g["mlm_probs"]), rand_idx=torch.from_numpy(g["mlm_rand_idx"]))
    pred, other = net(mel, encoder_win=False)
    assert np.array_equal(other["mask_id_seq"].cpu().numpy(), g["mlm_mask_ids"])
    S = lambda t: t[:, ::25, ::16]
    e = nerr(S(pred), g["mlm_pred_s"]); sc = float(np.abs(g["mlm_pred_s"]).max()); mreport(f"{tag} mlm pred", e, f"scale={sc:.2f}")
    print(f"{tag} mlm pred: {e:.3e} scale {sc:.2f}")
    assert e < 1e-3 * sc          # measured: win100 2.5e-3 on values up to 3.99 (6.1e-4 of scale), winheads 1.8e-3 on 3.86 (4.6e-4)
    loss = torch.nn.functional.mse_loss(other["frame_before_mask"][other["mask_id_seq"]], pred[other["mask_id_seq"]])
    rel = abs(float(loss) - float(g["mlm_loss"])) / float(g["mlm_loss"]); mreport(f"{tag} mlm loss rel", rel); print(f"{tag} mlm loss rel: {rel:.3e}")
    assert rel < 1e-4          # measured: win100 8.5e-6, winheads 4.6e-5
    loss.backward()
    names = [str(n) for n in g["mlm_grad_names"]]
    params = dict(net.named_parameters())
    got_names = {n for n, p in params.items() if p.grad is not None}
    assert got_names == set(names), (got_names ^ set(names))
    worst = 0.0
    for n, norm in zip(names, g["mlm_grad_norms"]):
        r = abs(float(params[n].grad.double().norm()) - norm) / (norm + 1e-12)
        mreport(f"{tag} mlm grad {n}", r); worst = max(worst, r); assert r < grad_tol(n, 3e-3), (n, r)     # measured worst: win100 9.3e-4, winheads 6.5e-4
    print(f"{tag} mlm worst grad-norm rel err: {worst:.3e}")


def test_band_model_full_width_matches_windowless_and_backward_repeats():
    """hw >= T on every head is the windowless model (2e-4: the B-invariance bound of tests/test_gpu_model.py:1178); two backwards of
    one windowed model give the same gradients run to run (tests/test_gpu_model.py:1025); another sequence length is refused."""
    mel = torch.from_numpy(synth.det_uniform("band/mel", (2, 128, 1000), -1.2, 1.2)).to(DEV)
    plain, wide = build_model(False, None), build_model(False, [2000] * 12)
    plain.eval(); wide.eval()
    with torch.no_grad():
        s0, w0, _ = plain(mel, encoder_win=False)
        s1, w1, _ = wide(mel, encoder_win=False)
    d = nerr(s0, s1); mreport("band hw >= T vs windowless: strong", d); assert d < 2e-4
    d = nerr(w0, w1); assert d < 2e-4
    net = build_model(False, 100)
    net.train()
    w = torch.from_numpy(synth.det_uniform("band/w", (2, 10, 1000))).to(DEV)
    names = ["backbone.blocks.0.attn.qkv.weight", "decoder.encoder_blocks.1.attn.in_proj.weight", "decoder.encoder_blocks.0.attn.linear_pos.weight",
             "decoder.encoder_blocks.2.attn.pos_bias_v", "classifier.weight"]
    pn = dict(net.named_parameters())
    runs = []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        s, _, _ = net(mel, encoder_win=False)
        (s * w).sum().backward()
        runs.append([pn[n].grad.detach().clone() for n in names])
    for n, a, b in zip(names, *runs):
        assert nerr(a, b) <= 2e-3 * float(a.abs().max()) + 1e-7, n
    assert float((s - s0).abs().max()) > 20e-3          # and the window is not ignored
    net.decoder.seq_len = 999                           # (what decoder_pos_emd_len=999 would build)
    with pytest.raises(RuntimeError, match="decoder_pos_emd_len"):
        net(mel, encoder_win=False)


def test_band_pmam_model_runs():
    """PaSST_CNN takes the window through `passt_sed_param` (PMAM engine path): forward and backward run and the window moves the output."""
    from transformer4sed_amd.passt_cnn import PaSST_CNN
    passt = dict(class_num=30, f_pool="attention", decode_ratio=10, at_adapter=True, decoder="transformerXL", decoder_layer_num=3,
                 decoder_pos_emd_len=1000, decoder_dim=384, mlm=True, lora_config=dict(r=8, lora_alpha=1, requires_grad_pretrain=False),
                 mlm_dict=dict(strategy="block", block_width=10, mask_rate=0.8, out_dim=768, mask_style=[0.9, 0.05, 0.05]),
                 load_pretrained_model=False, passt_feature_layer=2, encoder_depth=2)
    cnn = dict(n_in_channel=1, activation="cg", conv_dropout=0, kernel_size=[3] * 10, padding=[1] * 10, stride=[1] * 10,
               nb_filters=list(synth.PMAM_FILTERS), pooling=[list(p) for p in synth.PMAM_POOLING])
    sd = synth.pmam_state_dict_np(depth=12)
    mel = torch.from_numpy(synth.det_uniform("band/pmam_mel", (2, 128, 1000), -1.2, 1.2)).to(DEV)
    outs = {}
    for key, win in (("none", None), ("w64", 64), ("wide", [2000] * 12)):
        net = PaSST_CNN(passt_sed_param=dict(passt, decoder_win_len=win), cnn_param=cnn)
        own = net.state_dict()
        net.load_state_dict({k: (own[k] if k == "decoder.att_mask" else torch.from_numpy(np.asarray(sd[k]))) for k in own}, strict=True)
        net = net.cuda().train()
        torch.manual_seed(11)          # the same MLM mask draws for the three models
        pred, other = net(mel, encoder_win=False)
        assert bool(torch.isfinite(pred).all())
        if key == "w64":
            pred.square().mean().backward()
            gr = net.decoder.encoder_blocks[0].attn.in_proj.weight.grad
            assert gr is not None and bool(torch.isfinite(gr).all()) and float(gr.abs().max()) > 0
        outs[key] = pred.detach()
    # (full-width window vs windowless on this train-mode PMAM forward: measured 1.3e-3 .. 1.6e-3 on MLM logits up to 6.9; printed, not bounded here --
    #  the equivalence is asserted bit for bit at kernel level and at 2e-4 on the MAT-SED posteriors above)
    print(f"pmam hw >= T vs windowless: {nerr(outs['none'], outs['wide']):.3e} on scale {float(outs['none'].abs().max()):.2f}")
    assert nerr(outs["none"], outs["w64"]) > 1e-2
