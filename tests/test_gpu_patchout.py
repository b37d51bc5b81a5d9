"""Structured frequency patchout, `PaSST_SED(s_patchout_f=s)` (needs an MI355X).

Kernel level: the five row-aware entry points of csrc/norm_elem.hip (`sed_im2col_rows`, `sed_assemble_tokens_rows{,_bwd}`,
`sed_fpool_rows_{fwd,bwd}`) against torch on the device with the bounds of tests/test_gpu_kernels.py::test_patch_tokens_fpool_interp,
at the smallest shapes where the row or N handling can go wrong: 8 scattered rows of a full-length clip, ONE row (the last) of a
window slab, 11 rows of a 3-patch slab; time offsets 0 and 7 (7 with 99 patches lies outside the 99-column table: refused).  With rows = identity, F = 12 each new entry point gives the bits of the
old one.  `sed_mhsa_fwd/bwd` at the sequence lengths that become reachable, with the bounds of `test_mhsa_fwd_bwd`.

Model level: the depth-2 synth-weight model in training mode against the reference goldens of tools/gen_patchout_golden.py with the
bounds of tests/test_gpu_conformer.py / test_gpu_band_attention.py (posteriors within 1e-3: the project's contract), and two steps
of the trainer against the reference's own `Trainer.train` under the same seeds (no injection: pins the draw order)."""
import json
import math
import os
import random
from copy import deepcopy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from transformer4sed_amd import synth  # noqa: E402
from transformer4sed_amd.ops import call, pad64, BF16, F16  # noqa: E402
from transformer4sed_amd.passt_sed import PaSST_SED  # noqa: E402

DEV = "cuda"
TAG, STEP_TAG = "model_d768_l2_patchout4", "trainstep_patchout"
LOGDIR = os.environ.get("SED_TEST_LOG_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_logs")
LOG = os.path.join(LOGDIR, "patchout_errors.log")
T = 1000
CASES = [(2, 0, 99, [0, 3, 4, 5, 6, 7, 9, 11]), (2, 490, 50, [11]), (3, 0, 3, list(range(11)))]


def report(name, err, extra=""):
    os.makedirs(LOGDIR, exist_ok=True)
    with open(LOG, "a") as f:
        f.write(f"{name}: {err:.4e} {extra}\n")
    print(f"{name}: {err:.3e} {extra}")


def maxerr(a, b):
    a = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))
    b = b if isinstance(b, torch.Tensor) else torch.from_numpy(np.asarray(b))
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def z(*s):
    return torch.zeros(*s, device=DEV)


def dev_rows(rows):
    return torch.tensor(rows, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("toffset", [0, 7])
@pytest.mark.parametrize("B,tstart,tp,rows", CASES)
def test_row_kernels_vs_torch(B, tstart, tp, rows, toffset):
    F_, N = len(rows), 2 + len(rows) * tp
    rd = dev_rows(rows)
    tag = f"B={B} tstart={tstart} tp={tp} F={F_} toffset={toffset}"
    dropped = [r for r in range(12) if r not in rows]
    # ---- im2col: the kept rows of the slab's patch grid, exactly
    mel = rnd(B, 128, T, seed=70)
    grid = mel[:, :, tstart:tstart + 10 * (tp - 1) + 16].unfold(1, 16, 10).unfold(2, 16, 10)      # [B, 12, tp, 16, 16]
    want = grid[:, rows].reshape(B * F_ * tp, 256)
    for f16, dt in ((0, BF16), (1, F16)):
        cols = torch.empty(B * F_ * tp, 256, dtype=dt, device=DEV)
        call("sed_im2col_rows", mel, cols, rd, F_, B, T, tstart, tp, f16)
        assert torch.equal(cols, want.to(dt)), (tag, dt)
    # ---- assembly forward: kept row f' carries freq_pe[:, rows[f']], time columns toffset .. toffset + tp
    conv = rnd(B * F_ * tp, 768, seed=71)
    cls, dist, npe = rnd(768, seed=72), rnd(768, seed=73), rnd(2, 768, seed=74)
    fpe, tpe = rnd(768, 12, seed=75), rnd(768, 99, seed=76)
    x = torch.empty(B, N, 768, device=DEV)
    if toffset + tp > 99:
        # 99 patches fill the time table: there is no column toffset + t to read (the reference draws no offset for such a pass,
        # passt.py:504).  The two entry points that take an offset refuse it; the other three were checked by this case's toffset = 0 twin.
        from transformer4sed_amd._lib import SedHipError
        with pytest.raises(SedHipError, match="bad argument"):
            call("sed_assemble_tokens_rows", conv, cls, dist, npe, fpe, tpe, rd, F_, toffset, x, B, tp)
        with pytest.raises(SedHipError, match="bad argument"):
            call("sed_assemble_tokens_rows_bwd", x, torch.empty(B * F_ * tp, 768, dtype=BF16, device=DEV), None, None, None, None, None,
                 rd, F_, toffset, B, tp)
        return
    call("sed_assemble_tokens_rows", conv, cls, dist, npe, fpe, tpe, rd, F_, toffset, x, B, tp)
    xr = conv.view(B, F_, tp, 768) + tpe.t()[toffset:toffset + tp].view(1, 1, tp, 768) + fpe.t()[rows].view(1, F_, 1, 768)
    xr = torch.cat([(cls + npe[0]).expand(B, 1, 768), (dist + npe[1]).expand(B, 1, 768), xr.reshape(B, F_ * tp, 768)], 1)
    e = maxerr(x, xr); report(f"assemble fwd {tag}", e); assert e < 1e-6
    # ---- assembly backward
    dx = rnd(B, N, 768, seed=77)
    dconv = torch.empty(B * F_ * tp, 768, dtype=BF16, device=DEV)
    dcls, ddist, dnp, dfr, dti = z(768), z(768), z(2, 768), z(768, 12), z(768, 99)
    call("sed_assemble_tokens_rows_bwd", dx, dconv, dcls, ddist, dnp, dfr, dti, rd, F_, toffset, B, tp)
    assert torch.equal(dconv, dx[:, 2:].reshape(-1, 768).to(BF16))
    assert maxerr(dcls, dx[:, 0].sum(0)) < 1e-5 and maxerr(ddist, dx[:, 1].sum(0)) < 1e-5
    assert maxerr(dnp[0], dx[:, 0].sum(0)) < 1e-5 and maxerr(dnp[1], dx[:, 1].sum(0)) < 1e-5
    d4 = dx[:, 2:].view(B, F_, tp, 768)
    fr_want, ti_want = z(768, 12), z(768, 99)
    fr_want[:, rows] = d4.sum((0, 2)).t()
    ti_want[:, toffset:toffset + tp] = d4.sum((0, 1)).t()
    ef, et = maxerr(dfr, fr_want), maxerr(dti, ti_want); report(f"assemble bwd dfreq {tag}", ef); report(f"assemble bwd dtime {tag}", et)
    assert ef < 1e-3 and et < 1e-3
    assert float(dfr[:, dropped].abs().max()) == 0          # dropped rows get nothing, exactly
    outside = [t for t in range(99) if not toffset <= t < toffset + tp]
    assert not outside or float(dti[:, outside].abs().max()) == 0
    dconv2 = torch.empty_like(dconv)          # every table frozen: only the GEMM operand is written
    call("sed_assemble_tokens_rows_bwd", dx, dconv2, None, None, None, None, None, rd, F_, toffset, B, tp)
    assert torch.equal(dconv2, dconv)
    # ---- f_pool forward / backward: the mean over the F rows the sequence holds
    g = 1 + 0.2 * rnd(768, seed=78); b = 0.1 * rnd(768, seed=79)
    pooled = torch.empty(B, tp, 768, device=DEV); pm = z(B * N); pr = z(B * N)
    call("sed_fpool_rows_fwd", x, g, b, 1e-5, pooled, pm, pr, B, tp, F_)
    xx = x.clone().requires_grad_(True); gg = g.clone().requires_grad_(True); bb = b.clone().requires_grad_(True)
    pref = torch.nn.functional.layer_norm(xx[:, 2:], (768,), gg, bb, 1e-5).view(B, F_, tp, 768).mean(1)
    e = maxerr(pooled, pref); report(f"fpool fwd {tag}", e); assert e < 2e-5
    dpool = rnd(B, tp, 768, seed=80)
    pref.backward(dpool)
    dtok = torch.empty(B, N, 768, device=DEV); dxa = z(B, N, 768); dg, db = z(768), z(768)
    call("sed_fpool_rows_bwd", dpool, x, pm, pr, g, dtok, dxa, dg, db, B, tp, F_)
    e = maxerr(dxa, xx.grad); sc = float(xx.grad.abs().max()); report(f"fpool bwd dx {tag}", e, f"scale={sc:.3e}"); assert e < 2e-4 * sc + 1e-6
    assert maxerr(dg, gg.grad) < 2e-3 * float(gg.grad.abs().max()) and maxerr(db, bb.grad) < 2e-3 * float(bb.grad.abs().max())


@pytest.mark.parametrize("B,tstart,tp,toffset", [(2, 0, 99, 0), (3, 490, 50, 7)])
def test_identity_rows_give_the_old_entry_points_bits(B, tstart, tp, toffset):
    """rows = 0..11 (as a device table, and as the null pointer), F = 12: every new entry point equals the old one on the same buffers."""
    N = 2 + 12 * tp
    mel = rnd(B, 128, T, seed=60)
    conv = rnd(B * 12 * tp, 768, seed=61)
    cls, dist, npe, fpe, tpe = rnd(768, seed=62), rnd(768, seed=63), rnd(2, 768, seed=64), rnd(768, 12, seed=65), rnd(768, 99, seed=66)
    dx = rnd(B, N, 768, seed=67)
    g = 1 + 0.2 * rnd(768, seed=68); b = 0.1 * rnd(768, seed=69)
    dpool = rnd(B, tp, 768, seed=59)

    def run(new, rd):
        out = []
        for f16, dt in ((0, BF16), (1, F16)):
            cols = torch.empty(B * 12 * tp, 256, dtype=dt, device=DEV)
            if new: call("sed_im2col_rows", mel, cols, rd, 12, B, T, tstart, tp, f16)
            else: call("sed_im2col", mel, cols, B, T, tstart, tp, f16)
            out.append(cols)
        x = torch.empty(B, N, 768, device=DEV)
        if new: call("sed_assemble_tokens_rows", conv, cls, dist, npe, fpe, tpe, rd, 12, toffset, x, B, tp)
        else: call("sed_assemble_tokens", conv, cls, dist, npe, fpe, tpe, toffset, x, B, tp)
        dconv = torch.empty(B * 12 * tp, 768, dtype=BF16, device=DEV)
        tabs = [z(768), z(768), z(2, 768), z(768, 12), z(768, 99)]
        if new: call("sed_assemble_tokens_rows_bwd", dx, dconv, *tabs, rd, 12, toffset, B, tp)
        else: call("sed_assemble_tokens_bwd", dx, dconv, *tabs, toffset, B, tp)
        pooled = torch.empty(B, tp, 768, device=DEV); pm = z(B * N); pr = z(B * N)
        if new: call("sed_fpool_rows_fwd", x, g, b, 1e-5, pooled, pm, pr, B, tp, 12)
        else: call("sed_fpool_fwd", x, g, b, 1e-5, pooled, pm, pr, B, tp)
        dtok = torch.empty(B, N, 768, device=DEV); dxa = z(B, N, 768)
        if new: call("sed_fpool_rows_bwd", dpool, x, pm, pr, g, dtok, dxa, None, None, B, tp, 12)
        else: call("sed_fpool_bwd", dpool, x, pm, pr, g, dtok, dxa, None, None, B, tp)
        # (exact outputs only: the table sums of the assembly backward and dgamma / dbeta go through float atomics, whose order is
        #  not fixed from launch to launch -- those are checked against torch above)
        return out + [x, dconv, pooled, pm, pr, dtok, dxa]

    old = run(False, None)
    for rd in (dev_rows(list(range(12))), None):
        for i, (a, c) in enumerate(zip(old, run(True, rd))):
            assert torch.equal(a, c), (i, rd is None)


def test_row_entry_points_refuse_bad_counts():
    from transformer4sed_amd._lib import SedHipError
    mel = rnd(1, 128, T, seed=50)
    cols = torch.empty(12 * 99, 256, dtype=BF16, device=DEV)
    x = torch.empty(1, 2 + 12 * 99, 768, device=DEV)
    for F_ in (0, 13, -1):
        with pytest.raises(SedHipError, match="bad argument"):
            call("sed_im2col_rows", mel, cols, None, F_, 1, T, 0, 99, 0)
        with pytest.raises(SedHipError, match="bad argument"):
            call("sed_fpool_rows_fwd", x, x, x, 1e-5, x, None, None, 1, 99, F_)
        with pytest.raises(SedHipError, match="bad argument"):
            call("sed_assemble_tokens_rows_bwd", x, cols, None, None, None, None, None, None, F_, 0, 1, 99)
    with pytest.raises(SedHipError, match="bad argument"):
        call("sed_im2col_rows", mel, cols, None, 12, 1, T, 20, 99, 0)          # the slab would run past the clip
    with pytest.raises(SedHipError, match="bad argument"):
        call("sed_assemble_tokens_rows", x, x, x, x, x, x, None, 12, 1, x, 1, 99)      # toffset + tp > 99


@pytest.mark.parametrize("DT", [BF16, F16])
@pytest.mark.parametrize("B,N", [(2, 794), (2, 402), (1, 52), (1, 101), (1, 1091)])
def test_mhsa_at_the_patched_out_lengths(B, N, DT):
    """tests/test_gpu_kernels.py::test_mhsa_fwd_bwd at N = 2 + F tp for (F, tp) = (8, 99), (8, 50), (1, 50), (1, 99), (11, 99)."""
    Hh = 12
    f16 = 1 if DT == F16 else 0
    Npad = pad64(N)
    r16 = lambda t: t.to(BF16).float()
    q, k, v = [r16(rnd(B * Hh, N, 64, scale=1.3, seed=20 + i)) for i in range(3)]
    O = torch.empty(B, N, 768, dtype=DT, device=DEV)
    lse = torch.empty(B * Hh, N, device=DEV)
    call("sed_mhsa_fwd", q.to(DT), k.to(DT), v.to(DT), O, lse, B, Hh, N, Npad, f16)
    qq, kk, vv = [t.clone().requires_grad_(True) for t in (q, k, v)]
    s = (qq @ kk.transpose(1, 2)) * 0.125
    o = torch.softmax(s, dim=-1) @ vv
    oref = o.view(B, Hh, N, 64).permute(0, 2, 1, 3).reshape(B, N, 768)
    e = maxerr(O.float(), oref); report(f"mhsa fwd N={N} {DT}", e); assert e < (4e-3 if f16 else 2e-2)
    assert maxerr(lse, torch.logsumexp(s, dim=-1) / math.log(2.0)) < 2e-3
    dO = r16(rnd(B, N, 768, seed=33))
    oref.backward(dO)
    dqkv = torch.empty(B * N, 2304, dtype=BF16, device=DEV)
    Dt = torch.empty(B * Hh, N, device=DEV)
    call("sed_mhsa_bwd", q.to(DT), k.to(DT), v.to(DT), O, dO.to(BF16), lse, Dt, None, dqkv, B, Hh, N, Npad, f16, f16)
    g = dqkv.float().view(B, N, 3, Hh, 64).permute(2, 0, 3, 1, 4).reshape(3, B * Hh, N, 64)
    for i, (ref, nm) in enumerate(((qq.grad, "dq"), (kk.grad, "dk"), (vv.grad, "dv"))):
        e = maxerr(g[i], ref); sc = float(ref.abs().max()); report(f"mhsa bwd {nm} N={N} {DT}", e, f"scale={sc:.3e}")
        assert e < 0.03 * sc + 5e-3


# ------------------------------------------------------------------------------------------------ model level
def build_model(mlm=False, s=4, decoder="transformerXL"):
    kw = dict(mlm_dict=dict(strategy="block", block_width=10, mask_rate=0.75, out_dim=768)) if mlm else {}
    layers = 3 if decoder == "transformerXL" else 2
    net = PaSST_SED(passt_feature_layer=2, f_pool="mean_pool", decode_ratio=10, at_adapter=True, decoder=decoder, decoder_layer_num=layers,
                    decoder_pos_emd_len=1000, mlm=mlm, load_pretrained_model=False, encoder_depth=2, s_patchout_f=s, **kw)
    if decoder == "conformer":
        sd = synth.conformer_state_dict_np(tag="wc768", dec_layers=2, depth=12, mlm=mlm)
    else:
        sd = synth.matsed_state_dict_np(tag="w768", depth=12, mlm=mlm)
    own = net.state_dict()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items() if k in own}, strict=True)
    return net.to(DEV)


def grad_tol(name, base):
    """tests/test_gpu_model.py `_grad_tol`, unchanged."""
    if "pos_bias_u" in name:
        return 0.1
    if "pos_bias_v" in name or "linear_pos" in name:
        return 1e-2
    return base


def _mel(tag=TAG, B=2):
    return torch.from_numpy(synth.det_uniform(f"{tag}/mel", (B, 128, 1000), -1.2, 1.2)).to(DEV)


def _check_grad_norms(what, net, names, norms):
    params = dict(net.named_parameters())
    got_names = {n for n, p in params.items() if p.grad is not None}
    assert got_names == set(names), (got_names ^ set(names))
    worst, fails = 0.0, []
    for n, norm in zip(names, norms):
        r = abs(float(params[n].grad.double().norm()) - norm) / (norm + 1e-12)
        report(f"{what} grad {n}", r)
        worst = max(worst, r)
        if not r < grad_tol(n, 3e-3):
            fails.append((n, r))
    report(f"{what} worst grad-norm rel err", worst)
    assert not fails, fails


def test_patchout_model_vs_reference_golden(golden):
    """Training-mode outputs, loss and every gradient against the reference's, the fixture's kept rows injected."""
    g = golden(TAG)
    assert float(g["strong_vs_full_max"]) >= 20e-3 and float(g["strong_vs_first_rows_max"]) >= 20e-3
    rows = g["rows_global"].tolist()
    mel = _mel()
    net = build_model()
    net.train()
    net._patchout_rows = [rows]
    strong, weak, other = net(mel, encoder_win=False, temp_w=1)
    for nm, got in (("strong", strong), ("weak", weak), ("at_out", other["at_out"])):
        e = maxerr(got, g[nm]); report(f"{TAG} {nm} vs reference", e)
        assert e < 1e-3, (nm, e)          # measured: strong 6.3e-4, weak 3.6e-4, at_out 1.9e-4
    e = maxerr(other["frame_before_mask"][:, ::25, ::16], g["interp_s"]); report(f"{TAG} interp_s", e); assert e < 2e-2
    gs = torch.from_numpy(synth.det_uniform(f"{TAG}/gs", tuple(strong.shape))).to(DEV)
    gw = torch.from_numpy(synth.det_uniform(f"{TAG}/gw", tuple(weak.shape))).to(DEV)
    ga = torch.from_numpy(synth.det_uniform(f"{TAG}/ga", tuple(other["at_out"].shape))).to(DEV)
    loss = (strong * gs).sum() + (weak * gw).sum() + (other["at_out"] * ga).sum()
    loss.backward()
    rel = abs(float(loss.detach()) - float(g["ft_loss"])) / abs(float(g["ft_loss"])); report(f"{TAG} loss rel", rel)
    assert rel < 2e-3          # measured: 8.1e-4; worst of the 89 gradient norms below: 1.1e-3
    _check_grad_norms(TAG, net, [str(n) for n in g["ft_grad_names"]], g["ft_grad_norms"])
    dfreq = net.backbone.freq_new_pos_embed.grad.detach().reshape(768, 12).cpu()
    dropped = [r for r in range(12) if r not in rows]
    assert float(dfreq[:, dropped].abs().max()) == 0
    ref = torch.from_numpy(g["ft_dfreq"])
    for r in rows:          # the kept columns, one by one, by the gradient-norm measure of `_check_grad_norms` and its bound
        got_c, ref_c = dfreq[:, r].double(), ref[:, r].double()
        rel = abs(float(got_c.norm()) - float(ref_c.norm())) / float(ref_c.norm())
        # (reported only: the norm of the difference, which also sees the element-wise rounding of the bf16 gradient operands that the
        #  norm averages out -- a chain of ~8 roundings of 2^-9 / sqrt(3) each plus the f16 forward; measured 5.3e-3 - 5.5e-3 on all eight columns, the norm measure 1.1e-4 - 3.4e-4)
        report(f"{TAG} dfreq column {r} norm rel", rel, f"difference norm rel {float((got_c - ref_c).norm() / ref_c.norm()):.3e}")
        assert rel < 3e-3, (r, rel)


def test_patchout_model_mlm_vs_reference_golden(golden):
    g = golden(TAG)
    mel = _mel()
    net = build_model(mlm=True)
    net.train()
    for p in net.backbone.parameters():
        p.requires_grad_(False)
    net._patchout_rows = [g["mlm_rows"].tolist()]
    net._mlm_draws = dict(noise=torch.from_numpy(g["mlm_noise"]), probs=torch.from_numpy(g["mlm_probs"]), rand_idx=torch.from_numpy(g["mlm_rand_idx"]))
    pred, other = net(mel, encoder_win=False)
    assert np.array_equal(other["mask_id_seq"].cpu().numpy(), g["mlm_mask_ids"])
    S = lambda t: t[:, ::25, ::16]
    e = maxerr(S(pred), g["mlm_pred_s"]); sc = float(np.abs(g["mlm_pred_s"]).max()); report(f"{TAG} mlm pred", e, f"scale={sc:.2f}")
    assert e < 1e-3 * sc          # measured: 2.2e-3 on values up to 2.91 (7.5e-4 of scale); loss 1.6e-5; worst gradient norm 1.7e-3
    loss = torch.nn.functional.mse_loss(other["frame_before_mask"][other["mask_id_seq"]], pred[other["mask_id_seq"]])
    rel = abs(float(loss.detach()) - float(g["mlm_loss"])) / float(g["mlm_loss"]); report(f"{TAG} mlm loss rel", rel)
    assert rel < 1e-4
    loss.backward()
    _check_grad_norms(f"{TAG} mlm", net, [str(n) for n in g["mlm_grad_names"]], g["mlm_grad_norms"])


def test_patchout_windows_vs_reference_golden(golden):
    """The teacher's form: training mode under no_grad, 11 sliding windows, each with its own rows and time offset."""
    g = golden(TAG)
    net = build_model()
    net.train()
    net._patchout_rows = [g["rows_global"].tolist()] + g["win_rows"].tolist()
    net._win_toffsets = g["win_toffsets"].tolist()
    with torch.no_grad():
        strong, weak, other = net(_mel(), encoder_win=True, mix_rate=0.5, win_param=[512, 49], temp_w=1)
    for nm, got in (("win_strong", strong), ("win_weak", weak), ("win_at_out", other["at_out"])):
        e = maxerr(got, g[nm]); report(f"{TAG} {nm} vs reference", e)
        assert e < 1e-3, (nm, e)          # measured: win_strong 4.3e-4, win_weak 2.8e-4, win_at_out 1.7e-4


def test_eval_mode_drops_nothing():
    mel = _mel("patchout/eval")
    a, b = build_model(s=4), build_model(s=0)
    a.eval(); b.eval()
    state = torch.get_rng_state()
    with torch.no_grad():
        sa, wa, oa = a(mel, encoder_win=False)
        sb, wb, ob = b(mel, encoder_win=False)
    assert torch.equal(state, torch.get_rng_state())
    assert torch.equal(sa, sb) and torch.equal(wa, wb) and torch.equal(oa["at_out"], ob["at_out"])
    a.train()
    a._patchout_rows = [[0, 3, 4, 5, 6, 7, 9, 11]]
    with torch.no_grad():
        st, _, _ = a(mel, encoder_win=False)
    assert float((st - sa).abs().max()) > 20e-3          # and training mode does drop


def test_engine_refuses_malformed_row_sets():
    """`SedEngine.forward(rows=...)` checks the sets on the host before the upload: the kernels index mel rows and tables with them."""
    net = build_model()
    net.train()
    eng = net._make_engine()
    mel = _mel("patchout/eval")
    good = [0, 3, 4, 5, 6, 7, 9, 11]
    for bad in ([good, good], [[0, 3, 4, 5, 6, 7, 9, 12]], [[3, 0, 4, 5, 6, 7, 9, 11]], [[-1, 3, 4, 5, 6, 7, 9, 11]], [[0, 0, 4, 5, 6, 7, 9, 11]]):
        with pytest.raises(ValueError, match="rows"):
            eng.forward(mel, rows=bad)
    with pytest.raises(ValueError, match="rows"):          # windows without their sets
        eng.forward(mel, encoder_win=True, rows=[good])


def test_trainer_two_steps_vs_reference_trainer(golden):
    """`_check_trainer_steps` of tests/test_gpu_model.py for a patched-out student and a patched-out windowed teacher: two steps of
    MatSedTrainer.finetune_step against the reference's Trainer.train under the fixture's seeds.  Nothing is injected, so the row
    sets are the reference's only if every draw of the step comes in the reference's order."""
    from transformer4sed_amd.scheduler import ExponentialDown
    from transformer4sed_amd.trainer import FusedAdamWEMA, MatSedTrainer, get_params
    g = golden(STEP_TAG)
    meta = json.loads(str(g["config_json"]))
    cfg, sc = meta["cfg"], meta["sched"]
    net = build_model(s=int(g["s_patchout_f"]))
    ema_net = deepcopy(net)
    assert ema_net.backbone.s_patchout_f == 4
    for p in ema_net.parameters():
        p.detach_()
    opt = FusedAdamWEMA(net, get_params(net, cfg["opt"]["param_groups"]), ema_net=ema_net, betas=(0.9, 0.999), eps=1e-8)
    sched = ExponentialDown(opt, start_iter=sc["n_epochs_cut"] * sc["epoch_len"], total_iter=sc["n_epochs"] * sc["epoch_len"],
                            exponent=sc["exponent"], warmup_iter=sc["warmup_epochs"] * sc["epoch_len"], warmup_rate=sc["warmup_rate"])
    net.train(); ema_net.train()
    tr = MatSedTrainer(net, ema_net, opt, sched, cfg, epoch_len=1)
    random.seed(meta["seeds"][0]); np.random.seed(meta["seeds"][1]); torch.manual_seed(meta["seeds"][2])
    names = [str(n) for n in g["probe_names"]]
    for step in range(int(g["n_steps"])):
        wav = torch.from_numpy(synth.synth_wav(sum(meta["groups"]), seed=meta["wav_seed0"] + step)).to(DEV)
        labels = torch.from_numpy(synth.synth_batch_labels(*meta["groups"], seed=meta["label_seed0"] + step)).to(DEV)
        out = tr.finetune_step(wav, labels)
        for k in ("loss_total", "loss_class_strong", "loss_class_weak", "loss_class_at_specific", "loss_cons_strong",
                  "loss_cons_weak", "loss_cons_at_specific"):
            ref, got = float(g[f"s{step}_{k}"]), float(out[k])
            report(f"patchout trainer step {step} {k}", abs(got - ref), f"ref {ref:.6f}")
            assert abs(got - ref) <= 3e-3 * max(abs(ref), 0.05), (step, k, got, ref)          # measured: <= 4.4e-4 on terms up to 4.0
        assert abs(float(out["w_cons"]) - float(g[f"s{step}_w_cons"])) < 1e-9
        assert abs(sched._get_scale() - float(g[f"s{step}_lr_scaler"])) < 1e-12
        np.testing.assert_allclose([x["lr"] for x in opt.param_groups], g[f"s{step}_lrs"], rtol=1e-12)
        sp, ep = dict(net.named_parameters()), dict(ema_net.named_parameters())
        lr = max(x["lr"] for x in opt.param_groups)
        worst = 0.0
        for i, n in enumerate(names):
            ms = float(np.abs(sp[n].detach().reshape(-1)[:512].cpu().numpy() - g[f"s{step}_stu{i}"]).mean()) / lr
            me = float(np.abs(ep[n].detach().reshape(-1)[:512].cpu().numpy() - g[f"s{step}_ema{i}"]).mean()) / lr
            worst = max(worst, ms, me)
            assert ms < 0.1 and me < 0.1, (step, n, ms, me)
        report(f"patchout trainer step {step} worst probe mean|dp|/lr", worst)


def test_conformer_student_trains_with_patchout():
    import bench
    from transformer4sed_amd.scheduler import ExponentialDown
    from transformer4sed_amd.trainer import FusedAdamWEMA, MatSedTrainer, get_params
    net = build_model(decoder="conformer")
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
    before = {n: p.detach().clone() for n, p in net.named_parameters() if n in dec}
    out = tr.finetune_step(wav, labels.clone())
    assert all(np.isfinite(float(v)) for k, v in out.items() if k.startswith("loss_"))
    after = dict(net.named_parameters())
    assert len(dec) == 66
    for n in dec:
        assert not torch.equal(before[n], after[n].detach()), f"{n} did not move"
