"""The kernels of csrc/conformer.hip and csrc/fdy_cnn.hip past one pass of their grid (need an MI355X): the Conformer depthwise-conv
backward with a multi-step tile walk, the FDY head backward at its 32-slab cap, the frequency mean at widths that leave threads idle,
the mixing forward and the mean's backward past 16 384 workgroups, Swish' and scale-add past 65 536, and the depth-2 Conformer model at
B = 8 against the float64 sum of four pair runs.  Cases, references and the restated launch arithmetic: tests/walk_cases.py, proved on
the CPU by tests/test_walk_cases_cpu.py.

The bound is the one of tests/test_gpu_conformer.py / tests/test_gpu_fdy_cnn.py, per element:
|got - ref64| <= 8 max|ref32 - ref64| + half an ulp of the output's storage format.  Every output buffer is NaN before the call.  Errors,
yardsticks, worst error / bound and the drop ratios go to walk_kernel_errors.log under SED_TEST_LOG_DIR, else test_logs/."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import fdy_cases as FC  # noqa: E402
import walk_cases as X  # noqa: E402
from walk_cases import C, F32, F64  # noqa: E402
from transformer4sed_amd import synth  # noqa: E402
from transformer4sed_amd._lib import SedHipError  # noqa: E402
from transformer4sed_amd.ops import call, BF16, F16  # noqa: E402
from test_gpu_conformer import build_model, on_dev, run_fwd  # noqa: E402

DEV = "cuda"
LOGDIR = os.environ.get("SED_TEST_LOG_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_logs")
LOG = os.path.join(LOGDIR, "walk_kernel_errors.log")
NAN = float("nan")
GRAD_REL = 1e-3         # tests/test_gpu_batch_scale.py


def log(line):
    os.makedirs(LOGDIR, exist_ok=True)
    with open(LOG, "a") as f:
        f.write(line + "\n")
    print(line)


def check(name, got, ref64, ref32, storage="f32"):
    """Logs and asserts, per element,  |got - ref64| <= 8 max|ref32 - ref64| + half_ulp(storage) at |ref64|; a NaN left of the prefill
    fails (NaN <= tol is false)."""
    err, yard, worst, ok, mag = X.judge(got, ref64, ref32, storage)
    log(f"{name}: max_abs_err={err:.4e} yardstick_f32_vs_f64={yard:.4e} magnitude={mag:.3e} storage={storage} worst_err_over_bound={worst:.3f}")
    assert ok and not bool(torch.isnan(got).any()), (name, err, yard, worst)


def nans(*shape, dtype=F32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


# ================================================================================================ 1. Conformer backward, multi-step walk
def conv_bwd(t, B, T, conv, mean, rstd, partial_floats=None):
    """`run_bwd` of tests/test_gpu_conformer.py with dx NaN before the call and the partials' size open to the caller."""
    dx = nans(B * T, 2 * C, dtype=BF16)
    dw, db, dg, dbt = (torch.zeros(C, X.KW, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV))
    part = nans(X.conv_partial_floats(B, T))
    call("sed_conv_glu_dw_bwd", t["dy"], t["x"], conv, mean, rstd, t["w"], t["gamma"], t["beta"], dx, dw, db, dg, dbt, part,
         part.numel() if partial_floats is None else partial_floats, B, T, C)
    return dx, dw, db, dg, dbt


@pytest.mark.parametrize("B,T", X.CONV_WALK_SHAPES)
def test_conv_glu_dw_walk_vs_float64(B, T):
    """357 tiles on 256 workgroups (two steps for workgroups 0-100; workgroup 50 walks a ragged tile of clip 0, then clip 6) and 540
    tiles (three steps for workgroups 0-27, every clip ending in a ragged tile).
    Measured on an MI355X, worst error / bound over both shapes: y 0.14, conv 0.125, mean 0.13, rstd 0.16; dx 0.999 (the bf16 rounding),
    dw 0.33, dbias 0.18, dgamma 0.17, dbeta 0.19; a tile left out moves the float64 sums by 6.5e3 .. 2.5e4 bounds."""
    ntiles, nwg, steps = X.conv_walk(B, T)
    assert steps >= 2 and nwg == 256
    r64, r32 = X.reference(B, T)
    t = on_dev(X.inputs(B, T))
    M = B * T
    y16, y32, conv, mean, rstd = nans(M, 3 * C, dtype=F16), nans(M, C), nans(M, C), nans(M), nans(M)
    call("sed_conv_glu_dw_fwd", t["x"], t["w"], t["b"], t["gamma"], t["beta"], 1e-5, y16, y32, conv, mean, rstd, B, T, C, 4)
    tag = f"walk fwd B={B} T={T}"
    check(f"{tag} y (fp32)", y32, r64["y"], r32["y"])
    check(f"{tag} conv (fp32)", conv, r64["c"], r32["c"])
    check(f"{tag} mean", mean, r64["mean"], r32["mean"])
    check(f"{tag} rstd", rstd, r64["rstd"], r32["rstd"])
    hi = y32.to(F16)
    assert torch.equal(y16[:, :C], hi) and torch.equal(y16[:, 2 * C:], hi)
    assert torch.equal(y16[:, C:2 * C], (y32 - hi.float()).to(F16))
    dx, dw, db, dg, dbt = conv_bwd(t, B, T, conv, mean, rstd)
    tag = f"walk bwd B={B} T={T} ({ntiles} tiles, {steps} steps)"
    check(f"{tag} dx (bf16)", dx.float(), r64["dx"], r32["dx"], "bf16")
    check(f"{tag} dw", dw, r64["dw"], r32["dw"])
    check(f"{tag} dbias", db, r64["db"], r32["db"])
    check(f"{tag} dgamma", dg, r64["dgamma"], r32["dgamma"])
    check(f"{tag} dbeta", dbt, r64["dbeta"], r32["dbeta"])
    # the bound sees every walked tile: the float64 sums without the frames of one tile lie >= 10 bounds away
    for (nm, k), ratio in X.conv_drop_ratios(B, T).items():
        log(f"{tag} {k} without the {nm}: reference moves by {ratio:.3e} bounds")
        assert ratio >= X.SENS, (nm, k, ratio)
    again = conv_bwd(t, B, T, conv, mean, rstd)
    for nm, a, b in zip(("dx", "dw", "dbias", "dgamma", "dbeta"), (dx, dw, db, dg, dbt), again):
        assert torch.equal(a, b), (tag, nm)


def test_conv_glu_dw_walk_clip_isolation():
    """(7, 1010): clip 6 shares workgroups 50-100 with clips 0-1 (their second step).  Replacing its input and incoming gradient changes
    no bit of clips 0-5, forward and backward (test_conv_glu_dw_clip_isolation with an LDS slab reused across clips)."""
    B, T = 7, 1010
    t = on_dev(X.inputs(B, T))
    y16, y32, conv, mean, rstd = run_fwd(t, B, T)
    dx = conv_bwd(t, B, T, conv, mean, rstd)[0]
    t2 = dict(t, x=t["x"].clone(), dy=t["dy"].clone())
    last, prev = slice(6 * T, 7 * T), slice(5 * T, 6 * T)
    t2["x"][last] = 3.0 * t["x"][prev].flip(0)
    t2["dy"][last] = -t["dy"][prev].flip(0)
    z16, z32, conv2, mean2, rstd2 = run_fwd(t2, B, T)
    dz = conv_bwd(t2, B, T, conv2, mean2, rstd2)[0]
    keep = slice(0, 6 * T)
    for a, b in ((y16, z16), (y32, z32), (conv, conv2), (mean, mean2), (rstd, rstd2), (dx, dz)):
        assert torch.equal(a[keep], b[keep])
    assert not torch.equal(y32[last], z32[last]) and not torch.equal(dx[last], dz[last])


def test_conv_glu_dw_walk_refuses_short_partials():
    """One float short of nwg 34 768: refused before any launch, dx untouched."""
    B, T = 7, 1010
    t = on_dev(X.inputs(B, T))
    _, _, conv, mean, rstd = run_fwd(t, B, T)
    need = X.conv_partial_floats(B, T)
    assert need == 256 * 34 * 768 and not X.conv_args_ok(B, T, C, need - 1)
    dx = nans(B * T, 2 * C, dtype=BF16)
    g = [torch.zeros(C, X.KW, device=DEV)] + [torch.zeros(C, device=DEV) for _ in range(3)]
    with pytest.raises(SedHipError, match="bad argument"):
        call("sed_conv_glu_dw_bwd", t["dy"], t["x"], conv, mean, rstd, t["w"], t["gamma"], t["beta"], dx, *g, nans(need), need - 1, B, T, C)
    assert bool(torch.isnan(dx).all()) and all(float(v.abs().max()) == 0.0 for v in g)


# ================================================================================================ 2. FDY head backward at the slab cap
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("B,H,W,cin", X.HEAD_WALK_CASES)
def test_attention_head_at_the_slab_cap(B, H, W, cin, train):
    """The sequence of test_frequency_mean_and_attention_head (tests/test_gpu_fdy_cnn.py) at R >= 4224: dW1 is reduced over 32 slabs whose
    edges fall inside clips, the last one short.  Measured: att 0.10, dX 0.12, the five gradients 0.06 .. 0.19 of the bound, the same
    after the second call; the last slab's rows move the float64 gradients by 3.6e4 .. 1.8e5 bounds."""
    temperature = X.HEAD_WALK_T
    inp, r64, r32 = X.head_case(B, H, W, cin, train)
    hid, R, Cp = FC.hid_of(cin), B * H, max(64, cin)
    nslab, rows_per = X.fdy_slabs(R)
    assert nslab == 32 and R // 128 > 32
    name = f"head walk B{B} H{H} W{W} cin{cin} {'train' if train else 'eval'} ({nslab} slabs of {rows_per})"
    d = {k: v.to(DEV).contiguous() for k, v in inp.items()}
    for dt16 in (F16, BF16):
        Xd = nans(B, H, W, Cp, dtype=dt16); Xd[..., :cin] = d["x"].to(dt16)
        assert torch.equal(Xd[..., :cin].float(), d["x"]), "the activation is exact in its 16-bit format"
        pm = nans(R, cin)
        call("sed_fdy_freq_mean", Xd, 1 if dt16 == F16 else 0, pm, R, W, cin, Cp)
        check(name + f" pm ({'f16' if dt16 == F16 else 'bf16'} input)", pm, r64["pm"], r32["pm"])
    u, aff, att = torch.empty(R, hid, device=DEV), torch.empty(3, hid, device=DEV), nans(R, 4)
    part = torch.empty((R + 15) // 16 * 2 * hid, dtype=F64, device=DEV) if train else None
    rm, rv = d["bn_rm"].clone(), d["bn_rv"].clone()
    call("sed_fdy_attn_taps", pm, d["c1w"], u, part, B, H, cin, hid)
    call("sed_fdy_attn_softmax", u, part, d["bn_w"], d["bn_b"], rm, rv, d["c2w"], d["c2b"], float(temperature), 0.1, 1e-5, aff, att, R, hid)
    check(name + " att", att, r64["att"], r32["att"])
    assert float(att.min()) < 0.2 and float(att.max()) > 0.3, "the case exercises the softmax"
    if train:      # torch's rule: momentum 0.1, unbiased variance (bounds of test_frequency_mean_and_attention_head)
        want_m = 0.9 * inp["bn_rm"].double() + 0.1 * r64["mean"]
        want_v = 0.9 * inp["bn_rv"].double() + 0.1 * r64["var"] * R / (R - 1)
        log(f"{name} running statistics: mean err {X.maxerr(rm, want_m):.3e} var err {X.maxerr(rv, want_v):.3e}")
        assert X.maxerr(rm, want_m) < 1e-6 and X.maxerr(rv, want_v) < 1e-5
    else:
        assert torch.equal(rm, d["bn_rm"]) and torch.equal(rv, d["bn_rv"])
    # backward
    P6 = 6 * hid + 4
    need = X.head_ws_floats(R, cin, hid)
    ws = torch.empty(need, device=DEV)
    bpart = torch.empty((R + 15) // 16 * P6, dtype=F64, device=DEV)
    dz, dpm = torch.empty(R, hid, device=DEV), nans(R, cin)
    g = {k: torch.zeros_like(d[k]) for k in X.HEAD_GRADS}

    def bwd(dpm_, views, ws_floats=need):
        call("sed_fdy_attn_bwd", d["da"], att, u, aff, pm, d["c1w"], d["bn_b"], d["c2w"], float(temperature), 1 if train else 0, dz, bpart, ws, ws_floats,
             dpm_, *views, B, H, cin, hid)

    views = (g["c1w"], g["bn_w"], g["bn_b"], g["c2w"], g["c2b"])
    with pytest.raises(SedHipError, match="bad argument"):      # one float short of the 32-slab workspace
        bwd(dpm, views, need - 1)
    assert bool(torch.isnan(dpm).all()) and all(float(v.abs().max()) == 0.0 for v in views)
    bwd(dpm, views)
    dX = d["dx0"].clone()
    call("sed_fdy_mean_bwd_add", dX, dpm, R, W, cin)
    check(name + " dX", dX, r64["dX"], r32["dX"])
    for k in g:
        check(name + " grad " + k, g[k], r64["g_" + k], r32["g_" + k])
    if not train:      # rows are independent: the reference without the last slab's rows lies >= 10 bounds away, for every gradient
        for k, ratio in X.head_drop_ratios(B, H, W, cin).items():
            log(f"{name} grad {k} without the last slab's rows: reference moves by {ratio:.3e} bounds")
            assert ratio >= X.SENS, (k, ratio)
    # a second backward accumulates on top of what the gradient views hold, in the same order: exactly twice
    bwd(dpm, views)
    for k in g:
        check(name + " grad " + k + " accumulated", g[k], 2 * r64["g_" + k], 2 * r32["g_" + k])
    # frozen parameters: null gradient views
    dpm2 = nans(R, cin)
    bwd(dpm2, (None,) * 5)
    assert torch.equal(dpm, dpm2)


# ================================================================================================ 3. frequency mean, idle threads
@pytest.mark.parametrize("c", X.FREQ_CASES, ids=lambda c: f"C{c.C}-W{c.W}")
def test_freq_mean_at_widths_that_do_not_divide_256(c):
    nv, wl, idle = X.freq_mean_map(c.C)
    x = X.freq_inputs(c)
    r64, r32 = X.freq_refs(x)
    for dt16 in (F16, BF16):
        Xd = nans(c.R, c.W, c.Cp, dtype=dt16); Xd[..., :c.C] = x.to(DEV).to(dt16)
        assert torch.equal(Xd[..., :c.C].float().cpu(), x) and bool(torch.isnan(Xd[..., c.C:]).all())
        pm = nans(c.R, c.C)
        call("sed_fdy_freq_mean", Xd, 1 if dt16 == F16 else 0, pm, c.R, c.W, c.C, c.Cp)
        check(f"freq mean C{c.C} W{c.W} (nv {nv}, wl {wl}, {idle} idle) {'f16' if dt16 == F16 else 'bf16'} input", pm, r64, r32)


# ================================================================================================ 4. mixing forward past the grid cap
@pytest.mark.parametrize("c", X.MIX_WALK_CASES, ids=lambda c: f"B{c.B}-H{c.H}")
def test_mix_forward_past_the_grid_cap(c):
    M = c.B * c.H * c.W
    work = X.mix_items(M, c.ldy)
    blocks, first, passes = X.fdy_grid_items(work)
    assert blocks == X.FDY_CAP and passes >= 2
    Y4, A = X.mix_walk_inputs(c, DEV)
    assert Y4.shape == (M, c.ld4)
    Y = nans(M, c.ldy)
    call("sed_fdy_mix_fwd", Y4, c.ld4, A, Y, c.ldy, M, c.W, c.co)
    y4, att = Y4.cpu(), A.cpu()
    r64, r32 = X.mix_direct(y4, att, c.W, c.co, F64), X.mix_direct(y4, att, c.W, c.co, F32)
    name = f"mix walk B{c.B} H{c.H} W{c.W} co{c.co} ({work} items, {work - first} past the first pass, {passes} passes)"
    check(name + " fwd Y", Y[:, :c.co], r64, r32)
    assert float(Y[:, c.co:].abs().max()) == 0.0, "padding columns come back exactly zero"
    late = float(r64[X.mix_late_rows(c):].abs().max()) / X.bound32(r64, r32)
    log(f"{name}: max|ref| past the first pass = {late:.3e} bounds")
    assert late >= X.SENS


# ================================================================================================ 5. mean backward past the grid cap
@pytest.mark.parametrize("c", X.MEAN_WALK_CASES, ids=lambda c: f"W{c.W}")
def test_mean_bwd_add_past_the_grid_cap(c):
    dx0, dpm = X.mean_walk_inputs(c, DEV)
    work = X.mean_add_items(c.R, c.W, c.C)
    passes = X.fdy_grid_items(work)[2]
    dX = dx0.clone()
    call("sed_fdy_mean_bwd_add", dX, dpm, c.R, c.W, c.C)
    name = f"mean add walk R{c.R} W{c.W} C{c.C} ({work} items, {passes} passes)"
    if c.exact:      # dpm / W is exact: one rounding, whichever way the sum is computed
        assert passes == 2
        want = dx0 + dpm.unsqueeze(1) / c.W
        assert torch.equal(dX, want), name
        assert not torch.equal(dX[-1], dx0[-1]), "the last row, in the second pass, moved"
        log(f"{name}: bit-equal to dX0 + dpm / {c.W} in fp32")
    else:
        h0, hp = dx0.cpu(), dpm.cpu()
        check(name + " dX", dX, X.mean_add_direct(h0, hp, c.W, F64), X.mean_add_direct(h0, hp, c.W, F32))


# ================================================================================================ 6. Swish', scale-add past 65 536 blocks
def test_swish_bwd_and_scale_add_past_65536_blocks():
    n = X.ELEM_N
    free = torch.cuda.mem_get_info()[0]
    if free < 4 * 2 ** 30:
        pytest.skip(f"needs 4 GiB of free device memory for five {n}-element buffers, {free / 2 ** 30:.1f} GiB free")
    blocks, first, passes = X.elem_blocks(n)
    assert blocks == 65536 and passes == 2
    g = torch.Generator(device=DEV).manual_seed(4300)
    h = 2.0 * torch.randn(n, generator=g, device=DEV)
    dy = torch.rand(n, generator=g, device=DEV) * 2.0 - 1.0
    dh = nans(n, dtype=BF16)
    call("sed_swish_bwd", dy, h, dh, n)
    assert not bool(torch.isnan(dh).any()), "every element written"
    for nm, w in zip(("start", "straddling the end of the first pass", "end"), X.elem_windows(n)):
        hh, dd = h[w].cpu(), dy[w].cpu()
        check(f"swish bwd walk n={n} window {nm} [{w.start}, {w.stop}) (bf16)", dh[w].float(), X.swish_bwd_direct(dd, hh, F64),
              X.swish_bwd_direct(dd, hh, F32), "bf16")
    out, out16 = nans(n), nans(n, dtype=BF16)
    call("sed_scale_add_f32", h, dy, out, out16, n, 0.5)
    assert torch.equal(out, dy + 0.5 * h) and torch.equal(out16, out.to(BF16))
    out.fill_(NAN)
    s = float(torch.tensor(768.0).sqrt())
    call("sed_scale_add_f32", h, None, out, None, n, s)
    assert torch.equal(out, h * s)
    log(f"scale add walk n={n}: both forms and the bf16 image bit-equal to torch on the device")


# ================================================================================================ 7. model level
def test_conformer_depth2_batch8_gradients_are_the_sum_of_pair_runs():
    """test_depth2_batch32_gradients_are_the_sum_of_pair_runs (tests/test_gpu_batch_scale.py) for decoder="conformer" at B = 8, T = 1000:
    each depthwise backward walks 400 tiles.  Per parameter the B = 8 gradient equals the float64 sum of the four B = 2 runs norm-wise
    within GRAD_REL of sum_k ||g_k||, the last pair's share of that sum is >= 3 GRAD_REL, posteriors within 2e-4 of the pair runs.
    Measured: worst ratio 6.5e-4 (decoder.blocks.1.self_attn.linear_pos.weight; transformerXL at B = 32: 3.1e-4), the depthwise
    backward's own tensors 2.0e-7 at most, smallest share of the last pair 0.19, posteriors bit-identical."""
    B, T = X.MODEL_B, X.MODEL_T
    assert X.conv_walk(B, T) == (400, 256, 2)
    tag = "walk_conformer_d2"
    mel = torch.from_numpy(synth.det_uniform(f"{tag}/mel", (B, 128, T), -1.2, 1.2)).to(DEV)
    net = build_model(False, None).train()
    ws = {}

    def run(lo, hi):
        net.zero_grad()
        net._last_grad_arena = None
        strong, weak, other = net(mel[lo:hi].contiguous(), encoder_win=False, temp_w=1)
        if not ws:
            for nm, t in (("gs", strong), ("gw", weak), ("ga", other["at_out"])):
                ws[nm] = torch.from_numpy(synth.det_uniform(f"{tag}/{nm}", (B,) + tuple(t.shape[1:]))).to(DEV)
        loss = (strong * ws["gs"][lo:hi]).sum() + (weak * ws["gw"][lo:hi]).sum() + (other["at_out"] * ws["ga"][lo:hi]).sum()
        loss.backward()
        grads = {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
        return (strong.detach().clone(), weak.detach().clone(), other["at_out"].detach().clone()), grads

    out8, g8 = run(0, B)
    assert any("conv_module.depthwise_conv.weight" in n for n in g8)
    gsum = {n: torch.zeros_like(g, dtype=F64) for n, g in g8.items()}
    gnorm = {n: 0.0 for n in g8}
    glast, worst_post = {}, 0.0
    for k in range(B // 2):
        outk, gk = run(2 * k, 2 * k + 2)
        for nm, a, b in zip(("strong", "weak", "at"), out8, outk):
            dd = float((a[2 * k:2 * k + 2] - b).abs().max())
            worst_post = max(worst_post, dd)
            assert dd < 2e-4, (nm, k, dd)
        assert set(gk) == set(g8)
        for n, g in gk.items():
            gsum[n] += g.double()
            gnorm[n] += float(g.double().norm())
        if k == B // 2 - 1:
            glast = {n: float(g.double().norm()) for n, g in gk.items()}
    rel = {n: float((g.double() - gsum[n]).norm()) / gnorm[n] for n, g in g8.items()}
    share = {n: glast[n] / gnorm[n] for n in g8}
    wn, sn = max(rel, key=rel.get), min(share, key=share.get)
    conv_names = [n for n in g8 if ".conv_module.depthwise_conv." in n or ".conv_module.norm." in n]
    wc = max(conv_names, key=rel.get)
    log(f"conformer B={B} depth2: worst posterior difference vs pair runs (strong, weak, AT) {worst_post:.3e}")
    log(f"conformer B={B} depth2: worst |g8 - sum g_pair| / sum |g_pair| = {rel[wn]:.3e} ({wn}); bound {GRAD_REL:g}; "
        f"transformerXL at B = 32 recorded 3.1e-4")
    log(f"conformer B={B} depth2: worst of the depthwise-conv backward's own sums = {rel[wc]:.3e} ({wc})")
    log(f"conformer B={B} depth2: smallest share of the last pair in sum |g_pair| = {share[sn]:.3e} ({sn})")
    for n in g8:
        assert rel[n] < GRAD_REL, (n, rel[n])
        assert share[n] >= 3 * GRAD_REL, (n, "the bound cannot see a dropped pair", share[n])
