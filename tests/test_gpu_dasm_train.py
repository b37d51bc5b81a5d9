"""Training kernels of the DASM / AudioSet-Strong path (csrc/dasm.hip, transformer4sed_amd/dasm.py) against torch fp32 / fp64 autograd on
the CPU: the general fp32 GEMM (all three products of a Linear, batched einsum forms, dropout epilogue), the cross / self attention
backward (mask, dropout with the kernels' own counter-based bits dumped through sed_dropout_f32 and held to their host restatement,
tests/dropout_cases.py), the dual-stream finish backward, the
supervised-loss kernel, the closed-set head for 407 classes, and the whole query decoder + head forward / backward against
oracle/dasm_oracle.py under autograd (weights, frame tokens, SED decoder output; with and without dropout)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dropout_cases  # noqa: E402
from transformer4sed_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32


def relerr(got, want):
    want = want.double()
    return float((got.cpu().double() - want).norm() / want.norm().clamp_min(1e-30))


def logerr(msg):
    """measured errors of the precision-relevant asserts -> gpurun_out/dasm_errors.log (margins of the split-precision attention products)"""
    os.makedirs("gpurun_out", exist_ok=True)
    with open("gpurun_out/dasm_errors.log", "a") as f:
        f.write(msg + "\n")


def keep_mask(n, p, seed, site):
    from transformer4sed_amd.ops import call
    m = torch.empty(n, dtype=torch.uint8, device=DEV)
    call("sed_dropout_f32", None, None, m, n, float(p), int(seed), int(site))
    m = m.cpu()
    # the dump equals the host restatement of the bit function (tests/dropout_cases.py): every consumer test below that injects this mask
    # into its oracle is thereby a test against an independent reference, not only of the consumers' agreement with each other
    assert torch.equal(m, torch.from_numpy(dropout_cases.dasm_keep(n, float(p), int(seed), int(site))))
    return m


def test_gemm_f32_all_forms_vs_torch():
    from transformer4sed_amd.ops import call
    g = torch.Generator().manual_seed(0)
    R = lambda *s: torch.randn(*s, generator=g)
    # dx = dy W  (transB) for ragged shapes, including a one-column head (N = 1) and K not a multiple of 4
    for M, N, K in ((20, 768, 768), (130, 1, 768), (257, 13, 70), (64, 3072, 768)):
        dy, W = R(M, N), R(N, K) / N ** 0.5
        out = torch.empty(M, K, device=DEV)
        call("sed_gemm_f32", dy.to(DEV), W.to(DEV), None, None, out, None, M, K, N, N, K, K, 0, 1, 1, 0, 0, 0, 0, 0, 1, 0.0, 0, 0)
        assert relerr(out, dy.double() @ W.double()) < 3e-6, (M, N, K)
    # dW += dy^T x  (transA + transB, accumulate, split over the tokens), on top of existing content
    for M, N, K, ks in ((20, 768, 768, 1), (13024, 768, 768, 8), (500, 1, 768, 3), (777, 130, 70, 4), (4000, 1536, 768, 5)):
        dy, x, base = R(M, N), R(M, K), R(N, K)
        gW = base.clone().to(DEV)
        call("sed_gemm_f32", dy.to(DEV), x.to(DEV), None, None, gW, None, N, K, M, N, K, K, 1, 1, 1, 0, 0, 0, 0, 1, ks, 0.0, 0, 0)
        assert relerr(gW, base.double() + dy.double().t() @ x.double()) < 3e-6, (M, N, K, ks)
    # batched einsum gradients: d emb[b] = dl[b]^T xs[b] (transA, transB), d xs[b] = dl[b] emb[b] (transB), Q not a multiple of 4
    B, T, Q, D = 3, 70, 13, 64
    dl, xs, e = R(B, T, Q), R(B, T, D), R(B, Q, D)
    de, dxs = torch.empty(B, Q, D, device=DEV), torch.empty(B, T, D, device=DEV)
    call("sed_gemm_f32", dl.to(DEV), xs.to(DEV), None, None, de, None, Q, D, T, Q, D, D, 1, 1, B, T * Q, T * D, Q * D, 0, 0, 1, 0.0, 0, 0)
    call("sed_gemm_f32", dl.to(DEV), e.to(DEV), None, None, dxs, None, T, D, Q, Q, D, D, 0, 1, B, T * Q, Q * D, T * D, 0, 0, 1, 0.0, 0, 0)
    assert relerr(de, torch.einsum("btq,btd->bqd", dl.double(), xs.double())) < 3e-6
    assert relerr(dxs, torch.einsum("btq,bqd->btd", dl.double(), e.double())) < 3e-6
    # forward with the pre-activation kept and a dropout epilogue: out = drop(gelu(x W^T + b)) + res
    M, N, K, p, seed, site = 100, 768, 256, 0.25, 1234567, 5
    x, W, b, res = R(M, K), R(N, K) / K ** 0.5, R(N), R(M, N)
    out, pre = torch.empty(M, N, device=DEV), torch.empty(M, N, device=DEV)
    call("sed_gemm_f32", x.to(DEV), W.to(DEV), b.to(DEV), res.to(DEV), out, pre, M, N, K, K, K, N, 0, 0, 1, 0, 0, 0, 1, 0, 1, p, seed, site)
    keep = keep_mask(M * N, p, seed, site).view(M, N).double()
    assert 0.70 < float(keep.mean()) < 0.80
    want_pre = x.double() @ W.double().t() + b.double()
    assert relerr(pre, want_pre) < 3e-6
    want = torch.nn.functional.gelu(want_pre) * keep / (1 - p) + res.double()
    assert float((out.cpu().double() - want).abs().max()) < 2e-5
    # its backward helpers: gelu'(pre) with the same bits, and the plain dropout gradient
    dy = R(M, N)
    o1, o2 = torch.empty(M, N, device=DEV), torch.empty(M, N, device=DEV)
    call("sed_gelu_bwd_f32", dy.to(DEV), pre, o1, M * N, p, seed, site)
    call("sed_dropout_f32", dy.to(DEV), o2, None, M * N, p, seed, site)
    xx = want_pre.clone().requires_grad_(True)
    torch.nn.functional.gelu(xx).backward(dy.double() * keep / (1 - p))
    assert float((o1.cpu().double() - xx.grad).abs().max()) < 2e-5
    assert float((o2.cpu().double() - dy.double() * keep / (1 - p)).abs().max()) < 1e-6
    # GELU epilogue on non-finite pre-activations (common.h gelu_fast2): NaN stays NaN, +-inf becomes NaN -- never a finite value
    xe = torch.zeros(64, 32); xe[0, 0] = 1.0; xe[1, 0] = float("nan"); xe[2, 0] = float("inf"); xe[3, 0] = float("-inf")
    We = torch.zeros(64, 32); We[:, 0] = 1.0
    oe = torch.empty(64, 64, device=DEV)
    call("sed_gemm_f32", xe.to(DEV), We.to(DEV), None, None, oe, None, 64, 64, 32, 32, 32, 64, 0, 0, 1, 0, 0, 0, 1, 0, 1, 0.0, 0, 0)
    oe = oe.cpu()
    assert abs(float(oe[0, 0]) - 0.8413447) < 1e-5 and bool(torch.isnan(oe[1:4, 0]).all()) and bool(torch.isfinite(oe[4:]).all())
    # column sums (+=)
    xm = R(333, 1000)
    acc = torch.ones(1000, device=DEV)
    call("sed_colsum_f32", xm.to(DEV), acc, 333, 1000, 1000)
    assert float((acc.cpu().double() - (1 + xm.double().sum(0))).abs().max()) < 1e-4


@pytest.mark.parametrize("B,H,Nq,Nk,dh,masked,p", [(2, 12, 12, 60, 64, False, 0.0), (2, 12, 12, 12, 64, True, 0.1), (2, 4, 70, 300, 64, False, 0.1),
                                                   (1, 12, 130, 130, 32, True, 0.0), (2, 6, 5, 17, 32, False, 0.2), (1, 12, 407, 1188, 64, False, 0.1)])
def test_xattn_f32_train_fwd_bwd_vs_torch_autograd(B, H, Nq, Nk, dh, masked, p):
    """Packed layouts as the decoder uses them: self attention reads q | k | v out of one [M, 3 D] projection and writes dq | dk | dv into one."""
    from transformer4sed_amd.ops import call
    g = torch.Generator().manual_seed(Nq * 1000 + Nk)
    D = H * dh
    selfattn = Nq == Nk
    if selfattn:
        qkv = torch.randn(B, Nq, 3 * D, generator=g)
        q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
    else:
        q, k, v = torch.randn(B, Nq, D, generator=g), torch.randn(B, Nk, D, generator=g), torch.randn(B, Nk, D, generator=g)
    dO = torch.randn(B, Nq, D, generator=g)
    mask = None
    if masked:
        mask = torch.rand(Nq, Nk, generator=g) < 0.4
        mask.fill_diagonal_(False)
    seed, site = 99 + Nq, 3
    keep = None
    if p > 0:
        keep = keep_mask(B * H * Nq * Nk, p, seed, site).view(B, H, Nq, Nk).double()
        assert abs(float(keep.mean()) - (1 - p)) < 0.02
    qd, kd, vd = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    qh, kh, vh = (t.view(B, -1, H, dh).transpose(1, 2) for t in (qd, kd, vd))
    s = qh @ kh.transpose(-1, -2) / dh ** 0.5
    if mask is not None:
        s = s.masked_fill(mask[None, None], float("-inf"))
    pr = torch.softmax(s, -1)
    if keep is not None:
        pr = pr * keep / (1 - p)
    want = (pr @ vh).transpose(1, 2).reshape(B, Nq, D)
    want.backward(dO.double())
    m8 = None if mask is None else mask.to(torch.uint8).to(DEV)
    out, lse, Dq = torch.empty(B, Nq, D, device=DEV), torch.empty(B * H * Nq, device=DEV), torch.empty(B * H * Nq, device=DEV)
    if selfattn:
        x = qkv.contiguous().to(DEV)
        dx = torch.full((B, Nq, 3 * D), float("nan"), device=DEV)
        ptr, dptr = x.data_ptr(), dx.data_ptr()
        call("sed_xattn_f32_fwd_train", x, ptr + 4 * D, ptr + 8 * D, out, m8, lse, B, H, Nq, Nk, dh, 3 * D, 3 * D, 3 * D, D, Nq * 3 * D, p, seed, site)
        call("sed_xattn_f32_bwd", x, ptr + 4 * D, ptr + 8 * D, out, dO.to(DEV), lse, Dq, dx, dptr + 4 * D, dptr + 8 * D, m8, B, H, Nq, Nk, dh, 3 * D, 3 * D,
             3 * D, D, 3 * D, 3 * D, 3 * D, Nq * 3 * D, p, seed, site)
        dq, dk, dv = dx[..., :D], dx[..., D:2 * D], dx[..., 2 * D:]
    else:
        dq, dk, dv = torch.empty(B, Nq, D, device=DEV), torch.empty(B, Nk, D, device=DEV), torch.empty(B, Nk, D, device=DEV)
        call("sed_xattn_f32_fwd_train", q.to(DEV), k.to(DEV), v.to(DEV), out, m8, lse, B, H, Nq, Nk, dh, D, D, D, D, Nq * D, p, seed, site)
        call("sed_xattn_f32_bwd", q.to(DEV), k.to(DEV), v.to(DEV), out, dO.to(DEV), lse, Dq, dq, dk, dv, m8, B, H, Nq, Nk, dh, D, D, D, D, D, D, D, Nq * D,
             p, seed, site)
    e_out = float((out.cpu().double() - want.detach()).abs().max())
    lse_want = torch.logsumexp(s.detach(), -1) * 1.4426950408889634
    e_lse = float((lse.view(B, H, Nq).cpu().double() - lse_want).abs().max())
    e_g = {name: relerr(got, ref) for name, got, ref in (("dq", dq, qd.grad), ("dk", dk, kd.grad), ("dv", dv, vd.grad))}
    logerr(f"xattn train B={B} H={H} Nq={Nq} Nk={Nk} dh={dh} masked={masked} p={p}: out {e_out:.2e} lse {e_lse:.2e} " + " ".join(f"{k} {v:.2e}" for k, v in e_g.items()))
    # Three-term split-precision products (csrc/dasm.hip XA_SPLIT16): the forward's q, k, v, P as IEEE-half pairs (2^-22 per product), everything
    # that carries a gradient as bf16 pairs (2^-17 = 7.6e-6 per product, fp32 accumulation) -- bounds at ~3x the measured values, three
    # orders of magnitude inside the model-level parity bounds they feed (1e-3 posteriors, 3e-3 gradient norms)
    assert e_out < 3e-5, e_out
    assert e_lse < 1e-4, e_lse
    for name, e in e_g.items():
        assert e < 3e-5, (name, e)


def test_xattn_split_precision_range_sharp_scores_large_values_tiny_gradients():
    """The split-precision attention (csrc/dasm.hip) at the edges of its operand formats: scores of standard deviation ~16 (a near one-hot
    softmax), values of magnitude 1e3 (IEEE-half hi terms up to 65504 / lo terms down to the subnormals), and output gradients of 1e-9 (bf16
    pairs keep the fp32 exponent range) -- against fp64 autograd, errors relative to the size of what they are compared with."""
    from transformer4sed_amd.ops import call
    g = torch.Generator().manual_seed(7)
    B, H, Nq, Nk, dh = 2, 4, 40, 100, 64
    D = H * dh
    q, k = 4.0 * torch.randn(B, Nq, D, generator=g), 4.0 * torch.randn(B, Nk, D, generator=g)
    v = 1e3 * torch.randn(B, Nk, D, generator=g)
    dO = 1e-9 * torch.randn(B, Nq, D, generator=g)
    qd, kd, vd = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    qh, kh, vh = (t.view(B, -1, H, dh).transpose(1, 2) for t in (qd, kd, vd))
    s = qh @ kh.transpose(-1, -2) / dh ** 0.5
    assert float(torch.softmax(s.detach(), -1).max(-1).values.mean()) > 0.8          # sharp: most rows are dominated by one key
    want = (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, Nq, D)
    want.backward(dO.double())
    out, lse, Dq = torch.empty(B, Nq, D, device=DEV), torch.empty(B * H * Nq, device=DEV), torch.empty(B * H * Nq, device=DEV)
    dq, dk, dv = torch.empty(B, Nq, D, device=DEV), torch.empty(B, Nk, D, device=DEV), torch.empty(B, Nk, D, device=DEV)
    call("sed_xattn_f32_fwd_train", q.to(DEV), k.to(DEV), v.to(DEV), out, None, lse, B, H, Nq, Nk, dh, D, D, D, D, Nq * D, 0.0, 1, 0)
    call("sed_xattn_f32_bwd", q.to(DEV), k.to(DEV), v.to(DEV), out, dO.to(DEV), lse, Dq, dq, dk, dv, None, B, H, Nq, Nk, dh, D, D, D, D, D, D, D, Nq * D,
         0.0, 1, 0)
    e_out = relerr(out, want.detach())
    e_g = {n: relerr(got, ref) for n, got, ref in (("dq", dq, qd.grad), ("dk", dk, kd.grad), ("dv", dv, vd.grad))}
    logerr(f"xattn range test (scores sd 16, |v| 1e3, |dO| 1e-9): out {e_out:.2e} " + " ".join(f"{n} {e:.2e}" for n, e in e_g.items()))
    assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(t).all()) for t in (dq, dk, dv))
    # a near one-hot softmax turns a score error d into a relative probability error d on the runner-up keys (2^-21 |s| ~ 3e-5 here).
    # Measured: out 8.9e-7, dq / dk 1.8e-5, dv 6.0e-6
    assert e_out < 1e-5, e_out
    for n, e in e_g.items():
        assert e < 6e-5, (n, e)


def test_dasm_head_finish_bwd_and_sup_loss_vs_torch():
    from transformer4sed_amd.ops import call
    g = torch.Generator().manual_seed(5)
    B, T, Q, temp = 3, 70, 13, 0.5
    logits, at_logit = torch.randn(B, T, Q, generator=g) * 3, torch.randn(B, Q, generator=g) * 2
    at_logit[0, 0] = -30.0                       # a tagging probability of ~1e-13: every frame posterior of that query sits on the lower clamp
    pad = torch.zeros(B, T, dtype=torch.bool)
    pad[1, 50:] = True
    dstrong, dweak, dat = torch.randn(B, Q, T, generator=g), torch.randn(B, Q, generator=g), torch.randn(B, Q, generator=g)
    for with_at in (True, False):
        l, a_l = logits.double().clone().requires_grad_(True), at_logit.double().clone().requires_grad_(True)
        a = torch.sigmoid(a_l)
        sed = torch.sigmoid(l / temp) * (a.unsqueeze(1) if with_at else 1.0)
        sed = sed.masked_fill(pad.unsqueeze(-1), 0.0)
        if with_at:
            sed = torch.clamp(sed, 1e-7, 1.0)
        weak = torch.clamp((sed * sed).sum(1) / sed.sum(1), 1e-7, 1.0)
        loss = (sed.transpose(1, 2) * dstrong.double()).sum() + (weak * dweak.double()).sum() + ((a * dat.double()).sum() if with_at else 0.0)
        loss.backward()
        strong, weak_g, at_out = torch.empty(B, Q, T, device=DEV), torch.empty(B, Q, device=DEV), torch.empty(B, Q, device=DEV)
        pm = pad.to(torch.uint8).to(DEV)
        al = at_logit.to(DEV) if with_at else None
        call("sed_dasm_head_fwd", logits.to(DEV), al, pm, temp, strong, weak_g, at_out if with_at else None, B, T, Q, 1 if with_at else 0)
        assert float((strong.cpu().double() - sed.detach().transpose(1, 2)).abs().max()) < 2e-6
        assert float((weak_g.cpu().double() - weak.detach()).abs().max()) < 2e-6
        dlog, dal = torch.empty(B, T, Q, device=DEV), (torch.empty(B, Q, device=DEV) if with_at else None)
        call("sed_dasm_head_bwd", logits.to(DEV), al, pm, temp, strong, dstrong.to(DEV), dweak.to(DEV), dat.to(DEV) if with_at else None, dlog, dal,
             torch.empty(3 * B * Q, device=DEV), B, T, Q, 1 if with_at else 0)
        assert float((dlog.cpu().double() - l.grad).abs().max()) < 2e-5 * float(l.grad.abs().max()), with_at
        assert float(dlog[1, 50:].abs().max()) == 0.0
        if with_at:
            assert float((dal.cpu().double() - a_l.grad).abs().max()) < 2e-5 * float(a_l.grad.abs().max())
            assert float(dlog[0, :, 0].abs().max()) == 0.0        # clamped: no gradient to the logits
    # supervised losses (src/functional/loss/__init__.py): BCELoss, AsymmetricalFocalLoss(gamma, zeta), AslLoss(rp, rn, margin), MSELoss
    n = 5000
    pr = torch.rand(n, generator=g).clamp(1e-7, 1.0)
    pr[:3] = torch.tensor([1e-7, 1.0, 0.5])
    tg = (torch.rand(n, generator=g) < 0.3).float()
    tg[100:200] = torch.rand(100, generator=g)            # mixup makes soft labels
    for kind, gp, gn, margin in ((0, 0.0, 0.0, 0.0), (0, 1.0, 2.0, 0.0), (0, 0.5, 4.0, 0.05), (1, 0.0, 0.0, 0.0)):
        pd = pr.double().clone().requires_grad_(True)
        if kind == 1:
            want = torch.nn.functional.mse_loss(pd, tg.double())
        elif gp == gn == margin == 0.0:
            want = torch.nn.functional.binary_cross_entropy(pd, tg.double())
        else:
            pm_ = torch.maximum(pd - margin, torch.zeros_like(pd))
            want = torch.mean(-(((1 - pd) ** gp) * tg.double() * torch.clamp_min(torch.log(pd), -100) +
                                (pm_ ** gn) * (1 - tg.double()) * torch.clamp_min(torch.log(1 - pm_), -100)))
        want.backward()
        loss, grad = torch.zeros(1, device=DEV), torch.empty(n, device=DEV)
        call("sed_sup_loss", pr.to(DEV), tg.to(DEV), loss, grad, n, kind, gp, gn, margin)
        assert abs(float(loss) - float(want)) < 2e-5 * max(1.0, abs(float(want))), (kind, gp, gn, margin, float(loss), float(want))
        fin = torch.isfinite(pd.grad) & (pd.grad.abs() < 1e6)
        assert float((grad.cpu().double() - pd.grad)[fin].abs().max()) < 1e-4 * float(pd.grad[fin].abs().max()), (kind, gp, gn, margin)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("layout", ["contiguous", "transposed"])
def test_supervised_loss_dtypes_and_layouts_vs_float64_autograd(dtype, layout):
    """The drop-in loss (dasm_trainer.loss_function_factory) as the trainers call it: f32 / f16 / bf16 posteriors, contiguous or a
    transposed view, exact 0 and 1 among them (torch clamps the log at -100) -- loss and gradient against torch autograd in float64 on the
    same (rounded) values; the gradient comes back in the prediction's dtype and layout."""
    from transformer4sed_amd.dasm_trainer import loss_function_factory
    g = torch.Generator().manual_seed(23)
    B, C, T = 2, 8, 256
    pr = torch.rand(B, T, C, generator=g).clamp(1e-7, 1.0)
    pr[0, :4, 0] = torch.tensor([0.0, 1.0, 1e-7, 0.5])
    pr[1, :4, 1] = torch.tensor([1.0, 0.0, 1.0 - 2 ** -12, 0.5])
    tg = (torch.rand(B, C, T, generator=g) < 0.3).float()
    tg[1, 3, 100:150] = torch.rand(50, generator=g)          # soft labels (mixup)
    tg[0, 0, 0], tg[0, 0, 1], tg[1, 1, 0], tg[1, 1, 1] = 1.0, 0.0, 0.0, 1.0      # saturated edges with and against the target
    pr = pr.to(dtype)
    base = pr.transpose(1, 2) if layout == "transposed" else pr.transpose(1, 2).contiguous()       # [B, C, T]
    eps = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}[dtype]
    for name, kw, formula in (("BCELoss", None, "bce"), ("MSELoss", {}, "mse"), ("AsymmetricalFocalLoss", dict(gamma=1.0, zeta=2.0), "asl"),
                              ("AslLoss", dict(rp=0.5, rn=4.0, margin=0.05), "asl")):
        fn = loss_function_factory(name, kw)
        pred = base.to(DEV).detach().requires_grad_(True)
        if layout == "transposed":
            assert not pred.is_contiguous()
        loss = fn(pred, tg.to(DEV))
        loss.backward()
        pd = base.double().detach().requires_grad_(True)
        t64 = tg.double()
        if formula == "mse":
            want = torch.nn.functional.mse_loss(pd, t64)
        elif formula == "bce":
            want = torch.nn.functional.binary_cross_entropy(pd, t64)
        else:
            gp, gn, mg = (kw["gamma"], kw["zeta"], 0.0) if name == "AsymmetricalFocalLoss" else (kw["rp"], kw["rn"], kw["margin"])
            pm_ = torch.maximum(pd - mg, torch.zeros_like(pd))
            want = torch.mean(-(((1 - pd) ** gp) * t64 * torch.clamp_min(torch.log(pd), -100) +
                                (pm_ ** gn) * (1 - t64) * torch.clamp_min(torch.log(1 - pm_), -100)))
        want.backward()
        assert abs(float(loss) - float(want)) < 2e-5 * max(1.0, abs(float(want))), (name, dtype, layout, float(loss), float(want))
        assert pred.grad is not None and pred.grad.dtype == dtype and pred.grad.shape == pred.shape, (name, dtype, layout)
        got, ref = pred.grad.cpu().double(), pd.grad
        fin = torch.isfinite(ref) & (ref.abs() < 1e6)      # (torch's BCE gradient at p = 0 or 1 is 1 / max(p (1 - p), 1e-12): not a number to match)
        tol = 1e-4 * float(ref[fin].abs().max()) + 2 * eps * ref[fin].abs()
        bad = ((got - ref)[fin].abs() > tol)
        assert not bool(bad.any()), (name, dtype, layout, float((got - ref)[fin].abs().max()))
    # no gradient wanted: the value alone
    with torch.no_grad():
        v = loss_function_factory("BCELoss", None)(base.to(DEV), tg.to(DEV))
    assert abs(float(v) - float(torch.nn.functional.binary_cross_entropy(base.double(), tg.double()))) < 2e-5 * max(1.0, float(v))
    # keyword arguments that would change the result are refused; the defaults the YAMLs may spell out are not
    loss_function_factory("BCELoss", dict(reduction="mean"))
    for name, kw in (("BCELoss", dict(reduction="sum")), ("MSELoss", dict(reduction="none")), ("BCELoss", dict(weight=torch.ones(3))),
                     ("AslLoss", dict(rp=1, rn=1, margin=0, weight=[1.0]))):
        with pytest.raises((NotImplementedError, TypeError)):
            loss_function_factory(name, kw)


def test_wide_classifier_head_407_classes_vs_torch():
    """The closed-set head at the AudioSet-Strong class count (recipes/audioset_strong/base/passt_cnn; passt_cnn.py:74-86): forward and
    backward of classifier + sigmoid / temperature + pad mask + linear-softmax pooling."""
    from transformer4sed_amd.dasm import wide_head_fwd, wide_head_bwd
    g = torch.Generator().manual_seed(7)
    B, T, C, K, temp = 2, 250, 407, 384, 0.5
    x, W, b = torch.randn(B * T, K, generator=g), torch.randn(C, K, generator=g) / K ** 0.5, torch.randn(C, generator=g) * 0.1
    pad = torch.zeros(B, T, dtype=torch.bool)
    pad[0, 200:] = True
    ds, dw = torch.randn(B, C, T, generator=g), torch.randn(B, C, generator=g)
    xd, Wd, bd = (t.double().clone().requires_grad_(True) for t in (x, W, b))
    sed = torch.sigmoid((xd @ Wd.t() + bd).view(B, T, C) / temp).masked_fill(pad.unsqueeze(-1), 0.0)
    weak = torch.clamp((sed * sed).sum(1) / sed.sum(1), 1e-7, 1.0)
    ((sed.transpose(1, 2) * ds.double()).sum() + (weak * dw.double()).sum()).backward()
    strong, wk, hc = wide_head_fwd(x.to(DEV), W.to(DEV), b.to(DEV), temp, pad, B, T, True)
    assert float((strong.cpu().double() - sed.detach().transpose(1, 2)).abs().max()) < 2e-6
    assert float((wk.cpu().double() - weak.detach()).abs().max()) < 2e-6
    gW, gb = torch.zeros(C, K, device=DEV), torch.zeros(C, device=DEV)
    dx = wide_head_bwd(hc, W.to(DEV), ds.to(DEV), dw.to(DEV), gW, gb)
    assert relerr(dx, xd.grad) < 1e-5 and relerr(gW, Wd.grad) < 1e-5 and relerr(gb, bd.grad) < 1e-5


def _head(n_base=8, qdim=1024, layers=2):
    from transformer4sed_amd.dasm import DasmHead
    sd = synth.dasm_state_dict_np(n_queries=n_base, query_dim=qdim, at_layers=layers)
    return DasmHead({k: torch.from_numpy(v).to(DEV) for k, v in sd.items()}, layers), {k: torch.from_numpy(v) for k, v in sd.items()}


@pytest.mark.parametrize("B,P,T,Q,pdrop,external", [(2, 60, 60, 8, 0.0, False), (2, 60, 60, 12, 0.1, True), (2, 1188, 1000, 40, 0.1, True),
                                                     (3, 60, 120, 407, 0.1, True)])
def test_dasm_head_forward_backward_vs_oracle_autograd(B, P, T, Q, pdrop, external):
    """Query decoder + dual-stream head, train mode: outputs, the gradient of every parameter, of the frame tokens and of the SED decoder's
    output against torch autograd through oracle/dasm_oracle.py (fp64), with the dropout bits the kernels use injected into the oracle."""
    from oracle import dasm_oracle
    head, sd = _head(8, 1024, 2)
    head.dropout = pdrop
    g = torch.Generator().manual_seed(11)
    frame = torch.from_numpy(synth.det_uniform("dasm_tr/frame", (B, P, 768), -1.5, 1.5))
    x_dec = torch.from_numpy(synth.det_normal("dasm_tr/xdec", (B, T, 768))) * 0.5
    ext = None
    if external:
        ext = torch.from_numpy(synth.det_normal("dasm_tr/q", (Q, 1024)))
        ext = ext / ext.norm(dim=-1, keepdim=True)
    else:
        Q = 8
    tmask = dasm_oracle.att_mask(Q, max(1, Q // 2))
    pad = torch.zeros(B, T, dtype=torch.bool)
    pad[0, T - 7:] = True
    seed = 424242
    s, w, a, mf, ctx = head.forward(frame.to(DEV), x_dec.to(DEV), query=None if ext is None else ext.to(DEV), tgt_mask=tmask, temp_w=0.5, pad_mask=pad,
                                    save=True, train=pdrop > 0, drop_seed=seed)
    drops = None
    H, M, Dd = 12, B * Q, 768
    if pdrop > 0:
        drops = {"p": pdrop}
        for l in range(2):
            for site, shape in ((0, (B, H, Q, P)), (1, (B, Q, Dd)), (2, (B, H, Q, Q)), (3, (B, Q, Dd)), (4, (B, Q, Dd)), (5, (B, Q, Dd))):
                n = int(np.prod(shape))
                drops[(l, site)] = keep_mask(n, pdrop, seed, 8 * l + site).view(shape).double()
    sdd = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    fr, xd = frame.double().clone().requires_grad_(True), x_dec.double().clone().requires_grad_(True)
    so, wo, ao, mo = dasm_oracle.dasm_head(sdd, fr, xd, query=None if ext is None else ext.double(), tgt_mask=tmask, temp_w=0.5, pad_mask=pad, n_layers=2,
                                           drops=drops)
    assert float((s.cpu().double() - so.detach()).abs().max()) < 1e-4 and float((a.cpu().double() - ao.detach()).abs().max()) < 1e-5
    assert float((w.cpu().double() - wo.detach()).abs().max()) < 1e-4
    ds = torch.randn(B, Q, T, generator=g) / T
    dw, da = torch.randn(B, Q, generator=g), torch.randn(B, Q, generator=g)
    ((so * ds.double()).sum() + (wo * dw.double()).sum() + (ao * da.double()).sum()).backward()
    grads = {k: torch.zeros_like(v, device=DEV) for k, v in sd.items()}
    dframe, dxdec = head.backward(ctx, ds.to(DEV), dw.to(DEV), da.to(DEV), lambda n: grads.get(n))
    worst = {}
    for k, v in sdd.items():
        if v.grad is None:
            assert float(grads[k].abs().max()) == 0.0, k      # (the learned queries when a call brought its own)
            continue
        worst[k] = relerr(grads[k], v.grad)
    worst["frame_tokens"] = relerr(dframe, fr.grad)
    worst["x_dec"] = relerr(dxdec, xd.grad)
    # fp32 throughout: 2e-4.  A Linear with >= 1024 rows (dasm.DasmHead._big) runs its forward in split precision and its two backward
    # products on the 16-bit matrix pipe with bf16 gradient operands like the trunk's weight / input gradients: 3e-3 for what comes out of
    # those -- the memory-side projection and sed_head at the real token / frame counts, every layer at 407 queries
    if B * Q >= 1024:
        # (`relerr` is the relative L2 error of the whole tensor, element by element: with every product of the chain on bf16 operands that is
        #  2^-8 .. 2^-7 -- measured 6.4e-3 at worst; the NORMS, what the trainer fixtures bound at 3e-3, are a magnitude closer)
        tol = lambda k: 1e-2
    else:
        bf = (("at_projector.", "frame_tokens") if B * P >= 1024 else ()) + (("sed_head.", "x_dec") if B * T >= 1024 else ())
        tol = lambda k: 3e-3 if (k.startswith(bf) or (B * P >= 1024 and "multihead_attn.in_proj" in k)) else 2e-4
    bad = {k: f"{e:.2e}" for k, e in worst.items() if e > tol(k)}
    print("DASM head backward, worst relative gradient errors:", sorted(((e, k) for k, e in worst.items()), reverse=True)[:5])
    assert not bad, bad


def test_dasm_head_train_mode_without_saving_drops_at_all_six_sites():
    """Train mode under torch.no_grad() (`save=False, train=True`: a mean-teacher's teacher pass): the same dropout as a saving forward -- all
    six sites of both layers, bits of `drop_seed` -- against oracle/dasm_oracle.py (fp64) with the host reference's masks
    (tests/dropout_cases.py) injected at every site.  (Before the fix the attention probabilities, sites 0 and 2, went undropped.)"""
    from oracle import dasm_oracle
    B, P, T, Q, pdrop, seed = 2, 60, 60, 12, 0.1, 0x0123456789ABCDEF
    head, sd = _head(8, 1024, 2)
    head.dropout = pdrop
    frame = torch.from_numpy(synth.det_uniform("dasm_tr/frame", (B, P, 768), -1.5, 1.5))
    x_dec = torch.from_numpy(synth.det_normal("dasm_tr/xdec", (B, T, 768))) * 0.5
    ext = torch.from_numpy(synth.det_normal("dasm_tr/q", (Q, 1024)))
    ext = ext / ext.norm(dim=-1, keepdim=True)
    tmask = dasm_oracle.att_mask(Q, max(1, Q // 2))
    pad = torch.zeros(B, T, dtype=torch.bool)
    pad[0, T - 7:] = True
    with torch.no_grad():
        s, w, a, mf = head.forward(frame.to(DEV), x_dec.to(DEV), query=ext.to(DEV), tgt_mask=tmask, temp_w=0.5, pad_mask=pad, save=False, train=True,
                                   drop_seed=seed)
    H, Dd = 12, 768
    drops = {"p": pdrop}
    for l in range(2):
        for site, shape in ((0, (B, H, Q, P)), (1, (B, Q, Dd)), (2, (B, H, Q, Q)), (3, (B, Q, Dd)), (4, (B, Q, Dd)), (5, (B, Q, Dd))):
            drops[(l, site)] = torch.from_numpy(dropout_cases.dasm_keep(int(np.prod(shape)), pdrop, seed, 8 * l + site)).view(shape).double()
    sdd = {k: v.double() for k, v in sd.items()}
    so, wo, ao, mo = dasm_oracle.dasm_head(sdd, frame.double(), x_dec.double(), query=ext.double(), tgt_mask=tmask, temp_w=0.5, pad_mask=pad, n_layers=2,
                                           drops=drops)
    e_s, e_w, e_a = (float((got.cpu().double() - ref).abs().max()) for got, ref in ((s, so), (w, wo), (a, ao)))
    logerr(f"dasm head, train mode without saving, p={pdrop}: strong {e_s:.2e} weak {e_w:.2e} tagging {e_a:.2e} (bounds 1e-4, 1e-4, 1e-5)")
    assert e_s < 1e-4 and e_w < 1e-4 and e_a < 1e-5, (e_s, e_w, e_a)


# ---------------------------------------------------------------------------------------------------------------------- whole model
CNN = dict(n_in_channel=1, activation="cg", conv_dropout=0.0, kernel_size=[3] * 10, padding=[1] * 10, stride=[1] * 10,
           nb_filters=list(synth.PMAM_FILTERS), pooling=[list(p) for p in synth.PMAM_POOLING])
REF_NAME = (("decoder.", "sed_decoder."), ("out_norm.", "norm_before_pool."))


def ref_name(n):
    for mine, ref in REF_NAME:
        if n.startswith(mine):
            return ref + n[len(mine):]
    return n


def build_dasm(depth, nb=8, qdim=1024, dropout=0.0, sed_head_bias=None, sed_head_scale=1.0):
    from transformer4sed_amd.dasm import DASM
    sd = synth.dasm_full_state_dict_np(n_queries=nb, query_dim=qdim)
    if sed_head_bias is not None:      # the fixture's calibrated sed_head (oracle/make_golden.py:gen_dasm_train): scaled weight, bias that centres the logits
        sd["sed_head.weight"] = (np.asarray(sd["sed_head.weight"]) * np.float32(sed_head_scale)).astype(np.float32)
        sd["sed_head.bias"] = sed_head_bias
    net = DASM(cnn_param=dict(CNN), backbone_param=dict(embed_dim=768, passt_feature_layer=min(depth, 10), pretrain_model_path=None, lora_config=None),
               at_param=dict(at_decoder_layer=2, query_projector=True, query_dim=qdim, out_type="sigmoid", query=torch.from_numpy(sd["at_query"]).clone()),
               decoder="transformerXL", decoder_layer_num=3, decoder_dim=768, num_heads=12, class_num=nb, _encoder_depth=depth)
    own = net.state_dict()
    net.load_state_dict({k: torch.from_numpy(np.asarray(sd[k])) for k in own if not k.startswith("mel_trans.")}, strict=False)
    net.at_dropout = dropout
    return net.to(DEV)


@pytest.mark.parametrize("tag", ["dasmstep", "dasmstep12"])
def test_dasm_trainer_steps_vs_reference_trainer(golden, tag):
    """DasmTrainer.step (HIP path, fused AdamW) against the scalars the REFERENCE DASMTrainer.train logged, the gradient norm of every
    parameter at the first step and the probe parameters after every step (tests/golden/dasmstep.npz: 3 steps at encoder depth 2, batch 3;
    dasmstep12.npz: 1 step at depth 12, batch 2).  Same seeds => same augmentation draws (frontend, frame_shift with the recipe's
    max_shift_frame = 2 sr, mixup under the coin flip, FilterAugment)."""
    import json
    import random
    from transformer4sed_amd.dasm_trainer import DasmTrainer
    from transformer4sed_amd.pmam_trainer import get_param_lr
    from transformer4sed_amd.scheduler import ExponentialDown
    from transformer4sed_amd.trainer import FusedAdamWEMA
    g = golden(tag)
    meta = json.loads(str(g["config_json"]))
    cfg, sc, depth, B, steps = meta["cfg"], meta["sched"], meta["depth"], meta["B"], meta["steps"]
    net = build_dasm(depth, sed_head_bias=g["sed_head_bias"], sed_head_scale=float(g["sed_head_scale"]))
    groups = get_param_lr(net, cfg["opt"]["param_groups"])
    assert [len(x["params"]) for x in groups] == list(g["group_sizes"])
    assert sorted(ref_name(n) for n, p in net.named_parameters() if p.requires_grad) == sorted(str(n) for n in g["trainable"])
    opt = FusedAdamWEMA(net, groups, ema_net=None, betas=(0.9, 0.999), eps=1e-8)
    sched = ExponentialDown(opt, start_iter=sc["n_epochs_cut"] * sc["epoch_len"], total_iter=sc["n_epochs"] * sc["epoch_len"],
                            exponent=sc["exponent"], warmup_iter=sc["warmup_epochs"] * sc["epoch_len"], warmup_rate=sc["warmup_rate"])
    tr = DasmTrainer(net, opt, sched, cfg, sr=16000)
    random.seed(meta["seeds"][0]); np.random.seed(meta["seeds"][1]); torch.manual_seed(meta["seeds"][2])
    names = [str(n) for n in g["probe_names"]]
    mine = {ref_name(n): p for n, p in net.named_parameters()}
    os.makedirs("gpurun_out", exist_ok=True)
    for step in range(steps):
        wav = torch.from_numpy(synth.synth_wav(B, seed=meta["wav_seed0"] + step)).to(DEV)
        labels = torch.from_numpy(synth.synth_strong_labels(B, n_classes=8, seed=meta["label_seed0"] + step)).to(DEV)
        out = tr.step(wav, labels)
        for k in ("loss_total", "loss_class_strong", "loss_class_at_specific"):
            ref, got = float(g[f"s{step}_{k}"]), float(out[k])
            print(f"{tag} step {step} {k}: got {got:.6f} ref {ref:.6f}")
            assert abs(got - ref) <= 3e-3 * max(abs(ref), 0.05), (step, k, got, ref)
        assert abs(sched._get_scale() - float(g[f"s{step}_lr_scaler"])) < 1e-12
        np.testing.assert_allclose([x["lr"] for x in opt.param_groups], g[f"s{step}_lrs"], rtol=1e-12)
        if step == 0:
            gn = dict(zip((str(n) for n in g["gnorm_names"]), g["gnorm_values"]))
            worst, rows = 0.0, []
            for n, p in mine.items():
                ref = gn[n]
                if ref < 0:
                    assert p.grad is None, n
                    continue
                got = float(p.grad.norm())
                if n.startswith("cnn.cnn.conv") and n.endswith(".bias"):
                    # a bias in front of a train-mode BatchNorm: its gradient is zero in exact arithmetic (the batch mean removes it); both
                    # sides hold rounding noise, a thousandth and less of the weight's gradient
                    wn = gn[n[:-4] + "weight"]
                    assert ref < 2e-3 * wn and got < 2e-3 * wn, (n, got, ref, wn)
                    continue
                e = abs(got - ref) / max(ref, 1e-12)
                rows.append((e, n, got, ref))
                worst = max(worst, e)
            rows.sort(reverse=True)
            with open("gpurun_out/dasm_errors.log", "a") as f:
                f.write(f"{tag}: first-step gradient norms vs the reference, worst five of {len(rows)}: " +
                        "; ".join(f"{n} {e:.2e}" for e, n, _, _ in rows[:5]) + "\n")
            print(f"{tag}: worst gradient-norm errors", [(f"{e:.2e}", n) for e, n, _, _ in rows[:5]])
            with open(f"gpurun_out/dasm_gradnorms_{tag}.txt", "w") as f:
                for e, n, got, ref in rows:
                    f.write(f"{e:.3e} {n} got {got:.6e} ref {ref:.6e}\n")
            # everything this round added -- query decoder, dual-stream head, at_projector, norm_after_merge -- and the encoder blocks:
            # 3e-3 on every gradient norm.  The rest of the trunk (CNN branch, context network, pooling, token tables) keeps the bound its
            # own suite gives it (tests/test_gpu_pmam.py: 2e-2 -- bf16 gradient operands on tensors whose gradients are 1e-3 .. 1e-5 of
            # the largest), with the median of ALL tensors under 3e-3.
            new = ("at_", "query_projector", "mask_embedding_layer", "sed_head", "norm_after_merge", "backbone.blocks", "backbone.norm")
            bad = [(n, f"{e:.2e}") for e, n, _, _ in rows if e > (3e-3 if n.startswith(new) else 2e-2)]
            assert not bad, bad
            assert sorted(e for e, _, _, _ in rows)[len(rows) // 2] < 3e-3
        worst = 0.0
        for i, n in enumerate(names):
            p = mine[n]
            pn = [k for k, v in net.named_parameters() if v is p][0]
            lr = max(x["lr"] for x in opt.param_groups if pn in x["names"])
            d = p.detach().reshape(-1)[:256].cpu().numpy() - g[f"s{step}_p{i}"]
            ms = float(np.abs(d).mean()) / lr
            worst = max(worst, ms)
            assert ms < 0.15, (step, n, ms)
        print(f"{tag} step {step}: worst probe mean|dp|/lr {worst:.4f}")


def test_dasm_train_mode_dropout_multimodal_and_external_query_grad():
    """Train-mode forward / backward with the decoder's dropout ON (p = 0.1: finite, different bits per step, deterministic for a fixed seed);
    external queries that require grad receive their gradient through the model's autograd node (the open-vocabulary trainer trains rows
    of at_query this way, open_vocabulary.py:20-31); a model built with two modalities picks one per event."""
    from transformer4sed_amd.dasm import DASM
    net = build_dasm(2, dropout=0.1)
    net.train()
    mel = torch.from_numpy(synth.det_uniform("dasm_tr/mel", (2, 128, 1000), -1.2, 1.2)).to(DEV)
    q = net.at_query.detach()[:5].clone().requires_grad_(True)
    torch.manual_seed(3)
    s1, w1, o1 = net(mel, temp_w=0.5, query=q)
    (s1.mean() + o1["at_out"].mean()).backward()
    assert q.grad is not None and q.grad.shape == q.shape and float(q.grad.abs().max()) > 0 and bool(torch.isfinite(q.grad).all())
    assert net.at_query.grad is None
    g1 = net.sed_head.weight.grad.clone()
    s2, _, _ = net(mel, temp_w=0.5, query=q)
    assert float((s1 - s2).abs().max()) > 0            # new dropout bits
    net._drop_gen = None
    torch.manual_seed(3)
    for p_ in net.parameters():
        p_.grad = None
    net._last_grad_arena = None
    s3, w3, o3 = net(mel, temp_w=0.5, query=q)
    same, other = float((s1 - s3).abs().max()), float((s1 - s2).abs().max())
    print("same seed", same, "other seed", other)
    assert same < 5e-4 and other > 20 * same          # same seed, same dropout bits; what is left (1.2e-4 seen) is the order of the trunk's fp32 atomics at temperature 0.5
    # two modalities (text + audio embeddings of different widths)
    sd = synth.dasm_full_state_dict_np(n_queries=8, query_dim=1024)
    qa = torch.from_numpy(synth.det_normal("dasm_tr/audio_q", (8, 512)))
    net2 = DASM(cnn_param=dict(CNN), backbone_param=dict(embed_dim=768, passt_feature_layer=2, pretrain_model_path=None, lora_config=None),
                at_param=dict(at_decoder_layer=1, query_projector=True, query_dim=[1024, 512], out_type="sigmoid",
                              query=[torch.from_numpy(sd["at_query"]).clone(), qa]),
                decoder="transformerXL", decoder_layer_num=1, decoder_dim=768, num_heads=12, class_num=8, _encoder_depth=2)
    keys = set(net2.state_dict())
    assert {"at_query.0", "at_query.1", "query_projector.0.0.weight", "query_projector.1.0.weight"} <= keys
    net2 = net2.to(DEV).train()
    s, w, o = net2(mel, temp_w=0.5)
    (s.mean() + w.mean()).backward()
    g0, g1_ = net2.at_query[0].grad, net2.at_query[1].grad
    assert g0 is not None and g1_ is not None
    rows0, rows1 = (g0.abs().sum(1) > 0), (g1_.abs().sum(1) > 0)
    assert bool((rows0 ^ rows1).all())                 # every event took exactly one modality
    with torch.no_grad():
        net2.eval()
        s_t, _, _ = net2(mel, temp_w=0.5, query=torch.from_numpy(sd["at_query"]).to(DEV), query_type="text")
        assert s_t.shape == (2, 8, 1000)
        with pytest.raises(RuntimeError):
            net2(mel, temp_w=0.5, query=torch.from_numpy(sd["at_query"]).to(DEV))


def test_dasm_train_mode_under_no_grad_draws_fresh_dropout_bits():
    """A train-mode forward under torch.no_grad() (what a mean-teacher's teacher pass is) takes a fresh dropout seed like a forward that
    saves for the backward: two forwards differ, the same generator state repeats the first; eval mode has no dropout and leaves the
    model's seed generator where it was."""
    net = build_dasm(2, dropout=0.1).train()
    mel = torch.from_numpy(synth.det_uniform("dasm_tr/mel", (2, 128, 1000), -1.2, 1.2)).to(DEV)
    tol = 5e-4            # (the order of the trunk's fp32 atomics at temperature 0.5, as in the test above)
    with torch.no_grad():
        torch.manual_seed(3)
        s1 = net(mel, temp_w=0.5)[0].clone()
        s2 = net(mel, temp_w=0.5)[0].clone()
        net._drop_gen = None
        torch.manual_seed(3)
        s3 = net(mel, temp_w=0.5)[0].clone()
        same, other = float((s1 - s3).abs().max()), float((s1 - s2).abs().max())
        print("no_grad train mode: same seed", same, "other seed", other)
        assert other > 0
        assert same < tol, same
        assert other > 20 * tol, other
        # what differs between two forwards is the head's dropout and nothing else: without it they agree
        net.at_dropout = 0.0
        assert float((net(mel, temp_w=0.5)[0] - net(mel, temp_w=0.5)[0]).abs().max()) < tol
        net.at_dropout = 0.1
        net.eval()
        state = net._drop_gen.get_state().clone()
        e1 = net(mel, temp_w=0.5)[0].clone()
        e2 = net(mel, temp_w=0.5)[0].clone()
        assert float((e1 - e2).abs().max()) < tol
        assert torch.equal(net._drop_gen.get_state(), state)


def test_audioset_strong_trainer_steps_vs_reference_trainer(golden):
    """`AudiosetStrongTrainer.step` (HIP path, fused AdamW) against what the REFERENCE's closed-set loop logged and left behind
    (tests/golden/asstep.npz: two steps of `Trainer.train`, recipes/audioset_strong/base/passt_cnn/train.py:103-147, on PaSST_CNN with the 407
    AudioSet-Strong classes at encoder depth 2, batch 2; oracle/make_golden.py:gen_asstep): the logged loss and lr scale of both steps, the
    gradient norm of every parameter at the first step, the probe parameters after every step.  Same seeds => same augmentation draws."""
    import json
    import random
    from transformer4sed_amd.dasm_trainer import AudiosetStrongTrainer
    from transformer4sed_amd.passt_cnn import PaSST_CNN
    from transformer4sed_amd.pmam_trainer import get_param_lr
    from transformer4sed_amd.scheduler import ExponentialDown
    from transformer4sed_amd.trainer import FusedAdamWEMA
    g = golden("asstep")
    meta = json.loads(str(g["config_json"]))
    cfg, sc, depth, B, steps, C = meta["cfg"], meta["sched"], meta["depth"], meta["B"], meta["steps"], meta["class_num"]
    passt = dict(passt_feature_layer=depth, class_num=C, f_pool="attention", decode_ratio=10, at_adapter=False, decoder="transformerXL",
                 decoder_layer_num=3, decoder_pos_emd_len=1000, decoder_dim=384, mlm=False, load_pretrained_model=False, encoder_depth=depth)
    net = PaSST_CNN(passt_sed_param=passt, cnn_param=dict(CNN))
    sd = synth.pmam_state_dict_np(depth=12, mlm=False, lora_r=0, class_num=C)
    own = net.state_dict()
    net.load_state_dict({k: torch.from_numpy(np.asarray(sd[k])) for k in own if k in sd}, strict=False)
    net = net.to(DEV)
    groups = get_param_lr(net, cfg["opt"]["param_groups"])
    assert [len(x["params"]) for x in groups] == list(g["group_sizes"])
    assert sorted(n for n, p in net.named_parameters() if p.requires_grad) == sorted(str(n) for n in g["trainable"])
    opt = FusedAdamWEMA(net, groups, ema_net=None, betas=(0.9, 0.999), eps=1e-8)
    sched = ExponentialDown(opt, start_iter=sc["n_epochs_cut"] * sc["epoch_len"], total_iter=sc["n_epochs"] * sc["epoch_len"],
                            exponent=sc["exponent"], warmup_iter=sc["warmup_epochs"] * sc["epoch_len"], warmup_rate=sc["warmup_rate"])
    tr = AudiosetStrongTrainer(net, opt, sched, cfg, sr=16000)
    random.seed(meta["seeds"][0]); np.random.seed(meta["seeds"][1]); torch.manual_seed(meta["seeds"][2])
    names = [str(n) for n in g["probe_names"]]
    mine = dict(net.named_parameters())
    for step in range(steps):
        wav = torch.from_numpy(synth.synth_wav(B, seed=meta["wav_seed0"] + step)).to(DEV)
        labels = torch.from_numpy(synth.synth_strong_labels(B, n_classes=C, seed=meta["label_seed0"] + step)).to(DEV)
        out = tr.step(wav, labels)
        ref, got = float(g[f"s{step}_loss_class_strong"]), float(out["loss_class_strong"])
        logerr(f"asstep step {step} loss_class_strong: got {got:.6f} ref {ref:.6f} ({abs(got - ref) / ref:.2e})")
        assert abs(got - ref) <= 3e-3 * ref, (step, got, ref)
        assert abs(sched._get_scale() - float(g[f"s{step}_lr_scaler"])) < 1e-12
        np.testing.assert_allclose([x["lr"] for x in opt.param_groups], g[f"s{step}_lrs"], rtol=1e-12)
        if step == 0:
            gn = dict(zip((str(n) for n in g["gnorm_names"]), g["gnorm_values"]))
            rows = []
            for n, p in mine.items():
                ref = gn[n]
                if ref < 0:
                    assert p.grad is None, n
                    continue
                got = float(p.grad.norm())
                if n.startswith("cnn.cnn.conv") and n.endswith(".bias"):      # (zero in exact arithmetic: in front of a train-mode BatchNorm)
                    wn = gn[n[:-4] + "weight"]
                    assert ref < 2e-3 * wn and got < 2e-3 * wn, (n, got, ref, wn)
                    continue
                rows.append((abs(got - ref) / max(ref, 1e-12), n, got, ref))
            rows.sort(reverse=True)
            logerr(f"asstep: first-step gradient norms vs the reference, worst five of {len(rows)}: " + "; ".join(f"{n} {e:.2e}" for e, n, _, _ in rows[:5]))
            # the bounds of the PMAM trunk's own suite (tests/test_gpu_pmam.py): 2e-2 per tensor (`merge_weight`, one scalar of cancelling
            # products: 3e-2), the median of all tensors under 3e-3; the 407-class head itself within 3e-3
            bad = [(n, f"{e:.2e}") for e, n, _, _ in rows if e > (3e-3 if n.startswith("classifier.") else 3e-2 if n == "merge_weight" else 2e-2)]
            assert not bad, bad
            assert sorted(e for e, _, _, _ in rows)[len(rows) // 2] < 3e-3
        worst = 0.0
        for i, n in enumerate(names):
            lr = max(x["lr"] for x in opt.param_groups if n in x["names"])
            d = mine[n].detach().reshape(-1)[:256].cpu().numpy() - g[f"s{step}_p{i}"]
            ms = float(np.abs(d).mean()) / lr
            worst = max(worst, ms)
            assert ms < 0.15, (step, n, ms)
        logerr(f"asstep step {step}: worst probe mean|dp| / lr {worst:.4f}")


def test_audioset_strong_closed_set_step_407_classes():
    """`AudiosetStrongTrainer.step` = `Trainer.train` of recipes/audioset_strong/base/passt_cnn/train.py:103-140 on PaSST_CNN with the 407
    AudioSet-Strong classes (the head that was capped at 16 classes until round 6): loss and every gradient against torch autograd through
    the model's own outputs -- posteriors from the HIP forward, BCE in fp64 on the CPU, d loss / d posteriors fed to the HIP backward
    equals what the fused loss kernel feeds it -- and a step that lowers the loss on the same batch."""
    from transformer4sed_amd.dasm_trainer import AudiosetStrongTrainer
    from transformer4sed_amd.passt_cnn import PaSST_CNN
    from transformer4sed_amd.pmam_trainer import get_param_lr
    from transformer4sed_amd.scheduler import ExponentialDown
    from transformer4sed_amd.trainer import FusedAdamWEMA
    C = 407
    passt = dict(passt_feature_layer=2, class_num=C, f_pool="attention", decode_ratio=10, at_adapter=False, decoder="transformerXL",
                 decoder_layer_num=3, decoder_pos_emd_len=1000, decoder_dim=384, mlm=False, load_pretrained_model=False, encoder_depth=2)
    net = PaSST_CNN(passt_sed_param=passt, cnn_param=dict(CNN))
    sd = synth.pmam_state_dict_np(depth=12, mlm=False, lora_r=0, class_num=C)
    own = net.state_dict()
    net.load_state_dict({k: torch.from_numpy(np.asarray(sd[k])) for k in own if k in sd}, strict=False)
    net = net.to(DEV)
    cfg = dict(training=dict(clip_grad=True, transform=dict(n_transform=1, choice=[1, 0, 0, 1], filter_db_range=[-26, 26], filter_bands=[2, 5],
                                                           filter_minimum_bandwidth=4, filter_type="step")),
               class_loss=dict(loss_name="BCELoss", kwargs=None), PaSST_CNN=dict(train_kwargs=dict(encoder_win=False, temp_w=1)))
    lr = dict(cnn=dict(lr=1e-4, weight_decay=1e-4), passt=dict(lr=1e-5, weight_decay=1e-4, freeze_layer=0, step_lr=0),
              decoder=dict(lr=1e-4, weight_decay=1e-4), head=dict(lr=1e-3))
    opt = FusedAdamWEMA(net, get_param_lr(net, lr), ema_net=None)
    sched = ExponentialDown(opt, start_iter=40, total_iter=120, exponent=-1.5, warmup_iter=0, warmup_rate=0.1)
    tr = AudiosetStrongTrainer(net, opt, sched, cfg, sr=16000)
    B = 2
    wav = torch.from_numpy(synth.synth_wav(B, seed=4100)).to(DEV)
    labels = torch.from_numpy(synth.synth_strong_labels(B, n_classes=C, seed=900)).to(DEV)
    # the head's value and gradient on a plain train-mode forward
    net.train()
    mel = net.get_feature_extractor().logmel(wav)
    s, w, _ = net(mel, encoder_win=False, temp_w=1)
    assert s.shape == (B, C, 1000) and w.shape == (B, C)
    loss = tr.supervised_loss(s, labels)
    sd_ = s.detach().cpu().double().requires_grad_(True)
    want = torch.nn.functional.binary_cross_entropy(sd_, labels.cpu().double())
    want.backward()
    assert abs(float(loss) - float(want)) < 1e-5 * float(want)
    loss.backward()
    gw = net.classifier.weight.grad.clone()
    xd = None
    assert bool(torch.isfinite(gw).all()) and float(gw.abs().max()) > 0
    # classifier gradient = (d loss / d logits)^T x: recompute it from the posteriors on the CPU for the bias (column sums need no x)
    dlogit = (sd_.grad * sd_.detach() * (1 - sd_.detach())).sum(dim=(0, 2))
    assert relerr(net.classifier.bias.grad, dlogit) < 1e-4
    for p_ in net.parameters():
        p_.grad = None
    net._last_grad_arena = None
    import random
    random.seed(1); np.random.seed(2); torch.manual_seed(3)
    l0 = float(tr.step(wav, labels)["loss_total"])
    st = (random.getstate(), np.random.get_state(), torch.get_rng_state())
    random.seed(1); np.random.seed(2); torch.manual_seed(3)
    l1 = float(tr.step(wav, labels)["loss_total"])
    assert np.isfinite(l0) and l1 < l0, (l0, l1)
