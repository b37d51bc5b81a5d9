"""Frequency-wise transformer pooling, `PaSST_SED(f_pool="frequency_wise_tranformer_encoder")` (needs an MI355X).

Kernel level: the entry points of csrc/fpool_transformer.hip against plain-torch restatements of what they compute (timm 0.4.5
`Attention.forward` for 4 heads of 192; `out_norm` + the regrouping of passt_sed.py:202-214 + the tag row of pooling.py:28-29; the
closing LayerNorm on row 0, pooling.py:32-33), evaluated on the CPU in float64 and in float32; autograd gives the backward.  The bound
is the rule of tests/test_gpu_conformer.py, per element:
    |got - ref64| <= 8 max|ref32 - ref64| + half an ulp of the output's storage format at |ref64|
(2^(floor(log2 |x|) - 8) for bf16, 2^(floor(log2 |x|) - 11) for f16, nothing for fp32).

Model level: the depth-2 synth-weight model against the reference goldens of tools/gen_fpool_transformer_golden.py with the bounds of
tests/test_gpu_conformer.py::test_conformer_model_vs_reference_golden (posteriors within 1e-3: the project's contract)."""
import functools
import os
from copy import deepcopy

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu

from transformer4sed_amd import synth  # noqa: E402
from transformer4sed_amd.ops import call, BF16, F16, F32  # noqa: E402
from transformer4sed_amd.passt_sed import PaSST_SED  # noqa: E402

DEV = "cuda"
C, HEADS, HD = 768, 4, 192
FPOOL = "frequency_wise_tranformer_encoder"
TAG, PTAG, STAG = "model_d768_l2_fpooltr", "model_d768_l2_fpooltr_patchout4", "model_d768_l2_fpooltr_sharp"
NEW_ENTRY_POINTS = ("sed_fpool_seq_build_fwd", "sed_fpool_seq_build_bwd", "sed_fpool_rownorm_fwd", "sed_fpool_rownorm_bwd",
                    "sed_attn_short_fwd", "sed_attn_short_bwd")
LOGDIR = os.environ.get("SED_TEST_LOG_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_logs")
LOG = os.path.join(LOGDIR, "fpool_transformer_kernel_errors.log")
MLOG = os.path.join(LOGDIR, "fpool_transformer_model_errors.log")
ATTN_SHAPES = [(1, 2), (3, 13), (65, 9), (257, 13), (1188, 13)]
SEQ_SHAPES = [(1, 1, 12), (2, 50, 12), (3, 99, 8), (2, 7, 1)]
NORM_SHAPES = [(1, 2), (257, 13), (1188, 9)]
SIG_BITS = {"bf16": 8, "f16": 11}       # significand bits (with the hidden one) of the 16-bit storage formats


def maxerr(a, b):
    a = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))
    b = b if isinstance(b, torch.Tensor) else torch.from_numpy(np.asarray(b))
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def half_ulp(ref64, storage):
    if storage == "f32":
        return torch.zeros_like(ref64)
    _, e = torch.frexp(ref64.abs().clamp_min(1e-300))          # |x| = m 2^e, 0.5 <= m < 1
    h = torch.ldexp(torch.ones_like(ref64), e - 1 - SIG_BITS[storage])
    return h.clamp_min(2.0 ** -25) if storage == "f16" else h


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


# ------------------------------------------------------------------------------------------------ short attention
def attn_chain(qkv, S, N):
    """timm 0.4.5 Attention.forward between the qkv and proj linears: qkv [S N, 3 H 192] -> [S N, H 192], in qkv's dtype."""
    q, k, v = qkv.view(S, N, 3, HEADS, HD).permute(2, 0, 3, 1, 4)
    p = ((q @ k.transpose(-2, -1)) * HD ** -0.5).softmax(dim=-1)
    return (p @ v).transpose(1, 2).reshape(S * N, HEADS * HD)


def attn_inputs(S, N, tag="k"):
    """Values a 16-bit operand holds exactly: qkv as IEEE half (logits of a few units), dout as bf16."""
    qkv = torch.from_numpy(synth.det_normal(f"fpooltr/{tag}/qkv/{S}x{N}", (S * N, 3 * C), 1.6)).to(F16)
    dout = torch.from_numpy(synth.det_uniform(f"fpooltr/{tag}/dout/{S}x{N}", (S * N, C))).to(BF16)
    return qkv, dout


def attn_reference(qkv, dout, S, N):
    out = {}
    for dt in (torch.float64, torch.float32):
        x = qkv.to(dt).requires_grad_(True)
        o = attn_chain(x, S, N)
        (o * dout.to(dt)).sum().backward()
        out[dt] = (o.detach(), x.grad)
    return out[torch.float64], out[torch.float32]


@functools.lru_cache(maxsize=None)
def attn_case(S, N):
    qkv, dout = attn_inputs(S, N)
    return (qkv, dout) + attn_reference(qkv, dout, S, N)


def run_attn(qkv, dout, S, N, out_dt=F16):
    qkv, dout = qkv.to(DEV).contiguous(), dout.to(DEV).contiguous()
    kind = {BF16: 0, F16: 1, F32: 2}[qkv.dtype]
    o = torch.empty(S * N, C, dtype=out_dt, device=DEV)
    call("sed_attn_short_fwd", qkv, o, S, N, HEADS, kind, 1 if out_dt == F16 else 0)
    dqkv = torch.empty(S * N, 3 * C, dtype=BF16, device=DEV)
    call("sed_attn_short_bwd", qkv, dout, dqkv, S, N, HEADS, kind)
    return o, dqkv


@pytest.mark.parametrize("S,N", ATTN_SHAPES)
def test_attn_short_vs_float64(S, N):
    qkv, dout, r64, r32 = attn_case(S, N)
    o, dqkv = run_attn(qkv, dout, S, N)
    # measured at (1188, 13): out 1.95e-3 on values up to 5.3 (the f16 rounding itself, 0.955 of the bound; yardstick 1.1e-5), dqkv 1.56e-2
    # on values up to 7.6 (the bf16 rounding, 0.995; yardstick 8.4e-6); worst error / bound over the five shapes 0.986 / 0.998
    check(f"attn fwd S={S} N={N} out (f16)", o.float(), r64[0], r32[0], "f16")
    check(f"attn bwd S={S} N={N} dqkv (bf16)", dqkv.float(), r64[1], r32[1], "bf16")
    o2, dqkv2 = run_attn(qkv, dout, S, N)          # one wave per (sequence, head), no atomics: a second run gives the same bits
    assert torch.equal(o, o2) and torch.equal(dqkv, dqkv2)


def test_attn_short_other_operand_formats():
    """fp32 qkv with the f16 and the split-image output (the product path: the split-precision qkv GEMM leaves fp32) and bf16 qkv /
    bf16 output, at (65, 9)."""
    S, N = 65, 9
    qkv, dout, _, _ = attn_case(S, N)
    q32 = qkv.float() + 1e-4 * torch.from_numpy(synth.det_uniform("fpooltr/f32/noise", (S * N, 3 * C)))      # not representable in 16 bits
    r64, r32 = attn_reference(q32, dout, S, N)
    o, dqkv = run_attn(q32, dout, S, N)
    check("attn fwd fp32 qkv out (f16)", o.float(), r64[0], r32[0], "f16")
    check("attn bwd fp32 qkv dqkv (bf16)", dqkv.float(), r64[1], r32[1], "bf16")
    # the split-precision image [hi | lo | hi] of the same fp32 result (what the proj GEMM reads on the product path)
    img = torch.empty(S * N, 3 * C, dtype=F16, device=DEV)
    call("sed_attn_short_fwd", q32.to(DEV), img, S, N, HEADS, 2, 4)
    assert torch.equal(img[:, :C], o) and torch.equal(img[:, 2 * C:], o)
    check("attn fwd fp32 qkv out (split image, hi + lo)", img[:, :C].float() + img[:, C:2 * C].float(), r64[0], r32[0])
    qb = qkv.to(BF16)
    r64, r32 = attn_reference(qb, dout, S, N)
    o, dqkv = run_attn(qb, dout, S, N, out_dt=BF16)
    check("attn fwd bf16 qkv out (bf16)", o.float(), r64[0], r32[0], "bf16")
    check("attn bwd bf16 qkv dqkv (bf16)", dqkv.float(), r64[1], r32[1], "bf16")


def test_attn_short_known_answers():
    """q and k zero: every output row is the mean of that head's V rows.  N = 2 with k0 = k1: the rows mix 1/2, 1/2."""
    S, N = 5, 13
    qkv, dout = attn_inputs(S, N, tag="known")
    qkv[:, :2 * C] = 0
    o, _ = run_attn(qkv, dout, S, N)
    v = qkv[:, 2 * C:].contiguous()
    mean = {dt: v.to(dt).view(S, N, C).mean(1, keepdim=True).expand(S, N, C).reshape(S * N, C) for dt in (torch.float64, torch.float32)}
    check("attn known answer: uniform attention = mean of V", o.float(), mean[torch.float64], mean[torch.float32], "f16")
    S, N = 7, 2
    qkv, dout = attn_inputs(S, N, tag="known2")
    k = qkv.view(S, N, 3 * C)[:, :, C:2 * C]
    k[:, 1] = k[:, 0]
    o, _ = run_attn(qkv, dout, S, N)
    v = qkv[:, 2 * C:].contiguous()
    half = {dt: (0.5 * (v.to(dt).view(S, 2, C)[:, 0] + v.to(dt).view(S, 2, C)[:, 1])).unsqueeze(1).expand(S, 2, C).reshape(S * 2, C)
            for dt in (torch.float64, torch.float32)}
    check("attn known answer: equal keys mix 1/2, 1/2", o.float(), half[torch.float64], half[torch.float32], "f16")


def test_attn_short_sequence_isolation():
    """S = 3: replacing sequence 1's qkv and dout changes no bit of sequences 0 and 2, forward and backward, and does change sequence 1."""
    S, N = 3, 13
    qkv, dout = attn_inputs(S, N)
    o, d = run_attn(qkv, dout, S, N)
    q2, g2 = attn_inputs(S, N, tag="iso")
    qkv2, dout2 = qkv.clone(), dout.clone()
    qkv2[N:2 * N], dout2[N:2 * N] = q2[N:2 * N], g2[N:2 * N]
    o2, d2 = run_attn(qkv2, dout2, S, N)
    keep = torch.cat([torch.arange(0, N), torch.arange(2 * N, 3 * N)]).to(DEV)
    assert torch.equal(o[keep], o2[keep]) and torch.equal(d[keep], d2[keep])
    assert not torch.equal(o[N:2 * N], o2[N:2 * N]) and not torch.equal(d[N:2 * N], d2[N:2 * N])


# ------------------------------------------------------------------------------------------------ sequence build
def seq_chain(x, gamma, beta, tw, tb, Bx, tp, F):
    """passt_sed.py:202-214 + pooling.py:28-29: x [Bx, 2 + F tp, C] -> [Bx tp, 1 + F, C]."""
    n = Fn.layer_norm(x[:, 2:], (C,), gamma, beta, 1e-5).view(Bx, F, tp, C).transpose(1, 2).reshape(Bx * tp, F, C)
    tag = (tw.view(1, 1, C) + tb.view(1, 1, C)).expand(Bx * tp, 1, C)       # linear_emb(ones[S, 1, 1])
    return torch.cat([tag, n], dim=1)


def seq_inputs(Bx, tp, F):
    k = f"fpooltr/seq/{Bx}x{tp}x{F}"
    return dict(x=torch.from_numpy(synth.det_normal(k + "/x", (Bx, 2 + F * tp, C), 1.5)) + 0.3,
                gamma=torch.from_numpy(1.0 + 0.2 * synth.det_uniform(k + "/g", (C,))), beta=torch.from_numpy(0.1 * synth.det_uniform(k + "/b", (C,))),
                tw=torch.from_numpy(synth.det_uniform(k + "/tw", (C, 1))), tb=torch.from_numpy(0.1 * synth.det_uniform(k + "/tb", (C,))),
                dxs=torch.from_numpy(synth.det_uniform(k + "/dxs", (Bx * tp, 1 + F, C))))


@functools.lru_cache(maxsize=None)
def seq_reference(Bx, tp, F):
    out = {}
    for dt in (torch.float64, torch.float32):
        t = {k: v.to(dt).requires_grad_(k != "dxs") for k, v in seq_inputs(Bx, tp, F).items()}
        xs = seq_chain(t["x"], t["gamma"], t["beta"], t["tw"], t["tb"], Bx, tp, F)
        (xs * t["dxs"]).sum().backward()
        tok = t["x"].detach()[:, 2:].view(Bx, F, tp, C).transpose(1, 2).reshape(Bx * tp, F, C)
        out[dt] = dict(xs=xs.detach(), mean=tok.mean(-1), rstd=(tok.var(-1, unbiased=False) + 1e-5).rsqrt(), dx=t["x"].grad, dgamma=t["gamma"].grad,
                       dbeta=t["beta"].grad, dtag=t["tb"].grad, dtw=t["tw"].grad.view(C))
    return out[torch.float64], out[torch.float32]


def run_seq(t, Bx, tp, F):
    S, N = Bx * tp, 1 + F
    xs = torch.empty(S, N, C, device=DEV)
    mean, rstd = torch.empty(S * N, device=DEV), torch.empty(S * N, device=DEV)
    call("sed_fpool_seq_build_fwd", t["x"], t["gamma"], t["beta"], 1e-5, t["tw"], t["tb"], xs, mean, rstd, Bx, tp, F)
    dx = torch.full((Bx, 2 + F * tp, C), float("nan"), device=DEV)      # (written whole: no NaN may survive)
    dg, db, dtag = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    part = torch.empty(min((S * N + 3) // 4, 256) * 3 * C, device=DEV)
    call("sed_fpool_seq_build_bwd", t["dxs"], t["x"], mean, rstd, t["gamma"], dx, dg, db, dtag, part, part.numel(), Bx, tp, F)
    return xs, mean, rstd, dx, dg, db, dtag


@pytest.mark.parametrize("Bx,tp,F", SEQ_SHAPES)
def test_seq_build_vs_float64(Bx, tp, F):
    r64, r32 = seq_reference(Bx, tp, F)
    t = {k: v.to(DEV).contiguous() for k, v in seq_inputs(Bx, tp, F).items()}
    xs, mean, rstd, dx, dg, db, dtag = run_seq(t, Bx, tp, F)
    tag = f"seq_build Bx={Bx} tp={tp} F={F}"
    S, N = Bx * tp, 1 + F
    # measured at (3, 99, 8), error / yardstick (the bound is 8 x the yardstick): xs 6.6e-7 / 7.2e-7, mean 6.7e-8 / 6.6e-8, rstd 1.0e-7 / 7.4e-8,
    # dx 2.4e-7 / 1.9e-7, dgamma 4.2e-5 / 2.4e-5 (on sums up to 84), dbeta 5.0e-5 / 2.1e-5, dtag 1.5e-5 / 4.1e-6 (0.445 of the bound, the
    # worst of the four shapes); (1, 1, 12): dtag is one row, exact
    check(f"{tag} xs", xs, r64["xs"], r32["xs"])
    check(f"{tag} mean", mean.view(S, N)[:, 1:], r64["mean"], r32["mean"])
    check(f"{tag} rstd", rstd.view(S, N)[:, 1:], r64["rstd"], r32["rstd"])
    assert torch.equal(xs[:, 0], (t["tw"].view(C) + t["tb"]).expand(S, C))          # the tag row, bit for bit, in every sequence
    check(f"{tag} dx", dx, r64["dx"], r32["dx"])
    assert not dx[:, :2].any()              # cls / dist rows: exactly zero
    check(f"{tag} dgamma", dg, r64["dgamma"], r32["dgamma"])
    check(f"{tag} dbeta", db, r64["dbeta"], r32["dbeta"])
    check(f"{tag} dtag", dtag, r64["dtag"], r32["dtag"])
    check(f"{tag} dtag = d linear_emb.weight[:, 0]", dtag, r64["dtw"], r32["dtw"])
    again = run_seq(t, Bx, tp, F)           # fixed-order two-stage reductions, no atomics
    for nm, a, b in zip(("xs", "mean", "rstd", "dx", "dgamma", "dbeta", "dtag"), (xs, mean, rstd, dx, dg, db, dtag), again):
        assert torch.equal(a, b), (tag, nm)
    # the outputs accumulate (arena views): a second call into the same buffers doubles them; a frozen module passes no sinks
    call("sed_fpool_seq_build_bwd", t["dxs"], t["x"], mean, rstd, t["gamma"], None, dg, None, None, again[4].new_empty(256 * 3 * C), 256 * 3 * C, Bx, tp, F)
    assert torch.equal(dg, 2 * again[4]) and torch.equal(db, again[5])


# ------------------------------------------------------------------------------------------------ final norm of row 0
@pytest.mark.parametrize("S,N", NORM_SHAPES)
def test_rownorm_vs_float64(S, N):
    k = f"fpooltr/norm/{S}x{N}"
    inp = dict(xs=torch.from_numpy(synth.det_normal(k + "/x", (S, N, C), 2.0)) - 0.4, gamma=torch.from_numpy(1.0 + 0.2 * synth.det_uniform(k + "/g", (C,))),
               beta=torch.from_numpy(0.1 * synth.det_uniform(k + "/b", (C,))), dy=torch.from_numpy(synth.det_uniform(k + "/dy", (S, C))))
    ref = {}
    for dt in (torch.float64, torch.float32):
        t = {n: v.to(dt).requires_grad_(n != "dy") for n, v in inp.items()}
        y = Fn.layer_norm(t["xs"], (C,), t["gamma"], t["beta"], 1e-5)[:, 0]          # pooling.py:32-33
        (y * t["dy"]).sum().backward()
        ref[dt] = (y.detach(), t["xs"].grad, t["gamma"].grad, t["beta"].grad)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    t = {n: v.to(DEV).contiguous() for n, v in inp.items()}

    def run():
        pooled, mean, rstd = torch.empty(S, C, device=DEV), torch.empty(S, device=DEV), torch.empty(S, device=DEV)
        call("sed_fpool_rownorm_fwd", t["xs"], t["gamma"], t["beta"], 1e-5, pooled, mean, rstd, S, N)
        dxs = torch.full((S, N, C), float("nan"), device=DEV)
        dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        part = torch.empty(min((S + 3) // 4, 256) * 2 * C, device=DEV)
        call("sed_fpool_rownorm_bwd", t["dy"], t["xs"], mean, rstd, t["gamma"], dxs, dg, db, part, part.numel(), S, N)
        return pooled, dxs, dg, db
    pooled, dxs, dg, db = run()
    tag = f"rownorm S={S} N={N}"
    # measured at (1188, 9), error / yardstick: pooled 6.7e-7 / 6.5e-7, dxs 1.5e-7 / 1.6e-7, dgamma 5.5e-5 / 1.1e-5 (on sums up to 78, 0.604 of
    # the bound: the worst of the three shapes), dbeta 3.5e-5 / 1.1e-5
    check(f"{tag} pooled", pooled, r64[0], r32[0])
    check(f"{tag} dxs", dxs, r64[1], r32[1])
    assert not dxs[:, 1:].any()             # rows 1 .. F of the last block's output: exactly zero
    check(f"{tag} dgamma", dg, r64[2], r32[2])
    check(f"{tag} dbeta", db, r64[3], r32[3])
    for a, b in zip((pooled, dxs, dg, db), run()):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ model level
def mreport(name, err, extra=""):
    os.makedirs(LOGDIR, exist_ok=True)
    with open(MLOG, "a") as f:
        f.write(f"{name}: {err:.4e} {extra}\n")


def build_model(mlm=False, f_pool=FPOOL, decoder="transformerXL", qkv_gain=1.0, **kw):
    if mlm:
        kw["mlm_dict"] = dict(strategy="block", block_width=10, mask_rate=0.75, out_dim=768)
    net = PaSST_SED(passt_feature_layer=2, f_pool=f_pool, decode_ratio=10, at_adapter=True, decoder=decoder, decoder_layer_num=2,
                    decoder_pos_emd_len=1000, mlm=mlm, load_pretrained_model=False, encoder_depth=2, **kw)
    sd = synth.fpool_transformer_state_dict_np(tag="wft768", dec_layers=2, depth=12, mlm=mlm, qkv_gain=qkv_gain)
    if decoder == "conformer":
        sd.update({k: v for k, v in synth.conformer_state_dict_np(tag="wft768", dec_layers=2, depth=0, mlm=mlm).items() if k.startswith("decoder.")})
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


def _mel(tag, B=2):
    return torch.from_numpy(synth.det_uniform(f"{tag}/mel", (B, 128, 1000), -1.2, 1.2)).to(DEV)


def weighted_loss(tag, strong, weak, at):
    gs = torch.from_numpy(synth.det_uniform(f"{tag}/gs", tuple(strong.shape))).to(DEV)
    gw = torch.from_numpy(synth.det_uniform(f"{tag}/gw", tuple(weak.shape))).to(DEV)
    ga = torch.from_numpy(synth.det_uniform(f"{tag}/ga", tuple(at.shape))).to(DEV)
    return (strong * gs).sum() + (weak * gw).sum() + (at * ga).sum()


def check_posteriors(what, pairs):
    for nm, got, ref in pairs:
        e = maxerr(got, ref); mreport(f"{what} {nm} vs reference", e); print(f"{what} {nm}: {e:.3e}")
        assert e < 1e-3, (nm, e)


def check_loss_and_grads(what, net, loss, ref_loss, names, norms, loss_bound=2e-3, heads=None):
    """`heads` (the first 8 elements of every reference gradient): the direction check of the 26 new tensors.  A norm cannot see a gradient
    that points the wrong way; the elements can.  Their bound is not the norms' 3e-3: an element is a sum of products of bf16-rounded
    backward operands (2^-8 relative each, two or three per product), about 1.2e-2 of the terms' size without the averaging a norm over
    thousands of elements enjoys.  5e-2 of the largest of the 8 reference elements allows four times that and is twenty times below
    what a wrong sign, a transposed operand or a missing term gives (order 1)."""
    rel = abs(float(loss.detach()) - float(ref_loss)) / abs(float(ref_loss)); mreport(f"{what} loss rel", rel); print(f"{what} loss rel: {rel:.3e}")
    assert rel < loss_bound
    names = [str(n) for n in names]
    params = dict(net.named_parameters())
    got_names = {n for n, p in params.items() if p.grad is not None}
    assert got_names == set(names), (got_names ^ set(names))
    worst, worst_pool, fails = 0.0, 0.0, []
    for n, norm in zip(names, norms):
        r = abs(float(params[n].grad.double().norm()) - norm) / (norm + 1e-12)
        mreport(f"{what} grad {n}", r)
        worst = max(worst, r)
        if n.startswith("f_pool_module."):
            worst_pool = max(worst_pool, r)
        if not r < grad_tol(n, 3e-3):
            fails.append((n, r))
    if heads is not None:
        worst_head = 0.0
        for n, head in zip(names, heads):
            if n.startswith("f_pool_module."):
                k = min(8, params[n].grad.numel())
                h = maxerr(params[n].grad.reshape(-1)[:k], head[:k]) / (float(np.abs(head[:k]).max()) + 1e-12)
                mreport(f"{what} grad head {n}", h)
                worst_head = max(worst_head, h)
                if not h < 5e-2:
                    fails.append((n, "head", h))
        print(f"{what} worst element error of the new tensors' gradient heads: {worst_head:.3e} of the largest element")      # measured: 1.6e-2 finetune, 6.5e-3 MLM
    mreport(f"{what} worst grad-norm rel err", worst, f"f_pool_module={worst_pool:.3e}")
    print(f"{what} worst grad-norm rel err: {worst:.3e} (f_pool_module tensors: {worst_pool:.3e})")
    assert not fails, fails


def test_model_eval_vs_reference_golden(golden):
    """Eval-mode outputs with and without the pad mask and temperature, and with the sliding windows."""
    g = golden(TAG)
    assert float(g["strong_vs_uniform_attention_max"]) >= 20e-3 and float(g["strong_vs_zero_tag_max"]) >= 20e-3
    mel = _mel(TAG)
    net = build_model().eval()
    with torch.no_grad():
        strong, weak, other = net(mel, encoder_win=False, temp_w=1)
        pm = torch.zeros(2, 1000, dtype=torch.bool)
        pm[0, 900:] = True
        s2, w2, _ = net(mel, encoder_win=False, temp_w=0.5, pad_mask=pm.to(DEV))
        s3, w3, _ = net(mel, encoder_win=True, mix_rate=0.5, win_param=[512, 49], temp_w=1)
    check_posteriors("eval", (("strong", strong, g["strong"]), ("weak", weak, g["weak"]), ("at_out", other["at_out"], g["at_out"]),
                              ("strong_t05_pad", s2, g["strong_t05_pad"]), ("weak_t05_pad", w2, g["weak_t05_pad"]),
                              ("strong_win", s3, g["strong_win"]), ("weak_win", w3, g["weak_win"])))
    # measured: strong 3.3e-4, weak 6.1e-5, at_out 6.6e-5, strong_t05_pad 5.4e-4, weak_t05_pad 8.2e-5, strong_win 1.7e-4, weak_win 4.1e-5
    # (with plain f16 operands in evaluation too, measured during development: 4.8e-4, 1.8e-4, 6.6e-5, 8.6e-4, 2.5e-4, 3.4e-4, 1.9e-4); interp_s 1.5e-3, pooled_s 2.9e-3
    fbm = other["frame_before_mask"]
    e = maxerr(fbm[:, ::25, ::16], g["interp_s"]); mreport("eval interp_s", e); assert e < 2e-2
    # the module's own output (the stage's result, kept in the saved context of a forward that saves) against the strided probe of the
    # reference's forward hook; interp_s is a convex combination of these values, so its bound applies
    _, ctx = net.engine.forward(mel, save=True)
    e = maxerr(ctx["pooled"].reshape(2 * 99, 768)[::7, ::16], g["pooled_s"]); mreport("eval pooled_s", e); print(f"pooled_s: {e:.3e}"); assert e < 2e-2


def test_model_sharp_attention_vs_reference_golden(golden):
    """The same model with qkv at gain 1.6: sharp frequency attention.  The pooled frame is row 0 of the sequence, which sees the encoder's
    tokens only through the softmax; the sharper it is, the fewer rows it averages, and the rounding noise of the 16-bit encoder blocks,
    which mean pooling averages over 12 rows, comes through louder.  The 1e-3 contract was set behind mean pooling, so it does not
    carry over; what does is the reference's own behaviour: `noise_gain` in the fixture is how much further the REFERENCE moves `strong`
    under the same 3e-4 perturbation of out_norm's output with this module than with mean pooling on the same weights (three seeds each,
    float32 on the CPU; 3.43).  The posteriors are held to 1e-3 times that gain -- and the limitation is pinned: at this sharpness they do
    exceed 1e-3 at temperature 0.5."""
    g = golden(STAG)
    gain = float(g["noise_gain"])
    assert 1.0 < gain < 12 ** 0.5 * 1.5 and float(g["qkv_gain"]) == 1.6        # (no averaging at all would be sqrt(12) = 3.46)
    mel = _mel(STAG)
    net = build_model(qkv_gain=1.6).eval()
    with torch.no_grad():
        strong, weak, _ = net(mel, encoder_win=False, temp_w=1)
        pm = torch.zeros(2, 1000, dtype=torch.bool)
        pm[0, 900:] = True
        s2, w2, _ = net(mel, encoder_win=False, temp_w=0.5, pad_mask=pm.to(DEV))
    for nm, got, ref in (("strong", strong, g["strong"]), ("weak", weak, g["weak"]), ("strong_t05_pad", s2, g["strong_t05_pad"]),
                         ("weak_t05_pad", w2, g["weak_t05_pad"])):
        e = maxerr(got, ref); mreport(f"sharp attention {nm} vs reference", e, f"bound={1e-3 * gain:.3e}"); print(f"sharp attention {nm}: {e:.3e}")
        assert e < 1e-3 * gain, (nm, e, gain)          # measured: strong 1.1e-3, weak 2.3e-4, strong_t05_pad 2.1e-3, weak_t05_pad 3.1e-4 (bound 3.43e-3)


def test_model_finetune_gradients_vs_reference_golden(golden):
    g = golden(TAG)
    mel = _mel(TAG)
    net = build_model().train()
    strong, weak, other = net(mel, encoder_win=False, temp_w=1)
    loss = weighted_loss(TAG, strong, weak, other["at_out"])
    loss.backward()
    # measured: loss 1.0e-3 relative, worst gradient norm 7.6e-4 (one of the 26 new tensors)
    check_loss_and_grads("finetune", net, loss, g["ft_loss"], g["ft_grad_names"], g["ft_grad_norms"], heads=g["ft_grad_heads"])
    pn = dict(net.named_parameters())       # linear_emb is applied to 1: its weight column and its bias get the same gradient, bit for bit
    assert torch.equal(pn["f_pool_module.linear_emb.weight"].grad.view(-1), pn["f_pool_module.linear_emb.bias"].grad)


def test_model_gradients_through_windows_vs_reference_golden(golden):
    g = golden(TAG)
    mel = _mel(TAG)
    net = build_model().train()
    net._win_toffsets = g["win_toffsets"].tolist()
    strong, weak, other = net(mel, encoder_win=True, mix_rate=0.5, win_param=[512, 49], temp_w=1)
    net._win_toffsets = None
    check_posteriors("windows (train mode)", (("strong", strong, g["win_ft_strong"]),))
    loss = weighted_loss(TAG, strong, weak, other["at_out"])
    loss.backward()
    # measured: strong 4.2e-4, loss 3.5e-4 relative, worst gradient norm 2.2e-3 (a decoder tensor; the 26 new ones 7.0e-4)
    check_loss_and_grads("windows", net, loss, g["win_ft_loss"], g["win_ft_grad_names"], g["win_ft_grad_norms"])


def test_model_mlm_vs_reference_golden(golden):
    g = golden(TAG)
    mel = _mel(TAG)
    net = build_model(mlm=True).train()
    for p in net.backbone.parameters():
        p.requires_grad_(False)
    net._mlm_draws = dict(noise=torch.from_numpy(g["mlm_noise"]), probs=torch.from_numpy(g["mlm_probs"]), rand_idx=torch.from_numpy(g["mlm_rand_idx"]))
    pred, other = net(mel, encoder_win=False)
    assert np.array_equal(other["mask_id_seq"].cpu().numpy(), g["mlm_mask_ids"])
    e = maxerr(pred[:, ::25, ::16], g["mlm_pred_s"]); sc = float(np.abs(g["mlm_pred_s"]).max()); mreport("mlm pred", e, f"scale={sc:.2f}")
    print(f"mlm pred: {e:.3e} scale {sc:.2f}")
    ef = maxerr(other["frame_before_mask"][:, ::25, ::16], g["mlm_fbm_s"]); mreport("mlm frame_before_mask", ef); assert ef < 2e-2      # (interp_s's bound: the same quantity)
    assert e < 1e-3 * sc          # measured: 2.3e-3 on values up to 3.30 (7.1e-4 of scale); loss 4.5e-5, worst gradient norm 9.2e-4
    loss = torch.nn.functional.mse_loss(other["frame_before_mask"][other["mask_id_seq"]], pred[other["mask_id_seq"]])
    loss.backward()
    check_loss_and_grads("mlm", net, loss, g["mlm_loss"], g["mlm_grad_names"], g["mlm_grad_norms"], loss_bound=1e-4, heads=g["mlm_grad_heads"])


def test_model_frozen_module_vs_reference_golden(golden):
    """finetune1-style freezing: the pooling module, the context network and the encoder blocks are frozen; the gradient still flows through
    the frozen module to out_norm."""
    g = golden(TAG)
    mel = _mel(TAG)
    net = build_model().train()
    for k, p in net.named_parameters():
        p.requires_grad_(not (k.startswith(("f_pool_module.", "decoder.")) or (k.startswith("backbone.") and not k.startswith("backbone.norm."))))
    strong, weak, other = net(mel, encoder_win=False, temp_w=1)
    loss = weighted_loss(TAG, strong, weak, other["at_out"])
    loss.backward()
    # measured: loss 1.7e-4 relative, worst gradient norm 1.7e-4
    check_loss_and_grads("frozen module", net, loss, g["frozen_loss"], g["frozen_grad_names"], g["frozen_grad_norms"])
    params = dict(net.named_parameters())
    assert params["out_norm.weight"].grad is not None and float(params["out_norm.weight"].grad.abs().max()) > 0
    assert all(p.grad is None for n, p in params.items() if n.startswith("f_pool_module."))


def test_model_patchout_vs_reference_golden(golden):
    g = golden(PTAG)
    mel = _mel(PTAG)
    net = build_model(s_patchout_f=int(g["s_patchout_f"])).train()
    net._patchout_rows = [g["rows_global"].tolist()]
    strong, weak, other = net(mel, encoder_win=False, temp_w=1)
    check_posteriors("patchout 4", (("strong", strong, g["strong"]), ("weak", weak, g["weak"]), ("at_out", other["at_out"], g["at_out"])))
    loss = weighted_loss(PTAG, strong, weak, other["at_out"])
    loss.backward()
    # measured: strong 5.1e-4, weak 1.7e-4, at_out 1.0e-4, loss 2.0e-4 relative, worst gradient norm 1.4e-3 (the 26 new tensors 6.3e-4)
    check_loss_and_grads("patchout 4", net, loss, g["ft_loss"], g["ft_grad_names"], g["ft_grad_norms"])


def test_conformer_with_transformer_pooling_runs():
    """The pooling stage is independent of the context network: one forward and backward with decoder="conformer"."""
    net = build_model(decoder="conformer").train()
    strong, weak, other = net(_mel("fpooltr/conformer"), encoder_win=False, temp_w=1)
    weighted_loss("fpooltr/conformer", strong, weak, other["at_out"]).backward()
    assert all(bool(torch.isfinite(t).all()) for t in (strong, weak, other["at_out"]))
    params = dict(net.named_parameters())
    got = {n for n, p in params.items() if p.grad is not None}
    want = {n for n in params if not n.startswith("backbone.head")}
    assert got == want, got ^ want
    assert sum(n.startswith("f_pool_module.") for n in got) == 26 and sum(n.startswith("decoder.blocks.") for n in got) == 66
    assert all(bool(torch.isfinite(params[n].grad).all()) and float(params[n].grad.abs().max()) > 0 for n in got)


def _fwd_eval(net, mel):
    net.eval()
    with torch.no_grad():
        s, w, o = net(mel, encoder_win=False, temp_w=0.5)
    return torch.cat([s.reshape(-1), w.reshape(-1), o["at_out"].reshape(-1)]).clone()


WRITTEN = ("f_pool_module.frequency_transformer.0.attn.qkv.weight", "f_pool_module.frequency_transformer.1.mlp.fc1.weight",
           "f_pool_module.linear_emb.bias")


@pytest.mark.parametrize("how", ["mul_", "fused_adamw_ema"])
def test_weight_writes_show_in_next_forward(how):
    """In-place writes between two evaluations (plain `p.data.mul_(1.5)`; one FusedAdamWEMA step): the next forward equals a fresh model loaded
    with the written weights and differs from the first (the pattern of test_conformer_weight_writes_show_in_next_forward)."""
    from transformer4sed_amd.trainer import FusedAdamWEMA, get_params
    mel = _mel("fpooltr/writes")
    net = build_model()
    opt = None
    if how == "fused_adamw_ema":
        groups = get_params(net, {"encoder": {"lr": 5e-6, "weight_decay": 1e-4, "freeze_layer": 1, "step_lr": 4},
                                  "decoder": {"lr": 1e-3, "weight_decay": 1e-4}, "head": {"lr": 1e-4, "weight_decay": 1e-4}})
        opt = FusedAdamWEMA(net, groups)
    _fwd_eval(net, mel)
    before = _fwd_eval(net, mel)
    pn = dict(net.named_parameters())
    old = {n: pn[n].detach().clone() for n in WRITTEN}
    if how == "mul_":
        for n in WRITTEN:
            pn[n].data.mul_(1.5)
    else:
        gen = torch.Generator(device=DEV).manual_seed(3)
        arena = torch.zeros(opt.total, dtype=torch.float32, device=DEV)
        for n in WRITTEN:
            o, k = opt.offset[n]
            arena[o:o + k].copy_(torch.randn(k, generator=gen, device=DEV))
            pn[n].grad = arena[o:o + k].view(pn[n].shape)
        net._last_grad_arena = arena
        opt.step(None)
        opt.zero_grad()
    assert all(not torch.equal(old[n], pn[n].detach()) for n in WRITTEN)
    after = _fwd_eval(net, mel)
    fresh = build_model()
    fresh.load_state_dict({k: v.detach().clone() for k, v in net.state_dict().items()}, strict=True)
    want = _fwd_eval(fresh, mel)
    moved, err = maxerr(after, before), maxerr(after, want)
    mreport(f"weight write ({how})", err, f"moved={moved:.3e}")
    assert moved > 1e-4, moved
    assert err < 1e-6, err


def test_trainer_step_and_checkpoint(tmp_path):
    """Two optimisation steps of the mean-teacher trainer (finetune2: the teacher runs the sliding windows) at depth 2: every `f_pool_module.*`
    parameter moves, the teacher's copy is the EMA of the student's; a checkpoint loads back strictly and reproduces `strong` bit for bit."""
    import json
    import bench
    from transformer4sed_amd.scheduler import ExponentialDown, ema_alpha
    from transformer4sed_amd.trainer import FusedAdamWEMA, MatSedTrainer, get_params
    net = build_model()
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
    pool = [n for n, _ in net.named_parameters() if n.startswith("f_pool_module.")]
    assert len(pool) == 26
    tr.finetune_step(wav, labels.clone())        # (the first step's EMA factor is 0: the teacher becomes the student; check the second)
    s0 = {n: p.detach().clone() for n, p in net.named_parameters() if n in pool}
    e0 = {n: p.detach().clone() for n, p in ema.named_parameters() if n in pool}
    out = tr.finetune_step(wav, labels.clone())
    assert np.isfinite(float(out["loss_total"]))
    alpha = ema_alpha(sched.step_num, cfg["training"]["ema_factor"])
    assert 0 < alpha < 1
    sp, ep = dict(net.named_parameters()), dict(ema.named_parameters())
    for n in pool:
        assert not torch.equal(s0[n], sp[n].detach()), f"{n} did not move"
        want = alpha * e0[n] + (1 - alpha) * sp[n].detach()
        assert maxerr(ep[n], want) <= 1e-6 * max(1.0, float(want.abs().max())), n
    net.eval()
    mel = _mel("fpooltr/ckpt")
    with torch.no_grad():
        a, _, _ = net(mel, encoder_win=False)
    path = tmp_path / "fpooltr.pt"
    torch.save(net.state_dict(), path)
    fresh = build_model()
    fresh.load_state_dict(torch.load(path, map_location="cpu"), strict=True)
    fresh.eval()
    with torch.no_grad():
        b, _, _ = fresh(mel, encoder_win=False)
    assert torch.equal(a, b)


def test_mean_pool_issues_none_of_the_new_entry_points(monkeypatch):
    """A `mean_pool` model's forward (with windows) and backward launch none of the new kernels; the transformer pooling launches all six."""
    from transformer4sed_amd import engine, ops
    from transformer4sed_amd.engine import context, encoder, grads, heads, images, pooling
    seen = []
    real = ops.call

    def recording(name, *args):
        seen.append(name)
        return real(name, *args)
    for mod in (ops, engine, images, encoder, pooling, context, heads, grads):
        monkeypatch.setattr(mod, "call", recording)
    mel = _mel("fpooltr/launches")
    for f_pool, want in (("mean_pool", set()), (FPOOL, set(NEW_ENTRY_POINTS))):
        del seen[:]
        net = build_model(f_pool=f_pool).train()
        strong, weak, other = net(mel, encoder_win=True, mix_rate=0.5, win_param=[512, 49], temp_w=1)
        weighted_loss("fpooltr/launches", strong, weak, other["at_out"]).backward()
        assert "sed_layernorm_fwd" in seen and set(seen) & set(NEW_ENTRY_POINTS) == want, (f_pool, set(seen) & set(NEW_ENTRY_POINTS))
        assert ("sed_fpool_rows_fwd" in seen) == (f_pool == "mean_pool")
