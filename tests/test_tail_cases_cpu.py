"""tests/tail_cases.py proved on the CPU, before tests/test_gpu_tail_kernels.py holds the hardware to it:

1. every float64 reference agrees with float64 torch on small shapes (autograd over the plain formula, torch.nn.BCELoss / MSELoss,
   torch.optim.AdamW on a float64 parameter) to 1e-12 relative, apart from the documented NaN and empty-selection conventions;
2. the bounds are not vacuous: the same formula evaluated in plain fp32 torch stays inside every one of them;
3. every drop check holds: the reference with one named contribution removed differs from the full one by >= 10 bounds somewhere;
4. no pooled value of any head case lies within 1 % of a clamp edge, so no assertion depends on which side fp32 lands;
5. every case passes the argument checks of the entry points.
The two largest optimizer cases take part in 3 and 5 only (their 8.4 M-element references run on the device in the GPU test)."""
import functools

import pytest
import torch

import tail_cases as X
from tail_cases import D, F32, F64, H, U32

REL = 1e-12


def close64(a, b):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert bool((torch.isnan(a) == torch.isnan(b)).all())
    a, b = torch.nan_to_num(a), torch.nan_to_num(b)
    assert float((a - b).abs().max()) <= REL * max(float(b.abs().max()), 1e-300), float((a - b).abs().max())


def inside(got, ref, bound, what=""):
    """Plain fp32 result within the bound everywhere (NaN where the reference is NaN)."""
    got, ref = got.double(), ref.double()
    nan = torch.isnan(ref)
    assert bool((torch.isnan(got) == nan).all()), what
    ratio = float(torch.nan_to_num((got - ref).abs() / bound)[~nan].max()) if bool((~nan).any()) else 0.0
    assert ratio <= 1.0, (what, ratio)
    return ratio


def saw(drop, bound, what=""):
    s = X.sens(drop, bound)
    assert s >= X.SENS, (what, "the bound cannot see this contribution", s)


# ------------------------------------------------------------------------------------------------ head
def head_plain(x, W, b, temp, pm):
    """The head's forward in the dtype of its arguments: strong [B, C, T], weak, sums."""
    s = torch.sigmoid((x @ W.t() + b) / temp).masked_fill(pm.bool().unsqueeze(-1), 0.0).transpose(1, 2).contiguous()
    A, Bs = (s * s).sum(-1), s.sum(-1)
    return s, torch.clamp(A / Bs, 1e-7, 1.0), torch.stack([A, Bs], -1)


def head_bwd_plain(x, W, strong, sums, ds, dw, temp):
    s = strong.transpose(1, 2)
    g = ds.transpose(1, 2) if ds is not None else torch.zeros_like(s)
    if dw is not None:
        A, Bs = sums[..., 0].unsqueeze(1), sums[..., 1].unsqueeze(1)
        r = A / Bs
        g = g + dw.unsqueeze(1) * torch.where((r > 1e-7) & (r < 1.0), (2 * s * Bs - A) / (Bs * Bs), torch.zeros_like(s))
    dl = (g * s * (1 - s) / temp).reshape(-1, s.shape[-1])
    x2 = x.reshape(dl.shape[0], -1)
    return dl @ W, dl.t() @ x2, dl.sum(0)


@functools.lru_cache(maxsize=None)
def head_case(name):
    c = next(k for k in X.HEAD_CASES if k.name == name)
    i = X.head_inputs(c)
    strong, det, unit = X.head_fwd_ref(i["x"], i["W"], i["b"], c.temp, i["pm"])
    s32, w32, sums32 = head_plain(i["x"], i["W"], i["b"], f32t(c.temp), i["pm"])
    return c, i, strong, det, unit, s32, w32, sums32


def f32t(v):
    return torch.tensor(v, dtype=F32)


def test_head_reference_is_float64_autograd():
    c = next(k for k in X.HEAD_CASES if k.B == 2 and k.pad == "single")
    i = X.head_inputs(c)
    x, W, b = (i[k].double().requires_grad_(True) for k in ("x", "W", "b"))
    s, weak, sums = head_plain(x, W, b, c.temp, i["pm"])
    close64(X.head_fwd_ref(i["x"], i["W"], i["b"], c.temp, i["pm"])[0], s.detach())
    wk, sm, _, _ = X.head_pool_ref(s.detach())
    close64(wk, weak.detach()); close64(sm, sums.detach())
    for ds, dw in ((i["ds"], i["dw"]), (i["ds"], None), (None, i["dw"])):
        loss = (s * ds.double()).sum() if ds is not None else 0.0
        loss = loss + ((weak * dw.double()).sum() if dw is not None else 0.0)
        gx, gW, gb = torch.autograd.grad(loss, (x, W, b), retain_graph=True)
        r = X.head_bwd_ref(i["x"], i["W"], s.detach(), sums.detach(), ds, dw, c.temp)
        close64(r["dx"], gx.reshape(-1, D)); close64(r["dW"], gW); close64(r["db"], gb)


@pytest.mark.parametrize("case", X.HEAD_CASES, ids=[c.name for c in X.HEAD_CASES])
def test_head_bounds_hold_in_fp32_and_see_a_missing_contribution(case):
    c, i, strong, det, unit, s32, w32, sums32 = head_case(case.name)
    sb = X.head_strong_bound(det, unit)
    assert float(sb.max()) <= X.LEGACY_STRONG
    inside(s32, strong, sb, "strong")
    assert torch.equal(s32.transpose(1, 2)[i["pm"].bool()], torch.zeros(int(i["pm"].sum()), c.C))
    weak, sums, bw, bs = X.head_pool_ref(s32)
    assert float(torch.nan_to_num(bw).max()) <= X.LEGACY_STRONG
    inside(w32, weak, bw, "weak"); inside(sums32, sums, bs, "sums")
    # clamp edges: A / B of the float64 reference and of the fp32 values, 1 % away from 1e-7 and from 1
    for r in (X.head_ratio(X.head_pool_ref(strong)[1]), X.head_ratio(sums32)):
        r = r[~torch.isnan(r)]
        assert not bool((((r / 1e-7) - 1).abs() < 0.01).any()) and not bool(((r - 1).abs() < 0.01).any())
    if c.pad == "full":
        assert bool(torch.isnan(weak[0]).all()) and not bool(torch.isnan(weak[1:]).any())
    if c.shift:
        assert bool((X.head_ratio(sums32) < 0.5e-7).all()) and torch.equal(w32, torch.full_like(w32, 1e-7))
    # argument checks of the entry points
    assert c.C <= 16 and (not c.bwd or c.C == 10)
    if not c.bwd:
        return
    for form in X.HEAD_FORMS:
        ds = i["ds"] if form != "dweak" else None
        dw = i["dw"] if form != "dstrong" else None
        r = X.head_bwd_ref(i["x"], i["W"], s32, sums32, ds, dw, c.temp)
        gx, gW, gb = head_bwd_plain(i["x"], i["W"], s32, sums32, ds, dw, f32t(c.temp))
        for k, got in (("dx", gx), ("dW", gW), ("db", gb)):
            assert bool(torch.isfinite(r[k]).all())
            inside(got, r[k], r["b" + k[1:]], f"{form} {k}")
        if c.shift and form == "dweak":
            assert float(r["dx"].abs().max()) == 0.0            # the pooling's gate is closed
            continue
        for name, rows in X.head_drops(c.B, c.T).items():
            dv = X.head_drop_values(r, i["x"], rows)
            for k in ("dx", "dW", "db"):
                saw(dv[k], r["b" + k[1:]], f"{form} {k}: {name}")
        if c.pad == "full":
            assert float(r["dx"].view(c.B, c.T, D)[0].abs().max()) == 0.0


def test_head_second_pass_exists():
    big = [c for c in X.HEAD_CASES if c.B * c.T > X.HEAD_FIRST_PASS]
    assert big and all(c.B * c.T - X.HEAD_FIRST_PASS == 616 for c in big)
    assert {c.pad for c in big} == {"none", "single", "full"}


# ------------------------------------------------------------------------------------------------ attention pooling
def pool_plain(kv, q):
    B, N, _ = kv.shape
    k = kv[:, 2:, :D].reshape(B, N - 2, H, 64).permute(0, 2, 1, 3)
    v = kv[:, 2:, D:].reshape(B, N - 2, H, 64).permute(0, 2, 1, 3)
    p = torch.softmax((q.view(1, H, 1, 64) @ k.transpose(-2, -1)) * 0.125, -1)
    return p.reshape(B, H, N - 2), (p @ v).reshape(B, D)


def test_pool_reference_is_float64_autograd():
    for c in (k for k in X.POOL_CASES if k.B == 2 and k.P in (1, 5, 33) and not k.f16):
        i = X.pool_inputs(c)
        kv, q = i["kv"].double().requires_grad_(True), i["q"].double().requires_grad_(True)
        p, pooled = pool_plain(kv, q)
        r = X.pool_fwd_ref(i["kv"], i["q"])
        close64(r["p"], p.detach()); close64(r["pooled"], pooled.detach())
        gkv, gq = torch.autograd.grad(pooled, (kv, q), i["dout"].double())
        rb = X.pool_bwd_ref(i["kv"], i["q"], p.detach().reshape(c.B * H, c.P), i["dout"])
        close64(rb["dkv"], gkv); close64(rb["dq"], gq.view(-1))
        assert float(rb["dkv"][:, :2].abs().max()) == 0.0


@pytest.mark.parametrize("case", X.POOL_CASES, ids=[c.name for c in X.POOL_CASES])
def test_pool_bounds_hold_in_fp32_and_see_a_missing_contribution(case):
    c, i = case, X.pool_inputs(case)
    kv32 = i["kv"].float()
    r = X.pool_fwd_ref(i["kv"], i["q"])
    p32, pooled32 = pool_plain(kv32, i["q"])
    bp, bo = X.pool_probs_bound(r), X.pool_pooled_bound(r)
    assert float(bo.max()) <= X.LEGACY_POOLED
    inside(p32, r["p"], bp, "probs"); inside(pooled32, r["pooled"], bo, "pooled")
    tail = X.pool_drop_tokens(c.P)
    assert (c.P <= 28) == (len(tail) == c.P) and (len(X.pool_tail_tokens(c.P)) > 0) == (c.P != 256)
    saw(torch.einsum("bhp,bhpd->bhd", r["p"][:, :, tail], r["V"][:, :, tail]).reshape(c.B, D), bo, "pooled: tail tokens")
    # backward from the fp32 probs; the plain evaluation: autograd in fp32, rounded to bf16
    rb = X.pool_bwd_ref(i["kv"], i["q"], p32.reshape(c.B * H, c.P), i["dout"])
    kvg, qg = kv32.clone().requires_grad_(True), i["q"].clone().requires_grad_(True)
    gkv, gq = torch.autograd.grad(pool_plain(kvg, qg)[1], (kvg, qg), i["dout"])
    # (autograd differentiates its own fp32 softmax, not the saved probs: the two agree to the forward's bound, far inside dq's)
    inside(gq.view(-1), rb["dq"], rb["b_dq"] + 4 * U32 * rb["dq"].abs().max(), "dq")
    ours = (p32.unsqueeze(-1) * i["dout"].view(c.B, H, 1, 64)).permute(0, 2, 1, 3).reshape(c.B, c.P, D).to(torch.bfloat16)
    inside(ours.float(), rb["dkv"][:, 2:, D:], rb["b_dkv"][:, 2:, D:] + X.TINY, "dV as bf16")
    assert float(rb["b_dkv"][:, :2].max()) == 0.0
    if c.P > 1:                                                             # P = 1: softmax of one token, dS = 0, dq = 0
        saw(rb["dq_tail"], rb["b_dq"], "dq: tail tokens")
        saw(rb["dq_last_clip"], rb["b_dq"], "dq: last clip")
    else:
        assert float(rb["dq"].abs().max()) <= 1e-12


# ------------------------------------------------------------------------------------------------ small linear
@pytest.mark.parametrize("case", X.LIN_CASES, ids=[c.name for c in X.LIN_CASES])
def test_small_linear_reference_bounds_and_drops(case):
    c, i = case, X.lin_inputs(case)
    a, w, b = (i[k].double().requires_grad_(True) for k in ("a", "w", "b"))
    z = a @ w.t() + b
    out = torch.sigmoid(z) if c.act else z
    ref, det, unit = X.lin_fwd_ref(i["a"], i["w"], i["b"], c.act)
    close64(ref, out.detach())
    ga, gw, gb = torch.autograd.grad(out, (a, w, b), i["dout"].double())
    zero = torch.zeros_like
    r = X.lin_bwd_ref(i["a"], i["w"], out.detach(), i["dout"], c.act, zero(i["dw0"]), zero(i["db0"]))
    close64(r["da"], ga); close64(r["dW"], gw); close64(r["db"], gb)
    # fp32
    z32 = i["a"] @ i["w"].t() + i["b"]
    o32 = torch.sigmoid(z32) if c.act else z32
    inside(o32, ref, X.lin_out_bound(det, unit), "out")
    r = X.lin_bwd_ref(i["a"], i["w"], o32, i["dout"], c.act, i["dw0"], i["db0"])
    g32 = i["dout"] * o32 * (1 - o32) if c.act else i["dout"]
    inside(g32 @ i["w"], r["da"], r["b_da"], "da")
    inside(i["dw0"] + g32.t() @ i["a"], r["dW"], r["b_dW"], "dW")
    inside(i["db0"] + g32.sum(0), r["db"], r["b_db"], "db")
    saw(r["drop_da"], r["b_da"], "da: last output"); saw(r["drop_dW"], r["b_dW"], "dW: last row"); saw(r["drop_db"], r["b_db"], "db: last row")
    assert c.M > 0 and c.N > 0 and c.K > 0


# ------------------------------------------------------------------------------------------------ MLM masking
@pytest.mark.parametrize("case", X.MLM_CASES, ids=[c.name for c in X.MLM_CASES])
def test_mlm_reference_bounds_and_drops(case):
    c, i = case, X.mlm_inputs(case)
    act, src = i["action"], i["src"]
    assert int(src.min()) >= 0 and int(src.max()) < c.rows and int(act.max()) <= 2
    x, tok = i["x"].double().requires_grad_(True), i["tok"].double().requires_grad_(True)
    out = X.mlm_fwd_ref(x, tok, act, src)
    assert torch.equal(out.detach().float(), X.mlm_fwd_ref(i["x"], i["tok"], act, src))
    r = X.mlm_bwd_ref(i["dout"], act, src)
    gx, gt = torch.autograd.grad(out, (x, tok), i["dout"].double(), allow_unused=True)
    close64(r["dx"], gx)
    close64(r["dtok"], gt if gt is not None else torch.zeros(D, dtype=F64))
    # a copy of a masked or copied row takes the ORIGINAL row
    two = (act == 2).nonzero().view(-1)
    if len(two):
        assert torch.equal(out.detach()[two].float(), i["x"][src.long()[two]])
    if c.kind == "random":
        assert int(act[1]) == 1 and int(src[c.rows - 1]) == 1 and int(act[2]) == 2 and int(act[int(src[2])]) == 2
        if c.rows > X.MLM_FIRST_PASS_ROWS:
            assert src[0] > X.MLM_FIRST_PASS_ROWS - 1 and src[c.rows - 1] < X.MLM_FIRST_PASS_ROWS - 1
    # fp32
    d = i["dout"]
    dx32 = torch.zeros_like(d)
    dx32[act == 0] = d[act == 0]
    dx32.index_add_(0, src.long()[act == 2], d[act == 2])
    inside(dx32, r["dx"], r["b_dx"], "dx"); inside(d[act == 1].sum(0), r["dtok"], r["b_tok"], "dtoken")
    if c.kind == "none":
        assert float(r["dtok"].abs().max()) == 0.0 and torch.equal(r["dx"].float(), d)
    if bool((act == 1).any()):
        saw(r["drop_tok"], r["b_tok"], "dtoken: rows past the first pass")
    if c.kind == "hot":
        assert int(r["cnt"][7]) == 501
        saw(r["drop_dx"], r["b_dx"], "dx: copies past the first pass")
    if c.kind == "all":
        assert not bool((act == 0).any())


# ------------------------------------------------------------------------------------------------ masked MSE
@pytest.mark.parametrize("case", X.MSE_CASES, ids=[c.name for c in X.MSE_CASES])
def test_mse_reference_bounds_and_drops(case):
    c, i = case, X.mse_inputs(case)
    r = X.mse_ref(i["pred"], i["target"], i["mask"])
    m = i["mask"].bool()
    p32, t32 = i["pred"].clone().requires_grad_(True), i["target"].clone().requires_grad_(True)
    if c.mask == "none":
        assert r["n"] == 0 and float(r["loss"]) == 0.0 and float(r["dpred"].abs().max()) == 0.0
        return
    p, t = i["pred"].double().requires_grad_(True), i["target"].double().requires_grad_(True)
    loss = torch.nn.functional.mse_loss(t[m], p[m])
    gp, gt = torch.autograd.grad(loss, (p, t))
    close64(r["loss"].view(1), loss.detach().view(1)); close64(r["dpred"], gp); close64(-r["dpred"], gt)
    l32 = torch.nn.functional.mse_loss(t32[m], p32[m])
    g32, = torch.autograd.grad(l32, p32)
    inside(l32.detach().view(1), r["loss"].view(1), r["b_loss"].view(1), "loss"); inside(g32, r["dpred"], r["b_d"], "dpred")
    assert float(r["dpred"][~m].abs().max()) == 0.0 if bool((~m).any()) else True
    saw(r["drop"].view(1), r["b_loss"].view(1), "loss: second pass / last masked row")
    assert r["n"] > 0                                                       # the host-count form needs n_masked_rows > 0
    if c.mask == "late":
        assert not bool(m[:X.MSE_FIRST_PASS].any()) and bool(m[X.MSE_FIRST_PASS:].all())


# ------------------------------------------------------------------------------------------------ losses
@functools.lru_cache(maxsize=None)
def loss_inp(B, C, T):
    return X.loss_inputs(B, C, T)


def loss_plain(inp, c, w=X.LOSS_W, dt=F32):
    """The six terms with torch.nn.BCELoss / MSELoss and autograd, in dtype dt.  -> outs (7), grads (3)."""
    ss, sw, sa = (inp[k].to(dt).requires_grad_(True) for k in ("ss", "sw", "sa"))
    ts, ta, y, yw = (inp[k].to(dt) for k in ("ts", "ta", "y", "yw"))
    bce, mse = torch.nn.BCELoss(), torch.nn.MSELoss()
    ws = slice(c.weak_lo, c.weak_lo + c.weak_n)
    nan = torch.tensor(float("nan"), dtype=dt)
    ww, wwc, wat, wc = (float(torch.tensor(w[k], dtype=F32)) for k in ("w_weak", "w_weak_cons", "w_at", "w_cons"))
    l_s = bce(ss[:c.strong_n], y[:c.strong_n]) if c.strong_n else None
    l_w, l_a = (bce(sw[ws], yw[ws]), bce(sa[ws], yw[ws])) if c.weak_n else (None, None)
    lc_s, lc_w, lc_a = mse(ss, ts), mse(sw, ta), mse(sa, ta)
    fin = (lc_s + wwc * lc_w + wat * lc_a) * wc + (l_s if l_s is not None else 0.0) + (ww * l_w + wat * l_a if l_w is not None else 0.0)
    grads = torch.autograd.grad(fin, (ss, sw, sa))
    total = fin if (l_s is not None and l_w is not None) else nan
    outs = [total] + [t if t is not None else nan for t in (l_s, l_w, l_a)] + [lc_s, lc_w, lc_a]
    return [o.detach() for o in outs], grads


@pytest.mark.parametrize("case", X.LOSS_CASES, ids=[c.name for c in X.LOSS_CASES])
def test_loss_reference_bounds_and_drops(case):
    c = case
    assert X.loss_args_ok(c)
    inp = loss_inp(c.B, c.C, c.T)
    r = X.loss_ref(inp, c)
    small = c.B * c.C * c.T <= 2000
    if small:                                                               # 1: float64 torch modules
        o64, g64 = loss_plain(inp, c, dt=F64)
        for k in range(7):
            close64(r["outs"][k][0].view(1), o64[k].view(1))
        for (g, _), want in zip(r["grads"], g64):
            close64(g, want)
    o32, g32 = loss_plain(inp, c)
    for k in range(7):
        v, det, unit = r["outs"][k]
        if bool(torch.isnan(v)):
            assert bool(torch.isnan(o32[k])) and ((k in (0, 1) and c.strong_n == 0) or (k in (0, 2, 3) and c.weak_n == 0))
            continue
        b = X.loss_bound(v, det, unit)
        assert float(b) <= X.LEGACY_LOSS_REL * max(1.0, abs(float(v))) + X.TINY
        inside(o32[k].view(1), v.view(1), b.view(1), f"out[{k}]")
    for k, ((g, b), got) in enumerate(zip(r["grads"], g32)):
        assert bool(torch.isfinite(g).all())
        assert float(b.max()) <= X.LEGACY_GRAD_REL * max(1.0, float(g.abs().max()))
        inside(got, g, b, f"grad[{k}]")
    for (k, name), drop in r["drops"].items():
        v, det, unit = r["sums"][k]
        if float(drop) == 0.0:
            assert (k == 0 and c.strong_n < c.B) or (k in (1, 2) and c.weak_lo + c.weak_n < c.B), (k, name)   # the clip is not in the selection
            continue
        saw(drop.view(1), X.loss_bound(v, det, unit).view(1), f"sums[{k}]: {name}")


def test_loss_cases_reach_every_second_path():
    n = [c.B * c.C * c.T for c in X.LOSS_CASES]
    assert max(n) > 1024 * 1024 and X.loss_blocks(max(n)) == 1024
    assert any(c.B * c.C > 256 for c in X.LOSS_CASES)
    assert any(c.weak_lo != c.strong_n for c in X.LOSS_CASES) and any(c.weak_n == 0 for c in X.LOSS_CASES) and any(c.strong_n == 0 for c in X.LOSS_CASES)
    inp = loss_inp(2, 10, 7)
    assert float(inp["ss"].min()) == 0.0 and float(inp["ss"].max()) == 1.0 and bool((inp["ss"] == X.ONE_M).any())


# ------------------------------------------------------------------------------------------------ AdamW + EMA
def test_adam_reference_is_torch_adamw_in_float64():
    i = X.adam_inputs(64)
    p = torch.nn.Parameter(i["p"].double())
    lr, wd = X.f32(1e-3), X.f32(1e-4)
    opt = torch.optim.AdamW([p], lr=lr, betas=(X.f32(X.BETA1), X.f32(X.BETA2)), eps=X.f32(X.EPS), weight_decay=wd)
    mine = (i["p"].double(), torch.zeros(64, dtype=F64), torch.zeros(64, dtype=F64), i["ema"].double())
    for step in (1, 2, 3):
        g = i["g"].double() * step
        p.grad = g.clone()
        opt.step()
        alpha = X.f32(min(1 - 1 / (step + 1), 0.999))
        want_ema = alpha * mine[3] + (1 - alpha) * p.detach()
        mine, _ = X.adam_ref(mine[0], g, mine[1], mine[2], mine[3], 1e-3, 1e-4, step, alpha)
        close64(mine[0], p.detach()); close64(mine[3], want_ema)
        st = opt.state[p]
        close64(mine[1], st["exp_avg"]); close64(mine[2], st["exp_avg_sq"])


def adam_plain(p, g, m, v, ema, lr, wd, step, alpha, b1=X.BETA1, b2=X.BETA2, eps=X.EPS):
    t = lambda s: torch.tensor(s, dtype=F32)
    lr, wd, b1, b2, eps, alpha = (t(s) for s in (lr, wd, b1, b2, eps, alpha))
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    p = p * (1 - lr * wd)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - (lr / bc1) * (m / (torch.sqrt(v) / torch.sqrt(bc2) + eps))
    return p, m, v, ema * alpha + p * (1 - alpha)


@pytest.mark.parametrize("n", [n for n in X.ADAM_N if n < X.ADAM_FIRST_PASS])
@pytest.mark.parametrize("lr,wd", X.ADAM_HYPER)
def test_adam_bounds_hold_in_fp32(n, lr, wd):
    i = X.adam_inputs(n)
    for step in X.ADAM_STEPS:
        for alpha in X.ADAM_ALPHAS:
            ref, bound = X.adam_ref(i["p"], i["g"], i["m"], i["v"], i["ema"], lr, wd, step, alpha)
            got = adam_plain(i["p"], i["g"], i["m"], i["v"], i["ema"], lr, wd, step, alpha)
            for k in range(4):
                inside(got[k], ref[k], bound[k], f"step {step} alpha {alpha} [{k}]")
            z = i["zero"]
            assert float(ref[1][z].abs().max()) == 0.0 and float(ref[2][z].abs().max()) == 0.0
            assert torch.equal(ref[0][z], i["p"].double()[z] * (1.0 - X.f32(lr) * X.f32(wd)))          # only decay
            if lr == 0.0:
                assert torch.equal(ref[0], i["p"].double()) and not torch.equal(ref[1], i["m"].double())
            if alpha == 1.0:
                assert torch.equal(ref[3], i["ema"].double())
            if alpha == 0.0:
                assert torch.equal(ref[3], ref[0])


def test_adam_sizes_and_second_pass_drop():
    assert all(n % 4 == 0 for n in X.ADAM_N) and 6 % 4 != 0
    n = X.ADAM_N[-1]
    assert n - X.ADAM_FIRST_PASS == 64 and X.ADAM_N[-2] == X.ADAM_FIRST_PASS
    i = X.adam_inputs(n)
    tail = {k: v[X.ADAM_FIRST_PASS:] for k, v in i.items()}
    mag = i["g"].abs()
    assert float(mag[mag > 0].min()) >= 1e-6 and float(mag.max()) <= 1e2 and float(i["v"].min()) >= 0.0
    for lr, wd in X.ADAM_HYPER:
        ref, bound = X.adam_ref(tail["p"], tail["g"], tail["m"], tail["v"], tail["ema"], lr, wd, 10, 0.999)
        old = (tail["p"], tail["m"], tail["v"], tail["ema"])
        for k in range(4):                                                  # the second pass left undone: the state stays what it was
            if k == 0 and lr == 0.0:
                continue
            saw(ref[k] - old[k].double(), bound[k], f"second float4 pass, lr {lr} [{k}]")
