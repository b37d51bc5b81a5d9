"""The kernels every training step ends in -- head, attention pooling, small linear, MLM masking, masked MSE, the mean-teacher losses,
AdamW + EMA -- past their first grid pass and in every calling form, against the float64 references of tests/tail_cases.py (need an
MI355X).  tests/test_tail_cases_cpu.py proves those references, and that every bound used here holds for a plain fp32 evaluation and
can see a missing row block, grid pass or clip; the drop checks are repeated here next to each assertion on a sum, on the reference
built from what the kernel saved.

Each kernel runs once per case (memoised); every assertion reads the stored result.  The measured worst error, error / bound and the
constants K_EXP / K_LOG the measurements ask for go to tail_kernel_errors.log under SED_TEST_LOG_DIR, else test_logs/."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import tail_cases as X  # noqa: E402
from tail_cases import D, H, U32  # noqa: E402
from transformer4sed_amd._lib import SedHipError  # noqa: E402
from transformer4sed_amd.ops import call  # noqa: E402

DEV = "cuda"
LOG = os.path.join(os.environ.get("SED_TEST_LOG_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_logs"),
                   "tail_kernel_errors.log")
NAN = float("nan")
_MEMO = {}


def report(line):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(line + "\n")


def dev(d):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


def nans(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def zeros(*shape):
    return torch.zeros(*shape, device=DEV)


def check(name, got, ref, bound, drops=()):
    """|got - ref| <= bound everywhere (NaN exactly where the reference has one), nothing left of a NaN prefill, and every named
    contribution in `drops` moves the reference by >= 10 bounds somewhere.  -> worst err / bound."""
    got, ref = got.double(), ref.double()
    nan = torch.isnan(ref)
    assert bool((torch.isnan(got) == nan).all()), (name, "NaN pattern differs (an element was not written, or a NaN leaked)")
    err = torch.nan_to_num((got - ref).abs())
    ratio = float(torch.nan_to_num(err / bound).max())
    report(f"{name}: max_abs_err={float(err.max()):.4e} worst err/bound={ratio:.3f} bound_max={float(torch.nan_to_num(bound).max()):.3e}")
    assert ratio <= 1.0, (name, ratio)
    for what, drop in drops:
        s = X.sens(drop, bound)
        assert s >= X.SENS, (name, what, "the bound cannot see this contribution", s)
    return ratio


def needed_k(name, got, ref, det, unit):
    """The constant the measurement asks of an intrinsic's error model: max (|err| - det) / (u unit)."""
    err = torch.nan_to_num((got.double() - ref).abs())
    live = unit > 0
    if bool(live.any()):                                # (negative: the model of everything around the intrinsic covers the error alone)
        report(f"{name}: intrinsic constant needed={float(((err - det)[live] / (U32 * unit[live])).max()):.3f}")


def case_ids(cases):
    return [c.name for c in cases]


# ================================================================================================ SED head
def run_head(case):
    if ("head", case.name) in _MEMO:
        return _MEMO[("head", case.name)]
    c, i = case, dev(X.head_inputs(case))
    B, T, C = c.B, c.T, c.C
    pm = None if c.pad == "none" else i["pm"]
    strong, weak, sums = nans(B, C, T), nans(B, C), nans(B, C, 2)
    call("sed_head_fwd", i["x"], i["W"], i["b"], c.temp, pm, strong, weak, sums, B, T, C)
    r = dict(i=i, strong=strong, weak=weak, sums=sums, bwd={})
    if c.bwd:
        for form in X.HEAD_FORMS:
            ds = i["ds"] if form != "dweak" else None
            dw = i["dw"] if form != "dstrong" else None
            dx, dW, db = nans(B, T, D), zeros(C, D), zeros(C)
            call("sed_head_bwd", i["x"], i["W"], strong, sums, ds, dw, c.temp, dx, dW, db, B, T, C)
            r["bwd"][form] = (dx, dW, db)
        dx2 = nans(B, T, D)
        call("sed_head_bwd", i["x"], i["W"], strong, sums, i["ds"], i["dw"], c.temp, dx2, None, None, B, T, C)
        r["dx_only"] = dx2
        r["dW0"], r["db0"] = 0.1 * X.randn(C, D, seed=77).to(DEV), 0.1 * X.randn(C, seed=78).to(DEV)
        dW, db = r["dW0"].clone(), r["db0"].clone()
        call("sed_head_bwd", i["x"], i["W"], strong, sums, i["ds"], i["dw"], c.temp, nans(B, T, D), dW, db, B, T, C)
        r["acc"] = (dW, db)
    torch.cuda.synchronize()
    _MEMO[("head", case.name)] = r
    return r


@pytest.mark.parametrize("case", X.HEAD_CASES, ids=case_ids(X.HEAD_CASES))
def test_head_forward_vs_float64(case):
    """strong against sigmoid((x W^T + b) / temp) in float64 with the bound of tail_cases.head_fwd_ref (at most 1.3e-5, never above the
    2e-5 of test_gpu_kernels.py); masked frames exactly 0; weak and the saved sums against the float64 pooling of the kernel's own
    strong (bound (2 kappa + 4) u weak, kappa = ceil(T / 256) + 9: at most 1.7e-6); NaN for the clip whose every frame is padded and
    for no other; weak == 1e-7 in the low-bias case.  Measured worst err / bound: 0.43 on strong (2.3e-7 absolute; K_EXP needed: -12.7,
    see tail_cases.K_EXP), 0.13 on weak, 0.18 on the sums."""
    c, r = case, run_head(case)
    i = r["i"]
    ref, det, unit = X.head_fwd_ref(i["x"], i["W"], i["b"], c.temp, i["pm"])
    needed_k(f"head {c.name} strong", r["strong"], ref, det, unit)
    check(f"head {c.name} strong", r["strong"], ref, X.head_strong_bound(det, unit))
    masked = i["pm"].bool().unsqueeze(1).expand(c.B, c.C, c.T)
    assert float(r["strong"][masked].abs().max() if bool(masked.any()) else 0.0) == 0.0
    weak, sums, bw, bs = X.head_pool_ref(r["strong"])
    check(f"head {c.name} weak", r["weak"], weak, bw)
    check(f"head {c.name} sums", r["sums"], sums, bs)
    if c.pad == "full":
        assert bool(torch.isnan(r["weak"][0]).all()) and not bool(torch.isnan(r["weak"][1:]).any())
    if c.shift:
        assert torch.equal(r["weak"], torch.full_like(r["weak"], 1e-7))


BWD_CASES = [c for c in X.HEAD_CASES if c.bwd]


@pytest.mark.parametrize("form", X.HEAD_FORMS)
@pytest.mark.parametrize("case", BWD_CASES, ids=case_ids(BWD_CASES))
def test_head_backward_vs_float64(case, form):
    """dx, dW, db from the kernel's own strong / sums against the float64 closed form, bounds of tail_cases.head_bwd_ref (dx: 20 u
    sum_c |dlogit_c W_c|; dW / db: (rows per wave + 13) u sum|terms| + the chain over the 256 workgroups), with both gradients, dstrong
    alone and dweak alone.  Every sum carries its drop checks: a 16-row block past the first grid pass, the whole second pass (616
    rows at B T = 17000), the last clip.  A fully padded clip leaves dW / db / dx finite and its own dx rows exactly 0; the low-bias case
    closes the pooling's gate (dweak alone gives exact zeros).  Measured worst err / bound: 0.26 on dx, 0.10 on dW, 0.06 on db.  (With the
    dW sweep of a scratch build stopped after the first grid pass, the 17000-row cases miss dW's bound 2000 to 2700 times over.)"""
    c, r = case, run_head(case)
    i = r["i"]
    ds = i["ds"] if form != "dweak" else None
    dw = i["dw"] if form != "dstrong" else None
    ref = X.head_bwd_ref(i["x"], i["W"], r["strong"], r["sums"], ds, dw, c.temp)
    dx, dW, db = r["bwd"][form]
    gate_closed = bool(c.shift) and form == "dweak"
    drops = {k: [] for k in ("dx", "dW", "db")}
    if not gate_closed:
        for name, rows in X.head_drops(c.B, c.T).items():
            dv = X.head_drop_values(ref, i["x"], rows)
            for k in drops:
                drops[k].append((name, dv[k]))
    for k, got in (("dx", dx.view(-1, D)), ("dW", dW), ("db", db)):
        assert bool(torch.isfinite(got).all()), k
        check(f"head {c.name} {form} {k}", got, ref[k], ref["b" + k[1:]], drops[k])
    rows_masked = i["pm"].bool().view(-1)
    if bool(rows_masked.any()):
        assert float(dx.view(-1, D)[rows_masked].abs().max()) == 0.0
    if gate_closed:
        assert float(dx.abs().max()) == 0.0 and float(dW.abs().max()) == 0.0


@pytest.mark.parametrize("case", BWD_CASES, ids=case_ids(BWD_CASES))
def test_head_backward_forms(case):
    """dW == db == NULL: dx is bit-identical to the full call.  Accumulation into non-zero dW / db: the float64 sum of what was there
    and the reference, the bound widened by the chain's adds onto the initial value (workgroups u |dW0|) and one rounding of the
    result.  Measured worst err / bound: 0.46 on dW, 0.22 on db."""
    c, r = case, run_head(case)
    i = r["i"]
    assert torch.equal(r["dx_only"], r["bwd"]["both"][0])
    ref = X.head_bwd_ref(i["x"], i["W"], r["strong"], r["sums"], i["ds"], i["dw"], c.temp)
    nwg = int(X.head_wg_of_rows(c.B * c.T).max()) + 1
    for k, got, base in (("dW", r["acc"][0], r["dW0"]), ("db", r["acc"][1], r["db0"])):
        want = base.double() + ref[k]
        check(f"head {c.name} accumulate {k}", got, want, ref["b" + k[1:]] + U32 * (nwg * base.double().abs() + want.abs()))


def test_head_argument_errors_write_nothing():
    """C = 17 for the forward and C != 10 for the backward come back as the argument error and leave every output as it was."""
    B, T = 2, 15
    x, pm = torch.randn(B, T, D, device=DEV), None
    for C, fwd in ((17, True), (9, False), (16, False)):
        W, b = torch.randn(C, D, device=DEV), torch.randn(C, device=DEV)
        outs = [nans(B, C, T), nans(B, C), nans(B, C, 2)] if fwd else [nans(B, T, D), nans(C, D), nans(C)]
        with pytest.raises(SedHipError, match="bad argument"):
            if fwd:
                call("sed_head_fwd", x, W, b, 1.0, pm, *outs, B, T, C)
            else:
                call("sed_head_bwd", x, W, torch.rand(B, C, T, device=DEV), torch.rand(B, C, 2, device=DEV), torch.randn(B, C, T, device=DEV),
                     torch.randn(B, C, device=DEV), 1.0, *outs, B, T, C)
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(o).all()) for o in outs)


# ================================================================================================ attention pooling
def run_pool(case):
    if ("pool", case.name) in _MEMO:
        return _MEMO[("pool", case.name)]
    c, i = case, dev(X.pool_inputs(case))
    B, N = c.B, c.P + 2
    pooled, probs, pooled2 = nans(B, D), nans(B * H, c.P), nans(B, D)
    call("sed_attnpool_fwd", i["kv"], i["q"], pooled, probs, B, N, H, c.f16)
    call("sed_attnpool_fwd", i["kv"], i["q"], pooled2, None, B, N, H, c.f16)
    dkv, dq = nans(B, N, 2 * D, dtype=torch.bfloat16), zeros(D)
    call("sed_attnpool_bwd", i["kv"], i["q"], probs, i["dout"], dkv, dq, B, N, H, c.f16)
    torch.cuda.synchronize()
    _MEMO[("pool", case.name)] = dict(i=i, pooled=pooled, probs=probs, pooled2=pooled2, dkv=dkv, dq=dq)
    return _MEMO[("pool", case.name)]


@pytest.mark.parametrize("case", X.POOL_CASES, ids=case_ids(X.POOL_CASES))
def test_attnpool_forward_vs_float64(case):
    """probs and the pooled vector against the float64 softmax over tokens 2..N-1 of the 16-bit K / V the kernel reads, at every P
    around the unrolled loop's edges (t + 28 < P) and the 256-thread score loop, in bf16 and f16.  Bounds: tail_cases.pool_fwd_ref (the
    pooled vector's is at most 3.8e-5, never above the 1e-4 of test_gpu_kernels.py); the drop check removes the tail tokens after the
    unrolled loop (the loop's last pass at P = 256, which leaves no tail).  probs == NULL gives the same pooled bits.  Measured worst
    err / bound: 0.08 on probs (K_EXP needed: -12.0), 0.03 on the pooled vector."""
    c, r = case, run_pool(case)
    i = r["i"]
    ref = X.pool_fwd_ref(i["kv"], i["q"])
    got_p = r["probs"].view(c.B, H, c.P)
    needed_k(f"attnpool {c.name} probs", got_p / ref["p"].clamp(min=1e-300), torch.ones_like(ref["p"]), ref["det"], ref["unit"])
    check(f"attnpool {c.name} probs", got_p, ref["p"], X.pool_probs_bound(ref))
    tail = X.pool_drop_tokens(c.P)
    drop = torch.einsum("bhp,bhpd->bhd", ref["p"][:, :, tail], ref["V"][:, :, tail]).reshape(c.B, D)
    check(f"attnpool {c.name} pooled", r["pooled"], ref["pooled"], X.pool_pooled_bound(ref), [("tail tokens", drop)])
    assert torch.equal(r["pooled"], r["pooled2"])


@pytest.mark.parametrize("case", X.POOL_CASES, ids=case_ids(X.POOL_CASES))
def test_attnpool_backward_vs_float64(case):
    """dkv element by element within half an ulp of bf16 of the float64 value (+ the fp32 error of the value before it is rounded),
    from the kernel's own probs; rows 0-1 exactly zero and no other row left at the NaN prefill; dq within the bound of
    tail_cases.pool_bwd_ref, whose drop checks remove the tail tokens and the last clip (B = 32: the atomic chain over the batch).
    Measured worst err / bound: 1.00 on dkv -- by construction: round-to-nearest reaches half an ulp, and the bound is nothing else --
    and 0.02 on dq."""
    c, r = case, run_pool(case)
    i = r["i"]
    ref = X.pool_bwd_ref(i["kv"], i["q"], r["probs"], i["dout"])
    assert float(r["dkv"][:, :2].float().abs().max()) == 0.0
    check(f"attnpool {c.name} dkv", r["dkv"].float(), ref["dkv"], ref["b_dkv"] + X.TINY)
    drops = [("tail tokens", ref["dq_tail"]), ("last clip", ref["dq_last_clip"])] if c.P > 1 else []
    check(f"attnpool {c.name} dq", r["dq"], ref["dq"], ref["b_dq"], drops)


# ================================================================================================ small linear
@pytest.mark.parametrize("case", X.LIN_CASES, ids=case_ids(X.LIN_CASES))
def test_small_linear_vs_float64(case):
    """act(a W^T + b) and its three gradients (from the kernel's own `out`, accumulating into non-zero dW / db) at the shapes the model
    uses and at one with N, K no multiple of anything.  Drop checks: the last row for dW / db, the last output for da.  Measured worst
    err / bound: 0.14 on out (K_EXP needed: -11.2), 0.30 on da, 0.61 on dW and 0.50 on db (both at M = 1, where the "sum" is one
    product added to what was there: a bound of two to three roundings that one rounding half fills)."""
    c, i = case, dev(X.lin_inputs(case))
    out = nans(c.M, c.N)
    call("sed_small_linear", i["a"], i["w"], i["b"], out, c.M, c.N, c.K, c.act)
    ref, det, unit = X.lin_fwd_ref(i["a"], i["w"], i["b"], c.act)
    needed_k(f"small_linear {c.name} out", out, ref, det, unit)
    check(f"small_linear {c.name} out", out, ref, X.lin_out_bound(det, unit))
    da, dW, db = nans(c.M, c.K), i["dw0"].clone(), i["db0"].clone()
    call("sed_small_linear_bwd", i["a"], i["w"], out if c.act else None, i["dout"], da, dW, db, c.M, c.N, c.K, c.act)
    r = X.lin_bwd_ref(i["a"], i["w"], out, i["dout"], c.act, i["dw0"], i["db0"])
    check(f"small_linear {c.name} da", da, r["da"], r["b_da"], [("last output", r["drop_da"])])
    check(f"small_linear {c.name} dW", dW, r["dW"], r["b_dW"], [("last row", r["drop_dW"])])
    check(f"small_linear {c.name} db", db, r["db"], r["b_db"], [("last row", r["drop_db"])])
    da2 = nans(c.M, c.K)                                # untouched optional outputs
    call("sed_small_linear_bwd", i["a"], i["w"], out if c.act else None, i["dout"], da2, None, None, c.M, c.N, c.K, c.act)
    assert torch.equal(da2, da)


# ================================================================================================ MLM masking
@pytest.mark.parametrize("case", X.MLM_CASES, ids=case_ids(X.MLM_CASES))
def test_mlm_apply_and_backward(case):
    """sed_mlm_apply is exact row selection (torch.equal, every row written) across its 2730 2/3-row first pass, with sources on the
    other side of the boundary and copies of rows that are themselves masked or copied (they take the original row).  The backward:
    dx and dtoken against a float64 index_add, dx exact where one contribution lands, the chain bound on rows that many rows copy (500
    onto one) and on dtoken; drop checks remove the rows past the backward's own first pass (683).  With no masked row dtoken stays
    exactly 0.  Measured worst err / bound: 0.003 on dtoken (the worst-order chain over thousands of rows is far from the order the
    hardware takes), 1.00 on dx: a row with two contributions has the bound u (|a| + |b|) of one correctly rounded add, which an add
    of equal signs that lands half an ulp below a power of two reaches -- over 4 M such adds one does."""
    c, i = case, dev(X.mlm_inputs(case))
    out = nans(c.rows, D)
    call("sed_mlm_apply", i["x"], i["tok"], i["action"], i["src"], out, c.rows)
    assert torch.equal(out, X.mlm_fwd_ref(i["x"], i["tok"], i["action"], i["src"]))
    dx, dtok = zeros(c.rows, D), zeros(D)
    call("sed_mlm_apply_bwd", i["dout"], i["action"], i["src"], dx, dtok, c.rows)
    r = X.mlm_bwd_ref(i["dout"], i["action"], i["src"])
    check(f"mlm {c.name} dx", dx, r["dx"], r["b_dx"], [("copies past the first pass", r["drop_dx"])] if c.kind == "hot" else [])
    check(f"mlm {c.name} dtoken", dtok, r["dtok"], r["b_tok"], [("rows past the first pass", r["drop_tok"])] if bool((i["action"] == 1).any()) else [])
    single = r["cnt"] <= 1
    assert torch.equal(dx[single], r["dx"][single].float())
    if c.kind == "none":
        assert float(dtok.abs().max()) == 0.0 and torch.equal(dx, i["dout"])


# ================================================================================================ masked MSE
@pytest.mark.parametrize("case", X.MSE_CASES, ids=case_ids(X.MSE_CASES))
def test_masked_mse_vs_float64(case):
    """Loss and gradients with the row count passed by the host and read from device memory, across the 2048-row first pass, with every,
    no, random and only second-pass rows masked.  Loss bound: (12 passes + 13) u loss + the chain over the 512 workgroups; drop check: the
    second pass (or the last masked row).  dpred within 3 u, dtarget == -dpred bit for bit, unmasked rows exactly 0, every row written,
    NULL gradient outputs leave the other unchanged, both count forms give the same gradient bits.  With no masked row the device-count
    form divides by max(n, 1): loss 0, every gradient exactly 0 (torch's mean over an empty selection is NaN there); the host-count form
    refuses n = 0 as an argument error.  Measured worst err / bound: 0.03 on the loss, 0.78 on dpred (three roundings allowed, elementwise,
    over 4.7 M elements: two and a third of them lining up is the expected worst)."""
    c, i = case, dev(X.mse_inputs(case))
    r = X.mse_ref(i["pred"], i["target"], i["mask"])
    m = i["mask"].bool()
    ndev = torch.tensor([r["n"]], dtype=torch.int32, device=DEV)
    res = {}
    for form in ("host", "device"):
        loss, dp, dt = zeros(1), nans(c.rows, D), nans(c.rows, D)
        args = (r["n"], None) if form == "host" else (0, ndev)
        if form == "host" and r["n"] == 0:
            with pytest.raises(SedHipError, match="bad argument"):
                call("sed_masked_mse", i["pred"], i["target"], i["mask"], *args, loss, dp, dt, c.rows)
            assert bool(torch.isnan(dp).all()) and float(loss) == 0.0
            continue
        call("sed_masked_mse", i["pred"], i["target"], i["mask"], *args, loss, dp, dt, c.rows)
        drops = [("second pass / last masked row", r["drop"].view(1))] if r["n"] else []
        check(f"masked_mse {c.name} {form} loss", loss, r["loss"].view(1), r["b_loss"].view(1), drops)
        check(f"masked_mse {c.name} {form} dpred", dp, r["dpred"], r["b_d"])
        assert torch.equal(dt, -dp)
        if bool((~m).any()):
            assert float(dp[~m].abs().max()) == 0.0
        if r["n"] == 0:
            assert float(loss) == 0.0 and float(dp.abs().max()) == 0.0
        res[form] = (loss, dp)
        l2, dp2, dt2 = zeros(1), nans(c.rows, D), nans(c.rows, D)       # NULL forms
        call("sed_masked_mse", i["pred"], i["target"], i["mask"], *args, l2, dp2, None, c.rows)
        call("sed_masked_mse", i["pred"], i["target"], i["mask"], *args, zeros(1), None, dt2, c.rows)
        assert torch.equal(dp2, dp) and torch.equal(dt2, dt)
    if len(res) == 2:
        assert torch.equal(res["host"][1], res["device"][1])


# ================================================================================================ mean-teacher losses
_LOSS_INP = {}


def run_loss(case):
    if ("loss", case.name) in _MEMO:
        return _MEMO[("loss", case.name)]
    c = case
    key = (c.B, c.C, c.T)
    if key not in _LOSS_INP:
        _LOSS_INP.clear()                                   # one shape at a time on the device
        _LOSS_INP[key] = dev(X.loss_inputs(*key))
    i = _LOSS_INP[key]
    scratch, out = nans(8), nans(8)
    ds, dw, da = nans(c.B, c.C, c.T), nans(c.B, c.C), nans(c.B, c.C)
    w = X.LOSS_W
    call("sed_sed_losses", i["ss"], i["sw"], i["sa"], i["ts"], i["ta"], i["y"], i["yw"], c.B, c.C, c.T, c.strong_n, c.weak_lo, c.weak_n,
         w["w_weak"], w["w_weak_cons"], w["w_at"], w["w_cons"], scratch, out, ds, dw, da)
    torch.cuda.synchronize()
    _MEMO[("loss", case.name)] = dict(scratch=scratch.cpu(), out=out.cpu(), grads=(ds, dw, da), ref=X.loss_ref(i, c))
    return _MEMO[("loss", case.name)]


@pytest.mark.parametrize("case", X.LOSS_CASES, ids=case_ids(X.LOSS_CASES))
def test_sed_losses_sums_and_outputs_vs_float64(case):
    """The six un-normalised sums and the seven outputs against float64 BCE (log clamped at -100) / squared error on the fp32
    posteriors, for every partition (strong_n, weak_lo, weak_n) including weak_lo != strong_n and the empty selections: with
    strong_n == 0 or weak_n == 0 the affected terms and `total` are NaN and every other term is within bound.  Bound: the error model
    of tail_cases.loss_ref, capped at the 2e-6 max(1, |value|) of test_gpu_kernels.py (the cap is what binds above ~30 workgroups:
    the worst-order chain bound grows with their number, the measured error does not).  Drop checks: every grid pass after the first
    (1 048 680 elements: 104 past the 1024-workgroup cap's first pass), the clip-level values 256.., the last clip.  Measured worst
    err / bound: 0.53 on the sums -- at the 1 048 680-element case, where the 2e-6 cap binds: 1024 atomic adds in an order that
    changes from run to run leave 0.9e-6 to 1.1e-6 relative on sums[3], about two standard deviations of that random walk, the cap is
    about four -- 0.34 elsewhere; 0.18 on the outputs.  K_LOG needed: -12.2 (see tail_cases.K_LOG)."""
    c, r = case, run_loss(case)
    ref = r["ref"]
    for k in range(6):
        v, det, unit = (t.cpu() for t in ref["sums"][k])
        got = r["scratch"][k].double()
        if float(unit) > 0:
            report(f"losses {c.name} sums[{k}]: intrinsic constant needed={float((abs(got - v) - det) / (U32 * unit)):.3f}")
        drops = [(name, d.cpu().view(1)) for (kk, name), d in ref["drops"].items() if kk == k and float(d) != 0.0]
        check(f"losses {c.name} sums[{k}]", got.view(1), v.view(1), X.loss_bound(v, det, unit).view(1), drops)
    for k in range(7):
        v, det, unit = (t.cpu() for t in ref["outs"][k])
        expect_nan = (k in (0, 1) and c.strong_n == 0) or (k in (0, 2, 3) and c.weak_n == 0)
        assert bool(torch.isnan(v)) == expect_nan
        check(f"losses {c.name} out[{k}]", r["out"][k].view(1), v.view(1), X.loss_bound(v, det, unit).view(1))
    assert float(r["out"][7]) == 0.0


@pytest.mark.parametrize("case", X.LOSS_CASES, ids=case_ids(X.LOSS_CASES))
def test_sed_losses_gradients_vs_float64(case):
    """d_strong, d_weak, d_at against (p - y) / max(p (1 - p), 1e-12) and 2 (p - q) / n with the weights, element by element within
    12 u of the two parts' sizes (never above the 1e-6 relative of test_gpu_kernels.py), at posteriors exactly 0, 1 and 1 - 2^-24;
    finite and fully written whatever the partition (clips outside a selection carry the consistency part alone).  Measured worst
    err / bound: 0.26."""
    c, r = case, run_loss(case)
    for k, (got, (g, b)) in enumerate(zip(r["grads"], r["ref"]["grads"])):
        assert bool(torch.isfinite(got).all())
        assert float(b.max()) <= X.LEGACY_GRAD_REL * max(1.0, float(g.abs().max()))
        check(f"losses {c.name} grad[{k}]", got, g, b)


def test_sed_losses_argument_errors_write_nothing():
    i = dev(X.loss_inputs(2, 10, 7))
    for sn, lo, wn in ((3, 0, 1), (1, 1, 2), (-1, 0, 1), (1, -1, 1)):
        out, ds = nans(8), nans(2, 10, 7)
        with pytest.raises(SedHipError, match="bad argument"):
            call("sed_sed_losses", i["ss"], i["sw"], i["sa"], i["ts"], i["ta"], i["y"], i["yw"], 2, 10, 7, sn, lo, wn, 0.5, 0.5, 2.0, 13.7,
                 nans(8), out, ds, nans(2, 10), nans(2, 10))
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(ds).all())


# ================================================================================================ AdamW + EMA
def adam_call(s, lr, wd, step, alpha, do_adam=1, ema=True, g=None):
    call("sed_adamw_ema", s["p"], s["g"] if g is None else g, s["m"], s["v"], s["ema"] if ema else None, s["p"].numel(), lr, wd, X.BETA1, X.BETA2,
         X.EPS, step, alpha, do_adam)


def adam_check(name, before, after, lr, wd, step, alpha, do_adam=1, ema=True, drops=False):
    ref, bound = X.adam_ref(before["p"], before["g"], before["m"], before["v"], before["ema"] if ema else None, lr, wd, step, alpha, do_adam)
    worst = 0.0
    for k, key in enumerate(("p", "m", "v", "ema")):
        if ref[k] is None:
            continue
        d = []
        if drops and do_adam and not (key == "p" and lr == 0.0) and not (key == "ema" and alpha == 1.0):     # (those stay as they were anyway)
            sl = slice(X.ADAM_FIRST_PASS, None)
            d = [("second float4 pass", X.only(ref[k] - before[key].double(), sl))]
        worst = max(worst, check(f"adamw_ema {name} {key}", after[key], ref[k], bound[k], d))
    return worst


def clone(s):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in s.items()}


@pytest.mark.parametrize("n", X.ADAM_N)
def test_adamw_ema_vs_float64(n):
    """p, m, v, ema after one call against the float64 recurrence of torch.optim.AdamW + the EMA line from the fp32 state (error model
    of tail_cases.adam_ref; the largest term is the host's fp32 1 - powf(beta2, step), 1000 u relative at step 1): steps 1, 2, 3 in
    sequence from zero state, then single calls at step 10, 1000, 100 000 from a random state with every (lr, wd) and alpha of the case
    lists (a diagonal of them at the two 8.4 M-element sizes, whose references run in float64 on the device).  n = 8 388 672 has a
    64-float second pass; its drop check is the state left as it was there.  lr = 0 leaves p bit-unchanged while m, v move; alpha = 0
    gives ema the bits of the new p, alpha = 1 leaves it unchanged; elements with g = m = v = 0 only decay.  Measured worst err /
    bound: 0.36 on p, 0.65 on m, 0.50 on v, 0.44 on ema (m and v are three and four roundings, elementwise, over 8.4 M elements: two of
    three lining up is the expected worst)."""
    s0 = dev(X.adam_inputs(n))
    big = n >= X.ADAM_FIRST_PASS
    lr, wd = X.ADAM_HYPER[0]
    s = clone(s0)
    s["m"].zero_(); s["v"].zero_()
    for step in (1, 2, 3):
        before = clone(s)
        s["g"] = (s0["g"] * step).contiguous()
        before["g"] = s["g"]
        alpha = X.f32(min(1 - 1 / (step + 1), 0.999))
        adam_call(s, lr, wd, step, alpha)
        adam_check(f"n={n} seq step {step}", before, s, lr, wd, step, alpha, drops=n > X.ADAM_FIRST_PASS)
        z = s0["zero"]
        assert float(s["m"][z].abs().max()) == 0.0 and float(s["v"][z].abs().max()) == 0.0
    combos = [(h, st, a) for h in X.ADAM_HYPER for st in X.ADAM_STEPS for a in X.ADAM_ALPHAS]
    if big:
        combos = [(X.ADAM_HYPER[k % 3], X.ADAM_STEPS[k % 3], X.ADAM_ALPHAS[k]) for k in range(4)]
    for (lr, wd), step, alpha in combos:
        s = clone(s0)
        adam_call(s, lr, wd, step, alpha)
        adam_check(f"n={n} lr={lr} wd={wd} step={step} alpha={alpha}", s0, s, lr, wd, step, alpha, drops=n > X.ADAM_FIRST_PASS)
        if lr == 0.0:
            assert torch.equal(s["p"], s0["p"]) and not torch.equal(s["m"], s0["m"]) and not torch.equal(s["v"], s0["v"])
        if alpha == 0.0:
            assert torch.equal(s["ema"], s["p"])
        if alpha == 1.0:
            assert torch.equal(s["ema"], s0["ema"])


@pytest.mark.parametrize("n", [64, X.ADAM_FIRST_PASS + 64])
def test_adamw_ema_forms(n):
    """ema == NULL: p, m, v get the bits of the call with an ema.  do_adam == 0 in the trainer's calling form (g aliased to p): p, m, v
    keep their bits and ema is within the EMA line's bound (4 u).  n = 6 is refused as an argument error and writes nothing."""
    s0 = dev(X.adam_inputs(n))
    lr, wd = X.ADAM_HYPER[0]
    a, b = clone(s0), clone(s0)
    adam_call(a, lr, wd, 10, 0.999)
    adam_call(b, lr, wd, 10, 0.999, ema=False)
    assert all(torch.equal(a[k], b[k]) for k in ("p", "m", "v")) and torch.equal(b["ema"], s0["ema"])
    for alpha in (0.5, 0.999):
        e = clone(s0)
        adam_call(e, 0.0, 0.0, 10, alpha, do_adam=0, g=e["p"])
        assert all(torch.equal(e[k], s0[k]) for k in ("p", "m", "v"))
        adam_check(f"n={n} ema only alpha={alpha}", s0, e, 0.0, 0.0, 10, alpha, do_adam=0)
    t = dev(X.adam_inputs(8))
    t = {k: v[:6].clone() for k, v in t.items()}
    keep = clone(t)
    with pytest.raises(SedHipError, match="bad argument"):
        call("sed_adamw_ema", t["p"], t["g"], t["m"], t["v"], t["ema"], 6, 1e-3, 1e-4, X.BETA1, X.BETA2, X.EPS, 1, 0.5, 1)
    assert all(torch.equal(t[k], keep[k]) for k in ("p", "m", "v", "ema"))
