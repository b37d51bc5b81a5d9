"""sed_window_mix / sed_window_mix_bwd on ragged window sets, and sed_interp_fwd / sed_interp_bwd on their own, against the float64
reference of tests/window_cases.py (need an MI355X).  tests/test_window_cases_cpu.py proves on the CPU that a restatement of the
kernels' loops keeps the same bounds, and that the row -> window search the backward kernel used to have does not.

Both kernels run once per case; every test reads the stored results."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import window_cases as X  # noqa: E402
from oracle import matsed_oracle as O  # noqa: E402
from transformer4sed_amd.ops import call  # noqa: E402
from window_cases import F32, U32  # noqa: E402

DEV = "cuda"
D = 768
IDS = [c.name for c in X.CASES]
_MEMO = {}


def maxerr(a, b):
    return float((a.double() - b.double()).abs().max())


def run(case):
    """Inputs, float64 reference, bounds and the two kernels' results (CPU copies) of a case, computed once and left unchanged."""
    if case.name in _MEMO:
        return _MEMO[case.name]
    frames, x, g = X.inputs(case, D, seed=3)
    ref_out, ref_dfr, ref_dx = X.reference(case, frames, x, g)
    lefts, tps, offs, rows = X.tables(case)
    packed = X.pack(frames, case)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    wl, wt, wo = i32(lefts), i32(tps), i32(offs)
    out = x.to(DEV)                                                         # mixed in place
    call("sed_window_mix", packed.to(DEV), wl, wt, wo, len(tps), out, float(case.mix), case.B, case.T, case.ratio)
    dpooled = torch.full((rows, D), float("nan"), device=DEV)
    dglobal = torch.full((case.B, case.T, D), float("nan"), device=DEV)
    call("sed_window_mix_bwd", g.to(DEV), wl, wt, wo, len(tps), dpooled, dglobal, float(case.mix), case.B, case.T, case.ratio, rows)
    torch.cuda.synchronize()
    _MEMO[case.name] = dict(frames=frames, x=x, g=g, packed=packed, ref_out=ref_out, ref_dpacked=X.pack(ref_dfr, case), ref_dx=ref_dx,
                            out=out.cpu(), dpooled=dpooled.cpu(), dglobal=dglobal.cpu(), fb=X.fwd_bound(case, frames, x),
                            bb=X.bwd_bound(case, g))
    return _MEMO[case.name]


@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_window_mix_forward_vs_float64(case):
    r = run(case)
    assert r["fb"] <= 2e-5                      # no looser than the bound of test_gpu_kernels.py::test_patch_tokens_fpool_interp
    e = maxerr(r["out"], r["ref_out"])
    print(f"{case.name}: forward max |err| {e:.3e}  bound {r['fb']:.3e}")
    assert e <= r["fb"], (e, r["fb"])
    unc = X.coverage(case) == 0
    if bool(unc.any()):                         # frames no window covers: local part 0
        assert maxerr(r["out"][:, unc], (1.0 - case.mix) * r["x"][:, unc].double()) <= r["fb"]
    if case.mix == 0.0:
        assert torch.equal(r["out"], r["x"])


@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_window_mix_backward_vs_float64_autograd(case):
    r = run(case)
    assert not bool(torch.isnan(r["dpooled"]).any()), "a packed row was not written"
    e = maxerr(r["dpooled"], r["ref_dpacked"])
    print(f"{case.name}: backward max |err| {e:.3e}  bound {r['bb']:.3e}")
    assert e <= r["bb"], (e, r["bb"])
    s = torch.tensor(1.0, dtype=F32) - torch.tensor(case.mix, dtype=F32)
    assert torch.equal(r["dglobal"], s * r["g"])
    assert maxerr(r["dglobal"], r["ref_dx"]) <= U32 * float(r["g"].abs().max())
    if case.mix == 0.0:
        assert float(r["dpooled"].abs().max()) == 0.0


@pytest.mark.parametrize("eng,sf", X.ORDER_PAIRS, ids=[a for a, _ in X.ORDER_PAIRS])
def test_packing_order_does_not_change_a_bit(eng, sf):
    """The same windows with the 49-patch group packed first (offs not monotone in the window index): the forward output and every
    window's block of dpooled are bit-identical to the engine's order."""
    ce, cs = X.BY_NAME[eng], X.BY_NAME[sf]
    assert ce.windows == cs.windows and X.tables(ce)[2] != X.tables(cs)[2] and X.tables(cs)[2][0] > 0
    re, rs = run(ce), run(cs)
    assert torch.equal(re["out"], rs["out"])
    for w, (a, b) in enumerate(zip(X.unpack(re["dpooled"], ce), X.unpack(rs["dpooled"], cs))):
        assert torch.equal(a, b), w
    assert torch.equal(re["dglobal"], rs["dglobal"])


@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_adjoint_identity_on_device_results(case):
    """<mix(p, x), g> == <p, dpooled> + <x, dglobal>, the two sides from the device results, summed in float64.  Each forward element is
    within `fb` and each backward element within `bb` of the exact operator, the data are N(0, 1), so the two sums differ by a sum of N
    terms of mixed sign, each at most about fb + bb: bound (fb + bb) sqrt(N), N = all elements summed on either side."""
    r = run(case)
    lhs = float((r["out"].double() * r["g"].double()).sum())
    rhs = float((r["packed"].double() * r["dpooled"].double()).sum() + (r["x"].double() * r["dglobal"].double()).sum())
    n = r["out"].numel() + r["packed"].numel() + r["x"].numel()
    bound = (r["fb"] + r["bb"]) * math.sqrt(n)
    print(f"{case.name}: adjoint |lhs - rhs| {abs(lhs - rhs):.3e}  bound {bound:.3e}  (lhs {lhs:.6e})")
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)


@pytest.mark.parametrize("B", [1, 3, 14])
def test_interp_fwd_bwd_vs_float64(B):
    """sed_interp_fwd / sed_interp_bwd at the model's shape (99 pooled frames + 1 replicated, x10) on their own.  Forward: one lerp per
    element, bound (1 + 8) 2^-24 max|in| (the merge's forward bound with cnt = 1 and no global term).  Backward: a row sums at most
    2.5 ratio non-zero taps (the last row: 10 as upper tap, 15 as the clamped lower tap) of w dout with w >= 0 rounded once or twice,
    so |error| <= (2.5 ratio + 3) 2^-24 sum_j w_j |dout_j| element by element; the sum is the float64 adjoint applied to |dout|.
    B = 14 is 266 112 float4 of din, past the 262 144 of sed_interp_bwd's first grid pass (1024 x 256): there the rows that lie wholly in
    the second pass have to be >= 10 bounds large somewhere, so the bound would see them missing."""
    tin, pad, ratio = 99, 1, 10
    g = torch.Generator(device="cpu").manual_seed(17 + B)
    p = torch.randn(B, tin, D, generator=g)
    dout = torch.randn(B, (tin + pad) * ratio, D, generator=g)
    pp = p.double().requires_grad_(True)
    ref = O.interp_linear(torch.cat([pp, pp[:, -1:]], 1), ratio, fused_index=True)
    dref, = torch.autograd.grad(ref, pp, dout.double(), retain_graph=True)
    dabs, = torch.autograd.grad(ref, pp, dout.double().abs())
    out = torch.full((B, (tin + pad) * ratio, D), float("nan"), device=DEV)
    call("sed_interp_fwd", p.to(DEV), out, B, tin, pad, ratio)
    din = torch.full((B, tin, D), float("nan"), device=DEV)
    call("sed_interp_bwd", dout.to(DEV), din, B, tin, pad, ratio)
    e = maxerr(out.cpu(), ref.detach())
    fb = 9 * U32 * float(p.abs().max())
    print(f"interp B={B}: forward max |err| {e:.3e}  bound {fb:.3e}")
    assert e <= fb, (e, fb)
    err = (din.cpu().double() - dref).abs()
    assert not bool(torch.isnan(err).any())
    bound = (2.5 * ratio + 3) * U32 * dabs
    print(f"interp B={B}: backward max |err| {float(err.max()):.3e}  max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())
    first = 1024 * 256 * 4                                  # floats of din the first grid pass of sed_interp_bwd writes
    if B * tin * D > first:
        r0 = -(-first // D)
        assert float((dref.reshape(-1, D)[r0:].abs() / bound.reshape(-1, D)[r0:]).max()) >= 10.0
