"""CPU proof of tests/window_cases.py: the case tables are what they claim to be, the float64 reference is the oracle's merge, the
restated kernel loops agree with it and with its autograd inside the bounds tests/test_gpu_window_mix.py holds the hardware to, the
backward loop is the exact adjoint of the forward loop -- and the row -> window search the backward kernel used to have fails the
short-first packing while the range search passes it."""
import pytest
import torch

import window_cases as X
from oracle import matsed_oracle as O
from window_cases import F32, F64

D = 4                       # channels are independent in both kernels
IDS = [c.name for c in X.CASES]


_MEMO = {}


def data(case):
    """Inputs, float64 reference and bounds of a case, computed once and left unchanged."""
    if case.name not in _MEMO:
        frames, x, g = X.inputs(case, D, seed=3)
        out, dfr, dxg = X.reference(case, frames, x, g)
        _MEMO[case.name] = dict(frames=frames, x=x, g=g, out=out, dfr=dfr, dxg=dxg, packed=X.pack(frames, case),
                                dpacked=X.pack(dfr, case), fb=X.fwd_bound(case, frames, x), bb=X.bwd_bound(case, g))
    return _MEMO[case.name]


def emu64(case):
    """The two restated loops run in float64, once per case."""
    d = data(case)
    if "out64" not in d:
        d["out64"] = X.emulate_fwd(d["packed"].double(), d["x"].double(), case)
        d["dp64"], d["dg64"], _ = X.emulate_bwd(d["g"].double(), case)
    return d


def maxerr(a, b):
    return float((a.double() - b.double()).abs().max())


# ------------------------------------------------------------------------------------------------ the tables
def test_case_tables():
    lefts, tps, offs, rows = X.tables(X.BY_NAME["val17-B3-mix0.5"])
    assert tps == [50] * 16 + [49] and lefts == [31 * w for w in range(17)] and rows == 3 * 849
    assert offs == [150 * w for w in range(17)]                             # the engine's order: monotone, window 0 first
    cov = X.coverage(X.BY_NAME["val17-B3-mix0.5"])
    assert int(cov[985]) == 1 and int(cov[986:].max()) == 0 and int(cov[:986].min()) >= 1 and int(cov.max()) == 17
    _, _, offs, _ = X.tables(X.BY_NAME["val17-short-first-B3-mix0.5"])
    assert offs[16] == 0 and offs[0] == 3 * 49 and offs[:16] == [147 + 150 * w for w in range(16)]     # offs[0] > 0: not monotone
    _, tps, _, _ = X.tables(X.BY_NAME["three-sizes-B1-mix0.5"])
    assert tps == [49] * 11 + [45]
    tiny = X.BY_NAME["tiny-B3-mix0.5"]
    cov = X.coverage(tiny)
    assert sorted(t for _, t in tiny.windows) == [3, 3, 4, 5] and int(cov.max()) == 3
    assert int(cov[70:100].max()) == 0 and int(cov[100:].min()) == 1        # an uncovered stretch
    assert max(l + t * tiny.ratio for l, t in tiny.windows) > tiny.T        # one window runs past T
    one = X.BY_NAME["tiny-one-window-B1-mix0.5"]
    assert len(one.windows) == 1 and one.windows[0][0] + one.windows[0][1] * one.ratio > one.T
    assert {c.B for c in X.CASES} == {1, 3} and {c.mix for c in X.CASES} == {0.0, 0.5, 1.0}


def test_sweep_is_the_engines_grouping():
    """`sweep` / `groups_of` against the arithmetic written out: [512, 31] at B = 1 gives the two weight-gradient paths (M >= 1024 and
    M < 1024 token rows), [512, 49] gives one group."""
    g31 = X.groups_of(X.sweep(1000, 512, 31))
    assert {tp: len(w) for tp, w in g31.items()} == {50: 16, 49: 1}
    assert [len(w) * (2 + 12 * tp) for tp, w in g31.items()] == [9632, 590]
    g49 = X.groups_of(X.sweep(1000, 512, 49))
    assert {tp: len(w) for tp, w in g49.items()} == {50: 11} and 11 * (2 + 12 * 50) == 6622


def test_index_forms():
    """The kernels' source index is a fused multiply-add (one rounding).  It is NOT the quotient form of oracle.interp_linear's default:
    at ratio 10 the two differ by one fp32 ulp of `src` in about a fifth of the frames, which moves `lam` by up to 2^-18 for
    src >= 32 -- 64 times the 2^-24 the forward bound allows per operation.  The reference therefore asks for `fused_index`."""
    j = torch.arange(500, dtype=F32)
    quot = torch.clamp((j + 0.5) / 10 - 0.5, min=0.0)
    src = []
    for jj in range(500):
        i0, i1, lam = X.interp_coeff(jj, 10, 50, 50)
        src.append(i0 + lam)
        assert 0 <= i0 <= i1 <= 49 and i1 - i0 <= 1 and 0.0 <= lam < 1.0
    fused = torch.tensor(src, dtype=F64)
    n_diff = int((fused != quot.double()).sum())
    assert 50 < n_diff < 200, n_diff
    assert float((fused - quot.double()).abs().max()) <= 2.0 ** -18
    # oracle.interp_linear(fused_index=True) uses exactly these coefficients: interpolating the identity ramp returns src (up to the last
    # patch, where both taps are patch 49)
    ramp = O.interp_linear(torch.arange(50, dtype=F64).view(1, 50, 1), 10, fused_index=True).view(-1)
    assert torch.equal(ramp[:495], fused[:495]) and ramp[495:].tolist() == [49.0] * 5


def test_merge_windows_is_the_oracles_loop():
    """fp32, default index form: bit for bit the loop slide_window_features had inline (emb / acc with NaN -> 0)."""
    case = X.BY_NAME["val17-B1-mix1.0"]
    frames, _, _ = X.inputs(case, D, seed=5)
    emb, acc = torch.zeros(1, 1000, D), torch.zeros(1, 1000, D)
    for fr, (left, _) in zip(frames, case.windows):
        fr = O.interp_linear(fr, 10)
        right = int(min(1000, left + fr.shape[1]))
        emb[:, left:right] += fr[:, :right - left]
        acc[:, left:right] += 1
    emb = emb / acc
    emb[torch.isnan(emb)] = 0
    assert torch.equal(O.merge_windows(frames, [l for l, _ in case.windows], 1000, 10), emb)
    assert float(emb[:, 986:].abs().max()) == 0 and float(emb[:, :986].abs().min()) > 0


# ------------------------------------------------------------------------------------------------ emulation vs reference
@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_emulated_forward_vs_reference(case):
    d = data(case)
    assert d["fb"] <= 2e-5                                  # no looser than the bound tests/test_gpu_kernels.py uses on N(0, 1) data
    out = X.emulate_fwd(d["packed"], d["x"], case)
    assert out.dtype == F32
    e = maxerr(out, d["out"])
    assert e <= d["fb"], (e, d["fb"])
    unc = X.coverage(case) == 0
    assert maxerr(out[:, unc], (1.0 - case.mix) * d["x"][:, unc].double()) <= d["fb"]
    e64 = maxerr(emu64(case)["out64"], d["out"])
    assert e64 <= 1e-13, e64                                # same lam on both sides: only float64 rounding is left


@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_emulated_backward_vs_autograd(case):
    d = data(case)
    dp, dg, owner = X.emulate_bwd(d["g"], case)
    lefts, tps, offs, rows = X.tables(case)
    stray = [r for r, w in enumerate(owner) if not offs[w] <= r < offs[w] + case.B * tps[w]]
    e = maxerr(dp, d["dpacked"])
    assert not stray and e <= d["bb"], (f"{len(stray)} of {rows} packed rows given to the wrong window" +
                                        (f" (rows {stray[0]}..{stray[-1]})" if stray else "") + f"; max |err| {e:.3e}, bound {d['bb']:.3e}")
    assert torch.equal(dg, ((torch.tensor(1.0) - torch.tensor(case.mix)) * d["g"]))
    assert maxerr(dg, d["dxg"]) <= X.U32 * float(d["g"].abs().max())
    assert maxerr(emu64(case)["dp64"], d["dpacked"]) <= 1e-13
    if case.mix == 0.0:
        assert float(dp.abs().max()) == 0.0


@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_adjoint_identity_float64(case):
    """<mix(p, x), g> == <p, dpooled> + <x, dglobal> for the two restated loops run in float64."""
    d = emu64(case)
    p, x, g = d["packed"].double(), d["x"].double(), d["g"].double()
    out, dp, dg = d["out64"], d["dp64"], d["dg64"]
    lhs, rhs = float((out * g).sum()), float((p * dp).sum() + (x * dg).sum())
    scale = float((out * g).abs().sum())
    assert abs(lhs - rhs) <= 1e-13 * scale, (lhs, rhs)


# ------------------------------------------------------------------------------------------------ the search
def test_former_search_fails_the_short_first_packing():
    """The search the backward kernel had sends every packed row below offs[0] to window 0: nothing shows in the engine's order, the
    short window's B * 49 rows go wrong when its group is packed first."""
    eng, sf = X.BY_NAME["val17-B1-mix1.0"], X.BY_NAME["val17-short-first-B1-mix1.0"]
    for case, n_wrong in ((eng, 0), (sf, 49)):
        _, tps, offs, rows = X.tables(case)
        right = [X.search_range(r, offs, tps, case.B) for r in range(rows)]
        old = [X.search_largest_start(r, offs, tps, case.B) for r in range(rows)]
        wrong = [r for r in range(rows) if old[r] != right[r]]
        assert len(wrong) == n_wrong
        assert all(right[r] == 16 and old[r] == 0 for r in wrong)
    d = data(sf)
    dp_old, _, _ = X.emulate_bwd(d["g"], sf, search=X.search_largest_start)
    e = maxerr(dp_old, d["dpacked"])
    assert e > 1e3 * d["bb"], e                             # an O(1) error, not a rounding question
    dp_new, _, _ = X.emulate_bwd(d["g"], sf)
    assert maxerr(dp_new, d["dpacked"]) <= d["bb"]
