"""Batch-split and grid-stride reductions at production batch sizes (need an MI355X).

The kernel tests of test_gpu_kernels.py run at B <= 3 and at most 2383 rows; several kernels change how they split their work above
that: `sed_relpos_attn_bwd`'s positional-table reduction and `sed_assemble_tokens_bwd` hand ceil(B / 8) clips to each of min(B, 8)
batch slices, and the LayerNorm backward kernels cap their grid at 1024 blocks x 4 rows, so that above 4096 rows a grid-stride loop
and per-wave multi-row dgamma / dbeta partials take over.  Here:

1. every such reduction against a float64 sum of the kernel's own inputs (or intermediates), at and beyond each threshold, with a bound
   stated as an error model: u32 * (kappa * sum|terms| + an atomic-chain term), kappa read off the kernel's summation tree.  Every test
   also checks that leaving out one contribution -- the last clip of the last non-empty slice, or one row block past the first grid
   pass -- moves the float64 reference by at least 10x the bound, so the bound can see a dropped clip or row;
2. per-sequence bit-for-bit batch invariance of the attention kernels at production batch (a key leaking across sequences would be a
   ~1 % error, below the bounds of the parity tests);
3. the depth-2 model at B = 32 with a loss over every clip against the float64 sum of sixteen B = 2 runs.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from transformer4sed_amd import synth  # noqa: E402
from transformer4sed_amd.ops import call, pad64, BF16, F16  # noqa: E402

DEV = "cuda"
# measured errors and margins: SED_TEST_LOG_DIR, else test_logs/ at the repository root (kept out of git)
LOG = os.path.join(os.environ.get("SED_TEST_LOG_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_logs"),
                   "batch_scale_errors.log")
U32 = 2.0 ** -24        # unit roundoff of fp32
SCALE = 0.125           # 1 / sqrt(64): the attention kernels' score scale (a power of two: exact)
H = 12


def report(name, err, scale=None):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(f"{name}: max_abs_err={err:.4e}" + (f" ref_scale={scale:.3e}" if scale is not None else "") + "\n")


def randn(*shape, seed, scale=1.0, dev=DEV):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=dev) * scale


def chain(parts):
    """Rounding bound of an atomic chain that adds the float64 partials parts[0..n-1] (leading dim) in an unknown order:
    sum_k u |S_k| over the running sums, largest partials first (the worst order)."""
    a = parts.abs().sort(dim=0, descending=True).values
    w = torch.arange(a.shape[0], 0, -1, dtype=a.dtype, device=a.device).view(-1, *([1] * (a.dim() - 1)))
    return U32 * (a * w).sum(0)


def only(t, rows):
    """t with everything outside `rows` zeroed: the contribution of those rows alone."""
    z = torch.zeros_like(t)
    z[rows] = t[rows]
    return z


def check(name, got, ref, bound, drop):
    """|got - ref| <= bound everywhere, and leaving out the contribution `drop` moves ref by >= 10x the bound somewhere."""
    err = (got.double() - ref).abs()
    ratio = float((err / bound).max())
    report(f"{name}: worst err / bound = {ratio:.3f}", float(err.max()), float(bound.max()))
    assert ratio <= 1.0, (name, ratio)
    sens = float((drop.abs() / bound).max())
    assert sens >= 10.0, (name, "bound cannot see a dropped contribution", sens)
    return ratio


# ------------------------------------------------------------------------------------------------ LayerNorm backward family
def ln_stats(x, in_scale, eps):
    """float64 mean / rstd of in_scale * x rounded to fp32: the kernels' saved statistics, fed to them as inputs."""
    xs = x.double() * in_scale
    mu = xs.mean(1)
    rs = 1.0 / torch.sqrt(xs.var(1, unbiased=False) + eps)
    return mu.float(), rs.float()


def ln_bwd_ref(dy, x, mu, rs, g, in_scale, nblocks):
    """float64 LayerNorm backward over the fp32 inputs the kernel reads, with the bounds of its summation tree.

    dx: per row, two wave sums over D (D / 64 serial terms per lane, 6 butterfly levels) and ~6 roundings around them -> kappa = 24 on
    |dg| + mean|dg| + |xh| mean|dg xh| plus the propagated rounding of xh itself.  dgamma / dbeta: each wave adds its rows serially
    (rows_per_wave terms), 4 waves meet in LDS, 1024 blocks at most meet in an atomic chain (bounded by `chain` on the block partials).
    Returns dx, dgamma, dbeta, their bounds, and the block partials (leading dim = block)."""
    M, D = x.shape
    dy, x, g = dy.double(), x.double(), g.double()
    mu, rs = mu.double().unsqueeze(1), rs.double().unsqueeze(1)
    xs = x * in_scale
    xh = (xs - mu) * rs
    xe = xs.abs() * rs + 2 * xh.abs()            # |rounding error of the kernel's xh| / u
    dg = dy * g
    s1, s2 = dg.mean(1, keepdim=True), (dg * xh).mean(1, keepdim=True)
    dx = in_scale * rs * (dg - s1 - xh * s2)
    a1, a2 = dg.abs().mean(1, keepdim=True), (dg * xh).abs().mean(1, keepdim=True)
    t = dg.abs() + a1 + xh.abs() * a2 + s2.abs() * xe + (dg.abs() * xe).mean(1, keepdim=True)
    dx_bound = 24 * U32 * in_scale * rs * t
    rpw = -(-M // (4 * nblocks))
    pad = rpw * 4 * nblocks - M
    def blocks(v):   # row r belongs to block (r // 4) % nblocks
        v = torch.nn.functional.pad(v, (0, 0, 0, pad))
        return v.view(rpw, nblocks, 4, D).sum((0, 2))
    tg, tb = dy * xh, dy
    pg, pb = blocks(tg), blocks(tb)
    kap = rpw + 3 + 2
    bg = U32 * (kap * tg.abs().sum(0) + (dy.abs() * xe).sum(0)) + chain(pg)
    bb = U32 * kap * tb.abs().sum(0) + chain(pb)
    return dx, tg.sum(0), tb.sum(0), dx_bound, bg, bb, tg, tb


def drop_rows(M, nblocks):
    """Rows of one row block past the first grid pass (or of the last block when there is only one pass)."""
    r0 = 4 * nblocks if M > 4 * nblocks else 4 * (nblocks - 1)
    return slice(r0, min(r0 + 4, M))


def ln_inputs(M, D, seed, in_scale=1.0, eps=1e-6, dev=DEV):
    # distinct rows: per-row offsets and scales on top of the noise, so no two rows (and no two clips) carry the same data
    rows = torch.arange(M, device=dev, dtype=torch.float32).unsqueeze(1)
    x = randn(M, D, seed=seed, dev=dev) * (1.0 + 0.5 * torch.sin(rows * 0.37)) + 0.3 * torch.cos(rows * 0.11)
    dy = randn(M, D, seed=seed + 1, dev=dev) * (1.0 + 0.25 * torch.cos(rows * 0.23))
    g = 1 + 0.2 * randn(D, seed=seed + 2, dev=dev)
    mu, rs = ln_stats(x, in_scale, eps)
    return x, dy, g, mu, rs


def _ln_family(name, entry, M, D, in_scale, seed):
    """entry: 'std' (sed_layernorm_bwd), 'x16' (sed_layernorm_bwd_x16), 'any' (sed_ln_bwd_any)."""
    x, dy, g, mu, rs = ln_inputs(M, D, seed, in_scale)
    nb = min(-(-M // 4), 1024)
    dx, dgr, dbr, bx, bg, bb, tg, tb = ln_bwd_ref(dy, x, mu, rs, g, in_scale, nb)
    sl = drop_rows(M, nb)
    base = randn(M, D, seed=seed + 3)
    acc = base.clone()
    dgk, dbk = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    if entry == "any":
        call("sed_ln_bwd_any", dy, x, mu, rs, g, in_scale, acc, 1, dgk, dbk, M, D)
    elif entry == "x16":
        dx16 = torch.empty(M, D, dtype=BF16, device=DEV)
        call("sed_layernorm_bwd_x16", dy, x, mu, rs, g, in_scale, acc, 1, dgk, dbk, dx16, M, D)
        assert torch.equal(dx16, acc.to(BF16))
    else:
        call("sed_layernorm_bwd", dy, x, mu, rs, g, in_scale, acc, 1, dgk, dbk, M, D)
    # accumulate form: one more rounding of the sum
    want = base.double() + dx
    check(f"{name} M={M} dx (accumulate)", acc, want, bx + U32 * want.abs() + 1e-30, only(dx, sl))
    check(f"{name} M={M} dgamma", dgk, dgr, bg, tg[sl].sum(0))
    check(f"{name} M={M} dbeta", dbk, dbr, bb, tb[sl].sum(0))
    # store form (no dgamma / dbeta): every row written, whatever was there before
    st = torch.full((M, D), float("nan"), device=DEV)
    if entry == "any":
        call("sed_ln_bwd_any", dy, x, mu, rs, g, in_scale, st, 0, None, None, M, D)
    elif entry == "x16":
        dx16 = torch.empty(M, D, dtype=BF16, device=DEV)
        call("sed_layernorm_bwd_x16", dy, x, mu, rs, g, in_scale, st, 0, None, None, dx16, M, D)
        assert torch.equal(dx16, st.to(BF16))
    else:
        call("sed_layernorm_bwd", dy, x, mu, rs, g, in_scale, st, 0, None, None, M, D)
    check(f"{name} M={M} dx (store)", st, dx, bx + 1e-30, only(dx, sl))


@pytest.mark.parametrize("entry", ["std", "x16"])
@pytest.mark.parametrize("M", [4095, 4096, 4097, 8193, 38080])
def test_layernorm_bwd_grid_stride_vs_float64(M, entry):
    """sed_layernorm_bwd / _x16 at D = 768 across the 1024-block cap (4096 rows): dx on every row in both the accumulate and the store
    form, the x16 image == bf16(dx), dgamma / dbeta against a float64 sum (bounds: the error model of ln_bwd_ref).  Measured worst
    err / bound: 0.098 on dx (5.0e-6 absolute at most), 0.004 on dgamma / dbeta (6.6e-4 absolute at M = 38080)."""
    _ln_family(f"layernorm_bwd[{entry}]", entry, M, 768, 1.0, 100 + M % 97)


@pytest.mark.parametrize("D", [384, 768])
@pytest.mark.parametrize("M", [4097, 24 * 1000])
def test_ln_bwd_any_grid_stride_vs_float64(M, D):
    """sed_ln_bwd_any (PMAM context network: M = B T at B = 24, T = 1000) past the 1024-block cap, in_scale = 2.5 as the first
    decoder layer uses sqrt(D).  Measured worst err / bound: 0.108 on dx, 0.004 on dgamma / dbeta."""
    _ln_family(f"ln_bwd_any D={D}", "any", M, D, 2.5, 200 + D)


def test_fpool_bwd_batch32_vs_float64():
    """sed_fpool_bwd at B = 32, tp = 99 (38080 token rows through the grid-stride LayerNorm backward with dy = dpooled / 12; rows 0-1
    of every clip carry dy = 0 against zero placeholder statistics).  Measured worst err / bound: 0.41 on dx (5.0e-7 absolute), 0.004
    on dgamma, 0.010 on dbeta."""
    B, tp, D = 32, 99, 768
    N = 2 + 12 * tp
    M = B * N
    x, _, g, mu, rs = ln_inputs(M, D, 300, 1.0, 1e-5)
    dpool = randn(B, tp, D, seed=303) * (1 + 0.1 * torch.arange(B, device=DEV).view(B, 1, 1))
    tok = torch.zeros(B, N, dtype=torch.bool, device=DEV); tok[:, 2:] = True
    tok = tok.view(-1)
    mu[~tok] = 0.0; rs[~tok] = 0.0                    # what the host leaves there
    inv12 = float(np.float32(1.0 / 12.0))
    dy = torch.zeros(B, N, D, dtype=torch.float64, device=DEV)
    dy[:, 2:] = (dpool.double() * inv12).unsqueeze(1).expand(B, 12, tp, D).reshape(B, 12 * tp, D)
    dy = dy.view(M, D)
    nb = 1024
    dx, dgr, dbr, bx, bg, bb, tg, tb = ln_bwd_ref(dy, x, mu, rs, g, 1.0, nb)
    bx = bx + 2 * U32 * 24 * rs.double().unsqueeze(1) * dy.abs()     # (dy = dpooled * fl(1/12) rounded once more in the kernel)
    base = randn(B, N, D, seed=304)
    acc = base.clone()
    dtok = torch.empty(B, N, D, device=DEV)
    dgk, dbk = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    call("sed_fpool_bwd", dpool, x, mu, rs, g, dtok, acc, dgk, dbk, B, tp)
    want = base.view(M, D).double() + dx
    sl = drop_rows(M, nb)
    check("fpool_bwd B=32 dx", acc.view(M, D), want, bx + U32 * want.abs() + 1e-30, only(dx, sl))
    # the last clip of the batch as the left-out contribution for the parameter gradients
    last = slice((B - 1) * N, M)
    check("fpool_bwd B=32 dgamma", dgk, dgr, bg, tg[last].sum(0))
    check("fpool_bwd B=32 dbeta", dbk, dbr, bb, tb[last].sum(0))
    assert torch.equal(acc[:, :2], base[:, :2])
    check("fpool_bwd B=32 dgamma (one row block past the first pass)", dgk, dgr, bg, tg[sl].sum(0))
    check("fpool_bwd B=32 dbeta (one row block past the first pass)", dbk, dbr, bb, tb[sl].sum(0))


# ------------------------------------------------------------------------------------------------ token assembly backward
def assemble_bwd_ref(dx, tp, nsplit):
    """float64 table gradients of sed_assemble_tokens_bwd and their bounds.  Each (job, d-chunk, slice) block adds its slice's
    ceil(B / nsplit) clips serially (x tp time steps for a frequency row, x 12 rows for a time column), the slices meet in an atomic
    chain."""
    B, N, D = dx.shape
    x = dx.double()
    bper = -(-B // nsplit)
    sl = [slice(z * bper, min(B, (z + 1) * bper)) for z in range(nsplit)]
    out, bound, per_clip = {}, {}, {}
    d4 = x[:, 2:].view(B, 12, tp, D)
    terms = {"cls": (x[:, 0], 1), "dist": (x[:, 1], 1),
             "freq": (d4.sum(2).transpose(1, 2), tp),            # [B, D, 12]  (kept per clip: the serial inner loop)
             "time": (d4.sum(1).transpose(1, 2), 12)}            # [B, D, tp]
    absd = {"cls": x[:, 0].abs(), "dist": x[:, 1].abs(), "freq": d4.abs().sum(2).transpose(1, 2), "time": d4.abs().sum(1).transpose(1, 2)}
    for k, (t, inner) in terms.items():
        parts = torch.stack([t[s].sum(0) for s in sl])
        out[k] = t.sum(0)
        bound[k] = U32 * bper * inner * absd[k].sum(0) + chain(parts) + 1e-30
        per_clip[k] = t
    return out, bound, per_clip


@pytest.mark.parametrize("B,tp,toffset", [(1, 99, 0), (7, 99, 0), (8, 99, 0), (9, 99, 0), (13, 99, 0), (24, 99, 0), (32, 99, 0),
                                          (32, 50, 49)])
def test_assemble_tokens_bwd_batch_slices_vs_float64(B, tp, toffset):
    """sed_assemble_tokens_bwd across its batch split (grid.z = min(B, 8), ceil(B / 8) clips per slice; B = 9 and 13 leave uneven
    and empty slices), and one sliding-window slab (tp = 50 at a time offset).  All five table gradients against float64 sums, dconv ==
    bf16(dx) on every row.  Measured worst err / bound: 0.32 (cls / dist at B = 7), 0.27 (time), 0.027 (freq)."""
    D = 768
    N = 2 + 12 * tp
    dx = randn(B, N, D, seed=400 + B + tp) * (1 + 0.05 * torch.arange(B, device=DEV).view(B, 1, 1))
    dconv = torch.empty(B * 12 * tp, D, dtype=BF16, device=DEV)
    z = lambda *s: torch.zeros(*s, device=DEV)
    dcls, ddist, dnp, dfr, dti = z(D), z(D), z(2, D), z(D, 12), z(D, 99)
    call("sed_assemble_tokens_bwd", dx, dconv, dcls, ddist, dnp, dfr, dti, toffset, B, tp)
    assert torch.equal(dconv, dx[:, 2:].reshape(-1, D).to(BF16))
    ref, bnd, pc = assemble_bwd_ref(dx, tp, min(B, 8))
    tag = f"assemble_bwd B={B} tp={tp} toff={toffset}"
    check(f"{tag} cls", dcls, ref["cls"], bnd["cls"], pc["cls"][B - 1])
    check(f"{tag} dist", ddist, ref["dist"], bnd["dist"], pc["dist"][B - 1])
    check(f"{tag} new_pos[0]", dnp[0], ref["cls"], bnd["cls"], pc["cls"][B - 1])
    check(f"{tag} new_pos[1]", dnp[1], ref["dist"], bnd["dist"], pc["dist"][B - 1])
    check(f"{tag} freq", dfr, ref["freq"], bnd["freq"], pc["freq"][B - 1])
    check(f"{tag} time", dti[:, toffset:toffset + tp], ref["time"], bnd["time"], pc["time"][B - 1])
    # columns of the time table outside the slab are untouched
    assert float(dti[:, :toffset].abs().max() if toffset else 0.0) == 0.0 and float(dti[:, toffset + tp:].abs().max() if toffset + tp < 99 else 0.0) == 0.0


# ------------------------------------------------------------------------------------------------ rel-pos attention
def _relpos_inputs(B, T, DT, seed):
    Tpad, R = pad64(T), 2 * T - 1
    Rpad = pad64(R)
    f16 = 1 if DT == F16 else 0
    mk = lambda s, sc: randn(B * H, T, 64, seed=seed + s, scale=sc).to(BF16).float()
    qu, qv, k, v = mk(0, 1.2), mk(1, 1.2), mk(2, 1.2), mk(3, 1.0)
    tr = lambda t: torch.nn.functional.pad(t.transpose(1, 2), (0, Tpad - T)).to(BF16).contiguous()
    P = randn(H, R, 64, seed=seed + 4, scale=0.7).to(BF16).float()
    Pp = torch.zeros(H, Rpad, 64, dtype=DT, device=DEV); Pp[:, :R] = P.to(DT)
    Pt = torch.zeros(H, 64, Rpad, dtype=BF16, device=DEV); Pt[:, :, :R] = P.to(BF16).transpose(1, 2)
    vt = torch.nn.functional.pad(v.transpose(1, 2), (0, Tpad - T)).to(DT).contiguous()
    dO = randn(B, T, 768, seed=seed + 5).to(BF16)
    return dict(B=B, T=T, Tpad=Tpad, Rpad=Rpad, f16=f16, DT=DT, qu=qu.to(DT), qv=qv.to(DT), k=k.to(DT), v16=v.to(BF16), vt=vt,
                qut=tr(qu), qvt=tr(qv), kt=tr(k), Pp=Pp, Pt=Pt, dO=dO)


def _relpos_fwd(a):
    B, T = a["B"], a["T"]
    O = torch.empty(B, T, 768, dtype=a["DT"], device=DEV)
    lse = torch.empty(B * H, T, device=DEV)
    call("sed_relpos_attn_fwd", a["qu"], a["qv"], a["k"], a["vt"], a["Pp"], O, None, lse, B, H, T, a["Tpad"], a["Rpad"], a["f16"], 0)
    return O, lse


def _relpos_bwd(a, O, lse, stream_kv):
    B, T, Tpad, Rpad = a["B"], a["T"], a["Tpad"], a["Rpad"]
    dqkv = torch.empty(B * T, 2304, dtype=BF16, device=DEV)
    Dt = torch.empty(B * H, T, device=DEV)
    dOh = torch.empty(B * H, T, 64, dtype=BF16, device=DEV)
    dOt = torch.empty(B * H, 64, Tpad, dtype=BF16, device=DEV)
    dSt = torch.zeros(B * H, Tpad, Tpad, dtype=BF16, device=DEV)
    Pst = torch.zeros(B * H, Tpad, Tpad, dtype=BF16, device=DEV) if stream_kv else None
    dP = torch.zeros(Rpad, 768, device=DEV)
    du, dv = torch.zeros(H, 64, device=DEV), torch.zeros(H, 64, device=DEV)
    call("sed_relpos_attn_bwd", a["qu"], a["qut"], a["qv"], a["qvt"], a["k"], a["kt"], a["v16"], a["Pp"], a["Pt"], O, a["dO"],
         lse, Dt, dOh, dOt, dqkv, dSt, Pst, dP, du, dv, B, H, T, Tpad, Rpad, 1, a["f16"], a["f16"])
    return dict(dqkv=dqkv, dSt=dSt, Pst=Pst, dP=dP, du=du, dv=dv)


def relpos_param_grads_ref(dSt, qv, k, P, B, T, Tpad):
    """float64 dP [R, H 64], du / dv [H, 64] from the dS^T slab the kernel wrote (its own bf16 dS) and the bf16 / f16 operands it read,
    one clip at a time, with the bounds of the kernels' summation trees and each clip's own contribution (for the drop check).

    dP (relpos_bwd_dp_kernel): per workgroup an MFMA chain over its slice's clips x query tiles x 4 k-steps of 16 products, then one
    atomic per slice -> kappa = 16 + 4 ceil(T / 64) ceil(B / 8) plus `chain` over the slice partials.
    du / dv (dQ kernel): per query an MFMA chain over the key tiles (<= 3 Tpad / 64 steps of 32 products), a 16-query butterfly (4), then
    one atomic per (clip, 16-query group) -> kappa = 3 Tpad / 64 + 32 + 4 plus `chain` over the group partials."""
    R = 2 * T - 1
    nsplit = min(B, 8)
    bper = -(-B // nsplit)
    ng = -(-T // 16)
    i = torch.arange(T, device=DEV).view(1, T)
    r = torch.arange(R, device=DEV).view(R, 1)
    j = i + r - (T - 1)
    ok = (j >= 0) & (j < T)
    idx = j.clamp(0, T - 1).expand(H, R, T)
    P64 = P.double()
    dP = torch.zeros(H, R, 64, dtype=torch.float64, device=DEV); dPa = torch.zeros_like(dP)
    dP_split = torch.zeros(nsplit, H, R, 64, dtype=torch.float64, device=DEV)
    du = torch.zeros(H, 64, dtype=torch.float64, device=DEV); dua = torch.zeros_like(du)
    dv = torch.zeros_like(du); dva = torch.zeros_like(du)
    du_parts, dv_parts = [], []
    last = {}
    for b in range(B):
        S = dSt[b * H:(b + 1) * H, :T, :T].double()                   # [H, key j, query i]
        G = S.gather(1, idx) * ok                                     # [H, r, i] = dS[i, i + r - (T - 1)]
        Q = qv[b * H:(b + 1) * H].double()                            # [H, T, 64]
        Kb = k[b * H:(b + 1) * H].double()
        c = SCALE * torch.bmm(G, Q)
        dP += c; dP_split[b // bper] += c
        dPa += SCALE * torch.bmm(G.abs(), Q.abs())
        Sq = torch.nn.functional.pad(S, (0, ng * 16 - T)).view(H, T, ng, 16).sum(-1)      # [H, key, group]
        Gq = torch.nn.functional.pad(G, (0, ng * 16 - T)).view(H, R, ng, 16).sum(-1)      # [H, r, group]
        pu = SCALE * torch.einsum("hkg,hkd->ghd", Sq, Kb)
        pv = SCALE * torch.einsum("hrg,hrd->ghd", Gq, P64)
        du_parts.append(pu); dv_parts.append(pv)
        du += pu.sum(0); dv += pv.sum(0)
        dua += SCALE * torch.einsum("hk,hkd->hd", S.abs().sum(2), Kb.abs())
        dva += SCALE * torch.einsum("hr,hrd->hd", G.abs().sum(2), P64.abs())
        if b == B - 1:
            last = dict(dP=c, du=pu.sum(0), dv=pv.sum(0))
        del S, G
    tiles = -(-T // 64)
    kdp = 16 + 4 * tiles * bper
    bdp = U32 * kdp * dPa + chain(dP_split) + 1e-30
    kd = 3 * Tpad // 64 + 32 + 4
    bdu = U32 * kd * dua + chain(torch.cat(du_parts)) + 1e-30
    bdv = U32 * kd * dva + chain(torch.cat(dv_parts)) + 1e-30
    flat = lambda t: t.permute(1, 0, 2).reshape(R, H * 64)
    return (flat(dP), flat(bdp), flat(last["dP"])), (du, bdu, last["du"]), (dv, bdv, last["dv"])


@pytest.mark.parametrize("stream_kv", [True, False], ids=["Pst", "recompute"])
@pytest.mark.parametrize("DT", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("B,T", [(8, 200), (9, 200), (13, 200), (24, 1000), (32, 1000)])
def test_relpos_bwd_param_grads_batch_slices_vs_float64(B, T, DT, stream_kv):
    """sed_relpos_attn_bwd's dP (bsplit = min(B, 8) slices of ceil(B / 8) clips: one clip per slice at B = 8, uneven and empty slices
    at B = 9 / 13, 3 and 4 clips at the production B = 24 / 32) and the pos_bias_u / pos_bias_v gradients, against float64 sums of the
    kernel's own dS^T slab -- the reduction isolated from the rounding upstream of it.  Both dK / dV paths (they write the same slab).
    Measured worst err / bound: 0.098 on dP, 0.004 on du / dv."""
    a = _relpos_inputs(B, T, DT, 500 + B)
    O, lse = _relpos_fwd(a)
    out = _relpos_bwd(a, O, lse, stream_kv)
    R = 2 * T - 1
    (dPr, bdp, ldp), (dur, bdu, ldu), (dvr, bdv, ldv) = relpos_param_grads_ref(out["dSt"], a["qvt"][:, :, :T].transpose(1, 2).float(),
                                                                              a["k"], a["Pp"][:, :R].float(), B, T, a["Tpad"])
    tag = f"relpos_bwd B={B} T={T} {'f16' if a['f16'] else 'bf16'} {'Pst' if stream_kv else 'recompute'}"
    check(f"{tag} dP", out["dP"][:R], dPr, bdp, ldp)
    assert float(out["dP"][R:].abs().max()) == 0.0 if a["Rpad"] > R else True
    check(f"{tag} du", out["du"], dur, bdu, ldu)
    check(f"{tag} dv", out["dv"], dvr, bdv, ldv)


# ------------------------------------------------------------------------------------------------ batch invariance
def _picks(B):
    # first, last, middle, and the clips on both sides of an 8-(clip, head) boundary of attn_xcd_order (bh = 24 between clips 1 and 2)
    return sorted({0, 1, 2, B // 2, B - 1})


def _mhsa_inputs(B, N, DT, seed):
    mk = lambda s: randn(B * H, N, 64, seed=seed + s, scale=1.3).to(DT)
    return mk(0), mk(1), mk(2), randn(B, N, 768, seed=seed + 3).to(BF16)


def _mhsa_run(q, k, v, dO, B, N, f16):
    Npad = pad64(N)
    DT = q.dtype
    O = torch.empty(B, N, 768, dtype=DT, device=DEV)
    lse = torch.empty(B * H, N, device=DEV)
    call("sed_mhsa_fwd", q, k, v, O, lse, B, H, N, Npad, f16)
    Oh = torch.empty(B, N, 768, dtype=DT, device=DEV)
    call("sed_mhsa_fwd", q, k, v, Oh, torch.empty_like(lse), B, H, N, Npad, f16 | 2)
    dqkv = torch.empty(B * N, 2304, dtype=BF16, device=DEV)
    Dt = torch.empty(B * H, N, device=DEV)
    call("sed_mhsa_bwd", q, k, v, O, dO, lse, Dt, None, dqkv, B, H, N, Npad, f16, f16)
    return O, lse, Oh.view(H, B, N, 64), dqkv.view(B, N, 2304), Dt


@pytest.mark.parametrize("DT", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("B,N", [(352, 602), (32, 1190)])
def test_mhsa_per_sequence_batch_invariance(B, N, DT):
    """sed_mhsa_fwd (O, LSE; row-major and head-major output) and sed_mhsa_bwd (dqkv, D) at the teacher's 11-window shape (352 x 12
    sequences of 602 tokens) and the student's (32 x 12 of 1190): chosen sequences run alone (B = 1: 12 (clip, head) pairs, so the XCD
    order is off) must give the same bits as inside the batch.  No output of these kernels is reduced across sequences.  Measured: all
    bit-identical."""
    f16 = 1 if DT == F16 else 0
    q, k, v, dO = _mhsa_inputs(B, N, DT, 600 + N)
    O, lse, Oh, dqkv, Dt = _mhsa_run(q, k, v, dO, B, N, f16)
    for b in _picks(B):
        hs = slice(b * H, (b + 1) * H)
        O1, lse1, Oh1, dqkv1, Dt1 = _mhsa_run(q[hs].contiguous(), k[hs].contiguous(), v[hs].contiguous(), dO[b:b + 1].contiguous(), 1, N, f16)
        assert torch.equal(O[b], O1[0]), ("O", b)
        assert torch.equal(lse[hs], lse1), ("lse", b)
        assert torch.equal(Oh[:, b], Oh1[:, 0]), ("O head-major", b)
        assert torch.equal(dqkv[b], dqkv1[0]), ("dqkv", b)
        assert torch.equal(Dt[hs], Dt1), ("D", b)
    report(f"mhsa B={B} N={N} {DT}: per-sequence outputs bit-identical for clips {_picks(B)}", 0.0)


@pytest.mark.parametrize("DT", [BF16, F16], ids=["bf16", "f16"])
def test_relpos_per_sequence_batch_invariance(DT):
    """sed_relpos_attn_fwd (O, LSE) and the per-sequence outputs of sed_relpos_attn_bwd (dqkv, the dS^T and P^T slabs) at 32 x 12
    sequences of 1000 frames against the same sequences run alone, bit for bit, on both dK / dV paths.  dP, du and dv are summed over
    the batch by atomics (their order depends on the batch): they are checked against float64 in the test above."""
    B, T = 32, 1000
    a = _relpos_inputs(B, T, DT, 700)
    O, lse = _relpos_fwd(a)
    full = {kv: _relpos_bwd(a, O, lse, kv) for kv in (True, False)}
    for b in _picks(B):
        hs = slice(b * H, (b + 1) * H)
        a1 = dict(a, B=1, dO=a["dO"][b:b + 1].contiguous())
        for key in ("qu", "qv", "k", "v16", "vt", "qut", "qvt", "kt"):
            a1[key] = a[key][hs].contiguous()
        O1, lse1 = _relpos_fwd(a1)
        assert torch.equal(O[b], O1[0]) and torch.equal(lse[hs], lse1), ("fwd", b)
        for kv in (True, False):
            o1 = _relpos_bwd(a1, O1, lse1, kv)
            f = full[kv]
            assert torch.equal(f["dqkv"].view(B, T, 2304)[b], o1["dqkv"]), ("dqkv", b, kv)
            assert torch.equal(f["dSt"][hs], o1["dSt"]), ("dSt", b, kv)
            if kv:
                assert torch.equal(f["Pst"][hs], o1["Pst"]), ("Pst", b)
    assert torch.equal(full[True]["dqkv"][:, :768], full[False]["dqkv"][:, :768])
    report(f"relpos B={B} T={T} {DT}: per-sequence outputs bit-identical for clips {_picks(B)}", 0.0)


# ------------------------------------------------------------------------------------------------ model level: every clip counts
GRAD_REL = 1e-3         # per tensor, norm-wise against sum_k ||g_pair k|| (test_gpu_model's B = 32 vs B = 2 comparison allows 1e-2)


def test_depth2_batch32_gradients_are_the_sum_of_pair_runs():
    """The depth-2 MAT-SED student at D = 768, B = 32, train mode, with a loss that weights EVERY clip (its own det_uniform weights):
    per parameter the B = 32 gradient must equal the float64 sum of the sixteen B = 2 runs on the same clip pairs, norm-wise within
    GRAD_REL of sum_k ||g_k|| (so tensors whose pair gradients cancel need no exemption), and leaving out the last pair must move that
    sum by >= 3x the bound.  Strong / weak / AT posteriors of every clip match the clip's pair run within 2e-4, and so does the 11-window
    teacher forward at B = 32.  (PMAM is not run here: its batch-norm statistics couple the clips.)
    Measured: worst gradient ratio 3.1e-4 (decoder.encoder_blocks.2.attn.linear_pos.weight), smallest share of the last pair 2.8e-2;
    student posteriors bit-identical to the pair runs, 11-window teacher posteriors within 8.4e-5."""
    from transformer4sed_amd.passt_sed import PaSST_SED
    B = 32
    tag = "batch_scale_d2"
    mel = torch.from_numpy(synth.det_uniform(f"{tag}/mel", (B, 128, 1000), -1.2, 1.2)).to(DEV)
    net = PaSST_SED(passt_feature_layer=2, f_pool="mean_pool", decode_ratio=10, at_adapter=True, decoder="transformerXL",
                    decoder_layer_num=3, decoder_pos_emd_len=1000, mlm=False, load_pretrained_model=False, encoder_depth=2)
    sd = synth.matsed_state_dict_np(tag="w768", depth=12)
    own = net.state_dict()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items() if k in own}, strict=True)
    net = net.to(DEV).train()
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

    # (the B = 32 run first: it fixes the loss weights' shapes)
    out32, g32 = run(0, B)
    gsum = {n: torch.zeros_like(g, dtype=torch.float64) for n, g in g32.items()}
    gnorm = {n: 0.0 for n in g32}
    glast = {}
    worst_post = 0.0
    for k in range(B // 2):
        outk, gk = run(2 * k, 2 * k + 2)
        for nm, a, b in zip(("strong", "weak", "at"), out32, outk):
            d = float((a[2 * k:2 * k + 2] - b).abs().max())
            worst_post = max(worst_post, d)
            assert d < 2e-4, (nm, k, d)
        assert set(gk) == set(g32)
        for n, g in gk.items():
            gsum[n] += g.double()
            gnorm[n] += float(g.double().norm())
        if k == B // 2 - 1:
            glast = {n: float(g.double().norm()) for n, g in gk.items()}
    report("B=32 depth2: worst posterior difference vs pair runs (strong, weak, AT)", worst_post)
    rel = {n: float((g.double() - gsum[n]).norm()) / gnorm[n] for n, g in g32.items()}
    share = {n: glast[n] / gnorm[n] for n in g32}
    wn, sn = max(rel, key=rel.get), min(share, key=share.get)
    report(f"B=32 depth2: worst |g32 - sum g_pair| / sum |g_pair| ({wn})", rel[wn])
    report(f"B=32 depth2: smallest share of the last pair in sum |g_pair| ({sn})", share[sn])
    for n in g32:
        assert rel[n] < GRAD_REL, (n, rel[n])
        assert share[n] >= 3 * GRAD_REL, (n, "the bound cannot see a dropped pair", share[n])
    # ---- the 11-window teacher forward at B = 32 against the pair runs
    net.eval()
    with torch.no_grad():
        s3, w3, o3 = net(mel, encoder_win=True, mix_rate=0.5, win_param=[512, 49], temp_w=1)
        worst_win = 0.0
        for k in range(B // 2):
            s2, w2, o2 = net(mel[2 * k:2 * k + 2].contiguous(), encoder_win=True, mix_rate=0.5, win_param=[512, 49], temp_w=1)
            for nm, a, b in (("strong", s3, s2), ("weak", w3, w2), ("at", o3["at_out"], o2["at_out"])):
                d = float((a[2 * k:2 * k + 2] - b).abs().max())
                worst_win = max(worst_win, d)
                assert d < 2e-4, ("11 windows", nm, k, d)
    report("B=32 depth2 11 windows: worst posterior difference vs pair runs", worst_win)
