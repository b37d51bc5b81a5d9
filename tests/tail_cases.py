"""Cases, inputs, float64 references and error bounds for the kernels every training step ends in (csrc/norm_elem.hip, csrc/layout.hip):
sed_head_fwd / _bwd, sed_attnpool_fwd / _bwd, sed_small_linear / _bwd, sed_mlm_apply / _bwd, sed_masked_mse, sed_sed_losses and
sed_adamw_ema.  Pure construction helpers: no tests, no GPU code, no torch.nn loss or optimizer module.  Every function works on the
device of its arguments, so tests/test_tail_cases_cpu.py proves references and bounds on the CPU and tests/test_gpu_tail_kernels.py
holds the hardware to them (and may evaluate a large reference in float64 on the device).

Inputs come from a CPU generator with fixed seeds.  References are closed forms in float64 on the fp32 (or 16-bit) values the kernel
reads; a backward reference takes what the forward kernel saved (strong, sums, probs, out) as an input, so that a reduction is judged
apart from the rounding of the forward.  Bounds are error models, u = 2^-24:

  a sum            u * (kappa * sum|terms| + propagated input error) + chain(partials)    kappa = depth of the kernel's summation tree
                   for the terms of one workgroup, chain() = the worst-order bound of the atomic adds that merge the workgroups
  a 16-bit output  half an ulp of bf16 on the float64 value + the fp32 error of the value before it is rounded
  __expf / logf    the model of everything around the intrinsic + K u * unit, with one measured constant K (K_EXP, K_LOG)

Every `*_drops` function names contributions (one 16-row block past the first grid pass, the rows of the second pass, the last clip,
...) whose removal has to move the reference by >= 10x the bound: a bound that cannot see them proves nothing."""
import collections
import math

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
U32 = 2.0 ** -24            # unit roundoff of fp32
D = 768                     # the kernels are compiled for DM = 768
H = 12
TINY = 1e-30                # added to bounds so that an exact 0 compares as 0 <= bound
SENS = 10.0                 # a dropped contribution has to be this many bounds large

# Relative error of __expf(a), in units of u (1 + |a|): v_exp_f32 after one fp32 product with log2(e).  Measured on an MI355X as
# max (|err| - det) / (u unit) over every head, small-linear and attention-pooling case of this file: -12.7 (strong), -11.2 (small
# linear), -12.0 (probs) -- negative: the worst-case model of everything around the intrinsic (`det`) covers every measured error by
# itself, so the measurements ask for no constant at all.  The rule "next power of two above twice the worst value seen" has nothing
# positive to start from; K = 2^0 keeps one unit of the intrinsic's own rounding in the model and is the smallest constant used.
K_EXP = 1.0
# Error of logf(x) in units of u |log x|.  Measured the same way over the six sums of every loss case: -12.2 at most; as above.
K_LOG = 1.0

# what test_gpu_kernels.py asserts for the same outputs: no bound of this file may be looser
LEGACY_STRONG = 2e-5
LEGACY_POOLED = 1e-4
LEGACY_LOSS_REL = 2e-6
LEGACY_GRAD_REL = 1e-6


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=gen(seed)) * scale


def f32(v):
    """v rounded to fp32, as a Python float: the value a `float` argument of the C ABI carries."""
    return float(np.float32(v))


def chain(parts):
    """Rounding bound of an atomic chain that adds the float64 partials parts[0..n-1] (leading dim) in an unknown order:
    sum_k u |S_k| over the running sums, largest partials first (the worst order).  (As in tests/test_gpu_batch_scale.py.)"""
    a = parts.abs().sort(dim=0, descending=True).values
    w = torch.arange(a.shape[0], 0, -1, dtype=a.dtype, device=a.device).view(-1, *([1] * (a.dim() - 1)))
    return U32 * (a * w).sum(0)


def only(t, rows):
    """t with everything outside `rows` (leading dim) zeroed: the contribution of those rows alone."""
    z = torch.zeros_like(t)
    z[rows] = t[rows]
    return z


def sens(drop, bound):
    """How many bounds the removal of a contribution moves the reference by, at the most sensitive element."""
    return float((drop.abs() / bound).max())


def cdiv(a, b):
    return -(-a // b)


# ================================================================================================ SED head
# sed_head_fwd: one wave per row, a lane adds 12 products serially, 6 butterfly levels -> 18 roundings on sum|x w|, 2 more for the bias
# and the temperature; weak_pool: a thread adds ceil(T / 256) values, 6 levels, 3 LDS adds.
# sed_head_bwd: 256 workgroups x 4 waves, wave slot = block % 1024 owns 16-row blocks slot, slot + 1024, ...: first pass 16384 rows.
HEAD_SLOTS, HEAD_BLOCK = 1024, 16
HEAD_FIRST_PASS = HEAD_SLOTS * HEAD_BLOCK
HEAD_KAPPA_DL = 10          # roundings of one dlogit: 2 s B, - A, B B, /, * dweak, + dstrong, * s, 1 - s, *, / temp

HeadCase = collections.namedtuple("HeadCase", "name B T C temp pad shift bwd")


def _hc(B, T, temp, pad="none", C=10, shift=0.0, bwd=True):
    return HeadCase(f"B{B}-T{T}-C{C}-temp{temp}-{pad}" + ("-lowbias" if shift else ""), B, T, C, temp, pad, shift, bwd)


# pad: 'none'; 'single' = clip 0 keeps one valid frame; 'full' = clip 0 is padded entirely (needs B >= 2: the other clips are not).
# In the padded cases with B >= 3 clip 1 also loses its last third (the last clip stays whole: the drop checks remove it).  The low-bias case runs at temp = 1 only: at temp = 0.5 its s^2
# reaches 1e-39, below the fp32 normal range, and float64 does not model what the hardware does with denormals.
HEAD_CASES = [
    _hc(1, 1, 1.0), _hc(1, 1, 0.5),
    _hc(2, 15, 1.0), _hc(2, 15, 0.5, "single"), _hc(2, 15, 1.0, "full"),
    _hc(3, 257, 0.5), _hc(3, 257, 1.0, "single"), _hc(3, 257, 0.5, "full"), _hc(3, 257, 1.0, shift=-20.0),
    _hc(17, 1000, 1.0), _hc(17, 1000, 0.5, "single"), _hc(17, 1000, 1.0, "full"),
    _hc(3, 257, 1.0, "single", C=1, bwd=False), _hc(3, 257, 0.5, "full", C=16, bwd=False),
]
HEAD_FORMS = ("both", "dstrong", "dweak")


def head_inputs(case):
    seed = 1000 + 31 * case.B + case.T + 7 * case.C + int(10 * case.temp)
    B, T, C = case.B, case.T, case.C
    x = randn(B, T, D, seed=seed) * (1.0 + 0.02 * torch.arange(B, dtype=F32).view(B, 1, 1))    # no two clips alike
    W = randn(C, D, seed=seed + 1, scale=0.03)
    b = randn(C, seed=seed + 2, scale=0.3) + case.shift
    pm = torch.zeros(B, T, dtype=torch.uint8)
    if case.pad == "single":
        pm[0, 1:] = 1
    elif case.pad == "full":
        pm[0, :] = 1
    if case.pad != "none" and B >= 3:
        pm[1, T - T // 3:] = 1
    ds = randn(B, C, T, seed=seed + 3)
    dw = randn(B, C, seed=seed + 4)
    return dict(x=x, W=W, b=b, pm=pm, ds=ds, dw=dw)


def head_fwd_ref(x, W, b, temp, pm):
    """-> strong [B, C, T] in float64, and its bound split as det + K_EXP u unit."""
    xd, Wd, bd = x.double(), W.double(), b.double()
    logit = xd @ Wd.t() + bd
    z = logit / temp
    s = torch.sigmoid(z)
    absdot = xd.abs() @ Wd.abs().t()
    dz = U32 * (18 * absdot + 2 * (absdot + bd.abs())) / temp
    live = (pm == 0).unsqueeze(-1).to(F64)
    s = s * live                                                            # masked rows: exactly 0
    det = (s * (1 - s) * dz + 3 * U32 * s) * live                           # 1 + e, the division, and one to spare
    unit = s * (1 - s) * (1 + z.abs()) * live
    return s.transpose(1, 2).contiguous(), det.transpose(1, 2).contiguous(), unit.transpose(1, 2).contiguous()


def head_strong_bound(det, unit):
    return det + K_EXP * U32 * unit + TINY


def head_pool_ref(strong):
    """weak [B, C] and sums [B, C, 2] = (A, B) from a given `strong` (the kernel's own), with their bounds.  All terms are >= 0, so
    the summation error is relative: kappa = ceil(T / 256) + 6 + 3, one more for the square; A / B doubles it, the division and the
    clamp constant (1e-7 as fp32) add two."""
    s = strong.double()
    T = s.shape[-1]
    A, Bs = (s * s).sum(-1), s.sum(-1)
    weak = torch.clamp(A / Bs, 1e-7, 1.0)                                   # NaN (0 / 0: every frame padded) stays NaN
    kap = cdiv(T, 256) + 6 + 3
    sums = torch.stack([A, Bs], -1)
    return weak, sums, U32 * (2 * kap + 4) * weak + TINY, U32 * (kap + 1) * sums + TINY


def head_ratio(sums):
    s = sums.double()
    return s[..., 0] / s[..., 1]


def head_wg_of_rows(nrows, device="cpu"):
    blk = torch.arange(nrows, device=device) // HEAD_BLOCK
    return (blk % HEAD_SLOTS) // 4


def head_bwd_ref(x, W, strong, sums, ds, dw, temp):
    """Backward of the head from the saved `strong` [B, C, T] and `sums` [B, C, 2]; ds / dw may be None.  -> dict with dx [B T, D],
    dW [C, D], db [C], their bounds bx / bW / bb, and dl [B T, C] (dlogit) for the drop checks.

    dx: 10 products added serially (kappa 10) on dlogits that carry HEAD_KAPPA_DL roundings each.  dW / db: a wave adds the rows of its
    blocks serially -- 16 ceil(nblk / 1024) terms -- 2 LDS levels, 1 product, plus the dlogit's own; the 256 workgroups meet in an
    atomic chain.  Cancellation inside 2 s B - A is covered by carrying |dstrong| + |dweak| (2 s B + A) / B^2 as the dlogit's size."""
    s = strong.double().transpose(1, 2)
    Bn, T, C = s.shape
    xd, Wd = x.double().reshape(Bn * T, -1), W.double()
    g = ds.double().transpose(1, 2) if ds is not None else torch.zeros_like(s)
    ga = g.abs()
    if dw is not None:
        A, Bs = sums[..., 0].double().unsqueeze(1), sums[..., 1].double().unsqueeze(1)
        r = A / Bs
        gate = (r > 1e-7) & (r < 1.0)                                       # NaN: closed
        zero = torch.zeros_like(s)
        g = g + dw.double().unsqueeze(1) * torch.where(gate, (2 * s * Bs - A) / (Bs * Bs), zero)
        ga = ga + dw.double().abs().unsqueeze(1) * torch.where(gate, (2 * s * Bs + A) / (Bs * Bs), zero)
    sig = s * (1 - s) / temp
    dl, dla = (g * sig).reshape(Bn * T, C), (ga * sig).reshape(Bn * T, C)
    nrows = Bn * T
    dx = dl @ Wd
    bx = U32 * (10 + HEAD_KAPPA_DL) * (dla @ Wd.abs()) + TINY
    rpw = HEAD_BLOCK * cdiv(cdiv(nrows, HEAD_BLOCK), HEAD_SLOTS)
    kap = rpw + 2 + 1 + HEAD_KAPPA_DL
    wg = head_wg_of_rows(nrows, dl.device)
    nwg = int(wg.max()) + 1
    order = torch.argsort(wg, stable=True)
    counts = torch.bincount(wg, minlength=nwg).tolist()
    pW = torch.stack([dl[idx].t() @ xd[idx] for idx in torch.split(order, counts)])
    pb = torch.zeros(nwg, C, dtype=F64, device=dl.device).index_add_(0, wg, dl)
    bW = U32 * kap * (dla.t() @ xd.abs()) + chain(pW) + TINY
    bb = U32 * kap * dla.sum(0) + chain(pb) + TINY
    return dict(dl=dl, dx=dx, dW=dl.t() @ xd, db=dl.sum(0), bx=bx, bW=bW, bb=bb)


def head_drops(B, T):
    """{name: rows (slice of the B T rows)} of the contributions whose loss the bounds have to see."""
    nrows = B * T
    d = {}
    if nrows > HEAD_FIRST_PASS:
        d["block past the first pass"] = slice(HEAD_FIRST_PASS, min(HEAD_FIRST_PASS + HEAD_BLOCK, nrows))
        d["second pass"] = slice(HEAD_FIRST_PASS, nrows)
    else:
        d["last block"] = slice((cdiv(nrows, HEAD_BLOCK) - 1) * HEAD_BLOCK, nrows)
    if B > 1:
        d["last clip"] = slice((B - 1) * T, nrows)
    return d


def head_drop_values(ref, x, rows):
    xd = x.double().reshape(ref["dl"].shape[0], -1)
    dl = ref["dl"][rows]
    return dict(dx=only(ref["dx"], rows), dW=dl.t() @ xd[rows], db=dl.sum(0))


# ================================================================================================ attention pooling
# attnpool_fwd / _bwd: one workgroup per (b, h).  Scores: one lane per token, a 64-term serial dot; softmax sums: ceil(P / 256) per
# thread, 6 levels, 3 LDS adds; weighted sums over tokens: wave w takes tokens w, w + 4, ... serially -- ceil(P / 4) terms, eight at a
# time while t + 28 < P, then a tail -- and 3 LDS adds; dq: an atomic chain over the B clips.
PoolCase = collections.namedtuple("PoolCase", "name B P f16")
POOL_P = (1, 3, 4, 5, 28, 29, 33, 256, 257, 600, 792)
POOL_CASES = [PoolCase(f"B2-P{P}-{'f16' if f else 'bf16'}", 2, P, f) for f in (0, 1) for P in POOL_P] + \
             [PoolCase(f"B32-P600-{'f16' if f else 'bf16'}", 32, 600, f) for f in (0, 1)]


# attnpool_dot64 adds the products in pairs, serially and (IEEE build) in program order: element j of the 64 meets its product, its
# pair's sum, and the 32 - j // 2 accumulator adds from its pair's on
POOL_DOT_W = (34 - torch.arange(64) // 2).to(F64)


def pool_inputs(case):
    seed = 2000 + 13 * case.B + case.P + 5 * case.f16
    B, N = case.B, case.P + 2
    dt = torch.float16 if case.f16 else torch.bfloat16
    kv = (randn(B, N, 2 * D, seed=seed) * (1.0 + 0.02 * torch.arange(B, dtype=F32).view(B, 1, 1))).to(dt)
    return dict(kv=kv, q=randn(1, D, seed=seed + 1, scale=0.5), dout=randn(B, D, seed=seed + 2))


def pool_tail_tokens(P):
    """Tokens the loops after the unrolled eight-row loops handle (`for (; t + 28 < P; t += 32)` from t = wave, then `t += 4`)."""
    tail = []
    for w in range(4):
        t = w
        while t + 28 < P:
            t += 32
        tail += list(range(t, P, 4))
    return sorted(tail)


def pool_drop_tokens(P):
    """The tail tokens, or the last pass of the unrolled loops where they leave no tail (P = 256)."""
    return pool_tail_tokens(P) or list(range(P - 32, P))


def _pool_split(kv):
    B, N, _ = kv.shape
    kd = kv.double()
    K = kd[:, 2:, :D].reshape(B, N - 2, H, 64).permute(0, 2, 1, 3)
    V = kd[:, 2:, D:].reshape(B, N - 2, H, 64).permute(0, 2, 1, 3)
    return K, V                                                             # [B, H, P, 64]


def pool_fwd_ref(kv, q):
    """-> probs [B, H, P], pooled [B, D] and bounds.  probs' bound is p (det + K_EXP u unit): the score's roundings (POOL_DOT_W), the
    subtraction of the maximum, the exponential, and the same again for the normalising sum.  The error of the maximum itself shifts
    every score alike and cancels in the quotient."""
    K, V = _pool_split(kv)
    B, _, P, _ = K.shape
    qh = q.double().view(H, 64)
    sc = torch.einsum("bhpd,hd->bhp", K, qh) * 0.125
    e_sc = U32 * torch.einsum("bhpd,hd,d->bhp", K.abs(), qh.abs(), POOL_DOT_W.to(K.device)) * 0.125
    p = torch.softmax(sc, -1)
    a = (sc - sc.max(-1, keepdim=True).values).abs()
    ksum = cdiv(P, 256) + 6 + 3
    det = e_sc + e_sc.max(-1, keepdim=True).values + U32 * (a + a.max(-1, keepdim=True).values + ksum + 2)
    unit = (1 + a) + (1 + a.max(-1, keepdim=True).values)
    pooled = torch.einsum("bhp,bhpd->bhd", p, V).reshape(B, D)
    return dict(p=p, det=det, unit=unit, pooled=pooled, V=V, kv_terms=cdiv(P, 4) + 3 + 2)


def pool_probs_bound(r):
    return r["p"] * (r["det"] + K_EXP * U32 * r["unit"]) + TINY


def pool_pooled_bound(r):
    B = r["p"].shape[0]
    Va = r["V"].abs()
    return (torch.einsum("bhp,bhpd->bhd", pool_probs_bound(r), Va) + U32 * r["kv_terms"] * torch.einsum("bhp,bhpd->bhd", r["p"], Va)).reshape(B, D) + TINY


def half_ulp_bf16(v):
    """Half a unit in the last place of bf16 (8 significant bits) at the float64 value v; 0 at 0."""
    _, e = torch.frexp(v.abs())
    return torch.where(v == 0, torch.zeros_like(v), torch.ldexp(torch.ones_like(v), e - 9))


def pool_bwd_ref(kv, q, probs, dout):
    """Backward from the saved `probs` [B H, P] (fp32).  -> dkv [B, N, 2 D] with rows 0-1 zero, dq [D], bounds, and dq's per-clip and
    per-token parts for the drop checks."""
    K, V = _pool_split(kv)
    B, _, P, _ = K.shape
    p = probs.double().view(B, H, P)
    go, qh = dout.double().view(B, H, 64), q.double().view(H, 64)
    dP = torch.einsum("bhpd,bhd->bhp", V, go)
    dPa = torch.einsum("bhpd,bhd->bhp", V.abs(), go.abs())
    dot, dota = (p * dP).sum(-1, keepdim=True), (p * dPa).sum(-1, keepdim=True)
    dS = p * (dP - dot) * 0.125
    e_dP = U32 * torch.einsum("bhpd,bhd,d->bhp", V.abs(), go.abs(), POOL_DOT_W.to(V.device))
    e_dot = (p * e_dP).sum(-1, keepdim=True) + U32 * (cdiv(P, 256) + 6 + 3 + 1) * dota
    e_dS = (p * (e_dP + e_dot) + 3 * U32 * p * (dP.abs() + dot.abs())) * 0.125
    dK = dS.unsqueeze(-1) * qh.view(1, H, 1, 64)
    dV = p.unsqueeze(-1) * go.view(B, H, 1, 64)
    e_dK = e_dS.unsqueeze(-1) * qh.abs().view(1, H, 1, 64) + U32 * dK.abs()
    e_dV = U32 * dV.abs()
    pack = lambda k, v: torch.cat([torch.zeros(B, 2, 2 * D, dtype=F64, device=k.device),
                                   torch.cat([k.permute(0, 2, 1, 3).reshape(B, P, D), v.permute(0, 2, 1, 3).reshape(B, P, D)], -1)], 1)
    dkv = pack(dK, dV)
    b_dkv = half_ulp_bf16(dkv) + pack(e_dK, e_dV)                           # rows 0-1: bound 0, the kernel writes exact zeros
    tok = dS.unsqueeze(-1) * K                                              # [B, H, P, 64]: dq's terms
    parts = tok.sum(2).reshape(B, D)
    kq = cdiv(P, 4) + 3 + 2
    b_dq = (e_dS.unsqueeze(-1) * K.abs() + U32 * kq * tok.abs()).sum(2).reshape(B, D).sum(0) + chain(parts) + TINY
    tail = pool_drop_tokens(P)
    return dict(dkv=dkv, b_dkv=b_dkv, dq=parts.sum(0), b_dq=b_dq, dq_last_clip=parts[-1], dq_tail=tok[:, :, tail].sum(2).reshape(B, D).sum(0))


# ================================================================================================ small linear
# small_linear: one wave per output, ceil(K / 64) serial products, 6 levels, bias (, sigmoid).  small_linear_bwd: dW / db add M terms
# serially onto what is there; da splits N eight ways, four accumulators each, 5 adds to merge.
LinCase = collections.namedtuple("LinCase", "name M N K act")
LIN_CASES = [LinCase(f"M{m}-N{n}-K{k}-act{a}", m, n, k, a) for m, n, k, a in ((1, 768, 768, 0), (32, 10, 768, 1), (32, 768, 768, 0), (3, 7, 70, 1))]


def lin_inputs(case):
    seed = 3000 + case.M + 3 * case.N + case.K
    M, N, K = case.M, case.N, case.K
    return dict(a=randn(M, K, seed=seed), w=randn(N, K, seed=seed + 1, scale=0.05), b=randn(N, seed=seed + 2), dout=randn(M, N, seed=seed + 3),
                dw0=randn(N, K, seed=seed + 4), db0=randn(N, seed=seed + 5))


def lin_fwd_ref(a, w, b, act):
    ad, wd, bd = a.double(), w.double(), b.double()
    K = a.shape[1]
    z = ad @ wd.t() + bd
    absdot = ad.abs() @ wd.abs().t()
    dz = U32 * ((cdiv(K, 64) + 6) * absdot + (absdot + bd.abs()))
    if act == 0:
        return z, dz + TINY, torch.zeros_like(z)
    s = torch.sigmoid(z)
    return s, s * (1 - s) * dz + 3 * U32 * s + TINY, s * (1 - s) * (1 + z.abs())


def lin_out_bound(det, unit):
    return det + K_EXP * U32 * unit


def lin_bwd_ref(a, w, out, dout, act, dw0, db0):
    """From the saved `out` (fp32).  g = dout o (1 - o) carries 3 roundings; dW / db accumulate onto dw0 / db0."""
    ad, wd = a.double(), w.double()
    M, K = a.shape
    N = w.shape[0]
    g = dout.double()
    kg = 0
    if act == 1:
        o = out.double()
        g, kg = g * o * (1 - o), 3
    ga = g.abs()
    da, dW, db = g @ wd, dw0.double() + g.t() @ ad, db0.double() + g.sum(0)
    chunk = cdiv(N, 8)
    b_da = U32 * (cdiv(chunk, 4) + 2 + 3 + 1 + kg) * (ga @ wd.abs()) + TINY
    b_dW = U32 * ((M + 1 + kg) * (ga.t() @ ad.abs()) + dW.abs() + dw0.double().abs()) + TINY
    b_db = U32 * ((M + kg) * ga.sum(0) + db.abs() + db0.double().abs()) + TINY
    last = g[-1:]                                                           # drop checks: the last row m, the last output n
    return dict(da=da, dW=dW, db=db, b_da=b_da, b_dW=b_dW, b_db=b_db, drop_dW=last.t() @ ad[-1:], drop_db=last[0],
                drop_da=g[:, -1:] @ wd[-1:])


# ================================================================================================ MLM masking
# mlm_apply: 2048 x 256 float4 per pass = 2730 2/3 rows.  mlm_apply_bwd: 2048 x 256 floats per pass = 682 2/3 rows; every element is
# one atomic add, so a row of dx that k rows copy, and dtoken, are atomic chains.
MLM_FIRST_PASS_ROWS = 2048 * 256 * 4 / D
MLM_BWD_FIRST_PASS_ROWS = 683           # rows from here on lie wholly in the second or a later pass of the backward
MlmCase = collections.namedtuple("MlmCase", "name rows kind")
MLM_CASES = [MlmCase(f"rows{r}-{k}", r, k) for r, k in ((1, "mask"), (2730, "random"), (2731, "random"), (2732, "random"), (5500, "random"),
                                                        (5500, "hot"), (5500, "all"), (2731, "none"))]


def mlm_inputs(case):
    """action (0 keep, 1 mask token, 2 copy row src) and src.  'random' also plants, when there are two passes, copies whose source lies
    in the other pass, and copies whose source row is itself masked or copied.  'hot': 500 rows spread over the passes copy row 7."""
    rows = case.rows
    g = gen(4000 + rows)
    x, tok, dout = torch.randn(rows, D, generator=g), torch.randn(D, generator=g), torch.randn(rows, D, generator=g)
    action = torch.zeros(rows, dtype=torch.uint8)
    src = torch.zeros(rows, dtype=torch.int32)
    if case.kind == "mask":
        action[:] = 1
    elif case.kind == "all":
        action[:] = 1
        action[1::3] = 2
        src[:] = torch.randint(0, rows, (rows,), generator=g).to(torch.int32)
    elif case.kind == "hot":
        idx = torch.arange(10, rows, 10)[:500]
        action[idx] = 2
        src[idx] = 7
    elif case.kind == "random":
        action[:] = torch.randint(0, 3, (rows,), generator=g).to(torch.uint8)
        src[:] = torch.randint(0, rows, (rows,), generator=g).to(torch.int32)
        first = int(MLM_FIRST_PASS_ROWS)
        action[0], src[0] = 2, rows - 1                 # first pass <- last row (second pass when there is one)
        action[rows - 1], src[rows - 1] = 2, 1          # last row <- first pass
        action[1] = 1                                   # ... whose source is masked
        action[2], src[2] = 2, 0                        # a copy of a row that is itself a copy
        if rows > first + 1:
            action[first], src[first] = 2, 3            # the row that straddles the pass boundary
    return dict(x=x, tok=tok, dout=dout, action=action, src=src)


def mlm_fwd_ref(x, tok, action, src):
    ref = x.clone()
    ref[action == 1] = tok
    c = action == 2
    ref[c] = x[src.long()[c]]
    return ref


def mlm_bwd_ref(dout, action, src):
    """-> dx, dtoken (float64) and bounds: dx's rows take 1 + k adds onto zero (exact for one contribution), bound by the chain of its
    terms; dtoken is the chain over the masked rows."""
    d = dout.double()
    rows = d.shape[0]
    keep, mask, copy = action == 0, action == 1, action == 2
    dx = torch.zeros_like(d)
    dx[keep] = d[keep]
    s = src.long()[copy]
    dx.index_add_(0, s, d[copy])
    absx = torch.zeros_like(d)
    absx[keep] = d[keep].abs()
    absx.index_add_(0, s, d[copy].abs())
    cnt = keep.double()
    cnt.index_add_(0, s, torch.ones(int(copy.sum()), dtype=F64, device=d.device))
    b_dx = U32 * (cnt - 1).clamp(min=0).unsqueeze(1) * absx + TINY
    dtok = d[mask].sum(0)
    b_tok = chain(d[mask]) + TINY if bool(mask.any()) else torch.full((d.shape[1],), TINY, dtype=F64, device=d.device)
    late = torch.arange(rows, device=d.device) >= MLM_BWD_FIRST_PASS_ROWS
    late_tok = late
    if not bool((mask & late).any()):                   # a single pass: the last masked row instead
        late_tok = torch.arange(rows, device=d.device) == (int(mask.nonzero().max()) if bool(mask.any()) else -1)
    drop_tok = d[mask & late_tok].sum(0)
    drop_dx = torch.zeros_like(d).index_add_(0, src.long()[copy & late], d[copy & late])
    return dict(dx=dx, dtok=dtok, b_dx=b_dx, b_tok=b_tok, drop_tok=drop_tok, drop_dx=drop_dx, cnt=cnt)


# ================================================================================================ masked MSE
# masked_mse: 512 workgroups x 4 waves, one row per wave and pass: first pass 2048 rows.  A lane adds its 12 squares of every row of its
# wave, 6 levels, 3 LDS adds, one scale; the 512 workgroups meet in an atomic chain.
MSE_FIRST_PASS = 2048
MseCase = collections.namedtuple("MseCase", "name rows mask")
MSE_CASES = [MseCase(f"rows{r}-{m}", r, m) for r in (1, 4, 2047, 2048, 2049, 6151) for m in ("all", "none", "random")] + \
            [MseCase(f"rows{r}-late", r, "late") for r in (2049, 6151)]


def mse_inputs(case):
    rows = case.rows
    g = gen(5000 + rows)
    pred, target = torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g)
    if case.mask == "all":
        mask = torch.ones(rows, dtype=torch.uint8)
    elif case.mask == "none":
        mask = torch.zeros(rows, dtype=torch.uint8)
    elif case.mask == "late":
        mask = (torch.arange(rows) >= MSE_FIRST_PASS).to(torch.uint8)
    else:
        mask = (torch.rand(rows, generator=g) < 0.5).to(torch.uint8)
        mask[0] = 1
    return dict(pred=pred, target=target, mask=mask)


def mse_ref(pred, target, mask):
    """n = max(masked rows, 1): with no masked row the device-count form gives loss 0 and gradients exactly 0 (torch's mean over an empty
    selection is NaN; the trainers never get there, the kernel's count is clamped instead of branching on the host)."""
    m = mask.bool()
    rows = pred.shape[0]
    n = max(int(m.sum()), 1)
    d = (pred.double() - target.double()) * m.unsqueeze(1)
    per_row = (d * d).sum(1) / (n * D)
    loss = per_row.sum()
    passes = cdiv(rows, MSE_FIRST_PASS)
    wg = (torch.arange(rows, device=pred.device) // 4) % 512
    parts = torch.zeros(512, dtype=F64, device=pred.device).index_add_(0, wg, per_row)
    b_loss = U32 * (12 * passes + 6 + 3 + 2 + 2) * loss + chain(parts) + TINY
    dpred = 2 * d / (n * D)
    b_d = 3 * U32 * dpred.abs() + TINY                  # the difference, 1 / (n D), the product
    late = per_row[MSE_FIRST_PASS:].sum()
    drop = late if float(late) > 0 else (per_row[m][-1] if bool(m.any()) else loss)
    return dict(loss=loss, b_loss=b_loss, dpred=dpred, b_d=b_d, drop=drop, n=int(m.sum()))


# ================================================================================================ mean-teacher losses
# sed_losses_kernel: min(1024, ceil(B C T / 1024)) workgroups of 256 threads stride over the frame values (4 per thread below the cap);
# workgroup 0 alone strides over the B C clip-level values, 256 at a time; 6 levels, 3 LDS adds, one atomic per workgroup and sum.
LossCase = collections.namedtuple("LossCase", "name B C T strong_n weak_lo weak_n")
LOSS_SHAPES = ((1, 1, 1), (2, 10, 7), (26, 10, 3), (32, 10, 1000), (27, 10, 3884))
LOSS_W = dict(w_weak=0.5, w_weak_cons=0.5, w_at=2.0, w_cons=13.7)


def _loss_partitions(B):
    k = B // 3                                                              # the trainers' layout: k strong clips, then m weak ones
    parts = [(0, 0, B), (B, 0, 0), (B, 0, B)] + ([(2, 4, 2)] if B >= 6 else []) + ([(k, k, B - 2 * k)] if k > 0 else [])
    return parts


LOSS_CASES = [LossCase(f"B{B}-C{C}-T{T}-s{s}-lo{lo}-w{w}", B, C, T, s, lo, w) for B, C, T in LOSS_SHAPES for s, lo, w in _loss_partitions(B)]
ONE_M = float(np.float32(1.0) - np.float32(U32))                            # 1 - 2^-24, the largest fp32 below 1


def loss_blocks(n):
    return max(1, min(1024, cdiv(n, 1024)))


def loss_inputs(B, C, T):
    """Posteriors in (0, 1) with, where there is room, exactly 0, 1 and 1 - 2^-24 against labels 0 and 1 in the first clip (log clamp at
    -100, gradient clamp 1e-12)."""
    g = gen(6000 + B + C + T)
    r = lambda *s: torch.rand(*s, generator=g) * 0.998 + 0.001
    ss, sw, sa, ts, ta = r(B, C, T), r(B, C), r(B, C), r(B, C, T), r(B, C)
    y, yw = (torch.rand(B, C, T, generator=g) < 0.3).float(), (torch.rand(B, C, generator=g) < 0.5).float()
    if C * T >= 6:
        f, l = ss.view(B, -1), y.view(B, -1)
        f[0, :6] = torch.tensor([0.0, 0.0, 1.0, 1.0, ONE_M, ONE_M])
        l[0, :6] = torch.tensor([0.0, 1.0, 0.0, 1.0, 0.0, 1.0])
    if C >= 6:
        sw[0, :6] = torch.tensor([0.0, 0.0, 1.0, 1.0, ONE_M, ONE_M])
        sa[0, :6] = torch.tensor([1.0, ONE_M, 0.0, 0.0, 1.0, ONE_M])
        yw[0, :6] = torch.tensor([0.0, 1.0, 0.0, 1.0, 0.0, 1.0])
    return dict(ss=ss, sw=sw, sa=sa, ts=ts, ta=ta, y=y, yw=yw)


def _bce(p, y):
    """-> term, its float64 gradient factor (p - y) / max(p (1 - p), 1e-12f) (the clamp is an fp32 constant in the kernel and in ATen), and the term's own error split as det + K_LOG u unit:
    fl(1 - p) is exact above 1/2 and adds u to log(1 - p) below; two products and the sum."""
    lp, lq = torch.log(p).clamp(min=-100.0), torch.log(1 - p).clamp(min=-100.0)
    term = -(y * lp + (1 - y) * lq)
    unit = y * lp.abs() + (1 - y) * lq.abs()
    det = U32 * ((1 - y) * (p < 0.5) + 3 * term.abs())
    return term, (p - y) / (p * (1 - p)).clamp(min=f32(1e-12)), det, unit


def _sum_bound(terms, t_det, t_unit, blocks, per_thread, n_first=None):
    """Bound of one of the six sums: the terms' own errors, kappa = per_thread + 6 + 3 on sum|terms|, the chain over the workgroups
    (workgroup of element i: (i // 256) % blocks; clip-level sums live in workgroup 0 alone: blocks = 1)."""
    flat = terms.reshape(-1)
    n = flat.numel()
    if n == 0:
        z = torch.zeros((), dtype=F64, device=terms.device)
        return z, z
    wg = (torch.arange(n, device=flat.device) // 256) % blocks
    parts = torch.zeros(blocks, dtype=F64, device=flat.device).index_add_(0, wg, flat)
    det = t_det.sum() + U32 * (per_thread + 6 + 3) * flat.abs().sum() + chain(parts)
    return det, t_unit.sum()


def loss_ref(inp, case, w=LOSS_W):
    """The six sums (un-normalised, as the kernel's scratch holds them), the seven outputs and the three gradients, with bounds.
    sums / outs: (value, det, unit) with bound = det + K_LOG u unit, then capped at LEGACY_LOSS_REL max(1, |value|)."""
    B, C, T, sn, lo, wn = case.B, case.C, case.T, case.strong_n, case.weak_lo, case.weak_n
    dd = lambda k: inp[k].double()
    ss, sw, sa, ts, ta, y, yw = (dd(k) for k in ("ss", "sw", "sa", "ts", "ta", "y", "yw"))
    dev = ss.device
    n = B * C * T
    blocks = loss_blocks(n)
    per_thread = cdiv(n, blocks * 256)
    per_thread_c = cdiv(B * C, 256)
    ws = slice(lo, lo + wn)
    # -- the sums.  Frame-level terms of clips >= strong_n are absent from sums[0] but keep their place in the stride loop.
    t0, g0, d0, u0 = _bce(ss, y)
    in_s = (torch.arange(B, device=dev) < sn).view(B, 1, 1).to(F64)
    in_w = ((torch.arange(B, device=dev) >= lo) & (torch.arange(B, device=dev) < lo + wn)).view(B, 1).to(F64)
    t1, g1, d1, u1 = _bce(sw, yw)
    t2, g2, d2, u2 = _bce(sa, yw)
    se3, se4, se5 = (ss - ts) ** 2, (sw - ta) ** 2, (sa - ta) ** 2
    z = torch.zeros_like
    terms = [(t0 * in_s, d0 * in_s, u0 * in_s, blocks, per_thread), (t1 * in_w, d1 * in_w, u1 * in_w, 1, per_thread_c),
             (t2 * in_w, d2 * in_w, u2 * in_w, 1, per_thread_c), (se3, 3 * U32 * se3, z(se3), blocks, per_thread),
             (se4, 3 * U32 * se4, z(se4), 1, per_thread_c), (se5, 3 * U32 * se5, z(se5), 1, per_thread_c)]
    sums, sdet, sunit = [], [], []
    for t, dt, ut, nb, pt in terms:
        det, unit = _sum_bound(t, dt, ut, nb, pt)
        sums.append(t.sum()); sdet.append(det); sunit.append(unit)
    # -- the seven outputs, as sed_losses_final_kernel composes them (count products and the division: 4 more roundings each)
    nan = torch.tensor(float("nan"), dtype=F64, device=dev)
    cnt = [sn * C * T, wn * C, wn * C, B * C * T, B * C, B * C]
    val = [sums[k] / cnt[k] if cnt[k] > 0 else nan for k in range(6)]
    vdet = [(sdet[k] / cnt[k] + 4 * U32 * val[k].abs()) if cnt[k] > 0 else nan for k in range(6)]
    vunit = [sunit[k] / cnt[k] if cnt[k] > 0 else nan for k in range(6)]
    ww, wwc, wat, wc = (float(np.float32(w[k])) for k in ("w_weak", "w_weak_cons", "w_at", "w_cons"))
    coef = [1.0, ww, wat, wc, wwc * wc, wat * wc]
    total = sum(c * v for c, v in zip(coef, val))
    tdet = sum(c * d for c, d in zip(coef, vdet)) + 8 * U32 * sum(c * v.abs() for c, v in zip(coef, val))
    tunit = sum(c * u for c, u in zip(coef, vunit))
    outs = [(total, tdet, tunit)] + list(zip(val, vdet, vunit))
    # -- gradients (no intrinsic): each part is a chain of <= 12 products, differences and one division on the fp32 values
    gs_mse = 2 * wc / (B * C * T) * (ss - ts)
    gs_bce = (g0 * in_s / (sn * C * T)) if sn > 0 else z(ss)
    gw_mse, ga_mse = 2 * wc / (B * C) * wwc * (sw - ta), 2 * wc / (B * C) * wat * (sa - ta)
    gw_bce = (ww * g1 * in_w / (wn * C)) if wn > 0 else z(sw)
    ga_bce = (wat * g2 * in_w / (wn * C)) if wn > 0 else z(sa)
    grads = [(m + b, 12 * U32 * (m.abs() + b.abs()) + TINY) for m, b in ((gs_mse, gs_bce), (gw_mse, gw_bce), (ga_mse, ga_bce))]
    # -- contributions the bounds have to see
    drops = {}
    first = blocks * 256
    if n > first:
        for k in (0, 3):
            drops[(k, "grid passes after the first")] = terms[k][0].reshape(-1)[first:].sum()
    if B > 1:
        for k in range(6):
            drops[(k, "last clip")] = terms[k][0][B - 1].sum()
    if B * C > 256:
        for k in (1, 2, 4, 5):
            drops[(k, "clip-level values 256..")] = terms[k][0].reshape(-1)[256:].sum()
    return dict(sums=list(zip(sums, sdet, sunit)), outs=outs, grads=grads, drops=drops)


def loss_bound(value, det, unit):
    """det + K_LOG u unit, and never looser than the 2e-6 relative of test_gpu_kernels.py."""
    return torch.minimum(det + K_LOG * U32 * unit, LEGACY_LOSS_REL * value.abs().clamp(min=1.0)) + TINY


def loss_args_ok(c):
    """The argument check of sed_sed_losses."""
    return c.B > 0 and c.C > 0 and c.T > 0 and 0 <= c.strong_n <= c.B and c.weak_lo >= 0 and c.weak_n >= 0 and c.weak_lo + c.weak_n <= c.B


# ================================================================================================ AdamW + EMA
# adamw_ema_kernel: min(8192, ceil(n / 1024)) workgroups x 256 float4: first pass 8 388 608 floats.  Elementwise: no sums.
ADAM_FIRST_PASS = 8192 * 256 * 4
ADAM_N = (4, 64, 1020, ADAM_FIRST_PASS, ADAM_FIRST_PASS + 64)
ADAM_HYPER = ((1e-3, 1e-4), (1e-4, 0.0), (0.0, 1e-2))
ADAM_STEPS = (10, 1000, 100000)
ADAM_ALPHAS = (0.0, 0.5, 0.999, 1.0)
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


def adam_inputs(n, seed=7000):
    """p, g, m, v >= 0, ema.  |g| is 0 (every eighth element, where m = v = 0 too: those elements only decay) or lies in [1e-6, 1e2]:
    below that g^2 leaves the fp32 normal range, which float64 does not model."""
    g_ = gen(seed + n % 1009)
    p = torch.randn(n, generator=g_)
    mag = 10.0 ** (torch.rand(n, generator=g_) * 8.0 - 6.0)
    g = mag * torch.sign(torch.randn(n, generator=g_))
    m = torch.randn(n, generator=g_) * 0.1
    v = torch.rand(n, generator=g_) * 0.01 + 1e-8
    ema = torch.randn(n, generator=g_)
    z = torch.arange(n) % 8 == 3
    g[z] = 0.0; m[z] = 0.0; v[z] = 0.0
    return dict(p=p, g=g, m=m, v=v, ema=ema, zero=z)


def adam_ref(p, g, m, v, ema, lr, wd, step, alpha, do_adam=1, b1=BETA1, b2=BETA2, eps=EPS):
    """torch.optim.AdamW's recurrence and the EMA line in float64 from the fp32 state, hyper-parameters as the fp32 values the entry
    point receives, bias corrections in float64 from `step`.  -> (p, m, v, ema) and their bounds.

    Error model, element by element: m' 3 roundings, v' 4 (all terms >= 0); the host's fl(1 - powf(b, step)) is off by at most
    u (1 + 2 b^step), relative to bc = 1 - b^step; the denominator gathers sqrt, the division by sqrt(bc2) and eps, the step
    lr / bc1 * m' / denom three more; p (1 - lr wd) two, the subtraction one; the EMA line four on its two products."""
    lr, wd, b1, b2, eps, alpha = (f32(t) for t in (lr, wd, b1, b2, eps, alpha))
    pd, md, vd = p.double(), m.double(), v.double()
    if do_adam:
        gd = g.double()
        bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        r1, r2 = U32 * (1 + 2 * b1 ** step) / bc1, U32 * (1 + 2 * b2 ** step) / bc2
        pdec = pd * (1.0 - lr * wd)
        m2 = b1 * md + (1.0 - b1) * gd
        v2 = b2 * vd + (1.0 - b2) * gd * gd
        e_m = 3 * U32 * ((b1 * md).abs() + ((1.0 - b1) * gd).abs())
        e_v = 4 * U32 * v2
        root = torch.sqrt(v2) / math.sqrt(bc2)
        denom = root + eps
        e_den = root * (3 * U32 + r2 / 2 + 2 * U32) + U32 * denom
        upd = (lr / bc1) * (m2 / denom)
        e_upd = upd.abs() * (e_den / denom + r1 + 3 * U32) + (lr / bc1) * e_m / denom
        p2 = pdec - upd
        e_p = 3 * U32 * pd.abs() + e_upd + U32 * p2.abs()
    else:
        p2, m2, v2 = pd, md, vd
        e_p = e_m = e_v = torch.zeros_like(pd)
    if ema is None:
        return (p2, m2, v2, None), (e_p + TINY, e_m + TINY, e_v + TINY, None)
    ed = ema.double()
    e2 = alpha * ed + (1.0 - alpha) * p2
    e_e = U32 * (2 * (alpha * ed).abs() + 3 * ((1.0 - alpha) * p2).abs() + e2.abs()) + abs(1.0 - alpha) * e_p
    return (p2, m2, v2, e2), (e_p + TINY, e_m + TINY, e_v + TINY, e_e + TINY)
