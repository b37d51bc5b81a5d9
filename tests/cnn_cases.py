"""Cases, inputs, float64 / fp32 references and restated launch arithmetic for the CNN-branch kernels of csrc/cnn_branch.hip and
csrc/dw_narrow.hip (importable without a GPU: no test, no GPU code).  tests/test_cnn_cases_cpu.py proves on the CPU that every case
crosses the threshold it is named for, that every drop condition holds and that the references are right; tests/test_gpu_cnn_kernels.py
holds the hardware to them.

A. every layer geometry of the real stack (synth.PMAM_FILTERS / PMAM_POOLING) at T = 12, B = 2, with the arguments PmamEngine passes
   (`PmamEngine._cnn_fwd` / `_cnn_bwd`): LAYERS.
B. the smallest shape at which each entry point's grid-stride loop (or slab loop) takes a second trip: the *_B cases.

Bounds (all taken from the project, none tuned to a kernel):
  gathers / scatters    bit equality (im2col, col2im, the narrow transpose's image)
  element-wise outputs  walk_cases.judge:  |got - ref64| <= 8 max|ref32 - ref64| + half_ulp(storage)
  atomically added sums (d + 2) 2^-24 sum|term| per output word (`sum_bound`), d = the longest chain of additions a term passes through:
                        per-thread trips + the in-workgroup combination + the workgroups that add atomically to the word.

The functions under "launch arithmetic" copy INTEGER FORMULAS of the entry points (the source line is named at each), not kernels: they
exist so that the CPU test can assert what a shape does to a launch."""
import collections
import functools

import torch
import torch.nn.functional as F

from walk_cases import judge, half_ulp, bound32, maxerr, SENS, cdiv  # noqa: F401  (re-exported to the two test files)
from transformer4sed_amd import synth

F32, F64, F16, BF16 = torch.float32, torch.float64, torch.float16, torch.bfloat16
NAN = float("nan")
EPS32 = 2.0 ** -24
DROP_SCALE = float(torch.tensor(1.0 / 0.9, dtype=F32))      # the fp32 value the entry points receive (conv_dropout = 0.1)
B_A, T_A = 2, 12


def pad128(n):
    return (n + 127) // 128 * 128


def gen(seed):
    return torch.Generator().manual_seed(seed)


def uni(g, *shape, lo=-1.0, hi=1.0):
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


# ================================================================================================ A. the ten layers
Layer = collections.namedtuple("Layer", "i cin co H W ph pw Np Kp Cp ldy ldg cpin last")


def layers(T=T_A):
    """The geometry of `pmam_engine.geometry.cnn_geometry` (Np, Kp, Cp, ldg) and `cnn_layer_plans` (ldy, the im2col channel pitch, H and
    W per layer), restated on purpose: tests/test_pmam_geometry_cpu.py holds the two to each other."""
    out, H, W, cin = [], T, 128, 1
    n = len(synth.PMAM_FILTERS)
    for i, (co, (ph, pw)) in enumerate(zip(synth.PMAM_FILTERS, synth.PMAM_POOLING)):
        Np = pad128(co)
        out.append(Layer(i, cin, co, H, W, ph, pw, Np, 64 if i == 0 else pad128(9 * cin), max(64, co), co if co < Np else Np,
                         64 if co <= 64 else Np, max(64, cin), i + 1 == n))
        H, W, cin = H // ph, W // pw, co
    return out


LAYERS = layers()


# ================================================================================================ launch arithmetic
def grid_for(work, threads=256, cap=8192):
    """csrc/common.h:142-147."""
    return max(1, min(cap, cdiv(work, threads)))


def passes(work, cap):
    """A grid-stride loop over `work` items on grid_for(work, 256, cap) workgroups -> (workgroups, items of the first pass, trips)."""
    blocks = grid_for(work, 256, cap)
    return blocks, blocks * 256, cdiv(work, blocks * 256)


CAP_FUSED, CAP = 4096, 16384


def conv0_fwd16_launch(B, T):
    """csrc/cnn_branch.hip:62-63, 110: one item per pixel."""
    return (B * T * 128,) + passes(B * T * 128, CAP_FUSED)


def conv0_dw16_launch(B, T):
    """csrc/cnn_branch.hip:197-200 and the trip loop at :130 -> (rows per workgroup, slabs, trips per workgroup, rows of the last slab)."""
    M = B * T * 128
    rows = cdiv(cdiv(M, 1024), 128) * 128
    slabs = cdiv(M, rows)
    return rows, slabs, cdiv(rows, 128), M - (slabs - 1) * rows


def im2col_launch(M, Kp):
    """csrc/cnn_branch.hip:207-209, 229: one item per 16-byte chunk."""
    return (M * (Kp // 8),) + passes(M * (Kp // 8), CAP)


def col2im_launch(M, C):
    """csrc/cnn_branch.hip:235-237, 257: one item per four channels."""
    return (M * (C // 4),) + passes(M * (C // 4), CAP)


def colstats_launch(M, C):
    """csrc/cnn_branch.hip:298-302 and the kernel's map at :272-279 -> (rows per iteration, column groups, slabs, trips)."""
    rpi = 256 // min(C, 64)
    slabs = max(1, min(2048, cdiv(M, rpi * 16)))
    return rpi, cdiv(C, 64), slabs, cdiv(M, slabs * rpi)


def colstats_args_ok(M, C):
    """csrc/cnn_branch.hip:297."""
    return M > 0 and C > 0 and not (C < 64 and 256 % C)


def bn_act_launch(M, Cp):
    """csrc/cnn_branch.hip:350-352, 369."""
    return (M * (Cp // 4),) + passes(M * (Cp // 4), CAP)


def bn_bwd_launch(M, ldo):
    """csrc/cnn_branch.hip:378-381, 402."""
    return (M * (ldo // 4),) + passes(M * (ldo // 4), CAP)


def cg_pool_launch(B, H, W, Cpo, ph, pw):
    """csrc/cnn_branch.hip:413-416, 456: one item per four channels of an OUTPUT pixel."""
    work = B * (H // ph) * (W // pw) * (Cpo // 4)
    return (work,) + passes(work, CAP)


def cg_pool_bwd_launch(B, H, W, ldl16):
    """csrc/cnn_branch.hip:467-470, 503: one item per four columns of dL16 of an INPUT pixel."""
    return (B * H * W * (ldl16 // 4),) + passes(B * H * W * (ldl16 // 4), CAP)


def gate16_pool_launch(B, H, W, ph, pw):
    """csrc/cnn_branch.hip:523-525, 594: one item per OUTPUT pixel."""
    work = B * (H // ph) * (W // pw)
    return (work,) + passes(work, CAP)


def gate16_bwd_launch(B, H, W):
    """csrc/cnn_branch.hip:624-626, 705: one item per INPUT pixel."""
    return (B * H * W,) + passes(B * H * W, CAP_FUSED)


def transpose_narrow_launch(Rpad):
    """csrc/dw_narrow.hip:55-56 and the loop at :20 -> (workgroups, rows of the first pass, trips)."""
    blocks = min(2048, cdiv(Rpad, 256))
    return blocks, blocks * 256, cdiv(Rpad, blocks * 256)


# ---- d of the sum bound: trips of a thread + combination inside the workgroup + workgroups adding atomically to one word
def d_wave_reduce(trips, blocks):
    """conv0_fwd16 (cnn_branch.hip:86, 93, 101-102), cg_gate16_pool_bwd (:670-671, 686, 694-695), transpose_narrow (dw_narrow.hip:38,
    45, 49): one addition per trip, six shuffle steps, (a + b) + (c + d) over the four waves, one atomic per workgroup."""
    return trips + 6 + 2 + blocks


def d_colstats(M, C):
    """cnn_branch.hip:279-283 (one addition per trip), :289 (rpi partials added in order), :290-291 (one atomic per slab)."""
    rpi, _, slabs, trips = colstats_launch(M, C)
    return trips + rpi + slabs


def d_conv0_dw16(B, T):
    """cnn_branch.hip:130, 148-160 (two pixels per lane and trip), :165 (four shuffle steps), :182 / :191 (four waves, one atomic per slab)."""
    _, slabs, trips, _ = conv0_dw16_launch(B, T)
    return 2 * trips + 4 + 2 + slabs


def sum_bound(d, abs_sum64):
    return (d + 2) * EPS32 * abs_sum64.double()


def judge_sum(got, ref64, bound):
    """-> (max error, worst error / bound, every word inside)."""
    diff = (got.detach().double().cpu() - ref64.detach().double().cpu()).abs()
    ratio = diff / bound.detach().double().cpu().clamp_min(1e-300)
    return float(diff.max()), float(ratio.max()), bool((ratio <= 1.0).all())


def drop_ratio(late_sum64, bound):
    """How many bounds the float64 sum moves by, in its most affected word, when the late rows are left out."""
    return float((late_sum64.abs() / bound.clamp_min(1e-300)).max())


# ================================================================================================ the 3 x 3 taps
def tap_index(B, H, W, sign=1, check_h=True, check_w=True):
    """Pixel m = (b, h, w), tap = 3 (dh + 1) + (dw + 1) reads pixel (b, h + sign dh, w + sign dw) (cnn_branch.hip:216-218; col2im with
    sign = -1: :245-246) -> (flat source pixel [M, 9], in range [M, 9]).  check_h / check_w = False are the DROP conditions: the tap is
    treated as in range and reads the flat neighbour -- the other end of the neighbouring row, or the neighbouring clip."""
    M = B * H * W
    m = torch.arange(M)
    w, h, b = m % W, (m // W) % H, m // (W * H)
    tap = torch.arange(9)
    hh = h[:, None] + sign * (tap // 3 - 1)[None]
    ww = w[:, None] + sign * (tap % 3 - 1)[None]
    src = (b[:, None] * H + hh) * W + ww
    ok = (src >= 0) & (src < M)
    if check_h:
        ok &= (hh >= 0) & (hh < H)
    if check_w:
        ok &= (ww >= 0) & (ww < W)
    return src.clamp(0, M - 1), ok


def im2col_ref(Xbits, B, H, W, C, Kp, **leak):
    """Xbits [B, H, W, Cp] as int16 -> col [M, Kp] as int16: column tap C + c, zeros from 9 C (bit patterns: no arithmetic)."""
    M = B * H * W
    src, ok = tap_index(B, H, W, **leak)
    src, ok = src.to(Xbits.device), ok.to(Xbits.device)
    x = Xbits.reshape(M, -1)[:, :C]
    g = torch.where(ok[..., None], x[src], torch.zeros((), dtype=Xbits.dtype, device=Xbits.device))
    col = torch.zeros(M, Kp, dtype=Xbits.dtype, device=Xbits.device)
    col[:, :9 * C] = g.reshape(M, 9 * C)
    return col


def col2im_ref(dcol, B, H, W, C, **leak):
    """dcol [M, Kp] bf16 -> dX [M, C] fp32: the <= 9 bf16 terms added in fp32 in tap order 0..8 (cnn_branch.hip:244-250: the order is
    fixed, so the kernel's result is this one bit for bit)."""
    M = B * H * W
    src, ok = tap_index(B, H, W, sign=-1, **leak)
    src, ok = src.to(dcol.device), ok.to(dcol.device)
    acc = torch.zeros(M, C, dtype=F32, device=dcol.device)
    zero = torch.zeros((), dtype=F32, device=dcol.device)
    for tap in range(9):
        acc += torch.where(ok[:, tap, None], dcol[src[:, tap], tap * C:(tap + 1) * C].float(), zero)
    return acc


def bits(x):
    return x.contiguous().view(torch.int16)


# ================================================================================================ element-wise references
def geom_up(dout, B, H, W, ph, pw):
    """[B Ho Wo, C] -> [B H W, C]: every input pixel gets its window's value."""
    C = dout.shape[1]
    return dout.view(B, H // ph, W // pw, C).repeat_interleave(ph, 1).repeat_interleave(pw, 2).reshape(B * H * W, C)


def pool(x, B, H, W, ph, pw):
    C = x.shape[1]
    return F.avg_pool2d(x.view(B, H, W, C).permute(0, 3, 1, 2), (ph, pw)).permute(0, 2, 3, 1).reshape(-1, C)


def keep_of(mask, scale, dt):
    return 1.0 if mask is None else mask.to(dt) * scale


def bn_act_ref(Y, a, b, dt):
    return Y.to(dt) * a.to(dt) + b.to(dt)


def bn_bwd_ref(dz, Y, ah, bh, gamma, s1, s2, dt):
    """cnn_branch.hip:373-374: dY = gamma rstd (dz - s1 / M - xhat s2 / M), xhat = Y ah + bh, from the kernel's own inputs."""
    M = Y.shape[0]
    dz, Y, ah, bh, gamma, s1, s2 = (t.to(dt) for t in (dz, Y, ah, bh, gamma, s1, s2))
    return gamma * ah * (dz - s1 / M - (Y * ah + bh) * s2 / M)


def cg_pool_ref(Y, a, b, L, mask, scale, B, H, W, ph, pw, dt):
    z = bn_act_ref(Y, a, b, dt)
    return pool(z * torch.sigmoid(L.to(dt)) * keep_of(mask, scale, dt), B, H, W, ph, pw)


def cg_pool_bwd_ref(dout, Y, a, b, L, mask, scale, B, H, W, ph, pw, dt):
    """-> (dzd, dL): up sigmoid(l), up z s (1 - s), up = dout / (ph pw) keep (cnn_branch.hip:461-462)."""
    z, s = bn_act_ref(Y, a, b, dt), torch.sigmoid(L.to(dt))
    up = geom_up(dout.to(dt), B, H, W, ph, pw) / (ph * pw) * keep_of(mask, scale, dt)
    return up * s, up * z * s * (1 - s)


def gate16_fwd_ref(Y, a, b, Wg, bg, mask, scale, B, H, W, ph, pw, dt):
    """-> dict z, l, out (cnn_branch.hip:507-510)."""
    z = bn_act_ref(Y, a, b, dt)
    l = z @ Wg.to(dt).t() + bg.to(dt)
    return dict(z=z, l=l, out=pool(z * torch.sigmoid(l) * keep_of(mask, scale, dt), B, H, W, ph, pw))


def gate16_bwd_ref(dout, Y, a, b, L, Wg, mask, scale, B, H, W, ph, pw, dt):
    """-> (dz, dl) from the SAVED logits L, as the kernel (cnn_branch.hip:599-601): dz = up s + dl Wg."""
    dzd, dl = cg_pool_bwd_ref(dout, Y, a, b, L, mask, scale, B, H, W, ph, pw, dt)
    return dzd + dl @ Wg.to(dt), dl


def conv0_ref(mel, Wc, bias, dt):
    """mel [B, 128, T] -> Y [B T 128, 16] (passt_cnn.py:51: the spectrogram transposed to [B, 1, T, 128])."""
    x = mel.to(dt).transpose(1, 2).unsqueeze(1)
    return F.conv2d(x, Wc.to(dt), bias.to(dt), padding=1).permute(0, 2, 3, 1).reshape(-1, 16)


def conv0_patches(mel, dt, **leak):
    """[B T 128, 9]: the taps of every pixel, zero outside the spectrogram."""
    B, _, T = mel.shape
    src, ok = tap_index(B, T, 128, **leak)
    src, ok = src.to(mel.device), ok.to(mel.device)
    x = mel.to(dt).transpose(1, 2).reshape(-1)
    return torch.where(ok, x[src], torch.zeros((), dtype=dt, device=mel.device))


def conv0_dw_ref(dY, mel):
    """-> (dW [16, 9], sum|term|, dbias [16], sum|term|) in float64 from the bf16 dY and the fp32 spectrogram."""
    d, p = dY.double(), conv0_patches(mel, F64)
    return d.t() @ p, d.abs().t() @ p.abs(), d.sum(0), d.abs().sum(0)


def stats_terms(A, Bm=None, a=None, b=None, dt=F64):
    """sed_colstats' two term matrices: mode 0 (A, A^2), mode 1 (A, A (Bm a + b)) (cnn_branch.hip:264-265)."""
    A = A.to(dt)
    return A, (A * A if Bm is None else A * (Bm.to(dt) * a.to(dt) + b.to(dt)))


# ================================================================================================ A. inputs
@functools.lru_cache(maxsize=None)
def layer_inputs(i, B=B_A):
    """Production-like scales: a away from zero, logits over +-3, Y with a column mean, keep probability 0.9."""
    l, g = LAYERS[i], gen(7000 + i)
    M, Mo, co = B * l.H * l.W, B * (l.H // l.ph) * (l.W // l.pw), l.co
    d = dict(M=M, Mo=Mo)
    if i > 0:
        X = torch.full((B, l.H, l.W, l.cpin), NAN, dtype=F16)
        X[..., :l.cin] = torch.randn(B, l.H, l.W, l.cin, generator=g).to(F16)
        dcol = torch.full((M, l.Kp), NAN, dtype=BF16)
        dcol[:, :9 * l.cin] = (0.5 * torch.randn(M, 9 * l.cin, generator=g)).to(BF16)
        d.update(X=X, dcol=dcol)
    d["Y"] = 1.5 * torch.randn(M, l.ldy, generator=g) + 0.3
    d["a"], d["b"] = 0.5 + uni(g, co, lo=0.0), uni(g, co, lo=-0.3, hi=0.3)
    d["L"] = uni(g, M, l.ldy, lo=-3.0, hi=3.0)
    d["mask"] = (torch.rand(M, co, generator=g) < 0.9).to(torch.uint8)
    d["dout"] = uni(g, Mo, co)
    d["dz"] = uni(g, M, l.ldy) + 0.25
    d["gamma"] = 1.0 + uni(g, co, lo=-0.2, hi=0.2)
    y = d["Y"][:, :co].double()
    rstd = (y.var(0, unbiased=False) + 1e-3).rsqrt()
    d["ah"], d["bh"] = rstd.float(), (-y.mean(0) * rstd).float()
    t1, t2 = stats_terms(d["dz"][:, :co], d["Y"][:, :co], d["ah"], d["bh"])
    d["s1"], d["s2"] = t1.sum(0).float(), t2.sum(0).float()
    return d


@functools.lru_cache(maxsize=None)
def fused16_inputs(i, B=B_A):
    """Layers 0 and 1 (16 filters): the gate Linear of the fused path on top of layer_inputs."""
    d, g = dict(layer_inputs(i, B)), gen(7100 + i)
    d["Wg"], d["bg"] = uni(g, 16, 16, lo=-0.3, hi=0.3), uni(g, 16, lo=-0.5, hi=0.5)
    return d


@functools.lru_cache(maxsize=None)
def conv0_inputs(B, T, amp_from=None, amp=1.0, seed=7200):
    """mel [B, 128, T] with a mean (the sums do not cancel), conv0's weight and bias, a bf16 dY with a column mean.  Frames from
    `amp_from` on are multiplied by `amp` (part B: the rows only the last trip reaches)."""
    g = gen(seed + T)
    mel = uni(g, B, 128, T) + 0.5
    if amp_from is not None:
        mel[:, :, amp_from:] *= amp
    return dict(mel=mel, Wc=uni(g, 16, 1, 3, 3, lo=-0.3, hi=0.3), bias=uni(g, 16, lo=-0.2, hi=0.2),
                dY=(0.2 * uni(g, B * T * 128, 16) + 0.1).to(BF16))


# ================================================================================================ B. past one grid pass
FWD16_B = (1, 8193)
FWD16_AMP = 32.0
DW16_B = (1, 1025)
GATE16_BWD_B = (1, 8194, 128, 2, 2)
GATE16_AMP = 64.0
BN_B = dict(M=262145, C=32, pitch=64)                       # layer-2 widths: ldy = 32, Cp = ldo = 64
CG_POOL_B = dict(B=1, H=16386, W=64, C=32, Cpo=64, ph=2, pw=2)
CG_POOL_BWD_B = dict(B=1, H=8193, W=32, C=64, ldg=64, ph=1, pw=2)
IM2COL_B = dict(B=1, H=2049, W=64, C=16, Cp=64, Kp=256)
COL2IM_B = dict(B=1, H=65537, W=1, C=256, Kp=2304)
COLSTATS_B = dict(M=2048 * 4 * 16 + 4096 + 3, C=128)
TN_R = 524288 + 37
TN_RPAD = cdiv(TN_R, 64) * 64
TN_AMP = 128.0
TN_CASES = [(16, 0), (16, 1), (32, 0), (32, 1)]             # (C, in_f16)


def late(work_first, per_row=1):
    """First row all of whose items lie past the first grid pass."""
    return cdiv(work_first, per_row)


@functools.lru_cache(maxsize=None)
def fwd16_b_inputs():
    B, T = FWD16_B
    return conv0_inputs(B, T, amp_from=T - 2, amp=FWD16_AMP)


@functools.lru_cache(maxsize=None)
def dw16_b_inputs():
    return conv0_inputs(*DW16_B)


def cg_inputs(B, H, W, ph, pw, C, ldy, seed):
    g = gen(seed)
    M, Mo = B * H * W, B * (H // ph) * (W // pw)
    return dict(Y=1.5 * torch.randn(M, ldy, generator=g) + 0.3, a=0.5 + uni(g, C, lo=0.0), b=uni(g, C, lo=-0.3, hi=0.3),
                L=uni(g, M, ldy, lo=-3.0, hi=3.0), mask=(torch.rand(M, C, generator=g) < 0.9).to(torch.uint8), dout=uni(g, Mo, C))


@functools.lru_cache(maxsize=None)
def bn_b_inputs():
    """Y [M, 32], dz [M, 32] and the per-channel vectors of sed_bn_act / sed_bn_bwd, s1 / s2 the float64 sums rounded to fp32."""
    M, C = BN_B["M"], BN_B["C"]
    g = gen(7350)
    d = dict(Y=1.5 * torch.randn(M, C, generator=g) + 0.3, a=0.5 + uni(g, C, lo=0.0), b=uni(g, C, lo=-0.3, hi=0.3), dz=uni(g, M, C) + 0.25,
             gamma=1.0 + uni(g, C, lo=-0.2, hi=0.2))
    y = d["Y"].double()
    rstd = (y.var(0, unbiased=False) + 1e-3).rsqrt()
    d["ah"], d["bh"] = rstd.float(), (-y.mean(0) * rstd).float()
    t1, t2 = stats_terms(d["dz"], d["Y"], d["ah"], d["bh"])
    d["s1"], d["s2"] = t1.sum(0).float(), t2.sum(0).float()
    return d


@functools.lru_cache(maxsize=None)
def gate16_bwd_b_inputs():
    """Y, the gate, saved fp32 logits, a POSITIVE dout and a positive xhat affine (the terms of both sums share a sign); the output rows
    of the last two input rows (the 256 pixels of the second trip) carry GATE16_AMP times the gradient."""
    B, H, W, ph, pw = GATE16_BWD_B
    g = gen(7300)
    M, Mo = B * H * W, B * (H // ph) * (W // pw)
    d = dict(Y=uni(g, M, 16, lo=-1.5, hi=1.5) + 0.3, a=0.5 + uni(g, 16, lo=0.0), b=uni(g, 16, lo=-0.3, hi=0.3),
             Wg=uni(g, 16, 16, lo=-0.3, hi=0.3), bg=uni(g, 16, lo=-0.5, hi=0.5), mask=(torch.rand(M, 16, generator=g) < 0.9).to(torch.uint8),
             dout=uni(g, Mo, 16, lo=0.25, hi=1.25), ah=0.3 + 0.05 * uni(g, 16), bh=1.0 + 0.1 * uni(g, 16))
    d["dout"][-(W // pw):] *= GATE16_AMP
    z = bn_act_ref(d["Y"], d["a"], d["b"], F32)
    d["L"] = (z @ d["Wg"].t() + d["bg"]).contiguous()
    return d


@functools.lru_cache(maxsize=None)
def colstats_b_inputs():
    """A with a column mean, Bm a + b > 0: the terms of all four sums share a sign."""
    M, C = COLSTATS_B["M"], COLSTATS_B["C"]
    g = gen(7400)
    return dict(A=uni(g, M, C) + 0.5, Bm=uni(g, M, C), a=0.5 + 0.1 * uni(g, C), b=1.0 + 0.2 * uni(g, C))


@functools.lru_cache(maxsize=None)
def tn_inputs(C, in_f16):
    """[R, C] 16-bit values with a column mean; the rows of the second trip (R_first ..) carry TN_AMP times the value."""
    g = gen(7500 + C + in_f16)
    x = 0.5 * torch.randn(TN_R, C, generator=g) + 0.5
    x[transpose_narrow_launch(TN_RPAD)[1]:] *= TN_AMP
    return x.to(F16 if in_f16 else BF16)
