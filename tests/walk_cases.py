"""Cases, inputs, float64 references and restated launch arithmetic for the kernels of csrc/conformer.hip and csrc/fdy_cnn.hip past the
point where one pass of their grid ends (importable without a GPU: no test, no GPU code).  tests/test_walk_cases_cpu.py proves on the
CPU that every case crosses the threshold it is named for, that every drop condition holds and that the references are right;
tests/test_gpu_walk_kernels.py holds the hardware to them.

The bound is the one of tests/test_gpu_conformer.py and tests/test_gpu_fdy_cnn.py, per element (`judge`):

    |got - ref64| <= 8 max|ref32 - ref64| + half_ulp(storage)

The pure-torch half of those two files lives here and in tests/fdy_cases.py (they import it back): the Conformer restatement `chain`,
its `inputs` and `reference`, `half_ulp`, `maxerr`.

The functions `conv_walk`, `fdy_slabs`, `fdy_grid_items`, `freq_mean_map`, `elem_blocks` copy INTEGER FORMULAS of the entry points (the
source line is named at each), not kernels: they exist so that the CPU test can assert what a shape does to a launch."""
import collections
import functools

import torch
import torch.nn.functional as F

import fdy_cases as FC
from transformer4sed_amd import synth

F32, F64 = torch.float32, torch.float64
SENS = 10.0                 # a dropped contribution has to move the reference by this many bounds
C, KW = 768, 31
SIG_BITS = {"bf16": 8, "f16": 11}       # significand bits (with the hidden one) of the 16-bit storage formats


def cdiv(a, b):
    return -(-a // b)


def maxerr(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def half_ulp(ref64, storage):
    """Half a unit in the last place of `storage` at each element's magnitude: 2^(floor(log2 |x|) - p) for p significand bits (between
    2^-(p+1) and 2^-p of |x|; f16 subnormals: 2^-25).  Zero for fp32 outputs."""
    if storage == "f32":
        return torch.zeros_like(ref64)
    _, e = torch.frexp(ref64.abs().clamp_min(1e-300))          # |x| = m 2^e, 0.5 <= m < 1
    h = torch.ldexp(torch.ones_like(ref64), e - 1 - SIG_BITS[storage])
    return h.clamp_min(2.0 ** -25) if storage == "f16" else h


def judge(got, ref64, ref32, storage="f32"):
    """The bound of `check()` in tests/test_gpu_conformer.py and tests/test_gpu_fdy_cnn.py, without the logging:
    -> (max error, yardstick max|ref32 - ref64|, worst error / bound, every element inside, max|ref64|)."""
    got, ref64 = got.detach().double().cpu(), ref64.detach().double().cpu()
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    yard = maxerr(ref32, ref64)
    diff, tol = (got - ref64).abs(), 8 * yard + half_ulp(ref64, storage)
    return float(diff.max()), yard, float((diff / tol.clamp_min(1e-300)).max()), bool((diff <= tol).all()), float(ref64.abs().max())


def bound32(ref64, ref32):
    """The bound of an fp32 output: 8 yardsticks, one number."""
    return 8 * maxerr(ref32, ref64)


# ================================================================================================ Conformer: the restatement
def chain(x, w, b, gamma, beta, B, T, conv=True):
    """x [B T, 2 C] -> (y [B T, C], c [B T, C]) in x's dtype."""
    u = F.glu(x.view(B, T, 2 * C).transpose(1, 2), dim=1)
    c = F.conv1d(u, w.view(C, 1, KW), b, padding=KW // 2, groups=C) if conv else u
    c = c.transpose(1, 2)
    n = F.layer_norm(c, (C,), gamma, beta, 1e-5)
    return (n * torch.sigmoid(n)).reshape(B * T, C), c.reshape(B * T, C)


@functools.lru_cache(maxsize=None)
def _inputs(B, T, tag):
    M = B * T
    return dict(x=torch.from_numpy(synth.det_normal(f"conf/{tag}/x/{B}x{T}", (M, 2 * C), 1.5)),
                w=torch.from_numpy(0.35 * synth.det_uniform(f"conf/{tag}/w", (C, KW))),
                b=torch.from_numpy(0.1 * synth.det_uniform(f"conf/{tag}/b", (C,))),
                gamma=torch.from_numpy(1.0 + 0.2 * synth.det_uniform(f"conf/{tag}/g", (C,))),
                beta=torch.from_numpy(0.1 * synth.det_uniform(f"conf/{tag}/bt", (C,))),
                dy=torch.from_numpy(synth.det_uniform(f"conf/{tag}/dy/{B}x{T}", (M, C))))


def inputs(B, T, tag="k"):
    """fp32 inputs (the kernel's input format: nothing to round).  The values are hashed once per shape; every call gets its own copies."""
    return {k: v.clone() for k, v in _inputs(B, T, tag).items()}


@functools.lru_cache(maxsize=None)
def reference(B, T):
    """The restatement in float64 and float32 on the CPU, forward and (autograd) backward; computed once per shape."""
    out = {}
    for dt in (torch.float64, torch.float32):
        t = {k: v.to(dt).requires_grad_(k != "dy") for k, v in inputs(B, T).items()}
        y, c = chain(t["x"], t["w"], t["b"], t["gamma"], t["beta"], B, T)
        mu = c.mean(-1)
        rstd = (c.var(-1, unbiased=False) + 1e-5).rsqrt()
        (y * t["dy"]).sum().backward()
        out[dt] = dict(y=y.detach(), c=c.detach(), mean=mu.detach(), rstd=rstd.detach(), dx=t["x"].grad, dw=t["w"].grad, db=t["b"].grad,
                       dgamma=t["gamma"].grad, dbeta=t["beta"].grad)
    return out[torch.float64], out[torch.float32]


# ================================================================================================ Conformer: the tile walk
# csrc/conformer.hip:17-23
TT, HALO, BWD_MAX_WG, BWD_SLOTS = 20, 15, 256, KW + 3
CONV_SHAPES_TESTED = [(1, 8), (3, 31), (2, 65), (3, 100), (2, 1000)]        # SHAPES of tests/test_gpu_conformer.py
CONV_WALK_SHAPES = [(7, 1010), (27, 390)]
CONV_SUMS = ("dbeta", "dgamma", "db", "dw15")                              # the per-frame sums a workgroup carries over its tiles


def conv_walk(B, T):
    """sed_conv_glu_dw_bwd, csrc/conformer.hip:283-286 and the loop head at :170 -> (ntiles, nwg, steps of the busiest workgroup)."""
    ntiles = B * cdiv(T, TT)
    nwg = min(ntiles, BWD_MAX_WG)
    return ntiles, nwg, cdiv(ntiles, nwg)


def conv_partial_floats(B, T):
    """csrc/conformer.hip:287."""
    return conv_walk(B, T)[1] * BWD_SLOTS * C


def conv_tile(B, T, tile):
    """csrc/conformer.hip:171 -> (clip, first frame, frames owned: the `t >= T` break at :226 cuts a ragged tile)."""
    tiles = cdiv(T, TT)
    b, t0 = tile // tiles, (tile % tiles) * TT
    return b, t0, min(TT, T - t0)


def conv_tile_rows(B, T, tile):
    b, t0, n = conv_tile(B, T, tile)
    return slice(b * T + t0, b * T + t0 + n)


def conv_wg_tiles(B, T, wg):
    """The tiles workgroup `wg` walks, in order (csrc/conformer.hip:170)."""
    ntiles, nwg, _ = conv_walk(B, T)
    return list(range(wg, ntiles, nwg))


def conv_drop_tiles(B, T):
    """{name: tile}: the ragged tile of the first step, the first tile of every later step, the last tile."""
    ntiles, nwg, steps = conv_walk(B, T)
    tiles = cdiv(T, TT)
    d = {}
    if T % TT:
        d["ragged first-step tile"] = tiles - 1
    for s in range(1, steps):
        d[f"first tile of step {s + 1}"] = s * nwg
    d["last tile"] = ntiles - 1
    return d


@functools.lru_cache(maxsize=None)
def conv_terms(B, T):
    """Per frame and channel, in float64, the terms of the four sums a workgroup of the backward keeps in registers over the tiles it
    walks (csrc/conformer.hip:238-247): dbeta = sum d n, dgamma = sum d n h, dbias = sum d c, dw[:, 15] = sum u d c.  [B T, C] each."""
    r64, _ = reference(B, T)
    t = {k: v.double() for k, v in inputs(B, T).items()}
    a, g = t["x"][:, :C], t["x"][:, C:]
    u = a * torch.sigmoid(g)
    h = (r64["c"] - r64["mean"].reshape(-1, 1)) * r64["rstd"].reshape(-1, 1)
    n = h * t["gamma"] + t["beta"]
    s = torch.sigmoid(n)
    dn = t["dy"] * (s + n * s * (1 - s))
    dg = dn * t["gamma"]
    dc = r64["rstd"].reshape(-1, 1) * (dg - dg.mean(-1, keepdim=True) - h * (dg * h).mean(-1, keepdim=True))
    return dict(dbeta=dn, dgamma=dn * h, db=dc, dw15=u * dc)


def conv_sum_refs(B, T):
    """{sum: (ref64 [C], bound)} with the bound of its whole output tensor (dw: all 31 taps)."""
    r64, r32 = reference(B, T)
    return {k: ((r64["dw"][:, KW // 2] if k == "dw15" else r64[k]), bound32(r64["dw" if k == "dw15" else k], r32["dw" if k == "dw15" else k]))
            for k in CONV_SUMS}


def conv_drop_ratios(B, T):
    """{(tile name, sum): how many bounds the reference moves by when the tile's frames are left out of the sum}."""
    terms, refs = conv_terms(B, T), conv_sum_refs(B, T)
    return {(nm, k): float(terms[k][conv_tile_rows(B, T, tile)].sum(0).abs().max()) / refs[k][1]
            for nm, tile in conv_drop_tiles(B, T).items() for k in CONV_SUMS}


def conv_walk_emulated(terms, B, T, walk=True):
    """The sum of `terms` [B T, C] in fp32 in the kernel's order: a workgroup adds the frames of the tiles it walks one after the other
    (csrc/conformer.hip:224-250), then one thread adds the workgroups' partials in workgroup order (:273).  (The terms themselves are
    the float64 ones rounded to fp32: this emulates the ORDER of the additions, not the arithmetic inside a term.)
    walk=False: every workgroup stops after its first tile -- the grid capped at 256 without the loop."""
    ntiles, nwg, steps = conv_walk(B, T)
    M = B * T
    idx = torch.full((nwg, steps * TT), M, dtype=torch.long)            # M: a row of zeros (adding 0 is exact)
    for wg in range(nwg):
        pos = 0
        for tile in conv_wg_tiles(B, T, wg)[:None if walk else 1]:
            rows = conv_tile_rows(B, T, tile)
            n = rows.stop - rows.start
            idx[wg, pos:pos + n] = torch.arange(rows.start, rows.stop)
            pos += n
    padded = torch.cat([terms.to(F32), torch.zeros(1, terms.shape[1], dtype=F32)])
    acc = torch.zeros(nwg, terms.shape[1], dtype=F32)
    for j in range(idx.shape[1]):
        acc += padded[idx[:, j]]
    s = torch.zeros(terms.shape[1], dtype=F32)
    for g in range(nwg):
        s += acc[g]
    return s


def conv_args_ok(B, T, Cc, partial_floats):
    """The argument check of sed_conv_glu_dw_bwd (csrc/conformer.hip:282-287) without its pointer tests."""
    return Cc == C and B > 0 and T > 0 and B * cdiv(T, TT) <= 0x7fffffff and partial_floats >= conv_partial_floats(B, T)


# ================================================================================================ FDY: launch arithmetic
FDY_TR, FDY_K, FDY_CAP = 16, 4, 16384


def fdy_slabs(R):
    """csrc/fdy_cnn.hip:419-422, 440 -> (row slabs of dW1's reduction, rows per slab)."""
    s = min(32, max(1, R // 128))
    return s, cdiv(R, s)


def fdy_grid_items(work, threads=256, cap=FDY_CAP):
    """fdy_grid, csrc/fdy_cnn.hip:17-20, for `work` float4 items -> (workgroups, items of the first pass, passes)."""
    blocks = max(1, min(cap, cdiv(work, threads)))
    return blocks, blocks * threads, cdiv(work, blocks * threads)


def mix_items(M, ldy):
    """csrc/fdy_cnn.hip:230."""
    return M * (ldy // 4)


def mean_add_items(R, W, Cc):
    """csrc/fdy_cnn.hip:465."""
    return R * W * (Cc // 4)


def freq_mean_map(Cc):
    """fdy_freq_mean_kernel, csrc/fdy_cnn.hip:29-32 -> (threads per bin nv, bins in flight wl, threads with l >= wl: idle)."""
    nv = Cc // 8
    wl = 256 // nv
    return nv, wl, 256 - nv * wl


def elem_blocks(n, cap=65536):
    """sed_swish_bwd / sed_scale_add_f32, csrc/conformer.hip:350-351, 381-382 -> (workgroups, floats of the first pass, passes)."""
    blocks = min(cap, cdiv(n // 4, 256))
    return blocks, blocks * 1024, cdiv(n, blocks * 1024)


def mix_layout(co):
    """The engine's row pitches as tests/test_gpu_fdy_cnn.py's test_mix_forward_and_backward derives them -> (ld4, ldy)."""
    Nc = (4 * co + 127) // 128 * 128
    return (64 if 4 * co == 64 else Nc), (co if co < 128 else (co + 127) // 128 * 128)


# ================================================================================================ FDY head backward at the slab cap
HEAD_WALK_CASES = [(9, 500, 2, 16), (5, 1000, 2, 32)]
HEAD_WALK_T = 31.0
HEAD_GRADS = ("c1w", "bn_w", "bn_b", "c2w", "c2b")


def head_ws_floats(R, cin, hid):
    """csrc/fdy_cnn.hip:429-431."""
    P = 6 * hid + FDY_K
    return (P + 3) // 4 * 4 + fdy_slabs(R)[0] * hid * 3 * cin


def head_args_ok(B, H, cin, hid, temperature, ws_floats, train):
    """The argument checks of sed_fdy_attn_taps (:114-116), sed_fdy_attn_softmax (:192-194) and sed_fdy_attn_bwd (:428-433)."""
    R = B * H
    taps = B > 0 and H > 0 and cin > 0 and hid > 0 and R <= 0x7fffffff and ((FDY_TR + 2) * cin + FDY_TR * hid) * 4 <= 64 * 1024
    soft = R > 0 and temperature > 0 and not (train and R < 2) and (3 + FDY_K) * hid * 4 <= 64 * 1024
    bwd = temperature > 0 and ws_floats >= head_ws_floats(R, cin, hid) and (FDY_TR * FDY_K + 3 * FDY_TR * hid) * 4 <= 64 * 1024
    return taps and soft and bwd


@functools.lru_cache(maxsize=None)
def head_case(B, H, W, cin, train):
    """-> (inputs, ref64, ref32) of the head at temperature 31; computed once."""
    inp = FC.head_inputs(B, H, W, cin, HEAD_WALK_T)
    return inp, FC.head_ref(inp, HEAD_WALK_T, train, F64), FC.head_ref(inp, HEAD_WALK_T, train, F32)


@functools.lru_cache(maxsize=None)
def head_drop_ratios(B, H, W, cin):
    """Evaluation mode (rows independent): zeroing `da` on the rows of the LAST slab removes that slab from every parameter gradient
    -> {gradient: bounds the float64 reference moves by}."""
    inp, r64, r32 = head_case(B, H, W, cin, False)
    R = B * H
    nslab, rows_per = fdy_slabs(R)
    cut = dict(inp, da=inp["da"].clone())
    cut["da"][(nslab - 1) * rows_per:] = 0.0
    d64 = FC.head_ref(cut, HEAD_WALK_T, False, F64)
    return {k: float((r64["g_" + k] - d64["g_" + k]).abs().max()) / bound32(r64["g_" + k], r32["g_" + k]) for k in HEAD_GRADS}


# ================================================================================================ frequency mean off the powers of two
FREQ_WIDTHS_TESTED = (16, 32, 256)                                          # cin of fdy_cases.HEAD_CASES
FreqCase = collections.namedtuple("FreqCase", "C W Cp R")
FREQ_CASES = [FreqCase(8, 3, 64, 5), FreqCase(8, 300, 64, 5), FreqCase(24, 7, 64, 5), FreqCase(24, 100, 64, 5),
              FreqCase(384, 3, 448, 5), FreqCase(384, 7, 448, 5)]


def freq_inputs(c):
    """x [R, W, C], exact in bf16 and IEEE half (as head_inputs)."""
    return torch.from_numpy(FC.exact16(f"fdy/freq/{c.R}x{c.W}x{c.C}", (c.R, c.W, c.C), 2.0))


def freq_refs(x):
    return x.double().mean(1), x.mean(1)


def freq_mean_emulated(x):
    """The mean in fp32 in the kernel's order (csrc/fdy_cnn.hip:34-50): thread group l adds bins l, l + wl, ...; then the wl partials
    in order; one division by W."""
    R, W, Cc = x.shape
    _, wl, _ = freq_mean_map(Cc)
    red = torch.zeros(wl, R, Cc, dtype=F32)
    for w in range(W):
        red[w % wl] += x[:, w]
    s = torch.zeros(R, Cc, dtype=F32)
    for j in range(wl):
        s += red[j]
    return s / torch.tensor(float(W), dtype=F32)


def freq_args_ok(c):
    """csrc/fdy_cnn.hip:55."""
    return 0 < c.R <= 0x7fffffff and c.W > 0 and c.C > 0 and c.C % 8 == 0 and c.C <= 2048 and c.Cp % 8 == 0 and c.Cp >= c.C


# ================================================================================================ mixing forward past the grid cap
MixCase = collections.namedtuple("MixCase", "B H W co ld4 ldy")
MIX_WALK_CASES = [MixCase(2, 1025, 128, 16, 64, 64), MixCase(5, 1000, 128, 16, 64, 64)]


def mix_walk_inputs(c, dev="cpu"):
    """Y4 [M, 4 co] and the softmaxed att [B H, 4], drawn on `dev` from a seeded generator (synth.det_normal hashes every element: 7 s
    for the larger case) -> fp32 tensors on `dev`."""
    g = torch.Generator(device=dev).manual_seed(4100 + c.B * c.H)
    M, R = c.B * c.H * c.W, c.B * c.H
    y4 = torch.randn(M, 4 * c.co, generator=g, device=dev)
    att = torch.softmax(1.5 * torch.randn(R, FDY_K, generator=g, device=dev), -1)
    return y4, att


def mix_direct(y4, att, W, co, dt):
    """Y[m, o] = sum_k att[m // W, k] Y4[m, k co + o], the four-term sum written out in dtype dt."""
    R = att.shape[0]
    return (y4.to(dt).view(R, W, FDY_K, co) * att.to(dt).view(R, 1, FDY_K, 1)).sum(2).reshape(R * W, co)


def mix_late_rows(c):
    """Rows whose every item lies past the first grid pass."""
    return cdiv(fdy_grid_items(mix_items(c.B * c.H * c.W, c.ldy))[1], c.ldy // 4)


def mix_args_ok(c):
    """csrc/fdy_cnn.hip:229."""
    M = c.B * c.H * c.W
    return M > 0 and c.W > 0 and M % c.W == 0 and c.co > 0 and c.co % 4 == 0 and c.ld4 % 4 == 0 and c.ld4 >= FDY_K * c.co and c.ldy % 4 == 0 \
        and c.ldy >= c.co


# ================================================================================================ mean backward past the grid cap
MeanCase = collections.namedtuple("MeanCase", "R W C exact")
MEAN_WALK_CASES = [MeanCase(2050, 128, 64, True), MeanCase(2050, 100, 64, False)]


def mean_walk_inputs(c, dev="cpu"):
    """dX0 [R, W, C] fp32 and dpm [R, C] in multiples of 2^-6 (|dpm| <= 4): with W a power of two dpm / W is exact and
    dX0 + dpm / W is rounded once, whichever way it is computed."""
    g = torch.Generator(device=dev).manual_seed(4200 + c.W)
    dx0 = torch.randn(c.R, c.W, c.C, generator=g, device=dev)
    dpm = torch.randint(-256, 257, (c.R, c.C), generator=g, device=dev).to(F32) / 64.0
    return dx0, dpm


def mean_add_direct(dx0, dpm, W, dt):
    return dx0.to(dt) + dpm.to(dt).unsqueeze(1) / W


def mean_args_ok(c):
    """csrc/fdy_cnn.hip:464."""
    return c.R > 0 and c.W > 0 and c.C > 0 and c.C % 4 == 0


# ================================================================================================ Swish backward, scale-add past 65 536 blocks
ELEM_N_TESTED = 130 * C
ELEM_N = 65536 * 1024 + 1200
ELEM_WIN = 4096


def elem_windows(n=ELEM_N):
    """Start, the window straddling the end of the first pass, end."""
    first = elem_blocks(n)[1]
    return [slice(0, ELEM_WIN), slice(first - ELEM_WIN // 2, first + ELEM_WIN // 2), slice(n - ELEM_WIN, n)]


def swish_bwd_direct(dy, h, dt):
    dy, h = dy.to(dt), h.to(dt)
    s = torch.sigmoid(h)
    return dy * (s + h * s * (1 - s))


def elem_args_ok(n):
    """csrc/conformer.hip:349, 380."""
    return n > 0 and n % 4 == 0


# ================================================================================================ model level
MODEL_B, MODEL_T = 8, 1000
