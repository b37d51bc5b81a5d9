"""Exact-result cases, float64 references, deliberately wrong references and the restated launch arithmetic for the LoRA kernels:
sed_lora_rowproj, sed_lora_colreduce, sed_lora_grad, sed_lora_merge (csrc/lora.hip) and the LoRA term of sed_weight_images
(csrc/layout.hip).  Importable without a GPU: no test, no GPU code.  tests/test_lora_cases_cpu.py proves the constructions on the CPU,
tests/test_gpu_lora_kernels.py holds the hardware to them bit for bit.

Inputs.  Every operand is a small integer (exact in bf16 and IEEE half), the fp32 factors are integers too and every scale is a power of
two, so each product and each partial sum is an integer (or a multiple of 1/8) below 2^24: the fp32 result does not depend on the order
of accumulation -- wave quarters, slabs, atomics, grid passes cannot show -- and a correct kernel returns it bit for bit.  `budget`
raises for a case that would round.  Accumulated outputs (G, dA, dB) start from non-zero integers.  Pitched operands hold NaN in their
padding columns, operand buffers end with their last row.

`*_ref(case, inputs, fault)`: plain float64 matmuls; `fault` names one of the mistakes of `FAULTS`, for the CPU test to show that the
exact comparison sees each of them in every case that has the edge.

`*_geometry`: INTEGER FORMULAS of the entry points (grid cap, slab and rows-per-workgroup arithmetic, wave quarters), not kernels: they
let the CPU test assert which branch a named case reaches."""
import collections

import torch

from exact_cases import BF16, F16, check_budget, dyadic, int_operands, nonzero_ints

F32, F64 = torch.float32, torch.float64
GUARD = 256                 # NaN canary elements behind the last valid element of every output
AMAX = 7                    # operand magnitude of the matmul cases
G0_MAX = 100                # magnitude of the integers an accumulated output starts from
NAN = float("nan")
FAULTS = ("last_row", "last_colgroup", "quarter", "rank_shift", "layout", "assign", "decode")


def cdiv(a, b):
    return -(-a // b)


def dt16(f16):
    return F16 if f16 else BF16


def denom_of(scale):
    d = 1.0 / scale
    assert d == int(d) and int(d) & (int(d) - 1) == 0, scale
    return int(d)


def check_16bit(amax, DT, denom=1):
    """Raises unless every multiple of 1 / denom up to amax is exact in DT: 8 significant bits in bf16, 11 in IEEE half."""
    lim = 256 if DT == BF16 else 2048
    if amax * denom > lim:
        raise ValueError(f"{amax} x {denom} units exceed the {lim} consecutive integers of {DT}")
    return amax * denom


def nonzero_fill(shape, seed):
    """Integers in +-1 .. +-G0_MAX, none zero: what an accumulated output holds before the call."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    m = torch.randint(1, G0_MAX + 1, shape, generator=g).float()
    return m * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


def pitched16(x, ld, DT):
    """[M, K] integers -> [M, ld] of DT, NaN in the padding columns."""
    out = torch.full((x.shape[0], ld), NAN, dtype=DT)
    out[:, :x.shape[1]] = x.to(DT)
    return out


def as_other16(x16):
    """The bits of an IEEE-half tensor read as bf16 (fault 'decode'), as float64."""
    return x16.view(torch.int16).view(BF16).double()


def _shift_cols(w):
    """Column j taken from column j - 1 (fault 'rank_shift'); w [..., r]."""
    out = w.clone()
    out[..., 1:] = w[..., :-1]
    return out


# ================================================================================================ sed_lora_rowproj
Rowproj = collections.namedtuple("Rowproj", "K r w_kxr f16 M pad scale")
# (K, r, w_kxr, x_f16, M, ldx - K, scale).  K 64: wave 0 alone has work; 192: wave 3 empty; 320: wave 2 half filled, wave 3 empty;
# 1088: the [K, r] staging loops run again past k = 1024; 2112 / 3072: a second 512-column trip inside a wave quarter; 8256 (r <= 8): the
# [r, K] staging loop runs again past 2048 float4.  M 12305 (K 64): 770 tiles on 768 workgroups.
ROWPROJ_CASES = [Rowproj(*c) for c in [
    (64, 1, 0, 0, 1, 0, 1.0), (64, 3, 1, 1, 15, 8, 0.125), (64, 8, 1, 0, 16, 0, 1.0), (64, 9, 1, 1, 17, 8, 1.0),
    (64, 16, 0, 0, 12305, 0, 0.125), (64, 3, 1, 0, 12305, 8, 1.0),
    (192, 3, 1, 0, 17, 0, 1.0), (192, 16, 1, 1, 15, 8, 0.125),
    (320, 8, 0, 1, 17, 8, 1.0), (320, 1, 1, 0, 16, 0, 0.125), (320, 9, 0, 0, 1, 8, 1.0),
    (1088, 3, 1, 0, 17, 8, 1.0), (1088, 8, 1, 1, 15, 0, 0.125), (1088, 16, 1, 0, 16, 8, 1.0),
    (2112, 8, 0, 0, 17, 0, 1.0), (2112, 9, 1, 1, 15, 8, 0.125),
    (3072, 8, 1, 0, 17, 8, 0.125), (3072, 16, 0, 1, 16, 0, 1.0),
    (8256, 8, 0, 0, 17, 0, 1.0), (8256, 3, 0, 1, 15, 8, 0.125), (8256, 1, 1, 0, 16, 0, 1.0)]]


def rowproj_id(c):
    return f"K{c.K}-r{c.r}-{'kxr' if c.w_kxr else 'rxk'}-{'f16' if c.f16 else 'bf16'}-M{c.M}-ld{c.K + c.pad}-s{c.scale:g}"


def rowproj_budget(c):
    check_16bit(AMAX, dt16(c.f16))          # X, and the factor, which the kernel stages in X's type
    return check_budget(c.K, AMAX, AMAX, alpha=c.scale, denom=denom_of(c.scale))


def rowproj_inputs(c, seed=1000):
    """X [M, ldx] 16-bit (NaN padding); Wm fp32 as the kernel reads it ([K, r] if w_kxr else [r, K]); W [r, K] the same factor."""
    s = seed + 7 * ROWPROJ_CASES.index(c) if c in ROWPROJ_CASES else seed
    W = int_operands(c.r, c.K, AMAX, s + 1)
    return dict(X=pitched16(int_operands(c.M, c.K, AMAX, s), c.K + c.pad, dt16(c.f16)), W=W, Wm=W.t().contiguous() if c.w_kxr else W)


def rowproj_ref(c, i, fault=None, quarter=0):
    """u = scale X Wm^T in float64 [M, r]."""
    X, W = i["X"][:, :c.K].double(), i["W"].double()
    if fault == "decode":
        X = as_other16(i["X"][:, :c.K].contiguous())
    if fault == "layout":                   # the [K, r] buffer read as [r, K]
        W = i["Wm"].reshape(c.r, c.K).double()
    if fault == "rank_shift":
        W = _shift_cols(W.t()).t()
    if fault == "quarter":
        kb, ke = rowproj_geometry(c.M, c.K, c.r).quarters[quarter]
        X = X.clone()
        X[:, kb:ke] = 0
    u = c.scale * X @ W.t()
    if fault == "last_row":
        u[c.M - 1] = 0
    return u


RowprojGeometry = collections.namedtuple("RowprojGeometry", "blocks passes rows_w lds branch staging_trips kq quarters trips")


def rowproj_args_ok(M, K, ldx, r):
    """Argument check of sed_lora_rowproj (csrc/lora.hip), the LDS limit included."""
    return not (M <= 0 or K <= 0 or K % 64 or ldx % 8 or ldx < K or r <= 0 or r > 16) and (8 if r <= 8 else 16) * (2 * K + 16) <= 152 * 1024


def rowproj_geometry(M, K, r, w_kxr=0):
    """sed_lora_rowproj / lora_rowproj_kernel (csrc/lora.hip): workgroups (one 16-row tile at a time, at most 768) and passes over the
    tiles; staged rows and LDS bytes of the factor image; the staging branch and how often its loop runs; the wave quarter
    kq = ((K / 64 + 3) / 4) * 64 with each wave's [kb, ke) and its number of 512-column trips."""
    tiles = cdiv(M, 16)
    blocks = min(tiles, 768)
    rows_w = 8 if r <= 8 else 16
    branch = ("kxr8" if r == 8 else "kxr") if w_kxr else "rxk"
    staging = cdiv(K, 1024) if w_kxr else cdiv(K // 4, 2048)
    kq = ((K // 64 + 3) // 4) * 64
    quarters = [(w * kq, max(w * kq, min(w * kq + kq, K))) for w in range(4)]
    return RowprojGeometry(blocks, cdiv(tiles, blocks), rows_w, rows_w * (2 * K + 16), branch, staging, kq, quarters,
                           [cdiv(ke - kb, 512) for kb, ke in quarters])


# ================================================================================================ sed_lora_colreduce
Colreduce = collections.namedtuple("Colreduce", "C r g_cxr f16 M pad scale")
# (C, r, g_cxr, y_f16, M, ldy - C, scale).  C 4 / 252 / 260: lanes whose four columns lie past C (260: in a second column group);
# M 32805 at C 4: 64 rows per workgroup, two trips of the row loop.
COLREDUCE_CASES = [Colreduce(*c) for c in [
    (4, 1, 1, 0, 1, 0, 1.0), (4, 3, 0, 1, 31, 4, 0.125), (4, 8, 1, 0, 32805, 0, 1.0), (4, 3, 0, 1, 32805, 4, 0.125),
    (252, 8, 1, 1, 32, 4, 1.0), (252, 1, 0, 0, 33, 0, 0.125), (252, 3, 1, 0, 4099, 4, 1.0),
    (256, 3, 0, 0, 33, 0, 1.0), (256, 8, 1, 1, 31, 4, 0.125), (256, 1, 1, 0, 4099, 0, 1.0),
    (260, 8, 0, 0, 33, 4, 1.0), (260, 3, 1, 1, 32, 0, 0.125), (260, 1, 0, 1, 4099, 4, 1.0), (260, 8, 1, 0, 1, 0, 1.0),
    (768, 8, 0, 1, 4099, 0, 0.125), (768, 3, 1, 0, 31, 4, 1.0), (768, 1, 0, 0, 32, 0, 1.0), (768, 8, 1, 1, 33, 4, 1.0)]]


def colreduce_id(c):
    return f"C{c.C}-r{c.r}-{'cxr' if c.g_cxr else 'rxc'}-{'f16' if c.f16 else 'bf16'}-M{c.M}-ld{c.C + c.pad}-s{c.scale:g}"


def colreduce_budget(c):
    check_16bit(AMAX, dt16(c.f16))
    return check_budget(c.M, AMAX, AMAX, alpha=c.scale, res_max=G0_MAX, denom=denom_of(c.scale))


def colreduce_inputs(c, seed=2000):
    """Y [M, ldy] 16-bit (NaN padding), P [M, r] fp32, G0: what G holds before the call ([C, r] if g_cxr else [r, C])."""
    s = seed + 7 * COLREDUCE_CASES.index(c) if c in COLREDUCE_CASES else seed
    return dict(Y=pitched16(int_operands(c.M, c.C, AMAX, s), c.C + c.pad, dt16(c.f16)), P=int_operands(c.M, c.r, AMAX, s + 1),
                G0=nonzero_fill((c.C, c.r) if c.g_cxr else (c.r, c.C), s + 2))


def colreduce_ref(c, i, fault=None):
    """G = G0 + scale P^T Y in float64, in the layout of the case."""
    Y, P, G0 = i["Y"][:, :c.C].double(), i["P"].double(), i["G0"].double()
    if fault == "decode":
        Y = as_other16(i["Y"][:, :c.C].contiguous())
    if fault == "rank_shift":
        P = _shift_cols(P)
    if fault == "last_row":
        P = P.clone()
        P[c.M - 1] = 0
    d = c.scale * P.t() @ Y                                   # [r, C]
    if fault == "last_colgroup":
        d[:, c.C - 4:] = 0
    right = d.t() if c.g_cxr else d
    if fault == "layout":                                      # the update written in the order of the other layout
        right = (d if c.g_cxr else d.t()).contiguous().reshape(right.shape)
    return right if fault == "assign" else G0 + right


ColreduceGeometry = collections.namedtuple("ColreduceGeometry", "cgs rows_per_wg slabs row_trips guard_false")


def colreduce_args_ok(M, C, ldy, r):
    """Argument check of sed_lora_colreduce (csrc/lora.hip)."""
    return not (M <= 0 or C <= 0 or C % 4 or ldy % 4 or ldy < C or r <= 0 or r > 8)


def colreduce_geometry(M, C):
    """sed_lora_colreduce (csrc/lora.hip): column groups of 256, slabs = 1024 / groups, rows per workgroup = cdiv(M, slabs) rounded up
    to 32, the slabs that leaves, the trips of the 32-row loop, and whether some lane's columns lie past C (the `c < C` guard)."""
    cgs = cdiv(C, 256)
    slabs = max(1, 1024 // cgs)
    rows = cdiv(cdiv(M, slabs), 32) * 32
    return ColreduceGeometry(cgs, rows, cdiv(M, rows), rows // 32, cgs * 256 > C)


# ================================================================================================ sed_lora_grad
Grad = collections.namedtuple("Grad", "n_out k_in r s")
# k_in 513: a second 512-column trip; 1024: the last narrow width; 1025 / 1028: wide (four waves share a row) with ragged quarters;
# (100, 64): the dA half leaves workgroups of the shared grid idle; (64, 1025): the same in the wide form; (1, 3072), (3, 1024): the dB half does.
GRAD_CASES = [Grad(*c) for c in [
    (1, 1, 1, 1.0), (3, 63, 5, 0.125), (4, 64, 8, 1.0), (5, 65, 16, 1.0), (31, 257, 1, 0.125), (32, 513, 5, 1.0), (33, 1024, 8, 0.125),
    (100, 64, 16, 1.0), (64, 1025, 8, 1.0), (3, 1025, 1, 0.125), (33, 1028, 5, 1.0), (5, 3072, 16, 0.125), (1, 3072, 8, 1.0),
    (100, 513, 8, 0.125), (3, 1024, 16, 1.0), (31, 1028, 16, 0.125), (32, 3072, 5, 1.0), (4, 257, 16, 1.0), (100, 1025, 5, 1.0),
    (33, 65, 1, 1.0)]]


def grad_id(c):
    return f"n{c.n_out}-k{c.k_in}-r{c.r}-s{c.s:g}"


def grad_budget(c):
    return max(check_budget(n, AMAX, AMAX, alpha=c.s, res_max=G0_MAX, denom=denom_of(c.s)) for n in (c.k_in, c.n_out))


def grad_inputs(c, seed=3000):
    s = seed + 7 * GRAD_CASES.index(c) if c in GRAD_CASES else seed
    return dict(dW=int_operands(c.n_out, c.k_in, AMAX, s), A=int_operands(c.r, c.k_in, AMAX, s + 1), B=int_operands(c.n_out, c.r, AMAX, s + 2),
                dA0=nonzero_fill((c.r, c.k_in), s + 3), dB0=nonzero_fill((c.n_out, c.r), s + 4))


def grad_ref(c, i, fault=None, quarter=0):
    """(dA0 + s B^T dW [r, k_in], dB0 + s dW A^T [n_out, r]) in float64.  Fault 'quarter' drops one wave quarter of the dB sums."""
    dW, A, B = i["dW"].double(), i["A"].double(), i["B"].double()
    dWb = dW
    if fault == "last_row":
        dW = dW.clone()
        dW[c.n_out - 1] = 0
        dWb = dW
    if fault == "last_colgroup":
        dW = dW.clone()
        dW[:, (cdiv(c.k_in, 4) - 1) * 4:] = 0
        dWb = dW
    if fault == "quarter":
        kb, ke = grad_geometry(c.n_out, c.k_in).quarters[quarter]
        dWb = dW.clone()
        dWb[:, kb:ke] = 0
    if fault == "rank_shift":
        A, B = _shift_cols(A.t()).t(), _shift_cols(B)
    dA, dB = c.s * B.t() @ dW, c.s * dWb @ A.t()
    return (dA, dB) if fault == "assign" else (i["dA0"].double() + dA, i["dB0"].double() + dB)


GradGeometry = collections.namedtuple("GradGeometry", "wide kq quarters trips nb_a nb_b grid surplus_a surplus_b ragged_slab")


def grad_args_ok(n_out, k_in, r):
    """Argument check of sed_lora_grad (csrc/lora.hip)."""
    return n_out > 0 and k_in > 0 and 0 < r <= 16


def grad_geometry(n_out, k_in):
    """sed_lora_grad / lora_grad_kernel (csrc/lora.hip).  dB half: a wave per row, or, for k_in > 1024, a workgroup per row whose waves
    take kq = cdiv(cdiv(k_in, 4), 64) * 64 columns each; dA half: 32-row slabs x 256-column blocks.  Both halves share ONE grid.x, the
    larger of the two counts: the other half's surplus workgroups have nothing to do."""
    wide = k_in > 1024
    kq = cdiv(cdiv(k_in, 4), 64) * 64 if wide else k_in
    quarters = [(w * kq, max(w * kq, min(w * kq + kq, k_in))) for w in range(4)] if wide else [(0, k_in)]
    nb_a, nb_b = cdiv(n_out, 32) * cdiv(k_in, 256), (n_out if wide else cdiv(n_out, 4))
    grid = max(nb_a, nb_b)
    return GradGeometry(wide, kq, quarters, [cdiv(ke - kb, 512) for kb, ke in quarters], nb_a, nb_b, grid, grid - nb_a, grid - nb_b,
                        n_out % 32 != 0)


# ================================================================================================ sed_lora_merge
Merge = collections.namedtuple("Merge", "n_out k_in r s")
# 2049 x 4100: 2 100 225 float4 on 8192 x 256 threads, a second pass of the grid-stride loop
MERGE_CASES = [Merge(*c) for c in [(1, 4, 1, 1.0), (3, 4, 16, 0.125), (5, 12, 5, 1.0), (33, 12, 1, 0.125), (2, 12, 16, 1.0), (7, 768, 16, 1.0),
                                   (64, 768, 5, 0.125), (9, 768, 1, 1.0), (2049, 4100, 5, 0.125)]]
W_MAX = 100


def merge_budget(c):
    return check_budget(c.r, AMAX, AMAX, alpha=c.s, res_max=W_MAX, denom=denom_of(c.s))


def merge_inputs(c, seed=4000):
    s = seed + 7 * MERGE_CASES.index(c) if c in MERGE_CASES else seed
    return dict(W=nonzero_fill((c.n_out, c.k_in), s), A=int_operands(c.r, c.k_in, AMAX, s + 1), B=int_operands(c.n_out, c.r, AMAX, s + 2))


def merge_ref(c, i, fault=None):
    """W + s B A in float64 [n_out, k_in]."""
    A, B = i["A"].double(), i["B"].double()
    if fault == "rank_shift":
        B = _shift_cols(B)
    d = c.s * B @ A
    if fault == "last_row":
        d[c.n_out - 1] = 0
    if fault == "last_colgroup":
        d[:, c.k_in - 4:] = 0
    return i["W"].double() + d


def merge_args_ok(n_out, k_in, r):
    """Argument check of sed_lora_merge (csrc/lora.hip)."""
    return n_out > 0 and k_in > 0 and k_in % 4 == 0 and r > 0


def merge_launch(n_out, k_in):
    """sed_lora_merge: one thread per float4, at most 8192 workgroups of 256 (grid_for, csrc/common.h) -> (workgroups, passes)."""
    items = n_out * (k_in // 4)
    blocks = max(1, min(8192, cdiv(items, 256)))
    return blocks, cdiv(items, blocks * 256)


# ================================================================================================ the LoRA term of sed_weight_images
ImgDesc = collections.namedtuple("ImgDesc", "R C r f16 s")          # r = 0: a descriptor without the LoRA term
# Every launch mixes LoRA descriptors with one that has none; all three images (straight, transposed bf16, split) are asked of each.
IMAGE_LAUNCHES = [
    [ImgDesc(16, 64, 1, 0, 1.0), ImgDesc(80, 256, 0, 1, 1.0), ImgDesc(768, 64, 4, 1, 0.125)],
    [ImgDesc(80, 64, 8, 1, 1.0), ImgDesc(16, 256, 16, 0, 0.125), ImgDesc(16, 64, 0, 0, 1.0)],
    [ImgDesc(768, 256, 16, 0, 1.0), ImgDesc(80, 256, 1, 1, 0.125), ImgDesc(80, 64, 0, 1, 1.0), ImgDesc(16, 256, 4, 0, 1.0)],
    [ImgDesc(768, 64, 8, 0, 0.125), ImgDesc(80, 64, 0, 0, 1.0), ImgDesc(768, 256, 4, 1, 1.0), ImgDesc(80, 256, 8, 0, 1.0)]]


def image_id(launch):
    return "+".join(f"{d.R}x{d.C}r{d.r}{'h' if d.f16 else 'b'}" for d in launch)


def image_magnitudes(d):
    """(max |W|, max |A|, max |B|): integers with s = 1, multiples of 1/8 up to 8 in W and factors up to 2 with s = 1/8."""
    return (W_MAX, 3, 3) if d.s == 1.0 else (8, 2, 2)


def image_budget(d):
    """Raises unless every image element W + s B A is exact in bf16 (the transposed image is bf16 whatever the straight one is): at most
    256 units of 1 / denom.  Exact in bf16 is exact in IEEE half, so the split image's low third is zero."""
    wmax, amax, bmax = image_magnitudes(d)
    den = denom_of(d.s)
    tot = wmax + d.s * d.r * amax * bmax
    check_16bit(tot, BF16, den)
    return tot


def image_inputs(d, seed):
    wmax, amax, bmax = image_magnitudes(d)
    den = denom_of(d.s)
    i = dict(W=dyadic((d.R, d.C), wmax, den, seed))
    if d.r:
        i.update(A=nonzero_ints((d.r, d.C), amax, seed + 1), B=nonzero_ints((d.R, d.r), bmax, seed + 2))      # (no zeros: every row and rank counts)
    return i


def image_padded(d, i, seed):
    """The rank-2r descriptor with the same image: A' = [A; 0], B' = [B, arbitrary], same s."""
    _, _, bmax = image_magnitudes(d)
    return d._replace(r=2 * d.r), dict(W=i["W"], A=torch.cat([i["A"], torch.zeros_like(i["A"])]),
                                       B=torch.cat([i["B"], int_operands(d.R, d.r, bmax, seed + 3)], 1).contiguous())


def image_ref(d, i, fault=None):
    """W + s B A in float64 [R, C]."""
    if not d.r:
        return i["W"].double()
    return merge_ref(Merge(d.R, d.C, d.r, d.s), i, fault)


def image_expected(d, ref64):
    """-> (straight image in its type, transposed bf16 image, split image [hi | hi | lo] in IEEE half) of an exactly representable ref."""
    hi = ref64.to(F16)
    assert torch.equal(hi.double(), ref64) and torch.equal(ref64.to(BF16).double(), ref64)
    return ref64.to(dt16(d.f16)), ref64.t().contiguous().to(BF16), torch.cat([hi, hi, torch.zeros_like(hi)], 1)


def image_tiles(R, C):
    """One workgroup per 64 x 64 tile (weight_images_kernel, csrc/layout.hip)."""
    return cdiv(R, 64) * (C // 64)


# ================================================================================================ documented refusals
# (entry point, what is wrong) -> arguments the GPU test builds a call from; each fails the `*_args_ok` above
ROWPROJ_REFUSALS = [dict(K=96, ldx=96, r=8), dict(K=64, ldx=68, r=8), dict(K=128, ldx=64, r=8), dict(K=64, ldx=64, r=17),
                    dict(K=4864, ldx=4864, r=16), dict(K=9728, ldx=9728, r=8)]
COLREDUCE_REFUSALS = [dict(C=8, ldy=8, r=9), dict(C=6, ldy=8, r=8), dict(C=8, ldy=10, r=8)]
GRAD_REFUSALS = [dict(n_out=4, k_in=8, r=17)]
MERGE_REFUSALS = [dict(n_out=4, k_in=6, r=2)]
