"""Value sets, host references, shapes and restated launch arithmetic for the layout kernels of csrc/layout.hip, the family that
writes every GEMM operand: sed_cast_f32_bf16, sed_transpose_to_bf16, sed_f16_to_bf16_inplace, sed_split3_f16, sed_weight_residual_f16,
sed_weight_two_term_f8, sed_fp8_tail, sed_group_colmean(_ld), sed_weight_images (importable without a GPU: no test, no GPU code).
tests/test_image_cases_cpu.py proves on the CPU that the references are right and that every set and shape is what it is named for;
tests/test_gpu_image_kernels.py holds the hardware to them, bit for bit.

References.  Every conversion (f32 -> f16, f32 -> bf16, f16 -> bf16, bf16 -> f16, f32 -> OCP e4m3 after a clamp to +-448) exists twice:
(a) `*_bits`: integer arithmetic on the bit patterns in numpy (round to nearest even, the subnormal shift, the overflow to inf);
(b) `*_lib`: the library cast (numpy astype, torch-CPU .to()).  The derived images are the defining formula in IEEE fp32 on the host:
v - f32(f16(v)) is exact in fp32 whenever f16(v) is finite and the power-of-two scalings are exact, so each has ONE rounding and does
not depend on how -ffast-math contracts the expression.

Comparison rule (`compare`): bit patterns equal; a NaN matches any NaN; a zero matches a zero of either sign (counted).

The functions `flat_launch`, `*_args_ok`, `transpose_grid`, `colmean_visits` copy INTEGER FORMULAS of the entry points (the source line
is named at each), not kernels: they exist so that the CPU test can assert what a shape does to a launch."""
import collections
import functools
import itertools

import numpy as np
import torch

SENS = 10.0                 # a dropped or extra row has to move the reference by this many bounds (tests/walk_cases.py)
U16, U32, I64 = np.uint16, np.uint32, np.int64
SENT16, SENT8 = 0x7FFF, 0xFF          # prefill of 16-bit outputs (a NaN in both formats) and of bytes (an e4m3 NaN)
GUARD = 256                           # sentinel elements behind the end of every output


def cdiv(a, b):
    return -(-a // b)


# ================================================================================================ (a) conversions on the bit patterns
def _rne_shift(sig, shift):
    """sig >> shift, rounded to nearest, ties to even (int64 arrays; shift >= 1)."""
    shift = np.minimum(shift, 62)
    one = np.int64(1)
    q = sig >> shift
    rem = sig & ((one << shift) - 1)
    half = one << (shift - 1)
    return q + ((rem > half) | ((rem == half) & ((q & 1) == 1))).astype(I64)


def _narrow(u32, mbits, bias):
    """Magnitude code of fp32 bit patterns in a format of `mbits` mantissa bits and exponent bias `bias`, unsaturated (a carry out of the
    mantissa runs into the exponent, as it must); fp32 subnormals (< 2^-126, far below half the smallest subnormal of f16 and e4m3)
    give 0.  The caller treats NaN, inf and the top of the range."""
    u = np.asarray(u32, dtype=U32).astype(I64)
    e, m = (u >> 23) & 0xFF, u & 0x7FFFFF
    sig = np.where(e > 0, m | 0x800000, 0)
    he = e - 127 + bias                                        # biased exponent in the target; <= 0: subnormal there
    shift = (23 - mbits) + np.maximum(0, 1 - he)
    return (np.maximum(he - 1, 0) << mbits) + _rne_shift(sig, shift)


def _is_nan32(u32):
    return (np.asarray(u32, dtype=U32) & 0x7FFFFFFF) > 0x7F800000


def f32_to_f16_bits(u32):
    u32 = np.asarray(u32, dtype=U32)
    code = np.minimum(_narrow(u32, 10, 15), 0x7C00)            # past 65504 + half an ulp: inf (also inf itself)
    code = np.where(_is_nan32(u32), 0x7E00, code)
    return (((u32 >> 16) & 0x8000).astype(I64) | code).astype(U16)


def f32_to_bf16_bits(u32):
    u = np.asarray(u32, dtype=U32).astype(I64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16                    # carries into the exponent and, from 0x7F7F8000 on, to inf
    return np.where(_is_nan32(u32), ((u >> 16) & 0x8000) | 0x7FC0, r).astype(U16)


def f32_to_e4m3_bits(u32):
    """OCP e4m3 (bias 7, no inf, 0x7F = NaN, largest 448 = 0x7E) of clamp(v, -448, 448)."""
    u32 = np.asarray(u32, dtype=U32)
    mag = np.minimum(u32 & 0x7FFFFFFF, U32(0x43E00000))         # |v| > 448 -> 448 (bit patterns of non-negative floats are ordered)
    code = np.where(_is_nan32(u32), 0x7F, _narrow(mag, 3, 7))
    return (((u32 >> 24) & 0x80).astype(I64) | code).astype(np.uint8)


def f16_to_f32_bits(h):
    h = np.asarray(h, dtype=U16).astype(I64)
    s, e, m = (h & 0x8000) << 16, (h >> 10) & 31, h & 0x3FF
    p = sum((m >= (1 << i)).astype(I64) for i in range(1, 10))                      # floor(log2 m) of a subnormal's m (m > 0)
    sub = np.where(m == 0, 0, ((p - 24 + 127) << 23) | ((m << (23 - p)) & 0x7FFFFF))   # m 2^-24, normalised
    out = np.where(e == 0, sub, np.where(e == 31, 0x7F800000 | (m << 13), ((e + 112) << 23) | (m << 13)))
    return (s | out).astype(U32)


def bf16_to_f32_bits(b):
    return np.asarray(b, dtype=U16).astype(U32) << 16


def f16_to_bf16_bits(h):
    return f32_to_bf16_bits(f16_to_f32_bits(h))


def bf16_to_f16_bits(b):
    return f32_to_f16_bits(bf16_to_f32_bits(b))


# ================================================================================================ (b) the library casts
def _t32(u32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(u32, dtype=U32)).view(np.float32))


def _bits16(t):
    return t.contiguous().view(torch.int16).numpy().view(U16)


def f32_to_f16_lib(u32):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(u32, dtype=U32).view(np.float32).astype(np.float16).view(U16)


def f32_to_bf16_lib(u32):
    return _bits16(_t32(u32).to(torch.bfloat16))


def f32_to_e4m3_lib(u32):
    """(unclamped, torch's e4m3 cast returns NaN above 464: hence the clamp in front)"""
    return _t32(u32).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def f16_to_f32_lib(h):
    return np.ascontiguousarray(np.asarray(h, dtype=U16)).view(np.float16).astype(np.float32).view(U32)


def f16_to_bf16_lib(h):
    return _bits16(torch.from_numpy(np.ascontiguousarray(np.asarray(h, dtype=U16)).view(np.int16)).view(torch.float16).to(torch.bfloat16))


def bf16_to_f16_lib(b):
    return _bits16(torch.from_numpy(np.ascontiguousarray(np.asarray(b, dtype=U16)).view(np.int16)).view(torch.bfloat16).to(torch.float16))


CONVERSIONS = {                     # name: (form a, form b, output format)
    "f32->f16": (f32_to_f16_bits, f32_to_f16_lib, "f16"),
    "f32->bf16": (f32_to_bf16_bits, f32_to_bf16_lib, "bf16"),
    "f32->e4m3": (f32_to_e4m3_bits, f32_to_e4m3_lib, "e4m3"),
    "f16->bf16": (f16_to_bf16_bits, f16_to_bf16_lib, "bf16"),
    "bf16->f16": (bf16_to_f16_bits, bf16_to_f16_lib, "f16"),
    "f16->f32": (f16_to_f32_bits, f16_to_f32_lib, "f32"),
}


# ================================================================================================ the comparison rule
ABS = {"f16": 0x7FFF, "bf16": 0x7FFF, "e4m3": 0x7F, "f32": 0x7FFFFFFF}
INF = {"f16": 0x7C00, "bf16": 0x7F80, "f32": 0x7F800000}


def is_nan(bits, fmt):
    """bits: integer numpy array or torch tensor holding the patterns as non-negative integers."""
    mag = bits & ABS[fmt]
    return mag == 0x7F if fmt == "e4m3" else mag > INF[fmt]


def is_zero(bits, fmt):
    return (bits & ABS[fmt]) == 0


Verdict = collections.namedtuple("Verdict", "n nans zero_sign bad")


def compare(got, ref, fmt):
    """The rule: equal bits, or both NaN, or both zero.  got, ref: equally shaped integer arrays (numpy or torch, any device) of
    non-negative patterns -> Verdict(elements, NaNs in ref, zeros whose sign differed, mismatching elements)."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    eq = got == ref
    both_nan = is_nan(got, fmt) & is_nan(ref, fmt)
    both_zero = is_zero(got, fmt) & is_zero(ref, fmt)
    ok = eq | both_nan | both_zero
    n = int(np.prod(got.shape))
    return Verdict(n, int(is_nan(ref, fmt).sum()), int((both_zero & ~eq).sum()), n - int(ok.sum()))


# ================================================================================================ derived references (IEEE fp32 on the host)
def _f32(u32):
    return np.asarray(u32, dtype=U32).view(np.float32)


def _widen(conv):
    """The exact f16 -> f32 of the same form as `conv` (the library forms are the quick ones: the loop cases use them)."""
    return f16_to_f32_lib if conv is f32_to_f16_lib else f16_to_f32_bits


def hi_lo_f16(u32, conv=f32_to_f16_bits):
    """-> (hi, lo) f16 bit patterns: hi = f16(v), lo = f16(v - f32(f16(v)))."""
    hi = conv(u32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = _f32(u32) - _f32(_widen(conv)(hi))
    return hi, conv(d.view(U32))


def residual_f16(u32, scale, conv=f32_to_f16_bits):
    """f16(scale (v - f32(f16(v)))), scale a power of two."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.float32(scale) * (_f32(u32) - _f32(_widen(conv)(conv(u32))))
    return conv(d.view(U32))


def lo_e4m3(u32, s, conv16=f32_to_f16_bits, conv8=f32_to_e4m3_bits):
    """e4m3(clamp(2^s (v - f32(f16(v)))))."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.float32(2.0 ** s) * (_f32(u32) - _f32(_widen(conv16)(conv16(u32))))
    return conv8(d.view(U32))


def act_e4m3(h, conv8=f32_to_e4m3_bits):
    """e4m3(clamp(0.25 f32(h))) of f16 bit patterns: the activation image of sed_fp8_tail."""
    widen = f16_to_f32_lib if conv8 is f32_to_e4m3_lib else f16_to_f32_bits
    with np.errstate(invalid="ignore"):
        return conv8((np.float32(0.25) * _f32(widen(h))).view(U32))


# ================================================================================================ value sets
ALL_F16 = np.arange(65536, dtype=np.uint32).astype(U16)
ALL_BF16 = ALL_F16.copy()


def _bits_of(f64):
    f32 = np.asarray(f64, dtype=np.float64).astype(np.float32)
    assert np.array_equal(f32.astype(np.float64), f64)          # every member is an fp32 number as it stands
    return f32.view(U32)


@functools.lru_cache(maxsize=None)
def edge32_f16_core():
    """For every adjacent pair (a, b) of non-negative f16 values, (65504, 2^16: the overflow) included -> uint32 [31744, 4]:
    a, midpoint - 1 fp32 ulp, midpoint, midpoint + 1 fp32 ulp (positive)."""
    codes = np.arange(0x7C00, dtype=np.uint32).astype(U16)
    a = f16_to_f32_bits(codes).view(np.float32).astype(np.float64)
    b = np.append(a[1:], 65536.0)
    mid = _bits_of((a + b) / 2)
    return np.stack([_bits_of(a), mid - 1, mid, mid + 1], 1).astype(U32)


@functools.lru_cache(maxsize=None)
def edge32_bf16_core():
    """The same for bf16 (pairs up to (0x7F7F, 2^128)): the midpoint of bf16 patterns k, k + 1 is the fp32 pattern (k << 16) + 0x8000;
    the last one, 0x7F7F8000, ties to inf."""
    a = np.arange(0x7F80, dtype=np.uint32) << 16
    mid = a + 0x8000
    return np.stack([a, mid - 1, mid, mid + 1], 1).astype(U32)


EXTRAS32 = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000,               # +-0, +-inf, a NaN
                     0x00000001, 0x80000001, 0x00400000, 0x007FFFFF, 0x807FFFFF,               # fp32 subnormals
                     0x33000000, 0x33000001, 0xB3000000, 0xB3000001], dtype=U32)               # 2^-25 (ties to 0) and its successor


def _both_signs(core):
    flat = core.reshape(-1)
    return np.concatenate([flat, flat | U32(0x80000000), EXTRAS32])


EDGE32_F16 = _both_signs(edge32_f16_core())
EDGE32_BF16 = _both_signs(edge32_bf16_core())
EDGE32_ALL = np.concatenate([EDGE32_F16, EDGE32_BF16])


def padded(bits, multiple, fill=0x3F800000):
    """bits, followed by `fill` (1.0f) up to a multiple of `multiple`."""
    bits = np.asarray(bits)
    return np.concatenate([bits, np.full((-len(bits)) % multiple, fill, dtype=bits.dtype)])


# ------------------------------------------------------------------------------------------------ e4m3 boundaries of the lo byte
E4M3_VALUES = np.array([(c & 7) * 2.0 ** -9 if c < 8 else (8 + (c & 7)) * 2.0 ** ((c >> 3) - 10) for c in range(0x7F)])   # codes 0 .. 0x7E
E4M3_BOUNDARIES = (E4M3_VALUES[:-1] + E4M3_VALUES[1:]) / 2              # 126 midpoints; [c] lies between codes c and c + 1
LO_H_EXP = -5
LO_H = 1.5 * 2.0 ** LO_H_EXP          # 0.046875: an even f16 significand (0x200) off a power of two, so that H + d has H's fp32 ulp
LO_ULP32 = 2.0 ** (LO_H_EXP - 23)     # ... for every |d| < half an f16 ulp of H = 2^12 fp32 ulps
LO_JMAX = 2047                        # |d| <= 2047 fp32 ulps: f16(H + d) == H without calling on the tie
LoCase = collections.namedtuple("LoCase", "s w_bits target code kind")      # target = 2^s d (float64); kind: -1 below, 0 on, +1 above, 2 clamp
LO_CLAMP_J = (448, 449, 464, 465, 480, 481, 1000, LO_JMAX)                  # 2^s d at a step of 1.0: 448 itself, and beyond it


def _lo_step(boundary):
    """The step q = 2^(s + LO_H_EXP - 23) of a band: 1/64 of the boundary's lowest set bit (boundary = odd x 2^g, odd <= 31, so that
    boundary / q <= 1984 and one step either side stay inside LO_JMAX)."""
    m, e = np.frexp(boundary)
    g = int(e)
    while m != np.floor(m):
        m, g = m * 2, g - 1
    return g - 6


@functools.lru_cache(maxsize=None)
def edge_e4m3_lo():
    """-> list of LoCase: w = sw (H + sd j ulp32(H)) for both signs sw of the weight and sd of the residual, with 2^s j ulp32(H) on every
    e4m3 boundary, one step below and one above; then the clamp values.  One (H, s) cannot span the range (half an f16 ulp of H is 2^12
    fp32 ulps, e4m3 spans 2^-10 .. 448): one band per power of two of the step."""
    out = []
    for sw, sd in itertools.product((1.0, -1.0), repeat=2):
        cases = [(c, b, _lo_step(b), k) for c, b in enumerate(E4M3_BOUNDARIES) for k in (-1, 0, 1)]
        cases += [(0x7E, float(j), 0, 2) for j in LO_CLAMP_J]
        for c, b, qe, k in cases:
            q = 2.0 ** qe
            j = (b / q) + (k if k != 2 else 0)
            assert j == int(j) and 0 < j <= LO_JMAX, (b, q, j)
            w = sw * (LO_H + sd * j * LO_ULP32)
            s = qe - LO_H_EXP + 23
            code = 0x7E if k == 2 else (c + 1 if k == 1 else c if k == -1 else (c if c % 2 == 0 else c + 1))
            out.append(LoCase(s, int(_bits_of(np.array([w]))[0]), sw * sd * j * q, code | (0x80 if sw * sd < 0 else 0), k))
    return out


def lo_bands():
    """{s: uint32 weights of that band, padded with H (lo = 0) to a multiple of 8}."""
    bands = collections.defaultdict(list)
    for c in edge_e4m3_lo():
        bands[c.s].append(c.w_bits)
    hbits = int(_bits_of(np.array([LO_H]))[0])
    return {s: padded(np.array(v, dtype=U32), 8, hbits) for s, v in sorted(bands.items())}


# ================================================================================================ flat grid-stride launches
FlatLaunch = collections.namedtuple("FlatLaunch", "items blocks per_pass passes")


def flat_launch(items, cap, threads=256):
    """blocks = min(cdiv(items, 256), cap), every thread strides by blocks x 256 -> (items, workgroups, items per pass, passes)."""
    blocks = max(1, min(cap, cdiv(items, threads)))
    return FlatLaunch(items, blocks, blocks * threads, cdiv(items, blocks * threads))


CAP_4096, CAP_8192 = 4096, 8192
LoopCase = collections.namedtuple("LoopCase", "kernel shape launch note")
N_CAST = 4 * (2 * 2 ** 20 + 257)
N_INPLACE = 8 * (2 * 2 ** 20 + 257)
SPLIT_M, SPLIT_K = 2731, 1538
TAIL_SHAPES = [(5463, 3072, 4616), (10925, 3072, 4616)]            # (M, K, ld)
TWO_TERM_SHAPES = [(2731, 3080), (5462, 3080)]                      # (N, K)


def cast_launch(n):
    """sed_cast_f32_bf16 and sed_weight_residual_f16 (csrc/layout.hip): one thread per float4."""
    return flat_launch(n // 4, CAP_4096)


def inplace_launch(n):
    """sed_f16_to_bf16_inplace (csrc/layout.hip): one thread per 8 halves."""
    return flat_launch(n // 8, CAP_4096)


def split3_launch(M, K):
    """sed_split3_f16 (csrc/layout.hip): one thread per pair of columns."""
    return flat_launch(M * (K // 2), CAP_4096)


def tail_launch(M, K):
    """sed_fp8_tail (csrc/layout.hip): one thread per 8 columns."""
    return flat_launch(M * (K // 8), CAP_8192)


def two_term_launch(N, K):
    """sed_weight_two_term_f8 (csrc/layout.hip): one thread per 4 columns."""
    return flat_launch(N * (K // 4), CAP_8192)


def loop_cases():
    """Every loop case.  The first shape of sed_fp8_tail and of sed_weight_two_term_f8 makes TWO passes of their 8192-workgroup grid
    (2 x 2^20 + a tail items against 2^21 per pass); the second shape of each is the smallest that makes three."""
    cs = [LoopCase("cast", (N_CAST,), cast_launch(N_CAST), ""), LoopCase("residual", (N_CAST,), cast_launch(N_CAST), ""),
          LoopCase("inplace", (N_INPLACE,), inplace_launch(N_INPLACE), ""),
          LoopCase("split3", (SPLIT_M, SPLIT_K), split3_launch(SPLIT_M, SPLIT_K), "K = 2 mod 4")]
    cs += [LoopCase("fp8_tail", s, tail_launch(s[0], s[1]), "pitch with a gap") for s in TAIL_SHAPES]
    cs += [LoopCase("two_term_f8", s, two_term_launch(*s), "") for s in TWO_TERM_SHAPES]
    return cs


def cast_args_ok(n):
    """Argument checks of csrc/layout.hip: sed_cast_f32_bf16 (n == 0 launches one idle workgroup) and sed_weight_residual_f16 (n > 0)."""
    return n > 0 and n % 4 == 0


def inplace_args_ok(n):
    """Argument check of sed_f16_to_bf16_inplace (csrc/layout.hip)."""
    return n % 8 == 0


def split3_args_ok(M, K, mode):
    """Argument check of sed_split3_f16 (csrc/layout.hip)."""
    return K % 2 == 0 and M > 0 and 0 <= mode <= 2


def tail_args_ok(M, K, ld):
    """Argument check of sed_fp8_tail (csrc/layout.hip)."""
    return M > 0 and K % 8 == 0 and ld % 8 == 0 and ld >= K + K // 2


def two_term_args_ok(N, K, s):
    """Argument check of sed_weight_two_term_f8 (csrc/layout.hip)."""
    return N > 0 and K % 8 == 0 and -100 <= s <= 100


# ================================================================================================ transpose
KINDS = {"bf16": 0, "f32": 1, "f16": 2}                            # operand-kind codes of the C ABI
TRANSPOSE_RPAD = [(1, 16), (100, 112), (130, 144), (2380, 2432)]
TRANSPOSE_C = (64, 192)


def transpose_cases():
    """(R, Rpad, C, ldin, input kind) for every combination of the issue's lists."""
    return [(R, Rpad, C, C + g, k) for (R, Rpad) in TRANSPOSE_RPAD for C in TRANSPOSE_C for g in (0, 8) for k in ("bf16", "f32", "f16")]


def transpose_args_ok(R, Rpad, C, ldin, in_kind):
    """Argument check of sed_transpose_to_bf16 (csrc/layout.hip)."""
    return not (Rpad < R or in_kind < 0 or in_kind > 2 or C % 64 or Rpad % 16 or ldin % 8)


def transpose_grid(Rpad, C):
    """Grid of sed_transpose_to_bf16 (csrc/layout.hip) -> (tiles along C, tiles along R); each workgroup writes up to four 16-row segments
    of outT, the ones with r0 + seg < Rpad (transpose_kernel)."""
    return cdiv(C, 64), cdiv(Rpad, 64)


def transpose_segments(R, Rpad):
    """-> (16-row segments of the last row tile that are written, of those the ones that lie wholly past R: zeros only)."""
    r0 = (cdiv(Rpad, 64) - 1) * 64
    segs = [s for s in (0, 16, 32, 48) if r0 + s < Rpad]
    return segs, [s for s in segs if r0 + s >= R]


def transpose_input(R, C, ldin, seed=0):
    """Small integers in [-64, 64] (exact in bf16 and f16; a column of 2380 of them sums exactly in fp32) -> float32 [R, ldin]; the
    pitch gap holds 77, which must reach no output."""
    g = torch.Generator().manual_seed(7000 + 13 * R + C + ldin + seed)
    x = torch.full((R, ldin), 77.0)
    x[:, :C] = torch.randint(-64, 65, (R, C), generator=g).float()
    return x


# ================================================================================================ group colmean
COLMEAN_ROWS, COLMEAN_STEPS, COLMEAN_K, COLMEAN_GROUPS = (1, 7, 63, 64, 65, 602), (1, 3, 8), (256, 768), 3
UNVISITED = 1000.0                                                  # (exact in bf16 and f16)
SIG_BITS = {"bf16": 8, "f16": 11}


def colmean_cases():
    """(rows, step, K, ld)."""
    return [(r, s, K, ld) for r in COLMEAN_ROWS for s in COLMEAN_STEPS for K in COLMEAN_K for ld in (K, K + K // 2)]


def colmean_args_ok(groups, rows, K, ld, step):
    """Argument check of sed_group_colmean_ld (csrc/layout.hip)."""
    return not (groups <= 0 or rows <= 0 or K % 256 or step < 1 or ld < K or ld % 8)


def colmean_visits(rows, step):
    """group_colmean_kernel (csrc/layout.hip): slice sl of 8 starts at row sl x step and strides by 8 x step -> the rows read, and nvis."""
    vis = sorted(r for sl in range(8) for r in range(sl * step, rows, 8 * step))
    assert vis == list(range(0, rows, step))
    return vis, cdiv(rows, step)


def colmean_exact_input(rows, step, K, ld, storage, groups=COLMEAN_GROUPS):
    """[groups * rows, ld] in the storage dtype: multiples of 2^-6 in [-4, 4] (rounded once to the storage format, which keeps them
    multiples of 2^-6 in [-4, 4]) on the visited rows, 1000 on every other row and in the pitch gap."""
    dt = torch.bfloat16 if storage == "bf16" else torch.float16
    g = torch.Generator().manual_seed(9000 + 31 * rows + 7 * step + K + ld)
    x = torch.full((groups, rows, ld), UNVISITED)
    vis, _ = colmean_visits(rows, step)
    x[:, vis, :K] = (torch.randint(-256, 257, (groups, len(vis), K), generator=g).float() / 64.0).to(dt).float()
    return x.reshape(groups * rows, ld).to(dt)


def colmean_half_ulp(ref64, storage):
    """Half a unit in the last place of the storage format at |ref| (f16 subnormals: 2^-25), as walk_cases.half_ulp."""
    _, e = torch.frexp(ref64.abs().clamp_min(1e-300))
    h = torch.ldexp(torch.ones_like(ref64), e - 1 - SIG_BITS[storage])
    return h.clamp_min(2.0 ** -25) if storage == "f16" else h


def colmean_exact_ref(x, rows, step, K, storage, groups=COLMEAN_GROUPS):
    """-> (mean of the visited rows in float64 [groups, K], per-element bound).  The sums are exact in fp32 (<= 602 multiples of 2^-6 of
    magnitude <= 4: below 2^24 units), so the kernel's error is what it does with sum / nvis: -ffast-math may make that a reciprocal
    (<= 1 fp32 ulp off after its refinement, or 2.5 without) and a multiply (half an ulp): <= 4 fp32 ulps of |ref| = 4 x 2^-23 |ref|,
    then one rounding to the storage format: half an ulp of it."""
    vis, nvis = colmean_visits(rows, step)
    xs = x.double().view(groups, rows, -1)[:, vis, :K]
    ref = xs.sum(1) / nvis
    return ref, colmean_half_ulp(ref, storage) + 4 * 2.0 ** -23 * ref.abs()


def colmean_sensitivity(x, rows, step, K, storage, groups=COLMEAN_GROUPS):
    """{what went wrong: bounds the float64 mean moves by, at the column where it moves most}: the last visited row dropped from the
    sum (nvis > 1), one unvisited row (1000) added to it (step > 1 and rows > 1), the divisor taken as rows // step where that differs."""
    vis, nvis = colmean_visits(rows, step)
    ref, bound = colmean_exact_ref(x, rows, step, K, storage, groups)
    xs = x.double().view(groups, rows, -1)[:, :, :K]
    out = {}
    if nvis > 1:
        out["last visited row dropped"] = float(((xs[:, vis[-1]] / nvis).abs() / bound).max())
    if len(vis) < rows:
        out["an unvisited row added"] = float(((torch.full_like(ref, UNVISITED) / nvis) / bound).max())
    if rows // step != nvis:
        wrong = ref * nvis / (rows // step) if rows // step else torch.full_like(ref, float("inf"))
        out["nvis = rows / step"] = float(((wrong - ref).abs() / bound).max())
    return out


def colmean_gauss_input(K, ld, storage, rows=602, groups=COLMEAN_GROUPS):
    dt = torch.bfloat16 if storage == "bf16" else torch.float16
    g = torch.Generator().manual_seed(9500 + K + ld)
    return torch.randn(groups * rows, ld, generator=g).mul_(1.5).to(dt)


# ================================================================================================ weight images
WIMG_R, WIMG_C = (64, 80, 208), 128


def wimg_tiles(R, C):
    """One workgroup per 64 x 64 tile (weight_images_kernel, csrc/layout.hip; the engine's descriptor table counts them the same way)."""
    return cdiv(R, 64) * (C // 64)


def wimg_master(R, C, i):
    """fp32 bit patterns [R, C] taken from EDGE32_F16 at a stride that walks the whole set (subnormal, normal and overflow edges)."""
    n = R * C
    idx = (np.arange(n, dtype=np.int64) * 31 + 1009 * i) % len(EDGE32_F16)
    return EDGE32_F16[idx].reshape(R, C)


# ================================================================================================ loop-case inputs
def random_f32_bits(n, exp_lo, exp_hi, seed):
    """n random fp32 bit patterns, finite: random sign and mantissa, the exponent field uniform in [exp_lo, exp_hi] (1 .. 254).
    Every element depends on its position."""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    e = rng.integers(exp_lo, exp_hi + 1, n, dtype=np.uint64)
    return ((r & 0x807FFFFF) | (e << 23)).astype(U32)


def random_f16_bits(n, seed):
    """n random 16-bit patterns with the non-finite ones (exponent field 31) moved to exponent field 30."""
    h = np.random.default_rng(seed).integers(0, 1 << 16, n, dtype=np.uint32).astype(U16)
    return np.where((h & 0x7C00) == 0x7C00, h & U16(0xFBFF), h).astype(U16)
