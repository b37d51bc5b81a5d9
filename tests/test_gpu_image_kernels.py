"""The cast, transpose and operand-image kernels of csrc/layout.hip, bit for bit (need an MI355X): sed_cast_f32_bf16,
sed_transpose_to_bf16, sed_f16_to_bf16_inplace, sed_split3_f16, sed_weight_residual_f16, sed_weight_two_term_f8, sed_fp8_tail,
sed_group_colmean(_ld), sed_weight_images.  Value sets, host references, shapes and the restated launch arithmetic: tests/image_cases.py,
proved on the CPU by tests/test_image_cases_cpu.py.

Every output buffer holds a sentinel before the call (0x7FFF in 16-bit outputs, 0xFF in bytes), with a guard region behind its end and
in every pitch gap, which must be untouched afterwards.  Every element is compared under the rule of image_cases.compare: equal bit
patterns; a NaN matches any NaN; a zero matches a zero of either sign.  One line per case goes to image_kernel_bits.log under
SED_TEST_LOG_DIR, else test_logs/: elements compared, NaNs among them, zeros whose sign differed."""
import itertools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import image_cases as IC  # noqa: E402
import walk_cases as X  # noqa: E402
from image_cases import GUARD, SENT16, SENT8, U16, U32  # noqa: E402
from transformer4sed_amd._lib import SedHipError  # noqa: E402
from transformer4sed_amd.ops import call, BF16, F16  # noqa: E402

DEV = "cuda"
LOGDIR = os.environ.get("SED_TEST_LOG_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_logs")
LOG = os.path.join(LOGDIR, "image_kernel_bits.log")
DT = {"bf16": BF16, "f16": F16, "f32": torch.float32}
TO16 = {"f16": IC.f32_to_f16_bits, "bf16": IC.f32_to_bf16_bits}
TO16_LIB = {"f16": IC.f32_to_f16_lib, "bf16": IC.f32_to_bf16_lib}


def log(line):
    os.makedirs(LOGDIR, exist_ok=True)
    with open(LOG, "a") as f:
        f.write(line + "\n")
    print(line)


# ------------------------------------------------------------------------------------------------ buffers and the comparison
def dev_f32(bits):
    """uint32 patterns -> fp32 tensor on the device."""
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=U32).view(np.int32)).to(DEV).view(torch.float32)


def dev_16(bits):
    """uint16 patterns -> int16 tensor on the device (the kernels take pointers: the dtype of the holder does not matter)."""
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=U16).view(np.int16)).to(DEV)


def out16(n):
    """n 16-bit outputs and the guard behind them, all 0x7FFF."""
    return torch.full((n + GUARD,), SENT16, dtype=torch.int16, device=DEV)


def out8(n):
    return torch.full((n + GUARD,), SENT8, dtype=torch.uint8, device=DEV)


def pat(t):
    """int16 / uint8 holder -> the patterns as non-negative int32."""
    return t.to(torch.int32) & (0xFFFF if t.dtype == torch.int16 else 0xFF)


def untouched(buf, n):
    return bool((buf[n:] == (SENT16 if buf.dtype == torch.int16 else SENT8)).all())


def check(name, got, ref, fmt, keep=None):
    """got: device holder (int16 / uint8) of any shape; ref: numpy patterns of that shape; keep: numpy bool mask of the elements held
    to the rule (None: all).  Logs the counts, asserts that no element misses."""
    g, r = pat(got), torch.from_numpy(np.ascontiguousarray(ref).astype(np.int32)).to(DEV)
    assert g.shape == r.shape, (name, g.shape, r.shape)
    if keep is not None:
        k = torch.from_numpy(np.ascontiguousarray(keep)).to(DEV)
        g, r = g[k], r[k]
    v = IC.compare(g, r, fmt)
    log(f"{name}: compared={v.n} nans={v.nans} zero_sign_differs={v.zero_sign} mismatches={v.bad}")
    if v.bad:
        ok = (g == r) | (IC.is_nan(g, fmt) & IC.is_nan(r, fmt)) | (IC.is_zero(g, fmt) & IC.is_zero(r, fmt))
        at = (~ok).reshape(-1).nonzero().reshape(-1)[:8]
        raise AssertionError((name, v, [(int(i), hex(int(g.reshape(-1)[i])), hex(int(r.reshape(-1)[i]))) for i in at]))
    return v


# ================================================================================================ 1. values: casts
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_cast_on_every_rounding_boundary(kind):
    """sed_cast_f32_bf16 on EDGE32_F16 u EDGE32_BF16: every tie, one fp32 ulp either side, subnormals, the overflow edge, +-0, inf, NaN."""
    bits = IC.padded(IC.EDGE32_ALL, 4)
    n = len(bits)
    out = out16(n)
    call("sed_cast_f32_bf16", dev_f32(bits), out, n, int(kind == "f16"))
    check(f"cast f32->{kind} edges", out[:n], TO16[kind](bits), kind)
    assert untouched(out, n)


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_transpose_f32_in_on_every_rounding_boundary(kind):
    """sed_transpose_to_bf16, f32 in -> outT and outS of one kind, on both edge sets as an [R, 64] matrix (R = 8049, Rpad = 8064)."""
    bits = IC.padded(IC.EDGE32_ALL, 64).reshape(-1, 64)
    R, C = bits.shape
    Rpad = IC.cdiv(R, 16) * 16
    outT, outS = out16(C * Rpad), out16(R * C)
    call("sed_transpose_to_bf16", dev_f32(bits), 1, R, C, C, outT, Rpad, IC.KINDS[kind], outS, IC.KINDS[kind], None)
    ref = TO16[kind](bits.reshape(-1)).reshape(R, C)
    refT = np.zeros((C, Rpad), dtype=U16)
    refT[:, :R] = ref.T
    check(f"transpose f32->{kind} edges outS", outS[:R * C].view(R, C), ref, kind)
    check(f"transpose f32->{kind} edges outT", outT[:C * Rpad].view(C, Rpad), refT, kind)
    assert untouched(outT, C * Rpad) and untouched(outS, R * C)


@pytest.mark.parametrize("ikind,okind", [("f16", "f16"), ("f16", "bf16"), ("bf16", "bf16"), ("bf16", "f16")])
def test_transpose_16bit_in_on_all_patterns(ikind, okind):
    """All 65 536 patterns of the input kind as [1024, 64]: the same kind out is the identity on every non-NaN pattern."""
    bits = IC.ALL_F16.reshape(1024, 64)
    R, C = bits.shape
    outT, outS = out16(C * R), out16(R * C)
    call("sed_transpose_to_bf16", dev_16(bits), IC.KINDS[ikind], R, C, C, outT, R, IC.KINDS[okind], outS, IC.KINDS[okind], None)
    if ikind == okind:
        ref = bits
    else:
        ref = (IC.f16_to_bf16_bits if ikind == "f16" else IC.bf16_to_f16_bits)(bits.reshape(-1)).reshape(R, C)
    v = check(f"transpose {ikind}->{okind} all patterns outS", outS[:R * C].view(R, C), ref, okind)
    assert v.n == 65536 and v.nans == (2046 if ikind == "f16" else 254)
    check(f"transpose {ikind}->{okind} all patterns outT", outT[:C * R].view(C, R), np.ascontiguousarray(ref.T), okind)
    assert untouched(outT, C * R) and untouched(outS, R * C)


def test_f16_to_bf16_inplace_on_all_patterns():
    buf = out16(65536)
    buf[:65536] = dev_16(IC.ALL_F16)
    call("sed_f16_to_bf16_inplace", buf, 65536)
    check("f16->bf16 in place, all patterns", buf[:65536], IC.f16_to_bf16_bits(IC.ALL_F16), "bf16")
    assert untouched(buf, 65536)


# ================================================================================================ 2. values: hi / lo images
def split_blocks(mode, hi, lo):
    return {0: (hi, lo, hi), 1: (hi, hi, lo), 2: (hi, lo)}[mode]


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_split3_on_every_f16_boundary(mode):
    """sed_split3_f16 on EDGE32_F16 as [M, 64]: |v| >= 65520 gives hi = +-inf, lo = -+inf; v = +-inf gives a NaN lo.  The column blocks are
    held one by one: [hi | lo | hi] (0), [hi | hi | lo] (1), [hi | lo] (2) -- a swapped placement fails (hi != lo wherever lo != 0)."""
    bits = IC.padded(IC.EDGE32_F16, 64).reshape(-1, 64)
    M, K = bits.shape
    nb = 2 if mode == 2 else 3
    out = out16(M * nb * K)
    call("sed_split3_f16", dev_f32(bits), out, M, K, mode)
    hi, lo = (a.reshape(M, K) for a in IC.hi_lo_f16(bits.reshape(-1)))
    assert int(((hi != lo) & ((lo & 0x7FFF) != 0)).sum()) > 100000         # the blocks can be told apart
    got = out[:M * nb * K].view(M, nb, K)
    for b, (nm, ref) in enumerate(zip("hi lo hi".split() if mode == 0 else "hi hi lo".split() if mode == 1 else "hi lo".split(),
                                      split_blocks(mode, hi, lo))):
        check(f"split3 mode {mode} block {b} ({nm}) edges", got[:, b], ref, "f16")
    big = np.abs(bits.view(np.float32)) >= 65520.0
    assert big.sum() >= 6 and np.all((hi[big] & 0x7FFF) == 0x7C00)
    assert untouched(out, M * nb * K)


def test_weight_residual_on_every_f16_boundary():
    """sed_weight_residual_f16 at the engine's scale 2^11 on EDGE32_F16."""
    bits = IC.padded(IC.EDGE32_F16, 4)
    n = len(bits)
    out = out16(n)
    call("sed_weight_residual_f16", dev_f32(bits), out, n, 2048.0)
    check("weight residual x2048 edges", out[:n], IC.residual_f16(bits, 2048.0), "f16")
    assert untouched(out, n)


def two_term(bits2d, s):
    """-> (hi holder [N, K] int16, lo holder [N, K] uint8, whole output holder)."""
    N, K = bits2d.shape
    out = out8(N * 3 * K)
    call("sed_weight_two_term_f8", dev_f32(bits2d), out, N, K, s)
    rows = out[:N * 3 * K].view(N, 3 * K)
    return rows[:, :2 * K].contiguous().view(torch.int16), rows[:, 2 * K:], out


def test_two_term_f8_hi_half_and_lo_byte_on_every_f16_boundary():
    """The hi half on EDGE32_F16 where the input and f16(w) are finite; the lo byte there too (s = 16), without the non-finite inputs and
    |w| >= 65520: what the kernel's fmed3 clamp makes of a NaN is not defined by the project."""
    bits = IC.padded(IC.EDGE32_F16, 64).reshape(-1, 64)
    N, K = bits.shape
    hi_g, lo_g, out = two_term(bits, 16)
    v = bits.view(np.float32)
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(v) & (np.abs(v) < 65520.0)
    assert keep.sum() > 250000 and (~keep).sum() >= 7
    check("two-term f8 hi half edges", hi_g, IC.f32_to_f16_bits(bits.reshape(-1)).reshape(N, K), "f16", keep)
    check("two-term f8 lo byte edges s=16", lo_g, IC.lo_e4m3(bits.reshape(-1), 16).reshape(N, K), "e4m3", keep)
    assert untouched(out, N * 3 * K)


def test_two_term_f8_lo_byte_on_every_e4m3_boundary():
    """EDGE_E4M3_LO, one launch per band: 2^s (w - f16(w)) on every finite e4m3 boundary of both signs, one step either side, and past
    +-448."""
    cases, bands = IC.edge_e4m3_lo(), IC.lo_bands()
    want = {}
    for c in cases:
        want.setdefault(c.s, []).append(c.code)
    hbits = int(IC.f32_to_f16_bits(IC._bits_of(np.array([IC.LO_H])))[0])
    total = 0
    for s, w in bands.items():
        hi_g, lo_g, out = two_term(w.reshape(1, -1), s)
        ref = IC.lo_e4m3(w, s)
        assert ref[:len(want[s])].tolist() == want[s]                     # the reference gives the codes the set was built for
        check(f"two-term f8 lo byte, band s={s}", lo_g, ref.reshape(1, -1), "e4m3")
        assert bool(((pat(hi_g) & 0x7FFF) == hbits).all())
        assert untouched(out, 3 * len(w))
        total += len(want[s])
    assert total == len(cases) == 4 * (126 * 3 + len(IC.LO_CLAMP_J))


def test_fp8_tail_on_all_f16_patterns():
    """All 65 536 f16 patterns as 64 x 1024 (pitch 1544: a gap of 8 halfs): the e4m3 half is e4m3(clamp(x / 4)), +-448 beyond +-1792.
    The 2046 NaN patterns are left out of the e4m3 assertion only (the clamp of a NaN is not defined by the project; what they map
    to is logged); their f16 half, like everyone's, is unchanged and every other byte of their rows is right."""
    M, K, ld = 64, 1024, 1544
    buf = out8(M * ld * 2)
    rows = buf[:M * ld * 2].view(M, 2 * ld)
    rows[:, :2 * K] = dev_16(IC.ALL_F16.reshape(M, K)).view(torch.uint8)
    call("sed_fp8_tail", buf, M, K, ld)
    ref = IC.act_e4m3(IC.ALL_F16).reshape(M, K)
    nan_in = IC.is_nan(IC.ALL_F16.astype(np.int64), "f16").reshape(M, K)
    assert nan_in.sum() == 2046 and nan_in.any(1).sum() == 2              # (the NaNs sit at the end of two rows)
    assert torch.equal(rows[:, :2 * K].contiguous().view(torch.int16), dev_16(IC.ALL_F16.reshape(M, K)))
    check("fp8 tail all f16 patterns", rows[:, 2 * K:3 * K], ref, "e4m3", ~nan_in)
    assert bool((rows[:, 3 * K:] == SENT8).all()) and untouched(buf, M * ld * 2)
    h = IC.f16_to_f32_bits(IC.ALL_F16).view(np.float32).reshape(M, K)
    with np.errstate(invalid="ignore"):
        big = np.abs(h) >= 1792.0
    got = rows[:, 2 * K:3 * K].cpu().numpy()
    assert big.sum() == 2 * (0x7C00 - 0x6700 + 1) and np.array_equal(got[big], np.where(h[big] > 0, 0x7E, 0xFE))
    codes, counts = np.unique(got[nan_in], return_counts=True)
    log("fp8 tail NaN inputs (not asserted) map to " + ", ".join(f"0x{c:02X} x{n}" for c, n in zip(codes, counts)))


# ================================================================================================ 3. values: every image in one launch
def test_weight_images_three_descriptors_on_f16_boundaries():
    """One launch, three descriptors (plain; gather plan + scale plan; with the split image outP), R = 64, 80, 208, C = 128, masters from
    EDGE32_F16: outS (bf16, f16, f16), outT (bf16) and outP = [hi | hi | lo] equal what sed_cast_f32_bf16, sed_transpose_to_bf16 and
    sed_split3_f16 mode 1 are held to above."""
    C = IC.WIMG_C
    masters = [IC.wimg_master(R, C, i) for i, R in enumerate(IC.WIMG_R)]
    rng = np.random.default_rng(5)
    R1 = IC.WIMG_R[1]
    plan = rng.integers(0, R1 * C, (R1, C), dtype=np.int64).astype(np.int32)
    scale = rng.choice(np.array([1.0, 2.0, 0.0], dtype=np.float32), (R1, C))
    with np.errstate(invalid="ignore", over="ignore"):
        img1 = (masters[1].reshape(-1).view(np.float32)[plan] * scale).view(U32)
    images = [masters[0], img1, masters[2]]
    skinds = ["bf16", "f16", "f16"]
    d_in = [dev_f32(m) for m in masters]
    d_plan, d_scale = torch.from_numpy(plan).to(DEV), torch.from_numpy(scale).to(DEV)
    outT = [out16(C * R) for R in IC.WIMG_R]
    outS = [out16(R * C) for R in IC.WIMG_R]
    outP = out16(IC.WIMG_R[2] * 3 * C)
    rows, tiles = [], 0
    for i, R in enumerate(IC.WIMG_R):
        rows.append([d_in[i].data_ptr(), outT[i].data_ptr(), outS[i].data_ptr(), outP.data_ptr() if i == 2 else 0, R, C, IC.KINDS[skinds[i]],
                     tiles, d_plan.data_ptr() if i == 1 else 0, d_scale.data_ptr() if i == 1 else 0, 0, 0, 0, 0, 0, 0])
        tiles += IC.wimg_tiles(R, C)
    assert tiles == 14
    call("sed_weight_images", torch.tensor(rows, dtype=torch.int64, device=DEV), 3, tiles)
    for i, R in enumerate(IC.WIMG_R):
        flat = images[i].reshape(-1)
        check(f"weight images desc {i} outS ({skinds[i]})", outS[i][:R * C].view(R, C), TO16[skinds[i]](flat).reshape(R, C), skinds[i])
        check(f"weight images desc {i} outT (bf16)", outT[i][:C * R].view(C, R),
              np.ascontiguousarray(IC.f32_to_bf16_bits(flat).reshape(R, C).T), "bf16")
        assert untouched(outT[i], C * R) and untouched(outS[i], R * C)
    R = IC.WIMG_R[2]
    hi, lo = (a.reshape(R, C) for a in IC.hi_lo_f16(images[2].reshape(-1)))
    got = outP[:R * 3 * C].view(R, 3, C)
    for b, (nm, ref) in enumerate(zip(("hi", "hi", "lo"), (hi, hi, lo))):
        check(f"weight images desc 2 outP block {b} ({nm})", got[:, b], ref, "f16")
    assert untouched(outP, R * 3 * C)


# ================================================================================================ 4. past one pass of the grid
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_cast_three_passes(kind):
    n, L = IC.N_CAST, IC.cast_launch(IC.N_CAST)
    assert L.passes == 3
    bits = IC.random_f32_bits(n, 90, 145, 11)                             # 2^-37 .. 2^18: f16 flush, subnormals, normals, overflow
    out = out16(n)
    call("sed_cast_f32_bf16", dev_f32(bits), out, n, int(kind == "f16"))
    check(f"cast f32->{kind} n={n} ({L.passes} passes)", out[:n], TO16_LIB[kind](bits), kind)
    assert untouched(out, n)


def test_weight_residual_three_passes():
    n, L = IC.N_CAST, IC.cast_launch(IC.N_CAST)
    bits = IC.random_f32_bits(n, 90, 145, 12)
    out = out16(n)
    call("sed_weight_residual_f16", dev_f32(bits), out, n, 2048.0)
    check(f"weight residual n={n} ({L.passes} passes)", out[:n], IC.residual_f16(bits, 2048.0, IC.f32_to_f16_lib), "f16")
    assert untouched(out, n)


def test_f16_to_bf16_inplace_three_passes():
    """In place: an element visited twice would be converted from its own bf16 bits read as f16.  No element may equal that double
    conversion (where it differs from the single one)."""
    n, L = IC.N_INPLACE, IC.inplace_launch(IC.N_INPLACE)
    assert L.passes == 3
    h = IC.random_f16_bits(n, 13)
    buf = out16(n)
    buf[:n] = dev_16(h)
    call("sed_f16_to_bf16_inplace", buf, n)
    once = IC.f16_to_bf16_lib(h)
    twice = IC.f16_to_bf16_lib(once)
    check(f"f16->bf16 in place n={n} ({L.passes} passes)", buf[:n], once, "bf16")
    differs = twice != once
    assert differs.mean() > 0.9
    got = pat(buf[:n])
    dbl = int(((got == torch.from_numpy(twice.astype(np.int32)).to(DEV)) & torch.from_numpy(differs).to(DEV)).sum())
    log(f"f16->bf16 in place n={n}: elements equal to the double conversion={dbl}")
    assert dbl == 0 and untouched(buf, n)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_split3_three_passes(mode):
    M, K = IC.SPLIT_M, IC.SPLIT_K
    L = IC.split3_launch(M, K)
    assert L.passes == 3
    bits = IC.random_f32_bits(M * K, 90, 145, 14).reshape(M, K)
    nb = 2 if mode == 2 else 3
    out = out16(M * nb * K)
    call("sed_split3_f16", dev_f32(bits), out, M, K, mode)
    hi, lo = (a.reshape(M, K) for a in IC.hi_lo_f16(bits.reshape(-1), IC.f32_to_f16_lib))
    ref = np.stack(split_blocks(mode, hi, lo), 1)
    check(f"split3 mode {mode} M={M} K={K} ({L.passes} passes)", out[:M * nb * K].view(M, nb, K), ref, "f16")
    assert untouched(out, M * nb * K)


@pytest.mark.parametrize("M,K,ld", IC.TAIL_SHAPES)
def test_fp8_tail_past_one_pass(M, K, ld):
    L = IC.tail_launch(M, K)
    assert L.passes >= 2
    h = IC.random_f16_bits(M * K, 15).reshape(M, K)
    buf = out8(M * ld * 2)
    rows = buf[:M * ld * 2].view(M, 2 * ld)
    dh = dev_16(h)
    rows[:, :2 * K] = dh.view(torch.uint8)
    call("sed_fp8_tail", buf, M, K, ld)
    check(f"fp8 tail M={M} K={K} ld={ld} ({L.passes} passes)", rows[:, 2 * K:3 * K], IC.act_e4m3(h.reshape(-1), IC.f32_to_e4m3_lib).reshape(M, K),
          "e4m3")
    assert torch.equal(rows[:, :2 * K].contiguous().view(torch.int16), dh)
    assert bool((rows[:, 3 * K:] == SENT8).all()) and untouched(buf, M * ld * 2)


@pytest.mark.parametrize("N,K", IC.TWO_TERM_SHAPES)
def test_two_term_f8_past_one_pass(N, K):
    L = IC.two_term_launch(N, K)
    assert L.passes >= 2
    bits = IC.random_f32_bits(N * K, 100, 130, 16).reshape(N, K)           # 2^-27 .. 2^3: with s = 16 the lo byte spans the e4m3 range
    hi_g, lo_g, out = two_term(bits, 16)
    flat = bits.reshape(-1)
    check(f"two-term f8 hi N={N} K={K} ({L.passes} passes)", hi_g, IC.f32_to_f16_lib(flat).reshape(N, K), "f16")
    ref = IC.lo_e4m3(flat, 16, IC.f32_to_f16_lib, IC.f32_to_e4m3_lib).reshape(N, K)
    assert len(np.unique(ref)) > 200
    check(f"two-term f8 lo N={N} K={K} ({L.passes} passes)", lo_g, ref, "e4m3")
    assert untouched(out, N * 3 * K)


# ================================================================================================ 5. transpose: layout edges
def int_bits(x, kind):
    """integer-valued float tensor -> the 16-bit patterns of `kind` (exact: nothing rounds)."""
    return x.to(DT[kind]).contiguous().view(torch.int16).numpy().view(U16)


def same_bits(got, ref):
    """-> elements of `got` (device patterns) that differ from `ref` (numpy patterns): here every bit counts, the sign of a zero too."""
    return int((got != torch.from_numpy(np.ascontiguousarray(ref).astype(np.int32)).to(DEV)).sum())


@pytest.mark.parametrize("R,Rpad", IC.TRANSPOSE_RPAD)
def test_transpose_layout(R, Rpad):
    """Rpad any multiple of 16 past R (the guard r0 + seg < Rpad decides what is written), ldin > C, every input kind x outT kind x outS
    kind; outT only, outS only, colsum only.  Rows R .. Rpad-1 of outT are zeros, nothing is written behind C x Rpad, the pitch gap of
    the input reaches no output, colsum = start + the column sums exactly (integers: any order of the atomics gives the same)."""
    n = 0
    for C, gap, ikind in itertools.product(IC.TRANSPOSE_C, (0, 8), ("bf16", "f32", "f16")):
        ldin = C + gap
        assert IC.transpose_args_ok(R, Rpad, C, ldin, IC.KINDS[ikind])
        x = IC.transpose_input(R, C, ldin)
        dx = x.to(DT[ikind]).to(DEV)
        start = torch.arange(C, dtype=torch.float32) - 5.0
        want_sum = (start + x[:, :C].sum(0)).to(DEV)
        variants = [(tk, sk, True) for tk in ("bf16", "f16") for sk in ("bf16", "f16")]
        variants += [("bf16", None, False), (None, "f16", False), (None, None, True)]
        for tk, sk, with_sum in variants:
            outT, outS = out16(C * Rpad), out16(R * C)
            colsum = start.clone().to(DEV) if with_sum else None
            call("sed_transpose_to_bf16", dx, IC.KINDS[ikind], R, C, ldin, outT if tk else None, Rpad, IC.KINDS[tk or "bf16"],
                 outS if sk else None, IC.KINDS[sk or "bf16"], colsum)
            tag = f"transpose R={R} Rpad={Rpad} C={C} ldin={ldin} {ikind}->T:{tk} S:{sk} sum:{with_sum}"
            if tk:
                refT = np.zeros((C, Rpad), dtype=U16)
                refT[:, :R] = int_bits(x[:, :C], tk).T
                got = pat(outT[:C * Rpad]).view(C, Rpad)
                assert bool((got[:, R:] == 0).all()), (tag, "rows R .. Rpad-1 of outT are not all zero")
                assert same_bits(got, refT) == 0, (tag, "outT")
            else:
                assert untouched(outT, 0), tag
            if sk:
                assert same_bits(pat(outS[:R * C]).view(R, C), int_bits(x[:, :C], sk)) == 0, (tag, "outS")
            else:
                assert untouched(outS, 0), tag
            assert untouched(outT, C * Rpad) and untouched(outS, R * C), tag
            if with_sum:
                assert torch.equal(colsum, want_sum), tag
            n += 1
    log(f"transpose layout R={R} Rpad={Rpad}: launches={n} compared bit for bit, zero rows {R}..{Rpad - 1}, guards untouched")


# ================================================================================================ 6. group colmean
def colmean(x, groups, rows, K, ld, step, storage, plain=False):
    out = out16(groups * K)
    if plain:
        call("sed_group_colmean", x, out, groups, rows, K, step, int(storage == "f16"))
    else:
        call("sed_group_colmean_ld", x, out, groups, rows, K, ld, step, int(storage == "f16"))
    assert untouched(out, groups * K)
    return out[:groups * K].view(DT[storage]).view(groups, K)


@pytest.mark.parametrize("storage", ["bf16", "f16"])
def test_group_colmean_exact_inputs(storage):
    """Multiples of 2^-6 on the visited rows 0, step, 2 step, ..., 1000 on every other row and in the pitch gap: the sums are exact in
    fp32, so the bound is half an ulp of the storage format + 4 fp32 ulps of |ref| (derived in image_cases.colmean_exact_ref).
    A dropped or extra row moves the mean by >= 10 bounds (tests/test_image_cases_cpu.py)."""
    G, worst, at = IC.COLMEAN_GROUPS, 0.0, None
    for rows, step, K, ld in IC.colmean_cases():
        x = IC.colmean_exact_input(rows, step, K, ld, storage)
        ref, bound = IC.colmean_exact_ref(x, rows, step, K, storage)
        got = colmean(x.to(DEV), G, rows, K, ld, step, storage).double().cpu()
        ratio = float(((got - ref).abs() / bound).max())
        assert bool(((got - ref).abs() <= bound).all()), (rows, step, K, ld, ratio)
        if ld == K:                                        # the entry without a pitch is the same launch
            again = colmean(x.to(DEV), G, rows, K, ld, step, storage, plain=True).double().cpu()
            assert torch.equal(again, got)
        if ratio > worst:
            worst, at = ratio, (rows, step, K, ld)
    log(f"group colmean exact inputs {storage}: cases={len(IC.colmean_cases())} worst_err_over_bound={worst:.5f} at rows,step,K,ld={at}")


@pytest.mark.parametrize("storage", ["bf16", "f16"])
def test_group_colmean_gaussian_activations(storage):
    """rows = 602, step = 8 (the engine's), K = 768 in a pitch of 1152, under the bound of walk_cases.judge:
    |got - ref64| <= 8 max|ref32 - ref64| + half an ulp of the storage format."""
    G, rows, step, K, ld = IC.COLMEAN_GROUPS, 602, 8, 768, 1152
    x = IC.colmean_gauss_input(K, ld, storage)
    vis, nvis = IC.colmean_visits(rows, step)
    xs = x.view(G, rows, ld)[:, vis, :K]
    ref64, ref32 = xs.double().sum(1) / nvis, xs.float().sum(1) / nvis
    got = colmean(x.to(DEV), G, rows, K, ld, step, storage)
    err, yard, worst, ok, mag = X.judge(got.float(), ref64, ref32, storage)
    log(f"group colmean gaussian {storage} rows={rows} step={step}: max_abs_err={err:.4e} yardstick_f32_vs_f64={yard:.4e} "
        f"magnitude={mag:.3e} worst_err_over_bound={worst:.5f}")
    assert ok


# ================================================================================================ 7. refusals
def test_documented_refusals_leave_the_output_alone():
    x32 = torch.ones(4096, device=DEV)
    x16 = torch.ones(8192, dtype=F16, device=DEV)
    out = out16(16384)
    bad = [("sed_cast_f32_bf16", (x32, out, 6, 1)), ("sed_weight_residual_f16", (x32, out, 6, 2048.0)),
           ("sed_f16_to_bf16_inplace", (out, 12)),
           ("sed_split3_f16", (x32, out, 4, 7, 0)), ("sed_split3_f16", (x32, out, 4, 8, 3)), ("sed_split3_f16", (x32, out, 4, 8, -1)),
           ("sed_fp8_tail", (out, 4, 60, 96)), ("sed_fp8_tail", (out, 4, 64, 88)),
           ("sed_transpose_to_bf16", (x32, 1, 17, 64, 64, out, 16, 0, None, 0, None)),        # Rpad < R
           ("sed_transpose_to_bf16", (x32, 1, 16, 96, 96, out, 16, 0, None, 0, None)),        # C % 64
           ("sed_transpose_to_bf16", (x32, 1, 16, 64, 64, out, 24, 0, None, 0, None)),        # Rpad % 16
           ("sed_transpose_to_bf16", (x32, 1, 16, 64, 68, out, 16, 0, None, 0, None)),        # ldin % 8
           ("sed_group_colmean_ld", (x16, out, 3, 8, 128, 128, 1, 1)), ("sed_group_colmean_ld", (x16, out, 3, 8, 256, 248, 1, 1)),
           ("sed_group_colmean_ld", (x16, out, 3, 8, 256, 256, 0, 1)), ("sed_group_colmean", (x16, out, 3, 8, 256, 0, 1))]
    for name, args in bad:
        with pytest.raises(SedHipError):
            call(name, *args)
        assert untouched(out, 0), (name, args)
    log(f"refusals: {len(bad)} calls raised SedHipError, outputs untouched")
