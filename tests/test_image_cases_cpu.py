"""tests/image_cases.py proved on the CPU, before tests/test_gpu_image_kernels.py holds the hardware to it:

1. the two forms of every conversion (integer arithmetic on the bit patterns; the library cast) agree on every value set;
2. EDGE32_F16 / EDGE32_BF16 are the boundaries they claim to be: below the midpoint rounds down, above it rounds up, the midpoint goes
   to the even neighbour; every boundary of the format is there;
3. EDGE_E4M3_LO reaches every finite e4m3 boundary of both signs exactly, one step below and one above, and every weight keeps
   f16(w) == +-H;
4. v - f32(f16(v)) in fp32 is the float64 difference: the derived references have one rounding;
5. every loop case leaves the first pass of its restated grid and ends off a block boundary; every transpose and colmean case passes the
   restated argument checks, every refused size fails them;
6. a dropped row, an extra row or the divisor rows / step moves the exact colmean reference by >= 10 bounds."""
import numpy as np
import pytest
import torch

import image_cases as IC
from image_cases import U16, U32


def same(a, b, fmt):
    v = IC.compare(a.astype(np.int64), b.astype(np.int64), fmt)
    assert v.bad == 0 and v.zero_sign == 0, v
    return v


# ------------------------------------------------------------------------------------------------ 1. form (a) == form (b)
@pytest.mark.parametrize("name", ["f32->f16", "f32->bf16", "f32->e4m3"])
def test_f32_conversions_agree_on_every_set(name):
    fa, fb, fmt = IC.CONVERSIONS[name]
    lo_w = np.array([c.w_bits for c in IC.edge_e4m3_lo()], dtype=U32)
    for bits in (IC.EDGE32_F16, IC.EDGE32_BF16, lo_w, IC.f16_to_f32_bits(IC.ALL_F16), IC.bf16_to_f32_bits(IC.ALL_BF16)):
        same(fa(bits), fb(bits), fmt)
    # the e4m3 grid itself: every boundary, one fp32 ulp either side, both signs, and the clamp
    b = IC._bits_of(IC.E4M3_BOUNDARIES)
    dense = np.concatenate([b - 1, b, b + 1, IC._bits_of(IC.E4M3_VALUES), IC._bits_of(np.array([448.0, 449.0, 464.0, 465.0, 480.0, 1e9]))])
    dense = np.concatenate([dense, dense | U32(0x80000000)])
    same(fa(dense), fb(dense), fmt)


@pytest.mark.parametrize("name", ["f16->bf16", "bf16->f16", "f16->f32"])
def test_16bit_conversions_agree_on_all_patterns(name):
    fa, fb, fmt = IC.CONVERSIONS[name]
    v = same(fa(IC.ALL_F16), fb(IC.ALL_F16), fmt)
    assert v.n == 65536 and v.nans == (2046 if name != "bf16->f16" else 254)


def test_identities_on_non_nan_patterns():
    """f16 -> f32 -> f16 and bf16 -> f32 -> bf16 give the pattern back (what the transpose kernel's same-kind copies must do)."""
    ok = ~IC.is_nan(IC.ALL_F16.astype(np.int64), "f16")
    assert np.array_equal(IC.f32_to_f16_bits(IC.f16_to_f32_bits(IC.ALL_F16))[ok], IC.ALL_F16[ok])
    ok = ~IC.is_nan(IC.ALL_BF16.astype(np.int64), "bf16")
    assert np.array_equal(IC.f32_to_bf16_bits(IC.bf16_to_f32_bits(IC.ALL_BF16))[ok], IC.ALL_BF16[ok])


def test_derived_references_agree_in_both_forms():
    for bits in (IC.EDGE32_F16, np.concatenate(list(IC.lo_bands().values()))):
        for a, b in zip(IC.hi_lo_f16(bits), IC.hi_lo_f16(bits, IC.f32_to_f16_lib)):
            same(a, b, "f16")
        same(IC.residual_f16(bits, 2048.0), IC.residual_f16(bits, 2048.0, IC.f32_to_f16_lib), "f16")
        same(IC.lo_e4m3(bits, 20), IC.lo_e4m3(bits, 20, IC.f32_to_f16_lib, IC.f32_to_e4m3_lib), "e4m3")
    same(IC.act_e4m3(IC.ALL_F16), IC.act_e4m3(IC.ALL_F16, IC.f32_to_e4m3_lib), "e4m3")
    # |h| >= 1792 -> +-448, NaN -> NaN
    a, h = IC.act_e4m3(IC.ALL_F16).astype(np.int64), IC.f16_to_f32_bits(IC.ALL_F16).view(np.float32)
    big = np.abs(h) >= 1792.0
    assert big.sum() == 2 * (0x7C00 - 0x6700 + 1) and np.array_equal(a[big], np.where(h[big] > 0, 0x7E, 0xFE))
    assert IC.is_nan(a, "e4m3").sum() == 2046


# ------------------------------------------------------------------------------------------------ 2. the fp32 edge sets
@pytest.mark.parametrize("fmt", ["f16", "bf16"])
def test_edge32_sets_are_the_rounding_boundaries(fmt):
    core = IC.edge32_f16_core() if fmt == "f16" else IC.edge32_bf16_core()
    conv = IC.f32_to_f16_bits if fmt == "f16" else IC.f32_to_bf16_bits
    n = 0x7C00 if fmt == "f16" else 0x7F80                      # non-negative finite values = boundaries above them
    assert core.shape == (n, 4)
    k = np.arange(n, dtype=np.int64)
    lower, below, mid, above = (conv(core[:, i]).astype(np.int64) for i in range(4))
    assert np.array_equal(lower, k) and np.array_equal(below, k) and np.array_equal(above, k + 1)
    assert np.array_equal(mid, k + (k & 1))                      # ties to even; the last boundary goes to inf
    assert mid[-1] == IC.INF[fmt] and above[-1] == IC.INF[fmt] and below[-1] == IC.INF[fmt] - 1
    if fmt == "bf16":
        assert core[-1, 2] == 0x7F7F8000
    else:
        assert core[-1, 2] == np.array([65520.0], dtype=np.float32).view(U32)[0] and core[0, 2] == 0x33000000     # 2^-25
    # strictly between the neighbours, one fp32 ulp from the midpoint, and ascending: no boundary twice, none missing
    f = core.view(np.float32).astype(np.float64)
    assert np.all(f[:, 0] < f[:, 1]) and np.all(np.diff(core.astype(np.int64), axis=1)[:, 1:] == 1) and np.all(f[1:, 0] > f[:-1, 3])
    # both signs and the extras are in the set
    full = IC.EDGE32_F16 if fmt == "f16" else IC.EDGE32_BF16
    assert len(full) == 8 * n + len(IC.EXTRAS32)
    neg = conv(core.reshape(-1) | U32(0x80000000)).astype(np.int64)
    assert np.array_equal(neg, conv(core.reshape(-1)).astype(np.int64) | 0x8000)
    for pat in IC.EXTRAS32:
        assert pat in full
    assert conv(np.array([0x33000000, 0x33000001], dtype=U32)).tolist() == ([0, 1] if fmt == "f16" else [0x3300, 0x3300])


def test_hi_residual_is_exact_in_fp32():
    """v - f32(f16(v)) == the float64 difference on all of EDGE32_F16 with a finite hi."""
    v = IC.EDGE32_F16
    hi = IC.f16_to_f32_bits(IC.f32_to_f16_bits(v)).view(np.float32)
    fin = np.isfinite(hi) & np.isfinite(v.view(np.float32))
    d32 = (v.view(np.float32)[fin] - hi[fin]).astype(np.float64)
    assert fin.sum() > 250000 and np.array_equal(d32, v.view(np.float32)[fin].astype(np.float64) - hi[fin].astype(np.float64))
    # ... and the scalings by 2048 and by 2^s are exact wherever the product stays a normal fp32 number
    assert np.array_equal((np.float32(2048.0) * d32.astype(np.float32)).astype(np.float64), 2048.0 * d32)


def test_most_weight_residuals_are_f16_subnormals():
    """At a weight scale of 0.03 nearly every lo term W - f16(W) is an f16 subnormal: the corner the edge sets cover deliberately."""
    w = (0.03 * torch.randn(1 << 20, generator=torch.Generator().manual_seed(1))).numpy().view(U32)
    _, lo = IC.hi_lo_f16(w)
    assert np.mean((lo & 0x7C00) == 0) > 0.999


# ------------------------------------------------------------------------------------------------ 3. the e4m3 boundaries of the lo byte
def test_edge_e4m3_lo_reaches_every_boundary():
    cases = IC.edge_e4m3_lo()
    assert len(IC.E4M3_BOUNDARIES) == 126 and IC.E4M3_VALUES[-1] == 448.0 and IC.E4M3_VALUES[1] == 2.0 ** -9
    hbits = int(IC.f32_to_f16_bits(IC._bits_of(np.array([IC.LO_H])))[0])
    seen = set()
    for c in cases:
        w = np.array([c.w_bits], dtype=U32)
        hi = int(IC.f32_to_f16_bits(w)[0])
        assert hi & 0x7FFF == hbits and (hi >> 15) == (c.w_bits >> 31)                       # f16(w) == +-H
        d = w.view(np.float32).astype(np.float64)[0] - IC.f16_to_f32_bits(np.array([hi], dtype=U16)).view(np.float32).astype(np.float64)[0]
        assert d * 2.0 ** c.s == c.target                                                 # 2^s d lands where it was aimed
        got = int(IC.lo_e4m3(w, c.s)[0])
        assert got == c.code, (c, got)
        if c.kind != 2:
            mag, b = abs(c.target), None
            i = int(np.argmin(np.abs(IC.E4M3_BOUNDARIES - mag)))
            b = IC.E4M3_BOUNDARIES[i]
            assert (mag == b) if c.kind == 0 else (0 < (mag - b) * c.kind < b * 2.0 ** -5)
            seen.add((i, c.kind, c.target > 0, c.w_bits >> 31))
        else:
            assert abs(c.target) >= 448.0 and c.code & 0x7F == 0x7E
    # every boundary x {below, on, above} x sign of the lo term x sign of the weight
    assert len(seen) == 126 * 3 * 2 * 2
    assert sum(c.kind == 2 for c in cases) == 4 * len(IC.LO_CLAMP_J)
    bands = IC.lo_bands()
    assert len(bands) >= 10 and all(-100 <= s <= 100 and len(w) % 8 == 0 for s, w in bands.items())
    assert sum(len(w) for w in bands.values()) >= len(cases)


# ------------------------------------------------------------------------------------------------ 5. shapes against the restated checks
def test_loop_cases_leave_the_first_pass_off_a_block_boundary():
    cases = IC.loop_cases()
    assert {c.kernel for c in cases} == {"cast", "residual", "inplace", "split3", "fp8_tail", "two_term_f8"}
    for c in cases:
        L = c.launch
        assert L.blocks == (IC.CAP_8192 if c.kernel in ("fp8_tail", "two_term_f8") else IC.CAP_4096), c
        assert L.items > L.per_pass and L.items % 256 != 0 and L.items % L.per_pass != 0, c
    # some threads iterate three times: more than one full pass past the cap.  (The first shapes of the two 8192-workgroup kernels
    # stop at two passes; their second shapes are there for the third.)
    for k in {c.kernel for c in cases}:
        assert max(c.launch.passes for c in cases if c.kernel == k) == 3, k
        big = [c for c in cases if c.kernel == k and c.launch.passes == 3]
        assert all(c.launch.items > 2 * c.launch.per_pass for c in big)
    assert [c.launch.passes for c in cases if c.kernel == "fp8_tail"] == [2, 3]
    assert [c.launch.passes for c in cases if c.kernel == "two_term_f8"] == [2, 3]
    # the shapes the suite had before stay inside one pass
    assert IC.inplace_launch(2380 * 768).passes == 1 and IC.split3_launch(1000, 768).passes == 1 and IC.tail_launch(2380, 3072).passes == 1
    # and production crosses it
    assert IC.inplace_launch(38080 * 3072).passes > 10 and IC.tail_launch(38080, 3072).passes > 5
    assert IC.cast_args_ok(IC.N_CAST) and IC.inplace_args_ok(IC.N_INPLACE) and IC.SPLIT_K % 4 == 2
    assert all(IC.split3_args_ok(IC.SPLIT_M, IC.SPLIT_K, m) for m in (0, 1, 2))
    assert all(IC.tail_args_ok(*s) and s[2] > s[1] + s[1] // 2 for s in IC.TAIL_SHAPES)
    assert all(IC.two_term_args_ok(N, K, 16) for N, K in IC.TWO_TERM_SHAPES)
    assert max(4 * IC.N_CAST, 2 * IC.N_INPLACE, 12 * IC.SPLIT_M * IC.SPLIT_K // 2, 2 * IC.TAIL_SHAPES[0][0] * IC.TAIL_SHAPES[0][2]) < 52e6


def test_refused_sizes_fail_the_restated_checks():
    assert not IC.cast_args_ok(6) and not IC.inplace_args_ok(12)
    assert not IC.split3_args_ok(4, 7, 0) and not IC.split3_args_ok(4, 8, 3) and not IC.split3_args_ok(4, 8, -1)
    assert not IC.tail_args_ok(4, 60, 96) and not IC.tail_args_ok(4, 64, 88)
    assert not IC.transpose_args_ok(17, 16, 64, 64, 1) and not IC.transpose_args_ok(16, 16, 96, 96, 1)
    assert not IC.transpose_args_ok(16, 24, 64, 64, 1) and not IC.transpose_args_ok(16, 16, 64, 68, 1)
    assert not IC.colmean_args_ok(3, 8, 128, 128, 1) and not IC.colmean_args_ok(3, 8, 256, 248, 1) and not IC.colmean_args_ok(3, 8, 256, 256, 0)


def test_transpose_and_colmean_cases_are_accepted():
    cases = IC.transpose_cases()
    assert len(cases) == 4 * 2 * 2 * 3
    for R, Rpad, C, ldin, k in cases:
        assert IC.transpose_args_ok(R, Rpad, C, ldin, IC.KINDS[k]) and Rpad >= R and ldin >= C
    # Rpad off pad64(R): the write guard decides.  (2380, 2432) leaves a written segment that holds zeros only.
    assert [Rpad == (R + 63) // 64 * 64 for R, Rpad in IC.TRANSPOSE_RPAD] == [False, False, False, True]
    assert IC.transpose_grid(16, 64) == (1, 1) and IC.transpose_grid(2432, 192) == (3, 38)
    assert IC.transpose_segments(1, 16) == ([0], []) and IC.transpose_segments(100, 112) == ([0, 16, 32], [])
    assert IC.transpose_segments(130, 144) == ([0], []) and IC.transpose_segments(2380, 2432) == ([0, 16, 32, 48], [16, 32, 48])
    x = IC.transpose_input(2380, 192, 200)
    assert float(x[:, :192].abs().max()) == 64.0 and torch.equal(x.to(torch.bfloat16).float(), x) and bool((x[:, 192:] == 77).all())
    assert torch.equal(x[:, :192].sum(0).double(), x[:, :192].double().sum(0))
    cm = IC.colmean_cases()
    assert len(cm) == 6 * 3 * 2 * 2
    for rows, step, K, ld in cm:
        assert IC.colmean_args_ok(IC.COLMEAN_GROUPS, rows, K, ld, step)
        vis, nvis = IC.colmean_visits(rows, step)
        assert len(vis) == nvis
    for R in IC.WIMG_R:
        assert R % 16 == 0 and IC.WIMG_C % 64 == 0
    assert [IC.wimg_tiles(R, IC.WIMG_C) for R in IC.WIMG_R] == [2, 4, 8]


# ------------------------------------------------------------------------------------------------ 6. colmean: exact inputs, sensitivity
@pytest.mark.parametrize("storage", ["bf16", "f16"])
def test_colmean_exact_inputs_and_sensitivity(storage):
    worst, best = {}, {}
    for rows, step, K, ld in IC.colmean_cases():
        x = IC.colmean_exact_input(rows, step, K, ld, storage)
        vis, nvis = IC.colmean_visits(rows, step)
        xs = x.float().view(IC.COLMEAN_GROUPS, rows, ld)
        assert torch.equal(xs * 64, (xs * 64).round()) and float(xs[:, vis, :K].abs().max()) <= 4.0
        unvis = [r for r in range(rows) if r not in set(vis)]
        assert bool((xs[:, unvis] == IC.UNVISITED).all()) and bool((xs[:, :, K:] == IC.UNVISITED).all())
        # the fp32 sum in any order is the float64 sum
        assert torch.equal(xs[:, vis, :K].sum(1).double(), xs[:, vis, :K].double().sum(1))
        assert torch.equal(xs[:, vis, :K].flip(1).sum(1), xs[:, vis, :K].sum(1))
        # the plain fp32 division sits inside the bound
        ref, bound = IC.colmean_exact_ref(x, rows, step, K, storage)
        dt = torch.bfloat16 if storage == "bf16" else torch.float16
        got = (xs[:, vis, :K].sum(1) / nvis).to(dt).double()
        assert bool(((got - ref).abs() <= bound).all())
        for what, ratio in IC.colmean_sensitivity(x, rows, step, K, storage).items():
            # (a divisor off by one in 201 is 2.5 bounds of bf16 at rows = 602, step = 3: outside, but not by ten; rows = 7 is by 1000)
            assert ratio >= (IC.SENS if what != "nvis = rows / step" else 2.0), (rows, step, K, ld, what, ratio)
            worst[what] = min(worst.get(what, ratio), ratio)
            best[what] = max(best.get(what, ratio), ratio)
    assert set(worst) == {"last visited row dropped", "an unvisited row added", "nvis = rows / step"}
    assert best["nvis = rows / step"] >= 100 * IC.SENS
