"""The CNN-branch kernels of csrc/cnn_branch.hip and csrc/dw_narrow.hip at every layer geometry of the real stack and past one pass of
their grid (need an MI355X).  Cases, references and the restated launch arithmetic: tests/cnn_cases.py, proved on the CPU by
tests/test_cnn_cases_cpu.py.

A. The ten layers of PaSST_CNN's CNN branch (16, 16, 32, 32, 64, 64, 128, 128, 256, 384 filters; poolings (2,2), (1,1), (2,2), (1,1),
   (1,2) x 5, (1,1); widths 128 .. 1) at T = 12, B = 2, with the arguments PmamEngine passes: sed_conv3x3_im2col and sed_col2im3x3
   (layers 1-9, Kp 256 .. 2304, W = 2 and W = 1 where every left / right tap is padding), sed_colstats modes 0 and 1 (one to six column
   groups), sed_bn_act, sed_bn_bwd (ldo = ldg, and 16 on layer 0), sed_cg_pool / sed_cg_pool_bwd with and without a mask (pooling (1,2),
   C == Cpo, out16 = NULL on the last layer), and the 16-filter fused path on layers 0 and 1 (sed_conv0_fwd16 with and without sums,
   sed_conv0_dw16, sed_cg_gate16_pool, sed_cg_gate16_pool_bwd), also with a pitched Y (ldy = 64).
B. The smallest shape at which each entry point takes a second trip of its grid-stride or slab loop: sed_conv0_fwd16 (B 1, T 8193),
   sed_conv0_dw16 (T 1025: 513 slabs of 256 rows, the last half full), sed_cg_gate16_pool_bwd (H 8194), sed_bn_act / sed_bn_bwd
   (M 262 145), sed_cg_pool (H 16 386), sed_cg_pool_bwd (H 8193), sed_conv3x3_im2col (H 2049), sed_col2im3x3 (H 65 537, a 302 MB dcol),
   sed_colstats (17 trips of 2048 slabs), sed_transpose_narrow (R 524 325, C 16 / 32, both input types, column sums).
   Left out on purpose: the grid cap of sed_cg_gate16_pool (16384 x 256 OUTPUT pixels) is first reached at layer 1 above batch 131; a
   crossing case would need about 1 GB of operands.

Bounds: bit equality for the gathers (with in_f16 = 1 the transposed image is bf16(float(f16)), rounded to nearest even); per element
|got - ref64| <= 8 max|ref32 - ref64| + half an ulp of the storage format for element-wise outputs (walk_cases.judge); per word
(d + 2) 2^-24 sum|term| for the atomically added sums (cnn_cases.sum_bound).  Every output buffer is NaN before the call (sums, which
accumulate, are zero); padding columns the kernel must write come back exactly zero; columns it must not touch (dW past column 8, NaN
pitch columns of the inputs) stay out.  Errors, yardsticks, worst error / bound and drop ratios go to cnn_kernel_errors.log under
SED_TEST_LOG_DIR, else test_logs/.

Measured on an MI355X, worst error / bound (each test's docstring has its own): gathers bit-equal; fp32 element-wise outputs 0.08 .. 0.25;
16-bit images 0.98 .. 1.000 (their rounding is the bound); atomically added sums 0.003 .. 0.22 in part A and 0.006 .. 0.020 in part B,
where leaving out the last trip moves the float64 sums by 24 .. 914 bounds."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import cnn_cases as X  # noqa: E402
from cnn_cases import F32, F64, F16, BF16, LAYERS, DROP_SCALE  # noqa: E402
from transformer4sed_amd.ops import call  # noqa: E402

DEV = "cuda"
LOGDIR = os.environ.get("SED_TEST_LOG_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_logs")
LOG = os.path.join(LOGDIR, "cnn_kernel_errors.log")
NAN = float("nan")
B = X.B_A


def log(line):
    os.makedirs(LOGDIR, exist_ok=True)
    with open(LOG, "a") as f:
        f.write(line + "\n")
    print(line)


def check(name, got, ref64, ref32, storage="f32"):
    """Logs and asserts, per element,  |got - ref64| <= 8 max|ref32 - ref64| + half_ulp(storage) at |ref64|; a NaN left of the prefill
    fails (NaN <= tol is false)."""
    err, yard, worst, ok, mag = X.judge(got.float() if got.dtype != F32 else got, ref64, ref32, storage)
    log(f"{name}: max_abs_err={err:.4e} yardstick_f32_vs_f64={yard:.4e} magnitude={mag:.3e} storage={storage} worst_err_over_bound={worst:.3f}")
    assert ok and not bool(torch.isnan(got).any()), (name, err, yard, worst)


def check_sum(name, got, terms64, d, late=None):
    """An atomically added sum against the float64 sum of its terms [rows, ...]: per word within (d + 2) 2^-24 sum|term|."""
    ref, bound = terms64.sum(0), X.sum_bound(d, terms64.abs().sum(0))
    err, worst, ok = X.judge_sum(got.reshape(ref.shape), ref, bound)
    log(f"{name}: max_abs_err={err:.4e} d={d} magnitude={float(ref.abs().max()):.3e} worst_err_over_bound={worst:.4f}")
    assert ok and not bool(torch.isnan(got).any()), (name, err, worst)
    if late is not None:
        r = X.drop_ratio(terms64[late:].sum(0), bound)
        log(f"{name} without rows {late}..{terms64.shape[0] - 1}: reference moves by {r:.3e} bounds")
        assert r >= X.SENS, (name, r)


def same_bits(name, got, want):
    """16-bit images bit for bit (int16 views: an unwritten NaN differs, +0 and -0 differ)."""
    ok = torch.equal(X.bits(got).cpu(), X.bits(want).cpu())
    log(f"{name}: {'bit-equal' if ok else 'DIFFERS'} ({got.numel()} words)")
    assert ok, name


def nans(*shape, dtype=F32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def zeros(*shape):
    return torch.zeros(*shape, device=DEV)


def on_dev(d):
    return {k: (v.to(DEV).contiguous() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


def pitched(x, ld, dtype=None):
    """x [M, C] in a NaN buffer of pitch ld >= C."""
    out = nans(x.shape[0], ld, dtype=dtype or x.dtype)
    out[:, :x.shape[1]] = x.to(DEV)
    return out


def exactly_zero(t):
    return t.numel() == 0 or (not bool(torch.isnan(t).any()) and float(t.float().abs().max()) == 0.0)


# ================================================================================================ A. gathers
@pytest.mark.parametrize("i", range(1, 10))
def test_im2col_and_col2im_at_every_layer(i):
    """Bit equality, layers 1-9 (Kp 256 .. 2304; W = 2, W = 1 and H = 3 among them); the NaN channel pitch of X and NaN columns of dcol
    past 9 cin are never read.  Measured on an MI355X: bit-equal on all nine layers."""
    l, d = LAYERS[i], X.layer_inputs(i)
    M = d["M"]
    col = nans(M, l.Kp, dtype=F16)
    call("sed_conv3x3_im2col", d["X"].to(DEV), col, B, l.H, l.W, l.cin, l.cpin, l.Kp)
    same_bits(f"A layer {i} im2col (cin {l.cin}, H {l.H}, W {l.W}, Kp {l.Kp})", col, X.im2col_ref(X.bits(d["X"]), B, l.H, l.W, l.cin, l.Kp))
    assert bool((X.bits(col)[:, 9 * l.cin:] == 0).all()), "zeros from 9 cin to Kp"
    dX = nans(M, l.cin)
    call("sed_col2im3x3", d["dcol"].to(DEV), l.Kp, dX, B, l.H, l.W, l.cin)
    ok = torch.equal(dX.cpu(), X.col2im_ref(d["dcol"], B, l.H, l.W, l.cin))
    log(f"A layer {i} col2im (cin {l.cin}, H {l.H}, W {l.W}, Kp {l.Kp}): {'bit-equal' if ok else 'DIFFERS'} to the fp32 sum in tap order")
    assert ok


# ================================================================================================ A. column statistics
@pytest.mark.parametrize("i", range(10))
def test_colstats_at_every_layer(i):
    """Modes 0 and 1 with lda = ldb = ldy: 16 / 32 (the 256 % C == 0 path), 64, 128 (two column groups), 256 (four), 384 (six).
    Measured on an MI355X, worst error / bound over the ten layers: 0.003 .. 0.22."""
    l, d = LAYERS[i], X.layer_inputs(i)
    M, co = d["M"], l.co
    t = on_dev(d)
    dd = X.d_colstats(M, co)
    s1, s2 = zeros(co), zeros(co)
    call("sed_colstats", t["Y"], l.ldy, None, 0, None, None, s1, s2, M, co, 0)
    t1, t2 = X.stats_terms(d["Y"][:, :co])
    check_sum(f"A layer {i} colstats mode 0 s1 (C {co})", s1, t1, dd)
    check_sum(f"A layer {i} colstats mode 0 s2 (C {co})", s2, t2, dd)
    s1, s2 = zeros(co), zeros(co)
    call("sed_colstats", t["dz"], l.ldy, t["Y"], l.ldy, t["ah"], t["bh"], s1, s2, M, co, 1)
    t1, t2 = X.stats_terms(d["dz"][:, :co], d["Y"][:, :co], d["ah"], d["bh"])
    check_sum(f"A layer {i} colstats mode 1 s1 (C {co})", s1, t1, dd)
    check_sum(f"A layer {i} colstats mode 1 s2 (C {co})", s2, t2, dd)


# ================================================================================================ A. BatchNorm affine and backward
@pytest.mark.parametrize("i", range(10))
def test_bn_act_and_bn_bwd_at_every_layer(i):
    """Z (f16 image, zeros from co to Cp) and dY (bf16, ldo = ldg; 16 on layer 0 as well), zeros from co to ldo.
    Measured on an MI355X, worst error / bound over the ten layers: Z 0.998, dY 1.000 (the 16-bit rounding)."""
    l, d = LAYERS[i], X.layer_inputs(i)
    M, co = d["M"], l.co
    t = on_dev(d)
    Z = nans(M, l.Cp, dtype=F16)
    call("sed_bn_act", t["Y"], l.ldy, t["a"], t["b"], Z, M, co, l.Cp, 1)
    check(f"A layer {i} bn_act Z (f16, C {co}, Cp {l.Cp})", Z[:, :co], X.bn_act_ref(d["Y"], d["a"], d["b"], F64), X.bn_act_ref(d["Y"], d["a"], d["b"], F32), "f16")
    assert exactly_zero(Z[:, co:])
    args = (d["dz"], d["Y"], d["ah"], d["bh"], d["gamma"], d["s1"], d["s2"])
    r64, r32 = X.bn_bwd_ref(*args, F64), X.bn_bwd_ref(*args, F32)
    for ldo in ([l.ldg, 16] if i == 0 else [l.ldg]):
        dY = nans(M, ldo, dtype=BF16)
        call("sed_bn_bwd", t["dz"], l.ldy, t["Y"], l.ldy, t["ah"], t["bh"], t["gamma"], t["s1"], t["s2"], dY, ldo, M, co)
        check(f"A layer {i} bn_bwd dY (bf16, C {co}, ldo {ldo})", dY[:, :co], r64, r32, "bf16")
        assert exactly_zero(dY[:, co:])


# ================================================================================================ A. gate * dropout * pooling
@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("i", range(10))
def test_cg_pool_and_its_backward_at_every_layer(i, masked):
    """sed_cg_pool (fp32 rows and, except on the last layer, the f16 NHWC image with zeros from co to Cpo) and sed_cg_pool_bwd (dzd with
    ldz = ldy, dL16 with ldl16 = ldg, zeros from co) with a mask and drop_scale = 1 / 0.9, and with mask = NULL.
    Measured on an MI355X, worst error / bound over the ten layers: out32 0.22, out16 0.996, dzd 0.16, dL16 0.999 (the 16-bit rounding)."""
    l, d = LAYERS[i], X.layer_inputs(i)
    M, Mo, co = d["M"], d["Mo"], l.co
    t = on_dev(d)
    mask, scale = (d["mask"], DROP_SCALE) if masked else (None, 1.0)
    geo = (B, l.H, l.W, l.ph, l.pw)
    args = (d["Y"][:, :co], d["a"], d["b"], d["L"][:, :co], mask, scale)
    tag = f"A layer {i} {'mask' if masked else 'no mask'} (C {co}, H {l.H}, W {l.W}, pool ({l.ph}, {l.pw}))"
    out16 = None if l.last else nans(B, l.H // l.ph, l.W // l.pw, l.Cp, dtype=F16)
    out32 = nans(Mo, co)
    call("sed_cg_pool", t["Y"], l.ldy, t["a"], t["b"], t["L"], l.ldy, t["mask"] if masked else None, scale, out16, out32, B, l.H, l.W, co, l.Cp,
         l.ph, l.pw, 1)
    r64, r32 = X.cg_pool_ref(*args, *geo, F64), X.cg_pool_ref(*args, *geo, F32)
    check(f"{tag} cg_pool out32", out32, r64, r32)
    if out16 is not None:
        o = out16.view(Mo, l.Cp)
        check(f"{tag} cg_pool out16 (f16)", o[:, :co], r64, r32, "f16")
        assert exactly_zero(o[:, co:])
    dzd, dL16 = nans(M, l.ldy), nans(M, l.ldg, dtype=BF16)
    call("sed_cg_pool_bwd", t["dout"], t["Y"], l.ldy, t["a"], t["b"], t["L"], l.ldy, t["mask"] if masked else None, scale, dzd, l.ldy, dL16, l.ldg,
         B, l.H, l.W, co, l.ph, l.pw)
    (z64, l64), (z32, l32) = X.cg_pool_bwd_ref(d["dout"], *args, *geo, F64), X.cg_pool_bwd_ref(d["dout"], *args, *geo, F32)
    check(f"{tag} cg_pool_bwd dzd", dzd[:, :co], z64, z32)
    check(f"{tag} cg_pool_bwd dL16 (bf16, ldl16 {l.ldg})", dL16[:, :co], l64, l32, "bf16")
    assert exactly_zero(dzd[:, co:]) and exactly_zero(dL16[:, co:])


# ================================================================================================ A. the 16-filter fused path
@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("ldy", [16, 64])
@pytest.mark.parametrize("i", [0, 1])
def test_fused16_gate_pool_and_its_backward(i, ldy, masked):
    """sed_cg_gate16_pool (out32, the f16 image with zeros from 16 to Cpo = 64, side outputs L and Z) and sed_cg_gate16_pool_bwd (dz, dL16,
    the BatchNorm backward sums) at layer 0 (pooling (2,2)) and layer 1 ((1,1)), Y at pitch 16 and at pitch 64 with NaN in the pitch.
    Measured on an MI355X, worst error / bound: out32 0.13, out16 0.995, L 0.13, Z 0.997, dz 0.25, dL16 0.998, s1 / s2 0.023."""
    l, d = LAYERS[i], X.fused16_inputs(i)
    M, Mo = d["M"], d["Mo"]
    t = on_dev(d)
    Y = pitched(d["Y"], ldy)
    mask, scale = (d["mask"], DROP_SCALE) if masked else (None, 1.0)
    mdev = t["mask"] if masked else None
    geo = (B, l.H, l.W, l.ph, l.pw)
    tag = f"A fused16 layer {i} ldy {ldy} {'mask' if masked else 'no mask'}"
    L, Z, out16, out32 = nans(M, 16), nans(M, 16, dtype=F16), nans(Mo, l.Cp, dtype=F16), nans(Mo, 16)
    call("sed_cg_gate16_pool", Y, ldy, t["a"], t["b"], t["Wg"], t["bg"], mdev, scale, L, Z, out16, out32, *geo[:3], l.Cp, l.ph, l.pw, 1)
    fa = (d["Y"], d["a"], d["b"], d["Wg"], d["bg"], mask, scale)
    r64, r32 = X.gate16_fwd_ref(*fa, *geo, F64), X.gate16_fwd_ref(*fa, *geo, F32)
    check(f"{tag} out32", out32, r64["out"], r32["out"])
    check(f"{tag} out16 (f16)", out16[:, :16], r64["out"], r32["out"], "f16")
    assert exactly_zero(out16[:, 16:])
    check(f"{tag} L", L, r64["l"], r32["l"])
    check(f"{tag} Z (f16)", Z, r64["z"], r32["z"], "f16")
    o16, o32 = nans(Mo, l.Cp, dtype=F16), nans(Mo, 16)
    call("sed_cg_gate16_pool", Y, ldy, t["a"], t["b"], t["Wg"], t["bg"], mdev, scale, None, None, o16, o32, *geo[:3], l.Cp, l.ph, l.pw, 1)
    assert torch.equal(o32, out32) and torch.equal(o16, out16), "the side outputs change no bit of the result"
    # backward from the logits the forward saved
    Lh = L.cpu()
    ba = (d["dout"], d["Y"], d["a"], d["b"], Lh, d["Wg"], mask, scale)
    (z64, l64), (z32, l32) = X.gate16_bwd_ref(*ba, *geo, F64), X.gate16_bwd_ref(*ba, *geo, F32)
    dz, dL16, s1, s2 = nans(M, 16), nans(M, 16, dtype=BF16), zeros(16), zeros(16)
    call("sed_cg_gate16_pool_bwd", t["dout"], Y, ldy, t["a"], t["b"], L, t["Wg"], mdev, scale, dz, dL16, *geo, t["ah"], t["bh"], s1, s2)
    check(f"{tag} bwd dz", dz, z64, z32)
    check(f"{tag} bwd dL16 (bf16)", dL16, l64, l32, "bf16")
    _, blocks, _, trips = X.gate16_bwd_launch(B, l.H, l.W)
    t1, t2 = X.stats_terms(z64, d["Y"], d["ah"], d["bh"])
    check_sum(f"{tag} bwd s1", s1, t1, X.d_wave_reduce(trips, blocks))
    check_sum(f"{tag} bwd s2", s2, t2, X.d_wave_reduce(trips, blocks))
    dz2, dL2 = nans(M, 16), nans(M, 16, dtype=BF16)
    call("sed_cg_gate16_pool_bwd", t["dout"], Y, ldy, t["a"], t["b"], L, t["Wg"], mdev, scale, dz2, dL2, *geo, None, None, None, None)
    assert torch.equal(dz2, dz) and torch.equal(X.bits(dL2), X.bits(dL16))


def conv0_case(tag, d, Bc, T, ldys):
    """sed_conv0_fwd16 with and without sums, sed_conv0_dw16 at the given pitches of dY with ldw = 64."""
    t = on_dev(d)
    M = Bc * T * 128
    Y, s1, s2 = nans(M, 16), zeros(16), zeros(16)
    call("sed_conv0_fwd16", t["mel"], t["Wc"], t["bias"], Y, Bc, T, s1, s2)
    r64, r32 = X.conv0_ref(d["mel"], d["Wc"], d["bias"], F64), X.conv0_ref(d["mel"], d["Wc"], d["bias"], F32)
    check(f"{tag} conv0_fwd16 Y", Y, r64, r32)
    _, blocks, _, trips = X.conv0_fwd16_launch(Bc, T)
    check_sum(f"{tag} conv0_fwd16 s1", s1, r64, X.d_wave_reduce(trips, blocks))
    check_sum(f"{tag} conv0_fwd16 s2", s2, r64 * r64, X.d_wave_reduce(trips, blocks))
    Y2 = nans(M, 16)
    call("sed_conv0_fwd16", t["mel"], t["Wc"], t["bias"], Y2, Bc, T, None, None)
    assert torch.equal(Y2, Y)
    dY, p = d["dY"].double(), X.conv0_patches(d["mel"], F64)
    for ldy in ldys:
        dW = torch.full((16, 64), 7.0, device=DEV)
        dW[:, :9] = 0.0
        db = zeros(16)
        call("sed_conv0_dw16", pitched(d["dY"], ldy), ldy, t["mel"], dW, 64, db, Bc, T)
        dd = X.d_conv0_dw16(Bc, T)
        check_sum(f"{tag} conv0_dw16 dW (ldy {ldy})", dW[:, :9], dY[:, :, None] * p[:, None, :], dd)
        check_sum(f"{tag} conv0_dw16 dbias (ldy {ldy})", db, dY, dd)
        assert bool((dW[:, 9:] == 7.0).all()), "columns 9 .. ldw - 1 are not touched"


def test_conv0_direct_forward_and_weight_gradient_at_layer_0():
    """T = 12, B = 2 (3072 pixels: 12 workgroups of the forward, 24 slabs of the weight gradient), dY at pitch 16 and 64.
    Measured on an MI355X, worst error / bound: Y 0.12, s1 / s2 0.066, dW 0.067, dbias 0.038."""
    conv0_case("A layer 0", X.conv0_inputs(B, X.T_A), B, X.T_A, (16, 64))


# ================================================================================================ B. past one grid pass
def test_conv0_fwd16_past_the_grid_cap():
    """B = 1, T = 8193: 1 048 704 pixels on 4096 workgroups, the 128 pixels of the last frame in a second trip (their spectrogram
    frames carry 32 times the level, so that the sums see them).
    Measured on an MI355X, worst error / bound: Y 0.10, s1 0.007, s2 0.009; without the second trip the sums move by 24 / 914 bounds."""
    Bc, T = X.FWD16_B
    d = X.fwd16_b_inputs()
    t = on_dev(d)
    work, blocks, first, trips = X.conv0_fwd16_launch(Bc, T)
    assert trips == 2
    tag = f"B conv0_fwd16 T={T} ({work} pixels, {work - first} past the first pass)"
    Y, s1, s2 = nans(work, 16), zeros(16), zeros(16)
    call("sed_conv0_fwd16", t["mel"], t["Wc"], t["bias"], Y, Bc, T, s1, s2)
    r64, r32 = X.conv0_ref(d["mel"], d["Wc"], d["bias"], F64), X.conv0_ref(d["mel"], d["Wc"], d["bias"], F32)
    check(f"{tag} Y", Y, r64, r32)
    check_sum(f"{tag} s1", s1, r64, X.d_wave_reduce(trips, blocks), first)
    check_sum(f"{tag} s2", s2, r64 * r64, X.d_wave_reduce(trips, blocks), first)
    Y2 = nans(work, 16)
    call("sed_conv0_fwd16", t["mel"], t["Wc"], t["bias"], Y2, Bc, T, None, None)
    assert torch.equal(Y2, Y)


def test_conv0_dw16_past_one_trip():
    """B = 1, T = 1025: 256 rows per workgroup (two trips of 128), 513 slabs, the last one half full.
    Measured on an MI355X, worst error / bound: dW 0.020, dbias 0.020; without the last slab the sums move by 27 / 30 bounds."""
    Bc, T = X.DW16_B
    d = X.dw16_b_inputs()
    rows, slabs, trips, last = X.conv0_dw16_launch(Bc, T)
    assert trips == 2 and last < rows
    dY, p = d["dY"].double(), X.conv0_patches(d["mel"], F64)
    dW = torch.full((16, 64), 7.0, device=DEV)
    dW[:, :9] = 0.0
    db = zeros(16)
    call("sed_conv0_dw16", d["dY"].to(DEV), 16, d["mel"].to(DEV), dW, 64, db, Bc, T)
    tag = f"B conv0_dw16 T={T} ({slabs} slabs of {rows}, last {last})"
    check_sum(f"{tag} dW", dW[:, :9], dY[:, :, None] * p[:, None, :], X.d_conv0_dw16(Bc, T), (slabs - 1) * rows)
    check_sum(f"{tag} dbias", db, dY, X.d_conv0_dw16(Bc, T), (slabs - 1) * rows)
    assert bool((dW[:, 9:] == 7.0).all())


def test_cg_gate16_pool_bwd_past_the_grid_cap():
    """Layer-0 geometry, B = 1, H = 8194: 1 048 832 pixels on 4096 workgroups, the last two rows in a second trip (their output
    gradient carries 64 times the level).  Measured on an MI355X, worst error / bound: dz 0.23, dL16 0.999, s1 0.006, s2 0.010; without
    the second trip the sums move by 66 bounds."""
    Bc, H, W, ph, pw = X.GATE16_BWD_B
    d = X.gate16_bwd_b_inputs()
    t = on_dev(d)
    work, blocks, first, trips = X.gate16_bwd_launch(Bc, H, W)
    assert trips == 2
    tag = f"B cg_gate16_pool_bwd H={H} ({work} pixels, {work - first} past the first pass)"
    dz, dL16, s1, s2 = nans(work, 16), nans(work, 16, dtype=BF16), zeros(16), zeros(16)
    call("sed_cg_gate16_pool_bwd", t["dout"], t["Y"], 16, t["a"], t["b"], t["L"], t["Wg"], t["mask"], DROP_SCALE, dz, dL16, Bc, H, W, ph, pw,
         t["ah"], t["bh"], s1, s2)
    ba = (d["dout"], d["Y"], d["a"], d["b"], d["L"], d["Wg"], d["mask"], DROP_SCALE, Bc, H, W, ph, pw)
    (z64, l64), (z32, l32) = X.gate16_bwd_ref(*ba, F64), X.gate16_bwd_ref(*ba, F32)
    check(f"{tag} dz", dz, z64, z32)
    check(f"{tag} dL16 (bf16)", dL16, l64, l32, "bf16")
    t1, t2 = X.stats_terms(z64, d["Y"], d["ah"], d["bh"])
    check_sum(f"{tag} s1", s1, t1, X.d_wave_reduce(trips, blocks), first)
    check_sum(f"{tag} s2", s2, t2, X.d_wave_reduce(trips, blocks), first)


def test_bn_act_and_bn_bwd_past_the_grid_cap():
    """Layer-2 widths (C 32, pitch 64), M = 262 145: 4 194 320 items on 16 384 workgroups, 16 in a second trip.
    Measured on an MI355X, worst error / bound: Z 0.998, dY 0.999."""
    d = X.bn_b_inputs()
    t = on_dev(d)
    M, C, P = X.BN_B["M"], X.BN_B["C"], X.BN_B["pitch"]
    assert X.bn_act_launch(M, P)[3] == 2 and X.bn_bwd_launch(M, P)[3] == 2
    Z = nans(M, P, dtype=F16)
    call("sed_bn_act", t["Y"], C, t["a"], t["b"], Z, M, C, P, 1)
    check(f"B bn_act M={M} Z (f16)", Z[:, :C], X.bn_act_ref(d["Y"], d["a"], d["b"], F64), X.bn_act_ref(d["Y"], d["a"], d["b"], F32), "f16")
    assert exactly_zero(Z[:, C:])
    args = (d["dz"], d["Y"], d["ah"], d["bh"], d["gamma"], d["s1"], d["s2"])
    dY = nans(M, P, dtype=BF16)
    call("sed_bn_bwd", t["dz"], C, t["Y"], C, t["ah"], t["bh"], t["gamma"], t["s1"], t["s2"], dY, P, M, C)
    check(f"B bn_bwd M={M} dY (bf16)", dY[:, :C], X.bn_bwd_ref(*args, F64), X.bn_bwd_ref(*args, F32), "bf16")
    assert exactly_zero(dY[:, C:])


def test_cg_pool_past_the_grid_cap():
    """Layer-2 geometry (C 32, Cpo 64, W 64, (2,2)), B = 1, H = 16 386: 4 194 816 items, the last output row in a second trip.
    Measured on an MI355X, worst error / bound: out32 0.10, out16 0.995."""
    c = X.CG_POOL_B
    geo = (c["B"], c["H"], c["W"], c["ph"], c["pw"])
    d = X.cg_inputs(*geo, c["C"], c["C"], 7600)
    t = on_dev(d)
    assert X.cg_pool_launch(c["B"], c["H"], c["W"], c["Cpo"], c["ph"], c["pw"])[3] == 2
    Mo = d["dout"].shape[0]
    out16, out32 = nans(Mo, c["Cpo"], dtype=F16), nans(Mo, c["C"])
    call("sed_cg_pool", t["Y"], c["C"], t["a"], t["b"], t["L"], c["C"], t["mask"], DROP_SCALE, out16, out32, c["B"], c["H"], c["W"], c["C"], c["Cpo"],
         c["ph"], c["pw"], 1)
    args = (d["Y"], d["a"], d["b"], d["L"], d["mask"], DROP_SCALE)
    r64, r32 = X.cg_pool_ref(*args, *geo, F64), X.cg_pool_ref(*args, *geo, F32)
    check(f"B cg_pool H={c['H']} out32", out32, r64, r32)
    check(f"B cg_pool H={c['H']} out16 (f16)", out16[:, :c["C"]], r64, r32, "f16")
    assert exactly_zero(out16[:, c["C"]:])


def test_cg_pool_bwd_past_the_grid_cap():
    """Layer-4 geometry (C 64, W 32, (1,2), ldl16 64), B = 1, H = 8193: 4 194 816 items, the last row in a second trip.
    Measured on an MI355X, worst error / bound: dzd 0.13, dL16 0.999."""
    c = X.CG_POOL_BWD_B
    geo = (c["B"], c["H"], c["W"], c["ph"], c["pw"])
    d = X.cg_inputs(*geo, c["C"], c["C"], 7700)
    t = on_dev(d)
    assert X.cg_pool_bwd_launch(c["B"], c["H"], c["W"], c["ldg"])[3] == 2
    M = d["Y"].shape[0]
    dzd, dL16 = nans(M, c["C"]), nans(M, c["ldg"], dtype=BF16)
    call("sed_cg_pool_bwd", t["dout"], t["Y"], c["C"], t["a"], t["b"], t["L"], c["C"], t["mask"], DROP_SCALE, dzd, c["C"], dL16, c["ldg"], c["B"],
         c["H"], c["W"], c["C"], c["ph"], c["pw"])
    args = (d["dout"], d["Y"], d["a"], d["b"], d["L"], d["mask"], DROP_SCALE)
    (z64, l64), (z32, l32) = X.cg_pool_bwd_ref(*args, *geo, F64), X.cg_pool_bwd_ref(*args, *geo, F32)
    check(f"B cg_pool_bwd H={c['H']} dzd", dzd, z64, z32)
    check(f"B cg_pool_bwd H={c['H']} dL16 (bf16)", dL16[:, :c["C"]], l64, l32, "bf16")
    assert exactly_zero(dL16[:, c["C"]:])


def test_im2col_past_the_grid_cap():
    """Layer-1 geometry (cin 16, Kp 256, W 64), B = 1, H = 2049: 4 196 352 chunks, the last row's 2048 in a second trip.
    Measured on an MI355X: bit-equal."""
    c = X.IM2COL_B
    M = c["B"] * c["H"] * c["W"]
    assert X.im2col_launch(M, c["Kp"])[3] == 2
    g = torch.Generator(device=DEV).manual_seed(7800)
    Xd = nans(c["B"], c["H"], c["W"], c["Cp"], dtype=F16)
    Xd[..., :c["C"]] = torch.randn(c["B"], c["H"], c["W"], c["C"], generator=g, device=DEV).to(F16)
    col = nans(M, c["Kp"], dtype=F16)
    call("sed_conv3x3_im2col", Xd, col, c["B"], c["H"], c["W"], c["C"], c["Cp"], c["Kp"])
    same_bits(f"B im2col H={c['H']} ({M} pixels)", col, X.im2col_ref(X.bits(Xd), c["B"], c["H"], c["W"], c["C"], c["Kp"]))
    assert bool((X.bits(col)[:, 9 * c["C"]:] == 0).all())


def test_col2im_past_the_grid_cap():
    """Layer-9 geometry (C 256, Kp 2304, W 1), B = 1, H = 65 537: 4 194 368 items, 64 in a second trip; dcol is 302 MB.
    Measured on an MI355X: bit-equal to the fp32 sum in tap order."""
    c = X.COL2IM_B
    M = c["B"] * c["H"] * c["W"]
    assert X.col2im_launch(M, c["C"])[3] == 2
    g = torch.Generator(device=DEV).manual_seed(7900)
    dcol = torch.empty(M, c["Kp"], dtype=BF16, device=DEV)
    for k0 in range(0, c["Kp"], 256):      # (in slices: no 604 MB fp32 temporary)
        dcol[:, k0:k0 + 256] = (0.5 * torch.randn(M, 256, generator=g, device=DEV)).to(BF16)
    dX = nans(M, c["C"])
    call("sed_col2im3x3", dcol, c["Kp"], dX, c["B"], c["H"], c["W"], c["C"])
    ok = torch.equal(dX, X.col2im_ref(dcol, c["B"], c["H"], c["W"], c["C"]))
    log(f"B col2im H={c['H']} ({M} pixels): {'bit-equal' if ok else 'DIFFERS'} to the fp32 sum in tap order")
    assert ok and not bool(torch.isnan(dX).any())


def test_colstats_past_the_slab_cap():
    """C = 128, M = 135 171: 2048 slabs of four rows per iteration, a 17th trip of 4099 rows (M is no multiple of 4).
    Measured on an MI355X, worst error / bound: 0.011 .. 0.020; without the 17th trip the sums move by 207 .. 257 bounds."""
    M, C = X.COLSTATS_B["M"], X.COLSTATS_B["C"]
    d = X.colstats_b_inputs()
    t = on_dev(d)
    rpi, _, slabs, trips = X.colstats_launch(M, C)
    assert slabs == 2048 and trips == 17
    dd, lt = X.d_colstats(M, C), (trips - 1) * slabs * rpi
    s1, s2 = zeros(C), zeros(C)
    call("sed_colstats", t["A"], C, None, 0, None, None, s1, s2, M, C, 0)
    t1, t2 = X.stats_terms(d["A"])
    check_sum(f"B colstats M={M} mode 0 s1", s1, t1, dd, lt)
    check_sum(f"B colstats M={M} mode 0 s2", s2, t2, dd, lt)
    s1, s2 = zeros(C), zeros(C)
    call("sed_colstats", t["A"], C, t["Bm"], C, t["a"], t["b"], s1, s2, M, C, 1)
    t1, t2 = X.stats_terms(d["A"], d["Bm"], d["a"], d["b"])
    check_sum(f"B colstats M={M} mode 1 s1", s1, t1, dd, lt)
    check_sum(f"B colstats M={M} mode 1 s2", s2, t2, dd, lt)


@pytest.mark.parametrize("C,in_f16", X.TN_CASES)
def test_transpose_narrow_past_the_block_cap(C, in_f16):
    """R = 524 325, Rpad = 524 352: 2048 workgroups, rows 524 288 .. in a second trip (37 of the matrix, 27 of zero padding), input
    pitch 64 with NaN in the pitch.  The image is bit-equal to bf16(float(in)); measured on an MI355X, worst error / bound of the column
    sums: 0.008 .. 0.011; without the second trip they move by 69 .. 94 bounds."""
    x = X.tn_inputs(C, in_f16)
    blocks, first, trips = X.transpose_narrow_launch(X.TN_RPAD)
    assert blocks == 2048 and trips == 2
    outT, cs = nans(C, X.TN_RPAD, dtype=BF16), zeros(C)
    call("sed_transpose_narrow", pitched(x, 64), in_f16, X.TN_R, C, 64, outT, X.TN_RPAD, cs)
    want = torch.zeros(C, X.TN_RPAD, dtype=BF16)
    want[:, :X.TN_R] = x.float().to(BF16).t()
    tag = f"B transpose_narrow C={C} in_f16={in_f16} R={X.TN_R}"
    same_bits(f"{tag} image", outT, want)
    check_sum(f"{tag} colsum", cs, x.double(), X.d_wave_reduce(trips, blocks), first)
    outT2 = nans(C, X.TN_RPAD, dtype=BF16)
    call("sed_transpose_narrow", pitched(x, 64), in_f16, X.TN_R, C, 64, outT2, X.TN_RPAD, None)
    assert torch.equal(X.bits(outT2), X.bits(outT))
