"""tests/cnn_cases.py proved on the CPU, before tests/test_gpu_cnn_kernels.py holds the hardware to it:

1. the ten layers of part A have the geometry of the real stack, and reach what the one-layer test of test_gpu_pmam_kernels.py
   (640 pixels, 16 channels, Cp 64, Kp 256, pooling (2, 2)) never did;
2. every case of part B crosses the threshold it is named for by the restated launch arithmetic (blocks, trips and slabs are printed),
   the older shapes do not, and the set of items past the first pass is non-empty and smaller than one pass;
3. the references are right: the direct backward formulas are autograd of the forward restatement in float64, the tap index is
   F.unfold / F.fold / F.conv2d, the BatchNorm backward formula is autograd of batch normalisation;
4. the bounds are not vacuous: a plain fp32 sum lies inside (d + 2) 2^-24 sum|term|, and the element-wise yardstick IS the fp32 evaluation;
5. every drop condition holds: an out-of-range tap read as in range changes the bit-exact references on every layer (W = 1, W = 2 and
   H = 3 among them), ignoring the mask moves sed_cg_pool's outputs by >= 10 bounds, and the rows that only the last trip (or the last,
   half-full slab) reaches move at least one word of every atomically added sum by >= 10 bounds."""
import pytest
import torch
import torch.nn.functional as F

import cnn_cases as X
from cnn_cases import F32, F64, LAYERS

REL = 1e-12


def close64(a, b, rel=REL):
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= rel * max(float(b.abs().max()), 1e-300), float((a - b).abs().max())


# ------------------------------------------------------------------------------------------------ 1. the ten layers
def test_layers_are_the_real_stack_and_the_old_test_reached_one_of_them():
    assert [l.co for l in LAYERS] == [16, 16, 32, 32, 64, 64, 128, 128, 256, 384]
    assert [l.cin for l in LAYERS] == [1, 16, 16, 32, 32, 64, 64, 128, 128, 256]
    assert [l.H for l in LAYERS] == [12, 6, 6, 3, 3, 3, 3, 3, 3, 3]
    assert [l.W for l in LAYERS] == [128, 64, 64, 32, 32, 16, 8, 4, 2, 1]
    assert [(l.ph, l.pw) for l in LAYERS] == [(2, 2), (1, 1), (2, 2), (1, 1)] + [(1, 2)] * 5 + [(1, 1)]
    assert [l.Kp for l in LAYERS] == [64, 256, 256, 384, 384, 640, 640, 1152, 1152, 2304]
    assert [l.Cp for l in LAYERS] == [64, 64, 64, 64, 64, 64, 128, 128, 256, 384]
    assert [l.ldy for l in LAYERS] == [16, 16, 32, 32, 64, 64, 128, 128, 256, 384]
    assert [l.ldg for l in LAYERS] == [64, 64, 64, 64, 64, 64, 128, 128, 256, 384]
    assert [l.cpin for l in LAYERS] == [64, 64, 64, 64, 64, 64, 64, 128, 128, 256]
    assert [l.last for l in LAYERS] == [False] * 9 + [True]
    assert LAYERS[-1].W // LAYERS[-1].pw == 1 and all(l.H % l.ph == 0 and l.W % l.pw == 0 for l in LAYERS)
    # what test_cnn_branch_kernels_one_layer runs: layer 1's widths alone
    old = dict(co=16, Cp=64, Kp=256, pool=(2, 2), pixels=640)
    assert sum(1 for l in LAYERS if (l.co, l.Cp, l.Kp) == (old["co"], old["Cp"], old["Kp"])) == 1
    assert {X.colstats_launch(2 * l.H * l.W, l.co)[1] for l in LAYERS} == {1, 2, 4, 6}      # column groups of sed_colstats; the old test: 1
    assert all(X.colstats_args_ok(2 * l.H * l.W, l.co) for l in LAYERS) and all(256 % c == 0 for c in (16, 32))
    assert any(l.co == l.Cp for l in LAYERS) and any(l.ldg > l.co for l in LAYERS)
    for l in LAYERS:
        M = 2 * l.H * l.W
        print(f"layer {l.i}: cin {l.cin} co {l.co} H {l.H} W {l.W} pool ({l.ph}, {l.pw}) Np {l.Np} Kp {l.Kp} Cp {l.Cp} ldy {l.ldy} ldg {l.ldg}; "
              f"colstats (rpi, groups, slabs, trips) {X.colstats_launch(M, l.co)}; bn_act items {X.bn_act_launch(M, l.Cp)[0]}")


# ------------------------------------------------------------------------------------------------ 2. thresholds of part B
def elementwise(name, launch, cap, ragged):
    """Prints the launch and asserts: the cap is reached, a second trip exists, the items past the first pass are fewer than one pass.
    ragged: the item count leaves the last workgroup partly idle.  (Where W times the items of a pixel is a multiple of 256, as for
    the W = 128 / 64 / 32 geometries of the issue's table, no H can make the count ragged: asserted as such.)"""
    work, blocks, first, trips = launch
    print(f"{name}: {work} items on {blocks} workgroups, first pass {first}, {trips} trips, {work - first} items past the first pass, "
          f"last workgroup {'partly idle' if work % 256 else 'full'}")
    assert blocks == cap and trips == 2 and 0 < work - first < first, name
    assert (work % 256 != 0) == ragged, name
    return work - first


def test_part_b_cases_cross_their_thresholds_and_the_older_shapes_do_not():
    # the older tests: 640 pixels of 16 channels; conv0 at B, T = 2, 203
    assert X.passes(640 * 16, X.CAP)[2] == 1 and X.passes(640 * 32, X.CAP)[2] == 1 and X.colstats_launch(640, 16)[2:] == (3, 14)
    assert X.conv0_fwd16_launch(2, 203)[3] == 1 and X.conv0_dw16_launch(2, 203) == (128, 406, 1, 128)
    assert X.transpose_narrow_launch(704) == (3, 768, 1)
    # the production batch crosses them all (the gap)
    assert X.conv0_fwd16_launch(24, 1000)[3] == 3 and X.conv0_dw16_launch(24, 1000)[0] == 3072
    assert X.bn_act_launch(24 * 500 * 64, 64)[3] == 3
    B, T = X.FWD16_B
    assert elementwise("sed_conv0_fwd16", X.conv0_fwd16_launch(B, T), X.CAP_FUSED, True) == 128
    assert X.conv0_fwd16_launch(B, T - 1)[3] == 1, "the smallest T"
    rows, slabs, trips, last = X.conv0_dw16_launch(*X.DW16_B)
    print(f"sed_conv0_dw16: {rows} rows per workgroup, {slabs} slabs, {trips} trips, last slab {last} rows")
    assert (rows, slabs, trips, last) == (256, 513, 2, 128) and X.conv0_dw16_launch(1, 1024)[0] == 128
    B, H, W, ph, pw = X.GATE16_BWD_B
    assert elementwise("sed_cg_gate16_pool_bwd", X.gate16_bwd_launch(B, H, W), X.CAP_FUSED, False) == 2 * W
    assert X.gate16_bwd_launch(B, H - 2, W)[3] == 1
    # sed_cg_gate16_pool itself: its cap of 16384 x 256 OUTPUT pixels is first reached at layer 1 above batch 131 (left out on purpose)
    assert X.gate16_pool_launch(131, 500, 64, 1, 1)[3] == 1 and X.gate16_pool_launch(132, 500, 64, 1, 1)[3] == 2
    assert X.gate16_pool_launch(24, 1000, 128, 2, 2)[3] == 1
    M, C, P = X.BN_B["M"], X.BN_B["C"], X.BN_B["pitch"]
    assert M % 64 and M - 1 == 262144
    assert elementwise("sed_bn_act", X.bn_act_launch(M, P), X.CAP, True) == 16
    assert elementwise("sed_bn_bwd", X.bn_bwd_launch(M, P), X.CAP, True) == 16
    assert X.bn_act_launch(M - 1, P)[3] == 1
    c = X.CG_POOL_B
    assert elementwise("sed_cg_pool", X.cg_pool_launch(c["B"], c["H"], c["W"], c["Cpo"], c["ph"], c["pw"]), X.CAP, False) == 32 * 16
    assert X.cg_pool_launch(c["B"], c["H"] - 2, c["W"], c["Cpo"], c["ph"], c["pw"])[3] == 1
    c = X.CG_POOL_BWD_B
    assert elementwise("sed_cg_pool_bwd", X.cg_pool_bwd_launch(c["B"], c["H"], c["W"], c["ldg"]), X.CAP, False) == 32 * 16
    assert X.cg_pool_bwd_launch(c["B"], c["H"] - 1, c["W"], c["ldg"])[3] == 1
    c = X.IM2COL_B
    assert elementwise("sed_conv3x3_im2col", X.im2col_launch(c["B"] * c["H"] * c["W"], c["Kp"]), X.CAP, False) == 64 * 32
    assert X.im2col_launch((c["H"] - 1) * c["W"], c["Kp"])[3] == 1
    c = X.COL2IM_B
    assert elementwise("sed_col2im3x3", X.col2im_launch(c["B"] * c["H"] * c["W"], c["C"]), X.CAP, True) == 64
    assert X.col2im_launch(c["H"] - 1, c["C"])[3] == 1 and c["H"] * c["Kp"] * 2 < 303e6
    rpi, groups, slabs, trips = X.colstats_launch(X.COLSTATS_B["M"], X.COLSTATS_B["C"])
    print(f"sed_colstats: {rpi} rows per iteration, {groups} column groups, {slabs} slabs, {trips} trips")
    assert (rpi, groups, slabs, trips) == (4, 2, 2048, 17) and X.COLSTATS_B["M"] % rpi and X.COLSTATS_B["M"] - 16 * slabs * rpi == 4099
    blocks, first, trips = X.transpose_narrow_launch(X.TN_RPAD)
    print(f"sed_transpose_narrow: R {X.TN_R} Rpad {X.TN_RPAD}: {blocks} workgroups, first pass {first}, {trips} trips")
    assert (blocks, first, trips) == (2048, 524288, 2) and X.TN_RPAD == 524352 and first < X.TN_R < X.TN_RPAD and X.TN_RPAD % 64 == 0
    assert X.transpose_narrow_launch(524288)[2] == 1


# ------------------------------------------------------------------------------------------------ 3. the references
def test_direct_backward_formulas_are_autograd_of_the_forward():
    B, H, W, ph, pw, C = 2, 4, 6, 2, 3, 16
    d = X.cg_inputs(B, H, W, ph, pw, C, C, 1)
    g = X.gen(2)
    Wg, bg = X.uni(g, 16, 16, lo=-0.3, hi=0.3), X.uni(g, 16)
    for mask in (d["mask"], None):
        z = X.bn_act_ref(d["Y"], d["a"], d["b"], F64).requires_grad_(True)
        l = d["L"].double().requires_grad_(True)
        out = X.pool(z * torch.sigmoid(l) * X.keep_of(mask, X.DROP_SCALE, F64), B, H, W, ph, pw)
        close64(out, X.cg_pool_ref(d["Y"], d["a"], d["b"], d["L"], mask, X.DROP_SCALE, B, H, W, ph, pw, F64))
        (out * d["dout"].double()).sum().backward()
        dzd, dl = X.cg_pool_bwd_ref(d["dout"], d["Y"], d["a"], d["b"], d["L"], mask, X.DROP_SCALE, B, H, W, ph, pw, F64)
        close64(dzd, z.grad)
        close64(dl, l.grad)
        # the fused gate: l = Wg z + bg inside
        z = X.bn_act_ref(d["Y"], d["a"], d["b"], F64).requires_grad_(True)
        l = z @ Wg.double().t() + bg.double()
        l.retain_grad()
        out = X.pool(z * torch.sigmoid(l) * X.keep_of(mask, X.DROP_SCALE, F64), B, H, W, ph, pw)
        r = X.gate16_fwd_ref(d["Y"], d["a"], d["b"], Wg, bg, mask, X.DROP_SCALE, B, H, W, ph, pw, F64)
        close64(r["out"], out)
        close64(r["l"], l)
        (out * d["dout"].double()).sum().backward()
        dz, dl = X.gate16_bwd_ref(d["dout"], d["Y"], d["a"], d["b"], l.detach(), Wg, mask, X.DROP_SCALE, B, H, W, ph, pw, F64)
        close64(dz, z.grad)
        close64(dl, l.grad)


def test_bn_bwd_formula_is_autograd_of_batch_normalisation():
    d = X.layer_inputs(2)
    Y, dz, gamma = d["Y"].double().requires_grad_(True), d["dz"].double(), d["gamma"].double()
    mean, rstd = Y.mean(0), (Y.var(0, unbiased=False) + 1e-3).rsqrt()
    (((Y - mean) * rstd * gamma) * dz).sum().backward()
    ah, bh = rstd.detach(), (-mean * rstd).detach()
    t1, t2 = X.stats_terms(dz, Y.detach(), ah, bh)
    close64(X.bn_bwd_ref(dz, Y.detach(), ah, bh, gamma, t1.sum(0), t2.sum(0), F64), Y.grad, 1e-9)
    # ... and with the fp32 ah, bh, s1, s2 the kernel is given, to fp32 accuracy
    got = X.bn_bwd_ref(d["dz"], d["Y"], d["ah"], d["bh"], d["gamma"], d["s1"], d["s2"], F64)
    assert X.maxerr(got, Y.grad) < 1e-5 * float(Y.grad.abs().max())


@pytest.mark.parametrize("i", range(1, 10))
def test_tap_index_is_unfold_and_fold(i):
    l, d, B = LAYERS[i], X.layer_inputs(i), X.B_A
    M = d["M"]
    col = X.im2col_ref(X.bits(d["X"]), B, l.H, l.W, l.cin, l.Kp).view(torch.float16)
    x = d["X"][..., :l.cin].float().permute(0, 3, 1, 2)
    want = F.unfold(x, 3, padding=1).view(B, l.cin, 9, l.H * l.W).permute(0, 3, 2, 1).reshape(M, 9 * l.cin)
    assert torch.equal(col[:, :9 * l.cin].float(), want) and float(col[:, 9 * l.cin:].float().abs().max() if l.Kp > 9 * l.cin else 0.0) == 0.0
    dx = X.col2im_ref(d["dcol"], B, l.H, l.W, l.cin)
    fold = F.fold(d["dcol"][:, :9 * l.cin].double().view(B, l.H * l.W, 9, l.cin).permute(0, 3, 2, 1).reshape(B, l.cin * 9, l.H * l.W),
                  (l.H, l.W), 3, padding=1).permute(0, 2, 3, 1).reshape(M, l.cin)
    assert X.maxerr(dx, fold) <= 9 * X.EPS32 * float(d["dcol"][:, :9 * l.cin].float().abs().max()) * 9


def test_conv0_patches_are_conv2d():
    d = X.conv0_inputs(2, X.T_A)
    p = X.conv0_patches(d["mel"], F64)
    close64(p @ d["Wc"].double().view(16, 9).t() + d["bias"].double(), X.conv0_ref(d["mel"], d["Wc"], d["bias"], F64))
    # the weight gradient's terms add up to autograd's
    Wr, br = d["Wc"].double().requires_grad_(True), d["bias"].double().requires_grad_(True)
    y = F.conv2d(d["mel"].double().transpose(1, 2).unsqueeze(1), Wr, br, padding=1).permute(0, 2, 3, 1).reshape(-1, 16)
    (y * d["dY"].double()).sum().backward()
    dW, _, db, _ = X.conv0_dw_ref(d["dY"], d["mel"])
    close64(dW, Wr.grad.view(16, 9))
    close64(db, br.grad)


# ------------------------------------------------------------------------------------------------ 5. drops of part A
@pytest.mark.parametrize("i", range(1, 10))
def test_a_tap_read_out_of_range_changes_the_bit_exact_references(i):
    l, d, B = LAYERS[i], X.layer_inputs(i), X.B_A
    col = X.im2col_ref(X.bits(d["X"]), B, l.H, l.W, l.cin, l.Kp)
    dx = X.col2im_ref(d["dcol"], B, l.H, l.W, l.cin)
    for leak in (dict(check_w=False), dict(check_h=False)):
        # (check_w: the flat neighbour is the other end of the neighbouring row; check_h: a row of the neighbouring clip)
        n1 = int((X.im2col_ref(X.bits(d["X"]), B, l.H, l.W, l.cin, l.Kp, **leak) != col).sum())
        n2 = int((X.col2im_ref(d["dcol"], B, l.H, l.W, l.cin, **leak) != dx).sum())
        print(f"layer {i} (H {l.H}, W {l.W}) {leak}: {n1} words of col, {n2} words of dX change")
        assert n1 > 0 and n2 > 0
    assert not bool(torch.isnan(dx).any()) and not bool(torch.isnan(col.view(torch.float16)).any()), "the NaN padding is never read"


@pytest.mark.parametrize("i", range(10))
def test_ignoring_the_mask_moves_the_pooled_output(i):
    l, d, B = LAYERS[i], X.layer_inputs(i), X.B_A
    co = l.co
    args = (d["Y"][:, :co], d["a"], d["b"], d["L"][:, :co])
    geo = (B, l.H, l.W, l.ph, l.pw)
    r64, r32 = X.cg_pool_ref(*args, d["mask"], X.DROP_SCALE, *geo, F64), X.cg_pool_ref(*args, d["mask"], X.DROP_SCALE, *geo, F32)
    for nm, other in (("mask ignored, scale kept", X.cg_pool_ref(*args, None, 1.0, *geo, F64) * X.DROP_SCALE),
                      ("mask and scale ignored", X.cg_pool_ref(*args, None, 1.0, *geo, F64))):
        # f16 image: the bound of its largest element
        bound = X.bound32(r64, r32) + float(X.half_ulp(r64, "f16").max())
        ratio = X.maxerr(other, r64) / bound
        print(f"layer {i} sed_cg_pool, {nm}: reference moves by {ratio:.3e} bounds (of the f16 image)")
        assert ratio >= X.SENS
    dzd64, dl64 = X.cg_pool_bwd_ref(d["dout"], *args, d["mask"], X.DROP_SCALE, *geo, F64)
    dzd0, dl0 = X.cg_pool_bwd_ref(d["dout"], *args, None, 1.0, *geo, F64)
    dzd32, dl32 = X.cg_pool_bwd_ref(d["dout"], *args, d["mask"], X.DROP_SCALE, *geo, F32)
    assert X.maxerr(dzd0, dzd64) >= X.SENS * X.bound32(dzd64, dzd32)
    assert X.maxerr(dl0, dl64) >= X.SENS * (X.bound32(dl64, dl32) + float(X.half_ulp(dl64, "bf16").max()))


# ------------------------------------------------------------------------------------------------ 4. + 5. the sums
def sums(name, terms, d, late=None):
    """terms: {word: float64 term matrix [rows, ...]} summed over dim 0.  A plain fp32 sum lies inside the bound; without the rows from
    `late` on at least one word moves by >= SENS bounds."""
    worst = 0.0
    for k, t in terms.items():
        ref, bound = t.sum(0), X.sum_bound(d, t.abs().sum(0))
        err, ratio, ok = X.judge_sum(t.float().sum(0), ref, bound)
        print(f"{name} {k}: d = {d}, plain fp32 sum err {err:.3e} = {ratio:.3e} bounds")
        assert ok, (name, k, ratio)
        if late is not None:
            r = X.drop_ratio(t[late:].sum(0), bound)
            print(f"{name} {k} without rows {late}..{t.shape[0] - 1}: reference moves by {r:.3e} bounds")
            worst = max(worst, r)
            assert r >= X.SENS, (name, k, r)
    return worst


@pytest.mark.parametrize("i", range(10))
def test_part_a_sums_in_fp32(i):
    l, d = LAYERS[i], X.layer_inputs(i)
    M, co = d["M"], l.co
    t1, t2 = X.stats_terms(d["Y"][:, :co])
    u1, u2 = X.stats_terms(d["dz"][:, :co], d["Y"][:, :co], d["ah"], d["bh"])
    sums(f"layer {i} sed_colstats", dict(mode0_s1=t1, mode0_s2=t2, mode1_s1=u1, mode1_s2=u2), X.d_colstats(M, co))


def test_conv0_fwd16_sums_see_the_second_trip():
    B, T = X.FWD16_B
    d = X.fwd16_b_inputs()
    work, blocks, first, trips = X.conv0_fwd16_launch(B, T)
    y = X.conv0_ref(d["mel"], d["Wc"], d["bias"], F64)
    sums("sed_conv0_fwd16 B", dict(s1=y, s2=y * y), X.d_wave_reduce(trips, blocks), late=first)


def test_conv0_dw16_sums_see_the_last_half_full_slab():
    B, T = X.DW16_B
    d = X.dw16_b_inputs()
    rows, slabs, trips, last = X.conv0_dw16_launch(B, T)
    dY, p = d["dY"].double(), X.conv0_patches(d["mel"], F64)
    sums("sed_conv0_dw16 B", dict(dW=dY[:, :, None] * p[:, None, :], dbias=dY), X.d_conv0_dw16(B, T), late=(slabs - 1) * rows)
    assert B * T * 128 - (slabs - 1) * rows == last == rows // 2


def test_gate16_bwd_sums_see_the_second_trip():
    B, H, W, ph, pw = X.GATE16_BWD_B
    d = X.gate16_bwd_b_inputs()
    work, blocks, first, trips = X.gate16_bwd_launch(B, H, W)
    dz, _ = X.gate16_bwd_ref(d["dout"], d["Y"], d["a"], d["b"], d["L"], d["Wg"], d["mask"], X.DROP_SCALE, B, H, W, ph, pw, F64)
    t1, t2 = X.stats_terms(dz, d["Y"], d["ah"], d["bh"])
    # xhat > 0 and dz > 0 but for the pixels the mask dropped (only the gate Linear's share is left there): the terms barely cancel
    assert float((d["Y"] * d["ah"] + d["bh"]).min()) > 0.0 and float((t1.sum(0) / t1.abs().sum(0)).min()) > 0.9
    sums("sed_cg_gate16_pool_bwd B", dict(s1=t1, s2=t2), X.d_wave_reduce(trips, blocks), late=first)


def test_colstats_sums_see_the_17th_trip():
    M, C = X.COLSTATS_B["M"], X.COLSTATS_B["C"]
    d = X.colstats_b_inputs()
    rpi, _, slabs, trips = X.colstats_launch(M, C)
    t1, t2 = X.stats_terms(d["A"])
    u1, u2 = X.stats_terms(d["A"], d["Bm"], d["a"], d["b"])
    assert float((d["Bm"] * d["a"] + d["b"]).min()) > 0.0
    sums("sed_colstats B", dict(mode0_s1=t1, mode0_s2=t2, mode1_s1=u1, mode1_s2=u2), X.d_colstats(M, C), late=(trips - 1) * slabs * rpi)


@pytest.mark.parametrize("C,in_f16", X.TN_CASES)
def test_transpose_narrow_colsum_sees_the_second_trip(C, in_f16):
    x = X.tn_inputs(C, in_f16)
    blocks, first, trips = X.transpose_narrow_launch(X.TN_RPAD)
    sums(f"sed_transpose_narrow B C{C} f16={in_f16}", dict(colsum=x.double()), X.d_wave_reduce(trips, blocks), late=first)
    assert not bool(torch.isinf(x.float()).any())
    if in_f16:      # the image rounds a second time: f16 -> bf16
        assert not torch.equal(x.float().bfloat16().float(), x.float())
