"""tests/walk_cases.py proved on the CPU, before tests/test_gpu_walk_kernels.py holds the hardware to it:

1. every case crosses the threshold it is named for, by the restated launch arithmetic -- and no case of the older tests (SHAPES of
   test_gpu_conformer.py, MIX_CASES / HEAD_CASES of fdy_cases.py, the 130 rows of the Swish test) does: that is the gap;
2. every drop condition holds: the float64 reference with one named contribution removed (the frames of one walked tile, the rows of
   the last slab, everything past the first grid pass) differs from the full one by >= 10 bounds somewhere;
3. the bounds are not vacuous.  The yardstick of the bound IS the plain fp32 torch evaluation, which therefore sits at 1/8 of it by
   construction; what is shown here is that fp32 sums in the KERNEL's order (the tile walk and its 256 partials; the frequency mean's
   thread map) stay inside as well -- and that the tile walk cut back to its first step does not;
4. the direct mixing and mean-add references agree with autograd of fdy_cases.mix and of x.mean(3) to 1e-12, and the per-frame terms of
   the Conformer sums add up to the autograd gradients;
5. every case passes the entry points' argument checks, restated as Python, and the refused sizes fail them."""
import pytest
import torch

import fdy_cases as FC
import walk_cases as X
from walk_cases import F32, F64

REL = 1e-12


def close64(a, b):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= REL * max(float(b.abs().max()), 1e-300), float((a - b).abs().max())


# ------------------------------------------------------------------------------------------------ 1. thresholds
def test_conformer_cases_walk_and_the_older_shapes_do_not():
    for B, T in X.CONV_SHAPES_TESTED:
        ntiles, nwg, steps = X.conv_walk(B, T)
        assert steps == 1 and nwg == ntiles <= X.BWD_MAX_WG, (B, T)
    assert X.conv_walk(2, 1000) == (100, 100, 1) and X.conv_walk(32, 1000) == (1600, 256, 7)
    assert X.conv_walk(7, 1010) == (357, 256, 2) and X.conv_walk(27, 390) == (540, 256, 3)
    # (7, 1010): workgroups 0-100 take two steps; workgroup 50 walks clip 0's ragged 10-frame tile, then clip 6's first tile
    assert [len(X.conv_wg_tiles(7, 1010, g)) for g in (0, 100, 101, 255)] == [2, 2, 1, 1]
    assert [X.conv_tile(7, 1010, t) for t in X.conv_wg_tiles(7, 1010, 50)] == [(0, 1000, 10), (6, 0, 20)]
    # (27, 390): three steps for workgroups 0-27, two for the rest; every clip ends in a ragged tile; workgroups change clip mid-walk
    assert [len(X.conv_wg_tiles(27, 390, g)) for g in (0, 27, 28, 255)] == [3, 3, 2, 2]
    assert X.conv_tile(27, 390, 19) == (0, 380, 10) and X.conv_tile(27, 390, 539) == (26, 380, 10)
    for B, T in X.CONV_WALK_SHAPES:
        ntiles, nwg, steps = X.conv_walk(B, T)
        assert steps >= 2 and nwg == X.BWD_MAX_WG
        walked = sorted(t for g in range(nwg) for t in X.conv_wg_tiles(B, T, g))
        assert walked == list(range(ntiles))                                              # every tile once
        assert sum(X.conv_tile(B, T, t)[2] for t in walked) == B * T                      # every frame once
        assert any(len({X.conv_tile(B, T, t)[0] for t in X.conv_wg_tiles(B, T, g)}) > 1 for g in range(nwg))
        assert any(X.conv_tile(B, T, ts[0])[2] < X.TT and len(ts) > 1 for ts in (X.conv_wg_tiles(B, T, g) for g in range(nwg)))
        names = X.conv_drop_tiles(B, T)
        assert "ragged first-step tile" in names and names["first tile of step 2"] == 256 and names["last tile"] == ntiles - 1
    assert X.conv_drop_tiles(7, 1010)["ragged first-step tile"] == 50


def test_fdy_cases_cross_their_thresholds_and_the_older_cases_do_not():
    # slabs of dW1
    for B, H, W, cin in FC.HEAD_CASES:
        assert X.fdy_slabs(B * H)[0] < 32
        assert X.fdy_grid_items(X.mean_add_items(B * H, W, cin))[2] == 1
        assert X.freq_mean_map(cin)[2] == 0 and cin in X.FREQ_WIDTHS_TESTED
    assert max(X.fdy_slabs(B * H)[0] for B, H, _, _ in FC.HEAD_CASES) == 7
    assert X.fdy_slabs(4095)[0] == 31 and 4223 // 128 == 32 and 4224 // 128 == 33 and X.fdy_slabs(4224)[0] == 32      # the cap bites from R = 4224
    assert X.fdy_slabs(12000) == (32, 375)
    for B, H, W, cin in X.HEAD_WALK_CASES:
        R = B * H
        nslab, rows_per = X.fdy_slabs(R)
        assert nslab == 32 and R // 128 > 32
        assert any((s * rows_per) % H for s in range(1, nslab)), "slab edges fall inside clips"
        assert 0 < R - (nslab - 1) * rows_per < rows_per, "the last slab is short"
    assert X.fdy_slabs(4500) == (32, 141) and 4500 - 31 * 141 == 129
    # grid cap of the mixing forward and of the mean's backward
    for B, H, W, co in FC.MIX_CASES:
        assert X.fdy_grid_items(X.mix_items(B * H * W, X.mix_layout(co)[1]))[2] == 1
    assert max(X.mix_items(B * H * W, X.mix_layout(co)[1]) for B, H, W, co in FC.MIX_CASES) < 0.3e6
    first = X.FDY_CAP * 256
    assert first == 4194304
    for c, items in zip(X.MIX_WALK_CASES, (4198400, 10240000)):
        work = X.mix_items(c.B * c.H * c.W, c.ldy)
        blocks, fp, passes = X.fdy_grid_items(work)
        assert work == items and blocks == X.FDY_CAP and fp == first and passes == X.cdiv(items, first) >= 2
        assert (c.ld4, c.ldy) == (64, 64) and c.ldy > c.co, "padding columns exist"
        assert X.mix_late_rows(c) == first // 16 < c.B * c.H * c.W
    c = X.MEAN_WALK_CASES[0]
    assert X.mean_add_items(c.R, c.W, c.C) == 4198400 and X.fdy_grid_items(4198400)[2] == 2 and c.W & (c.W - 1) == 0
    assert X.MEAN_WALK_CASES[1].W & (X.MEAN_WALK_CASES[1].W - 1), "and one width whose reciprocal is not exact"
    # thread map of the frequency mean
    assert [X.freq_mean_map(w) for w in (8, 24, 384)] == [(1, 256, 0), (3, 85, 1), (48, 5, 16)]
    for w in (8, 24, 384):
        assert w not in X.FREQ_WIDTHS_TESTED
        wl = X.freq_mean_map(w)[1]
        ws = sorted(c.W for c in X.FREQ_CASES if c.C == w)
        assert len(ws) == 2 and ws[0] < wl < ws[1], (w, wl, ws)
    assert all(c.Cp > c.C for c in X.FREQ_CASES)
    assert sum(1 for c in X.FREQ_CASES if X.freq_mean_map(c.C)[2] > 0) == 4
    # elementwise kernels
    assert X.elem_blocks(X.ELEM_N_TESTED)[2] == 1 and X.elem_blocks(X.ELEM_N_TESTED)[0] < 65536
    blocks, fp, passes = X.elem_blocks(X.ELEM_N)
    assert (blocks, fp, passes) == (65536, 67108864, 2) and X.ELEM_N - fp == 1200
    w = X.elem_windows()
    assert w[1].start < fp < w[1].stop and w[0].start == 0 and w[2].stop == X.ELEM_N and all(s.stop - s.start == X.ELEM_WIN for s in w)


# ------------------------------------------------------------------------------------------------ 2. - 4. Conformer
@pytest.mark.parametrize("B,T", X.CONV_WALK_SHAPES)
def test_conformer_terms_drops_and_the_walk_in_fp32(B, T):
    terms, refs = X.conv_terms(B, T), X.conv_sum_refs(B, T)
    for k in X.CONV_SUMS:                                                                 # 4. the terms are the gradients' terms
        close64(terms[k].sum(0), refs[k][0])
    for (nm, k), ratio in X.conv_drop_ratios(B, T).items():                               # 2.
        print(f"B={B} T={T} {k} without the {nm}: {ratio:.3e} bounds")
        assert ratio >= X.SENS, (nm, k, ratio)
    for k in X.CONV_SUMS:                                                                 # 3.
        ref, bound = refs[k]
        full = float((X.conv_walk_emulated(terms[k], B, T).double() - ref).abs().max())
        cut = float((X.conv_walk_emulated(terms[k], B, T, walk=False).double() - ref).abs().max())
        print(f"B={B} T={T} {k} fp32 in the kernel's order: {full / (bound / 8):.2f} yardsticks; first step only: {cut / bound:.3e} bounds")
        assert full <= bound, (k, full, bound)
        assert cut >= X.SENS * bound, (k, "a walk that stops after its first step would pass", cut, bound)
    assert X.conv_args_ok(B, T, X.C, X.conv_partial_floats(B, T))                         # 5.
    assert not X.conv_args_ok(B, T, X.C, X.conv_partial_floats(B, T) - 1)
    assert X.conv_partial_floats(B, T) == 256 * 34 * 768


# ------------------------------------------------------------------------------------------------ FDY head
@pytest.mark.parametrize("B,H,W,cin", X.HEAD_WALK_CASES)
def test_head_last_slab_is_seen_by_every_gradient(B, H, W, cin):
    for k, ratio in X.head_drop_ratios(B, H, W, cin).items():
        print(f"head B{B} H{H} cin{cin}: grad {k} without the last slab's rows: {ratio:.3e} bounds")
        assert ratio >= X.SENS, (k, ratio)
    hid, R = FC.hid_of(cin), B * H
    need = X.head_ws_floats(R, cin, hid)
    assert need == (6 * hid + 4 + 3) // 4 * 4 + 32 * 3 * hid * cin
    for train in (True, False):
        assert X.head_args_ok(B, H, cin, hid, X.HEAD_WALK_T, need, train) and not X.head_args_ok(B, H, cin, hid, X.HEAD_WALK_T, need - 1, train)
    _, r64, _ = X.head_case(B, H, W, cin, False)
    assert float(r64["att"].min()) < 0.2 and float(r64["att"].max()) > 0.3, "the case exercises the softmax"


# ------------------------------------------------------------------------------------------------ frequency mean
@pytest.mark.parametrize("c", X.FREQ_CASES, ids=lambda c: f"C{c.C}-W{c.W}")
def test_freq_mean_thread_map_in_fp32(c):
    x = X.freq_inputs(c)
    assert torch.equal(x.half().float(), x) and torch.equal(x.bfloat16().float(), x)
    r64, r32 = X.freq_refs(x)
    err, yard, worst, ok, _ = X.judge(X.freq_mean_emulated(x), r64, r32)
    print(f"freq mean C{c.C} W{c.W}: fp32 in the kernel's order err {err:.3e} yardstick {yard:.3e} worst err / bound {worst:.3f}")
    assert ok and X.freq_args_ok(c)
    # a thread group left out (the last bin in flight) moves the mean by >= 10 bounds
    _, wl, _ = X.freq_mean_map(c.C)
    last = (min(c.W, wl) - 1)
    drop = x[:, last::wl].double().sum(1) / c.W
    assert float(drop.abs().max()) >= X.SENS * max(8 * yard, 1e-300) or yard == 0.0


# ------------------------------------------------------------------------------------------------ mixing, mean-add
def test_direct_references_are_autograd_of_the_restatement():
    B, H, W, co = 2, 5, 3, 8
    g = torch.Generator().manual_seed(1)
    y4, att = torch.randn(B * H * W, 4 * co, generator=g), torch.softmax(torch.randn(B * H, 4, generator=g), -1)
    y4n = y4.double().view(B, H, W, 4 * co).permute(0, 3, 1, 2).contiguous()
    an = att.double().view(B, H, 4).permute(0, 2, 1).contiguous()
    close64(X.mix_direct(y4, att, W, co, F64), FC.mix(y4n, an).permute(0, 2, 3, 1).reshape(-1, co))
    # d/dx of sum(x.mean(3) dpm) is dpm / W on every bin
    cin = 8
    x = torch.randn(B, cin, H, W, generator=g, dtype=F64, requires_grad=True)
    dpm, dx0 = torch.randn(B * H, cin, generator=g), torch.randn(B * H, W, cin, generator=g)
    (x.mean(3).permute(0, 2, 1).reshape(-1, cin) * dpm.double()).sum().backward()
    close64(X.mean_add_direct(dx0, dpm, W, F64), dx0.double() + x.grad.permute(0, 2, 3, 1).reshape(B * H, W, cin))
    # Swish'
    h = torch.randn(64, generator=g, dtype=F64, requires_grad=True)
    dy = torch.randn(64, generator=g)
    (h * torch.sigmoid(h) * dy.double()).sum().backward()
    close64(X.swish_bwd_direct(dy, h.detach(), F64), h.grad)


@pytest.mark.parametrize("c", X.MIX_WALK_CASES, ids=lambda c: f"B{c.B}-H{c.H}")
def test_mix_rows_past_the_first_pass_are_seen(c):
    y4, att = X.mix_walk_inputs(c)
    r64, r32 = X.mix_direct(y4, att, c.W, c.co, F64), X.mix_direct(y4, att, c.W, c.co, F32)
    bound = X.bound32(r64, r32)
    late = float(r64[X.mix_late_rows(c):].abs().max())
    print(f"mix B{c.B} H{c.H}: max|ref| past the first pass {late:.3e} = {late / bound:.3e} bounds")
    assert late >= X.SENS * bound and X.mix_args_ok(c)


@pytest.mark.parametrize("c", X.MEAN_WALK_CASES, ids=lambda c: f"W{c.W}")
def test_mean_add_inputs(c):
    dx0, dpm = X.mean_walk_inputs(c)
    assert torch.equal(dpm * 64, (dpm * 64).round()) and float(dpm.abs().max()) <= 4.0 and X.mean_args_ok(c)
    r64, r32 = X.mean_add_direct(dx0, dpm, c.W, F64), X.mean_add_direct(dx0, dpm, c.W, F32)
    if c.exact:      # dpm / W is exact, so the sum is rounded once: fp32 is the correctly rounded float64 value
        assert torch.equal(r32, r64.float())
    # rows past the first grid pass carry a dpm / W no rounding of dX0 hides: leaving the second pass out changes bits
    first_rows = X.cdiv(X.fdy_grid_items(X.mean_add_items(c.R, c.W, c.C))[1], c.W * c.C // 4)
    if c.exact:
        assert first_rows < c.R and not torch.equal(r32[first_rows:], dx0[first_rows:])


def test_elementwise_sizes():
    assert X.elem_args_ok(X.ELEM_N) and X.elem_args_ok(X.ELEM_N_TESTED) and not X.elem_args_ok(X.ELEM_N + 1)
