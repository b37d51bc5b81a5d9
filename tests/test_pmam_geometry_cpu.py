"""The CNN branch's layer plan (transformer4sed_amd/pmam_engine/geometry.py: `cnn_geometry`, `cnn_layer_plans`) against the restatements
the kernel tests keep on purpose (tests/cnn_cases.py `layers`, the formulas of tests/test_gpu_fdy_cnn.py, fdy_cases.hid_of) and against
the route predicates written out literally here.  Pure integer work: no GPU, no library."""
import pytest
import torch

import cnn_cases as CC
import fdy_cases as FC
from test_weight_image_table_cpu import pmam
from transformer4sed_amd import synth
from transformer4sed_amd.pmam_engine import geometry as GEO
from transformer4sed_amd.pmam_engine.geometry import cnn_geometry, cnn_layer_plans

SHAPES = [(2, 12), (24, 1000)]
STACKS = {"pmam": (synth.PMAM_FILTERS, synth.PMAM_POOLING, None), "fdy": (synth.FDY_FILTERS, synth.FDY_POOLING, synth.FDY_DY_LAYERS)}


def walk(filters, pooling, B, T):
    """The test's own walk of the pooling: (H, W, M) per layer."""
    out, H, W = [], T, 128
    for (ph, pw) in pooling:
        out.append((H, W, B * H * W))
        H, W = H // ph, W // pw
    return out


def images(g, M, dw_tn):
    """Per weight-gradient image of a layer, restated: (name, rows, k, n_valid, k_valid, operand row width)."""
    fused16 = dw_tn and g["co"] == 16 and M >= 1024
    conv = ("conv", g["ldg4"], g["Kp"], 4 * g["co"], 9 * g["cin"], g["Kp"]) if g["dyn"] else ("conv", g["ldg"], g["Kp"], g["co"], 9 * g["cin"], g["Kp"])
    return [("gate", g["ldg"], g["Cp"], g["co"], g["co"], 16 if fused16 else g["Cp"]), conv]


@pytest.mark.parametrize("B,T", SHAPES)
def test_real_static_stack_matches_cnn_cases(B, T):
    geo = cnn_geometry(synth.PMAM_FILTERS, synth.PMAM_POOLING, None)
    plans = cnn_layer_plans(geo, synth.PMAM_POOLING, B, T, True)
    want = CC.layers(T)
    assert len(geo) == len(plans) == len(want) == 10
    for g, p, l in zip(geo, plans, want):
        got = dict(cin=g["cin"], co=g["co"], H=p.H, W=p.W, Np=g["Np"], Kp=g["Kp"], Cp=g["Cp"], ldy=p.ldy, ldg=g["ldg"], cpin=g["cpin"], last=p.last)
        assert got == {k: getattr(l, k) for k in got}, l.i
        assert (p.M, p.Ho, p.Wo) == (B * l.H * l.W, l.H // l.ph, l.W // l.pw) and not g["dyn"]
    # the next layer's channel pitch is this layer's output pitch
    assert [p.Cpo for p in plans[:-1]] == [l.cpin for l in want[1:]]


def test_fdy_stack_matches_the_kernel_tests_formulas():
    geo = cnn_geometry(synth.FDY_FILTERS, synth.FDY_POOLING, synth.FDY_DY_LAYERS)
    assert [g["dyn"] for g in geo] == [bool(d) for d in synth.FDY_DY_LAYERS]
    for g in geo:
        if not g["dyn"]:
            assert not {"Nc", "ld4", "ldg4", "hid"} & set(g)
            continue
        co = g["co"]
        Nc = (4 * co + 127) // 128 * 128                    # (tests/test_gpu_fdy_cnn.py, the mixing test)
        assert (g["Nc"], g["ld4"], g["ldg4"], g["hid"]) == (Nc, 64 if 4 * co == 64 else Nc, 64 if 4 * co <= 64 else Nc, FC.hid_of(g["cin"]))


def test_engine_builds_its_geometry_from_cnn_geometry():
    net = pmam()
    geo = net._make_engine()._image_specs(torch.device("cpu"))[2]
    assert geo == cnn_geometry(net.cnn_filters, net.cnn_pooling, net.cnn_dynamic) and [g["co"] for g in geo] == [16, 64]


def test_direct0_and_fused16_thresholds():
    geo = cnn_geometry(synth.PMAM_FILTERS, synth.PMAM_POOLING, None)
    at = lambda B, T, tn: cnn_layer_plans(geo, synth.PMAM_POOLING, B, T, tn)
    p = at(2, 4, True)
    assert p[0].M == 1024 and p[0].direct0 and p[0].fused16
    assert not p[1].direct0 and p[1].fused16 == (p[1].M >= 1024) and not any(q.direct0 or q.fused16 for q in p[2:])
    p = at(1, 4, True)
    assert p[0].M == 512 and not p[0].direct0 and not p[0].fused16
    for B, T in SHAPES + [(2, 4), (1, 4)]:
        assert not any(q.direct0 or q.fused16 for q in at(B, T, False))
        for tn in (True, False):
            for g, q in zip(geo, at(B, T, tn)):
                if q.direct0:
                    assert q.conv == GEO.DwImage(g["ldg"], g["Kp"], True, GEO.CONV0_DW16) and q.ldyo == 16
                else:
                    assert q.ldyo == g["ldg"] and q.conv.route != GEO.CONV0_DW16


@pytest.mark.parametrize("dw_tn", [True, False])
@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("stack", sorted(STACKS))
def test_slot_layouts_routes_and_sizes(stack, B, T, dw_tn):
    filters, pooling, dynamic = STACKS[stack]
    geo = cnn_geometry(filters, pooling, dynamic)
    plans = cnn_layer_plans(geo, pooling, B, T, dw_tn)
    for g, p, (H, W, M) in zip(geo, plans, walk(filters, pooling, B, T)):
        assert (p.H, p.W, p.M) == (H, W, M)
        assert p.M * g["co"] == B * H * W * g["co"]                   # the dropout mask `_cnn_fwd` allocates for the layer
        for name, rows, k, n_valid, k_valid, ldx in images(g, M, dw_tn):
            im = getattr(p, name)
            assert (im.rows, im.k) == (rows, k) and im.rows * im.k == rows * k      # the slot `_grad_slots` allocates
            tn = bool(dw_tn and (M >= 1024 or rows < 128 or k < 128) and rows % 64 == 0 and k % 64 == 0)
            assert im.tn == tn, (name, g)
            if im.route == GEO.CONV0_DW16:
                assert name == "conv" and p.direct0
                continue
            small = tn and n_valid in (16, 32) and k_valid <= 32 and ldx >= (k_valid + 3) // 4 * 4
            assert im.route == (GEO.SMALL_DW if small else GEO.TN if tn else GEO.COPY), (name, g)
    if stack == "pmam" and dw_tn:       # the streaming reduction takes the gates of the 16 / 32-filter layers; layer 0's convolution is direct
        small = [(i, n) for i, p in enumerate(plans) for n in ("gate", "conv") if getattr(p, n).route == GEO.SMALL_DW]
        assert plans[0].direct0 and small == [(i, "gate") for i in range(4)]


def test_plans_are_cached_per_shape_and_dw_tn():
    eng = pmam()._make_engine()
    cpu = torch.device("cpu")
    a = eng._cnn_plan(2, 12, cpu)
    assert eng._cnn_plan(2, 12, cpu) is a and eng._cnn_plan(3, 12, cpu) is not a
    eng.dw_tn = False
    b = eng._cnn_plan(2, 12, cpu)
    assert b is not a and b != a and eng._cnn_plan(2, 12, cpu) is b
    eng.dw_tn = True
    assert eng._cnn_plan(2, 12, cpu) is a
