"""Gradient-norm clipping without a GPU: the chunk table of the flat gradient arena (`grad_chunk_table`), the float64 restatement of the
finalising kernel that the GPU tests compare with (tests/grad_clip_cases.py) against torch.nn.utils.clip_grad_norm_ on the same values, the
refusals of the public API and of the trainers' `max_grad_norm` key, and the ABI."""
import ctypes

import numpy as np
import pytest
import torch

import grad_clip_cases as GC
import transformer4sed_amd
from transformer4sed_amd.grad_clip import GRAD_CHUNK, grad_chunk_table, max_grad_norm_of, model_layout

CH = GRAD_CHUNK
NEW_ENTRY_POINTS = ("sed_grad_sumsq_chunks", "sed_grad_norm_finalize", "sed_scale_by_dev")


def check_table(layout, CH, tab, first):
    """Exact cover of every tensor's elements, no chunk across a slice boundary, arena order, at most CH floats, 16-byte aligned starts."""
    assert tab.dtype == np.int32 and first.dtype == np.int32 and tab.ndim == 2 and tab.shape[1] == 2
    assert first.shape == (len(layout) + 1,) and first[0] == 0 and first[-1] == len(tab)
    assert (np.diff(first) >= 0).all()
    total = max((o + k for _, o, k in layout), default=0)
    seen = np.zeros(total, dtype=np.int32)
    for t, (_, o, k) in enumerate(layout):
        c0, c1 = int(first[t]), int(first[t + 1])
        assert c1 - c0 == (k + CH - 1) // CH, (t, k)
        for off, ln in tab[c0:c1]:
            assert 0 < ln <= CH and off % 4 == 0
            assert o <= off and off + ln <= o + k, "a chunk leaves its tensor's slice"
            seen[off:off + ln] += 1
    want = np.zeros(total, dtype=np.int32)
    for _, o, k in layout:
        want[o:o + k] = 1
    assert np.array_equal(seen, want), "every element of every tensor in exactly one chunk, the padding in none"
    if len(tab) > 1:
        assert (tab[1:, 0] >= tab[:-1, 0] + tab[:-1, 1]).all(), "chunks in arena order, disjoint"


@pytest.mark.parametrize("ch", [CH, 64, 4096])
def test_chunk_table_synthetic_layouts(ch):
    sizes = tuple(s for base in (GC.SIZES, (1, 63, 64, 65, ch - 1, ch, ch + 1, 3 * ch + 7)) for s in base if s > 0)
    layout, total = GC.synthetic_layout(sizes)
    assert all(o % 64 == 0 for _, o, _ in layout)
    tab, first = grad_chunk_table(layout, ch)
    check_table(layout, ch, tab, first)
    # an empty tensor owns no chunk; an empty layout gives an empty table
    tab, first = grad_chunk_table([("a", 0, 5), ("empty", 64, 0), ("b", 64, 70)], ch)
    assert first.tolist()[1] == first.tolist()[2]
    check_table([("a", 0, 5), ("empty", 64, 0), ("b", 64, 70)], ch, tab, first)
    tab, first = grad_chunk_table([], ch)
    assert tab.shape == (0, 2) and first.tolist() == [0]


def test_chunk_table_refuses_bad_layouts():
    with pytest.raises(ValueError, match="aligned"):
        grad_chunk_table([("a", 0, 10), ("b", 10, 10)])
    with pytest.raises(ValueError, match="overlaps"):
        grad_chunk_table([("a", 0, 100), ("b", 64, 10)])
    with pytest.raises(ValueError, match="multiple of 64"):
        grad_chunk_table([("a", 0, 100)], 100)
    with pytest.raises(ValueError, match="2\\^31"):
        grad_chunk_table([("a", 0, 2 ** 31)], 2 ** 24)


@pytest.fixture(scope="module")
def cpu_net():
    from transformer4sed_amd.passt_sed import PaSST_SED
    return PaSST_SED(load_pretrained_model=False, encoder_depth=2, decoder="transformerXL")


def test_chunk_table_real_layouts(cpu_net):
    """The model's own packing (no optimiser bound) and a FusedAdamWEMA's layout of the depth-2 model."""
    from transformer4sed_amd.trainer import FusedAdamWEMA, get_params
    key, layout, total = model_layout(cpu_net)
    assert key[0] == "own" and total % 64 == 0 and len(layout) > 60
    assert not any(n.startswith("backbone.head") for n, _, _ in layout), "PaSST's unused heads are not part of the model's own arena"
    params = dict(cpu_net.named_parameters())
    assert [n for n, _, _ in layout] == [n for n in params if not n.startswith("backbone.head")]
    assert all(k == params[n].numel() and o % 64 == 0 for n, o, k in layout)
    check_table(layout, CH, *grad_chunk_table(layout))
    opt = FusedAdamWEMA(cpu_net, get_params(cpu_net, {"encoder": {"lr": 5e-6, "weight_decay": 1e-4, "freeze_layer": 0, "step_lr": 4},
                                                      "decoder": {"lr": 1e-4, "weight_decay": 1e-4}, "head": {"lr": 1e-4, "weight_decay": 1e-4}}))
    try:
        key, layout, total = model_layout(cpu_net)
        assert key[0] == "flat" and layout is opt.layout and total == opt.total
        assert sorted(n for n, _, _ in layout) == sorted(params)
        tab, first = grad_chunk_table(layout)
        check_table(layout, CH, tab, first)
        assert len(tab) == sum((k + CH - 1) // CH for _, _, k in layout)
    finally:
        del cpu_net._flat_layout, cpu_net._inert_param_names


def torch_clip(arena, layout, max_norm):
    """torch.nn.utils.clip_grad_norm_ on CPU parameters whose gradients hold the arena's values -> (total, clipped arena)."""
    ps = []
    for _, o, k in layout:
        p = torch.nn.Parameter(torch.zeros(k))
        p.grad = torch.from_numpy(arena[o:o + k].copy())
        ps.append(p)
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm, norm_type=2.0, error_if_nonfinite=False)
    out = np.zeros_like(arena)
    for (_, o, k), p in zip(layout, ps):
        out[o:o + k] = p.grad.numpy()
    return float(total), out


def test_restatement_vs_torch_clip_grad_norm():
    arena, layout, total_n = GC.synthetic_arena()
    norms, total, _ = GC.reference(arena, layout, 0.0)
    # per-tensor norms against torch's float64 norm of the same values; the all-zero tensor exactly 0, the one-element tensor |g|
    for (n, o, k), got in zip(layout, norms):
        want = float(torch.from_numpy(arena[o:o + k]).double().norm())
        assert abs(got - want) <= 1e-12 * want, n
    assert norms[[n for n, _, _ in layout].index(GC.ZERO_TENSOR)] == 0.0
    assert norms[0] == abs(float(arena[0]))
    assert norms.max() / norms[norms > 0].min() > 1e5, "the tensors are meant to span decades"
    assert abs(total - float(torch.from_numpy(arena).double().norm())) <= 1e-12 * total
    for factor in (0.37, 0.999, 1.0, 1.5, 100.0):
        m = factor * total
        _, _, scale = GC.reference(arena, layout, m)
        t_total, t_arena = torch_clip(arena, layout, m)
        assert abs(t_total - total) <= 2e-6 * total          # (torch's total is an fp32 norm of fp32 norms)
        assert scale.dtype == np.float32 and scale <= 1
        if factor > 1:
            assert scale == 1 and GC.same_bits(GC.scaled(arena, scale), arena)
        # torch's coefficient comes from ITS fp32 total: equal to the restatement's to a few ulps, and so is the clipped arena
        want = min(1.0, m / (t_total + 1e-6))
        assert abs(float(scale) - want) <= 4e-6 * want, (factor, scale, want)
        np.testing.assert_allclose(GC.scaled(arena, scale), t_arena, rtol=4e-6, atol=0)
    # measure only
    for m in (0.0, -1.0):
        assert GC.reference(arena, layout, m)[2] == 1


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_restatement_nonfinite_vs_torch(bad):
    """error_if_nonfinite=False: nothing is special-cased.  inf -> total inf, coefficient max_norm / inf = 0 (finite gradients become 0,
    the inf becomes NaN); NaN -> total, coefficient and every gradient NaN."""
    arena, layout, _ = GC.synthetic_arena()
    o = layout[3][1]
    arena[o + 5] = bad
    norms, total, scale = GC.reference(arena, layout, 1.0)
    t_total, t_arena = torch_clip(arena, layout, 1.0)
    if np.isnan(bad):
        assert np.isnan(total) and np.isnan(t_total) and np.isnan(scale) and np.isnan(norms[3])
        assert np.isnan(GC.scaled(arena, scale)).all()
        for _, o2, k2 in layout:
            assert np.isnan(t_arena[o2:o2 + k2]).all()
    else:
        assert np.isinf(total) and np.isinf(t_total) and np.isinf(norms[3]) and scale == 0
        got = GC.scaled(arena, scale)
        assert np.isnan(got[o + 5]) and np.count_nonzero(np.nan_to_num(got)) == 0
        assert GC.same_bits(got, t_arena)
    assert np.isfinite(np.delete(norms, 3)).all()
    assert GC.reference(arena, layout, 0.0)[2] == 1          # measuring never scales


def test_refusals(cpu_net):
    for nt in (1, 1.0, float("inf"), 0):
        with pytest.raises(ValueError, match="norm_type"):
            transformer4sed_amd.clip_grad_norm_(cpu_net, 1.0, norm_type=nt)
    for m in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_norm"):
            transformer4sed_amd.clip_grad_norm_(cpu_net, m)
    # a model that is not on the GPU: like the forward, no CPU path
    with pytest.raises(RuntimeError, match="no CPU path|MI355X"):
        transformer4sed_amd.clip_grad_norm_(cpu_net, 1.0)
    with pytest.raises(RuntimeError, match="no CPU path|MI355X"):
        transformer4sed_amd.grad_norms(cpu_net)


def test_max_grad_norm_config_key():
    assert max_grad_norm_of({}) is None and max_grad_norm_of({"max_grad_norm": None}) is None
    assert max_grad_norm_of({"clip_grad": True}) is None, "the reference's key alone stays the reference's no-op"
    assert max_grad_norm_of({"max_grad_norm": 20}) == 20.0 and max_grad_norm_of({"max_grad_norm": 0}) == 0.0
    for bad in (-1, -1e-9, float("nan"), float("inf"), "20", True):
        with pytest.raises(ValueError, match="max_grad_norm"):
            max_grad_norm_of({"max_grad_norm": bad})


@pytest.mark.parametrize("bad", [-0.5, float("inf"), float("nan")])
def test_trainers_refuse_a_bad_max_grad_norm_at_construction(bad):
    from transformer4sed_amd.dasm_trainer import AudiosetStrongTrainer, DasmTrainer, OvDasmTrainer
    from transformer4sed_amd.pmam_trainer import PmamTrainer
    from transformer4sed_amd.trainer import MatSedTrainer
    tr = {"training": {"clip_grad": True, "max_grad_norm": bad}, "class_loss": {"loss_name": "BCELoss"}}
    with pytest.raises(ValueError, match="max_grad_norm"):
        MatSedTrainer(None, None, None, None, tr, epoch_len=1)
    with pytest.raises(ValueError, match="max_grad_norm"):
        PmamTrainer(torch.nn.Linear(2, 2), None, None, torch.zeros(3, 4), tr)
    for cls in (AudiosetStrongTrainer, DasmTrainer):
        with pytest.raises(ValueError, match="max_grad_norm"):
            cls(None, None, None, tr)
    with pytest.raises(ValueError, match="max_grad_norm"):
        OvDasmTrainer(None, None, None, tr, labels=["a"], type_dict={"a": "common"})


def test_abi_declares_and_exports_the_entry_points():
    from transformer4sed_amd import _lib, build
    protos = _lib.parse_header()
    for name in NEW_ENTRY_POINTS:
        assert name in protos, name
    assert [t for t, _ in protos["sed_scale_by_dev"]] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    assert [n for _, n in protos["sed_grad_norm_finalize"]] == ["partial", "tensor_first_chunk", "n_tensors", "max_norm", "norms",
                                                                "total_and_scale", "stream"]
    dll = ctypes.CDLL(build.build(verbose=False))
    for name in NEW_ENTRY_POINTS:
        assert hasattr(dll, name), name
    assert dll.sed_abi_version(0) == 7, "entry points were only added: the ABI version stays"
    for name in ("clip_grad_norm_", "grad_norms", "grad_chunk_table"):
        assert callable(getattr(transformer4sed_amd, name)), name
