"""Gradient-norm clipping on an MI355X (csrc/grad_clip.hip, transformer4sed_amd/grad_clip.py): the three kernels on a synthetic arena
against the float64 restatement of tests/grad_clip_cases.py, the public API on the depth-2 model under both arena layouts, and the
`training["max_grad_norm"]` key through every trainer.

Error bound of the norms.  A chunk has at most CH = 16384 floats over 256 lanes: a lane adds e <= 64 squares -- in this kernel as four
chains of 16 fused multiply-adds (one per component of its 16-byte loads) and two adds, so at most 18 roundings, below the e = 64 the
bound is stated for; the wave butterfly and the four wave sums add log2(256) = 8 levels.  Sum of squares of one chunk:
(e + log2(256) + 2) 2^-24 = 74 x 2^-24 = 4.4e-6 relative (all terms are non-negative, so the bound is relative to the sum itself); the
fp64 sums over chunks and tensors add nothing at this level; the square root halves it and rounds once more (6e-8): 2.3e-6 on a norm.
The tests assert 1e-5."""
import os
import random
import sys

import numpy as np
import pytest
import torch

import grad_clip_cases as GC
from transformer4sed_amd import synth
from transformer4sed_amd.grad_clip import _Plan, arena_norms, clip_grad_norm_, grad_norms

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORM_TOL = 1e-5
CFG = {"encoder": {"lr": 5e-6, "weight_decay": 1e-4, "freeze_layer": 0, "step_lr": 4},
       "decoder": {"lr": 1e-4, "weight_decay": 1e-4}, "head": {"lr": 1e-4, "weight_decay": 1e-4}}


def rel(got, want):
    return abs(float(got) - float(want)) / abs(float(want))


# ------------------------------------------------------------------------------------------------------------------ kernel level
@pytest.fixture(scope="module")
def case():
    arena, layout, total = GC.synthetic_arena()
    norms, tot, _ = GC.reference(arena, layout, 0.0)
    return dict(arena=arena, layout=layout, total=total, norms=norms, tot=tot, plan=_Plan(layout, total, torch.device(DEV)))


def run(case, arena_np, max_norm=0.0, scale_arena=False):
    """-> (norms, total, scale, arena afterwards) as numpy, from one pass of the launches over a device copy of `arena_np`."""
    a = torch.from_numpy(arena_np).to(DEV)
    norms, total, scale = arena_norms(a, case["plan"], max_norm, scale_arena=scale_arena)
    torch.cuda.synchronize()
    return norms.cpu().numpy(), total.cpu().numpy().reshape(()), scale.cpu().numpy().reshape(()), a.cpu().numpy()


def test_norms_and_total_vs_float64_restatement(case):
    """Per-tensor norms and the total within the derived bound (module docstring; 1e-5 asserted), the all-zero tensor exactly 0;
    measuring leaves the arena alone and reports scale 1."""
    norms, total, scale, after = run(case, case["arena"])
    names = [n for n, _, _ in case["layout"]]
    for n, got, want in zip(names, norms, case["norms"]):
        print(f"norm {n}: got {got:.9e} want {want:.9e}")
        if want == 0:
            assert got == 0, n
        else:
            assert rel(got, want) <= NORM_TOL, (n, got, want)
    assert norms[names.index(GC.ZERO_TENSOR)] == 0.0
    print(f"total: got {total:.9e} want {case['tot']:.9e}")
    assert rel(total, case["tot"]) <= NORM_TOL
    assert scale == 1 and GC.same_bits(after, case["arena"])


def test_two_runs_are_bit_identical(case):
    a, b = run(case, case["arena"]), run(case, case["arena"])
    assert GC.same_bits(a[0], b[0]) and GC.same_bits(a[1], b[1])


def test_max_norm_above_the_total_leaves_the_arena_alone(case):
    base = run(case, case["arena"])
    norms, total, scale, after = run(case, case["arena"], max_norm=3.0 * float(case["tot"]), scale_arena=True)
    assert scale == 1
    assert GC.same_bits(after, case["arena"]), "a step that does not clip must not touch the gradients"
    assert GC.same_bits(total, base[1]) and GC.same_bits(norms, base[0])


def test_clipping_scales_every_element_once(case):
    """max_norm = 0.37 x total: the arena afterwards is float32(g) * float32(scale) bit for bit with the scale the DEVICE computed; that
    scale is torch's coefficient of the restatement to the accuracy of the total; the padding between the slices stays zero."""
    m = 0.37 * float(case["tot"])
    norms, total, scale, after = run(case, case["arena"], max_norm=m, scale_arena=True)
    want_scale = GC.reference(case["arena"], case["layout"], m)[2]
    print(f"scale: got {scale:.9e} want {want_scale:.9e}")
    assert scale.dtype == np.float32 and 0 < scale < 1 and rel(scale, want_scale) <= NORM_TOL
    assert rel(total, case["tot"]) <= NORM_TOL, "the returned total is the norm BEFORE clipping"
    assert GC.same_bits(after, GC.scaled(case["arena"], scale))
    pad = np.ones(case["total"], dtype=bool)
    for _, o, k in case["layout"]:
        pad[o:o + k] = False
    assert pad.any() and not after[pad].any()
    # the clipped gradients have norm max_norm
    assert rel(run(case, after)[1], m) <= 2 * NORM_TOL


@pytest.mark.parametrize("bad", [np.inf, np.nan], ids=["inf", "nan"])
def test_nonfinite_gradient_behaves_like_torch(case, bad):
    """error_if_nonfinite=False: one inf planted in one tensor -> that tensor's norm and the total are inf, the coefficient is
    max_norm / inf = 0, finite gradients become (signed) zeros and the inf becomes NaN -- what the restatement and torch give on the same
    values.  A NaN makes total, coefficient and every gradient NaN.  (Data in a buffer; nothing faults.)"""
    arena = case["arena"].copy()
    t = 3
    o = case["layout"][t][1]
    arena[o + 5] = bad
    norms, total, scale, after = run(case, arena, max_norm=1.0, scale_arena=True)
    r_norms, r_total, r_scale = GC.reference(arena, case["layout"], 1.0)
    assert GC.same_bits(np.float32(total), np.float32(r_total)) and GC.same_bits(scale, r_scale)
    assert GC.same_bits(norms[t], np.float32(r_norms[t]))
    others = np.delete(np.arange(len(norms)), t)
    assert np.isfinite(norms[others]).all() and np.allclose(norms[others], r_norms[others], rtol=NORM_TOL, atol=0)
    assert GC.same_bits(after, GC.scaled(arena, r_scale))
    # torch on CPU tensors holding the same values
    ps = []
    for _, o2, k2 in case["layout"]:
        p = torch.nn.Parameter(torch.zeros(k2))
        p.grad = torch.from_numpy(arena[o2:o2 + k2].copy())
        ps.append(p)
    t_total = torch.nn.utils.clip_grad_norm_(ps, 1.0, norm_type=2.0, error_if_nonfinite=False)
    assert GC.same_bits(np.float32(total), t_total.numpy())
    for (_, o2, k2), p in zip(case["layout"], ps):
        assert GC.same_bits(after[o2:o2 + k2], p.grad.numpy())


def test_entry_points_refuse_bad_arguments(case):
    from transformer4sed_amd._lib import SedHipError
    from transformer4sed_amd.ops import call
    a = torch.zeros(6, device=DEV)
    with pytest.raises(SedHipError, match="bad argument"):
        call("sed_scale_by_dev", a, 6, torch.ones(1, device=DEV))          # not a multiple of 4
    with pytest.raises(RuntimeError, match="the layout describes"):
        arena_norms(torch.zeros(case["total"] + 64, device=DEV), case["plan"])


# ------------------------------------------------------------------------------------------------------------------- model level
@pytest.fixture(scope="module")
def weights():
    return {k: torch.from_numpy(v) for k, v in synth.matsed_state_dict_np(tag="w768", depth=12).items()}


def build(weights):
    from transformer4sed_amd.passt_sed import PaSST_SED
    net = PaSST_SED(passt_feature_layer=2, f_pool="mean_pool", decode_ratio=10, at_adapter=True, decoder="transformerXL", decoder_layer_num=3,
                    decoder_pos_emd_len=1000, mlm=False, load_pretrained_model=False, encoder_depth=2)
    own = net.state_dict()
    net.load_state_dict({k: v for k, v in weights.items() if k in own}, strict=True)
    return net.to(DEV).train()


def one_backward(net):
    tag = "model_d768_l2"
    mel = torch.from_numpy(synth.det_uniform(f"{tag}/mel", (2, 128, 1000), -1.2, 1.2)).to(DEV)
    strong, weak, other = net(mel, encoder_win=False, temp_w=1)
    gs = torch.from_numpy(synth.det_uniform(f"{tag}/gs", tuple(strong.shape))).to(DEV)
    gw = torch.from_numpy(synth.det_uniform(f"{tag}/gw", tuple(weak.shape))).to(DEV)
    ga = torch.from_numpy(synth.det_uniform(f"{tag}/ga", tuple(other["at_out"].shape))).to(DEV)
    ((strong * gs).sum() + (weak * gw).sum() + (other["at_out"] * ga).sum()).backward()


@pytest.mark.parametrize("optimizer", ["FusedAdamWEMA", "torch.optim.AdamW"])
def test_model_grad_norms_and_clip(weights, optimizer):
    """`grad_norms` against the host loop over `named_parameters()` (p.grad.double().norm(), 1e-5) and `clip_grad_norm_` on the depth-2
    model after one backward -- with a FusedAdamWEMA bound (its layout: every parameter, group order) and with torch.optim.AdamW (the
    model's own packing: the parameters it computes gradients for, `named_parameters()` order)."""
    from transformer4sed_amd.trainer import FusedAdamWEMA, get_params
    net = build(weights)
    with pytest.raises(RuntimeError, match="no flat gradient arena"):
        grad_norms(net)
    if optimizer == "FusedAdamWEMA":
        opt = FusedAdamWEMA(net, get_params(net, CFG))
        want_names = [n for n, _, _ in opt.layout]
        assert sorted(want_names) == sorted(n for n, _ in net.named_parameters())
    else:
        opt = torch.optim.AdamW(net.parameters(), lr=1e-4)
        want_names = [n for n, _ in net.named_parameters() if not n.startswith("backbone.head")]
    one_backward(net)
    names, norms, total = grad_norms(net)
    assert names == want_names and norms.shape == (len(names),) and total.dim() == 0 and norms.is_cuda and total.is_cuda
    params = dict(net.named_parameters())
    got = dict(zip(names, norms.cpu().tolist()))
    sumsq, with_grad = 0.0, 0
    for n, p in net.named_parameters():
        if p.grad is None:
            assert got.get(n, 0.0) == 0.0, n          # no gradient this step: a zero slice (or no slice at all)
            continue
        want = float(p.grad.double().norm())
        sumsq += want * want
        with_grad += 1
        assert n in got and rel(got[n], want) <= NORM_TOL, (n, got.get(n), want)
    assert with_grad > 60
    assert rel(total, sumsq ** 0.5) <= NORM_TOL
    # the arena is untouched by measuring; a second call returns the same bits
    names2, norms2, total2 = grad_norms(net)
    assert torch.equal(norms, norms2) and torch.equal(total, total2)
    # ---- clip
    before = net._last_grad_arena.clone()
    big, small = params["backbone.blocks.0.mlp.fc1.weight"], params["classifier.bias"]
    g_big, g_small = big.grad.clone(), small.grad.clone()
    m = 0.37 * float(total)
    ret = clip_grad_norm_(net, m)
    assert ret.dim() == 0 and ret.is_cuda and torch.equal(ret, total), "torch's return value: the total norm before clipping"
    scale = net._last_clip_scale.cpu().numpy().reshape(())
    assert 0 < scale < 1 and rel(scale, np.float32(m) / (np.float32(float(total)) + np.float32(1e-6))) <= 1e-6
    assert GC.same_bits(net._last_grad_arena.cpu().numpy(), GC.scaled(before.cpu().numpy(), scale))
    for p, g0 in ((big, g_big), (small, g_small)):          # p.grad is a view of the arena: it sees the clip
        assert GC.same_bits(p.grad.cpu().numpy(), GC.scaled(g0.cpu().numpy(), scale))
    assert rel(grad_norms(net)[2], m) <= 2 * NORM_TOL
    # a max_norm above the total: nothing moves
    now = net._last_grad_arena.clone()
    clip_grad_norm_(net, 10.0 * m)
    assert float(net._last_clip_scale) == 1.0 and torch.equal(net._last_grad_arena, now)
    if optimizer == "FusedAdamWEMA":
        assert torch.equal(opt.clip_grad_norm_(10.0 * m), grad_norms(net)[2])
        w0 = params["classifier.weight"].detach().clone()
        opt.step(None)
        assert not torch.equal(w0, params["classifier.weight"].detach())
    else:
        opt.step()
    with pytest.raises(ValueError, match="norm_type"):
        clip_grad_norm_(net, 1.0, norm_type=1)
    opt.zero_grad()
    if optimizer == "FusedAdamWEMA":
        with pytest.raises(RuntimeError, match="no flat gradient arena"):
            clip_grad_norm_(net, 1.0)


# ----------------------------------------------------------------------------------------------------------------- trainer level
def _seed(k=0):
    random.seed(101 + k); np.random.seed(102 + k); torch.manual_seed(103 + k); torch.cuda.manual_seed(104 + k)


def _matsed_trainer(weights, golden, max_grad_norm=None):
    """The smallest finetune configuration of the trainer tests (tests/golden/trainstep.npz's config: depth 2, six clips) with an optimiser
    whose step is LINEAR in the gradient: lr 1, eps 1, no weight decay, so the first AdamW update is g / (|g| + 1) ~ g.  With the recipes'
    eps = 1e-8 the first Adam update is lr * g / (|g| + eps) = lr * sign(g) whatever the gradient's scale, and a clip that did nothing
    would pass the comparison below."""
    import json
    from copy import deepcopy
    from transformer4sed_amd.scheduler import ExponentialDown
    from transformer4sed_amd.trainer import FusedAdamWEMA, MatSedTrainer, get_params
    meta = json.loads(str(golden("trainstep")["config_json"]))
    cfg, sc = deepcopy(meta["cfg"]), meta["sched"]
    for grp in cfg["opt"]["param_groups"].values():
        grp["lr"], grp["weight_decay"] = 1.0, 0.0
    assert cfg["training"]["clip_grad"] is True          # the reference's key is set in every variant: alone it clips nothing
    if max_grad_norm is not None:
        cfg["training"]["max_grad_norm"] = max_grad_norm
    net = build(weights)
    ema = deepcopy(net)
    for p in ema.parameters():
        p.detach_()
    opt = FusedAdamWEMA(net, get_params(net, cfg["opt"]["param_groups"]), ema_net=ema, betas=(0.9, 0.999), eps=1.0)
    sched = ExponentialDown(opt, start_iter=sc["n_epochs_cut"] * sc["epoch_len"], total_iter=sc["n_epochs"] * sc["epoch_len"],
                            exponent=sc["exponent"], warmup_iter=0, warmup_rate=1.0)
    ema.train()
    tr = MatSedTrainer(net, ema, opt, sched, cfg, epoch_len=1)
    wav = torch.from_numpy(synth.synth_wav(6, seed=meta["wav_seed0"])).to(DEV)
    labels = torch.from_numpy(synth.synth_batch_labels(2, 2, 2, seed=meta["label_seed0"])).to(DEV)

    def step():
        _seed()
        out = tr.finetune_step(wav, labels.clone())
        torch.cuda.synchronize()
        return out
    return tr, step


def _max_diff(a, b):
    return max(float((x.detach() - y.detach()).abs().max()) for t in ("arena", "ema_arena")
               for x, y in [(getattr(a.optimizer, t), getattr(b.optimizer, t))])


def test_matsed_trainer_clip_equals_scaling_the_arena_by_hand(weights, golden):
    """Trainer A (`max_grad_norm` = half the step's gradient norm) against trainer B (no key; the test multiplies `net._last_grad_arena`
    by A's read-back scale with torch.mul_ just before `optimizer.step`): parameters and EMA parameters after one step.  A dry run of two
    identical unclipped steps measures whether the step is bit-reproducible; if it is, A and B must agree bit for bit, otherwise within
    twice the dry run's difference.  A's parameters differ from the unclipped step's by far more (at least 100 x that bound), so a clip
    that does nothing fails.  `grad_norm` is in A's result and not in B's.

    Measured on an MI355X: the step is NOT bit-reproducible (split-K atomics in the weight gradients) -- run-to-run max |dp| of the dry
    run 1.34e-7, so the bound is 2.68e-7; A vs B 1.19e-7; A vs the unclipped step 1.6e-1 (total gradient norm 57.3)."""
    from transformer4sed_amd.grad_clip import grad_norms as measure
    d1, step1 = _matsed_trainer(weights, golden)
    seen = {}
    o_step = d1.optimizer.step

    def spy(*a, **k):
        seen["total"] = float(measure(d1.net)[2])
        return o_step(*a, **k)
    d1.optimizer.step = spy
    out1 = step1()
    d2, step2 = _matsed_trainer(weights, golden)
    out2 = step2()
    assert "grad_norm" not in out1 and "grad_norm" not in out2
    noise = _max_diff(d1, d2)
    bit_equal = noise == 0.0
    total = seen["total"]
    assert np.isfinite(total) and total > 0
    print(f"dry run: total gradient norm {total:.6e}, run-to-run max |dp| {noise:.3e} (bit-equal: {bit_equal})")
    # ---- A: the key
    a, step_a = _matsed_trainer(weights, golden, max_grad_norm=0.5 * total)
    assert a.max_grad_norm == 0.5 * total
    out_a = step_a()
    assert "grad_norm" in out_a and out_a["grad_norm"].is_cuda and out_a["grad_norm"].dim() == 0
    assert rel(out_a["grad_norm"], total) <= 1e-3, "the norm before clipping, of the same step as the dry run's"
    scale = float(a.net._last_clip_scale)
    assert rel(scale, 0.5 * total / float(out_a["grad_norm"])) <= 1e-5 and 0.4 < scale < 0.6
    # ---- B: no key, the arena scaled by hand
    b, step_b = _matsed_trainer(weights, golden)
    ob_step = b.optimizer.step

    def scaled_step(*args, **k):
        b.net._last_grad_arena.mul_(scale)
        return ob_step(*args, **k)
    b.optimizer.step = scaled_step
    out_b = step_b()
    assert "grad_norm" not in out_b
    ab, au = _max_diff(a, b), _max_diff(a, d1)
    print(f"A vs B max |dp| {ab:.3e}; A vs unclipped step max |dp| {au:.3e}; bound {2 * noise:.3e}")
    if bit_equal:
        assert ab == 0.0
    else:
        assert ab <= 2 * noise, (ab, noise)
    assert au > 0 and au >= 100 * max(2 * noise, ab), (au, noise, ab)
    for k in ("loss_total", "loss_class_strong"):          # the forward of the step is not touched by the key
        assert rel(out_a[k], out1[k]) <= 1e-5, k


def _clipped_step_check(trainer_module, plain, clipped, step_of, monkeypatch):
    """One step of `plain` (no key: no `grad_norm`), one of `clipped` (same model and optimiser, `max_grad_norm` set): `grad_norm` is
    returned, and the arena the optimiser read is the pre-clip arena times the device's scale, bit for bit."""
    rec = {}
    real = trainer_module.clip_grad_norm_

    def spy(net, max_norm, *a, **k):
        arena = net._last_grad_arena
        rec["before"] = arena.clone()
        total = real(net, max_norm, *a, **k)
        lo, hi = arena.data_ptr(), arena.data_ptr() + 4 * arena.numel()
        rec.update(after=arena.clone(), scale=net._last_clip_scale.clone(), total=total, max_norm=max_norm,
                   outside=[n for n, p in net.named_parameters() if p.grad is not None and not lo <= p.grad.data_ptr() < hi],
                   n_grads=sum(p.grad is not None for p in net.parameters()))
        return total
    monkeypatch.setattr(trainer_module, "clip_grad_norm_", spy)
    assert plain.max_grad_norm is None
    out = step_of(plain)
    assert "grad_norm" not in out and not rec, "without the key nothing is measured or clipped"
    out = step_of(clipped)
    torch.cuda.synchronize()
    assert "grad_norm" in out and rec and rec["max_norm"] == clipped.max_grad_norm
    assert torch.equal(out["grad_norm"], rec["total"])
    before, after = rec["before"].cpu().numpy(), rec["after"].cpu().numpy()
    scale = rec["scale"].cpu().numpy().reshape(())
    want_total = float(np.sqrt(np.sum(before.astype(np.float64) ** 2)))
    print(f"total {float(rec['total']):.6e} (float64 of the arena {want_total:.6e}), scale {scale:.6e}")
    assert rel(rec["total"], want_total) <= NORM_TOL
    assert 0 < scale < 1 and rel(scale, clipped.max_grad_norm / (want_total + 1e-6)) <= 2 * NORM_TOL
    assert GC.same_bits(after, GC.scaled(before, scale))
    # every parameter gradient the optimiser steps on is a view of the arena the clip scaled
    assert rec["n_grads"] > 10 and not rec["outside"], rec["outside"]


MAX_NORM = 1e-3      # far below any of these steps' gradient norms (order 0.1 .. 10): every step scales


def test_pretrain_step_clips(monkeypatch):
    import bench
    import transformer4sed_amd.trainer as T
    net, _, opt, plain, _ = bench.build(4, 2, torch.device(DEV), "pretrain")
    cfg = {**plain.cfg, "training": {**plain.cfg["training"], "max_grad_norm": MAX_NORM}}
    clipped = T.MatSedTrainer(net, None, opt, plain.scheduler, cfg, plain.epoch_len)
    wav = torch.from_numpy(synth.synth_wav(4, seed=77)).to(DEV)
    _seed(1)
    _clipped_step_check(T, plain, clipped, lambda t: t.pretrain_step(wav), monkeypatch)


def test_pmam_trainer_clips(monkeypatch):
    import bench
    import transformer4sed_amd.pmam_trainer as T
    net, opt, plain = bench.build_pmam(2, torch.device(DEV))
    assert plain.cfg["training"]["clip_grad"] is True and plain.max_grad_norm is None
    cfg = {**plain.cfg, "training": {**plain.cfg["training"], "max_grad_norm": MAX_NORM}}
    clipped = T.PmamTrainer(net, opt, plain.scheduler, torch.from_numpy(synth.det_normal("pmam/gmm_means", (30, 768))), cfg)
    wav = torch.from_numpy(synth.synth_wav(4, seed=77)).to(DEV)
    labels = torch.from_numpy(synth.synth_strong_labels(4, n_classes=30, seed=77)).to(DEV)
    _seed(2)
    _clipped_step_check(T, plain, clipped, lambda t: t.step(wav, labels.clone()), monkeypatch)


def test_dasm_trainer_clips(monkeypatch):
    import bench
    import transformer4sed_amd.dasm_trainer as T
    net, opt, plain = bench.build_dasm_train(2, torch.device(DEV), 12)
    assert plain.config["training"]["clip_grad"] is True and plain.max_grad_norm is None
    cfg = {**plain.config, "training": {**plain.config["training"], "max_grad_norm": MAX_NORM}}
    clipped = T.DasmTrainer(net, opt, plain.scheduler, cfg, sr=16000)
    wav = torch.from_numpy(synth.synth_wav(3, seed=77)).to(DEV)
    labels = torch.from_numpy(synth.synth_strong_labels(3, n_classes=12, seed=77)).to(DEV)
    _seed(3)
    _clipped_step_check(T, plain, clipped, lambda t: t.step(wav, labels.clone()), monkeypatch)


# ------------------------------------------------------------------------------------------------------------ two ranks, one GPU
def _rank_worker(rank, world, port, q):
    """One finetune step with `max_grad_norm` set on two ranks that see different clips (cuda:0, gloo -- the set-up of
    tests/test_gpu_ddp.py): every rank clips the same averaged gradients, so `grad_norm`, the clip scale, parameters and EMA are
    bit-equal across the ranks."""
    try:
        import json
        import torch.distributed as dist
        from test_gpu_ddp import DEPTH, _gather_equal
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        sys.path.insert(0, ROOT)
        import bench
        from transformer4sed_amd.ddp import GradBucketReducer
        from transformer4sed_amd.trainer import MatSedTrainer
        random.seed(50 + rank); np.random.seed(50 + rank); torch.manual_seed(50 + rank)
        net, ema_net, opt, built, _ = bench.build(6, DEPTH, dev, "finetune2")
        cfg = json.loads(json.dumps(bench.FINETUNE2))
        cfg["training"]["batch_size"] = [2, 0, 2, 2]
        cfg["training"]["max_grad_norm"] = MAX_NORM
        trainer = MatSedTrainer(net, ema_net, opt, built.scheduler, cfg, built.epoch_len, ddp=GradBucketReducer(net, opt))
        labels = torch.from_numpy(synth.synth_batch_labels(2, 2, 2, seed=60 + rank)).to(dev)
        wav = torch.from_numpy(synth.synth_wav(6, seed=70 + rank)).to(dev)
        start = opt.arena.detach().clone()
        out = trainer.finetune_step(wav, labels)
        torch.cuda.synchronize()
        assert trainer.ddp.last_issued, "no gradient slice was exchanged"
        losses = [None] * world
        dist.all_gather_object(losses, float(out["loss_total"]))
        assert losses[0] != losses[1], "the ranks were meant to see different clips"
        scale = net._last_clip_scale
        assert 0 < float(scale) < 1 and np.isfinite(float(out["grad_norm"]))
        assert _gather_equal(out["grad_norm"], world), "grad_norm differs between the ranks"
        assert _gather_equal(scale, world)
        assert not torch.equal(start, opt.arena)
        for name, t in (("parameters", opt.arena), ("EMA", opt.ema_arena), ("adam m", opt.m), ("adam v", opt.v)):
            assert _gather_equal(t, world), f"{name} differ between the ranks after a clipped step"
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok", float(out["grad_norm"])))
    except Exception:
        import traceback
        q.put((rank, "fail", traceback.format_exc()))
        raise


def test_two_ranks_clip_identically():
    import queue
    import time
    from multiprocessing.connection import wait
    import torch.multiprocessing as mp
    from test_gpu_ddp import _free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    deadline = time.monotonic() + 300          # the children's time limit; the first abnormal exit ends the other one too
    live = list(procs)
    try:
        while live and not any(p.exitcode not in (None, 0) for p in procs):
            left = deadline - time.monotonic()
            if left <= 0:
                break
            done = wait([p.sentinel for p in live], timeout=left)
            live = [p for p in live if p.sentinel not in done]
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
            p.join(10)
    res = []
    try:
        for _ in procs:
            res.append(q.get(timeout=5))
    except queue.Empty:
        pass
    assert [p.exitcode for p in procs] == [0, 0], (res, [p.exitcode for p in procs])
    assert len(res) == 2 and all(r[1] == "ok" for r in res), res
    assert res[0][2] == res[1][2]
