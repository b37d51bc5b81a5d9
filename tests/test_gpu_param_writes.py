"""The derived images of the fp32 weights (engine/images.py `_lnf_image` / `_w2_image` / `_w2f8_image` / `_wlo_image`, the PMAM statics of
frozen LoRA blocks, DASM's folded K / V projection) are cached between forwards and rebuilt only when their key (engine.version_key)
moves.  Every write a training script can make to the masters -- torch.optim.AdamW (foreach, for-loop, fused), trainer.FusedAdamWEMA
(student, EMA teacher), `p.copy_` under no_grad, load_state_dict of the model / of a sub-module / through the compat
DataParallelWrapper, the compat `update_ema`, the recipes' freeze / unfreeze sequence -- must show in the next forward: forward, write,
forward again must equal a FRESH model loaded with the written weights (same kernels, same weights: bit level) and differ from the first
forward.  White box: every populated cache slot whose masters the write touched got a new key, every other slot kept its own (frozen
images survive optimiser steps)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from transformer4sed_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EQ = 1e-6              # after the write vs a fresh model with the written weights (test_gpu_model.py: eval / step / eval)
MOVED = 100 * EQ       # the write must move the outputs far above that bound (no case passes vacuously)
LR = 1e-3


def _log_path():
    from test_gpu_model import LOG as MODEL_LOG        # (the measured errors go beside the other GPU tests' logs)
    return os.path.join(os.path.dirname(MODEL_LOG), "param_writes.log")


def report(name, moved, err, extra=""):
    log = _log_path()
    os.makedirs(os.path.dirname(log), exist_ok=True)
    with open(log, "a") as f:
        f.write(f"{name}: moved={moved:.4e} err={err:.4e} {extra}\n")


def maxerr(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


# ---------------------------------------------------------------------------------------------------------------- models and forwards
def matsed(teacher=False):
    from test_gpu_model import _build
    from transformer4sed_amd.trainer import get_params
    net, _ = _build(False, 2, 2)
    if teacher:
        for p in net.parameters():
            p.detach_()
        return net, None
    groups = get_params(net, {"encoder": {"lr": 5e-6, "weight_decay": 1e-4, "freeze_layer": 1, "step_lr": 4},
                              "decoder": {"lr": 1e-4, "weight_decay": 1e-4}, "head": {"lr": 1e-4, "weight_decay": 1e-4}})
    return net, groups


PMAM_LR = dict(cnn=dict(lr=1.5e-4, weight_decay=1e-4), passt=dict(lr=5e-6, weight_decay=1e-4, freeze_layer=1, step_lr=0),
               decoder=dict(lr=1.5e-4, weight_decay=1e-4), head=dict(lr=2e-4))


def pmam():
    """PaSST_CNN with LoRA encoder linears and the finetune heads (mlm off); block 0 below `freeze_layer` with its LoRA factors frozen (the
    statics path of pmam_engine._weights), block 1 trains its LoRA factors (mark_only_lora_as_trainable, get_param_lr)."""
    from test_gpu_pmam import PASST, CNN
    from transformer4sed_amd.passt_cnn import PaSST_CNN
    from transformer4sed_amd.pmam_trainer import get_param_lr, mark_only_lora_as_trainable
    ps = {k: v for k, v in PASST.items() if k != "mlm_dict"}
    ps.update(mlm=False, class_num=10, passt_feature_layer=2, encoder_depth=2)
    net = PaSST_CNN(passt_sed_param=ps, cnn_param=dict(CNN, conv_dropout=0.0))
    sd = synth.pmam_state_dict_np(depth=12, mlm=False, lora_r=8, class_num=10)
    own = net.state_dict()
    net.load_state_dict({k: torch.from_numpy(np.asarray(sd[k])) for k in own}, strict=True)
    net = net.to(DEV)
    mark_only_lora_as_trainable(net.backbone)
    return net, get_param_lr(net, PMAM_LR)


def dasm():
    from test_gpu_dasm_train import build_dasm
    from transformer4sed_amd.pmam_trainer import get_param_lr
    net = build_dasm(2)
    lr = dict(cnn=dict(lr=1.5e-4, weight_decay=1e-4), passt=dict(lr=5e-6, weight_decay=1e-4, freeze_layer=0, step_lr=0),
              decoder=dict(lr=1.5e-4, weight_decay=1e-4), head=dict(lr=2e-4))
    return net, get_param_lr(net, lr)


BUILD = {"matsed": matsed, "teacher": lambda: matsed(teacher=True), "pmam": pmam, "dasm": dasm}


def _mel():
    return torch.from_numpy(synth.det_uniform("param_writes/mel", (2, 128, 1000), -1.2, 1.2)).to(DEV)


def _query():
    q = torch.from_numpy(synth.det_normal("param_writes/q", (12, 1024)))
    return (q / q.norm(dim=-1, keepdim=True)).to(DEV)


def fwd_eval_win(net):       # MAT-SED validation: evaluation mode, window encoding (two-term / fp8 / residual images)
    net.eval()
    with torch.no_grad():
        s, w, o = net(_mel(), encoder_win=True, win_param=[512, 31], mix_rate=0.5, temp_w=0.5)
    return torch.cat([s.reshape(-1), w.reshape(-1), o["at_out"].reshape(-1)]).clone()


def fwd_train_nograd(net):   # the teacher inside the train step (MAT-SED: LayerNorm-folded images) / PMAM's unmerged LoRA images
    net.train()
    with torch.no_grad():
        s, w, o = net(_mel(), encoder_win=False, temp_w=1)
    return torch.cat([s.reshape(-1), w.reshape(-1), o["at_out"].reshape(-1)]).clone()


def fwd_eval(net):
    net.eval()
    with torch.no_grad():
        s, w, o = net(_mel(), encoder_win=False, temp_w=0.5)
    return torch.cat([s.reshape(-1), w.reshape(-1), o["at_out"].reshape(-1)]).clone()


def fwd_dasm_query(net):
    net.eval()
    with torch.no_grad():
        s, w, o = net(_mel(), temp_w=0.5, query=_query())
    return torch.cat([s.reshape(-1), w.reshape(-1), o["at_out"].reshape(-1)]).clone()


FWD = {"eval_win": fwd_eval_win, "train_nograd": fwd_train_nograd, "eval": fwd_eval, "eval_query": fwd_dasm_query}


# ---------------------------------------------------------------------------------------------------------------- cache slots
def slots(net):
    """{(slot, name): key} of every populated cache slot; PMAM statics only while all their masters are frozen (a block with a trainable
    tensor is re-imaged on every forward, its stale statics entry is not a cache)."""
    eng, pbn, out = net.engine, net._param_by_name, {}
    for n, ent in eng.cache.items():
        for s in ("lnf_key", "w2_key", "wlo_key"):
            if getattr(ent, s) is not None:
                out[(s, n)] = getattr(ent, s)
    for n, k in eng.__dict__.get("_static_keys", {}).items():
        if not any(pbn[d].requires_grad for d in deps(net, ("static", n))):
            out[("static", n)] = k
    head = getattr(net, "dasm_head", None)
    for s in ("_fused_key", "_fused_split_key"):
        if head is not None and getattr(head, s) is not None:
            out[(s, "dasm")] = getattr(head, s)
    return out


def deps(net, slot):
    """Names of the fp32 masters a cache slot is built from."""
    kind, n = slot
    if kind in ("w2_key", "wlo_key"):
        return {n}
    if kind == "lnf_key":
        blk = n[:n.index(".attn.") if ".attn." in n else n.index(".mlp.")] + "."
        norm = "norm1" if ".attn.qkv." in n else "norm2"
        return {n, n[:-len("weight")] + "bias", blk + norm + ".weight", blk + norm + ".bias"}
    if kind == "static":
        spec = next(sp for sp in net.engine._specs[0] if sp.name == n)
        return {spec.master, spec.lora + ".lora_A", spec.lora + ".lora_B"}
    L = net.dasm_head.L          # (the DASM head's fold and its split image)
    return {f"at_decoder.decoder.layers.{l}.multihead_attn.in_proj_{s}" for l in range(L) for s in ("weight", "bias")} | \
        {"at_projector.weight", "at_projector.bias"}


def check_slots(net, s0, s1, written, what, reach=True):
    """`reach`: the write must reach at least one cached image (False: a write to tensors without cached images -- nothing may be
    rebuilt).  A requires_grad flip is no write: it re-keys nothing."""
    assert s0, f"{what}: no cached image populated -- the forward ran a path without a cache"
    lost = {k for k in set(s0) - set(s1) if k[0] != "static"}      # (a PMAM statics entry leaves the set while its block trains)
    assert not lost, f"{what}: slots vanished {sorted(lost)}"
    common = set(s0) & set(s1)
    changed = {k for k in common if s0[k] != s1[k]}
    expect = {k for k in common if deps(net, k) & written}
    assert expect or not reach, f"{what}: the write reaches no cached image"
    assert changed == expect, (what, "stale:", sorted(expect - changed), "rebuilt without a write:", sorted(changed - expect))
    return len(expect), len(common)


# ---------------------------------------------------------------------------------------------------------------- writers
def _noise(t, seed, rel=0.1, floor=0.01):
    g = torch.Generator(device=t.device).manual_seed(seed)
    r = torch.randn(t.shape, generator=g, device=t.device, dtype=torch.float32)
    return t * (1 + rel * r) + floor * torch.randn(t.shape, generator=g, device=t.device, dtype=torch.float32)


def _grads(net, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    names = set()
    for n, p in net.named_parameters():
        p.grad = torch.randn(p.shape, generator=g, device=DEV) if p.requires_grad else None
        if p.requires_grad:
            names.add(n)
    return names


def adamw(groups, impl):
    kw = {"foreach": dict(foreach=None), "forloop": dict(foreach=False), "fused": dict(fused=True)}[impl]
    return torch.optim.AdamW([dict(params=[p for _, p in g["params"]], lr=LR, weight_decay=g["weight_decay"]) for g in groups],
                             betas=(0.9, 0.999), eps=1e-8, **kw)


def adamw_step(net, groups, impl, seed=1):
    written = _grads(net, seed)
    try:
        opt = adamw(groups, impl)
        opt.step()
    except RuntimeError as e:
        if impl == "fused":
            pytest.skip(f"this torch build refuses torch.optim.AdamW(fused=True) on the device: {e}")
        raise
    opt.zero_grad(set_to_none=True)
    return written


def copy_write(net, name):
    p = net._param_by_name[name]
    with torch.no_grad():
        p.copy_(_noise(p, 7))
    return {name}


def _perturbed_state(module, seed):
    """state_dict of `module` with every parameter (not the BatchNorm statistics) perturbed."""
    sd = module.state_dict(keep_vars=True)
    return {k: (_noise(v.detach(), seed + i) if isinstance(v, torch.nn.Parameter) else v.detach().clone()) for i, (k, v) in enumerate(sd.items())}


def compat_utils():
    """`src.utils` as the recipes import it (transformer4sed_amd/compat in front of sys.path); the `src` package is not left in sys.modules."""
    import importlib
    sys.path.insert(0, os.path.join(ROOT, "transformer4sed_amd", "compat"))
    try:
        return importlib.import_module("src.utils")
    finally:
        sys.path.pop(0)
        for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
            del sys.modules[k]


def load_write(net, how):
    if how == "full":
        net.load_state_dict(_perturbed_state(net, 11), strict=True)
        return set(net._param_by_name)
    if how == "wrapper":
        DataParallelWrapper = compat_utils().DataParallelWrapper
        DataParallelWrapper(torch.nn.DataParallel(net)).load_state_dict(_perturbed_state(net, 13), strict=True)
        return set(net._param_by_name)
    prefix = how
    sub = net.get_submodule(prefix)
    sub.load_state_dict(_perturbed_state(sub, 17), strict=True)
    return {n for n in net._param_by_name if n.startswith(prefix + ".")}


# ---------------------------------------------------------------------------------------------------------------- the check
def fresh_like(kind, net):
    fresh, _ = BUILD[kind]()
    fresh.train(net.training)      # (PaSST_CNN: eval() folds the LoRA product into `weight`, a state_dict taken in eval mode holds it)
    fresh.load_state_dict({k: v.detach().clone() for k, v in net.state_dict().items()}, strict=True)
    return fresh


def run_case(kind, fwd, write, what, reach=True, setup=None):
    """before = fwd(net); written = write(net, groups); after = fwd(net) == fwd(fresh model with net's state) and != before.  `setup(net,
    groups)`, before the first forward, replaces `groups` with what `write` needs."""
    net, groups = BUILD[kind]()
    if setup is not None:
        groups = setup(net, groups)
    f = FWD[fwd]
    f(net)
    before = f(net)
    s0 = slots(net)
    written = write(net, groups)
    after = f(net)
    s1 = slots(net)
    want = f(fresh_like(kind, net))
    moved, err = maxerr(after, before), maxerr(after, want)
    try:
        n_hit, n_all = check_slots(net, s0, s1, written, what, reach=reach)
    finally:        # (the measured errors are logged whether or not the white-box check holds)
        report(f"{kind} / {fwd} / {what}", moved, err, f"(slots rebuilt {n_hit} of {n_all})" if "n_all" in locals() else "(slot check failed)")
    assert moved > MOVED, (what, moved)
    assert err < EQ, (what, err)


# ---------------------------------------------------------------------------------------------------------------- (a) torch AdamW
ADAMW_CASES = [(k, f) for k, f in (("matsed", "eval_win"), ("pmam", "eval"), ("dasm", "eval"), ("dasm", "eval_query"))]


@pytest.mark.parametrize("impl", ["foreach", "forloop", "fused"])
@pytest.mark.parametrize("kind,fwd", ADAMW_CASES)
def test_torch_adamw_step(kind, fwd, impl):
    # (PMAM in evaluation mode: the trained tensors -- LoRA factors of block 1, CNN, context network, heads -- have no cached image; the
    #  frozen encoder's images must all survive the step)
    run_case(kind, fwd, lambda net, groups: adamw_step(net, groups, impl), f"torch.optim.AdamW ({impl})", reach=kind != "pmam")


def test_dasm_after_adamw_vs_float64_oracle():
    """The fresh-model comparison cannot see a kernel that is wrong the same way twice: after the AdamW step, the head's outputs of the
    evaluation forward against oracle/dasm_oracle.py in float64 on the same frame tokens / SED decoder output (test_gpu_dasm.py's bounds
    for a fresh head)."""
    from oracle import dasm_oracle

    net, groups = dasm()
    fwd_eval(net)
    before = fwd_eval(net)
    adamw_step(net, groups, "foreach")
    net.eval()
    with torch.no_grad():
        s, w, o = net(_mel(), temp_w=0.5)
    B, D = s.shape[0], 768
    ft = net.engine._frame32.view(B, -1, D)[:, 2:, :].double().cpu()
    xd = net._last_x_dec.double().cpu()
    sd = {n: p.detach().double().cpu() for n, p in net._param_by_name.items()}
    so, wo, ao, _ = dasm_oracle.dasm_head(sd, ft, xd, temp_w=0.5, n_layers=net.at_layers)
    after = torch.cat([s.reshape(-1), w.reshape(-1), o["at_out"].reshape(-1)])
    es, ew, ea = maxerr(s, so), maxerr(w, wo), maxerr(o["at_out"], ao)
    report("dasm / eval / torch.optim.AdamW (foreach) vs float64 oracle", maxerr(after, before), max(es, ew, ea),
           f"(strong {es:.3e} weak {ew:.3e} at {ea:.3e})")
    assert maxerr(after, before) > MOVED
    assert es < 1e-4 and ew < 1e-4 and ea < 1e-5, (es, ew, ea)


# ---------------------------------------------------------------------------------------------------------------- (a') FusedAdamWEMA
def fused_opt(student, groups, teacher=None):
    """trainer.FusedAdamWEMA: binds the masters into its arena, so it is built before the first forward (`run_case(setup=...)`)."""
    from transformer4sed_amd.trainer import FusedAdamWEMA
    return FusedAdamWEMA(student, groups, ema_net=teacher)


def fused_step(opt, seed, ema_alpha=None):
    """Random gradients for the student's trainable parameters, laid out in the optimiser's arena as the model's backward lays them out
    (passt_sed._SedFunction.backward), and one FusedAdamWEMA step; -> the student parameters it stepped."""
    net, g = opt.net, torch.Generator(device=DEV).manual_seed(seed)
    arena = torch.zeros(opt.total, dtype=torch.float32, device=DEV)
    byname = dict(net.named_parameters())
    for n, p in byname.items():
        if p.requires_grad and n not in net._inert_param_names:
            o, k = opt.offset[n]
            arena[o:o + k].copy_(torch.randn(k, generator=g, device=DEV))
            p.grad = arena[o:o + k].view(p.shape)
    net._last_grad_arena = arena
    opt.step(ema_alpha)
    written = {n for g_ in opt.param_groups for n in g_["names"] if byname[n].grad is not None}
    opt.zero_grad()
    return written


@pytest.mark.parametrize("kind,fwd", ADAMW_CASES)
def test_fused_adamw_ema_student_step(kind, fwd):
    run_case(kind, fwd, lambda net, opt: fused_step(opt, 41), "FusedAdamWEMA.step (student)", reach=kind != "pmam", setup=fused_opt)


@pytest.mark.parametrize("kind,fwd", [("teacher", "train_nograd"), ("teacher", "eval_win"), ("pmam", "eval")])
def test_fused_adamw_ema_teacher_sweep(kind, fwd):
    """MatSedTrainer's step: AdamW on a (perturbed) student, then the EMA sweep rewrites every tensor of the teacher whatever its
    requires_grad says -- MAT-SED's detached teacher, PMAM's frozen LoRA block (statics)."""
    def setup(teacher, _):
        student, groups = BUILD["matsed" if kind == "teacher" else kind]()
        student.load_state_dict(_perturbed_state(student, 43), strict=True)
        return fused_opt(student, groups, teacher)

    def write(teacher, opt):
        fused_step(opt, 47, ema_alpha=0.5)
        return set(teacher._param_by_name)
    run_case(kind, fwd, write, "FusedAdamWEMA.step (EMA teacher)", setup=setup)


# ---------------------------------------------------------------------------------------------------------------- (b) p.copy_
COPY_CASES = [
    ("matsed", "eval_win", "backbone.blocks.1.attn.qkv.weight"),      # two-term image
    ("matsed", "eval_win", "backbone.blocks.1.mlp.fc1.weight"),       # residual image (per-clip mean correction)
    ("matsed", "eval_win", "backbone.blocks.1.mlp.fc2.weight"),       # fp8 two-term image
    ("teacher", "train_nograd", "backbone.blocks.1.norm1.weight"),    # LayerNorm-folded qkv image
    ("teacher", "train_nograd", "backbone.blocks.0.norm2.weight"),    # LayerNorm-folded fc1 image
    ("teacher", "train_nograd", "backbone.blocks.1.mlp.fc1.weight"),
    ("teacher", "eval_win", "backbone.blocks.0.attn.qkv.weight"),
    ("pmam", "eval", "backbone.blocks.0.attn.qkv.weight"),             # frozen LoRA block: statics + two-term image
    ("pmam", "eval", "backbone.blocks.1.mlp.fc2.weight"),
    ("dasm", "eval", "at_decoder.decoder.layers.1.multihead_attn.in_proj_bias"),      # DASM fold
    ("dasm", "eval", "at_projector.bias"),
    ("dasm", "eval", "at_decoder.decoder.layers.0.multihead_attn.in_proj_weight"),
    ("dasm", "eval_query", "at_projector.weight"),
    ("dasm", "eval", "backbone.blocks.1.attn.qkv.weight"),
]


@pytest.mark.parametrize("kind,fwd,name", COPY_CASES)
def test_copy_under_no_grad(kind, fwd, name):
    run_case(kind, fwd, lambda net, groups: copy_write(net, name), f"p.copy_ {name}")


@pytest.mark.parametrize("name", ["backbone.blocks.0.attn.qkv.lora_A", "backbone.blocks.0.mlp.fc1.lora_B"])
def test_pmam_frozen_lora_factor_write(name):
    """A frozen block's LoRA factor written between two evaluations: in train mode (unmerged, like an optimiser would), then eval() folds
    s B A into every LoRA linear's weight again (lora/layers.py semantics) -- the statics images of the frozen block must follow.  (The
    train-mode forward itself is not used here: its batch-statistics sums are not bit-reproducible.)"""
    def write(net, groups):
        pbn = net._param_by_name
        v0 = {n: p._version for n, p in pbn.items()}
        net.train()
        copy_write(net, name)
        net.eval()
        written = {n for n, p in pbn.items() if p._version != v0[n]}
        assert name in written and name.replace(name.rsplit(".", 1)[1], "weight") in written
        return written
    run_case("pmam", "eval", write, f"train(), p.copy_ {name}, eval()")


# ---------------------------------------------------------------------------------------------------------------- (c) load_state_dict
LOAD_CASES = [(k, f, how) for k, f in (("matsed", "eval_win"), ("teacher", "train_nograd"), ("pmam", "eval"), ("dasm", "eval"))
              for how in ("full", "backbone.blocks.1", "wrapper")] + [("dasm", "eval", "at_decoder.decoder.layers.1")]


@pytest.mark.parametrize("kind,fwd,how", LOAD_CASES)
def test_load_state_dict_after_a_forward(kind, fwd, how):
    run_case(kind, fwd, lambda net, groups: load_write(net, how), f"load_state_dict ({how})")


# ---------------------------------------------------------------------------------------------------------------- (d) compat update_ema
@pytest.mark.parametrize("fwd", ["eval_win", "train_nograd"])
def test_compat_update_ema_teacher(fwd):
    """recipes: `update_ema(net, ema_net, step, ema_factor)` (src.utils through the compat layer) after the student moved; the teacher (a
    deepcopy with detached parameters) is evaluated afterwards."""
    update_ema = compat_utils().update_ema

    def write(ema, _):
        student, _ = matsed()
        student.load_state_dict(_perturbed_state(ema, 23), strict=True)
        update_ema(student, ema, 2, 0.999)          # alpha = min(1 - 1/2, 0.999): half way to the student
        return set(ema._param_by_name)
    run_case("teacher", fwd, write, "compat update_ema")


# ---------------------------------------------------------------------------------------------------------------- (e) freeze / unfreeze
@pytest.mark.parametrize("kind,fwd,block", [("matsed", "eval_win", "backbone.blocks.0."), ("pmam", "eval", "backbone.blocks.0.")])
def test_freeze_unfreeze_sequence(kind, fwd, block):
    """recipes/desed/finetune/*/setting.py: forward with a block frozen; unfreeze it and step; forward; freeze it again and step the rest;
    forward.  Each forward equals a fresh model with the same weights; the re-frozen block does not move in the second step and its
    images are keyed again as constants."""
    net, groups = BUILD[kind]()
    f = FWD[fwd]
    blk = {n: p for n, p in net._param_by_name.items() if n.startswith(block)}
    assert blk and not any(p.requires_grad for p in blk.values())
    f(net)
    out0, s0 = f(net), slots(net)
    opt = adamw(groups, "foreach")
    for p in blk.values():
        p.requires_grad_(True)
    written = _grads(net, 31)
    opt.step()
    opt.zero_grad(set_to_none=True)
    out1, s1 = f(net), slots(net)
    want1 = f(fresh_like(kind, net))
    for p in blk.values():
        p.requires_grad_(False)
    frozen = {n: p.detach().clone() for n, p in blk.items()}
    written2 = _grads(net, 37)
    opt.step()
    opt.zero_grad(set_to_none=True)
    out2, s2 = f(net), slots(net)
    assert all(torch.equal(frozen[n], p) for n, p in blk.items()), "a re-frozen tensor moved in the optimiser step"
    want2 = f(fresh_like(kind, net))
    for step, (a, b, want, sa, sb, w) in enumerate(((out0, out1, want1, s0, s1, written), (out1, out2, want2, s1, s2, written2))):
        what = f"freeze / unfreeze {block} step {step + 1}"
        n_hit, n_all = check_slots(net, sa, sb, w, what, reach=kind != "pmam" or step == 0)
        moved, err = maxerr(b, a), maxerr(b, want)
        report(f"{kind} / {fwd} / {what}", moved, err, f"(slots rebuilt {n_hit} of {n_all})")
        assert moved > MOVED, (what, moved)
        assert err < EQ, (what, err)
