#!/usr/bin/env python
"""Generate tests/golden/pmam_fdy_d2.npz and pmam_fdy_ft_d2.npz: the depth-2 synth-weight REFERENCE `PaSST_CNN` with the frequency-dynamic
CNN branch -- `cnn_param["cnn_name"] = "FDY-CNN"`, src/models/cnn/FDY_cnn.py, src/models/cnn_transformer/passt_cnn.py:21-30,51-60 -- with
the canonical 7-layer stack (synth.FDY_FILTERS / FDY_POOLING / FDY_DY_LAYERS) and the weights of synth.fdy_cnn_state_dict_np.

The reference is imported through oracle/make_golden.py (which puts it and its third-party stand-ins on sys.path); nothing of it is
copied.  Inputs, weights and the dropout keep-masks are regenerated from synth.py by the tests, so only strided probes are stored.

pmam_fdy_d2.npz (post-pretrain stage: mlm, LoRA, 30 prototypes, B = 2)
  * `state_names` / `state_shapes`: the reference's `state_dict()`;
  * eval mode: the MLM draws `ev_noise` / `ev_probs` / `ev_rand_idx` / `ev_mask_ids`, `ev_pred_s`, `ev_fbm_s`, `ev_at_out`, `ev_strong_s`
    (prototype posteriors), `ev_cnn_s` (strided CNN features), and per dynamic layer the attention: `ev_att_min` / `ev_att_max` [6] and `ev_att{i}_s` (every 5th frame);
  * train mode with conv dropout 0.5 under the keep-masks of tests/fdy_cases.py `drop_masks_np("pmam_fdy_d2", ...)` (`drop_p`): `tr_*`
    as above, `tr_loss*`, `tr_grad_names` / `tr_grad_norms` / `tr_grad_heads`, and the running statistics after that forward:
    `tr_bn{i}_running_*` (BatchNorm2d), `tr_abn{i}_running_*` (the attention heads' BatchNorm1d);
  * `pm10_cnn_s`: eval-mode CNN features [B, 384, 250] (every 10th frame, every 16th channel) of the reference's FDY_CNN alone with the 10-layer PMAM
    stack (synth.PMAM_FILTERS / PMAM_POOLING, DY_layers [0] + [1] * 9, weights tag "fdy10") on the same spectrograms.
pmam_fdy_ft_d2.npz (fine-tune stage: mlm False, no LoRA, 10 classes)
  * `strong`, `weak`, `at_out`, `strong_t05_pad` / `weak_t05_pad`, `strong_win49` / `weak_win49` / `fbm_win49_s`, `tr_loss`, `tr_grad_*` (dropout 0);
  * `strong_vs_uniform_attention_max`: `strong` against the same reference model with every attention weight forced to 0.25.
Guards (asserted here, re-asserted by tests/test_fdy_cnn_cpu.py): every dynamic layer's attention reaches min <= 0.10 and max >= 0.50;
strong_vs_uniform_attention_max >= 20e-3; every BatchNorm1d has running_mean != 0 and running_var != 1.

Run on the authoring machine:  python tools/gen_fdy_cnn_golden.py
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from oracle import make_golden as MG  # noqa: E402  (puts the reference and its shims on sys.path)
from transformer4sed_amd import synth  # noqa: E402
import fdy_cases as FC  # noqa: E402

TAG, FTAG = "pmam_fdy_d2", "pmam_fdy_ft_d2"
B, DEPTH, FL, DROP_P = 2, 2, 2, 0.5
GUARD = 20 * 1e-3
t2n = MG.t2n
S = (slice(None), slice(None, None, 25), slice(None, None, 16))
DYN = [i for i, d in enumerate(synth.FDY_DY_LAYERS) if d]


def build_reference(conv_dropout, mlm=True, lora=True, class_num=30):
    from src.models.cnn_transformer.passt_cnn import PaSST_CNN
    passt = dict(passt_feature_layer=FL, class_num=class_num, f_pool="attention", decode_ratio=10, at_adapter=True, decoder="transformerXL",
                 decoder_layer_num=3, decoder_pos_emd_len=1000, decoder_dim=384, mlm=mlm)
    if lora:
        passt["lora_config"] = dict(r=8, lora_alpha=1, requires_grad_pretrain=False)
    if mlm:
        passt["mlm_dict"] = dict(strategy="block", block_width=10, mask_rate=0.8, out_dim=768, mask_style=[0.9, 0.05, 0.05])
    cnn = dict(FC.FDY_CNN_PARAM, conv_dropout=conv_dropout)
    o_load = torch.load
    torch.load = lambda *a, **k: {}         # the PaSST checkpoint is unavailable; every weight is set below
    try:
        net = PaSST_CNN(passt_sed_param=passt, cnn_param=cnn)
    finally:
        torch.load = o_load
    assert net.cnn_name == "FDY-CNN"
    sd_np = synth.fdy_cnn_state_dict_np(depth=12, mlm=mlm, lora_r=8 if lora else 0, class_num=class_num)
    ref_shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert ref_shapes == {k: tuple(v.shape) for k, v in sd_np.items()}, "PaSST_CNN (FDY-CNN) state_dict contract drifted"
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd_np.items()}, strict=True)
    net.backbone.blocks = net.backbone.blocks[:DEPTH]
    return net


def hook_attention(net, store):
    hs = []
    for i in DYN:
        hs.append(getattr(net.cnn.cnn, f"conv{i}").attention.register_forward_hook(lambda _m, _i, o, i=i: store.__setitem__(i, o.detach())))
    return hs


def grads_of(net, out, prefix):
    names, norms, heads = [], [], []
    for k, p in net.named_parameters():
        if p.grad is None:
            continue
        names.append(k)
        norms.append(float(p.grad.double().norm()))
        g = p.grad.reshape(-1)
        heads.append(t2n(torch.cat([g, g.new_zeros(8)])[:8]))
    out[prefix + "grad_names"], out[prefix + "grad_norms"], out[prefix + "grad_heads"] = np.asarray(names), np.asarray(norms), np.stack(heads)


def check_attention(att, out, prefix):
    mins, maxs = [], []
    for i in DYN:
        a = att[i]
        assert tuple(a.shape[:2]) == (B, 4)
        mins.append(float(a.min())); maxs.append(float(a.max()))
        out[f"{prefix}att{i}_s"] = t2n(a[:, :, ::5])
    print(f"   attention min {['%.3f' % v for v in mins]} max {['%.3f' % v for v in maxs]}", flush=True)
    assert max(mins) <= 0.10 and min(maxs) >= 0.50, "attention too flat: raise FDY_ATT_GAIN in synth.fdy_cnn_state_dict_np"
    out[prefix + "att_min"], out[prefix + "att_max"] = np.asarray(mins), np.asarray(maxs)


class InjectedDropout:
    """While active, the CNN branch's nn.Dropout modules multiply by the given keep-masks ([B, C, H, W]) / (1 - p) instead of drawing."""

    def __init__(self, net, masks, p):
        self.mods = [getattr(net.cnn.cnn, f"dropout{i}") for i in range(len(masks))]
        self.masks, self.p = masks, p

    def __enter__(self):
        self.hs = [m.register_forward_hook(lambda _m, inp, _o, mk=mk: inp[0] * mk.to(inp[0].dtype) / (1.0 - self.p))
                   for m, mk in zip(self.mods, self.masks)]
        for m in self.mods:
            m.p_saved, m.p = m.p, 0.0

    def __exit__(self, *exc):
        for h in self.hs:
            h.remove()
        for m in self.mods:
            m.p = m.p_saved


def gen_pretrain():
    from src.models.lora import mark_only_lora_as_trainable
    from recipes.desed.pmam.train import Trainer
    out = {}
    mel = torch.from_numpy(synth.det_uniform(f"{TAG}/mel", (B, 128, 1000), -1.2, 1.2))
    gmm = torch.from_numpy(synth.det_normal(MG.PMAM_SYNTH["gmm_name"], (30, 768)))
    labels = torch.from_numpy(synth.synth_strong_labels(B, n_classes=30, seed=MG.PMAM_SYNTH["label_seed"]))
    net = build_reference(conv_dropout=DROP_P).eval()
    sd = net.state_dict()
    out["state_names"] = np.asarray(list(sd.keys()))
    out["state_shapes"] = np.asarray([",".join(str(d) for d in v.shape) for v in sd.values()])
    hooks, att = {}, {}
    net.cnn.register_forward_hook(lambda m, i, o: hooks.__setitem__("cnn", o))
    hs = hook_attention(net, att)
    torch.manual_seed(51)
    rec = MG.DrawRecorder()
    with rec.recording(), torch.no_grad():
        pred, other = net(mel, encoder_win=False)
    out["ev_noise"], out["ev_probs"] = t2n(rec.of("rand")[0]), t2n(rec.of("rand")[1])
    out["ev_rand_idx"] = t2n(rec.of("randint")[0])
    out["ev_mask_ids"] = t2n(other["mask_id_seq"])
    out["ev_pred_s"] = t2n(pred[S])
    out["ev_fbm_s"] = t2n(other["frame_before_mask"][S])
    out["ev_at_out"] = t2n(other["at_out"])
    feat = hooks["cnn"].squeeze(-1)
    out["ev_cnn_s"] = t2n(feat[:, ::16, ::10])
    check_attention(att, out, "ev_")
    tr = Trainer.__new__(Trainer)
    tr.gmm_means = torch.nn.functional.normalize(gmm, dim=-1)
    out["ev_strong_s"] = t2n(tr.get_predict_from_logit(pred)[:, ::25])
    # the restatement of tests/fdy_cases.py against the module itself (the CPU test repeats this on the stored features)
    f64, _ = FC.branch(FC.cnn_tensors(synth.fdy_cnn_state_dict_np(depth=12), torch.float64), mel.double(), synth.FDY_POOLING, synth.FDY_DY_LAYERS,
                       31.0, train=False)
    d = float((f64.squeeze(-1) - feat.double()).abs().max())
    print(f"   restatement (float64) vs reference CNN features: max |d| {d:.2e} (|feat| max {float(feat.abs().max()):.2f})", flush=True)
    assert d < 1e-4
    for h in hs:
        h.remove()

    # ---- train mode: LoRA unmerged, batch statistics in BatchNorm2d and BatchNorm1d, dropout 0.5 under injected keep-masks
    net = build_reference(conv_dropout=DROP_P)
    mark_only_lora_as_trainable(net.backbone)
    net.backbone.norm.weight.requires_grad_(True)      # "norm." rule of get_param_lr (setting.py:73-76)
    net.backbone.norm.bias.requires_grad_(True)
    net.train()
    masks = [torch.from_numpy(m.transpose(0, 3, 1, 2).copy()) for m in FC.drop_masks_np(TAG, B, synth.FDY_FILTERS, synth.FDY_POOLING, DROP_P)]
    att = {}
    hook_attention(net, att)
    torch.manual_seed(53)
    rec = MG.DrawRecorder()
    with rec.recording(), InjectedDropout(net, masks, DROP_P):
        pred, other = net(mel, encoder_win=False)
    out["drop_p"] = np.float64(DROP_P)
    out["tr_noise"], out["tr_probs"] = t2n(rec.of("rand")[0]), t2n(rec.of("rand")[1])
    out["tr_rand_idx"] = t2n(rec.of("randint")[0])
    out["tr_pred_s"] = t2n(pred[S])
    out["tr_fbm_s"] = t2n(other["frame_before_mask"][S])
    out["tr_at_out"] = t2n(other["at_out"])
    out["tr_att_min"], out["tr_att_max"] = np.asarray([float(att[i].min()) for i in DYN]), np.asarray([float(att[i].max()) for i in DYN])
    strong = tr.get_predict_from_logit(pred)
    m = other["mask_id_seq"]
    loss_strong = torch.nn.functional.binary_cross_entropy(strong[m], labels.transpose(1, 2)[m])
    loss_weak = torch.nn.functional.binary_cross_entropy(other["at_out"], (labels.sum(-1) >= 1).float())
    loss = loss_strong + 0.1 * loss_weak
    loss.backward()
    out["tr_loss_strong"], out["tr_loss_weak"], out["tr_loss"] = t2n(loss_strong), t2n(loss_weak), t2n(loss)
    grads_of(net, out, "tr_")
    sd_after = net.state_dict()
    for i in range(len(synth.FDY_FILTERS)):
        for st in ("running_mean", "running_var"):
            out[f"tr_bn{i}_{st}"] = t2n(sd_after[f"cnn.cnn.batchnorm{i}.{st}"]).copy()
            if i in DYN:
                v = t2n(sd_after[f"cnn.cnn.conv{i}.attention.bn.{st}"]).copy()
                assert (v != (0.0 if st == "running_mean" else 1.0)).all()
                out[f"tr_abn{i}_{st}"] = v
        if i in DYN:
            assert int(sd_after[f"cnn.cnn.conv{i}.attention.bn.num_batches_tracked"]) == 4

    # ---- the 10-layer PMAM stack with dynamic layers: the reference's FDY_CNN alone, eval mode
    from src.models.cnn import FDY_CNN
    cnn10 = FDY_CNN(**{k: v for k, v in FC.FDY10_CNN_PARAM.items() if k != "cnn_name"})
    sd10 = {k[len("cnn."):]: torch.from_numpy(np.asarray(v)) for k, v in
            synth.fdy_cnn_state_dict_np(tag="fdy10", nb_filters=synth.PMAM_FILTERS, dy_layers=FC.PMAM10_DY, depth=12).items() if k.startswith("cnn.")}
    cnn10.load_state_dict(sd10, strict=True)
    cnn10.eval()
    att10 = {}
    for i in range(1, 10):
        getattr(cnn10.cnn, f"conv{i}").attention.register_forward_hook(lambda _m, _i, o, i=i: att10.__setitem__(i, o.detach()))
    with torch.no_grad():
        f10 = cnn10(mel.transpose(1, 2).unsqueeze(1)).squeeze(-1)
    assert tuple(f10.shape) == (B, 384, 250)
    out["pm10_cnn_s"] = t2n(f10[:, ::16, ::10])
    out["pm10_att_min"], out["pm10_att_max"] = np.asarray([float(att10[i].min()) for i in range(1, 10)]), np.asarray([float(att10[i].max()) for i in range(1, 10)])
    print(f"   10-layer stack attention min {out['pm10_att_min'].round(3)} max {out['pm10_att_max'].round(3)}", flush=True)
    MG.save(TAG, **out)


def gen_finetune():
    out = {}
    mel = torch.from_numpy(synth.det_uniform(f"{FTAG}/mel", (B, 128, 1000), -1.2, 1.2))
    net = build_reference(conv_dropout=DROP_P, mlm=False, lora=False, class_num=10).eval()
    att = {}
    hs = hook_attention(net, att)
    pm = torch.zeros(B, 1000, dtype=torch.bool)
    pm[0, 900:] = True
    with torch.no_grad():
        s1, w1, o1 = net(mel, encoder_win=False, temp_w=1)
        check_attention(att, out, "")
        s2, w2, _ = net(mel, encoder_win=False, temp_w=0.5, pad_mask=pm)
        s3, w3, o3 = net(mel, encoder_win=True, mix_rate=0.5, win_param=[512, 49], temp_w=0.5)
    for h in hs:
        h.remove()
    out["strong"], out["weak"], out["at_out"] = t2n(s1), t2n(w1), t2n(o1["at_out"])
    out["strong_t05_pad"], out["weak_t05_pad"] = t2n(s2), t2n(w2)
    out["strong_win49"], out["weak_win49"] = t2n(s3), t2n(w3)
    out["fbm_win49_s"] = t2n(o3["frame_before_mask"][:, ::25, ::16])
    # guard: the attention must move the posteriors far beyond the parity bound
    import importlib
    FDY_cnn = importlib.import_module("src.models.cnn.FDY_cnn")
    o_fwd = FDY_cnn.attention2d.forward
    FDY_cnn.attention2d.forward = lambda self, x: torch.full((x.shape[0], 4, x.shape[2]), 0.25, dtype=x.dtype)
    try:
        with torch.no_grad():
            s_uni, _, _ = net(mel, encoder_win=False, temp_w=1)
    finally:
        FDY_cnn.attention2d.forward = o_fwd
    d = float((s1 - s_uni).abs().max())
    print(f"   {FTAG}: strong_vs_uniform_attention_max {d:.4f}", flush=True)
    assert d >= GUARD, "too small for a 1e-3 parity test to notice; raise FDY_ATT_GAIN in synth.fdy_cnn_state_dict_np"
    out["strong_vs_uniform_attention_max"] = np.float64(d)
    net = build_reference(conv_dropout=0.0, mlm=False, lora=False, class_num=10).train()
    strong, weak, other = net(mel, encoder_win=False, temp_w=1)
    wgt_s = torch.from_numpy(synth.det_uniform(f"{FTAG}/gs", tuple(strong.shape)))
    wgt_w = torch.from_numpy(synth.det_uniform(f"{FTAG}/gw", tuple(weak.shape)))
    wgt_a = torch.from_numpy(synth.det_uniform(f"{FTAG}/ga", tuple(other["at_out"].shape)))
    loss = (strong * wgt_s).sum() + (weak * wgt_w).sum() + (other["at_out"] * wgt_a).sum()
    loss.backward()
    out["tr_strong"], out["tr_weak"], out["tr_loss"] = t2n(strong), t2n(weak), t2n(loss)
    grads_of(net, out, "tr_")
    MG.save(FTAG, **out)


if __name__ == "__main__":
    torch.manual_seed(0)
    gen_pretrain()
    gen_finetune()
    for name in (TAG, FTAG):
        size = os.path.getsize(os.path.join(MG.GOLD, name + ".npz"))
        assert size < 589 * 1024, f"{name}.npz is {size / 1024:.1f} KiB: the fixtures are held below 589 KiB"
