#!/usr/bin/env python
"""Generate tests/golden/model_d768_l2_conformer.npz and model_d768_l2_conformer_win100.npz: the depth-2 synth-weight REFERENCE model
with the Conformer context network -- `PaSST_SED(decoder="conformer", decoder_layer_num=2, at_adapter=True)`,
src/models/passt/passt_sed.py:179-184, src/models/transformer_decoder.py:125-165 -- without a window and with decoder_win_len=100.

The reference is imported through oracle/make_golden.py (which puts it and its third-party stand-ins on sys.path); nothing of it is
copied.  `model_fixture` there hard-codes `encoder_blocks` and three layers, so this tool carries its own fixture function with the
same key set where it applies (finetune-mode outputs, strided block probes, loss and gradient norms; MLM-mode prediction, loss,
recorded mask draws and gradient norms), plus
  * `state_names` / `state_shapes`: the reference's `state_dict()`;
  * `strong_vs_centre_tap_max`: distance of `strong` from the same model with every depthwise kernel cut to its centre tap;
  * window file: `strong_vs_full_max`, distance of `strong` from the windowless model, and `win_len`.
Both distances are asserted >= 20 x 1e-3, so a parity test at 1e-3 cannot pass on a kernel that ignores the taps or the window.

Run on the authoring machine:  python tools/gen_conformer_golden.py
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import make_golden as MG  # noqa: E402  (puts the reference and its shims on sys.path)
from transformer4sed_amd import synth  # noqa: E402

FIXTURES = (("model_d768_l2_conformer", None), ("model_d768_l2_conformer_win100", 100))
B, DEPTH, LAYERS, WTAG = 2, 2, 2, "wc768"
t2n = MG.t2n


def build_reference(mlm, win):
    from src.models.passt.passt_sed import PaSST_SED
    o_load = torch.load
    torch.load = lambda *a, **k: {}         # the PaSST checkpoint is unavailable; every weight is set below
    try:
        kw = dict(passt_feature_layer=DEPTH, f_pool="mean_pool", decode_ratio=10, at_adapter=True, decoder="conformer",
                  decoder_layer_num=LAYERS, decoder_pos_emd_len=1000, decoder_win_len=win, mlm=mlm, embed_dim=768, decoder_dim=768,
                  load_pretrained_model=True)
        if mlm:
            kw["mlm_dict"] = dict(strategy="block", block_width=10, mask_rate=0.75, out_dim=768)
        net = PaSST_SED(**kw)
    finally:
        torch.load = o_load
    sd = {k: torch.from_numpy(v) for k, v in synth.conformer_state_dict_np(tag=WTAG, dec_layers=LAYERS, depth=12, mlm=mlm).items()}
    own = net.state_dict()
    if win is not None:
        sd["decoder.att_mask"] = own["decoder.att_mask"]        # the constructor's own buffer
    net.load_state_dict(sd, strict=True)
    assert {k: tuple(v.shape) for k, v in own.items()} == {k: tuple(v.shape) for k, v in sd.items()}, "state_dict contract drifted"
    net.backbone.blocks = net.backbone.blocks[:DEPTH]
    return net


def grads_of(net):
    names, norms, heads = [], [], []
    for k, p in net.named_parameters():
        if p.grad is None:
            continue
        names.append(k)
        norms.append(float(p.grad.double().norm()))
        heads.append(t2n(p.grad.reshape(-1)[:8]))
    return np.asarray(names), np.asarray(norms), np.stack(heads)


def gen(tag, win):
    out = {}
    mel = torch.from_numpy(synth.det_uniform(f"{tag}/mel", (B, 128, 1000), -1.2, 1.2))
    S = (slice(None), slice(None, None, 25), slice(None, None, 16))
    net = build_reference(False, win).eval()
    sd = net.state_dict()
    out["state_names"] = np.asarray(list(sd.keys()))
    out["state_shapes"] = np.asarray([",".join(str(d) for d in v.shape) for v in sd.values()])
    hooks = {}

    def grab(name):
        def fn(_m, _i, o):
            hooks[name] = o
        return fn

    for i, blk in enumerate(net.decoder.blocks):
        blk.register_forward_hook(grab(f"dec{i}"))
    net.interpolate_module.register_forward_hook(grab("interp"))
    net.decoder.register_forward_hook(grab("decoder"))
    with torch.no_grad():
        strong, weak, other = net(mel, encoder_win=False, temp_w=1)
    out["strong"], out["weak"], out["at_out"] = t2n(strong), t2n(weak), t2n(other["at_out"])
    out["interp_s"] = t2n(hooks["interp"][S])
    for i in range(LAYERS):
        out[f"dec{i}_s"] = t2n(hooks[f"dec{i}"].permute(1, 0, 2)[S])
    out["decoder_s"] = t2n(hooks["decoder"][S])
    with torch.no_grad():
        pm = torch.zeros(B, 1000, dtype=torch.bool)
        pm[0, 900:] = True
        s2, w2, _ = net(mel, encoder_win=False, temp_w=0.5, pad_mask=pm)
    out["strong_t05_pad"], out["weak_t05_pad"] = t2n(s2), t2n(w2)

    # ---- guards: the taps (and the window) must move the posteriors far beyond the parity bound
    cut = build_reference(False, win).eval()
    with torch.no_grad():
        for blk in cut.decoder.blocks:
            w = blk.conv_module.depthwise_conv.weight
            w[:, :, :15] = 0
            w[:, :, 16:] = 0
        s_cut, _, _ = cut(mel, encoder_win=False, temp_w=1)
    d = float((strong - s_cut).abs().max())
    print(f"   {tag}: strong vs centre-tap-only max {d:.4f}", flush=True)
    assert d >= 20 * 1e-3, "the off-centre taps do not move the output enough for a 1e-3 parity test to notice them: raise tap_scale in synth.py"
    out["strong_vs_centre_tap_max"] = np.float64(d)
    if win is not None:
        full = build_reference(False, None).eval()
        with torch.no_grad():
            s_full, _, _ = full(mel, encoder_win=False, temp_w=1)
        d = float((strong - s_full).abs().max())
        print(f"   {tag}: strong vs windowless max {d:.4f}", flush=True)
        assert d >= 20 * 1e-3, "the window does not move the output enough for a 1e-3 parity test to notice it"
        out["strong_vs_full_max"] = np.float64(d)
        out["win_len"] = np.asarray([win], dtype=np.int32)

    # ---- finetune-mode gradients
    net.train()     # (dropout p = 0 everywhere)
    for p in net.parameters():
        p.requires_grad_(True)
    strong, weak, other = net(mel, encoder_win=False, temp_w=1)
    wgt_s = torch.from_numpy(synth.det_uniform(f"{tag}/gs", tuple(strong.shape)))
    wgt_w = torch.from_numpy(synth.det_uniform(f"{tag}/gw", tuple(weak.shape)))
    wgt_a = torch.from_numpy(synth.det_uniform(f"{tag}/ga", tuple(other["at_out"].shape)))
    loss = (strong * wgt_s).sum() + (weak * wgt_w).sum() + (other["at_out"] * wgt_a).sum()
    loss.backward()
    out["ft_loss"] = t2n(loss)
    out["ft_grad_names"], out["ft_grad_norms"], out["ft_grad_heads"] = grads_of(net)

    # ---- MLM mode (encoder frozen: recipes/desed/mlm/mlm_passt/passt_mlm_setting.py:5-9)
    net = build_reference(True, win)
    net.train()
    for p in net.backbone.parameters():
        p.requires_grad_(False)
    torch.manual_seed(43)
    rec = MG.DrawRecorder()
    with rec.recording():
        pred, other = net(mel, encoder_win=False)
    ru, ri = rec.of("rand"), rec.of("randint")
    out["mlm_noise"], out["mlm_probs"], out["mlm_rand_idx"] = t2n(ru[0]), t2n(ru[1]), t2n(ri[0])
    out["mlm_mask_ids"] = t2n(other["mask_id_seq"])
    out["mlm_pred_s"] = t2n(pred[S])
    out["mlm_fbm_s"] = t2n(other["frame_before_mask"][S])
    loss = torch.nn.functional.mse_loss(other["frame_before_mask"][other["mask_id_seq"]], pred[other["mask_id_seq"]])
    out["mlm_loss"] = t2n(loss)
    loss.backward()
    out["mlm_grad_names"], out["mlm_grad_norms"], out["mlm_grad_heads"] = grads_of(net)
    MG.save(tag, **out)


if __name__ == "__main__":
    torch.manual_seed(0)
    for tag, w in FIXTURES:
        gen(tag, w)
