#!/usr/bin/env python
"""Generate tests/golden/model_d768_l2_fpooltr.npz and model_d768_l2_fpooltr_patchout4.npz: the depth-2 synth-weight REFERENCE model
with the frequency-wise transformer pooling -- `PaSST_SED(f_pool="frequency_wise_tranformer_encoder", decoder="transformerXL",
decoder_layer_num=2, at_adapter=True)`, src/models/pooling.py:18-34, src/models/passt/passt_sed.py:146-154,199-218.

The reference is imported through oracle/make_golden.py (which puts it and its third-party stand-ins on sys.path); nothing of it is
copied.  `FrequencyWiseTranformerPooling.forward` calls `.cuda()` on its tag input unconditionally (pooling.py:28): while a reference
model runs here, `torch.Tensor.cuda` is the identity (`on_cpu`), and is restored afterwards.

model_d768_l2_fpooltr.npz
  * `state_names` / `state_shapes`: the reference's `state_dict()`;
  * eval: `strong`, `weak`, `at_out`, `strong_t05_pad` / `weak_t05_pad` (temp_w = 0.5, clip 0 padded from frame 900), `pooled_s` (strided
    probe of the `f_pool_module` forward-hook output [B 99, 768]), `interp_s`; `strong_win` / `weak_win` (encoder_win, [512, 49]);
  * finetune mode: `ft_loss`, `ft_grad_names`, `ft_grad_norms`, `ft_grad_heads`; through the sliding windows: `win_toffsets` (recorded
    draws) and `win_ft_*`;
  * MLM mode (encoder frozen, block strategy, width 10, rate 0.75): `mlm_*`;
  * finetune1-style freezing (`f_pool_module.*`, `decoder.*` and the backbone except `backbone.norm` frozen): `frozen_loss`,
    `frozen_grad_names`, `frozen_grad_norms`;
  * guards, asserted >= 20 x 1e-3 so that a parity test at 1e-3 cannot pass on a kernel that ignores part of the module:
    `strong_vs_uniform_attention_max` (q and k row blocks of both qkv weights zeroed) and `strong_vs_zero_tag_max` (linear_emb zeroed).
model_d768_l2_fpooltr_patchout4.npz: train mode with `backbone.s_patchout_f = 4`: `seed`, `rows_global` (the recorded kept rows),
  `strong`, `weak`, `at_out`, `ft_loss`, `ft_grad_names`, `ft_grad_norms`.

model_d768_l2_fpooltr_sharp.npz: the same model with qkv at the encoder's synthetic gain of 1.6 (sharp frequency attention), eval mode:
  `strong`, `weak`, `strong_t05_pad`, `weak_t05_pad`, and the reference's own sensitivity to noise below the pooling: `sens_module` /
  `sens_mean_pool` = the largest movement of `strong` (temp_w 0.5) when out_norm's output is perturbed by 3e-4 relative Gaussian noise
  (three seeds each), with this module and with mean pooling on the same weights.  `noise_gain` = their ratio of means: how much louder
  than under mean pooling, for which the 1e-3 contract was set, the reference itself passes the encoder's rounding noise on.

Run on the authoring machine:  python tools/gen_fpool_transformer_golden.py [--only sharp]
"""
import contextlib
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import make_golden as MG  # noqa: E402  (puts the reference and its shims on sys.path)
from transformer4sed_amd import synth  # noqa: E402

TAG, PTAG, STAG = "model_d768_l2_fpooltr", "model_d768_l2_fpooltr_patchout4", "model_d768_l2_fpooltr_sharp"
SHARP_GAIN, NOISE, NOISE_SEEDS = 1.6, 3e-4, (1, 2, 3)
B, DEPTH, LAYERS, WTAG = 2, 2, 2, "wft768"
WIN_SEED, MLM_SEED, PATCHOUT_SEED, S_F = 53, 43, 7, 4
GUARD = 20 * 1e-3
t2n = MG.t2n


@contextlib.contextmanager
def on_cpu():
    o_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        yield
    finally:
        torch.Tensor.cuda = o_cuda


def build_reference(mlm, qkv_gain=1.0):
    from src.models.passt.passt_sed import PaSST_SED
    o_load = torch.load
    torch.load = lambda *a, **k: {}         # the PaSST checkpoint is unavailable; every weight is set below
    try:
        kw = dict(passt_feature_layer=DEPTH, f_pool="frequency_wise_tranformer_encoder", decode_ratio=10, at_adapter=True,
                  decoder="transformerXL", decoder_layer_num=LAYERS, decoder_pos_emd_len=1000, mlm=mlm, embed_dim=768, decoder_dim=768,
                  load_pretrained_model=True)
        if mlm:
            kw["mlm_dict"] = dict(strategy="block", block_width=10, mask_rate=0.75, out_dim=768)
        net = PaSST_SED(**kw)
    finally:
        torch.load = o_load
    sd = {k: torch.from_numpy(v) for k, v in synth.fpool_transformer_state_dict_np(tag=WTAG, dec_layers=LAYERS, depth=12, mlm=mlm,
                                                                                    qkv_gain=qkv_gain).items()}
    net.load_state_dict(sd, strict=True)
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}, "state_dict contract drifted"
    net.backbone.blocks = net.backbone.blocks[:DEPTH]
    return net


def grads_of(net, out, prefix, heads=True):
    names, norms, hd = [], [], []
    for k, p in net.named_parameters():
        if p.grad is None:
            continue
        names.append(k)
        norms.append(float(p.grad.double().norm()))
        hd.append(t2n(p.grad.reshape(-1)[:8]))
    out[prefix + "grad_names"], out[prefix + "grad_norms"] = np.asarray(names), np.asarray(norms)
    if heads:
        out[prefix + "grad_heads"] = np.stack(hd)


def weighted_loss(tag, strong, weak, at):
    wgt_s = torch.from_numpy(synth.det_uniform(f"{tag}/gs", tuple(strong.shape)))
    wgt_w = torch.from_numpy(synth.det_uniform(f"{tag}/gw", tuple(weak.shape)))
    wgt_a = torch.from_numpy(synth.det_uniform(f"{tag}/ga", tuple(at.shape)))
    return (strong * wgt_s).sum() + (weak * wgt_w).sum() + (at * wgt_a).sum()


def gen_model():
    out = {}
    mel = torch.from_numpy(synth.det_uniform(f"{TAG}/mel", (B, 128, 1000), -1.2, 1.2))
    S = (slice(None), slice(None, None, 25), slice(None, None, 16))
    net = build_reference(False).eval()
    sd = net.state_dict()
    out["state_names"] = np.asarray(list(sd.keys()))
    out["state_shapes"] = np.asarray([",".join(str(d) for d in v.shape) for v in sd.values()])
    assert sum(k.startswith("f_pool_module.") for k in sd) == 26
    hooks = {}
    h1 = net.f_pool_module.register_forward_hook(lambda _m, _i, o: hooks.__setitem__("pooled", o))
    h2 = net.interpolate_module.register_forward_hook(lambda _m, _i, o: hooks.__setitem__("interp", o))
    with torch.no_grad():
        strong, weak, other = net(mel, encoder_win=False, temp_w=1)
    out["strong"], out["weak"], out["at_out"] = t2n(strong), t2n(weak), t2n(other["at_out"])
    assert tuple(hooks["pooled"].shape) == (B * 99, 768)
    out["pooled_s"] = t2n(hooks["pooled"][::7, ::16])
    out["interp_s"] = t2n(hooks["interp"][S])
    h1.remove(); h2.remove()
    with torch.no_grad():
        pm = torch.zeros(B, 1000, dtype=torch.bool)
        pm[0, 900:] = True
        s2, w2, _ = net(mel, encoder_win=False, temp_w=0.5, pad_mask=pm)
        s3, w3, _ = net(mel, encoder_win=True, mix_rate=0.5, win_param=[512, 49], temp_w=1)
    out["strong_t05_pad"], out["weak_t05_pad"] = t2n(s2), t2n(w2)
    out["strong_win"], out["weak_win"] = t2n(s3), t2n(w3)

    # ---- guards: the attention weights and the tag row must move the posteriors far beyond the parity bound
    cut = build_reference(False).eval()
    with torch.no_grad():
        for blk in cut.f_pool_module.frequency_transformer:
            blk.attn.qkv.weight[:2 * 768] = 0           # q and k rows: every score 0, uniform attention
        s_uni, _, _ = cut(mel, encoder_win=False, temp_w=1)
    cut = build_reference(False).eval()
    with torch.no_grad():
        cut.f_pool_module.linear_emb.weight.zero_()
        cut.f_pool_module.linear_emb.bias.zero_()
        s_tag, _, _ = cut(mel, encoder_win=False, temp_w=1)
    for key, other_s, hint in (("strong_vs_uniform_attention_max", s_uni, "qkv_gain"), ("strong_vs_zero_tag_max", s_tag, "tag_scale")):
        d = float((strong - other_s).abs().max())
        print(f"   {TAG}: {key} {d:.4f}", flush=True)
        assert d >= GUARD, f"{key}: too small for a 1e-3 parity test to notice; raise {hint} in synth.fpool_transformer_state_dict_np"
        out[key] = np.float64(d)

    # ---- finetune-mode gradients, without and through the sliding windows
    net.train()     # (dropout p = 0 everywhere)
    for p in net.parameters():
        p.requires_grad_(True)
    strong, weak, other = net(mel, encoder_win=False, temp_w=1)
    loss = weighted_loss(TAG, strong, weak, other["at_out"])
    loss.backward()
    out["ft_loss"] = t2n(loss)
    grads_of(net, out, "ft_")
    net.zero_grad(set_to_none=True)
    torch.manual_seed(WIN_SEED)
    rec = MG.DrawRecorder()
    with rec.recording():
        strong, weak, other = net(mel, encoder_win=True, mix_rate=0.5, win_param=[512, 49], temp_w=1)
    out["win_toffsets"] = np.asarray([int(x.item()) for x in rec.of("randint")], dtype=np.int32)
    loss = weighted_loss(TAG, strong, weak, other["at_out"])
    loss.backward()
    out["win_ft_loss"], out["win_ft_strong"] = t2n(loss), t2n(strong)
    grads_of(net, out, "win_ft_", heads=False)

    # ---- finetune1-style freezing: the gradient flows through the frozen pooling module to out_norm
    net.zero_grad(set_to_none=True)
    for k, p in net.named_parameters():
        frozen = k.startswith(("f_pool_module.", "decoder.")) or (k.startswith("backbone.") and not k.startswith("backbone.norm."))
        p.requires_grad_(not frozen)
    strong, weak, other = net(mel, encoder_win=False, temp_w=1)
    loss = weighted_loss(TAG, strong, weak, other["at_out"])
    loss.backward()
    out["frozen_loss"] = t2n(loss)
    grads_of(net, out, "frozen_", heads=False)
    assert "out_norm.weight" in out["frozen_grad_names"] and not any(str(n).startswith("f_pool_module.") for n in out["frozen_grad_names"])

    # ---- MLM mode (encoder frozen: recipes/desed/mlm/mlm_passt/passt_mlm_setting.py:5-9)
    net = build_reference(True)
    net.train()
    for p in net.backbone.parameters():
        p.requires_grad_(False)
    torch.manual_seed(MLM_SEED)
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
    grads_of(net, out, "mlm_")
    MG.save(TAG, **out)


def gen_patchout():
    out = {}
    mel = torch.from_numpy(synth.det_uniform(f"{PTAG}/mel", (B, 128, 1000), -1.2, 1.2))
    net = build_reference(False).train()
    net.backbone.s_patchout_f = S_F
    rows = []
    net.backbone.register_forward_hook(lambda _m, _i, o: rows.append([int(r) for r in o["select_f_indices"]]))
    for p in net.parameters():
        p.requires_grad_(True)
    torch.manual_seed(PATCHOUT_SEED)
    strong, weak, other = net(mel, encoder_win=False, temp_w=1)
    assert len(rows) == 1 and len(rows[0]) == 12 - S_F
    out["seed"], out["rows_global"], out["s_patchout_f"] = np.int64(PATCHOUT_SEED), np.asarray(rows[0], dtype=np.int32), np.int64(S_F)
    out["strong"], out["weak"], out["at_out"] = t2n(strong), t2n(weak), t2n(other["at_out"])
    loss = weighted_loss(PTAG, strong, weak, other["at_out"])
    loss.backward()
    out["ft_loss"] = t2n(loss)
    grads_of(net, out, "ft_", heads=False)
    MG.save(PTAG, **out)


def gen_sharp():
    out = {}
    mel = torch.from_numpy(synth.det_uniform(f"{STAG}/mel", (B, 128, 1000), -1.2, 1.2))
    net = build_reference(False, SHARP_GAIN).eval()
    pm = torch.zeros(B, 1000, dtype=torch.bool)
    pm[0, 900:] = True
    with torch.no_grad():
        strong, weak, _ = net(mel, encoder_win=False, temp_w=1)
        s2, w2, _ = net(mel, encoder_win=False, temp_w=0.5, pad_mask=pm)
    out["strong"], out["weak"], out["strong_t05_pad"], out["weak_t05_pad"] = t2n(strong), t2n(weak), t2n(s2), t2n(w2)
    out["qkv_gain"] = np.float64(SHARP_GAIN)

    def sensitivity():
        with torch.no_grad():
            base, _, _ = net(mel, encoder_win=False, temp_w=0.5)
            moves = []
            for seed in NOISE_SEEDS:
                torch.manual_seed(seed)
                h = net.out_norm.register_forward_hook(lambda _m, _i, o: o + NOISE * torch.randn_like(o) * o.abs().clamp_min(0.1))
                s, _, _ = net(mel, encoder_win=False, temp_w=0.5)
                h.remove()
                moves.append(float((s - base).abs().max()))
        return np.asarray(moves)
    out["sens_module"] = sensitivity()
    net.f_pool_name = "mean_pool"           # the same weights behind mean pooling
    out["sens_mean_pool"] = sensitivity()
    out["noise_gain"] = np.float64(out["sens_module"].mean() / out["sens_mean_pool"].mean())
    print(f"   {STAG}: strong moves by {out['sens_module']} with the module, {out['sens_mean_pool']} under mean pooling: noise gain {float(out['noise_gain']):.2f}", flush=True)
    MG.save(STAG, **out)


if __name__ == "__main__":
    torch.manual_seed(0)
    with on_cpu():
        if "sharp" not in sys.argv:
            gen_model()
            gen_patchout()
        gen_sharp()
    for name in (TAG, PTAG, STAG):
        size = os.path.getsize(os.path.join(MG.GOLD, name + ".npz"))
        assert size < 589 * 1024, f"{name}.npz is {size / 1024:.1f} KiB: the fixtures are held below 589 KiB"
