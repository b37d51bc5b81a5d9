"""The context network walked frozen (`trainable=False`, no gradient view for any of its tensors) against the same walk with every
`decoder.*` gradient taken, on both engines (needs an MI355X): SedEngine's Transformer-XL at 768 and PmamEngine's 384-wide one, which
run one schedule (`SedEngine._decoder_fwd` / `_decoder_bwd`) and differ in the LayerNorm form, the bias triple and the gradient sink.

Networks as tools/context_dump.py builds them, T = 200 (Tpad = 256), called through `_decoder_fwd(save=True)` / `_decoder_bwd` directly.
B = 2 (M = 400 < 1024): transposed-copy weight gradients on the main stream, three-term in_proj for the 768-wide network.  B = 6
(M = 1200): the TN weight-gradient kernel on the side stream, two-term in_proj.

Input gradient, frozen against trainable: no dX kernel reads a dW product, so the two walks launch the same kernels on the same values
along the input-gradient path.  The frozen walk runs twice: without any gradient view (`{}.get`), and with every view offered
(`trainable=False` alone must keep the engine from writing through them).  Measured on the commit before the schedules were merged (each engine's own schedule) and on this one:
max|a - b| / max|a| = 0 in all six cases -- asserted bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from transformer4sed_amd import synth  # noqa: E402
from transformer4sed_amd.ops import call  # noqa: E402

DEV = "cuda"
T = 200
_NETS = {}


def network(kind, win):
    """The model (synth weights, train mode) with a fresh engine; built once per (kind, window)."""
    if (kind, win) in _NETS:
        return _NETS[kind, win]
    if kind == "pmam":
        from transformer4sed_amd.passt_cnn import PaSST_CNN
        passt = dict(class_num=30, f_pool="attention", decode_ratio=10, at_adapter=True, decoder="transformerXL", decoder_layer_num=3,
                     decoder_pos_emd_len=T, decoder_dim=384, mlm=True, lora_config=dict(r=8, lora_alpha=1, requires_grad_pretrain=False),
                     mlm_dict=dict(strategy="block", block_width=10, mask_rate=0.8, out_dim=768, mask_style=[0.9, 0.05, 0.05]),
                     load_pretrained_model=False, passt_feature_layer=2, encoder_depth=2, decoder_win_len=win)
        cnn = dict(n_in_channel=1, activation="cg", conv_dropout=0, kernel_size=[3] * 10, padding=[1] * 10, stride=[1] * 10,
                   nb_filters=list(synth.PMAM_FILTERS), pooling=[list(p) for p in synth.PMAM_POOLING])
        net, sd = PaSST_CNN(passt_sed_param=passt, cnn_param=cnn), synth.pmam_state_dict_np(depth=12)
    else:
        from transformer4sed_amd.passt_sed import PaSST_SED
        net = PaSST_SED(passt_feature_layer=2, f_pool="mean_pool", decode_ratio=10, at_adapter=True, decoder_layer_num=2,
                        decoder="transformerXL", decoder_pos_emd_len=T, load_pretrained_model=False, encoder_depth=2, decoder_win_len=win)
        sd = synth.matsed_state_dict_np(depth=2, dec_layers=2)
    own = net.state_dict()      # (the synth weights carry no window mask: the model's own buffer is the constructor's)
    net.load_state_dict({k: (own[k] if k == "decoder.att_mask" else torch.from_numpy(np.asarray(sd[k]))) for k in own}, strict=True)
    net = net.to(DEV).train()
    net.engine = net._make_engine()
    _NETS[kind, win] = net
    return net


def walk(net, kind, x, gout, trainable, offer=False):
    """`_decoder_fwd(save=True)` + `_decoder_bwd` -> (output, input gradient, {name: gradient} of every decoder.* tensor, zeroed
    before the walk).  A frozen walk (`trainable` false) is given no gradient view at all, or, with `offer`, every view the trainable
    walk gets -- the engine then holds the pointers and must still leave them alone."""
    eng = net.engine
    B = x.shape[0]
    grads = {n: torch.zeros_like(p) for n, p in net.named_parameters() if n.startswith("decoder.")}
    G = grads.get if (trainable or offer) else {}.get
    W = eng._weights(need_t=True)
    lease = eng._lease(True)        # (as the full forward does: the saved transposed images come from the engine's pool)
    y, dctx = eng._decoder_fwd(W, x, True)
    scatter = {}
    if kind == "pmam":      # (as PmamEngine._context_bwd: the padded gradient images, returned to the masters after the walk)
        dctx["slots"], scatter = eng._grad_slots(B, torch.device(DEV, 0), G, trainable, False)
    gin = eng._decoder_bwd(W, dctx, gout.clone(), G, trainable)
    eng._join_dw()
    if "dec" in scatter:
        call("sed_scatter_add_f32", *scatter["dec"])
    torch.cuda.synchronize()
    del dctx, lease
    return y, gin, grads


@pytest.mark.parametrize("kind,B,win", [("xl", 2, None), ("xl", 6, None), ("pmam", 2, None), ("pmam", 6, None), ("pmam", 2, 100),
                                        ("pmam", 6, 100)])
def test_frozen_context_network(kind, B, win):
    net = network(kind, win)
    width = 384 if kind == "pmam" else 768
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn(B, T, width, device=DEV, generator=g)
    gout = torch.randn(B, T, width, device=DEV, generator=g)
    y_t, gin_t, grads_t = walk(net, kind, x, gout, True)
    y_f, gin_f, grads_f = walk(net, kind, x, gout, False)
    y_o, gin_o, grads_o = walk(net, kind, x, gout, False, offer=True)
    assert grads_t and y_t.shape == x.shape and gin_t.shape == x.shape
    assert bool(torch.isfinite(y_t).all()) and torch.equal(y_t, y_f) and torch.equal(y_t, y_o)
    for n, t in list(grads_f.items()) + list(grads_o.items()):
        assert not bool(t.any()), f"frozen walk wrote a gradient of {n}"
    for n, p in net.named_parameters():      # (nor did any walk reach the parameters' own .grad past the views it was given)
        assert not n.startswith("decoder.") or p.grad is None, n
    for n, t in grads_t.items():
        assert bool(torch.isfinite(t).all()) and bool(t.any()), n
    rel = float((gin_t - gin_f).abs().max() / gin_t.abs().max())
    print(f"{kind} B={B} win={win}: input gradient frozen vs trainable max|a-b|/max|a| = {rel:.3e} on scale {float(gin_t.abs().max()):.3e}")
    assert bool(torch.isfinite(gin_t).all()) and float(gin_t.abs().max()) > 0
    assert torch.equal(gin_t, gin_f) and torch.equal(gin_t, gin_o)
