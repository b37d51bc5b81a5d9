#!/usr/bin/env python
"""Generate tests/golden/model_d768_l2_win100.npz and model_d768_l2_winheads.npz: the depth-2 synth-weight REFERENCE model of
oracle/make_golden.py (`build_reference_model`, imported, not copied) with a local attention window in its context network --
`PaSST_SED(decoder_win_len=...)`, src/models/passt/passt_sed.py:54,137,173-178.  One width (100) for all heads, and one width per head.

Each file holds the key set of `model_fixture(..., do_windows=False, do_grads=True)` (finetune-mode outputs, strided block probes and
gradient norms; MLM-mode prediction, loss, recorded mask draws and gradient norms) plus
  * `win_len`: the widths; `mask_bounds`: per (head,) query row the [lo, hi) range of keys the reference's mask allows -- read off the
    `att_mask` buffer that the reference's own `TransformerXLDecoder(window_len=...)` constructor makes;
  * `strong_vs_full_max` / `strong_vs_full_median`: distance of `strong` from the full-window reference model on the same input.  The
    generator asserts max >= 20 x 1e-3, so a parity test at 1e-3 cannot pass on a model that ignores the window.

Run on the authoring machine (needs the reference tree that oracle/make_golden.py imports):  python tools/gen_band_golden.py
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import make_golden as MG  # noqa: E402  (puts the reference and its shims on sys.path)
from transformer4sed_amd import synth  # noqa: E402

HEAD_WIDTHS = [8, 16, 32, 64, 100, 128, 200, 256, 400, 600, 1000, 2000]
FIXTURES = (("model_d768_l2_win100", 100), ("model_d768_l2_winheads", HEAD_WIDTHS))
T, HEADS, B = 1000, 12, 2


def reference_mask(win_len):
    """The `att_mask` buffer of the reference's own decoder constructor (transformer_decoder.py:96-108)."""
    from src.models.transformer_decoder import TransformerXLDecoder
    dec = TransformerXLDecoder(input_dim=768, seq_len=T, decoder_layer_num=1, window_len=win_len, num_heads=HEADS)
    mask = dec.att_mask
    assert mask.dtype == torch.bool and tuple(mask.shape) == ((T, T) if isinstance(win_len, int) else (HEADS, T, T))
    return mask


def mask_bounds(mask):
    """[..., T, 2]: first allowed key and one past the last, per query row; asserts that the allowed keys are one contiguous run."""
    allowed = ~mask
    lo = allowed.int().argmax(-1)
    n = allowed.sum(-1)
    j = torch.arange(T)
    assert torch.equal(allowed, (j >= lo.unsqueeze(-1)) & (j < (lo + n).unsqueeze(-1)))
    return torch.stack([lo, lo + n], -1).to(torch.int16)


def gen(tag, win_len):
    mask = reference_mask(win_len)
    widths = [win_len] * HEADS if isinstance(win_len, int) else list(win_len)
    i, j = torch.arange(T).unsqueeze(1), torch.arange(T).unsqueeze(0)
    closed = torch.stack([~((j >= i - w // 2) & (j < i + w // 2)) for w in widths])
    assert torch.equal(mask if mask.ndim == 3 else mask.unsqueeze(0).expand(HEADS, T, T), closed), "closed form != diagonal_mask"

    o_build, o_save = MG.build_reference_model, MG.save
    captured = {}

    def build(*a, **k):
        net = o_build(*a, **k)
        net.decoder.att_mask = mask.clone()          # the registered (None) buffer of the decoder built without a window
        assert "decoder.att_mask" in net.state_dict() and torch.equal(net.decoder.att_mask, reference_mask(win_len))
        return net

    MG.build_reference_model, MG.save = build, (lambda name, **arrays: captured.update(arrays))
    try:
        MG.model_fixture(tag, embed_dim=768, depth=2, feature_layer=2, B=B, do_windows=False, do_grads=True)
    finally:
        MG.build_reference_model, MG.save = o_build, o_save
    # the full-window reference on the same input: how far the window moves the posteriors
    mel = torch.from_numpy(synth.det_uniform(f"{tag}/mel", (B, 128, 1000), -1.2, 1.2))
    full = MG.build_reference_model(768, False, 2, 2).eval()
    with torch.no_grad():
        strong_full, _, _ = full(mel, encoder_win=False, temp_w=1)
    d = (torch.from_numpy(captured["strong"]) - strong_full).abs()
    captured["strong_vs_full_max"] = np.float64(d.max())
    captured["strong_vs_full_median"] = np.float64(d.median())
    print(f"   {tag}: strong vs full window max {float(d.max()):.4f} median {float(d.median()):.4f}", flush=True)
    assert float(d.max()) >= 20 * 1e-3, "the window does not move the output enough for a 1e-3 parity test to notice it"
    captured["win_len"] = np.asarray(widths if not isinstance(win_len, int) else [win_len], dtype=np.int32)
    captured["mask_bounds"] = mask_bounds(mask).numpy()
    MG.save(tag, **captured)


if __name__ == "__main__":
    for tag, w in FIXTURES:
        gen(tag, w)
