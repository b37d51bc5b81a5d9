"""The Conformer context network without a GPU: constructor, parameter contract, fixtures and ABI (`PaSST_SED(decoder="conformer")`)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from transformer4sed_amd import synth
from transformer4sed_amd.passt_sed import PaSST_SED

LOGDIR = os.environ.get("SED_TEST_LOG_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_logs")
FIXTURES = (("model_d768_l2_conformer", None), ("model_d768_l2_conformer_win100", 100))
NEW_ENTRY_POINTS = ("sed_conv_glu_dw_fwd", "sed_conv_glu_dw_bwd", "sed_swish_fwd", "sed_swish_bwd", "sed_scale_add_f32")


def build(win=None, **kw):
    return PaSST_SED(decoder="conformer", decoder_layer_num=2, at_adapter=True, load_pretrained_model=False, passt_feature_layer=2,
                     f_pool="mean_pool", encoder_depth=2, decoder_win_len=win, **kw)      # (the fixtures' encoder is truncated to two blocks)


@pytest.mark.parametrize("tag,win", FIXTURES)
def test_state_dict_is_the_references(golden, tag, win):
    """Names and shapes of `state_dict()` equal the reference model's (recorded by tools/gen_conformer_golden.py), with and without a window."""
    g = golden(tag)
    want = {str(n): tuple(int(d) for d in str(s).split(",") if d) for n, s in zip(g["state_names"], g["state_shapes"])}
    got = {k: tuple(v.shape) for k, v in build(win).state_dict().items()}
    assert got == want, (set(got) ^ set(want), [(k, got[k], want[k]) for k in set(got) & set(want) if got[k] != want[k]])
    blk = {k: s for k, s in got.items() if k.startswith("decoder.blocks.0.")}
    assert len(blk) == 33
    assert blk["decoder.blocks.0.conv_module.pointwise_conv1.weight"] == (1536, 768, 1)
    assert blk["decoder.blocks.0.conv_module.depthwise_conv.weight"] == (768, 1, 31)
    assert ("decoder.att_mask" in got) == (win is not None)


@pytest.mark.parametrize("win", [None, 100])
def test_synth_weights_load_strictly(win):
    net = build(win)
    sd = {k: torch.from_numpy(v) for k, v in synth.conformer_state_dict_np(dec_layers=2, depth=2).items()}
    if win is not None:      # the synth weights carry no mask: the buffer is the constructor's own
        sd["decoder.att_mask"] = net.state_dict()["decoder.att_mask"]
    missing, unexpected = net.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    w = net.decoder.blocks[1].conv_module.depthwise_conv.weight
    assert float(w.detach()[:, :, :15].abs().mean()) > 0.1 and abs(float(net.decoder.blocks[0].norm_final.weight.detach().mean()) - 1) < 0.05
    # both directions: the holder's state_dict loads into a plain dict round trip with the same keys
    assert set(net.state_dict()) == set(sd)


def test_window_buffer_behaves_like_the_xl_decoders():
    from transformer4sed_amd.passt_sed import band_mask
    net = build(100)
    assert torch.equal(net.decoder.att_mask, band_mask(1000, 50)) and net.decoder.half_widths == [50] * 12
    sd = dict(net.state_dict())
    sd["decoder.att_mask"] = band_mask(1000, 51)
    with pytest.raises(RuntimeError, match="diagonal band"):
        net.load_state_dict(sd, strict=True)
    assert build(None).decoder.att_mask is None


@pytest.mark.parametrize("win", [[100] * 12, (8, 16), 100.0, True])
def test_sequence_window_is_refused(win):
    with pytest.raises(TypeError, match="one int or None"):
        build(win)


def test_other_refusals_stay():
    for kw in (dict(decoder="gru"), dict(decoder="transformer"), dict(decoder="no")):
        with pytest.raises(NotImplementedError, match="decoder="):
            PaSST_SED(load_pretrained_model=False, **kw)
    with pytest.raises(NotImplementedError, match="f_pool"):
        PaSST_SED(decoder="conformer", f_pool="attention", load_pretrained_model=False)
    with pytest.raises(NotImplementedError, match="LoRA"):
        PaSST_SED(decoder="conformer", lora_config=dict(r=8), load_pretrained_model=False)


def test_pmam_and_dasm_still_refuse_conformer():
    from transformer4sed_amd.dasm import DASM
    from transformer4sed_amd.passt_cnn import PaSST_CNN
    passt = dict(class_num=30, f_pool="attention", decode_ratio=10, at_adapter=True, decoder="conformer", decoder_layer_num=1,
                 decoder_pos_emd_len=1000, decoder_dim=384, mlm=False, load_pretrained_model=False, passt_feature_layer=1, encoder_depth=1)
    cnn = dict(n_in_channel=1, activation="cg", conv_dropout=0, kernel_size=[3] * 10, padding=[1] * 10, stride=[1] * 10,
               nb_filters=list(synth.PMAM_FILTERS), pooling=[list(p) for p in synth.PMAM_POOLING])
    with pytest.raises(NotImplementedError, match="decoder='conformer'"):
        PaSST_CNN(passt_sed_param=passt, cnn_param=cnn)
    with pytest.raises(NotImplementedError, match="decoder='conformer'"):
        DASM(cnn_param=cnn, decoder="conformer", at_param=dict(at_decoder_layer=2, query_projector=True, query_dim=1024, out_type="sigmoid"))


def test_param_groups_and_gradient_names_cover_the_new_parameters():
    """The name-driven plumbing: recipe parameter groups, the model's gradient-name set, the data-parallel stage of a name."""
    from transformer4sed_amd import ddp
    from transformer4sed_amd.trainer import get_params
    net = build(None)
    dec = {n for n, _ in net.named_parameters() if n.startswith("decoder.blocks.")}
    assert len(dec) == 66
    groups = get_params(net, {"encoder": {"lr": 5e-6, "weight_decay": 1e-4, "freeze_layer": 1, "step_lr": 4},
                              "decoder": {"lr": 1e-4, "weight_decay": 1e-4}, "head": {"lr": 1e-4, "weight_decay": 1e-4}})
    assert {n for n, _ in groups[-2]["params"]} == dec
    assert dec <= net._grad_names()
    assert {ddp.stage_of(n, 2) for n in dec} == {"decoder"}


def test_abi_additions_only():
    from transformer4sed_amd import _lib, build as B
    protos = _lib.parse_header()
    dll = ctypes.CDLL(B.build(verbose=False))
    for name in NEW_ENTRY_POINTS:
        assert name in protos and hasattr(dll, name), name
        assert protos[name][-1] == (ctypes.c_void_p, "stream")
    assert "conformer.hip" in B.SOURCES
    src = open(_lib.HEADER_PATH).read()
    assert "#define SED_HIP_ABI_VERSION 7" in " ".join(src.split())


@pytest.mark.parametrize("tag,win", FIXTURES)
def test_fixture_guards(golden, tag, win):
    """A 1e-3 parity test must not be passable by a kernel that ignores the off-centre taps or the window."""
    g = golden(tag)
    assert float(g["strong_vs_centre_tap_max"]) >= 20e-3
    if win is not None:
        assert float(g["strong_vs_full_max"]) >= 20e-3 and list(g["win_len"]) == [win]
    names = {str(n) for n in g["ft_grad_names"]}
    assert {n for n in names if n.startswith("decoder.blocks.")} == {str(n) for n in g["state_names"] if str(n).startswith("decoder.blocks.")}
    assert g["strong"].shape == (2, 10, 1000) and os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", tag + ".npz")) < 589 * 1024
