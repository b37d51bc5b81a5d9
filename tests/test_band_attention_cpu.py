"""Host side of the context network's local attention window (`PaSST_SED(decoder_win_len=...)`, reference
src/models/passt/passt_sed.py:54,137,173-178): constructor contract, the persistent `decoder.att_mask` buffer (checkpoint interchange:
src/models/transformer_decoder.py:96-108, mask.py:7-23), refusals, and the two C entry points.  No GPU needed."""
import ctypes
import os

import numpy as np
import pytest
import torch

from transformer4sed_amd.passt_sed import PaSST_SED

T, HEADS = 1000, 12
HEAD_WIDTHS = [8, 16, 32, 64, 100, 128, 200, 256, 400, 600, 1000, 2000]


def build(win, **kw):
    return PaSST_SED(decoder="transformerXL", decoder_layer_num=3, at_adapter=True, load_pretrained_model=False, encoder_depth=1,
                     passt_feature_layer=1, decoder_win_len=win, **kw)


def closed_form(w):
    """~((j >= i - hw) & (j < i + hw)), hw = w // 2: hw keys to the left, the key itself, hw - 1 to the right."""
    i = torch.arange(T).unsqueeze(1)
    j = torch.arange(T).unsqueeze(0)
    return ~((j >= i - w // 2) & (j < i + w // 2))


def from_bounds(b):
    """The mask a fixture's per-row [lo, hi) bounds (read off the reference's own buffer, tools/gen_band_golden.py) describe."""
    b = torch.from_numpy(b.astype(np.int64))
    j = torch.arange(T)
    return ~((j >= b[..., :1]) & (j < b[..., 1:]))


def test_constructs_with_one_width(golden):
    net = build(100)
    m = net.state_dict()["decoder.att_mask"]
    assert m.dtype == torch.bool and tuple(m.shape) == (T, T)
    assert torch.equal(m, closed_form(100))
    g = golden("model_d768_l2_win100")
    assert g["win_len"].tolist() == [100] and torch.equal(m, from_bounds(g["mask_bounds"]))
    assert net.decoder.half_widths == [50] * HEADS
    # row 500 sees the keys 450 .. 549: the right edge is exclusive
    assert (~m[500]).nonzero().flatten().tolist() == list(range(450, 550))
    assert dict(net.named_buffers())["decoder.att_mask"] is net.decoder.att_mask       # a buffer, not a parameter
    assert all(not n.endswith("att_mask") for n, _ in net.named_parameters())


def test_constructs_with_one_width_per_head(golden):
    for widths in (HEAD_WIDTHS, tuple(HEAD_WIDTHS)):
        net = build(widths)
        m = net.state_dict()["decoder.att_mask"]
        assert m.dtype == torch.bool and tuple(m.shape) == (HEADS, T, T)
        for h, w in enumerate(HEAD_WIDTHS):
            assert torch.equal(m[h], closed_form(w)), h
        assert net.decoder.half_widths == [w // 2 for w in HEAD_WIDTHS]
    g = golden("model_d768_l2_winheads")
    assert g["win_len"].tolist() == HEAD_WIDTHS and torch.equal(m, from_bounds(g["mask_bounds"]))
    assert not bool(m[11].any())          # hw = 1000 >= T: that head sees everything


def test_pmam_model_takes_the_window():
    from transformer4sed_amd.passt_cnn import PaSST_CNN
    cnn = dict(n_in_channel=1, activation="cg", conv_dropout=0, kernel_size=[3] * 2, padding=[1] * 2, stride=[1] * 2, nb_filters=[16, 32],
               pooling=[[1, 8], [1, 16]])
    sed = dict(passt_feature_layer=1, f_pool="attention", decoder="transformerXL", decoder_layer_num=1, decoder_dim=384, at_adapter=True,
               load_pretrained_model=False, encoder_depth=1, class_num=10)
    net = PaSST_CNN(passt_sed_param=dict(sed, decoder_win_len=64), cnn_param=cnn)
    assert torch.equal(net.state_dict()["decoder.att_mask"], closed_form(64))
    assert "decoder.att_mask" not in PaSST_CNN(passt_sed_param=sed, cnn_param=cnn).state_dict()
    # its engine walks the one Transformer-XL schedule (windowed or not), overriding pieces of it only
    from transformer4sed_amd.engine import SedEngine
    from transformer4sed_amd.pmam_engine import PmamEngine
    assert isinstance(net._make_engine(), PmamEngine)
    assert PmamEngine._decoder_fwd is SedEngine._decoder_fwd and PmamEngine._decoder_bwd is SedEngine._decoder_bwd


def test_state_dict_round_trip_and_absent_key():
    a, b = build(100), build(100)
    sd = a.state_dict()
    assert "decoder.att_mask" in sd
    missing, unexpected = b.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    plain = build(None)
    assert "decoder.att_mask" not in plain.state_dict() and plain.decoder.att_mask is None and plain.decoder.half_widths is None
    with pytest.raises(RuntimeError, match="att_mask"):       # a windowed checkpoint into a model built without the window
        plain.load_state_dict(sd, strict=True)
    with pytest.raises(RuntimeError, match="att_mask"):       # and the other way round
        b.load_state_dict(plain.state_dict(), strict=True)
    import copy
    t = copy.deepcopy(a)                                      # a teacher copy carries the buffer and the widths
    assert torch.equal(t.decoder.att_mask, a.decoder.att_mask) and t.decoder.half_widths == a.decoder.half_widths


def test_refusals():
    for w in (1, 0, -4, [100] * 11 + [1]):
        with pytest.raises(ValueError):
            build(w)
    for w in ([100] * 11, [100] * 13, []):
        with pytest.raises(ValueError):
            build(w)
    for w in (100.0, "100", [100.0] * 12, True):
        with pytest.raises(TypeError):
            build(w)
    # a loaded mask that is not this model's diagonal band: the kernels cannot express it
    net = build(100)
    sd = net.state_dict()
    other = dict(sd)
    other["decoder.att_mask"] = closed_form(102)
    with pytest.raises(RuntimeError, match="diagonal band"):
        net.load_state_dict(other, strict=True)
    assert torch.equal(net.decoder.att_mask, closed_form(100))          # and the model's own buffer is untouched
    off_by_one = dict(sd)
    m = closed_form(100).clone()
    m[500, 550] = False                                                  # one extra key on the right edge of one row
    off_by_one["decoder.att_mask"] = m
    with pytest.raises(RuntimeError, match="diagonal band"):
        net.load_state_dict(off_by_one, strict=True)


def test_library_exports_the_band_entry_points():
    from transformer4sed_amd import _lib, build as B
    protos = _lib.parse_header()
    dll = ctypes.CDLL(B.build(verbose=False))
    for name, base in (("sed_relpos_attn_band_fwd", "sed_relpos_attn_fwd"), ("sed_relpos_attn_band_bwd", "sed_relpos_attn_bwd")):
        assert name in protos and hasattr(dll, name)
        # the unbanded argument list, plus `half_width` (a pointer) before the stream
        assert [n for _, n in protos[name]] == [n for _, n in protos[base]][:-1] + ["half_width", "stream"]
        assert protos[name][-2][0] is ctypes.c_void_p
    src = open(_lib.HEADER_PATH).read()
    assert "mask.py:7-23" in src and "transformer_decoder.py:96-119" in src
    assert "#define SED_HIP_ABI_VERSION 7" in " ".join(src.split())
