"""The frequency-wise transformer pooling without a GPU: constructor, parameter contract, fixtures and ABI
(`PaSST_SED(f_pool="frequency_wise_tranformer_encoder")`, src/models/pooling.py:18-34)."""
import ctypes
import os

import pytest
import torch

from transformer4sed_amd import synth
from transformer4sed_amd.passt_sed import PaSST_SED

FPOOL = "frequency_wise_tranformer_encoder"
FIXTURES = ("model_d768_l2_fpooltr", "model_d768_l2_fpooltr_patchout4")
NEW_ENTRY_POINTS = ("sed_fpool_seq_build_fwd", "sed_fpool_seq_build_bwd", "sed_fpool_rownorm_fwd", "sed_fpool_rownorm_bwd",
                    "sed_attn_short_fwd", "sed_attn_short_bwd")
LR = {"encoder": {"lr": 5e-6, "weight_decay": 1e-4, "freeze_layer": 1, "step_lr": 4},
      "decoder": {"lr": 1e-4, "weight_decay": 1e-4}, "head": {"lr": 1e-4, "weight_decay": 1e-4}}


def build(**kw):
    kw = dict(dict(decoder="transformerXL", decoder_layer_num=2, at_adapter=True, load_pretrained_model=False, passt_feature_layer=2,
                   f_pool=FPOOL, encoder_depth=2), **kw)      # (the fixtures' encoder is truncated to two blocks)
    return PaSST_SED(**kw)


def pool_names(net):
    return [n for n, _ in net.named_parameters() if n.startswith("f_pool_module.")]


def test_state_dict_is_the_references(golden):
    """Names, order and shapes of `state_dict()` equal the reference model's (recorded by tools/gen_fpool_transformer_golden.py)."""
    g = golden(FIXTURES[0])
    want = [(str(n), tuple(int(d) for d in str(s).split(",") if d)) for n, s in zip(g["state_names"], g["state_shapes"])]
    got = [(k, tuple(v.shape)) for k, v in build().state_dict().items()]
    assert got == want, set(got) ^ set(want)
    pool = dict((k, s) for k, s in got if k.startswith("f_pool_module."))
    assert len(pool) == 26 and sum(int(torch.Size(s).numel()) for s in pool.values()) == 14174208
    assert pool["f_pool_module.linear_emb.weight"] == (768, 1)
    assert pool["f_pool_module.frequency_transformer.1.attn.qkv.weight"] == (2304, 768)
    assert "f_pool_module.frequency_transformer.0.attn.qkv.bias" not in pool
    assert pool["f_pool_module.frequency_transformer.0.mlp.fc1.weight"] == (3072, 768)


@pytest.mark.parametrize("kw", [dict(), dict(decoder="conformer"), dict(mlm=True, mlm_dict=dict(out_dim=768)), dict(s_patchout_f=11),
                                dict(decoder_win_len=100)])
def test_synth_weights_load_strictly(kw):
    net = build(**kw)
    mk = synth.conformer_state_dict_np if kw.get("decoder") == "conformer" else synth.matsed_state_dict_np
    sd = mk(tag="wft768", dec_layers=2, depth=2, mlm=bool(kw.get("mlm")))
    sd.update({k: v for k, v in synth.fpool_transformer_state_dict_np(tag="wft768", dec_layers=0, depth=0).items() if k.startswith("f_pool_module.")})
    sd = {k: torch.from_numpy(v) for k, v in sd.items()}
    if "decoder.att_mask" in net.state_dict():
        sd["decoder.att_mask"] = net.state_dict()["decoder.att_mask"]
    missing, unexpected = net.load_state_dict(sd, strict=True)
    assert not missing and not unexpected and set(net.state_dict()) == set(sd)
    m = net.f_pool_module
    assert abs(float(m.frequency_transformer_norm.weight.detach().mean()) - 1) < 0.05
    assert abs(float(m.frequency_transformer[0].norm1.weight.detach().mean()) - 1) < 0.05
    # (uniform in +-1: mean |w| 0.5; unit gain, uniform in +-sqrt(3 / 768): mean |w| 0.03125)
    assert float(m.linear_emb.weight.detach().abs().mean()) > 0.25 and float(m.frequency_transformer[1].attn.qkv.weight.detach().abs().mean()) > 0.03


def test_existing_synth_functions_are_unchanged_by_the_new_one():
    """`fpool_transformer_state_dict_np` = the depth-2 synth state + the 26 tensors; the tensors every committed golden depends on keep their bytes."""
    new = synth.fpool_transformer_state_dict_np(tag="w768", dec_layers=2, depth=2)
    old = synth.matsed_state_dict_np(tag="w768", dec_layers=2, depth=2)
    assert set(new) - set(old) == set(synth.fpool_transformer_shapes()) and len(set(new) - set(old)) == 26
    assert all(new[k].tobytes() == v.tobytes() for k, v in old.items())


def test_refusals_stay():
    from transformer4sed_amd.dasm import DASM
    from transformer4sed_amd.passt_cnn import PaSST_CNN
    for bad in ("frequency_wise_transformer_encoder", "max_pool", "attention"):      # (the correct spelling is not the reference's)
        with pytest.raises(NotImplementedError, match="f_pool"):
            build(f_pool=bad)
    with pytest.raises(NotImplementedError, match="f_pool"):
        PaSST_SED(decoder="conformer", f_pool="attention", load_pretrained_model=False)
    for kw in (dict(decoder="gru"), dict(decoder="transformer"), dict(decoder="no")):
        with pytest.raises(NotImplementedError, match="decoder="):
            build(**kw)
    with pytest.raises(NotImplementedError, match="s_patchout_t"):
        build(s_patchout_t=10)
    with pytest.raises(ValueError):
        build(s_patchout_f=12)
    passt = dict(class_num=30, f_pool=FPOOL, decode_ratio=10, at_adapter=True, decoder="transformerXL", decoder_layer_num=1,
                 decoder_pos_emd_len=1000, decoder_dim=384, mlm=False, load_pretrained_model=False, passt_feature_layer=1, encoder_depth=1)
    cnn = dict(n_in_channel=1, activation="cg", conv_dropout=0, kernel_size=[3] * 10, padding=[1] * 10, stride=[1] * 10,
               nb_filters=list(synth.PMAM_FILTERS), pooling=[list(p) for p in synth.PMAM_POOLING])
    with pytest.raises(NotImplementedError, match="f_pool"):
        PaSST_CNN(passt_sed_param=passt, cnn_param=cnn)
    # (DASM fixes its pooling to "attention" and takes no f_pool argument; the constructor branch it shares with PaSST_CNN refuses the value)
    with pytest.raises(TypeError):
        DASM(cnn_param=cnn, f_pool=FPOOL, at_param=dict(at_decoder_layer=2, query_projector=True, query_dim=1024, out_type="sigmoid"))
    with pytest.raises(NotImplementedError, match="f_pool"):
        PaSST_SED(_pmam=True, f_pool=FPOOL, decoder="transformerXL", decoder_dim=384, load_pretrained_model=False, encoder_depth=1)


def test_param_groups_gradient_names_and_stage():
    """The name-driven plumbing: recipe parameter groups, the model's gradient-name set, the data-parallel stage of a name."""
    from transformer4sed_amd import ddp
    from transformer4sed_amd.engine import SedEngine
    from transformer4sed_amd.trainer import get_params
    net = build()
    pool = set(pool_names(net))
    assert len(pool) == 26
    groups = get_params(net, LR)
    dec_group = {n for n, _ in groups[-2]["params"]}
    assert pool <= dec_group and {n for n in dec_group - pool if not n.startswith("decoder.")} == set()
    assert pool <= net._grad_names()
    assert {ddp.stage_of(n, 2) for n in pool} == {"heads"} == {ddp.stage_of("out_norm.weight", 2)}
    assert all(n.startswith(SedEngine._BELOW_HEADS) for n in pool)
    mlm = build(mlm=True, mlm_dict=dict(out_dim=768))
    mlm._last_mask_effective = False
    assert pool <= mlm._grad_names()


def test_finetune1_freezing_keeps_out_norm_trainable_under_the_frozen_module():
    """Decoder lr 0 (recipes/desed/finetune/passt/setting.py) freezes `f_pool_module.*` with the context network; out_norm and backbone.norm
    stay trainable, and a backward still has to walk through the frozen module to reach them."""
    from transformer4sed_amd.engine import SedEngine
    from transformer4sed_amd.trainer import get_params
    net = build()
    get_params(net, {"encoder": {"lr": 0.0, "weight_decay": 1e-4}, "decoder": {"lr": 0.0, "weight_decay": 1e-4},
                     "head": {"lr": 1e-4, "weight_decay": 1e-4}})
    names = net._grad_names()
    assert {"out_norm.weight", "out_norm.bias", "backbone.norm.weight", "backbone.norm.bias", "classifier.weight"} <= names
    assert not any(n.startswith(("f_pool_module.", "decoder.", "backbone.blocks.")) for n in names)
    eng = SedEngine(net)
    assert eng._walks_decoder_fwd() and eng._lowest_trainable_fwd(net.depth) == net.depth
    views = {n: torch.zeros(1) for n in names}
    assert eng._walks_decoder(views.get, net.depth) and eng._lowest_trainable(views.get, net.depth) == (net.depth, False)


def test_abi_additions_only():
    from transformer4sed_amd import _lib, build as B
    protos = _lib.parse_header()
    dll = ctypes.CDLL(B.build(verbose=False))
    for name in NEW_ENTRY_POINTS:
        assert name in protos and hasattr(dll, name), name
        assert protos[name][-1] == (ctypes.c_void_p, "stream")
    assert "fpool_transformer.hip" in B.SOURCES
    src = open(_lib.HEADER_PATH).read()
    assert "#define SED_HIP_ABI_VERSION 7" in " ".join(src.split())


def test_fixture_guards_shapes_and_sizes(golden):
    """A 1e-3 parity test must not be passable by a kernel that ignores the attention weights or the tag row."""
    g, gp = golden(FIXTURES[0]), golden(FIXTURES[1])
    assert float(g["strong_vs_uniform_attention_max"]) >= 20e-3 and float(g["strong_vs_zero_tag_max"]) >= 20e-3
    pool = {str(n) for n in g["state_names"] if str(n).startswith("f_pool_module.")}
    assert len(pool) == 26
    for key in ("ft_grad_names", "win_ft_grad_names", "mlm_grad_names"):
        assert pool <= {str(n) for n in g[key]}, key
    frozen = {str(n) for n in g["frozen_grad_names"]}
    assert {"out_norm.weight", "out_norm.bias", "backbone.norm.weight"} <= frozen
    assert not any(n.startswith(("f_pool_module.", "decoder.", "backbone.blocks.")) for n in frozen)
    assert g["strong"].shape == g["strong_t05_pad"].shape == g["strong_win"].shape == g["win_ft_strong"].shape == (2, 10, 1000)
    assert g["weak"].shape == g["weak_win"].shape == g["at_out"].shape == (2, 10)
    assert g["pooled_s"].shape == (29, 48) and g["interp_s"].shape == (2, 40, 48) and g["mlm_pred_s"].shape == (2, 40, 48)
    assert g["win_toffsets"].shape == (11,) and len(g["ft_grad_names"]) == len(g["ft_grad_norms"]) == len(g["ft_grad_heads"])
    assert gp["strong"].shape == (2, 10, 1000) and gp["rows_global"].shape == (8,) and int(gp["s_patchout_f"]) == 4
    assert list(gp["rows_global"]) == sorted(set(int(r) for r in gp["rows_global"])) and pool <= {str(n) for n in gp["ft_grad_names"]}
    gs = golden("model_d768_l2_fpooltr_sharp")          # sharp attention: the reference's own noise gain over mean pooling, recorded
    assert gs["sens_module"].shape == gs["sens_mean_pool"].shape == (3,) and gs["strong"].shape == gs["strong_t05_pad"].shape == (2, 10, 1000)
    assert abs(float(gs["noise_gain"]) - float(gs["sens_module"].mean() / gs["sens_mean_pool"].mean())) < 1e-12 and float(gs["noise_gain"]) > 1
    for tag in FIXTURES + ("model_d768_l2_fpooltr_sharp",):
        assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", tag + ".npz")) < 589 * 1024
