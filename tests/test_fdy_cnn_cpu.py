"""`PaSST_CNN(cnn_param={"cnn_name": "FDY-CNN", ...})` without a GPU: the module's state_dict contract against the names the reference
module recorded (tests/golden/pmam_fdy_d2.npz), every refusal, the plain-torch restatement of tests/fdy_cases.py against the reference's
recorded outputs (which licenses it as the checker of the kernels in tests/test_gpu_fdy_cnn.py), the fixture guards, the name-driven
plumbing (parameter groups, gradient names, buffer synchronisation) and the C ABI additions."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

import fdy_cases as FC
from transformer4sed_amd import synth

PASST = dict(class_num=30, f_pool="attention", decode_ratio=10, at_adapter=True, decoder="transformerXL", decoder_layer_num=3,
             decoder_pos_emd_len=1000, decoder_dim=384, mlm=True, lora_config=dict(r=8, lora_alpha=1, requires_grad_pretrain=False),
             mlm_dict=dict(strategy="block", block_width=10, mask_rate=0.8, out_dim=768, mask_style=[0.9, 0.05, 0.05]),
             load_pretrained_model=False, passt_feature_layer=2, encoder_depth=2)
BASE_CNN = dict(n_in_channel=1, activation="cg", conv_dropout=0.5, kernel_size=[3] * 10, padding=[1] * 10, stride=[1] * 10,
                nb_filters=list(synth.PMAM_FILTERS), pooling=[list(p) for p in synth.PMAM_POOLING])
DYN = [i for i, d in enumerate(synth.FDY_DY_LAYERS) if d]
NEW_ENTRY_POINTS = ("sed_fdy_freq_mean", "sed_fdy_attn_taps", "sed_fdy_attn_softmax", "sed_fdy_mix_fwd", "sed_fdy_mix_bwd", "sed_fdy_attn_bwd",
                    "sed_fdy_mean_bwd_add")


def build(**over):
    from transformer4sed_amd.passt_cnn import PaSST_CNN
    return PaSST_CNN(passt_sed_param=dict(PASST), cnn_param=dict(FC.FDY_CNN_PARAM, **over))


@pytest.fixture(scope="module")
def net():
    return build()


def test_state_dict_names_and_shapes_are_the_reference_modules(net, golden):
    g = golden("pmam_fdy_d2")
    ref = {str(n): tuple(int(x) for x in str(s).split(",") if x) for n, s in zip(g["state_names"], g["state_shapes"])}
    own = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert own == ref
    assert list(net.state_dict().keys()) == [str(n) for n in g["state_names"]], "same order as the reference module's state_dict"
    assert net.cnn_name == "FDY-CNN"
    for i in DYN:
        pre = f"cnn.cnn.conv{i}."
        cin, co = synth.FDY_FILTERS[i - 1], synth.FDY_FILTERS[i]
        hid = FC.hid_of(cin)
        assert own[pre + "weight"] == (4, co, cin, 3, 3) and pre + "bias" not in own
        assert own[pre + "attention.conv1d1.weight"] == (hid, cin, 3) and own[pre + "attention.conv1d2.weight"] == (4, hid, 1)
        assert own[pre + "attention.conv1d2.bias"] == (4,) and own[pre + "attention.bn.num_batches_tracked"] == ()
        for k in ("weight", "bias", "running_mean", "running_var"):
            assert own[pre + "attention.bn." + k] == (hid,)
        bn = getattr(net.cnn.cnn, f"conv{i}").attention.bn
        assert bn.eps == 1e-5 and bn.momentum == 0.1
    assert own["cnn.cnn.conv0.weight"] == (16, 1, 3, 3) and own["cnn.cnn.conv0.bias"] == (16,)


def test_strict_load_round_trip(net):
    sd = synth.fdy_cnn_state_dict_np(depth=12)
    own = net.state_dict()
    assert {k: tuple(v.shape) for k, v in own.items()} == {k: tuple(np.shape(sd[k])) for k in own}
    net.load_state_dict({k: torch.from_numpy(np.asarray(sd[k])) for k in own}, strict=True)
    other = build()
    other.load_state_dict(net.state_dict(), strict=True)
    for k, v in other.state_dict().items():
        assert torch.equal(v, torch.from_numpy(np.asarray(sd[k]))), k


def test_base_branch_is_built_as_before():
    from transformer4sed_amd.passt_cnn import PaSST_CNN, _CNN
    want = synth.pmam_param_shapes(depth=2)
    for cnn in (dict(BASE_CNN), dict(BASE_CNN, cnn_name="base")):
        n = PaSST_CNN(passt_sed_param=dict(PASST), cnn_param=cnn)
        assert n.cnn_name == "base" and type(n.cnn) is _CNN and not any(n.cnn_dynamic)
        got = {k: tuple(v.shape) for k, v in n.state_dict().items()}
        assert got == {k: tuple(v) for k, v in want.items()}
        assert all(isinstance(getattr(n.cnn.cnn, f"conv{i}"), torch.nn.Conv2d) for i in range(10))
    assert "cnn_name" in dict(BASE_CNN, cnn_name="base"), "the caller's dict is not consumed"


@pytest.mark.parametrize("over, word", [
    (dict(activation="glu"), "activation"), (dict(activation="relu"), "activation"), (dict(activation="leakyrelu"), "activation"),
    (dict(normalization="layer"), "normalization"), (dict(n_basis_kernels=2), "n_basis_kernels"),
    (dict(pool_dim="time"), "pool_dim"), (dict(pool_dim="both"), "pool_dim"), (dict(pool_dim="chan"), "pool_dim"),
    (dict(DY_layers=[1, 1, 1, 1, 1, 1, 1]), r"DY_layers\[0\]"), (dict(DY_layers=[0, 1, 1]), "DY_layers"),
    (dict(DY_layers=[0, 2, 1, 1, 1, 1, 1]), "DY_layers"), (dict(temperature=0), "temperature"),
    (dict(n_in_channel=1), "n_in_channel"), (dict(kernel_size=[3] * 7), "kernel_size"), (dict(padding=[1] * 7), "padding"),
    (dict(n_input_ch=2), "n_input_ch"), (dict(kernel=[5] * 7), "3x3"), (dict(nb_filters=[16, 32, 64, 128, 128, 128, 100]), "multiples of 16"),
    (dict(cnn_name="resnet"), "resnet"), (dict(cnn_name="fdy-cnn"), "cnn_name")])
def test_refusals_name_the_offending_key(over, word):
    with pytest.raises(NotImplementedError, match=word):
        build(**over)


def test_pooling_must_reach_one_mel_bin():
    with pytest.raises(NotImplementedError, match="128 mel bins"):
        build(pooling=[[2, 2]] * 6 + [[1, 1]])


def test_dasm_refuses_every_other_cnn_name():
    from transformer4sed_amd.dasm import DASM
    at = dict(at_decoder_layer=2, query_projector=True, query_dim=1024, out_type="sigmoid", query=None)
    for cnn in (dict(FC.FDY_CNN_PARAM), dict(BASE_CNN, cnn_name="FDY-CNN"), dict(BASE_CNN, cnn_name="resnet")):
        with pytest.raises(NotImplementedError, match="cnn_name"):
            DASM(cnn_param=cnn, at_param=at, decoder="transformerXL", decoder_layer_num=1, _encoder_depth=1)


def test_restatement_reproduces_the_reference_module(golden):
    """float64 restatement of the branch on the synthetic weights against the CNN features and the attention the reference's own
    FDY_CNN produced: the restatement is what the kernel tests compare with."""
    g = golden("pmam_fdy_d2")
    mel = torch.from_numpy(synth.det_uniform("pmam_fdy_d2/mel", (2, 128, 1000), -1.2, 1.2)).double()
    sd = FC.cnn_tensors(synth.fdy_cnn_state_dict_np(depth=12), torch.float64)
    feat, rec = FC.branch(sd, mel, synth.FDY_POOLING, synth.FDY_DY_LAYERS, 31.0, train=False)
    assert tuple(feat.shape) == (2, 128, 250, 1)
    d = np.abs(feat.squeeze(-1)[:, ::16, ::10].numpy() - g["ev_cnn_s"]).max()
    assert d < 2e-6, d              # (the recorded features are fp32 results of magnitude <= 0.4)
    for j, i in enumerate(DYN):
        att = rec[i]["att"]
        assert np.abs(att[:, :, ::5].numpy() - g[f"ev_att{i}_s"]).max() < 2e-5, i
        assert abs(float(att.min()) - g["ev_att_min"][j]) < 2e-5 and abs(float(att.max()) - g["ev_att_max"][j]) < 2e-5
    # the 10-layer PMAM stack
    sd10 = FC.cnn_tensors(synth.fdy_cnn_state_dict_np(tag="fdy10", nb_filters=synth.PMAM_FILTERS, dy_layers=FC.PMAM10_DY, depth=12), torch.float64)
    f10, _ = FC.branch(sd10, mel, synth.PMAM_POOLING, FC.PMAM10_DY, 31.0, train=False)
    assert np.abs(f10.squeeze(-1)[:, ::16, ::10].numpy() - g["pm10_cnn_s"]).max() < 2e-6
    # forcing the attention to 0.25 is far from the module
    uni, _ = FC.branch(sd, mel, synth.FDY_POOLING, synth.FDY_DY_LAYERS, 31.0, train=False, uniform_attention=True)
    assert float((uni - feat).abs().max()) > 0.2 * float(feat.abs().max())


def test_fixture_guards(golden):
    """Conditions on the fixtures, not measurements: a kernel that hard-codes an attention of 0.25 must not pass a 1e-3 parity test."""
    g, gf = golden("pmam_fdy_d2"), golden("pmam_fdy_ft_d2")
    for key in (g["ev_att_min"], g["tr_att_min"], gf["att_min"], g["pm10_att_min"]):
        assert (key <= 0.10).all(), key
    for key in (g["ev_att_max"], g["tr_att_max"], gf["att_max"], g["pm10_att_max"]):
        assert (key >= 0.50).all(), key
    assert float(gf["strong_vs_uniform_attention_max"]) >= 20e-3
    sd = synth.fdy_cnn_state_dict_np(depth=12)
    for i in DYN:
        for src in (lambda st: g[f"tr_abn{i}_{st}"], lambda st: sd[f"cnn.cnn.conv{i}.attention.bn.{st}"]):
            assert (src("running_mean") != 0).all() and (src("running_var") != 1).all(), i
    names = {str(n) for n in g["tr_grad_names"]}
    for i in DYN:
        for k in ("weight", "attention.conv1d1.weight", "attention.bn.weight", "attention.bn.bias", "attention.conv1d2.weight", "attention.conv1d2.bias"):
            assert f"cnn.cnn.conv{i}.{k}" in names and f"cnn.cnn.conv{i}.{k}" in {str(n) for n in gf["tr_grad_names"]}
    assert gf["strong"].shape == gf["strong_t05_pad"].shape == gf["strong_win49"].shape == (2, 10, 1000)


def test_param_groups_freezing_and_grad_names():
    from transformer4sed_amd.pmam_trainer import get_param_lr, mark_only_lora_as_trainable
    lr = dict(cnn=dict(lr=1.5e-4, weight_decay=1e-4), passt=dict(lr=5e-5, weight_decay=1, freeze_layer=1, step_lr=0),
              decoder=dict(lr=1.5e-4, weight_decay=1e-4), head=dict(lr=2e-4))
    n = build()
    mark_only_lora_as_trainable(n.backbone)
    groups = get_param_lr(n, lr)
    att = {k for k, _ in n.named_parameters() if ".attention." in k}
    assert len(att) == 5 * len(DYN)
    cnn_group = [gr for gr in groups if any(k == "cnn.cnn.conv0.weight" for k, _ in gr["params"])]
    assert len(cnn_group) == 1 and att <= {k for k, _ in cnn_group[0]["params"]}
    assert sum(k in att for gr in groups for k, _ in gr["params"]) == len(att), "in no other group"
    assert att <= n._grad_names() and "cnn.cnn.conv1.weight" in n._grad_names() and "cnn.cnn.conv1.bias" not in n._grad_names()
    frozen = build()
    get_param_lr(frozen, dict(lr, cnn=dict(lr=0.0, weight_decay=1e-4)))
    assert not any(p.requires_grad for k, p in frozen.named_parameters() if k.startswith("cnn."))
    assert not any(k.startswith("cnn.") for k in frozen._grad_names())


def test_buffer_synchronisation_covers_the_attention_batchnorms(monkeypatch):
    from transformer4sed_amd import ddp
    n = build()
    sent = []
    monkeypatch.setattr(ddp.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(ddp.dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(ddp.dist, "get_backend", lambda group=None: "gloo")
    monkeypatch.setattr(ddp.dist, "broadcast", lambda t, src=0, group=None: sent.append(t.clone()))
    bn = n.cnn.cnn.conv3.attention.bn
    with torch.no_grad():
        bn.running_mean.fill_(0.25)
    assert ddp.broadcast_buffers(n) == 3 * (len(synth.FDY_FILTERS) + len(DYN))
    hid = [FC.hid_of(synth.FDY_FILTERS[i - 1]) for i in DYN]
    assert sent[0].numel() == sum(2 * c + 1 for c in synth.FDY_FILTERS) + sum(2 * h + 1 for h in hid)
    assert int((sent[0] == 0.25).sum()) == bn.running_mean.numel()


def test_synth_functions_keep_their_bytes():
    """The FDY state is built on top of `pmam_state_dict_np`; what existed keeps its values."""
    def digest(sd, keys):
        h = hashlib.sha256()
        for k in keys:
            h.update(k.encode())
            h.update(np.ascontiguousarray(sd[k]).tobytes())
        return h.hexdigest()
    pm = synth.pmam_state_dict_np(depth=2)
    keys = sorted(k for k in pm if k.startswith(("cnn.", "cnn_projector", "merge_weight", "backbone.blocks.1.attn.qkv", "decoder.encoder_blocks.0")))
    assert digest(pm, keys) == PMAM_DIGEST
    fd = synth.fdy_cnn_state_dict_np(tag="pmam0", depth=2, nb_filters=synth.PMAM_FILTERS, dy_layers=[0] * 10)
    assert list(fd) == list(pm) and all(np.array_equal(fd[k], pm[k]) for k in pm), "no dynamic layer: the PMAM state itself"
    fdy = synth.fdy_cnn_state_dict_np(depth=2)
    shared = [k for k in fdy if not k.startswith("cnn.")]
    ref = synth.pmam_state_dict_np(tag="fdy0", depth=2, nb_filters=synth.FDY_FILTERS)
    assert all(np.array_equal(fdy[k], ref[k]) for k in shared)
    assert synth.PMAM_FILTERS == (16, 16, 32, 32, 64, 64, 128, 128, 256, 384)
    w = fdy["cnn.cnn.conv2.weight"]
    assert not np.array_equal(w[0], w[1]), "four different basis kernels"


PMAM_DIGEST = "09ff4e3fb7eca68ecba910c4103904f8ef5691be828a2d6eb0152d97de691450"


def test_abi_additions_only():
    from transformer4sed_amd import _lib, build as B
    protos = _lib.parse_header()
    dll = ctypes.CDLL(B.build(verbose=False))
    for name in NEW_ENTRY_POINTS:
        assert name in protos and hasattr(dll, name), name
        assert protos[name][-1] == (ctypes.c_void_p, "stream")
    assert "fdy_cnn.hip" in B.SOURCES
    src = open(_lib.HEADER_PATH).read()
    assert "#define SED_HIP_ABI_VERSION 7" in " ".join(src.split())
    assert "FDY_cnn.py" in src
