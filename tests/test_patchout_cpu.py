"""Structured frequency patchout, `PaSST_SED(s_patchout_f=s)`, without a GPU: constructor and refusals, the train-mode draws of one
forward against the reference's recorded ones (tests/golden/model_d768_l2_patchout4.npz, tools/gen_patchout_golden.py), the ABI
additions and the fixtures' guards."""
import ctypes
import os

import numpy as np
import pytest
import torch

from transformer4sed_amd import synth
from transformer4sed_amd.engine import window_starts
from transformer4sed_amd.passt_sed import PaSST_SED

TAG, STEP_TAG = "model_d768_l2_patchout4", "trainstep_patchout"
NEW_ENTRY_POINTS = ("sed_im2col_rows", "sed_assemble_tokens_rows", "sed_assemble_tokens_rows_bwd", "sed_fpool_rows_fwd", "sed_fpool_rows_bwd")
GOLDEN_DIR = os.path.join(os.path.dirname(__file__), "golden")


def build(s=4, decoder="transformerXL", **kw):
    layers = 3 if decoder == "transformerXL" else 2        # (the fixture's model: oracle/make_golden.py build_reference_model)
    return PaSST_SED(decoder=decoder, decoder_layer_num=layers, at_adapter=True, load_pretrained_model=False, passt_feature_layer=2,
                     f_pool="mean_pool", encoder_depth=2, s_patchout_f=s, **kw)


def pmam_params():
    passt = dict(class_num=30, f_pool="attention", decode_ratio=10, at_adapter=True, decoder="transformerXL", decoder_layer_num=1,
                 decoder_pos_emd_len=1000, decoder_dim=384, mlm=False, load_pretrained_model=False, passt_feature_layer=1, encoder_depth=1)
    cnn = dict(n_in_channel=1, activation="cg", conv_dropout=0, kernel_size=[3] * 10, padding=[1] * 10, stride=[1] * 10,
               nb_filters=list(synth.PMAM_FILTERS), pooling=[list(p) for p in synth.PMAM_POOLING])
    return passt, cnn


def reference_offsets(T, win, step):
    """passt.py:504-509 restated: one `randint(1 + 99 - tp)` per window pass whose tp patches are fewer than the 99 of the table."""
    offs = []
    for left in window_starts(T, win, step):
        tp = (min(left + win, T) - left - 16) // 10 + 1
        offs.append(int(torch.randint(1 + 99 - tp, (1,)).item()) if tp < 99 else 0)
    return offs


# ------------------------------------------------------------------------------------------------ constructor
def test_constructs_with_both_decoders_and_owns_no_tensor(golden):
    g = golden(TAG)
    want = {str(n): tuple(int(d) for d in str(s).split(",") if d) for n, s in zip(g["state_names"], g["state_shapes"])}
    net = build(4)
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert got == want, set(got) ^ set(want)
    assert got == {k: tuple(v.shape) for k, v in build(0).state_dict().items()}
    assert net.backbone.s_patchout_f == 4 and build(0).backbone.s_patchout_f == 0
    conf = build(4, decoder="conformer")
    assert conf.backbone.s_patchout_f == 4
    assert set(conf.state_dict()) == set(build(0, decoder="conformer").state_dict())
    from copy import deepcopy
    assert deepcopy(net).backbone.s_patchout_f == 4          # the EMA teacher is a deepcopy of the student


@pytest.mark.parametrize("s,exc", [(-1, ValueError), (12, ValueError), (13, ValueError), (2.5, TypeError), (True, TypeError)])
def test_bad_row_counts_are_refused(s, exc):
    with pytest.raises(exc, match="s_patchout_f"):
        build(s)
    net = build(4)
    net.backbone.s_patchout_f = s         # ... and again at forward time: the attribute is writable, as in the reference
    with pytest.raises(exc, match="s_patchout_f"):
        net._train_draws(1000)


def test_time_patchout_stays_refused():
    with pytest.raises(NotImplementedError, match="s_patchout_t"):
        PaSST_SED(decoder="transformerXL", load_pretrained_model=False, s_patchout_t=1)
    with pytest.raises(NotImplementedError, match="s_patchout_t"):
        PaSST_SED(decoder="transformerXL", load_pretrained_model=False, s_patchout_f=4, s_patchout_t=1)


def test_pmam_and_dasm_keep_refusing_patchout():
    from transformer4sed_amd.dasm import DASM
    from transformer4sed_amd.passt_cnn import PaSST_CNN
    passt, cnn = pmam_params()
    for kw in (dict(s_patchout_f=4), dict(s_patchout_t=1)):
        with pytest.raises(NotImplementedError, match="unsupported: patchout"):
            PaSST_CNN(passt_sed_param=dict(passt, **kw), cnn_param=cnn)
    # DASM's constructor has no such argument (nor has the reference's); the knob on its backbone is refused when a forward reads it
    for net in (PaSST_CNN(passt_sed_param=passt, cnn_param=cnn),
                DASM(cnn_param=cnn, decoder="transformerXL", _encoder_depth=1,
                     at_param=dict(at_decoder_layer=2, query_projector=True, query_dim=1024, out_type="sigmoid"))):
        net.train()
        net.backbone.s_patchout_f = 4
        with pytest.raises(NotImplementedError, match="unsupported: patchout"):
            net._train_draws(1000)


# ------------------------------------------------------------------------------------------------ draws
def test_draws_are_the_references(golden):
    g = golden(TAG)
    net = build(4).train()
    torch.manual_seed(int(g["seed"]))
    offs, rows = net._train_draws(1000, False)
    assert offs is None and rows == [g["rows_global"].tolist()]
    torch.manual_seed(int(g["seed"]))
    offs, rows = net._train_draws(1000, True, [512, 49])
    assert offs == g["win_toffsets"].tolist()
    assert rows == [g["rows_global"].tolist()] + g["win_rows"].tolist()
    # the call order itself: nothing else is drawn, so the generator ends where a plain restatement of the order ends
    end = torch.get_rng_state()
    torch.manual_seed(int(g["seed"]))
    torch.randperm(12)
    for left in window_starts(1000, 512, 49):
        torch.randint(1 + 99 - 50, (1,))
        torch.randperm(12)
    assert torch.equal(end, torch.get_rng_state())
    torch.manual_seed(int(g["mlm_seed"]))
    assert net._train_draws(1000, False)[1] == [g["mlm_rows"].tolist()]


@pytest.mark.parametrize("win_param", [(512, 49), (512, 31), (1000, 49)])
def test_without_patchout_the_randint_stream_is_todays(win_param):
    passt, cnn = pmam_params()
    from transformer4sed_amd.passt_cnn import PaSST_CNN
    for net in (build(0), PaSST_CNN(passt_sed_param=passt, cnn_param=cnn)):
        net.train()
        torch.manual_seed(11)
        want = reference_offsets(1000, *win_param)
        end = torch.get_rng_state()
        torch.manual_seed(11)
        offs, rows = net._train_draws(1000, True, win_param)
        assert offs == want and rows is None and torch.equal(end, torch.get_rng_state())
        torch.manual_seed(11)
        start = torch.get_rng_state()
        assert net._train_draws(1000, False) == (None, None) and torch.equal(start, torch.get_rng_state())


def test_eval_mode_draws_nothing():
    net = build(4).eval()
    torch.manual_seed(5)
    start = torch.get_rng_state()
    assert net._train_draws(1000, False) == (None, None)
    assert net._train_draws(1000, True, [512, 49]) == (None, None)
    assert torch.equal(start, torch.get_rng_state())


def test_predraw_keeps_the_students_draws_first(golden):
    """The trainer issues the teacher's forward before the student's; `predraw` makes the student's draws at the reference's place."""
    g = golden(TAG)
    stu, tch = build(4).train(), build(4).train()
    torch.manual_seed(int(g["seed"]))
    want_stu = stu._train_draws(1000, False)
    want_tch = tch._train_draws(1000, True, [512, 49])
    torch.manual_seed(int(g["seed"]))
    stu.predraw(1000, False)
    assert tch._train_draws(1000, True, [512, 49]) == want_tch and stu._pending_draws == want_stu
    assert want_stu[1] == [g["rows_global"].tolist()] and want_tch[1][0] != want_stu[1][0]


def test_injected_rows_are_validated(golden):
    g = golden(TAG)
    net = build(4).train()
    good = [g["rows_global"].tolist()] + g["win_rows"].tolist()
    net._patchout_rows, net._win_toffsets = good, g["win_toffsets"].tolist()
    torch.manual_seed(5)
    start = torch.get_rng_state()
    assert net._train_draws(1000, True, [512, 49]) == (g["win_toffsets"].tolist(), good)
    assert torch.equal(start, torch.get_rng_state())          # injected values replace the draws
    net._patchout_rows = good[:1]
    assert net._train_draws(1000, False)[1] == good[:1]
    with pytest.raises(ValueError, match="_patchout_rows"):       # one set for 1 + 11 backbone calls
        net._train_draws(1000, True, [512, 49])
    for bad in ([0, 1, 2, 3, 4, 5, 6], [0, 1, 2, 3, 4, 5, 6, 7, 8], [3, 0, 4, 5, 6, 7, 9, 11], [0, 0, 4, 5, 6, 7, 9, 11],
                [0, 3, 4, 5, 6, 7, 9, 12], [-1, 3, 4, 5, 6, 7, 9, 11]):
        net._patchout_rows = [bad]
        with pytest.raises(ValueError, match="_patchout_rows"):
            net._train_draws(1000, False)
    net._patchout_rows = [[0.0, 3, 4, 5, 6, 7, 9, 11]]
    with pytest.raises(TypeError, match="_patchout_rows"):
        net._train_draws(1000, False)


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_additions_only():
    from transformer4sed_amd import _lib, build as B
    protos = _lib.parse_header()
    dll = ctypes.CDLL(B.build(verbose=False))
    for name in NEW_ENTRY_POINTS:
        assert name in protos and hasattr(dll, name), name
        assert protos[name][-1] == (ctypes.c_void_p, "stream")
    args = lambda n: [a for _, a in protos[n]]
    assert args("sed_im2col_rows")[2:4] == ["rows", "F"] and args("sed_fpool_rows_fwd")[-2] == "F" and args("sed_fpool_rows_bwd")[-2] == "F"
    # the old entry points keep their signatures
    assert args("sed_im2col") == ["mel", "cols", "B", "T", "tstart", "tp", "f16", "stream"]
    assert args("sed_assemble_tokens_bwd") == ["dx", "dconv", "dcls", "ddist", "dnew_pos", "dfreq", "dtime", "toffset", "B", "tp", "stream"]
    assert args("sed_fpool_fwd")[-3:] == ["B", "tp", "stream"] and args("sed_fpool_bwd")[-3:] == ["B", "tp", "stream"]
    src = open(_lib.HEADER_PATH).read()
    assert "#define SED_HIP_ABI_VERSION 7" in " ".join(src.split())


# ------------------------------------------------------------------------------------------------ fixtures
def test_fixture_guards(golden):
    """A 1e-3 parity test must not be passable by code that ignores the kept rows or takes the wrong ones."""
    g = golden(TAG)
    assert float(g["strong_vs_full_max"]) >= 20e-3 and float(g["strong_vs_first_rows_max"]) >= 20e-3
    rows = g["rows_global"].tolist()
    assert len(rows) == 8 and rows != list(range(8)) and rows == sorted(set(rows)) and 0 <= rows[0] and rows[-1] < 12
    wr = g["win_rows"].tolist()
    assert len(wr) == len(window_starts(1000, 512, 49)) == len(g["win_toffsets"]) and any(r != wr[0] for r in wr)
    assert g["win_draw_kinds"].tolist() == ["randperm"] + ["randint", "randperm"] * len(wr)
    dropped = [r for r in range(12) if r not in rows]
    assert g["ft_dfreq"].shape == (768, 12) and not g["ft_dfreq"][:, dropped].any() and g["ft_dfreq"][:, rows].any(axis=0).all()
    assert "backbone.freq_new_pos_embed" in {str(n) for n in g["ft_grad_names"]}
    assert g["strong"].shape == (2, 10, 1000) and g["win_strong"].shape == (2, 10, 1000)
    s = golden(STEP_TAG)
    assert int(s["n_steps"]) == 2 and int(s["s_patchout_f"]) == 4
    # a step ends with the student's global pass, then the windowed teacher (1 + 11 backbone calls): 13 row draws (the augmentation's
    # own two randperm come earlier)
    for step in range(2):
        kinds = s[f"s{step}_draw_kinds"].tolist()
        assert kinds[-24:] == ["randperm", "randperm"] + ["randint", "randperm"] * 11 and kinds.count("randperm") == 15
    for tag in (TAG, STEP_TAG):
        assert os.path.getsize(os.path.join(GOLDEN_DIR, tag + ".npz")) < 589 * 1024
