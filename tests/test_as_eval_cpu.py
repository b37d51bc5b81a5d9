"""Open-vocabulary helpers (dasm_trainer: get_att_mask, get_common_first_query, reorder_pred, common_type_mask) against a direct
restatement of recipes/audioset_strong/detect_any_sound/passt/open_vocabulary.py:98-145, and the pure-Python parts of the AudioSet-Strong
evaluation (evaluation.mean_psds_per_type, remove_extra_events, MultilabelAveragePrecision's argument checks).  No GPU needed."""
import os
import sys

import numpy as np
import pandas as pd
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from transformer4sed_amd import dasm_trainer as DT  # noqa: E402
from transformer4sed_amd import evaluation as E  # noqa: E402


# ---- restatement of open_vocabulary.py:98-145 (num_gpu = the reference's torch.cuda.device_count())
def r_att_mask(mask, num_gpu):
    common = torch.count_nonzero(mask)
    rare = len(mask) - common
    att = torch.ones(common + rare, common + rare, dtype=torch.bool)
    att[:, :common] = False
    att.fill_diagonal_(False)
    if num_gpu > 1:
        att = att.unsqueeze(0).expand(num_gpu, -1, -1)
    return att


def r_common_first(q, mask, num_gpu):
    q = torch.cat([q[mask, :], q[torch.logical_not(mask), :]])
    if num_gpu > 1:
        q = q.unsqueeze(0).expand(num_gpu, -1, -1)
    return q


def r_reorder(pred, mask):
    common = torch.count_nonzero(mask)
    ret = torch.zeros_like(pred)
    ret[:, mask, ...] = pred[:, :common, ...]
    ret[:, torch.logical_not(mask), ...] = pred[:, common:, ...]
    return ret


MASKS = [np.array([1, 0, 1, 1, 0, 1, 0, 1], bool), np.ones(8, bool), np.zeros(8, bool),
         np.random.RandomState(0).rand(407) < 0.6]


@pytest.mark.parametrize("mi", range(len(MASKS)))
@pytest.mark.parametrize("num_gpu", [1, 2])
def test_open_vocabulary_helpers_vs_restatement(mi, num_gpu):
    mask = torch.from_numpy(MASKS[mi])
    C = mask.numel()
    q = torch.randn(C, 16, generator=torch.Generator().manual_seed(mi))
    assert torch.equal(DT.get_att_mask(mask, num_gpu), r_att_mask(mask, num_gpu))
    got = DT.get_common_first_query(q, mask, num_gpu)
    assert torch.equal(got, r_common_first(q, mask, num_gpu)) and not got.requires_grad
    two = DT.get_common_first_query(torch.nn.ParameterList([torch.nn.Parameter(q), torch.nn.Parameter(q * 2)]), mask, num_gpu)
    assert torch.equal(two[1], r_common_first(q * 2, mask, num_gpu))
    for shape in ((3, C, 50), (3, C)):
        pred = torch.randn(*shape, generator=torch.Generator().manual_seed(7))
        assert torch.equal(DT.reorder_pred(pred, mask), r_reorder(pred, mask))
        # reorder_pred inverts the common-first permutation
        first = torch.cat([pred[:, mask, ...], pred[:, ~mask, ...]], 1)
        assert torch.equal(DT.reorder_pred(first, mask), pred)


def test_common_type_mask_and_type_dict(tmp_path):
    labels = ["a", "b", "c", "d"]
    td = {"a": "common", "b": "rare", "c": "common", "d": "rare"}
    p = tmp_path / "state.json"
    p.write_text('{"a": "common", "b": "rare", "c": "common", "d": "rare"}')
    assert DT.load_type_dict(str(p)) == td and DT.load_type_dict(td) == td
    assert DT.common_type_mask(labels, td).tolist() == [True, False, True, False]


def test_mean_psds_per_type_and_remove_extra_events():
    td = {"a": "common", "b": "rare", "c": "common"}
    assert E.mean_psds_per_type({"a": 0.5, "b": 0.25, "c": 0.25}, td) == {"common": 0.375, "rare": 0.25}
    buf = {"x": pd.DataFrame([[0.0, 0.1, 1, 2, 3]], columns=["onset", "offset", "a", "b", "c"])}
    out = E.remove_extra_events(buf, {"b"})
    assert out is buf and list(buf["x"].columns) == ["onset", "offset", "a", "c"]


def test_average_precision_arguments():
    with pytest.raises(NotImplementedError):
        E.MultilabelAveragePrecision(10, average="micro")
    with pytest.raises(ValueError):
        E.MultilabelAveragePrecision(10, average="samples")
    m = E.MultilabelAveragePrecision(10, average="macro", compute_on_step=False)
    assert m.to("cuda") is m
    with pytest.raises(RuntimeError):
        m.compute()                  # no update
    with pytest.raises(ValueError):
        m.update(torch.rand(2, 9), torch.ones(2, 9))
