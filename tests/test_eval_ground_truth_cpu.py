"""The ground-truth builder of the evaluation package on a hand-written table, the state `IntersectionPSDS` and `EventSegmentF1` take
from it, and the public names of `transformer4sed_amd.evaluation`.  No GPU needed."""
import importlib
import sys

import numpy as np
import pandas as pd
import pytest

from transformer4sed_amd import evaluation as EV
from transformer4sed_amd.evaluation import ground_truth as GT

CLASSES = ["Cat", "Dog"]
ROWS = [("a", "Dog", 1.0, 2.0), ("b", np.nan, np.nan, np.nan), ("a", "Cat", 0.5, 0.75), ("a", "Dog", 0.1, 0.3), ("c", "Cat", 3.0, 4.5)]
EVENTS = {"a": [[0, 500000, 750000], [1, 100000, 300000], [1, 1000000, 2000000]], "c": [[0, 3000000, 4500000]]}

# every top-level name of the single-file evaluation.py this package replaced
NAMES = ["Encoder", "create_score_dataframe", "write_sed_scores", "read_sed_scores", "_scores_device", "_scores_tables",
         "batched_decode_preds", "_events_device", "_events_frames", "decode_pred_batch_fast", "WeakF1Macro", "AP_CHUNK",
         "MultilabelAveragePrecision", "PSDS_MAX_FRAMES", "PSDS_MAX_CLIP_EVENTS", "PSDS_MAX_CT_CLASSES", "PSDS_PADDED_CLASSES",
         "PSDS_BLOCK_CLIPS", "_PSDS_UNITS", "_microseconds", "_table", "IntersectionPSDS", "compute_psds_from_scores", "F1_MAX_FRAMES",
         "F1_MAX_CLIP_EVENTS", "F1_MAX_ESTIMATES", "F1_MAX_SEGMENTS", "F1_COUNTS", "EventSegmentF1", "log_sedeval_metrics",
         "ScoreBufferTuple", "_HostStage", "Evaluator", "mean_psds_per_type", "remove_extra_events", "AudiosetStrongEvaluator"]


def table(rows=ROWS):
    return pd.DataFrame([dict(filename=f"audio/{f}.wav", event_label=l, onset=on, offset=off) for f, l, on, off in rows])


def test_fixed_clip_order():
    g = GT.build_ground_truth(table(), CLASSES, ["c", "a", "b"])
    assert g.clip_ids == ["c", "a", "b"] and g.clip_index == {"c": 0, "a": 1, "b": 2}
    assert g.gt_ptr.dtype == np.int32 and g.gt_ptr.tolist() == [0, 1, 4, 4]
    assert g.gt.dtype == np.int64 and g.gt.tolist() == EVENTS["c"] + EVENTS["a"]
    assert g.gt_clips == {"a", "b", "c"}                           # b: a ground-truth clip without events


def test_clips_by_first_appearance():
    g = GT.build_ground_truth(table(), CLASSES)
    assert g.clip_ids == ["a", "b", "c"] and g.clip_index == {"a": 0, "b": 1, "c": 2}
    assert g.gt_ptr.dtype == np.int32 and g.gt_ptr.tolist() == [0, 3, 3, 4]
    assert g.gt.dtype == np.int64 and g.gt.tolist() == EVENTS["a"] + EVENTS["c"]
    assert g.gt_clips == {"a", "b", "c"}


def test_a_table_without_events():
    g = GT.build_ground_truth(table(ROWS[1:2]), CLASSES, nan_to_num=True)
    assert g.clip_ids == ["b"] and g.gt_ptr.tolist() == [0, 0] and g.gt.shape == (0, 3) and g.gt_clips == {"b"}


def test_refusals():
    with pytest.raises(ValueError, match="ground-truth label 'Bird' is not one of event_classes"):
        GT.build_ground_truth(table(ROWS + [("c", "Bird", 1.0, 2.0)]), CLASSES)
    for off in (1.0, 0.5):
        with pytest.raises(ValueError, match="ground-truth event of 'c' with offset <= onset"):
            GT.build_ground_truth(table(ROWS + [("c", "Dog", 1.0, off)]), CLASSES)
    with pytest.raises(ValueError, match="ground-truth clip 'b' is missing from audio_durations"):
        GT.build_ground_truth(table(), CLASSES, ["c", "a"])
    GT.build_ground_truth(table(ROWS[1:]), CLASSES, max_clip_events=2, owner="Metric")                     # two events of a: allowed
    with pytest.raises(NotImplementedError, match=r"Metric: clip 'a' has 3 events \(at most 2\)"):
        GT.build_ground_truth(table(), CLASSES, max_clip_events=2, owner="Metric")
    early = table(ROWS + [("c", "Dog", -0.5, 1.0)])
    assert GT.build_ground_truth(early, CLASSES).gt.tolist()[-1] == [1, -500000, 1000000]
    with pytest.raises(ValueError, match="ground-truth event of 'c' with a negative onset"):
        GT.build_ground_truth(early, CLASSES, refuse_negative_onset=True)


def test_accumulators_expose_the_builders_arrays():
    ts = np.arange(11) * 0.5
    dur = pd.DataFrame(dict(filename=["x/c.wav", "x/a.wav", "x/b.wav"], duration=[5.0, 5.0, 5.0]))
    psds = EV.IntersectionPSDS(table(), dur, CLASSES, ts, 0.5, 0.5)
    f1 = EV.EventSegmentF1(table(), CLASSES, ts)
    for acc, order in ((psds, ["c", "a", "b"]), (f1, None)):
        g = GT.build_ground_truth(table(), CLASSES, order, nan_to_num=order is None)
        assert acc.clip_ids == g.clip_ids and acc._clip_index == g.clip_index
        assert acc.gt_ptr.dtype == np.int32 and np.array_equal(acc.gt_ptr, g.gt_ptr)
        assert acc.gt.dtype == np.int64 and np.array_equal(acc.gt, g.gt)
        assert acc._seen == set() and acc._status is None


def test_public_names_resolve_without_the_library(monkeypatch):
    """A fresh import of the package and every name of the old module, with the library loader replaced by one that fails."""
    import transformer4sed_amd as pkg
    from transformer4sed_amd import _lib, ops

    def refuse():
        raise AssertionError("the evaluation package loaded the HIP library at import")

    monkeypatch.setattr(_lib, "lib", refuse)
    monkeypatch.setattr(ops, "lib", refuse)
    monkeypatch.setattr(pkg, "evaluation", EV)                       # (the import below rebinds it; put back afterwards)
    for name in [m for m in sys.modules if m == EV.__name__ or m.startswith(EV.__name__ + ".")]:
        monkeypatch.delitem(sys.modules, name)
    fresh = importlib.import_module(EV.__name__)
    assert fresh is not EV
    missing = [n for n in NAMES if not hasattr(fresh, n)]
    assert not missing, missing
    for n in NAMES:
        assert getattr(EV, n) is not None
    assert pkg.IntersectionPSDS is fresh.IntersectionPSDS and pkg.EventSegmentF1 is fresh.EventSegmentF1      # the lazy names
