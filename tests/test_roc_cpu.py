"""ROC area without a device: the two host references of tests/roc_cases.py against each other, against
scikit-learn and against the product's float64 finish; the case set; the host pooling reference against the golden recorded from the
reference's get_segment_scores / get_segment_scores_and_overlap_add; every refusal; the constants of include/sed_hip.h."""
import os
import re
import sys

import numpy as np
import pandas as pd
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import roc_cases as RC  # noqa: E402
from transformer4sed_amd.evaluation import roc  # noqa: E402

CASES = RC.cpu_cases()
SK_TOL = 1e-9           # scikit-learn sums at most N <= 1e5 float64 trapezoids of magnitude <= 1: error <= N 4 2^-53 ~ 5e-11, with slack
POOL_TOL = 2.0 ** -24 * 1.01


@pytest.fixture(scope="module")
def refs():
    return [(c, RC.reference(c, RC.ref_points), RC.reference(c, RC.ref_items)) for c in CASES]


def test_two_references_agree_exactly(refs):
    for c, a, b in refs:
        assert np.array_equal(a, b), (c["name"], a, b)


def test_references_match_sklearn_and_the_products_finish(refs):
    sk = pytest.importorskip("sklearn.metrics")
    checked = 0
    for c, ints, _ in refs:
        f = c["max_fpr"]
        auroc, pauc = roc.roc_scores(ints, f, "mcclish")
        _, ratio = roc.roc_scores(ints, f, "max_fpr")
        for k in range(ints.shape[0]):
            want_auroc, want_pauc = RC.finish_fraction(ints[k], f, "mcclish")
            if want_auroc is None:
                assert k in c["nan_classes"], (c["name"], k)              # only the designated classes may be NaN
                assert np.isnan(auroc[k]) and np.isnan(pauc[k]) and np.isnan(ratio[k])
                continue
            assert k not in c["nan_classes"], (c["name"], k)
            y, s = c["labels"][k], c["scores"][k].astype(np.float64)
            full, part = sk.roc_auc_score(y, s), sk.roc_auc_score(y, s, max_fpr=f)
            assert abs(float(want_auroc) - full) <= SK_TOL and abs(float(want_pauc) - part) <= SK_TOL, (c["name"], k)
            assert abs(auroc[k] - full) <= SK_TOL and abs(pauc[k] - part) <= SK_TOL, (c["name"], k)
            assert abs(ratio[k] - float(RC.finish_fraction(ints[k], f, "max_fpr")[1])) <= SK_TOL
            checked += 1
    assert checked >= 50


def test_case_set_holds_every_designated_property(refs):
    seen = set()
    for c, ints, _ in refs:
        for k in range(ints.shape[0]):
            P, Nn, auc2, area2, fp_a, tp_a, fp_b, tp_b = (int(v) for v in ints[k])
            s, y = c["scores"][k], c["labels"][k]
            x = float(np.float64(c["max_fpr"]) * np.float64(Nn))
            if P and Nn and RC.auc2_strict(s, y) != auc2:
                seen.add("ties change auc2")
            if P and Nn and fp_a < x < fp_b and fp_b - fp_a >= 2:
                seen.add("cut inside a tie group")
            if P and Nn and c["max_fpr"] < 1.0 and fp_a > 0 and x == fp_a:
                seen.add("cut on a point")
            if c["max_fpr"] == 1.0 and P and Nn:
                assert area2 == auc2 and fp_a == Nn and tp_a == P
                seen.add("max_fpr 1")
            if P == 1 and Nn > 1:
                seen.add("one positive")
            if P == 0 and Nn > 1:
                seen.add("no positive")
            if Nn == 0 and P > 1:
                seen.add("no negative")
            zeros = s[s == 0]
            if P and Nn and np.signbit(zeros).any() and not np.signbit(zeros).all():
                seen.add("signed zeros")
                assert np.array_equal(ints[k], RC.ref_points(np.where(s == 0, np.float32(0.0), s), y, c["max_fpr"]))        # -0.0 and +0.0 are one value
            if P and Nn and s.size > 2 and (RC.score_key(s) == RC.score_key(s)[0]).all():
                assert auc2 == P * Nn
                seen.add("all tied")
    assert seen == {"ties change auc2", "cut inside a tie group", "cut on a point", "max_fpr 1", "one positive", "no positive",
                    "no negative", "signed zeros", "all tied"}, seen


def test_macro_mean_leaves_nan_classes_out_with_a_warning():
    c = next(c for c in CASES if c["name"].startswith("one positive"))
    ints = RC.reference(c)
    auroc, _ = roc.roc_scores(ints)
    with pytest.warns(UserWarning, match="Ignoring these classes in macro"):
        got = roc._mean(auroc, ints[:, 0], "AUROC score", "macro")
    assert got == auroc[0] and np.isnan(auroc[1:]).all()
    d = float(roc.d_prime(0.75))
    from statistics import NormalDist
    assert abs(d - 2 ** 0.5 * NormalDist().inv_cdf(0.75)) <= 1e-12


# ---------------------------------------------------------------------------------------------------- segments
def test_host_pooling_matches_the_reference_golden(golden):
    g = golden("segment_scores")
    for name in RC.GEOMETRIES:
        ts_us, clip_us = RC.geometry(name)
        assert np.array_equal(ts_us, RC.microseconds(g[name + "/ts"])) and clip_us == int(RC.microseconds(g[name + "/clip"]))
        got = RC.pool_ref(g[name + "/scores"], ts_us, clip_us, 1000000)
        assert got.shape == g[name + "/out"].shape == (10, 3)
        assert np.abs(got.astype(np.float64) - g[name + "/out"]).max() <= POOL_TOL, name
        assert np.array_equal(g[name + "/out_ts"], np.r_[np.arange(10.0), g[name + "/clip"]])
        assert np.array_equal(roc.segment_weights(ts_us, clip_us, 1000000).sum(1) > 0, np.ones(10, dtype=bool))
    ts_us = RC.microseconds(g["ola/ts"])
    onsets = RC.microseconds(g["ola/onsets"]).tolist()
    clips = [(on, RC.pool_ref(s, ts_us, 10000000, 1000000)) for on, s in zip(onsets, g["ola/scores"])]
    got = RC.overlap_add_ref(clips, 24, 1000000)
    assert np.abs(got.astype(np.float64) - g["ola/out"]).max() <= POOL_TOL
    assert (got[23] == 0).all() and (g["ola/out"][23] == 0).all()            # no clip reaches the last segment: it scores 0
    assert np.array_equal(g["ola/out_ts"], np.minimum(np.arange(25.0), 23.4))


def test_segment_targets_rule():
    # one file of 3.5 s, Ls = 1 s: 4 segments, the last one [3, 3.5)
    gt = np.array([[0, 500000, 1000000], [0, 2999999, 3000001], [1, 3400000, 9000000], [2, 1000000, 2000000]], dtype=np.int64)
    target, ptr = roc.segment_targets(gt, np.array([0, 4]), [3500000], 1000000, 4)
    assert ptr.tolist() == [0, 4]
    assert target.tolist() == [[1, 0, 1, 1], [0, 0, 0, 1], [0, 1, 0, 0], [0, 0, 0, 0]]
    # brute force over random events, two files
    rng = np.random.RandomState(0)
    dur = [2300000, 5000000]
    ev = [[(int(rng.randint(3)), on, on + int(rng.randint(1, 2500000))) for on in rng.randint(0, d, size=6).tolist()] for d in dur]
    flat = np.array(sorted(ev[0]) + sorted(ev[1]), dtype=np.int64)
    target, ptr = roc.segment_targets(flat, np.array([0, 6, 12]), dur, 700000, 3)
    for i, d in enumerate(dur):
        for k in range(int(ptr[i + 1] - ptr[i])):
            for c in range(3):
                want = any(e[0] == c and e[1] < min((k + 1) * 700000, d) and e[2] > k * 700000 for e in ev[i])
                assert target[c, ptr[i] + k] == want


def test_merge_functions():
    ev = {"f": [(0.0, 1.0, "a"), (1.0, 2.0, "a"), (2.5, 3.0, "a"), (0.5, 0.7, "b"), (0.1, 4.0, "a")], "g": []}
    out = roc.merge_overlapping_events(ev)
    assert out == {"f": [[0.0, 4.0, "a"], [0.5, 0.7, "b"]], "g": []}
    clips = {"x-y-0-1000": [(1.0, 2.0, "a")], "x-y-150-1150": [(0.5, 3.0, "a"), (9.0, 9.5, "b")], "z-200-1200": [(0.0, 1.0, "a")]}
    out = roc.merge_maestro_ground_truth(clips)
    assert out == {"x-y": [[1.0, 4.0, "a"], [10.0, 10.5, "b"]], "z": [[2.0, 3.0, "a"]]}          # 150 // 100 = 1 whole second


def _acc(**kw):
    gt = pd.DataFrame({"filename": ["f.wav", "f.wav", "g.wav"], "onset": [0.5, 3.0, 1.0], "offset": [1.5, 9.0, 2.0],
                       "event_label": ["a", "b", "a"]})
    args = dict(ground_truth=gt, audio_durations={"f": 23.4, "g": 10.0}, event_classes=["a", "b"], timestamps=np.arange(157) * 0.064)
    args.update(kw)
    return roc.SegmentAUROC(**args)


def test_refusals():
    for bad in (dict(max_fpr=0.0), dict(max_fpr=1.5), dict(normalize="area"), dict(clip_ids="window"), dict(segment_length=0.0),
                dict(timestamps=[0.0, 0.2, 0.1]), dict(audio_durations={"f": 23.4, "g": 0.0}),
                dict(audio_durations=pd.DataFrame({"filename": ["f.wav", "f.flac", "g.wav"], "duration": [1.0, 1.0, 1.0]}))):
        with pytest.raises(ValueError):
            _acc(**bad)
    with pytest.raises(ValueError, match="missing from audio_durations"):
        _acc(audio_durations={"f": 23.4})                                  # a ground-truth file without a duration
    for cls in (roc.MultilabelAUROC,):
        with pytest.raises(NotImplementedError):
            cls(4, average="micro")
        with pytest.raises(NotImplementedError):
            cls(4, thresholds=100)
        with pytest.raises(NotImplementedError):
            cls(4, ignore_index=-1)
        with pytest.raises(ValueError):
            cls(4, average="samples")
        with pytest.raises(ValueError):
            cls(4, max_fpr=0.0)
        with pytest.raises(ValueError):
            cls(4, max_fpr=0.5, normalize="none")
        with pytest.raises(RuntimeError, match="before any update"):
            cls(4).compute()
    # update's refusals come before anything touches a device: a fake "cuda" tensor is not needed, the checks run on the host first
    x = torch.zeros(1, 156, 2)
    acc = _acc(clip_ids="sliding")
    for name, msg in (("f-0", "is not"), ("f-a-b", "is not"), ("f-1000-1000", "no length"), ("h-0-1000", "missing from"),
                      ("f-1500-2500", "runs past"), ("g-100-1100", "runs past")):
        with pytest.raises(ValueError, match=msg):
            acc.update(x, [name])
    with pytest.raises(ValueError, match="scored twice"):
        acc.update(torch.zeros(2, 156, 2), ["f-0-1000", "f-0-1000"])
    with pytest.raises(ValueError, match="overlaps no frame"):
        acc.update(x, ["f-0-1100"])                                        # 11 segments, the frames end at 9.984 s
    with pytest.raises(ValueError, match="overlaps no frame"):
        _acc().update(x, ["f"])                                            # a whole 23.4 s file under 156 frames of 64 ms
    with pytest.raises(ValueError, match=r"\[n, 156, 2\]"):
        acc.update(torch.zeros(1, 100, 2), ["f-0-1000"])
    with pytest.raises(ValueError, match="one filename"):
        acc.update(x, [])
    with pytest.raises(RuntimeError, match="no CPU path"):
        acc.update(x, ["f-0-1000"])
    with pytest.raises(RuntimeError, match="no clip was scored"):
        acc.segment_scores()
    assert acc._clips == [] and acc._seen == set()                         # a refused update leaves nothing behind


def test_header_constants_equal_pythons():
    src = open(os.path.join(ROOT, "include", "sed_hip.h")).read()
    names = re.findall(r"#define\s+(SED_(?:ROC|SEG)_\w+)\s+(\d+)", src)
    assert len(names) == 7
    for name, value in names:
        assert getattr(roc, name) == int(value), name
    assert roc.SED_ROC_MAX_CHUNK == roc.AP_CHUNK and roc.SED_ROC_OUT == len(roc.ROC_INTS) == len(RC.INTS)
    from transformer4sed_amd import _lib
    protos = _lib.parse_header()
    for name in ("sed_roc_compute", "sed_segment_pool", "sed_segment_gather"):
        assert name in protos
    assert int(re.search(r"#define\s+SED_HIP_ABI_VERSION\s+(\d+)", src).group(1)) == 7
