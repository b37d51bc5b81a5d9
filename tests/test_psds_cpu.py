"""The intersection-based PSDS without a GPU: the two host references of tests/psds_cases.py against each other, hand-computed anchors,
the equal-score trap, the sensitivity of the cases, and the host API of `IntersectionPSDS` / `compute_psds_from_scores` with the device
sweep replaced by `psds_cases.cpu_sweep` (everything behind the sweep -- merge, integer cumulation, rates, areas -- is the product's)."""
import os
import sys

import numpy as np
import pandas as pd
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import psds_cases as PC  # noqa: E402
from transformer4sed_amd import evaluation as EV  # noqa: E402

GPU_TOL = 1e-9          # tests/test_gpu_psds.py's bound on the PSDS


@pytest.fixture
def host_sweep(monkeypatch):
    monkeypatch.setattr(EV.IntersectionPSDS, "_sweep", lambda self, s, rows, nf: PC.cpu_sweep(self)(s, rows, nf))


def _accumulate(case, a, max_efpr=PC.MAX_EFPR, batches=None):
    gt, dur = PC.frames(case)
    acc = EV.IntersectionPSDS(gt, dur, case.classes, case.ts, a.dtc, a.gtc, a.cttc, a.alpha_ct, a.alpha_st, max_efpr)
    n = len(case.names)
    for lo, hi in batches or [(0, n)]:
        acc.update(torch.from_numpy(case.scores[lo:hi]), case.names[lo:hi], None if case.n_frames is None else case.n_frames[lo:hi])
    return acc


# ------------------------------------------------------------------------------------------------ the references agree
@pytest.mark.parametrize("name", ["psds1", "psds2"])
def test_sweep_equals_brute_on_a_and_b(name):
    a = PC.ARG_SETS[name]
    decreasing = 0
    for case in [PC.case_a(seed) for seed in range(30)] + [PC.case_b()]:
        b, s = PC.brute(case, a), PC.sweep_ref(case, a)
        assert b == s                                               # integer for integer, value for value
        pb, ps = PC.psds_from_points(case, a, b), PC.psds_from_points(case, a, s)
        assert abs(pb[0] - ps[0]) <= 1e-12 and np.allclose(pb[1], ps[1], rtol=0, atol=1e-12)
        decreasing += sum(PC.has_decreasing_tp(b))
    print(f"{name}: class curves with a decreasing TP step: {decreasing}")
    assert decreasing >= 1, "the cases are too tame: no detection ever fails the DTC after growing"


# ------------------------------------------------------------------------------------------------ anchors
def _aligned_case():
    """Two clips, 10 frames of 1 s, 2 classes; the scores ARE the frame-aligned ground truth."""
    gt = [(0, 0, 2.0, 5.0), (0, 1, 6.0, 9.0), (1, 0, 0.0, 3.0), (1, 1, 1.0, 4.0), (1, 1, 7.0, 10.0)]
    scores = np.zeros((2, 10, 2), np.float32)
    for clip, k, on, off in gt:
        scores[clip, int(on):int(off), k] = 1.0
    return PC.Case(scores, np.arange(11.0), None, gt, [10.0, 10.0], ["u", "v"], ["x", "y"])


@pytest.mark.parametrize("name", ["psds1", "psds2"])
def test_anchor_perfect_scores(name, host_sweep):
    """At value 1 every detection is exactly one event: TP = n_ref, FP = 0, eFPR = 0.  At value 0 the whole clip is one detection; it
    only adds points to the right.  The staircase is 1 from eFPR 0 on: PSDS and every single-class value are 1.0."""
    case, a = _aligned_case(), PC.ARG_SETS[name]
    for points in (PC.brute(case, a), PC.sweep_ref(case, a)):
        psds, single, _, _ = PC.psds_from_points(case, a, points, max_efpr=100.0)
        assert psds == 1.0 and single == [1.0, 1.0]
        assert [p[0][1:3] for p in points] == [(2, 0), (3, 0)]
    got, got_single = _accumulate(case, a, max_efpr=100.0).compute()
    assert got == 1.0 and got_single == {"x": 1.0, "y": 1.0}


def test_anchor_constant_scores(host_sweep):
    """Constant scores: one operating point per class, one whole-clip detection (10 s) per clip.  dtc = gtc = 0.3, no cttc.
    Class x: clip u holds 2..5 (3 s >= 0.3 * 10: passes, covers the event: TP), clip v holds 0..3 (passes, TP): TP 2 of 2, FP 0.
    Class y: clip u holds 6..9 (3 s: passes, TP 1), clip v holds 1..4 and 7..10 (6 s: passes, both covered: TP 2): TP 3 of 3, FP 0.
    With dtc = 0.5: x fails in both clips (3 < 5): TP 0, FP 2; y fails in u (FP 1), passes in v (TP 2 of 3).
    20 s of audio: one FP is 180 per hour.  max_efpr 720: x is 0 throughout -> 0; y is 2/3 from eFPR 180 on
    -> 2/3 * (720 - 180) / 720 = 0.5; mean 1/3 over [180, 720] -> PSDS (alpha_st 0) = 1/3 * 540 / 720 = 0.25."""
    case = _aligned_case()._replace(scores=np.full((2, 10, 2), 0.25, np.float32))
    easy = PC.Args(0.3, 0.3, None, 0.0, 0.0)
    assert PC.brute(case, easy) == [[(0.25, 2, 0, [0, 0])], [(0.25, 3, 0, [0, 0])]]
    hard = PC.Args(0.5, 0.5, None, 0.0, 0.0)
    assert PC.brute(case, hard) == PC.sweep_ref(case, hard) == [[(0.25, 0, 2, [0, 0])], [(0.25, 2, 1, [0, 0])]]
    psds, single, _, _ = PC.psds_from_points(case, hard, PC.brute(case, hard), max_efpr=720.0)
    assert abs(psds - 0.25) < 1e-15 and single[0] == 0.0 and abs(single[1] - 0.5) < 1e-15
    acc = _accumulate(case, hard, max_efpr=720.0)
    got, got_single = acc.compute()
    assert abs(got - 0.25) < 1e-15 and got_single["x"] == 0.0 and abs(got_single["y"] - 0.5) < 1e-15
    assert PC.counts_as_rows(acc) == [[(np.float32(0.25), 0, 2, 0)], [(np.float32(0.25), 2, 1, 0)]]


def _two_class_case():
    gt = [(0, 0, 0.0, 2.0), (0, 0, 6.0, 8.0), (0, 1, 4.0, 6.0)]
    scores = np.zeros((1, 10, 2), np.float32)
    scores[0, :, 0] = [0.9, 0.9, 0.1, 0.7, 0.1, 0.1, 0.5, 0.5, 0.1, 0.1]
    scores[0, :, 1] = [0.1, 0.8, 0.1, 0.1, 0.6, 0.6, 0.1, 0.1, 0.1, 0.1]
    return PC.Case(scores, np.arange(11.0), None, gt, [10.0], ["w"], ["x", "y"])


def test_anchor_two_classes_five_points(host_sweep):
    """One clip of 10 s, frames of 1 s, dtc = gtc = 0.5, no cttc, alpha_st = 0, max_efpr = 720 per hour; one FP is 360 per hour.
    Class x, events 0..2 and 6..8; scores 0.9 on frames 0-1, 0.7 on frame 3, 0.5 on frames 6-7, 0.1 elsewhere:
        v = 0.9: detection 0..2 passes, covers the first event      -> TP 1, FP 0   (eFPR   0, TPR 0.5)
        v = 0.7: + detection 3..4, no overlap                       -> TP 1, FP 1   (eFPR 360, TPR 0.5)
        v = 0.5: + detection 6..8 passes                            -> TP 2, FP 1   (eFPR 360, TPR 1.0)
        v = 0.1: one detection 0..10, 4 s of 10 < 0.5               -> TP 0, FP 1   (eFPR 360, TPR 0)
    Class y, event 4..6; scores 0.8 on frame 1, 0.6 on frames 4-5, 0.1 elsewhere:
        v = 0.8: detection 1..2, no overlap                         -> TP 0, FP 1   (eFPR 360, TPR 0)
        v = 0.6: + detection 4..6 passes                            -> TP 1, FP 1   (eFPR 360, TPR 1)
        v = 0.1: detection 0..10, 2 s of 10                         -> TP 0, FP 1   (eFPR 360, TPR 0)
    Staircases: x = 0.5 on [0, 360), 1 from 360; y = 0 on [0, 360), 1 from 360.  PSD-ROC (mean): (0, 0.25), (360, 1.0).
    PSDS = (0.25 * 360 + 1.0 * 360) / 720 = 0.625; single-class: x 0.75, y 0.5."""
    case, a = _two_class_case(), PC.Args(0.5, 0.5, None, 0.0, 0.0)
    want = [[(0.9, 1, 0), (0.7, 1, 1), (0.5, 2, 1), (0.1, 0, 1)], [(0.8, 0, 1), (0.6, 1, 1), (0.1, 0, 1)]]
    for points in (PC.brute(case, a), PC.sweep_ref(case, a)):
        assert [[(round(v, 6), tp, fp) for v, tp, fp, _ in pts] for pts in points] == want
        psds, single, (grid, eff), _ = PC.psds_from_points(case, a, points, max_efpr=720.0)
        assert grid.tolist() == [0.0, 360.0] and eff.tolist() == [0.25, 1.0]
        assert psds == 0.625 and single == [0.75, 0.5]
    acc = _accumulate(case, a, max_efpr=720.0)
    assert acc.compute() == (0.625, {"x": 0.75, "y": 0.5})
    (grid, eff), per_class = acc.roc()
    assert grid.tolist() == [0.0, 360.0] and eff.tolist() == [0.25, 1.0]
    assert per_class["x"][1][-1] == 1.0 and per_class["y"][0].max() == 360.0


# ------------------------------------------------------------------------------------------------ the tie trap
def _tie_case():
    """Two clips hold the score value 0.5 in one frame each: in clip p it lies on the event (a TP), in clip q there is no event (an FP).
    Merged, the value is ONE point (TP 1, FP 1).  A running sum that visits p first exposes (TP 1, FP 0): TPR 1 at eFPR 0."""
    scores = np.zeros((2, 4, 1), np.float32)
    scores[0, 1, 0] = 0.5
    scores[1, 2, 0] = 0.5
    return PC.Case(scores, np.arange(5.0), None, [(0, 0, 1.0, 2.0)], [4.0, 4.0], ["p", "q"], ["x"])


def test_tie_trap_one_point_per_value(host_sweep):
    case, a = _tie_case(), PC.Args(0.5, 0.5, None, 0.0, 0.0)
    merged = PC.sweep_ref(case, a)
    assert merged == PC.brute(case, a)
    assert merged[0][0] == (0.5, 1, 1, [0])
    # one FP in 8 s = 450 per hour: the staircase is 0 on [0, 450), 1 from there
    right = PC.psds_from_points(case, a, merged, max_efpr=900.0)[0]
    assert right == 0.5
    wrong = PC.psds_from_points(case, a, PC.sweep_ref(case, a, merge_equal=False), max_efpr=900.0)[0]
    assert wrong == 1.0 and wrong > right                          # the invented point dominates: the test sees the mistake
    acc = _accumulate(case, a, max_efpr=900.0, batches=[(0, 1), (1, 2)])
    assert acc.compute()[0] == 0.5
    assert PC.counts_as_rows(acc)[0][0] == (np.float32(0.5), 1, 1, 0)


# ------------------------------------------------------------------------------------------------ sensitivity of case A
@pytest.mark.parametrize("name", ["psds1", "psds2"])
def test_case_a_sees_what_it_should(name):
    case, a = PC.case_a(), PC.ARG_SETS[name]
    base = PC.psds_from_points(case, a, PC.brute(case, a))[0]
    dropped_clip = PC.psds_from_points(case, a, PC.brute(case, a, clips=[0, 1, 2]), clips=[0, 1, 2])[0]
    no_last_group = PC.psds_from_points(case, a, [pts[:-1] for pts in PC.brute(case, a)])[0]
    strict = PC.psds_from_points(case, a, PC.brute(case, a, strict=True))[0]
    print(f"{name}: base {base:.12f}, one clip less {dropped_clip:.12f}, last value group dropped {no_last_group:.12f}, "
          f"ties with > {strict:.12f}")
    for other in (dropped_clip, no_last_group, strict):
        assert abs(other - base) > GPU_TOL


# ------------------------------------------------------------------------------------------------ host API
def test_class_equals_reference_on_a(host_sweep):
    for name, a in PC.ARG_SETS.items():
        case = PC.case_a()
        ref = PC.sweep_ref(case, a)
        want = PC.psds_from_points(case, a, ref)
        acc = _accumulate(case, a, batches=[(0, 3), (3, 4)])
        assert PC.counts_as_rows(acc) == PC.canonical(ref, acc.ct_q)
        got, single = acc.compute()
        assert abs(got - want[0]) <= GPU_TOL
        assert np.allclose([single[c] for c in case.classes], want[1], rtol=0, atol=GPU_TOL)
        one = _accumulate(case, a)
        assert PC.counts_as_rows(one) == PC.counts_as_rows(acc) and one.compute() == (got, single)


def test_compute_psds_from_scores_on_tables(host_sweep, tmp_path):
    case, a = PC.case_a(), PC.PSDS2
    gt, dur = PC.frames(case)
    gt_file, dur_file = tmp_path / "gt.tsv", tmp_path / "dur.tsv"
    gt.to_csv(gt_file, sep="\t", index=False)
    dur.to_csv(dur_file, sep="\t", index=False)
    tables = PC.score_tables(case)
    psds, single = EV.compute_psds_from_scores(tables, str(gt_file), str(dur_file), a.dtc, a.gtc, a.cttc, a.alpha_ct, a.alpha_st,
                                               max_efpr=PC.MAX_EFPR, save_dir=str(tmp_path / "out"))
    want = PC.psds_from_points(case, a, PC.sweep_ref(case, a))
    assert abs(psds - want[0]) <= GPU_TOL and set(single) == set(case.classes)
    assert sorted(os.listdir(tmp_path / "out" / "scores")) == [n + ".tsv" for n in case.names]
    import transformer4sed_amd
    assert transformer4sed_amd.compute_psds_from_scores is EV.compute_psds_from_scores
    assert transformer4sed_amd.IntersectionPSDS is EV.IntersectionPSDS


def test_argument_checks_and_refusals(host_sweep):
    case = PC.case_a()
    gt, dur = PC.frames(case)
    make = lambda **kw: EV.IntersectionPSDS(**{**dict(ground_truth=gt, audio_durations=dur, event_classes=case.classes, timestamps=case.ts,
                                                     dtc_threshold=0.7, gtc_threshold=0.7), **kw})
    with pytest.raises(NotImplementedError, match="1024"):
        make(timestamps=np.arange(1026) * 0.01)
    many = [f"class{k}" for k in range(33)]
    with pytest.raises(NotImplementedError, match="cttc"):
        make(event_classes=many, cttc_threshold=0.3)
    with pytest.raises(ValueError, match="without a ground-truth event"):
        make(event_classes=many)
    for bad in (dict(dtc_threshold=0.0), dict(gtc_threshold=1.5), dict(cttc_threshold=-0.1), dict(unit_of_time="day"),
                dict(max_efpr=0), dict(timestamps=[0.0]), dict(timestamps=[0.0, 1.0, 0.5]), dict(event_classes=["class0", "class0"])):
        with pytest.raises(ValueError):
            make(**bad)
    with pytest.raises(ValueError, match="not one of event_classes"):
        make(event_classes=case.classes[:2])
    with pytest.raises(ValueError, match="missing from audio_durations"):
        make(audio_durations=dur.iloc[:3])
    acc = make()
    x = torch.from_numpy(case.scores)
    with pytest.raises(ValueError, match="scores must be"):
        acc.update(x[:, :-1], case.names)
    with pytest.raises(ValueError, match="fp32"):
        acc.update(x.double(), case.names)
    with pytest.raises(ValueError, match="missing from audio_durations"):
        acc.update(x[:1], ["stranger.wav"])
    acc.update(x[:2], ["some/dir/clip0.wav", "clip1"])
    with pytest.raises(ValueError, match="clip1.*twice"):
        acc.update(x[1:3], case.names[1:3])
    with pytest.raises(ValueError, match="twice"):
        acc.update(x[2:4], ["clip2", "clip2"])
    with pytest.raises(ValueError, match=r"without scores.*clip2.*clip3"):
        acc.compute()
    acc.update(x[2:], case.names[2:])
    assert 0.0 <= acc.compute()[0] <= 1.0


def test_sweep_has_no_host_fallback():
    """Without the test's stand-in the sweep is the HIP kernel: a CPU tensor is refused, not quietly evaluated on the host."""
    case = PC.case_a()
    gt, dur = PC.frames(case)
    acc = EV.IntersectionPSDS(gt, dur, case.classes, case.ts, 0.7, 0.7)
    with pytest.raises(RuntimeError, match="MI355X"):
        acc.update(torch.from_numpy(case.scores), case.names)
    assert not acc._seen
