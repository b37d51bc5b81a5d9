"""The intersection-based PSDS on the device (csrc/psds.hip + IntersectionPSDS) against the host references of tests/psds_cases.py:
integer counts exact, PSDS and single-class PSDS within 1e-9 -- float64 sums of at most 1e7 terms: far above their rounding, far below
one operating point's share of the area."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import psds_cases as PC  # noqa: E402
from transformer4sed_amd import evaluation as EV  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-9
CASES = {"a": PC.case_a, "b": PC.case_b, "c": PC.case_c, "d": PC.case_d}


@functools.lru_cache(maxsize=None)
def _case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def _reference(name, args):
    """Computed once per (case, argument set), shared by the tests and never changed: `brute` where it is affordable (A, B), else the
    sweep restatement."""
    case, a = _case(name), PC.ARG_SETS[args]
    points = (PC.brute if name in ("a", "b") else PC.sweep_ref)(case, a)
    return points, PC.psds_from_points(case, a, points)


def _accumulate(case, a, max_efpr=PC.MAX_EFPR, batches=None, n_frames_on_device=False):
    gt, dur = PC.frames(case)
    acc = EV.IntersectionPSDS(gt, dur, case.classes, case.ts, a.dtc, a.gtc, a.cttc, a.alpha_ct, a.alpha_st, max_efpr)
    n = len(case.names)
    for lo, hi in batches or [(0, n)]:
        nf = None if case.n_frames is None else case.n_frames[lo:hi]
        if nf is not None and n_frames_on_device:
            nf = torch.tensor(nf, dtype=torch.int32, device=DEV)
        acc.update(torch.from_numpy(case.scores[lo:hi]).to(DEV), case.names[lo:hi], nf)
    return acc


@pytest.mark.parametrize("name,args", [("a", "psds1"), ("a", "psds2"), ("b", "psds1"), ("b", "psds2"), ("c", "psds1"), ("c", "psds2"),
                                       ("d", "psds1")])
def test_counts_exact_and_psds_vs_reference(name, args):
    case, a = _case(name), PC.ARG_SETS[args]
    points, (psds, single, _, _) = _reference(name, args)
    acc = _accumulate(case, a)
    got_rows = PC.counts_as_rows(acc)
    want_rows = PC.canonical(points, acc.ct_q)
    for c in range(len(case.classes)):
        assert got_rows[c] == want_rows[c], f"class {c}"          # value, TP, FP and the folded cross-trigger count, exactly
    got, got_single = acc.compute()
    err = max(abs(got_single[c] - s) for c, s in zip(case.classes, single))
    print(f"case {name} {args}: psds {got:.12f} (reference {psds:.12f}, diff {abs(got - psds):.2e}), single-class max diff {err:.2e}, "
          f"{sum(len(r) for r in got_rows)} points")
    assert abs(got - psds) <= TOL and err <= TOL
    assert (case.scores.shape[2] <= EV.PSDS_PADDED_CLASSES) == (name != "d")      # D is the many-class path


def test_many_classes_refuse_a_cross_trigger_threshold():
    case = _case("d")
    gt, dur = PC.frames(case)
    with pytest.raises(NotImplementedError, match="cttc"):
        EV.IntersectionPSDS(gt, dur, case.classes, case.ts, 0.1, 0.1, cttc_threshold=0.3, alpha_ct=0.5, alpha_st=1)


@pytest.mark.parametrize("args", ["psds1", "psds2"])
def test_batches_of_3_and_1_equal_one_batch(args):
    case, a = _case("a"), PC.ARG_SETS[args]
    one, split = _accumulate(case, a), _accumulate(case, a, batches=[(0, 3), (3, 4)])
    assert PC.counts_as_rows(one) == PC.counts_as_rows(split)       # bit for bit
    assert one.compute() == split.compute()


def test_n_frames_from_a_device_tensor():
    case, a = _case("b"), PC.PSDS2
    assert PC.counts_as_rows(_accumulate(case, a, n_frames_on_device=True)) == PC.counts_as_rows(_accumulate(case, a))


def test_anchors_on_the_device():
    """The hand-computed cases of tests/test_psds_cpu.py (their docstrings hold the arithmetic)."""
    from test_psds_cpu import _aligned_case, _tie_case, _two_class_case
    for a in PC.ARG_SETS.values():
        assert _accumulate(_aligned_case(), a, max_efpr=100.0).compute() == (1.0, {"x": 1.0, "y": 1.0})
    const = _aligned_case()._replace(scores=np.full((2, 10, 2), 0.25, np.float32))
    acc = _accumulate(const, PC.Args(0.5, 0.5, None, 0.0, 0.0), max_efpr=720.0)
    assert PC.counts_as_rows(acc) == [[(np.float32(0.25), 0, 2, 0)], [(np.float32(0.25), 2, 1, 0)]]
    got, single = acc.compute()
    assert abs(got - 0.25) < 1e-15 and single["x"] == 0.0 and abs(single["y"] - 0.5) < 1e-15
    acc = _accumulate(_two_class_case(), PC.Args(0.5, 0.5, None, 0.0, 0.0), max_efpr=720.0)
    assert acc.compute() == (0.625, {"x": 0.75, "y": 0.5})
    (grid, eff), _ = acc.roc()
    assert grid.tolist() == [0.0, 360.0] and eff.tolist() == [0.25, 1.0]
    tie = _accumulate(_tie_case(), PC.Args(0.5, 0.5, None, 0.0, 0.0), max_efpr=900.0, batches=[(0, 1), (1, 2)])
    assert tie.compute()[0] == 0.5 and PC.counts_as_rows(tie)[0][0] == (np.float32(0.5), 1, 1, 0)


def test_nan_scores_are_reported_at_compute():
    case, a = _case("a"), PC.PSDS1
    gt, dur = PC.frames(case)
    acc = EV.IntersectionPSDS(gt, dur, case.classes, case.ts, a.dtc, a.gtc)
    x = torch.from_numpy(case.scores).to(DEV)
    x[2, 7, 1] = float("nan")
    acc.update(x, case.names)                   # (stream-ordered: nothing is read back here)
    with pytest.raises(ValueError, match="NaN"):
        acc.compute()


def test_evaluator_psds_equals_psds_of_its_tables(tmp_path):
    """`Evaluator(..., ground_truth=, audio_durations=)` feeds the post-processed scores to the accumulators on the device; the result is
    the PSDS of the very tables it writes.  Without the arguments nothing changes: same tables, same event lists."""
    from copy import deepcopy

    import pandas as pd
    from oracle import eval_oracle as EO
    from test_gpu_model import _build
    from transformer4sed_amd import synth
    net, _ = _build(False, 2, 2)
    ema = deepcopy(net)
    with torch.no_grad():
        for p_ in ema.parameters():
            p_.mul_(1.01)
    cfg = {"training": {"median_window": [5, 20, 5, 5, 5, 20, 20, 20, 5, 20], "filter_type": "median", "weak_mask": True},
           "PaSST_SED": {"val_kwargs": {"encoder_win": True, "win_param": [512, 31], "mix_rate": 0.5, "temp_w": 0.5}}}
    enc = EV.Encoder(EO.LABELS, audio_len=10, frame_len=1024, frame_hop=320, net_pooling=1, sr=32000)
    rng = np.random.RandomState(5)
    rows = [(f"u{1 + i % 2}.wav", on, round(on + float(rng.uniform(0.5, 4.0)), 3), label)
            for i, label in enumerate(list(EO.LABELS) * 2) for on in [round(float(rng.uniform(0, 5.5)), 3)]]
    gt = pd.DataFrame(rows, columns=["filename", "onset", "offset", "event_label"])
    dur = pd.DataFrame({"filename": ["u1.wav", "u2.wav"], "duration": [10.0, 10.0]})
    gt_file, dur_file = str(tmp_path / "gt.tsv"), str(tmp_path / "dur.tsv")
    gt.to_csv(gt_file, sep="\t", index=False)
    dur.to_csv(dur_file, sep="\t", index=False)
    B = 2
    wav = torch.from_numpy(synth.synth_wav(B, seed=77)).to(DEV)
    labels = torch.from_numpy(synth.synth_batch_labels(B, 0, 0, seed=78)).to(DEV)
    pad = torch.zeros(B, 1000, dtype=torch.bool)
    paths = ["/x/val/u1.wav", "/x/val/u2.wav"]
    ev = EV.Evaluator(net, ema, enc, cfg, ground_truth=gt_file, audio_durations=dur_file)
    plain = EV.Evaluator(net, ema, enc, cfg)
    ev.step(wav, labels, pad, paths)
    plain.step(wav, labels, pad, paths)
    res = ev.psds()
    for who, tag in (("post_student", "s"), ("post_teacher", "t")):
        tables = getattr(ev.scores, who)
        for key, kw in EV.Evaluator.PSDS_ARGS.items():
            want, want_single = EV.compute_psds_from_scores(tables, gt_file, dur_file, **kw)
            assert res[f"{key}/{tag}"] == want and res["single"][f"{key}/{tag}"] == want_single
            assert 0.0 <= want <= 1.0 and set(want_single) == set(EO.LABELS)
    for name in EV.ScoreBufferTuple._fields:
        a, b = getattr(ev.scores, name), getattr(plain.scores, name)
        assert sorted(a) == sorted(b) == ["u1", "u2"] and all(a[k].equals(b[k]) for k in a)
    for who in ("student", "teacher"):
        assert ev.event_frame(who).equals(plain.event_frame(who))
    with pytest.raises(RuntimeError, match="ground_truth"):
        plain.psds()


def test_audioset_strong_evaluator_psds_honours_events_set(tmp_path):
    """`AudiosetStrongEvaluator(..., events_set=, ground_truth=, audio_durations=)`: the many-class path behind a real forward (402 of
    407 classes, no cross-trigger threshold, arguments of passt_cnn/train.py:174-186) equals the PSDS of the tables it keeps -- the
    ones with the classes outside `events_set` dropped."""
    import pandas as pd
    from test_gpu_as_eval import C, _encoder, build_dasm
    from transformer4sed_amd import synth
    net = build_dasm(2, nb=C)
    cfg = {net.get_model_name(): dict(val_kwargs=dict(encoder_win=False, temp_w=0.5), init_kwargs=dict(at_param=dict(out_type="sigmoid"))),
           "training": dict(median_window=7), "feature": dict(pred_len=1000)}
    enc = _encoder()
    kept = enc.labels[:-5]
    rng = np.random.RandomState(11)
    rows = [(f"clip_{i % 2}.wav", on, round(on + float(rng.uniform(0.3, 3.0)), 3), label)
            for i, label in enumerate(kept) for on in [round(float(rng.uniform(0, 6.5)), 3)]]
    gt = pd.DataFrame(rows, columns=["filename", "onset", "offset", "event_label"])
    dur = pd.DataFrame({"filename": ["clip_0.wav", "clip_1.wav"], "duration": [10.0, 10.0]})
    gt_file, dur_file = str(tmp_path / "gt.tsv"), str(tmp_path / "dur.tsv")
    gt.to_csv(gt_file, sep="\t", index=False)
    dur.to_csv(dur_file, sep="\t", index=False)
    ev = EV.AudiosetStrongEvaluator(net, enc, cfg, "dasm", events_set=set(kept), ground_truth=gt_file, audio_durations=dur_file)
    wav = torch.from_numpy(synth.synth_wav(2, seed=5100)).to(DEV)
    labels = torch.from_numpy(synth.synth_strong_labels(2, n_classes=C, seed=950)).to(DEV)
    ev.step(wav, labels, torch.zeros(2, 1000, dtype=torch.bool, device=DEV), ["/data/clip_0.wav", "/data/clip_1.wav"])
    psds, single = ev.psds()
    assert list(single) == kept and list(ev.scores["clip_0"].columns[2:]) == kept
    want, want_single = EV.compute_psds_from_scores(ev.scores, gt_file, dur_file, **EV.AudiosetStrongEvaluator.PSDS_ARGS)
    assert psds == want and single == want_single and 0.0 <= psds <= 1.0
