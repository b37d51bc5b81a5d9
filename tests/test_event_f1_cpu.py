"""The event-based and segment-based F1 without a GPU: the two host references of tests/f1_cases.py against each other, hand-computed
cases, what the case set can tell apart, the scores from hand-written counts, and the host API of `EventSegmentF1` /
`log_sedeval_metrics` with the device kernel replaced by `f1_cases.cpu_counts` (everything around the counting -- ground-truth lists,
refusals, list building, scores, files -- is the product's)."""
import functools
import os
import sys

import numpy as np
import pandas as pd
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f1_cases as FC  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ev():
    from transformer4sed_amd import evaluation as EV
    return EV


@pytest.fixture
def host_counts(monkeypatch):
    monkeypatch.setattr(_ev().EventSegmentF1, "_run", lambda self, rows, active=None, est=None: FC.cpu_counts(self)(rows, active, est))


@functools.lru_cache(maxsize=None)
def _cases():
    return FC.cpu_cases()


def _accumulate(case, batches=None, order=None, **kw):
    acc = _ev().EventSegmentF1(FC.frames(case), case.classes, case.ts, **kw)
    n = len(case.names)
    order = list(range(n)) if order is None else order
    for lo, hi in batches or [(0, n)]:
        idx = order[lo:hi]
        acc.update(torch.from_numpy(case.active[idx]), [case.names[i] for i in idx])
    return acc


# ------------------------------------------------------------------------------------------------ the references agree
def test_brute_equals_greedy_on_all_cases():
    pairs = 0
    for name, case in _cases():
        counts, status = FC.greedy_ref(case)
        assert status == 0, f"{name}: the estimates a reference event hits are not one interval"
        assert FC.brute(case) == counts, name
        pairs += case.active.shape[0] * case.active.shape[2]
    print(f"{len(_cases())} cases, {pairs} (clip, class) pairs")


def _changed(**kw):
    n = 0
    for _, case in _cases():
        right, wrong = FC.pair_tp(case), FC.pair_tp(case, **kw)
        n += sum(1 for k in right if right[k] != wrong[k])
    return n


def test_the_cases_tell_first_fit_from_the_maximum():
    n = _changed(matching="first_fit")
    print(f"(clip, class) pairs where first-fit in reference order misses the maximum: {n}")
    assert n >= 10


@pytest.mark.parametrize("mode", ["no_offset", "strict", "no_max"])
def test_the_cases_see_each_mistake_of_the_predicate(mode):
    n = _changed(mode=mode)
    print(f"(clip, class) pairs whose tp changes with the mistake {mode!r}: {n}")
    assert n >= 10


def test_planted_ties_are_exact():
    """Every pair of `case_ties` behaves as its docstring says, pair by pair."""
    case = FC.case_ties()
    ok, strict, no_max, no_off = (FC.pair_tp(case, mode=m) for m in ("ok", "strict", "no_max", "no_offset"))
    for b in range(len(case.names)):
        assert [ok[(b, k)] for k in range(5)] == [1, 1, 1, 1, 0]
        assert [strict[(b, k)] for k in range(5)] == [0, 0, 0, 1, 0]
        assert [no_max[(b, k)] for k in range(5)] == [1, 1, 0, 0, 0]
        assert [no_off[(b, k)] for k in range(5)] == [1, 1, 1, 1, 1]
    refs, ests = FC.lists_of_case(case)
    assert refs[(0, 0)] == [(2000000, 4000000)] and ests[(0, 0)] == [(2200000, 4000000)]       # |d on| = 200000 = collar
    assert ests[(1, 1)] == [(2000000, 3600000)] and ests[(0, 2)] == [(2000000, 2700000)]       # 0.2 * 2 s; collar on a 0.5 s event


# ------------------------------------------------------------------------------------------------ hand-computed
def test_two_references_two_estimates_first_fit_finds_one(host_counts):
    """`case_first_fit`'s docstring holds the arithmetic: per clip n_ref 2, n_sys 2, maximum 2, first-fit 1.  Segments (1 s): the first
    clip's references cover 0.99 .. 1.34 -> segments 0 and 1, the estimates 1.00 .. 1.40 -> segment 1: tp 1, fp 0, fn 1."""
    case = FC.case_first_fit()
    n = len(case.names)
    assert FC.brute(case)["tp"] == [2 * n] and FC.brute(case, matching="first_fit")["tp"] == [n]
    assert FC.greedy_ref(case) == (FC.brute(case), 0)
    one = case._replace(active=case.active[:1], gt=[g for g in case.gt if g[0] == 0], names=case.names[:1])
    want = dict(n_ref=[2], n_sys=[2], tp=[2], seg_tp=[1], seg_fp=[0], seg_fn=[1])
    assert FC.brute(one) == want and FC.counts_of(_accumulate(one)) == want
    res = _accumulate(one).compute()
    assert res["event_micro"] == res["event_macro"] == 1.0 and res["segment_micro"] == 2 / 3


def _hand_case():
    """One clip of 10 s, frames of 1 s, classes x, y, z.
    x: references 1 .. 4 and 6 .. 7; estimates 1 .. 4 (frames 1-3), 6 .. 8 (frames 6-7), 9 .. 10 (frame 9).
       1..4 / 1..4 hit.  6..7 / 6..8: |d off| = 1.0 > max(0.2, 0.2): no hit.  -> n_ref 2, n_sys 3, tp 1.
       segments: reference {1, 2, 3, 6}, estimates {1, 2, 3, 6, 7, 9} -> tp 4, fp 2, fn 0.
    y: reference 0 .. 5; estimate 0 .. 6 (frames 0-5): |d off| = 1.0 <= max(0.2, 1.0), a tie: hit.  -> 1, 1, 1; segments 5, 1, 0.
    z: reference 2.5 .. 3.5, no estimate -> 1, 0, 0; segments {2, 3}: 0, 0, 2."""
    active = np.zeros((1, 10, 3), dtype=bool)
    active[0, [1, 2, 3, 6, 7, 9], 0] = True
    active[0, 0:6, 1] = True
    gt = [(0, 0, 1.0, 4.0), (0, 0, 6.0, 7.0), (0, 1, 0.0, 5.0), (0, 2, 2.5, 3.5)]
    return FC.Case(active, np.arange(11.0), gt, ["w"], ["x", "y", "z"])


def test_hand_computed_counts_and_scores(host_counts):
    case = _hand_case()
    want = dict(n_ref=[2, 1, 1], n_sys=[3, 1, 0], tp=[1, 1, 0], seg_tp=[4, 5, 0], seg_fp=[2, 1, 0], seg_fn=[0, 0, 2])
    assert FC.brute(case) == want and FC.greedy_ref(case) == (want, 0)
    acc = _accumulate(case)
    assert FC.counts_of(acc) == want
    res = acc.compute()
    # event: x 2 / 5, y 2 / 2, z 0 -> macro (0.4 + 1 + 0) / 3; micro 2 * 2 / (4 + 4)
    assert res["event_macro"] == pytest.approx((0.4 + 1.0) / 3, abs=1e-15) and res["event_micro"] == 0.5
    # segment: x 8 / 10, y 10 / 11, z 0 -> macro; micro 18 / (18 + 3 + 2)
    assert res["segment_macro"] == pytest.approx((0.8 + 10 / 11) / 3, abs=1e-15) and res["segment_micro"] == pytest.approx(18 / 23, abs=1e-15)
    assert res["class_wise"]["x"] == dict(event_f1=0.4, segment_f1=0.8, n_ref=2, n_sys=3, tp=1, seg_tp=4, seg_fp=2, seg_fn=0)
    assert res["class_wise"]["z"]["event_f1"] == 0.0 and res["class_wise"]["z"]["segment_f1"] == 0.0


def test_scores_from_hand_written_counts():
    scores = _ev().EventSegmentF1.scores
    c = dict(n_ref=[4, 0, 2, 0], n_sys=[2, 3, 0, 0], tp=[2, 0, 0, 0], seg_tp=[3, 0, 0, 0], seg_fp=[1, 2, 0, 0], seg_fn=[2, 0, 5, 0])
    s = scores(c)
    assert s["event_f1"].tolist() == [4 / 6, 0.0, 0.0, 0.0]
    assert s["event_macro"] == (4 / 6 + 0.0) / 2                    # classes 0 and 2 have reference events; 1 and 3 are left out
    assert s["event_micro"] == 4 / 11
    assert s["segment_f1"].tolist() == [6 / 9, 0.0, 0.0, 0.0]
    assert s["segment_macro"] == (6 / 9 + 0.0) / 2 and s["segment_micro"] == 6 / (6 + 3 + 7)
    z = scores({k: [0, 0] for k in FC.NAMES})                       # nothing detected, nothing to detect
    assert (z["event_macro"], z["event_micro"], z["segment_macro"], z["segment_micro"]) == (0.0, 0.0, 0.0, 0.0)
    nothing = scores(dict(n_ref=[3], n_sys=[0], tp=[0], seg_tp=[0], seg_fp=[0], seg_fn=[4]))
    assert nothing["event_micro"] == 0.0 and nothing["event_macro"] == 0.0


# ------------------------------------------------------------------------------------------------ host API on the stand-in
def test_class_equals_brute_and_ignores_the_split(host_counts):
    for name, case in _cases()[:3] + _cases()[-3:]:
        want = FC.brute(case)
        n = len(case.names)
        assert FC.counts_of(_accumulate(case)) == want, name
        if n >= 4:
            assert FC.counts_of(_accumulate(case, batches=[(0, 3), (3, n)], order=list(reversed(range(n))))) == want, name


def test_list_form_equals_frame_form_and_decode_strong(host_counts):
    EV = _ev()
    case = FC.case_trailing()
    enc = EV.Encoder(case.classes, audio_len=10, frame_len=1024, frame_hop=1024, net_pooling=1, sr=16000)     # 64 ms frames, 10 s
    assert FC.us(enc._frame_to_time(np.arange(case.active.shape[1] + 1))) == FC.us(case.ts)
    pred = EV._events_frames([case.active], case.names, enc, [0.5])[0.5]
    rows = lambda df: sorted((l, FC.us(a)[0], FC.us(z)[0], f) for l, a, z, f in df[["event_label", "onset", "offset", "filename"]].values.tolist())
    assert rows(pred) == rows(FC.events_frame(case))
    assert (pred["onset"] == pred["offset"]).sum() >= 3                 # the zero-length events are in the list
    acc = EV.EventSegmentF1(FC.frames(case), case.classes, case.ts)
    acc.update_events(pred, case.names)
    assert FC.counts_of(acc) == FC.brute(case) == FC.counts_of(_accumulate(case))
    assert FC.brute(case)["tp"][0] >= 1


def test_log_sedeval_metrics(host_counts, tmp_path):
    EV = _ev()
    case = FC.case_random(1)
    gt_file = tmp_path / "gt.tsv"
    FC.frames(case).to_csv(gt_file, sep="\t", index=False)
    pred = FC.events_frame(case)
    stranger = pd.DataFrame([("class0", 1.0, 2.0, "not_in_the_ground_truth.wav")], columns=pred.columns)
    got = EV.log_sedeval_metrics(pd.concat([pred, stranger], ignore_index=True), str(gt_file), save_dir=str(tmp_path / "out"))
    want = EV.EventSegmentF1.scores(FC.brute(case))
    assert got == (want["event_macro"], want["event_micro"], want["segment_macro"], want["segment_micro"])
    assert all(0.0 <= v <= 1.0 for v in got) and got[1] > 0.0
    assert sorted(os.listdir(tmp_path / "out")) == ["event_f1.txt", "segment_f1.txt"]
    assert f"micro {got[1]:.6f}" in open(tmp_path / "out" / "event_f1.txt").read()
    five = EV.log_sedeval_metrics(pred, str(gt_file), return_class_wise=True)
    assert (five[0], five[1], five[3], five[4]) == got and set(five[2]) <= set(case.classes)


def test_log_sedeval_metrics_on_an_empty_frame(tmp_path):
    import transformer4sed_amd
    empty = pd.DataFrame(columns=["event_label", "onset", "offset", "filename"])
    assert transformer4sed_amd.log_sedeval_metrics(empty, str(tmp_path / "never_read.tsv")) == (0.0, 0.0, 0.0, 0.0)


def test_exports_resolve():
    import transformer4sed_amd
    EV = _ev()
    assert transformer4sed_amd.EventSegmentF1 is EV.EventSegmentF1
    assert transformer4sed_amd.log_sedeval_metrics is EV.log_sedeval_metrics


def test_source_is_built_and_declared():
    from transformer4sed_amd import build
    from transformer4sed_amd._lib import parse_header
    assert "event_f1.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "event_f1.hip"))
    protos = parse_header(os.path.join(REPO, "include", "sed_hip.h"))
    assert [n for _, n in protos["sed_event_f1_counts"]][:2] == ["active", "est_ptr"] and len(protos["sed_event_f1_counts"]) == 20
    header = open(os.path.join(REPO, "include", "sed_hip.h")).read()
    assert "evaluation_measures.py:52-152" in header


def test_refusals(host_counts):
    EV = _ev()
    case = FC.case_random(0)
    gt = FC.frames(case)
    make = lambda **kw: EV.EventSegmentF1(**{**dict(ground_truth=gt, event_classes=case.classes, timestamps=case.ts), **kw})
    row = lambda **kw: pd.DataFrame([{**dict(filename="clip0.wav", onset=1.0, offset=2.0, event_label="class0"), **kw}])
    with pytest.raises(ValueError, match="offset <= onset"):
        make(ground_truth=pd.concat([gt, row(offset=1.0)], ignore_index=True))
    with pytest.raises(ValueError, match="not one of event_classes"):
        make(ground_truth=pd.concat([gt, row(event_label="stranger")], ignore_index=True))
    with pytest.raises(NotImplementedError, match="1024"):
        make(timestamps=np.arange(1026) * 0.01)
    with pytest.raises(NotImplementedError, match=r"events \(at most 256\)"):
        make(ground_truth=pd.concat([gt] + [row(onset=0.01 * i, offset=0.01 * i + 0.5) for i in range(257)], ignore_index=True))
    with pytest.raises(NotImplementedError, match="65 segments"):
        make(ground_truth=pd.concat([gt, row(onset=64.0, offset=64.5)], ignore_index=True))
    with pytest.raises(NotImplementedError, match="segments"):
        make(timestamps=np.arange(66.0))
    with pytest.raises(NotImplementedError, match="segments"):
        make(time_resolution=0.1)
    for bad in (dict(time_resolution=0.0), dict(t_collar=-0.1), dict(percentage_of_length=1.5), dict(event_classes=["class0", "class0"]),
                dict(timestamps=[0.0]), dict(timestamps=[0.0, 1.0, 0.5])):
        with pytest.raises(ValueError):
            make(**bad)
    acc = make()
    x = torch.from_numpy(case.active)
    with pytest.raises(ValueError, match="active must be a"):
        acc.update(x[:, :-1], case.names)
    with pytest.raises(ValueError, match="bool or uint8"):
        acc.update(x.float(), case.names)
    with pytest.raises(ValueError, match="missing from the ground truth"):
        acc.update(x[:1], ["stranger.wav"])
    acc.update(x[:2], ["some/dir/clip0.wav", "clip1"])
    with pytest.raises(ValueError, match="clip1.*twice"):
        acc.update(x[1:3], case.names[1:3])
    with pytest.raises(ValueError, match="twice"):
        acc.update(x[2:4], ["clip2", "clip2"])
    with pytest.raises(ValueError, match=r"without scores.*clip2.*clip3"):
        acc.compute()
    ev = lambda rows: pd.DataFrame(rows, columns=["event_label", "onset", "offset", "filename"])
    with pytest.raises(ValueError, match="overlapping"):
        acc.update_events(ev([("class0", 1.0, 2.0, "clip2.wav"), ("class0", 1.5, 2.5, "clip2.wav")]))
    with pytest.raises(NotImplementedError, match="513 estimated"):
        acc.update_events(ev([("class1", 0.01 * i, 0.01 * i + 0.005, "clip2.wav") for i in range(513)]))
    with pytest.raises(NotImplementedError, match="segments"):
        acc.update_events(ev([("class0", 70.0, 71.0, "clip2.wav")]))
    with pytest.raises(ValueError, match="not one of event_classes"):
        acc.update_events(ev([("stranger", 1.0, 2.0, "clip2.wav")]))
    with pytest.raises(ValueError, match="missing from the ground truth"):
        acc.update_events(ev([("class0", 1.0, 2.0, "stranger.wav")]))
    assert acc._seen == {"clip0", "clip1"}                             # a refused call scores nothing
    acc.update_events(ev([("class0", 1.0, 2.0, "clip2.wav"), ("class0", 2.0, 2.5, "clip2.wav"), (np.nan, np.nan, np.nan, "clip3.wav")]))
    assert 0.0 <= acc.compute()["event_micro"] <= 1.0
    acc.reset()
    assert not acc._seen and int(acc._counts.sum()) == 0


def test_broken_invariant_is_an_error(host_counts):
    """Status bit 1 (a non-hit between two hits) turns into RuntimeError at `compute`."""
    case = _hand_case()
    acc = _accumulate(case)
    acc._status |= 1
    with pytest.raises(RuntimeError, match="interval"):
        acc.compute()


def test_counting_has_no_host_fallback():
    """Without the test's stand-in the counting is the HIP kernel: a CPU tensor is refused, not quietly evaluated on the host."""
    case = _hand_case()
    acc = _ev().EventSegmentF1(FC.frames(case), case.classes, case.ts)
    with pytest.raises(RuntimeError, match="MI355X"):
        acc.update(torch.from_numpy(case.active), case.names)
    assert not acc._seen
