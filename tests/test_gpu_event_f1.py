"""The event-based and segment-based F1 counts on the device (csrc/event_f1.hip + EventSegmentF1) against `f1_cases.brute`: every
comparison is integer equality, there is no tolerance to choose.  The shapes are the smallest at which the kernel can still go wrong:
one frame, runs across the 64-lane boundary, the 512-estimate cap, more reference events of a class than lanes, more classes and
more (clip, class) pairs than any single pass would cover."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f1_cases as FC  # noqa: E402
from transformer4sed_amd import evaluation as EV  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _crossing(t):
    """Runs that cross (or end at) the boundary between the first and the second pass of 64 lanes, and the clip's last frame."""
    case = FC.case_shape(2, t, 2, seed=t)
    active = case.active.copy()
    active[:, 58:t, 0] = True
    active[0, 62:min(t, 66), 1] = True
    active[1, 63:64, 1] = True
    end = FC.GRID * t                                               # the crossing run spans 1.16 .. end
    gt = sorted(case.gt + [(0, 0, 1.1, round(end - 0.04, 3)), (1, 0, 1.2, round(end, 3)), (1, 0, 1.0, round(end + 0.2, 3))])
    return case._replace(active=active, gt=gt)


def _cap():
    """1024 alternating frames of 10 ms: 512 one-frame estimates per class.  Class 0: a one-frame reference event that 21 estimates hit and
    a longer one in the same place; class 1: a reference event only the 512th estimate (10.22 .. 10.23) hits."""
    case = FC.case_shape(1, 1024, 2, step=0.01, per_class=4, fill="alternate")
    return case._replace(gt=sorted(case.gt + [(0, 0, 5.0, 5.01), (0, 0, 5.0, 5.3), (0, 0, 4.9, 5.0), (0, 1, 10.4, 10.43)]))


def _encoder_ts():
    from oracle import eval_oracle as EO
    enc = EV.Encoder(EO.LABELS, audio_len=10, frame_len=1024, frame_hop=320, net_pooling=1, sr=32000)
    case = FC.case_shape(3, 1000, 10, step=0.01)
    return case._replace(ts=enc._frame_to_time(np.arange(1001)))


CASES = {
    "one_frame_on": lambda: FC.case_shape(1, 1, 1, step=1.0, fill="on"),
    "one_frame_off": lambda: FC.case_shape(1, 1, 1, step=1.0, fill="off"),
    "two_frames": lambda: FC.case_shape(2, 2, 1, step=0.5, fill="alternate"),
    "t63": lambda: _crossing(63), "t64": lambda: _crossing(64), "t65": lambda: _crossing(65),
    "cap_512_estimates": _cap,
    "encoder_ts": _encoder_ts,
    "many_refs": FC.case_many_refs,
    "c33": lambda: FC.case_shape(2, 100, 33),
    "n70": lambda: FC.case_shape(70, 64, 10),
    "trailing": FC.case_trailing,
    "ties": FC.case_ties, "first_fit": FC.case_first_fit, "dense": FC.case_dense, "random": FC.case_random,
}


@functools.lru_cache(maxsize=None)
def _case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def _reference(name):
    """Computed once per case, shared by the tests and never changed."""
    return FC.brute(_case(name))


def _accumulate(case, batches=None, order=None):
    acc = EV.EventSegmentF1(FC.frames(case), case.classes, case.ts)
    n = len(case.names)
    order = list(range(n)) if order is None else order
    for lo, hi in batches or [(0, n)]:
        idx = order[lo:hi]
        acc.update(torch.from_numpy(case.active[idx]).to(DEV), [case.names[i] for i in idx])
    return acc


@pytest.mark.parametrize("name", list(CASES))
def test_counts_equal_brute(name):
    case, want = _case(name), _reference(name)
    acc = _accumulate(case)
    got = FC.counts_of(acc)
    print(f"{name}: shape {case.active.shape}, n_ref {sum(want['n_ref'])}, n_sys {sum(want['n_sys'])}, tp {sum(want['tp'])}, "
          f"segments tp {sum(want['seg_tp'])} fp {sum(want['seg_fp'])} fn {sum(want['seg_fn'])}; device tp {sum(got['tp'])}")
    assert got == want
    assert int(acc._status.item()) == 0
    if name not in ("one_frame_on", "one_frame_off", "two_frames"):
        assert sum(want["tp"]) > 0, "the case matches nothing: it would not see a kernel that never matches"
    if name == "cap_512_estimates":
        assert want["n_sys"] == [512, 512] and want["tp"][1] == 1
    if name == "many_refs":
        assert want["n_ref"][0] == 130 and sum(want["n_ref"]) == 256
    if name == "first_fit":
        assert want["tp"] == [2 * len(case.names)] != FC.brute(case, matching="first_fit")["tp"]


def test_uint8_input_counts_any_non_zero_byte():
    case = _case("random")
    acc = EV.EventSegmentF1(FC.frames(case), case.classes, case.ts)
    acc.update(torch.from_numpy(case.active.astype(np.uint8) * 7).to(DEV), case.names)
    assert FC.counts_of(acc) == _reference("random") and int(acc._status.item()) == 0


def test_split_and_permutation_give_the_same_counts():
    case = _case("random")
    assert len(case.names) == 4
    one = FC.counts_of(_accumulate(case))
    assert one == FC.counts_of(_accumulate(case, batches=[(0, 3), (3, 4)])) == _reference("random")       # bit for bit: integers
    assert one == FC.counts_of(_accumulate(case, batches=[(0, 1), (1, 4)], order=[2, 0, 3, 1]))


@pytest.mark.parametrize("name", ["trailing", "dense", "cap_512_estimates", "many_refs"])
def test_list_form_equals_frame_form(name):
    case = _case(name)
    acc = EV.EventSegmentF1(FC.frames(case), case.classes, case.ts)
    acc.update_events(FC.events_frame(case), case.names)
    assert FC.counts_of(acc) == _reference(name) and int(acc._status.item()) == 0
    no_ts = EV.EventSegmentF1(FC.frames(case), case.classes, None)          # (the form log_sedeval_metrics uses)
    no_ts.update_events(FC.events_frame(case), case.names)
    assert FC.counts_of(no_ts) == _reference(name)


def test_list_and_frame_form_share_one_accumulator():
    case = _case("random")
    acc = EV.EventSegmentF1(FC.frames(case), case.classes, case.ts)
    pred = FC.events_frame(case)
    acc.update_events(pred[pred["filename"].isin(["clip0.wav", "clip1.wav"])], case.names[:2])          # the list form first
    acc.update(torch.from_numpy(case.active[2:]).to(DEV), case.names[2:])
    assert FC.counts_of(acc) == _reference("random") and int(acc._status.item()) == 0


def test_reset_and_log_sedeval_metrics(tmp_path):
    case = _case("random")
    acc = _accumulate(case)
    acc.reset()
    acc.update(torch.from_numpy(case.active).to(DEV), case.names)
    assert FC.counts_of(acc) == _reference("random")
    gt_file = tmp_path / "gt.tsv"
    FC.frames(case).to_csv(gt_file, sep="\t", index=False)
    want = EV.EventSegmentF1.scores(_reference("random"))
    got = EV.log_sedeval_metrics(FC.events_frame(case), str(gt_file))
    assert got == (want["event_macro"], want["event_micro"], want["segment_macro"], want["segment_micro"])


def test_evaluator_f1_equals_brute_on_its_event_lists(tmp_path):
    """`Evaluator(..., ground_truth=, audio_durations=)` feeds the device `bin` tensor to one EventSegmentF1 per model: `f1()` is `brute`
    on the event lists the same evaluator decodes on the host.  The PSDS and the tables do not move, and an Evaluator without ground
    truth gives bit-identical outputs, tables and event lists.  The ground truth is cut from the student's own events (moved by up to
    0.3 s), so that there is something to match."""
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
    B = 2
    wav = torch.from_numpy(synth.synth_wav(B, seed=77)).to(DEV)
    labels = torch.from_numpy(synth.synth_batch_labels(B, 0, 0, seed=78)).to(DEV)
    pad = torch.zeros(B, 1000, dtype=torch.bool)
    paths = ["/x/val/u1.wav", "/x/val/u2.wav"]
    plain = EV.Evaluator(net, ema, enc, cfg)
    out_plain = plain.step(wav, labels, pad, paths)
    rng = np.random.RandomState(5)
    rows = [(f, round(on + float(rng.choice([0.0, 0.1, -0.1, 0.2, 0.3])), 3), round(off + float(rng.choice([0.0, 0.1, 0.2, 0.5])), 3), label)
            for label, on, off, f in plain.event_frame("student").values.tolist()[:60] if off > on]
    rows = [(f, max(on, 0.0), min(off, 10.0), label) for f, on, off, label in rows if min(off, 10.0) > max(on, 0.0)]
    rows += [(f"u{1 + i % 2}.wav", on, round(on + float(rng.uniform(0.5, 4.0)), 3), label)
             for i, label in enumerate(list(EO.LABELS) * 2) for on in [round(float(rng.uniform(0, 5.5)), 3)]]
    gt = pd.DataFrame(rows, columns=["filename", "onset", "offset", "event_label"])
    dur = pd.DataFrame({"filename": ["u1.wav", "u2.wav"], "duration": [10.0, 10.0]})
    gt_file, dur_file = str(tmp_path / "gt.tsv"), str(tmp_path / "dur.tsv")
    gt.to_csv(gt_file, sep="\t", index=False)
    dur.to_csv(dur_file, sep="\t", index=False)

    ev = EV.Evaluator(net, ema, enc, cfg, ground_truth=gt_file, audio_durations=dur_file)
    no_f1 = EV.Evaluator(net, ema, enc, cfg, ground_truth=gt_file, audio_durations=dur_file)
    no_f1._f1_update = lambda who, binm, p: None            # the evaluator as it was before the F1 accumulators
    out_ev = ev.step(wav, labels, pad, paths)
    no_f1.step(wav, labels, pad, paths)
    res = ev.f1()
    gt_read = pd.read_csv(gt_file, sep="\t")
    for who, tag in (("student", "s"), ("teacher", "t")):
        pred = ev.event_frame(who)
        pred = pred if len(pred) else pd.DataFrame(columns=["event_label", "onset", "offset", "filename"])
        refs, ests = FC.lists_of_frames(gt_read, pred, ["u1", "u2"], EO.LABELS)
        want = FC.count_lists(refs, ests, len(EO.LABELS))
        assert FC.counts_of(ev._f1[who]) == want
        assert int(ev._f1[who]._status.item()) == 0
        s = EV.EventSegmentF1.scores(want)
        for k in ("event_macro", "event_micro", "segment_macro", "segment_micro"):
            assert res[f"{k}/{tag}"] == s[k] and 0.0 <= s[k] <= 1.0
        assert [res["class_wise"][tag][c]["tp"] for c in EO.LABELS] == want["tp"]
        print(f"{who}: n_ref {sum(want['n_ref'])}, n_sys {sum(want['n_sys'])}, tp {sum(want['tp'])}, event micro {s['event_micro']:.4f}, "
              f"segment micro {s['segment_micro']:.4f}")
    assert ev.psds() == no_f1.psds()
    for name in EV.ScoreBufferTuple._fields:
        a, b, c = (getattr(e.scores, name) for e in (ev, no_f1, plain))
        assert sorted(a) == sorted(b) == sorted(c) == ["u1", "u2"] and all(a[k].equals(b[k]) and a[k].equals(c[k]) for k in a)
    for who in ("student", "teacher"):
        assert ev.event_frame(who).equals(plain.event_frame(who)) and ev.event_frame(who).equals(no_f1.event_frame(who))
        assert all(torch.equal(x, y) for x, y in zip(out_ev[who], out_plain[who]))
    with pytest.raises(RuntimeError, match="ground_truth"):
        plain.f1()
