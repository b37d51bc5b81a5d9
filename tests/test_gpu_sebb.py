"""Sound event bounding boxes on the device (csrc/sebb.hip, transformer4sed_amd/sebb.py) against the host references
of tests/sebb_cases.py: scores, boxes, confidences and counts with exact equality, sentinels around every output and in the unused box
slots; the bank against its single-row launches; overflow and clamping in the status words; `SebbPostprocessor`, `Evaluator` with and
without one, and the two tools."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda"

import f1_cases as FC  # noqa: E402
import psds_cases as PC  # noqa: E402
import search_cases as SC  # noqa: E402
import sebb_cases as BC  # noqa: E402
from transformer4sed_amd import evaluation as EV, filter as dev_filter, sebb as SB  # noqa: E402
from transformer4sed_amd._lib import SedHipError  # noqa: E402
from transformer4sed_amd.ops import call, h2d  # noqa: E402

GUARD = 64
F_SENT, I_SENT = -12345.0, -777


def _guarded(n, dtype, sentinel):
    buf = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _launch(x, rows, scale=None, cap=None):
    """One raw launch into sentinel-filled, guarded buffers -> dict of host arrays; asserts the guards are intact."""
    B, T, C = x.shape
    K = len(rows)
    cap = (T + 1) // 2 if cap is None else cap
    params = SB.check_rows(rows, T, C)
    x_d = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    sc_d = None if scale is None else torch.from_numpy(np.ascontiguousarray(scale, dtype=np.float32)).to(DEV)
    shapes = dict(scores=((K, B, T, C), torch.float32, F_SENT), boxes=((K, B, C, cap, 2), torch.int32, I_SENT),
                  conf=((K, B, C, cap), torch.float32, F_SENT), counts=((K, B, C), torch.int32, I_SENT), status=((2,), torch.int32, I_SENT))
    bufs = {k: _guarded(int(np.prod(s)), dt, sent) for k, (s, dt, sent) in shapes.items()}
    call("sed_sebb_bank", x_d, sc_d, h2d(params, torch.int32, x_d.device), bufs["scores"][1], bufs["boxes"][1], bufs["conf"][1],
         bufs["counts"][1], bufs["status"][1], B, T, C, K, cap)
    out = {}
    for k, (s, _, sent) in shapes.items():
        whole = bufs[k][0].cpu().numpy()
        assert (whole[:GUARD] == sent).all() and (whole[-GUARD:] == sent).all(), f"{k}: a write outside the buffer"
        out[k] = whole[GUARD:-GUARD].reshape(s)
    return out


def _check_against_host(got, x, rows, scale=None, cap=None):
    """Exact equality with the host reference; slots from the count on still hold the sentinel."""
    B, T, C = x.shape
    cap = (T + 1) // 2 if cap is None else cap
    scores, boxes = BC.bank_ref(x, rows, scale)
    assert np.array_equal(got["scores"].view(np.int32), scores.view(np.int32))
    n_boxes, over = 0, False
    for (k, b, c), (bx, cf) in boxes.items():
        assert got["counts"][k, b, c] == len(bx), (k, b, c)
        m = min(len(bx), cap)
        over = over or len(bx) > cap
        assert got["boxes"][k, b, c, :m].tolist() == [list(v) for v in bx[:m]], (k, b, c)
        assert np.array_equal(got["conf"][k, b, c, :m].view(np.int32), np.asarray(cf[:m], dtype=np.float32).view(np.int32))
        assert (got["boxes"][k, b, c, m:] == I_SENT).all() and (got["conf"][k, b, c, m:] == F_SENT).all()
        n_boxes += len(bx)
    assert got["status"].tolist() == [int(over), 0]
    return n_boxes


def _rows(C, T):
    """Four rows with L = 1, 2, 25, 512 (one of them with parameters that differ per class), tau and rho from tight to loose."""
    mixed = ([(1, 2, 25, 512)[c % 4] for c in range(C)], [(0.0, 0.1, 0.2, 1.0)[c % 4] for c in range(C)], [(1.0, 1.5, 2.0, 16.0)[(c // 2) % 4] for c in range(C)])
    return [BC.uniform_row(C, 1, 0.2, 2.0), BC.uniform_row(C, 2, 0.05, 1.25), BC.uniform_row(C, 25, 0.3, 3.0), BC.uniform_row(C, 512, 0.15, 1.5),
            mixed]


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("C", [1, 10, 17])
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 1000, 1024])
def test_bank_equals_the_host_reference(T, C):
    """Smooth rows and rows on {0, 0.25, 0.5, 1} (ties in D and in the means everywhere), every L of {1, 2, 25, 512} (so L below, at and
    beyond T), two clips."""
    n = 0
    for x in (BC.smooth(2, T, C, seed=1), BC.grid(2, T, C, seed=2)):
        rows = _rows(C, T)
        n += _check_against_host(_launch(x, rows), x, rows)
    assert n > 0


def test_constructed_rows():
    """All zeros, all ones, a plateau at each end and one in the middle, as five clips of one class."""
    T = 40
    x = np.stack([np.zeros(T, dtype=np.float32), np.ones(T, dtype=np.float32), BC.plateau(T, 0, 7), BC.plateau(T, 33, 40, 0.625),
                  BC.plateau(T, 10, 20)])[:, :, None]
    rows = [BC.uniform_row(1, L, 0.2, 2.0) for L in (1, 5, 12, 64)]
    got = _launch(x, rows)
    _check_against_host(got, x, rows)
    assert got["counts"][:, :, 0].tolist() == [[0, 1, 1, 1, 1]] * 4
    assert got["boxes"][1, :, 0, 0].tolist()[1:] == [[0, T], [0, 7], [33, 40], [10, 20]] and got["conf"][1, 3, 0, 0] == np.float32(0.625)


def test_weak_scale():
    """The scale is multiplied in with one fp32 multiply before quantisation; a zero scale leaves no box."""
    x = BC.smooth(3, 200, 5, seed=3)
    scale = np.random.RandomState(4).rand(3, 5).astype(np.float32)
    scale[1, 2], scale[0, 0] = 0.0, 1.0
    rows = _rows(5, 200)[:3]
    got = _launch(x, rows, scale)
    _check_against_host(got, x, rows, scale)
    assert not got["scores"][:, 1, :, 2].any() and not got["counts"][:, 1, 2].any()


def test_more_rows_than_one_pass_of_any_grid():
    """300 x 17 = 5100 (clip, class) columns: one workgroup each (the launch does not stride), several per CU."""
    x = np.concatenate([BC.smooth(150, 33, 17, seed=5), BC.grid(150, 33, 17, seed=6)])
    rows = [BC.uniform_row(17, 2, 0.2, 2.0), BC.uniform_row(17, 7, 0.1, 1.5)]
    assert _check_against_host(_launch(x, rows), x, rows) > 5100


def test_bank_equals_its_single_row_launches():
    """Nine rows with mixed and repeated L (shared steps 1-4) against nine launches of one row each, bit for bit."""
    x = np.concatenate([BC.smooth(2, 1000, 10, seed=7), BC.grid(1, 1000, 10, seed=8)])
    Ls = (16, 24, 16, 32, 24, 16, 1, 32, 1000)
    rows = [BC.uniform_row(10, L, (0.15, 0.2, 0.3)[k % 3], (1.5, 2.0, 3.0)[(k // 3) % 3]) for k, L in enumerate(Ls)]
    rows[4] = ([16, 24, 32, 16, 24, 32, 1, 2, 3, 500], rows[4][1], [1.0 + 0.25 * c for c in range(10)])
    bank = _launch(x, rows)
    for k, row in enumerate(rows):
        one = _launch(x, [row])
        for name in ("scores", "boxes", "conf", "counts"):
            assert np.array_equal(bank[name][k].view(np.int32), one[name][0].view(np.int32)), (k, name)
    assert bank["status"].tolist() == [0, 0] and bank["counts"].sum() > 0


def test_overflow_is_reported_and_nothing_is_written_past_the_capacity():
    x = BC.grid(2, 300, 3, seed=9)
    rows = [BC.uniform_row(3, 1, 0.0, 1.0), BC.uniform_row(3, 25, 0.2, 2.0)]
    full = _launch(x, rows)
    assert full["counts"].max() > 8 and full["status"].tolist() == [0, 0]
    got = _launch(x, rows, cap=3)
    _check_against_host(got, x, rows, cap=3)                        # (guards, sentinels and the first three boxes of every row)
    assert got["status"].tolist() == [1, 0] and np.array_equal(got["counts"], full["counts"])
    assert np.array_equal(got["scores"].view(np.int32), full["scores"].view(np.int32))
    bank = SB.sebb_bank(torch.from_numpy(x).to(DEV), rows, capacity=3)
    with pytest.raises(RuntimeError, match="capacity"):
        SB.box_lists(bank)


def test_scores_outside_the_unit_interval_are_clamped_and_flagged():
    """What the host's check refuses: the kernel treats NaN and negative scores as 0, scores above 1 as 1, and sets status[1]."""
    x = BC.smooth(2, 100, 3, seed=10)
    bad = x.copy()
    bad[0, 10:14, 1], bad[1, 50, 2], bad[1, 60:70, 0] = np.nan, -0.5, 1.5
    rows = _rows(3, 100)[:3]
    got = _launch(bad, rows)
    assert got["status"].tolist() == [0, 1]
    clamped = np.clip(np.nan_to_num(bad, nan=0.0), 0, 1)
    want = BC.bank_ref(clamped, rows)[0]
    assert np.array_equal(got["scores"].view(np.int32), want.view(np.int32))
    with pytest.raises(ValueError, match="NaN"):
        SB.sebb_bank(torch.from_numpy(bad).to(DEV), rows)


def test_bad_arguments_are_refused_before_anything_is_written():
    x = torch.rand(1, 8, 2, device=DEV)
    p = h2d(SB.check_rows([BC.uniform_row(2, 1, 0.2, 2.0)], 8, 2), torch.int32, x.device)
    for T, K, cap in ((1025, 1, 4), (8, 65, 4), (8, 0, 4), (8, 1, 0), (8, 1, 1025), (0, 1, 4)):
        out = torch.full((64,), F_SENT, device=DEV)
        ints = torch.full((64,), I_SENT, dtype=torch.int32, device=DEV)
        with pytest.raises(SedHipError):
            call("sed_sebb_bank", x, None, p, out, ints, out, ints, ints, 1, T, 2, K, cap)
        assert (out == F_SENT).all() and (ints == I_SENT).all()


# ------------------------------------------------------------------------------------------------ the Python layer
def test_postprocessor_scores_boxes_and_events():
    from transformer4sed_amd.longform import decode_events
    case = SC.planted()
    enc = SC.planted_encoder(case)
    weak = SC.planted_weak(case)
    pp = SB.SebbPostprocessor(enc, [0.3, 0.7, 1.5], [0.1, 0.2, 0.3], 2.0)
    assert pp.half_lengths == [3, 7, 15]
    strong = torch.from_numpy(case.scores).transpose(1, 2).contiguous().to(DEV)
    weak_d = torch.from_numpy(weak).to(DEV)
    for w, w_d in ((None, None), (weak, weak_d)):
        want, boxes = BC.bank_ref(case.scores, [pp.row], w)
        got = pp.scores(strong, w_d)
        assert got.shape == (8, 160, 3) and np.array_equal(got.cpu().numpy().view(np.int32), want[0].view(np.int32))
        lists = pp.boxes(strong, w_d)
        for b in range(8):
            for c in range(3):
                bx, cf = boxes[(0, b, c)]
                assert [(a, e) for a, e, _ in lists[b][c]] == bx and [np.float32(v) for _, _, v in lists[b][c]] == cf
        for th in (0.3, [0.2, 0.5, 0.7]):
            events = pp.events(strong, w_d, th)
            for b in range(8):
                assert np.array_equal(events[b], decode_events(got[b], th).cpu().numpy())
        assert sum(len(e) for e in events) > 0
    assert pp.scores(strong[:0]).shape == (0, 160, 3) and pp.boxes(strong[:0]) == []


def _evaluator_inputs():
    case = SC.planted()
    enc = SC.planted_encoder(case)
    gt, dur = PC.frames(case)
    weak = SC.planted_weak(case)
    weak[1, 2], weak[5, 0] = 0.25, 0.375                            # two (clip, class) pairs below the half-point mask
    strong = torch.from_numpy(case.scores).transpose(1, 2).contiguous().to(DEV)
    return case, enc, gt, dur, weak, strong, [n + ".wav" for n in case.names]


def test_evaluator_with_a_postprocessor_equals_the_host_pipeline():
    case, enc, gt, dur, weak, strong, names = _evaluator_inputs()
    cfg = {"training": {"median_window": [5, 20, 7], "filter_type": "median", "weak_mask": True}}
    pp = SB.SebbPostprocessor(enc, [0.3, 0.7, 1.5], 0.2, [1.5, 2.0, 3.0])
    ev = EV.Evaluator(None, None, enc, cfg, ground_truth=gt, audio_durations=dur, sebb=pp)
    weak_d = torch.from_numpy(weak).to(DEV)
    for who in ("student", "teacher"):
        ev._finish(ev._enqueue(who, strong, weak_d, names))
    soft = BC.bank_ref(case.scores, [pp.row], weak)[0][0]                            # the score tables: soft weak scale
    hard = BC.bank_ref(case.scores, [pp.row], (weak >= np.float32(0.5)).astype(np.float32))[0][0] > np.float32(0.5)
    psds, f1 = ev.psds(), ev.f1()
    for name in ("psds1", "psds2"):
        host = EV.IntersectionPSDS(gt, dur, case.classes, case.ts, **EV.Evaluator.PSDS_ARGS[name])
        host._sweep = PC.cpu_sweep(host)
        host.update(torch.from_numpy(soft), case.names)
        overall, single = host.compute()
        assert psds[name + "/s"] == overall == psds[name + "/t"] and psds["single"][name + "/s"] == single
    host = EV.EventSegmentF1(gt, case.classes, case.ts)
    host._run = FC.cpu_counts(host)
    host.update(torch.from_numpy(hard), case.names)
    want = host.compute()
    assert f1["class_wise"]["s"] == want["class_wise"] == f1["class_wise"]["t"]
    for key in ("event_macro", "event_micro", "segment_macro", "segment_micro"):
        assert f1[key + "/s"] == want[key] == f1[key + "/t"]
    assert want["segment_macro"] > 0 and int(host.counts()["n_sys"].sum()) > 0     # (boxes were found and overlap the ground truth)
    for b, n in enumerate(case.names):
        assert np.array_equal(ev.scores.post_student[n][case.classes].to_numpy(), soft[b].astype(np.float64))
    events = ev.event_frame("student")
    assert len(events) == sum(len(enc.decode_strong(hard[b])) for b in range(8)) > 0
    # the same through the reference's call contract
    raw, post = EV.batched_decode_preds(strong, names, enc, filter=[5, 20, 7], weak_preds=weak_d, need_weak_mask=True, sebb=pp)
    assert all(post[n].equals(ev.scores.post_student[n]) and raw[n].equals(ev.scores.raw_student[n]) for n in case.names)


def test_evaluator_without_a_postprocessor_is_the_filter_path():
    """The default is today's path: the tables are the scipy median's bits and the events the torch median's, as before."""
    case, enc, gt, dur, weak, strong, names = _evaluator_inputs()
    cfg = {"training": {"median_window": [5, 20, 7], "filter_type": "median", "weak_mask": True}}
    weak_d = torch.from_numpy(weak).to(DEV)
    ev = EV.Evaluator(None, None, enc, cfg, ground_truth=gt, audio_durations=dur)
    assert ev.sebb is None
    ev._finish(ev._enqueue("student", strong, weak_d, names))
    x = strong.transpose(1, 2).contiguous()
    post = dev_filter.median_filter_scipy(x, ev.median_filter, weak_d).cpu().numpy()
    binm = (dev_filter.median_filter_torch(x * (weak_d >= 0.5).float().unsqueeze(1), ev.median_filter) > 0.5).cpu().numpy()
    for b, n in enumerate(case.names):
        assert np.array_equal(ev.scores.post_student[n][case.classes].to_numpy(), post[b].astype(np.float64))
    want = EV._events_frames([binm], names, enc, [0.5])[0.5]
    assert ev.event_frame("student").equals(want) and len(want) > 0
    host = EV.IntersectionPSDS(gt, dur, case.classes, case.ts, **EV.Evaluator.PSDS_ARGS["psds1"])
    host.update(torch.from_numpy(post).to(DEV), case.names)
    assert ev._psds["student"]["psds1"].compute() == host.compute()


def test_search_on_the_device_equals_the_search_through_the_host_references():
    case, enc, gt, dur, weak, strong, names = _evaluator_inputs()
    kw = dict(objectives=("psds1", "psds2", "event_f1", "segment_f1"), thresholds=(0.3, 0.5), weak_mask=True, **BC.SEARCH_GRID)
    dev = SB.SebbSearch(enc, gt, dur, **kw)
    weak_d = torch.from_numpy(weak).to(DEV)
    dev.update(strong[:3], weak_d[:3], names[:3])
    dev.update(strong[3:], weak_d[3:], names[3:])
    host = BC.host_search(case, **kw)
    host.update(strong.cpu(), torch.from_numpy(weak), names)
    assert dev.results().equals(host.results()) and len(dev.results()) == 12 * 3 * (2 + 2 * 2)
    for name in kw["objectives"]:
        assert dev.best(name) == host.best(name)


# ------------------------------------------------------------------------------------------------ the tools
LABELS = ["Alarm_bell_ringing", "Blender", "Cat", "Dishes", "Dog", "Electric_shaver_toothbrush", "Frying", "Running_water", "Speech",
          "Vacuum_cleaner"]
FAST = {"encoder_win": False, "temp_w": 0.5}


def test_tune_tool_with_sebb_then_detect_tool_with_its_choice(tmp_path, monkeypatch):
    """`tools/tune_postprocess.py --sebb` writes the table, the choices and the YAML fragment of a direct `SebbSearch`;
    `tools/detect.py --postprocess` with that choice writes the bounding-box scores and events of the recording's raw timeline."""
    import pandas as pd
    import yaml
    from test_gpu_model import _build
    from transformer4sed_amd import LongFormDetector, synth
    from transformer4sed_amd.data import WavBatchStream, write_wav
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import detect
    import tune_postprocess
    net = _build(False, 2, 2)[0]
    names = ["a", "b", "c"]
    rng = np.random.RandomState(3)
    rows = []
    for n in names:
        for label in LABELS:
            on = round(float(rng.uniform(0, 7)), 3)
            rows.append((n + ".wav", on, round(on + float(rng.uniform(0.3, 2.5)), 3), label))
    gt = pd.DataFrame(rows, columns=["filename", "onset", "offset", "event_label"])
    dur = pd.DataFrame({"filename": [n + ".wav" for n in names], "duration": [10.0] * 3})
    gt.to_csv(tmp_path / "val.tsv", sep="\t", index=False)
    dur.to_csv(tmp_path / "dur.tsv", sep="\t", index=False)
    os.makedirs(tmp_path / "wav")
    for n, x in zip(names, synth.synth_wav(3, seed=95)):
        write_wav(str(tmp_path / "wav" / (n + ".wav")), x[::2].copy(), 16000)
    cfg = {"training": {"median_window": [5, 20, 5, 5, 5, 20, 20, 20, 5, 20], "filter_type": "median", "weak_mask": True},
           "PaSST_SED": {"init_kwargs": {}, "val_kwargs": FAST},
           "feature": {"sr": 32000, "hopsize": 320, "win_length": 1024, "audio_max_len": 10, "net_subsample": 1}}
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    monkeypatch.setattr(detect, "load_model", lambda cfg, checkpoint, device: net)
    tune_postprocess.main(["--config", str(tmp_path / "cfg.yaml"), "--tsv", str(tmp_path / "val.tsv"), "--durations", str(tmp_path / "dur.tsv"),
                           "--wav-dir", str(tmp_path / "wav"), "--out", str(tmp_path / "out"), "--objectives", "psds1,event_f1",
                           "--thresholds", "0.3,0.5", "--sebb", "--step-filter-lengths", "0.32,0.64", "--merge-thresholds-abs", "0.15,0.3"])
    enc = EV.Encoder(LABELS, audio_len=10, frame_len=1024, frame_hop=320, net_pooling=1, sr=32000)
    search = SB.SebbSearch(enc, gt, dur, step_filter_lengths=(0.32, 0.64), merge_thresholds_abs=(0.15, 0.3), weak_mask=True,
                           objectives=("psds1", "event_f1"), thresholds=(0.3, 0.5))
    paths = [str(tmp_path / "wav" / (n + ".wav")) for n in names]
    net.eval()
    with torch.no_grad():
        for wav, pad_mask, idx in WavBatchStream(paths, [[0, 1, 2]], DEV, encoder=enc):
            ext = net.get_feature_extractor()
            ext.eval()
            strong, weak, _ = net(ext.logmel(wav), pad_mask=pad_mask.to(DEV), **FAST)
            search.update(strong, weak, [names[i] + ".wav" for i in idx])
    for name in ("psds1", "event_f1"):
        assert SB.SebbChoice.load(tmp_path / "out" / f"choice_{name}.json") == search.best(name)
    best = SB.SebbChoice.load(tmp_path / "out" / "choice.json")
    assert best == search.best("psds1") and yaml.safe_load(open(tmp_path / "out" / "postprocess.yaml"))["training"] == best.to_config()
    table = pd.read_csv(tmp_path / "out" / "search_table.tsv", sep="\t", float_precision="round_trip")
    assert np.array_equal(table["value"].to_numpy(), search.results()["value"].to_numpy()) and len(table) == 12 * 10 * (1 + 2)
    # detect: an 8 s recording (one clip) with the F1 choice, which carries per-class thresholds
    wav = synth.synth_wav(1, seed=91).reshape(-1)[:8 * 32000].copy()
    write_wav(str(tmp_path / "rec.wav"), wav, 32000)
    choice = SB.SebbChoice.load(tmp_path / "out" / "choice_event_f1.json")
    detect.main([str(tmp_path / "rec.wav"), "--config", str(tmp_path / "cfg.yaml"), "--out", str(tmp_path / "det"),
                 "--postprocess", str(tmp_path / "out" / "choice_event_f1.json")])
    det = LongFormDetector(net, enc, cfg)
    out = det.posteriors(det.load(str(tmp_path / "rec.wav")))
    out["post"] = choice.postprocessor(enc).scores_btc(out["raw"][None])[0]
    want = det.events(out, choice.thresholds)
    got = pd.read_csv(tmp_path / "det" / "events.tsv", sep="\t", float_precision="round_trip")
    assert got["event_label"].tolist() == want["event_label"].tolist()
    assert np.array_equal(got[["onset", "offset"]].to_numpy(), want[["onset", "offset"]].to_numpy())
    post = pd.read_csv(tmp_path / "det" / "scores_post" / "rec.tsv", sep="\t", float_precision="round_trip")
    assert np.array_equal(post.to_numpy(), det.tables(out, "rec")[1]["rec"].to_numpy()) and len(post) == 800
    assert os.path.exists(tmp_path / "det" / "scores_raw" / "rec.tsv")
    # a recording beyond one clip is refused
    write_wav(str(tmp_path / "long.wav"), synth.synth_wav(2, seed=92).reshape(-1)[:12 * 32000].copy(), 32000)
    with pytest.raises(SystemExit, match="1024"):
        detect.main([str(tmp_path / "long.wav"), "--config", str(tmp_path / "cfg.yaml"), "--out", str(tmp_path / "det2"),
                     "--postprocess", str(tmp_path / "out" / "choice_event_f1.json")])
