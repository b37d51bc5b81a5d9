"""The post-processing search on the device (csrc/median_filter.hip, transformer4sed_amd/postproc_search.py): the filter
bank bit for bit against per-row `sed_median_filter_k` launches and against the host filters of tests/search_cases.py, then the search on
the planted case against the same search run through the host stand-ins, `Evaluator` and per-threshold `EventSegmentF1` runs."""
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

import search_cases as SC  # noqa: E402
from transformer4sed_amd import filter as dev_filter  # noqa: E402
from transformer4sed_amd._lib import SedHipError  # noqa: E402
from transformer4sed_amd.ops import call, h2d  # noqa: E402

SENTINEL = -12345.0
GUARD = 64


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _launch_bank(x_d, rows, mode, scale_d, max_size):
    """-> (out [W, B, T, C], guard [GUARD]) of one raw launch into a sentinel-filled buffer."""
    B, T, C = x_d.shape
    W = len(rows)
    buf = torch.full((W * B * T * C + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    call("sed_median_filter_bank", x_d, buf, h2d(rows, torch.int32, x_d.device), scale_d, B, T, C, W, mode, max_size)
    got = buf.cpu().numpy()
    return got[:W * B * T * C].reshape(W, B, T, C), got[W * B * T * C:]


def _per_row(x_d, rows, mode, scale_d, max_size):
    B, T, C = x_d.shape
    out = []
    for row in rows:
        o = torch.full((B, T, C), SENTINEL, dtype=torch.float32, device=DEV)
        call("sed_median_filter_k", x_d, o, h2d(list(row), torch.int32, x_d.device), scale_d, B, T, C, mode, max_size)
        out.append(o.cpu().numpy())
    return np.stack(out)


def _pool(T, mode):
    """Window sizes: 1, 2 (even), both sides of the 24-frame switch, 129, and in the scipy modes a window equal to T."""
    pool = [1, 2, 23, 24, 25, 129] + ([T] if mode != 0 else [])
    return [k for k in pool if mode == 0 or k <= T]


def _rows(W, C, pool):
    """W rows whose windows differ per class and mix sizes below and from 24 frames within one class's column of the bank."""
    return [[pool[(2 * w + 3 * c + w * c) % len(pool)] for c in range(C)] for w in range(W)]


SHAPES = [(1, 8, 1), (3, 31, 3), (2, 65, 10), (2, 1000, 10), (37, 31, 29)]     # (the kernel does not cap its grid: 1073 workgroups)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_bank_is_the_clip_kernel_row_by_row_and_the_host_filter(shape, mode):
    """out[w] == sed_median_filter_k(sizes[w]) under the same bound, bit for bit, == the scipy / numpy reference; nothing is written
    behind the planes; a second run gives the same bits."""
    B, T, C = shape
    pool = _pool(T, mode)
    for W in (1, 3, 12):
        rows = _rows(W, C, pool)
        max_size = max(max(r) for r in rows)
        for ties in (False, True):
            x = SC.bank_input(B, T, C, seed=W, ties=ties)
            x_d = torch.from_numpy(x).to(DEV)
            for scaled in (False, True):
                scale = np.random.RandomState(W).randint(0, 9, size=(B, C)).astype(np.float32) / 8 if scaled else None
                scale_d = torch.from_numpy(scale).to(DEV) if scaled else None
                got, guard = _launch_bank(x_d, rows, mode, scale_d, max_size)
                assert np.all(guard == SENTINEL)
                assert np.array_equal(_bits(got), _bits(_per_row(x_d, rows, mode, scale_d, max_size))), (W, ties, scaled)
                assert np.array_equal(got, SC.bank_ref(x, rows, mode, scale)), (W, ties, scaled)
                again, _ = _launch_bank(x_d, rows, mode, scale_d, max_size)
                assert np.array_equal(_bits(got), _bits(again))
                if W == 3 and not scaled:
                    assert np.array_equal(_bits(dev_filter.filter_bank(x_d, rows, mode).cpu().numpy()), _bits(got))


@pytest.mark.parametrize("mode", [0, 1])
def test_bank_short_windows_only_at_1000_frames(mode):
    """All windows below 24 frames: the rank search in window order, as the clip kernel does it under that bound."""
    B, T, C = 2, 1000, 10
    rows = [[[1, 2, 5, 9, 23][(w + c) % 5] for c in range(C)] for w in range(4)]
    x = SC.bank_input(B, T, C, ties=True)
    x_d = torch.from_numpy(x).to(DEV)
    got, guard = _launch_bank(x_d, rows, mode, None, 23)
    assert np.all(guard == SENTINEL)
    assert np.array_equal(_bits(got), _bits(_per_row(x_d, rows, mode, None, 23)))
    assert np.array_equal(got, SC.bank_ref(x, rows, mode))


@pytest.mark.parametrize("T", [31, 300])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_window_out_of_range_is_a_nan_plane(T, mode):
    """A (row, class) window above max_size -- and in the scipy modes above T -- comes out as NaN; every other plane is intact.  T = 300
    with a bound of 30 is the order-statistics form, T = 31 the rank search."""
    B, C = 2, 3
    rows = [[5, 5, 5], [5, 40, 7], [7, 24, 30]]
    x = SC.bank_input(B, T, C)
    x_d = torch.from_numpy(x).to(DEV)
    got, guard = _launch_bank(x_d, rows, mode, None, 30)
    assert np.all(guard == SENTINEL)
    bad = np.zeros((3, B, T, C), dtype=bool)
    bad[1, :, :, 1] = True
    assert np.isnan(got[bad]).all() and not np.isnan(got[~bad]).any()
    ok_rows = [[5, 5, 5], [5, 5, 7], [7, 24, 30]]
    assert np.array_equal(got[~bad], SC.bank_ref(x, ok_rows, mode)[~bad])
    if mode != 0 and T == 31:                           # 40 > T under a bound that admits it
        got, _ = _launch_bank(x_d, rows, mode, None, 64)
        assert np.isnan(got[bad]).all() and np.array_equal(got[~bad], SC.bank_ref(x, ok_rows, mode)[~bad])


def _launch_clip(x_d, sizes, mode, scale_d, max_size):
    """-> (out [B, T, C], guard [GUARD]) of one raw `sed_median_filter_k` launch into a sentinel-filled buffer."""
    B, T, C = x_d.shape
    buf = torch.full((B * T * C + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    call("sed_median_filter_k", x_d, buf, h2d(list(sizes), torch.int32, x_d.device), scale_d, B, T, C, mode, max_size)
    got = buf.cpu().numpy()
    return got[:B * T * C].reshape(B, T, C), got[B * T * C:]


NAN_SIZES = [24, 5, 33]                                 # bound 33 at T = 256: the global-rank form, the 5-frame window riding along
NAN_ROWS = [[24, 5, 33], [5, 33, 24], [33, 24, 5]]
NAN_AT = ((1, 0), (0, 1))                               # (clip, class)


def _nan_case(partly=False):
    """-> (x finite, x under test, scale finite, scale under test, bad [B, C]) at [2, 256, 3]: NaN enters the two (clip, class) columns
    of NAN_AT through `scale` (the weak mask's route), or, `partly`, as every 7th frame of the input."""
    B, T, C = 2, 256, 3
    x = SC.bank_input(B, T, C, seed=4)
    scale = (np.random.RandomState(4).randint(1, 9, size=(B, C)) / 8).astype(np.float32)
    x_bad, scale_bad, bad = x.copy(), scale.copy(), np.zeros((B, C), dtype=bool)
    for b, c in NAN_AT:
        bad[b, c] = True
        if partly:
            x_bad[b, ::7, c] = np.nan
        else:
            scale_bad[b, c] = np.nan
    return x, x_bad, scale, scale_bad, bad


@pytest.mark.parametrize("mode", [0, 1])
def test_nan_column_is_a_nan_column_in_the_clip_kernel(mode):
    """A (clip, class) column that is all NaN (a fully padded clip's NaN weak posterior as `scale`) comes out all NaN from the global-rank
    form; every other column holds the bits of the same launch with a finite scale; nothing is written behind the buffer.  NaN is the
    references' own answer: `scipy.ndimage.median_filter` of an all-NaN line and `torch.median` of one both give NaN (checked on the
    host).  Payload bits are not compared."""
    x, _, scale, scale_bad, bad = _nan_case()
    x_d = torch.from_numpy(x).to(DEV)
    want, _ = _launch_clip(x_d, NAN_SIZES, mode, torch.from_numpy(scale).to(DEV), 33)
    got, guard = _launch_clip(x_d, NAN_SIZES, mode, torch.from_numpy(scale_bad).to(DEV), 33)
    assert np.all(guard == SENTINEL)
    sel = np.broadcast_to(bad[:, None, :], got.shape)
    assert np.isnan(got[sel]).all() and not np.isnan(want).any()
    assert np.array_equal(_bits(got[~sel]), _bits(want[~sel]))


@pytest.mark.parametrize("mode", [0, 1])
def test_nan_column_is_a_nan_column_in_the_bank(mode):
    """The same through the bank, three rows over the same windows: NaN where the column is NaN, the finite launch's bits elsewhere."""
    x, _, scale, scale_bad, bad = _nan_case()
    x_d = torch.from_numpy(x).to(DEV)
    want, _ = _launch_bank(x_d, NAN_ROWS, mode, torch.from_numpy(scale).to(DEV), 33)
    got, guard = _launch_bank(x_d, NAN_ROWS, mode, torch.from_numpy(scale_bad).to(DEV), 33)
    assert np.all(guard == SENTINEL)
    sel = np.broadcast_to(bad[None, :, None, :], got.shape)
    assert np.isnan(got[sel]).all() and not np.isnan(want).any()
    assert np.array_equal(_bits(got[~sel]), _bits(want[~sel]))


@pytest.mark.parametrize("mode", [0, 1])
def test_partly_nan_column_stays_inside_its_buffers(mode):
    """Every 7th frame of two columns NaN: their values are unspecified (colliding ranks); the launches return, write nothing behind
    their buffers and leave the NaN-free columns bit-equal to the finite launch."""
    x, x_bad, scale, _, bad = _nan_case(partly=True)
    x_d, bad_d, scale_d = torch.from_numpy(x).to(DEV), torch.from_numpy(x_bad).to(DEV), torch.from_numpy(scale).to(DEV)
    want, _ = _launch_clip(x_d, NAN_SIZES, mode, scale_d, 33)
    got, guard = _launch_clip(bad_d, NAN_SIZES, mode, scale_d, 33)
    sel = np.broadcast_to(bad[:, None, :], got.shape)
    assert np.all(guard == SENTINEL) and np.array_equal(_bits(got[~sel]), _bits(want[~sel]))
    want, _ = _launch_bank(x_d, NAN_ROWS, mode, scale_d, 33)
    got, guard = _launch_bank(bad_d, NAN_ROWS, mode, scale_d, 33)
    sel = np.broadcast_to(bad[None, :, None, :], got.shape)
    assert np.all(guard == SENTINEL) and np.array_equal(_bits(got[~sel]), _bits(want[~sel]))


@pytest.mark.parametrize("mode", [0, 1])
def test_clip_kernel_window_above_the_bound_is_a_nan_plane(mode):
    """Device sizes [5, 80, 7] under a bound of 30 at T = 300 (the global-rank form; 300 + 79 entries exceed its 11-word bitmaps): class 1
    comes out as NaN, classes 0 and 2 equal the host reference.  The bank's `test_window_out_of_range_is_a_nan_plane`, for the clip kernel."""
    B, T, C = 2, 300, 3
    x = SC.bank_input(B, T, C)
    got, guard = _launch_clip(torch.from_numpy(x).to(DEV), [5, 80, 7], mode, None, 30)
    assert np.all(guard == SENTINEL)
    assert np.isnan(got[:, :, 1]).all()
    want = SC.bank_ref(x, [[5, 5, 7]], mode)[0]
    assert np.array_equal(got[:, :, [0, 2]], want[:, :, [0, 2]])


def test_bad_arguments_write_nothing():
    B, T, C = 2, 31, 3
    x_d = torch.from_numpy(SC.bank_input(B, T, C)).to(DEV)
    for W, mode, max_size in ((65, 1, 5), (0, 1, 5), (2, 3, 5), (2, 1, 0)):
        rows = [[5] * C] * max(W, 1)
        buf = torch.full((max(W, 1) * B * T * C,), SENTINEL, dtype=torch.float32, device=DEV)
        with pytest.raises(SedHipError):
            call("sed_median_filter_bank", x_d, buf, h2d(rows, torch.int32, x_d.device), None, B, T, C, W, mode, max_size)
        assert bool((buf == SENTINEL).all())
    with pytest.raises(ValueError):
        dev_filter.filter_bank(x_d, [[5] * C] * 65, 1)
    with pytest.raises(ValueError):
        dev_filter.filter_bank(x_d, [[5, 32, 5]], 1)                # longer than the sequence, scipy semantics
    with pytest.raises(ValueError):
        dev_filter.filter_bank(x_d, [[5, 0, 5]], 0)
    with pytest.raises(ValueError):
        dev_filter.filter_bank(x_d, [[5, 5]], 0)


# ------------------------------------------------------------------------------------------------------------------ the search
import psds_cases as PC  # noqa: E402
from transformer4sed_amd import evaluation as EV  # noqa: E402
from transformer4sed_amd.postproc_search import PostprocChoice, PostprocSearch  # noqa: E402

THETAS = (0.3, 0.5, 0.7)
OBJECTIVES = ("psds1", "psds2", "event_f1", "segment_f1")


def _device_search(case, **kw):
    gt, dur = PC.frames(case)
    return PostprocSearch(SC.planted_encoder(case), gt, dur, **kw)


def _feed(search, case, weak, batches=None, order=None, dev=DEV):
    order = list(range(len(case.names))) if order is None else order
    strong = torch.from_numpy(case.scores).transpose(1, 2).contiguous().to(dev)
    weak = torch.from_numpy(weak).to(dev)
    for lo, hi in batches or [(0, len(order))]:
        idx = order[lo:hi]
        search.update(strong[idx].contiguous(), weak[idx].contiguous(), [case.names[i] + ".wav" for i in idx])
    return search


@pytest.fixture(scope="module")
def planted():
    case = SC.planted()
    weak = SC.planted_weak(case)
    kw = dict(windows=SC.PLANTED_WINDOWS, config_windows=SC.PLANTED_CONFIG, thresholds=THETAS, objectives=OBJECTIVES)
    return case, weak, kw, _feed(_device_search(case, **kw), case, weak)


def test_device_table_equals_the_host_table(planted):
    """The same search with the bank, the sweep and the counting kernel replaced by the host references: the same integers reach the same
    host arithmetic, so the tables and the choices are equal, not close."""
    case, weak, kw, dev = planted
    host = _feed(SC.host_search(case, **kw), case, weak, dev="cpu")
    got, want = dev.results(), host.results()
    assert len(got) == (2 * 2 + 2 * 3) * 6 * 3 and got.equals(want)
    for name in OBJECTIVES:
        for ft in ((None, "median", "max") if name.startswith("psds") else (None,)):
            assert dev.best(name, ft) == host.best(name, ft), (name, ft)
    best = dev.best("psds1")
    assert best.windows_frames == [31, 1, 7] and best.filter_type == "median"
    assert best.overall > max(v for k, v in dev.overall("psds1").items() if k != "config") and best.overall > best.config_overall


def test_batching_and_order_do_not_change_the_table(planted):
    case, weak, kw, dev = planted
    want = dev.results()
    perm = list(np.random.RandomState(5).permutation(8))
    for batches, order in (([(0, 3), (3, 8)], None), ([(0, 8)], perm)):
        assert _feed(_device_search(case, **kw), case, weak, batches, order).results().equals(want)


def test_f1_objectives_equal_per_threshold_accumulators(planted):
    """One `EventSegmentF1` per (threshold, candidate), fed what `_events_device` decodes with that candidate's windows."""
    case, weak, kw, dev = planted
    strong = torch.from_numpy(case.scores).transpose(1, 2).contiguous().to(DEV)
    weak_d = torch.from_numpy(weak).to(DEV)
    counts = dev._f1_counts()
    table = dev.results()
    for ti, th in enumerate(THETAS):
        for ci, cand in enumerate(dev.candidates):
            acc = EV.EventSegmentF1(PC.frames(case)[0], case.classes, case.ts)
            acc.update(EV._events_device(strong, weak_d, [th], cand.frames)[0], case.names)
            want = acc.counts()
            assert all(np.array_equal(want[k], counts[ti][ci][k]) for k in EV.F1_COUNTS), (th, cand.name)
            res = acc.compute()["class_wise"]
            for kind in ("event_f1", "segment_f1"):
                got = table[(table["objective"] == kind) & (table["candidate"] == cand.name) & (table["threshold"] == th)]
                assert got["value"].tolist() == [res[c][kind] for c in case.classes]


def test_config_row_equals_the_evaluator_on_the_same_clips():
    """1000 frames per clip, the frame count `Evaluator` scales the YAML's windows for: its PSDS (student) and its class-wise F1 at 0.5 are
    the search's "config" row."""
    case = SC.planted(seed=5, n=4, t=1000)
    weak = SC.planted_weak(case)
    enc = SC.planted_encoder(case)
    assert enc.n_frames == 1000
    gt, dur = PC.frames(case)
    config = [5, 20, 7]
    cfg = {"training": {"median_window": config, "filter_type": "median", "weak_mask": True}}
    ev = EV.Evaluator(None, None, enc, cfg, ground_truth=gt, audio_durations=dur)
    strong = torch.from_numpy(case.scores).transpose(1, 2).contiguous().to(DEV)
    weak_d = torch.from_numpy(weak).to(DEV)
    names = [n + ".wav" for n in case.names]
    for who in ("student", "teacher"):
        ev._finish(ev._enqueue(who, strong, weak_d, names))
    search = PostprocSearch(enc, gt, dur, windows=(5, 20), config_windows=config, weak_mask=True, filter_types=("median",),
                            objectives=("psds1", "psds2", "event_f1", "segment_f1"))
    assert search.candidates[-1].frames == ev.median_filter == [32, 128, 44]
    search.update(strong, weak_d, names)
    table = search.results()
    table = table[table["candidate"] == "config"]
    psds, f1 = ev.psds(), ev.f1()
    for name in ("psds1", "psds2"):
        assert search.overall(name)["config"] == psds[name + "/s"]
        assert table[table["objective"] == name]["value"].tolist() == [psds["single"][name + "/s"][c] for c in case.classes]
    for kind in ("event_f1", "segment_f1"):
        assert table[table["objective"] == kind]["value"].tolist() == [f1["class_wise"]["s"][c][kind] for c in case.classes]
    assert search.overall("event_f1")["config"] == f1["event_macro/s"]


# ------------------------------------------------------------------------------------------------------------------ model and tool
LABELS = ["Alarm_bell_ringing", "Blender", "Cat", "Dishes", "Dog", "Electric_shaver_toothbrush", "Frying", "Running_water", "Speech",
          "Vacuum_cleaner"]
FAST = {"encoder_win": False, "temp_w": 0.5}


@pytest.fixture(scope="module")
def net():
    from test_gpu_model import _build
    return _build(False, 2, 2)[0]


def _truth(names, seed=0):
    import pandas as pd
    rng = np.random.RandomState(seed)
    rows = []
    for i, n in enumerate(names):
        for label in LABELS:
            on = round(float(rng.uniform(0, 7)), 3)
            rows.append((n + ".wav", on, round(on + float(rng.uniform(0.3, 2.5)), 3), label))
    gt = pd.DataFrame(rows, columns=["filename", "onset", "offset", "event_label"])
    return gt, pd.DataFrame({"filename": [n + ".wav" for n in names], "duration": [10.0] * len(names)})


def test_one_update_from_a_real_forward(net):
    from transformer4sed_amd import synth
    enc = EV.Encoder(LABELS, audio_len=10, frame_len=1024, frame_hop=320, net_pooling=1, sr=32000)
    names = ["a", "b", "c"]
    gt, dur = _truth(names)
    wav = torch.from_numpy(synth.synth_wav(3, seed=81)).to(DEV)
    net.eval()
    with torch.no_grad():
        ext = net.get_feature_extractor()
        ext.eval()
        strong, weak, _ = net(ext.logmel(wav), pad_mask=torch.zeros(3, 1000, dtype=torch.bool, device=DEV), **FAST)
    search = PostprocSearch(enc, gt, dur, config_windows=[5, 20, 5, 5, 5, 20, 20, 20, 5, 20], weak_mask=True,
                            objectives=("psds1", "psds2", "event_f1"), thresholds=(0.3, 0.5))
    search.update(strong, weak, [n + ".wav" for n in names])
    assert [c.frames[0] for c in search.candidates[:-1]] == [6, 12, 19, 32, 44, 64, 89, 128, 179]
    table = search.results()
    assert len(table) == (2 * 2 + 2) * 10 * 10 and np.isfinite(table["value"].to_numpy()).all()
    for name in ("psds1", "psds2", "event_f1"):
        best = search.best(name)
        allowed = [set(c.frames[k] for c in search.candidates) for k in range(10)]
        assert all(f in allowed[k] for k, f in enumerate(best.windows_frames)) and len(best.windows_units) == 10
        assert 0.0 <= best.overall <= 1.0 and best.filter_type in ("median", "max")
        if name == "event_f1":
            assert all(t in (0.3, 0.5) for t in best.thresholds)
    # the bank's slice under the config row is the score-table path's own output
    x = strong.detach().transpose(1, 2).contiguous().float()
    rows = [c.frames for c in search.candidates]
    want = EV._scores_device(strong, 3, rows[-1], "median", weak, True)[1]
    assert torch.equal(dev_filter.filter_bank(x, rows, 1, weak.float())[-1], want)


def test_detect_tool_with_a_saved_choice(net, tmp_path, monkeypatch):
    """`tools/detect.py --postprocess CHOICE.json` writes what a `LongFormDetector` built with the choice's lists gives."""
    import pandas as pd
    import yaml
    from transformer4sed_amd import LongFormDetector, synth
    from transformer4sed_amd.data import write_wav
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import detect
    choice = PostprocChoice(objective="event_f1", filter_type="max", labels=LABELS, candidates=["3"] * 10, windows_units=[3, 1, 2, 5, 1, 2, 3, 7, 1, 5],
                            windows_frames=[19, 6, 12, 32, 6, 12, 19, 44, 6, 32], thresholds=[0.5, 0.4, 0.3, 0.5, 0.45, 0.5, 0.35, 0.5, 0.25, 0.5],
                            per_class=[0.0] * 10, overall=0.0)
    choice.save(tmp_path / "choice.json")
    cfg = {"training": {"median_window": [5, 20, 5, 5, 5, 20, 20, 20, 5, 20], "filter_type": "median", "weak_mask": True},
           "PaSST_SED": {"init_kwargs": {}, "val_kwargs": FAST},
           "feature": {"sr": 32000, "hopsize": 320, "win_length": 1024, "audio_max_len": 10, "net_subsample": 1}}
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    n = 12 * 32000
    wav = synth.synth_wav(2, seed=91).reshape(-1)[:n].copy()
    write_wav(str(tmp_path / "rec.wav"), wav, 32000)
    monkeypatch.setattr(detect, "load_model", lambda cfg, checkpoint, device: net)
    detect.main([str(tmp_path / "rec.wav"), "--config", str(tmp_path / "cfg.yaml"), "--out", str(tmp_path / "out"),
                 "--postprocess", str(tmp_path / "choice.json")])
    enc = EV.Encoder(LABELS, audio_len=10, frame_len=1024, frame_hop=320, net_pooling=1, sr=32000)
    det = LongFormDetector(net, enc, cfg, median_filter=choice.windows_frames, filter_type="max")
    out = det.posteriors(det.load(str(tmp_path / "rec.wav")))
    want = det.events(out, choice.thresholds)
    got = pd.read_csv(tmp_path / "out" / "events.tsv", sep="\t", float_precision="round_trip")
    print(f"12 s recording with the saved choice: {len(want)} events")
    assert got["event_label"].tolist() == want["event_label"].tolist() and (got["filename"] == "rec.wav").all()
    assert np.array_equal(got[["onset", "offset"]].to_numpy(), want[["onset", "offset"]].to_numpy())
    post = pd.read_csv(tmp_path / "out" / "scores_post" / "rec.tsv", sep="\t", float_precision="round_trip")
    assert np.array_equal(post.to_numpy(), det.tables(out, "rec")[1]["rec"].to_numpy())
    assert det.median_filter == choice.windows_frames and det.filter_type == "max" and det.weak_mask


def test_tune_tool_writes_the_choice_of_a_direct_search(net, tmp_path, monkeypatch):
    """`tools/tune_postprocess.py` on three synthetic 16 kHz files: its table and choice are those of a `PostprocSearch` fed the same
    model's posteriors of the same batch."""
    import pandas as pd
    import yaml
    from transformer4sed_amd import synth
    from transformer4sed_amd.data import WavBatchStream, write_wav
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import detect
    import tune_postprocess
    names = ["a", "b", "c"]
    gt, dur = _truth(names, seed=3)
    gt.to_csv(tmp_path / "val.tsv", sep="\t", index=False)
    dur.to_csv(tmp_path / "dur.tsv", sep="\t", index=False)
    os.makedirs(tmp_path / "wav")
    for n, x in zip(names, synth.synth_wav(3, seed=95)):
        write_wav(str(tmp_path / "wav" / (n + ".wav")), x[::2].copy(), 16000)
    config = [5, 20, 5, 5, 5, 20, 20, 20, 5, 20]
    cfg = {"training": {"median_window": config, "filter_type": "median", "weak_mask": True},
           "PaSST_SED": {"init_kwargs": {}, "val_kwargs": FAST},
           "feature": {"sr": 32000, "hopsize": 320, "win_length": 1024, "audio_max_len": 10, "net_subsample": 1}}
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    monkeypatch.setattr(detect, "load_model", lambda cfg, checkpoint, device: net)
    tune_postprocess.main(["--config", str(tmp_path / "cfg.yaml"), "--tsv", str(tmp_path / "val.tsv"), "--durations", str(tmp_path / "dur.tsv"),
                           "--wav-dir", str(tmp_path / "wav"), "--out", str(tmp_path / "out"), "--objectives", "psds1,event_f1",
                           "--thresholds", "0.3,0.5", "--windows", "2,7,20"])
    enc = EV.Encoder(LABELS, audio_len=10, frame_len=1024, frame_hop=320, net_pooling=1, sr=32000)
    search = PostprocSearch(enc, gt, dur, windows=(2, 7, 20), config_windows=config, weak_mask=True, objectives=("psds1", "event_f1"),
                            thresholds=(0.3, 0.5))
    paths = [str(tmp_path / "wav" / (n + ".wav")) for n in names]
    net.eval()
    with torch.no_grad():
        for wav, pad_mask, idx in WavBatchStream(paths, [[0, 1, 2]], DEV, encoder=enc):
            ext = net.get_feature_extractor()
            ext.eval()
            strong, weak, _ = net(ext.logmel(wav), pad_mask=pad_mask.to(DEV), **FAST)
            search.update(strong, weak, [names[i] + ".wav" for i in idx])
    for name in ("psds1", "event_f1"):
        assert PostprocChoice.load(tmp_path / "out" / f"choice_{name}.json") == search.best(name)
    best = PostprocChoice.load(tmp_path / "out" / "choice.json")
    assert best == search.best("psds1") and yaml.safe_load(open(tmp_path / "out" / "postprocess.yaml"))["training"] == best.to_config()
    table = pd.read_csv(tmp_path / "out" / "search_table.tsv", sep="\t", float_precision="round_trip")
    assert np.array_equal(table["value"].to_numpy(), search.results()["value"].to_numpy()) and len(table) == (2 * 4 + 4 * 2) * 10
