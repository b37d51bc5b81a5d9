"""Score-level ensembling on the device (csrc/ensemble.hip, transformer4sed_amd/ensemble.py): mode 0 bit for bit against
the float32 restatement of tests/ensemble_cases.py, mode 1 against the float64 definition, the reference's functions against
tests/golden/ensemble.npz, `EnsembleSearch` against the same search on host stand-ins, and tools/ensemble.py in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda"

import ensemble_cases as EC  # noqa: E402
import psds_cases as PC  # noqa: E402
import search_cases as SC  # noqa: E402
from transformer4sed_amd import ensemble as E  # noqa: E402
from transformer4sed_amd._lib import SedHipError  # noqa: E402
from transformer4sed_amd.ops import call, h2d  # noqa: E402

GUARD = 256
# Mode 1 against the float64 definition on `ensemble_cases.mode1_fixture`, measured on an MI355X (profiles/ensemble_timing.txt): the kernel computes in
# float64 and rounds to fp32 once, so the figure is half an ulp of a value in [0.5, 1).  The test asserts 4 x this and the ceiling below.
MODE1_MEASURED = 2.98e-8
MODE1_CEILING = 1e-5            # a tenth of the score tables' 4-decimal grid: above it the mode is wrong, not imprecise


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _launch(members, w, T, mode=0, decimals=None):
    """One raw launch into a sentinel-filled buffer -> out [W, n, T, C]; asserts that nothing was written before or behind it."""
    xs = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV) for x in members]
    W, M, C = w.shape
    n = xs[0].shape[0]
    size = W * n * T * C
    buf = torch.full((size + 2 * GUARD,), float(EC.SENTINEL), dtype=torch.float32, device=DEV)
    table = h2d([x.data_ptr() for x in xs], torch.int64, xs[0].device)
    tms = h2d([x.shape[1] for x in xs], torch.int32, xs[0].device)
    call("sed_ensemble_bank", table, tms, torch.from_numpy(w).to(DEV), buf[GUARD:GUARD + size], M, W, n, T, C, mode,
         -1 if decimals is None else decimals)
    got = buf.cpu().numpy()
    assert np.all(got[:GUARD] == EC.SENTINEL) and np.all(got[GUARD + size:] == EC.SENTINEL)
    return got[GUARD:GUARD + size].reshape(W, n, T, C)


LENGTHS = {  # T -> member lengths by M: T, T/2, T/4, 1 and lengths that are no divisor of T, mixed inside one call
    40: {1: (20,), 2: (40, 10), 8: (40, 20, 10, 1, 28, 40, 13, 5)},
    10: {1: (7,), 2: (7, 10), 8: (7, 10, 5, 1, 3, 9, 2, 10)},
    1000: {1: (3,), 2: (3, 1000), 8: (3, 1000, 500, 250, 1, 999, 333, 7)},
}


def _weights(form, W, M, C):
    if form == "M":
        return E.normalise_weights(EC.weights(1, M, rows_only=True), M, C)
    return E.normalise_weights(EC.weights(W, M, C if form == "WMC" else None, seed=C), M, C)


@pytest.mark.parametrize("M", [1, 2, 8])
@pytest.mark.parametrize("T", [40, 10, 1000])
def test_mode0_is_the_float32_restatement_bit_for_bit(T, M):
    n = 3 if T < 1000 else 1
    for C in (1, 3, 10, 33):
        members = EC.members(n, LENGTHS[T][M], C, seed=M)
        for form, W in (("M", 1), ("WM", 5), ("WMC", 5), ("WMC", 64), ("WM", 1)):
            w = _weights(form, W, M, C)
            for decimals in (None, 4):
                got = _launch(members, w, T, 0, decimals)
                want = EC.combine32(members, w, T, 0, decimals)
                assert np.array_equal(_bits(got), _bits(want)), (C, form, W, decimals, float(np.abs(got - want).max()))
    again = _launch(members, w, T, 0, decimals)
    assert np.array_equal(_bits(got), _bits(again))


@pytest.mark.parametrize("shape", [(1, 4161, 63), (2, 1024, 128), (1, 52429, 5), (3, 1024, 128)])
def test_mode0_around_one_grid_pass(shape):
    """n T C one below, at, one above one pass of the grid-stride loop (`ensemble.GRID_PASS`), and a pass and a half."""
    n, T, C = shape
    N = n * T * C
    assert N - E.GRID_PASS in (-1, 0, 1, E.GRID_PASS // 2) and E.GRID_PASS == E.MAX_GRID * E.GRID_THREADS
    members = EC.members(n, (T, max(T // 4, 1)), C)
    w = E.normalise_weights(EC.weights(2, 2, C) + 0.25, 2, C)
    got = _launch(members, w, T)
    want = EC.combine32(members, w, T)
    assert np.array_equal(_bits(got), _bits(want))
    if N > E.GRID_PASS:          # what a kernel without its second pass would leave behind is not what is there
        missing = EC.combine32(members, w, T, fault="missing_pass", grid_pass=E.GRID_PASS)
        assert not np.array_equal(_bits(got), _bits(missing))


def test_copy_and_broadcast_bit_for_bit():
    """T_m == T with one member at weight 1 is the input bit for bit, whatever the other member holds; T_m == 1 is a broadcast."""
    x = EC.members(2, (50,), 10)[0]
    x[0, 0, 0], x[0, 1, 0], x[1, 2, 1] = 0.0, 1e-40, 1.0
    other = EC.members(2, (25,), 10, seed=1)[0]
    got = _launch([x, other], E.normalise_weights([[1.0, 0.0], [0.0, 1.0]], 2, 10), 50)
    assert np.array_equal(_bits(got[0]), _bits(x))
    assert np.array_equal(_bits(got[1]), _bits(EC.resample32(other, 50)))
    x[0, 0, 0] = -0.0
    assert np.array_equal(_bits(_launch([x], E.normalise_weights([2.0], 1, 10), 50)[0]), _bits(x))
    weak = EC.members(4, (1,), 10, seed=2)[0]
    assert np.array_equal(_launch([weak], E.normalise_weights([1.0], 1, 10), 7)[0], np.broadcast_to(weak, (4, 7, 10)))


def test_combine_wrapper_forms_split_and_refusals():
    members = EC.members(3, (40, 20, 1), 10)
    xs = [torch.from_numpy(x).to(DEV) for x in members]
    for raw in (EC.weights(1, 3, rows_only=True), EC.weights(5, 3), EC.weights(5, 3, 10), EC.weights(130, 3) + 0.5):
        for decimals in (None, 4):
            got = E.combine(xs, raw, decimals=decimals)
            want = EC.combine32(members, E.normalise_weights(raw, 3, 10), 40, 0, decimals)
            assert got.shape == want.shape and np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    got = E.combine(xs[1:], [1, 1], T=60)                                              # an output size above every member
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(EC.combine32(members[1:], E.normalise_weights([1, 1], 2, 10), 60)))
    with pytest.raises(ValueError):
        E.combine(xs, [1, 1, 1], T=30)
    with pytest.raises(ValueError):
        E.combine([xs[0], xs[1].double()], [1, 1])
    with pytest.raises(ValueError):
        E.combine([xs[0].transpose(0, 1)], [1])
    with pytest.raises(NotImplementedError):
        E.combine([xs[0], torch.from_numpy(members[1])], [1, 1])


def test_bad_arguments_write_nothing():
    x = torch.from_numpy(EC.members(2, (10,), 3)[0]).to(DEV)
    table = h2d([x.data_ptr()] * 9, torch.int64, x.device)
    tms = h2d([10] * 9, torch.int32, x.device)
    w = torch.full((65 * 9 * 3,), 1.0 / 9, dtype=torch.float32, device=DEV)
    for M, W, n, T, C, mode, dec in ((0, 1, 2, 10, 3, 0, -1), (9, 1, 2, 10, 3, 0, -1), (1, 0, 2, 10, 3, 0, -1), (1, 65, 2, 10, 3, 0, -1),
                                     (1, 1, 0, 10, 3, 0, -1), (1, 1, 2, 0, 3, 0, -1), (1, 1, 2, 10, 0, 0, -1), (1, 1, 2, 10, 3, 2, -1),
                                     (1, 1, 2, 10, 3, 0, -2), (1, 1, 2, 10, 3, 0, 10), (8, 64, 2, 10, 65, 0, -1)):
        buf = torch.full((4096,), float(EC.SENTINEL), dtype=torch.float32, device=DEV)
        with pytest.raises(SedHipError):
            call("sed_ensemble_bank", table, tms, w, buf, M, W, n, T, C, mode, dec)
        assert bool((buf == float(EC.SENTINEL)).all())


# ------------------------------------------------------------------------------------------------ mode 1
def test_mode1_against_the_float64_definition():
    members, w, raw = EC.mode1_fixture()
    got = _launch(members, w, 40, 1)
    want = EC.combine64(members, w, 40, 1)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"mode 1: max |device - float64 definition| = {err:.3e} (asserted: {4 * MODE1_MEASURED:.3e} and {MODE1_CEILING:.0e})")
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0
    assert err <= 4 * MODE1_MEASURED and err <= MODE1_CEILING
    mean = EC.combine64(members, w, 40, 0)
    assert np.abs(want - mean).max() > 1000 * MODE1_CEILING                            # (the bound tells the two modes apart)
    r = _launch(members, w, 40, 1, 4).astype(np.float64)
    tie = EC.near_tie(want)
    assert np.abs(r - np.round(want, 4))[~tie].max() <= EC.U and np.abs(r - np.round(want, 4)).max() <= 1e-4 + EC.U
    xs = [torch.from_numpy(x).to(DEV) for x in members]
    assert np.array_equal(_bits(E.combine(xs, raw, mode="logit").cpu().numpy()), _bits(got))


# ------------------------------------------------------------------------------------------------ the reference's functions
def test_reference_functions_against_the_golden_and_the_contracts():
    from test_ensemble_cpu import check_against_golden, check_score_containers
    check_against_golden(E.weighted_average_ensemble)
    check_score_containers()


# ------------------------------------------------------------------------------------------------ the search
SEARCH_KW = dict(step=0.25, objectives=("psds1", "psds2", "event_f1"), median_window=[7, 3, 7], weak_mask=True)


@pytest.fixture(scope="module")
def searched():
    case, strongs, weaks = EC.search_case()
    gt, dur = PC.frames(case)
    dev = EC.feed(E.EnsembleSearch(SC.planted_encoder(case), gt, dur, 2, **SEARCH_KW), case, strongs, weaks, batches=[(0, 2), (2, 6)],
                  dev=DEV)
    return case, strongs, weaks, dev


def test_device_search_equals_the_host_search(searched):
    """2 members of 200 and 100 frames fed straight from their [n, C, T_m] tensors, step 0.25, 6 clips, 3 classes: the bank is bit-exact
    and the accumulators are integer-exact, so the tables and the choices are equal, not close."""
    case, strongs, weaks, dev = searched
    host = EC.feed(EC.host_search(case, 2, **SEARCH_KW), case, strongs, weaks)
    got, want = dev.results(), host.results()
    assert len(got) == 3 * 5 * 3 and got.equals(want)
    for name in SEARCH_KW["objectives"]:
        assert dev.best(name) == host.best(name), name
        assert dev.overall(name) == host.overall(name)
    best = dev.best("psds1")
    assert len(set(best.rows)) >= 2 and best.overall > max(dev.overall("psds1").values())


def test_logit_search_runs_and_single_rows_agree_with_the_mean_search(searched):
    """The single-member rows do not depend on the mode where the member is copied (member 0: T_m == T)."""
    case, strongs, weaks, dev = searched
    gt, dur = PC.frames(case)
    kw = dict(SEARCH_KW, objectives=("psds1",), mode="logit", median_window=None, weak_mask=False)
    logit = EC.feed(E.EnsembleSearch(SC.planted_encoder(case), gt, dur, 2, **kw), case, strongs, weaks, dev=DEV)
    mean = EC.feed(E.EnsembleSearch(SC.planted_encoder(case), gt, dur, 2, **dict(kw, mode="mean")), case, strongs, weaks, dev=DEV)
    assert np.isfinite(logit.results()["value"].to_numpy()).all() and logit.best("psds1").mode == "logit"
    assert abs(logit.overall("psds1")["1/0"] - mean.overall("psds1")["1/0"]) <= 1e-12


# ------------------------------------------------------------------------------------------------ the tool
def test_tool_combine_then_search_in_a_child_process(tmp_path, searched):
    import yaml
    case, strongs, weaks, _ = searched
    dirs = EC.write_score_folders(str(tmp_path / "scores"), case, strongs)
    tool = os.path.join(ROOT, "tools", "ensemble.py")
    run = subprocess.run([sys.executable, tool, "combine", *dirs, "--weights", "0.7,0.3", "--out", str(tmp_path / "combined")],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    want = E.weighted_average_ensemble(E.load_predictions(dirs), [0.7, 0.3])
    assert sorted(os.listdir(tmp_path / "combined")) == sorted(want) and len(want) == 6
    for f, df in want.items():
        got = pd.read_csv(tmp_path / "combined" / f, sep="\t")
        assert list(got.columns) == list(df.columns) and len(got) == 200 and np.array_equal(got.values, df.values)
    gt, dur = PC.frames(case)
    gt.to_csv(tmp_path / "val.tsv", sep="\t", index=False)
    dur.to_csv(tmp_path / "dur.tsv", sep="\t", index=False)
    cfg = {"training": {"median_window": [7, 3, 7], "filter_type": "median"},
           "feature": {"sr": 16000, "hopsize": 800, "win_length": 1600, "audio_max_len": 10, "net_subsample": 1}}
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    run = subprocess.run([sys.executable, tool, "search", *dirs, "--ground-truth", str(tmp_path / "val.tsv"), "--durations",
                          str(tmp_path / "dur.tsv"), "--config", str(tmp_path / "cfg.yaml"), "--out", str(tmp_path / "choice.json"),
                          "--step", "0.25", "--objectives", "psds1,event_f1", "--batch-size", "4"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    # the same search in this process, from the same tables
    pred = E.load_predictions(dirs)
    search = E.EnsembleSearch(SC.planted_encoder(case), gt, dur, 2, step=0.25, objectives=("psds1", "event_f1"), median_window=[7, 3, 7])
    xs = [torch.from_numpy(np.stack([pred[f][m][1].values[:, 2:].astype(np.float32).T for f in pred])).to(DEV) for m in range(2)]
    search.update(xs, [x.amax(dim=2) for x in xs], [os.path.splitext(f)[0] + ".wav" for f in pred])
    assert E.EnsembleChoice.load(tmp_path / "choice.json") == search.best("psds1")
    assert E.EnsembleChoice.load(tmp_path / "choice_event_f1.json") == search.best("event_f1")
    table = pd.read_csv(tmp_path / "choice_table.tsv", sep="\t", float_precision="round_trip")
    assert np.array_equal(table["value"].to_numpy(), search.results()["value"].to_numpy())
    assert json.load(open(tmp_path / "choice.json"))["labels"] == case.classes
