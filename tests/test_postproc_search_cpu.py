"""The post-processing search without a GPU (transformer4sed_amd/postproc_search.py): candidate bookkeeping, then
selection, the tie rule and the composition on the planted case of tests/search_cases.py with the device steps replaced by the host
references (`search_cases.host_search`: everything behind the bank, the sweep and the counting kernel is the product's), against the
literal loop of `search_cases`; the visibility of three wrong searches on the GPU tests' own inputs; and the ABI of the bank."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f1_cases as FC  # noqa: E402
import psds_cases as PC  # noqa: E402
import search_cases as SC  # noqa: E402
import transformer4sed_amd as pkg  # noqa: E402
from transformer4sed_amd import evaluation as EV, postproc_search as PS  # noqa: E402

THETAS = (0.3, 0.5, 0.7)
# the product's rates (IntersectionPSDS._class_rocs) and the literal reference's (psds_cases.psds_from_points) are the same float64
# formulas written in another order of operations: a few units in the last place of values <= 1, as in tests/test_psds_cpu.py
RATE_TOL = 1e-12


# ------------------------------------------------------------------------------------------------ candidates
def test_candidates():
    """int(u / 156 * T); units that map to one frame count are merged, the first kept; the YAML's list is the last row, "config", kept
    even where it repeats a uniform row."""
    assert PS.window_frames(PS.DEFAULT_WINDOWS, 1000) == [6, 12, 19, 32, 44, 64, 89, 128, 179]
    assert PS.window_frames([5, 20], 1000) == EV.scaled_median_window([5, 20])
    cands = PS.make_candidates((1, 1.5, 3, 3.5, 7), 160, 3, config_windows=(7, 7, 7))
    assert [(c.name, c.frames) for c in cands] == [("1", [1] * 3), ("3", [3] * 3), ("7", [7] * 3), ("config", [7] * 3)]
    assert cands[1].units == [3] * 3 and cands[3].units == [7, 7, 7]
    assert [c.name for c in PS.make_candidates((2, 1), 1000, 2)] == ["2", "1"]      # order as given
    for bad in (dict(windows=(0.5,)), dict(windows=(1, 157)), dict(windows=(1,), config_windows=(1, 2)),
                dict(windows=(1,), config_windows=(1, 0.2, 1)), dict(windows=()), dict(windows=tuple(range(1, 70)))):
        with pytest.raises(ValueError):
            PS.make_candidates(**{"T": 160, "C": 3, **bad})
    assert PS.make_candidates((157,), 160, 3, scipy=False)[0].frames == [161] * 3   # the torch-semantics median replicates the edge


def test_constructor_refusals_and_exports():
    assert pkg.PostprocSearch is PS.PostprocSearch and pkg.PostprocChoice is PS.PostprocChoice
    case = SC.planted()
    for bad in (dict(objectives=("psds3",)), dict(objectives=()), dict(filter_types=("mean",)), dict(windows=(157,)),
                dict(objectives=("event_f1",), thresholds=())):
        with pytest.raises(ValueError):
            SC.host_search(case, **bad)
    s = SC.host_search(case, windows=(157,), objectives=("event_f1",))              # beyond T is refused for the scipy modes only
    assert s.candidates[0].frames == [161] * 3
    s = SC.host_search(case, objectives=("loose",), psds_args={"loose": dict(dtc_threshold=0.5, gtc_threshold=0.5)})
    assert s.psds_objectives == ["loose"] and s._psds[("loose", "median")][0].dtc == 0.5


# ------------------------------------------------------------------------------------------------ the planted case
def _feed(search, case, weak, batches=None, order=None):
    order = list(range(len(case.names))) if order is None else order
    strong = torch.from_numpy(case.scores).transpose(1, 2).contiguous()
    weak = torch.from_numpy(weak)
    for lo, hi in batches or [(0, len(order))]:
        idx = order[lo:hi]
        search.update(strong[idx], weak[idx], [case.names[i] + ".wav" for i in idx])
    return search


@functools.lru_cache(maxsize=None)
def _planted_search():
    case = SC.planted()
    weak = SC.planted_weak(case)
    s = SC.host_search(case, windows=SC.PLANTED_WINDOWS, config_windows=SC.PLANTED_CONFIG, thresholds=THETAS,
                       objectives=("psds1", "psds2", "event_f1", "segment_f1"))
    return case, weak, _feed(s, case, weak, batches=[(0, 3), (3, 8)])


def _rows(case):
    return SC.candidate_rows(SC.PLANTED_WINDOWS, case.scores.shape[1], case.scores.shape[2], SC.PLANTED_CONFIG)


@pytest.mark.parametrize("name", ["psds1", "psds2"])
@pytest.mark.parametrize("ft", ["median", "max"])
def test_psds_table_choice_and_composition_against_the_literal_loop(name, ft):
    case, _, s = _planted_search()
    rows = _rows(case)
    ref = SC.psds_search_ref(case, rows, PC.ARG_SETS[name], ft)
    table = s.results()
    table = table[(table["objective"] == name) & (table["filter_type"] == ft)]
    assert len(table) == len(rows) * 3
    for w, (rname, frames) in enumerate(rows):
        got = table[table["candidate"] == str(rname)]
        assert got["class"].tolist() == case.classes and got["frames"].tolist() == frames and got["threshold"].isna().all()
        assert np.allclose(got["value"].to_numpy(), ref["single"][w], rtol=0, atol=RATE_TOL)
        assert abs(s.overall(name, ft)[str(rname)] - ref["overall"][w]) <= RATE_TOL
    best = s.best(name, ft)
    assert best.candidates == [str(rows[w][0]) for w in ref["choice"]] and best.windows_frames == ref["mixed"]
    assert best.thresholds is None and best.filter_type == ft and best.labels == case.classes
    assert abs(best.overall - ref["composed"]) <= RATE_TOL and ref["composed"] == ref["fresh"]
    # the product's own fresh run on the mixed windows: the same integers, the same arithmetic -> the same float
    gt, dur = PC.frames(case)
    fresh = EV.IntersectionPSDS(gt, dur, case.classes, case.ts, **EV.Evaluator.PSDS_ARGS[name])
    fresh._sweep = PC.cpu_sweep(fresh)
    fresh.update(torch.from_numpy(SC.bank_ref(case.scores, [best.windows_frames], SC.MODES[ft])[0]), case.names)
    overall, single = fresh.compute()
    assert best.overall == overall and best.per_class == [single[c] for c in case.classes]
    assert best.config_overall == s._psds[(name, ft)][-1].compute()[0]


def test_planted_conditions():
    """What the case was planted for, on psds1 with the median."""
    case, _, s = _planted_search()
    best = s.best("psds1", "median")
    values = np.asarray([v[1] for v in s._psds_values("psds1", "median")])[:-1]      # [window, class], without the config row
    assert len(set(best.windows_frames)) >= 2                                        # classes choose different windows
    tied = [c for c in range(3) if (values[:, c] == values[:, c].max()).sum() > 1]
    assert tied, "no exact tie for the order to resolve"
    for c in tied:
        assert best.windows_frames[c] == [f for f, v in zip(SC.PLANTED_WINDOWS, values[:, c]) if v == values[:, c].max()][0]
    singles = [v for k, v in s.overall("psds1", "median").items() if k != "config"]
    assert best.overall > max(singles) and best.overall > best.config_overall
    f1 = s.best("event_f1")
    assert f1.windows_frames != best.windows_frames                                  # psds1 and the event F1 disagree on a class
    assert s.best("psds1").filter_type == "median" and s.best("psds1").overall == best.overall
    print(f"psds1 / median: windows {best.windows_frames}, composed {best.overall:.4f}, best single window {max(singles):.4f}, "
          f"config {best.config_overall:.4f}; event F1 windows {f1.windows_frames} thresholds {f1.thresholds}")


@pytest.mark.parametrize("kind", ["event_f1", "segment_f1"])
def test_f1_table_choice_and_composition_against_the_literal_loop(kind):
    case, weak, s = _planted_search()
    rows = _rows(case)
    ref = SC.f1_search_ref(case, rows, THETAS, weak, kind)
    counts = s._f1_counts()
    for ti in range(len(THETAS)):
        for ci in range(len(rows)):
            assert {k: [int(v) for v in counts[ti][ci][k]] for k in FC.NAMES} == ref["counts"][ci][ti]
    table = s.results()
    table = table[table["objective"] == kind]
    assert len(table) == len(rows) * len(THETAS) * 3 and (table["filter_type"] == "median").all()
    for ci, (rname, _) in enumerate(rows):
        for ti, th in enumerate(THETAS):
            got = table[(table["candidate"] == str(rname)) & (table["threshold"] == th)]
            assert got["value"].tolist() == ref["values"][ci][ti]                    # integer counts, one division: exact
    best = s.best(kind)
    assert best.candidates == [str(rows[ci][0]) for ci, _ in ref["choice"]]
    assert best.thresholds == [THETAS[ti] for _, ti in ref["choice"]]
    want = EV.EventSegmentF1.scores(ref["composed"])
    tag = kind.replace("_f1", "")
    assert best.overall == want[tag + "_macro"] and best.overall_micro == want[tag + "_micro"]
    # a fresh accumulator on the frames decoded with the chosen per-class windows and thresholds
    active = np.stack([SC.bank_ref(case.scores, [[best.windows_frames[c]] * 3], 0,
                                   (weak >= np.float32(best.thresholds[c])).astype(np.float32))[0][:, :, c] > np.float32(best.thresholds[c])
                       for c in range(3)], axis=2)
    fresh = EV.EventSegmentF1(PC.frames(case)[0], case.classes, case.ts)
    fresh._run = FC.cpu_counts(fresh)
    fresh.update(torch.from_numpy(active), case.names)
    res = fresh.compute()
    assert best.overall == res[tag + "_macro"] and best.overall_micro == res[tag + "_micro"]
    assert best.per_class == [res["class_wise"][c][kind] for c in case.classes]


def test_batching_and_order_do_not_change_the_table():
    case, weak, s = _planted_search()
    kw = dict(windows=SC.PLANTED_WINDOWS, config_windows=SC.PLANTED_CONFIG, thresholds=THETAS, objectives=("psds1", "psds2", "event_f1"))
    want = s.results()
    want = want[want["objective"] != "segment_f1"].reset_index(drop=True)
    perm = list(np.random.RandomState(5).permutation(8))
    for batches, order in (([(0, 8)], None), ([(0, 8)], perm)):
        got = _feed(SC.host_search(case, **kw), case, weak, batches, order).results()
        assert got.equals(want)


def test_clips_outside_the_ground_truth_are_left_out_of_the_f1_counts():
    case, weak, s = _planted_search()
    t = SC.host_search(case, windows=(3, 15), objectives=("event_f1",))
    strong = torch.from_numpy(case.scores).transpose(1, 2).contiguous()
    names = [n + ".wav" for n in case.names]
    t.update(torch.cat([strong[:5], strong[2:3]]), torch.from_numpy(np.concatenate([weak[:5], weak[2:3]])), names[:5] + ["stranger.wav"])
    t.update(strong[2:3], torch.from_numpy(weak[2:3]), ["nobody.wav"])
    t.update(strong[5:], torch.from_numpy(weak[5:]), names[5:])
    u = _feed(SC.host_search(case, windows=(3, 15), objectives=("event_f1",)), case, weak)
    assert t.results().equals(u.results())


def test_choice_round_trip(tmp_path):
    _, _, s = _planted_search()
    for best in (s.best("psds1"), s.best("event_f1")):
        path = tmp_path / "choice.json"
        best.save(path)
        assert PS.PostprocChoice.load(path) == best
        assert best.to_config() == {"median_window": best.windows_units, "filter_type": best.filter_type}
        assert PS.window_frames(best.to_config()["median_window"], 160) == best.windows_frames
        assert best.to_yaml().startswith("training:\n  median_window: [")
    with pytest.raises(ValueError):
        s.best("psds1", "mean")
    with pytest.raises(ValueError):
        s.best("event_f1", "max")
    with pytest.raises(ValueError):
        s.best("psds3")


# ------------------------------------------------------------------------------------------------ the faults are visible
def test_three_wrong_searches_change_the_result_on_the_planted_case():
    """On the GPU tests' own inputs the literal reference tells apart: a search that ignores the filter type (the max table is the
    median's), one that takes the LAST candidate on ties, one that composes class c from the window chosen for class c + 1."""
    case = SC.planted()
    rows = _rows(case)[:-1]
    a = PC.ARG_SETS["psds1"]
    right = SC.psds_search_ref(case, rows, a, "median")
    right_max = SC.psds_search_ref(case, rows, a, "max")
    ignored = SC.psds_search_ref(case, rows, a, "max", ignore_filter_type=True)
    assert ignored["single"] == right["single"] and ignored["single"] != right_max["single"]
    assert max(abs(x - y) for p, q in zip(ignored["single"], right_max["single"]) for x, y in zip(p, q)) > 0.5
    last = SC.psds_search_ref(case, rows, a, "median", last_on_ties=True)
    assert last["choice"] != right["choice"] and last["mixed"] != right["mixed"]
    wrong = SC.psds_search_ref(case, rows, a, "median", wrong_class=True)
    assert wrong["choice"] == right["choice"] and abs(wrong["composed"] - right["composed"]) > 0.5
    assert right["composed"] == right["fresh"] and wrong["composed"] != wrong["fresh"]


# ------------------------------------------------------------------------------------------------ ABI
def test_bank_abi_header_library_and_build():
    from transformer4sed_amd import _lib, build
    protos = _lib.parse_header()
    args = protos["sed_median_filter_bank"]
    assert [n for _, n in args] == ["in", "out", "sizes", "scale", "B", "T", "C", "W", "mode", "max_size", "stream"]
    assert args[-1][0] is ctypes.c_void_p and [t for t, _ in args[4:10]] == [ctypes.c_int] * 6
    header = open(_lib.HEADER_PATH).read()
    proto = re.search(r"int\s+sed_median_filter_bank\s*\(([^)]*)\)\s*;", header, flags=re.S).group(1)
    assert " ".join(proto.split()).endswith("hipStream_t stream")
    assert int(re.search(r"#define\s+SED_HIP_ABI_VERSION\s+(\d+)", header).group(1)) == 7
    assert "median_filter.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "median_filter.hip"))
    dll = ctypes.CDLL(build.build(verbose=False))
    assert hasattr(dll, "sed_median_filter_bank") and dll.sed_abi_version(0) == 7
    src = open(os.path.join(build.CSRC, "median_filter.hip")).read()
    assert int(re.search(r"#define\s+FB_MAX_W\s+(\d+)", src).group(1)) == pkg.filter.FILTER_BANK_MAX_ROWS == 64
    # the dispatch the bank follows is the clip filter's by construction: one predicate over one set of constants, stated once
    core = open(os.path.join(build.CSRC, "median_select.h")).read()
    consts = [int(re.search(rf"#define\s+{n}\s+(\d+)", core).group(1)) for n in ("MEDSEL_RANK_MIN", "MEDSEL_RANK_MIN_T", "MEDSEL_MAXN")]
    assert consts == [24, 256, 2048]
    assert "mode != 2 && max_size >= MEDSEL_RANK_MIN && T >= MEDSEL_RANK_MIN_T && T + max_size + 1 <= MEDSEL_MAXN" in core
    assert src.count("if (medsel_use_ranks(mode, T, max_size))") == 2 and not re.search(r"max_size\s*>=\s*\d", src)
    assert not any(re.search(rf"#define\s+{n}\b", src) for n in ("FB_RANK_MIN", "FB_RANK_MIN_T", "FB_RANK_MAXN", "MEDR_MAXN"))


def test_filter_bank_refuses_on_the_host_first():
    from transformer4sed_amd.filter import check_bank_sizes
    assert check_bank_sizes([[1, 2], [3, 160]], 160, 2, 1) == [[1, 2], [3, 160]]
    assert check_bank_sizes([[200, 2]], 160, 2, 0) == [[200, 2]]
    for rows, mode in (([[1, 161]], 1), ([[1, 161]], 2), ([[0, 1]], 0), ([[1]], 0), ([], 1), ([[1, 1]] * 65, 1), ([[1, 1]], 3)):
        with pytest.raises(ValueError):
            check_bank_sizes(rows, 160, 2, mode)
