"""Score-level ensembling without a GPU (transformer4sed_amd/ensemble.py, csrc/ensemble.hip): the two host
restatements of tests/ensemble_cases.py against each other under the stated error model and the five wrong kernels that model catches;
the reference's `weighted_average_ensemble` (tests/golden/ensemble.npz) and the score containers with the device step replaced by the
float32 restatement; the candidate rows; the refusals; `EnsembleSearch` on host stand-ins; and the ABI of the bank."""
import copy
import ctypes
import functools
import math
import os
import re
import sys

import numpy as np
import pandas as pd
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ensemble_cases as EC  # noqa: E402
import psds_cases as PC  # noqa: E402
import transformer4sed_amd as pkg  # noqa: E402
from transformer4sed_amd import ensemble as E, evaluation as EV  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "ensemble.npz")


# ------------------------------------------------------------------------------------------------ the two restatements
@pytest.mark.parametrize("Tm,T", [(7, 10), (3, 1000), (20, 40), (10, 40), (1, 5), (40, 40), (333, 999), (250, 1000)])
def test_integer_coordinate_is_the_half_pixel_rule(Tm, T):
    """The float64 definition's resampling is `F.interpolate(size=T, mode="linear", align_corners=False)` on float64 input (which finds
    the coordinate in floating point: a few float64 roundings of values <= 1 apart)."""
    x = np.random.RandomState(Tm + T).rand(2, Tm, 3)
    ref = torch.nn.functional.interpolate(torch.from_numpy(x).transpose(1, 2), size=T, mode="linear", align_corners=False)
    assert np.abs(EC.resample64(x, T) - ref.transpose(1, 2).numpy()).max() <= 1e-12
    i0, i1, rem = EC.coords(T, Tm)
    assert i0.min() >= 0 and i1.max() <= Tm - 1 and (i1 - i0).max() <= 1 and rem.min() >= 0 and rem.max() < 2 * T
    if Tm == T:
        assert np.array_equal(i0, np.arange(T)) and not rem.any()
        assert np.array_equal(EC.resample32(x.astype(np.float32), T).view(np.int32), x.astype(np.float32).view(np.int32))


CASES = [  # (n, member lengths, T, C, W, per-class weights)
    (3, (40, 20, 10, 1), 40, 5, 7, True),
    (2, (7, 10), 10, 3, 5, False),
    (1, (3, 1000), 1000, 10, 3, True),
    (2, (16,) * 8, 16, 4, 6, True),
    (5, (13, 26), 26, 10, 4, True),           # 1300 elements: past a grid pass of 512
]


@pytest.mark.parametrize("case", CASES)
def test_float32_restatement_within_the_rounding_count_and_the_faults_are_not(case):
    """(a) against (b): at most (4 + M) roundings of 2^-24 apart (`ensemble_cases.bound`), and each of the five wrong kernels -- i1 = i0, a
    dropped member, weight rows shifted by one, per-class weights applied class-shifted, a missing last grid pass -- is far outside it."""
    n, Tms, T, C, W, per_class = case
    M = len(Tms)
    members = EC.members(n, Tms, C)
    raw = EC.weights(W, M, C if per_class else None) + 0.25            # (all positive: every member and class counts)
    w = E.normalise_weights(raw, M, C)
    assert w.dtype == np.float32 and w.shape == (W, M, C) and np.abs(w.astype(np.float64).sum(axis=1) - 1).max() <= M * EC.U
    want = EC.combine64(members, w, T)
    got = EC.combine32(members, w, T)
    err = np.abs(got - want).max()
    print(f"M = {M}: |float32 - float64| max {err:.3g}, bound {EC.bound(M):.3g}")
    assert got.dtype == np.float32 and err <= EC.bound(M)
    grid_pass = 512
    for fault in EC.FAULTS:
        if (fault == "wrong_neighbour" and all(tm in (1, T) for tm in Tms)) or (fault == "class_shift" and not per_class) \
                or (fault == "dropped_member" and M == 1) or (fault == "missing_pass" and n * T * C <= grid_pass):
            continue
        bad = np.abs(EC.combine32(members, w, T, fault=fault, grid_pass=grid_pass) - want).max()
        assert bad > 1000 * EC.bound(M), (fault, bad)
    # the rounding to 4 decimals: the float64 definition's rounding, one grid step off at most and only next to a tie
    r32 = EC.combine32(members, w, T, decimals=4).astype(np.float64)
    r64 = np.round(want, 4)
    tie = EC.near_tie(want)
    assert np.abs(r32 - r64)[~tie].max() <= EC.U and np.abs(r32 - r64).max() <= 1e-4 + EC.U


def test_every_fault_is_exercised_by_some_case():
    seen = set()
    for n, Tms, T, C, W, per_class in CASES:
        seen |= {"row_shift"} | ({"wrong_neighbour"} if any(tm not in (1, T) for tm in Tms) else set()) \
            | ({"class_shift"} if per_class else set()) | ({"dropped_member"} if len(Tms) > 1 else set()) \
            | ({"missing_pass"} if n * T * C > 512 else set())
    assert seen == set(EC.FAULTS)


def test_copy_and_broadcast_are_bit_exact():
    """T_m == T with one member at weight 1 is the input bit for bit (denormals too; alone also -0.0, which a second member's + 0 x v
    turns into +0.0); T_m == 1 broadcasts."""
    x = EC.members(2, (12,), 3)[0]
    x[0, 0, 0], x[0, 1, 0], x[1, 2, 1] = 0.0, 1e-40, 1.0
    other = EC.members(2, (6,), 3, seed=1)[0]
    w = E.normalise_weights([[1.0, 0.0]], 2, 3)
    assert np.array_equal(EC.combine32([x, other], w, 12)[0].view(np.int32), x.view(np.int32))
    x[0, 0, 0] = -0.0
    assert np.array_equal(EC.combine32([x], E.normalise_weights([2.0], 1, 3), 12)[0].view(np.int32), x.view(np.int32))
    weak = EC.members(2, (1,), 3, seed=2)[0]
    got = EC.combine32([weak], E.normalise_weights([3.0], 1, 3), 5)[0]
    assert np.array_equal(got, np.broadcast_to(weak, (2, 5, 3)))


def test_logit_mode_definition():
    """Mode 1 in float64: sigmoid of the weighted logits, the clamp at the fp32 numbers 1e-7 and 1 - 1e-7; equal members are a fixed
    point, and the geometric mean of the odds lies between the members."""
    a = EC.members(2, (8,), 3)[0]
    w = E.normalise_weights([[1.0, 3.0]], 2, 3)
    same = EC.combine64([a, a], w, 8, mode=1)[0]
    inside = (a > 1e-6) & (a < 1 - 1e-6)
    assert np.abs(same - a)[inside].max() <= 1e-12
    b = EC.members(2, (8,), 3, seed=1)[0]
    y = EC.combine64([a, b], w, 8, mode=1)[0]
    assert (y >= np.minimum(a, b) - 1e-12).all() and (y <= np.maximum(a, b) + 1e-12).all()
    ends = np.asarray([[[0.0, 1.0, 0.5]]], dtype=np.float32)
    y = EC.combine64([ends], np.ones((1, 1, 3), dtype=np.float32), 1, mode=1)[0, 0, 0]
    assert abs(y[0] - float(EC.LO)) <= 1e-15 and abs(y[1] - float(EC.HI)) <= 1e-15 and y[2] == 0.5


# ------------------------------------------------------------------------------------------------ weights and rows
def test_normalise_weights_forms():
    assert np.array_equal(E.normalise_weights([7, 3], 2, 3), np.broadcast_to(np.float32([0.7, 0.3])[None, :, None], (1, 2, 3)))
    w = E.normalise_weights([[1, 1], [1, 3]], 2, 4)
    assert w.shape == (2, 2, 4) and np.array_equal(w[1, :, 2], np.float32([0.25, 0.75]))
    w = E.normalise_weights(np.ones((3, 2, 4)) * np.arange(1, 5), 2, 4)
    assert np.array_equal(w, np.full((3, 2, 4), 0.5, dtype=np.float32))


@pytest.mark.parametrize("M,step", [(1, 0.5), (2, 0.1), (2, 0.25), (3, 0.1), (3, 0.25), (4, 0.2), (8, 0.5)])
def test_simplex_grid(M, step):
    K, grid = E.simplex_grid(M, step)
    assert K == round(1 / step) and len(grid) == math.comb(K + M - 1, M - 1) == len(set(grid))
    assert all(sum(k) == K and min(k) >= 0 and len(k) == M for k in grid)
    rows = E.make_rows(M, step)
    assert len(rows) == len(grid)                                          # the single-member rows are in the grid already
    w = np.asarray([r.weights for r in rows])
    assert np.abs(w.sum(axis=1) - 1).max() <= 1e-12 and len({tuple(np.round(r, 9)) for r in w}) == len(rows)
    for m in range(M):
        assert (w == np.eye(M)[m]).all(axis=1).sum() == 1
    assert len({r.name for r in rows}) == len(rows)


def test_rows_with_explicit_weights_and_refusals():
    assert len(E.make_rows(3, 0.1)) == 66
    rows = E.make_rows(2, 0.25, weights=[[1, 0], [0.7, 0.3], [7, 3], [2, 2]])          # equal after normalisation: left out
    assert [r.name for r in rows] == ["1/0", "0.75/0.25", "0.5/0.5", "0.25/0.75", "0/1", "0.7/0.3"]
    for bad in (dict(step=0.3), dict(step=0.0), dict(step=2.0), dict(weights=[[1, 2, 3]]), dict(weights=[1, 2]), dict(weights=[[0, 0]]),
                dict(weights=[[-1, 2]])):
        with pytest.raises(ValueError):
            E.make_rows(**{"M": 2, "step": 0.25, **bad})


# ------------------------------------------------------------------------------------------------ refusals
def test_combine_refuses():
    x = torch.rand(2, 10, 3)
    half = torch.rand(2, 5, 3)
    for members, weights, kw in (
            ([], [1.0], {}),                                                           # M outside 1 .. 8
            ([x] * 9, [1.0] * 9, {}),
            ([x, torch.rand(3, 10, 3)], [1, 1], {}),                                   # mixed n
            ([x, torch.rand(2, 10, 4)], [1, 1], {}),                                   # mixed C
            ([x, half], [1, 1], dict(T=5)),                                            # T_m > T
            ([x, half], [1, 1], dict(T=0)),
            ([x, half], [1, -1], {}),                                                  # negative weight
            ([x, half], [[1, 1], [0, 0]], {}),                                         # a row summing to 0
            ([x, half], [1, 1, 1], {}),                                                # weights for another M
            ([x, half], np.ones((2, 2, 4)), {}),                                       # per-class weights for another C
            ([x, half], np.ones((0, 2)), {}),                                          # W outside 1 .. (no row)
            ([x, half], np.ones((1, 1, 2, 3)), {}),
            ([x, half], [1, float("nan")], {}),
            ([x.double(), half.double()], [1, 1], {}),                                 # not fp32
            ([x.half(), half.half()], [1, 1], {}),
            ([x.transpose(0, 1), half], [1, 1], {}),                                   # not contiguous
            ([x[:, ::2], half], [1, 1], {}),
            ([x, torch.rand(2, 0, 3)], [1, 1], {}),
            ([x, torch.rand(2, 5)], [1, 1], {}),
            ([x, half.numpy()], [1, 1], {}),
            ([x, half], [1, 1], dict(mode="rank")),
            ([x, half], [1, 1], dict(decimals=12)),
            ([x, half], [1, 1], dict(decimals=1.5)),
            ([torch.rand(1, 2, 5000)] * 8, [1.0] * 8, {})):                            # one row beyond the weights a launch holds
        with pytest.raises(ValueError):
            E.combine(members, weights, **kw)
    with pytest.raises(NotImplementedError):                                           # valid, but on the host: there is no fallback
        E.combine([x, half], [0.7, 0.3])
    with pytest.raises(NotImplementedError):
        E.combine([x], np.ones((100, 1)), mode="logit", decimals=4)                    # (more than 64 rows is split, not refused)
    assert E.rows_per_launch(2, 10) == 64 and E.rows_per_launch(8, 33) == 64 and E.rows_per_launch(8, 100) == 40


def test_search_constructor_refuses():
    case, _, _ = EC.search_case()
    for bad in (dict(objectives=("psds3",)), dict(objectives=()), dict(filter_type="mean"), dict(mode="rank"), dict(step=0.3),
                dict(objectives=("event_f1",), thresholds=()), dict(median_window=[7, 7]), dict(median_window=[7, 0.1, 7]),
                dict(weights=[[1, 1, 1]])):
        with pytest.raises(ValueError):
            EC.host_search(case, 2, **bad)
    for M in (0, 9):
        with pytest.raises(ValueError):
            EC.host_search(case, M)
    s = EC.host_search(case, 2, step=0.5)
    t = torch.zeros(2, 3, 200)
    wk = torch.zeros(2, 3)
    for strongs, weaks in (([t], [wk]), ([t, t], [wk]), ([t, torch.zeros(2, 3, 201)], [wk, wk]), ([t, torch.zeros(2, 4, 100)], [wk, wk]),
                           ([t, t], [wk, torch.zeros(2, 4)]), ([t, torch.zeros(3, 3, 100)], [wk, wk])):
        with pytest.raises(ValueError):
            s.update(strongs, weaks, ["a.wav", "b.wav"])
    with pytest.raises(IndexError):
        s.update([t, t], [wk, wk], ["a.wav"])
    assert pkg.EnsembleSearch is E.EnsembleSearch and pkg.EnsembleChoice is E.EnsembleChoice


# ------------------------------------------------------------------------------------------------ the reference's functions
def _golden_predictions(g):
    columns = [str(c) for c in g["columns"]]
    files = [str(f) for f in g["files"]]
    models = [str(m) for m in g["models"]]
    return files, columns, {f: [(models[m], pd.DataFrame(g[f"member{m}"][j].copy(), columns=columns)) for m in range(len(models))]
                            for j, f in enumerate(files)}


def check_against_golden(weighted_average_ensemble):
    """Shared with the GPU test.  Every entry equals the reference's up to the fp32 representation of k 1e-4, except next to a rounding
    tie of the float64 definition (within 1e-6), where it may sit one grid step away; such entries are at most 4 %."""
    g = np.load(GOLDEN)
    files, columns, predictions = _golden_predictions(g)
    members = [g[f"member{m}"][:, :, 2:] for m in range(3)]
    assert [x.shape[1] for x in members] == [40, 20, 10] and members[0].shape[2] == 4 and len(files) == 3
    assert float(g["near_tie_share"]) <= 0.04
    assert abs(g["weights"][0].sum() - 1) < 1e-12 and abs(g["weights"][1].sum() - 1) > 0.5
    for k, w in enumerate(g["weights"]):
        got = weighted_average_ensemble(predictions, w)
        assert list(got) == files
        out = np.stack([got[f].values for f in files])
        assert all(list(got[f].columns) == columns for f in files) and out.dtype == np.float64
        want = g[f"out{k}"]
        assert np.array_equal(out[:, :, :2], want[:, :, :2])                           # onset / offset of the longest member
        w32 = E.normalise_weights(w, 3, 4)
        tie = EC.near_tie(EC.combine64(members, w32, 40)[0])
        assert tie.mean() <= 0.04
        diff = np.abs(out[:, :, 2:] - want[:, :, 2:])
        print(f"weights {w}: near-ties {tie.mean():.4f}, entries off the golden {int((diff > EC.U).sum())}")
        assert diff[~tie].max() <= EC.U and diff.max() <= 1e-4 + EC.U


def test_weighted_average_ensemble_against_the_reference_golden(monkeypatch):
    monkeypatch.setattr(E, "_combine_host", EC.host_combine)
    check_against_golden(E.weighted_average_ensemble)


def test_every_length_ratio_works_and_folders_round_trip(tmp_path, monkeypatch):
    """122 -> 1000 frames, where the reference's scale-factor call (floor(122 * (1000 / 122)) = 999 frames) fails; load / save / `ensemble` on folders; the
    compat re-exports."""
    monkeypatch.setattr(E, "_combine_host", EC.host_combine)
    sys.path.insert(0, os.path.join(ROOT, "transformer4sed_amd", "compat"))
    from src.postprocess import ensemble as compat_ensemble, score as compat_score
    assert compat_ensemble.weighted_average_ensemble is E.weighted_average_ensemble and compat_ensemble.ensemble is E.ensemble
    assert compat_ensemble.load_predictions is E.load_predictions and compat_ensemble.save_predictions is E.save_predictions
    assert compat_score.Score is E.Score and compat_score.ScoreContainer is E.ScoreContainer and compat_score.score_average is E.score_average
    rng = np.random.RandomState(0)
    cols = ["onset", "offset", "Cat", "Dog"]
    for name, T in (("long", 1000), ("short", 122)):
        os.makedirs(tmp_path / "in" / name)
        for f in ("a.tsv", "b.tsv"):
            t = np.round(10.0 / T * np.arange(T + 1), 6)
            pd.DataFrame(np.column_stack([t[:-1], t[1:], rng.rand(T, 2).astype(np.float32)]), columns=cols).to_csv(
                tmp_path / "in" / name / f, sep="\t", index=False)
    E.ensemble(str(tmp_path / "in"), str(tmp_path / "out"), ["short", "long"], [0.3, 0.7])
    pred = E.load_predictions([str(tmp_path / "in" / "short"), str(tmp_path / "in" / "long")])
    assert sorted(pred) == ["a.tsv", "b.tsv"] and [m for m, _ in pred["a.tsv"]] == ["short", "long"]
    for f in ("a.tsv", "b.tsv"):
        got = pd.read_csv(tmp_path / "out" / f, sep="\t")
        assert list(got.columns) == cols and len(got) == 1000
        members = [df.values[None, :, 2:].astype(np.float32) for _, df in pred[f]]
        want = np.round(EC.combine64(members, E.normalise_weights([0.3, 0.7], 2, 2), 1000)[0, 0], 4)
        tie = EC.near_tie(EC.combine64(members, E.normalise_weights([0.3, 0.7], 2, 2), 1000)[0, 0])
        diff = np.abs(got.values[:, 2:] - want)
        assert diff[~tie].max() <= EC.U and diff.max() <= 1e-4 + EC.U
        assert np.array_equal(got.values[:, :2], np.round(pred[f][1][1].values[:, :2], 4))          # the long member's times
    os.remove(tmp_path / "in" / "short" / "b.tsv")
    with pytest.raises(ValueError):
        E.load_predictions([str(tmp_path / "in" / "long"), str(tmp_path / "in" / "short")])
    with pytest.raises(ValueError):
        E.ensemble(str(tmp_path / "in"), str(tmp_path / "out2"), ["short", "long"], [1.0])


def check_score_containers():
    """Shared with the GPU test: `score_average` against a pandas restatement of src/postprocess/score.py's contracts.  The scores are
    fp32 numbers, so the only difference is the bank's arithmetic (`ensemble_cases.bound`); a class outside `reload_events` keeps the first
    container's scores exactly, and so do onset / offset."""
    events = ["Cat", "Dog", "Speech"]
    rng = np.random.RandomState(4)
    lengths = {"a": 50, "b": 50, "c": 31}

    def container():
        buf = {}
        for f, T in lengths.items():
            t = np.round(0.064 * np.arange(T + 1), 6)
            buf[f] = pd.DataFrame(np.column_stack([t[:-1], t[1:], rng.rand(T, 3).astype(np.float32)]), columns=["onset", "offset", *events])
        return E.ScoreContainer(events, buf)

    cs = [container() for _ in range(3)]
    before = copy.deepcopy(cs)
    reload_events = ["Speech", "Cat"]
    got = E.score_average(reload_events, cs)
    assert isinstance(got, E.ScoreContainer) and got.files == list(lengths) and len(got) == 3
    for f in lengths:
        want = before[0].score_dict[f].df.copy()
        for e in reload_events:
            want[e] = sum(c.score_dict[f].df[e] for c in before) / 3.0
        g = got.get_score_buffer()[f]
        assert list(g.columns) == list(want.columns) and len(g.index) == lengths[f]
        assert np.abs(g[reload_events].values - want[reload_events].values).max() <= EC.bound(3)
        assert np.array_equal(g[["onset", "offset", "Dog"]].values, want[["onset", "offset", "Dog"]].values)
        for c, b in zip(cs, before):                                                   # the inputs are left as they were
            assert c.score_dict[f].df.equals(b.score_dict[f].df)
    one = E.score_average(reload_events, cs[:1])
    assert one is not cs[0] and one.score_dict["a"].df.equals(cs[0].score_dict["a"].df)
    s = E.Score(events, before[0].score_dict["a"].df.copy())
    s.average_events(["Dog"], [before[1].score_dict["a"].df])
    want = (before[0].score_dict["a"].df["Dog"] + before[1].score_dict["a"].df["Dog"]) / 2.0
    assert np.abs(s.df["Dog"].values - want.values).max() <= EC.bound(2) and len(s) == 50
    s.reload_events(["Cat"], before[2].score_dict["a"].df)
    assert np.array_equal(s.df["Cat"].values, before[2].score_dict["a"].df["Cat"].values)
    with pytest.raises(Exception, match="misses in table"):
        s.average_events(["Bird"], [before[1].score_dict["a"].df])
    with pytest.raises(Exception, match="same length"):
        s.average_events(["Dog"], [before[1].score_dict["c"].df])
    with pytest.raises(Exception, match="Don't find event"):
        E.Score(["Bird"], before[0].score_dict["a"].df)


def test_score_average_against_a_pandas_restatement(monkeypatch):
    monkeypatch.setattr(E, "_combine_host", EC.host_combine)
    check_score_containers()


# ------------------------------------------------------------------------------------------------ the search on host stand-ins
SEARCH_KW = dict(step=0.25, objectives=("psds1", "psds2", "event_f1"), median_window=[7, 3, 7], weak_mask=True)


@functools.lru_cache(maxsize=None)
def host_search_fed():
    case, strongs, weaks = EC.search_case()
    return case, strongs, weaks, EC.feed(EC.host_search(case, 2, **SEARCH_KW), case, strongs, weaks, batches=[(0, 2), (2, 6)])


def test_search_choice_beats_every_row_per_class_and_composes_exactly():
    case, strongs, weaks, s = host_search_fed()
    assert [r.name for r in s.rows] == ["1/0", "0.75/0.25", "0.5/0.5", "0.25/0.75", "0/1"] and s.median_filter == [8, 3, 8]
    table = s.results()
    assert len(table) == 3 * 5 * 3 and set(table["objective"]) == {"psds1", "psds2", "event_f1"}
    for name in ("psds1", "psds2", "event_f1"):
        best = s.best(name)
        t = table[table["objective"] == name]
        for c, label in enumerate(case.classes):
            values = t[t["class"] == label]["value"].to_numpy()
            assert best.per_class[c] == values.max()                                   # at least as good as every single row
            first = t[(t["class"] == label) & (t["value"] == values.max())]["row"].iloc[0]
            assert best.rows[c] == first                                               # the first row on ties
            assert best.weights[c] == s.normalised([r.name for r in s.rows].index(first))
        assert best.member_overall == [s.overall(name)["1/0"], s.overall(name)["0/1"]] and best.mode == "mean"
    best = s.best("psds1")
    assert len(set(best.rows)) >= 2 and best.overall > max(s.overall("psds1").values())        # classes differ: the mix beats every row
    # an accumulator fed the chosen per-class mix directly: the same integers, the same arithmetic -> the same float
    for name in ("psds1", "psds2"):
        best = s.best(name)
        cfg = best.to_config()
        assert np.asarray(cfg["weights"]).shape == (1, 2, 3) and cfg["mode"] == "mean"
        views = [np.ascontiguousarray(x.transpose(0, 2, 1)) for x in strongs]
        strong = torch.from_numpy(EC.host_combine(views, cfg["weights"], 200, "mean", None)[0]).transpose(1, 2)
        weak = torch.from_numpy(EC.host_combine([w[:, None, :] for w in weaks], cfg["weights"], 1, "mean", None)[0, :, 0])
        fresh = s._psds_accumulator(case.ts, EV.Evaluator.PSDS_ARGS[name])
        fresh.update(s._scores(strong, weak), case.names)
        overall, single = fresh.compute()
        assert best.overall == overall and best.per_class == [single[c] for c in case.classes]


def test_search_batching_does_not_change_the_table():
    case, strongs, weaks, s = host_search_fed()
    once = EC.feed(EC.host_search(case, 2, **SEARCH_KW), case, strongs, weaks)
    assert once.results().equals(s.results()) and once.best("psds1") == s.best("psds1")


def test_single_member_row_is_that_member_alone():
    """`weights=[[1, 0]]` (already in the grid: not added twice) reproduces member 0's PSDS exactly: T_m == T at weight 1 is a copy."""
    case, strongs, weaks, _ = host_search_fed()
    kw = dict(SEARCH_KW, objectives=("psds1", "psds2"), step=1.0, weights=[[1, 0]])
    s = EC.feed(EC.host_search(case, 2, **kw), case, strongs, weaks)
    assert [r.name for r in s.rows] == ["1/0", "0/1"]
    for name in ("psds1", "psds2"):
        alone = s._psds_accumulator(case.ts, EV.Evaluator.PSDS_ARGS[name])
        alone.update(s._scores(torch.from_numpy(strongs[0]), torch.from_numpy(weaks[0])), case.names)
        assert s.overall(name)["1/0"] == alone.compute()[0]
        got = s.results()
        got = got[(got["objective"] == name) & (got["row"] == "1/0")]["value"].tolist()
        assert got == [alone.compute()[1][c] for c in case.classes]


def test_choice_round_trip(tmp_path):
    _, _, _, s = host_search_fed()
    for name in ("psds1", "event_f1"):
        best = s.best(name)
        best.save(tmp_path / "choice.json")
        assert E.EnsembleChoice.load(tmp_path / "choice.json") == best
        assert (best.thresholds is None) == (name == "psds1")
    with pytest.raises(ValueError):
        s.best("segment_f1")
    with pytest.raises(ValueError):
        s.overall("psds3")


# ------------------------------------------------------------------------------------------------ ABI
def test_bank_abi_header_library_and_build():
    from transformer4sed_amd import _lib, build
    args = _lib.parse_header()["sed_ensemble_bank"]
    assert [n for _, n in args] == ["members", "Tm", "w", "out", "M", "W", "n", "T", "C", "mode", "decimals", "stream"]
    assert [t for t, _ in args[:4]] == [ctypes.c_void_p] * 4 and [t for t, _ in args[4:11]] == [ctypes.c_int] * 7
    header = open(_lib.HEADER_PATH).read()
    proto = re.search(r"int\s+sed_ensemble_bank\s*\(([^)]*)\)\s*;", header, flags=re.S).group(1)
    assert " ".join(proto.split()).endswith("hipStream_t stream")
    assert int(re.search(r"#define\s+SED_HIP_ABI_VERSION\s+(\d+)", header).group(1)) == 7
    assert "ensemble.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "ensemble.hip"))
    assert "-ffp-contract=off" in build.FILE_FLAGS["ensemble.hip"] and "-ffast-math" not in build.FILE_FLAGS["ensemble.hip"]
    dll = ctypes.CDLL(build.build(verbose=False))
    assert hasattr(dll, "sed_ensemble_bank") and dll.sed_abi_version(0) == 7
    src = open(os.path.join(build.CSRC, "ensemble.hip")).read()

    def const(name):
        return int(re.search(rf"#define\s+{name}\s+(\d+)", src).group(1))

    assert (const("ENS_MAX_M"), const("ENS_MAX_W"), const("ENS_THREADS"), const("ENS_MAX_GRID"), const("ENS_MAX_WEIGHTS")) \
        == (E.MAX_MEMBERS, E.MAX_ROWS, E.GRID_THREADS, E.MAX_GRID, E.MAX_WEIGHTS) == (8, 64, 256, 1024, 32768)
    assert E.GRID_PASS == 1024 * 256
