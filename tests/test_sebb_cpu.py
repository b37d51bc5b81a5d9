"""Sound event bounding boxes without a GPU (transformer4sed_amd/sebb.py): the two host statements of the
definition in tests/sebb_cases.py against each other bit for bit and against rows whose answer is known by hand, the invariants of the
output, the ABI of the bank, `SebbSearch` with the device steps replaced by the host references against a brute force over them, and
what the host refuses."""
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
import sebb_cases as BC  # noqa: E402
import transformer4sed_amd as pkg  # noqa: E402
from transformer4sed_amd import evaluation as EV, sebb as SB  # noqa: E402

Q = BC.Q
THETAS = (0.3, 0.5, 0.7)
RATE_TOL = 1e-12          # as in tests/test_postproc_search_cpu.py: the same float64 formulas in another order of operations


def _both(y, L, tau, rho):
    """Both references on one row, equal bit for bit -> (boxes, conf, scores)."""
    a, b = BC.row_loop(y, L, tau, rho), BC.row_numpy(y, L, tau, rho)
    assert a[0] == b[0], (a[0], b[0])
    assert [np.float32(c).view(np.int32) for c in a[1]] == [np.float32(c).view(np.int32) for c in b[1]]
    assert np.array_equal(a[2].view(np.int32), b[2].view(np.int32))
    return a


def _invariants(y, boxes, conf, scores):
    T = len(y)
    q = BC.quantise(y)
    prev = -1
    want = np.zeros(T, dtype=np.float32)
    for (a, b), c in zip(boxes, conf):
        assert 0 <= a < b <= T and a > prev                       # sorted, disjoint, at least one frame apart
        prev = b
        assert np.float32(c) == np.float32(np.float64(int(q[a:b].sum())) / np.float64((b - a) << 24))
        want[a:b] = c
    assert np.array_equal(scores.view(np.int32), want.view(np.int32))


# ------------------------------------------------------------------------------------------------ the two references
@pytest.mark.parametrize("T", [1, 2, 3, 17, 64, 161])
@pytest.mark.parametrize("kind", ["smooth", "grid"])
def test_the_two_references_agree_and_keep_the_invariants(T, kind):
    x = (BC.smooth if kind == "smooth" else BC.grid)(3, T, 2, seed=T)
    n_boxes = 0
    for L in (1, 2, 5, 25, T, T + 7):
        for tau, rho in ((0.2, 2.0), (0.0, 1.0), (1.0, 16.0), (0.05, 1.25)):
            for b in range(3):
                for c in range(2):
                    boxes, conf, scores = _both(x[b, :, c], L, tau, rho)
                    _invariants(x[b, :, c], boxes, conf, scores)
                    n_boxes += len(boxes)
    assert n_boxes > 0


def test_half_to_even_quantisation():
    y = np.asarray([0.5 * 2.0 ** -24, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 1.0, 0.0], dtype=np.float32)
    assert BC.quantise(y).tolist() == [0, 2, 2, Q, 0]
    assert BC.quantise_params(0.2, 1.5) == (int(np.rint(0.2 * Q)), 384)


# ------------------------------------------------------------------------------------------------ answers known by hand
@pytest.mark.parametrize("T", [1, 2, 9, 40])
@pytest.mark.parametrize("L", [1, 3, 40, 100])
def test_all_zeros_and_all_ones(T, L):
    assert _both(np.zeros(T, dtype=np.float32), L, 0.2, 2.0)[0] == []
    boxes, conf, scores = _both(np.ones(T, dtype=np.float32), L, 0.2, 2.0)
    assert boxes == [(0, T)] and conf == [np.float32(1.0)] and (scores == 1).all()


@pytest.mark.parametrize("L", [1, 2, 5, 12, 64])
@pytest.mark.parametrize("a,b", [(10, 20), (0, 7), (33, 40), (0, 40), (5, 6), (39, 40), (0, 1)])
def test_one_plateau_gives_its_exact_bounds(L, a, b):
    """Also the event touching frame 0 and the one touching T (T = 40).  A plateau of n >= L frames comes out as [a, b) with its own
    level.  With n < L the forward window holds the whole plateau from boundary a - (L - n) on, D is flat from there to a, and the
    earliest of the equal maxima is the onset (the mirror rule keeps the offset at b: there the earliest is b itself)."""
    n = b - a
    onset = a if L <= n else max(0, a - (L - n))
    for high in (1.0, 0.625):
        boxes, conf, scores = _both(BC.plateau(40, a, b, high), L, 0.2, 2.0)
        want = np.float32(np.float64(n * int(high * Q)) / np.float64((b - onset) << 24))
        assert boxes == [(onset, b)] and conf == [want]
        assert (scores[onset:b] == want).all() and not scores[:onset].any() and not scores[b:].any()


def _two_events(l_q, g_q, k_q, n_e=4, n_g=3, n_k=5):
    """0 0 | E: n_e frames at l_q | gap: n_g at g_q | K: n_k at k_q | 0 0, levels as integer multiples of 2^-24 (exact in fp32)."""
    q = [0, 0] + [l_q] * n_e + [g_q] * n_g + [k_q] * n_k + [0, 0]
    return (np.asarray(q, dtype=np.float64) / Q).astype(np.float32), 2, 2 + n_e, 2 + n_e + n_g, 2 + n_e + n_g + n_k


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_the_absolute_merge_inequality_one_unit_to_either_side_of_equality(d):
    """With L = 1 the candidates are the two plateaus.  lo = E (mean 1/2 < 3/4); mean(G) > mean(lo) - tau is, in integers,
    g_q + tau_q > l_q: with tau_q = 2^22 equality sits at g_q = 2^22, which does not merge; one unit above merges."""
    l_q, k_q, tau_q = 1 << 23, 3 << 22, 1 << 22
    y, a1, b1, a2, b2 = _two_events(l_q, l_q - tau_q + d, k_q)
    boxes, conf, _ = _both(y, 1, tau_q / Q, 16.0)                  # (rho = 16: the relative inequality holds by far)
    if d <= 0:
        assert boxes == [(a1, b1), (a2, b2)] and conf == [np.float32(0.5), np.float32(0.75)]
    else:
        assert boxes == [(a1, b2)]
        assert conf == [np.float32(np.float64(4 * l_q + 3 * (l_q - tau_q + 1) + 5 * k_q) / np.float64(12 << 24))]


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_the_relative_merge_inequality_one_unit_to_either_side_of_equality(d):
    """rho mean(G) > mean(lo) is rho_q g_q > 256 l_q: with rho = 2 equality sits at g_q = l_q / 2."""
    l_q, k_q = 1 << 23, 3 << 22
    y, a1, b1, a2, b2 = _two_events(l_q, (l_q >> 1) + d, k_q)
    boxes, _, _ = _both(y, 1, 1.0, 2.0)                             # (tau = 1: the absolute inequality holds by far)
    assert boxes == ([(a1, b1), (a2, b2)] if d <= 0 else [(a1, b2)])


def test_lo_is_the_later_event_when_its_mean_is_smaller():
    """E at 3/4, K at 1/2: lo = K.  With tau_q = 2^22 the gap merges from g_q = 2^22 + 1 on, whichever side holds the smaller mean."""
    l_q, k_q, tau_q = 3 << 22, 1 << 23, 1 << 22
    for d, merged in ((0, False), (1, True)):
        y, a1, b1, a2, b2 = _two_events(l_q, k_q - tau_q + d, k_q)
        assert _both(y, 1, tau_q / Q, 16.0)[0] == ([(a1, b2)] if merged else [(a1, b1), (a2, b2)])


def test_rho_one_and_tau_zero_never_merge_across_a_lower_gap():
    """rho = 1 asks mean(G) > mean(lo), tau = 0 the same: a gap below both events stays a gap whatever the other parameter is."""
    y, a1, b1, a2, b2 = _two_events(1 << 23, (1 << 23) - 1, 3 << 22)
    for tau, rho in ((1.0, 1.0), (0.0, 16.0), (0.0, 1.0)):
        assert _both(y, 1, tau, rho)[0] == [(a1, b1), (a2, b2)]
    assert _both(y, 1, 1.0, 16.0)[0] == [(a1, b2)]


def test_a_chain_of_merges_carries_the_merged_sum():
    """Three events: E and K merge, then the merged box (its sum covers the gap) is compared with the third."""
    q = [0] + [1 << 23] * 3 + [1 << 22] * 2 + [1 << 23] * 3 + [1 << 20] * 4 + [1 << 23] * 2 + [0]
    y = (np.asarray(q, dtype=np.float64) / Q).astype(np.float32)
    boxes, conf, _ = _both(y, 1, 0.3, 4.0)
    assert boxes == [(1, 9), (13, 15)]
    assert conf[0] == np.float32(np.float64(6 * (1 << 23) + 2 * (1 << 22)) / np.float64(8 << 24))


def test_equal_maxima_in_D_the_earliest_wins():
    """L = 1: D[t] = q[t] - q[t-1].  0 .5 1 1 1 0 0 has D = 0 .5 .5 0 0 -1 0 0: the onset is boundary 1, not 2.  Mirrored, 1 1 .5 0 0 has
    D = 1 0 -.5 -.5 0 0: the offset is boundary 2, not 3."""
    boxes, conf, _ = _both(np.asarray([0, .5, 1, 1, 1, 0, 0], dtype=np.float32), 1, 0.2, 2.0)
    assert boxes == [(1, 5)] and conf == [np.float32(0.875)]
    boxes, conf, _ = _both(np.asarray([1, 1, .5, 0, 0], dtype=np.float32), 1, 0.2, 2.0)
    assert boxes == [(0, 2)] and conf == [np.float32(1.0)]


def test_T_one():
    for v in (0.0, 2.0 ** -24, 0.3, 1.0):
        boxes, conf, scores = _both(np.asarray([v], dtype=np.float32), 1, 0.2, 2.0)
        assert boxes == ([(0, 1)] if v > 0 else []) and scores.tolist() == [np.float32(v)]


def test_bank_ref_applies_the_scale_and_the_per_class_parameters():
    x = BC.smooth(2, 50, 3, seed=5)
    scale = np.asarray([[1.0, 0.5, 0.0], [0.25, 1.0, 0.75]], dtype=np.float32)
    rows = [([2, 5, 9], [0.1, 0.2, 0.3], [1.5, 2.0, 3.0]), BC.uniform_row(3, 5, 0.2, 2.0)]
    scores, boxes = BC.bank_ref(x, rows, scale)
    for k, (Ls, taus, rhos) in enumerate(rows):
        for b in range(2):
            for c in range(3):
                bx, cf, sc = BC.row_loop(x[b, :, c] * scale[b, c], Ls[c], taus[c], rhos[c])
                assert boxes[(k, b, c)][0] == bx and np.array_equal(scores[k, b, :, c], sc)
    assert not scores[:, 0, :, 2].any()


# ------------------------------------------------------------------------------------------------ ABI
def test_sebb_abi_header_library_and_build():
    from transformer4sed_amd import _lib, build
    args = _lib.parse_header()["sed_sebb_bank"]
    assert [n for _, n in args] == ["in", "scale", "params", "out", "boxes", "conf", "counts", "status", "B", "T", "C", "K", "cap", "stream"]
    assert [t for t, _ in args[:8]] == [ctypes.c_void_p] * 8 and [t for t, _ in args[8:13]] == [ctypes.c_int] * 5
    header = open(_lib.HEADER_PATH).read()
    proto = re.search(r"int\s+sed_sebb_bank\s*\(([^)]*)\)\s*;", header, flags=re.S).group(1)
    src = open(os.path.join(build.CSRC, "sebb.hip")).read()
    defn = re.search(r'extern "C" int\s+sed_sebb_bank\s*\(([^)]*)\)', src, flags=re.S).group(1)
    assert " ".join(proto.split()) == " ".join(defn.split())
    assert int(re.search(r"#define\s+SED_HIP_ABI_VERSION\s+(\d+)", header).group(1)) == 7
    assert "sebb.hip" in build.SOURCES
    dll = ctypes.CDLL(build.build(verbose=False))
    assert hasattr(dll, "sed_sebb_bank") and dll.sed_abi_version(0) == 7
    assert int(re.search(r"#define\s+SEBB_MAX_K\s+(\d+)", src).group(1)) == SB.SEBB_MAX_ROWS == 64
    assert int(re.search(r"#define\s+SEBB_MAX_T\s+(\d+)", src).group(1)) == SB.SEBB_MAX_FRAMES == 1024
    assert SB.Q == Q and "16777216.0f" in src and SB.RHO_Q == 256


# ------------------------------------------------------------------------------------------------ refusals, parameters
def test_refusals_come_from_the_host_before_any_launch():
    x = torch.rand(2, 30, 3)
    row = BC.uniform_row(3, 5, 0.2, 2.0)
    bad_rows = [[], [row] * 65, [([5, 5], [0.2] * 3, [2.0] * 3)], [([5] * 3, [0.2] * 2, [2.0] * 3)], [([5] * 3, [0.2] * 3, [2.0] * 4)],
                [([5, 0, 5], [0.2] * 3, [2.0] * 3)], [([5, 2.5, 5], [0.2] * 3, [2.0] * 3)], [([5] * 3, [0.2] * 3, [2.0, 0.99, 2.0])],
                [([5] * 3, [0.2] * 3, [2.0, 17.0, 2.0])], [([5] * 3, [-0.1, 0.2, 0.2], [2.0] * 3)], [([5] * 3, [0.2, 1.5, 0.2], [2.0] * 3)],
                [([5] * 3, [0.2] * 3)]]
    for rows in bad_rows:
        with pytest.raises(ValueError):
            SB.sebb_bank(x, rows)
    with pytest.raises(ValueError, match="1024"):
        SB.sebb_bank(torch.rand(1, 1025, 3), [row])
    with pytest.raises(ValueError):
        SB.sebb_bank(torch.rand(30, 3), [row])
    for v in (float("nan"), -0.01, 1.5, float("inf")):
        y = x.clone()
        y[1, 7, 2] = v
        with pytest.raises(ValueError, match="NaN"):
            SB.sebb_bank(y, [row])
        w = torch.ones(2, 3)
        w[0, 1] = v
        with pytest.raises(ValueError, match="NaN"):
            SB.sebb_bank(x, [row], w)
    with pytest.raises(ValueError):
        SB.sebb_bank(x, [row], torch.ones(2, 4))
    for cap in (0, 1025):
        with pytest.raises(ValueError):
            SB.sebb_bank(x, [row], capacity=cap)
    with pytest.raises(RuntimeError, match="no CPU path"):          # everything passed: the launch itself needs the device
        SB.sebb_bank(x, [row])
    assert SB.check_rows([row], 30, 3).tolist() == [[[5, int(np.rint(0.2 * Q)), 512]] * 3]


def test_postprocessor_parameters_config_and_round_trip(tmp_path):
    assert pkg.SebbPostprocessor is SB.SebbPostprocessor and pkg.SebbSearch is SB.SebbSearch and pkg.sebb_bank is SB.sebb_bank
    enc = EV.Encoder(["a", "b", "c"], audio_len=10, frame_len=1024, frame_hop=320, net_pooling=1, sr=32000)       # 10 ms frames
    assert [SB.half_length(s, 0.01) for s in (0.32, 0.48, 0.64, 0.001, 0.03, 0.05)] == [16, 24, 32, 1, 2, 3]
    pp = SB.SebbPostprocessor(enc, 0.48, [0.15, 0.2, 0.3], 2.0)
    assert pp.half_lengths == [24] * 3 and pp.row == ([24] * 3, [0.15, 0.2, 0.3], [2.0] * 3)
    assert pp.to_config() == {"sebb": {"step_filter_length": [0.48] * 3, "merge_threshold_abs": [0.15, 0.2, 0.3], "merge_threshold_rel": [2.0] * 3}}
    pp.save(tmp_path / "pp.json")
    back = SB.SebbPostprocessor.load(tmp_path / "pp.json", enc)
    assert back.row == pp.row and SB.is_sebb_file(tmp_path / "pp.json")
    other = EV.Encoder(["a", "b", "x"], audio_len=10, frame_len=1024, frame_hop=320, net_pooling=1, sr=32000)
    with pytest.raises(ValueError):
        SB.SebbPostprocessor.load(tmp_path / "pp.json", other)
    for bad in (dict(step_filter_length=[0.3, 0.3]), dict(merge_threshold_rel=0.5), dict(merge_threshold_abs=[0.1, 0.2, 2.0]),
                dict(step_filter_length=0.0)):
        with pytest.raises(ValueError):
            SB.SebbPostprocessor(enc, **bad)


# ------------------------------------------------------------------------------------------------ the search
def _feed(search, case, weak, batches=None):
    strong = torch.from_numpy(case.scores).transpose(1, 2).contiguous()
    weak = torch.from_numpy(weak)
    for lo, hi in batches or [(0, len(case.names))]:
        search.update(strong[lo:hi], weak[lo:hi], [n + ".wav" for n in case.names[lo:hi]])
    return search


@functools.lru_cache(maxsize=None)
def _planted_search():
    case = SC.planted()
    weak = SC.planted_weak(case)
    s = BC.host_search(case, thresholds=THETAS, objectives=("psds1", "psds2", "event_f1", "segment_f1"), **BC.SEARCH_GRID)
    return case, weak, _feed(s, case, weak, batches=[(0, 3), (3, 8)])


def _rows(case):
    return BC.grid_rows(case.scores.shape[2], SC.FRAME, **BC.SEARCH_GRID)


def test_search_candidates_and_default_grid():
    case, _, s = _planted_search()
    rows = _rows(case)
    assert [c.name for c in s.candidates] == [n for n, _ in rows] and len(rows) == 12
    assert s._rows == [r for _, r in rows] and [r[0][0] for _, r in rows[::4]] == [3, 7, 15]
    enc = EV.Encoder(case.classes, audio_len=10, frame_len=1024, frame_hop=320, net_pooling=1, sr=32000)      # 10 ms frames
    gt, dur = PC.frames(case)
    d = SB.SebbSearch(enc, gt, dur)
    assert len(d.candidates) == 27 and d.candidates[0].name == "0.32/0.15/1.5" and d.candidates[-1].name == "0.64/0.3/3"
    assert sorted({c.frames[0] for c in d.candidates}) == [16, 24, 32]
    for bad in (dict(objectives=("psds3",)), dict(objectives=()), dict(step_filter_lengths=()), dict(merge_thresholds_rel=(0.5,)),
                dict(objectives=("event_f1",), thresholds=()), dict(step_filter_lengths=tuple(0.1 * i for i in range(1, 9)))):
        with pytest.raises(ValueError):
            SB.SebbSearch(enc, gt, dur, **bad)


@pytest.mark.parametrize("name", ["psds1", "psds2"])
def test_psds_search_against_the_brute_force(name):
    case, _, s = _planted_search()
    rows = _rows(case)
    ref = BC.psds_search_ref(case, rows, PC.ARG_SETS[name])
    table = s.results()
    table = table[table["objective"] == name]
    assert len(table) == len(rows) * 3 and (table["filter_type"] == "sebb").all()
    for k, (rname, row) in enumerate(rows):
        got = table[table["candidate"] == rname]
        assert got["class"].tolist() == case.classes and got["frames"].tolist() == row[0]
        assert np.allclose(got["value"].to_numpy(), ref["single"][k], rtol=0, atol=RATE_TOL)
        assert abs(s.overall(name)[rname] - ref["overall"][k]) <= RATE_TOL
    best = s.best(name)
    assert best.candidates == [rows[k][0] for k in ref["choice"]] and best.thresholds is None and best.labels == case.classes
    assert (best.half_lengths, best.merge_threshold_abs, best.merge_threshold_rel) == tuple(ref["mixed"])
    assert abs(best.overall - ref["composed"]) <= RATE_TOL and ref["composed"] == ref["fresh"]
    assert len(set(ref["choice"])) > 1 or name == "psds2"            # (psds1: the classes of the planted case choose different rows)
    # the product's own fresh run on the mixed parameters: the same integers, the same arithmetic -> the same float
    gt, dur = PC.frames(case)
    fresh = EV.IntersectionPSDS(gt, dur, case.classes, case.ts, **EV.Evaluator.PSDS_ARGS[name])
    fresh._sweep = PC.cpu_sweep(fresh)
    pp = best.postprocessor(SC.planted_encoder(case))
    assert pp.row == tuple(ref["mixed"])
    fresh.update(torch.from_numpy(BC.bank_ref(case.scores, [pp.row])[0][0]), case.names)
    overall, single = fresh.compute()
    assert best.overall == overall and best.per_class == [single[c] for c in case.classes]


@pytest.mark.parametrize("kind", ["event_f1", "segment_f1"])
def test_f1_search_against_the_brute_force(kind):
    case, weak, s = _planted_search()
    rows = _rows(case)
    ref = BC.f1_search_ref(case, rows, THETAS, weak, kind)
    counts = s._f1_counts()
    for ti in range(len(THETAS)):
        for k in range(len(rows)):
            assert {n: [int(v) for v in counts[ti][k][n]] for n in FC.NAMES} == ref["counts"][k][ti]
    table = s.results()
    table = table[table["objective"] == kind]
    for k, (rname, _) in enumerate(rows):
        for ti, th in enumerate(THETAS):
            got = table[(table["candidate"] == rname) & (table["threshold"] == th)]
            assert got["value"].tolist() == ref["values"][k][ti]                      # integer counts, one division: exact
    best = s.best(kind)
    assert best.candidates == [rows[k][0] for k, _ in ref["choice"]] and best.thresholds == [THETAS[ti] for _, ti in ref["choice"]]
    want = EV.EventSegmentF1.scores(ref["composed"])
    tag = kind.replace("_f1", "")
    assert best.overall == want[tag + "_macro"] and best.overall_micro == want[tag + "_micro"]
    assert max(best.per_class) > 0


def test_choice_round_trip_and_batching(tmp_path):
    case, weak, s = _planted_search()
    for best in (s.best("psds1"), s.best("event_f1")):
        best.save(tmp_path / "choice.json")
        assert SB.SebbChoice.load(tmp_path / "choice.json") == best and SB.is_sebb_file(tmp_path / "choice.json")
        enc = SC.planted_encoder(case)
        pp = SB.SebbPostprocessor.load(tmp_path / "choice.json", enc)
        assert pp.row == (best.half_lengths, best.merge_threshold_abs, best.merge_threshold_rel)
        assert best.to_config() == pp.to_config() and best.to_yaml().startswith("training:\n  sebb:\n    step_filter_length: [")
        import yaml
        assert yaml.safe_load(best.to_yaml())["training"] == best.to_config()
    with pytest.raises(ValueError):
        s.best("psds3")
    one = _feed(BC.host_search(case, thresholds=THETAS, objectives=("psds1", "psds2", "event_f1", "segment_f1"), **BC.SEARCH_GRID), case, weak)
    assert one.results().equals(s.results())
