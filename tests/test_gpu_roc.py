"""ROC area on the device: `sed_roc_compute`, `sed_segment_pool` and `sed_segment_gather` against the host
references of tests/roc_cases.py -- integers and pooled bits must be equal -- and the classes on top against scikit-learn."""
import os
import sys
import warnings

import numpy as np
import pandas as pd
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda"

import roc_cases as RC  # noqa: E402
from transformer4sed_amd._lib import SedHipError  # noqa: E402
from transformer4sed_amd.evaluation import (AP_CHUNK, AudiosetStrongEvaluator, MultilabelAUROC, MultilabelAveragePrecision,  # noqa: E402
                                            SegmentAUROC, roc)
from transformer4sed_amd.ops import call  # noqa: E402

SK_TOL = 1e-9           # as in tests/test_roc_cpu.py
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def device_ints(c, chunk=AP_CHUNK):
    return roc.roc_integers(dev(c["scores"]), dev(c["labels"]), c["scores"].shape[1], c["max_fpr"], chunk).cpu().numpy()


@pytest.mark.parametrize("N,chunk", [(1, AP_CHUNK), (2, AP_CHUNK), (63, AP_CHUNK), (64, AP_CHUNK), (65, AP_CHUNK), (1000, AP_CHUNK),
                                     (64, 64), (65, 64), (200, 64)])
def test_roc_compute_equals_host_reference(N, chunk):
    for levels in (8, None):
        for max_fpr in (0.1, 0.25, 1.0):
            c = RC.random_case(N, levels, max_fpr, seed=N + chunk, C=3)
            got, want = device_ints(c, chunk), RC.reference(c)
            assert np.array_equal(got, want), (c["name"], chunk, got, want)


def test_roc_compute_on_the_designated_cases():
    for c in RC.designated_cases():
        want = RC.reference(c)
        for chunk in (AP_CHUNK, 5):
            assert np.array_equal(device_ints(c, chunk), want), (c["name"], chunk)


def test_roc_integers_do_not_depend_on_order_or_chunk():
    for levels in (8, None):
        c = RC.random_case(1000, levels, 0.1, seed=5)
        want = RC.reference(c)
        perm = np.random.RandomState(2).permutation(1000)
        shuffled = dict(c, scores=c["scores"][:, perm], labels=c["labels"][:, perm])
        for chunk in (64, 100, 20000):
            assert np.array_equal(device_ints(c, chunk), want), chunk
            assert np.array_equal(device_ints(shuffled, chunk), want), chunk


def test_bad_arguments_return_err_arg_and_write_nothing():
    s, y = torch.rand(3, 100, device=DEV), torch.zeros(3, 100, dtype=torch.uint8, device=DEV)
    out = torch.full((3, 8), -7, dtype=torch.int64, device=DEV)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=DEV)
    scratch = torch.zeros(3 * 5, dtype=torch.int64, device=DEV)
    ok = dict(scores=s, labels=y, C=3, N=100, cap=100, chunk=AP_CHUNK, max_fpr=0.1, a=None, p=None, cnt=None, scratch=None, out=out)
    for bad in (dict(C=0), dict(N=0), dict(cap=99), dict(chunk=0), dict(chunk=AP_CHUNK + 1), dict(max_fpr=0.0), dict(max_fpr=1.5),
                dict(max_fpr=float("nan")), dict(scores=None), dict(labels=None), dict(out=None), dict(chunk=64),
                dict(chunk=64, a=i32(600), p=i32(600), cnt=i32(6)), dict(chunk=64, a=i32(600), p=i32(600), scratch=scratch)):
        with pytest.raises(SedHipError, match="code -1"):
            call("sed_roc_compute", *{**ok, **bad}.values())
    pooled, status = torch.full((10, 2), -7.0, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    x, ts = torch.rand(1, 5, 2, device=DEV), torch.arange(6, device=DEV) * 200000
    length, row = torch.tensor([1000000], device=DEV), i32(1)
    ok = dict(x=x, ts=ts, length=length, row=row, seg=1000000, n=1, T=5, C=2, max_seg=1, cap=10, pooled=pooled, status=status)
    for bad in (dict(n=-1), dict(T=0), dict(C=0), dict(seg=0), dict(max_seg=0), dict(cap=-1), dict(status=None), dict(x=None),
                dict(ts=None), dict(length=None), dict(row=None), dict(pooled=None), dict(n=65536)):
        with pytest.raises(SedHipError, match="code -1"):
            call("sed_segment_pool", *{**ok, **bad}.values())
    ptr, rows, res = i32(3), i32(2), torch.full((2, 2), -7.0, device=DEV)
    ok = dict(pooled=pooled, ptr=ptr, rows=rows, S=2, C=2, n_rows=10, nnz=0, max_rows=0, ld=2, out=res, status=status)
    for bad in (dict(S=0), dict(C=0), dict(n_rows=-1), dict(nnz=-1), dict(max_rows=-1), dict(ld=1), dict(ptr=None), dict(out=None),
                dict(status=None), dict(nnz=2, rows=None), dict(nnz=2, pooled=None), dict(nnz=2, n_rows=0)):
        with pytest.raises(SedHipError, match="code -1"):
            call("sed_segment_gather", *{**ok, **bad}.values())
    assert (out == -7).all() and (pooled == -7).all() and (res == -7).all() and (status == 0).all()
    # rows a clip or a list may not reach are reported, never written or read
    call("sed_segment_pool", x, ts, length, torch.tensor([10], dtype=torch.int32, device=DEV), 1000000, 1, 5, 2, 1, 10, pooled, status)
    assert (pooled == -7).all() and status.tolist() == [0, 0, 1, 0]
    status.zero_()
    call("sed_segment_gather", pooled, torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV),
         torch.tensor([3, 10], dtype=torch.int32, device=DEV), 2, 2, 10, 2, 1, 2, res, status)
    assert status.tolist() == [0, 0, 1, 0] and res.tolist() == [[-7.0, 0.0], [-7.0, 0.0]]


# ---------------------------------------------------------------------------------------------------- segments
TS1 = (np.array([0, 1000000], dtype=np.int64), 1000000)          # T = 1: one frame of a second


@pytest.mark.parametrize("seg_s", [1.0, 0.7])
@pytest.mark.parametrize("name", ["156x64ms", "1000x10ms", "9.5s", "T=1"])
def test_segment_pool_is_bit_equal(name, seg_s):
    ts_us, clip_us = TS1 if name == "T=1" else RC.geometry(name)
    T, seg_us = ts_us.size - 1, int(RC.microseconds(seg_s))
    x = np.stack([RC.frame_scores(T, 3, seed=s) for s in (1, 2)])
    acc = SegmentAUROC(roc._empty_ground_truth(), {"u": clip_us / 1e6, "v": clip_us / 1e6}, ["a", "b", "c"], ts_us / 1e6, seg_s)
    xd = dev(x)
    torch.cuda.set_sync_debug_mode("error")                       # update() never waits for the device
    try:
        acc.update(xd, ["u.wav", "v.wav"])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    want = np.concatenate([RC.pool_ref(x[i], ts_us, clip_us, seg_us) for i in range(2)])
    got = acc._pooled[:acc._used].cpu().numpy()
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
    tables = acc.segment_scores()
    n_seg = want.shape[0] // 2
    assert list(tables) == ["u", "v"] and list(tables["v"].columns) == ["onset", "offset", "a", "b", "c"]
    assert np.array_equal(bits(tables["v"][["a", "b", "c"]].to_numpy()), bits(want[n_seg:]))
    assert tables["u"]["offset"].iloc[-1] == clip_us / 1e6 and tables["u"]["onset"].iloc[-1] == (n_seg - 1) * (seg_us / 1e6)


@pytest.fixture(scope="module")
def sliding():
    ids, onsets, duration = RC.sliding_file()
    ts_us, clip_us = RC.geometry("156x64ms")
    x = np.stack([RC.frame_scores(156, 3, seed=70 + j) for j in range(len(ids))])
    return ids, onsets, duration, ts_us, clip_us, x


@pytest.mark.parametrize("seg_s", [1.0, 0.7])
def test_overlap_add_is_bit_equal_in_any_batching(sliding, seg_s):
    ids, onsets, duration, ts_us, clip_us, x = sliding
    seg_us = int(RC.microseconds(seg_s))
    n_seg = -(-int(RC.microseconds(duration)) // seg_us)
    want = RC.overlap_add_ref([(on, RC.pool_ref(x[j], ts_us, clip_us, seg_us)) for j, on in enumerate(onsets)], n_seg, seg_us)
    xd = dev(x)
    for batch in (1, 5, 14):
        order = np.random.RandomState(batch).permutation(len(ids))
        acc = SegmentAUROC(roc._empty_ground_truth(), {"long": duration}, ["a", "b", "c"], ts_us / 1e6, seg_s, clip_ids="sliding")
        for lo in range(0, len(ids), batch):
            take = order[lo:lo + batch]
            acc.update(xd[torch.from_numpy(take).to(DEV)], [ids[j] for j in take])
        got = acc._file_scores().cpu().numpy()
        assert got.shape == (3, n_seg) and np.array_equal(bits(got.T), bits(want)), (seg_s, batch)
    if seg_s == 1.0:
        assert (want[23] == 0).all() and (want[:23] > 0).all()


def test_reference_functions_on_dataframes(sliding, golden):
    ids, onsets, duration, ts_us, clip_us, x = sliding
    g = golden("segment_scores")
    classes = ["a", "b", "c"]
    frame = lambda s, ts: roc.create_score_dataframe(s, ts, classes)
    df = roc.get_segment_scores(frame(g["9.5s/scores"], g["9.5s/ts"]), clip_length=9.5)
    assert np.abs(df[classes].to_numpy() - g["9.5s/out"]).max() <= 2.0 ** -24 * 1.01
    assert np.array_equal(np.r_[df["onset"].to_numpy(), df["offset"].to_numpy()[-1]], g["9.5s/out_ts"])
    assert np.array_equal(x, g["ola/scores"])
    out = roc.get_segment_scores_and_overlap_add({cid: frame(s, g["ola/ts"]) for cid, s in zip(ids, x)}, {"long": duration}, classes)
    assert list(out) == ["long"]
    assert np.abs(out["long"][classes].to_numpy() - g["ola/out"]).max() <= 2.0 ** -24 * 1.01
    assert np.array_equal(np.r_[out["long"]["onset"].to_numpy(), out["long"]["offset"].to_numpy()[-1]], g["ola/out_ts"])


def test_segment_auroc_matches_sklearn_on_the_downloaded_scores(sliding):
    sk = pytest.importorskip("sklearn.metrics")
    ids, onsets, duration, ts_us, clip_us, x = sliding
    rng = np.random.RandomState(4)
    files = {"long": duration, "mid": 17.0, "short": 10.0}
    rows = [(f + ".wav", on, on + float(rng.uniform(0.3, 4.0)), "abc"[int(rng.randint(3))])
            for f, d in files.items() for on in rng.uniform(0, d - 0.5, size=int(d / 3)).tolist()]
    gt = pd.DataFrame(rows, columns=["filename", "onset", "offset", "event_label"])
    names = ids + [f"mid-{100 * o}-{100 * o + 1000}" for o in range(0, 8, 2)] + ["short-0-1000"]
    scores = np.concatenate([x, np.stack([RC.frame_scores(156, 3, seed=90 + j) for j in range(5)])])
    results = {}
    for normalize in ("mcclish", "max_fpr"):
        acc = SegmentAUROC(gt, files, ["a", "b", "c"], ts_us / 1e6, max_fpr=0.1, normalize=normalize, clip_ids="sliding")
        with pytest.raises(ValueError, match="files without scores"):
            acc.compute()
        acc.update(dev(scores[:14]), names[:14])
        with pytest.raises(ValueError, match="files without scores"):
            acc.compute()
        acc.update(dev(scores[14:]), names[14:])
        results[normalize] = (acc, acc.compute(), acc.segment_scores())
    acc, res, tables = results["mcclish"]
    assert acc.target.shape == (3, 24 + 17 + 10) and list(tables) == ["long", "mid", "short"]
    host = np.concatenate([tables[f][["a", "b", "c"]].to_numpy() for f in files])
    ints = acc.counts()
    for c, name in enumerate("abc"):
        y = acc.target[c]
        assert 0 < y.sum() < y.size
        assert np.array_equal(ints[c], RC.ref_points(host[:, c].astype(np.float32), y, 0.1))
        assert abs(res["per_class"][name]["pauc"] - sk.roc_auc_score(y, host[:, c], max_fpr=0.1)) <= SK_TOL
        assert abs(res["per_class"][name]["auroc"] - sk.roc_auc_score(y, host[:, c])) <= SK_TOL
        assert abs(results["max_fpr"][1]["per_class"][name]["pauc"] - float(RC.finish_fraction(ints[c], 0.1, "max_fpr")[1])) <= SK_TOL
    assert abs(res["mpauc"] - np.mean([res["per_class"][n]["pauc"] for n in "abc"])) <= 1e-15
    assert abs(res["auroc"] - np.mean([res["per_class"][n]["auroc"] for n in "abc"])) <= 1e-15
    # a new epoch: reset forgets the clips, the same updates give the same integers
    acc.reset()
    acc.update(dev(scores), names)
    assert np.array_equal(acc.counts(), ints)
    acc.reset()
    bad = scores.copy()
    bad[3, 7, 1] = np.nan
    acc.update(dev(bad), names)
    with pytest.raises(ValueError, match="NaN"):
        acc.counts()


# ---------------------------------------------------------------------------------------------------- multilabel
def test_multilabel_auroc_matches_sklearn_and_the_sigmoid_rule():
    sk = pytest.importorskip("sklearn.metrics")
    rng = np.random.RandomState(8)
    C = 5
    probs = (np.round(rng.rand(300, C) * 31) / 31).astype(np.float32)
    logits = (rng.randn(200, C) * 3).astype(np.float32)
    assert (logits > 1).any()
    y = (rng.rand(500, C) < 0.3).astype(np.int64)
    y[:, 4] = 0                                                     # a class without a positive: NaN, left out with a warning
    stored = np.concatenate([probs, torch.sigmoid(torch.from_numpy(logits)).numpy()])
    for max_fpr in (None, 0.1):
        m = MultilabelAUROC(C, average=None, max_fpr=max_fpr)
        batches = [(dev(probs), dev(y[:300])), (dev(logits), dev(y[300:]))]
        torch.cuda.set_sync_debug_mode("error")
        try:
            m.update(*batches[0])
            m(*batches[1])
        finally:
            torch.cuda.set_sync_debug_mode(0)
        kept = m.scores[:, :500].t().cpu().numpy()
        assert np.array_equal(kept[:300], probs) and np.abs(kept[300:] - stored[300:]).max() <= 1e-7     # a logit batch is sigmoid-ed
        got = m.compute()
        assert got.dtype == torch.float64 and got.shape == (C,) and got.is_cuda and bool(torch.isnan(got[4]))
        want = [sk.roc_auc_score(y[:, c], kept[:, c].astype(np.float64), max_fpr=max_fpr) for c in range(4)]
        assert np.abs(got[:4].cpu().numpy() - want).max() <= SK_TOL
        ints = m.per_class().cpu().numpy()
        assert np.array_equal(ints, [RC.ref_points(kept[:, c], y[:, c], max_fpr or 1.0) for c in range(C)])
        for avg in ("macro", "weighted"):
            m.average = avg
            with pytest.warns(UserWarning, match="Ignoring these classes in " + avg):
                val = float(m.compute())
            w = y.sum(0)[:4] if avg == "weighted" else np.ones(4)
            assert abs(val - np.dot(want, w) / w.sum()) <= SK_TOL
        full = np.mean([sk.roc_auc_score(y[:, c], kept[:, c].astype(np.float64)) for c in range(4)])
        m.average = "macro"
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            dp = m.d_prime()
        from statistics import NormalDist
        assert abs(float(dp) - 2 ** 0.5 * NormalDist().inv_cdf(full)) <= 1e-8
    m.reset()
    with pytest.raises(RuntimeError, match="before any update"):
        m.compute()
    m.update(torch.full((4, C), float("nan"), device=DEV), torch.ones(4, C, device=DEV))
    with pytest.raises(RuntimeError, match="NaN"):
        m.compute()


def test_compute_auroc_reads_compute_maps_storage():
    rng = np.random.RandomState(12)
    C = 7
    batches = [(dev((np.round(rng.rand(n, C) * 63) / 63).astype(np.float32)), dev((rng.rand(n, C) < 0.25).astype(np.int64)))
               for n in (33, 64, 150)]
    ev = AudiosetStrongEvaluator.__new__(AudiosetStrongEvaluator)   # (the two methods read `map` only: no network is needed)
    ev.map = MultilabelAveragePrecision(C, average="macro", compute_on_step=False)
    fresh = {f: MultilabelAUROC(C, average="macro", max_fpr=f) for f in (None, 0.25)}
    for p, t in batches:
        ev.map.update(p, t)
        for m in fresh.values():
            m.update(p, t)
    before = ev.compute_map()
    ap_bits = ev.map.per_class()[0].clone()
    where = (ev.map.scores.data_ptr(), ev.map.labels.data_ptr(), ev.map.n, ev.map.cap)
    for f, m in fresh.items():
        res = ev.compute_auroc(max_fpr=f)
        assert set(res) == {"auroc", "d_prime", "per_class"}
        assert res["auroc"] == float(m.compute()) and np.array_equal(res["per_class"], m.per_class().cpu().numpy())
        assert res["d_prime"] == float(fresh[None].d_prime())
    assert where == (ev.map.scores.data_ptr(), ev.map.labels.data_ptr(), ev.map.n, ev.map.cap)          # no second copy
    after = ev.compute_map()
    assert torch.equal(before.view(torch.int32), after.view(torch.int32))
    assert torch.equal(ap_bits.view(torch.int64), ev.map.per_class()[0].view(torch.int64))
