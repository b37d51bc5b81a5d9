"""Long-form detection on the device (csrc/longform.hip, transformer4sed_amd/longform.py): the four kernels against the
float64 host references of tests/longform_cases.py, then the detector end to end on the depth-2 model with synthetic audio."""
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

import longform_cases as LC  # noqa: E402
from transformer4sed_amd import longform as LF, synth  # noqa: E402
from transformer4sed_amd.evaluation import Encoder, batched_decode_preds, write_sed_scores  # noqa: E402
from transformer4sed_amd.ops import call, h2d  # noqa: E402

LABELS = ["Alarm_bell_ringing", "Blender", "Cat", "Dishes", "Dog", "Electric_shaver_toothbrush", "Frying", "Running_water", "Speech",
          "Vacuum_cleaner"]
TILE = LF.FILTER_TILE
SENTINEL = -12345.0


def _enc():
    return Encoder(LABELS, audio_len=10, frame_len=1024, frame_hop=320, net_pooling=1, sr=32000)


# ------------------------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("L", [5, 320000 - 3, 320000 + 1281])
@pytest.mark.parametrize("shift", [0, 1])
def test_gather_bit_exact_with_sentinels(L, shift):
    """Chunks are numpy slices of the zero-extended waveform, bit for bit, and nothing is written behind them.  `shift` = 1 hands the kernel
    a waveform that is not 16-byte aligned (the sample-by-sample path)."""
    Tc, S, Hf = 1000, 320, 500
    Lc = Tc * S
    plan = LF.chunk_plan(L, Hf, Tc, S)
    assert plan.n_chunks == (1 if L <= Lc else 2)
    wav = np.random.RandomState(L).uniform(-1, 1, L + shift).astype(np.float32)
    wav_d = torch.from_numpy(wav).to(DEV)[shift:]
    padded = np.concatenate([wav[shift:], np.zeros(plan.n_chunks * Lc, dtype=np.float32)])
    for k0, nk in ((0, plan.n_chunks), (plan.n_chunks - 1, 1)):
        buf = torch.full((nk * Lc + 256,), SENTINEL, dtype=torch.float32, device=DEV)
        call("sed_longform_gather", wav_d, buf, L, Hf * S, Lc, k0, nk)
        got = buf.cpu().numpy()
        want = np.stack([padded[(k0 + j) * Hf * S:(k0 + j) * Hf * S + Lc] for j in range(nk)])
        assert np.array_equal(got[:nk * Lc].reshape(nk, Lc), want)
        assert np.all(got[nk * Lc:] == SENTINEL)
    want = np.stack([padded[j * Hf * S:j * Hf * S + Lc] for j in range(plan.n_chunks)])
    assert np.array_equal(LF.gather_chunks(wav_d, plan, 0, plan.n_chunks).cpu().numpy(), want)


def test_gather_odd_geometry_takes_the_scalar_path():
    """A hop and a chunk length that are no multiples of four samples."""
    L, hop, Lc = 1003, 7, 30
    wav = np.arange(1, L + 1, dtype=np.float32)
    nk = 150                                                     # the last chunks run past the waveform
    buf = torch.full((nk * Lc + 64,), SENTINEL, dtype=torch.float32, device=DEV)
    call("sed_longform_gather", torch.from_numpy(wav).to(DEV), buf, L, hop, Lc, 2, nk)
    padded = np.concatenate([wav, np.zeros(nk * hop + Lc, dtype=np.float32)])
    want = np.stack([padded[(2 + j) * hop:(2 + j) * hop + Lc] for j in range(nk)])
    got = buf.cpu().numpy()
    assert np.array_equal(got[:nk * Lc].reshape(nk, Lc), want) and np.all(got[nk * Lc:] == SENTINEL)


# ------------------------------------------------------------------------------------------------------------------ stitch
@pytest.mark.parametrize("Tc,C", [(8, 1), (8, 10), (8, 407), (1000, 1), (1000, 10), (1000, 407)])
def test_stitch_vs_float64_reference(Tc, C):
    """Single-cover frames bit-exact; elsewhere |got - ref64| <= (n + 2) 2^-24 ref64 with n the number of covering chunks: the fp32 rounding
    of n products, the weak scale, n - 1 additions and one division (longform_cases.stitch_bound) -- derived, not tuned."""
    shapes = [s for s in LC.stitch_shapes() if s[2] == Tc and s[1] == C]
    assert len(shapes) >= 5
    for K, _, _, Hf, Tt in shapes:
        strong, weak = LC.stitch_inputs(K, C, Tc)
        s_d, w_d = torch.from_numpy(strong).to(DEV), torch.from_numpy(weak).to(DEV)
        for wm in (False, True):
            ref, n = LC.stitch_ref(strong, weak, Hf, Tt, wm)
            buf = torch.full((Tt * C + 64,), SENTINEL, dtype=torch.float32, device=DEV)
            call("sed_longform_stitch", s_d, w_d if wm else None, buf, K, C, Tc, Hf, Tt)
            got = buf.cpu().numpy()
            assert np.all(got[Tt * C:] == SENTINEL)
            got = got[:Tt * C].reshape(Tt, C).astype(np.float64)
            one = n == 1
            assert np.array_equal(got[one], ref[one]), (K, C, Tc, Hf, wm)
            err, bound = np.abs(got - ref), LC.stitch_bound(ref, n)
            worst = float((err / np.maximum(bound, 1e-300))[~one].max()) if (~one).any() else 0.0
            print(f"stitch K={K} C={C} Tc={Tc} Hf={Hf} weak={wm}: worst err / bound = {worst:.3f}")
            assert np.all(err <= bound), (K, C, Tc, Hf, wm, worst)
            assert torch.equal(LF.stitch_scores(s_d, w_d, Hf, Tt, weak_mask=wm), buf[:Tt * C].view(Tt, C))


# ------------------------------------------------------------------------------------------------------------------ filter
SIZES_LONG = [1, 2, 7, 24, 33, 128, 129, 64, 5, 100]            # 1, even sizes, the rank kernel's range (>= 24)
SIZES_SHORT = [1, 2, 3, 5, 7, 23, 4, 6, 9, 11]                 # all below it: the launch without rank storage
_FILTERS = {0: ("median", "torch"), 1: ("median", "scipy"), 2: ("max", "scipy")}


def _long(x_d, sizes, mode):
    return LF.median_filter_long(x_d, sizes, *_FILTERS[mode])


@pytest.mark.parametrize("T", [129, 1000, 1025, 2000])
def test_long_filter_bit_exact_with_the_clip_filter(T):
    for sizes in (SIZES_LONG, SIZES_SHORT):
        x_d = torch.from_numpy(LC.filter_input(T, 10, seed=T)).to(DEV)
        sz = h2d(sizes, torch.int32, x_d.device)
        for mode in (0, 1, 2):
            want = torch.empty(1, T, 10, dtype=torch.float32, device=DEV)
            call("sed_median_filter_k", x_d[None].contiguous(), want, sz, None, 1, T, 10, mode, max(sizes))
            assert torch.equal(_long(x_d, sizes, mode), want[0]), (T, mode, sizes)
    x1 = torch.from_numpy(LC.filter_input(T, 5, seed=T)[:, 4:5].copy()).to(DEV)         # C = 1, a quantised column
    for mode in (0, 1, 2):
        want = torch.empty(1, T, 1, dtype=torch.float32, device=DEV)
        call("sed_median_filter_k", x1[None].contiguous(), want, h2d([33], torch.int32, x1.device), None, 1, T, 1, mode, 33)
        assert torch.equal(_long(x1, [33], mode), want[0])


@pytest.mark.parametrize("C", [1, 10])
@pytest.mark.parametrize("T", [TILE - 1, TILE, TILE + 1, 2 * TILE + max(SIZES_LONG) - 1])
def test_long_filter_vs_host_references_across_tiles(T, C):
    """TILE - 1 and TILE: both true ends in one tile; TILE + 1: a one-frame last tile whose whole window is halo; the last: three tiles, the
    last as long as the longest window's halo."""
    sizes = SIZES_LONG[:C] if C > 1 else [129]
    x = LC.filter_input(T, 10, seed=7)[:, :C].copy() if C > 1 else LC.filter_input(T, 5, seed=7)[:, 1:2].copy()
    x_d = torch.from_numpy(x).to(DEV)
    for mode in (0, 1, 2):
        buf = torch.full((T * C + 64,), SENTINEL, dtype=torch.float32, device=DEV)
        call("sed_longform_filter", x_d, buf, h2d(sizes, torch.int32, x_d.device), T, C, mode, max(sizes))
        got = buf.cpu().numpy()
        assert np.all(got[T * C:] == SENTINEL)
        assert np.array_equal(got[:T * C].reshape(T, C), LC.filter_ref(x, sizes, mode)), (T, C, mode)
    for sz in ([2] * C, [23] * C):
        for mode in (0, 1, 2):
            assert np.array_equal(_long(x_d, sz, mode).cpu().numpy(), LC.filter_ref(x, sz, mode)), (T, C, mode, sz)


def test_long_filter_refusals_and_limits():
    x = torch.zeros(100, 3, device=DEV)
    for ftype in ("median", "max"):
        with pytest.raises(ValueError):
            LF.median_filter_long(x, [3, 101, 3], ftype, "scipy")                  # scipy-mode window longer than T
    assert LF.median_filter_long(x, [3, 101, 3], "median", "torch").shape == (100, 3)    # replicate padding has no such limit
    with pytest.raises(ValueError):
        LF.median_filter_long(torch.zeros(3000, 1, device=DEV), [LF.FILTER_MAX_SIZE + 1], "median", "scipy")
    T = 2 * TILE + 5                                                                # the longest window there is
    xx = LC.filter_input(T, 2, seed=3)
    for mode, k in ((0, LF.FILTER_MAX_SIZE), (1, LF.FILTER_MAX_SIZE), (2, LF.FILTER_MAX_SIZE)):
        got = _long(torch.from_numpy(xx).to(DEV), [k, 3], mode).cpu().numpy()
        assert np.array_equal(got, LC.filter_ref(xx, [k, 3], mode)), mode


@pytest.mark.parametrize("partly", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
def test_long_filter_nan_column(mode, partly):
    """T = 300, windows [24, 33] (both by global ranks): column 0 all NaN comes out all NaN -- the references' own answer, see
    test_gpu_postproc_search.test_nan_column_is_a_nan_column_in_the_clip_kernel; with every 7th frame NaN its values are unspecified.
    Either way the launch returns, writes nothing behind the buffer and column 1 holds the bits of the launch on a finite column 0."""
    T, C, sizes = 300, 2, [24, 33]
    x = LC.filter_input(T, 10, seed=5)[:, :C].copy()
    x_bad = x.copy()
    x_bad[::7 if partly else 1, 0] = np.nan
    out = []
    for inp in (x, x_bad):
        buf = torch.full((T * C + 64,), SENTINEL, dtype=torch.float32, device=DEV)
        call("sed_longform_filter", torch.from_numpy(inp).to(DEV), buf, h2d(sizes, torch.int32, buf.device), T, C, mode, max(sizes))
        got = buf.cpu().numpy()
        assert np.all(got[T * C:] == SENTINEL)
        out.append(got[:T * C].reshape(T, C))
    want, got = out
    assert not np.isnan(want).any()
    assert np.array_equal(got[:, 1].view(np.int32), want[:, 1].view(np.int32))
    if not partly:
        assert np.isnan(got[:, 0]).all()


# ------------------------------------------------------------------------------------------------------------------ events
@pytest.mark.parametrize("T", [1, 2, LF.EVENT_TILE, 3 * LF.EVENT_TILE + 1])
def test_events_vs_find_contiguous_regions(T):
    post, th = LC.event_cases(T, LF.EVENT_TILE)
    want = LC.events_ref(post, th)
    post_d = torch.from_numpy(post).to(DEV)
    for seg in (LF.EVENT_SEGMENT, LF.EVENT_TILE, 300, 1):
        if seg == 1 and T > 2:
            continue
        got = LF.decode_events(post_d, th, segment=seg)
        assert got.dtype == torch.int32 and got.is_cuda
        assert np.array_equal(got.cpu().numpy().astype(np.int64), want), (T, seg)
    # one threshold for all classes, and nothing active at all
    assert np.array_equal(LF.decode_events(post_d, 0.5).cpu().numpy(), LC.events_ref(post, 0.5))
    assert LF.decode_events(post_d, 2.0).shape == (0, 3)
    with pytest.raises(ValueError):
        LF.decode_events(post_d, [0.5] * 9)


def test_events_many_classes_and_segments():
    rng = np.random.RandomState(9)
    T, C = 2500, 407
    post = (rng.rand(T, C) < rng.rand(C)[None] * 0.5 + 0.25).astype(np.float32) * 0.5 + 0.25
    th = np.full(C, 0.5, dtype=np.float32)
    got = LF.decode_events(torch.from_numpy(post).to(DEV), th, segment=700).cpu().numpy()
    assert np.array_equal(got.astype(np.int64), LC.events_ref(post, th))


# ------------------------------------------------------------------------------------------------------------------ the detector
CFG = {"training": {"median_window": [5, 20, 5, 5, 5, 20, 20, 20, 5, 20], "filter_type": "median", "weak_mask": True},
       "PaSST_SED": {"val_kwargs": {"encoder_win": True, "win_param": [512, 31], "mix_rate": 0.5, "temp_w": 0.5}}}
FAST = {"encoder_win": False, "temp_w": 0.5}


@pytest.fixture(scope="module")
def net():
    from test_gpu_model import _build
    return _build(False, 2, 2)[0]


def _audio(seconds, seed):
    n = int(round(seconds * 32000))
    return synth.synth_wav(-(-n // 320000), seed=seed).reshape(-1)[:n].copy()


def _sizes():
    return [int(i / 156 * 1000) for i in CFG["training"]["median_window"]]


@pytest.mark.parametrize("weak_mask", [False, True])
@pytest.mark.parametrize("ftype", ["median", "max"])
def test_a_ten_second_recording_reproduces_the_clip_path(net, weak_mask, ftype):
    """One chunk, no stitching: the tables equal `batched_decode_preds` of a direct call of the model on the clip and the events equal
    `Encoder.decode_strong` of the filtered posteriors above 0.5, bit for bit."""
    enc = _enc()
    wav = torch.from_numpy(_audio(10.0, seed=31)).to(DEV)
    det = LF.LongFormDetector(net, enc, CFG, weak_mask=weak_mask, filter_type=ftype, forward_kwargs=FAST)
    raw, post = det.scores(wav, "rec")
    net.eval()
    with torch.no_grad():
        ext = net.get_feature_extractor()
        ext.eval()
        strong, weak, _ = net(ext.logmel(wav[None]), pad_mask=torch.zeros(1, 1000, dtype=torch.bool, device=DEV), **FAST)
    r0, p0 = batched_decode_preds(strong, ["rec.wav"], enc, filter=_sizes(), filter_type=ftype, weak_preds=weak, need_weak_mask=weak_mask)
    assert list(raw) == ["rec"] and raw["rec"].shape == (1000, 12)
    assert raw["rec"].equals(r0["rec"]) and post["rec"].equals(p0["rec"])
    events = det.detect(wav)
    want = enc.decode_strong(p0["rec"].to_numpy()[:, 2:] > 0.5)
    print(f"10 s recording, weak_mask={weak_mask}, {ftype}: {len(want)} events")
    assert events["event_label"].tolist() == [e[0] for e in want]
    assert np.array_equal(events[["onset", "offset"]].to_numpy(), np.asarray([e[1:] for e in want], dtype=np.float64).reshape(-1, 2))
    assert float(strong.max()) > 0.0


def test_a_23_7_second_recording_chunk_by_chunk(net, tmp_path):
    """K = 4 at a hop of 500 frames, batches of 3 (a ragged last batch): every stage against its own reference."""
    enc = _enc()
    wav_h = _audio(23.7, seed=41)
    wav = torch.from_numpy(wav_h).to(DEV)
    det = LF.LongFormDetector(net, enc, CFG, batch_size=3, forward_kwargs=FAST)
    out = det.posteriors(wav)
    plan = out["plan"]
    assert (plan.n_chunks, plan.n_frames, plan.pad_frames) == (4, 2370, [1000, 1000, 1000, 870])
    # chunks: the model called directly on the detector's own batches
    net.eval()
    sizes = []
    with torch.no_grad():
        for k0, chunks, pad in det.chunk_batches(wav):
            sizes.append(chunks.shape[0])
            s, w, _ = net(net.get_feature_extractor().logmel(chunks), pad_mask=pad, **FAST)
            assert torch.equal(out["chunk_strong"][k0:k0 + s.shape[0]], s) and torch.equal(out["chunk_weak"][k0:k0 + s.shape[0]], w)
            for j in range(chunks.shape[0]):
                a = (k0 + j) * 500 * 320
                seg = wav_h[a:a + 320000]
                assert np.array_equal(chunks[j].cpu().numpy(), np.concatenate([seg, np.zeros(320000 - len(seg), dtype=np.float32)]))
    assert sizes == [3, 1]
    assert float(out["chunk_strong"][3, :, 870:].abs().max()) == 0.0 and float(out["chunk_strong"][3, :, :870].max()) > 0.0
    # timeline: the host stitch of those chunks
    strong, weak = out["chunk_strong"].cpu().numpy(), out["chunk_weak"].cpu().numpy()
    ref, n = LC.stitch_ref(strong, weak, 500, plan.n_frames, True)
    raw = out["raw"].cpu().numpy()
    assert raw.shape == (2370, 10) and n.max() == 2 and (n == 1).sum() == 500 + 370
    assert np.array_equal(raw[n == 1].astype(np.float64), ref[n == 1])
    assert np.all(np.abs(raw - ref) <= LC.stitch_bound(ref, n))
    # filter and events: host references on the device's own input
    post = out["post"].cpu().numpy()
    assert np.array_equal(post, LC.filter_ref(raw, _sizes(), 1))
    th = [0.5, 0.4, 0.3, 0.5, 0.45, 0.5, 0.35, 0.5, 0.25, 0.5]
    want = LC.events_ref(post, th)
    events = det.detect(wav, th)
    print(f"23.7 s recording: {len(want)} events in {len(set(want[:, 0].tolist()))} classes")
    assert events["event_label"].tolist() == [LABELS[c] for c in want[:, 0]]
    assert np.array_equal(events[["onset", "offset"]].to_numpy(), np.clip(want[:, 1:] * 320 / 32000, 0.0, len(wav_h) / 32000))
    # tables: Tt rows, Tt + 1 timestamps, the last one the end of the recording; write_sed_scores takes them as they are
    raw_t, post_t = det.scores(wav_h, "long")                       # (a host waveform: uploaded once)
    assert np.array_equal(post_t["long"].to_numpy()[:, 2:], post.astype(np.float64)) and len(post_t["long"]) == 2370
    assert post_t["long"]["offset"].iloc[-1] == 23.7 and post_t["long"]["onset"].iloc[1] == 0.01
    write_sed_scores(post_t, tmp_path / "post")
    assert os.listdir(tmp_path / "post") == ["long.tsv"]


def test_twelve_seconds_with_the_configs_validation_kwargs(net):
    enc = _enc()
    det = LF.LongFormDetector(net, enc, CFG)
    assert det.forward_kwargs == CFG["PaSST_SED"]["val_kwargs"] and det.weak_mask and det.filter_type == "median"
    out = det.posteriors(torch.from_numpy(_audio(12.0, seed=51)).to(DEV))
    assert out["plan"].n_chunks == 2 and out["raw"].shape == out["post"].shape == (1200, 10)
    raw = out["raw"].cpu().numpy()
    ref, n = LC.stitch_ref(out["chunk_strong"].cpu().numpy(), out["chunk_weak"].cpu().numpy(), 500, 1200, True)
    assert np.all(np.abs(raw - ref) <= LC.stitch_bound(ref, n)) and np.isfinite(raw).all() and raw.max() > 0
    assert np.array_equal(out["post"].cpu().numpy(), LC.filter_ref(raw, _sizes(), 1))


def test_half_a_second(net):
    """K = 1, Tt = 50, 950 padded frames: the tables have 50 rows and no time passes the end of the recording."""
    enc = _enc()
    wav = _audio(0.5, seed=61)
    det = LF.LongFormDetector(net, enc, CFG, forward_kwargs=FAST, median_filter=[7] * 10)
    out = det.posteriors(wav)
    assert out["plan"].n_chunks == 1 and out["plan"].pad_frames == [50] and out["raw"].shape == (50, 10)
    assert torch.equal(out["raw"], (out["chunk_strong"][0, :, :50] * out["chunk_weak"][0][:, None]).t())
    raw_t, post_t = det.scores(wav, "short")
    assert raw_t["short"].shape == (50, 12) and post_t["short"].shape == (50, 12) and post_t["short"]["offset"].iloc[-1] == 0.5
    ev = det.detect(wav, 0.0)
    assert (ev["offset"] <= 0.5).all()
    # the config's windows (32 / 128 frames) are longer than this timeline: the scipy-semantics filter refuses, as on a clip
    with pytest.raises(ValueError):
        LF.LongFormDetector(net, enc, CFG, forward_kwargs=FAST).posteriors(wav)


def test_detect_file_resamples_a_16k_file_on_the_device(net, tmp_path):
    from transformer4sed_amd.data import read_wav, resample_poly_device, write_wav
    enc = _enc()
    x16 = _audio(6.0, seed=71)[::2].copy()                           # 96 000 samples, written as a 6 s PCM file at 16 kHz
    path = tmp_path / "clip16k.wav"
    write_wav(str(path), x16, 16000)
    back, sr = read_wav(str(path))
    assert sr == 16000 and len(back) == len(x16)
    det = LF.LongFormDetector(net, enc, CFG, forward_kwargs=FAST, median_filter=[7] * 10)
    wav32 = resample_poly_device(torch.from_numpy(back).to(DEV)[None], 32000, 16000)[0].contiguous()
    assert wav32.numel() == 2 * len(x16)
    want = det.detect(wav32, 0.3)
    got = det.detect_file(str(path), 0.3)
    assert list(got.columns) == ["event_label", "onset", "offset", "filename"] and (got["filename"] == "clip16k.wav").all()
    assert got[["event_label", "onset", "offset"]].equals(want)
