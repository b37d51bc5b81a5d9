"""Long-form detection without a GPU: the chunk plan, the host references of tests/longform_cases.py (that they are what they claim, and
that the defects the GPU tests are meant to catch are visible on the GPU tests' own inputs), the argument refusals, the build wiring."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import longform_cases as LC  # noqa: E402
from transformer4sed_amd import longform as LF  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("Hf", LC.PLAN_HOPS)
def test_chunk_plan(Hf):
    Tc, S = 1000, 320
    for L in LC.plan_lengths(Hf, Tc, S):
        p = LF.chunk_plan(L, Hf, Tc, S)
        Tt = -(-L // S)
        assert p.n_samples == L and p.n_frames == Tt == int(np.ceil(L / S))
        assert p.n_chunks == 1 + int(np.ceil(max(0, Tt - Tc) / Hf)) == len(p.starts_frames)
        assert p.starts_frames == [k * Hf for k in range(p.n_chunks)] and p.starts_samples == [k * Hf * S for k in range(p.n_chunks)]
        covered = np.zeros(Tt, dtype=int)
        for k in range(p.n_chunks):
            real = min(Tc * S, L - p.starts_samples[k])
            assert real >= 1 and p.real_samples[k] == real
            assert p.pad_frames[k] == int(np.ceil(real / S)) <= Tc
            covered[p.starts_frames[k]:p.starts_frames[k] + Tc] += 1
            # every real frame of the chunk lies on the timeline, every frame of the timeline inside the chunk is real
            assert p.starts_frames[k] + p.pad_frames[k] == min(Tt, p.starts_frames[k] + Tc)
        assert covered.min() >= 1                                              # every frame < Tt is covered
        assert covered.max() <= int(np.ceil(Tc / Hf))
        if p.n_chunks > 1:
            assert p.pad_frames[-1] > Tc - Hf                                  # the last chunk is needed: it holds frames no other covers
    assert LF.chunk_plan(Tc * S, Hf, Tc, S).n_chunks == 1 and LF.chunk_plan(Tc * S + 1, Hf, Tc, S).n_chunks == 2


def test_chunk_plan_pad_rule_is_pad_wavs():
    """`pad_frames` is the first frame `data.pad_wav` marks for a clip of `real_samples` samples."""
    from transformer4sed_amd.data import pad_wav
    from transformer4sed_amd.evaluation import Encoder
    enc = Encoder(["a"], audio_len=10, frame_len=1024, frame_hop=320, net_pooling=1, sr=32000)
    for L in (1, 319, 320, 321, 16000, 319999, 320000, 320001, 327581):
        p = LF.chunk_plan(L, 500, enc.n_frames, enc.frame_hop * enc.net_pooling)
        for k in range(p.n_chunks):
            _, mask = pad_wav(np.zeros(p.real_samples[k], dtype=np.float32), 320000, enc)
            want = int(np.argmax(mask.numpy())) if mask.any() else enc.n_frames
            assert p.pad_frames[k] == want, (L, k)


def test_stitch_weights():
    assert LF.stitch_weights(8, 4).tolist() == [1, 2, 3, 4, 4, 3, 2, 1]
    assert LF.stitch_weights(8, 6).tolist() == [1, 2, 2, 2, 2, 2, 2, 1]
    assert LF.stitch_weights(8, 8).tolist() == [1] * 8 and LF.stitch_weights(8, 7).tolist() == [1] * 8
    assert LF.stitch_weights(8, 1).tolist() == [1, 2, 3, 4, 4, 3, 2, 1]


def test_host_stitch_is_a_weighted_mean_and_copies_single_cover_frames():
    for K, C, Tc, Hf, Tt in LC.stitch_shapes():
        const = np.full((K, C, Tc), 0.375, dtype=np.float32)
        ref, n = LC.stitch_ref(const, None, Hf, Tt)
        assert np.array_equal(ref, np.full((Tt, C), 0.375)), (K, C, Tc, Hf)      # a constant input gives the constant, exactly (0.375 w sums exactly)
        assert n.min() >= 1 and n.max() <= -(-Tc // Hf)
        strong, weak = LC.stitch_inputs(K, C, Tc)
        for wm in (False, True):
            ref, n = LC.stitch_ref(strong, weak, Hf, Tt, wm)
            lo = np.min(strong * (weak[:, :, None] if wm else 1), axis=(0, 2))
            hi = np.max(strong * (weak[:, :, None] if wm else 1), axis=(0, 2))
            assert np.all(ref >= lo[None] * (1 - 1e-6)) and np.all(ref <= hi[None] * (1 + 1e-6))
            for t in np.nonzero(n == 1)[0][:50]:
                k = min(t // Hf, K - 1)
                want = strong[k, :, t - k * Hf] * weak[k] if wm else strong[k, :, t - k * Hf]
                assert np.array_equal(ref[t], want.astype(np.float64))
    # hand-computed: two chunks of 4 frames, hop 2: w = (1, 2, 2, 1)
    s = np.array([[[1, 2, 3, 4]], [[10, 20, 30, 40]]], dtype=np.float32)
    ref, n = LC.stitch_ref(s, None, 2, 6)
    assert n.tolist() == [1, 1, 2, 2, 1, 1]
    assert np.allclose(ref[:, 0], [1, 2, (2 * 3 + 1 * 10) / 3, (1 * 4 + 2 * 20) / 3, 30, 40], rtol=0, atol=1e-15)


def test_stitch_defects_are_visible_on_the_gpu_tests_inputs():
    for K, C, Tc, Hf, Tt in LC.stitch_shapes():
        strong, weak = LC.stitch_inputs(K, C, Tc)
        ref, n = LC.stitch_ref(strong, weak, Hf, Tt, True)
        multi = n.max() > 1
        if K > 1:
            bad, _ = LC.stitch_ref(strong, weak, Hf, Tt, True, drop=1)
            assert np.abs(bad - ref).max() >= 1e-3, ("dropped chunk", K, C, Tc, Hf)
            bad, _ = LC.stitch_ref(strong, weak, Hf, Tt, True, hop_error=1)
            assert np.abs(bad - ref).max() >= 1e-3, ("hop off by one", K, C, Tc, Hf)
        if multi:
            bad, _ = LC.stitch_ref(strong, weak, Hf, Tt, True, normalise=False)
            assert np.abs(bad - ref).max() >= 1e-3, ("no normalisation", K, C, Tc, Hf)
        if multi and Tc - Hf > 1:                                            # (with R = 1 the capped window IS rectangular)
            bad, _ = LC.stitch_ref(strong, weak, Hf, Tt, True, window="rect")
            assert np.abs(bad - ref).max() >= 1e-3, ("rectangular window", K, C, Tc, Hf)
        bad, _ = LC.stitch_ref(strong, weak, Hf, Tt, False)                  # the weak scale left out
        assert np.abs(bad - ref).max() >= 1e-3


def test_filter_references_agree_with_the_oracles_restatement_and_see_tile_edges():
    tile = LF.FILTER_TILE
    sizes = [1, 2, 7, 24, 33, 128, 129, 64, 5, 100]
    for T in (tile + 1, 2 * tile + max(sizes) - 1):
        x = LC.filter_input(T, 10)
        for mode in (0, 1, 2):
            ref = LC.filter_ref(x, sizes, mode)
            assert np.array_equal(ref[:, 0], x[:, 0])                            # a window of one frame copies
            assert np.array_equal(ref[:, 2], x[:, 2])                            # a constant column stays
            bad = LC.filter_ref_tiled(x, sizes, mode, tile)
            assert np.abs(bad - ref).max() >= 1e-3, (T, mode)                    # the boundary rule at a tile edge is visible
            edge = np.abs(bad - ref).max(axis=1).nonzero()[0]
            assert np.all(np.abs(edge[:, None] - np.arange(tile, T, tile)[None]).min(axis=1) <= max(sizes))      # ... and only there
    # the scipy restatement every other filter test of the suite uses: window [i - k // 2, i - k // 2 + k), symmetric padding, rank k // 2
    x = LC.filter_input(300, 5)
    for k in (2, 3, 24, 33, 64):
        xp = np.pad(x[:, 1], (k // 2, k - 1 - k // 2), mode="symmetric")
        want = np.sort(np.lib.stride_tricks.sliding_window_view(xp, k), axis=-1)
        assert np.array_equal(LC.filter_ref(x[:, 1:2], [k], 1)[:, 0], want[:, k // 2])
        assert np.array_equal(LC.filter_ref(x[:, 1:2], [k], 2)[:, 0], want[:, -1])


def test_event_reference_and_the_strict_comparison():
    for T in (1, 2, LF.EVENT_TILE, 3 * LF.EVENT_TILE + 1):
        post, th = LC.event_cases(T, LF.EVENT_TILE)
        ev = LC.events_ref(post, th)
        per = {c: ev[ev[:, 0] == c][:, 1:] for c in range(10)}
        assert per[0][0].tolist() == [0, min(3, T)] and per[1][-1][1] == T
        assert len(per[2]) == (T + 1) // 2 and len(per[3]) == 0 and per[4].tolist() == [[0, T]]
        assert np.all(ev[:, 2] > ev[:, 1]) and np.all(np.diff(ev[:, 0]) >= 0)
        for c in range(10):
            assert np.all(per[c][1:, 0] > per[c][:-1, 1])                        # maximal runs: a gap between two of a class
        if T > 2:
            bad = LC.events_ref(post, th, strict=False)                          # `>=` turns the frames equal to the threshold on
            assert len(bad) != len(ev) or not np.array_equal(bad, ev)
            assert bad[bad[:, 0] == 9].tolist() == [[9, 0, T]]


def test_argument_refusals():
    import torch
    with pytest.raises(ValueError):
        LF.chunk_plan(0)
    for Hf in (0, 1001, -1):
        with pytest.raises(ValueError):
            LF.chunk_plan(1000, Hf)
    from transformer4sed_amd.evaluation import Encoder
    enc = Encoder([f"c{i}" for i in range(10)], audio_len=10, frame_len=1024, frame_hop=320, net_pooling=1, sr=32000)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

        def get_model_name(self):
            return "PaSST_SED"

    for Hf in (0, 1001):
        with pytest.raises(ValueError):
            LF.LongFormDetector(Net(), enc, hop_frames=Hf)
    with pytest.raises(ValueError):
        LF.LongFormDetector(Net(), enc, filter_type="mean")
    with pytest.raises(ValueError):
        LF.LongFormDetector(Net(), enc, median_filter=[3] * 9)
    det = LF.LongFormDetector(Net(), enc, {"training": {"median_window": [5, 20, 5, 5, 5, 20, 20, 20, 5, 20], "filter_type": "max",
                                                        "weak_mask": True},
                                           "PaSST_SED": {"val_kwargs": {"encoder_win": True, "temp_w": 0.5}}})
    assert det.median_filter == [32, 128, 32, 32, 32, 128, 128, 128, 32, 128] and det.filter_type == "max" and det.weak_mask
    assert det.forward_kwargs == {"encoder_win": True, "temp_w": 0.5}
    assert (det.frame_samples, det.chunk_frames, det.sr) == (320, 1000, 32000)
    with pytest.raises(ValueError):
        det.detect(np.zeros(0, dtype=np.float32))                                # empty
    with pytest.raises(ValueError):
        det.detect(np.zeros((2, 100), dtype=np.float32))                         # more than one dimension
    with pytest.raises(ValueError):
        det.detect(np.zeros(100, dtype=np.float32), thresholds=[0.5] * 9)        # a threshold list whose length is not C
    with pytest.raises(ValueError):
        det.posteriors(torch.zeros(0))
    x = torch.zeros(5, 3)
    with pytest.raises(ValueError):
        LF.median_filter_long(x, [3, 3], "median")                               # one size per class
    with pytest.raises(ValueError):
        LF.median_filter_long(x, [3, 3, 3], "max", "torch")                      # no such filter
    with pytest.raises(ValueError):
        LF.median_filter_long(x, [3, 3, 7], "median", "scipy")                   # scipy-mode window longer than T
    with pytest.raises(ValueError):
        LF.median_filter_long(x, [3, 0, 3], "median", "torch")
    with pytest.raises(ValueError):
        LF.decode_events(x, [0.5, 0.5])
    with pytest.raises(ValueError):
        LF.stitch_scores(torch.zeros(2, 3, 8), None, 9, 10)                      # hop beyond the chunk
    with pytest.raises(ValueError):
        LF.stitch_scores(torch.zeros(2, 3, 8), None, 4, 13)                      # more frames than the chunks cover
    with pytest.raises(ValueError):
        LF.stitch_scores(torch.zeros(2, 3, 8), None, 4, 12, weak_mask=True)      # the mask without weak predictions


def test_header_build_and_package_wiring():
    import transformer4sed_amd as pkg
    from transformer4sed_amd import build
    from transformer4sed_amd._lib import parse_header
    protos = parse_header()
    for name in ("sed_longform_gather", "sed_longform_stitch", "sed_longform_filter", "sed_longform_event_count",
                 "sed_longform_event_write"):
        assert name in protos, name
    assert "longform.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "longform.hip"))
    for name in ("LongFormDetector", "chunk_plan", "stitch_scores", "median_filter_long", "decode_events"):
        assert getattr(pkg, name) is getattr(LF, name)
    src = open(os.path.join(build.CSRC, "longform.hip")).read()
    assert int(re.search(r"#define\s+LF_TILE\s+(\d+)", src).group(1)) == LF.FILTER_TILE
    assert int(re.search(r"#define\s+LF_MAXN\s+(\d+)", src).group(1)) - LF.FILTER_TILE == LF.FILTER_MAX_SIZE
