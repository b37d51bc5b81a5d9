"""Detection on a recording of any length (csrc/longform.hip; DESIGN.md section 7d holds the definitions).

Every model of this package takes one 10 s clip.  `LongFormDetector` runs a trained one over a longer (or shorter) recording: the waveform
is cut on the device into overlapping chunks of one clip each (`chunk_plan`, `sed_longform_gather`), the chunks go through the model's own
frontend and forward in batches, the chunks' frame posteriors are stitched into one timeline (`stitch_scores`), the timeline is median /
max filtered with the score tables' semantics (`median_filter_long`) and thresholded into events (`decode_events`).  A recording of at
most one clip reproduces `batched_decode_preds` of a direct model call bit for bit.  The reference has only an unused stub for this
(`get_segment_scores_and_overlap_add`, src/codec/decoder.py), so the definitions are this project's.

The detector works for any model whose forward returns `(strong [B, C, Tc], weak [B, C], other)` and whose `get_feature_extractor()` has
`logmel`; the tests pin `PaSST_SED` only.

`chunk_plan` is host arithmetic and importable without the HIP library; everything else launches hand-written kernels and raises without
them."""
from collections import namedtuple

import numpy as np

FILTER_TILE = 1024          # frames per workgroup of sed_longform_filter (csrc/longform.hip: LF_TILE)
FILTER_MAX_SIZE = 1024      # longest window it takes (tile + halo fit one LDS segment of 2048 frames)
EVENT_TILE = 256            # frames per block scan of sed_longform_event_write
EVENT_SEGMENT = 8192        # frames per workgroup of the two event passes

_MODES = {("median", "torch"): 0, ("median", "scipy"): 1, ("max", "scipy"): 2}

ChunkPlan = namedtuple("ChunkPlan", "n_samples n_frames n_chunks hop_frames chunk_frames frame_samples starts_frames starts_samples "
                                    "real_samples pad_frames")


def chunk_plan(L, hop_frames=500, chunk_frames=1000, frame_samples=320):
    """The chunks of a mono waveform of `L` samples: `Tt = ceil(L / S)` timeline frames, `K = 1 + ceil(max(0, Tt - Tc) / Hf)` chunks, chunk
    k = frames [k Hf, k Hf + Tc) = samples [k Hf S, k Hf S + Tc S).  -> ChunkPlan; `real_samples[k]` of the chunk lie before L (the rest
    is zero) and `pad_frames[k] = ceil(real_samples[k] / S)` is the first frame its pad mask marks (the rule of `data.pad_wav`)."""
    L, Hf, Tc, S = int(L), int(hop_frames), int(chunk_frames), int(frame_samples)
    if L < 1:
        raise ValueError("chunk_plan: the recording is empty")
    if Tc < 1 or S < 1:
        raise ValueError("chunk_plan: chunk_frames and frame_samples must be positive")
    if not 1 <= Hf <= Tc:
        raise ValueError(f"chunk_plan: hop_frames must lie in [1, {Tc}], got {hop_frames}")
    Tt = -(-L // S)
    K = 1 + -(-max(0, Tt - Tc) // Hf)
    starts_f = [k * Hf for k in range(K)]
    starts_s = [f * S for f in starts_f]
    real = [min(Tc * S, L - s) for s in starts_s]
    pad = [-(-r // S) for r in real]
    return ChunkPlan(L, Tt, K, Hf, Tc, S, starts_f, starts_s, real, pad)


def stitch_weights(chunk_frames, hop_frames):
    """w(i) = min(i + 1, Tc - i, R), R = max(1, Tc - Hf): integer weights of a chunk's frames in the stitch (int64 [Tc])."""
    Tc, Hf = int(chunk_frames), int(hop_frames)
    i = np.arange(Tc, dtype=np.int64)
    return np.minimum(np.minimum(i + 1, Tc - i), max(1, Tc - Hf))


def _f32(x, dev=None):
    import torch
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(x))
    t = t.detach()
    if dev is not None and t.device != dev:
        t = t.to(dev)
    return t.float().contiguous()


def gather_chunks(wav, plan, k0, nk):
    """wav [L] fp32 on the device -> chunks k0 .. k0 + nk - 1 of `plan` as [nk, Tc S], zero behind the recording."""
    import torch
    from .ops import call
    Lc = plan.chunk_frames * plan.frame_samples
    if wav.dim() != 1 or wav.numel() != plan.n_samples:
        raise ValueError("gather_chunks: wav must be the 1-D waveform the plan was made for")
    if k0 < 0 or nk < 1 or k0 + nk > plan.n_chunks:
        raise ValueError("gather_chunks: chunk range outside the plan")
    out = torch.empty(nk, Lc, dtype=torch.float32, device=wav.device)
    call("sed_longform_gather", wav, out, plan.n_samples, plan.hop_frames * plan.frame_samples, Lc, k0, nk)
    return out


def stitch_scores(strong, weak, hop_frames, n_frames, weak_mask=False):
    """strong [K, C, Tc] (weak [K, C]) on the device -> the timeline [n_frames, C] fp32: the weighted mean, with `stitch_weights`, of the
    chunks that cover a frame; a frame one chunk covers is copied.  `weak_mask`: every chunk's posteriors are first multiplied by its own
    weak prediction (the soft weak mask of `batched_decode_preds`, per chunk)."""
    import torch
    from .ops import call
    if strong.dim() != 3:
        raise ValueError("stitch_scores: strong must have shape (chunks, classes, frames)")
    K, C, Tc = strong.shape
    Hf, Tt = int(hop_frames), int(n_frames)
    if not 1 <= Hf <= Tc:
        raise ValueError(f"stitch_scores: hop_frames must lie in [1, {Tc}], got {hop_frames}")
    if not 1 <= Tt <= (K - 1) * Hf + Tc:
        raise ValueError(f"stitch_scores: {K} chunks cover {(K - 1) * Hf + Tc} frames, n_frames = {n_frames}")
    s = _f32(strong)
    w = None
    if weak_mask:
        if weak is None or tuple(weak.shape) != (K, C):
            raise ValueError("stitch_scores: weak_mask needs weak of shape (chunks, classes)")
        w = _f32(weak, s.device)
    out = torch.empty(Tt, C, dtype=torch.float32, device=s.device)
    call("sed_longform_stitch", s, w, out, K, C, Tc, Hf, Tt)
    return out


def median_filter_long(x, sizes, filter_type="median", semantics="scipy"):
    """x [T, C] on the device, any T -> the per-class median / maximum filter along T.  semantics "scipy": `ndimage.median_filter` /
    `maximum_filter` as the score tables use them (src/codec/decoder.py:91,94); "torch": `median_filter_torch`
    (src/postprocess/filter.py:4-36; median only).  Bit-exact with `filter.median_filter_scipy` / `max_filter_scipy` /
    `median_filter_torch` wherever those apply."""
    import torch
    from .ops import call, h2d
    mode = _MODES.get((filter_type, semantics))
    if mode is None:
        raise ValueError(f"median_filter_long: no filter_type={filter_type!r} with semantics={semantics!r} (median: scipy or torch; max: scipy)")
    if x.dim() != 2:
        raise ValueError("median_filter_long: x must have shape (frames, classes)")
    T, C = x.shape
    sizes = [int(s) for s in sizes]
    if len(sizes) != C:
        raise ValueError("Length of median_filter_sizes must match the number of classes")
    if C == 0 or T == 0:
        return _f32(x).clone()
    if min(sizes) < 1 or max(sizes) > FILTER_MAX_SIZE:
        raise ValueError(f"median_filter_long: window sizes must lie in [1, {FILTER_MAX_SIZE}]")
    if mode != 0 and max(sizes) > T:
        raise ValueError("scipy-semantics filter: window longer than the sequence is outside the reproduced domain")
    x = _f32(x)
    out = torch.empty_like(x)
    call("sed_longform_filter", x, out, h2d(sizes, torch.int32, x.device), T, C, mode, max(sizes))
    return out


def _thresholds(thresholds, C):
    th = np.asarray(thresholds, dtype=np.float64).reshape(-1) if np.ndim(thresholds) else np.full(C, float(thresholds))
    if th.shape != (C,):
        raise ValueError(f"thresholds: one float or one per class ({C}), got {th.size}")
    return th.astype(np.float32)


def decode_events(post, thresholds=0.5, segment=EVENT_SEGMENT):
    """post [T, C] on the device -> int32 tensor [n, 3] of (class, onset frame, offset frame = last active frame + 1) on the device: the
    maximal runs of `post[:, c] > thresholds[c]` (strict), class-major, onsets ascending -- the order of `Encoder.decode_strong`."""
    import torch
    from .ops import call, h2d
    if post.dim() != 2:
        raise ValueError("decode_events: post must have shape (frames, classes)")
    T, C = post.shape
    th = _thresholds(thresholds, C)
    if T == 0 or C == 0:
        return torch.empty(0, 3, dtype=torch.int32, device=post.device)
    post = _f32(post)
    seg = int(segment)
    nseg = -(-T // seg)
    th_d = h2d(th, torch.float32, post.device)
    seg_counts = torch.empty(C * nseg, dtype=torch.int32, device=post.device)
    seg_offs = torch.empty(C * nseg + 1, dtype=torch.int32, device=post.device)
    cls_offs = torch.empty(C + 1, dtype=torch.int32, device=post.device)
    call("sed_longform_event_count", post, th_d, T, C, seg, seg_counts, seg_offs, cls_offs)
    n = int(cls_offs.cpu()[-1])                  # the one read the host makes: the C + 1 class offsets
    events = torch.empty(n, 3, dtype=torch.int32, device=post.device)
    if n:
        call("sed_longform_event_write", post, th_d, T, C, seg, seg_offs, events)
    return events


class LongFormDetector:
    """Runs `net` (eval mode) over recordings of any length at `encoder.sr`.

    `config` (the recipe's dict) supplies `training.median_window` (scaled `int(i / 156 * 1000)` like `Evaluator`), `training.filter_type`,
    `training.weak_mask` and `config[net.get_model_name()]["val_kwargs"]`; each keyword overrides its config value.  Without a config and
    without `median_filter` the timeline is not filtered (`post` is None and `scores` / `detect` use the raw timeline)."""

    def __init__(self, net, encoder, config=None, *, hop_frames=500, batch_size=32, median_filter=None, filter_type=None, weak_mask=None,
                 forward_kwargs=None):
        self.net, self.encoder = net, encoder
        self.frame_samples = int(encoder.frame_hop * encoder.net_pooling)
        self.chunk_frames = int(encoder.n_frames)
        self.sr = int(encoder.sr)
        if not 1 <= int(hop_frames) <= self.chunk_frames:
            raise ValueError(f"hop_frames must lie in [1, {self.chunk_frames}], got {hop_frames}")
        if int(batch_size) < 1:
            raise ValueError("batch_size must be positive")
        self.hop_frames, self.batch_size = int(hop_frames), int(batch_size)
        from .evaluation.codec import check_filter_type, scaled_median_window
        tr = (config or {}).get("training", {})
        if median_filter is None and "median_window" in tr:
            median_filter = scaled_median_window(tr["median_window"])
        self.median_filter = None if median_filter is None else [int(s) for s in median_filter]
        if self.median_filter is not None and len(self.median_filter) != len(encoder.labels):
            raise ValueError("Length of median_filter_sizes must match the number of classes")
        self.filter_type = check_filter_type(filter_type if filter_type is not None else tr.get("filter_type", "median"))
        self.weak_mask = bool(weak_mask if weak_mask is not None else tr.get("weak_mask", False))
        if forward_kwargs is None:
            forward_kwargs = config[net.get_model_name()]["val_kwargs"] if config is not None else {}
        self.forward_kwargs = dict(forward_kwargs)

    # ---- device half
    def _wav(self, wav):
        import torch
        t = wav if isinstance(wav, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(wav))
        if t.dim() != 1:
            raise ValueError(f"wav must be one mono waveform [L], got shape {tuple(t.shape)}")
        if t.numel() == 0:
            raise ValueError("wav is empty")
        if not t.is_cuda:
            t = t.to(next(self.net.parameters()).device)                # (one upload)
        return t.detach().float().contiguous()

    def chunk_batches(self, wav, plan=None):
        """Yields (k0, chunks [n, Tc S], pad_mask [n, Tc] bool) for the batches the detector forwards, in order."""
        import torch
        from .ops import h2d
        wav = self._wav(wav)
        plan = plan or chunk_plan(wav.numel(), self.hop_frames, self.chunk_frames, self.frame_samples)
        frames = np.arange(plan.chunk_frames)
        for k0 in range(0, plan.n_chunks, self.batch_size):
            nk = min(self.batch_size, plan.n_chunks - k0)
            pad = frames[None, :] >= np.asarray(plan.pad_frames[k0:k0 + nk])[:, None]
            yield k0, gather_chunks(wav, plan, k0, nk), h2d(pad, torch.bool, wav.device)

    def posteriors(self, wav):
        """-> {"raw": [Tt, C], "post": [Tt, C] or None, "chunk_strong": [K, C, Tc], "chunk_weak": [K, C], "plan"}, tensors on the device."""
        import torch
        wav = self._wav(wav)
        plan = chunk_plan(wav.numel(), self.hop_frames, self.chunk_frames, self.frame_samples)
        self.net.eval()
        ext = self.net.get_feature_extractor()
        ext.eval()
        strong = weak = None
        with torch.no_grad():
            for k0, chunks, pad in self.chunk_batches(wav, plan):
                s, w, _ = self.net(ext.logmel(chunks), pad_mask=pad, **self.forward_kwargs)
                if strong is None:
                    strong = torch.empty((plan.n_chunks,) + tuple(s.shape[1:]), dtype=torch.float32, device=s.device)
                    weak = torch.empty((plan.n_chunks,) + tuple(w.shape[1:]), dtype=torch.float32, device=s.device)
                strong[k0:k0 + s.shape[0]].copy_(s)
                weak[k0:k0 + w.shape[0]].copy_(w)
        if strong.shape[-1] != plan.chunk_frames:
            raise ValueError(f"the model returned {strong.shape[-1]} frames per chunk, the encoder says {plan.chunk_frames}")
        raw = stitch_scores(strong, weak, plan.hop_frames, plan.n_frames, weak_mask=self.weak_mask)
        post = None if not self.median_filter else median_filter_long(raw, self.median_filter, self.filter_type, "scipy")
        return {"raw": raw, "post": post, "chunk_strong": strong, "chunk_weak": weak, "plan": plan}

    # ---- host half
    def frame_times(self, plan):
        """Tt + 1 frame boundaries in seconds (float64): frame S / sr, clipped to the recording."""
        return np.clip(np.arange(plan.n_frames + 1) * plan.frame_samples / self.sr, 0.0, plan.n_samples / self.sr)

    def scores(self, wav, audio_id):
        """-> (scores_raw, scores_post) like `batched_decode_preds`: two dicts `{audio_id: DataFrame}` in `create_score_dataframe`'s layout
        (Tt rows, Tt + 1 timestamps), which `write_sed_scores` takes unchanged; the post table is the raw one when nothing filters."""
        return self.tables(self.posteriors(wav), audio_id)

    def tables(self, out, audio_id):
        """`scores` from what `posteriors` returned (a caller that wants tables and events runs the model once)."""
        from .evaluation import create_score_dataframe
        ts = self.frame_times(out["plan"])
        raw_df = create_score_dataframe(out["raw"].cpu().numpy(), ts, self.encoder.labels)
        post_df = raw_df if out["post"] is None else create_score_dataframe(out["post"].cpu().numpy(), ts, self.encoder.labels)
        return {str(audio_id): raw_df}, {str(audio_id): post_df}

    def detect(self, wav, thresholds=0.5):
        """-> DataFrame(event_label, onset, offset) in seconds: the runs of the filtered timeline above `thresholds` (one float or one
        per class), class-major like `Encoder.decode_strong`."""
        _thresholds(thresholds, len(self.encoder.labels))               # (refuse before any device work)
        return self.events(self.posteriors(wav), thresholds)

    def events(self, out, thresholds=0.5):
        """`detect` from what `posteriors` returned."""
        import pandas as pd
        plan = out["plan"]
        ev = decode_events(out["post"] if out["post"] is not None else out["raw"], thresholds).cpu().numpy()
        end = plan.n_samples / self.sr
        t = np.clip(ev[:, 1:].astype(np.float64) * plan.frame_samples / self.sr, 0.0, end)
        return pd.DataFrame({"event_label": [self.encoder.labels[c] for c in ev[:, 0]], "onset": t[:, 0], "offset": t[:, 1]},
                            columns=["event_label", "onset", "offset"])

    def load(self, path):
        """File -> mono waveform at the encoder's rate on the device (`data.read_wav`, `to_mono`, `resample_poly_device` if needed)."""
        import torch
        from .data import read_wav, resample_poly_device, to_mono
        wav, sr = read_wav(path)
        wav = np.ascontiguousarray(to_mono(wav), dtype=np.float32)
        if wav.size == 0:
            raise ValueError(f"{path}: no samples")
        dev = next(self.net.parameters()).device
        t = torch.from_numpy(wav).to(dev)
        if sr != self.sr:
            t = resample_poly_device(t[None], self.sr, sr)[0].contiguous()
        return t

    def detect_file(self, path, thresholds=0.5):
        """`detect` on a wav file, with a `filename` column."""
        import os
        df = self.detect(self.load(path), thresholds)
        df["filename"] = os.path.basename(str(path))
        return df
