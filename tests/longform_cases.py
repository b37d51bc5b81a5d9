"""Seeded cases and float64 host references for long-form detection (transformer4sed_amd/longform.py).

  * `stitch_ref`   the stitch, written from the definition in float64 -- and, through its keyword switches, four WRONG stitches (a chunk
                   dropped, the hop off by one frame, no normalisation, a rectangular window) that the CPU tests show to be visible on
                   the very inputs the GPU tests use.
  * `filter_ref`   the timeline filters: `scipy.ndimage.median_filter` / `maximum_filter` per class (modes 1 / 2) and a numpy restatement
                   of `median_filter_torch` (mode 0); `filter_ref_tiled` is the wrong filter that applies the boundary rule at tile edges.
  * `events_ref`   the events of a thresholded timeline from `Encoder.find_contiguous_regions`, class by class.

Everything is generated from seeds; no test reads anything outside the repository."""
import numpy as np

U24 = 2.0 ** -24            # unit roundoff of fp32


# ------------------------------------------------------------------------------------------------------------------ chunk plan
PLAN_HOPS = (1, 250, 500, 999, 1000)


def plan_lengths(Hf, Tc=1000, S=320):
    Lc = Tc * S
    return (1, 319, 320, 321, Lc - 1, Lc, Lc + 1, Lc + Hf * S, 3 * Lc + 7)


# ------------------------------------------------------------------------------------------------------------------ stitch
def stitch_shapes():
    """(K, C, Tc, Hf, Tt): Tc in {8, 1000}, C in {1, 10, 407}, Hf in {1, 3, Tc / 2, Tc - 1, Tc}, K = 5 (K = 1 once), Tt no multiple of
    the kernel's 32-frame tile."""
    out = []
    for Tc in (8, 1000):
        for C in (1, 10, 407):
            for Hf in (1, 3, Tc // 2, Tc - 1, Tc):
                K = 5
                Tt = (K - 1) * Hf + Tc
                out.append((K, C, Tc, Hf, Tt - 1 if Tt % 32 == 0 else Tt))
    out.append((1, 10, 1000, 500, 999))
    out.append((3, 10, 1000, 500, 1700))          # a timeline that ends inside the last chunk
    return out


def stitch_inputs(K, C, Tc, seed=0):
    rng = np.random.RandomState(1000 + seed)
    return rng.uniform(0.05, 1.0, (K, C, Tc)).astype(np.float32), rng.uniform(0.05, 1.0, (K, C)).astype(np.float32)


def stitch_ref(strong, weak, Hf, Tt, weak_mask=False, *, drop=None, hop_error=0, normalise=True, window="capped"):
    """-> (ref float64 [Tt, C], n int [Tt]: chunks covering each frame).  A frame one chunk covers holds the fp32 value the kernel must copy
    (x weak: the fp32 product, exactly representable in float64); elsewhere the weighted mean in float64 of the exact products.
    The keyword switches make the wrong stitches of the defect-visibility tests."""
    strong = np.asarray(strong, dtype=np.float32)
    K, C, Tc = strong.shape
    R = max(1, Tc - Hf)
    i = np.arange(Tc)
    w = np.minimum(np.minimum(i + 1, Tc - i), R).astype(np.float64) if window == "capped" else np.ones(Tc)
    num, den, n = np.zeros((Tt, C)), np.zeros(Tt), np.zeros(Tt, dtype=np.int64)
    single = np.zeros((Tt, C), dtype=np.float32)
    for k in range(K):
        if k == drop:
            continue
        v32 = strong[k] * np.asarray(weak, dtype=np.float32)[k][:, None] if weak_mask else strong[k]          # fp32, as the kernel copies it
        v64 = strong[k].astype(np.float64) * (np.asarray(weak, dtype=np.float64)[k][:, None] if weak_mask else 1.0)
        a = k * Hf + (hop_error if k > 0 else 0)
        b = min(a + Tc, Tt)
        if b <= a:
            continue
        num[a:b] += (w[:b - a, None] * v64.T[:b - a])
        den[a:b] += w[:b - a]
        n[a:b] += 1
        single[a:b] = v32.T[:b - a]
    ref = num / np.maximum(den, 1.0)[:, None] if normalise else num
    one = n == 1
    if normalise and window == "capped":
        ref[one] = single[one].astype(np.float64)
    return ref, n


def stitch_bound(ref, n):
    """|got - ref| <= (n + 2) 2^-24 ref: n products by the weights, one more by the weak scale, n - 1 additions and one division, each within
    one unit roundoff (all terms positive: no cancellation).  Zero where one chunk covers the frame: a copy."""
    return np.where(n[:, None] == 1, 0.0, (n[:, None] + 2) * U24 * np.abs(ref))


# ------------------------------------------------------------------------------------------------------------------ filters
def filter_input(T, C, seed=0):
    """[T, C] fp32 in [0, 1): a plain column, a column quantised to eighths (many ties), a constant one, a monotone one, then plain ones."""
    rng = np.random.RandomState(2000 + seed)
    x = rng.rand(T, C).astype(np.float32)
    if C > 1:
        x[:, 1] = np.round(x[:, 1] * 8) / 8
    if C > 2:
        x[:, 2] = 0.25
    if C > 3:
        x[:, 3] = np.sort(x[:, 3])
    if C > 4:
        x[:, 4] = np.round(x[:, 4] * 64) / 64
    return x


def filter_ref(x, sizes, mode):
    """mode 1 / 2: scipy.ndimage.median_filter / maximum_filter per class; mode 0: even size -> size + 1, replicate padding, the element of
    rank k // 2 of the (odd) window -- `median_filter_torch`."""
    from scipy import ndimage
    x = np.asarray(x, dtype=np.float32)
    out = np.empty_like(x)
    for c, k in enumerate(int(s) for s in sizes):
        if mode == 1:
            out[:, c] = ndimage.median_filter(x[:, c], k)
        elif mode == 2:
            out[:, c] = ndimage.maximum_filter(x[:, c], k)
        else:
            k = k + 1 if k % 2 == 0 else k
            xp = np.pad(x[:, c], (k // 2, k // 2), mode="edge")
            out[:, c] = np.sort(np.lib.stride_tricks.sliding_window_view(xp, k), axis=-1)[:, k // 2]
    return out


def filter_ref_tiled(x, sizes, mode, tile):
    """The WRONG filter: every tile of `tile` frames filtered on its own, the boundary rule applied at tile edges."""
    return np.concatenate([filter_ref(x[a:a + tile], sizes, mode) for a in range(0, len(x), tile)], axis=0)


# ------------------------------------------------------------------------------------------------------------------ events
def event_cases(T, tile):
    """-> (post [T, 10] fp32, th [10] fp32): per-class thresholds, one column per case."""
    rng = np.random.RandomState(3000 + T)
    th = np.linspace(0.3, 0.75, 10).astype(np.float32)
    lo, hi = th - np.float32(0.2), th + np.float32(0.2)
    on = np.zeros((T, 10), dtype=bool)
    on[:min(3, T), 0] = True                                       # a run at frame 0
    on[max(0, T - 4):, 1] = True                                   # a run to the last frame
    on[::2, 2] = True                                              # alternating frames: ceil(T / 2) runs
    on[:, 4] = True                                                # all active (3: all inactive)
    if T > tile + 1:
        on[tile - 2:tile + 3, 5] = True                            # a run across a tile edge
        on[tile:tile + 2, 6] = True                                # a run that starts on one
        on[tile - 3:tile, 6] = False
        on[max(0, 2 * tile - 5):2 * tile, 7] = True                # a run that ends on one
    on[:, 8] = rng.rand(T) < 0.3                                   # random runs
    post = np.where(on, hi[None, :], lo[None, :]).astype(np.float32)
    eq = rng.rand(T) < 0.5                                         # scores EQUAL to the threshold are inactive (strict >)
    post[:, 9] = np.where(eq, th[9], hi[9])
    return post, th


def events_ref(post, th, strict=True):
    """[n, 3] int64 (class, onset, offset) from `Encoder.find_contiguous_regions`, class-major; `strict=False` is the wrong `>=` decoder."""
    from transformer4sed_amd.evaluation import Encoder
    enc = Encoder([str(c) for c in range(post.shape[1])], audio_len=10, frame_len=1024, frame_hop=320, net_pooling=1, sr=32000)
    th = np.broadcast_to(np.asarray(th, dtype=np.float32), (post.shape[1],))
    rows = []
    for c in range(post.shape[1]):
        act = post[:, c] > th[c] if strict else post[:, c] >= th[c]
        rows += [(c, int(a), int(b)) for a, b in enc.find_contiguous_regions(act)]
    return np.asarray(rows, dtype=np.int64).reshape(-1, 3)
