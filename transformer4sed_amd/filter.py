"""Median / max filtering of frame posteriors on device, bit-exact with both reference semantics
(src/postprocess/filter.py:4-36 and the scipy calls at src/codec/decoder.py:91,94)."""
import torch

from .ops import call, h2d


def _run(x, sizes, mode, scale=None):
    if x.dim() != 3:
        raise ValueError("input_tensor must have shape (Batch, Length, Classes)")
    B, T, C = x.shape
    if len(sizes) != C:
        raise ValueError("Length of median_filter_sizes must match the number of classes")
    x = x.contiguous().float()
    out = torch.empty_like(x)
    if B == 0 or T == 0:
        return out                                    # the reference's loops simply do not run
    if mode != 0 and max(int(s) for s in sizes) > T:
        # scipy's line extension for windows longer than the sequence is not periodic reflection (ndimage.median_filter of a
        # 5-sample line with size 33 returns zeros); that regime never occurs on this path (T = 1000, windows <= 129)
        raise ValueError("scipy-semantics filter: window longer than the sequence is outside the reproduced domain")
    sz = h2d(list(sizes), torch.int32, x.device)
    sc = None if scale is None else scale.contiguous().float()
    call("sed_median_filter_k", x, out, sz, sc, B, T, C, mode, max(int(s) for s in sizes))     # (the bound selects the long-window kernel)
    return out


def median_filter_torch(input_tensor, filter_size: list):
    """Drop-in for src/postprocess/filter.py:4 (even sizes -> +1, replicate padding, true median)."""
    return _run(input_tensor, filter_size, 0)


def median_filter_scipy(scores, filter_size, weak_scale=None):
    """scores [B,T,C]; semantics of `ndimage.filters.median_filter(c_scores[:, idx], filter[idx])` (decoder.py:91),
    optionally after the soft weak mask `c_scores * weak_preds[j]` (decoder.py:80)."""
    return _run(scores, filter_size, 1, weak_scale)


def max_filter_scipy(scores, filter_size, weak_scale=None):
    return _run(scores, filter_size, 2, weak_scale)


FILTER_BANK_MAX_ROWS = 64      # csrc/median_filter.hip: window rows of one launch


def check_bank_sizes(sizes, T, C, mode):
    """The window rows of a bank as [W][C] ints, after the bounds the kernel answers with NaN planes: ValueError first."""
    if mode not in (0, 1, 2):
        raise ValueError("mode must be 0 (torch median), 1 (scipy median) or 2 (scipy max)")
    rows = [[int(s) for s in row] for row in sizes]
    if not 1 <= len(rows) <= FILTER_BANK_MAX_ROWS:
        raise ValueError(f"filter_bank takes 1 .. {FILTER_BANK_MAX_ROWS} window rows, got {len(rows)}")
    for row in rows:
        if len(row) != C:
            raise ValueError("every row of sizes must hold one window per class")
        if min(row) < 1:
            raise ValueError("window sizes must be at least 1 frame")
        if mode != 0 and max(row) > T:
            raise ValueError("scipy-semantics filter: window longer than the sequence is outside the reproduced domain")
    return rows


def filter_bank(x, sizes, mode, scale=None):
    """x [B, T, C], sizes [W][C] -> [W, B, T, C]: out[w] is bit for bit what `sed_median_filter_k` writes for the row sizes[w] under the
    bank's bound (the largest window of all rows) -- the values of `_run(x, sizes[w], mode, scale)` -- all W rows from one launch that
    stages and ranks every (clip, class) column once (csrc/median_filter.hip)."""
    if x.dim() != 3:
        raise ValueError("input_tensor must have shape (Batch, Length, Classes)")
    B, T, C = x.shape
    rows = check_bank_sizes(sizes, T, C, mode)
    x = x.contiguous().float()
    out = torch.empty((len(rows), B, T, C), dtype=torch.float32, device=x.device)
    if B == 0 or T == 0:
        return out
    sz = h2d(rows, torch.int32, x.device)
    sc = None if scale is None else scale.contiguous().float()
    call("sed_median_filter_bank", x, out, sz, sc, B, T, C, len(rows), mode, max(max(r) for r in rows))
    return out
