"""Gradient-norm clipping and gradient-norm telemetry on the flat fp32 gradient arena (csrc/grad_clip.hip).

`clip_grad_norm_(net, max_norm)` is `torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm, norm_type=2)` as three launches over
`net._last_grad_arena` -- chunked sums of squares, one finalising workgroup, one in-place scaling pass that reads the clip coefficient from
device memory -- instead of one norm kernel and one multiply per parameter tensor; nothing travels to the host.  `grad_norms(net)` is the
measuring half alone.  The trainers call the clip only when `training["max_grad_norm"]` is set (`max_grad_norm_of`); the recipes' `clip_grad`
key keeps the reference's meaning, a clip of gradients that were just cleared.

The chunk table is host arithmetic on the arena layout (`grad_chunk_table`, importable without the HIP library); it is built and uploaded once
per layout and cached on the model."""
import math

import numpy as np

GRAD_CHUNK = 16384      # floats per chunk = per workgroup of sed_grad_sumsq_chunks (csrc/grad_clip.hip: 16 x 16 bytes in flight per lane)


def grad_chunk_table(layout, CH=GRAD_CHUNK):
    """layout: [(name, offset, numel)] with 64-aligned offsets, in arena order -> (chunk_tab int32 [n_chunks, 2] = {offset, length},
    tensor_first_chunk int32 [n_tensors + 1]).  A tensor's elements [offset, offset + numel) are cut into runs of CH floats and one shorter
    tail; the alignment padding behind a slice belongs to no chunk (it is not part of any gradient).  Chunks are in arena order, tensor t
    owns chunks [first[t], first[t + 1]) -- none for an empty tensor."""
    CH = int(CH)
    if CH <= 0 or CH % 64:
        raise ValueError(f"grad_chunk_table: the chunk length must be a positive multiple of 64, got {CH}")
    tab, first, end = [], [], 0
    for name, off, numel in layout:
        off, numel = int(off), int(numel)
        if off % 64 or numel < 0:
            raise ValueError(f"grad_chunk_table: slice of {name!r} at offset {off} ({numel} elements) is not 64-float aligned")
        if off < end:
            raise ValueError(f"grad_chunk_table: slice of {name!r} at offset {off} overlaps or precedes the slice before it (ends at {end})")
        first.append(len(tab))
        for o in range(0, numel, CH):
            tab.append((off + o, min(CH, numel - o)))
        end = off + numel
    first.append(len(tab))
    if end >= 2 ** 31:
        raise ValueError("grad_chunk_table: arena offsets beyond 2^31 - 1 do not fit the int32 table")
    return np.asarray(tab, dtype=np.int32).reshape(-1, 2), np.asarray(first, dtype=np.int32)


def max_grad_norm_of(training):
    """The optional `training["max_grad_norm"]` of a trainer config -> float, or None (absent / None: no clipping, no launches).  0 measures
    only (the step reports `grad_norm`, nothing is scaled).  Negative or non-finite values raise."""
    v = training.get("max_grad_norm")
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
        raise ValueError(f"training['max_grad_norm'] must be a finite float >= 0 (or absent / None for no clipping), got {v!r}")
    return float(v)


def model_layout(net):
    """(key, [(name, offset, numel)], total) of the gradient arena the model's backward fills: the bound FusedAdamWEMA's layout, otherwise
    the model's own packing of the parameters it computes gradients for (passt_sed._SedFunction.backward)."""
    flat = getattr(net, "_flat_layout", None)
    if flat is not None:
        return ("flat", id(flat), flat.total), flat.layout, flat.total
    inert = getattr(net, "_inert_param_names", ())
    layout, off = [], 0
    for n in net._param_names:
        p = net._param_by_name[n]
        if p.requires_grad and not n.startswith("backbone.head") and n not in inert:
            layout.append((n, off, p.numel()))
            off += (p.numel() + 63) // 64 * 64
    return ("own", tuple(layout)), layout, off


class _Plan:
    """Device copies of one layout's chunk table and the partial-sum scratch."""

    def __init__(self, layout, total, dev):
        import torch
        from .ops import h2d
        tab, first = grad_chunk_table(layout)
        if len(tab) and int((tab[:, 0].astype(np.int64) + tab[:, 1]).max()) > total:
            raise RuntimeError("grad_clip: the chunk table reaches past the gradient arena")
        self.names = [n for n, _, _ in layout]
        self.n_chunks, self.n_tensors, self.total = len(tab), len(layout), total
        self.tab = h2d(tab.reshape(-1) if len(tab) else np.zeros(2, np.int32), torch.int32, dev)
        self.first = h2d(first, torch.int32, dev)
        self.partial = torch.empty(max(self.n_chunks, 1), dtype=torch.float32, device=dev)


def _plan_of(net, dev):
    key, layout, total = model_layout(net)
    cached = getattr(net, "_grad_clip_plan", None)
    if cached is None or cached[0] != (key, str(dev)):
        cached = net._grad_clip_plan = ((key, str(dev)), _Plan(layout, total, dev))
    return cached[1]


def arena_norms(arena, plan, max_norm=0.0, scale_arena=False):
    """The launches on a flat arena with a `_Plan`: -> (norms [n_tensors], total 0-dim, scale 0-dim), all device tensors of one fresh
    buffer.  `scale_arena`: also arena *= scale (skipped on the device when scale >= 1)."""
    import torch
    from .ops import call
    if arena.dtype != torch.float32 or arena.dim() != 1 or arena.numel() != plan.total:
        raise RuntimeError(f"grad_clip: the gradient arena holds {arena.numel()} {arena.dtype} elements, the layout describes {plan.total} float32")
    n = plan.n_tensors
    out = torch.empty(n + 2, dtype=torch.float32, device=arena.device)
    call("sed_grad_sumsq_chunks", arena, plan.tab, plan.n_chunks, plan.partial)
    call("sed_grad_norm_finalize", plan.partial, plan.first, n, float(max_norm), out, out[n:])
    if scale_arena:
        call("sed_scale_by_dev", arena, arena.numel(), out[n + 1:])
    return out[:n], out[n], out[n + 1]


def _arena_and_plan(net, what):
    p = next(net.parameters())
    if not p.is_cuda:
        raise RuntimeError(f"{what} needs the model on an MI355X (HIP) device; there is no CPU path")
    arena = getattr(net, "_last_grad_arena", None)
    if arena is None:
        raise RuntimeError(f"{what}: no flat gradient arena (call loss.backward() on the model output first)")
    return arena, _plan_of(net, arena.device)


def grad_norms(net):
    """-> (names, norms, total): per-parameter L2 norms of the gradients of the last backward as a device tensor [n] in arena-layout order
    (`names`), and their global L2 norm as a 0-dim device tensor.  No host synchronisation.  A parameter without a gradient this step has
    a zero arena slice: norm 0, no contribution (torch skips it: the same total)."""
    arena, plan = _arena_and_plan(net, "grad_norms")
    norms, total, _ = arena_norms(arena, plan)
    return list(plan.names), norms, total


def clip_grad_norm_(net, max_norm, norm_type=2.0):
    """torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm, norm_type=2, error_if_nonfinite=False) on the flat gradient arena: scales
    it in place by min(1, max_norm / (total + 1e-6)) -- every `p.grad` is a view of the arena -- and returns the total norm BEFORE clipping
    (0-dim device tensor).  The coefficient stays on the device; `net._last_clip_scale` holds it (0-dim device tensor) for whoever wants to
    log it.  max_norm = 0 measures only.  Gradients that did not come from the model's backward into the arena (an external query input
    of DASM) are not parameters' and are not touched."""
    if float(norm_type) != 2.0:
        raise ValueError(f"clip_grad_norm_: only norm_type=2 is implemented on the HIP path, got {norm_type!r}")
    max_norm = float(max_norm)
    if not math.isfinite(max_norm) or max_norm < 0:
        raise ValueError(f"clip_grad_norm_: max_norm must be a finite float >= 0, got {max_norm!r}")
    arena, plan = _arena_and_plan(net, "clip_grad_norm_")
    _, total, scale = arena_norms(arena, plan, max_norm, scale_arena=max_norm > 0)
    net._last_clip_scale = scale
    return total
