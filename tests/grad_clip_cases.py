"""Shared by tests/test_grad_clip_cpu.py and tests/test_gpu_grad_clip.py: synthetic arena layouts and values, and a float64 numpy
restatement of what the gradient-clip kernels compute (csrc/grad_clip.hip), written from torch.nn.utils.clip_grad_norm_'s definition."""
import numpy as np

from transformer4sed_amd import synth
from transformer4sed_amd.grad_clip import GRAD_CHUNK

CH = GRAD_CHUNK
# every size at which the chunking takes another path: below / at / above the 64-float alignment, below / at / above one chunk, several
# chunks with a ragged tail; plus a one-element tensor and (in `synthetic_arena`) an all-zero tensor
SIZES = (1, 63, 64, 65, CH - 1, CH, CH + 1, 3 * CH + 7)
ZERO_TENSOR = "t5"        # the CH-element tensor is the all-zero one (a whole chunk of zeros)


def pad64(n):
    return (n + 63) // 64 * 64


def synthetic_layout(sizes=SIZES):
    """[(name, offset, numel)] packed like the gradient arena: every slice starts on a multiple of 64 floats."""
    layout, off = [], 0
    for i, k in enumerate(sizes):
        layout.append((f"t{i}", off, k))
        off += pad64(k)
    return layout, off


def synthetic_arena(tag="grad_clip/arena"):
    """(arena float32 [total], layout, total): det_uniform values scaled per tensor over six decades (1e-3 .. 1e3, so one tensor dominates
    the total and others vanish beside it), one all-zero tensor, zero padding between the slices."""
    layout, total = synthetic_layout()
    arena = np.zeros(total, dtype=np.float32)
    for i, (n, o, k) in enumerate(layout):
        if n == ZERO_TENSOR:
            continue
        scale = np.float32(10.0 ** (-3 + 6 * ((i * 3) % len(layout)) / (len(layout) - 1)))
        arena[o:o + k] = synth.det_uniform(f"{tag}/{n}", (k,)) * scale
    return arena, layout, total


def reference(arena, layout, max_norm):
    """float64 restatement: -> (norms float64 [n], total float64, scale float32).  Sums of squares per tensor and over the tensors in
    float64; the clip coefficient as torch.nn.utils.clip_grad_norm_ computes it, in its precision: the fp32 total norm,
    max_norm / (total + 1e-6) in fp32, clamped to at most 1 (torch.clamp keeps a NaN).  max_norm <= 0: measure only, scale 1."""
    a = np.asarray(arena, dtype=np.float64)
    with np.errstate(all="ignore"):
        sumsq = np.array([np.sum(a[o:o + k] * a[o:o + k]) for _, o, k in layout], dtype=np.float64)
        norms, total = np.sqrt(sumsq), np.sqrt(np.sum(sumsq))
        scale = np.float32(1.0)
        if max_norm > 0:
            coef = np.float32(max_norm) / (np.float32(total) + np.float32(1e-6))
            scale = np.float32(1.0) if coef > 1 else np.float32(coef)
    return norms, total, scale


def scaled(arena, scale):
    """What sed_scale_by_dev leaves: untouched for a scale >= 1, else float32(g) * float32(scale), one rounding per element."""
    arena = np.asarray(arena, dtype=np.float32)
    if scale >= 1:
        return arena.copy()
    with np.errstate(all="ignore"):
        return arena * np.float32(scale)


def same_bits(a, b):
    """Bit equality of two float32 arrays, any NaN equal to any NaN."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))
