"""Ragged window sets for the sliding-window merge (csrc/norm_elem.hip: sed_window_mix, sed_window_mix_bwd), their float64 reference
and a restatement of the two kernels' loops on the CPU (pure construction helpers; no tests here).

A case is (B, T, ratio, windows, order, mix): `windows[w]` = (left, tp_w) -- first output frame and number of pooled frames of window
w; `order` = the window indices in the order their [B, tp_w, D] blocks lie in the packed buffer, so offs[order[0]] = 0 and the row
ranges [offs[w], offs[w] + B tp_w) tile [0, rows).  The engine packs group by group (windows of equal tp_w, groups in order of first
appearance: `engine_order`), which puts window 0 first; the *-short-first cases do not.

Reference: oracle.matsed_oracle.merge_windows in float64 with autograd, its interpolation index in the fused fp32 form the kernels
compile to (`fused_index`), so that both sides use the same `lam` and the bounds below only have to cover fp32 rounding:
  forward   (cnt_max + 8) 2^-24 (max|pooled| + max|x|)    a sum of cnt lerps, one scale, one mix
  backward  (4 ratio + 8) 2^-24 max|dx|                   the taps one packed row examines
`emulate_fwd` / `emulate_bwd` restate the loops of window_mix_kernel / window_mix_bwd_kernel (row -> window search, jlo / jhi clamps,
the j >= T break, the per-frame cnt recount) in the type of their inputs; tests/test_window_cases_cpu.py holds them to the reference,
tests/test_gpu_window_mix.py holds the hardware to it."""
import collections
import functools

import torch

from oracle import matsed_oracle as O

F32, F64 = torch.float32, torch.float64
U32 = 2.0 ** -24            # unit roundoff of fp32

WindowCase = collections.namedtuple("WindowCase", "name B T ratio windows order mix")


# ------------------------------------------------------------------------------------------------ window geometry
def sweep(T, win, step, emb_len=None):
    """(left, tp_w) of every window of a sweep, with the arithmetic of SedEngine.forward: window w covers input frames
    [left, min(left + win, T)), holds (width - 16) // 10 + 1 time patches and starts at output frame round(left emb_len / T)."""
    emb_len = T if emb_len is None else emb_len
    out = []
    for left in O.window_starts(T, win, step):
        width = min(left + win, T) - left
        out.append((round(left * (emb_len / T)), (width - 16) // 10 + 1))
    return out


def groups_of(windows):
    """{tp_w: [window indices]} in order of first appearance -- the groups SedEngine.forward folds into one encoder pass each."""
    g = {}
    for w, (_, tp) in enumerate(windows):
        g.setdefault(tp, []).append(w)
    return g


def engine_order(windows):
    return [w for wis in groups_of(windows).values() for w in wis]


def short_first(windows):
    """The groups in reverse order of first appearance: the shorter last window's block comes first."""
    return [w for wis in reversed(list(groups_of(windows).values())) for w in wis]


def tables(case):
    """lefts, tps, offs (lists indexed by window) and the number of packed rows."""
    lefts = [l for l, _ in case.windows]
    tps = [t for _, t in case.windows]
    offs, row = [0] * len(tps), 0
    for w in case.order:
        offs[w] = row
        row += case.B * tps[w]
    assert sorted(case.order) == list(range(len(tps)))
    return lefts, tps, offs, row


def coverage(case):
    """Number of windows that cover each output frame [T] (long)."""
    cnt = torch.zeros(case.T, dtype=torch.long)
    for left, tp in case.windows:
        cnt[left:min(case.T, left + tp * case.ratio)] += 1
    return cnt


VAL17 = sweep(1000, 512, 31)            # 16 windows of 50 patches + one of 49; frames 986..999 uncovered
THREE = sweep(1000, 500, 49)            # 11 windows of 49 patches + one of 45
TINY = [(0, 5), (30, 4), (20, 3), (100, 3)]     # T = 120: frames 30..49 under three windows, 70..99 under none, 120..129 cut off
TINY_ONE = [(90, 4)]                            # nW = 1: frames 0..89 uncovered, 120..129 cut off


def _cases():
    out = []
    for B, mix in ((3, 0.5), (1, 1.0)):
        out.append(WindowCase(f"val17-B{B}-mix{mix}", B, 1000, 10, VAL17, engine_order(VAL17), mix))
        out.append(WindowCase(f"val17-short-first-B{B}-mix{mix}", B, 1000, 10, VAL17, short_first(VAL17), mix))
    for B in (1, 3):
        out.append(WindowCase(f"three-sizes-B{B}-mix0.5", B, 1000, 10, THREE, engine_order(THREE), 0.5))
    for B in (1, 3):
        for mix in (0.0, 0.5, 1.0):         # mix = 0: no local part, dpooled == 0; mix = 1: no global part, dglobal == 0
            out.append(WindowCase(f"tiny-B{B}-mix{mix}", B, 120, 10, TINY, [3, 1, 0, 2], mix))
        out.append(WindowCase(f"tiny-one-window-B{B}-mix0.5", B, 120, 10, TINY_ONE, [0], 0.5))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
# (engine order, short-first order) of the same windows, batch and mix: the packing-order invariance pairs
ORDER_PAIRS = [("val17-B3-mix0.5", "val17-short-first-B3-mix0.5"), ("val17-B1-mix1.0", "val17-short-first-B1-mix1.0")]


# ------------------------------------------------------------------------------------------------ inputs, packing
def inputs(case, D, seed=0):
    """N(0, 1) fp32: per-window frames [B, tp_w, D], the global pass x [B, T, D] and the output gradient g [B, T, D].  The draw of a
    window depends on its index alone, so two packing orders of the same windows get the same numbers."""
    frames = []
    for w, (_, tp) in enumerate(case.windows):
        g = torch.Generator(device="cpu").manual_seed(1000 * seed + w)
        frames.append(torch.randn(case.B, tp, D, generator=g))
    g = torch.Generator(device="cpu").manual_seed(1000 * seed + 999)
    return frames, torch.randn(case.B, case.T, D, generator=g), torch.randn(case.B, case.T, D, generator=g)


def pack(frames, case):
    """[rows, D]: window w's [B, tp_w, D] block at row offs[w]."""
    _, tps, offs, rows = tables(case)
    out = frames[0].new_full((rows, frames[0].shape[-1]), float("nan"))
    for w, fr in enumerate(frames):
        out[offs[w]:offs[w] + case.B * tps[w]] = fr.reshape(case.B * tps[w], -1)
    assert not bool(torch.isnan(out).any())         # the ranges tile [0, rows)
    return out


def unpack(packed, case):
    _, tps, offs, _ = tables(case)
    return [packed[offs[w]:offs[w] + case.B * tps[w]].reshape(case.B, tps[w], -1) for w in range(len(tps))]


# ------------------------------------------------------------------------------------------------ float64 reference and bounds
def reference(case, frames, x, g):
    """Float64 merge and its autograd: out [B, T, D], d(frames) (list, per window), d(x)."""
    fr = [f.double().requires_grad_(True) for f in frames]
    xx = x.double().requires_grad_(True)
    out = O.merge_windows(fr, [l for l, _ in case.windows], case.T, case.ratio, mix=case.mix, x=xx, fused_index=True)
    out.backward(g.double())
    return out.detach(), [f.grad for f in fr], xx.grad


def fwd_bound(case, frames, x):
    amax = max(float(f.abs().max()) for f in frames) + float(x.abs().max())
    return (int(coverage(case).max()) + 8) * U32 * amax


def bwd_bound(case, g):
    return (4 * case.ratio + 8) * U32 * float(g.abs().max())


# ------------------------------------------------------------------------------------------------ the kernels' loops
@functools.lru_cache(maxsize=None)
def interp_coeff(j, ratio, tlen, tin):
    """interp_coeff of csrc/norm_elem.hip: (i0, i1, lam) with lam an fp32 value (held in a Python float)."""
    scale = float(torch.tensor(1.0 / ratio, dtype=F64).float())
    src = float(torch.tensor(scale * (j + 0.5) - 0.5, dtype=F64).float())   # fmaf(scale, j + 0.5f, -0.5f): exact product, one rounding
    src = 0.0 if src < 0.0 else src
    i0 = int(src)
    i1 = i0 + 1 if i0 + 1 < tlen else tlen - 1
    lam = float(torch.tensor(src - i0, dtype=F64).float())
    return min(i0, tin - 1), min(i1, tin - 1), lam


def search_range(row, offs, tps, B):
    """The window whose row range [offs[w], offs[w] + B tps[w]) holds `row` (ranges in any order)."""
    w = 0
    for k in range(len(offs)):
        r = row - offs[k]
        w = k if 0 <= r < B * tps[k] else w
    return w


def search_largest_start(row, offs, tps, B):
    """The search the kernel had before: the largest offs[k] <= row among k >= 1 that is also >= offs[0] -- every row below offs[0]
    goes to window 0.  Kept to show what the short-first cases catch."""
    w = 0
    for k in range(1, len(offs)):
        w = (k if offs[k] >= offs[w] else w) if row >= offs[k] else w
    return w


def emulate_fwd(packed, x, case):
    """window_mix_kernel: one (b, j) at a time over the windows in index order; returns the mixed [B, T, D] in the type of `packed`."""
    lefts, tps, offs, _ = tables(case)
    B, T, ratio, mix = case.B, case.T, case.ratio, case.mix
    out = torch.empty_like(x)
    barange = torch.arange(B)
    for j in range(T):
        acc, cnt = torch.zeros(B, x.shape[-1], dtype=packed.dtype), 0
        for w in range(len(tps)):
            jj, tpw = j - lefts[w], tps[w]
            if jj < 0 or jj >= tpw * ratio:
                continue
            i0, i1, lam = interp_coeff(jj, ratio, tpw, tpw)
            base = offs[w] + barange * tpw
            acc = acc + ((1.0 - lam) * packed[base + i0] + lam * packed[base + i1])
            cnt += 1
        inv = 1.0 / cnt if cnt > 0 else 0.0
        out[:, j] = mix * (acc * inv) + (1.0 - mix) * x[:, j]
    return out


def emulate_bwd(dx, case, search=search_range):
    """window_mix_bwd_kernel: one packed row at a time; returns (dpooled [rows, D], dglobal [B, T, D], owner [rows]) in the type of dx,
    `owner` being the window `search` gave each row."""
    lefts, tps, offs, rows = tables(case)
    B, T, ratio, mix = case.B, case.T, case.ratio, case.mix
    nW = len(tps)
    dpooled = torch.empty(rows, dx.shape[-1], dtype=dx.dtype)
    owner = []
    for row in range(rows):
        w = search(row, offs, tps, B)
        owner.append(w)
        tpw, rel, left = tps[w], row - offs[w], lefts[w]
        b = abs(rel) // tpw * (1 if rel >= 0 else -1)           # C division truncates (rel < 0 only when the search went wrong)
        i = rel - b * tpw
        jlo, jhi = max((i - 1) * ratio - ratio, 0), min((i + 1) * ratio + ratio, tpw * ratio - 1)
        acc = torch.zeros(dx.shape[-1], dtype=dx.dtype)
        for jj in range(jlo, jhi + 1):
            j = left + jj
            if j >= T:
                break
            i0, i1, lam = interp_coeff(jj, ratio, tpw, tpw)
            wgt = (1.0 - lam if i0 == i else 0.0) + (lam if i1 == i else 0.0)
            if wgt == 0.0:
                continue
            cnt = sum(1 for k in range(nW) if 0 <= j - lefts[k] < tps[k] * ratio)
            acc = acc + (wgt * (mix / cnt)) * dx[b % B, j]      # (b >= B only when the search went wrong: keep the read in bounds)
        dpooled[row] = acc
    return dpooled, (1.0 - mix) * dx, owner
