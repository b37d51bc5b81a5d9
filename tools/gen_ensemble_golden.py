#!/usr/bin/env python
"""Generate tests/golden/ensemble.npz: the REFERENCE's own `weighted_average_ensemble` (src/postprocess/ensemble.py:33) on 3 files x 3
members of 40 / 20 / 10 frames (integer ratios: the reference's scale-factor call fails on others), 4 classes, with the weights
0.5 / 0.3 / 0.2 and with 2 / 1 / 1, which do not sum to 1.

The reference is imported through oracle/make_golden.py (which puts it and its third-party stand-ins on sys.path); nothing of it is
copied.  The file holds numbers and names only: the members' tables (`member0` .. `member2` [file, T_m, 2 + C], float64: onset, offset,
scores that are fp32 numbers, as score tables written from fp32 posteriors are), `columns`, `files`, `models`, the two weight sets and the
reference's outputs `out0`, `out1` [file, 40, 2 + C].

An entry whose float64 definition (tests/ensemble_cases.py `combine64`) lies within 1e-6 of a rounding tie (k + 1/2) 1e-4 may come out
one grid step away in fp32; the share of such entries is asserted <= 4 % here (2 % is expected for uniform scores) and stored as
`near_tie_share`; every other entry of the reference's output must be the rounded definition, which is asserted too.

Run on the authoring machine:  python tools/gen_ensemble_golden.py
"""
import os
import sys

import numpy as np
import pandas as pd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from oracle import make_golden as MG  # noqa: E402  (puts the reference and its shims on sys.path)
import ensemble_cases as EC  # noqa: E402

LENGTHS = (40, 20, 10)
FILES = ("clip_a.tsv", "clip_b.tsv", "clip_c.tsv")
MODELS = ("frames40", "frames20", "frames10")
CLASSES = ("Alarm_bell_ringing", "Blender", "Cat", "Dishes")
WEIGHTS = ((0.5, 0.3, 0.2), (2.0, 1.0, 1.0))
CLIP_SECONDS = 10.0
NEAR_TIE_MAX = 0.04


def tables(seed=0):
    rng = np.random.RandomState(9100 + seed)
    out = []
    for T in LENGTHS:
        hop = CLIP_SECONDS / T
        times = np.stack([np.round(hop * np.arange(T), 6), np.round(hop * np.arange(1, T + 1), 6)], axis=1)
        out.append(np.stack([np.concatenate([times, rng.rand(T, len(CLASSES)).astype(np.float32).astype(np.float64)], axis=1)
                             for _ in FILES]))
    return out


def main():
    from src.postprocess.ensemble import weighted_average_ensemble
    columns = ["onset", "offset", *CLASSES]
    members = tables()
    predictions = {f: [(MODELS[m], pd.DataFrame(members[m][j].copy(), columns=columns)) for m in range(len(LENGTHS))]
                   for j, f in enumerate(FILES)}
    arrays = {f"member{m}": members[m] for m in range(len(LENGTHS))}
    share = 0.0
    for k, w in enumerate(WEIGHTS):
        got = weighted_average_ensemble(predictions, np.asarray(w))
        out = np.stack([got[f].values for f in FILES]).astype(np.float64)
        assert out.shape == (len(FILES), LENGTHS[0], len(columns)) and list(got[FILES[0]].columns) == columns
        wn = np.asarray(w, dtype=np.float64) / np.sum(w)
        w32 = np.broadcast_to(wn.astype(np.float32)[None, :, None], (1, len(w), len(CLASSES)))
        y64 = EC.combine64([x[:, :, 2:] for x in members], w32, LENGTHS[0])[0]
        tie = EC.near_tie(y64)
        share = max(share, float(tie.mean()))
        diff = np.abs(out[:, :, 2:] - np.round(y64, 4))
        print(f"weights {w}: near-ties {tie.mean():.4f}; |reference - rounded definition| max {diff[~tie].max():.3g} away from ties, "
              f"{diff.max():.3g} over all entries")
        assert tie.mean() <= NEAR_TIE_MAX, "too many near-ties: change the seed"
        assert diff[~tie].max() <= 1e-12 and diff.max() <= 1e-4 + 1e-12
        assert np.array_equal(out[:, :, :2], np.round(members[0][:, :, :2], 4))
        arrays[f"out{k}"] = out
    MG.save("ensemble", columns=np.asarray(columns), files=np.asarray(FILES), models=np.asarray(MODELS),
            weights=np.asarray(WEIGHTS, dtype=np.float64), near_tie_share=np.float64(share), **arrays)


if __name__ == "__main__":
    main()
