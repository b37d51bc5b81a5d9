#!/usr/bin/env python
"""Generate tests/golden/segment_scores.npz: the outputs of the REFERENCE's own `get_segment_scores` and
`get_segment_scores_and_overlap_add` (src/codec/decoder.py:138-230) on the inputs of tests/roc_cases.py.  Numbers only: the inputs
(frame scores, frame boundaries, lengths, onsets) and what the reference returned for them.

  * per geometry of roc_cases.GEOMETRIES (156 frames of 64 ms, 1000 frames of 10 ms, the 9.5 s clip): `<name>/scores` [T, 3] f32,
    `<name>/ts` [T + 1] seconds, `<name>/clip` seconds, `<name>/out` [segments, 3] float64, `<name>/out_ts` [segments + 1];
  * the 23.4 s file under 14 sliding clips of 156 frames: `ola/scores` [14, 156, 3] f32, `ola/ts`, `ola/onsets` (seconds),
    `ola/duration`, `ola/out` [24, 3] float64, `ola/out_ts` [25].  Segment length 1.0, the only one the reference's overlap-add pools
    with (decoder.py:178 hard-codes it).

The reference module imports two functions of sed_scores_eval; this tool installs its own stand-in for them before the import
(`validate_score_dataframe` -> (timestamps [T + 1], event classes), which is what decoder.py:212 unpacks).

Run on the authoring machine:  python tools/gen_segment_golden.py --reference <root of the reference tree>
"""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import pandas as pd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import roc_cases as RC  # noqa: E402

CLASSES = ["a", "b", "c"]


def create_score_dataframe(scores, timestamps, event_classes):
    scores, timestamps = np.asarray(scores), np.asarray(timestamps)
    return pd.DataFrame(np.concatenate((timestamps[:-1, None], timestamps[1:, None], scores), axis=1),
                        columns=["onset", "offset", *event_classes])


def validate_score_dataframe(scores, timestamps=None, event_classes=None):
    cols = list(scores.columns)
    assert cols[:2] == ["onset", "offset"]
    on, off = scores["onset"].to_numpy(), scores["offset"].to_numpy()
    assert (on[1:] == off[:-1]).all()
    return np.concatenate((on, off[-1:])), cols[2:]


def reference_decoder(root):
    pkg = types.ModuleType("sed_scores_eval")
    base = types.ModuleType("sed_scores_eval.base_modules")
    mod = types.ModuleType("sed_scores_eval.base_modules.scores")
    mod.create_score_dataframe, mod.validate_score_dataframe = create_score_dataframe, validate_score_dataframe
    pkg.base_modules, base.scores = base, mod
    sys.modules.update({"sed_scores_eval": pkg, "sed_scores_eval.base_modules": base, "sed_scores_eval.base_modules.scores": mod})
    sys.path.insert(0, root)
    return importlib.import_module("src.codec.decoder")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "segment_scores.npz"))
    args = ap.parse_args()
    dec = reference_decoder(args.reference)
    out = {}
    for i, (name, (T, hop, clip)) in enumerate(RC.GEOMETRIES.items()):
        scores, ts = RC.frame_scores(T, len(CLASSES), seed=50 + i), np.arange(T + 1) * hop
        df = dec.get_segment_scores(create_score_dataframe(scores, ts, CLASSES), clip_length=clip, segment_length=1.)
        out.update({f"{name}/scores": scores, f"{name}/ts": ts, f"{name}/clip": np.float64(clip),
                    f"{name}/out": df[CLASSES].to_numpy(dtype=np.float64),
                    f"{name}/out_ts": np.r_[df["onset"].to_numpy(), df["offset"].to_numpy()[-1]]})
    ids, onsets_us, duration = RC.sliding_file()
    T, hop, _ = RC.GEOMETRIES["156x64ms"]
    ts = np.arange(T + 1) * hop
    scores = np.stack([RC.frame_scores(T, len(CLASSES), seed=70 + j) for j in range(len(ids))])
    res = dec.get_segment_scores_and_overlap_add({cid: create_score_dataframe(s, ts, CLASSES) for cid, s in zip(ids, scores)},
                                                 {"long": duration}, CLASSES, segment_length=1.)
    df = res["long"]
    out.update({"ola/scores": scores, "ola/ts": ts, "ola/onsets": np.asarray(onsets_us, dtype=np.float64) / 1e6,
                "ola/duration": np.float64(duration), "ola/out": df[CLASSES].to_numpy(dtype=np.float64),
                "ola/out_ts": np.r_[df["onset"].to_numpy(), df["offset"].to_numpy()[-1]]})
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: " + ", ".join(f"{k} {np.asarray(v).shape}" for k, v in out.items()))


if __name__ == "__main__":
    main()
