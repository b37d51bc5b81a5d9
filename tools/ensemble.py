#!/usr/bin/env python
"""Combine the frame scores of several systems, or search the weights that do it best (transformer4sed_amd/ensemble.py).

    python tools/ensemble.py combine DIR [DIR ...] --weights 0.7,0.3 --out OUT [--mode mean|logit]
    python tools/ensemble.py search DIR [DIR ...] --ground-truth VAL.tsv --durations VAL_DUR.tsv --config CONFIG.yaml --out choice.json \\
        [--step 0.1] [--weights 0.7,0.3[;0.6,0.4]] [--mode mean|logit] [--objectives psds1,psds2] [--objective psds1] [--thresholds 0.5] \\
        [--no-filter]

Every DIR is one system's folder of score tables, one <clip>.tsv per clip with the columns onset, offset and one column per class, as
`batched_decode_preds` and sed_scores_eval write them -- from any framework and at any frame rate; all folders must hold the same files.

`combine` is src/postprocess/ensemble.py of the reference: the weighted mean at the frame rate of the longest member, 4 decimals, onset /
offset of the longest member, written to OUT/<clip>.tsv.

`search` feeds the folders to an `EnsembleSearch`: CONFIG.yaml gives the frame clock (`feature`) and the post-processing every candidate
row goes through (`training.median_window`, `filter_type`; `--no-filter` leaves it out).  The folders hold no clip-level scores, so the
weak prediction of a member is its greatest frame score per clip and class -- the event path's mask weak >= threshold then removes
nothing a threshold would keep -- and the soft weak mask is off.  Prints the table and writes the choice of `--objective` (default: the
first objective) as JSON, next to it <stem>_<objective>.json for every objective and <stem>_table.tsv."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _rows(text):
    return [[float(v) for v in row.split(",")] for row in text.split(";")]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)
    c = sub.add_parser("combine")
    c.add_argument("dirs", nargs="+")
    c.add_argument("--weights", required=True, help="comma-separated, one per folder (divided by their sum)")
    c.add_argument("--out", required=True)
    c.add_argument("--mode", choices=("mean", "logit"), default="mean")
    s = sub.add_parser("search")
    s.add_argument("dirs", nargs="+")
    s.add_argument("--ground-truth", required=True, help="strong ground truth (filename, onset, offset, event_label)")
    s.add_argument("--durations", required=True)
    s.add_argument("--config", required=True)
    s.add_argument("--out", required=True, help="the choice's JSON file")
    s.add_argument("--step", type=float, default=0.1)
    s.add_argument("--weights", default=None, help="explicit rows next to the grid: comma-separated weights, rows separated by ';'")
    s.add_argument("--mode", choices=("mean", "logit"), default="mean")
    s.add_argument("--objectives", default="psds1,psds2", help="of psds1, psds2, event_f1, segment_f1")
    s.add_argument("--objective", default=None)
    s.add_argument("--thresholds", default="0.5")
    s.add_argument("--no-filter", action="store_true")
    s.add_argument("--batch-size", type=int, default=32)
    s.add_argument("--gpu", type=int, default=0)
    a = ap.parse_args(argv)
    import numpy as np
    import pandas as pd
    import torch
    from transformer4sed_amd import ensemble as E
    if a.command == "combine":
        weights = _rows(a.weights)[0]
        if len(weights) != len(a.dirs):
            raise SystemExit("The number of weights must match the number of folders.")
        E.save_predictions(E.weighted_average_ensemble(E.load_predictions(a.dirs), weights, mode=a.mode), a.out)
        print(f"wrote {len(os.listdir(a.out))} tables to {a.out}")
        return
    from transformer4sed_amd.compat.src.utils import load_yaml_with_relative_ref
    from transformer4sed_amd.evaluation import Encoder
    from transformer4sed_amd.ops import h2d
    cfg = load_yaml_with_relative_ref(a.config)
    predictions = E.load_predictions(a.dirs)
    files = list(predictions)
    if not files:
        raise SystemExit("the folders hold no .tsv file")
    labels = list(predictions[files[0]][0][1].columns[2:])
    f = cfg["feature"]
    enc = Encoder(labels, audio_len=f["audio_max_len"], frame_len=f["win_length"], frame_hop=f["hopsize"], net_pooling=f["net_subsample"],
                  sr=f["sr"])
    tr = cfg.get("training", {})
    objectives = a.objectives.split(",")
    search = E.EnsembleSearch(enc, a.ground_truth, a.durations, len(a.dirs), step=a.step, weights=_rows(a.weights) if a.weights else None,
                              mode=a.mode, objectives=objectives, thresholds=[float(v) for v in a.thresholds.split(",")],
                              median_window=None if a.no_filter else tr.get("median_window"), filter_type=tr.get("filter_type", "median"))
    device = torch.device("cuda", a.gpu)
    for lo in range(0, len(files), a.batch_size):
        batch = files[lo:lo + a.batch_size]
        strongs = []
        for m in range(len(a.dirs)):
            x = np.stack([predictions[file][m][1].values[:, 2:].astype(np.float32).T for file in batch])       # [n, C, T_m]
            strongs.append(h2d(np.ascontiguousarray(x), torch.float32, device))
        search.update(strongs, [x.amax(dim=2) for x in strongs], [os.path.splitext(file)[0] + ".wav" for file in batch])
    table = search.results()
    with pd.option_context("display.max_rows", None, "display.width", 200):
        print(table.to_string(index=False))
    stem = os.path.splitext(a.out)[0]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    table.to_csv(stem + "_table.tsv", sep="\t", index=False)
    for name in objectives:
        best = search.best(name)
        best.save(f"{stem}_{name}.json")
        if name == (a.objective or objectives[0]):
            best.save(a.out)
        print(f"{name}: rows {best.rows}" + (f", thresholds {best.thresholds}" if best.thresholds is not None else "")
              + f" -> {best.overall:.4f} (each member alone: {', '.join(f'{v:.4f}' for v in best.member_overall)})")


if __name__ == "__main__":
    main()
