#!/usr/bin/env python
"""Search the per-class post-processing parameters of a trained model on a validation set (transformer4sed_amd.PostprocSearch).

    python tools/tune_postprocess.py --config CONFIG.yaml --checkpoint CK.pt --tsv VAL.tsv --durations VAL_DUR.tsv --wav-dir VAL_WAVS \\
        --out OUT [--objective psds1] [--model student|teacher]

CONFIG.yaml is the recipe's YAML, read as tools/detect.py reads it (model under `PaSST_SED` / `PaSST_CNN`, clock under `feature`,
`training.median_window` -- searched along as the row "config" -- and `training.weak_mask`).  VAL.tsv is the strong ground truth (filename,
onset, offset, event_label), VAL_DUR.tsv the durations (filename, duration); the wav files (16-bit PCM at --sr-in) are looked up in VAL_WAVS
by the file names of VAL_DUR.tsv.  CK.pt is a state dict, a dict holding one under "state_dict", or -- with `--model teacher` -- a dict
holding the EMA weights under "ema_state_dict".  Every batch is read with `data.WavBatchStream`, goes through the frontend and
`net(feat, pad_mask=..., **val_kwargs)`, and its posteriors feed the search on the device.

Prints the table (one row per objective, filter type, candidate[, threshold] and class), and writes OUT/search_table.tsv, one
OUT/choice_<objective>.json per searched objective (what `tools/detect.py --postprocess` takes; `--objective` names the one also written
as OUT/choice.json) and OUT/postprocess.yaml, the fragment for the recipe's `training:` section.

`--sebb` searches sound event bounding boxes instead (transformer4sed_amd.SebbSearch): the candidates are the grid `--step-filter-lengths`
(seconds) x `--merge-thresholds-abs` x `--merge-thresholds-rel`, `--windows` / `--filter-types` play no part, and the choices are
`SebbChoice` files, which `tools/detect.py --postprocess` takes as well."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", required=True)
    ap.add_argument("--checkpoint", default=None, help="without one the model keeps its initial weights")
    ap.add_argument("--model", choices=("student", "teacher"), default="student")
    ap.add_argument("--tsv", required=True, help="strong ground truth of the validation set")
    ap.add_argument("--durations", required=True)
    ap.add_argument("--wav-dir", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--labels", default=None, help="comma-separated class names in the model's order (default: the ten DESED classes)")
    ap.add_argument("--windows", default=None, help="comma-separated candidate windows in the YAML's unit (default: 1,2,3,5,7,10,14,20,28)")
    ap.add_argument("--filter-types", default="median,max")
    ap.add_argument("--objectives", default="psds1,psds2", help="of psds1, psds2, event_f1, segment_f1")
    ap.add_argument("--thresholds", default="0.5", help="comma-separated thresholds of the F1 objectives")
    ap.add_argument("--objective", default=None, help="the objective whose choice becomes choice.json / postprocess.yaml (default: the first)")
    ap.add_argument("--sebb", action="store_true", help="search sound event bounding boxes (a grid of SEBB parameters) instead of filter windows")
    ap.add_argument("--step-filter-lengths", default=None, help="with --sebb: comma-separated seconds (default: 0.32,0.48,0.64)")
    ap.add_argument("--merge-thresholds-abs", default=None, help="with --sebb (default: 0.15,0.2,0.3)")
    ap.add_argument("--merge-thresholds-rel", default=None, help="with --sebb (default: 1.5,2,3)")
    ap.add_argument("--sr-in", type=int, default=16000)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--gpu", type=int, default=0)
    a = ap.parse_args(argv)
    import pandas as pd
    import torch
    import detect
    from transformer4sed_amd import PostprocSearch, SebbSearch
    from transformer4sed_amd.compat.src.utils import load_yaml_with_relative_ref
    from transformer4sed_amd.data import WavBatchStream
    from transformer4sed_amd.evaluation import Encoder
    cfg = load_yaml_with_relative_ref(a.config)
    labels = a.labels.split(",") if a.labels else detect.DESED_LABELS
    f = cfg["feature"]
    enc = Encoder(labels, audio_len=f["audio_max_len"], frame_len=f["win_length"], frame_hop=f["hopsize"], net_pooling=f["net_subsample"],
                  sr=f["sr"])
    device = torch.device("cuda", a.gpu)
    ck = a.checkpoint
    if ck and a.model == "teacher":
        sd = torch.load(ck, map_location="cpu")
        if not isinstance(sd, dict) or "ema_state_dict" not in sd:
            raise SystemExit(f"{ck} holds no 'ema_state_dict': --model teacher needs the EMA weights")
        net = detect.load_model(cfg, None, device)
        net.load_state_dict(sd["ema_state_dict"])
    else:
        net = detect.load_model(cfg, ck, device)
    net.eval()
    ext = net.get_feature_extractor()
    ext.eval()
    kw = cfg[net.get_model_name()]["val_kwargs"]
    tr = cfg.get("training", {})
    objectives = a.objectives.split(",")
    thresholds = [float(v) for v in a.thresholds.split(",")]
    if a.sebb:
        grid = {k: [float(v) for v in given.split(",")] for k, given in (("step_filter_lengths", a.step_filter_lengths),
                                                                         ("merge_thresholds_abs", a.merge_thresholds_abs),
                                                                         ("merge_thresholds_rel", a.merge_thresholds_rel)) if given}
        search = SebbSearch(enc, a.tsv, a.durations, objectives=objectives, thresholds=thresholds, weak_mask=tr.get("weak_mask", False), **grid)
    else:
        search = PostprocSearch(enc, a.tsv, a.durations, objectives=objectives, filter_types=a.filter_types.split(","),
                                thresholds=thresholds, weak_mask=tr.get("weak_mask", False), config_windows=tr.get("median_window"),
                                **({"windows": [float(v) if "." in v else int(v) for v in a.windows.split(",")]} if a.windows else {}))
    names = list(pd.read_csv(a.durations, sep="\t")["filename"])
    paths = [os.path.join(a.wav_dir, n) for n in names]
    batches = [list(range(s, min(s + a.batch_size, len(paths)))) for s in range(0, len(paths), a.batch_size)]
    stream = WavBatchStream(paths, batches, device, sr_in=a.sr_in, sr_out=enc.sr, seconds=int(f["audio_max_len"]), encoder=enc)
    with torch.no_grad():
        for wav, pad_mask, idx in stream:
            strong, weak, _ = net(ext.logmel(wav), pad_mask=pad_mask.to(device), **kw)
            search.update(strong, weak, [names[i] for i in idx])
    os.makedirs(a.out, exist_ok=True)
    table = search.results()
    with pd.option_context("display.max_rows", None, "display.width", 200):
        print(table.to_string(index=False))
    table.to_csv(os.path.join(a.out, "search_table.tsv"), sep="\t", index=False)
    main_objective = a.objective or objectives[0]
    for name in objectives:
        best = search.best(name)
        best.save(os.path.join(a.out, f"choice_{name}.json"))
        if a.sebb:
            what, gain = f"sebb, {best.to_config()['sebb']} = half lengths {best.half_lengths} frames", ""
        else:
            what = f"{best.filter_type}, median_window {best.windows_units} = {best.windows_frames} frames"
            gain = "" if best.config_overall is None else f" (the YAML's own list: {best.config_overall:.4f})"
        print(f"{name}: {what}" + (f", thresholds {best.thresholds}" if best.thresholds is not None else "") + f" -> {best.overall:.4f}{gain}")
        if name == main_objective:
            best.save(os.path.join(a.out, "choice.json"))
            with open(os.path.join(a.out, "postprocess.yaml"), "w") as out:
                out.write(best.to_yaml())


if __name__ == "__main__":
    main()
