#!/usr/bin/env python
"""Sound event detection on recordings of any length with a trained model (transformer4sed_amd.LongFormDetector).

    python tools/detect.py --config CONFIG.yaml --checkpoint CK.pt --out OUT  a.wav b.wav ...

CONFIG.yaml is the recipe's YAML (with its `include:` of a base file, as the recipes load it): the model under `PaSST_SED` (or `PaSST_CNN`)
`.init_kwargs` with its `val_kwargs`, the clock under `feature` (sr, hopsize, win_length, audio_max_len, net_subsample), and
`training.median_window` / `filter_type` / `weak_mask`.  CK.pt is a state dict, or a dict holding one under "state_dict".  Writes
OUT/scores_raw/<file>.tsv and OUT/scores_post/<file>.tsv (the sed_scores_eval layout `write_sed_scores` writes) and OUT/events.tsv
(event_label, onset, offset, filename).  Files at another sample rate than the model's are resampled on the device.

`--postprocess CHOICE.json` takes the per-class windows (in frames), the filter type and -- where the choice holds them -- the per-class
thresholds that `tools/tune_postprocess.py` searched on a validation set (transformer4sed_amd.PostprocChoice), in place of the YAML's
`median_window` / `filter_type` and of `--threshold`.  A `SebbChoice` (`tools/tune_postprocess.py --sebb`) or a saved `SebbPostprocessor`
is taken as well: the post-processed scores are then the bounding-box scores of the raw timeline and the events the boxes whose
confidence exceeds the threshold.  That path covers recordings of up to 1024 frames (one clip); a longer one is refused."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DESED_LABELS = ["Alarm_bell_ringing", "Blender", "Cat", "Dishes", "Dog", "Electric_shaver_toothbrush", "Frying", "Running_water", "Speech",
                "Vacuum_cleaner"]


def load_model(cfg, checkpoint, device):
    import torch
    if "PaSST_CNN" in cfg:
        from transformer4sed_amd.passt_cnn import PaSST_CNN
        net = PaSST_CNN(**cfg["PaSST_CNN"]["init_kwargs"])
    else:
        from transformer4sed_amd.passt_sed import PaSST_SED
        net = PaSST_SED(**cfg["PaSST_SED"]["init_kwargs"])
    if checkpoint:
        sd = torch.load(checkpoint, map_location="cpu")
        net.load_state_dict(sd.get("state_dict", sd) if isinstance(sd, dict) else sd)
    return net.to(device).eval()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("files", nargs="+", help="wav files (PCM 16 / 24 / 32 bit or float32, any sample rate, any length)")
    ap.add_argument("--config", required=True)
    ap.add_argument("--checkpoint", default=None, help="without one the model keeps its initial weights")
    ap.add_argument("--out", required=True)
    ap.add_argument("--labels", default=None, help="comma-separated class names in the model's order (default: the ten DESED classes)")
    ap.add_argument("--threshold", default="0.5", help="one value, or a comma-separated list with one per class")
    ap.add_argument("--postprocess", default=None, help="a PostprocChoice JSON (tools/tune_postprocess.py): windows, filter type, thresholds; or a SebbChoice / SebbPostprocessor JSON")
    ap.add_argument("--hop-frames", type=int, default=500)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--gpu", type=int, default=0)
    a = ap.parse_args(argv)
    import pandas as pd
    import torch
    from transformer4sed_amd import LongFormDetector
    from transformer4sed_amd.compat.src.utils import load_yaml_with_relative_ref
    from transformer4sed_amd.evaluation import Encoder, write_sed_scores
    cfg = load_yaml_with_relative_ref(a.config)
    labels = a.labels.split(",") if a.labels else DESED_LABELS
    f = cfg["feature"]
    enc = Encoder(labels, audio_len=f["audio_max_len"], frame_len=f["win_length"], frame_hop=f["hopsize"], net_pooling=f["net_subsample"],
                  sr=f["sr"])
    device = torch.device("cuda", a.gpu)
    th = [float(v) for v in a.threshold.split(",")]
    th = th[0] if len(th) == 1 else th
    override, sebb = {}, None
    from transformer4sed_amd.sebb import SEBB_MAX_FRAMES, SebbPostprocessor, is_sebb_file
    if a.postprocess and is_sebb_file(a.postprocess):
        import json
        try:
            sebb = SebbPostprocessor.load(a.postprocess, enc)
        except ValueError as e:
            raise SystemExit(str(e))
        with open(a.postprocess) as saved:
            th = json.load(saved).get("thresholds") or th          # (a SebbChoice of an F1 objective holds per-class thresholds)
    elif a.postprocess:
        from transformer4sed_amd import PostprocChoice
        choice = PostprocChoice.load(a.postprocess)
        if list(choice.labels) != list(labels):
            raise SystemExit(f"{a.postprocess} was searched for the classes {choice.labels}, the model's are {labels}")
        override = dict(median_filter=choice.windows_frames, filter_type=choice.filter_type)
        th = choice.thresholds if choice.thresholds is not None else th
    det = LongFormDetector(load_model(cfg, a.checkpoint, device), enc, cfg, hop_frames=a.hop_frames, batch_size=a.batch_size, **override)
    raw, post, events = {}, {}, []
    for path in a.files:
        wav = det.load(path)
        audio_id = os.path.splitext(os.path.basename(path))[0]
        out = det.posteriors(wav)                    # one pass of the model for the tables and the events
        if sebb is not None:
            if out["raw"].shape[0] > SEBB_MAX_FRAMES:
                raise SystemExit(f"{path}: {out['raw'].shape[0]} frames; bounding boxes cover up to {SEBB_MAX_FRAMES} (long-form is out of scope)")
            out["post"] = sebb.scores_btc(out["raw"][None])[0]
        r, p = det.tables(out, audio_id)
        raw.update(r)
        post.update(p)
        ev = det.events(out, th)
        ev["filename"] = os.path.basename(path)
        events.append(ev)
        print(f"{path}: {wav.numel() / enc.sr:.2f} s, {len(r[audio_id])} frames, {len(ev)} events")
    write_sed_scores(raw, os.path.join(a.out, "scores_raw"))
    write_sed_scores(post, os.path.join(a.out, "scores_post"))
    pd.concat(events, ignore_index=True).to_csv(os.path.join(a.out, "events.tsv"), sep="\t", index=False)


if __name__ == "__main__":
    main()
