"""Steps 1-3 of the PMAM loop on the device, with the arguments of the reference's three scripts
(recipes/desed/pmam/extractor_feature.py, gmm.py, generate_pseudo_label.py):

  extract  --config_dir C --save_folder S --feature_layer L --downsample_rate R [--checkpoint CK]
           frame features of every wav under the config's strong / weak / unlabeled folders -> S/feature_L.pt ([n, C] fp32 tensor)
  fit      --data_path S/feature_L.pt --model_dir M --dim D --algorithm GMM|kmeans --cluster_num K
           -> M/gmm_means.pt (the plain [K, D] tensor the PMAM trainer loads, as the reference writes it) and M/tokenizer.pt (state_dict,
           plain tensors).  --dim below the feature width (PCA) is refused.
  label    --config_dir C --tokenizer_path M/tokenizer.pt --save_dir OUT --feature_layer L [--algorithm GMM|kmeans] [--checkpoint CK]
           -> OUT/<folder key>/<clip>.tsv, the frame-wise label files `FrameWiseLabeledDataset` reads.

C/config.yaml is the reference's YAML: the model under `PaSST_CNN` (or `PaSST_SED`) `.init_kwargs`, wav folders under `dataset`,
`feature.sr` / `feature.audio_max_len` / `generals.batch_size`.  Files the reference pickles (gmm.pkl, pca.pkl, feature pickles) are
neither written nor read: interchange is gmm_means.pt and the TSVs."""
import argparse
import os
import sys
from glob import glob

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TRAIN_FOLDERS = ("strong_folder", "weak_folder", "unlabeled_folder")          # extractor_feature.py:33
LABEL_FOLDERS = TRAIN_FOLDERS + ("val_folder",)                               # generate_pseudo_label.py: every real-data set


class _Clock:
    """What `data.pad_wav` asks of the reference's label encoder: sample rate, clip length, frame count."""

    def __init__(self, sr, audio_len, n_frames):
        self.sr, self.audio_len, self.n_frames, self.labels = sr, audio_len, n_frames, []

    def _time_to_frame(self, t):
        return t * self.n_frames / self.audio_len


def _load(config_dir, checkpoint, device):
    import yaml
    with open(os.path.join(config_dir, "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    if "PaSST_CNN" in cfg:
        from transformer4sed_amd.passt_cnn import PaSST_CNN
        net = PaSST_CNN(**cfg["PaSST_CNN"]["init_kwargs"])
    else:
        from transformer4sed_amd.passt_sed import PaSST_SED
        net = PaSST_SED(**cfg["PaSST_SED"]["init_kwargs"])
    if checkpoint:
        sd = torch.load(checkpoint, map_location="cpu")
        net.load_state_dict(sd.get("state_dict", sd) if isinstance(sd, dict) else sd)
    return cfg, net.to(device).eval()


def _batches(cfg, net, keys, device):
    """yields (folder key, mel [B, 128, T], filenames) over the wav files of the config's folders."""
    from transformer4sed_amd.data import waveform_modification
    sr, audio_len = cfg["feature"]["sr"], cfg["feature"]["audio_max_len"]
    clock = _Clock(sr, audio_len, 1000)
    bs = cfg["generals"]["batch_size"]
    bs = sum(bs) if isinstance(bs, (list, tuple)) else int(bs)
    ext = net.get_feature_extractor()
    for key in keys:
        folder = cfg["dataset"].get(key)
        if not folder:
            continue
        paths = sorted(glob(os.path.join(folder, "*.wav")))
        for i in range(0, len(paths), bs):
            chunk = paths[i:i + bs]
            wav = torch.stack([waveform_modification(p, audio_len * sr, clock, resample_device=device)[0] for p in chunk]).to(device)
            with torch.no_grad():
                yield key, ext.logmel(wav), [os.path.basename(p) for p in chunk]


def cmd_extract(a):
    from transformer4sed_amd.tokenizer import FeatureExtractor
    device = torch.device("cuda", a.gpu)
    cfg, net = _load(a.config_dir, a.checkpoint, device)
    feats = FeatureExtractor(net).extract((mel for _, mel, _ in _batches(cfg, net, TRAIN_FOLDERS, device)), a.feature_layer, a.downsample_rate)
    os.makedirs(a.save_folder, exist_ok=True)
    out = os.path.join(a.save_folder, f"feature_{a.feature_layer}.pt")
    torch.save(feats.cpu(), out)
    print(f"{feats.shape[0]} frames of width {feats.shape[1]} -> {out}")


def make_tokenizer(algorithm, cluster_num, dim=None):
    from transformer4sed_amd.tokenizer import GaussianMixtureTokenizer, KMeansTokenizer
    if algorithm == "GMM":
        return GaussianMixtureTokenizer(cluster_num, batch_size=1_500_000, dim=dim)
    if algorithm.lower() == "kmeans":
        return KMeansTokenizer(cluster_num, dim=dim)
    raise RuntimeError("Unknown algorithm")


def cmd_fit(a):
    data = torch.load(a.data_path, map_location="cpu")
    print(f"length of data is {data.shape[0]}")
    if a.dim is not None and a.dim < data.shape[-1]:
        raise NotImplementedError(f"--dim {a.dim} below the feature width {data.shape[-1]} asks for PCA, which is not implemented: the PMAM "
                                  "pipeline compares the means with full-width logits and never reduces")
    tok = make_tokenizer(a.algorithm, a.cluster_num, a.dim)
    gen = torch.Generator().manual_seed(a.seed)
    data = data[torch.randperm(data.shape[0], generator=gen)].float().to(torch.device("cuda", a.gpu))
    tok.fit(data, generator=gen)
    os.makedirs(a.model_dir, exist_ok=True)
    tok.save_means(os.path.join(a.model_dir, "gmm_means.pt"))
    torch.save(tok.state_dict(), os.path.join(a.model_dir, "tokenizer.pt"))
    if a.algorithm == "GMM":
        print(f"log-likelihood per frame: {tok.log_likelihood_}; converged {tok.converged_}; collapsed components {tok.collapsed_}")


def cmd_label(a):
    from transformer4sed_amd.tokenizer import PseudoLabelGenerator, save_prob
    if a.pca_path is not None:
        raise NotImplementedError("--pca_path: PCA is not implemented (see `fit`)")
    device = torch.device("cuda", a.gpu)
    cfg, net = _load(a.config_dir, a.checkpoint, device)
    sd = torch.load(a.tokenizer_path, map_location="cpu")
    tok = make_tokenizer(a.algorithm, 1).load_state_dict(sd, device=device)
    gen = PseudoLabelGenerator(net, tok)
    n = 0
    for key, mel, names in _batches(cfg, net, LABEL_FOLDERS, device):
        prob, _ = gen.extract([(mel, names)], a.feature_layer)
        out_dir = os.path.join(a.save_dir, key.replace("_folder", ""))
        os.makedirs(out_dir, exist_ok=True)
        for name, p in zip(names, prob.cpu()):
            save_prob(os.path.join(out_dir, name.replace(".wav", ".tsv")), p, sr=100)
            n += 1
    print(f"{n} label files under {a.save_dir}")


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    e = sub.add_parser("extract")
    e.add_argument("--gpu", default=0, type=int)
    e.add_argument("--config_dir", type=str, required=True)
    e.add_argument("--save_folder", type=str, required=True)
    e.add_argument("--feature_layer", type=str, required=True)
    e.add_argument("--downsample_rate", type=int, required=True)
    e.add_argument("--checkpoint", type=str, default=None)
    e.set_defaults(fn=cmd_extract)
    f = sub.add_parser("fit")
    f.add_argument("--gpu", default=0, type=int)
    f.add_argument("--data_path", type=str, required=True)
    f.add_argument("--model_dir", type=str, required=True)
    f.add_argument("--dim", type=int)
    f.add_argument("--algorithm", type=str, default="GMM")
    f.add_argument("--cluster_num", type=int, required=True)
    f.add_argument("--seed", type=int, default=0)
    f.set_defaults(fn=cmd_fit)
    l = sub.add_parser("label")
    l.add_argument("--gpu", default=0, type=int)
    l.add_argument("--config_dir", type=str, required=True)
    l.add_argument("--tokenizer_path", type=str, required=True)
    l.add_argument("--pca_path", type=str, default=None)
    l.add_argument("--save_dir", type=str, required=True)
    l.add_argument("--feature_layer", type=str, required=True)
    l.add_argument("--algorithm", type=str, default="GMM")
    l.add_argument("--checkpoint", type=str, default=None)
    l.set_defaults(fn=cmd_label)
    return ap


if __name__ == "__main__":
    args = parser().parse_args()
    args.fn(args)
