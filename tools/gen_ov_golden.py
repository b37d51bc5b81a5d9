#!/usr/bin/env python
"""Generate tests/golden/ovstep.npz: two steps of the REFERENCE's own `OV_DASM_Trainer.train`
(recipes/audioset_strong/detect_any_sound/passt/open_vocabulary.py:34-96) at encoder depth 2, batch 3, 8 queries of which 5 are
"common" -- the open-vocabulary counterpart of oracle/make_golden.py's `dasmstep` (same weights, calibrated sed_head, configuration,
schedule and seeds; built with that file's builders, imported, not copied).

Recorded per step: the logged loss terms, the learning rates, the first 256 elements of the probe parameters and the whole `at_query`
after the step; for the first step the L2 norm of every parameter's gradient.  Each step is one `train()` call over a one-batch loader:
the reference takes the common-query slice once per epoch and backpropagates through it once per batch, so a second batch in one epoch
fails.

Run on the authoring machine (needs the reference tree that oracle/make_golden.py imports):  python tools/gen_ov_golden.py
"""
import json
import os
import random
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import make_golden as MG  # noqa: E402  (puts the reference and its shims on sys.path)
from transformer4sed_amd import synth  # noqa: E402

OV_COMMON = [True, False, True, True, False, True, False, True]      # 5 common classes of 8
DEPTH, B, STEPS = 2, 3, 2


def gen_ov_train():
    from recipes.audioset_strong.detect_any_sound.passt.open_vocabulary import OV_DASM_Trainer
    cfg = json.loads(json.dumps(MG.DASMSTEP_CFG))
    net = MG.build_reference_dasm(DEPTH)
    # the calibrated sed_head of `dasmstep` (make_golden.gen_dasm_train)
    with torch.no_grad():
        net.eval()
        tap = {}
        hnd = net.sed_head.register_forward_hook(lambda m, i, o: tap.update(xin=i[0].detach()))
        ext = net.get_feature_extractor()
        net.sed_head.weight.mul_(MG.DASMSTEP_SED_HEAD_SCALE)
        net(ext.normalize(ext(torch.from_numpy(synth.synth_wav(B, seed=3100)))), temp_w=0.5)
        hnd.remove()
        net.sed_head.bias.copy_(net.sed_head.bias * MG.DASMSTEP_SED_HEAD_SCALE - net.sed_head.weight @ tap["xin"].mean(dim=(0, 1)))
        cal_bias = net.sed_head.bias.detach().clone()
    tr, opt, scalars = MG._dasm_trainer(net, cfg)
    tr.__class__ = OV_DASM_Trainer           # (same constructor; the reference's subclass only adds methods)
    tr._common_type_mask = torch.tensor(OV_COMMON, dtype=torch.bool)
    random.seed(MG.DASMSTEP_SEEDS[0]); np.random.seed(MG.DASMSTEP_SEEDS[1]); torch.manual_seed(MG.DASMSTEP_SEEDS[2])
    names = dict(net.named_parameters())
    probes = [n for n in MG.DASMSTEP_PROBES if n in names]
    out = dict(probe_names=np.array(probes), common_mask=np.array(OV_COMMON), at_query0=MG.t2n(net.at_query).copy())
    gnorms = {}
    o_step = opt.step

    def step_hook(*a, **k):
        if not gnorms:
            for n, p in net.named_parameters():
                gnorms[n] = float(p.grad.norm()) if p.grad is not None else -1.0
        return o_step(*a, **k)
    opt.step = step_hook
    for step in range(STEPS):
        wav = torch.from_numpy(synth.synth_wav(B, seed=3100 + step))
        labels = torch.from_numpy(synth.synth_strong_labels(B, n_classes=8, seed=700 + step))
        tr.train_loader = [(wav, labels, None, None)]
        scalars.append({})
        rec = MG.DrawRecorder()
        with rec.recording():
            tr.train(step)
        for k, v in scalars[-1].items():
            out[f"s{step}_{k}"] = np.float64(v)
        out[f"s{step}_lrs"] = np.array([g["lr"] for g in opt.param_groups], dtype=np.float64)
        out[f"s{step}_draw_kinds"] = np.array([k for k, _ in rec.log])
        sp = dict(net.named_parameters())
        for i, n in enumerate(probes):
            out[f"s{step}_p{i}"] = MG.t2n(sp[n]).reshape(-1)[:256].astype(np.float32).copy()
        out[f"s{step}_at_query"] = MG.t2n(net.at_query).astype(np.float32).copy()
        print(f"   ovstep step {step}: " + " ".join(f"{k}={v:.6f}" for k, v in scalars[-1].items()), flush=True)
    out["sed_head_bias"] = MG.t2n(cal_bias)
    out["sed_head_scale"] = np.float64(MG.DASMSTEP_SED_HEAD_SCALE)
    out["gnorm_names"] = np.array(list(gnorms))
    out["gnorm_values"] = np.array([gnorms[n] for n in gnorms], dtype=np.float64)
    out["group_sizes"] = np.array([len(g["params"]) for g in opt.param_groups])
    out["group_wd"] = np.array([g["weight_decay"] for g in opt.param_groups], dtype=np.float64)
    out["config_json"] = np.array(json.dumps(dict(cfg=MG.DASMSTEP_CFG, sched=MG.DASMSTEP_SCHED, seeds=MG.DASMSTEP_SEEDS, wav_seed0=3100,
                                                  label_seed0=700, depth=DEPTH, B=B, steps=STEPS)))
    MG.save("ovstep", **out)


if __name__ == "__main__":
    gen_ov_train()
