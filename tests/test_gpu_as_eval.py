"""AudioSet-Strong validation on the HIP path: `OvDasmTrainer` against the reference's OV_DASM_Trainer.train (tests/golden/ovstep.npz,
tools/gen_ov_golden.py) and `AudiosetStrongEvaluator` at 407 classes in its three modes."""
import json
import os
import random
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu
DEV = "cuda"

from transformer4sed_amd import synth  # noqa: E402

CNN = dict(n_in_channel=1, activation="cg", conv_dropout=0.0, kernel_size=[3] * 10, padding=[1] * 10, stride=[1] * 10,
           nb_filters=list(synth.PMAM_FILTERS), pooling=[list(p) for p in synth.PMAM_POOLING])
REF_NAME = (("decoder.", "sed_decoder."), ("out_norm.", "norm_before_pool."))


def ref_name(n):
    for mine, ref in REF_NAME:
        if n.startswith(mine):
            return ref + n[len(mine):]
    return n


def build_dasm(depth, nb=8, qdim=1024, sed_head_bias=None, sed_head_scale=1.0):
    from transformer4sed_amd.dasm import DASM
    sd = synth.dasm_full_state_dict_np(n_queries=nb, query_dim=qdim)
    if sed_head_bias is not None:
        sd["sed_head.weight"] = (np.asarray(sd["sed_head.weight"]) * np.float32(sed_head_scale)).astype(np.float32)
        sd["sed_head.bias"] = sed_head_bias
    net = DASM(cnn_param=dict(CNN), backbone_param=dict(embed_dim=768, passt_feature_layer=min(depth, 10), pretrain_model_path=None, lora_config=None),
               at_param=dict(at_decoder_layer=2, query_projector=True, query_dim=qdim, out_type="sigmoid", query=torch.from_numpy(sd["at_query"]).clone()),
               decoder="transformerXL", decoder_layer_num=3, decoder_dim=768, num_heads=12, class_num=nb, _encoder_depth=depth)
    own = net.state_dict()
    net.load_state_dict({k: torch.from_numpy(np.asarray(sd[k])) for k in own if not k.startswith("mel_trans.")}, strict=False)
    net.at_dropout = 0.0
    return net.to(DEV)


def _trainer(g, cls, mask=None):
    from transformer4sed_amd.pmam_trainer import get_param_lr
    from transformer4sed_amd.scheduler import ExponentialDown
    from transformer4sed_amd.trainer import FusedAdamWEMA
    meta = json.loads(str(g["config_json"]))
    cfg, sc = meta["cfg"], meta["sched"]
    net = build_dasm(meta["depth"], sed_head_bias=g["sed_head_bias"], sed_head_scale=float(g["sed_head_scale"]))
    opt = FusedAdamWEMA(net, get_param_lr(net, cfg["opt"]["param_groups"]), ema_net=None, betas=(0.9, 0.999), eps=1e-8)
    sched = ExponentialDown(opt, start_iter=sc["n_epochs_cut"] * sc["epoch_len"], total_iter=sc["n_epochs"] * sc["epoch_len"],
                            exponent=sc["exponent"], warmup_iter=sc["warmup_epochs"] * sc["epoch_len"], warmup_rate=sc["warmup_rate"])
    if mask is None:
        return cls(net, opt, sched, cfg, sr=16000), net, opt, meta
    labels = [f"class_{i}" for i in range(len(mask))]
    td = {l: ("common" if m else "rare") for l, m in zip(labels, mask)}
    return cls(net, opt, sched, cfg, labels=labels, type_dict=td, sr=16000), net, opt, meta


def _batch(meta, step):
    B = meta["B"]
    wav = torch.from_numpy(synth.synth_wav(B, seed=meta["wav_seed0"] + step)).to(DEV)
    labels = torch.from_numpy(synth.synth_strong_labels(B, n_classes=8, seed=meta["label_seed0"] + step)).to(DEV)
    return wav, labels


def test_ov_dasm_trainer_steps_vs_reference_trainer(golden):
    """OvDasmTrainer.step against what the reference's OV_DASM_Trainer.train logged and left behind: loss terms, learning rates, every
    first-step gradient norm (the tolerances of test_gpu_dasm_train's dasmstep test), probes, and `at_query`: its rare rows only decay
    (AdamW with a zero gradient), its common rows train."""
    from transformer4sed_amd.dasm_trainer import OvDasmTrainer
    g = golden("ovstep")
    mask = g["common_mask"].astype(bool)
    tr, net, opt, meta = _trainer(g, OvDasmTrainer, mask)
    assert tr.common_type_mask.cpu().numpy().tolist() == mask.tolist()
    random.seed(meta["seeds"][0]); np.random.seed(meta["seeds"][1]); torch.manual_seed(meta["seeds"][2])
    mine = {ref_name(n): p for n, p in net.named_parameters()}
    names = [str(n) for n in g["probe_names"]]
    gq = [x for x in opt.param_groups if "at_query" in x["names"]][0]
    q0 = g["at_query0"].astype(np.float64)
    assert np.array_equal(net.at_query.detach().cpu().numpy(), g["at_query0"])
    decay = np.ones(1)
    for step in range(meta["steps"]):
        out = tr.step(*_batch(meta, step))
        for k in ("loss_total", "loss_class_strong", "loss_class_at_specific"):
            ref, got = float(g[f"s{step}_{k}"]), float(out[k])
            print(f"ovstep step {step} {k}: got {got:.6f} ref {ref:.6f}")
            assert abs(got - ref) <= 3e-3 * max(abs(ref), 0.05), (step, k, got, ref)
        np.testing.assert_allclose([x["lr"] for x in opt.param_groups], g[f"s{step}_lrs"], rtol=1e-12)
        if step == 0:
            gn = dict(zip((str(n) for n in g["gnorm_names"]), g["gnorm_values"]))
            assert gn["at_query"] > 0
            rows = []
            for n, p in mine.items():
                ref = gn[n]
                if ref < 0:
                    assert p.grad is None, n
                    continue
                got = float(p.grad.norm())
                if n.startswith("cnn.cnn.conv") and n.endswith(".bias"):
                    wn = gn[n[:-4] + "weight"]
                    assert ref < 2e-3 * wn and got < 2e-3 * wn, (n, got, ref, wn)
                    continue
                rows.append((abs(got - ref) / max(ref, 1e-12), n))
            rows.sort(reverse=True)
            print("ovstep: worst gradient-norm errors", [(f"{e:.2e}", n) for e, n in rows[:5]])
            new = ("at_", "query_projector", "mask_embedding_layer", "sed_head", "norm_after_merge", "backbone.blocks", "backbone.norm")
            bad = [(n, f"{e:.2e}") for e, n in rows if e > (3e-3 if n.startswith(new) else 2e-2)]
            assert not bad, bad
            assert sorted(e for e, _ in rows)[len(rows) // 2] < 3e-3
            # the queries' gradient: dense, zero on the rare rows, inside the optimiser's arena
            qg = net.at_query.grad
            assert float(qg[torch.from_numpy(~mask).to(DEV)].abs().max()) == 0.0 and float(qg[torch.from_numpy(mask).to(DEV)].abs().max()) > 0
            o, k = opt.offset["at_query"]
            assert qg.data_ptr() == net._last_grad_arena[o:o + k].data_ptr()
        for i, n in enumerate(names):
            p = mine[n]
            pn = [k for k, v in net.named_parameters() if v is p][0]
            lr = max(x["lr"] for x in opt.param_groups if pn in x["names"])
            ms = float(np.abs(p.detach().reshape(-1)[:256].cpu().numpy() - g[f"s{step}_p{i}"]).mean()) / lr
            assert ms < 0.15, (step, n, ms)
        q = net.at_query.detach().cpu().numpy()
        ref_q = g[f"s{step}_at_query"]
        decay = decay * (1.0 - gq["lr"] * gq["weight_decay"])
        rare = ~mask
        np.testing.assert_allclose(q[rare], ref_q[rare], rtol=1e-6, atol=0)             # weight decay only, as the reference
        np.testing.assert_allclose(q[rare], q0[rare] * decay, rtol=1e-6, atol=0)
        assert float(np.abs(q[mask] - q0[mask] * decay).max()) > 0.1 * gq["lr"]          # the common rows move with their gradient
        ms = float(np.abs(q[mask] - ref_q[mask]).mean()) / gq["lr"]
        assert ms < 0.15, (step, ms)


def test_ov_trainer_all_common_equals_dasm_trainer(golden):
    """With every class common the open-vocabulary step (queries through the external-query path, their gradient moved into the optimiser's
    arena) follows DasmTrainer's step (learned queries) under the same seeds.  The trunk's fp32 atomics make two runs of one trainer differ
    in the last bits, so the bound is that run-to-run spread (2.3e-5 seen on a loss): losses within 1e-4; `at_query` within 5 % of a step's learning rate
    on average over its elements.  (Other tensors with a noise-level gradient -- biases in front of BatchNorm, the K
    bias of an attention -- differ by whole Adam steps from run to run and say nothing about the query path.)"""
    from transformer4sed_amd.dasm_trainer import DasmTrainer, OvDasmTrainer
    g = golden("ovstep")
    runs = []
    for cls, mask in ((DasmTrainer, None), (DasmTrainer, None), (OvDasmTrainer, np.ones(8, bool))):
        tr, net, opt, meta = _trainer(g, cls, mask)
        random.seed(5); np.random.seed(6); torch.manual_seed(7)
        losses = [{k: float(v) for k, v in tr.step(*_batch(meta, s)).items()} for s in range(2)]
        lr = {n: x["lr"] for x in opt.param_groups for n in x["names"]}
        runs.append((losses, {n: p.detach().cpu().clone() for n, p in net.named_parameters()}, lr))
    (l0, p0, lr), (l1, p1, _), (l2, p2, _) = runs
    for other_l, tag in ((l1, "DasmTrainer again"), (l2, "OvDasmTrainer all common")):
        for a, b in zip(l0, other_l):
            assert all(abs(a[k] - b[k]) <= 1e-4 * abs(a[k]) for k in a), (tag, a, b)
    # the queries: the only tensor whose update takes another route (external-query gradient, moved into the arena).  Mean over the
    # elements: one whose gradient is at the noise level of the trunk's atomics can step either way in two runs of the same trainer; a
    # gradient lost on the way (the arena's zeros) moves every element by a whole Adam step or more
    spread = float((p1["at_query"] - p0["at_query"]).abs().mean())
    d = float((p2["at_query"] - p0["at_query"]).abs().mean())
    print(f"at_query after two steps, mean |difference|: OvDasmTrainer vs DasmTrainer {d / lr['at_query']:.3e} x lr, DasmTrainer run to run "
          f"{spread / lr['at_query']:.3e} x lr")
    assert d < 0.05 * lr["at_query"], (d, spread)


@pytest.mark.parametrize("comm", [torch.float32, torch.bfloat16], ids=["fp32-exchange", "bf16-exchange"])
def test_ov_trainer_under_grad_bucket_reducer(golden, comm):
    """OvDasmTrainer with the data-parallel reducer (one gloo rank, collectives forced as the DDP tests do): the queries' gradient reaches
    the arena after the model's stage hooks, so the reducer must leave that slice to `allreduce_grads`.  If a stage hook exchanged it,
    the bf16 path would write the exchanged zeros back over it (and the fp32 path would race the copy); the queries would then only decay.
    Compared with the same steps without the reducer: losses within 1e-4, `at_query` within 5 % of a step's learning rate on average."""
    import torch.distributed as dist
    from transformer4sed_amd.dasm_trainer import OvDasmTrainer
    from transformer4sed_amd.ddp import GradBucketReducer
    g = golden("ovstep")
    mask = g["common_mask"].astype(bool)
    tr, net, opt, meta = _trainer(g, OvDasmTrainer, mask)
    random.seed(5); np.random.seed(6); torch.manual_seed(7)
    plain = [{k: float(v) for k, v in tr.step(*_batch(meta, s)).items()} for s in range(2)]
    q_plain = net.at_query.detach().cpu().clone()
    lr = [x for x in opt.param_groups if "at_query" in x["names"]][0]["lr"]
    import socket
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(sock.getsockname()[1]))
    sock.close()
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        from transformer4sed_amd.pmam_trainer import get_param_lr
        from transformer4sed_amd.scheduler import ExponentialDown
        from transformer4sed_amd.trainer import FusedAdamWEMA
        cfg, sc = meta["cfg"], meta["sched"]
        net2 = build_dasm(meta["depth"], sed_head_bias=g["sed_head_bias"], sed_head_scale=float(g["sed_head_scale"]))
        opt2 = FusedAdamWEMA(net2, get_param_lr(net2, cfg["opt"]["param_groups"]), ema_net=None, betas=(0.9, 0.999), eps=1e-8)
        sched2 = ExponentialDown(opt2, start_iter=sc["n_epochs_cut"] * sc["epoch_len"], total_iter=sc["n_epochs"] * sc["epoch_len"],
                                 exponent=sc["exponent"], warmup_iter=sc["warmup_epochs"] * sc["epoch_len"], warmup_rate=sc["warmup_rate"])
        red = GradBucketReducer(net2, opt2, comm_dtype=comm)
        red.force = True
        labels = [f"class_{i}" for i in range(len(mask))]
        tr2 = OvDasmTrainer(net2, opt2, sched2, cfg, labels=labels, type_dict={l: ("common" if m else "rare") for l, m in zip(labels, mask)},
                            sr=16000, ddp=red)
        o, k = opt2.offset["at_query"]
        assert red.deferred == {"at_query"} and [o, o + (k + 63) // 64 * 64] in red.ranges["deferred"]
        random.seed(5); np.random.seed(6); torch.manual_seed(7)
        dd = [{k_: float(v) for k_, v in tr2.step(*_batch(meta, s)).items()} for s in range(2)]
        assert any(a <= o < b for a, b in red.last_issued)             # exchanged by allreduce_grads, after the move
        red.close()
    finally:
        dist.destroy_process_group()
    for a, b in zip(plain, dd):
        assert all(abs(a[k_] - b[k_]) <= 1e-4 * abs(a[k_]) for k_ in a), (a, b)
    q = net2.at_query.detach().cpu()
    d = (q - q_plain).abs()
    print(f"{comm}: at_query with the reducer vs without: mean {float(d.mean()) / lr:.3e} x lr, max {float(d.max()) / lr:.3e} x lr")
    # (mean, not max: an element whose gradient is at the level of the trunk's fp32-atomics noise can take an Adam step of either sign in
    #  two runs of the same trainer; a zero gradient -- the failure -- leaves every common element a whole step or more away)
    assert float(d.mean()) < 0.05 * lr, float(d.mean()) / lr
    common = torch.from_numpy(mask)
    assert float((q[common] - q_plain[common]).abs().mean()) < 0.05 * lr


# ------------------------------------------------------------------------------------------------------------ evaluator, 407 classes
C = 407


def _ap_restatement():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_gpu_as_ap import ref_per_class
    return ref_per_class


def _encoder():
    from transformer4sed_amd.evaluation import Encoder
    return Encoder([f"/m/{i:04d}" for i in range(C)], audio_len=10, frame_len=1024, frame_hop=320, net_pooling=1, sr=32000)


def _closed_net():
    from transformer4sed_amd.passt_cnn import PaSST_CNN
    passt = dict(passt_feature_layer=2, class_num=C, f_pool="attention", decode_ratio=10, at_adapter=False, decoder="transformerXL",
                 decoder_layer_num=3, decoder_pos_emd_len=1000, decoder_dim=384, mlm=False, load_pretrained_model=False, encoder_depth=2)
    net = PaSST_CNN(passt_sed_param=passt, cnn_param=dict(CNN))
    sd = synth.pmam_state_dict_np(depth=12, mlm=False, lora_r=0, class_num=C)
    own = net.state_dict()
    net.load_state_dict({k: torch.from_numpy(np.asarray(sd[k])) for k in own if k in sd}, strict=False)
    return net.to(DEV)


@pytest.mark.parametrize("mode", ["closed", "dasm", "open_vocabulary"])
def test_audioset_strong_evaluator_407_classes(mode):
    """Two batches through AudiosetStrongEvaluator.  DASM modes: posteriors, weak and tagging outputs against the float64 oracle of the
    query decoder and head (oracle/dasm_oracle.py) run on the frame tokens and SED-decoder output the model handed its head -- in
    open-vocabulary mode with the common-first queries and `dasm_oracle.att_mask`, then un-permuted.  Closed set (PaSST_CNN, no DASM
    head): the model's own forward, i.e. the evaluator's wiring only; that head is pinned by the trainer tests.  Post-processed tables bit-exact with
    scipy's median filter of window [w] * 407 applied to the raw tables; the mAP equal to the torchmetrics restatement of what the evaluator
    fed it; the classes missing from the ground truth dropped from the tables."""
    from scipy import ndimage
    from transformer4sed_amd.evaluation import AudiosetStrongEvaluator
    ref_per_class = _ap_restatement()
    net = _closed_net() if mode == "closed" else build_dasm(2, nb=C)
    name = net.get_model_name()
    cfg = {name: dict(val_kwargs=dict(encoder_win=False, temp_w=0.5), test_kwargs=dict(encoder_win=False, temp_w=0.5),
                      init_kwargs=dict(at_param=dict(out_type="sigmoid"))),
           "training": dict(median_window=7), "feature": dict(pred_len=1000)}
    enc = _encoder()
    rng = np.random.RandomState(3)
    common = rng.rand(C) < 0.6
    td = {l: ("common" if c else "rare") for l, c in zip(enc.labels, common)}
    absent = set(enc.labels[-5:])
    ev = AudiosetStrongEvaluator(net, enc, cfg, mode, type_dict=td, events_set=set(enc.labels) - absent)
    w = int(7 / 156 * 1000)
    assert ev.median_filter == [w] * C
    taps = []
    if mode != "closed":
        from oracle import dasm_oracle
        head_keys = synth.dasm_state_dict_np(n_queries=C, query_dim=1024, at_layers=2).keys()
        own = net.state_dict()
        sd64 = {k: own[k].detach().cpu().double() for k in head_keys}
        orig = net.dasm_head.forward

        def tap(ft, xd, *a, **k):        # what the model hands its query decoder / head
            taps.append((ft.detach().cpu().double(), xd.detach().cpu().double()))
            return orig(ft, xd, *a, **k)
        net.dasm_head.forward = tap
    outs, weak_labels, paths = [], [], []
    for b in range(2):
        wav = torch.from_numpy(synth.synth_wav(2, seed=5100 + b)).to(DEV)
        labels = torch.from_numpy(synth.synth_strong_labels(2, n_classes=C, seed=950 + b)).to(DEV)
        pad = torch.zeros(2, 1000, dtype=torch.bool, device=DEV)
        pth = [f"/data/clip_{b}_{j}.wav" for j in range(2)]
        strong, weak, at_out = ev.step(wav, labels, pad, pth)
        outs.append((strong.cpu(), weak.cpu(), None if at_out is None else at_out.cpu()))
        strong, weak, at_out = outs[-1]
        weak_labels.append((labels.sum(-1) >= 1).cpu().numpy())
        paths += pth
        if mode == "closed":
            with torch.no_grad():
                s2, _, _ = net(net.get_feature_extractor().logmel(wav), pad_mask=pad, encoder_win=False, temp_w=0.5)
            es = float((strong - s2.cpu()).abs().max())
            print(f"closed batch {b}: evaluator vs direct forward, strong {es:.2e}")
            assert es < 1e-3
            continue
        ft, xd = taps.pop()
        assert not taps
        if mode == "open_vocabulary":
            first = np.r_[np.nonzero(common)[0], np.nonzero(~common)[0]]
            q = sd64["at_query"][torch.from_numpy(first)]
            so, wo, ao, _ = dasm_oracle.dasm_head(sd64, ft, xd, query=q, tgt_mask=dasm_oracle.att_mask(C, int(common.sum())), temp_w=0.5,
                                                  pad_mask=pad.cpu(), n_layers=2)
            inv = torch.from_numpy(np.argsort(first, kind="stable"))
            so, wo, ao = so[:, inv], wo[:, inv], ao[:, inv]
        else:
            so, wo, ao, _ = dasm_oracle.dasm_head(sd64, ft, xd, temp_w=0.5, pad_mask=pad.cpu(), n_layers=2)
        es, ew, ea = (float((x_.double() - y_).abs().max()) for x_, y_ in ((strong, so), (weak, wo), (at_out, ao)))
        print(f"{mode} batch {b}: evaluator vs float64 oracle head, strong {es:.2e} weak {ew:.2e} at_out {ea:.2e}")
        assert es < 1e-3 and ew < 1e-3 and ea < 1e-3, (es, ew, ea)
    scores, raw = ev.scores, ev.raw_scores
    assert sorted(scores) == sorted(os.path.splitext(os.path.basename(p))[0] for p in paths)
    for k in scores:
        assert list(scores[k].columns) == ["onset", "offset"] + [l for l in enc.labels if l not in absent]
        r = raw[k][enc.labels].to_numpy().astype(np.float32)
        want = np.stack([ndimage.median_filter(r[:, c], w) for c in range(C)], 1)
        keep = [i for i, l in enumerate(enc.labels) if l not in absent]
        assert np.array_equal(scores[k].iloc[:, 2:].to_numpy().astype(np.float32), want[:, keep]), k
    x = np.concatenate([(o[1] if mode == "closed" else o[2]).numpy() for o in outs])
    t = np.concatenate(weak_labels).astype(np.int64)
    ok = t.sum(0) > 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = float(ev.compute_map())
    want = ref_per_class(x, t)[ok].mean()
    assert abs(got - want) <= 2e-6, (got, want)
    assert ev.mean_psds_per_type({l: 0.5 for l in enc.labels})["common"] == 0.5
