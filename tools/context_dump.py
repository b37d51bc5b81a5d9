"""Context network alone, every branch of its host path at small shapes, dumped as .npy (developer tool; needs a GPU).

Builds the three context networks with synth weights (Transformer-XL and Conformer at 768, PaSST_CNN's 384-wide one), calls the engine's
`_decoder_fwd` / `_conformer_fwd` directly at T = 200 (Tpad = 256: padding, several 64-wide tiles per side of a band), B = 2 (M = 400,
below the two-term in_proj threshold of 1024) and B = 6 (M = 1200, above it), without a window, with one and with per-head widths;
every configuration once with save=False and once with save=True followed by the matching `_bwd`, trainable and frozen.  Writes the
forward outputs, the saved `lse`, the returned input gradient and every parameter gradient of the context network into OUT.

  python tools/context_dump.py OUT [--tree DIR]      (--tree: the checkout put on sys.path -- e.g. a `git worktree` of another commit
                                                       with its own built library; default: this one)
  python tools/context_dump.py --compare A B [C ...] (no GPU: per configuration and tensor class, A against B; with more runs C ... of
                                                       B's tree, the atomically accumulated gradients against that tree's own
                                                       run-to-run spread)

Forward output, lse and input gradient are deterministic (no atomics on that path): two trees that launch the same kernels on the same
arguments give them bit for bit.  One run per process: chain the runs of a comparison with && under their own time limits."""
import os
import sys

import numpy as np

T = 200
HEADS = [40, 100, 400] * 4      # per-head window: narrow, medium, >= 2 T (= no window on that head)
CONFIGS = [("xl", B, win) for B in (2, 6) for win in (None, 100, HEADS)] + [("conformer", B, win) for B in (2, 6) for win in (None, 100)] \
    + [("pmam", B, win) for B in (2, 6) for win in (None, 100)]


def tag_of(kind, B, win):
    return f"{kind}_b{B}_" + ("full" if win is None else "heads" if isinstance(win, list) else f"win{win}")


def compare(a, refs):
    """A against the runs `refs` of the other tree, a row per configuration and tensor class.  Deterministic classes: equal to refs[0]
    or not.  Parameter gradients (atomic accumulation, bf16 casts of atomically accumulated sums): the worst relative difference of A
    to any of `refs` beside the worst between two of `refs`, that tree's own run-to-run spread.  Relative difference of a tensor:
    max|x - y| / max|x|."""
    def rel(x, y):
        return 0.0 if np.array_equal(x, y) else float(np.abs(x - y).max() / max(np.abs(x).max(), 1e-30))
    names = sorted(os.listdir(a))
    assert all(names == sorted(os.listdir(r)) for r in refs), "the runs wrote different sets of files"
    rows = {}
    for n in names:
        cfg, cls = n[:-4].split(".", 1)
        grad = cls.startswith("grad_")
        x = np.load(os.path.join(a, n)).astype(np.float64)
        ys = [np.load(os.path.join(r, n)).astype(np.float64) for r in (refs if grad else refs[:1])]
        r = rows.setdefault((cfg, cls.split(".", 1)[0] if grad else ".".join(cls.split(".")[:2])), [0, 0.0, 0.0])
        r[0] += 1
        r[1] = max([r[1]] + [rel(y, x) for y in ys])
        r[2] = max([r[2]] + [rel(ys[i], ys[j]) for i in range(len(ys)) for j in range(i)])
    bad = 0
    for (cfg, cls), (cnt, d, spread) in sorted(rows.items()):
        if cls.startswith("grad_"):
            over = len(refs) > 1 and d > spread
            print(f"{cfg:20s} {cls:12s} {cnt:3d} tensors  A|refs worst {d:.3e}   refs|refs worst {spread:.3e}" + ("   OVER" if over else ""))
        else:
            over = d > 0.0
            print(f"{cfg:20s} {cls:12s} {cnt:3d} tensors  " + ("NOT EQUAL" if over else "equal"))
        bad += over
    print("result:", "ok" if not bad else f"{bad} rows not equal / over")
    return bad


def main(out, tree):
    sys.path.insert(0, tree)
    import torch
    from transformer4sed_amd import synth
    from transformer4sed_amd.passt_sed import PaSST_SED
    from transformer4sed_amd.passt_cnn import PaSST_CNN
    from transformer4sed_amd.ops import call
    dev = "cuda"
    os.makedirs(out, exist_ok=True)

    def model(kind, win):
        if kind == "pmam":
            passt = dict(class_num=30, f_pool="attention", decode_ratio=10, at_adapter=True, decoder="transformerXL", decoder_layer_num=3,
                         decoder_pos_emd_len=T, decoder_dim=384, mlm=True, lora_config=dict(r=8, lora_alpha=1, requires_grad_pretrain=False),
                         mlm_dict=dict(strategy="block", block_width=10, mask_rate=0.8, out_dim=768, mask_style=[0.9, 0.05, 0.05]),
                         load_pretrained_model=False, passt_feature_layer=2, encoder_depth=2, decoder_win_len=win)
            cnn = dict(n_in_channel=1, activation="cg", conv_dropout=0, kernel_size=[3] * 10, padding=[1] * 10, stride=[1] * 10,
                       nb_filters=list(synth.PMAM_FILTERS), pooling=[list(p) for p in synth.PMAM_POOLING])
            net, sd = PaSST_CNN(passt_sed_param=passt, cnn_param=cnn), synth.pmam_state_dict_np(depth=12)
        else:
            net = PaSST_SED(passt_feature_layer=2, f_pool="mean_pool", decode_ratio=10, at_adapter=True, decoder_layer_num=2,
                            decoder="conformer" if kind == "conformer" else "transformerXL", decoder_pos_emd_len=T,
                            load_pretrained_model=False, encoder_depth=2, decoder_win_len=win)
            sd = (synth.conformer_state_dict_np(dec_layers=2, depth=2) if kind == "conformer" else synth.matsed_state_dict_np(depth=2, dec_layers=2))
        own = net.state_dict()      # (the synth weights carry no window mask: the model's own buffer is the constructor's)
        net.load_state_dict({k: (own[k] if k == "decoder.att_mask" else torch.from_numpy(np.asarray(sd[k]))) for k in own}, strict=True)
        net = net.to(dev).train()
        net.engine = net._make_engine()
        return net

    def save(name, t):
        np.save(os.path.join(out, name + ".npy"), t.detach().float().cpu().numpy())

    for kind, B, win in CONFIGS:
        tag = tag_of(kind, B, win)
        torch.manual_seed(1234)
        net = model(kind, win)
        eng = net.engine
        fwd, bwd = (eng._conformer_fwd, eng._conformer_bwd) if kind == "conformer" else (eng._decoder_fwd, eng._decoder_bwd)
        width = 384 if kind == "pmam" else 768
        g = torch.Generator(device=dev).manual_seed(7)
        x = torch.randn(B, T, width, device=dev, generator=g)
        gout = torch.randn(B, T, width, device=dev, generator=g)
        y, _ = fwd(eng._weights(need_t=False), x, False)
        save(f"{tag}.out.nosave", y)
        for trainable in (True, False):
            grads = {n: torch.zeros_like(p) for n, p in net.named_parameters() if n.startswith("decoder.")} if trainable else {}
            W = eng._weights(need_t=True)
            lease = eng._lease(True)        # (as the full forward does: the saved transposed images come from the engine's pool)
            y, dctx = fwd(W, x, True)
            mode = "train" if trainable else "frozen"
            save(f"{tag}.out.{mode}", y)
            for li, L in enumerate(dctx["layers"]):
                save(f"{tag}.lse.{mode}.{li}", L["lse"])
            scatter = {}
            if kind == "pmam":      # (as PmamEngine._context_bwd: the padded gradient images, returned to the masters after the walk)
                dctx["slots"], scatter = eng._grad_slots(B, torch.device(dev, 0), grads.get, trainable, False)
            gin = bwd(W, dctx, gout.clone(), grads.get, trainable)
            eng._join_dw()
            if "dec" in scatter:
                call("sed_scatter_add_f32", *scatter["dec"])
            torch.cuda.synchronize()
            save(f"{tag}.gin.{mode}", gin)
            for n, t in grads.items():
                save(f"{tag}.grad_{mode}.{n}", t)
            del dctx, lease
        print(tag, "done", flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "--compare":
        sys.exit(1 if compare(a[1], a[2:]) else 0)
    tree = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if "--tree" in a:
        tree = os.path.abspath(a[a.index("--tree") + 1])
        del a[a.index("--tree"):a.index("--tree") + 2]
    main(a[0], tree)
