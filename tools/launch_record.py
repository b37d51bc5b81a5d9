"""Launch record of the engines, for host-side refactors that must not change a launch (developer tool; `record` needs a GPU).

  python tools/launch_record.py record OUT.json [--tree DIR] [--grads FILE.pt]
  python tools/launch_record.py compare NEW.json OLD.json [OLD2.json OLD3.json]

`record` runs depth-2 synthetic-weight models (B = 2, the builders of the GPU tests of the tree DIR, default: this tree) through train steps,
no-grad and scored passes, with `call` wrapped in every loaded transformer4sed_amd module that bound it (each module imports it by name).
Per launch it keeps the entry name, every non-tensor argument, shape / dtype / None-ness of every tensor argument and whether the current
stream is an engine's weight-gradient side stream; per configuration the SHA-256 of every output tensor, and (--grads) the parameter
gradients.  `compare` checks a new record against one to three records of the parent: launches equal one for one (the integer arguments of
the `sed_xattn_f32_*` entries are raw device addresses: listed, not compared), output hashes equal, and every parameter gradient
(atomic accumulation) within twice the parent's own worst pairwise difference -- equal where the parent's runs are equal."""
import argparse
import hashlib
import itertools
import json
import os
import sys

import torch

ADDRESS_ENTRIES = "sed_xattn_f32_"


def record(tree, out_path, grads_path):
    sys.path[:0] = [tree, os.path.join(tree, "tests")]
    os.chdir(tree)
    import transformer4sed_amd
    from transformer4sed_amd import dasm, ops, passt_cnn, passt_sed, pmam_engine, synth        # noqa: F401  (loaded before `call` is wrapped)
    import test_gpu_conformer as TC, test_gpu_dasm_train as TD, test_gpu_fdy_cnn as TF, test_gpu_fpool_transformer as TT
    import test_gpu_model as TM, test_gpu_patchout as TP, test_gpu_pmam as TQ
    assert os.path.dirname(transformer4sed_amd.__file__).startswith(tree), transformer4sed_amd.__file__
    real, records, nets, section = ops.call, [], [], [None]

    def desc(a):
        if torch.is_tensor(a):
            return ["tensor", list(a.shape), str(a.dtype)]
        return a if a is None or isinstance(a, (bool, int, float, str)) else repr(a)

    def recording(name, *args):
        cur = torch.cuda.current_stream()
        side = any(getattr(getattr(n, "engine", None), "_dw_stream", None) == cur for n in nets)
        records.append([section[0], name, bool(side), [desc(a) for a in args]])
        return real(name, *args)
    wrapped = sorted(n for n, mod in sys.modules.items() if n.startswith("transformer4sed_amd") and getattr(mod, "call", None) is real)
    for n in wrapped:
        sys.modules[n].call = recording
    mel = torch.from_numpy(synth.det_uniform("launch_record/mel", (2, 128, 1000), -1.2, 1.2)).cuda()
    results, grads = {}, {}

    def tensors(out, pre=""):
        items = out.items() if isinstance(out, dict) else enumerate(out) if isinstance(out, (tuple, list)) else [("", out)]
        for k, v in items:
            if torch.is_tensor(v):
                yield f"{pre}{k}", v
            elif isinstance(v, (dict, tuple, list)):
                yield from tensors(v, f"{pre}{k}.")

    def run(tag, net, train, grad=None, **kw):
        """One pass of `net` in train / eval mode; `grad` (default: train): with a backward of the sum of every output."""
        if net not in nets:
            nets.append(net)
        section[0] = tag
        torch.manual_seed(1234)
        net.train(train)
        with torch.enable_grad() if (train if grad is None else grad) else torch.no_grad():
            out = list(tensors(net(mel, **kw)))
            diff = [t for _, t in out if t.requires_grad]
            if diff:
                net.zero_grad(set_to_none=True)
                sum(t.float().sum() for t in diff).backward()
        torch.cuda.synchronize()
        results[tag] = {k: hashlib.sha256(t.detach().float().cpu().numpy().tobytes()).hexdigest() for k, t in out}
        if diff and grads_path:
            grads[tag] = {n: p.grad.detach().cpu().clone() for n, p in net.named_parameters() if p.grad is not None}

    win = dict(encoder_win=True, mix_rate=0.5, win_param=[512, 49], temp_w=1)
    net = TM._build(False, 2, 2)[0]          # (every PaSST_SED below has the AT head: at_adapter=True)
    run("xl train windows", net, True, **win)
    run("xl train", net, True, encoder_win=False, temp_w=1)
    run("xl no-grad train-mode", net, True, grad=False, encoder_win=False, temp_w=1)
    run("xl eval windows", net, False, **win)
    net = TC.build_model(False, None)
    run("conformer train windows", net, True, **win)
    run("conformer eval", net, False, encoder_win=False, temp_w=1)
    run("conformer win100 train", TC.build_model(False, 100), True, encoder_win=False, temp_w=1)
    net = TT.build_model()
    run("fpool-transformer train windows", net, True, **win)
    run("fpool-transformer eval windows", net, False, **win)
    net = TP.build_model(s=4)
    run("patchout train windows", net, True, **win)
    run("patchout eval", net, False, encoder_win=False, temp_w=1)
    net = TM._build(True, 2, 2)[0]
    run("mlm pretrain train", net, True, encoder_win=False)
    run("mlm pretrain eval", net, False, encoder_win=False)
    # (the CNN branch's batch statistics are summed with atomics: a train pass, and every pass after it through the running statistics, is
    #  not bit-reproducible between two runs of one tree -- so the scored passes of these models come first)
    net = TQ.build(2, 2)                     # (PaSST_CNN: f_pool="attention", LoRA r = 8, MLM head)
    run("pmam lora eval", net, False, encoder_win=False)
    run("pmam lora train", net, True, encoder_win=False)
    net = TQ.build_ft()
    run("pmam finetune eval windows", net, False, **win)
    run("pmam finetune eval", net, False, encoder_win=False, temp_w=1)
    run("pmam finetune train", net, True, encoder_win=False, temp_w=1)
    run("fdy-cnn pretrain train", TF.build(), True, encoder_win=False)
    net = TF.build(ft=True)
    run("fdy-cnn finetune eval", net, False, encoder_win=False, temp_w=1)
    run("fdy-cnn finetune train", net, True, encoder_win=False, temp_w=1)
    net = TD.build_dasm(2, dropout=0.1)
    run("dasm eval", net, False, temp_w=0.5)
    run("dasm train", net, True, temp_w=0.5)
    with open(out_path, "w") as f:
        json.dump(dict(tree=tree, wrapped=wrapped, records=records, results=results), f)
    if grads_path:
        torch.save(grads, grads_path)
    print(f"{tree}: {len(records)} launches, {sum(r[2] for r in records)} on the side stream, call wrapped in {wrapped}")


def compare(new_path, old_paths):
    load = lambda p: json.load(open(p))
    new, olds = load(new_path), [load(p) for p in old_paths]
    old = olds[0]
    print(f"new tree {new['tree']}: call wrapped in {new['wrapped']}\nold tree {old['tree']}: call wrapped in {old['wrapped']}")
    print(f"records: old {len(old['records'])}, new {len(new['records'])}; on the side stream: old {sum(r[2] for r in old['records'])}, "
          f"new {sum(r[2] for r in new['records'])}")
    bad, addr = 0, []
    for i, (a, b) in enumerate(itertools.zip_longest(new["records"], old["records"])):
        if a is None or b is None or a != b:
            if a and b and a[:3] == b[:3] and a[1].startswith(ADDRESS_ENTRIES) and len(a[3]) == len(b[3]) and all(
                    x == y or (isinstance(x, int) and isinstance(y, int) and not isinstance(x, bool)) for x, y in zip(a[3], b[3])):
                addr.append(f"[{a[0]}] {a[1]}")
                continue
            bad += 1
            if bad <= 20:
                print(f"  launch {i} differs:\n    new {a}\n    old {b}")
    print(f"records that differ in address arguments only: {len(addr)}")
    for line in addr:
        print("  " + line)
    print(f"differing records: {bad}")
    for tag in old["results"]:
        n = sum(r[0] == tag for r in new["records"])
        same = new["results"].get(tag) == old["results"][tag]
        self_same = all(o["results"][tag] == old["results"][tag] for o in olds)
        bad += self_same and not same
        print(f"  [{tag}] {n} launches; {len(old['results'][tag])} output tensors: {'identical' if same else 'DIFFERENT'}"
              f"{'' if self_same else ' (the parent runs differ from each other)'}  sha256 {sorted(old['results'][tag].items())[0][1][:16]}..")
    gfile = lambda p: p[:-5] + ".pt"
    if all(os.path.exists(gfile(p)) for p in [new_path] + old_paths):
        gn, gos = torch.load(gfile(new_path)), [torch.load(gfile(p)) for p in old_paths]

        def worst(a, b):       # over the tensors of one configuration: max |a - b| / max |b|
            assert a.keys() == b.keys()
            return max(float((a[k] - b[k]).abs().max() / b[k].abs().max().clamp_min(1e-30)) for k in a)
        for tag in gos[0]:
            own = max([worst(x[tag], y[tag]) for x, y in itertools.combinations(gos, 2)], default=0.0)
            got = max(worst(gn[tag], o[tag]) for o in gos)
            ok = got <= 2 * own
            bad += not ok
            print(f"  [{tag}] {len(gn[tag])} gradient tensors: new|parent worst {got:.3e}  parent|parent worst {own:.3e}  bound {2 * own:.3e}  "
                  f"{'inside' if ok else 'OVER'}")
    print(f"result: {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["record", "compare"])
    ap.add_argument("files", nargs="+")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--grads", default=None)
    a = ap.parse_args()
    sys.exit(record(os.path.abspath(a.tree), os.path.abspath(a.files[0]), a.grads and os.path.abspath(a.grads)) if a.mode == "record"
             else compare(a.files[0], a.files[1:]))
