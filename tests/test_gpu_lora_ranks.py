"""The engine's two LoRA gradient routes at ranks other than 8 (PmamEngine._enc_layer_bwd / _dw_accum, pmam_engine/grads.py): the skinny
products (sed_lora_rowproj + sed_lora_colreduce, r <= 8) and the full-dW scratch that sed_lora_grad projects after the side-stream join
(`lora_skinny` False, or r > 8).  Depth 2, B 2, dropout 0, only the LoRA factors of the encoder trainable, the draws of the pmam_d2 golden.

Four models from the rank-8 synthetic state (A = lora_A [8, in], B = lora_B [out, 8]), all with s = lora_alpha / r = 0.125:
  R8   r 8   the state as it is                      alpha 1
  R16  r 16  A' = [A; 0],      B' = [B, B]           alpha 2
  R4   r 4   A[:4],            B[:, :4]              alpha 0.5
  P8   r 8   [A[:4]; 0],       [B[:, :4], B[:, :4]]  alpha 1
An fma with a zero row of A leaves the accumulator of the weight image as it is, so R16 multiplies with the weights of R8 and P8 with
those of R4, bit for bit, and the gradients obey:  gA'[:r] ~ gA,  gA'[r:] ~ gA (B' repeats B),  gB'[:, :r] ~ gB,  gB'[:, r:] == 0.

Every "~" is max |difference| / max |gradient| per LoRA tensor below 6e-3, the route-agreement bound of test_lora_skinny_gradients
(tests/test_gpu_pmam_kernels.py): the pairs differ by the 16-bit rounding of the fp32 factors in sed_lora_rowproj and by atomic order,
while a wrong index, rank column or a missed join gives errors of order 1.

What is compared is the MEAN gradient of RUNS = 16 runs of each model and route (10 ms a run).  Two runs of ONE model on ONE route are
not equal: float atomics order the forward's and the backward's sums differently, the 16-bit gradient images round the difference up,
and it grows from stage to stage on the way down (measured on identical runs, same ratio: mlm_mlp.2.weight 1e-4, the context network
2e-4 .. 9e-4, the encoder's LoRA factors 4e-4 .. 2.8e-3, the CNN branch up to 1.4e-2).  For the worst LoRA tensor that run-to-run
spread alone was 2.3e-3 .. 3.0e-3 at rank 8 and 3.0e-3 .. 7.8e-3 at rank 4 (30 pairs each), so single runs of the rank-4 models would
cross the bound now and then with nothing wrong.  It is zero-mean noise, a routing fault is not: over 16 runs the noise of a mean
falls to a quarter, and what remains is the difference the bound is about (means of 8: rank 4 against itself 1.2e-3 .. 1.6e-3, skinny
against dW route 3.3e-3 .. 4.0e-3 at rank 4 and 2.6e-3 .. 2.9e-3 at rank 8, over 9 pairs of disjoint groups).  The exact statement
(gB'[:, r:] == 0) is checked in every single run; the two consecutive runs of the join test are single runs (rank 8).
Every observed ratio goes to lora_errors.log in the log directory of the kernel tests (beside kernel_errors.log), the single-run
spread beside it (measured values: profiles/lora_rank_tests.txt)."""
import os

import numpy as np
import pytest
import torch

from transformer4sed_amd import synth

pytestmark = pytest.mark.gpu

from test_gpu_pmam import PASST, CNN, draws  # noqa: E402
from test_gpu_kernels import LOG as KERNEL_LOG  # noqa: E402

BOUND = 6e-3
RUNS = 16
B = 2
LOG = os.path.join(os.path.dirname(KERNEL_LOG), "lora_errors.log")      # (the suite's one log directory)
_MEMO = {}


def log(line):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a" if _MEMO.get("log") else "w") as f:
        f.write(line + "\n")
    _MEMO["log"] = True
    print(line)


def factors(name, A, Bm):
    """(rank, lora_alpha, A', B') of model `name` from the rank-8 factors."""
    z = np.zeros_like
    if name == "R8":
        return 8, 1, A, Bm
    if name == "R16":
        return 16, 2, np.concatenate([A, z(A)]), np.concatenate([Bm, Bm], 1)
    if name == "R4":
        return 4, 0.5, A[:4], Bm[:, :4]
    if name == "P8":
        return 8, 1, np.concatenate([A[:4], z(A[:4])]), np.concatenate([Bm[:, :4], Bm[:, :4]], 1)
    raise KeyError(name)


def model(name):
    if ("net", name) in _MEMO:
        return _MEMO[("net", name)]
    from transformer4sed_amd.passt_cnn import PaSST_CNN
    from transformer4sed_amd.pmam_trainer import mark_only_lora_as_trainable
    if "sd" not in _MEMO:
        _MEMO["sd"] = synth.pmam_state_dict_np(depth=12)
    sd = dict(_MEMO["sd"])
    r, alpha = factors(name, sd["backbone.blocks.0.attn.qkv.lora_A"], sd["backbone.blocks.0.attn.qkv.lora_B"])[:2]
    for k in [k for k in sd if k.endswith(".lora_A")]:
        kb = k[:-1] + "B"
        _, _, sd[k], sd[kb] = factors(name, sd[k], sd[kb])
    lora = dict(r=r, lora_alpha=alpha, requires_grad_pretrain=False)
    net = PaSST_CNN(passt_sed_param=dict(PASST, lora_config=lora, passt_feature_layer=2, encoder_depth=2), cnn_param=dict(CNN, conv_dropout=0.0))
    assert net.lora_r == r and net.lora_scaling == 0.125
    own = net.state_dict()
    net.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(sd[k])) for k in own}, strict=True)
    net = net.cuda()
    mark_only_lora_as_trainable(net.backbone)
    net.train()
    _MEMO[("net", name)] = net
    return net


def lora_names(net):
    return [n for n, _ in net.named_parameters() if n.startswith("backbone.blocks.") and "lora_" in n]


def run(golden, name, skinny, again=0):
    """LoRA gradients {name: tensor} and the loss of one forward + backward of model `name` on the given route (memoised; `again`
    numbers repeated runs of the same model and route)."""
    key = ("run", name, skinny, again)
    if key in _MEMO:
        return _MEMO[key]
    from transformer4sed_amd.pmam_trainer import ProtoBCE
    g = golden("pmam_d2")
    if "in" not in _MEMO:
        mel = torch.from_numpy(synth.det_uniform("pmam_d2/mel", (B, 128, 1000), -1.2, 1.2)).cuda()
        gmm = torch.from_numpy(synth.det_normal("pmam/gmm_means", (30, 768))).cuda()
        labels = torch.from_numpy(synth.synth_strong_labels(B, n_classes=30, seed=500)).cuda()
        _MEMO["in"] = (mel, torch.nn.functional.normalize(gmm, dim=-1), labels)
    mel, protos, labels = _MEMO["in"]
    net = model(name)
    net.zero_grad()
    net._last_grad_arena = None
    if net.engine is None:
        net.engine = net._make_engine()
    net.engine.lora_skinny = skinny
    net._mlm_draws = draws(g, "tr")
    pred, other = net(mel, encoder_win=False)
    loss = ProtoBCE.apply(pred, protos, labels, other["mask_id_seq"].reshape(-1), 0.1) \
        + 0.1 * torch.nn.functional.binary_cross_entropy(other["at_out"], (labels.sum(-1) >= 1).float())
    loss.backward()
    torch.cuda.synchronize()
    pn = dict(net.named_parameters())
    missing = [n for n in lora_names(net) if pn[n].grad is None]
    assert not missing, f"{name} skinny={skinny}: no gradient for {missing}"
    out = ({n: pn[n].grad.detach().clone() for n in lora_names(net)}, float(loss.detach()))
    for n, t in out[0].items():
        assert bool(torch.isfinite(t).all()), (name, skinny, n)
    _MEMO[key] = out
    return out


def mean_grads(golden, name, skinny):
    """The LoRA gradients of model `name` on the given route, averaged over RUNS runs (float64), and the single runs."""
    key = ("mean", name, skinny)
    if key not in _MEMO:
        runs = [run(golden, name, skinny, again=k)[0] for k in range(RUNS)]
        _MEMO[key] = ({n: torch.stack([r[n].double() for r in runs]).mean(0) for n in runs[0]}, runs)
    return _MEMO[key]


def ratio(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def agree(what, got, ref, pick=lambda n, t: t):
    """max |got - ref| / max |ref| per LoRA tensor, logged, all below BOUND; `pick(name, tensor)` cuts the part of `got` to compare."""
    worst = (0.0, "")
    for n, r in ref.items():
        e = ratio(pick(n, got[n]), r)
        log(f"{what:<36} {n:<40} {e:.3e}")
        worst = max(worst, (e, n))
    log(f"{what:<36} {'WORST':<40} {worst[0]:.3e}")
    assert worst[0] < BOUND, (what, worst)
    return worst[0]


def single_run_spread(what, a, b, pick=lambda n, t: t):
    """For the log only: the worst ratio between single runs (run k of one side against run k of the other)."""
    w = [max(ratio(pick(n, x[n]), y[n]) for n in y) for x, y in zip(a, b)]
    log(f"{what:<36} {'single runs, worst tensor: min / max':<40} {min(w):.3e} / {max(w):.3e}")


def test_every_lora_tensor_gets_a_gradient_on_both_routes(golden):
    for name in ("R8", "R4"):
        for skinny in (True, False):
            grads, loss = run(golden, name, skinny)
            assert len(grads) == 2 * 2 * 4 and np.isfinite(loss)          # two blocks x (qkv, proj, fc1, fc2) x (A, B)
            assert all(float(t.abs().max()) > 0 for t in grads.values()), (name, skinny)
    for name, skinny in (("R8", True), ("R8", False), ("R16", False), ("R4", True), ("R4", False), ("P8", True)):
        log(f"loss {name} skinny={skinny}: {run(golden, name, skinny)[1]:.9f}")      # (the same weight images within each triple)


@pytest.mark.parametrize("name", ["R8", "R4"])
def test_skinny_route_against_dw_route(golden, name):
    (a, ra), (b, rb) = mean_grads(golden, name, True), mean_grads(golden, name, False)
    agree(f"{name} skinny vs dW route", a, b)
    single_run_spread(f"{name} skinny vs dW route", ra, rb)


def padded_relations(what, big, small, r):
    """gA'[:r] ~ gA, gA'[r:] ~ gA, gB'[:, :r] ~ gB on the mean gradients; gB'[:, r:] == 0 exactly in every single run."""
    (big, big_runs), (small, small_runs) = big, small
    assert all(t.shape[0 if n.endswith("lora_A") else 1] == 2 * r for n, t in big.items())
    first = lambda n, t: t[:r] if n.endswith("lora_A") else t[:, :r]
    agree(what + ", first half", big, small, first)
    agree(what + ", second half of A", big, {n: t for n, t in small.items() if n.endswith("lora_A")}, lambda n, t: t[r:])
    single_run_spread(what + ", first half", big_runs, small_runs, first)
    for k, g in enumerate(big_runs):
        for n, t in g.items():
            if n.endswith("lora_B"):
                assert not bool(t[:, r:].any()), f"{what}: run {k}: {n}[:, {r}:] must be zero, A' has zero rows there"


def test_rank16_against_rank8(golden):
    """R16 takes the dW route (r > 8) whatever `lora_skinny` says."""
    big = mean_grads(golden, "R16", False)
    padded_relations("R16 vs R8, both dW", big, mean_grads(golden, "R8", False), 8)
    padded_relations("R16 dW vs R8 skinny", big, mean_grads(golden, "R8", True), 8)
    agree("R16 skinny flag on vs off", mean_grads(golden, "R16", True)[0], big[0])


def test_rank4_against_padded_rank8(golden):
    """R4 stages its [K, 4] factor through the general branch of sed_lora_rowproj, P8 through the r == 8 branch; both skinny."""
    padded_relations("P8 vs R4, both skinny", mean_grads(golden, "P8", True), mean_grads(golden, "R4", True), 4)


def test_dw_route_twice_in_one_process(golden):
    """Two dW-route runs in a row, single runs: the second must wait for its OWN scratch.  Between them a NaN-filled copy of the LoRA
    gradients is freed, so the blocks the allocator hands to the second run's scratch tensors hold NaN until that run's own work has
    been written and joined.  (R8 against itself: single runs differ by 2.3e-3 .. 3.0e-3, see the module docstring.)"""
    first = run(golden, "R8", False, again="join 1")[0]
    poison = {n: torch.full_like(t, float("nan")) for n, t in first.items()}
    torch.cuda.synchronize()
    del poison
    second = run(golden, "R8", False, again="join 2")[0]
    agree("R8 dW route, run 2 vs run 1", second, first)


