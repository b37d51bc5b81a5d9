"""The PMAM tokenizer on an MI355X (csrc/gmm.hip, transformer4sed_amd/tokenizer.py) against the float64 reference of
tests/tokenizer_cases.py.

Bounds.  Mahalanobis terms, the M-step and the fit are held to 4 x the distance of the fp32 numpy restatement of the same quantity from
float64 (computed on the CPU from the same inputs; tests/test_tokenizer_cpu.py prints them and proves that a missing tile, bias, row,
component or log det lies >= 20 x outside).  Posteriors / log-densities of sed_gmm_resp: `score_tolerance` (absolute, derived from the
number format there).  Measured values are appended to test_logs/tokenizer_errors.log.

Launch geometry of sed_gmm_maha: grid (min(ceil(N / 128), 1024), K), 256 threads, a workgroup strides over the 128-row blocks; the case
N = 1024 * 128 + 77 is one row block past a full grid pass."""
import json
import os
import types

import numpy as np
import pytest
import torch

import tokenizer_cases as TC
from transformer4sed_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# measured errors: SED_TEST_LOG_DIR, else test_logs/ at the repository root (kept out of git)
LOG = os.path.join(os.environ.get("SED_TEST_LOG_DIR") or os.path.join(ROOT, "test_logs"), "tokenizer_errors.log")
GUARD = 256


def report(name, err, bound):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(f"{name}: err={err:.4e} bound={bound:.4e}\n")
    print(f"{name}: err={err:.4e} bound={bound:.4e}")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def guarded(n, fill, dtype=torch.float32):
    """-> (whole buffer, the n-element middle of it): GUARD sentinel elements on either side."""
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf, n, fill):
    edge = torch.cat([buf[:GUARD], buf[GUARD + n:]])
    return bool((edge == fill).all())


def pitched(x, ldx):
    """x [N, D] fp32 numpy -> device view [N, D] of row pitch ldx whose pitch gap holds NaN."""
    N, D = x.shape
    buf = torch.full((N, ldx), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :D] = torch.from_numpy(x).to(DEV)
    return buf[:, :D]


# ------------------------------------------------------------------------------------------------------------------ sed_gmm_maha
@pytest.mark.parametrize("D,K,N", TC.MAHA_CASES)
def test_maha_vs_float64(D, K, N):
    from transformer4sed_amd.tokenizer import gmm_maha
    c = TC.maha_case(D, K, N)
    ldx = D + (3 if N % 2 == 0 else 4)          # (even N: rows that are not 16-byte addressable, the element-wise loader)
    x = pitched(c["x"], ldx)
    P, b = dev(c["P"]), dev(c["b"])
    runs = []
    for _ in range(2):
        buf, mid = guarded(N * K, -7.0)
        gmm_maha(x, P, b, out=mid.view(N, K))
        torch.cuda.synchronize()
        assert guards_intact(buf, N * K, -7.0), "wrote outside maha [N, K]"
        runs.append(mid.view(N, K).cpu())
    assert torch.equal(runs[0], runs[1]), "two runs differ"
    got = runs[0].numpy()
    assert np.isfinite(got).all()
    err = TC.rel_err(got, c["ref"])
    report(f"maha D={D} K={K} N={N} ldx={ldx}", err, c["bound"])
    assert err <= c["bound"]


def test_maha_argument_errors():
    from transformer4sed_amd._lib import SedHipError
    from transformer4sed_amd.ops import call
    x = torch.zeros(8, 64, device=DEV)
    P, b, out = torch.zeros(1, 64, 64, device=DEV), torch.zeros(1, 64, device=DEV), torch.zeros(8, 1, device=DEV)
    call("sed_gmm_maha", x, P, b, out, 8, 64, 1, 64)
    for N, D, K, ldx in ((8, 48, 1, 64), (8, 800, 1, 800), (8, 0, 1, 64), (8, 64, 0, 64), (8, 64, 65, 64), (0, 64, 1, 64), (8, 64, 1, 32)):
        with pytest.raises(SedHipError, match="bad argument"):
            call("sed_gmm_maha", x, P, b, out, N, D, K, ldx)
    with pytest.raises(SedHipError, match="bad argument"):
        call("sed_gmm_resp", out, b, None, None, None, None, 1, 8, 65)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ sed_gmm_resp
@pytest.mark.parametrize("D,K,N", TC.POSTERIOR_CASES[:2])
def test_resp_vs_float64_on_overlapping_components(D, K, N):
    from transformer4sed_amd.tokenizer import gmm_resp, resp_blocks
    c = TC.posterior_case(D, K, N)
    tol = c["score_tol"]
    maha, logc = dev(c["maha32"]), dev(c["logc32"])
    outs = []
    for _ in range(2):
        cs = torch.zeros(K, dtype=torch.float64, device=DEV)
        rbuf, rmid = guarded(N * K, -7.0)
        resp, logp, am = gmm_resp(maha, logc, resp=rmid.view(N, K), logp=True, argmax=True, colsum=cs)
        torch.cuda.synchronize()
        assert guards_intact(rbuf, N * K, -7.0)
        outs.append((resp.cpu().clone(), logp.cpu(), am.cpu(), cs.cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a, b), "two runs differ"
    resp, logp, am, cs = (t.numpy() for t in outs[0])
    e_resp, e_logp = float(np.abs(resp - c["resp"]).max()), float(np.abs(logp - c["logp"]).max())
    report(f"resp D={D} K={K} N={N}", e_resp, tol)
    report(f"logp D={D} K={K} N={N}", e_logp, tol)
    assert e_resp <= tol and e_logp <= tol
    s = c["logc32"].astype(np.float64)[None] - 0.5 * c["maha32"].astype(np.float64)
    top2 = np.sort(s, axis=1)[:, -2:]
    decided = (top2[:, 1] - top2[:, 0]) > 2 * tol
    assert decided.mean() > 0.99 and (am[decided] == s.argmax(1)[decided]).all()
    assert ((am >= 0) & (am < K)).all()
    # column sums: a posterior's error is relative (the exponential of a score error), a wave adds ceil(N / (4 blocks)) of them in fp32
    chain = -(-N // (4 * resp_blocks(N)))
    ref_cs = c["resp"].sum(0)
    e_cs = float((np.abs(cs - ref_cs) / ref_cs).max())
    report(f"colsum D={D} K={K} N={N}", e_cs, tol + (chain + 8) * 2.0 ** -24)
    assert e_cs <= tol + (chain + 8) * 2.0 ** -24
    # ... and they are the sums of the posteriors that were written
    assert float((np.abs(cs - resp.astype(np.float64).sum(0)) / ref_cs).max()) <= (chain + 8) * 2.0 ** -24
    # every output is optional
    only = gmm_resp(maha, logc, resp=False, logp=False, argmax=True)
    assert only[0] is None and only[1] is None and torch.equal(only[2].cpu(), outs[0][2])


def test_resp_single_component_and_extreme_rows():
    from transformer4sed_amd.tokenizer import gmm_resp
    N = 1001
    rng = np.random.default_rng(3)
    maha = rng.uniform(0, 900, (N, 1)).astype(np.float32)
    logc = np.array([-31.5], np.float32)
    cs = torch.zeros(1, dtype=torch.float64, device=DEV)
    resp, logp, am = gmm_resp(dev(maha), dev(logc), argmax=True, colsum=cs)
    assert bool((resp == 1.0).all()) and bool((am == 0).all()) and float(cs) == float(N)
    ref = logc.astype(np.float64)[0] - 0.5 * maha[:, 0].astype(np.float64)
    assert np.abs(logp.cpu().numpy() - ref).max() <= TC.score_tolerance(maha, logc)
    # scores further apart than fp32's exponent range (2 * 127 ln 2 = 176): exact one-hot rows, no NaN, log p = the best score
    K = 5
    rows = np.full((4, K), 3.0e38, np.float32)
    rows[0, 2], rows[1, 0], rows[2, 4], rows[3, 1] = 10.0, 0.0, 5000.0, 1.0e30
    rows[3, 3] = 2.0e30
    logc = np.linspace(-3, 1, K).astype(np.float32)
    resp, logp, am = gmm_resp(dev(rows), dev(logc), argmax=True)
    want = np.array([2, 0, 4, 1])
    r = resp.cpu().numpy()
    assert np.isfinite(r).all() and np.isfinite(logp.cpu().numpy()).all()
    assert (r == np.eye(K, dtype=np.float32)[want]).all()
    assert (am.cpu().numpy() == want).all()
    s = logc.astype(np.float64)[None] - 0.5 * rows.astype(np.float64)
    assert np.abs(logp.cpu().numpy() - s.max(1)).max() <= 4 * 2.0 ** -24 * np.abs(s.max(1)).max()


# ------------------------------------------------------------------------------------------------------------------ M-step
def test_center_scale_writes_its_rows_and_nothing_else():
    from transformer4sed_amd.ops import call
    N, D, K, k, ldx = 333, 96, 5, 3, 100
    rng = np.random.default_rng(4)
    x, mu, w = rng.standard_normal((N, D)).astype(np.float32), rng.standard_normal(D).astype(np.float32), rng.uniform(0, 1, (N, K)).astype(np.float32)
    xv, wd, mud = pitched(x, ldx), dev(w), dev(mu)
    buf, mid = guarded(N * D, -7.0)
    call("sed_gmm_center_scale", xv.data_ptr(), mud, wd.data_ptr() + 4 * k, mid, N, D, ldx, K)
    torch.cuda.synchronize()
    assert guards_intact(buf, N * D, -7.0)
    ref = np.sqrt(w[:, k].astype(np.float64))[:, None] * (x.astype(np.float64) - mu.astype(np.float64))
    got = mid.view(N, D).cpu().numpy()
    # sqrt, subtraction and product round once each: 3 x 2^-24 relative (+ one more for a sqrt good to 1 ulp)
    assert (np.abs(got - ref) <= 4 * 2.0 ** -24 * np.abs(ref) + 1e-30).all()


def test_m_step_vs_float64():
    from transformer4sed_amd.tokenizer import GaussianMixtureTokenizer
    ms = TC.mstep_case()
    tok = GaussianMixtureTokenizer(3, covariance_regularization=ms["reg"])
    tok.m_step_from(dev(ms["x"]), dev(ms["resp"]))
    torch.cuda.synchronize()
    got = (tok.weights_.cpu().numpy(), tok.means_.cpu().numpy(), tok.covariances_.cpu().numpy())
    for name, g, r, bound in zip(("weights", "means", "covariances"), got, ms["ref"], ms["bound"]):
        err = TC.scaled_err(g, r)
        bound = max(bound, 1500 * 2.0 ** -53)        # (weights: float64 sums of the same 1500 fp32 posteriors on both sides, in two orders)
        report(f"M-step {name}", err, bound)
        assert err <= bound, name
    assert tuple(tok.means.shape) == (3, 768) and tok.means.dtype == torch.float32


# ------------------------------------------------------------------------------------------------------------------ fit
def test_fit_five_iterations_vs_float64():
    from transformer4sed_amd.tokenizer import GaussianMixtureTokenizer
    fc = TC.fit_case()
    x, init = dev(fc["x"]), dev(fc["init"])
    for it in range(1, TC.FIT_ITERS + 1):
        tok = GaussianMixtureTokenizer(4, covariance_regularization=TC.FIT_REG, convergence_tolerance=0.0, max_iter=it).fit(x, init_means=init)
        assert len(tok.log_likelihood_) == it and not tok.collapsed_
        got = (tok.weights_.cpu().numpy(), tok.means_.cpu().numpy(), tok.covariances_.cpu().numpy())
        for name, g, r, bound in zip(("weights", "means", "covariances"), got, fc["params"][it - 1], fc["pbound"]):
            err = TC.scaled_err(g, r)
            report(f"fit iteration {it} {name}", err, bound)
            assert err <= bound, (it, name)
    ll, ref = np.array(tok.log_likelihood_), np.array(fc["ll"])
    err = float((np.abs(ll - ref) / np.abs(ref)).max())
    report("fit log-likelihood trajectory", err, fc["llbound"])
    assert err <= fc["llbound"]
    assert all(b >= a - fc["llbound"] * abs(a) for a, b in zip(ll, ll[1:])), ll
    # the fitted model's public surface
    p = tok.predict_proba(x)
    assert tuple(p.shape) == (x.shape[0], 4) and float((p.sum(1) - 1).abs().max()) < 1e-5
    assert torch.equal(tok.predict(x), p.argmax(1)) or float((p.gather(1, tok.predict(x)[:, None])[:, 0] - p.max(1).values).abs().max()) == 0
    # (EM never lowers the likelihood: the parameters after the last M-step score at least what the last E-step saw)
    assert float(tok.score_samples(x).double().mean()) >= ll[-1] - fc["llbound"] * abs(ll[-1])
    again = GaussianMixtureTokenizer(4).load_state_dict(tok.state_dict())
    assert torch.equal(again.predict_proba(x), p)
    assert all(type(v) is torch.Tensor for v in tok.state_dict().values())


# ------------------------------------------------------------------------------------------------------------------ k-means
def test_kmeans_assignments_equal_float64_argmin():
    from transformer4sed_amd.tokenizer import KMeansTokenizer, nearest_centre
    km = TC.kmeans_case()
    x = dev(km["x"])
    assert (nearest_centre(x, dev(km["centres"])).cpu().numpy() == km["argmin"]).all()
    assert (nearest_centre(x, dev(km["start"])).cpu().numpy() == km["start_argmin"]).all()
    tok = KMeansTokenizer(7, max_iter=5).fit(x, init_centroids=dev(km["start"]))
    assert (tok.predict(x).cpu().numpy() == km["labels"]).all()
    ref = np.stack([km["x"][km["labels"] == k].astype(np.float64).mean(0) for k in range(7)])
    nk = np.bincount(km["labels"]).max()
    # fp32 sum of n_k terms: at most n_k 2^-24 max|x| per entry, worst case
    assert np.abs(tok.centroids.cpu().numpy() - ref).max() <= nk * 2.0 ** -24 * np.abs(km["x"]).max()
    p = tok.predict_proba(x).cpu().numpy()
    assert (p == np.eye(7, dtype=np.float32)[km["labels"]]).all()
    free = KMeansTokenizer(7, max_iter=8).fit(x, generator=torch.Generator().manual_seed(11))
    assert tuple(free.centroids.shape) == (7, 96) and bool(torch.isfinite(free.centroids).all())


# ------------------------------------------------------------------------------------------------------------------ end to end
def _build_net():
    from transformer4sed_amd.passt_sed import PaSST_SED
    net = PaSST_SED(passt_feature_layer=2, f_pool="mean_pool", decode_ratio=10, at_adapter=True, decoder="transformerXL", decoder_layer_num=3,
                    decoder_pos_emd_len=1000, mlm=False, load_pretrained_model=False, encoder_depth=2)
    sd = synth.matsed_state_dict_np(tag="w768", depth=12, mlm=False)
    own = net.state_dict()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items() if k in own}, strict=True)
    return net.to(DEV)


def test_extract_features_on_passt_cnn(golden):
    """PaSST_CNN projects before it interpolates, so its 768-wide "after_interpolate" sequence is made for the tap alone: against the
    reference's interpolate_module hook of the depth-2 PMAM fixture, within the bound the same hook has on PaSST_SED (2e-2)."""
    import bench
    from transformer4sed_amd.passt_cnn import PaSST_CNN
    g = golden("pmam_d2")
    kw = json.loads(json.dumps(bench.PMAM))["PaSST_CNN"]["init_kwargs"]
    net = PaSST_CNN(passt_sed_param=dict(kw["passt_sed_param"], load_pretrained_model=False, encoder_depth=2, passt_feature_layer=2),
                    cnn_param=kw["cnn_param"])
    sd = synth.pmam_state_dict_np(depth=12)
    net.load_state_dict({k: torch.from_numpy(np.asarray(sd[k])) for k in net.state_dict()}, strict=True)
    net = net.to(DEV).eval()
    mel = torch.from_numpy(synth.det_uniform("pmam_d2/mel", (2, 128, 1000), -1.2, 1.2)).to(DEV)
    feat = net.extract_features(mel, "after_interpolate")
    assert tuple(feat.shape) == (2, 1000, 768) and not net.training
    e = float(np.abs(feat[:, ::25, ::16].double().cpu().numpy() - g["ev_interp_s"]).max())
    report("PaSST_CNN extract_features after_interpolate vs reference", e, 2e-2)
    assert e < 2e-2
    dec = net.extract_features(mel, "transformer_1")
    assert tuple(dec.shape) == (2, 1000, net.decoder_dim) and bool(torch.isfinite(dec).all())


def test_extract_fit_label_train_end_to_end(golden, tmp_path):
    from transformer4sed_amd.data import FrameWiseLabeledDataset
    from transformer4sed_amd.pmam_trainer import PmamTrainer
    from transformer4sed_amd.tokenizer import FeatureExtractor, GaussianMixtureTokenizer, PseudoLabelGenerator, save_prob
    g = golden("model_d768_l2")
    tag = "model_d768_l2"
    mel = torch.from_numpy(synth.det_uniform(f"{tag}/mel", (2, 128, 1000), -1.2, 1.2)).to(DEV)
    net = _build_net()
    net.train()
    S = lambda t: t[:, ::25, ::16].double().cpu().numpy()
    feat = net.extract_features(mel, "after_interpolate")
    assert net.training and net.engine.feature_tap is None and tuple(feat.shape) == (2, 1000, 768) and not feat.requires_grad
    e = float(np.abs(S(feat) - g["interp_s"]).max())
    report("extract_features after_interpolate vs reference", e, 2e-2)
    assert e < 2e-2                                  # (the bound tests/test_gpu_model.py puts on the same sequence)
    dec0 = net.extract_features(mel, "transformer_0")
    e = float(np.abs(S(dec0) - g["dec0_s"]).max())
    report("extract_features transformer_0 vs reference", e, 8e-2)
    assert tuple(dec0.shape) == (2, 1000, 768) and e < 8e-2     # (4 x the bound of its input, as tests/test_oracle_golden.py scales the context blocks)
    with pytest.raises(ValueError):
        net.extract_features(mel, "transformer_3")
    net.eval()
    with torch.no_grad():
        strong, _, other = net(mel, encoder_win=False, temp_w=1)
    # the forward's own outputs are what they were (same kernels on the same input; only the order of split-K atomics may differ)
    assert float((other["frame_before_mask"] - feat).abs().max()) <= 1e-5
    assert float(np.abs(strong.cpu().numpy() - g["strong"]).max()) < 1e-3
    # extract (injected draws) -> fit -> label
    rate = 2
    offs = torch.from_numpy(np.random.default_rng(8).integers(0, rate, 1000))
    feats = FeatureExtractor(net).extract([mel], "after_interpolate", rate, offsets=[offs])
    assert torch.equal(feats, feat.reshape(-1, 768)[torch.arange(0, 2000, rate) + offs])
    assert tuple(FeatureExtractor(net, generator=torch.Generator().manual_seed(1)).extract([(mel, None)], "transformer_1", 10).shape) == (200, 768)
    tok = GaussianMixtureTokenizer(4, covariance_regularization=1e-2, max_iter=3, kmeans_iter=3).fit(feats, generator=torch.Generator().manual_seed(5))
    assert len(tok.log_likelihood_) >= 1 and all(np.isfinite(tok.log_likelihood_))
    prob, names = PseudoLabelGenerator(net, tok).extract([(mel, ["clip_a.wav", "clip_b.wav"])], "after_interpolate")
    assert names == ["clip_a.wav", "clip_b.wav"] and tuple(prob.shape) == (2, 1000, 4)
    assert bool(torch.isfinite(prob).all()) and float((prob.sum(-1) - 1).abs().max()) < 1e-5
    tsv_dir = tmp_path / "labels"
    tsv_dir.mkdir()
    for name, p in zip(names, prob):
        save_prob(str(tsv_dir / name.replace(".wav", ".tsv")), p, sr=100)
    tok.save_means(str(tmp_path / "gmm_means.pt"))
    enc = types.SimpleNamespace(audio_len=10, sr=16000, n_frames=1000, labels=list(range(4)))
    ds = FrameWiseLabeledDataset(str(tsv_dir), str(tmp_path), False, enc)
    by_name = {r[0]: r[2] for r in ds.records}
    labels = torch.stack([by_name[n] for n in names])
    assert tuple(labels.shape) == (2, 4, 1000)
    assert float((labels - prob.transpose(1, 2).cpu()).abs().max()) <= 5e-5 + 1e-7
    # one PMAM step against the new prototypes and labels
    import sys
    sys.path.insert(0, ROOT)
    import bench
    torch.manual_seed(3)
    pnet, opt, wired = bench.build_pmam(2, torch.device(DEV))
    cfg = json.loads(json.dumps(wired.cfg))
    cfg["training"]["w_AT"] = 0          # (the tagging head of the synthetic config has 30 classes; the prototype loss is what is new here)
    means = torch.load(str(tmp_path / "gmm_means.pt"))
    assert tuple(means.shape) == (4, 768)
    trainer = PmamTrainer(pnet, opt, wired.scheduler, means, cfg)
    wav = torch.from_numpy(synth.synth_wav(2, seed=77)).to(DEV)
    out = trainer.step(wav, labels.to(DEV))
    assert np.isfinite(float(out["loss_total"])) and float(out["loss_total"]) > 0
