"""CPU-side proof of the PMAM tokenizer tests: the float64 reference of tests/tokenizer_cases.py agrees with scikit-learn, the
posterior cases overlap, every mutant of the reference lies far outside the bound the GPU tests use, the bounds themselves (4 x the
fp32 restatement's own error; printed, quoted in DESIGN.md 8), the file round trips and the presence / refusal checks."""
import os
import types
import warnings

import numpy as np
import pytest
import torch

import tokenizer_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- sklearn agreement
def test_reference_predict_proba_agrees_with_sklearn():
    from sklearn.mixture import GaussianMixture
    D, K, N = 32, 3, 300
    means, covs, P, b, logdet = TC.maha_params(D, K)
    rng = np.random.default_rng(5)
    weights = np.array([0.2, 0.5, 0.3])
    x = means[rng.integers(0, K, N)] + 2.0 * rng.standard_normal((N, D))
    gm = GaussianMixture(K, covariance_type="full")
    gm.weights_, gm.means_, gm.covariances_ = weights, means, covs
    gm.precisions_cholesky_ = np.stack([P[k].T for k in range(K)])
    resp, logp = TC.posterior(TC.maha(x, P, b), TC.log_coefficients(weights, logdet, D))
    assert np.abs(resp - gm.predict_proba(x)).max() < 1e-9
    assert np.abs(logp - gm.score_samples(x)).max() < 1e-9 * np.abs(logp).max()


def test_reference_em_agrees_with_sklearn():
    from sklearn.mixture import GaussianMixture
    D, K, N = 32, 4, 4096
    c = TC.overlap_case(D, K, N)
    x = c["x"].astype(np.float64)
    w0, mu0, cov0 = TC.init_from_means(x, c["means"] + 0.05, 1e-6)
    params, ll = TC.em(x, w0, mu0, cov0, 5, 1e-6)
    gm = GaussianMixture(K, covariance_type="full", tol=0.0, reg_covar=1e-6, max_iter=5, n_init=1, weights_init=w0, means_init=mu0,
                         precisions_init=np.stack([np.linalg.inv(cv) for cv in cov0]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gm.fit(x)
    w, mu, cv = params[-1]
    assert gm.n_iter_ == 5
    assert np.abs(w - gm.weights_).max() < 1e-9
    assert np.abs(mu - gm.means_).max() < 1e-9 * np.abs(mu).max()
    assert np.abs(cv - gm.covariances_).max() < 1e-9 * np.abs(cv).max()
    assert abs(ll[-1] - gm.lower_bound_) < 1e-9 * abs(ll[-1])
    assert all(b >= a - 1e-12 for a, b in zip(ll, ll[1:])), ll


# ---------------------------------------------------------------------------------------------------------------- input conditions
@pytest.mark.parametrize("D,K,N", TC.POSTERIOR_CASES)
def test_posterior_cases_overlap(D, K, N):
    c = TC.posterior_case(D, K, N)
    top = c["resp"].max(1)
    frac = float((top < 0.9).mean())
    print(f"posterior case D={D} K={K} N={N}: {100 * frac:.1f} % of rows with largest posterior < 0.9, score tolerance {c['score_tol']:.2e}")
    assert frac >= 0.5
    # arg-max is compared on rows whose two best scores differ by more than twice the score tolerance: nearly all of them
    s = np.sort(c["logc32"].astype(np.float64)[None] - 0.5 * c["maha32"].astype(np.float64), axis=1)
    assert ((s[:, -1] - s[:, -2]) > 2 * c["score_tol"]).mean() > 0.99


def test_kmeans_and_fit_initialisation_are_decided_beyond_fp32():
    km = TC.kmeans_case()
    for pre in ("", "start_"):
        print(f"kmeans {pre or 'centres'}: margin {km[pre + 'margin']:.3e}, fp32 distance error {km[pre + 'dist_err']:.3e}")
        assert km[pre + "margin"] > 2 * TC.BOUND_FACTOR * km[pre + "dist_err"]
        assert (km[pre + "argmin"] == km["labels"]).all()
    fc = TC.fit_case()
    print(f"fit init: margin {fc['init_margin']:.3e}, fp32 distance error {fc['init_dist_err']:.3e}")
    assert fc["init_margin"] > 2 * TC.BOUND_FACTOR * fc["init_dist_err"]


# ---------------------------------------------------------------------------------------------------------------- bounds and mutants
@pytest.mark.parametrize("D,K,N", TC.MAHA_CASES)
def test_maha_bound_and_mutants(D, K, N):
    c = TC.maha_case(D, K, N)
    print(f"maha D={D} K={K} N={N}: fp32 restatement rel err {c['fp32_err']:.3e}, GPU bound {c['bound']:.3e}")
    assert 0 < c["bound"] < 1e-4
    for mutant in TC.MAHA_MUTANTS:
        if not TC.mutant_applies(mutant, D, K, N):
            continue
        moved = TC.rel_err(TC.maha(c["x"], c["P"], c["b"], mutant=mutant), c["ref"])
        assert moved >= TC.MUTANT_FACTOR * c["bound"], (mutant, moved, c["bound"])


def test_every_mutant_is_exercised():
    for mutant in TC.MAHA_MUTANTS:
        assert sum(TC.mutant_applies(mutant, *case) for case in TC.MAHA_CASES) >= 10, mutant


@pytest.mark.parametrize("D,K,N", TC.POSTERIOR_CASES)
def test_logdet_and_component_mutants_move_logp(D, K, N):
    """log p with one component's log det dropped, and with the last component dropped, against the bound the GPU test puts on log p."""
    c = TC.posterior_case(D, K, N)
    m64 = c["maha32"].astype(np.float64)
    logdet = c["logdet"].copy()
    logdet[0] = 0.0
    _, lp_det = TC.posterior(m64, TC.log_coefficients(c["weights"], logdet, D))
    _, lp_comp = TC.posterior(m64[:, :K - 1], c["logc32"].astype(np.float64)[:K - 1])
    for name, lp in (("log det", lp_det), ("last component", lp_comp)):
        moved = float(np.abs(lp - c["logp"]).max())
        assert moved >= TC.MUTANT_FACTOR * c["score_tol"], (name, moved, c["score_tol"])


def test_mstep_and_fit_bounds():
    ms = TC.mstep_case()
    print("M-step D=768 K=3 N=1500: fp32 restatement err (weights, means, covs) " + ", ".join(f"{e:.3e}" for e in ms["fp32_err"]))
    assert ms["fp32_err"][0] == 0.0          # (N_k is a float64 sum of the given fp32 posteriors on both sides)
    assert 0 < ms["bound"][1] < 1e-5 and 0 < ms["bound"][2] < 1e-4
    # a missing row chunk (the last 64 rows) moves the covariances far outside the bound
    cut = TC.m_step(ms["x"][:-64], ms["resp"][:-64], ms["reg"])
    assert TC.scaled_err(cut[2], ms["ref"][2]) >= TC.MUTANT_FACTOR * ms["bound"][2]
    assert TC.scaled_err(cut[1], ms["ref"][1]) >= TC.MUTANT_FACTOR * ms["bound"][1]
    fc = TC.fit_case()
    print("fit D=32 K=4 N=4096: fp32 restatement err per iteration (weights, means, covs) "
          + "; ".join(", ".join(f"{e:.2e}" for e in it) for it in fc["fp32_perr"]))
    print("fit log-likelihood: " + ", ".join(f"{v:.6f}" for v in fc["ll"]) + "; fp32 rel err " + ", ".join(f"{e:.2e}" for e in fc["fp32_llerr"]))
    assert all(0 < b < 1e-3 for b in fc["pbound"]) and 0 < fc["llbound"] < 1e-4
    assert all(b >= a for a, b in zip(fc["ll"], fc["ll"][1:]))
    # the trajectory moves by far more than the bound from one iteration to the next: a skipped iteration cannot pass
    assert abs(fc["ll"][1] - fc["ll"][0]) / abs(fc["ll"][0]) >= TC.MUTANT_FACTOR * fc["llbound"]


# ---------------------------------------------------------------------------------------------------------------- round trips
def test_save_prob_round_trip_through_framewise_dataset(tmp_path):
    from transformer4sed_amd.data import FrameWiseLabeledDataset
    from transformer4sed_amd.tokenizer import save_prob
    K, T = 30, 1000
    prob = TC.posterior(np.random.default_rng(1).uniform(0, 40, (T, K)), np.zeros(K))[0]
    save_prob(str(tmp_path / "clip_a.tsv"), torch.from_numpy(prob), sr=100)
    text = open(tmp_path / "clip_a.tsv").read().splitlines()
    assert text[0].split("\t") == ["onset", "offset"] + [str(k) for k in range(K)]
    assert text[1].split("\t")[:2] == ["0.0", "0.01"] and text[-1].split("\t")[:2] == ["9.99", "10.0"]
    enc = types.SimpleNamespace(audio_len=10, sr=16000, n_frames=T, labels=list(range(K)))
    ds = FrameWiseLabeledDataset(str(tmp_path), str(tmp_path), False, enc)
    assert len(ds) == 1 and ds.records[0][0] == "clip_a.wav"
    label = ds._label(ds.records[0][2])
    assert tuple(label.shape) == (K, T)
    assert float((label.sum(0) - 1).abs().max()) <= K * 5e-5
    assert float((label.double() - torch.from_numpy(prob).T).abs().max()) <= 5e-5 + 1e-7


def test_save_means_round_trip_into_pmam_trainer(tmp_path):
    from transformer4sed_amd.pmam_trainer import PmamTrainer
    from transformer4sed_amd.tokenizer import GaussianMixtureTokenizer
    tok = GaussianMixtureTokenizer(30)
    tok.means_ = torch.from_numpy(np.random.default_rng(2).standard_normal((30, 768)))
    tok.save_means(str(tmp_path / "gmm_means.pt"))
    means = torch.load(str(tmp_path / "gmm_means.pt"))
    assert type(means) is torch.Tensor and means.dtype == torch.float32 and tuple(means.shape) == (30, 768)
    tr = PmamTrainer(torch.nn.Linear(2, 2), None, None, means, {})
    assert tuple(tr.protos.shape) == (30, 768) and float((tr.protos.norm(dim=-1) - 1).abs().max()) < 1e-5


# ---------------------------------------------------------------------------------------------------------------- presence / refusals
def test_entry_points_header_library_sources_and_abi():
    import ctypes
    import re
    from transformer4sed_amd import _lib, build
    protos = _lib.parse_header()
    dll = ctypes.CDLL(build.build(verbose=False))
    for name in ("sed_gmm_maha", "sed_gmm_resp", "sed_gmm_colsum_reduce", "sed_gmm_center_scale"):
        assert name in protos and protos[name][-1] == (ctypes.c_void_p, "stream"), name
        assert hasattr(dll, name), name
    assert "gmm.hip" in build.SOURCES
    header = open(os.path.join(ROOT, "include", "sed_hip.h")).read()
    assert int(re.search(r"#define\s+SED_HIP_ABI_VERSION\s+(\d+)", header).group(1)) == 7
    assert dll.sed_abi_version(0) == 7


def test_package_exports_and_refusals():
    import transformer4sed_amd as pkg
    from transformer4sed_amd import tokenizer
    for name in ("GaussianMixtureTokenizer", "KMeansTokenizer", "FeatureExtractor", "PseudoLabelGenerator", "save_prob"):
        assert getattr(pkg, name) is getattr(tokenizer, name)
    with pytest.raises(RuntimeError, match="MI355X|no CPU"):
        tokenizer.GaussianMixtureTokenizer(4).fit(torch.zeros(16, 32))
    from transformer4sed_amd.passt_sed import PaSST_SED
    assert callable(PaSST_SED.extract_features)
    with pytest.raises(ValueError):
        tokenizer.GaussianMixtureTokenizer(65)


@pytest.mark.parametrize("cls", ["GaussianMixtureTokenizer", "KMeansTokenizer"])
def test_pca_request_is_refused(cls, monkeypatch):
    from transformer4sed_amd import tokenizer
    # (the width check precedes every launch; the device check is taken out so that the refusal itself is what is observed here)
    monkeypatch.setattr(tokenizer, "_rows", lambda x: (x, x.shape[0], x.shape[1], x.stride(0)))
    tok = getattr(tokenizer, cls)(4, dim=16)
    with pytest.raises(NotImplementedError, match="PCA"):
        tok.fit(torch.zeros(64, 32))
