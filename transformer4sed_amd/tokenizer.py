"""The PMAM tokenizer on the device: steps 1-3 of the prototype-modelling loop (recipes/desed/pmam/extractor_feature.py, gmm.py,
generate_pseudo_label.py), which the reference runs on pycave.

`GaussianMixtureTokenizer`   full-covariance Gaussian mixture fitted by EM over row chunks; the densities of every frame under every
                             component come from `sed_gmm_maha` (fp32-input MFMA against the inverse Cholesky factors), posteriors /
                             log-likelihood / N_k from `sed_gmm_resp`, the M-step's products from `sed_gemm_f32`.  Parameters live in
                             float64 on the device; Cholesky and the triangular inverse run in float64 through torch.linalg.
`KMeansTokenizer`            Lloyd iterations on the same kernels (distances = `sed_gemm_f32_nt` with B = -2 C and bias |c|^2).
`FeatureExtractor`           `sample_feature` (extractor_feature.py:64-69) over `net.extract_features`, features stay on the device.
`PseudoLabelGenerator`       frame posteriors of every clip, `save_prob` writes the reference's TSV (generate_pseudo_label.py:132-141),
                             which `data.FrameWiseLabeledDataset` reads.
Interchange with the reference is `gmm_means.pt` (`save_means`) and the TSVs; its pickled pycave objects are not read.  Parity with
pycave's own fit is NOT pinned (pycave is not available to the tests): what is pinned is float64 EM and scikit-learn."""
import math

import torch

from .ops import call

F32, F64 = torch.float32, torch.float64
MAX_RESP_BLOCKS = 1024          # workgroups of sed_gmm_resp (4 rows each per pass): fixes the order of the N_k sums for a given N
MSTEP_ROWS = 262144             # rows of the centred / scaled operand A of the covariance product held at a time
DIST_ROWS = 1 << 20            # rows of one k-means distance product (sed_gemm_f32 puts its 64-row tiles on grid.y)
TINY_NK = 10.0 * torch.finfo(torch.float32).eps     # an N_k at or below this has underflowed: the component keeps its parameters


def _rows(x):
    """x [N, D] fp32 on the device with unit column stride (any row pitch) -> (x, N, D, ldx)."""
    if not x.is_cuda:
        raise RuntimeError("the tokenizer runs on MI355X only: move the features to 'cuda'.  There is no CPU path.")
    if x.dim() != 2 or x.dtype != F32 or x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        raise ValueError("features must be an fp32 [N, D] tensor with contiguous rows")
    return x, x.shape[0], x.shape[1], x.stride(0)


def gmm_maha(x, P, b, out=None):
    """maha[n, k] = |P_k x_n + b_k|^2 (`sed_gmm_maha`): x [N, D] fp32 (rows may be pitched), P [K, D, D] lower triangular, b [K, D]."""
    x, N, D, ldx = _rows(x)
    K = P.shape[0]
    if out is None:
        out = torch.empty(N, K, dtype=F32, device=x.device)
    call("sed_gmm_maha", x.data_ptr(), P, b, out, N, D, K, ldx)
    return out


def resp_blocks(N):
    return max(1, min((N + 3) // 4, MAX_RESP_BLOCKS))


def gmm_resp(maha, logc, resp=True, logp=True, argmax=False, colsum=None, accumulate=False):
    """Posteriors of `sed_gmm_resp` from maha [N, K] and logc [K].  Returns (resp | None, logp | None, argmax | None); `colsum`: a float64
    [K] tensor that receives (accumulate: is increased by) the column sums of resp, added in a fixed order."""
    N, K = maha.shape
    dev = maha.device
    r = torch.empty(N, K, dtype=F32, device=dev) if resp is True else (resp if torch.is_tensor(resp) else None)
    lp = torch.empty(N, dtype=F32, device=dev) if logp else None
    am = torch.empty(N, dtype=torch.int32, device=dev) if argmax else None
    nb = resp_blocks(N)
    part = torch.empty(nb, K, dtype=F32, device=dev) if colsum is not None else None
    call("sed_gmm_resp", maha, logc, r, lp, am, part, nb, N, K)
    if colsum is not None:
        call("sed_gmm_colsum_reduce", part, nb, K, colsum, int(bool(accumulate)))
    return r, lp, am


def _ksplit(tiles, rows):
    """Split of the contraction (the rows) of a transposed product: enough workgroups to fill 256 CUs twice."""
    return max(1, min(512 // max(tiles, 1), rows // 256, 65535))


def _accum_tn(A, lda, B, ldb, C, M, N, rows):
    """C[M, N] += A[rows, M]^T . B[rows, N] on `sed_gemm_f32` (transA = transB = 1, accumulating)."""
    tiles = ((M + 63) // 64) * ((N + 63) // 64)
    call("sed_gemm_f32", A, B, None, None, C, None, M, N, rows, lda, ldb, C.stride(0), 1, 1, 1, 0, 0, 0, 0, 1, _ksplit(tiles, rows), 0.0, 0, 0)


def nearest_centre(x, centres):
    """Index of the nearest centre of every row (int32 [N]): |c|^2 - 2 x.c from `sed_gemm_f32_nt` (B = -2 C, bias = |c|^2), whose arg-min is
    the arg-max `sed_gmm_resp` takes with logc = 0."""
    x, N, D, ldx = _rows(x)
    K = centres.shape[0]
    c = centres.to(F32).contiguous()
    B = (-2.0 * c).contiguous()
    bias = (c.double() ** 2).sum(1).to(F32).contiguous()
    zero = torch.zeros(K, dtype=F32, device=x.device)
    labels = torch.empty(N, dtype=torch.int32, device=x.device)
    rows = min(N, DIST_ROWS)
    dist = torch.empty(rows, K, dtype=F32, device=x.device)
    for r0 in range(0, N, rows):
        n = min(rows, N - r0)
        call("sed_gemm_f32_nt", x.data_ptr() + 4 * r0 * ldx, B, bias, None, dist, n, K, D, ldx, D, K, 1, 0, 0, 0, 0)
        labels[r0:r0 + n] = gmm_resp(dist[:n], zero, resp=False, logp=False, argmax=True)[2]
    return labels


def weighted_sums(x, resp):
    """R^T X [K, D] fp32 over all rows."""
    x, N, D, ldx = _rows(x)
    K = resp.shape[1]
    sums = torch.zeros(K, D, dtype=F32, device=x.device)
    _accum_tn(resp, K, x.data_ptr(), ldx, sums, K, D, N)
    return sums


def weighted_scatter(x, resp, k, mu, scratch=None):
    """sum_n r_nk (x_n - mu)(x_n - mu)^T [D, D] fp32: `sed_gmm_center_scale` into A, then A^T A, over row chunks."""
    x, N, D, ldx = _rows(x)
    K = resp.shape[1]
    S = torch.zeros(D, D, dtype=F32, device=x.device)
    rows = min(N, MSTEP_ROWS)
    A = scratch if scratch is not None else torch.empty(rows, D, dtype=F32, device=x.device)
    mu32 = mu.to(F32).contiguous()
    for r0 in range(0, N, rows):
        n = min(rows, N - r0)
        call("sed_gmm_center_scale", x.data_ptr() + 4 * r0 * ldx, mu32, resp.data_ptr() + 4 * (r0 * K + k), A, n, D, ldx, K)
        _accum_tn(A, D, A, D, S, D, D, n)
    return S


class GaussianMixtureTokenizer:
    """Full-covariance Gaussian mixture (pycave's `GaussianMixture(num_components, covariance_type="full")` as recipes/desed/pmam/gmm.py
    uses it; the three numeric defaults are pycave's as far as they are known here)."""

    def __init__(self, num_components, covariance_regularization=1e-6, convergence_tolerance=1e-3, max_iter=100, batch_size=1_500_000,
                 kmeans_iter=10, dim=None):
        if not 1 <= int(num_components) <= 64:
            raise ValueError("num_components must lie in 1 .. 64")
        self.num_components = int(num_components)
        self.reg, self.tol, self.max_iter = float(covariance_regularization), float(convergence_tolerance), int(max_iter)
        self.batch_size, self.kmeans_iter, self.dim = int(batch_size), int(kmeans_iter), dim
        self.weights_ = self.means_ = self.covariances_ = None
        self.log_likelihood_, self.collapsed_, self.converged_ = [], [], False
        self._P = self._b = self._logc = None

    # ------------------------------------------------------------------ parameters
    @property
    def means(self):
        return self.means_.to(F32)

    def save_means(self, path):
        """What the reference's `gmm_means.pt` holds: the plain [K, D] fp32 tensor `PmamTrainer(gmm_means=...)` takes."""
        torch.save(self.means.cpu(), path)

    def state_dict(self):
        return {"weights": self.weights_.cpu(), "means": self.means_.cpu(), "covariances": self.covariances_.cpu()}

    def load_state_dict(self, sd, device="cuda"):
        self.weights_, self.means_, self.covariances_ = (sd[k].to(device=device, dtype=F64) for k in ("weights", "means", "covariances"))
        self.num_components = self.means_.shape[0]
        self._prepare()
        return self

    def _prepare(self, keep=()):
        """Covariances -> the operands of the E-step: P_k = L_k^-1, b_k = -P_k mu_k, logc_k.  float64 on the device, cast once.  `keep`:
        components whose operands stay as they are."""
        K, D = self.means_.shape
        L = torch.linalg.cholesky(self.covariances_)
        eye = torch.eye(D, dtype=F64, device=L.device).expand(K, D, D)
        Linv = torch.linalg.solve_triangular(L, eye, upper=False).tril()
        logdet = 2.0 * torch.log(torch.diagonal(L, dim1=1, dim2=2)).sum(1)
        logc = torch.log(self.weights_.clamp_min(1e-300)) - 0.5 * (D * math.log(2.0 * math.pi) + logdet)
        P, b, lc = Linv.to(F32).contiguous(), (-(Linv @ self.means_.unsqueeze(2)).squeeze(2)).to(F32).contiguous(), logc.to(F32).contiguous()
        for k in keep:
            P[k], b[k] = self._P[k], self._b[k]
        self._P, self._b, self._logc = P, b, lc

    # ------------------------------------------------------------------ E-step / M-step
    def _check(self, x):
        x, N, D, _ = _rows(x)
        if self.dim is not None and int(self.dim) < D:
            raise NotImplementedError("PCA before the mixture (dim below the feature width) is not implemented: the PMAM pipeline compares "
                                      "the means with full-width logits and never reduces")
        if D % 32 or not 32 <= D <= 768:
            raise ValueError("feature width must be a multiple of 32 in 32 .. 768")
        return x, N, D

    def _e_step(self, x, resp=None, want_argmax=False):
        """-> (resp [N, K] | None, logp [N], argmax | None, N_k float64 [K]) over row chunks of batch_size."""
        x, N, D = self._check(x)
        K = self.num_components
        dev = x.device
        logp = torch.empty(N, dtype=F32, device=dev)
        am = torch.empty(N, dtype=torch.int32, device=dev) if want_argmax else None
        nk = torch.zeros(K, dtype=F64, device=dev)
        for r0 in range(0, N, self.batch_size):
            n = min(self.batch_size, N - r0)
            maha = gmm_maha(x[r0:r0 + n], self._P, self._b)
            _, lp, a = gmm_resp(maha, self._logc, resp=resp[r0:r0 + n] if resp is not None else False, logp=True, argmax=want_argmax,
                                colsum=nk, accumulate=True)
            logp[r0:r0 + n] = lp
            if want_argmax:
                am[r0:r0 + n] = a
        return resp, logp, am, nk

    def _m_step(self, x, resp, nk):
        x, N, D = self._check(x)
        K = self.num_components
        dev = x.device
        dead = [k for k, v in enumerate(nk.tolist()) if not v > TINY_NK]
        sums = weighted_sums(x, resp).to(F64)
        means = sums / nk.clamp_min(TINY_NK).unsqueeze(1)
        covs = torch.empty(K, D, D, dtype=F64, device=dev)
        A = torch.empty(min(N, MSTEP_ROWS), D, dtype=F32, device=dev)
        eye = torch.eye(D, dtype=F64, device=dev)
        for k in range(K):
            if k in dead:
                continue
            S = weighted_scatter(x, resp, k, means[k], scratch=A).to(F64)
            covs[k] = 0.5 * (S + S.T) / nk[k] + self.reg * eye
        for k in dead:      # keeps its previous parameters
            if self.means_ is None:
                raise RuntimeError(f"component {k} received no points at initialisation")
            means[k], covs[k] = self.means_[k], self.covariances_[k]
            if k not in self.collapsed_:
                self.collapsed_.append(k)
        self.weights_, self.means_, self.covariances_ = nk / nk.sum(), means, covs
        self._prepare(keep=dead if self._P is not None else ())

    def m_step_from(self, x, resp):
        """One M-step from given responsibilities [N, K] (N_k = their column sums, float64): sets weights / means / covariances."""
        resp = resp.to(F32).contiguous()
        self._m_step(x, resp, resp.to(F64).sum(0))
        return self

    def fit(self, x, init_means=None, generator=None):
        """EM.  Initialisation: `init_means` [K, D], or the centres of a k-means run (drawn with `generator`); then every point is given to its
        nearest centre and one M-step from those hard assignments sets weights, means and covariances.  Stops when the mean log-likelihood
        moves by less than convergence_tolerance; its trajectory is `log_likelihood_`, components that ran empty are in `collapsed_`."""
        x, N, D = self._check(x)
        K = self.num_components
        if init_means is None:
            init_means = KMeansTokenizer(K, max_iter=self.kmeans_iter).fit(x, generator=generator).centroids
        if tuple(init_means.shape) != (K, D):
            raise ValueError(f"init_means must be [{K}, {D}]")
        self.log_likelihood_, self.collapsed_, self.converged_ = [], [], False
        self.weights_ = self._P = None
        # what a centre without a single point keeps (it is reported in collapsed_): its own position and the covariance of all points
        ones = torch.ones(N, 1, dtype=F32, device=x.device)
        centre = weighted_sums(x, ones).to(F64)[0] / N
        S = weighted_scatter(x, ones, 0, centre).to(F64)
        self.means_ = init_means.to(device=x.device, dtype=F64).clone()
        self.covariances_ = (0.5 * (S + S.T) / N + self.reg * torch.eye(D, dtype=F64, device=x.device)).expand(K, D, D).clone()
        labels = nearest_centre(x, init_means.to(x.device))
        resp = torch.nn.functional.one_hot(labels.long(), K).to(F32)
        self._m_step(x, resp, resp.to(F64).sum(0))
        prev = None
        for _ in range(self.max_iter):
            _, logp, _, nk = self._e_step(x, resp=resp)
            ll = float(logp.to(F64).mean())
            self.log_likelihood_.append(ll)
            self._m_step(x, resp, nk)
            if prev is not None and abs(ll - prev) < self.tol:
                self.converged_ = True
                break
            prev = ll
        return self

    # ------------------------------------------------------------------ inference
    def predict_proba(self, x):
        x, N, D = self._check(x)
        resp = torch.empty(N, self.num_components, dtype=F32, device=x.device)
        return self._e_step(x, resp=resp)[0]

    def score_samples(self, x):
        return self._e_step(x)[1]

    def predict(self, x):
        return self._e_step(x, want_argmax=True)[2].long()


class KMeansTokenizer:
    """Lloyd's k-means (`--algorithm KMeans` of recipes/desed/pmam/gmm.py).  `predict_proba` is the one-hot code of the cluster index, as
    `label_to_one_hot` (generate_pseudo_label.py:144-148) makes it."""

    def __init__(self, num_clusters, max_iter=10, dim=None):
        if not 1 <= int(num_clusters) <= 64:
            raise ValueError("num_clusters must lie in 1 .. 64")
        self.num_clusters, self.max_iter, self.dim = int(num_clusters), int(max_iter), dim
        self.centroids = None
        self.num_components = self.num_clusters

    @property
    def means(self):
        return self.centroids

    def fit(self, x, init_centroids=None, generator=None):
        x, N, D, _ = _rows(x)
        if self.dim is not None and int(self.dim) < D:
            raise NotImplementedError("PCA before the clustering (dim below the feature width) is not implemented")
        K = self.num_clusters
        if init_centroids is None:
            if N < K:
                raise ValueError("fewer points than clusters")
            idx = torch.randperm(N, generator=generator)[:K].to(x.device)
            init_centroids = x[idx]
        c = init_centroids.to(device=x.device, dtype=F32).contiguous()
        for _ in range(self.max_iter):
            labels = nearest_centre(x, c).long()
            onehot = torch.nn.functional.one_hot(labels, K).to(F32)
            cnt = torch.bincount(labels, minlength=K).to(F64)
            new = (weighted_sums(x, onehot).to(F64) / cnt.clamp_min(1.0).unsqueeze(1)).to(F32)
            new = torch.where(cnt.unsqueeze(1) > 0, new, c)          # an empty cluster keeps its centre
            done = torch.equal(new, c)
            c = new
            if done:
                break
        self.centroids = c
        return self

    def predict(self, x):
        return nearest_centre(x, self.centroids).long()

    def predict_proba(self, x):
        return torch.nn.functional.one_hot(self.predict(x), self.num_clusters).to(F32)

    def save_means(self, path):
        torch.save(self.centroids.cpu(), path)

    def state_dict(self):
        return {"centroids": self.centroids.cpu()}

    def load_state_dict(self, sd, device="cuda"):
        self.centroids = sd["centroids"].to(device=device, dtype=F32)
        self.num_clusters = self.num_components = self.centroids.shape[0]
        return self


def _mel_of(batch):
    return batch[0] if isinstance(batch, (tuple, list)) else batch


class FeatureExtractor:
    """`Extractor.extract` (extractor_feature.py:71-117): frame features of every batch at `feature_layer`, one random frame out of every
    block of `downsample_rate` consecutive frames of the flattened batch (`sample_feature`).  `batches` yields mel spectrograms
    [B, 128, T] on the device (or tuples that start with one).  Draws: `offsets`, one integer tensor per batch with a value in
    [0, downsample_rate) per block, or torch.randint with `generator`.  Returns [L, C] fp32 on the device."""

    def __init__(self, net, generator=None):
        self.net, self.generator = net, generator

    @staticmethod
    def sample_feature(feature, downsample_rate, offsets=None, generator=None):
        n = feature.shape[0]
        starts = torch.arange(0, n, downsample_rate)
        if offsets is None:
            offsets = torch.randint(0, downsample_rate, size=(starts.shape[0],), generator=generator)
        offsets = torch.as_tensor(offsets).cpu().long()
        if offsets.shape != starts.shape or int(offsets.min()) < 0 or int(offsets.max()) >= downsample_rate:
            raise ValueError("offsets: one value in [0, downsample_rate) per block")
        index = (starts + offsets).clamp_max(n - 1)      # (a short last block: the reference would index past the end)
        return feature[index.to(feature.device)]

    def extract(self, batches, feature_layer, downsample_rate, offsets=None):
        out = []
        offsets = iter(offsets) if offsets is not None else None
        for batch in batches:
            f = self.net.extract_features(_mel_of(batch), feature_layer)
            f = f.reshape(-1, f.shape[-1])
            out.append(self.sample_feature(f, downsample_rate, next(offsets) if offsets is not None else None, self.generator))
        return torch.cat(out, 0)


class PseudoLabelGenerator:
    """`Generator.extract` (generate_pseudo_label.py:60-129): posteriors of every frame of every clip under the tokenizer.  `batches` yields
    (mel [B, 128, T], filenames).  Returns (prob [n_clips, T, K] fp32 on the device, filenames)."""

    def __init__(self, net, tokenizer):
        self.net, self.tokenizer = net, tokenizer

    def extract(self, batches, feature_layer):
        probs, names = [], []
        for mel, filenames in batches:
            f = self.net.extract_features(mel, feature_layer)
            B, T, C = f.shape
            probs.append(self.tokenizer.predict_proba(f.reshape(B * T, C)).view(B, T, -1))
            names.extend(filenames)
        return torch.cat(probs, 0), names


def save_prob(path, prob, sr=100):
    """The reference's label TSV (generate_pseudo_label.py:132-141): columns onset, offset, 0 .. K-1, tab separated, rounded to 4 decimals;
    prob [T, K]."""
    import numpy as np
    import pandas as pd
    prob = prob.detach().cpu().double().numpy() if torch.is_tensor(prob) else np.asarray(prob, dtype=np.float64)
    T, K = prob.shape
    onset = np.arange(T) / float(sr)
    data = np.round(np.concatenate((onset[:, None], onset[:, None] + 1.0 / sr, prob), axis=1), decimals=4)
    pd.DataFrame(data, columns=["onset", "offset", *range(K)]).to_csv(path, sep="\t", index=False)
