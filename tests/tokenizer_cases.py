"""Float64 reference and input constructions for the PMAM tokenizer tests (tests/test_tokenizer_cpu.py, tests/test_gpu_tokenizer.py).

The reference is a plain numpy restatement of full-covariance EM: E-step through the inverse Cholesky factors, M-step, covariance
regularisation, mean log-likelihood.  Every product also exists as an fp32 RESTATEMENT (`dtype=np.float32`: the operands the device
gets -- P, b, logc made in float64 and rounded once -- and fp32 numpy products): its distance from float64 is the error the number format
itself causes, and the GPU bounds are 4 x that distance.  The kernels sum in another order (tile-wise, triangular, split over
workgroups); 4 covers the square root of the term count between two orders and stays far below what a missing tile, bias, row or
component moves the result by (the mutants below; test_tokenizer_cpu.py proves >= 20 x the bound for each)."""
import functools

import numpy as np
from scipy.linalg import solve_triangular

F32, F64 = np.float32, np.float64
TILE_J = 64                       # width of a j tile of sed_gmm_maha
ROWS_PER_BLOCK = 128              # rows of X per workgroup
MAX_ROW_BLOCKS = 1024             # grid.x cap: launch geometry (min(ceil(N / 128), 1024), K), a workgroup strides over the row blocks
GRID_PASS_N = MAX_ROW_BLOCKS * ROWS_PER_BLOCK + 77      # one N past a full grid pass
MAHA_DS, MAHA_KS, MAHA_NS = (32, 96, 768), (1, 3, 30), (1, 63, 65, 200)
MAHA_CASES = [(D, K, N) for D in MAHA_DS for K in MAHA_KS for N in MAHA_NS] + [(32, 1, GRID_PASS_N)]
BOUND_FACTOR, MUTANT_FACTOR = 4.0, 20.0
MAHA_MUTANTS = ("drop_last_j_tile", "drop_bias", "drop_rows_ge_64", "drop_last_component")


def _seed(tag):
    return int.from_bytes(tag.encode(), "little") % (2 ** 31)


# ---------------------------------------------------------------------------------------------------------------- float64 EM
def operands(means, covs):
    """-> P [K, D, D] = L^-1 (lower triangular), b [K, D] = -P mu, logdet [K] of covs = L L^T; float64."""
    K, D = means.shape
    P, b, logdet = np.zeros((K, D, D)), np.zeros((K, D)), np.zeros(K)
    eye = np.eye(D)
    for k in range(K):
        L = np.linalg.cholesky(covs[k])
        P[k] = np.tril(solve_triangular(L, eye, lower=True))
        b[k] = -P[k] @ means[k]
        logdet[k] = 2.0 * np.log(np.diag(L)).sum()
    return P, b, logdet


def log_coefficients(weights, logdet, D):
    return np.log(weights) - 0.5 * (D * np.log(2.0 * np.pi) + logdet)


def maha(x, P, b, dtype=F64, mutant=None):
    """maha[n, k] = |P_k x_n + b_k|^2 in `dtype` arithmetic."""
    x, P, b = x.astype(dtype), P.astype(dtype), b.astype(dtype)
    N, D = x.shape
    K = P.shape[0]
    out = np.zeros((N, K), dtype=dtype)
    for k in range(K):
        y = x @ P[k].T
        if mutant != "drop_bias":
            y = y + b[k]
        if mutant == "drop_last_j_tile":
            y = y[:, :(D - 1) // TILE_J * TILE_J]
        out[:, k] = (y * y).sum(1, dtype=dtype)
    if mutant == "drop_rows_ge_64":
        out[64:] = 0
    if mutant == "drop_last_component":
        out[:, K - 1] = 0
    return out


def posterior(mh, logc, dtype=F64):
    """-> resp [N, K], logp [N] from s = logc - maha / 2 (max-subtracted softmax / log-sum-exp)."""
    s = logc.astype(dtype)[None, :] - dtype(0.5) * mh.astype(dtype)
    m = s.max(1, keepdims=True)
    e = np.exp(s - m)
    tot = e.sum(1, keepdims=True, dtype=dtype)
    return e / tot, (m + np.log(tot))[:, 0]


def e_step(x, weights, means, covs, dtype=F64):
    """-> resp, logp.  The operands are made in float64 either way (as the device path does); dtype = arithmetic of the products."""
    P, b, logdet = operands(means, covs)
    logc = log_coefficients(weights, logdet, x.shape[1])
    return posterior(maha(x, P, b, dtype), logc.astype(dtype), dtype)


def m_step(x, resp, reg, dtype=F64):
    """-> weights, means, covs (float64).  dtype = arithmetic of the sums over the points (N_k and the divisions stay float64)."""
    N, D = x.shape
    K = resp.shape[1]
    nk = resp.astype(F64).sum(0)
    xd, rd = x.astype(dtype), resp.astype(dtype)
    means = (rd.T @ xd).astype(F64) / nk[:, None]
    covs = np.zeros((K, D, D))
    for k in range(K):
        a = np.sqrt(rd[:, k])[:, None] * (xd - means[k].astype(dtype))
        S = (a.T @ a).astype(F64)
        covs[k] = 0.5 * (S + S.T) / nk[k] + reg * np.eye(D)
    return nk / nk.sum(), means, covs


def nearest(x, centres, dtype=F64):
    """-> (arg-min over centres of |c|^2 - 2 x.c, the distances)."""
    c = centres.astype(dtype)
    d = (c * c).sum(1, dtype=dtype)[None, :] - dtype(2) * (x.astype(dtype) @ c.T)
    return d.argmin(1), d


def init_from_means(x, init_means, reg, dtype=F64):
    """Initialisation of `GaussianMixtureTokenizer.fit`: hard assignment to the nearest centre, one M-step."""
    labels, _ = nearest(x, init_means)
    return m_step(x, np.eye(init_means.shape[0])[labels], reg, dtype)


def em(x, weights, means, covs, n_iter, reg, dtype=F64):
    """-> (list of (weights, means, covs) after each M-step, log-likelihood trajectory): iteration i = E-step under the current
    parameters (its mean log-density is ll[i]) then M-step."""
    params, ll = [], []
    for _ in range(n_iter):
        resp, logp = e_step(x, weights, means, covs, dtype)
        ll.append(float(logp.astype(F64).mean()))
        weights, means, covs = m_step(x, resp, reg, dtype)
        params.append((weights, means, covs))
    return params, ll


# ---------------------------------------------------------------------------------------------------------------- error metrics
def rel_err(got, ref):
    """Worst element-wise relative error (quantities that are bounded away from zero: maha, log-densities)."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    return float((np.abs(got - ref) / np.abs(ref)).max()) if ref.size else 0.0


def scaled_err(got, ref):
    """Worst absolute error over the largest magnitude of the reference (means, covariances: single entries may be ~0)."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


# ---------------------------------------------------------------------------------------------------------------- constructions
def random_spd(rng, D):
    """Random covariance, condition number ~1e2: diag(s) (I / 4 + G G^T / D) diag(s), s log-spaced over one decade."""
    G = rng.standard_normal((D, D))
    s = np.logspace(-0.5, 0.5, D)[rng.permutation(D)]
    return (0.25 * np.eye(D) + G @ G.T / D) * s[:, None] * s[None, :]


@functools.lru_cache(maxsize=None)
def maha_params(D, K):
    """Distinct random covariances and means per component -> (means, covs, P, b, logdet) float64."""
    rng = np.random.default_rng(_seed(f"maha{D}x{K}"))
    covs = np.stack([random_spd(rng, D) * (0.5 + k % 3) for k in range(K)])
    means = rng.standard_normal((K, D)) * 1.5 + 0.5
    return (means, covs) + operands(means, covs)


@functools.lru_cache(maxsize=None)
def maha_case(D, K, N):
    """-> dict(x fp32 [N, D], P, b fp32, ref float64 maha of the fp32 operands, restated fp32 maha, bound).  Points are drawn around the
    means (every third one far out), so the terms are of the size the fit sees."""
    means, covs, P, b, _ = maha_params(D, K)
    rng = np.random.default_rng(_seed(f"x{D}x{K}x{N}"))
    comp = rng.integers(0, K, N)
    x = (means[comp] + rng.standard_normal((N, D)) * np.where(np.arange(N) % 3 == 0, 3.0, 1.0)[:, None]).astype(F32)
    P32, b32 = P.astype(F32), b.astype(F32)
    ref = maha(x, P32, b32, F64)
    own = rel_err(maha(x, P32, b32, F32), ref)
    return dict(x=x, P=P32, b=b32, ref=ref, fp32_err=own, bound=BOUND_FACTOR * own)


def mutant_applies(mutant, D, K, N):
    """A mutant that cannot touch a case (no row >= 64 in it) says nothing about it."""
    return N > 64 if mutant == "drop_rows_ge_64" else True


@functools.lru_cache(maxsize=None)
def overlap_case(D, K, N, tag="overlap"):
    """Overlapping mixture: ONE shared covariance Sigma = L L^T, means mu_k = mu_0 + L u_k with |u_k| in [1, 2] (whitened distance
    from the common centre), points drawn from the components with equal weights.  -> dict(x fp32, weights, means, covs, labels)."""
    rng = np.random.default_rng(_seed(f"{tag}{D}x{K}x{N}"))
    cov = random_spd(rng, D)
    L = np.linalg.cholesky(cov)
    u = rng.standard_normal((K, D))
    u *= (rng.uniform(1.0, 2.0, K) / np.linalg.norm(u, axis=1))[:, None]
    means = 0.3 + u @ L.T
    labels = rng.integers(0, K, N)
    x = (means[labels] + rng.standard_normal((N, D)) @ L.T).astype(F32)
    return dict(x=x, weights=np.full(K, 1.0 / K), means=means, covs=np.stack([cov] * K), labels=labels)


POSTERIOR_CASES = [(32, 4, 4096), (32, 64, 2048), (768, 3, 1500)]        # (resp kernel / fit, resp at K = 64, M-step)


@functools.lru_cache(maxsize=None)
def posterior_case(D, K, N):
    """Overlap case with its float64 posteriors: maha32 = the float64 maha rounded to fp32 (the resp kernel's input), logc32, and
    resp / logp = float64 posteriors OF THOSE fp32 inputs."""
    c = dict(overlap_case(D, K, N))
    P, b, logdet = operands(c["means"], c["covs"])
    c["logdet"] = logdet
    c["maha32"] = maha(c["x"], P, b).astype(F32)
    c["logc32"] = log_coefficients(c["weights"], logdet, D).astype(F32)
    c["resp"], c["logp"] = posterior(c["maha32"], c["logc32"])
    c["score_tol"] = score_tolerance(c["maha32"], c["logc32"])
    return c


def score_tolerance(maha32, logc32):
    """fp32 evaluation of a row of sed_gmm_resp: s = logc - maha / 2 is rounded twice (2 x 2^-24 |s|), s - max once more, expf and
    logf are good to 2 ulp, the sum of K <= 64 terms adds (K - 1) 2^-24 relative, the division one more: an absolute error of at most
    (4 max|s| + K + 8) 2^-24 on log p and -- a posterior being the exponential of a score difference, at most 1 -- on every posterior."""
    s = logc32.astype(F64)[None, :] - 0.5 * maha32.astype(F64)
    return float((4.0 * np.abs(s).max() + maha32.shape[1] + 8) * 2.0 ** -24)


def mstep_case():
    """D = 768, K = 3, N = 1500: x and the fp32-rounded float64 posteriors of the overlap case; float64 M-step of those inputs, the
    fp32 restatement's own error per quantity and the bounds."""
    D, K, N = POSTERIOR_CASES[2]
    c = posterior_case(D, K, N)
    resp32 = c["resp"].astype(F32)
    reg = 1e-6
    ref = m_step(c["x"], resp32, reg)
    own = m_step(c["x"], resp32, reg, F32)
    errs = tuple(scaled_err(o, r) for o, r in zip(own, ref))
    return dict(x=c["x"], resp=resp32, reg=reg, ref=ref, fp32_err=errs, bound=tuple(BOUND_FACTOR * e for e in errs))


FIT_ITERS, FIT_REG = 5, 1e-6


@functools.lru_cache(maxsize=None)
def fit_case():
    """D = 32, K = 4, N = 4096, overlapping, with init_means = the true means moved by a tenth of a whitened unit.  Reference: float64
    initialisation + five EM iterations; bounds: 4 x the distance of the fp32 restatement of the same run, per iteration and quantity
    (weights, means, covs by scaled_err; the log-likelihood relative to its size)."""
    D, K, N = POSTERIOR_CASES[0]
    c = overlap_case(D, K, N)
    rng = np.random.default_rng(_seed("fit-init"))
    init = c["means"] + 0.1 * rng.standard_normal((K, D)) @ np.linalg.cholesky(c["covs"][0]).T
    x = c["x"]
    runs = {}
    for dt in (F64, F32):
        w, mu, cv = init_from_means(x, init, FIT_REG, dt)
        runs[dt] = em(x, w, mu, cv, FIT_ITERS, FIT_REG, dt)
    (pref, llref), (pown, llown) = runs[F64], runs[F32]
    perr = [tuple(scaled_err(o, r) for o, r in zip(po, pr)) for po, pr in zip(pown, pref)]
    llerr = [abs(a - b) / abs(b) for a, b in zip(llown, llref)]
    # one bound per quantity for the whole trajectory: 4 x the worst iteration of the restatement
    pbound = tuple(BOUND_FACTOR * max(e[i] for e in perr) for i in range(3))
    _, d = nearest(x, init)
    d.sort(axis=1)
    return dict(x=x, init=init.astype(F32), params=pref, ll=llref, fp32_perr=perr, fp32_llerr=llerr, pbound=pbound,
                llbound=BOUND_FACTOR * max(llerr), init_margin=float((d[:, 1] - d[:, 0]).min()), init_dist_err=distance_error(x, init))


def distance_error(x, centres):
    """Worst absolute error of the fp32 restatement of |c|^2 - 2 x.c against float64 (same fp32 operands)."""
    c32 = centres.astype(F32)
    return float(np.abs(nearest(x, c32, F32)[1].astype(F64) - nearest(x, c32, F64)[1]).max())


@functools.lru_cache(maxsize=None)
def kmeans_case(D=96, K=7, N=1001):
    """Well separated clusters: centres ~ N(0, 9 I), points = centre + 0.3 N(0, I).  `margin` = the smallest gap between the two nearest
    centres of a point, `dist_err` = fp32 distance error: the construction holds iff margin > 2 * BOUND_FACTOR * dist_err."""
    rng = np.random.default_rng(_seed(f"kmeans{D}x{K}x{N}"))
    centres = (3.0 * rng.standard_normal((K, D))).astype(F32)
    labels = np.arange(N) % K
    x = (centres[labels] + 0.3 * rng.standard_normal((N, D))).astype(F32)
    start = (centres + 0.5 * rng.standard_normal((K, D))).astype(F32)
    out = dict(x=x, centres=centres, start=start, labels=labels)
    for name, c in (("", centres), ("start_", start)):
        got, d = nearest(x, c)
        d = np.sort(d, axis=1)
        out[name + "margin"] = float((d[:, 1] - d[:, 0]).min()) if K > 1 else np.inf
        out[name + "dist_err"] = distance_error(x, c)
        out[name + "argmin"] = got
    return out
