"""Timing of the PMAM tokenizer kernels at the production width (D = 768, K = 30) -> profiles/tokenizer_timing.txt.

One process, the two paths taking turns per round (device events around each, after a warm-up of every shape):
  * `sed_gmm_maha` against the composition the library could run before it existed: per component `sed_gemm_f32_nt` with bias into an
    [N, D] buffer + a torch row sum of squares;
  * one full E-step (maha + posteriors + N_k) and one full M-step (R^T X, then per component centre / scale + A^T A) of
    `GaussianMixtureTokenizer` on the same points.
Rates: the operations the algorithm needs (N K D (D + 32) multiply-adds for the triangular product in 32-wide d tiles) over the event time,
beside the fp32 matrix peak.  Usage: python tools/tokenizer_bench.py [--n N] [--rounds R] [--out PATH]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from transformer4sed_amd.ops import call  # noqa: E402
from transformer4sed_amd import tokenizer as TK  # noqa: E402

PEAK_F32_TF = 157.3


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tokenizer_timing.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tokenizer_bench needs an MI355X: there is nothing to time without one")
    dev = torch.device("cuda")
    N, D, K = a.n, 768, 30
    g = torch.Generator(device="cpu").manual_seed(0)
    # overlapping mixture: one shared random covariance, means a whitened unit or two apart
    G = torch.randn(D, D, generator=g, dtype=torch.float64)
    cov = 0.25 * torch.eye(D, dtype=torch.float64) + G @ G.T / D
    L = torch.linalg.cholesky(cov)
    u = torch.randn(K, D, generator=g, dtype=torch.float64)
    u = u / u.norm(dim=1, keepdim=True) * (1.0 + torch.rand(K, 1, generator=g, dtype=torch.float64))
    means = u @ L.T
    x = (means[torch.randint(0, K, (N,), generator=g)] + torch.randn(N, D, generator=g, dtype=torch.float64) @ L.T).float().to(dev)
    tok = TK.GaussianMixtureTokenizer(K)
    tok.weights_ = torch.full((K,), 1.0 / K, dtype=torch.float64, device=dev)
    tok.means_, tok.covariances_ = means.to(dev), cov.to(dev).expand(K, D, D).contiguous()
    tok._prepare()
    P, b = tok._P, tok._b
    maha = torch.empty(N, K, device=dev)
    maha2 = torch.empty(N, K, device=dev)
    Y = torch.empty(N, D, device=dev)
    resp = torch.empty(N, K, device=dev)

    def fused():
        TK.gmm_maha(x, P, b, out=maha)

    def composed():
        for k in range(K):
            call("sed_gemm_f32_nt", x, P[k], b[k], None, Y, N, D, D, D, D, D, 1, 0, 0, 0, 0)
            maha2[:, k] = (Y * Y).sum(1)

    def e_step():
        tok._e_step(x, resp=resp)

    def m_step():
        tok._m_step(x, resp, resp.double().sum(0))

    paths = [("sed_gmm_maha", fused), ("gemm_f32_nt + row sum of squares", composed), ("E-step", e_step), ("M-step", m_step)]
    for _, fn in paths:         # warm-up of every shape
        fn()
    torch.cuda.synchronize()
    rel = float(((maha - maha2).abs() / maha2.abs()).max())
    times = {name: [] for name, _ in paths}
    for _ in range(a.rounds):
        for name, fn in paths:
            times[name].append(timed(fn))
    tri = 2.0 * N * K * D * (D + 32) / 2          # flops of the triangular product in 32-wide tiles
    full = 2.0 * N * K * D * D
    mflops = 2.0 * N * K * D + 2.0 * N * K * D * D
    lines = [f"PMAM tokenizer timing, N = {N} frames, D = {D}, K = {K}; {a.rounds} rounds, paths taking turns, device events, ms (min / median / max)",
             f"fused vs composed maha: worst relative difference {rel:.2e}"]
    for name, _ in paths:
        t = sorted(times[name])
        lo, med, hi = t[0], t[len(t) // 2], t[-1]
        fl = {"sed_gmm_maha": tri, "gemm_f32_nt + row sum of squares": full, "E-step": tri, "M-step": mflops}[name]
        lines.append(f"{name:36s} {lo:9.3f} {med:9.3f} {hi:9.3f}   {fl / med / 1e9:7.1f} TFLOP/s needed-op rate at the median"
                     f" ({100 * fl / med / 1e9 / PEAK_F32_TF:4.1f} % of the {PEAK_F32_TF} TF fp32 matrix peak)")
    f_med, c_med = sorted(times["sed_gmm_maha"])[a.rounds // 2], sorted(times["gemm_f32_nt + row sum of squares"])[a.rounds // 2]
    lines.append(f"composition / fused (medians): {c_med / f_med:.2f} x")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
