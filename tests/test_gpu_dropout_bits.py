"""The dropout bits the kernels evaluate against the host restatement of their definition (tests/dropout_cases.py, whose statistics
tests/test_dropout_bits_cpu.py proves): bit equality of sed_dropout_f32's and sed_dropout_mask's dumps, and every other consumer --
sed_dropout_f32's values, sed_act_drop_res_f32, sed_gemm_f32's epilogue index ((z M + m) N + n), the attention forward / backward on
the per-element and the one-hash-per-quad path -- against fp64 with the REFERENCE's mask, none of them with a mask dumped from the
code under test.  Measured errors and margins go to dropout_bits.log (SED_TEST_LOG_DIR, else test_logs/)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dropout_cases as X  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
# measured errors and margins: SED_TEST_LOG_DIR, else test_logs/ at the repository root (kept out of git), as tests/test_gpu_batch_scale.py
LOGDIR = os.environ.get("SED_TEST_LOG_DIR") or os.path.join(ROOT, "test_logs")
LOG = os.path.join(LOGDIR, "dropout_bits.log")


def logerr(msg):
    print(msg)
    os.makedirs(LOGDIR, exist_ok=True)
    with open(LOG, "a") as f:
        f.write(msg + "\n")


def call(*a):
    from transformer4sed_amd.ops import call as c
    return c(*a)


def ulp32(t):
    """Spacing of fp32 at |t| (t float64 tensor): what one unit in the last place of the fp32 result is worth."""
    return torch.from_numpy(np.spacing(np.abs(t.numpy()).astype(np.float32)).astype(np.float64))


@functools.lru_cache(maxsize=None)
def signed_pair(n):
    """x, res fp32 [n] of magnitude [0.5, 2) that share their sign: x scale + res never cancels, so an fp32 evaluation stays within a
    few ulp OF THE RESULT whether or not the compiler contracts the multiply-add."""
    g = torch.Generator().manual_seed(n)
    s = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    return s * (0.5 + 1.5 * torch.rand(n, generator=g)), s * (0.5 + 1.5 * torch.rand(n, generator=g))


@functools.lru_cache(maxsize=None)
def gelu_inputs(n):
    """x uniform in [-6, 6] with its fp64 erf-GELU, res uniform in [-1, 1]."""
    g = torch.Generator().manual_seed(n + 1)
    x = (12.0 * torch.rand(n, generator=g) - 6.0).float()
    xd = x.double()
    return x, 2.0 * torch.rand(n, generator=g) - 1.0, 0.5 * xd * (1.0 + torch.special.erf(xd * 0.7071067811865476))


# ---------------------------------------------------------------------------------------------------------------------- the bits
@pytest.mark.parametrize("n,p,seed,site", X.DASM_BIT_CASES)
def test_dasm_dropout_bits_and_values_equal_the_reference(n, p, seed, site):
    want = torch.from_numpy(X.dasm_keep(n, p, seed, site))
    m = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    call("sed_dropout_f32", None, None, m, n, float(p), seed, site)
    assert torch.equal(m.cpu(), want), int((m.cpu() != want).sum())
    # values: one fp32 multiply by 1 / (1 - p) where kept, exactly 0 where dropped; mask and values from one launch agree as well
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, generator=g)
    out, m2 = torch.full((n,), float("nan"), device=DEV), torch.empty(n, dtype=torch.uint8, device=DEV)
    call("sed_dropout_f32", x.to(DEV), out, m2, n, float(p), seed, site)
    assert torch.equal(m2.cpu(), want)
    assert torch.equal(out.cpu(), torch.where(want.bool(), x * float(X.scale(p)), torch.zeros(n)))


@pytest.mark.parametrize("n,p,seed", X.PMAM_BIT_CASES)
def test_pmam_dropout_mask_bits_equal_the_reference(n, p, seed):
    from transformer4sed_amd._lib import SedHipError
    m = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    call("sed_dropout_mask", m, n, float(p), seed)
    want = torch.from_numpy(X.pmam_keep(n, p, seed))
    assert torch.equal(m.cpu(), want), int((m.cpu() != want).sum())
    for bad in (n + 1, n + 2, n - 1):
        with pytest.raises(SedHipError):
            call("sed_dropout_mask", m, bad, float(p), seed)


# ---------------------------------------------------------------------------------------------------------------------- act_drop_res
@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("n,p,seed,site", [(5, 0.5, -1, 255), (1000, 0.25, (1 << 62) - 1, 5), ((1 << 21) + 5, 0.1, 0x0123456789ABCDEF, 8)])
def test_act_drop_res_vs_float64_under_the_reference_mask(n, p, seed, site, with_res):
    keep = torch.from_numpy(X.dasm_keep(n, p, seed, site)).bool()
    sc = float(X.scale(p))
    # act 0: out = keep ? x scale : 0  (+ res)
    x, res = signed_pair(n)
    out = torch.full((n,), float("nan"), device=DEV)
    call("sed_act_drop_res_f32", x.to(DEV), res.to(DEV) if with_res else None, out, n, 0, float(p), seed, site)
    got = out.cpu()
    assert torch.equal(got[~keep], res[~keep] if with_res else torch.zeros(int((~keep).sum())))       # dropped: res exactly, or 0
    want = x.double() * sc + (res.double() if with_res else 0.0)
    e0 = ((got.double() - want).abs() / ulp32(want))[keep]
    # act 1: GELU first.  gelu_fast is within 9.3e-7 of erf-GELU (csrc/common.h), scaled by 1 / (1 - p); the product and the sum round once each
    xg, rg, gelu64 = gelu_inputs(n)
    call("sed_act_drop_res_f32", xg.to(DEV), rg.to(DEV) if with_res else None, out, n, 1, float(p), seed, site)
    got1 = out.cpu()
    assert torch.equal(got1[~keep], rg[~keep] if with_res else torch.zeros(int((~keep).sum())))
    want1 = gelu64 * sc + (rg.double() if with_res else 0.0)
    d1 = (got1.double() - want1).abs()
    tol1 = 2e-6 * sc + 4 * ulp32(want1)
    logerr(f"act_drop_res n={n} p={p} res={with_res}: act 0 worst {float(e0.max()):.2f} ulp (bound 4); act 1 worst error {float(d1[keep].max()):.2e}, "
           f"worst error / bound {float((d1 / tol1)[keep].max()):.3f} (bound 2e-6 scale + 4 ulp = {2e-6 * sc:.2e} + 4 ulp)")
    assert float(e0.max()) <= 4.0, float(e0.max())
    assert bool((d1 <= tol1)[keep].all()), float((d1 / tol1)[keep].max())


def test_act_drop_res_identity_tail_and_argument_refusals():
    from transformer4sed_amd._lib import SedHipError
    n = 1000
    x, res = signed_pair(n)
    xg, rg, gelu64 = gelu_inputs(n)
    out = torch.full((n,), float("nan"), device=DEV)
    call("sed_act_drop_res_f32", x.to(DEV), None, out, n, 0, 0.0, 424242, 1)
    assert torch.equal(out.cpu(), x)                                    # p = 0: nothing dropped, nothing scaled
    call("sed_act_drop_res_f32", x.to(DEV), res.to(DEV), out, n, 0, 0.0, 424242, 1)
    assert torch.equal(out.cpu(), x + res)                              # one fp32 addition
    call("sed_act_drop_res_f32", xg.to(DEV), rg.to(DEV), out, n, 1, 0.0, 424242, 1)
    want = gelu64 + rg.double()
    assert bool(((out.cpu().double() - want).abs() <= 2e-6 + 4 * ulp32(want)).all())
    xd = x.to(DEV)
    for args in ((n, 2, 0.1), (n, -1, 0.1), (n, 0, 1.0), (n, 0, -0.1), (0, 0, 0.1)):
        with pytest.raises(SedHipError):
            call("sed_act_drop_res_f32", xd, None, out, args[0], args[1], args[2], 1, 0)


# ---------------------------------------------------------------------------------------------------------------------- GEMM epilogue
def test_gemm_f32_epilogue_drop_index_over_batch_and_ragged_rows():
    """NT form, batch 3, M = 70, N = 13: rows do not start on a quad boundary and the batch term of ((z M + m) N + n) matters.  Strictly
    positive operands: an output is 0 exactly where its element was dropped."""
    batch, M, N, K, p, seed, site = 3, 70, 13, 32, 0.5, 0x0123456789ABCDEF, 13
    g = torch.Generator().manual_seed(3)
    A, W = 0.05 + 0.2 * torch.rand(batch, M, K, generator=g), 0.05 + 0.2 * torch.rand(batch, N, K, generator=g)
    out = torch.full((batch, M, N), float("nan"), device=DEV)
    call("sed_gemm_f32", A.to(DEV), W.to(DEV), None, None, out, None, M, N, K, K, K, N, 0, 0, batch, M * K, N * K, M * N, 0, 0, 1, p, seed, site)
    keep = torch.from_numpy(X.dasm_keep(batch * M * N, p, seed, site)).view(batch, M, N)
    got = out.cpu()
    assert torch.equal((got == 0).to(torch.uint8), 1 - keep)
    want = torch.einsum("bmk,bnk->bmn", A.double(), W.double()) * keep.double() * float(X.scale(p))
    err = float((got.double() - want).abs().max())
    logerr(f"gemm_f32 epilogue batch={batch} M={M} N={N} K={K} p={p}: worst error {err:.2e} (bound 2e-5)")
    assert err < 2e-5, err


# ---------------------------------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("Nk", [61, 60])
def test_xattn_train_fwd_bwd_under_the_reference_mask_and_one_flipped_bit_is_visible(Nk):
    """Unmasked attention with ragged query / key tiles at p = 0.5: Nk = 61 takes the per-element hash, Nk = 60 one hash per key quad.
    Output and dq / dk / dv against fp64 autograd under the reference's mask, and -- on the CPU -- the proof that a single wrong bit
    could not hide inside the tolerance: with every probability in [0.5 / Nk, 2 / Nk] and |v| in [0.5, 1.5], flipping any one bit moves
    an output element by at least (0.5 / Nk) 2 (0.5) = 8e-3, more than 100 x the 3e-5 bound."""
    B, H, Nq, dh, p, seed, site = 1, 2, 33, 32, 0.5, (1 << 62) - 1, 5
    D, bound = H * dh, 3e-5
    g = torch.Generator().manual_seed(Nk)
    q, k = 0.1 * torch.randn(B, Nq, D, generator=g), torch.randn(B, Nk, D, generator=g)
    v = (0.5 + torch.rand(B, Nk, D, generator=g)) * torch.where(torch.rand(B, Nk, D, generator=g) < 0.5, -1.0, 1.0)
    dO = torch.randn(B, Nq, D, generator=g)
    keep = torch.from_numpy(X.dasm_keep(B * H * Nq * Nk, p, seed, site)).view(B, H, Nq, Nk)
    sc = float(X.scale(p))

    def oracle(kp, grad):
        qd, kd, vd = (t.double().clone().requires_grad_(grad) for t in (q, k, v))
        qh, kh, vh = (t.view(B, -1, H, dh).transpose(1, 2) for t in (qd, kd, vd))
        pr = torch.softmax(qh @ kh.transpose(-1, -2) / dh ** 0.5, -1)
        o = ((pr * kp.double() * sc) @ vh).transpose(1, 2).reshape(B, Nq, D)
        if grad:
            o.backward(dO.double())
        return o.detach(), pr.detach(), (qd.grad, kd.grad, vd.grad)

    want, pr, (gq, gk, gv) = oracle(keep, True)
    assert float(pr.min()) * Nk >= 0.5 and float(pr.max()) * Nk <= 2.0, (float(pr.min()) * Nk, float(pr.max()) * Nk)
    # the bit whose flip moves the output least: its probability times the largest |v| of its key and head
    vmax = v.double().view(B, Nk, H, dh).abs().amax(-1).permute(0, 2, 1).unsqueeze(2)                 # [B, H, 1, Nk]
    effect = pr * sc * vmax
    b_, h_, i_, j_ = np.unravel_index(int(effect.argmin()), effect.shape)
    flipped = keep.clone()
    flipped[b_, h_, i_, j_] ^= 1
    moved = float((oracle(flipped, False)[0] - want).abs().max())
    logerr(f"xattn Nk={Nk}: flipping the least visible bit ({b_}, {h_}, {i_}, {j_}) moves the fp64 output by {moved:.2e} = {moved / bound:.0f} x the bound")
    assert moved > 100 * bound and abs(moved - float(effect.min())) < 1e-12

    out, lse, Dq = torch.empty(B, Nq, D, device=DEV), torch.empty(B * H * Nq, device=DEV), torch.empty(B * H * Nq, device=DEV)
    dq, dk, dv = torch.empty(B, Nq, D, device=DEV), torch.empty(B, Nk, D, device=DEV), torch.empty(B, Nk, D, device=DEV)
    qg, kg, vg = q.to(DEV), k.to(DEV), v.to(DEV)
    call("sed_xattn_f32_fwd_train", qg, kg, vg, out, None, lse, B, H, Nq, Nk, dh, D, D, D, D, Nq * D, p, seed, site)
    call("sed_xattn_f32_bwd", qg, kg, vg, out, dO.to(DEV), lse, Dq, dq, dk, dv, None, B, H, Nq, Nk, dh, D, D, D, D, D, D, D, Nq * D, p, seed, site)
    e_out = float((out.cpu().double() - want).abs().max())
    rel = lambda got, ref: float((got.cpu().double() - ref).norm() / ref.norm())
    e_g = {"dq": rel(dq, gq), "dk": rel(dk, gk), "dv": rel(dv, gv)}
    logerr(f"xattn Nk={Nk} p={p}: out {e_out:.2e} (bound 3e-5) " + " ".join(f"{n_} {e:.2e}" for n_, e in e_g.items()) + " (bound 3e-5 relative)")
    assert e_out < bound, e_out
    for n_, e in e_g.items():
        assert e < 3e-5, (n_, e)
