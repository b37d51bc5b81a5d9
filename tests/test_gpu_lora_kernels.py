"""The LoRA kernels on the hardware, bit for bit: sed_lora_rowproj, sed_lora_colreduce, sed_lora_grad, sed_lora_merge (csrc/lora.hip) and
the LoRA term of sed_weight_images (csrc/layout.hip) on the exact-result cases of tests/lora_cases.py -- every rank, both layouts, both
16-bit types, pitched operands, ragged tiles and slabs, empty wave quarters, second trips and grid passes, false column guards and the
surplus workgroups of sed_lora_grad's shared grid.  tests/test_lora_cases_cpu.py proves on the CPU that the expected results are exact
in fp32 whatever the order of accumulation and that the comparison sees a dropped row, column group or K quarter, a shifted rank column,
a swapped layout, `=` for `+=` and a wrong 16-bit decode.  Every output carries a NaN canary tail, every pitched operand NaN padding.
(The real-valued tests of these entry points, which see the 16-bit rounding of the fp32 factors, are in tests/test_gpu_pmam_kernels.py.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import lora_cases as L  # noqa: E402
from lora_cases import GUARD, NAN  # noqa: E402
from transformer4sed_amd._lib import SedHipError  # noqa: E402
from transformer4sed_amd.ops import call, BF16, F16  # noqa: E402

DEV = "cuda"


def dev(t):
    return t.contiguous().to(DEV)


def out_buf(n, dtype=torch.float32, start=None):
    """n valid elements (NaN, or `start`) followed by GUARD NaN canaries."""
    b = torch.full((n + GUARD,), NAN, dtype=dtype, device=DEV)
    if start is not None:
        b[:n] = dev(start).reshape(-1)
    return b


def same(buf, ref64, what):
    """The valid region equals the exact reference, holds no NaN, and the canaries behind it are untouched."""
    n = ref64.numel()
    got, ref = buf[:n].view(ref64.shape), dev(ref64).to(buf.dtype)
    assert not bool(torch.isnan(got.float()).any()), f"{what}: NaN in the output"
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        first = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {n} elements differ, first at {first}: got {float(got[first])}, exact {float(ref[first])}")
    assert bool(torch.isnan(buf[n:].float()).all()), f"{what}: canary overwritten"


# ================================================================================================ exact results
@pytest.mark.parametrize("c", L.ROWPROJ_CASES, ids=[L.rowproj_id(c) for c in L.ROWPROJ_CASES])
def test_rowproj_exact(c):
    i = L.rowproj_inputs(c)
    u = out_buf(c.M * c.r)
    call("sed_lora_rowproj", dev(i["X"]), c.f16, c.M, c.K, c.K + c.pad, dev(i["Wm"]), c.w_kxr, c.r, c.scale, u)
    torch.cuda.synchronize()
    same(u, L.rowproj_ref(c, i), "u")


@pytest.mark.parametrize("c", L.COLREDUCE_CASES, ids=[L.colreduce_id(c) for c in L.COLREDUCE_CASES])
def test_colreduce_exact(c):
    i = L.colreduce_inputs(c)
    G = out_buf(c.C * c.r, start=i["G0"])
    call("sed_lora_colreduce", dev(i["Y"]), c.f16, c.M, c.C, c.C + c.pad, dev(i["P"]), c.r, c.scale, G, c.g_cxr)
    torch.cuda.synchronize()
    same(G, L.colreduce_ref(c, i), "G")


@pytest.mark.parametrize("c", L.GRAD_CASES, ids=[L.grad_id(c) for c in L.GRAD_CASES])
def test_grad_exact(c):
    i = L.grad_inputs(c)
    dA, dB = out_buf(c.r * c.k_in, start=i["dA0"]), out_buf(c.n_out * c.r, start=i["dB0"])
    call("sed_lora_grad", dev(i["dW"]), dev(i["A"]), dev(i["B"]), c.s, dA, dB, c.n_out, c.k_in, c.r)
    torch.cuda.synchronize()
    rA, rB = L.grad_ref(c, i)
    same(dB, rB, "dB")
    same(dA, rA, "dA")


@pytest.mark.parametrize("c", L.MERGE_CASES, ids=[L.grad_id(c) for c in L.MERGE_CASES])
def test_merge_exact(c):
    i = L.merge_inputs(c)
    out = out_buf(c.n_out * c.k_in)
    call("sed_lora_merge", dev(i["W"]), dev(i["A"]), dev(i["B"]), c.s, out, c.n_out, c.k_in, c.r)
    torch.cuda.synchronize()
    same(out, L.merge_ref(c, i), "W + s B A")


def image_launch(descs, inputs):
    """One sed_weight_images launch over `descs`, all three images asked of each -> [(straight, transposed, split) buffers]."""
    rows, outs, keep, tiles = [], [], [], 0
    for d, i in zip(descs, inputs):
        n = d.R * d.C
        W, A, B = dev(i["W"]), (dev(i["A"]) if d.r else None), (dev(i["B"]) if d.r else None)
        S, T, P = out_buf(n, L.dt16(d.f16)), out_buf(n, BF16), out_buf(3 * n, F16)
        sbits = int(torch.tensor(d.s, dtype=torch.float32).view(torch.int32))
        rows.append([W.data_ptr(), T.data_ptr(), S.data_ptr(), P.data_ptr(), d.R, d.C, 2 if d.f16 else 0, tiles, 0, 0,
                     A.data_ptr() if d.r else 0, B.data_ptr() if d.r else 0, d.r, sbits if d.r else 0, 0, 0])
        tiles += L.image_tiles(d.R, d.C)
        outs.append((S, T, P))
        keep += [W, A, B]
    call("sed_weight_images", torch.tensor(rows, dtype=torch.int64, device=DEV), len(rows), tiles)
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("launch", L.IMAGE_LAUNCHES, ids=[L.image_id(x) for x in L.IMAGE_LAUNCHES])
def test_weight_images_lora_term_exact(launch):
    """W + s B A in the straight (bf16 / f16), the transposed bf16 and the split [hi | hi | lo] image, LoRA descriptors and one without
    the term in the same launch; then the zero-padding identity: rank 2r with A' = [A; 0], B' = [B, anything] gives the same bits."""
    inputs = [L.image_inputs(d, 5000 + 10 * n) for n, d in enumerate(launch)]
    outs = image_launch(launch, inputs)
    for d, i, (S, T, P) in zip(launch, inputs, outs):
        s, t, p = L.image_expected(d, L.image_ref(d, i))
        same(S, s, f"{d}: straight image")
        same(T, t, f"{d}: transposed image")
        same(P, p, f"{d}: split image")
    padded = [L.image_padded(d, i, 5000 + 10 * n) if d.r else (d, i) for n, (d, i) in enumerate(zip(launch, inputs))]
    outs2 = image_launch([d for d, _ in padded], [i for _, i in padded])
    for d, a, b in zip(launch, outs, outs2):
        for x, y, name in zip(a, b, ("straight", "transposed", "split")):
            n = x.numel() - GUARD
            assert torch.equal(x[:n].view(torch.int16), y[:n].view(torch.int16)), f"{d}: {name} image changes with zero-padded factors"
            assert bool(torch.isnan(y[n:].float()).all())


# ================================================================================================ refusals
def nans(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def refused(name, outs, *args):
    with pytest.raises(SedHipError, match="bad argument"):
        call(name, *args)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs), name


def test_lora_argument_errors_write_nothing():
    """Every documented refusal comes back as the argument error and leaves NaN-filled outputs as they were: rowproj with K % 64, a pitch
    that is no multiple of 8 or below K, r 17, and the two widths one step past the LDS limit; colreduce with r 9, C % 4, ldy % 4; grad
    with r 17; merge with k_in % 4."""
    M = 16
    for a in L.ROWPROJ_REFUSALS:
        K, ldx, r = a["K"], a["ldx"], a["r"]
        u = nans(M, r)
        refused("sed_lora_rowproj", [u], torch.ones(M, max(K, ldx), dtype=BF16, device=DEV), 0, M, K, ldx, torch.ones(r, K, device=DEV), 0, r, 1.0, u)
    for a in L.COLREDUCE_REFUSALS:
        C, ldy, r = a["C"], a["ldy"], a["r"]
        G = nans(C, r)
        refused("sed_lora_colreduce", [G], torch.ones(M, ldy, dtype=BF16, device=DEV), 0, M, C, ldy, torch.ones(M, r, device=DEV), r, 1.0, G, 1)
    for a in L.GRAD_REFUSALS:
        n, k, r = a["n_out"], a["k_in"], a["r"]
        dA, dB = nans(r, k), nans(n, r)
        refused("sed_lora_grad", [dA, dB], torch.ones(n, k, device=DEV), torch.ones(r, k, device=DEV), torch.ones(n, r, device=DEV), 1.0, dA, dB, n, k, r)
    for a in L.MERGE_REFUSALS:
        n, k, r = a["n_out"], a["k_in"], a["r"]
        out = nans(n, k)
        refused("sed_lora_merge", [out], torch.ones(n, k, device=DEV), torch.ones(r, k, device=DEV), torch.ones(n, r, device=DEV), 1.0, out, n, k, r)
