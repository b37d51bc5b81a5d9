"""tests/lora_cases.py proved on the CPU, before tests/test_gpu_lora_kernels.py holds the hardware to it:

1. every case passes its budget, and the budget helpers raise for a case that would round;
2. the result is exact: the float64 reference equals the int64 product, and so does fp32 arithmetic in two different summation orders
   (one matmul; partial sums over chunks taken last to first) -- bit equality is therefore the right demand on a kernel;
3. every 16-bit operand and every 16-bit image round-trips through its type;
4. the restated launch arithmetic shows that the named cases reach the branch they are named for;
5. each deliberately wrong reference differs from the exact one in every case that has the edge it is about, so the GPU assertions
   cannot pass a kernel with that fault;
6. every case passes the argument checks of the entry points, every documented refusal fails them."""
import pytest
import torch

import lora_cases as L
from exact_cases import BF16, F16, check_budget

F32, F64, I64 = torch.float32, torch.float64, torch.int64


def ids(cases, f):
    return [f(c) for c in cases]


def chunked_f32(a, b, chunk):
    """a [m, k] @ b [k, n] in fp32, as partial products over chunks of k summed from the last chunk to the first."""
    out = torch.zeros(a.shape[0], b.shape[1])
    for k0 in reversed(range(0, a.shape[1], chunk)):
        out = out + a[:, k0:k0 + chunk].float() @ b[k0:k0 + chunk].float()
    return out


def exact_everywhere(ref64, int_prod, scale, base, a, b, chunk):
    """ref64 == base + scale * int64 product == the same in fp32, two summation orders."""
    want = base.double() + scale * int_prod.double()
    assert torch.equal(ref64, want)
    for prod in (a.float() @ b.float(), chunked_f32(a, b, chunk)):
        got = base.float() + F32_scale(scale) * prod
        assert got.dtype == F32 and torch.equal(got.double(), want)


def F32_scale(scale):
    return torch.tensor(scale, dtype=F32)


# ------------------------------------------------------------------------------------------------ 1. budgets
def test_every_case_passes_its_budget():
    for c in L.ROWPROJ_CASES:
        L.rowproj_budget(c)
    for c in L.COLREDUCE_CASES:
        L.colreduce_budget(c)
    for c in L.GRAD_CASES:
        L.grad_budget(c)
    for c in L.MERGE_CASES:
        L.merge_budget(c)
    for launch in L.IMAGE_LAUNCHES:
        for d in launch:
            assert L.image_budget(d) * L.denom_of(d.s) <= 256


def test_budgets_raise_for_a_case_that_would_round():
    with pytest.raises(ValueError):
        check_budget(8256, 64, 64)                                   # 8256 x 4096 >= 2^24
    with pytest.raises(ValueError):
        check_budget(32805, 7, 7, alpha=0.125, res_max=100, denom=128)  # exact as a sum, not in units of 1/128
    with pytest.raises(ValueError):
        L.check_16bit(257, BF16)
    with pytest.raises(ValueError):
        L.check_16bit(33, BF16, denom=8)                             # 264 units of 1/8: nine significant bits
    with pytest.raises(ValueError):
        L.check_16bit(2049, F16)
    real = L.image_magnitudes
    try:
        L.image_magnitudes = lambda d: (200, 3, 3)                   # 200 + 16 x 9 = 344 > 256
        with pytest.raises(ValueError):
            L.image_budget(L.ImgDesc(16, 64, 16, 0, 1.0))
    finally:
        L.image_magnitudes = real


# ------------------------------------------------------------------------------------------------ 2. exact in any order, 3. round trips
def round_trips(x16, K):
    v = x16[:, :K]
    assert torch.equal(v.float().to(x16.dtype), v) and torch.equal(v.float(), v.float().round()) and not bool(torch.isnan(v.float()).any())
    assert bool(torch.isnan(x16[:, K:].float()).all())              # the padding is poison


@pytest.mark.parametrize("c", L.ROWPROJ_CASES, ids=ids(L.ROWPROJ_CASES, L.rowproj_id))
def test_rowproj_is_exact(c):
    i = L.rowproj_inputs(c)
    round_trips(i["X"], c.K)
    assert i["X"].shape == (c.M, c.K + c.pad) and i["Wm"].shape == ((c.K, c.r) if c.w_kxr else (c.r, c.K))
    assert torch.equal(i["W"].to(L.dt16(c.f16)).float(), i["W"])    # the factor survives the kernel's 16-bit staging
    X = i["X"][:, :c.K].float()
    prod = X.to(I64) @ i["W"].to(I64).t()
    exact_everywhere(L.rowproj_ref(c, i), prod, c.scale, torch.zeros(c.M, c.r), X, i["W"].t(), 64)


@pytest.mark.parametrize("c", L.COLREDUCE_CASES, ids=ids(L.COLREDUCE_CASES, L.colreduce_id))
def test_colreduce_is_exact(c):
    i = L.colreduce_inputs(c)
    round_trips(i["Y"], c.C)
    assert bool((i["G0"] != 0).all())
    Y = i["Y"][:, :c.C].float()
    prod = i["P"].to(I64).t() @ Y.to(I64)                            # [r, C]
    base = i["G0"].t() if c.g_cxr else i["G0"]
    ref = L.colreduce_ref(c, i)
    exact_everywhere(ref.t() if c.g_cxr else ref, prod, c.scale, base, i["P"].t(), Y, 32)


@pytest.mark.parametrize("c", L.GRAD_CASES, ids=ids(L.GRAD_CASES, L.grad_id))
def test_grad_is_exact(c):
    i = L.grad_inputs(c)
    assert bool((i["dA0"] != 0).all()) and bool((i["dB0"] != 0).all())
    dA, dB = L.grad_ref(c, i)
    exact_everywhere(dA, i["B"].to(I64).t() @ i["dW"].to(I64), c.s, i["dA0"], i["B"].t(), i["dW"], 8)
    exact_everywhere(dB, i["dW"].to(I64) @ i["A"].to(I64).t(), c.s, i["dB0"], i["dW"], i["A"].t(), 64)


@pytest.mark.parametrize("c", L.MERGE_CASES, ids=ids(L.MERGE_CASES, L.grad_id))
def test_merge_is_exact(c):
    i = L.merge_inputs(c)
    exact_everywhere(L.merge_ref(c, i), i["B"].to(I64) @ i["A"].to(I64), c.s, i["W"], i["B"], i["A"], 3)


@pytest.mark.parametrize("launch", L.IMAGE_LAUNCHES, ids=ids(L.IMAGE_LAUNCHES, L.image_id))
def test_images_are_exact_in_every_type_and_padding_changes_nothing(launch):
    assert sum(1 for d in launch if not d.r) >= 1 and sum(1 for d in launch if d.r) >= 2
    for n, d in enumerate(launch):
        i = L.image_inputs(d, 5000 + 10 * n)
        ref = L.image_ref(d, i)
        s, t, p = L.image_expected(d, ref)                            # (asserts that bf16 and IEEE half hold ref exactly)
        assert torch.equal(s.double(), ref) and torch.equal(t.double(), ref.t()) and p.shape == (d.R, 3 * d.C)
        assert torch.equal(p[:, :d.C].double(), ref) and torch.equal(p[:, d.C:2 * d.C], p[:, :d.C]) and not bool(p[:, 2 * d.C:].any())
        if d.r:
            den = L.denom_of(d.s)
            prod = i["B"].to(I64) @ i["A"].to(I64)
            exact_everywhere(ref, prod, d.s, i["W"], i["B"], i["A"], 3)
            assert torch.equal(ref * den, (i["W"].double() * den) + prod.double())       # in units of 1 / den: integers
            d2, i2 = L.image_padded(d, i, 5000 + 10 * n)
            assert d2.r == 2 * d.r and not bool(i2["A"][d.r:].any()) and bool(i2["B"][:, d.r:].any())
            assert torch.equal(L.image_ref(d2, i2), ref)


# ------------------------------------------------------------------------------------------------ the lists hold what they are meant to
def test_case_lists_cover_the_named_values():
    R = L.ROWPROJ_CASES
    assert {c.K for c in R} == {64, 192, 320, 1088, 2112, 3072, 8256} and {c.r for c in R} == {1, 3, 8, 9, 16}
    assert {c.M for c in R} == {1, 15, 16, 17, 12305} and {c.K for c in R if c.M == 12305} == {64}
    for f in ("w_kxr", "f16"):
        assert {getattr(c, f) for c in R} == {0, 1}
    assert {c.pad for c in R} == {0, 8} and {c.scale for c in R} == {1.0, 0.125}
    assert all(c.r <= 8 for c in R if c.K == 8256)
    C = L.COLREDUCE_CASES
    assert {c.C for c in C} == {4, 252, 256, 260, 768} and {c.r for c in C} == {1, 3, 8} and {c.M for c in C} == {1, 31, 32, 33, 4099, 32805}
    assert {c.C for c in C if c.M == 32805} == {4} and {c.pad for c in C} == {0, 4}
    assert {(c.g_cxr, c.f16) for c in C} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    G = L.GRAD_CASES
    assert {c.k_in for c in G} == {1, 63, 64, 65, 257, 513, 1024, 1025, 1028, 3072} and {c.r for c in G} == {1, 5, 8, 16}
    assert {c.n_out for c in G} == {1, 3, 4, 5, 31, 32, 33, 100, 64}
    assert any((c.n_out, c.k_in) == (100, 64) for c in G) and any((c.n_out, c.k_in) == (64, 1025) for c in G)
    M = L.MERGE_CASES
    assert {c.k_in for c in M} == {4, 12, 768, 4100} and {c.r for c in M} == {1, 5, 16} and any((c.n_out, c.k_in) == (2049, 4100) for c in M)
    D = [d for launch in L.IMAGE_LAUNCHES for d in launch]
    assert {d.r for d in D} == {0, 1, 4, 8, 16} and {d.R for d in D} == {16, 80, 768} and {d.C for d in D} == {64, 256}
    assert {(d.r > 0, d.f16) for d in D} == {(False, 0), (False, 1), (True, 0), (True, 1)}
    assert max(len(x) for x in (R, C, G, M)) <= 21


# ------------------------------------------------------------------------------------------------ 4. which branch a case reaches
def test_rowproj_geometry_of_the_named_cases():
    lens = lambda K: [ke - kb for kb, ke in L.rowproj_geometry(17, K, 8).quarters]
    assert lens(64) == [64, 0, 0, 0]                                 # wave 0 alone
    assert lens(192) == [64, 64, 64, 0]                              # wave 3 empty
    assert lens(320) == [128, 128, 64, 0]                            # wave 2 half filled, wave 3 empty
    for K in {c.K for c in L.ROWPROJ_CASES}:
        g = L.rowproj_geometry(17, K, 8)
        assert sum(lens(K)) == K and all(g.quarters[w][1] <= g.quarters[w + 1][0] for w in range(3))
        assert (max(g.trips) >= 2) == (K in (2112, 3072, 8256)), K   # a second 512-column trip inside a quarter
    assert L.rowproj_geometry(17, 2112, 8).trips == [2, 2, 2, 1] and L.rowproj_geometry(17, 3072, 8).trips == [2, 2, 2, 2]
    assert L.rowproj_geometry(17, 1088, 3, 1).staging_trips == 2 and L.rowproj_geometry(17, 320, 3, 1).staging_trips == 1
    assert L.rowproj_geometry(17, 8256, 8, 0).staging_trips == 2 and L.rowproj_geometry(17, 3072, 8, 0).staging_trips == 1
    g = L.rowproj_geometry(12305, 64, 16)
    assert (g.blocks, g.passes) == (768, 2) and L.rowproj_geometry(12288, 64, 16).passes == 1
    seen = {(L.rowproj_geometry(c.M, c.K, c.r, c.w_kxr).branch, L.rowproj_geometry(c.M, c.K, c.r).rows_w, L.rowproj_geometry(c.M, c.K, c.r, c.w_kxr).staging_trips)
            for c in L.ROWPROJ_CASES}
    # every staging branch in its one-trip and its two-trip form; the general [K, r] branch with 8 (r < 8) and with 16 staged rows
    assert seen >= {("kxr8", 8, 1), ("kxr8", 8, 2), ("kxr", 8, 1), ("kxr", 8, 2), ("kxr", 16, 1), ("kxr", 16, 2), ("rxk", 8, 1), ("rxk", 8, 2), ("rxk", 16, 1)}
    assert any(L.rowproj_geometry(c.M, c.K, c.r).passes == 2 and c.w_kxr and c.r < 8 for c in L.ROWPROJ_CASES)
    # ragged last tile and a single row
    assert {c.M % 16 for c in L.ROWPROJ_CASES} >= {0, 1, 15}


def test_colreduce_geometry_of_the_named_cases():
    for C, false_guard, groups in ((4, True, 1), (252, True, 1), (256, False, 1), (260, True, 2), (768, False, 3)):
        g = L.colreduce_geometry(33, C)
        assert (g.guard_false, g.cgs) == (false_guard, groups), C
    g = L.colreduce_geometry(32805, 4)
    assert (g.rows_per_wg, g.row_trips, g.slabs) == (64, 2, 513)
    assert L.colreduce_geometry(32768, 4).rows_per_wg == 32           # the last M with the 32-row slab
    for c in L.COLREDUCE_CASES:
        g = L.colreduce_geometry(c.M, c.C)
        assert g.slabs * g.rows_per_wg >= c.M > (g.slabs - 1) * g.rows_per_wg and g.slabs <= 1024
    assert L.colreduce_geometry(4099, 768).slabs > 1 and L.colreduce_geometry(33, 256).slabs == 2 and L.colreduce_geometry(32, 256).slabs == 1


def test_grad_geometry_of_the_named_cases():
    for k in {c.k_in for c in L.GRAD_CASES}:
        g = L.grad_geometry(33, k)
        assert g.wide == (k in (1025, 1028, 3072))
        assert g.quarters[0][0] == 0 and g.quarters[-1][1] == k and all(a[1] == b[0] for a, b in zip(g.quarters, g.quarters[1:])), k
    # the quarters tile [0, k_in) at every wide width (a quarter taken from k_in / 4 rounded DOWN would leave columns 1024.. of 1025 to nobody)
    for k in range(1025, 4300):
        q = L.grad_geometry(1, k).quarters
        assert q[0][0] == 0 and q[-1][1] == k and all(a[1] == b[0] for a, b in zip(q, q[1:])) and q[0][1] % 64 == 0, k
    assert [ke - kb for kb, ke in L.grad_geometry(1, 1025).quarters] == [320, 320, 320, 65]
    assert [ke - kb for kb, ke in L.grad_geometry(1, 1028).quarters] == [320, 320, 320, 68]
    assert L.grad_geometry(1, 513).trips == [2] and L.grad_geometry(1, 512).trips == [1] and L.grad_geometry(1, 3072).trips == [2] * 4
    a, b = L.grad_geometry(100, 64), L.grad_geometry(64, 1025)
    assert (a.nb_a, a.nb_b, a.surplus_a, a.wide) == (4, 25, 21, False)     # 21 workgroups of the dA half return at once
    assert (b.nb_a, b.nb_b, b.surplus_a, b.wide) == (10, 64, 54, True)
    assert L.grad_geometry(1, 3072).surplus_b == 11 and L.grad_geometry(3, 1024).surplus_b == 3      # ... and of the dB half, wide and narrow
    assert {c.n_out % 32 for c in L.GRAD_CASES} >= {0, 1, 31} and any(L.grad_geometry(c.n_out, c.k_in).ragged_slab for c in L.GRAD_CASES)


def test_merge_and_image_launches():
    assert L.merge_launch(2049, 4100) == (8192, 2)
    assert all(L.merge_launch(c.n_out, c.k_in)[1] == 1 for c in L.MERGE_CASES if c.n_out != 2049)
    assert L.image_tiles(80, 256) == 8 and L.image_tiles(16, 64) == 1 and L.image_tiles(768, 64) == 12


# ------------------------------------------------------------------------------------------------ 5. the faults are seen
def differs(a, b):
    return a.shape == b.shape and not torch.equal(a, b)


@pytest.mark.parametrize("c", L.ROWPROJ_CASES, ids=ids(L.ROWPROJ_CASES, L.rowproj_id))
def test_rowproj_faults_are_seen(c):
    i = L.rowproj_inputs(c)
    ref = L.rowproj_ref(c, i)
    assert differs(L.rowproj_ref(c, i, "last_row"), ref)
    for q, (kb, ke) in enumerate(L.rowproj_geometry(c.M, c.K, c.r).quarters):
        if ke > kb:
            assert differs(L.rowproj_ref(c, i, "quarter", q), ref), q
    if c.r > 1:
        assert differs(L.rowproj_ref(c, i, "rank_shift"), ref)
        if c.w_kxr:
            assert differs(L.rowproj_ref(c, i, "layout"), ref)
    if c.f16:
        assert differs(L.rowproj_ref(c, i, "decode"), ref)


@pytest.mark.parametrize("c", L.COLREDUCE_CASES, ids=ids(L.COLREDUCE_CASES, L.colreduce_id))
def test_colreduce_faults_are_seen(c):
    i = L.colreduce_inputs(c)
    ref = L.colreduce_ref(c, i)
    for fault in ("last_row", "last_colgroup", "assign") + (("rank_shift", "layout") if c.r > 1 else ()) + (("decode",) if c.f16 else ()):
        assert differs(L.colreduce_ref(c, i, fault), ref), fault


@pytest.mark.parametrize("c", L.GRAD_CASES, ids=ids(L.GRAD_CASES, L.grad_id))
def test_grad_faults_are_seen(c):
    i = L.grad_inputs(c)
    dA, dB = L.grad_ref(c, i)
    for fault in ("last_row", "last_colgroup", "assign") + (("rank_shift",) if c.r > 1 else ()):
        wA, wB = L.grad_ref(c, i, fault)
        assert differs(wA, dA) and differs(wB, dB), fault
    g = L.grad_geometry(c.n_out, c.k_in)
    if g.wide:
        for q in range(4):
            assert differs(L.grad_ref(c, i, "quarter", q)[1], dB), q


@pytest.mark.parametrize("c", L.MERGE_CASES, ids=ids(L.MERGE_CASES, L.grad_id))
def test_merge_faults_are_seen(c):
    i = L.merge_inputs(c)
    ref = L.merge_ref(c, i)
    for fault in ("last_row", "last_colgroup") + (("rank_shift",) if c.r > 1 else ()):
        assert differs(L.merge_ref(c, i, fault), ref), fault


def test_image_faults_are_seen():
    for launch in L.IMAGE_LAUNCHES:
        for n, d in enumerate(launch):
            if d.r:
                i = L.image_inputs(d, 5000 + 10 * n)
                ref = L.image_ref(d, i)
                for fault in ("last_row", "last_colgroup") + (("rank_shift",) if d.r > 1 else ()):
                    assert differs(L.image_ref(d, i, fault), ref), (d, fault)


# ------------------------------------------------------------------------------------------------ 6. argument checks
def test_cases_pass_and_refusals_fail_the_argument_checks():
    assert all(L.rowproj_args_ok(c.M, c.K, c.K + c.pad, c.r) for c in L.ROWPROJ_CASES)
    assert all(L.colreduce_args_ok(c.M, c.C, c.C + c.pad, c.r) for c in L.COLREDUCE_CASES)
    assert all(L.grad_args_ok(*c[:3]) for c in L.GRAD_CASES) and all(L.merge_args_ok(*c[:3]) for c in L.MERGE_CASES)
    assert not any(L.rowproj_args_ok(16, a["K"], a["ldx"], a["r"]) for a in L.ROWPROJ_REFUSALS)
    assert not any(L.colreduce_args_ok(16, a["C"], a["ldy"], a["r"]) for a in L.COLREDUCE_REFUSALS)
    assert not any(L.grad_args_ok(**a) for a in L.GRAD_REFUSALS) and not any(L.merge_args_ok(**a) for a in L.MERGE_REFUSALS)
    # the LDS limit sits exactly between the largest accepted width and the refused one
    assert L.rowproj_args_ok(16, 4800, 4800, 16) and L.rowproj_args_ok(16, 9664, 9664, 8) and L.rowproj_args_ok(16, 8256, 8264, 8)
