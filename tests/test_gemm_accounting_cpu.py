"""The kernel timer's GEMM accounting (ops._flops_of / _bytes_of / _shape_of): one argument tuple per GEMM entry point in its C signature's
order (include/sed_hip.h, stream left out), against recorded values.  The roofline line of bench.py is built from these numbers and nothing
else reads them back, so a shifted argument index would otherwise go unnoticed.  No GPU."""
import pytest

from transformer4sed_amd import ops

M, K, H, N, N4 = 1024, 768, 12, 768, 3072
A, B, X = "A", "B", "x"      # stand-ins for tensors: the accounting only tests pointers for None
CASES = [
    # (label, entry point, arguments in the C signature's order, without the stream)
    ("nt_f32", "sed_gemm_nt", (A, B, M, N, K, K, K, 0, X, None, X, None, None, None, N, 1.0, 1, 0)),
    ("nt_gelu_both", "sed_gemm_nt", (A, B, M, N4, K, K, K, 3, X, None, None, X, X, None, N4, 1.0, 1, 1)),
    ("nt_gb_gelu_one", "sed_gemm_nt_gb", (A, B, M, N4, K, K, K, 3, X, None, None, None, X, None, N4, 1.0, 1, X, 256)),
    ("nt_gb_e4m3", "sed_gemm_nt_gb_e4m3", (A, B, M, N4, K, K, K, X, X, N4 + N4 // 2, X, 256)),
    ("nt_w2_resid", "sed_gemm_nt_w2", (A, B, M, N, N4, N4, 2 * N4, 1, X, X, X, None, None, N, 1)),
    ("nt_w2_gelu", "sed_gemm_nt_w2", (A, B, M, N4, K, K, 2 * K, 3, X, None, None, None, X, N4, 1)),
    ("nt_w2f8_gelu", "sed_gemm_nt_w2f8", (A, B, M, N4, K, K + K // 2, K + K // 2, 3, X, None, None, None, X, N4 + N4 // 2, 1, 4)),
    ("nt_w2f8_resid", "sed_gemm_nt_w2f8", (A, B, M, N, N4, N4 + N4 // 2, N4 + N4 // 2, 1, X, X, X, None, None, N, 0, 4)),
    ("nt_lnp_f32", "sed_gemm_nt_lnp", (A, B, M, N, K, K, K, X, X, None, None, X, X, None, X, N)),
    ("nt_lnp_planes", "sed_gemm_nt_lnp", (A, B, M, N, K, K, K, X, None, X, X, None, X, X, X, N)),
    ("nt_lnp8_planes_f32out", "sed_gemm_nt_lnp8", (A, B, M, N, N4, N4, N4, X, None, X, X, X, X, None, X, N)),
    ("nt_lnp8_planes_planes", "sed_gemm_nt_lnp8", (A, B, M, N, N4, 64, N4, X, None, X, X, None, X, X, X, N)),
    ("nt_lnc", "sed_gemm_nt_lnc", (A, B, M, N4, K, K, K, X, X, X, X, N4)),
    ("nt_lnc8", "sed_gemm_nt_lnc8", (A, B, M, N4, K, K, K, X, X, X, X, 64)),
    ("qkv_lnc", "sed_gemm_qkv_lnc", (A, B, X, X, X, M, K, H, 256, 256, X, X, X)),
    ("qkv_lnc8", "sed_gemm_qkv_lnc8", (A, B, X, X, X, M, K, H, 256, 256, X, X, None)),
    ("qkv_3", "sed_gemm_qkv", (A, B, X, M, K, H, 256, 256, X, X, X, None, None, None, None, None, None, None, 1)),
    ("qkv_8", "sed_gemm_qkv", (A, B, X, M, K, H, 256, 256, X, X, X, X, X, X, X, X, X, X, 3)),
    ("qkv_w2s_8", "sed_gemm_qkv_w2s", (A, B, X, M, K, H, 256, 256, X, X, X, X, X, X, X, X, X, X, 1)),
    ("qkv_gb", "sed_gemm_qkv_gb", (A, B, X, M, K, H, 256, 256, X, X, None, 1, X, 256)),
    ("qkv_w2", "sed_gemm_qkv_w2", (A, B, X, M, K, H, 256, 256, X, X, None, 1)),
    ("qkv_w2f8", "sed_gemm_qkv_w2f8", (A, B, X, M, K, H, 256, 256, X, X, X, 4)),
    ("dw_tn", "sed_gemm_dw_tn", (A, B, 1, M, N4, K, N4, K, X, K, X, X, 1 << 20)),
]

# (flops, bytes, shape) of each case: what the three functions returned before they shared one table
EXPECTED = {
    "nt_f32": (1207959552.0, 5898240.0, (1024, 768, 768, "epi0")),
    "nt_gelu_both": (4831838208.0, 18874368.0, (1024, 3072, 768, "epi3")),
    "nt_gb_gelu_one": (4831838208.0, 12582912.0, (1024, 3072, 768, "epi3gb")),
    "nt_gb_e4m3": (4831838208.0, 0.0, None),
    "nt_w2_resid": (4831838208.0, 22020096.0, (1024, 768, 3072, "epi1w2")),
    "nt_w2_gelu": (4831838208.0, 17301504.0, (1024, 3072, 768, "epi3w2")),
    "nt_w2f8_gelu": (4831838208.0, 15728640.0, (1024, 3072, 768, "epi3w2f8")),
    "nt_w2f8_resid": (4831838208.0, 22806528.0, (1024, 768, 3072, "epi1w2f8")),
    "nt_lnp_f32": (1207959552.0, 10616832.0, (1024, 768, 768, "epi1lnp")),
    "nt_lnp_planes": (1207959552.0, 9043968.0, (1024, 768, 768, "epi1lnp")),
    "nt_lnp8_planes_f32out": (4831838208.0, 18087936.0, (1024, 768, 3072, "epi1lnp")),
    "nt_lnp8_planes_planes": (4831838208.0, 15728640.0, (1024, 768, 3072, "epi1lnp")),
    "nt_lnc": (4831838208.0, 12582912.0, (1024, 3072, 768, "epi3lnc")),
    "nt_lnc8": (4831838208.0, 12582912.0, (1024, 3072, 768, "epi3lnc")),
    "qkv_lnc": (3623878656.0, 9830400.0, (1024, 2304, 768, "qkv3lnc")),
    "qkv_lnc8": (3623878656.0, 9830400.0, (1024, 2304, 768, "qkv3lnc")),
    "qkv_3": (3623878656.0, 9830400.0, (1024, 2304, 768, "qkv3")),
    "qkv_8": (3623878656.0, 17694720.0, (1024, 2304, 768, "qkv8")),
    "qkv_w2s_8": (3623878656.0, 21233664.0, (1024, 2304, 768, "qkv8w2s")),
    "qkv_gb": (3623878656.0, 9830400.0, (1024, 2304, 768, "qkv3gb")),
    "qkv_w2": (3623878656.0, 13369344.0, (1024, 2304, 768, "qkv3w2")),
    "qkv_w2f8": (3623878656.0, 12386304.0, (1024, 2304, 768, "qkv3w2f8")),
    "dw_tn": (4831838208.0, 26738688.0, (3072, 768, 1024, "tn")),
}

GEMM_ENTRY_POINTS = {"sed_gemm_nt", "sed_gemm_nt_gb", "sed_gemm_nt_gb_e4m3", "sed_gemm_nt_w2", "sed_gemm_nt_w2f8", "sed_gemm_nt_lnp",
                     "sed_gemm_nt_lnp8", "sed_gemm_nt_lnc", "sed_gemm_nt_lnc8", "sed_gemm_qkv_lnc", "sed_gemm_qkv_lnc8", "sed_gemm_qkv",
                     "sed_gemm_qkv_gb", "sed_gemm_qkv_w2", "sed_gemm_qkv_w2f8", "sed_gemm_qkv_w2s", "sed_gemm_dw_tn"}


def test_every_gemm_entry_point_has_a_case():
    assert {name for _, name, _ in CASES} == GEMM_ENTRY_POINTS
    assert {label for label, _, _ in CASES} == set(EXPECTED)


@pytest.mark.parametrize("label,name,args", CASES, ids=[c[0] for c in CASES])
def test_gemm_accounting(label, name, args):
    flops, nbytes, shape = EXPECTED[label]
    assert ops._flops_of(name, args) == flops
    assert ops._bytes_of(name, args) == nbytes
    assert ops._shape_of(name, args) == shape


def test_names_outside_the_table_are_not_accounted():
    assert ops._flops_of("sed_layernorm_fwd", (None,) * 12) == 0.0
    assert ops._bytes_of("sed_layernorm_fwd", (None,) * 12) == 0.0
    assert ops._shape_of("sed_layernorm_fwd", (None,) * 12) is None
