"""CPU-side checks of the boundary: libsed_hip.so builds/loads and exports exactly the C ABI of include/sed_hip.h;
the product path refuses to run without a HIP device (no fallback)."""
import ctypes
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    from transformer4sed_amd import build
    return build.build(verbose=False)


def test_library_exports_every_declared_symbol(built):
    from transformer4sed_amd import _lib
    protos = _lib.parse_header()
    assert len(protos) >= 30
    dll = ctypes.CDLL(built)
    for name in protos:
        assert hasattr(dll, name), f"{name} declared in include/sed_hip.h but not exported"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", built]).decode()
    extra = [l.split()[-1] for l in exported.splitlines() if " T sed_" in l and l.split()[-1] not in protos]
    assert not extra, f"exported but undeclared: {extra}"
    assert _lib.lib() is not None


def test_every_hip_source_is_built():
    from transformer4sed_amd import build
    on_disk = {f for f in os.listdir(build.CSRC) if f.endswith(".hip")}
    assert on_disk == set(build.SOURCES), f"csrc/*.hip and build.SOURCES differ: {sorted(on_disk ^ set(build.SOURCES))}"
    assert len(build.SOURCES) == len(set(build.SOURCES))


def test_header_cites_reference_for_every_entry():
    src = open(os.path.join(ROOT, "include", "sed_hip.h")).read()
    for token in ("passt_feature_extraction.py", "data_aug.py", "filter.py", "decoder.py", "passt.py", "transformerXL.py",
                  "passt_sed.py", "pooling.py", "mask.py", "encoder_slide_window.py", "scheduler.py", "setting.py"):
        assert token in src, token


def test_product_fails_loudly_without_gpu():
    from transformer4sed_amd.passt_sed import PaSST_SED
    net = PaSST_SED(decoder="transformerXL", decoder_layer_num=3, at_adapter=True, load_pretrained_model=False,
                    encoder_depth=1, passt_feature_layer=1)
    with pytest.raises(RuntimeError, match="no CPU fallback|MI355X"):
        net(torch.zeros(1, 128, 1000))
    from transformer4sed_amd.filter import median_filter_torch
    with pytest.raises(RuntimeError):
        median_filter_torch(torch.zeros(1, 10, 10), [3] * 10)


def test_product_never_imports_oracle():
    import re
    pkg = os.path.join(ROOT, "transformer4sed_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            assert not re.search(r"^\s*(from|import)\s+oracle", open(os.path.join(pkg, fn)).read(), flags=re.M), fn


def test_state_dict_contract_and_param_groups():
    """Key names / shapes of SURVEY 8(b) and the name patterns get_params relies on
    (recipes/desed/finetune/passt/setting.py:28-103)."""
    from transformer4sed_amd import synth
    from transformer4sed_amd.passt_sed import PaSST_SED
    for mlm in (False, True):
        kw = dict(mlm_dict=dict(strategy="block", block_width=10, mask_rate=0.75, out_dim=768)) if mlm else {}
        net = PaSST_SED(decoder="transformerXL", decoder_layer_num=3, at_adapter=True, load_pretrained_model=False,
                        mlm=mlm, **kw)
        want = synth.matsed_param_shapes(mlm=mlm)
        got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        assert got == want
    names = [k for k, _ in net.backbone.named_parameters()]
    assert any(k.startswith("blocks.11.") for k in names) and "norm.weight" in names
    assert net.get_model_name() == "PaSST_SED" and net.get_backbone_upsample_ratio() == 10
