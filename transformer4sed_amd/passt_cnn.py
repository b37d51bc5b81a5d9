"""`PaSST_CNN` -- drop-in for the reference's PMAM model class (src/models/cnn_transformer/passt_cnn.py:9-91): PaSST encoder with
LoRA linears, a 10-layer CNN branch, attention frequency pooling and a 384-wide Transformer-XL context network.  Constructor
kwargs (`passt_sed_param`, `cnn_param`), forward signature / return values, parameter and buffer names (state_dict interchange,
including the BatchNorm running statistics and the eval-mode LoRA weight folding) follow the reference; forward runs on the HIP
kernels of the pmam_engine package.  The nn.Modules are parameter containers only."""
import re

import torch
import torch.nn as nn

from .passt_sed import PaSST_SED, _Holder
from .pmam_engine import PmamEngine


class _CG(_Holder):
    def __init__(self, n):
        super().__init__()
        self.linear = nn.Linear(n, n)


class _CNN(_Holder):
    """Parameter layout of `CNN` (src/models/cnn/base.py:33-98) for activation 'cg' / normalization 'batch'."""

    def __init__(self, n_in_channel, nb_filters):
        super().__init__()
        self.cnn = nn.Sequential()
        cin = n_in_channel
        for i, co in enumerate(nb_filters):
            self.cnn.add_module(f"conv{i}", nn.Conv2d(cin, co, 3, 1, 1))
            self.cnn.add_module(f"batchnorm{i}", nn.BatchNorm2d(co, eps=0.001, momentum=0.99))
            self.cnn.add_module(f"cg{i}", _CG(co))
            cin = co


class _FdyAttention(_Holder):
    """Parameter layout of `attention2d` (src/models/cnn/FDY_cnn.py:66-93) for pool_dim 'freq'."""

    def __init__(self, cin, n_basis):
        super().__init__()
        hid = max(cin // 4, 4)
        self.conv1d1 = nn.Conv1d(cin, hid, 3, stride=1, padding=1, bias=False)
        self.bn = nn.BatchNorm1d(hid)
        self.conv1d2 = nn.Conv1d(hid, n_basis, 1, bias=True)
        for mod in (self.conv1d1, self.conv1d2):
            nn.init.kaiming_normal_(mod.weight, mode="fan_out", nonlinearity="relu")
        nn.init.constant_(self.conv1d2.bias, 0)


class _DynamicConv2d(_Holder):
    """Parameter layout of `Dynamic_conv2d` (FDY_cnn.py:7-32): `weight` [n_basis, co, cin, 3, 3], no bias, and the attention head."""

    def __init__(self, cin, co, n_basis=4):
        super().__init__()
        self.attention = _FdyAttention(cin, n_basis)
        self.weight = nn.Parameter(torch.randn(n_basis, co, cin, 3, 3))
        for k in range(n_basis):
            nn.init.kaiming_normal_(self.weight.data[k])


class _FDY_CNN(_Holder):
    """Parameter layout of `FDY_CNN` (FDY_cnn.py:119-173) for activation 'cg' / normalization 'batch': the base branch's modules, with
    `conv{i}` a `Dynamic_conv2d` where DY_layers[i] == 1."""

    def __init__(self, n_in_channel, nb_filters, dy_layers):
        super().__init__()
        self.cnn = nn.Sequential()
        cin = n_in_channel
        for i, co in enumerate(nb_filters):
            self.cnn.add_module(f"conv{i}", _DynamicConv2d(cin, co) if dy_layers[i] else nn.Conv2d(cin, co, 3, 1, 1))
            self.cnn.add_module(f"batchnorm{i}", nn.BatchNorm2d(co, eps=0.001, momentum=0.99))
            self.cnn.add_module(f"cg{i}", _CG(co))
            cin = co


_BASE_KEYS = ("n_in_channel", "kernel_size", "padding")      # `CNN`'s names (base.py:36-45) of what `FDY_CNN` calls n_input_ch / kernel / pad
_FDY_KEYS = ("n_input_ch", "activation", "conv_dropout", "kernel", "pad", "stride", "nb_filters", "pooling", "normalization",
             "n_basis_kernels", "DY_layers", "temperature", "pool_dim")


class PaSST_CNN(PaSST_SED):
    def __init__(self, passt_sed_param, cnn_param):
        super().__init__(**passt_sed_param, _pmam=True)
        if cnn_param is None:
            raise NotImplementedError("PaSST_CNN without the CNN branch is PaSST_SED")
        cp = dict(cnn_param)
        bad = []
        self.cnn_name = cp.pop("cnn_name", "base")
        fdy = self.cnn_name == "FDY-CNN"
        if self.cnn_name not in ("base", "FDY-CNN"):      # (each branch has its own key names: nothing else of the dict can be judged)
            raise NotImplementedError(f"the HIP PaSST_CNN path covers the PMAM configs only; unsupported: cnn_name={self.cnn_name!r} (not 'base' / 'FDY-CNN')")
        if fdy:
            # `FDY_CNN(**cnn_param)` (passt_cnn.py:28) takes its own key names (FDY_cnn.py:120-133); `CNN`'s are a TypeError there
            for k in cp:
                if k not in _FDY_KEYS:
                    bad.append(f"{k} (not a key of FDY_CNN" + ("; CNN's name" if k in _BASE_KEYS else "") + ")")
            cp = dict(cp, n_in_channel=cp.get("n_input_ch"), kernel_size=cp.get("kernel", [3, 3, 3]), padding=cp.get("pad", [1, 1, 1]))
            if "n_input_ch" not in cnn_param: bad.append("n_input_ch missing")
            cp.setdefault("nb_filters", [64, 64, 64])
            cp.setdefault("pooling", [(1, 4), (1, 4), (1, 4)])
            cp.setdefault("stride", [1, 1, 1])
        if cp.get("activation", "Relu").lower() != "cg": bad.append("activation != 'cg'")
        if cp.get("normalization", "batch") != "batch": bad.append("normalization != 'batch'")
        n = len(cp["nb_filters"])
        if cp.get("n_in_channel", 1) != 1: bad.append("n_input_ch != 1" if fdy else "n_in_channel != 1")
        if list(cp["kernel_size"]) != [3] * n or list(cp["padding"]) != [1] * n or list(cp["stride"]) != [1] * n:
            bad.append("only 3x3 / pad 1 / stride 1 convolutions")
        if any(c % 16 for c in cp["nb_filters"]): bad.append("filter counts must be multiples of 16")
        if "cnn_1d_dict" in cp: bad.append("cnn_1d_dict")
        dy = [0] * n
        if fdy:
            dy = list(cp.get("DY_layers", [0, 1, 1, 1, 1, 1, 1]))
            if cp.get("n_basis_kernels", 4) != 4: bad.append("n_basis_kernels != 4")
            if cp.get("pool_dim", "freq") != "freq": bad.append("pool_dim != 'freq'")
            if not float(cp.get("temperature", 31)) > 0: bad.append("temperature <= 0")
            if len(dy) != n or any(d not in (0, 1) for d in dy): bad.append("DY_layers must be a 0/1 list of the stack's length")
            elif dy[0] != 0: bad.append("DY_layers[0] != 0 (a dynamic first layer)")
        if bad:
            raise NotImplementedError("the HIP PaSST_CNN path covers the PMAM configs only; unsupported: " + ", ".join(bad))
        self.cnn_filters = tuple(cp["nb_filters"])
        self.cnn_pooling = tuple(tuple(p) for p in cp["pooling"])
        self.conv_dropout = float(cp.get("conv_dropout", 0) or 0)
        fr = 128
        for _, pw in self.cnn_pooling:
            fr //= pw
        if fr != 1:
            raise NotImplementedError("the CNN branch must pool the 128 mel bins down to 1 (passt_cnn.py:53)")
        self.cnn_dynamic = tuple(bool(d) for d in dy)       # per layer: frequency-dynamic convolution (FDY_cnn.py:143-150)
        self.cnn_temperature = float(cp.get("temperature", 31)) if fdy else None
        self.cnn = _FDY_CNN(1, self.cnn_filters, dy) if fdy else _CNN(1, self.cnn_filters)
        self.cnn_feat_dim = self.cnn_filters[-1]
        self.cnn_projector = nn.Linear(self.cnn_feat_dim, self.decoder_dim)
        self.merge_weight = nn.Parameter(torch.tensor([0.5]), requires_grad=bool(self.mlm))
        self.transformer_projector = nn.Linear(self.embed_dim, self.decoder_dim)
        self._drop_masks = None      # tests may inject the per-layer dropout masks ([B*H*W, C] uint8, layer order)
        self._mask_always_effective = True   # the merged sequence is contiguous: mask.py:66-80 writes in place (cf. DESIGN quirk 15)
        self._index_params()

    def _make_engine(self):
        return PmamEngine(self)

    def _grad_names(self):
        """Parameters the PMAM losses reach (the reference leaves `.grad` None on the others): the classifier is unused in MLM mode;
        the AT head, the final norm and the encoder blocks above the feature layer only through `at_out`."""
        at = getattr(self, "_at_grad_seen", False)
        names = set()
        for n, p in self._param_by_name.items():
            if not p.requires_grad or n.startswith("backbone.head") or (self.mlm and n.startswith("classifier.")):
                continue
            if n.startswith(("at_adpater", "backbone.norm.")) and not at:
                continue
            mt = re.match(r"backbone\.blocks\.(\d+)\.", n)
            if mt and int(mt.group(1)) >= self.passt_feature_layer and not at:
                continue
            names.add(n)
        return names

    def get_model_name(self):
        return "PaSST_CNN"
