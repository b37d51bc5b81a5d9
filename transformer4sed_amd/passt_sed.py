"""`PaSST_SED` -- drop-in for the reference model class (src/models/passt/passt_sed.py:37-308) whose forward and
backward run entirely on hand-written gfx950 kernels (the engine/ package).

Contract kept: constructor kwargs, forward signature and return values, accessors
(`get_feature_extractor`, `get_model_name`, `get_backbone_upsample_ratio`, `get_backbone`), sub-module / parameter
names (so `state_dict()` interchanges with reference checkpoints and `recipes/desed/finetune/passt/setting.py`
`get_params` works on `net.backbone.named_parameters()`), train/eval RNG behaviour.  The nn.Modules below are
parameter containers only; their torch `forward`s are never used.
"""
import math
from collections.abc import Sequence

import torch
import torch.nn as nn

from .engine import SedEngine, window_starts, D, H, FPOOL_TRANSFORMER
from .frontend import PasstFeatureExtractor


class SEDModel(nn.Module):
    """src/models/sed_model.py:7-24."""

    def get_feature_extractor(self):
        raise NotImplementedError

    def get_model_name(self) -> str:
        raise NotImplementedError

    def get_backbone_upsample_ratio(self):
        raise NotImplementedError


class _Holder(nn.Module):
    def forward(self, *a, **k):
        raise RuntimeError("parameter container: the MAT-SED forward runs in transformer4sed_amd.engine (HIP)")


class _LoraLinear(nn.Linear):
    """Parameter layout and train/eval weight folding of the reference's LoRA linear (src/models/lora/layers.py:88-153): frozen
    `weight` (+ bias), trainable `lora_A` [r, in] / `lora_B` [out, r]; `eval()` folds scaling * B A into `weight`, `train()` takes it
    out again, so a state_dict saved after `eval()` holds merged weights exactly like the reference's checkpoints."""

    def __init__(self, n_in, n_out, r, lora_alpha=1, requires_grad_pretrain=False):
        super().__init__(n_in, n_out)
        self.r, self.scaling, self.merged = r, lora_alpha / r, False
        self.lora_A = nn.Parameter(torch.zeros(r, n_in))
        self.lora_B = nn.Parameter(torch.zeros(n_out, r))
        nn.init.kaiming_uniform_(self.lora_A, a=math.sqrt(5))
        self.weight.requires_grad = requires_grad_pretrain

    def train(self, mode=True):
        super().train(mode)
        if mode == self.merged:   # entering train while merged, or entering eval while unmerged
            with torch.no_grad():
                self.weight.add_(self.lora_B @ self.lora_A, alpha=-self.scaling if mode else self.scaling)
            self.merged = not mode
        return self

    def forward(self, *a, **k):
        raise RuntimeError("parameter container: the forward runs in transformer4sed_amd.pmam_engine (HIP)")


def _linear(n_in, n_out, lora):
    return _LoraLinear(n_in, n_out, **lora) if lora else nn.Linear(n_in, n_out)


class _Mlp(_Holder):
    def __init__(self, dim, hidden, lora=None):
        super().__init__()
        self.fc1 = _linear(dim, hidden, lora)
        self.fc2 = _linear(hidden, dim, lora)


class _Attn(_Holder):
    def __init__(self, dim, lora=None):
        super().__init__()
        self.qkv = _linear(dim, 3 * dim, lora)
        self.proj = _linear(dim, dim, lora)


class _Block(_Holder):
    def __init__(self, dim, mlp_ratio, eps, lora=None):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=eps)
        self.attn = _Attn(dim, lora)
        self.norm2 = nn.LayerNorm(dim, eps=eps)
        self.mlp = _Mlp(dim, int(dim * mlp_ratio), lora)


class _PatchEmbed(_Holder):
    def __init__(self, dim):
        super().__init__()
        self.proj = nn.Conv2d(1, dim, kernel_size=16, stride=10)


def patchout_f(s):
    """`s_patchout_f` (passt.py:533-547: how many of the 12 frequency rows of the patch grid a training-mode backbone call drops) as a
    checked int.  12 would leave an empty sequence (NaN in the reference) and is refused."""
    if isinstance(s, bool) or not isinstance(s, int):
        raise TypeError(f"s_patchout_f must be an int, got {s!r}")
    if not 0 <= s <= 11:
        raise ValueError(f"s_patchout_f must lie in [0, 11] (12 frequency rows, at least one is kept), got {s!r}")
    return s


def patchout_rows(rows, s, n_sets):
    """Injected row sets (tests): `n_sets` lists (the global pass, then one per window) of 12 - s strictly increasing ints in [0, 12)."""
    rows = [[r for r in rs] for rs in rows]
    if len(rows) != n_sets:
        raise ValueError(f"_patchout_rows: {len(rows)} row sets for {n_sets} backbone calls (the global pass + one per window)")
    for rs in rows:
        if any(isinstance(r, bool) or not isinstance(r, int) for r in rs):
            raise TypeError(f"_patchout_rows must hold ints, got {rs!r}")
        if len(rs) != 12 - s or any(not 0 <= r < 12 for r in rs) or any(a >= b for a, b in zip(rs, rs[1:])):
            raise ValueError(f"_patchout_rows: expected {12 - s} strictly increasing rows in [0, 12), got {rs!r}")
    return rows


class _Backbone(_Holder):
    """Parameter layout of `PaSST` (src/models/passt/passt.py:392-452)."""

    def __init__(self, dim, depth, lora=None, s_patchout_f=0):
        super().__init__()
        self.s_patchout_f = s_patchout_f    # (read at every forward, as in the reference; deepcopy carries it to the EMA teacher)
        self.patch_embed = _PatchEmbed(dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, dim))
        self.dist_token = nn.Parameter(torch.zeros(1, 1, dim))
        self.new_pos_embed = nn.Parameter(torch.zeros(1, 2, dim))
        self.freq_new_pos_embed = nn.Parameter(torch.zeros(1, dim, 12, 1))
        self.time_new_pos_embed = nn.Parameter(torch.zeros(1, dim, 1, 99))
        self.blocks = nn.Sequential(*[_Block(dim, 4, 1e-6, lora) for _ in range(depth)])
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        # dead parameters kept for checkpoint compatibility (never used in forward)
        self.head = nn.Sequential(nn.LayerNorm(dim), _linear(dim, 527, lora))
        self.head_dist = _linear(dim, 527, lora)
        for t in (self.cls_token, self.dist_token, self.new_pos_embed, self.freq_new_pos_embed, self.time_new_pos_embed):
            nn.init.trunc_normal_(t, std=0.02)
        for mod in self.modules():
            if isinstance(mod, nn.Linear):
                with torch.no_grad():
                    nn.init.trunc_normal_(mod.weight, std=0.02)
                nn.init.zeros_(mod.bias)


class _RelAttn(_Holder):
    def __init__(self, dim, heads):
        super().__init__()
        self.in_proj = nn.Linear(dim, 3 * dim, bias=True)
        self.out_proj = nn.Linear(dim, dim, bias=True)
        self.linear_pos = nn.Linear(dim, dim, bias=False)
        self.pos_bias_u = nn.Parameter(torch.empty(heads, dim // heads))
        self.pos_bias_v = nn.Parameter(torch.empty(heads, dim // heads))
        nn.init.xavier_uniform_(self.in_proj.weight)
        nn.init.constant_(self.in_proj.bias, 0.0)
        nn.init.constant_(self.out_proj.bias, 0.0)
        nn.init.xavier_uniform_(self.pos_bias_u)
        nn.init.xavier_uniform_(self.pos_bias_v)


class _XLBlock(_Holder):
    def __init__(self, dim, heads):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.attn = _RelAttn(dim, heads)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = _Mlp(dim, dim)  # mlp_ratio 1 (src/models/transformer_decoder.py:84,91)


def band_half_widths(win_len, heads):
    """`decoder_win_len` (an int, or one int per head: transformer_decoder.py:96-103) -> the per-head half widths hw = w // 2 of
    mask.py:7-23.  A width below 2 masks whole rows (the reference then yields NaN) and is refused."""
    if isinstance(win_len, bool) or not isinstance(win_len, (int, Sequence)) or isinstance(win_len, (str, bytes)):
        raise TypeError(f"decoder_win_len must be an int or a sequence of {heads} ints, got {win_len!r}")
    per_head = not isinstance(win_len, int)
    widths = list(win_len) if per_head else [win_len] * heads
    if len(widths) != heads:
        raise ValueError(f"decoder_win_len: {len(widths)} widths for {heads} heads")
    if any(isinstance(w, bool) or not isinstance(w, int) for w in widths):
        raise TypeError(f"decoder_win_len must hold ints, got {win_len!r}")
    if any(w < 2 for w in widths):
        raise ValueError(f"decoder_win_len: a width below 2 masks whole rows of the attention matrix (NaN in the reference), got {win_len!r}")
    return [w // 2 for w in widths], per_head


def band_mask(seq_len, hw):
    """mask.py:7-23 `diagonal_mask(seq_len, w)` in closed form for hw = w // 2: True = masked; query i sees the keys
    max(0, i - hw) <= j < min(seq_len, i + hw) -- hw to the left, itself, hw - 1 to the right."""
    i = torch.arange(seq_len).unsqueeze(1)
    j = torch.arange(seq_len).unsqueeze(0)
    return ~((j >= i - hw) & (j < i + hw))


class _Decoder(_Holder):
    def __init__(self, dim, layers, heads, seq_len=1000, win_len=None):
        super().__init__()
        self.encoder_blocks = nn.ModuleList([_XLBlock(dim, heads) for _ in range(layers)])
        self.seq_len = seq_len
        self.half_widths = None          # per-head hw (ints) when a local window is set
        self._hw_dev = {}                # device -> int32 [heads], what the band kernels read
        mask = None
        if win_len is not None:
            self.half_widths, per_head = band_half_widths(win_len, heads)
            mask = torch.stack([band_mask(seq_len, hw) for hw in self.half_widths]) if per_head else band_mask(seq_len, self.half_widths[0])
        # the reference's persistent buffer (transformer_decoder.py:108): [T, T] or [heads, T, T] bool, absent from the state_dict
        # without a window.  Checkpoint interchange only -- the kernels take the band from `half_widths`.
        self.register_buffer("att_mask", mask)

    def half_width_tensor(self, dev):
        t = self._hw_dev.get(dev)
        if t is None:
            t = self._hw_dev[dev] = torch.tensor(self.half_widths, dtype=torch.int32, device=dev)
        return t

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        key = prefix + "att_mask"
        got = state_dict.get(key)
        if self.att_mask is not None and got is not None and tuple(got.shape) == tuple(self.att_mask.shape) \
                and not torch.equal(got.to(self.att_mask.device, torch.bool), self.att_mask):
            error_msgs.append(f"{key} is not the diagonal band of this model's decoder_win_len: the attention kernels express "
                              "diagonal bands only (hw = w // 2 keys to the left, hw - 1 to the right)")
            state_dict = {k: v for k, v in state_dict.items() if k != key}
            state_dict[key] = self.att_mask
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)


class _ConvModule(_Holder):
    """Parameter layout of `ConvolutionModule` (src/models/transformer/conformer.py:155-213); the convolutions keep their Conv1d shapes
    ([out, in, 1], [channels, 1, 31]) and torch's default initialisation."""

    def __init__(self, dim, kernel_size=31):
        super().__init__()
        self.pointwise_conv1 = nn.Conv1d(dim, 2 * dim, kernel_size=1)
        self.depthwise_conv = nn.Conv1d(dim, dim, kernel_size, padding=(kernel_size - 1) // 2, groups=dim)
        self.norm = nn.LayerNorm(dim)
        self.pointwise_conv2 = nn.Conv1d(dim, dim, kernel_size=1)


class _Identity(nn.Module):
    """Parameter-free placeholder that keeps the reference's nn.Sequential indices (Swish at 1, Dropout at 2)."""


class _ConformerBlock(_Holder):
    """Parameter layout of `ConformerEncoderLayer` (conformer.py:32-73), in the reference's registration order."""

    def __init__(self, dim, heads):
        super().__init__()
        self.self_attn = _RelAttn(dim, heads)
        self.feed_forward = nn.Sequential(nn.Linear(dim, dim), _Identity(), _Identity(), nn.Linear(dim, dim))
        self.feed_forward_macaron = nn.Sequential(nn.Linear(dim, dim), _Identity(), _Identity(), nn.Linear(dim, dim))
        self.conv_module = _ConvModule(dim)
        self.norm_ff_macaron = nn.LayerNorm(dim)
        self.norm_ff = nn.LayerNorm(dim)
        self.norm_mha = nn.LayerNorm(dim)
        self.norm_conv = nn.LayerNorm(dim)
        self.norm_final = nn.LayerNorm(dim)


class _ConformerDecoder(_Decoder):
    """Parameter layout of `ConformerDecoder` (src/models/transformer_decoder.py:125-155): `blocks` instead of `encoder_blocks`, the same
    `att_mask` buffer.  The reference hands `window_len` straight to `diagonal_mask`, which takes ONE width: a sequence is refused."""

    def __init__(self, dim, layers, heads, seq_len=1000, win_len=None):
        if win_len is not None and (isinstance(win_len, bool) or not isinstance(win_len, int)):
            raise TypeError("decoder_win_len of the conformer decoder must be one int or None (the reference passes it to diagonal_mask, "
                            f"which takes a single width; per-head windows exist for decoder='transformerXL' only), got {win_len!r}")
        super().__init__(dim, 0, heads, seq_len=seq_len, win_len=win_len)
        del self.encoder_blocks
        self.blocks = nn.ModuleList([_ConformerBlock(dim, heads) for _ in range(layers)])


class _AttnPool(_Holder):
    def __init__(self, dim, heads):
        super().__init__()
        self.f_att_token = nn.Parameter(torch.zeros(1, 1, dim))
        nn.init.normal_(self.f_att_token, std=0.02)
        self.frequency_att = nn.MultiheadAttention(embed_dim=dim, num_heads=heads, batch_first=True)


class _FreqTransformerPool(_Holder):
    """Parameter layout of `FrequencyWiseTranformerPooling` (src/models/pooling.py:18-25): the tag embedding `linear_emb`, two timm
    0.4.5 `Block`s of 4 heads (qkv without a bias, LayerNorm eps 1e-5) and the closing LayerNorm; torch's default initialisation."""

    def __init__(self, dim):
        super().__init__()
        self.linear_emb = nn.Linear(1, dim)
        self.frequency_transformer = nn.ModuleList([_Block(dim, 4, 1e-5) for _ in range(2)])
        for blk in self.frequency_transformer:
            blk.attn.qkv = nn.Linear(dim, 3 * dim, bias=False)
        self.frequency_transformer_norm = nn.LayerNorm(dim)


class _Hookable(nn.Module):
    def forward(self, x, *a):
        return x


class _SedFunction(torch.autograd.Function):
    """The whole MAT-SED network as ONE autograd node: forward = engine.forward, backward = engine.backward.

    The parameters are NOT inputs of the node (torch walks every argument of `Function.apply` several times per call: with the
    ~220 parameter tensors that was 20 ms of host time per step); a one-element `anchor` leaf keeps the node in the graph and the
    backward assigns / accumulates `p.grad` itself, as views of the flat gradient arena."""

    @staticmethod
    def forward(ctx, module, kw, mel, anchor, *extras):
        # (`extras`: differentiable inputs other than the parameters -- DASM's external query embeddings, dasm.py; the engine reads them from
        #  the module, they are arguments here so that autograd routes their gradients)
        save = kw.pop("save")
        ctx.set_materialize_grads(False)
        out, ectx = module.engine.forward(mel, save=save, **kw)
        keys = [k for k in ("strong", "weak", "at_out", "mlm_pred", "frame_before_mask") if k in out]
        ctx.module, ctx.ectx, ctx.keys, ctx.n_extras = module, ectx, keys, len(extras)
        module._last_mask_ids = out.get("mask_id_seq")
        module._out_keys = keys
        return tuple(out[k] for k in keys)

    @staticmethod
    def backward(ctx, *gouts):
        module = ctx.module
        if ctx.ectx is None:
            raise RuntimeError("backward through a forward that was run without saving activations")
        grads = {k: g for k, g in zip(ctx.keys, gouts)}
        names = module._param_names
        params = [module._param_by_name[n] for n in names]
        inert = getattr(module, "_inert_param_names", ())      # groups the optimiser will never move (lr 0): no gradient is computed for them
        live = [(n, p) for n, p in zip(names, params) if p.requires_grad and not n.startswith("backbone.head") and n not in inert]
        flat = getattr(module, "_flat_layout", None)
        views = {}
        if flat is not None:  # optimiser-owned layout: gradient arena offsets == parameter arena offsets
            arena = torch.zeros(flat.total, dtype=torch.float32, device=params[0].device)
            for n, p in live:
                o, k = flat.offset[n]
                views[n] = arena[o:o + k].view(p.shape)
        else:
            total = sum((p.numel() + 63) // 64 * 64 for _, p in live)
            arena = torch.zeros(total, dtype=torch.float32, device=params[0].device)
            off = 0
            for n, p in live:
                views[n] = arena[off:off + p.numel()].view(p.shape)
                off += (p.numel() + 63) // 64 * 64
        # a second backward before zero_grad() accumulates (autograd semantics): the arena the optimiser / all-reduce read is the sum
        prev = getattr(module, "_last_grad_arena", None)
        accumulate = prev is not None and prev.numel() == arena.numel() and any(p.grad is not None for _, p in live)
        module._last_grad_arena = arena
        hook = getattr(module, "_grad_ready_hook", None)
        module.engine.backward(ctx.ectx, grads, lambda n: views.get(n), hook=hook)
        ctx.ectx = None
        if accumulate:
            owner = getattr(hook, "__self__", None)
            if owner is not None and hasattr(owner, "wait_pending"):
                owner.wait_pending()      # the slices being averaged must be final before the earlier (already averaged) sum is added
            arena.add_(prev)
        touched = module._grad_names()
        for n, p in live:
            if n in touched or (accumulate and p.grad is not None):
                p.grad = views[n]
        eg = list(getattr(module, "_extra_input_grads", None) or [])
        module._extra_input_grads = None
        eg = (eg + [None] * ctx.n_extras)[:ctx.n_extras]
        return (None, None, None, None, *eg)


class PaSST_SED(SEDModel):
    def __init__(self, decode_ratio=10, interpolate_mode="linear", passt_feature_layer=10, embed_dim=768,
                 decoder_dim=768, f_pool="mean_pool", s_patchout_f=0, s_patchout_t=0, decoder="gru", decoder_layer_num=2,
                 decoder_pos_emd_len=1000, load_pretrained_model=True, class_num=10, at_adapter=False,
                 decoder_win_len=None, mlm=False, mlm_dict=dict(), lora_config=None, encoder_depth=12, _pmam=False):
        super().__init__()
        unsupported = []
        if _pmam:   # the PaSST_CNN subclass (passt_cnn.py): 384-wide context network, attention pooling, LoRA
            if embed_dim != D or decoder_dim % 128 or decoder_dim // H > 64: unsupported.append("embed_dim != 768 / decoder_dim")
            if f_pool not in ("mean_pool", "attention"): unsupported.append(f"f_pool={f_pool!r}")
        else:
            if embed_dim != D or decoder_dim != D: unsupported.append("embed_dim/decoder_dim != 768")
            if f_pool not in ("mean_pool", FPOOL_TRANSFORMER): unsupported.append(f"f_pool={f_pool!r}")
            if lora_config is not None: unsupported.append("LoRA")
        if decoder not in (("transformerXL",) if _pmam else ("transformerXL", "conformer")):
            unsupported.append(f"decoder={decoder!r}" + (" (the conformer decoder exists for PaSST_SED only)" if decoder == "conformer" else ""))
        if _pmam:
            if s_patchout_f or s_patchout_t: unsupported.append("patchout")
        else:
            patchout_f(s_patchout_f)
            if s_patchout_t: unsupported.append("s_patchout_t (the reference asserts it off: passt_sed.py:77)")
        if interpolate_mode != "linear": unsupported.append(f"interpolate_mode={interpolate_mode!r}")
        if unsupported:
            raise NotImplementedError("the HIP MAT-SED path covers the MAT-SED configs only; unsupported: "
                                      + ", ".join(unsupported))
        self.mel_trans = PasstFeatureExtractor(n_mels=128, sr=32000, win_length=800, hopsize=320, n_fft=1024, htk=False,
                                               fmin=0.0, fmax=None, wav_norm=True, fmin_aug_range=10,
                                               fmax_aug_range=2000)
        self.depth = encoder_depth
        lora = None
        self.lora_r, self.lora_scaling = 0, 0.0
        if lora_config:
            lora = dict(r=lora_config["r"], lora_alpha=lora_config.get("lora_alpha", 1),
                        requires_grad_pretrain=lora_config.get("requires_grad_pretrain", False))
            self.lora_r, self.lora_scaling = lora["r"], lora["lora_alpha"] / lora["r"]
        self.backbone = _Backbone(embed_dim, encoder_depth, lora, s_patchout_f)
        if load_pretrained_model:
            sd = torch.load("./pretrained_model/passt-s-f128-p16-s10-ap.476-swa.pt", map_location="cpu")
            self.backbone.load_state_dict(sd, strict=False)
        self.f_pool_name = f_pool
        self.passt_feature_layer = passt_feature_layer
        self.decoder_name = decoder
        self.decode_ratio = decode_ratio
        self.class_num = class_num
        self.embed_dim = embed_dim
        self.decoder_dim = decoder_dim
        self.out_norm = nn.LayerNorm(embed_dim)
        if f_pool == "attention":
            self.f_pool_module = _AttnPool(embed_dim, 6)
        elif f_pool == FPOOL_TRANSFORMER:
            self.f_pool_module = _FreqTransformerPool(embed_dim)
        self.interpolate_module = _Hookable()
        self.slide_window_layer = nn.Identity()
        self.mlm = mlm
        if mlm:
            self.mlm_cfg = dict(mask_rate=mlm_dict.get("mask_rate", 0.15), strategy=mlm_dict.get("strategy", "random"),
                                block_width=mlm_dict.get("block_width", 10),
                                mask_style=tuple(mlm_dict.get("mask_style", (0.8, 0.1, 0.1))))
            self.mask_token = nn.Parameter(torch.zeros(1, 1, decoder_dim))
            nn.init.normal_(self.mask_token, std=0.02)
            self.mlm_mlp = nn.Sequential(nn.Linear(decoder_dim, decoder_dim), nn.GELU(),
                                         nn.Linear(decoder_dim, mlm_dict["out_dim"]))
            self.mlm_out = mlm_dict["out_dim"]
            if mlm_dict["out_dim"] != D:
                raise NotImplementedError("mlm out_dim != 768")
        self.decoder_layer_num = decoder_layer_num
        self.decoder = (_ConformerDecoder if decoder == "conformer" else _Decoder)(decoder_dim, decoder_layer_num, H, seq_len=decoder_pos_emd_len,
                                                                                     win_len=decoder_win_len)
        self.classifier = nn.Linear(decoder_dim, class_num)
        self.has_at = bool(at_adapter)
        self.at_adpater = at_adapter  # (sic) spelling is part of the checkpoint contract
        if at_adapter:
            self.at_adpater = nn.Sequential(_AttnPool(embed_dim, 12), nn.Linear(embed_dim, class_num))
        self.engine = None
        self._mlm_draws = None       # tests may inject {"noise","probs","rand_idx"}
        self._win_toffsets = None    # tests may inject the train-mode window offsets
        self._patchout_rows = None   # ... and the train-mode kept frequency rows: the global pass's set, then one per window
        self._pmam = bool(_pmam)
        self._pending_draws = None   # (toffsets, rows) drawn ahead of the forward that uses them: `predraw`
        self.mask_effective_override = None
        self._index_params()

    # ------------------------------------------------------------------ bookkeeping
    def _index_params(self):
        self._param_names = [n for n, _ in self.named_parameters()]
        self._param_by_name = dict(self.named_parameters())
        self._buffer_by_name = dict(self.named_buffers())

    @property
    def lora_merged(self):
        return bool(self.lora_r) and self.backbone.blocks[0].attn.qkv.merged

    def _make_engine(self):
        return SedEngine(self)

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self._index_params()
        return r

    def _grad_names(self):
        """Parameters that receive a gradient in the reference for the current mode (others stay None)."""
        names = set()
        for n, p in self._param_by_name.items():
            if not p.requires_grad or n.startswith("backbone.head"):
                continue
            if self.mlm and (n.startswith("classifier.") or n.startswith("at_adpater")):
                continue  # unused by the MLM loss
            if self.mlm and n == "mask_token" and not self._last_mask_effective:
                continue
            if self.mlm and n in ("backbone.norm.weight", "backbone.norm.bias"):
                continue
            names.add(n)
        return names

    # ------------------------------------------------------------------ MLM plan (mask.py:49-107)
    def _mlm_plan(self, B, T, dev, encoder_win):
        cfg = self.mlm_cfg
        dr = self._mlm_draws
        if cfg["strategy"] == "block":
            nseg = T // cfg["block_width"]
            noise = dr["noise"].to(dev) if dr else torch.rand(B, nseg, device=dev)
            srt, _ = noise.sort()
            thr = srt[:, min(int(nseg * cfg["mask_rate"]), nseg - 1)]
            ids = torch.zeros(B, T, dtype=torch.bool, device=dev)
            ids[:, :nseg * cfg["block_width"]] = (noise <= thr.unsqueeze(-1)).repeat_interleave(cfg["block_width"], dim=1)
        else:
            noise = dr["noise"].to(dev) if dr else torch.rand(B, T, device=dev)
            ids = noise <= cfg["mask_rate"]
        probs = dr["probs"].to(dev) if dr else torch.rand(B * T, device=dev)
        flat = ids.view(-1)
        s0, s1 = cfg["mask_style"][0], cfg["mask_style"][1]
        mm = flat & (probs < s0)
        rm = flat & (probs >= s0) & (probs < s0 + s1)
        action = mm.to(torch.uint8) + 2 * rm.to(torch.uint8)
        if dr:   # injected draws (tests): one index per 'random' row, in row order like mask.py:79
            src = torch.zeros(B * T, dtype=torch.int32, device=dev)
            src[rm] = dr["rand_idx"].to(dev).to(torch.int32)
        else:    # one draw per row, used where the row is a 'random' one: no count has to travel to the host
            src = torch.where(rm, torch.randint(0, B * T, (B * T,), device=dev, dtype=torch.int32), 0)
        # Reference quirk: the in-place masking only takes effect when the sequence is contiguous
        # (sliding windows) or B == 1; otherwise the decoder sees the unmasked sequence.
        eff = bool(encoder_win) or B == 1 or getattr(self, "_mask_always_effective", False)
        if self.mask_effective_override is not None:
            eff = bool(self.mask_effective_override)
        self._last_mask_effective = eff
        return dict(mask_ids=ids, action=action, src_idx=src, effective=eff)

    # ------------------------------------------------------------------ train-mode draws of one forward (needs no GPU)
    def _train_draws(self, T, encoder_win=False, win_param=(512, 49)):
        """-> (toffsets, rows) of one forward over T mel frames, either None when the engine's default (offset 0 / all 12 rows) applies.
        Every backbone call of the reference in training mode draws, on the CPU default generator, a time-position offset
        `randint(1 + 99 - tp)` when its tp < 99 patches are fewer than the table (passt.py:504-509), then -- with s_patchout_f -- the
        kept rows `randperm(12)[:12 - s].sort()` (passt.py:537).  The global pass comes first (99 patches: no offset), then the windows
        in sweep order.  Eval mode draws nothing and drops nothing; injected values replace the draws they stand for."""
        s = patchout_f(self.backbone.s_patchout_f)
        if s and self._pmam:
            raise NotImplementedError("the HIP MAT-SED path covers the MAT-SED configs only; unsupported: patchout")
        starts = window_starts(T, win_param[0], win_param[1]) if encoder_win else []
        toffsets = list(self._win_toffsets) if (encoder_win and self._win_toffsets is not None) else None
        if not self.training:
            return toffsets, None
        rows = patchout_rows(self._patchout_rows, s, 1 + len(starts)) if (s and self._patchout_rows is not None) else None
        draw_off, draw_rows = encoder_win and toffsets is None, bool(s) and rows is None
        draw = lambda: torch.randperm(12)[:12 - s].sort().values.tolist()
        if draw_off: toffsets = []
        if draw_rows: rows = [draw()]
        for left in starts:
            tpw = (min(left + win_param[0], T) - left - 16) // 10 + 1
            if draw_off:
                toffsets.append(int(torch.randint(1 + 99 - tpw, (1,)).item()) if tpw < 99 else 0)
            if draw_rows:
                rows.append(draw())
        return toffsets, rows

    def predraw(self, T, encoder_win=False, win_param=(512, 49)):
        """Make the train-mode draws of the NEXT forward now.  For a caller that issues another model's forward first although the
        reference runs this one first (the trainer's teacher on its side stream): the draw order stays the reference's."""
        self._pending_draws = self._train_draws(T, bool(encoder_win), win_param)

    # ------------------------------------------------------------------ forward (passt_sed.py:242-296)
    def forward(self, input, encoder_win=False, mix_rate=0.5, win_param=[512, 49], temp_w=1, pad_mask=None):
        if not input.is_cuda:
            raise RuntimeError("PaSST_SED (transformer4sed_amd) runs on MI355X only: move the model and input to 'cuda'. "
                               "There is no CPU fallback on the product path.")
        if self.engine is None:
            self.engine = self._make_engine()
        B, _, T = input.shape
        kw = dict(encoder_win=bool(encoder_win), mix_rate=float(mix_rate), win_param=tuple(win_param),
                  temp_w=float(temp_w), pad_mask=pad_mask)
        pending, self._pending_draws = getattr(self, "_pending_draws", None), None
        toffsets, rows = pending if pending is not None else self._train_draws(T, bool(encoder_win), win_param)
        if toffsets is not None:
            kw["toffsets"] = toffsets
        if rows is not None:
            kw["rows"] = rows
        self._last_mask_effective = False
        if self.mlm:
            kw["mlm_plan"] = self._mlm_plan(B, (99 + 1) * self.decode_ratio, input.device, encoder_win)
        if getattr(self, "_drop_masks", None) is not None:
            kw["drop_masks"] = self._drop_masks
        inert = getattr(self, "_inert_param_names", ())
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for n, p in self._param_by_name.items() if n not in inert)
        kw["save"] = need_grad
        anchor = getattr(self, "_anchor", None)
        if anchor is None or anchor.device != input.device:
            anchor = self._anchor = torch.zeros(1, device=input.device, requires_grad=True)
        extras = [t for t in getattr(self, "_extra_inputs", ()) if need_grad]
        outs = _SedFunction.apply(self, kw, input, anchor if need_grad else anchor.detach(), *extras)
        o = dict(zip(self._out_keys, outs))
        other = {"frame_before_mask": o["frame_before_mask"]}
        if self.mlm:
            other["mask_id_seq"] = self._last_mask_ids
        if self.has_at or "at_out" in o:      # (DASM: the tagging stream of its head)
            other["at_out"] = o["at_out"]
        if self.mlm:
            return o["mlm_pred"], other
        return o["strong"], o["weak"], other

    @torch.no_grad()
    def extract_features(self, mel, feature_layer):
        """Frame features for the PMAM tokenizer (the forward hooks of recipes/desed/pmam/extractor_feature.py:81-104), from one
        evaluation-mode, no-grad pass through the engine: "after_interpolate" = the pooled encoder features at the decoder's frame rate
        [B, 1000, 768] (the reference's `interpolate_module` hook); "transformer_<k>" = the output of context block k
        [B, 1000, decoder_dim].  The training mode of the module is restored."""
        import re
        mt = re.fullmatch(r"transformer_(\d+)", feature_layer)
        if mt is not None and int(mt.group(1)) < self.decoder_layer_num:
            layer = int(mt.group(1))
        elif feature_layer == "after_interpolate":
            layer = feature_layer
        else:
            raise ValueError(f"feature_layer must be 'after_interpolate' or 'transformer_<k>' with k < {self.decoder_layer_num}, got {feature_layer!r}")
        was_training = self.training
        self.eval()
        if self.engine is None:
            self.engine = self._make_engine()
        tap = self.engine.feature_tap = dict(layer=layer, out=None)
        try:
            self.forward(mel)
        finally:
            self.engine.feature_tap = None
            self.train(was_training)
        return tap["out"]

    def get_feature_extractor(self):
        return self.mel_trans

    def get_model_name(self):
        return "PaSST_SED"

    def get_backbone_upsample_ratio(self):
        return self.decode_ratio

    def get_backbone(self):
        return self.backbone
