"""Weight images of the engine: the 16-bit operand images every forward rewrites (`sed_weight_images` and its descriptor table), the
images cached across forwards on the masters' versions, the relative-position tables and the pooled zero-padded buffers."""
import math
from typing import NamedTuple, Optional

import torch
from torch.optim.optimizer import register_optimizer_step_post_hook

from ..ops import BF16, F16, F32, call, h2d, gemm_nt, pad64, transpose_bf16, is_f16, split3, two_term_weight, two_term_weight_f8, EPI_F32
from . import ACT, D, FPOOL_TRANSFORMER, WCORR_STEP


def version_key(sources, form=None):
    """Cache key of an image derived from the tensors `sources`: (device, data_ptr, _version) of each, plus a form tag.  The one rule of
    every cached weight image: it is rebuilt iff the storage or the version of one of its sources moved.  torch moves `_version` on every
    in-place write (optimisers, `copy_`, load_state_dict); the project's raw-pointer writers (FusedAdamWEMA, update_ema) move it
    themselves with torch.autograd.graph.increment_version."""
    return tuple((t.device, t.data_ptr(), t._version) for t in sources) + (form,)


def cached_image(holder, slot, sources, build, form=None):
    """`holder.<slot>`, rebuilt with `build()` when the `version_key` of `sources` / `form` differs from `holder.<slot>_key`."""
    key = version_key(sources, form)
    if getattr(holder, slot + "_key") != key:
        setattr(holder, slot, build())
        setattr(holder, slot + "_key", key)
    return getattr(holder, slot)


def _fused_step_moves_versions(optimizer, args, kwargs):
    """torch.optim's fused implementations (`fused=True`: torch._fused_adamw_ and its kin) rewrite the parameters without moving their
    version counters, unlike the foreach and for-loop forms.  The weight-image caches key on `_version` (`version_key`): move it for
    every parameter such a step updated (the ones with a gradient)."""
    for g in optimizer.param_groups:
        if g.get("fused"):
            ps = [p for p in g["params"] if p.grad is not None]
            if ps:
                torch.autograd.graph.increment_version(ps)


register_optimizer_step_post_hook(_fused_step_moves_versions)


def rel_pos_table(T, Dm=D):
    """Sin/cos relative-position table [2T-1, D]; row k encodes relative position T-1-k
    (src/models/transformer/transformerXL.py:84-127).  Host-built once per T (fp32, like the reference)."""
    pos = torch.arange(0, T, dtype=torch.float32).unsqueeze(1)
    div = torch.exp(torch.arange(0, Dm, 2, dtype=torch.float32) * -(math.log(10000.0) / Dm))
    pp = torch.zeros(T, Dm)
    pn = torch.zeros(T, Dm)
    pp[:, 0::2] = torch.sin(pos * div)
    pp[:, 1::2] = torch.cos(pos * div)
    pn[:, 0::2] = torch.sin(-1 * pos * div)
    pn[:, 1::2] = torch.cos(-1 * pos * div)
    return torch.cat([torch.flip(pp, [0]), pn[1:]], dim=0)


class _W:
    """bf16 operand images of one fp32 weight matrix [n_out, k_in] (rewritten by every forward), and the images cached across forwards
    (`cached_image`): LayerNorm-folded `lnf`, two-term `w2` (f16 or fp8 form), residual `wlo`, each beside its key."""
    __slots__ = ("w", "wt", "ws", "wlo", "wlo_key", "w2", "w2_key", "lnf", "lnf_key")

    def __init__(self, w, wt):
        self.w, self.wt, self.ws = w, wt, None
        self.wlo = self.wlo_key = self.w2 = self.w2_key = self.lnf = self.lnf_key = None


class ImageSpec(NamedTuple):
    """One operand image of `sed_weight_images`: the [R, C] image `name` (key of the engine's cache) of the fp32 master `master`.
    plan: (gather index int32, scale fp32, image shape) of a padded image or None; lora: prefix of the lora_A / lora_B factors whose
    product the image adds in while they are unmerged, or None; split: also the split-precision image [R, 3 C] = [hi | hi | lo];
    kind 'act': straight image in the activation type + transposed bf16 image; 'bf16': straight bf16 image only."""
    name: str
    master: str
    R: int
    C: int
    plan: Optional[tuple] = None
    lora: Optional[str] = None
    split: bool = False
    kind: str = "act"


def image_table(specs, P, cache, need_t, lora=None):
    """-> (rows, tiles): the int64 descriptor rows of `sed_weight_images` for `specs`, in their order, and its tile count.  Per row:
    master, transposed image (0 unless `need_t`, and for kind 'bf16'), straight image, split image (0 unless asked for), R, C, kind, tile
    offset, gather plan and its scale, lora_A, lora_B, r, the bits of the fp32 LoRA scale, 0, 0.  `P`: name -> master tensor; `cache`: name
    -> `_W`, whose images are allocated here and reused while device and shape stand; `lora`: (r, scale bits) while the factors are
    unmerged, else None.  Launches nothing and reads only pointers, shapes and devices."""
    rows, tiles = [], 0
    for sp in specs:
        w32, R, C = P(sp.master), sp.R, sp.C
        if R % 16 or C % 64 or not w32.is_contiguous():
            raise RuntimeError(f"weight {sp.name}: unsupported shape / layout for the operand images")
        dev, act = w32.device, sp.kind == "act"
        ent = cache.get(sp.name)
        if ent is None or ent.w.device != dev or ent.w.shape != (R, C):
            ent = cache[sp.name] = _W(torch.empty(R, C, dtype=ACT if act else BF16, device=dev), torch.empty(C, R, dtype=BF16, device=dev) if act else None)
        if sp.split and (ent.ws is None or ent.ws.device != dev):
            ent.ws = torch.empty(R, 3 * C, dtype=F16, device=dev)
        plan = sp.plan or (None, None)
        fac = (P(sp.lora + ".lora_A").data_ptr(), P(sp.lora + ".lora_B").data_ptr(), *lora) if (sp.lora and lora) else (0, 0, 0, 0)
        rows.append([w32.data_ptr(), ent.wt.data_ptr() if (act and need_t) else 0, ent.w.data_ptr(), ent.ws.data_ptr() if sp.split else 0,
                     R, C, 2 if act else 0, tiles, *(0 if t is None else t.data_ptr() for t in plan[:2]), *fac, 0, 0])
        tiles += ((R + 63) // 64) * (C // 64)
    return rows, tiles


class _PoolLease:
    """Held by the saved-activation context of one forward: while it lives, the engine's pooled zero-padded buffers belong to that
    context (a second forward before the backward gets fresh allocations instead)."""

    def __init__(self, eng):
        self.eng = eng

    def __del__(self):
        self.eng._pool_busy = False


class Images:
    def _wcorr_on(self, save):
        """Does this pass run the evaluation-mode encoder weights?"""
        if save:
            return False
        if getattr(self.m, "lora_r", 0) and not getattr(self.m, "lora_merged", False):
            return False        # PaSST_CNN in train mode: the GEMM operand is W + s B A, not the master the residual image is taken from
        return not self.m.training

    def _fpool_split_on(self, save):
        """Does this pass run the transformer pooling's GEMMs in split precision?  Scored passes do (module in eval mode, nothing saved);
        training-mode passes run them on plain f16 operands like the encoder blocks."""
        return self._wcorr_on(save)

    def _lnf_image(self, W, wname, bname, gname, btname):
        """(f16(gamma (.) W), colS, colC) of a Linear that follows a LayerNorm (sed_ln_fold_weight), cached per weight on all four
        masters."""
        w, b, g, bt = ps = [self.P(n) for n in (wname, bname, gname, btname)]

        def build():
            n_out, k_in = W[wname].w.shape
            w16 = torch.empty(n_out, k_in, dtype=F16, device=w.device)
            cs, cc = torch.empty(n_out, device=w.device), torch.empty(n_out, device=w.device)
            call("sed_ln_fold_weight", w.detach().reshape(n_out, k_in).contiguous(), g.detach(), bt.detach(), b.detach(), w16, cs, cc, n_out, k_in)
            return w16, cs, cc
        return cached_image(W[wname], "lnf", ps, build)

    def _w2_image(self, W, name):
        """Two-term f16 image [n_out, 2 k_in] of an fp32 weight, cached per weight."""
        p = self.P(name)
        return cached_image(W[name], "w2", [p], lambda: two_term_weight(p.detach().reshape(W[name].w.shape)), "f16")

    def _w2f8_image(self, W, name):
        """(uint8 image [n_out, 3 k_in] = rows [f16(W) | e4m3(2^s (W - f16(W)))], s) of an fp32 weight, cached like `_w2_image` (same slot:
        a module runs one of the two forms)."""
        p = self.P(name)
        return cached_image(W[name], "w2", [p], lambda: two_term_weight_f8(p.detach().reshape(W[name].w.shape)), "f8")

    def _wlo_image(self, W, name):
        """f16 image of 2^11 (W - f16(W)), cached per weight."""
        p = self.P(name)

        def build():
            src = p.detach().reshape(W[name].w.shape).contiguous()
            wlo = torch.empty(src.shape, dtype=F16, device=src.device)
            call("sed_weight_residual_f16", src, wlo, src.numel(), 2048.0)
            return wlo
        return cached_image(W[name], "wlo", [p], build)

    def _wcorr_bias(self, W, name, x16, groups, rows, ld=None):
        """Row-group bias [groups, n_out] = mean over the `rows` tokens of each clip of x16 . (W - f16(W))^T (fp32).  `ld`: row pitch of
        x16 when its rows carry more than the K operand columns (the [f16 | e4m3] rows of the fp8 form)."""
        wlo = self._wlo_image(W, name)
        K = wlo.shape[1]
        mean = torch.empty(groups, K, dtype=x16.dtype, device=x16.device)
        call("sed_group_colmean_ld", x16, mean, groups, rows, K, ld or x16.shape[-1], WCORR_STEP, is_f16(x16))
        out = torch.empty(groups, wlo.shape[0], dtype=F32, device=x16.device)
        gemm_nt(mean, wlo, EPI_F32, outF=out, alpha=1.0 / 2048.0)
        return out

    def _lease(self, save):
        """Start of a forward: claim the pooled saved-tensor buffers for this pass when it saves activations and nobody holds them."""
        self._lease_ok = False
        if save and not self._pool_busy:
            self._pool_busy = self._lease_ok = True
            return _PoolLease(self)
        return None

    def _zeros(self, key, shape, dtype, dev, pooled=True):
        if not pooled:
            return torch.zeros(*shape, dtype=dtype, device=dev)
        t = self._zpool.get(key)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != dev:
            t = self._zpool[key] = torch.zeros(*shape, dtype=dtype, device=dev)
        return t

    def _weight_names(self):
        """Master (= cache) name of every GEMM weight of the model, in the order of the descriptor table."""
        m = self.m
        blk = ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight")
        names = ["backbone.patch_embed.proj.weight"] + [f"backbone.blocks.{i}.{s}" for i in range(m.depth) for s in blk]
        if m.decoder_name == "conformer":       # (the 1-tap Conv1d weights [out, in, 1] are [out, in] matrices to the image kernel)
            dec, sub = "decoder.blocks", ("self_attn.in_proj", "self_attn.out_proj", "self_attn.linear_pos", "feed_forward_macaron.0", "feed_forward_macaron.3",
                                          "conv_module.pointwise_conv1", "conv_module.pointwise_conv2", "feed_forward.0", "feed_forward.3")
        else:
            dec, sub = "decoder.encoder_blocks", ("attn.in_proj", "attn.out_proj", "attn.linear_pos", "mlp.fc1", "mlp.fc2")
        names += [f"{dec}.{i}.{s}.weight" for i in range(m.decoder_layer_num) for s in sub]
        if m.mlm:
            names += ["mlm_mlp.0.weight", "mlm_mlp.2.weight"]
        if m.has_at:
            names += ["at_adpater.0.frequency_att.in_proj_weight"]
        if m.f_pool_name == FPOOL_TRANSFORMER:
            names += [f"f_pool_module.frequency_transformer.{i}.{s}" for i in range(2) for s in blk]
        return names

    def _weight_specs(self, need_t):
        """`_weight_names` as image specs; the context network and the MLM head get a split image, the transformer pooling in the passes
        that run it in split precision (`need_t` is the forward's `save`)."""
        P, fp_split = self.P, self._fpool_split_on(need_t)
        return [ImageSpec(n, n, P(n).shape[0], P(n).numel() // P(n).shape[0],
                          split=n.startswith(("decoder.", "mlm_mlp")) or (fp_split and n.startswith("f_pool_module."))) for n in self._weight_names()]

    def _weights(self, need_t):
        """(Re)build the 16-bit operand images of every GEMM weight from the fp32 masters: one `sed_weight_images` launch."""
        names = self._weight_names()
        key = tuple(self.P(n).data_ptr() for n in names) + (bool(need_t), self._fpool_split_on(need_t))
        if getattr(self, "_wimg_key", None) != key:
            # descriptor table of sed_weight_images: rebuilt only when a master moved (optimizer arenas, .to(device))
            rows, tiles = image_table(self._weight_specs(need_t), self.P, self.cache, need_t)
            self._wimg_desc = h2d(rows, torch.int64, self.P(names[0]).device)
            self._wimg_n, self._wimg_tiles, self._wimg_key = len(rows), tiles, key
        call("sed_weight_images", self._wimg_desc, self._wimg_n, self._wimg_tiles)
        return self.cache

    def _pos(self, T, dev, Dm=D, want_plain=True):
        key = (T, str(dev), Dm)
        if key not in self.pos_cache:
            R = 2 * T - 1
            Rpad = pad64(R)
            tab = torch.zeros(Rpad, Dm)
            tab[:R] = rel_pos_table(T, Dm)
            tab = tab.to(dev)
            pos16 = tab.to(ACT).contiguous()
            posT16 = torch.empty(Dm, Rpad, dtype=BF16, device=dev)
            transpose_bf16(tab, Rpad, Dm, posT16)
            pos16s = split3(tab, Rpad, Dm)
            self.pos_cache[key] = (pos16, posT16, Rpad, pos16s)
        ent = self.pos_cache[key]
        # (pos16: split image [hi | lo | hi] when the split-precision linear_pos GEMM reads it, the plain f16 table for `dec_terms2`)
        return (ent[0] if (self.dec_terms2 and want_plain) else ent[3]), ent[1], ent[2]
