"""Padded operand images: the padding plans, the image table of the whole model (`_image_specs`) and the per-step `_weights`."""
import math

import torch

from ..engine import ImageSpec, image_table, H, version_key
from ..ops import F32, call, h2d
from . import HD_PAD
from .geometry import cnn_geometry, cnn_layer_plans


class PmamImages:
    def _plan(self, tag, src_shape, dev, fn):
        """(plan int32, scale fp32, image shape) of a padded image: `fn(w, k)` is the padding expression on a tensor of the master's
        shape (k: the scale of the sqrt(2) rows); it is run ONCE on an enumeration of the master's elements and on ones, after which the
        image -- and the way its gradient returns to the master -- is a gather / scatter with a per-element scale (0 on the padding)."""
        plans = self.__dict__.setdefault("_pad_plans", {})
        key = (tag, tuple(src_shape), str(dev))
        if key not in plans:
            if fn is None:
                raise RuntimeError(f"padding plan {tag} requested before the forward built it")
            n = 1
            for v in src_shape:
                n *= v
            ids = torch.arange(1, n + 1, dtype=torch.float32, device=dev).view(src_shape)
            mapped = fn(ids, 1.0)
            # K / P rows: the attention kernels divide the scores by sqrt(64); a model head of width hd needs 1 / sqrt(hd) -- sqrt(64 / hd)
            # on one operand (sqrt 2 for the 384-wide PMAM context net, 1 for DASM's 768-wide one)
            scale = fn(torch.ones(src_shape, dtype=torch.float32, device=dev), math.sqrt(HD_PAD / (self.m.decoder_dim // H)))
            plans[key] = ((mapped.reshape(-1).long() - 1).clamp_(min=0).to(torch.int32), scale.reshape(-1).contiguous(), tuple(mapped.shape))
        return plans[key]

    def _image_specs(self, dev):
        """Every 16-bit operand image of the model as an `ImageSpec`, every padded fp32 vector as (slot, master name, plan) and the
        geometry of the CNN branch (`cnn_geometry`).  Shapes only: built once per device."""
        key = ("specs", str(dev))
        if getattr(self, "_specs_key", None) == key:
            return self._specs
        m = self.m
        Dd, hd = m.decoder_dim, m.decoder_dim // H
        P = lambda n: self.P(n)

        def rows(w, scale=1.0):      # [H*hd, K] -> [H*64, K]
            o = w.new_zeros(H, HD_PAD, w.shape[1])
            o[:, :hd] = w.view(H, hd, -1) * scale
            return o.view(H * HD_PAD, -1)

        def vec(b, scale=1.0):
            o = b.new_zeros(H, HD_PAD)
            o[:, :hd] = b.view(H, hd) * scale
            return o.view(-1)

        def pad2(w, R, C):
            o = w.new_zeros(R, C)
            o[:w.shape[0], :w.shape[1]] = w
            return o

        win = lambda w, k: torch.cat([rows(w[:Dd]), rows(w[Dd:2 * Dd], k), rows(w[2 * Dd:])], 0)
        binf = lambda b, k: torch.cat([vec(b[:Dd]), vec(b[Dd:2 * Dd], k), vec(b[2 * Dd:])], 0)
        wout = lambda w, k: pad2(w.view(Dd * H, hd), Dd * H, HD_PAD).view(Dd, H * HD_PAD)
        wpos = lambda w, k: rows(w, k)
        uv = lambda b, k: vec(b).view(H, HD_PAD)
        mats, vecs = [], []

        def mat(name, master, plan=None, lora=None, split=False, kind="act", shape=None):
            if plan is not None:
                R, C = plan[2]
            else:
                R = shape[0] if shape else P(master).shape[0]
                C = P(master).numel() // R
            mats.append(ImageSpec(name, master, R, C, plan, lora, split, kind))

        mat("backbone.patch_embed.proj.weight", "backbone.patch_embed.proj.weight")
        for i in range(m.depth):
            for sub in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2"):
                n = f"backbone.blocks.{i}.{sub}"
                mat(n + ".weight", n + ".weight", lora=n if m.lora_r else None)
        for n in ("at_adpater.0.frequency_att.in_proj_weight", "f_pool_module.frequency_att.in_proj_weight",
                  "f_pool_module.frequency_att.out_proj.weight"):
            if n.startswith("at_adpater") and not m.has_at:      # (DASM: its tagging stream is the query decoder, dasm.py)
                continue
            mat(n, n)
        for n in ("transformer_projector.weight", "cnn_projector.weight", "mlm_mlp.0.weight", "mlm_mlp.2.weight"):
            if n.startswith("mlm_mlp") and not m.mlm:
                continue
            mat(n, n, split=True)
        # context network: heads zero-padded from hd to 64 in the images; CNN branch: conv weight [co, ci, 3, 3] -> [pad128(co), Kp]
        # with column = tap * ci + c, gate weight [co, co] -> [pad128(co), Cp]
        for i in range(m.decoder_layer_num):
            p = f"decoder.encoder_blocks.{i}."
            for sub, tag, fn in (("attn.in_proj.weight", "win", win), ("attn.out_proj.weight", "wout", wout), ("attn.linear_pos.weight", "wpos", wpos)):
                mat(p + sub, p + sub, plan=self._plan(tag, P(p + sub).shape, dev, fn), split=True)
            mat(p + "mlp.fc1.weight", p + "mlp.fc1.weight", split=True)
            mat(p + "mlp.fc2.weight", p + "mlp.fc2.weight", split=True)
            vecs.append((("dec", i, "bin"), p + "attn.in_proj.bias", self._plan("bin", P(p + "attn.in_proj.bias").shape, dev, binf)))
            vecs.append((("dec", i, "u"), p + "attn.pos_bias_u", self._plan("uv", P(p + "attn.pos_bias_u").shape, dev, uv)))
            vecs.append((("dec", i, "v"), p + "attn.pos_bias_v", self._plan("uv", P(p + "attn.pos_bias_v").shape, dev, uv)))
        geo = cnn_geometry(m.cnn_filters, m.cnn_pooling, getattr(m, "cnn_dynamic", None))
        for i, g in enumerate(geo):
            Np, Kp, Cp, ldg = g["Np"], g["Kp"], g["Cp"], g["ldg"]
            cw, gw = f"cnn.cnn.conv{i}.weight", f"cnn.cnn.cg{i}.linear.weight"
            # a dynamic layer's four basis kernels [4, co, ci, 3, 3] are one [4 co, 9 ci] operand: rows k co + o (FDY_cnn.py:44)
            Nc = g["Nc"] if g["dyn"] else Np
            mat(cw, cw, plan=self._plan(("conv", Nc, Kp), P(cw).shape, dev,
                                        lambda w, k, Nc=Nc, Kp=Kp: pad2(w.reshape(-1, *w.shape[-3:]).permute(0, 2, 3, 1).reshape(w.numel() // (9 * w.shape[-3]), -1), Nc, Kp)))
            mat(gw, gw, plan=self._plan(("gate", Np, Cp), P(gw).shape, dev, lambda w, k, Np=Np, Cp=Cp: pad2(w, Np, Cp)))
            # backward operand of the gate GEMM: [Np (N), ldg (K)] = W_gate^T, zero padded, bf16 (ldg: row width of the gradient images)
            mat(gw + "#T", gw, plan=self._plan(("gateT", Np, ldg), P(gw).shape, dev, lambda w, k, Np=Np, ldg=ldg: pad2(w.t(), Np, ldg)), kind="bf16")
            bplan = lambda n, Np=Np: self._plan(("b", Np), P(n).shape, dev, lambda b, k: pad2(b.view(1, -1), 1, Np).view(-1))
            if not g["dyn"]:      # (Dynamic_conv2d has no bias, FDY_cnn.py:145-147)
                vecs.append((("cnn", i, "bias"), f"cnn.cnn.conv{i}.bias", bplan(f"cnn.cnn.conv{i}.bias")))
            vecs.append((("cnn", i, "gbias"), f"cnn.cnn.cg{i}.linear.bias", bplan(f"cnn.cnn.cg{i}.linear.bias")))
        self._specs, self._specs_key = (mats, vecs, geo), key
        return self._specs

    def _weights(self, need_t):
        """Operand images of every GEMM weight and the padded fp32 vectors, from the fp32 masters: one `sed_weight_images` launch for
        what can change between steps, one for whichever frozen images went stale (normally none), one `sed_gather_f32`.  The LoRA
        linears' train-mode weight W + s B A (lora/layers.py:148-151) is formed inside the image kernel."""
        m = self.m
        dev = self.P("out_norm.weight").device
        mats, vecs, geo = self._image_specs(dev)
        merged = m.lora_merged or not m.lora_r
        lora = None if merged else (m.lora_r, int(torch.tensor(float(m.lora_scaling), dtype=torch.float32).view(torch.int32)))
        statics = self.__dict__.setdefault("_static_keys", {})
        # Frozen operands (the blocks below `freeze_layer`, cnn_trans/setting.py:66-82) keep their images across steps.  A tensor without
        # requires_grad is not necessarily constant (the EMA teacher's masters, load_state_dict, p.copy_): like every cached weight image,
        # a block's statics are rebuilt iff the storage or the version of one of its masters moved (engine.version_key).
        live, stale = [], []
        for sp in mats:
            if not (sp.name.startswith("backbone.blocks.") and sp.lora is not None):
                live.append(sp)
                continue
            parts = [self.P(sp.master), self.P(sp.lora + ".lora_A"), self.P(sp.lora + ".lora_B")]
            if any(p.requires_grad for p in parts):
                live.append(sp)
                continue
            key = version_key(parts, (merged, bool(need_t)))
            if statics.get(sp.name) != key or sp.name not in self.cache:
                stale.append(sp)
                statics[sp.name] = key
        for specs, cached in ((stale, False), (live, True)):
            if not specs:
                continue
            ptrs = tuple(self.P(sp.master).data_ptr() for sp in specs) + tuple(self.P(sp.lora + ".lora_A").data_ptr() for sp in specs if sp.lora) + \
                (bool(need_t), merged, len(specs))
            if cached and getattr(self, "_wimg_key", None) == ptrs:
                desc, n, tiles = self._wimg_desc
            else:
                rows_, tiles = image_table(specs, self.P, self.cache, need_t, lora)
                desc, n = h2d(rows_, torch.int64, dev), len(rows_)
                if cached:
                    self._wimg_desc, self._wimg_key = (desc, n, tiles), ptrs
            call("sed_weight_images", desc, n, tiles)
        # padded fp32 vectors
        vkey = tuple(self.P(mn).data_ptr() for _, mn, _ in vecs)
        if getattr(self, "_vimg_key", None) != vkey:
            total = sum(pl[0].numel() for _, _, pl in vecs)
            buf = torch.empty(total, dtype=F32, device=dev)
            rows_, off, blocks, views = [], 0, 0, {}
            for slot, mn, pl in vecs:
                nel = pl[0].numel()
                dst = buf[off:off + nel]
                rows_.append([self.P(mn).data_ptr(), pl[0].data_ptr(), pl[1].data_ptr(), dst.data_ptr(), nel, blocks, 0, 0])
                views[slot] = dst.view(pl[2])
                off += nel
                blocks += (nel + 255) // 256
            self._vimg = (h2d(rows_, torch.int64, dev), len(rows_), blocks, buf, views)
            self._vimg_key = vkey
        vdesc, vn, vblocks, _, views = self._vimg
        call("sed_gather_f32", vdesc, vn, vblocks)
        self.dec_aux = [dict(bin=views[("dec", i, "bin")], u=views[("dec", i, "u")], v=views[("dec", i, "v")]) for i in range(m.decoder_layer_num)]
        self.cnn_aux = [dict(g, bias=views.get(("cnn", i, "bias")), gbias=views[("cnn", i, "gbias")],
                             wtg=self.cache[f"cnn.cnn.cg{i}.linear.weight#T"].w if need_t else None) for i, g in enumerate(geo)]
        return self.cache

    def _cnn_plan(self, B, T, dev):
        """The layer plans of the CNN branch (`geometry.cnn_layer_plans`) for a [B, 128, T] spectrogram, built once per shape and `dw_tn`."""
        key = (B, T, bool(self.dw_tn))
        plans = self._cnn_plans.get(key)
        if plans is None:
            plans = self._cnn_plans[key] = cnn_layer_plans(self._image_specs(dev)[2], self.m.cnn_pooling, B, T, key[2])
        return plans
