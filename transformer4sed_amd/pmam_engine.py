"""Forward engine of the PMAM variant (`PaSST_CNN`, src/models/cnn_transformer/passt_cnn.py:9-91).

Reuses every encoder / context-network kernel of the MAT-SED engine and adds, in HIP (csrc/lora.hip, cnn_branch.hip, dw_narrow.hip for
the first two items and the narrow layers' weight gradients, csrc/pmam.hip for the rest):
  * LoRA linears (src/models/lora/layers.py:88-153): the operand image of each encoder weight is W + s B A (one merge kernel per
    weight), so the forward GEMMs are the MAT-SED ones;
  * the CNN branch (src/models/cnn/base.py:62-113): NHWC 16-bit activations, every 3x3 convolution = patch gather + one NT GEMM
    (K = 9 C padded to 64, N = filters padded to 128), BatchNorm folded to a per-channel affine, ContextGating as a second
    GEMM over the channels, gate * dropout * average pooling fused;
  * `attention` frequency pooling (src/models/pooling.py:37-51, 6 heads): k | v projection GEMM + one wave per (frame, head);
  * the 384-wide / 12 x 32-head context network on the 64-wide attention kernels: every head is zero-padded to 64 dims in the
    WEIGHT IMAGES (in_proj / linear_pos rows, out_proj columns, pos_bias_u / v), K and P rows scaled by sqrt(2) so that the
    kernels' 1/8 score scale becomes 1/sqrt(32); the padded dims are exact zeros end to end;
  * the projector merge (passt_cnn.py:57-62) with both projections applied before the interpolations (exact: the interpolation
    weights sum to one), which shrinks the two GEMMs from 1000 to 99 / 250 rows per clip.
"""
import math
import os

import torch

from . import ops

from .engine import SedEngine, ImageSpec, image_table, ACT, D, H, version_key, empty, stats
from .ops import BF16, F16, F32, call, h2d, gemm_nt, gemm_nt_cols, gemm_dw, gemm_dw_tn, dw_tn_ok, pad64, transpose_bf16, split3, is_f16
from .ops import EPI_F32, EPI_F32_RESID, EPI_BF16

HD_PAD = 64          # head width the attention kernels are built for
SQRT2 = math.sqrt(2.0)


def pad128(n):
    return (n + 127) // 128 * 128


class _LoraSlot:
    """What the encoder backward receives in place of a LoRA linear's weight-gradient view: the factors and their gradient views."""
    __slots__ = ("A", "B", "gA", "gB", "r", "s", "shape")

    def __init__(self, A, B, gA, gB, r, s):
        self.A, self.B, self.gA, self.gB, self.r, self.s = A, B, gA, gB, r, s
        self.shape = (B.shape[0], A.shape[1])


class PmamEngine(SedEngine):
    def __init__(self, module):
        super().__init__(module)
        # (round 6: the three PMAM A/B switches SED_LORA_SKINNY / SED_SMALL_DW / SED_CG_FUSED16 are gone -- results in DESIGN section 8; the
        #  attributes remain for the kernel tests that exercise the general paths)
        self.lora_skinny = True
        self.small_dw = True
        self.cg_fused16 = True
        self.dec_terms2 = False      # (this context network keeps three split-precision terms in every GEMM)
        self._drop_gen = None

    def _dropout_generator(self):
        """Seed source of the CNN dropout masks: a generator private to this engine (seeded from torch.initial_seed() on first use), so
        that the process-global CPU generator is advanced only by the draws the reference also makes on it (the augmentation)."""
        if self._drop_gen is None:
            self._drop_gen = torch.Generator()
            self._drop_gen.manual_seed((torch.initial_seed() * 0x9E3779B1 + 0x5ED) % (1 << 63))
        return self._drop_gen

    # ------------------------------------------------------------------ operand images
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
        """Every 16-bit operand image of the model as an `ImageSpec` and every padded fp32 vector as (slot, master name, plan).  Shapes
        only: built once per device."""
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
        geo = []
        cin = 1
        dynamic = getattr(m, "cnn_dynamic", None) or (False,) * len(m.cnn_filters)
        for i, co in enumerate(m.cnn_filters):
            Np = pad128(co)
            Kp = 64 if i == 0 else pad128(9 * cin)
            Cp = max(64, co)
            cw, gw = f"cnn.cnn.conv{i}.weight", f"cnn.cnn.cg{i}.linear.weight"
            # a dynamic layer's four basis kernels [4, co, ci, 3, 3] are one [4 co, 9 ci] operand: rows k co + o (FDY_cnn.py:44)
            dyn = bool(dynamic[i])
            Nc = pad128(4 * co) if dyn else Np
            mat(cw, cw, plan=self._plan(("conv", Nc, Kp), P(cw).shape, dev,
                                        lambda w, k, Nc=Nc, Kp=Kp: pad2(w.reshape(-1, *w.shape[-3:]).permute(0, 2, 3, 1).reshape(w.numel() // (9 * w.shape[-3]), -1), Nc, Kp)))
            mat(gw, gw, plan=self._plan(("gate", Np, Cp), P(gw).shape, dev, lambda w, k, Np=Np, Cp=Cp: pad2(w, Np, Cp)))
            # backward operand of the gate GEMM: [Np (N), ldg (K)] = W_gate^T, zero padded, bf16 (ldg: row width of the gradient images)
            ldg = 64 if co <= 64 else Np
            mat(gw + "#T", gw, plan=self._plan(("gateT", Np, ldg), P(gw).shape, dev, lambda w, k, Np=Np, ldg=ldg: pad2(w.t(), Np, ldg)), kind="bf16")
            bplan = lambda n, Np=Np: self._plan(("b", Np), P(n).shape, dev, lambda b, k: pad2(b.view(1, -1), 1, Np).view(-1))
            if not dyn:      # (Dynamic_conv2d has no bias, FDY_cnn.py:145-147)
                vecs.append((("cnn", i, "bias"), f"cnn.cnn.conv{i}.bias", bplan(f"cnn.cnn.conv{i}.bias")))
            vecs.append((("cnn", i, "gbias"), f"cnn.cnn.cg{i}.linear.bias", bplan(f"cnn.cnn.cg{i}.linear.bias")))
            geo.append(dict(Np=Np, Kp=Kp, Cp=Cp, cin=cin, co=co, ldg=ldg, dyn=dyn))
            if dyn:
                # Y4 [pixels, ld4] fp32: 64 columns for 16 filters (the GEMM writes only the valid columns), the padded width otherwise;
                # ldg4: row width of the bf16 gradient operand a (x) dY, as ldg for the static layers
                geo[-1].update(Nc=Nc, ld4=64 if 4 * co == 64 else Nc, ldg4=64 if 4 * co <= 64 else Nc, hid=max(cin // 4, 4))
            cin = co
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

    # ------------------------------------------------------------------ attention frequency pooling
    def _fpool_fwd(self, W, x, Bx, tp, save, ctx):
        m = self.m
        if m.f_pool_name != "attention":
            return super()._fpool_fwd(W, x, Bx, tp, save, ctx)
        dev = x.device
        N = 2 + 12 * tp
        M = Bx * N
        E = empty(dev)
        pre = "f_pool_module."
        h16 = E(M, D, dt=ACT)
        pm, pr = stats(E, M, save)
        call("sed_layernorm_fwd", x, self.P("out_norm.weight"), self.P("out_norm.bias"), 1e-5, 1.0, h16, None, pm, pr, M, D, 1)
        q, kv16 = self._token_query_fwd(W, pre, h16)
        att16 = E(Bx * tp, D, dt=ACT)
        probs = E(Bx * tp, 6, 12) if save else None
        call("sed_fpool_attn_fwd", kv16, q, att16, None, probs, Bx, N, tp, 1)
        pooled = E(Bx, tp, D)
        gemm_nt(att16, W[pre + "frequency_att.out_proj.weight"].w, EPI_F32, bias=self.P(pre + "frequency_att.out_proj.bias"),
                outF=pooled.view(Bx * tp, D))
        if save:
            ctx.update(pool_x=x, pool_mean=pm, pool_rstd=pr, pool_h16=h16, pool_q=q, pool_kv16=kv16, pool_att16=att16, pool_probs=probs)
        return pooled

    # ------------------------------------------------------------------ CNN branch
    def _cnn_fwd(self, W, mel, train, save, drop_masks=None):
        """-> (feat fp32 [B * T/4, C_last], ctx).  train: batch statistics (and running-statistics update, torch BatchNorm semantics:
        momentum 0.99, unbiased variance); eval: running statistics."""
        m = self.m
        dev = mel.device
        B, _, T = mel.shape
        E = empty(dev)
        Hc, Wc = T, 128
        X = None
        layers = []
        feat = None
        nl = len(self.cnn_aux)
        cmax = max(a_["co"] for a_ in self.cnn_aux)
        sums = torch.zeros(nl, 2, cmax, device=dev) if train else None      # batch-statistics sums of every layer: one fill
        aff = E(nl, 4, cmax)                                                # a | b | ah | bh of every layer (saved for the backward)
        if train:
            torch._foreach_add_([m._buffer_by_name[f"cnn.cnn.batchnorm{i}.num_batches_tracked"] for i in range(nl)] +
                                [m._buffer_by_name[f"cnn.cnn.conv{i}.attention.bn.num_batches_tracked"] for i in range(nl) if self.cnn_aux[i]["dyn"]], 1)
        gen_masks = None
        if train and m.conv_dropout > 0 and drop_masks is None:
            # keep-masks of every layer from one launch.  The seed comes from a generator of this engine's own (seeded once from
            # torch.initial_seed(), so runs stay reproducible under torch.manual_seed): the process-global CPU stream is consumed only
            # where the reference consumes it (the augmentation draws, data_aug.py) -- nn.Dropout draws from the device generator there
            sizes, Hm, Wm = [], T, 128
            for i, a_ in enumerate(self.cnn_aux):
                sizes.append(B * Hm * Wm * a_["co"])
                Hm, Wm = Hm // m.cnn_pooling[i][0], Wm // m.cnn_pooling[i][1]
            flat = torch.empty(sum(sizes), dtype=torch.uint8, device=dev)
            call("sed_dropout_mask", flat, flat.numel(), float(m.conv_dropout), int(torch.randint(0, 2 ** 62, (1,), generator=self._dropout_generator()).item()))
            gen_masks, off = [], 0
            for n_ in sizes:
                gen_masks.append(flat[off:off + n_])
                off += n_
        for i, aux in enumerate(self.cnn_aux):
            co, Np, Kp, Cp, cin = aux["co"], aux["Np"], aux["Kp"], aux["Cp"], aux["cin"]
            Mi = B * Hc * Wc
            ldy = co if co < Np else Np     # 16 / 32 / 64 filters: the GEMM writes only the valid columns of its 128-wide tile
            Y = E(Mi, ldy)
            # first convolution with 16 filters: direct on the fp32 spectrogram (`sed_conv0_fwd16`: no patch matrix, no GEMM); its weight
            # gradient gathers the patches again (`sed_conv0_dw16`)
            direct0 = i == 0 and co == 16 and self.cg_fused16 and self.small_dw and self.dw_tn and Mi >= 1024
            col = None
            if direct0:      # (train: the batch-statistics sums come out of the same pass)
                call("sed_conv0_fwd16", mel, self.P("cnn.cnn.conv0.weight").detach(), self.P("cnn.cnn.conv0.bias").detach(), Y, B, T,
                     sums[i, 0] if train else None, sums[i, 1] if train else None)
            else:
                col = E(Mi, Kp, dt=ACT)
                if i == 0:
                    call("sed_conv0_im2col", mel, col, B, T, 1)
                else:
                    call("sed_conv3x3_im2col", X, col, B, Hc, Wc, cin, max(64, cin), Kp)
                if aux["dyn"]:
                    dynctx = self._fdy_mix_fwd(W, i, aux, X, col, Y, ldy, B, Hc, Wc, train)
                elif ldy < Np:
                    gemm_nt_cols(col, W[f"cnn.cnn.conv{i}.weight"].w, EPI_F32, co, bias=aux["bias"], outF=Y)
                else:
                    gemm_nt(col, W[f"cnn.cnn.conv{i}.weight"].w, EPI_F32, bias=aux["bias"], outF=Y)
            bn = f"cnn.cnn.batchnorm{i}."
            g, bt = self.P(bn + "weight").detach(), self.P(bn + "bias").detach()
            s1 = s2 = None
            if train:   # batch statistics; running statistics updated with torch's BatchNorm rule (momentum 0.99, unbiased variance)
                s1, s2 = sums[i, 0], sums[i, 1]
                if not direct0:
                    call("sed_colstats", Y, ldy, None, 0, None, None, s1, s2, Mi, co, 0)
            a, b, ah, bh = aff[i, 0], aff[i, 1], aff[i, 2], aff[i, 3]
            call("sed_bn_finalize", s1, s2, g, bt, m._buffer_by_name[bn + "running_mean"], m._buffer_by_name[bn + "running_var"], Mi, co,
                 0.99, 1e-3, a, b, ah, bh)
            # the gate Linear inside the pooling kernel (`sed_cg_gate16_pool`); its narrow z image is an operand `sed_small_dw` alone takes
            fused16 = self.cg_fused16 and self.small_dw and self.dw_tn and co == 16 and ldy == 16 and Mi >= 1024
            Z = L = None
            if not fused16:
                Z = E(Mi, Cp, dt=ACT)
                call("sed_bn_act", Y, ldy, a, b, Z, Mi, co, Cp, 1)
                L = E(Mi, ldy)
                if ldy < Np:
                    gemm_nt_cols(Z, W[f"cnn.cnn.cg{i}.linear.weight"].w, EPI_F32, co, bias=aux["gbias"], outF=L)
                else:
                    gemm_nt(Z, W[f"cnn.cnn.cg{i}.linear.weight"].w, EPI_F32, bias=aux["gbias"], outF=L)
            ph, pw = m.cnn_pooling[i]
            last = i + 1 == len(self.cnn_aux)
            Cpo = max(64, co)
            Xn = None if last else E(B, Hc // ph, Wc // pw, Cpo, dt=ACT)
            if last:
                feat = E(B * (Hc // ph) * (Wc // pw), co)
            mask = None
            scale = 1.0
            if train and m.conv_dropout > 0:
                mask = drop_masks[i] if drop_masks is not None else gen_masks[i].view(Mi, co)
                scale = 1.0 / (1.0 - m.conv_dropout)
            if fused16:
                # 16 filters: z = Y a + b, l = W_g z + b_g (fp32, 256 FMAs per pixel), gate, dropout and pooling in one pass over Y; the
                # backward's operands -- the logits and the 16-column 16-bit image of z -- are side outputs of a saving pass
                if save:
                    L, Z = E(Mi, 16), E(Mi, 16, dt=ACT)
                call("sed_cg_gate16_pool", Y, ldy, a, b, self.P(f"cnn.cnn.cg{i}.linear.weight").detach(), self.P(f"cnn.cnn.cg{i}.linear.bias").detach(),
                     mask, float(scale), L, Z, Xn, feat, B, Hc, Wc, Cpo, ph, pw, 1)
            else:
                call("sed_cg_pool", Y, ldy, a, b, L, ldy, mask, float(scale), Xn, feat, B, Hc, Wc, co, Cpo, ph, pw, 1)
            if save:
                layers.append(dict(col=col, mel=mel if direct0 else None, Y=Y, a=a, b=b, ah=ah, bh=bh, Z=Z, L=L, mask=mask, scale=scale, H=Hc,
                                   W=Wc, ldy=ldy, dyn=dynctx if aux["dyn"] else None))
            X = Xn
            Hc, Wc = Hc // ph, Wc // pw
        assert Wc == 1
        return feat, dict(layers=layers, Tc=Hc)

    def _fdy_mix_fwd(self, W, i, aux, X, col, Y, ldy, B, Hc, Wc, train):
        """The convolution of a dynamic layer (FDY_cnn.py:34-63) into Y: the attention head on the frequency mean of the layer's input X
        (train: BatchNorm1d batch statistics, running statistics updated by torch's rule with momentum 0.1), the four basis convolutions
        as one GEMM of the patch matrix, and the per-frame mixing.  -> what the backward needs (Y4 is kept in fp32)."""
        m = self.m
        dev = col.device
        co, cin, hid, ld4 = aux["co"], aux["cin"], aux["hid"], aux["ld4"]
        R, Mi = B * Hc, B * Hc * Wc
        E = empty(dev)
        pre = f"cnn.cnn.conv{i}.attention."
        pm, u, aff1, att = E(R, cin), E(R, hid), E(3, hid), E(R, 4)
        call("sed_fdy_freq_mean", X, is_f16(X), pm, R, Wc, cin, X.shape[-1])
        part = E((R + 15) // 16 * 2 * hid, dt=torch.float64) if train else None
        call("sed_fdy_attn_taps", pm, self.P(pre + "conv1d1.weight").detach(), u, part, B, Hc, cin, hid)
        call("sed_fdy_attn_softmax", u, part, self.P(pre + "bn.weight").detach(), self.P(pre + "bn.bias").detach(),
             m._buffer_by_name[pre + "bn.running_mean"], m._buffer_by_name[pre + "bn.running_var"], self.P(pre + "conv1d2.weight").detach(),
             self.P(pre + "conv1d2.bias").detach(), float(m.cnn_temperature), 0.1, 1e-5, aff1, att, R, hid)
        Y4 = E(Mi, ld4)
        if ld4 < aux["Nc"]:
            gemm_nt_cols(col, W[f"cnn.cnn.conv{i}.weight"].w, EPI_F32, ld4, outF=Y4)
        else:
            gemm_nt(col, W[f"cnn.cnn.conv{i}.weight"].w, EPI_F32, outF=Y4)
        call("sed_fdy_mix_fwd", Y4, ld4, att, Y, ldy, Mi, Wc, co)
        return dict(pm=pm, u=u, aff=aff1, att=att, Y4=Y4, train=bool(train))

    def _fdy_mix_bwd(self, W, i, aux, L, dY16, B, G, slots):
        """Backward of `_fdy_mix_fwd` from dY (bf16 [pixels, ldo]): the weight gradient of the four basis kernels into its slot, the input
        gradient through the patch matrix, the attention head's parameter gradients, and the head's path into the input gradient."""
        dev = dY16.device
        co, cin, hid, ld4, ldg4, Kp = aux["co"], aux["cin"], aux["hid"], aux["ld4"], aux["ldg4"], aux["Kp"]
        Hc, Wc, D = L["H"], L["W"], L["dyn"]
        R, Mi = B * Hc, B * Hc * Wc
        E = empty(dev)
        pre = f"cnn.cnn.conv{i}.attention."
        dY4, da = E(Mi, ldg4, dt=BF16), E(R, 4)
        call("sed_fdy_mix_bwd", dY16, dY16.shape[1], D["Y4"], ld4, D["att"], dY4, ldg4, da, R, Wc, co)
        self._dw_swapped(dY4, L["col"], Mi, 4 * co, 9 * cin, out=(slots[("conv", i)], slots[("conv_b", i)]), n_img=ldg4)
        dcol = E(Mi, Kp, dt=BF16)
        gemm_nt(dY4, W[f"cnn.cnn.conv{i}.weight"].wt, EPI_BF16, outH=dcol, K=ldg4)
        dout = E(B, Hc, Wc, cin)
        call("sed_col2im3x3", dcol, Kp, dout, B, Hc, Wc, cin)
        del dcol, dY4
        P6 = 6 * hid + 4
        ws = E((P6 + 3) // 4 * 4 + max(1, min(32, R // 128)) * 3 * hid * cin)
        part = E((R + 15) // 16 * P6, dt=torch.float64)
        dz, dpm = E(R, hid), E(R, cin)
        call("sed_fdy_attn_bwd", da, D["att"], D["u"], D["aff"], D["pm"], self.P(pre + "conv1d1.weight").detach(), self.P(pre + "bn.bias").detach(),
             self.P(pre + "conv1d2.weight").detach(), float(self.m.cnn_temperature), 1 if D["train"] else 0, dz, part, ws, ws.numel(), dpm,
             G(pre + "conv1d1.weight"), G(pre + "bn.weight"), G(pre + "bn.bias"), G(pre + "conv1d2.weight"), G(pre + "conv1d2.bias"),
             B, Hc, cin, hid)
        call("sed_fdy_mean_bwd_add", dout, dpm, R, Wc, cin)
        return dout

    # ------------------------------------------------------------------ 384-wide context network on the 64-wide attention kernels
    # SedEngine's Transformer-XL schedule at decoder_dim; what differs here are these pieces.  (The weights at the attention's prefix are
    # the padded-head images: the shared attention path runs H * HD_PAD wide.)
    def _ctx_ln_fwd(self, x, norm, scale, mean, rstd, plain=False, want32=False):
        """Any width: `sed_ln_fwd_any` to fp32, then the [hi | lo | hi] image of that (`dec_terms2` is off here: never `plain`)."""
        Dm = x.shape[-1]
        M = x.numel() // Dm
        y32 = torch.empty(x.shape if want32 else (M, Dm), dtype=F32, device=x.device)
        call("sed_ln_fwd_any", x, self.P(norm + ".weight"), self.P(norm + ".bias"), 1e-5, scale, None, y32, mean, rstd, M, Dm, 1)
        return split3(y32, M, Dm), (y32 if want32 else None)

    _ctx_ln_bwd = "sed_ln_bwd_any"

    def _relattn_bias(self, pa, li):
        aux = self.dec_aux[li]      # (the padded vectors `_weights` gathered)
        return aux["bin"], aux["u"], aux["v"]

    def _relattn_sink(self, Gl, pa, li, dctx, dev):
        """The gradient images (padded heads) in the zeroed slots of `_grad_slots` that `_context_bwd` left in `dctx`; one scatter
        launch after the walk un-pads them."""
        Dd, Dp = self.m.decoder_dim, H * HD_PAD
        slots = dctx["slots"]
        if ("gwo", li) not in slots:       # frozen: `_grad_slots` made no images for the context network
            Z = lambda *s: torch.zeros(*s, dtype=F32, device=dev)
            return dict(out_proj=(None, None), linear_pos=None, in_proj=(None, None), pos_bias_u=Z(Dp), pos_bias_v=Z(Dp))
        return dict(out_proj=(slots[("gwo", li)].view(Dd, Dp), Gl(pa + "out_proj.bias")), linear_pos=slots[("gwp", li)].view(Dp, Dd),
                    in_proj=(slots[("gwi", li)].view(3 * Dp, Dd), slots[("gbi", li)]),
                    pos_bias_u=slots[("du", li)], pos_bias_v=slots[("dv", li)])

    # ------------------------------------------------------------------ stages of SedEngine.forward (passt_cnn.py:31-88)
    _mlm_c = True               # the merged sequence is decoder_dim wide
    _embed_stage_always = True  # (ddp.GradReducer's stage order of these models ends with "embed" whenever the stack is walked)

    def _walks_decoder_fwd(self):
        return True     # no heads-only shortcut here: the context network is always walked, forward and backward

    def _walks_decoder(self, G, depth):
        return True

    def _check_forward(self, T, opt, save):
        assert T == 1000
        if opt["rows"] is not None:
            raise NotImplementedError("frequency patchout is not part of the PMAM path")
        if opt["win"] is not None and save:
            raise NotImplementedError("gradient through the sliding-window path is not needed by any PMAM config")

    def _project(self, W, name, x, rows):
        """Linear `name` on fp32 rows in split precision -> fp32 [rows, decoder_dim]."""
        out = torch.empty(rows, self.m.decoder_dim, dtype=F32, device=x.device)
        with ops.split_precision():
            gemm_nt(split3(x, rows, x.shape[1]), W[name + ".weight"].ws, EPI_F32, bias=self.P(name + ".bias"), outF=out)
        return out

    def _trunk_fwd(self, W, mel, pooled, tp, Tdec, opt, save):
        """CNN branch, the two projectors, the merge (passt_cnn.py:57-62); DASM: LayerNorm after the merge (detect_any_sound.py:346)."""
        m = self.m
        dev = mel.device
        B, Dd = mel.shape[0], m.decoder_dim
        E = empty(dev)
        feat, cctx = self._cnn_fwd(W, mel, train=m.training, save=save, drop_masks=opt["drop_masks"])
        Tc = cctx["Tc"]
        P2 = self._project(W, "cnn_projector", feat, B * Tc)
        assert Tdec % Tc == 0
        xg = E(B, Tdec, Dd)
        if opt["win"] is not None:
            # sliding windows (teacher / validation of the PMAM finetune stage): local and global features are mixed at encoder
            # width (passt_cnn.py:41-46), so the projector runs on all Tdec frames
            x768 = E(B, Tdec, D)
            call("sed_interp_fwd", pooled, x768, B, tp, 1, m.decode_ratio)
            self._window_features(W, mel, x768, Tdec, opt, False)
            src, rows, pad, up = x768, Tdec, 0, 1
        else:       # transformer_projector / cnn_projector before the interpolations
            src, rows, pad, up = pooled, tp, 1, m.decode_ratio
        P1 = self._project(W, "transformer_projector", src.view(B * rows, D), B * rows)
        call("sed_pmam_merge", P1, P2, self.P("merge_weight"), xg, B, rows, pad, up, Tc, Tdec // Tc, Dd)
        nam = None
        if getattr(m, "dasm_head", None) is not None:
            xn = E(B, Tdec, Dd)
            nm_, nr_ = stats(E, B * Tdec, save)
            call("sed_layernorm_fwd", xg.view(B * Tdec, Dd), self.P("norm_after_merge.weight"), self.P("norm_after_merge.bias"), 1e-5, 1.0,
                 None, xn.view(B * Tdec, Dd), nm_, nr_, B * Tdec, Dd, 0)
            if save:
                nam = dict(x=xg, mean=nm_, rstd=nr_)
            xg = xn
        return xg, dict(cctx=cctx, feat=feat, P1=P1, P2=P2, nam=nam)

    def _heads_fwd(self, W, xd, ectx, opt, save, out):
        m = self.m
        dasm = getattr(m, "dasm_head", None)       # DASM (dasm.py): same trunk, query decoder + dual-stream head
        if dasm is not None:
            # frame tokens of the final norm without the cls / dist tokens (detect_any_sound.py:364), fp32 (engine._encoder_fwd wrote them
            # beside the 16-bit image); the SED decoder's output goes to sed_head inside the head
            ft = self._frame32.view(xd.shape[0], ectx["N"], D)[:, 2:, :].contiguous()
            m._last_x_dec = xd            # (kept for tests / inspection: the SED decoder's output that sed_head reads)
            dc = m.__dict__["_dasm_call"]
            hd = dasm.forward(ft, xd, query=dc["query"], tgt_mask=dc["tgt_mask"], temp_w=float(opt["temp_w"]), pad_mask=opt["pad_mask"],
                              query_type=dc["query_type"], save=save, train=bool(m.training), drop_seed=m._next_drop_seed() if m.training else 0)
            out["strong"], out["weak"], out["at_out"] = hd[0], hd[1], hd[2]
            hctx = hd[4] if save else None
            if save:
                hctx["query_grads"] = list(getattr(m, "_dasm_query_grads", ()) or ()) or None
            return hctx
        if m.mlm:
            out["mlm_pred"], hctx = self._mlm_head_fwd(W, xd, BF16 if save else ACT)
            return hctx
        return super()._heads_fwd(W, xd, ectx, opt, save, out)      # classifier + sigmoid + linear-softmax pooling (passt_cnn.py:74-86)

    def _wide_head(self, save):
        return self.m.class_num != 10      # any class count (the 407 AudioSet-Strong classes): GEMM head, dasm.wide_head_fwd

    def _head10_fwd(self, xd, temp, pm):
        """The 768-wide head kernel on the decoder output and the classifier weight zero-padded from decoder_dim to 768 columns (the dot
        products are unchanged)."""
        B, Tdec, Dd = xd.shape
        C, dev = self.m.class_num, xd.device
        E = empty(dev)
        xd_pad = torch.zeros(B, Tdec, D, dtype=F32, device=dev)
        xd_pad[:, :, :Dd] = xd
        w_pad = torch.zeros(C, D, dtype=F32, device=dev)
        w_pad[:, :Dd] = self.P("classifier.weight").detach()
        strong, weak, sums = E(B, C, Tdec), E(B, C), E(B, C, 2)
        call("sed_head_fwd", xd_pad, w_pad, self.P("classifier.bias"), temp, pm, strong, weak, sums, B, Tdec, C)
        return strong, weak, dict(strong=strong, sums=sums, temp=temp, xd_pad=xd_pad, w_pad=w_pad)

    # ==================================================================== backward
    def _dw_accum(self, dy, x, M, gW, bias=None, dy16=None, k_in=None):
        """As SedEngine._dw_accum; a `_LoraSlot` in place of the weight-gradient view selects the LoRA form: dB += s dy^T (x A^T),
        dA += (s dy B)^T x (lora/layers.py:148-151 under autograd) as two projections onto the r factors and two reductions over the
        tokens -- each one pass over x or dy, on the weight-gradient side stream like the TN GEMM they replace."""
        if not isinstance(gW, _LoraSlot):
            return super()._dw_accum(dy, x, M, gW, bias, dy16=dy16, k_in=k_in)
        sl = gW
        n_out, kin = sl.shape
        g16 = super()._dw_accum(dy, x, M, None, bias, dy16=dy16, k_in=kin)     # bf16 image of dy (cast pass only if there is none yet)
        if x.dtype not in (F16, BF16) or g16.dtype != BF16:
            raise RuntimeError("LoRA gradient products expect 16-bit saved operands")
        dev = g16.device
        ldx = x.shape[1]

        def run():
            u, du = torch.empty(M, sl.r, device=dev), torch.empty(M, sl.r, device=dev)
            call("sed_lora_rowproj", x, is_f16(x), M, kin, ldx, sl.A, 0, sl.r, 1.0, u)
            call("sed_lora_rowproj", g16, 0, M, n_out, g16.shape[1], sl.B, 1, sl.r, sl.s, du)
            call("sed_lora_colreduce", g16, 0, M, n_out, g16.shape[1], u, sl.r, sl.s, sl.gB, 1)
            call("sed_lora_colreduce", x, is_f16(x), M, kin, ldx, du, sl.r, 1.0, sl.gA, 0)

        self._on_dw_stream(run, g16, x)
        return g16

    def _dw_swapped_tn(self, M, n, k):
        """Does `_dw_swapped` run the TN kernel for these shapes (gradient image laid out [n, k]) or the transposed-copy path ([k, n])?"""
        # (below 1024 rows the transposed-copy path is the cheaper one -- but its split-K GEMM needs both widths to fill a 128-wide tile:
        #  the 64-wide images of the narrow layers stay on the TN kernel at any row count)
        return bool(self.dw_tn and (M >= 1024 or n < 128 or k < 128) and dw_tn_ok(M, n, k))

    def _dw_swapped(self, dy16, x, M, n_valid, k_valid, out=None, k_img=None, n_img=None):
        """(dy^T x)^T = x^T dy for operand widths that are not multiples of 128 on the x side: returns fp32 [k, n] and the fp32 column
        sums of dy; only [:k_valid, :n_valid] / [:n_valid] are meaningful.  The operands are zero padded to GEMM-friendly widths
        (16 filters sit in 128 columns): only the 64-column groups that hold valid data are transposed, the other rows of the
        transposed images stay uninitialised and only feed output elements nobody reads.  `out` = (zeroed flat fp32 [n k], zeroed
        fp32 [n]): the gradient-image slots of `_grad_slots` (accumulated into; nothing is allocated or filled here)."""
        dev = dy16.device
        # (n_img / k_img: rows / row width of the gradient image when the operand itself is narrower -- the 16-column images of the 16-filter layers)
        n, k = (dy16.shape[1] if n_img is None else n_img), (x.shape[1] if k_img is None else k_img)
        tn = self._dw_swapped_tn(M, n, k) and dy16.dtype == BF16 and x.dtype in (F16, BF16)
        if out is not None and tn != self._dw_swapped_tn(M, n, k):
            raise RuntimeError("gradient-image slot laid out for the TN kernel, operands are not 16-bit")
        if tn and out is not None and self.small_dw and n_valid in (16, 32) and k_valid <= 32 and x.shape[1] >= (k_valid + 3) // 4 * 4:
            # 16 / 32 filters against <= 32 columns (the gate Linear, the first convolution's 9 taps): a streaming reduction instead of a
            # 256 x 256 tile's K loop (`sed_small_dw`; measured: 429 -> 165 us on layer 0, 207 -> 45 us on layer 1; the 144 / 288-column
            # convolution gradients stay on the TN kernel -- 169 / 457 us here against 164 / 201 there); same [n, k] image layout
            call("sed_small_dw", dy16, dy16.shape[1], n_valid, x, is_f16(x), x.shape[1], (k_valid + 3) // 4 * 4, out[0], k, out[1], M)
            return out[0].view(n, k).t(), out[1]
        if x.shape[1] != k or dy16.shape[1] != n:
            raise RuntimeError("weight-gradient operand narrower than its gradient image: only the streaming-reduction path takes it")
        if tn:
            # TN kernel on the operands as they lie: dW [n, k] = dy^T x and the column sums of dy from the same launch.  Padding columns
            # of either operand only reach output elements outside [:n_valid, :k_valid], which nobody reads.
            gW, csum = (torch.zeros(n, k, device=dev), torch.zeros(n, device=dev)) if out is None else (out[0].view(n, k), out[1])
            # this launch runs on the CURRENT stream and uses the per-device split-K workspace that weight-gradient GEMMs still pending on
            # the side stream (`_dw_accum`: the cnn_projector's dW was issued just before the CNN backward) are writing / reducing: order them
            self._join_dw()
            gemm_dw_tn(dy16, x, gW, dbias=csum)
            return gW.t(), csum
        n_eff, k_eff = min(n, pad64(n_valid)), min(k, pad64(k_valid))
        Mpad = pad64(M)
        gT = torch.empty(n, Mpad, dtype=BF16, device=dev)
        csum = torch.zeros(n, device=dev) if out is None else out[1]
        pad8 = lambda v: (v + 7) // 8 * 8

        def tr(src, valid, eff, dst, colsum):
            if pad8(valid) <= 32 and src.dtype in (BF16, F16):     # 16 / 32 data columns in a 64+ wide row: row-per-thread kernel
                call("sed_transpose_narrow", src, is_f16(src), M, pad8(valid), src.shape[1], dst, Mpad, colsum)
            else:
                transpose_bf16(src, M, eff, dst, colsum=colsum, ld=src.shape[1])

        tr(dy16, n_valid, n_eff, gT, csum)
        xT = torch.empty(k, Mpad, dtype=BF16, device=dev)
        tr(x, k_valid, k_eff, xT, None)
        gWT = torch.zeros(k, n, device=dev) if out is None else out[0].view(k, n)
        gemm_dw(xT, gT, gWT)
        return gWT, csum

    def _grad_slots(self, B, dev, G, dec_train, cnn_train, T=1000):
        """Gradient images of every padded weight / vector of one backward, as views of ONE zeroed fp32 arena, and the two
        `sed_scatter_add_f32` tables (context network, CNN branch) that return them to the masters' gradients through the forward
        plans -- scale sqrt(2) on the K / P rows, nothing from the padding.  Replaces a `zeros` per image and an `add_` of a sliced /
        permuted view per master (~190 launches per step) by one fill and two launches."""
        m = self.m
        mats, vecs, geo = self._image_specs(dev)
        Dd = m.decoder_dim
        Dp = H * HD_PAD
        items = []       # (group, slot, numel, master grad name, plan or None, n, C, ld_i, ld_j)
        if dec_train:
            for li in range(m.decoder_layer_num):
                p = f"decoder.encoder_blocks.{li}."
                pl = lambda tag, n: self._plan(tag, self.P(n).shape, dev, None)
                items += [("dec", ("gwo", li), Dd * Dp, p + "attn.out_proj.weight", pl("wout", p + "attn.out_proj.weight"), Dd * Dp, Dp, Dp, 1),
                          ("dec", ("gwp", li), Dp * Dd, p + "attn.linear_pos.weight", pl("wpos", p + "attn.linear_pos.weight"), Dp * Dd, Dd, Dd, 1),
                          ("dec", ("gwi", li), 3 * Dp * Dd, p + "attn.in_proj.weight", pl("win", p + "attn.in_proj.weight"), 3 * Dp * Dd, Dd, Dd, 1),
                          ("dec", ("gbi", li), 3 * Dp, p + "attn.in_proj.bias", pl("bin", p + "attn.in_proj.bias"), 3 * Dp, 3 * Dp, 0, 1),
                          ("dec", ("du", li), Dp, p + "attn.pos_bias_u", pl("uv", p + "attn.pos_bias_u"), Dp, Dp, 0, 1),
                          ("dec", ("dv", li), Dp, p + "attn.pos_bias_v", pl("uv", p + "attn.pos_bias_v"), Dp, Dp, 0, 1)]
        if cnn_train:
            Hc, Wc = T, 128
            for i, g in enumerate(geo):
                co, Np, Kp, Cp, cin, ldg = g["co"], g["Np"], g["Kp"], g["Cp"], g["cin"], g["ldg"]
                Mi = B * Hc * Wc
                cw, gw = f"cnn.cnn.conv{i}.weight", f"cnn.cnn.cg{i}.linear.weight"
                bplan = self._plan(("b", Np), self.P(f"cnn.cnn.cg{i}.linear.bias").shape, dev, None)
                # the gradient images hold the first ldg of the weight images' Np rows (64 for the 16 / 32 / 64-filter layers: the bf16
                # gradient operands are 64 columns wide there, round 4); the plans are read up to row ldg
                # (dynamic layer: the convolution's image has the 4 co rows of the basis kernels, ldg4 of them in the gradient image)
                Nc, ldc = (g["Nc"], g["ldg4"]) if g["dyn"] else (Np, ldg)
                for slot, master, plan, k, rows_ in ((("gate", i), gw, self._plan(("gate", Np, Cp), self.P(gw).shape, dev, None), Cp, ldg),
                                                     (("conv", i), cw, self._plan(("conv", Nc, Kp), self.P(cw).shape, dev, None), Kp, ldc)):
                    tn = self._dw_swapped_tn(Mi, rows_, k)      # image element (i, j) of [rows, k] sits at i k + j (TN) or j rows + i
                    items.append(("cnn", slot, rows_ * k, master, plan, rows_ * k, k, k if tn else 1, 1 if tn else rows_))
                items += [("cnn", ("gate_b", i), ldg, f"cnn.cnn.cg{i}.linear.bias", bplan, ldg, ldg, 0, 1),
                          # (the column sums of a (x) dY that the weight-gradient GEMM also writes have no master in a dynamic layer)
                          ("cnn", ("conv_b", i), ldc, None if g["dyn"] else f"cnn.cnn.conv{i}.bias", None if g["dyn"] else bplan, ldc, ldc, 0, 1),
                          ("cnn", ("bn_s1", i), co, f"cnn.cnn.batchnorm{i}.bias", None, co, co, 0, 1),
                          ("cnn", ("bn_s2", i), co, f"cnn.cnn.batchnorm{i}.weight", None, co, co, 0, 1)]
                ph, pw = m.cnn_pooling[i]
                Hc, Wc = Hc // ph, Wc // pw
        if not items:
            return {}, {}
        gp = lambda n: G(n).data_ptr() if (n is not None and G(n) is not None) else 0      # (a master without a gradient slot: its image is formed and dropped)
        key = (B, T, str(dev), dec_train, cnn_train, tuple(gp(it[3]) for it in items))
        if getattr(self, "_gslot_key", None) != key:
            total = sum((it[2] + 63) // 64 * 64 for it in items)
            arena = torch.empty(total, dtype=F32, device=dev)
            views, tables, off = {}, {}, 0
            rows_ = {"dec": [], "cnn": []}
            blocks = {"dec": 0, "cnn": 0}
            for grp, slot, numel, master, plan, n, C, ld_i, ld_j in items:
                v = arena[off:off + numel]
                views[slot] = v
                off += (numel + 63) // 64 * 64
                if not gp(master):
                    continue
                rows_[grp].append([v.data_ptr(), plan[0].data_ptr() if plan is not None else 0, plan[1].data_ptr() if plan is not None else 0,
                                   gp(master), n, blocks[grp], C | (ld_i << 32), ld_j])
                blocks[grp] += (n + 255) // 256
            for grp in ("dec", "cnn"):
                if rows_[grp]:
                    tables[grp] = (h2d(rows_[grp], torch.int64, dev), len(rows_[grp]), blocks[grp])
            self._gslot_key, self._gslot = key, (arena, views, tables)
        arena, views, tables = self._gslot
        arena.zero_()
        return views, tables

    def _cnn_bwd(self, W, cctx, dfeat, B, G, slots):
        m = self.m
        dev = dfeat.device
        E = empty(dev)
        dout = dfeat
        for i in range(len(self.cnn_aux) - 1, -1, -1):
            aux, L = self.cnn_aux[i], cctx["layers"][i]
            co, Np, Kp, Cp, cin = aux["co"], aux["Np"], aux["Kp"], aux["Cp"], aux["cin"]
            Hc, Wc = L["H"], L["W"]
            Mi = B * Hc * Wc
            ph, pw = m.cnn_pooling[i]
            ldy = L["ldy"]
            ldg = aux["ldg"]       # row width of the bf16 gradient operands: 64 columns hold the 16 / 32 / 64 filters (128 until round 4)
            dz = E(Mi, ldy)
            fused16 = L["Z"].shape[1] == 16 and co == 16      # the forward ran `sed_cg_gate16_pool`: its backward carries the gate Linear too
            if fused16:
                dL16 = E(Mi, 16, dt=BF16)
                call("sed_cg_gate16_pool_bwd", dout, L["Y"], ldy, L["a"], L["b"], L["L"], self.P(f"cnn.cnn.cg{i}.linear.weight").detach(), L["mask"],
                     float(L["scale"]), dz, dL16, B, Hc, Wc, ph, pw, L["ah"], L["bh"], slots[("bn_s1", i)], slots[("bn_s2", i)])
            else:
                dL16 = E(Mi, ldg, dt=BF16)
                call("sed_cg_pool_bwd", dout, L["Y"], ldy, L["a"], L["b"], L["L"], ldy, L["mask"], float(L["scale"]), dz, ldy, dL16, ldg, B, Hc,
                     Wc, co, ph, pw)
            # weight / bias gradient images land in the zeroed slots; `sed_scatter_add_f32` returns them to the masters after the loop
            self._dw_swapped(dL16, L["Z"], Mi, co, co, out=(slots[("gate", i)], slots[("gate_b", i)]), k_img=Cp, n_img=ldg)
            if fused16:
                pass              # (dz is already complete)
            elif ldy < Np:      # dz += dL W_gate
                gemm_nt_cols(dL16, aux["wtg"], EPI_F32_RESID, co, res=dz, outF=dz)
            else:
                gemm_nt(dL16, aux["wtg"], EPI_F32_RESID, res=dz, outF=dz)
            s1, s2 = slots[("bn_s1", i)], slots[("bn_s2", i)]
            if not fused16:      # (the fused backward accumulated the BatchNorm backward sums itself)
                call("sed_colstats", dz, ldy, L["Y"], ldy, L["ah"], L["bh"], s1, s2, Mi, co, 1)
            bn = f"cnn.cnn.batchnorm{i}."
            # (first layer with 16 filters: dY only feeds the streaming weight-gradient reduction -- 16 columns are all it needs)
            ldyo = 16 if (i == 0 and fused16) else ldg
            dY16 = E(Mi, ldyo, dt=BF16)
            call("sed_bn_bwd", dz, ldy, L["Y"], ldy, L["ah"], L["bh"], self.P(bn + "weight"), s1, s2, dY16, ldyo, Mi, co)
            del dz, dL16
            if aux["dyn"]:
                pass              # (the weight gradient of the four basis kernels takes a (x) dY: `_fdy_mix_bwd` below)
            elif L["col"] is None:      # direct first convolution: the patches come from the spectrogram again; [ldg, Kp] image as the TN kernel's
                call("sed_conv0_dw16", dY16, ldyo, L["mel"], slots[("conv", i)], Kp, slots[("conv_b", i)], B, Hc)
            else:
                self._dw_swapped(dY16, L["col"], Mi, co, 9 * cin, out=(slots[("conv", i)], slots[("conv_b", i)]), n_img=ldg)
            cv = f"cnn.cnn.conv{i}."
            if aux["dyn"]:
                dout = self._fdy_mix_bwd(W, i, aux, L, dY16, B, G, slots)
            elif i > 0:
                dcol = E(Mi, Kp, dt=BF16)
                gemm_nt(dY16, W[cv + "weight"].wt, EPI_BF16, outH=dcol, K=ldg)      # (the first ldg of the transposed image's Np columns)
                dout = E(B, Hc, Wc, cin)
                call("sed_col2im3x3", dcol, Kp, dout, B, Hc, Wc, cin)
            cctx["layers"][i] = None

    def _fpool_bwd(self, W, ectx, dpooled, G, need_dx):
        if self.m.f_pool_name != "attention":
            return super()._fpool_bwd(W, ectx, dpooled, G, need_dx)
        dev = dpooled.device
        B, N, tp = ectx["B"], ectx["N"], ectx["tp"]
        M = B * N
        E = empty(dev)
        pre = "f_pool_module."
        gw = G(pre + "frequency_att.out_proj.weight")
        g16 = self._dw_accum(dpooled, ectx["pool_att16"], B * tp, gw, G(pre + "frequency_att.out_proj.bias"))
        datt = E(B * tp, D)
        gemm_nt(g16, W[pre + "frequency_att.out_proj.weight"].wt, EPI_F32, outF=datt)
        dkv = E(M, 2 * D, dt=BF16)
        dq = torch.zeros(1, D, dtype=F32, device=dev)
        call("sed_fpool_attn_bwd", ectx["pool_kv16"], ectx["pool_q"], ectx["pool_probs"], datt, dkv, dq, B, N, tp, is_f16(ectx["pool_kv16"]))
        dh = self._token_query_bwd(W, pre, ectx["pool_h16"], dq, dkv, G, train=gw is not None)
        gpool = E(B, N, D)
        call("sed_layernorm_bwd", dh, ectx["pool_x"], ectx["pool_mean"], ectx["pool_rstd"], self.P("out_norm.weight"), 1.0,
             gpool.view(M, D), 0, G("out_norm.weight"), G("out_norm.bias"), M, D)
        return gpool

    # ------------------------------------------------------------------ stages of SedEngine._backward_impl
    def _heads_bwd(self, W, ctx, grads, G):
        m = self.m
        m._at_grad_seen = m.has_at and grads.get("at_out") is not None
        dasm = getattr(m, "dasm_head", None)
        if dasm is None:
            return super()._heads_bwd(W, ctx, grads, G)
        # query decoder + dual-stream head (dasm.py): gradients of the SED decoder's output and of the backbone's frame tokens
        hc = ctx["hctx"]
        need_dframe = self._lowest_trainable_fwd(m.depth) < m.depth or G("backbone.norm.weight") is not None
        dframe, g = dasm.backward(hc, grads.get("strong"), grads.get("weak"), grads.get("at_out"), G, need_dframe=need_dframe)
        m._extra_input_grads = [d for d, want in zip(hc.get("dquery") or [], hc.get("query_grads") or []) if want]
        return g, dframe

    def _head10_bwd(self, ctx, ds, dw, G):
        m, hc = self.m, ctx["hctx"]
        B, Tdec, Dd = ctx["xd"].shape
        Z = lambda *s: torch.zeros(*s, dtype=F32, device=ctx["xd"].device)
        g_pad = torch.empty(B, Tdec, D, dtype=F32, device=ctx["xd"].device)
        gw_pad = Z(m.class_num, D)
        call("sed_head_bwd", hc["xd_pad"], hc["w_pad"], hc["strong"], hc["sums"], ds, dw, hc["temp"], g_pad, gw_pad,
             G("classifier.bias") if G("classifier.bias") is not None else Z(m.class_num), B, Tdec, m.class_num)
        if G("classifier.weight") is not None:
            G("classifier.weight").add_(gw_pad[:, :Dd])
        return g_pad[:, :, :Dd].contiguous()

    def _context_bwd(self, W, ctx, g, G):
        """The context network's backward into the gradient-image slots of this backward (`_grad_slots`: the CNN branch's are filled by
        `_trunk_bwd`), then the scatter that returns the context network's to the masters."""
        dec_train = G("decoder.encoder_blocks.0.attn.in_proj.weight") is not None
        cnn_train = G("cnn.cnn.conv0.weight") is not None
        slots, scatter = ctx["gslots"] = self._grad_slots(ctx["B"], g.device, G, dec_train, cnn_train)
        ctx["dctx"]["slots"] = slots        # (`_relattn_sink` reads them)
        g = self._decoder_bwd(W, ctx["dctx"], g, G, dec_train)
        if dec_train:
            self._join_dw()      # out_proj / in_proj gradient images were filled on the weight-gradient side stream
            if "dec" in scatter:
                call("sed_scatter_add_f32", *scatter["dec"])
        return g

    def _trunk_bwd(self, W, ctx, g, G):
        """norm_after_merge (DASM), the projector merge, the CNN branch, the two projections -> d(pooled) [B tp, D]."""
        m = self.m
        B, Tdec, tp = ctx["B"], ctx["Tdec"], ctx["tp"]
        Dd = m.decoder_dim
        M = B * Tdec
        E = empty(g.device)
        slots, scatter = ctx["gslots"]
        if ctx.get("nam") is not None:
            nam = ctx["nam"]
            gm = E(B, Tdec, Dd)
            call("sed_layernorm_bwd", g.contiguous().view(M, Dd), nam["x"].view(M, Dd), nam["mean"], nam["rstd"], self.P("norm_after_merge.weight"), 1.0,
                 gm.view(M, Dd), 0, G("norm_after_merge.weight"), G("norm_after_merge.bias"), M, Dd)
            g = gm
        Tc = ctx["cctx"]["Tc"]
        dP1, dP2 = E(B * tp, Dd), E(B * Tc, Dd)
        call("sed_pmam_merge_bwd", g.contiguous(), ctx["P2"], self.P("merge_weight"), dP1, dP2, G("merge_weight"), B, tp, 1, m.decode_ratio,
             Tc, Tdec // Tc, Dd)
        g16 = self._dw_accum(dP2, ctx["feat"], B * Tc, G("cnn_projector.weight"), G("cnn_projector.bias"))
        dfeat = E(B * Tc, ctx["feat"].shape[1])
        gemm_nt(g16, W["cnn_projector.weight"].wt, EPI_F32, outF=dfeat)
        if G("cnn.cnn.conv0.weight") is not None:
            self._cnn_bwd(W, ctx["cctx"], dfeat, B, G, slots)
            if "cnn" in scatter:
                call("sed_scatter_add_f32", *scatter["cnn"])
        g16 = self._dw_accum(dP1, ctx["pooled"].view(B * tp, D), B * tp, G("transformer_projector.weight"), G("transformer_projector.bias"))
        dpooled = E(B * tp, D)
        gemm_nt(g16, W["transformer_projector.weight"].wt, EPI_F32, outF=dpooled)
        return dpooled

    def _scan_lowest_trainable(self, G, depth):
        """From the requires_grad flags (a LoRA block's frozen base weights have no gradient view, its factors do): the lowest block with
        a trainable parameter; 0 when the patch embedding trains."""
        pbn = self.m._param_by_name
        if any(pbn[n].requires_grad for n in ("backbone.patch_embed.proj.weight", "backbone.cls_token")):
            return 0, True
        live = {int(n.split(".")[2]) for n, p in pbn.items() if p.requires_grad and n.startswith("backbone.blocks.")}
        return min((i for i in live if i < depth), default=depth), False

    def _enc_layer_bwd(self, W, ectx, li, g, G):
        """The block's backward with the LoRA linears' weight gradients redirected: to the factors' gradients through the skinny products
        of `_dw_accum` (`_LoraSlot`), or through a scratch of the full dW that `sed_lora_grad` projects onto the factors afterwards."""
        m = self.m
        s = float(m.lora_scaling) if m.lora_r else 0.0
        tmp = {}

        def Gl(name):
            base = name[:-7]
            if not (name.endswith(".weight") and base + ".lora_A" in m._param_by_name and G(base + ".lora_A") is not None and G(name) is None):
                return G(name)
            if self.lora_skinny and m.lora_r <= 8:
                # (`_dw_accum` turns this into the four skinny products; the gradient of the merged weight is never formed)
                return _LoraSlot(self.P(base + ".lora_A").detach(), self.P(base + ".lora_B").detach(), G(base + ".lora_A"),
                                 G(base + ".lora_B"), m.lora_r, s)
            if name not in tmp:
                tmp[name] = torch.zeros_like(m._param_by_name[name])
            return tmp[name]
        g = super()._enc_layer_bwd(W, ectx, li, g, Gl)
        if tmp:
            self._join_dw()      # the full dW_eff scratch of a LoRA layer comes from the side stream; sed_lora_grad reads it here
        for name, dW in tmp.items():
            base = name[:-7]
            call("sed_lora_grad", dW, self.P(base + ".lora_A").detach(), self.P(base + ".lora_B").detach(), s, G(base + ".lora_A"),
                 G(base + ".lora_B"), dW.shape[0], dW.shape[1], m.lora_r)
        return g
