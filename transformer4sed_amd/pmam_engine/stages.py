"""The stages of SedEngine's forward / backward drivers that this variant replaces (passt_cnn.py:31-88): attention frequency pooling,
the 384-wide context-network adapters, the trunk (CNN branch, projectors, merge) and the heads."""
import torch

from .. import ops
from ..engine import ACT, D, H, empty, stats
from ..ops import BF16, F32, call, gemm_nt, split3, is_f16
from ..ops import EPI_F32
from . import HD_PAD


class Stages:
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

    def _context_bwd(self, W, ctx, g, G):
        """The context network's backward into the gradient-image slots of this backward (`_grad_slots`: the CNN branch's are filled by
        `_trunk_bwd`), then the scatter that returns the context network's to the masters."""
        dec_train = G("decoder.encoder_blocks.0.attn.in_proj.weight") is not None
        cnn_train = G("cnn.cnn.conv0.weight") is not None
        slots, scatter = ctx["gslots"] = self._grad_slots(ctx["B"], g.device, G, dec_train, cnn_train, T=ctx["T"])
        ctx["dctx"]["slots"] = slots        # (`_relattn_sink` reads them)
        g = self._decoder_bwd(W, ctx["dctx"], g, G, dec_train)
        if dec_train:
            self._join_dw()      # out_proj / in_proj gradient images were filled on the weight-gradient side stream
            if "dec" in scatter:
                call("sed_scatter_add_f32", *scatter["dec"])
        return g

    # ------------------------------------------------------------------ trunk
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

    # ------------------------------------------------------------------ heads
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
