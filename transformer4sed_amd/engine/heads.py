"""The heads of the engine: MLM masking and head, the classifier heads, and the AT head with the token-query attention input path it
shares with the PMAM attention pooling."""
import torch

from .. import ops
from ..ops import BF16, F32, call, h2d, gemm_nt, is_f16, split3
from ..ops import EPI_F32, EPI_BF16, EPI_GELU32
from . import ACT, D, H, NCLS_MAX, empty


class Heads:
    _mlm_c = False      # MLM masking on the any-width `_c` kernels (which take the width) instead of the 768-only ones

    def _mlm_mask_fwd(self, xg, plan):
        """The MLM plan applied to the frame sequence (mask token / random frame / kept), at the sequence's own width."""
        B, Tdec, Dm = xg.shape
        dec_in = torch.empty_like(xg)
        call("sed_mlm_apply_c" if self._mlm_c else "sed_mlm_apply", xg, self.P("mask_token").reshape(Dm), plan["action"], plan["src_idx"],
             dec_in, B * Tdec, *((Dm,) if self._mlm_c else ()))
        return dec_in

    def _mlm_mask_bwd(self, g, plan, G):
        B, Tdec, Dm = g.shape
        gx = torch.zeros_like(g)
        dtok = G("mask_token") if G("mask_token") is not None else torch.zeros(Dm, dtype=F32, device=g.device)
        call("sed_mlm_apply_bwd_c" if self._mlm_c else "sed_mlm_apply_bwd", g, plan["action"], plan["src_idx"], gx, dtok, B * Tdec,
             *((Dm,) if self._mlm_c else ()))
        return gx

    def _mlm_head_fwd(self, W, xd, hpre_dt):
        """mlm_mlp on the context network's output, at its width.  -> (prediction [B, Tdec, out], saved operands); `hpre_dt`: type of
        the saved GELU pre-activation."""
        B, Tdec, Dm = xd.shape
        M = B * Tdec
        n_out = W["mlm_mlp.2.weight"].w.shape[0]
        E = empty(xd.device)
        hpre = E(M, Dm, dt=hpre_dt)
        act = E(M, Dm)
        pred = E(B, Tdec, n_out)
        with ops.split_precision():
            xd16 = split3(xd.view(M, Dm), M, Dm)
            gemm_nt(xd16, W["mlm_mlp.0.weight"].ws, EPI_GELU32, bias=self.P("mlm_mlp.0.bias"), outH=hpre, outF=act)
            act = split3(act, M, Dm)      # split images: the first third is the weight-gradient operand
            gemm_nt(act, W["mlm_mlp.2.weight"].ws, EPI_F32, bias=self.P("mlm_mlp.2.bias"), outF=pred.view(M, n_out))
        return pred, dict(xd16=xd16, hpre=hpre, act=act)

    def _mlm_head_bwd(self, W, ctx, dpred, G):
        B, Tdec, Dm = ctx["xd"].shape
        if dpred is None:
            return torch.zeros(B, Tdec, Dm, dtype=F32, device=ctx["xd"].device)
        hc = ctx["hctx"]
        M = B * Tdec
        return self._mlp_bwd(W, "mlm_mlp.0", "mlm_mlp.2", dpred.contiguous().float().view(M, -1), hc["xd16"], hc["hpre"], hc["act"], M,
                             G, residual=None).view(B, Tdec, Dm)

    def _heads_fwd(self, W, xd, ectx, opt, save, out):
        """Heads stage: fills `out` from the context network's output xd [B, Tdec, width] (MLM head, or the classifier with its sigmoid
        and linear-softmax pooling) and returns what `_heads_bwd` reads."""
        m = self.m
        B, Tdec, Dm = xd.shape
        if m.mlm:
            out["mlm_pred"], hctx = self._mlm_head_fwd(W, xd, ACT)
        elif self._wide_head(save):
            # any class count (AudioSet-Strong's 407): logits on the fp32 matrix instruction + the transposing sigmoid / pooling kernel
            # (dasm.wide_head_fwd); the dedicated kernels serve the 10-class DESED head
            from ..dasm import wide_head_fwd
            out["strong"], out["weak"], hctx = wide_head_fwd(xd.view(B * Tdec, Dm), self.P("classifier.weight").detach(),
                                                             self.P("classifier.bias").detach(), opt["temp_w"], opt["pad_mask"], B, Tdec, save)
        else:
            # (pinned staging of the mask: a pageable .to(device) here blocks the host until the whole forward has run)
            pm = None if opt["pad_mask"] is None else h2d(opt["pad_mask"], torch.uint8, xd.device)
            out["strong"], out["weak"], hctx = self._head10_fwd(xd, float(opt["temp_w"]), pm)
        return hctx or {}

    def _wide_head(self, save):
        C = self.m.class_num
        return C > NCLS_MAX or (save and C != 10)

    def _head10_fwd(self, xd, temp, pm):
        B, Tdec, C = xd.shape[0], xd.shape[1], self.m.class_num
        E = empty(xd.device)
        strong, weak, sums = E(B, C, Tdec), E(B, C), E(B, C, 2)
        call("sed_head_fwd", xd, self.P("classifier.weight"), self.P("classifier.bias"), temp, pm, strong, weak, sums, B, Tdec, C)
        return strong, weak, dict(strong=strong, sums=sums, temp=temp)

    def _heads_bwd(self, W, ctx, grads, G):
        """-> (gradient of the context network's output [B, Tdec, width], gradient of the final-norm patch tokens or None)."""
        if self.m.mlm:
            return self._mlm_head_bwd(W, ctx, grads.get("mlm_pred"), G), None
        hc = ctx["hctx"]
        ds, dw = grads.get("strong"), grads.get("weak")
        if ds is None and dw is None:
            return torch.zeros_like(ctx["xd"]), None
        if hc.get("wide"):
            from ..dasm import wide_head_bwd
            g = wide_head_bwd(hc, self.P("classifier.weight").detach(), ds, dw, G("classifier.weight"), G("classifier.bias"))
            return g.view(ctx["xd"].shape), None
        return self._head10_bwd(ctx, None if ds is None else ds.contiguous().float(), None if dw is None else dw.contiguous().float(), G), None

    def _head10_bwd(self, ctx, ds, dw, G):
        hc, g = ctx["hctx"], torch.empty_like(ctx["xd"])
        call("sed_head_bwd", ctx["xd"], self.P("classifier.weight"), hc["strong"], hc["sums"], ds, dw, hc["temp"],
             g, G("classifier.weight"), G("classifier.bias"), ctx["B"], ctx["Tdec"], self.m.class_num)
        return g

    # ------------------------------------------------------------------ a learned token queries a K/V projection of the tokens
    def _token_query_fwd(self, W, pre, x16):
        """Input path of the attention module `pre`frequency_att whose one query is the learned `pre`f_att_token (the AT head, the PMAM
        attention pooling): q [1, D] = the token through in_proj[:D], kv16 [M, 2 D] = the 16-bit tokens x16 [M, D] through in_proj[D:]."""
        E = empty(x16.device)
        win, bin_ = self.P(pre + "frequency_att.in_proj_weight"), self.P(pre + "frequency_att.in_proj_bias")
        q = E(1, D)
        call("sed_small_linear", self.P(pre + "f_att_token").reshape(1, D), win[:D], bin_[:D], q, 1, D, D, 0)
        kv16 = E(x16.shape[0], 2 * D, dt=ACT)
        gemm_nt(x16, W[pre + "frequency_att.in_proj_weight"].w[D:], EPI_BF16, bias=bin_[D:], outH=kv16)
        return q, kv16

    def _token_query_bwd(self, W, pre, x16, dq, dkv, G, train, need_dx=True):
        """Backward of `_token_query_fwd` from dq [1, D] fp32 and dkv [M, 2 D] bf16: the gradients of the token and of in_proj (when
        `train`), and -> dX [M, D] fp32 (None unless `need_dx`)."""
        M = dkv.shape[0]
        if train:
            gin, gib = G(pre + "frequency_att.in_proj_weight"), G(pre + "frequency_att.in_proj_bias")
            dtok = torch.zeros(1, D, dtype=F32, device=dkv.device)
            call("sed_small_linear_bwd", self.P(pre + "f_att_token").reshape(1, D), self.P(pre + "frequency_att.in_proj_weight")[:D], None, dq,
                 dtok, gin[:D], gib[:D], 1, D, D, 0)
            G(pre + "f_att_token").view(1, D).add_(dtok)
            self._dw_accum(dkv, x16, M, gin[D:], gib[D:])
        if not need_dx:
            return None
        dx = torch.empty(M, D, dtype=F32, device=dkv.device)
        gemm_nt(dkv, W[pre + "frequency_att.in_proj_weight"].wt[:, D:].contiguous(), EPI_F32, outF=dx)
        return dx

    # ------------------------------------------------------------------ AT head
    def _at_fwd(self, W, frame16, ectx, save):
        B, N, C = ectx["B"], ectx["N"], self.m.class_num
        E = empty(frame16.device)
        pre = "at_adpater.0."
        q, kv16 = self._token_query_fwd(W, pre, frame16)
        pooled = E(B, D)
        probs = E(B * H, N - 2) if save else None
        call("sed_attnpool_fwd", kv16, q, pooled, probs, B, N, H, is_f16(kv16))
        att = E(B, D)
        call("sed_small_linear", pooled, self.P(pre + "frequency_att.out_proj.weight"), self.P(pre + "frequency_att.out_proj.bias"), att, B, D, D, 0)
        at_out = E(B, C)
        call("sed_small_linear", att, self.P("at_adpater.1.weight"), self.P("at_adpater.1.bias"), at_out, B, C, D, 1)
        return dict(q=q, kv16=kv16, pooled=pooled, probs=probs, att=att, at_out=at_out)

    def _at_bwd(self, W, a, ectx, dat, G, need_dx):
        """Backward of the AT head.  Returns d(encoder residual stream) [B, N, D] (or None when not needed)."""
        B, N, C = ectx["B"], ectx["N"], self.m.class_num
        M = B * N
        E = empty(dat.device)
        pre = "at_adpater.0."
        datt = E(B, D)
        call("sed_small_linear_bwd", a["att"], self.P("at_adpater.1.weight"), a["at_out"], dat, datt,
             G("at_adpater.1.weight"), G("at_adpater.1.bias"), B, C, D, 1)
        dpool = E(B, D)
        call("sed_small_linear_bwd", a["pooled"], self.P(pre + "frequency_att.out_proj.weight"), None, datt, dpool,
             G(pre + "frequency_att.out_proj.weight"), G(pre + "frequency_att.out_proj.bias"), B, D, D, 0)
        dkv = E(M, 2 * D, dt=BF16)
        dq = torch.zeros(1, D, dtype=F32, device=dat.device)
        call("sed_attnpool_bwd", a["kv16"], a["q"], a["probs"], dpool, dkv, dq, B, N, H, is_f16(a["kv16"]))
        dframe = self._token_query_bwd(W, pre, ectx["frame16"], dq, dkv, G, train=G("at_adpater.1.weight") is not None,
                                       need_dx=need_dx or G("backbone.norm.weight") is not None)       # (a trainable final norm: its gradient below)
        if dframe is None:
            return None
        genc = E(B, N, D)
        call("sed_layernorm_bwd", dframe, ectx["x_final"], ectx["fmean"], ectx["frstd"], self.P("backbone.norm.weight"),
             1.0, genc.view(M, D), 0, G("backbone.norm.weight"), G("backbone.norm.bias"), M, D)
        return genc if need_dx else None
