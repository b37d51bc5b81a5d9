"""Frequency pooling at the tapped encoder layer: 'mean_pool' and the frequency-wise transformer, forward and backward; and the backward
of the final norm for a head that reads the frame tokens."""
import contextlib

import torch

from .. import ops
from ..ops import BF16, F16, F32, call, gemm_nt, split3, o_kind
from ..ops import EPI_F32, EPI_F32_RESID, EPI_BF16, EPI_GELU, EPI_GELU32
from . import ACT, D, FPOOL_HEADS, FPOOL_TRANSFORMER, empty, stats


class Pooling:
    def _fpool_fwd(self, W, x, Bx, tp, save, ctx):
        """'mean_pool' frequency pooling (passt_sed.py:199-210): out_norm + mean over the frequency rows of the sequence (12, or the
        kept ones of structured patchout) -> [Bx, tp, D].  Other values of `f_pool` have a stage pair of their own."""
        if self.m.f_pool_name == FPOOL_TRANSFORMER:
            return self._fpool_tr_fwd(W, x, Bx, tp, save, ctx)
        dev = x.device
        F = ctx["F"]
        M = Bx * (2 + F * tp)
        pooled = torch.empty(Bx, tp, D, dtype=F32, device=dev)
        pm, pr = stats(lambda n: torch.zeros(n, device=dev), M, save)
        call("sed_fpool_rows_fwd", x, self.P("out_norm.weight"), self.P("out_norm.bias"), 1e-5, pooled, pm, pr, Bx, tp, F)
        if save:
            ctx.update(pool_x=x, pool_mean=pm, pool_rstd=pr)
        return pooled

    def _fpool_tr_fwd(self, W, x, Bx, tp, save, ctx):
        """Frequency-wise transformer pooling (src/models/pooling.py:18-34 behind passt_sed.py:199-218): out_norm, then per (clip or
        window, time column) the sequence [tag | F frequency rows] through two pre-LN timm blocks of 4 heads (LayerNorm eps 1e-5, qkv
        without a bias), the closing LayerNorm, and row 0 of every sequence -> [Bx, tp, D].  The residual stream is fp32 [S N, D] with
        S = Bx tp, N = 1 + F; the GEMMs and block LayerNorms are the model's own, on M = S N rows.
        Operand precision (`_fpool_split_on`): training-mode passes run the four GEMMs of a block on plain f16 operands like the encoder
        blocks; scored passes (module in eval mode, nothing saved) run them in split precision like the context network's
        ([hi | lo | hi] activations against [hi | hi | lo] weight images, which `_weights` rewrites every forward) -- qkv then leaves
        its GEMM in fp32 and the attention kernel writes the split image of its output itself.  DESIGN.md section 3 has the measured
        posterior errors of both forms."""
        F = ctx["F"]
        N, S = 1 + F, Bx * tp
        M = S * N
        E = empty(x.device)
        SP = self._fpool_split_on(save)
        mode = 4 if SP else 1
        img = lambda k=D: E(M, 3 * k, dt=F16) if SP else E(M, k, dt=ACT)       # operand image of an [M, k] activation
        wk = (lambda n: W[n].ws) if SP else (lambda n: W[n].w)
        pre = "f_pool_module."
        cur = E(M, D)
        pm, pr = stats(E, M, save)
        call("sed_fpool_seq_build_fwd", x, self.P("out_norm.weight"), self.P("out_norm.bias"), 1e-5, self.P(pre + "linear_emb.weight"),
             self.P(pre + "linear_emb.bias"), cur, pm, pr, Bx, tp, F)
        layers = []
        with (ops.split_precision() if SP else contextlib.nullcontext()):
            for i in range(2):
                p = f"{pre}frequency_transformer.{i}."
                h16 = img()
                mean1, rstd1 = stats(E, M, save)
                call("sed_layernorm_fwd", cur, self.P(p + "norm1.weight"), self.P(p + "norm1.bias"), 1e-5, 1.0, h16, None, mean1, rstd1, M, D, mode)
                if SP:
                    qkv = E(M, 3 * D)
                    gemm_nt(h16, wk(p + "attn.qkv.weight"), EPI_F32, outF=qkv)
                else:
                    qkv = E(M, 3 * D, dt=ACT)
                    gemm_nt(h16, wk(p + "attn.qkv.weight"), EPI_BF16, outH=qkv)
                o16 = img()
                call("sed_attn_short_fwd", qkv, o16, S, N, FPOOL_HEADS, o_kind(qkv), mode)
                x_mid = E(M, D) if save else cur        # (nothing saved: the stream is updated in place)
                gemm_nt(o16, wk(p + "attn.proj.weight"), EPI_F32_RESID, bias=self.P(p + "attn.proj.bias"), res=cur, outF=x_mid)
                h2 = img()
                mean2, rstd2 = stats(E, M, save)
                call("sed_layernorm_fwd", x_mid, self.P(p + "norm2.weight"), self.P(p + "norm2.bias"), 1e-5, 1.0, h2, None, mean2, rstd2, M, D, mode)
                hpre = E(M, 4 * D, dt=BF16 if save else ACT)      # (GELU pre-activation: read by the backward only)
                if SP:
                    act = E(M, 4 * D)
                    gemm_nt(h2, wk(p + "mlp.fc1.weight"), EPI_GELU32, bias=self.P(p + "mlp.fc1.bias"), outH=hpre, outF=act)
                    act = split3(act, M, 4 * D)         # forward operand and (first third) weight-gradient operand of fc2
                else:
                    act = E(M, 4 * D, dt=ACT)
                    gemm_nt(h2, wk(p + "mlp.fc1.weight"), EPI_GELU, bias=self.P(p + "mlp.fc1.bias"), outH=hpre, outH2=act)
                x_out = E(M, D) if save else x_mid
                gemm_nt(act, wk(p + "mlp.fc2.weight"), EPI_F32_RESID, bias=self.P(p + "mlp.fc2.bias"), res=x_mid, outF=x_out)
                if save:
                    # (split images [M, 3 k]: the first third is the f16 operand of the weight gradients)
                    layers.append(dict(x_in=cur, h16=h16, qkv=qkv, o16=o16, x_mid=x_mid, h2=h2, hpre=hpre, act=act, mean1=mean1, rstd1=rstd1,
                                       mean2=mean2, rstd2=rstd2))
                cur = x_out
        pooled = E(Bx, tp, D)
        fm, fr = stats(E, S, save)
        call("sed_fpool_rownorm_fwd", cur, self.P(pre + "frequency_transformer_norm.weight"), self.P(pre + "frequency_transformer_norm.bias"),
             1e-5, pooled, fm, fr, S, N)
        if save:
            ctx.update(pool_x=x, pool_mean=pm, pool_rstd=pr, pool_tr=dict(layers=layers, x_out=cur, fmean=fm, frstd=fr))
        return pooled

    def _fpool_bwd(self, W, ectx, dpooled, G, need_dx):
        """Backward of `_fpool_fwd`; -> its gradient at the encoder residual stream of the tapped layer [B, N, D] (cls / dist rows
        zero), or None when `need_dx` is false and the form can skip it."""
        if self.m.f_pool_name == FPOOL_TRANSFORMER:
            return self._fpool_tr_bwd(W, ectx, dpooled, G, need_dx)
        B, N, tp, F = ectx["B"], ectx["N"], ectx["tp"], ectx["F"]
        dev = dpooled.device
        pool_dx, dtok_tmp = torch.zeros(B, N, D, dtype=F32, device=dev), torch.empty(B, N, D, dtype=F32, device=dev)
        call("sed_fpool_rows_bwd", dpooled.contiguous(), ectx["pool_x"], ectx["pool_mean"], ectx["pool_rstd"], self.P("out_norm.weight"),
             dtok_tmp, pool_dx, G("out_norm.weight"), G("out_norm.bias"), B, tp, F)
        return pool_dx if need_dx else None

    def _fpool_tr_bwd(self, W, ectx, dpooled, G, need_dx):
        """Backward of `_fpool_tr_fwd`.  A frozen module (finetune1: `G` names none of its tensors) is still walked: out_norm and the
        encoder lie under it."""
        B, tp, F = ectx["B"], ectx["tp"], ectx["F"]
        T = ectx.pop("pool_tr")
        N, S = 1 + F, B * tp
        M = S * N
        dev = dpooled.device
        E = empty(dev)
        pre = "f_pool_module."
        part = getattr(self, "_fpool_ws", None)       # per-workgroup partials of the parameter-gradient reductions (see include/sed_hip.h)
        if part is None or part.device != dev:
            part = self._fpool_ws = torch.empty(256 * 3 * D, dtype=F32, device=dev)
        g = E(M, D)
        call("sed_fpool_rownorm_bwd", dpooled.contiguous(), T["x_out"], T["fmean"], T["frstd"], self.P(pre + "frequency_transformer_norm.weight"),
             g, G(pre + "frequency_transformer_norm.weight"), G(pre + "frequency_transformer_norm.bias"), part, part.numel(), S, N)
        for i in (1, 0):
            L = T["layers"][i]

            def attn_bwd(do16, dqkv):
                call("sed_attn_short_bwd", L["qkv"], do16, dqkv, S, N, FPOOL_HEADS, o_kind(L["qkv"]))
            self._preln_block_bwd(W, f"{pre}frequency_transformer.{i}.", L, g, G, attn_bwd, x16=False, qkv_bias=False)
            T["layers"][i] = None       # free saved activations
        # ---- the sequence build: out_norm, and the tag row (linear_emb applied to 1: weight[:, 0] and bias get the same gradient)
        gw, gb = G(pre + "linear_emb.weight"), G(pre + "linear_emb.bias")
        dtag = torch.zeros(D, dtype=F32, device=dev) if (gw is not None or gb is not None) else None
        gpool = E(B, ectx["N"], D) if need_dx else None
        call("sed_fpool_seq_build_bwd", g, ectx["pool_x"], ectx["pool_mean"], ectx["pool_rstd"], self.P("out_norm.weight"), gpool,
             G("out_norm.weight"), G("out_norm.bias"), dtag, part, part.numel(), B, tp, F)
        if gw is not None:
            gw.view(D).add_(dtag)
        if gb is not None:
            gb.add_(dtag)
        return gpool

    def _frame_norm_bwd(self, ectx, dframe, G, need_dx):
        """A head that reads the final-norm patch tokens (DASM's tagging stream, detect_any_sound.py:350): their gradient [B, N - 2, D]
        through backbone.norm into the top of the stack, like the AT head's."""
        B, N = ectx["B"], ectx["N"]
        dfull = torch.zeros(B, N, D, dtype=F32, device=dframe.device)
        dfull[:, 2:, :] = dframe
        genc = torch.empty(B, N, D, dtype=F32, device=dframe.device)
        call("sed_layernorm_bwd", dfull.view(B * N, D), ectx["x_final"], ectx["fmean"], ectx["frstd"], self.P("backbone.norm.weight"), 1.0,
             genc.view(B * N, D), 0, G("backbone.norm.weight"), G("backbone.norm.bias"), B * N, D)
        return genc if need_dx else None
