"""The context networks of the engine: the shared rel-pos attention sub-block, the Transformer-XL schedule (at any width) and the
Conformer, forward and backward."""
import contextlib
import math

import torch

from .. import ops
from ..ops import BF16, F16, F32, call, gemm_nt, gemm_dw, pad64, transpose_bf16, to_bf16_, is_f16, split3, o_kind
from ..ops import EPI_F32, EPI_F32_RESID, EPI_BF16, EPI_GELU32
from . import ACT, D, H, empty, stats


def band_half_width(model, dev, T):
    """The context network's local window (PaSST_SED(decoder_win_len=...)) as the band kernels take it: int32 [H] on `dev`, made once
    per device; None without a window.  The reference's mask has side decoder_pos_emd_len and fails at any other length."""
    dec = model.decoder
    if dec.half_widths is None:
        return None
    if T != dec.seq_len:
        raise RuntimeError(f"decoder_win_len: the attention mask has side {dec.seq_len} (decoder_pos_emd_len), the sequence has {T} frames")
    return dec.half_width_tensor(dev)


def in_split_precision(fwd):
    """Decorator of a context-network forward: every GEMM of it runs on split-precision operands (3x K issued), so the whole call runs
    inside ops.split_precision(), entered once."""
    def run(self, *args):
        if getattr(self, "_in_split", False):
            return fwd(self, *args)
        self._in_split = True
        try:
            with ops.split_precision():
                return fwd(self, *args)
        finally:
            self._in_split = False
    run.__doc__ = fwd.__doc__
    return run


class Context:
    def _relattn_terms2(self, M):
        """in_proj on two split-precision terms and linear_pos on plain operands (see `dec_terms2`; the 256^2 kernel's domain).  Decides the
        image the LayerNorm in front of `_relattn_fwd` writes, the table `_pos` hands out and the qkv entry point."""
        return self.dec_terms2 and M >= 1024

    def _ctx_ln_fwd(self, x, norm, scale, mean, rstd, plain=False, want32=False):
        """LayerNorm `norm` (parameter prefix) of the context network's stream x [..., width] fp32 -> (operand image of the result for
        the GEMM that follows, the fp32 result shaped like x or None).  Here the kernel writes the image itself: [hi | lo | hi] in split
        precision, the plain f16 image when `plain` (`_relattn_terms2`)."""
        Dm = x.shape[-1]
        M = x.numel() // Dm
        y16 = torch.empty(M, Dm if plain else 3 * Dm, dtype=ACT, device=x.device)
        y32 = torch.empty(x.shape, dtype=F32, device=x.device) if want32 else None
        call("sed_layernorm_fwd", x, self.P(norm + ".weight"), self.P(norm + ".bias"), 1e-5, scale, y16, y32, mean, rstd, M, Dm, 1 if plain else 4)
        return y16, y32

    _ctx_ln_bwd = "sed_layernorm_bwd"       # backward of `_ctx_ln_fwd`'s LayerNorm (entry point; same arguments in every form)

    def _relattn_bias(self, pa, li):
        """(in_proj bias, pos_bias_u, pos_bias_v) of the attention at prefix `pa` (layer `li`) as the qkv kernel reads them."""
        return self.P(pa + "in_proj.bias"), self.P(pa + "pos_bias_u"), self.P(pa + "pos_bias_v")

    def _relattn_fwd(self, W, pa, li, ctx, pos16, hwt, yop, res, bias, save):
        """res + out_proj(relattn(y)): the rel-pos attention sub-block of every context network (Transformer-XL, Conformer, PMAM's 384-wide
        one).  `pa`: parameter prefix of in_proj / linear_pos / out_proj; `ctx`: B / T / Tpad / Rpad of this forward; `hwt`: the local
        window (`band_half_width`) or None; `yop`: operand image of the normalised input y -- plain f16 under `_relattn_terms2`, else
        [hi | lo | hi] in split precision; `res` fp32: what out_proj adds to, its last dim is the model width; `bias`: (in_proj bias,
        pos_bias_u, pos_bias_v) as the qkv kernel reads them.  The attention is H * 64 wide whatever the model width (a narrower model
        passes padded-head weight images).  Returns the new stream (shaped like `res`) and the tensors `_relattn_bwd` reads."""
        B, T, Tpad, Rpad = ctx["B"], ctx["T"], ctx["Tpad"], ctx["Rpad"]
        M, Dm, Da = B * T, res.shape[-1], H * 64
        dev = res.device
        E = empty(dev)
        T2 = self._relattn_terms2(M)
        # p = linear_pos(pos_emb), head-split [H, Rpad, 64] (+ transposed [H, 64, Rpad] for backward)
        Ph = E(H, Rpad, 64, dt=ACT)
        Pt = torch.zeros(H, 64, Rpad, dtype=ACT, device=dev) if save else None
        ptmp = E(Rpad, Da, dt=ACT)
        with (ops.plain_precision() if T2 else contextlib.nullcontext()):
            gemm_nt(pos16, W[pa + "linear_pos.weight"].w if T2 else W[pa + "linear_pos.weight"].ws, EPI_BF16, outH=ptmp)
        Ph.copy_(ptmp.view(Rpad, H, 64).permute(1, 0, 2))
        if save:
            Pt.copy_(ptmp.view(Rpad, H, 64).permute(1, 2, 0))
        B16 = BF16 if save else ACT   # backward-only tensors (row-major V, transposed q+u / q+v / K)
        qu, k, v, qv = E(B * H, T, 64, dt=ACT), E(B * H, T, 64, dt=ACT), E(B * H, T, 64, dt=B16), E(B * H, T, 64, dt=ACT)
        use_pool = getattr(self, "_lease_ok", False) or not save
        vt = self._zeros(("dec_vt", li, B, Tpad), (B * H, 64, Tpad), ACT, dev, use_pool)
        qut = kt = qvt = None
        if save:
            qut, kt, qvt = [self._zeros(("dec", li, j, B, Tpad), (B * H, 64, Tpad), B16, dev, use_pool) for j in range(3)]
        call("sed_gemm_qkv_w2s" if T2 else "sed_gemm_qkv", yop, W[pa + "in_proj.weight"].ws, bias[0], M, Dm if T2 else 3 * Dm, H, T, Tpad,
             qu, k, v, qut, kt, vt, qv, qvt, bias[1], bias[2], 3 if save else 1)
        o16, lse = E(M, Da), E(B * H, T)
        o16s = E(M, 3 * Da, dt=F16)      # split-precision image of the attention output, written by the kernel itself
        # (local window, decoder_win_len: the band kernels skip the key tiles no query of a workgroup sees)
        call("sed_relpos_attn_fwd" if hwt is None else "sed_relpos_attn_band_fwd", qu, qv, k, vt, Ph, o16, o16s, lse, B, H, T, Tpad, Rpad, 1, 1,
             *(() if hwt is None else (hwt,)))
        out = E(*res.shape)
        gemm_nt(o16s, W[pa + "out_proj.weight"].ws, EPI_F32_RESID, bias=self.P(pa + "out_proj.bias"), res=res, outF=out)
        # (y16 / o16s are [M, 3 K] images whose first third is the f16 operand of the weight gradients)
        return out, (dict(y16=yop, Ph=Ph, Pt=Pt, qu=qu, qut=qut, qv=qv, qvt=qvt, k=k, kt=kt, v=v, o16=o16, o16s=o16s, lse=lse) if save else None)

    @in_split_precision
    def _decoder_fwd(self, W, x, save):
        """TransformerXLDecoder (src/models/transformer_decoder.py:110-122, transformerXL.py:31-35) at the width of x [B, T, width] f32: the
        one Transformer-XL schedule of every engine.  A variant overrides `_ctx_ln_fwd` / `_ctx_ln_bwd`, `_relattn_bias` and
        `_relattn_sink`, never the schedule."""
        m, dev = self.m, x.device
        B, T, Dm = x.shape
        M = B * T
        T2 = self._relattn_terms2(M)
        pos16, _, Rpad = self._pos(T, dev, Dm, want_plain=T2)
        E = empty(dev)
        ctx = dict(B=B, T=T, Tpad=pad64(T), Rpad=Rpad, layers=[])
        cur = x
        hwt = band_half_width(m, dev, T)
        for li in range(m.decoder_layer_num):
            p = f"decoder.encoder_blocks.{li}."
            pa = p + "attn."
            in_scale = math.sqrt(Dm) if li == 0 else 1.0
            mean1, rstd1 = stats(E, M, save)
            # (two-term in_proj: the plain f16 image is all it reads)
            y16, y32 = self._ctx_ln_fwd(cur, p + "norm1", in_scale, mean1, rstd1, plain=T2, want32=True)
            x1, att = self._relattn_fwd(W, pa, li, ctx, pos16, hwt, y16, y32, self._relattn_bias(pa, li), save)
            mean2, rstd2 = stats(E, M, save)
            # (the [hi | lo | hi] image is the only form of LN2's output anybody reads -- the fc1 GEMM now, the weight gradient of fc1
            #  later through its first third)
            h2, _ = self._ctx_ln_fwd(x1, p + "norm2", 1.0, mean2, rstd2)
            hpre = E(M, Dm, dt=BF16 if save else ACT)      # (read by the backward only)
            act = E(M, Dm)
            gemm_nt(h2, W[p + "mlp.fc1.weight"].ws, EPI_GELU32, bias=self.P(p + "mlp.fc1.bias"), outH=hpre, outF=act)
            x2 = E(B, T, Dm)
            act = split3(act, M, Dm)     # the fp32 activation is not read again: forward operand and (first third) dW operand of fc2
            gemm_nt(act, W[p + "mlp.fc2.weight"].ws, EPI_F32_RESID, bias=self.P(p + "mlp.fc2.bias"), res=x1, outF=x2)
            if save:
                # y16 / h2 / act / o16s are the [M, 3 K] split-precision images the forward GEMMs consumed; their first third is the f16
                # operand of the weight gradients (TN kernel, `_dw_accum`) -- no fp32 copies saved, no transposes in the backward
                ctx["layers"].append(dict(att, x_in=cur, in_scale=in_scale, mean1=mean1, rstd1=rstd1, x1=x1, h2=h2, mean2=mean2,
                                          rstd2=rstd2, hpre=hpre, act=act))
            cur = x2
            self._tap(li, cur)
        return cur, ctx

    # ------------------------------------------------------------------ decoder="conformer"
    def _swish_ffn_fwd(self, W, ff, norm, xin, M, save):
        """xin + 0.5 * Linear(Swish(Linear(LayerNorm(xin)))) (conformer.py:98-101,134-137); `ff` / `norm`: parameter prefixes.  Returns the
        new stream [M, D] fp32 and what `_swish_ffn_bwd` reads."""
        E = empty(xin.device)
        img = lambda: E(M, 3 * D, dt=F16)       # [hi | lo | hi] operand image of an [M, D] activation
        y = img()
        mean, rstd = stats(E, M, save)
        call("sed_layernorm_fwd", xin, self.P(norm + ".weight"), self.P(norm + ".bias"), 1e-5, 1.0, y, None, mean, rstd, M, D, 4)
        h = E(M, D)
        gemm_nt(y, W[ff + ".0.weight"].ws, EPI_F32, bias=self.P(ff + ".0.bias"), outF=h)
        a = img()
        call("sed_swish_fwd", h, a, None, M, D, 4)
        out = E(M, D)
        gemm_nt(a, W[ff + ".3.weight"].ws, EPI_F32, bias=self.P(ff + ".3.bias"), outF=out)
        call("sed_scale_add_f32", out, xin, out, None, M * D, 0.5)
        return out, (dict(x_in=xin, y=y, mean=mean, rstd=rstd, h=h, a=a) if save else None)

    @in_split_precision
    def _conformer_fwd(self, W, x, save):
        """ConformerDecoder (src/models/transformer_decoder.py:157-165, conformer.py:75-144).  x [B,T,D] f32.  Per block, on the residual
        stream s (which starts as sqrt(D) x: RelPositionalEncoding's scaling is applied to the stream itself here):
            s += 0.5 ffn_macaron(norm_ff_macaron(s));  s += relattn(norm_mha(s));  s += conv_module(norm_conv(s));
            s += 0.5 ffn(norm_ff(s));  s = norm_final(s)
        The attention is the Transformer-XL block's (same kernels, same split-precision terms, same local window)."""
        m, dev = self.m, x.device
        B, T, _ = x.shape
        M = B * T
        T2 = self._relattn_terms2(M)
        pos16, _, Rpad = self._pos(T, dev, want_plain=T2)
        E = empty(dev)
        img = lambda: E(M, 3 * D, dt=F16)       # [hi | lo | hi] operand image of an [M, D] activation
        ctx = dict(B=B, T=T, Tpad=pad64(T), Rpad=Rpad, layers=[])
        hwt = band_half_width(m, dev, T)
        cur = E(M, D)
        call("sed_scale_add_f32", x, None, cur, None, M * D, math.sqrt(D))
        for li in range(m.decoder_layer_num):
            p = f"decoder.blocks.{li}."
            pa = p + "self_attn."
            x1, ffm = self._swish_ffn_fwd(W, p + "feed_forward_macaron", p + "norm_ff_macaron", cur, M, save)
            # ---- attention: x2 = x1 + out_proj(relattn(norm_mha(x1)))
            mean1, rstd1 = stats(E, M, save)
            y16, _ = self._ctx_ln_fwd(x1, p + "norm_mha", 1.0, mean1, rstd1, plain=T2)
            x2, att = self._relattn_fwd(W, pa, li, ctx, pos16, hwt, y16, x1, self._relattn_bias(pa, li), save)
            # ---- convolution module: x3 = x2 + pointwise_conv2(swish(norm(depthwise(glu(pointwise_conv1(norm_conv(x2)))))))
            pc = p + "conv_module."
            yc = img()
            meanc, rstdc = stats(E, M, save)
            call("sed_layernorm_fwd", x2, self.P(p + "norm_conv.weight"), self.P(p + "norm_conv.bias"), 1e-5, 1.0, yc, None, meanc, rstdc, M, D, 4)
            xp = E(M, 2 * D)
            gemm_nt(yc, W[pc + "pointwise_conv1.weight"].ws, EPI_F32, bias=self.P(pc + "pointwise_conv1.bias"), outF=xp)
            ys = img()
            conv, cmean, crstd = (E(M, D), E(M), E(M)) if save else (None, None, None)
            call("sed_conv_glu_dw_fwd", xp, self.P(pc + "depthwise_conv.weight"), self.P(pc + "depthwise_conv.bias"),
                 self.P(pc + "norm.weight"), self.P(pc + "norm.bias"), 1e-5, ys, None, conv, cmean, crstd, B, T, D, 4)
            x3 = E(M, D)
            gemm_nt(ys, W[pc + "pointwise_conv2.weight"].ws, EPI_F32_RESID, bias=self.P(pc + "pointwise_conv2.bias"), res=x2, outF=x3)
            x4, ff = self._swish_ffn_fwd(W, p + "feed_forward", p + "norm_ff", x3, M, save)
            out = E(M, D)
            fmean, frstd = stats(E, M, save)
            call("sed_layernorm_fwd", x4, self.P(p + "norm_final.weight"), self.P(p + "norm_final.bias"), 1e-5, 1.0, None, out, fmean, frstd, M, D, 1)
            if save:
                ctx["layers"].append(dict(att, ffm=ffm, ff=ff, x1=x1, mean1=mean1, rstd1=rstd1, x2=x2, yc=yc, meanc=meanc, rstdc=rstdc, xp=xp,
                                          ys=ys, conv=conv, cmean=cmean, crstd=crstd, x4=x4, fmean=fmean, frstd=frstd))
            cur = out
            self._tap(li, cur.view(B, T, D))
        return cur.view(B, T, D), ctx

    # ==================================================================== backward
    def _context_bwd(self, W, ctx, g, G):
        if self.m.decoder_name == "conformer":
            return self._conformer_bwd(W, ctx["dctx"], g, G, G("decoder.blocks.0.self_attn.in_proj.weight") is not None)
        return self._decoder_bwd(W, ctx["dctx"], g, G, G("decoder.encoder_blocks.0.attn.in_proj.weight") is not None)

    def _relattn_sink(self, Gl, pa, li, dctx, dev):
        """Where `_relattn_bwd` adds the parameter gradients of the attention at prefix `pa` (layer `li` of the forward behind `dctx`),
        as arena views: (weight, bias) of out_proj and in_proj, linear_pos's weight, pos_bias_u / v.  `Gl` names nothing in a frozen
        context network; the kernel still writes du / dv somewhere."""
        scratch_uv = torch.zeros(2, D, dtype=F32, device=dev)
        du, dv = Gl(pa + "pos_bias_u"), Gl(pa + "pos_bias_v")
        return dict(out_proj=(Gl(pa + "out_proj.weight"), Gl(pa + "out_proj.bias")), linear_pos=Gl(pa + "linear_pos.weight"),
                    in_proj=(Gl(pa + "in_proj.weight"), Gl(pa + "in_proj.bias")),
                    pos_bias_u=du if du is not None else scratch_uv[0], pos_bias_v=dv if dv is not None else scratch_uv[1])

    def _relattn_bwd(self, W, pa, L, dctx, posT16, hwt, g2, sink, residual):
        """Backward of `_relattn_fwd` given the stream gradient g2 [M, model width] fp32 and the forward's saved tensors `L`.  `sink`: the
        gradient destinations by role (see `_relattn_sink`; linear_pos None = frozen: only the input gradient is computed).  The
        gradient at the normalised input is added into `residual` (fp32 [M, model width]) when given, else returned in a new tensor."""
        B, T, Tpad, Rpad = dctx["B"], dctx["T"], dctx["Tpad"], dctx["Rpad"]
        M, Dm, Da = B * T, g2.shape[1], H * 64
        dev = g2.device
        E = empty(dev)
        train = sink["linear_pos"] is not None
        g16 = self._dw_accum(g2, L["o16s"], M, *sink["out_proj"], k_in=Da)
        do16 = E(M, Da, dt=BF16)
        gemm_nt(g16, W[pa + "out_proj.weight"].wt, EPI_BF16, outH=do16)
        dqkv = E(M, 3 * Da, dt=BF16)
        Dtmp = E(B * H, T)
        dOh = E(B * H, T, 64, dt=BF16)
        dOt = E(B * H, 64, Tpad, dt=BF16)
        dSt = self._zeros(("dSt", B, Tpad), (B * H, Tpad, Tpad), BF16, dev)      # scratch of this call: one buffer for all layers
        # P^T slab beside it: dK / dV as contractions over the two stored slabs the dQ kernel writes, instead of recomputing the scores
        Pst = self._zeros(("Pst", B, Tpad), (B * H, Tpad, Tpad), BF16, dev)
        dP = torch.zeros(Rpad, Da, dtype=F32, device=dev)
        # (local window: the pooled slabs may hold the full-window content of an earlier call outside the band -- the band kernels
        #  neither write nor read those tiles, see relpos_attention.hip band_tile_lo / band_tile_hi)
        call("sed_relpos_attn_bwd" if hwt is None else "sed_relpos_attn_band_bwd", L["qu"], to_bf16_(L["qut"]), L["qv"],
             to_bf16_(L["qvt"]), L["k"], to_bf16_(L["kt"]), to_bf16_(L["v"]), L["Ph"], to_bf16_(L["Pt"]), L["o16"], do16, L["lse"],
             Dtmp, dOh, dOt, dqkv, dSt, Pst, dP, sink["pos_bias_u"], sink["pos_bias_v"],
             B, H, T, Tpad, Rpad, 1 if train else 0, is_f16(L["qu"]), o_kind(L["o16"]), *(() if hwt is None else (hwt,)))
        del dSt, Pst, dOh, dOt, do16
        if train:
            dPT = E(Da, Rpad, dt=BF16)
            transpose_bf16(dP, Rpad, Da, dPT)
            gemm_dw(dPT, posT16, sink["linear_pos"])
            self._dw_accum(dqkv, L["y16"], M, *sink["in_proj"], k_in=Dm)
        dy = residual if residual is not None else E(M, Dm)       # (into `residual`: + the gradient through the residual from the normalised input)
        gemm_nt(dqkv, W[pa + "in_proj.weight"].wt, EPI_F32 if residual is None else EPI_F32_RESID, res=residual, outF=dy)
        return dy

    def _decoder_bwd(self, W, dctx, g, G, trainable):
        """Backward of `_decoder_fwd` given g = d(output) [B, T, width]; -> d(input).  Parameter gradients go to the views `G` names
        (the attention's: where `_relattn_sink` says); none is computed when `trainable` is false.  (The PMAM form of the sink needs
        `dctx["slots"]`: the views of `_grad_slots` made with `dec_train` = `trainable`, as `PmamEngine._context_bwd` (pmam_engine/stages.py) leaves them.)"""
        m = self.m
        B, T, Dm = g.shape
        M = B * T
        dev = g.device
        _, posT16, _ = self._pos(T, dev, Dm)
        hwt = band_half_width(m, dev, T)
        Gl = G if trainable else (lambda n: None)
        g = g.contiguous()
        for li in range(m.decoder_layer_num - 1, -1, -1):
            p = f"decoder.encoder_blocks.{li}."
            pa = p + "attn."
            L = dctx["layers"][li]
            g2 = g.view(M, Dm)
            # MLP branch
            dln = self._mlp_bwd(W, p + "mlp.fc1", p + "mlp.fc2", g2, L["h2"], L["hpre"], L["act"], M, Gl, residual=None)
            call(self._ctx_ln_bwd, dln, L["x1"], L["mean2"], L["rstd2"], self.P(p + "norm2.weight"), 1.0, g2, 1,
                 Gl(p + "norm2.weight"), Gl(p + "norm2.bias"), M, Dm)
            del dln
            # attention branch: x1 = y + out_proj(relattn(y)),  y = LN1(in_scale * x_in)
            self._relattn_bwd(W, pa, L, dctx, posT16, hwt, g2, self._relattn_sink(Gl, pa, li, dctx, dev), residual=g2)
            gnew = torch.empty(B, T, Dm, dtype=F32, device=dev)
            call(self._ctx_ln_bwd, g2, L["x_in"], L["mean1"], L["rstd1"], self.P(p + "norm1.weight"), L["in_scale"],
                 gnew.view(M, Dm), 0, Gl(p + "norm1.weight"), Gl(p + "norm1.bias"), M, Dm)
            g = gnew
            dctx["layers"][li] = None
        return g

    def _swish_ffn_bwd(self, W, ff, norm, S, g2, M, Gl):
        """Backward of `_swish_ffn_fwd`: adds d(xin) of the branch into the stream gradient g2 [M, D] fp32 (which already is the
        gradient through the residual connection)."""
        E = empty(g2.device)
        gh16 = E(M, D, dt=BF16)
        call("sed_scale_add_f32", g2, None, None, gh16, M * D, 0.5)        # the branch enters the stream at 0.5
        self._dw_accum(gh16, S["a"], M, Gl(ff + ".3.weight"), Gl(ff + ".3.bias"), k_in=D)
        dact = E(M, D)
        gemm_nt(gh16, W[ff + ".3.weight"].wt, EPI_F32, outF=dact)
        dh16 = E(M, D, dt=BF16)
        call("sed_swish_bwd", dact, S["h"], dh16, M * D)
        self._dw_accum(dh16, S["y"], M, Gl(ff + ".0.weight"), Gl(ff + ".0.bias"), k_in=D)
        gemm_nt(dh16, W[ff + ".0.weight"].wt, EPI_F32, outF=dact)
        call("sed_layernorm_bwd", dact, S["x_in"], S["mean"], S["rstd"], self.P(norm + ".weight"), 1.0, g2, 1, Gl(norm + ".weight"), Gl(norm + ".bias"), M, D)

    def _conv_partials(self, B, T, dev):
        """Scratch of sed_conv_glu_dw_bwd: one partial of every parameter gradient per workgroup (see include/sed_hip.h)."""
        n = min(B * ((T + 19) // 20), 256) * 34 * D
        t = getattr(self, "_conv_ws", None)
        if t is None or t.numel() < n or t.device != dev:
            t = self._conv_ws = torch.empty(n, dtype=F32, device=dev)
        return t

    def _conformer_bwd(self, W, dctx, g, G, trainable):
        m = self.m
        B, T = dctx["B"], dctx["T"]
        M = B * T
        dev = g.device
        E = empty(dev)
        _, posT16, _ = self._pos(T, dev)
        hwt = band_half_width(m, dev, T)
        Gl = G if trainable else (lambda n: None)
        g = g.contiguous()
        for li in range(m.decoder_layer_num - 1, -1, -1):
            p = f"decoder.blocks.{li}."
            pa, pc = p + "self_attn.", p + "conv_module."
            L = dctx["layers"][li]
            g2 = E(M, D)
            call("sed_layernorm_bwd", g.view(M, D), L["x4"], L["fmean"], L["frstd"], self.P(p + "norm_final.weight"), 1.0, g2, 0,
                 Gl(p + "norm_final.weight"), Gl(p + "norm_final.bias"), M, D)
            self._swish_ffn_bwd(W, p + "feed_forward", p + "norm_ff", L["ff"], g2, M, Gl)
            # ---- convolution module
            wv = lambda n: None if Gl(n) is None else Gl(n).view(W[n].w.shape)         # Conv1d [out, in, 1] gradient as the [out, in] matrix
            g16 = self._dw_accum(g2, L["ys"], M, wv(pc + "pointwise_conv2.weight"), Gl(pc + "pointwise_conv2.bias"), k_in=D)
            dys = E(M, D)
            gemm_nt(g16, W[pc + "pointwise_conv2.weight"].wt, EPI_F32, outF=dys)
            dxp = E(M, 2 * D, dt=BF16)
            call("sed_conv_glu_dw_bwd", dys, L["xp"], L["conv"], L["cmean"], L["crstd"], self.P(pc + "depthwise_conv.weight"),
                 self.P(pc + "norm.weight"), self.P(pc + "norm.bias"), dxp, Gl(pc + "depthwise_conv.weight"), Gl(pc + "depthwise_conv.bias"),
                 Gl(pc + "norm.weight"), Gl(pc + "norm.bias"), self._conv_partials(B, T, dev), self._conv_partials(B, T, dev).numel(), B, T, D)
            self._dw_accum(dxp, L["yc"], M, wv(pc + "pointwise_conv1.weight"), Gl(pc + "pointwise_conv1.bias"), k_in=D)
            gemm_nt(dxp, W[pc + "pointwise_conv1.weight"].wt, EPI_F32, outF=dys)
            call("sed_layernorm_bwd", dys, L["x2"], L["meanc"], L["rstdc"], self.P(p + "norm_conv.weight"), 1.0, g2, 1,
                 Gl(p + "norm_conv.weight"), Gl(p + "norm_conv.bias"), M, D)
            del dys, dxp
            # ---- attention
            dln = self._relattn_bwd(W, pa, L, dctx, posT16, hwt, g2, self._relattn_sink(Gl, pa, li, dctx, dev), residual=None)
            call(self._ctx_ln_bwd, dln, L["x1"], L["mean1"], L["rstd1"], self.P(p + "norm_mha.weight"), 1.0, g2, 1,
                 Gl(p + "norm_mha.weight"), Gl(p + "norm_mha.bias"), M, D)
            del dln
            self._swish_ffn_bwd(W, p + "feed_forward_macaron", p + "norm_ff_macaron", L["ffm"], g2, M, Gl)
            g = g2
            dctx["layers"][li] = None
        call("sed_scale_add_f32", g, None, g, None, M * D, math.sqrt(D))       # the stream started as sqrt(D) x
        return g.view(B, T, D)
