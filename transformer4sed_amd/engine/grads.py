"""Gradient plumbing every backward stage shares: the weight-gradient side stream, `_dw_accum`, the MLP backward and the backward of
one pre-LN transformer block."""
import torch

from .. import ops
from ..ops import BF16, F16, F32, call, gemm_nt, gemm_dw, gemm_dw_tn, dw_tn_ok, pad64, transpose_bf16, to_bf16_
from ..ops import EPI_F32, EPI_F32_RESID, EPI_BF16, EPI_DGELU
from . import D, empty


class Grads:
    def _join_dw(self):
        """Make the current stream wait for the weight-gradient GEMMs issued on the side stream so far."""
        if self._dw_pending:
            torch.cuda.current_stream().wait_stream(self._dw_stream)
            self._dw_pending = False

    def _g16_take(self, g):
        """bf16 image of the residual-stream gradient `g` if the LayerNorm backward that last wrote `g` left one (and nobody touched `g`
        through torch since); consumed by the call."""
        t, self._genc16 = getattr(self, "_genc16", None), None
        return t[1] if (t is not None and t[0] is g and t[2] == g._version) else None

    def _on_dw_stream(self, run, *operands):
        """`run()` (weight-gradient work reading `operands`) on the weight-gradient side stream -- see `dw_side`; on the current stream
        while the kernel timer instruments a step or off the GPU.  `_join_dw` orders the current stream behind it."""
        if not (self.dw_side and ops.TIMER is None and operands[0].is_cuda):
            return run()
        dev = operands[0].device
        if self._dw_stream is None:
            self._dw_stream = torch.cuda.Stream(device=dev)
        self._dw_stream.wait_stream(torch.cuda.current_stream(dev))        # dY, the saved operand and the zeroed arena are ready
        with torch.cuda.stream(self._dw_stream):
            run()
        for t in operands:      # the caching allocator must not hand these out again before the side stream has read them
            t.record_stream(self._dw_stream)
        self._dw_pending = True

    def _dw_accum(self, dy, x, M, gW, bias=None, dy16=None, k_in=None):
        """gW += dy^T x (weight gradient), bias += column sums of dy.  dy [M, n_out] f32 or bf16, x [M, k_in] (saved forward
        operand, 16-bit or f32); gW / bias are arena views or None.  Returns dy as a bf16 [M, n_out] tensor (operand of the
        dX GEMM that follows).  TN kernel on the operands as they lie when the shapes allow it (tokens % 64, features % 256);
        otherwise transposed copies + the NT split-K kernel."""
        if dy16 is not None:      # the producer of dy already wrote its bf16 image (sed_layernorm_bwd_x16): no cast pass, bias sums in the TN kernel
            dy = dy16
        n_out, ldx = dy.shape[1], x.shape[1]
        # a saved split-precision image [M, 3 k_in] = [hi | lo | hi] (context network, MLM head) serves as the f16 operand through its
        # first third: the weight gradient sees the activation at the precision the encoder's gradients see theirs
        # (callers that hold split images pass `k_in`; otherwise it is inferred from the gradient view)
        if k_in is None:
            k_in = gW.shape[1] if (gW is not None and x.dtype == F16 and ldx == 3 * gW.shape[1]) else ldx
        E = empty(dy.device)
        # (the TN kernel masks a ragged last 64-token tile itself)
        tn = self.dw_tn and M >= 1024 and dw_tn_ok(M, n_out, k_in) and x.dtype in (F16, BF16, F32)
        if tn and x.dtype == F32 and gW is not None:
            # an fp32 saved operand (projector / pooling inputs): one cast pass to bf16 instead of a transposing pass, then the TN kernel
            x16 = E(M, ldx, dt=BF16)
            transpose_bf16(x, M, ldx, None, out_s=x16)
            x = x16
        if tn:
            g16 = E(M, n_out, dt=BF16) if dy.dtype == F32 else None
            # bias gradient: with a 16-bit dy the TN kernel sums its own dY fragments (no extra pass over dy); an fp32 dy needs the
            # cast pass anyway, which also yields the column sums
            bias_in_gemm = g16 is None and bias is not None and gW is not None
            if g16 is not None or (bias is not None and not bias_in_gemm):
                transpose_bf16(dy, M, n_out, None, out_s=g16, colsum=bias)   # cast and/or column sums only, one pass
            dy16 = g16 if g16 is not None else dy
            if gW is not None:
                self._on_dw_stream(lambda: gemm_dw_tn(dy16, x, gW, tokens=M, dbias=bias if bias_in_gemm else None, k_in=k_in), dy16, x)
            return dy16
        Mpad = pad64(M)
        g16 = E(M, n_out, dt=BF16) if dy.dtype == F32 else None
        gT = E(n_out, Mpad, dt=BF16)
        transpose_bf16(dy, M, n_out, gT, out_s=g16, colsum=bias)
        if gW is not None:
            xT = E(k_in, Mpad, dt=BF16)
            transpose_bf16(x, M, k_in, xT, ld=ldx)
            # this path adds into gW with atomics on the CURRENT stream; TN work still pending on the side stream adds its split-K
            # workspace into the same gW with a plain read-modify-write (a window group of another M may have taken that path): order them
            self._join_dw()
            gemm_dw(gT, xT, gW)
        return g16 if g16 is not None else dy

    def _mlp_bwd(self, W, n1, n2, dy, x16, hpre, act, M, G, residual, dy16=None):
        # (operand widths of the two weight gradients come from the weight images: a saved split image [M, 3 k] serves through its first third)
        """Backward of y = fc2(gelu(fc1(x))) given dy [M, n_out] f32.  Returns dx f32 [M, D] (new tensor), or adds
        into `residual` (f32 [M, D]) when given.  Weight/bias grads go to the arena when trainable."""
        E = empty(dy.device)
        w1, w2 = W[n1 + ".weight"], W[n2 + ".weight"]
        hid = w1.w.shape[0]
        train = G(n1 + ".weight") is not None
        hpre = to_bf16_(hpre)
        g16 = self._dw_accum(dy, act, M, G(n2 + ".weight") if train else None, G(n2 + ".bias") if train else None, dy16=dy16, k_in=w2.w.shape[1])
        dh16 = E(M, hid, dt=BF16)
        gemm_nt(g16, w2.wt, EPI_DGELU, outH=dh16, aux=hpre)
        if train:
            self._dw_accum(dh16, x16, M, G(n1 + ".weight"), G(n1 + ".bias"), k_in=w1.w.shape[1])
        dx = residual if residual is not None else E(M, w1.wt.shape[0])
        gemm_nt(dh16, w1.wt, EPI_F32 if residual is None else EPI_F32_RESID, res=residual, outF=dx)
        return dx

    def _preln_block_bwd(self, W, p, L, g2, G, attn_bwd, x16, dy16=None, qkv_bias=True):
        """Backward of one pre-LN block at parameter prefix `p` (an encoder block, a block of the transformer pooling) on the stream
        gradient g2 [M, D] fp32, in place:  x_mid = x_in + proj(attn(qkv(LN1(x_in)))),  x_out = x_mid + fc2(gelu(fc1(LN2(x_mid)))).
        `L`: the forward's saved tensors; `attn_bwd(do16, dqkv)`: the attention backward, d(output) bf16 [M, D] -> d(qkv) bf16 [M, 3 D];
        `dy16`: bf16 image of the incoming g2 if there is one.  `x16`: the LayerNorm backwards also leave the bf16 image of the g2 they just
        updated (sed_layernorm_bwd_x16) -- LN2's feeds proj's weight gradient and dX GEMM, LN1's is returned (None without `x16`)."""
        M = g2.shape[0]
        E = empty(g2.device)

        def ln_bwd(dln, x, mean, rstd, norm):
            g16 = E(M, D, dt=BF16) if x16 else None
            call("sed_layernorm_bwd_x16" if x16 else "sed_layernorm_bwd", dln, x, mean, rstd, self.P(p + norm + ".weight"), 1.0, g2, 1,
                 G(p + norm + ".weight"), G(p + norm + ".bias"), *((g16,) if x16 else ()), M, D)
            return g16
        dln = self._mlp_bwd(W, p + "mlp.fc1", p + "mlp.fc2", g2, L["h2"], L["hpre"], L["act"], M, G, residual=None, dy16=dy16)
        gmid16 = ln_bwd(dln, L["x_mid"], L["mean2"], L["rstd2"], "norm2")
        del dln
        g16 = self._dw_accum(g2, L["o16"], M, G(p + "attn.proj.weight"), G(p + "attn.proj.bias"), dy16=gmid16, k_in=D)
        do16 = E(M, D, dt=BF16)
        gemm_nt(g16, W[p + "attn.proj.weight"].wt, EPI_BF16, outH=do16)
        dqkv = E(M, 3 * D, dt=BF16)
        attn_bwd(do16, dqkv)
        del do16
        self._dw_accum(dqkv, L["h16"], M, G(p + "attn.qkv.weight"), G(p + "attn.qkv.bias") if qkv_bias else None, k_in=D)
        dln = E(M, D)
        gemm_nt(dqkv, W[p + "attn.qkv.weight"].wt, EPI_F32, outF=dln)
        return ln_bwd(dln, L["x_in"], L["mean1"], L["rstd1"], "norm1")
