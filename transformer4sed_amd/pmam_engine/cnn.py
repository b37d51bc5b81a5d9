"""The CNN branch, forward and backward, and the mixing of its frequency-dynamic layers.  Shapes, row pitches and kernel routes come
from the layer plans (`_cnn_plan`, geometry.py); the forward leaves them in its context for the backward."""
import torch

from ..engine import ACT, empty
from ..ops import BF16, call, gemm_nt, gemm_nt_cols, is_f16
from ..ops import EPI_F32, EPI_F32_RESID, EPI_BF16


class Cnn:
    def _cnn_fwd(self, W, mel, train, save, drop_masks=None):
        """-> (feat fp32 [B * T/4, C_last], ctx).  train: batch statistics (and running-statistics update, torch BatchNorm semantics:
        momentum 0.99, unbiased variance); eval: running statistics."""
        m = self.m
        dev = mel.device
        B, _, T = mel.shape
        E = empty(dev)
        plans = self._cnn_plan(B, T, dev)
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
            sizes = [pl.M * a_["co"] for a_, pl in zip(self.cnn_aux, plans)]
            flat = torch.empty(sum(sizes), dtype=torch.uint8, device=dev)
            call("sed_dropout_mask", flat, flat.numel(), float(m.conv_dropout), int(torch.randint(0, 2 ** 62, (1,), generator=self._dropout_generator()).item()))
            gen_masks, off = [], 0
            for n_ in sizes:
                gen_masks.append(flat[off:off + n_])
                off += n_
        for i, (aux, pl) in enumerate(zip(self.cnn_aux, plans)):
            co, Np, Kp, Cp, cin = aux["co"], aux["Np"], aux["Kp"], aux["Cp"], aux["cin"]
            Hc, Wc, Mi, ldy = pl.H, pl.W, pl.M, pl.ldy
            Y = E(Mi, ldy)
            col = None
            if pl.direct0:      # (train: the batch-statistics sums come out of the same pass; its weight gradient: `sed_conv0_dw16`)
                call("sed_conv0_fwd16", mel, self.P("cnn.cnn.conv0.weight").detach(), self.P("cnn.cnn.conv0.bias").detach(), Y, B, T,
                     sums[i, 0] if train else None, sums[i, 1] if train else None)
            else:
                col = E(Mi, Kp, dt=ACT)
                if i == 0:
                    call("sed_conv0_im2col", mel, col, B, T, 1)
                else:
                    call("sed_conv3x3_im2col", X, col, B, Hc, Wc, cin, aux["cpin"], Kp)
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
                if not pl.direct0:
                    call("sed_colstats", Y, ldy, None, 0, None, None, s1, s2, Mi, co, 0)
            a, b, ah, bh = aff[i, 0], aff[i, 1], aff[i, 2], aff[i, 3]
            call("sed_bn_finalize", s1, s2, g, bt, m._buffer_by_name[bn + "running_mean"], m._buffer_by_name[bn + "running_var"], Mi, co,
                 0.99, 1e-3, a, b, ah, bh)
            Z = L = None
            if not pl.fused16:
                Z = E(Mi, Cp, dt=ACT)
                call("sed_bn_act", Y, ldy, a, b, Z, Mi, co, Cp, 1)
                L = E(Mi, ldy)
                if ldy < Np:
                    gemm_nt_cols(Z, W[f"cnn.cnn.cg{i}.linear.weight"].w, EPI_F32, co, bias=aux["gbias"], outF=L)
                else:
                    gemm_nt(Z, W[f"cnn.cnn.cg{i}.linear.weight"].w, EPI_F32, bias=aux["gbias"], outF=L)
            ph, pw = m.cnn_pooling[i]
            Xn = None if pl.last else E(B, pl.Ho, pl.Wo, pl.Cpo, dt=ACT)
            if pl.last:
                feat = E(B * pl.Ho * pl.Wo, co)
            mask = None
            scale = 1.0
            if train and m.conv_dropout > 0:
                mask = drop_masks[i] if drop_masks is not None else gen_masks[i].view(Mi, co)
                scale = 1.0 / (1.0 - m.conv_dropout)
            if pl.fused16:
                # 16 filters: z = Y a + b, l = W_g z + b_g (fp32, 256 FMAs per pixel), gate, dropout and pooling in one pass over Y; the
                # backward's operands -- the logits and the 16-column 16-bit image of z -- are side outputs of a saving pass
                if save:
                    L, Z = E(Mi, 16), E(Mi, 16, dt=ACT)
                call("sed_cg_gate16_pool", Y, ldy, a, b, self.P(f"cnn.cnn.cg{i}.linear.weight").detach(), self.P(f"cnn.cnn.cg{i}.linear.bias").detach(),
                     mask, float(scale), L, Z, Xn, feat, B, Hc, Wc, pl.Cpo, ph, pw, 1)
            else:
                call("sed_cg_pool", Y, ldy, a, b, L, ldy, mask, float(scale), Xn, feat, B, Hc, Wc, co, pl.Cpo, ph, pw, 1)
            if save:
                layers.append(dict(col=col, mel=mel if pl.direct0 else None, Y=Y, a=a, b=b, ah=ah, bh=bh, Z=Z, L=L, mask=mask, scale=scale,
                                   dyn=dynctx if aux["dyn"] else None))
            X = Xn
        return feat, dict(layers=layers, Tc=plans[-1].Ho, plans=plans)

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

    def _fdy_mix_bwd(self, W, i, aux, pl, L, dY16, B, G, slots):
        """Backward of `_fdy_mix_fwd` from dY (bf16 [pixels, ldo]): the weight gradient of the four basis kernels into its slot, the input
        gradient through the patch matrix, the attention head's parameter gradients, and the head's path into the input gradient."""
        dev = dY16.device
        co, cin, hid, ld4, ldg4, Kp = aux["co"], aux["cin"], aux["hid"], aux["ld4"], aux["ldg4"], aux["Kp"]
        Hc, Wc, D = pl.H, pl.W, L["dyn"]
        R, Mi = B * Hc, pl.M
        E = empty(dev)
        pre = f"cnn.cnn.conv{i}.attention."
        dY4, da = E(Mi, ldg4, dt=BF16), E(R, 4)
        call("sed_fdy_mix_bwd", dY16, dY16.shape[1], D["Y4"], ld4, D["att"], dY4, ldg4, da, R, Wc, co)
        self._dw_swapped(dY4, L["col"], Mi, 4 * co, 9 * cin, out=(slots[("conv", i)], slots[("conv_b", i)]), image=pl.conv)
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

    def _cnn_bwd(self, W, cctx, dfeat, B, G, slots):
        m = self.m
        dev = dfeat.device
        E = empty(dev)
        dout = dfeat
        plans = cctx["plans"]
        if slots.get("cnn_plans") is not plans:
            raise RuntimeError("gradient-image slots were laid out for another shape or dw_tn than this forward's layer plans")
        for i in range(len(self.cnn_aux) - 1, -1, -1):
            aux, pl, L = self.cnn_aux[i], plans[i], cctx["layers"][i]
            co, Np, Kp, cin = aux["co"], aux["Np"], aux["Kp"], aux["cin"]
            Hc, Wc, Mi, ldy = pl.H, pl.W, pl.M, pl.ldy
            ph, pw = m.cnn_pooling[i]
            ldg = aux["ldg"]       # row width of the bf16 gradient operands: 64 columns hold the 16 / 32 / 64 filters (128 until round 4)
            dz = E(Mi, ldy)
            if pl.fused16:      # the forward ran `sed_cg_gate16_pool`: its backward carries the gate Linear too
                dL16 = E(Mi, 16, dt=BF16)
                call("sed_cg_gate16_pool_bwd", dout, L["Y"], ldy, L["a"], L["b"], L["L"], self.P(f"cnn.cnn.cg{i}.linear.weight").detach(), L["mask"],
                     float(L["scale"]), dz, dL16, B, Hc, Wc, ph, pw, L["ah"], L["bh"], slots[("bn_s1", i)], slots[("bn_s2", i)])
            else:
                dL16 = E(Mi, ldg, dt=BF16)
                call("sed_cg_pool_bwd", dout, L["Y"], ldy, L["a"], L["b"], L["L"], ldy, L["mask"], float(L["scale"]), dz, ldy, dL16, ldg, B, Hc,
                     Wc, co, ph, pw)
            # weight / bias gradient images land in the zeroed slots; `sed_scatter_add_f32` returns them to the masters after the loop
            self._dw_swapped(dL16, L["Z"], Mi, co, co, out=(slots[("gate", i)], slots[("gate_b", i)]), image=pl.gate)
            if pl.fused16:
                pass              # (dz is already complete)
            elif ldy < Np:      # dz += dL W_gate
                gemm_nt_cols(dL16, aux["wtg"], EPI_F32_RESID, co, res=dz, outF=dz)
            else:
                gemm_nt(dL16, aux["wtg"], EPI_F32_RESID, res=dz, outF=dz)
            s1, s2 = slots[("bn_s1", i)], slots[("bn_s2", i)]
            if not pl.fused16:      # (the fused backward accumulated the BatchNorm backward sums itself)
                call("sed_colstats", dz, ldy, L["Y"], ldy, L["ah"], L["bh"], s1, s2, Mi, co, 1)
            bn = f"cnn.cnn.batchnorm{i}."
            ldyo = pl.ldyo
            dY16 = E(Mi, ldyo, dt=BF16)
            call("sed_bn_bwd", dz, ldy, L["Y"], ldy, L["ah"], L["bh"], self.P(bn + "weight"), s1, s2, dY16, ldyo, Mi, co)
            del dz, dL16
            if aux["dyn"]:
                pass              # (the weight gradient of the four basis kernels takes a (x) dY: `_fdy_mix_bwd` below)
            elif pl.direct0:      # direct first convolution: the patches come from the spectrogram again; [ldg, Kp] image as the TN kernel's
                call("sed_conv0_dw16", dY16, ldyo, L["mel"], slots[("conv", i)], Kp, slots[("conv_b", i)], B, Hc)
            else:
                self._dw_swapped(dY16, L["col"], Mi, co, 9 * cin, out=(slots[("conv", i)], slots[("conv_b", i)]), image=pl.conv)
            cv = f"cnn.cnn.conv{i}."
            if aux["dyn"]:
                dout = self._fdy_mix_bwd(W, i, aux, pl, L, dY16, B, G, slots)
            elif i > 0:
                dcol = E(Mi, Kp, dt=BF16)
                gemm_nt(dY16, W[cv + "weight"].wt, EPI_BF16, outH=dcol, K=ldg)      # (the first ldg of the transposed image's Np columns)
                dout = E(B, Hc, Wc, cin)
                call("sed_col2im3x3", dcol, Kp, dout, B, Hc, Wc, cin)
            cctx["layers"][i] = None
