"""The PaSST encoder of the engine: forward (every form of its linear sites), backward walk, sliding windows, and the two views of
"which blocks does a backward reach"."""
import torch

from ..ops import BF16, F16, F32, call, h2d, gemm_nt, pad64, is_f16, gemm_nt_w2f8
from ..ops import EPI_F32, EPI_F32_RESID, EPI_GELU
from . import ACT, D, H, empty, stats


def window_starts(n_in=1000, win=512, step=49):
    """src/models/encoder_slide_window.py:27."""
    return list(range(0, n_in + step - win, step))


class Encoder:
    def _encoder_fwd(self, W, mel, tstarts, tp, toffsets, save, want_frame, rows=None, F=12):
        """PaSST encoder on `len(tstarts)` slabs of every clip (slabs folded into the batch, slab-major).
        mel [B,128,T]; returns pooled [nS*B, tp, D] (f_pool of layer `feature_layer`), frame16 (final norm), ctx.
        `rows`: per slab the device int32 [F] kept frequency rows of structured patchout (None: all 12); the sequence is then
        N = 2 + F tp tokens from the im2col on -- every kernel below takes N."""
        m = self.m
        dev = mel.device
        B, _, T = mel.shape
        nS = len(tstarts)
        Bx = nS * B
        N = 2 + F * tp
        Npad = pad64(N)
        M = Bx * N
        E = empty(dev)
        rows = [None] * nS if rows is None else rows
        ctx = dict(B=Bx, N=N, Npad=Npad, tp=tp, layers=[], toffsets=toffsets, nS=nS, F=F, rows=rows)
        Ms = B * F * tp             # patch rows of one slab
        cols = E(nS * Ms, 256, dt=ACT)
        for s, ts in enumerate(tstarts):
            call("sed_im2col_rows", mel, cols[s * Ms:(s + 1) * Ms], rows[s], F, B, T, ts, tp, 1)
        conv = E(nS * Ms, D)
        gemm_nt(cols, W["backbone.patch_embed.proj.weight"].w, EPI_F32, bias=self.P("backbone.patch_embed.proj.bias"), outF=conv)
        x = E(Bx, N, D)
        fpe = self.P("backbone.freq_new_pos_embed").reshape(D, 12)
        tpe = self.P("backbone.time_new_pos_embed").reshape(D, 99)
        for s in range(nS):
            call("sed_assemble_tokens_rows", conv[s * Ms:(s + 1) * Ms], self.P("backbone.cls_token"),
                 self.P("backbone.dist_token"), self.P("backbone.new_pos_embed"), fpe, tpe, rows[s], F, int(toffsets[s]),
                 x[s * B:(s + 1) * B], B, tp)
        if save:
            ctx["cols"] = cols
        # Blocks below the lowest one with a trainable tensor are never walked by the backward (frozen encoder of the pretrain / finetune1
        # stages, `freeze_layer`): they run like a no-grad pass -- nothing saved, in place, LayerNorms folded -- even inside a pass that saves.
        lo_f = self._lowest_trainable_fwd(m.depth) if save else m.depth
        # q, k, v stay row-major: the attention forward and backward take every transposed operand out of their LDS tiles
        # (ds_read_b64_tr_b16); the backward makes the bf16 images of the saved f16 Q / K / V tiles on the way into LDS
        scratch = None          # per-call scratch (reused across layers when not saving)
        pooled = None
        # Form of each linear site in this pass (the constructor's comment on the evaluation-mode encoder): "f16" plain weights (training,
        # saving blocks, N < 128), "gb" f16 weights + the per-clip mean correction, "w2" two-term weights, "w2f8" two-term weights with the
        # lo product on the fp8 path.  fc1 never goes beyond gb; inputs below the 256^2 kernel's domain (M < 1024) run gb everywhere.
        wc = self._wcorr_on(save) and N >= 128
        w2 = wc and M >= 1024
        w2f8 = w2 and self.w2_f8

        def form_of(site):
            if not wc:
                return "f16"
            if not w2 or site == "fc1":
                return "gb"
            return "w2f8" if w2f8 and site in self.w2_f8_set else "w2"
        f_qkv, f_proj, f_fc1, f_fc2 = form_of("qkv"), form_of("proj"), form_of("fc1"), form_of("fc2")
        # the operand rows of a w2f8 GEMM are [f16 | e4m3], written by the producing kernel -- pitch 3 D / 2
        q8, p8, f28 = f_qkv == "w2f8", f_proj == "w2f8", f_fc2 == "w2f8"
        pitch = lambda on: D + D // 2 if on else D

        def linear(p, site, form, xin, epi=None, K=D, qkv=None, **out):
            """The qkv / proj / fc1 / fc2 GEMM of block `p` in its form; `qkv`: the head-split (q, k, v) the qkv site writes instead of `out`"""
            wn, b = p + site + ".weight", self.P(p + site + ".bias")
            heads = (M, D, H, N, Npad, *qkv) if qkv else None
            if form == "w2f8":
                img, s = self._w2f8_image(W, wn)
                return call("sed_gemm_qkv_w2f8", xin, img, b, *heads, s) if qkv else gemm_nt_w2f8(xin, img, s, epi, K, bias=b, **out)
            if form == "w2":
                img = self._w2_image(W, wn)
                return call("sed_gemm_qkv_w2", xin, img, b, *heads, 1) if qkv else gemm_nt(xin, img, epi, bias=b, two_term=True, **out)
            gb = self._wcorr_bias(W, wn, xin, Bx, N) if form == "gb" else None
            if not qkv:
                return gemm_nt(xin, W[wn].w, epi, bias=b, gbias=gb, gb_rows=N if form == "gb" else 0, **out)
            if form == "gb":
                return call("sed_gemm_qkv_gb", xin, W[wn].w, b, *heads, 1, gb, N)
            call("sed_gemm_qkv", xin, W[wn].w, b, *heads, None, None, None, None, None, None, None, 1)
        # No-grad f16 passes that are not scored (the teacher inside the train step, frozen encoders): LayerNorm folded into the GEMMs around
        # it -- the residual GEMM writes the f16 image of the new stream + per-row partial sums, the next GEMM consumes the RAW image against
        # gamma-scaled weights and normalises in its epilogue (csrc/gemm_args.h, GemmArgs.rowpart / rowstat).  Two passes over the stream less
        # per block.  SED_LN_FOLD=0 keeps the LayerNorm kernels.
        fold_ok = self.ln_fold and not wc and M >= 1024 and not getattr(m, "lora_r", 0) and (not save or lo_f > 0)
        have_stat = False       # statistics of the current stream available (false before the first residual GEMM)
        if fold_ok:
            # between folded blocks the residual stream lives as two planes (x16f = f16 hi, which is also the consumers' A operand, + xlo:
            # 8-bit lo) instead of fp32: a producer then moves 6 bytes per element instead of 10 (csrc/gemm_args.h, GemmArgs.res_lo / out_lo)
            # (slab-major planes are addressed through one 32-bit buffer range: a plane has to stay below 2 GiB -- M < 1.4 M tokens for the
            #  stream planes, M < 349 k for the fc1 activation; beyond that the f16 planes / the row-major activation)
            lo8 = M * D * 2 < 2 ** 31
            x16f, xlo, partf, statf = E(M, D, dt=F16), E(M, D, dt=torch.uint8 if lo8 else F16), E(M, D // 64, 2), E(M, 2)
            lnp = "sed_gemm_nt_lnp8" if lo8 else "sed_gemm_nt_lnp"      # (lnp8: both planes slab-major, read back by the *_lnc8 consumers)
            qkv_lnc, nt_lnc = ("sed_gemm_qkv_lnc8", "sed_gemm_nt_lnc8") if lo8 else ("sed_gemm_qkv_lnc", "sed_gemm_nt_lnc")
        planes = False              # the current stream value is in (x16f, xlo) rather than in the fp32 tensor
        for li in range(m.depth):
            p = f"backbone.blocks.{li}."
            sv = save and li >= lo_f          # this block's activations are read by a backward
            fold = fold_ok and not sv
            if sv or scratch is None:
                h16 = E(M, pitch(q8), dt=ACT)
                q, k, v = E(Bx * H, N, 64, dt=ACT), E(Bx * H, N, 64, dt=ACT), E(Bx * H, N, 64, dt=ACT)
                o16 = E(M, pitch(p8), dt=ACT)
                lse = E(Bx * H, N)
                h2 = E(M, D, dt=ACT)
                hpre = E(M, 4 * D, dt=BF16) if sv else None       # (GELU pre-activation: only the backward reads it, so bf16 right away)
                act = E(M, 4 * pitch(f28), dt=ACT)
                (mean1, rstd1), (mean2, rstd2) = stats(E, M, sv), stats(E, M, sv)
                scratch = (h16, q, k, v, o16, lse, h2, hpre, act)
            else:
                h16, q, k, v, o16, lse, h2, hpre, act = scratch
                mean1 = rstd1 = mean2 = rstd2 = None
            x_in = x
            # Saving blocks: the LayerNorm writes its result twice -- f16 for the forward GEMM, bf16 for the backward's weight
            # gradient, which otherwise converts the saved f16 fragments in registers (17-20 % of that launch).  The f16 tensors are not kept.
            dual = sv and not getattr(m, "lora_r", 0)      # (LoRA factors take their gradients from the f16 operand)
            h16s = h2s = None
            if dual:
                h16s, h2s = E(M, D, dt=BF16), E(M, D, dt=BF16)
                call("sed_layernorm_fwd_dual", x_in, self.P(p + "norm1.weight"), self.P(p + "norm1.bias"), 1e-6, 1.0, h16, h16s, mean1, rstd1, M, D)
            elif not (fold and have_stat):
                call("sed_layernorm_fwd", x_in, self.P(p + "norm1.weight"), self.P(p + "norm1.bias"), 1e-6, 1.0, h16, None,
                     mean1, rstd1, M, D, 8 if q8 else 1)
            if fold:
                last = li + 1 == m.depth or (li + 1 == m.passt_feature_layer and not want_frame) or (save and li + 1 >= lo_f)
                if have_stat:
                    wf, sq, cq = self._lnf_image(W, p + "attn.qkv.weight", p + "attn.qkv.bias", p + "norm1.weight", p + "norm1.bias")
                    call(qkv_lnc, x16f, wf, cq, sq, statf, M, D, H, N, Npad, q, k, v)
                else:       # first block: its LayerNorm ran above (the stream comes from the token assembly, not from a GEMM)
                    linear(p, "attn.qkv", "f16", h16, qkv=(q, k, v))
                # (byte-plane runs: the attention output goes head-major = slab-major into the proj GEMM's A operand)
                call("sed_mhsa_fwd", q, k, v, o16, lse, Bx, H, N, Npad, 1 | (2 if lo8 else 0))
                call(lnp, o16, W[p + "attn.proj.weight"].w, M, D, D, 64 if lo8 else D, D, self.P(p + "attn.proj.bias"),
                     None if planes else x_in, x16f if planes else None, xlo if planes else None, None, x16f, xlo, partf, D)
                call("sed_ln_fold_stats", partf, statf, M, D // 64, D, 1e-6)
                w1, s1, c1 = self._lnf_image(W, p + "mlp.fc1.weight", p + "mlp.fc1.bias", p + "norm2.weight", p + "norm2.bias")
                # (byte-plane runs: the fc1 activation goes slab-major from fc1's epilogue into fc2's A operand -- ldc / lda = 64)
                slab_act = lo8 and M * 4 * D * 2 < 2 ** 31
                call(nt_lnc, x16f, w1, M, 4 * D, D, D, D, c1, s1, statf, act, 64 if slab_act else 4 * D)
                # the block's output has an fp32 reader (f_pool, the final norm, a saving block) -> fp32 out; otherwise it stays in planes
                f32_out = last or li + 1 == m.passt_feature_layer
                call(lnp, act, W[p + "mlp.fc2.weight"].w, M, D, 4 * D, 64 if slab_act else 4 * D, 4 * D, self.P(p + "mlp.fc2.bias"),
                     None, x16f, xlo, x_in if f32_out else None, x16f, None if f32_out else xlo, partf, D)
                planes = not f32_out
                if not last:
                    call("sed_ln_fold_stats", partf, statf, M, D // 64, D, 1e-6)
                    have_stat = True
                x_out = x_in
            else:
                linear(p, "attn.qkv", f_qkv, h16, qkv=(q, k, v))
                call("sed_mhsa_fwd", q, k, v, o16, lse, Bx, H, N, Npad, 1 | (4 if p8 else 0))
                x_mid = E(Bx, N, D) if sv else x_in
                linear(p, "attn.proj", f_proj, o16, EPI_F32_RESID, D, res=x_in, outF=x_mid)
                if dual:
                    call("sed_layernorm_fwd_dual", x_mid, self.P(p + "norm2.weight"), self.P(p + "norm2.bias"), 1e-6, 1.0, h2, h2s, mean2, rstd2, M, D)
                else:
                    call("sed_layernorm_fwd", x_mid, self.P(p + "norm2.weight"), self.P(p + "norm2.bias"), 1e-6, 1.0, h2, None, mean2, rstd2, M, D, 1)
                if f28:     # fc1's gb form whose epilogue also writes the e4m3 image of the activation beside it, for fc2's lo product
                    call("sed_gemm_nt_gb_e4m3", h2, W[p + "mlp.fc1.weight"].w, M, 4 * D, D, D, D, self.P(p + "mlp.fc1.bias"), act, 4 * pitch(f28),
                         self._wcorr_bias(W, p + "mlp.fc1.weight", h2, Bx, N), N)
                else:
                    linear(p, "mlp.fc1", f_fc1, h2, EPI_GELU, D, outH=hpre, outH2=act)
                x_out = E(Bx, N, D) if sv else x_mid
                linear(p, "mlp.fc2", f_fc2, act, EPI_F32_RESID, 4 * D, res=x_mid, outF=x_out)
            if sv:
                ctx["layers"].append(dict(x_in=x_in, h16=h16s if dual else h16, q=q, k=k, v=v, o16=o16, lse=lse, x_mid=x_mid,
                                          h2=h2s if dual else h2, hpre=hpre, act=act, mean1=mean1, rstd1=rstd1, mean2=mean2, rstd2=rstd2))
            elif save:
                ctx["layers"].append(None)      # (a frozen block below the lowest trainable one: index kept, nothing saved)
            x = x_out
            if li + 1 == m.passt_feature_layer:
                pooled = self._fpool_fwd(W, x, Bx, tp, save, ctx)
                if not want_frame:
                    break  # later blocks only feed the AT head (`frame`); windows never need them
                if save and (fold or li + 1 < lo_f):
                    x = x.clone()       # f_pool's backward reads the tensor it was given; the in-place blocks that follow must not touch it
        frame16 = None
        if want_frame:
            frame16 = E(M, D, dt=ACT)
            fm, fr = stats(E, M, save)
            # (DASM's head reads the tokens in fp32: the same pass writes them beside the 16-bit image)
            self._frame32 = E(M, D) if getattr(m, "dasm_head", None) is not None else None
            call("sed_layernorm_fwd", x, self.P("backbone.norm.weight"), self.P("backbone.norm.bias"), 1e-6, 1.0, frame16, self._frame32, fm, fr, M, D, 1)
            if save:
                ctx.update(x_final=x, fmean=fm, frstd=fr, frame16=frame16)
        return pooled, frame16, ctx

    def _window_features(self, W, mel, xg, Tdec, opt, save):
        """Sliding windows (encoder_slide_window.py): the encoder on every window, the windows' features mixed into the 768-wide global
        sequence `xg` [B, Tdec, D] in place.  Returns what the backward needs (None unless `save`)."""
        dev = mel.device
        B, _, T = mel.shape
        win, step = opt["win"]["param"]
        toffsets, rows_dev = opt["win"]["toffsets"], opt["rows_dev"]
        starts = window_starts(T, win, step)
        if toffsets is None:
            toffsets = [0] * len(starts)
        # group the windows by their number of time patches (the last slab of a sweep can be shorter:
        # min(left + win, T) - left frames, encoder_slide_window.py:28) and fold each group into the batch
        groups = {}
        for wi, left in enumerate(starts):
            width = min(left + win, T) - left
            groups.setdefault((width - 16) // 10 + 1, []).append(wi)
        lefts, tps, offs, chunks, row = [0] * len(starts), [0] * len(starts), [0] * len(starts), [], 0
        wgroups = []
        for tpw, wis in groups.items():
            pw, _, gctx = self._encoder_fwd(W, mel, [starts[w] for w in wis], tpw, [toffsets[w] for w in wis], save, want_frame=False,
                                            rows=None if rows_dev is None else [rows_dev[1 + w] for w in wis], F=opt["F"])
            chunks.append(pw.view(-1, D))
            wgroups.append(dict(ectx=gctx, row0=row, rows=len(wis) * B * tpw))
            for k, w in enumerate(wis):
                lefts[w], tps[w], offs[w] = round(starts[w] * (Tdec / T)), tpw, row + k * B * tpw
            row += len(wis) * B * tpw
        packed = chunks[0] if len(chunks) == 1 else torch.cat(chunks, 0)
        wl, wt, wo = h2d([lefts, tps, offs], torch.int32, dev)       # one upload for the three window tables
        call("sed_window_mix", packed, wl, wt, wo, len(starts), xg, opt["win"]["mix"], B, Tdec, self.m.decode_ratio)
        if not save:
            return None
        return dict(groups=wgroups, lefts=wl, tps=wt, offs=wo, n=len(starts), mix=opt["win"]["mix"], rows=row)

    _BELOW_HEADS = ("decoder.", "out_norm.", "mask_token", "f_pool_module.")

    def _walks_decoder_fwd(self):
        """Will a backward have to pass through the context network?  Yes when one of its own tensors trains, or anything under it: the
        f_pool normalisation, the MLM mask token, an encoder block, the patch embedding (requires_grad flags; `_walks_decoder` is the
        backward's twin on gradient views)."""
        pbn = self.m._param_by_name
        inert = getattr(self.m, "_inert_param_names", ())
        if any(p_.requires_grad for n, p_ in pbn.items() if n.startswith(self._BELOW_HEADS) and n not in inert):
            return True
        return self._lowest_trainable_fwd(self.m.depth) < self.m.depth

    def _walks_decoder(self, G, depth):
        names = [n for n in self.m._param_by_name if n.startswith(self._BELOW_HEADS)]
        if any(G(n) is not None for n in names):
            return True
        lo, embed = self._lowest_trainable(G, depth)
        return embed or lo < depth

    def _lowest_trainable_fwd(self, depth):
        """The forward's view of `_lowest_trainable` (requires_grad flags instead of gradient views): index of the first encoder block
        whose activations a backward can need -- 0 when the patch embedding / position tables train, `depth` when nothing below the
        pooling does."""
        pbn = self.m._param_by_name
        inert = getattr(self.m, "_inert_param_names", ())      # (lr-0 groups: FusedAdamWEMA; no gradient is computed for them)
        cache = getattr(self, "_blk_params", None)
        if cache is None or cache[0] is not pbn or cache[3] is not inert:
            embed = [p_ for n, p_ in pbn.items() if n.startswith("backbone.") and not n.startswith("backbone.blocks.") and
                     not n.startswith("backbone.norm.") and not n.startswith("backbone.head") and n not in inert]
            blocks = [[p_ for n, p_ in pbn.items() if n.startswith(f"backbone.blocks.{i}.") and n not in inert] for i in range(depth)]
            cache = self._blk_params = (pbn, embed, blocks, inert)
        if any(p_.requires_grad for p_ in cache[1]):
            return 0
        for i, ps in enumerate(cache[2][:depth]):
            if any(p_.requires_grad for p_ in ps):
                return i
        return depth

    def _lowest_trainable(self, G, depth):
        """(index of the lowest encoder block a backward has to reach -- `depth` if none --, does the patch embedding train): decided
        once per backward (`_scan_lowest_trainable`), then read by every stage that asks."""
        key = (id(G), depth)
        hit = getattr(self, "_lo_cache", None)
        if hit is not None and hit[0] == key:
            return hit[1]
        res = self._scan_lowest_trainable(G, depth)
        self._lo_cache = (key, res, G)      # (G kept alive so that its id cannot be recycled while cached)
        return res

    def _scan_lowest_trainable(self, G, depth):
        """From the gradient views: the lowest block with a trainable tensor; 0 when the patch embedding / position tables train
        (recipes/desed/finetune/passt/setting.py:44-60 freezes everything below `freeze_layer` except the final norm)."""
        embed = ("backbone.patch_embed.proj.weight", "backbone.patch_embed.proj.bias", "backbone.cls_token", "backbone.dist_token",
                 "backbone.new_pos_embed", "backbone.freq_new_pos_embed", "backbone.time_new_pos_embed")
        block = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "norm2.weight",
                 "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")
        if any(G(n) is not None for n in embed):           # ANY tensor of a stage makes the stage (and everything above it) run
            return 0, True
        for i in range(depth):
            if any(G(f"backbone.blocks.{i}.{t}") is not None for t in block):
                return i, False
        return depth, False

    _embed_stage_always = False     # fire the "embed" stage hook after every walk of the stack, whether or not the embedding trains

    def _encoder_bwd(self, W, ectx, genc, dpooled, G, hook):
        """Backward of one encoder pass (the global one, or a group of sliding windows folded into the batch): f_pool at the tapped
        layer, the blocks from the top saved one down to the lowest trainable one, then the patch embedding.  `genc` is the gradient
        arriving at the top of the stack (AT head) or None; gradients accumulate into the arena views.  Overridable pieces:
        `_fpool_bwd`, `_enc_layer_bwd` (where a block's weight gradients go), `_scan_lowest_trainable`."""
        m = self.m
        B, N, tp, F = ectx["B"], ectx["N"], ectx["tp"], ectx["F"]
        dev = dpooled.device
        depth = len(ectx["layers"])
        lo, embed_train = self._lowest_trainable(G, depth)
        tap = m.passt_feature_layer - 1                      # f_pool reads the output of block `tap`
        gpool = self._fpool_bwd(W, ectx, dpooled, G, need_dx=lo <= tap)
        if hook is not None:
            hook("heads")  # AT head, out_norm (and backbone.norm) gradients are final
        if lo >= depth:
            return
        if genc is None:
            genc = torch.zeros(B, N, D, dtype=F32, device=dev)
        for li in range(depth - 1, lo - 1, -1):
            if li == tap:
                genc.add_(gpool)
            genc = self._enc_layer_bwd(W, ectx, li, genc, G)
            if hook is not None:
                hook(("block", li))
        if embed_train:
            # patch embedding + positional tables (one slab of the batch per window / time offset)
            nS = ectx["nS"]
            Bs = B // nS
            Ms = Bs * F * tp
            Mp = nS * Ms
            dconv16 = torch.empty(Mp, D, dtype=BF16, device=dev)
            for sidx in range(nS):
                call("sed_assemble_tokens_rows_bwd", genc[sidx * Bs:(sidx + 1) * Bs], dconv16[sidx * Ms:(sidx + 1) * Ms],
                     G("backbone.cls_token"), G("backbone.dist_token"), G("backbone.new_pos_embed"), G("backbone.freq_new_pos_embed"),
                     G("backbone.time_new_pos_embed"), ectx["rows"][sidx], F, int(ectx["toffsets"][sidx]), Bs, tp)
            self._dw_accum(dconv16, ectx["cols"], Mp, G("backbone.patch_embed.proj.weight"), G("backbone.patch_embed.proj.bias"))
        if hook is not None and (embed_train or self._embed_stage_always):
            hook("embed")

    def _enc_layer_bwd(self, W, ectx, li, g, G):
        """Backward of encoder block `li` on the stream gradient g [B, N, D] in place (`_preln_block_bwd`).  Its LayerNorm backwards
        leave the bf16 image of the gradient they just updated: the dY operand of the next weight-gradient / dX GEMMs (no cast pass over the
        fp32 stream; the bias gradient comes out of the TN kernel) -- the one of LN1 goes to the block below through `_genc16`."""
        L = ectx["layers"][li]
        B, N, Npad = ectx["B"], ectx["N"], ectx["Npad"]

        def attn_bwd(do16, dqkv):
            Dtmp = torch.empty(B * H, N, dtype=F32, device=g.device)
            call("sed_mhsa_bwd", L["q"], L["k"], L["v"], L["o16"], do16, L["lse"], Dtmp, None, dqkv, B, H, N, Npad, is_f16(L["q"]), is_f16(L["v"]))
        gout16 = self._preln_block_bwd(W, f"backbone.blocks.{li}.", L, g.view(B * N, D), G, attn_bwd, x16=self.dw_tn, dy16=self._g16_take(g))
        if gout16 is not None:
            self._genc16 = (g, gout16, g._version)      # for the block below (`_g16_take`)
        ectx["layers"][li] = None  # free saved activations
        return g
