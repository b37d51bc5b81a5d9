"""Forward/backward engine of the MI355X-native MAT-SED model.

This is the host-side orchestration of the HIP kernels behind `PaSST_SED.forward`
(reference: src/models/passt/passt_sed.py:242-296 and everything it calls).  It owns
  * the bf16 operand copies of all GEMM weights (straight [out,in] and transposed [in,out]),
  * the explicit forward schedule (saving exactly what the hand-written backward needs),
  * the explicit backward schedule writing into ONE flat fp32 gradient arena (views of which become `p.grad`,
    and which the data-parallel layer all-reduces in buckets, see ddp.py).
There is no autograd tape inside: `_SedFunction` in passt_sed.py exposes the whole model as a single
autograd node so that the reference's training loops (loss via torch ops, loss.backward()) keep working.
"""
import contextlib
import math

import torch
from torch.optim.optimizer import register_optimizer_step_post_hook

from . import ops
import os

from .ops import BF16, F16, F32, call, h2d, gemm_nt, gemm_dw, gemm_dw_tn, dw_tn_ok, pad64, transpose_bf16, to_bf16_, is_f16, split3, o_kind, two_term_weight
from .ops import two_term_weight_f8, gemm_nt_w2f8
from .ops import EPI_F32, EPI_F32_RESID, EPI_BF16, EPI_GELU, EPI_DGELU, EPI_F32_BF16, EPI_GELU32

D = 768
H = 12
# 16-bit type of the FORWARD MFMA operands (activations + weight images).  IEEE half keeps the frame posteriors within 1e-3 of the fp32
# reference at the bf16 MFMA rate; gradient-side operands are always bf16.  (A bf16 forward misses that bound, so it is not a mode; the
# kernels stay templated on the type -- the `f16` / `mode` arguments the host passes as constants -- and the kernel tests exercise both.)
ACT = F16
NCLS_MAX = 16
FPOOL_TRANSFORMER = "frequency_wise_tranformer_encoder"     # f_pool value of the frequency-wise transformer pooling ((sic) the reference's spelling)
FPOOL_HEADS = 4         # its blocks: 4 heads of 192 (src/models/pooling.py:24)
WCORR_STEP = 8      # `_wcorr_bias`: clip means from every 8th token (1/8 of the extra read)


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


def band_half_width(model, dev, T):
    """The context network's local window (PaSST_SED(decoder_win_len=...)) as the band kernels take it: int32 [H] on `dev`, made once
    per device; None without a window.  The reference's mask has side decoder_pos_emd_len and fails at any other length."""
    dec = model.decoder
    if dec.half_widths is None:
        return None
    if T != dec.seq_len:
        raise RuntimeError(f"decoder_win_len: the attention mask has side {dec.seq_len} (decoder_pos_emd_len), the sequence has {T} frames")
    return dec.half_width_tensor(dev)


def window_starts(n_in=1000, win=512, step=49):
    """src/models/encoder_slide_window.py:27."""
    return list(range(0, n_in + step - win, step))


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


class _W:
    """bf16 operand images of one fp32 weight matrix [n_out, k_in] (rewritten by every forward), and the images cached across forwards
    (`cached_image`): LayerNorm-folded `lnf`, two-term `w2` (f16 or fp8 form), residual `wlo`, each beside its key."""
    __slots__ = ("w", "wt", "ws", "wlo", "wlo_key", "w2", "w2_key", "lnf", "lnf_key")

    def __init__(self, w, wt):
        self.w, self.wt, self.ws = w, wt, None
        self.wlo = self.wlo_key = self.w2 = self.w2_key = self.lnf = self.lnf_key = None


class _PoolLease:
    """Held by the saved-activation context of one forward: while it lives, the engine's pooled zero-padded buffers belong to that
    context (a second forward before the backward gets fresh allocations instead)."""

    def __init__(self, eng):
        self.eng = eng

    def __del__(self):
        self.eng._pool_busy = False


class SedEngine:
    def __init__(self, module):
        self.m = module
        self.dev = None
        self.cache = {}
        self.pos_cache = {}
        # zero-PADDED scratch / saved tensors (transposed q, k, v images, dS^T): the kernels only ever write the valid region, so the
        # padding written once stays zero and the buffers can be reused step after step instead of being re-zeroed (1.1 ms / step)
        self._zpool = {}
        self._pool_busy = False
        # The context-network (and MLM head) GEMMs always run in split precision: f16 hi + f16 lo operands, three MFMA products via the
        # concatenated reduction dim.  Their operand rounding is what limits posterior parity: with
        # it 1e-3 holds with a 10x margin, for ~4 % of step time; without it the posteriors miss 1e-3.
        # weight gradients: TN kernel on the operands as they lie (default) or transposed copies + NT split-K kernel
        self.dw_tn = True                 # (attribute kept for tools/trajectory_probe.py's summation-order experiment; no environment switch)
        # weight-gradient (TN) GEMMs on a side stream: they depend only on dY and the saved operand, nothing in the backward chain
        # reads their result, so they fill the partially occupied last rounds of the dX GEMMs and run under the HBM-bound
        # LayerNorm / cast passes.  Joined before every stage hook and at the end of backward.  Off while the kernel timer
        # instruments a step (interleaved kernels inflate every per-launch duration).
        self.dw_side = os.environ.get("SED_DW_STREAM", "1") != "0"
        # No-grad passes that are not scored run their LayerNorms folded into the GEMMs around them (`_encoder_fwd`); between folded
        # blocks the residual stream lives as two planes, f16 hi + 8-bit lo (6 bytes per element through a producer, the stream to ~2^-19).
        # SED_LN_FOLD=0 keeps the LayerNorm kernels.
        self.ln_fold = os.environ.get("SED_LN_FOLD", "1") != "0"
        # Context-network GEMMs that do not need all three split-precision terms (tools/err_sim.py SIM_DEC_TERMS=1: logit error of the whole
        # decoder 3.96e-4 with three terms everywhere): in_proj without the activation's lo part (5.4e-4; the weight's lo part is the one that
        # matters there: 1.9e-3 without it) -> two K passes instead of three on the largest decoder GEMM, and its LayerNorm writes a plain f16
        # image; linear_pos on plain f16 operands (5.3e-4).  out_proj / fc1 / fc2 keep three terms.
        self.dec_terms2 = True
        self._genc16 = None
        self._dw_stream = None
        self._dw_pending = False
        # Evaluation-mode encoder.  The f16 weight images are the largest single term of the posterior error (tools/err_sim.py: logit
        # error 1.6e-3 of 2.0e-3 in total), so passes whose posteriors are SCORED (module in eval mode: validation, test, inference)
        # do not round the weights; training-mode passes (student, and the teacher inside the train step) never pay for it.  Per GEMM:
        #   w2    two-term weights [f16(W) | f16(W - f16(W))], the activation panel walked twice (sed_gemm_*_w2): the fp32 weight to ~2^-19
        #         for twice the GEMM work -- qkv, proj and fc2;
        #   gb    f16 weights + mean_t(x) . (W - f16(W))^T per clip as a row-group bias (`_wcorr_bias`): the part of the rounding that is
        #         common to all tokens of a clip, ~2 % of an inference pass, about a third of the gain -- fc1 (the weight whose rounding
        #         matters least, and a third of the encoder's GEMM work), and every GEMM of an input below the 256^2 kernel's domain.
        # The lo product of w2, x . (W - f16(W))^T, is 2^-12 of the result: it can run on the fp8 matrix path (w2f8: e4m3 images of both
        # factors, v_mfma_scale_f32_16x16x128_f8f6f4: half of an f16 K pass; csrc/gemm_args.h GemmArgs.k8).  The activations' e4m3 images come
        # out of the producing kernels (LayerNorm, attention, fc1's epilogue) in the same rows as the f16 values.  e4m3 keeps ~5 % of the lo
        # product as error, which is not free here (every posterior of the validation configuration sits within 15 % of its bound), so the
        # default takes only the GEMM that pays for it with margin to spare on both fixtures: fc2 (DESIGN.md section 2 has the measured
        # speed and error of every subset; qkv is opt-in because e4m3 flushes |x| / 4 < 2^-9 and clamps at 1792 -- a checkpoint with louder
        # channels than the synthetic weights can cross the bound unseen).
        # SED_ENC_W2=f16: both products in f16; f8:<subset of qkv,proj,fc2>: that subset on the fp8 path.
        mode = os.environ.get("SED_ENC_W2", "f8")
        head, _, which = mode.partition(":")
        self.w2_f8_set = frozenset(w for w in (which.split(",") if which else ("fc2",)) if w)
        if head not in ("f8", "f16") or (head == "f16" and which) or not self.w2_f8_set <= {"qkv", "proj", "fc2"}:
            raise ValueError(f"SED_ENC_W2={mode!r}: expected f16, f8, or f8:<subset of qkv,proj,fc2>")
        self.w2_f8 = head == "f8"

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
            call("sed_ln_fold_weight", w.detach().reshape(n_out, k_in).contiguous(), g.detach(), bt.detach(), b.detach(),
                 w16, cs, cc, n_out, k_in)
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

    def __deepcopy__(self, memo):
        return None  # `ema_net = deepcopy(net)` (finetune/passt/setting.py:8-15): the copy rebuilds its engine lazily

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

    # ------------------------------------------------------------------ parameters
    def P(self, name):
        return self.m._param_by_name[name]

    def _weights(self, need_t):
        """(Re)build the 16-bit operand images of every GEMM weight from the fp32 masters: one `sed_weight_images` launch."""
        m = self.m
        names = ["backbone.patch_embed.proj.weight"]
        for i in range(m.depth):
            p = f"backbone.blocks.{i}."
            names += [p + "attn.qkv.weight", p + "attn.proj.weight", p + "mlp.fc1.weight", p + "mlp.fc2.weight"]
        for i in range(m.decoder_layer_num):
            if m.decoder_name == "conformer":       # (the 1-tap Conv1d weights [out, in, 1] are [out, in] matrices to the image kernel)
                p = f"decoder.blocks.{i}."
                names += [p + "self_attn.in_proj.weight", p + "self_attn.out_proj.weight", p + "self_attn.linear_pos.weight",
                          p + "feed_forward_macaron.0.weight", p + "feed_forward_macaron.3.weight",
                          p + "conv_module.pointwise_conv1.weight", p + "conv_module.pointwise_conv2.weight",
                          p + "feed_forward.0.weight", p + "feed_forward.3.weight"]
                continue
            p = f"decoder.encoder_blocks.{i}."
            names += [p + "attn.in_proj.weight", p + "attn.out_proj.weight", p + "attn.linear_pos.weight",
                      p + "mlp.fc1.weight", p + "mlp.fc2.weight"]
        if m.mlm:
            names += ["mlm_mlp.0.weight", "mlm_mlp.2.weight"]
        if m.has_at:
            names += ["at_adpater.0.frequency_att.in_proj_weight"]
        if m.f_pool_name == FPOOL_TRANSFORMER:
            for i in range(2):
                p = f"f_pool_module.frequency_transformer.{i}."
                names += [p + "attn.qkv.weight", p + "attn.proj.weight", p + "mlp.fc1.weight", p + "mlp.fc2.weight"]
        fp_split = self._fpool_split_on(need_t)         # (`need_t` is the forward's `save`)
        ptrs = tuple(self.P(n).data_ptr() for n in names) + (bool(need_t), fp_split)
        if getattr(self, "_wimg_key", None) != ptrs:
            # descriptor table of sed_weight_images: rebuilt only when a master moved (optimizer arenas, .to(device))
            rows, tiles = [], 0
            for n in names:
                w32 = self.P(n).detach()
                n_out = w32.shape[0]
                k_in = w32.numel() // n_out
                if not w32.is_contiguous() or n_out % 16 or k_in % 64:
                    raise RuntimeError(f"weight {n}: unsupported shape / layout for the operand images")
                ent = self.cache.get(n)
                if ent is None or ent.w.device != w32.device:
                    ent = _W(torch.empty(n_out, k_in, dtype=ACT, device=w32.device),
                             torch.empty(k_in, n_out, dtype=BF16, device=w32.device))
                    self.cache[n] = ent
                want_split = n.startswith(("decoder.", "mlm_mlp")) or (fp_split and n.startswith("f_pool_module."))
                if want_split and (ent.ws is None or ent.ws.device != w32.device):
                    ent.ws = torch.empty(n_out, 3 * k_in, dtype=F16, device=w32.device)
                rows.append([w32.data_ptr(), ent.wt.data_ptr() if need_t else 0, ent.w.data_ptr(), ent.ws.data_ptr() if want_split else 0,
                             n_out, k_in, 2, tiles, 0, 0, 0, 0, 0, 0, 0, 0])   # (no gather plan, no LoRA term)
                tiles += ((n_out + 63) // 64) * (k_in // 64)
            self._wimg_desc = h2d(rows, torch.int64, self.P(names[0]).device)
            self._wimg_n, self._wimg_tiles, self._wimg_key = len(rows), tiles, ptrs
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

    # ------------------------------------------------------------------ encoder
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
        E = lambda *s, dt=F32: torch.empty(*s, dtype=dt, device=dev)
        rows = [None] * nS if rows is None else rows
        ctx = dict(B=Bx, N=N, Npad=Npad, tp=tp, layers=[], toffsets=toffsets, nS=nS, F=F, rows=rows)
        Ms = B * F * tp             # patch rows of one slab
        cols = E(nS * Ms, 256, dt=ACT)
        for s, ts in enumerate(tstarts):
            call("sed_im2col_rows", mel, cols[s * Ms:(s + 1) * Ms], rows[s], F, B, T, ts, tp, 1)
        conv = E(nS * Ms, D)
        gemm_nt(cols, W["backbone.patch_embed.proj.weight"].w, EPI_F32, bias=self.P("backbone.patch_embed.proj.bias"),
                outF=conv)
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
        mk_qkv = lambda: [E(Bx * H, N, 64, dt=ACT), E(Bx * H, N, 64, dt=ACT), E(Bx * H, N, 64, dt=ACT)]
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

        def linear(p, site, form, xin, epi, K, **out):
            """The proj / fc1 / fc2 GEMM of block `p` in its form"""
            wn, b = p + site + ".weight", self.P(p + site + ".bias")
            if form == "w2f8":
                img, s = self._w2f8_image(W, wn)
                gemm_nt_w2f8(xin, img, s, epi, K, bias=b, **out)
            elif form == "w2":
                gemm_nt(xin, self._w2_image(W, wn), epi, bias=b, two_term=True, **out)
            elif form == "gb":
                gemm_nt(xin, W[wn].w, epi, bias=b, gbias=self._wcorr_bias(W, wn, xin, Bx, N), gb_rows=N, **out)
            else:
                gemm_nt(xin, W[wn].w, epi, bias=b, **out)
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
                q, k, v = mk_qkv()
                o16 = E(M, pitch(p8), dt=ACT)
                lse = E(Bx * H, N)
                h2 = E(M, D, dt=ACT)
                hpre = E(M, 4 * D, dt=BF16) if sv else None       # (GELU pre-activation: only the backward reads it, so bf16 right away)
                act = E(M, 4 * pitch(f28), dt=ACT)
                mean1, rstd1, mean2, rstd2 = (E(M), E(M), E(M), E(M)) if sv else (None, None, None, None)
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
            wq, bq = p + "attn.qkv.weight", self.P(p + "attn.qkv.bias")
            if fold:
                last = li + 1 == m.depth or (li + 1 == m.passt_feature_layer and not want_frame) or (save and li + 1 >= lo_f)
                if have_stat:
                    wf, sq, cq = self._lnf_image(W, wq, p + "attn.qkv.bias", p + "norm1.weight", p + "norm1.bias")
                    call(qkv_lnc, x16f, wf, cq, sq, statf, M, D, H, N, Npad, q, k, v)
                else:       # first block: its LayerNorm ran above (the stream comes from the token assembly, not from a GEMM)
                    call("sed_gemm_qkv", h16, W[wq].w, bq, M, D, H, N, Npad, q, k, v, None, None, None, None, None, None, None, 1)
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
                if f_qkv == "w2f8":
                    img, s = self._w2f8_image(W, wq)
                    call("sed_gemm_qkv_w2f8", h16, img, bq, M, D, H, N, Npad, q, k, v, s)
                elif f_qkv == "w2":
                    call("sed_gemm_qkv_w2", h16, self._w2_image(W, wq), bq, M, D, H, N, Npad, q, k, v, 1)
                elif f_qkv == "gb":
                    call("sed_gemm_qkv_gb", h16, W[wq].w, bq, M, D, H, N, Npad, q, k, v, 1, self._wcorr_bias(W, wq, h16, Bx, N), N)
                else:
                    call("sed_gemm_qkv", h16, W[wq].w, bq, M, D, H, N, Npad, q, k, v, None, None, None, None, None, None, None, 1)
                call("sed_mhsa_fwd", q, k, v, o16, lse, Bx, H, N, Npad, 1 | (4 if p8 else 0))
                x_mid = E(Bx, N, D) if sv else x_in
                linear(p, "attn.proj", f_proj, o16, EPI_F32_RESID, D, res=x_in, outF=x_mid)
                if dual:
                    call("sed_layernorm_fwd_dual", x_mid, self.P(p + "norm2.weight"), self.P(p + "norm2.bias"), 1e-6, 1.0, h2, h2s, mean2, rstd2, M, D)
                else:
                    call("sed_layernorm_fwd", x_mid, self.P(p + "norm2.weight"), self.P(p + "norm2.bias"), 1e-6, 1.0, h2, None,
                         mean2, rstd2, M, D, 1)
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
            fm, fr = (E(M), E(M)) if save else (None, None)
            # (DASM's head reads the tokens in fp32: the same pass writes them beside the 16-bit image)
            self._frame32 = E(M, D) if getattr(m, "dasm_head", None) is not None else None
            call("sed_layernorm_fwd", x, self.P("backbone.norm.weight"), self.P("backbone.norm.bias"), 1e-6, 1.0,
                 frame16, self._frame32, fm, fr, M, D, 1)
            if save:
                ctx.update(x_final=x, fmean=fm, frstd=fr, frame16=frame16)
        return pooled, frame16, ctx

    def _fpool_fwd(self, W, x, Bx, tp, save, ctx):
        """'mean_pool' frequency pooling (passt_sed.py:199-210): out_norm + mean over the frequency rows of the sequence (12, or the
        kept ones of structured patchout) -> [Bx, tp, D].  Other values of `f_pool` have a stage pair of their own."""
        if self.m.f_pool_name == FPOOL_TRANSFORMER:
            return self._fpool_tr_fwd(W, x, Bx, tp, save, ctx)
        dev = x.device
        F = ctx["F"]
        M = Bx * (2 + F * tp)
        pooled = torch.empty(Bx, tp, D, dtype=F32, device=dev)
        pm = torch.zeros(M, device=dev) if save else None
        pr = torch.zeros(M, device=dev) if save else None
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
        dev = x.device
        F = ctx["F"]
        N, S = 1 + F, Bx * tp
        M = S * N
        E = lambda *s, dt=F32: torch.empty(*s, dtype=dt, device=dev)
        SP = self._fpool_split_on(save)
        mode = 4 if SP else 1
        img = lambda k=D: E(M, 3 * k, dt=F16) if SP else E(M, k, dt=ACT)       # operand image of an [M, k] activation
        wk = (lambda n: W[n].ws) if SP else (lambda n: W[n].w)
        pre = "f_pool_module."
        cur = E(M, D)
        pm, pr = (E(M), E(M)) if save else (None, None)
        call("sed_fpool_seq_build_fwd", x, self.P("out_norm.weight"), self.P("out_norm.bias"), 1e-5, self.P(pre + "linear_emb.weight"),
             self.P(pre + "linear_emb.bias"), cur, pm, pr, Bx, tp, F)
        layers = []
        with (ops.split_precision() if SP else contextlib.nullcontext()):
            for i in range(2):
                p = f"{pre}frequency_transformer.{i}."
                stats = lambda: (E(M), E(M)) if save else (None, None)
                h16 = img()
                mean1, rstd1 = stats()
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
                mean2, rstd2 = stats()
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
        fm, fr = (E(S), E(S)) if save else (None, None)
        call("sed_fpool_rownorm_fwd", cur, self.P(pre + "frequency_transformer_norm.weight"), self.P(pre + "frequency_transformer_norm.bias"),
             1e-5, pooled, fm, fr, S, N)
        if save:
            ctx.update(pool_x=x, pool_mean=pm, pool_rstd=pr, pool_tr=dict(layers=layers, x_out=cur, fmean=fm, frstd=fr))
        return pooled

    # ------------------------------------------------------------------ context network
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
        call("sed_layernorm_fwd", x, self.P(norm + ".weight"), self.P(norm + ".bias"), 1e-5, scale, y16, y32, mean, rstd, M, Dm,
             1 if plain else 4)
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
        E = lambda *s, dt=F32: torch.empty(*s, dtype=dt, device=dev)
        T2 = self._relattn_terms2(M)
        # p = linear_pos(pos_emb), head-split [H, Rpad, 64] (+ transposed [H, 64, Rpad] for backward)
        Ph = E(H, Rpad, 64, dt=ACT)
        Pt = torch.zeros(H, 64, Rpad, dtype=ACT, device=dev) if save else None
        ptmp = E(Rpad, Da, dt=ACT)
        if T2:
            with ops.plain_precision():
                gemm_nt(pos16, W[pa + "linear_pos.weight"].w, EPI_BF16, outH=ptmp)
        else:
            gemm_nt(pos16, W[pa + "linear_pos.weight"].ws, EPI_BF16, outH=ptmp)
        Ph.copy_(ptmp.view(Rpad, H, 64).permute(1, 0, 2))
        if save:
            Pt.copy_(ptmp.view(Rpad, H, 64).permute(1, 2, 0))
        B16 = BF16 if save else ACT   # backward-only tensors (row-major V, transposed q+u / q+v / K)
        qu, k = [E(B * H, T, 64, dt=ACT) for _ in range(2)]
        v = E(B * H, T, 64, dt=B16)
        qv = E(B * H, T, 64, dt=ACT)
        use_pool = getattr(self, "_lease_ok", False) or not save
        vt = self._zeros(("dec_vt", li, B, Tpad), (B * H, 64, Tpad), ACT, dev, use_pool)
        qut = kt = qvt = None
        if save:
            qut, kt, qvt = [self._zeros(("dec", li, j, B, Tpad), (B * H, 64, Tpad), B16, dev, use_pool) for j in range(3)]
        if T2:
            call("sed_gemm_qkv_w2s", yop, W[pa + "in_proj.weight"].ws, bias[0], M, Dm, H, T, Tpad,
                 qu, k, v, qut, kt, vt, qv, qvt, bias[1], bias[2], 3 if save else 1)
        else:
            call("sed_gemm_qkv", yop, W[pa + "in_proj.weight"].ws, bias[0], M, 3 * Dm, H, T, Tpad,
                 qu, k, v, qut, kt, vt, qv, qvt, bias[1], bias[2], 3 if save else 1)
        o16 = E(M, Da)
        lse = E(B * H, T)
        o16s = E(M, 3 * Da, dt=F16)      # split-precision image of the attention output, written by the kernel itself
        if hwt is None:
            call("sed_relpos_attn_fwd", qu, qv, k, vt, Ph, o16, o16s, lse, B, H, T, Tpad, Rpad, 1, 1)
        else:       # local window (decoder_win_len): the band kernels skip the key tiles no query of a workgroup sees
            call("sed_relpos_attn_band_fwd", qu, qv, k, vt, Ph, o16, o16s, lse, B, H, T, Tpad, Rpad, 1, 1, hwt)
        out = E(*res.shape)
        gemm_nt(o16s, W[pa + "out_proj.weight"].ws, EPI_F32_RESID, bias=self.P(pa + "out_proj.bias"), res=res, outF=out)
        # (y16 / o16s are [M, 3 K] images whose first third is the f16 operand of the weight gradients)
        return out, (dict(y16=yop, Ph=Ph, Pt=Pt, qu=qu, qut=qut, qv=qv, qvt=qvt, k=k, kt=kt, v=v, o16=o16, o16s=o16s, lse=lse) if save else None)

    @in_split_precision
    def _decoder_fwd(self, W, x, save):
        """TransformerXLDecoder (src/models/transformer_decoder.py:110-122, transformerXL.py:31-35) at the width of x [B, T, width] f32: the
        one Transformer-XL schedule of every engine.  A variant overrides `_ctx_ln_fwd` / `_ctx_ln_bwd`, `_relattn_bias` and
        `_relattn_sink`, never the schedule."""
        m = self.m
        dev = x.device
        B, T, Dm = x.shape
        M = B * T
        T2 = self._relattn_terms2(M)
        pos16, _, Rpad = self._pos(T, dev, Dm, want_plain=T2)
        E = lambda *s, dt=F32: torch.empty(*s, dtype=dt, device=dev)
        ctx = dict(B=B, T=T, Tpad=pad64(T), Rpad=Rpad, layers=[])
        cur = x
        hwt = band_half_width(m, dev, T)
        for li in range(m.decoder_layer_num):
            p = f"decoder.encoder_blocks.{li}."
            pa = p + "attn."
            in_scale = math.sqrt(Dm) if li == 0 else 1.0
            mean1, rstd1 = (E(M), E(M)) if save else (None, None)
            # (two-term in_proj: the plain f16 image is all it reads)
            y16, y32 = self._ctx_ln_fwd(cur, p + "norm1", in_scale, mean1, rstd1, plain=T2, want32=True)
            x1, att = self._relattn_fwd(W, pa, li, ctx, pos16, hwt, y16, y32, self._relattn_bias(pa, li), save)
            mean2, rstd2 = (E(M), E(M)) if save else (None, None)
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

    def _tap(self, where, value):
        """`extract_features` (passt_sed.py): hand out the stage output it asked for.  `feature_tap` is None on every other forward."""
        tap = getattr(self, "feature_tap", None)
        if tap is not None and tap["layer"] == where:
            tap["out"] = value

    # ------------------------------------------------------------------ context network, decoder="conformer"
    def _swish_ffn_fwd(self, W, ff, norm, xin, M, save):
        """xin + 0.5 * Linear(Swish(Linear(LayerNorm(xin)))) (conformer.py:98-101,134-137); `ff` / `norm`: parameter prefixes.  Returns the
        new stream [M, D] fp32 and what `_swish_ffn_bwd` reads."""
        dev = xin.device
        E = lambda *s, dt=F32: torch.empty(*s, dtype=dt, device=dev)
        img = lambda: E(M, 3 * D, dt=F16)       # [hi | lo | hi] operand image of an [M, D] activation
        y = img()
        mean, rstd = (E(M), E(M)) if save else (None, None)
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
        m = self.m
        dev = x.device
        B, T, _ = x.shape
        M = B * T
        T2 = self._relattn_terms2(M)
        pos16, _, Rpad = self._pos(T, dev, want_plain=T2)
        E = lambda *s, dt=F32: torch.empty(*s, dtype=dt, device=dev)
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
            mean1, rstd1 = (E(M), E(M)) if save else (None, None)
            y16, _ = self._ctx_ln_fwd(x1, p + "norm_mha", 1.0, mean1, rstd1, plain=T2)
            x2, att = self._relattn_fwd(W, pa, li, ctx, pos16, hwt, y16, x1, self._relattn_bias(pa, li), save)
            # ---- convolution module: x3 = x2 + pointwise_conv2(swish(norm(depthwise(glu(pointwise_conv1(norm_conv(x2)))))))
            pc = p + "conv_module."
            yc = img()
            meanc, rstdc = (E(M), E(M)) if save else (None, None)
            call("sed_layernorm_fwd", x2, self.P(p + "norm_conv.weight"), self.P(p + "norm_conv.bias"), 1e-5, 1.0, yc, None, meanc, rstdc,
                 M, D, 4)
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
            fmean, frstd = (E(M), E(M)) if save else (None, None)
            call("sed_layernorm_fwd", x4, self.P(p + "norm_final.weight"), self.P(p + "norm_final.bias"), 1e-5, 1.0, None, out, fmean, frstd,
                 M, D, 1)
            if save:
                ctx["layers"].append(dict(att, ffm=ffm, ff=ff, x1=x1, mean1=mean1, rstd1=rstd1, x2=x2, yc=yc, meanc=meanc, rstdc=rstdc, xp=xp,
                                          ys=ys, conv=conv, cmean=cmean, crstd=crstd, x4=x4, fmean=fmean, frstd=frstd))
            cur = out
            self._tap(li, cur.view(B, T, D))
        return cur.view(B, T, D), ctx

    # ------------------------------------------------------------------ full forward
    # `forward` and `_backward_impl` are the only whole-model drivers: each is a fixed sequence of stages, and a model variant (the
    # PMAM / DASM engine) overrides stages, never the drivers.  DESIGN.md lists the stages and both forms of each.
    def forward(self, mel, encoder_win=False, mix_rate=0.5, win_param=(512, 49), temp_w=1.0, pad_mask=None,
                mlm_plan=None, toffsets=None, rows=None, save=False, drop_masks=None):
        """`rows`: structured frequency patchout (passt.py:533-547) -- the kept frequency rows of every backbone call of this forward
        as lists of ints, the global pass first, then one set per sliding window in sweep order; None: nothing is dropped.
        `drop_masks`: injected dropout keep-masks of the CNN branch (PMAM)."""
        m = self.m
        dev = mel.device
        if mel.dtype != F32 or not mel.is_contiguous():
            mel = mel.contiguous().float()
        B, Fm, T = mel.shape
        assert Fm == 128
        # what the stages read of this call; `win`: the sliding-window sweep or None
        opt = dict(win=dict(mix=float(mix_rate), param=win_param, toffsets=toffsets) if encoder_win else None, rows=rows, F=12,
                   rows_dev=None, drop_masks=drop_masks, temp_w=temp_w, pad_mask=pad_mask)
        self._check_forward(T, opt, save)
        W = self._weights(need_t=save)
        lease = self._lease(save)
        out = {}
        tp = min((T - 16) // 10 + 1, 99)
        if rows is not None:
            opt["F"] = len(rows[0])
            opt["rows_dev"] = h2d(rows, torch.int32, dev)      # [1 + windows, F]: one upload for every row set of this forward
        pooled, frame16, ectx = self._encoder_fwd(W, mel, [0], tp, [0], save, want_frame=m.has_at or getattr(m, "dasm_head", None) is not None,
                                                  rows=None if rows is None else [opt["rows_dev"][0]], F=opt["F"])
        Tdec = (tp + 1) * m.decode_ratio      # 99 -> 100 frames (passt_sed.py:258)
        xg, tctx = self._trunk_fwd(W, mel, pooled, tp, Tdec, opt, save)
        out["frame_before_mask"] = xg
        if getattr(self, "feature_tap", None) is not None and self.feature_tap["layer"] == "after_interpolate":
            # what the reference's interpolate_module hook sees: the pooled encoder features at Tdec frames, encoder width
            x768 = xg
            if xg.shape[-1] != D or type(self)._trunk_fwd is not SedEngine._trunk_fwd:       # (a trunk that projects before it interpolates)
                x768 = torch.empty(B, Tdec, D, dtype=F32, device=dev)
                call("sed_interp_fwd", pooled, x768, B, tp, 1, m.decode_ratio)
            self._tap("after_interpolate", x768)
        dec_in = xg
        plan = mlm_plan if (m.mlm and mlm_plan is not None) else None
        if plan is not None:
            out["mask_id_seq"] = plan["mask_ids"]
            if plan["effective"]:
                dec_in = self._mlm_mask_fwd(xg, plan)
        # (heads-only training -- the finetune1 stage: nothing at or below the context network learns, its backward is never walked)
        dec_fwd = self._conformer_fwd if m.decoder_name == "conformer" else self._decoder_fwd
        xd, dctx = dec_fwd(W, dec_in, save and self._walks_decoder_fwd())
        actx = None
        if m.has_at:
            actx = self._at_fwd(W, frame16, ectx, save)
            out["at_out"] = actx["at_out"]
        hctx = self._heads_fwd(W, xd, ectx, opt, save, out)
        ctx = None
        if save:
            ctx = dict(B=B, T=T, tp=tp, Tdec=Tdec, ectx=ectx, dctx=dctx, actx=actx, hctx=hctx, xd=xd, W=W,
                       mlm_plan=plan if (plan is not None and plan["effective"]) else None, pooled=pooled, lease=lease, **tctx)
        self._lease_ok = False
        return out, ctx

    def _check_forward(self, T, opt, save):
        """What this engine refuses, before anything is launched.  (Checked on the host: the kernels index the mel rows and the
        frequency table with the values of `rows`.)"""
        rows = opt["rows"]
        if rows is None:
            return
        F = len(rows[0])
        n_sets = 1 + (len(window_starts(T, *opt["win"]["param"])) if opt["win"] else 0)
        if len(rows) != n_sets or not 1 <= F <= 12 or any(
                len(r) != F or min(r) < 0 or max(r) >= 12 or any(a >= b for a, b in zip(r, r[1:])) for r in rows):
            raise ValueError(f"rows: expected {n_sets} sets of equally many strictly increasing frequency rows in [0, 12), got {rows!r}")

    def _trunk_fwd(self, W, mel, pooled, tp, Tdec, opt, save):
        """Trunk stage: pooled encoder features [B, tp, D] -> the frame sequence the context network reads (`frame_before_mask`) and
        what `_trunk_bwd` needs of it (merged into the saved context).  Here: interpolation to 1000 frames, then the sliding windows."""
        assert Tdec == 1000, "MAT-SED expects 1000 decoder frames (passt_sed.py:260)"
        B = mel.shape[0]
        xg = torch.empty(B, Tdec, D, dtype=F32, device=mel.device)
        call("sed_interp_fwd", pooled, xg, B, tp, 1, self.m.decode_ratio)
        return xg, dict(wctx=self._window_features(W, mel, xg, Tdec, opt, save) if opt["win"] else None)

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
        wdesc = h2d([lefts, tps, offs], torch.int32, dev)       # one upload for the three window tables
        wl, wt, wo = wdesc[0], wdesc[1], wdesc[2]
        call("sed_window_mix", packed, wl, wt, wo, len(starts), xg, opt["win"]["mix"], B, Tdec, self.m.decode_ratio)
        if not save:
            return None
        return dict(groups=wgroups, lefts=wl, tps=wt, offs=wo, n=len(starts), mix=opt["win"]["mix"], rows=row)

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
        E = lambda *s, dt=F32: torch.empty(*s, dtype=dt, device=xd.device)
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
            from .dasm import wide_head_fwd
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
        E = lambda *s: torch.empty(*s, dtype=F32, device=xd.device)
        strong, weak, sums = E(B, C, Tdec), E(B, C), E(B, C, 2)
        call("sed_head_fwd", xd, self.P("classifier.weight"), self.P("classifier.bias"), temp, pm, strong, weak, sums, B, Tdec, C)
        return strong, weak, dict(strong=strong, sums=sums, temp=temp)

    # ------------------------------------------------------------------ AT head
    def _at_fwd(self, W, frame16, ectx, save):
        m = self.m
        dev = frame16.device
        B, N = ectx["B"], ectx["N"]
        E = lambda *s, dt=F32: torch.empty(*s, dtype=dt, device=dev)
        pre = "at_adpater.0."
        win = self.P(pre + "frequency_att.in_proj_weight")
        bin_ = self.P(pre + "frequency_att.in_proj_bias")
        q = E(1, D)
        call("sed_small_linear", self.P(pre + "f_att_token").reshape(1, D), win[:D], bin_[:D], q, 1, D, D, 0)
        kv16 = E(B * N, 2 * D, dt=ACT)
        gemm_nt(frame16, W[pre + "frequency_att.in_proj_weight"].w[D:], EPI_BF16, bias=bin_[D:], outH=kv16)
        pooled = E(B, D)
        probs = E(B * H, N - 2) if save else None
        call("sed_attnpool_fwd", kv16, q, pooled, probs, B, N, H, is_f16(kv16))
        att = E(B, D)
        call("sed_small_linear", pooled, self.P(pre + "frequency_att.out_proj.weight"),
             self.P(pre + "frequency_att.out_proj.bias"), att, B, D, D, 0)
        C = m.class_num
        at_out = E(B, C)
        call("sed_small_linear", att, self.P("at_adpater.1.weight"), self.P("at_adpater.1.bias"), at_out, B, C, D, 1)
        return dict(q=q, kv16=kv16, pooled=pooled, probs=probs, att=att, at_out=at_out)

    # ==================================================================== backward
    def _join_dw(self):
        """Make the current stream wait for the weight-gradient GEMMs issued on the side stream so far."""
        if self._dw_pending:
            torch.cuda.current_stream().wait_stream(self._dw_stream)
            self._dw_pending = False

    def backward(self, ctx, grads, garena, hook=None):
        """Backward of the whole model (see `_backward_impl`); gradients in the arena are complete when it returns, and the ones of a
        stage are complete when its hook fires."""
        h = hook
        if hook is not None:
            def h(stage):
                self._join_dw()
                hook(stage)
        try:
            return self._backward_impl(ctx, grads, garena, h)
        finally:
            self._join_dw()
            self._lo_cache = None
            self._genc16 = None       # (the bf16 gradient image handed from block to block does not outlive the backward)

    def _backward_impl(self, ctx, grads, garena, hook=None):
        """grads: dict of upstream gradients (strong / weak / at_out / mlm_pred / frame_before_mask, any may be None).
        garena: callable name -> fp32 gradient view (zero-initialised) or None when the parameter is frozen."""
        m = self.m
        W, G = ctx["W"], garena
        ectx = ctx["ectx"]
        depth = len(ectx["layers"])
        at_grad = grads["at_out"].contiguous().float() if (m.has_at and grads.get("at_out") is not None) else None
        # ---------------- heads -> d(context-network output) [B, Tdec, width] (and d(final-norm frame tokens) of a head that reads them)
        g, dframe = self._heads_bwd(W, ctx, grads, G)
        # ---------------- nothing at or below the context network learns (finetune1: heads only): neither it nor the encoder is walked
        if not self._walks_decoder(G, depth) and grads.get("frame_before_mask") is None:
            if hook is not None:
                hook("decoder")
            if at_grad is not None:
                self._at_bwd(W, ctx["actx"], ectx, at_grad, G, need_dx=False)
            if hook is not None:
                hook("heads")
            return
        g = self._context_bwd(W, ctx, g, G)        # d(context-network input)
        if ctx["mlm_plan"] is not None:
            g = self._mlm_mask_bwd(g, ctx["mlm_plan"], G)
        if hook is not None:
            hook("decoder")  # classifier / mlm head / context-network / mask_token gradients are final
        dfbm = grads.get("frame_before_mask")
        if dfbm is not None:
            g = g + dfbm.contiguous().float()
        dpooled = self._trunk_bwd(W, ctx, g, G)
        # ---------------- what arrives at the top of the encoder stack (AT head, a head's frame tokens), then f_pool and the stack
        lo, _ = self._lowest_trainable(G, depth)
        genc = None
        if at_grad is not None:
            genc = self._at_bwd(W, ctx["actx"], ectx, at_grad, G, need_dx=lo < depth)
        if dframe is not None:
            genc = self._frame_norm_bwd(ectx, dframe, G, need_dx=lo < depth)
        self._encoder_bwd(W, ectx, genc, dpooled, G, hook)

    def _heads_bwd(self, W, ctx, grads, G):
        """-> (gradient of the context network's output [B, Tdec, width], gradient of the final-norm patch tokens or None)."""
        if self.m.mlm:
            return self._mlm_head_bwd(W, ctx, grads.get("mlm_pred"), G), None
        hc = ctx["hctx"]
        ds, dw = grads.get("strong"), grads.get("weak")
        if ds is None and dw is None:
            return torch.zeros_like(ctx["xd"]), None
        if hc.get("wide"):
            from .dasm import wide_head_bwd
            g = wide_head_bwd(hc, self.P("classifier.weight").detach(), ds, dw, G("classifier.weight"), G("classifier.bias"))
            return g.view(ctx["xd"].shape), None
        return self._head10_bwd(ctx, None if ds is None else ds.contiguous().float(), None if dw is None else dw.contiguous().float(), G), None

    def _head10_bwd(self, ctx, ds, dw, G):
        hc, g = ctx["hctx"], torch.empty_like(ctx["xd"])
        call("sed_head_bwd", ctx["xd"], self.P("classifier.weight"), hc["strong"], hc["sums"], ds, dw, hc["temp"],
             g, G("classifier.weight"), G("classifier.bias"), ctx["B"], ctx["Tdec"], self.m.class_num)
        return g

    def _context_bwd(self, W, ctx, g, G):
        if self.m.decoder_name == "conformer":
            return self._conformer_bwd(W, ctx["dctx"], g, G, G("decoder.blocks.0.self_attn.in_proj.weight") is not None)
        return self._decoder_bwd(W, ctx["dctx"], g, G, G("decoder.encoder_blocks.0.attn.in_proj.weight") is not None)

    def _trunk_bwd(self, W, ctx, g, G):
        """Backward of `_trunk_fwd`: d(frame_before_mask) -> d(pooled) [B, tp, D].  Here the sliding windows (student with
        encoder_win=True: x = (1 - mix) global + mix * local), each group's encoder pass without stage hooks, then the interpolation."""
        m = self.m
        B, Tdec, tp = ctx["B"], ctx["Tdec"], ctx["tp"]
        E = lambda *s: torch.empty(*s, dtype=F32, device=g.device)
        wctx = ctx.get("wctx")
        if wctx is not None:
            dpacked = E(wctx["rows"], D)
            gglob = E(B, Tdec, D)
            call("sed_window_mix_bwd", g.contiguous(), wctx["lefts"], wctx["tps"], wctx["offs"], wctx["n"], dpacked, gglob,
                 wctx["mix"], B, Tdec, m.decode_ratio, wctx["rows"])
            g = gglob
            for grp in wctx["groups"]:
                gctx = grp["ectx"]
                self._encoder_bwd(W, gctx, None, dpacked[grp["row0"]:grp["row0"] + grp["rows"]].view(gctx["B"], gctx["tp"], D), G, None)
        dpooled = E(B, tp, D)
        call("sed_interp_bwd", g, dpooled, B, tp, 1, m.decode_ratio)
        return dpooled

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

    def _fpool_bwd(self, W, ectx, dpooled, G, need_dx):
        """Backward of `_fpool_fwd`; -> its gradient at the encoder residual stream of the tapped layer [B, N, D] (cls / dist rows
        zero), or None when `need_dx` is false and the form can skip it."""
        if self.m.f_pool_name == FPOOL_TRANSFORMER:
            return self._fpool_tr_bwd(W, ectx, dpooled, G, need_dx)
        B, N, tp, F = ectx["B"], ectx["N"], ectx["tp"], ectx["F"]
        dev = dpooled.device
        Z = lambda *s: torch.zeros(*s, dtype=F32, device=dev)
        gpool = Z(B, N, D) if need_dx else None
        dtok_tmp = torch.empty(B, N, D, dtype=F32, device=dev)
        pool_dx = gpool if need_dx else Z(B, N, D)
        call("sed_fpool_rows_bwd", dpooled.contiguous(), ectx["pool_x"], ectx["pool_mean"], ectx["pool_rstd"], self.P("out_norm.weight"),
             dtok_tmp, pool_dx, G("out_norm.weight"), G("out_norm.bias"), B, tp, F)
        return gpool

    def _fpool_tr_bwd(self, W, ectx, dpooled, G, need_dx):
        """Backward of `_fpool_tr_fwd`.  A frozen module (finetune1: `G` names none of its tensors) is still walked: out_norm and the
        encoder lie under it."""
        B, tp, F = ectx["B"], ectx["tp"], ectx["F"]
        T = ectx.pop("pool_tr")
        N, S = 1 + F, B * tp
        M = S * N
        dev = dpooled.device
        E = lambda *s, dt=F32: torch.empty(*s, dtype=dt, device=dev)
        pre = "f_pool_module."
        part = getattr(self, "_fpool_ws", None)       # per-workgroup partials of the parameter-gradient reductions (see include/sed_hip.h)
        if part is None or part.device != dev:
            part = self._fpool_ws = torch.empty(256 * 3 * D, dtype=F32, device=dev)
        g = E(M, D)
        call("sed_fpool_rownorm_bwd", dpooled.contiguous(), T["x_out"], T["fmean"], T["frstd"], self.P(pre + "frequency_transformer_norm.weight"),
             g, G(pre + "frequency_transformer_norm.weight"), G(pre + "frequency_transformer_norm.bias"), part, part.numel(), S, N)
        for i in (1, 0):
            p = f"{pre}frequency_transformer.{i}."
            L = T["layers"][i]
            # ---- MLP branch: x_out = x_mid + fc2(gelu(fc1(LN2(x_mid))))
            dln = self._mlp_bwd(W, p + "mlp.fc1", p + "mlp.fc2", g, L["h2"], L["hpre"], L["act"], M, G, residual=None)
            call("sed_layernorm_bwd", dln, L["x_mid"], L["mean2"], L["rstd2"], self.P(p + "norm2.weight"), 1.0, g, 1,
                 G(p + "norm2.weight"), G(p + "norm2.bias"), M, D)
            del dln
            # ---- attention branch: x_mid = x_in + proj(attn(LN1(x_in)))
            g16 = self._dw_accum(g, L["o16"], M, G(p + "attn.proj.weight"), G(p + "attn.proj.bias"), k_in=D)
            do16 = E(M, D, dt=BF16)
            gemm_nt(g16, W[p + "attn.proj.weight"].wt, EPI_BF16, outH=do16)
            dqkv = E(M, 3 * D, dt=BF16)
            call("sed_attn_short_bwd", L["qkv"], do16, dqkv, S, N, FPOOL_HEADS, o_kind(L["qkv"]))
            del do16
            self._dw_accum(dqkv, L["h16"], M, G(p + "attn.qkv.weight"), None, k_in=D)
            dln = E(M, D)
            gemm_nt(dqkv, W[p + "attn.qkv.weight"].wt, EPI_F32, outF=dln)
            call("sed_layernorm_bwd", dln, L["x_in"], L["mean1"], L["rstd1"], self.P(p + "norm1.weight"), 1.0, g, 1,
                 G(p + "norm1.weight"), G(p + "norm1.bias"), M, D)
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
        dev = dy.device
        if dy16 is not None:      # the producer of dy already wrote its bf16 image (sed_layernorm_bwd_x16): no cast pass, bias sums in the TN kernel
            dy = dy16
        n_out, ldx = dy.shape[1], x.shape[1]
        # a saved split-precision image [M, 3 k_in] = [hi | lo | hi] (context network, MLM head) serves as the f16 operand through its
        # first third: the weight gradient sees the activation at the precision the encoder's gradients see theirs
        # (callers that hold split images pass `k_in`; otherwise it is inferred from the gradient view)
        if k_in is None:
            k_in = gW.shape[1] if (gW is not None and x.dtype == F16 and ldx == 3 * gW.shape[1]) else ldx
        E = lambda *s, dt=F32: torch.empty(*s, dtype=dt, device=dev)
        Mt = M                 # (the TN kernel masks a ragged last 64-token tile itself; rounds 1-3 sent the tail through the NT kernel)
        tn = self.dw_tn and Mt >= 1024 and dw_tn_ok(Mt, n_out, k_in) and x.dtype in (F16, BF16, F32)
        if tn and x.dtype == F32 and gW is not None:
            # an fp32 saved operand (projector / pooling inputs): one cast pass to bf16 instead of a transposing pass, then the TN kernel
            x16 = E(M, ldx, dt=BF16)
            transpose_bf16(x, M, ldx, None, out_s=x16)
            x = x16
        if tn:
            g16 = E(M, n_out, dt=BF16) if dy.dtype == F32 else None
            # bias gradient: with a 16-bit dy the TN kernel sums its own dY fragments (no extra pass over dy); an fp32 dy needs the
            # cast pass anyway, which also yields the column sums
            bias_in_gemm = g16 is None and bias is not None and gW is not None and Mt == M
            if g16 is not None or (bias is not None and not bias_in_gemm):
                transpose_bf16(dy, M, n_out, None, out_s=g16, colsum=bias)   # cast and/or column sums only, one pass
            dy16 = g16 if g16 is not None else dy
            if gW is not None:
                def run():
                    gemm_dw_tn(dy16, x, gW, tokens=Mt, dbias=bias if bias_in_gemm else None, k_in=k_in)
                    if Mt < M:
                        gT, xT = E(n_out, 64, dt=BF16), E(k_in, 64, dt=BF16)
                        transpose_bf16(dy16[Mt:], M - Mt, n_out, gT)
                        transpose_bf16(x[Mt:], M - Mt, k_in, xT, ld=ldx)
                        gemm_dw(gT, xT, gW)
                self._on_dw_stream(run, dy16, x)
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
        dev = dy.device
        E = lambda *s, dt=F32: torch.empty(*s, dtype=dt, device=dev)
        w1, w2 = W[n1 + ".weight"], W[n2 + ".weight"]
        hid = w1.w.shape[0]
        n_out = w2.w.shape[0]
        train = G(n1 + ".weight") is not None
        hpre = to_bf16_(hpre)
        g16 = self._dw_accum(dy, act, M, G(n2 + ".weight") if train else None, G(n2 + ".bias") if train else None, dy16=dy16,
                             k_in=w2.w.shape[1])
        dh16 = E(M, hid, dt=BF16)
        gemm_nt(g16, w2.wt, EPI_DGELU, outH=dh16, aux=hpre)
        if train:
            self._dw_accum(dh16, x16, M, G(n1 + ".weight"), G(n1 + ".bias"), k_in=w1.w.shape[1])
        if residual is not None:
            gemm_nt(dh16, w1.wt, EPI_F32_RESID, res=residual, outF=residual)
            return residual
        dx = E(M, w1.wt.shape[0])
        gemm_nt(dh16, w1.wt, EPI_F32, outF=dx)
        return dx

    def _enc_layer_bwd(self, W, ectx, li, g, G):
        p = f"backbone.blocks.{li}."
        L = ectx["layers"][li]
        B, N, Npad = ectx["B"], ectx["N"], ectx["Npad"]
        M = B * N
        dev = g.device
        E = lambda *s, dt=F32: torch.empty(*s, dtype=dt, device=dev)
        g2 = g.view(M, D)
        # The LayerNorm backward kernels leave the bf16 image of the residual-stream gradient they just updated: it is the dY operand of the
        # next weight-gradient / dX GEMMs (no cast pass over the fp32 stream; the bias gradient comes out of the TN kernel).
        x16_on = self.dw_tn
        gin16 = self._g16_take(g)
        # ---- MLP branch: x_out = x_mid + fc2(gelu(fc1(LN2(x_mid))))
        dln = self._mlp_bwd(W, p + "mlp.fc1", p + "mlp.fc2", g2, L["h2"], L["hpre"], L["act"], M, G, residual=None, dy16=gin16)
        gmid16 = E(M, D, dt=BF16) if x16_on else None
        if gmid16 is not None:
            call("sed_layernorm_bwd_x16", dln, L["x_mid"], L["mean2"], L["rstd2"], self.P(p + "norm2.weight"), 1.0, g2, 1,
                 G(p + "norm2.weight"), G(p + "norm2.bias"), gmid16, M, D)
        else:
            call("sed_layernorm_bwd", dln, L["x_mid"], L["mean2"], L["rstd2"], self.P(p + "norm2.weight"), 1.0, g2, 1,
                 G(p + "norm2.weight"), G(p + "norm2.bias"), M, D)
        del dln
        # ---- attention branch: x_mid = x_in + proj(attn(LN1(x_in)))
        g16 = self._dw_accum(g2, L["o16"], M, G(p + "attn.proj.weight"), G(p + "attn.proj.bias"), dy16=gmid16)
        do16 = E(M, D, dt=BF16)
        gemm_nt(g16, W[p + "attn.proj.weight"].wt, EPI_BF16, outH=do16)
        dqkv = E(M, 3 * D, dt=BF16)
        Dtmp = E(B * H, N)
        f16 = is_f16(L["q"])
        call("sed_mhsa_bwd", L["q"], L["k"], L["v"], L["o16"], do16, L["lse"], Dtmp, None, dqkv, B, H, N, Npad, f16, is_f16(L["v"]))
        del do16
        self._dw_accum(dqkv, L["h16"], M, G(p + "attn.qkv.weight"), G(p + "attn.qkv.bias"))
        dln = E(M, D)
        gemm_nt(dqkv, W[p + "attn.qkv.weight"].wt, EPI_F32, outF=dln)
        gout16 = E(M, D, dt=BF16) if x16_on else None
        if gout16 is not None:
            call("sed_layernorm_bwd_x16", dln, L["x_in"], L["mean1"], L["rstd1"], self.P(p + "norm1.weight"), 1.0, g2, 1,
                 G(p + "norm1.weight"), G(p + "norm1.bias"), gout16, M, D)
            self._genc16 = (g, gout16, g._version)      # for the block below (`_g16_take`)
        else:
            call("sed_layernorm_bwd", dln, L["x_in"], L["mean1"], L["rstd1"], self.P(p + "norm1.weight"), 1.0, g2, 1,
                 G(p + "norm1.weight"), G(p + "norm1.bias"), M, D)
        ectx["layers"][li] = None  # free saved activations
        return g

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
        E = lambda *s, dt=F32: torch.empty(*s, dtype=dt, device=dev)
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
        if residual is not None:       # (+ the gradient through the residual from the normalised input)
            gemm_nt(dqkv, W[pa + "in_proj.weight"].wt, EPI_F32_RESID, res=residual, outF=residual)
            return residual
        dy = E(M, Dm)
        gemm_nt(dqkv, W[pa + "in_proj.weight"].wt, EPI_F32, outF=dy)
        return dy

    def _decoder_bwd(self, W, dctx, g, G, trainable):
        """Backward of `_decoder_fwd` given g = d(output) [B, T, width]; -> d(input).  Parameter gradients go to the views `G` names
        (the attention's: where `_relattn_sink` says); none is computed when `trainable` is false.  (The PMAM form of the sink needs
        `dctx["slots"]`: the views of `_grad_slots` made with `dec_train` = `trainable`, as `PmamEngine._context_bwd` leaves them.)"""
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
        dev = g2.device
        E = lambda *s, dt=F32: torch.empty(*s, dtype=dt, device=dev)
        gh16 = E(M, D, dt=BF16)
        call("sed_scale_add_f32", g2, None, None, gh16, M * D, 0.5)        # the branch enters the stream at 0.5
        self._dw_accum(gh16, S["a"], M, Gl(ff + ".3.weight"), Gl(ff + ".3.bias"), k_in=D)
        dact = E(M, D)
        gemm_nt(gh16, W[ff + ".3.weight"].wt, EPI_F32, outF=dact)
        dh16 = E(M, D, dt=BF16)
        call("sed_swish_bwd", dact, S["h"], dh16, M * D)
        self._dw_accum(dh16, S["y"], M, Gl(ff + ".0.weight"), Gl(ff + ".0.bias"), k_in=D)
        gemm_nt(dh16, W[ff + ".0.weight"].wt, EPI_F32, outF=dact)
        call("sed_layernorm_bwd", dact, S["x_in"], S["mean"], S["rstd"], self.P(norm + ".weight"), 1.0, g2, 1,
             Gl(norm + ".weight"), Gl(norm + ".bias"), M, D)

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
        E = lambda *s, dt=F32: torch.empty(*s, dtype=dt, device=dev)
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

    def _at_bwd(self, W, a, ectx, dat, G, need_dx):
        """Backward of the AT head.  Returns d(encoder residual stream) [B, N, D] (or None when not needed)."""
        m = self.m
        dev = dat.device
        B, N = ectx["B"], ectx["N"]
        M = B * N
        E = lambda *s, dt=F32: torch.empty(*s, dtype=dt, device=dev)
        Z = lambda *s, dt=F32: torch.zeros(*s, dtype=dt, device=dev)
        pre = "at_adpater.0."
        C = m.class_num
        train = G("at_adpater.1.weight") is not None
        datt = E(B, D)
        call("sed_small_linear_bwd", a["att"], self.P("at_adpater.1.weight"), a["at_out"], dat, datt,
             G("at_adpater.1.weight"), G("at_adpater.1.bias"), B, C, D, 1)
        dpool = E(B, D)
        call("sed_small_linear_bwd", a["pooled"], self.P(pre + "frequency_att.out_proj.weight"), None, datt, dpool,
             G(pre + "frequency_att.out_proj.weight"), G(pre + "frequency_att.out_proj.bias"), B, D, D, 0)
        dkv = E(M, 2 * D, dt=BF16)
        dq = Z(1, D)
        call("sed_attnpool_bwd", a["kv16"], a["q"], a["probs"], dpool, dkv, dq, B, N, H, is_f16(a["kv16"]))
        gin = G(pre + "frequency_att.in_proj_weight")
        gib = G(pre + "frequency_att.in_proj_bias")
        win = self.P(pre + "frequency_att.in_proj_weight")
        if train:
            dtok = Z(1, D)
            call("sed_small_linear_bwd", self.P(pre + "f_att_token").reshape(1, D), win[:D], None, dq, dtok, gin[:D],
                 gib[:D], 1, D, D, 0)
            G(pre + "f_att_token").view(1, D).add_(dtok)
            self._dw_accum(dkv, ectx["frame16"], M, gin[D:], gib[D:])
        norm_train = G("backbone.norm.weight") is not None
        if not (need_dx or norm_train):
            return None
        dframe = E(M, D)
        gemm_nt(dkv, W[pre + "frequency_att.in_proj_weight"].wt[:, D:].contiguous(), EPI_F32, outF=dframe)
        genc = E(B, N, D)
        call("sed_layernorm_bwd", dframe, ectx["x_final"], ectx["fmean"], ectx["frstd"], self.P("backbone.norm.weight"),
             1.0, genc.view(M, D), 0, G("backbone.norm.weight"), G("backbone.norm.bias"), M, D)
        return genc if need_dx else None
