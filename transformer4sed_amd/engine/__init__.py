"""Forward/backward engine of the MI355X-native MAT-SED model.

This is the host-side orchestration of the HIP kernels behind `PaSST_SED.forward`
(reference: src/models/passt/passt_sed.py:242-296 and everything it calls).  It owns
  * the bf16 operand copies of all GEMM weights (straight [out,in] and transposed [in,out]),
  * the explicit forward schedule (saving exactly what the hand-written backward needs),
  * the explicit backward schedule writing into ONE flat fp32 gradient arena (views of which become `p.grad`,
    and which the data-parallel layer all-reduces in buckets, see ddp.py).
There is no autograd tape inside: `_SedFunction` in passt_sed.py exposes the whole model as a single
autograd node so that the reference's training loops (loss via torch ops, loss.backward()) keep working.

`SedEngine` is one class; its methods live in one module per subsystem (images, encoder, pooling, context, heads, grads), each a plain
method-holding base without state of its own: every attribute is set in `SedEngine.__init__` below.
"""
import os

import torch

from ..ops import F16, F32, call, h2d

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


def empty(dev):
    """E(*shape, dt=F32): an uninitialised tensor on `dev`."""
    def E(*s, dt=F32):
        return torch.empty(*s, dtype=dt, device=dev)
    return E


def stats(E, M, save):
    """(mean, rstd) [M] of a LayerNorm whose backward will read them; (None, None) in a pass that saves nothing."""
    return (E(M), E(M)) if save else (None, None)


# (the subsystem modules import the names above from this package: they come after them)
from .images import Images, ImageSpec, image_table, _W, version_key, cached_image, rel_pos_table       # noqa: E402
from .encoder import Encoder, window_starts       # noqa: E402
from .pooling import Pooling       # noqa: E402
from .context import Context, band_half_width, in_split_precision       # noqa: E402
from .heads import Heads       # noqa: E402
from .grads import Grads       # noqa: E402


class SedEngine(Images, Encoder, Pooling, Context, Heads, Grads):
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

    def __deepcopy__(self, memo):
        return None  # `ema_net = deepcopy(net)` (finetune/passt/setting.py:8-15): the copy rebuilds its engine lazily

    def P(self, name):
        return self.m._param_by_name[name]

    def _tap(self, where, value):
        """`extract_features` (passt_sed.py): hand out the stage output it asked for.  `feature_tap` is None on every other forward."""
        tap = getattr(self, "feature_tap", None)
        if tap is not None and tap["layer"] == where:
            tap["out"] = value

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

    # ==================================================================== backward
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

    def _trunk_bwd(self, W, ctx, g, G):
        """Backward of `_trunk_fwd`: d(frame_before_mask) -> d(pooled) [B, tp, D].  Here the sliding windows (student with
        encoder_win=True: x = (1 - mix) global + mix * local), each group's encoder pass without stage hooks, then the interpolation."""
        m = self.m
        B, Tdec, tp = ctx["B"], ctx["Tdec"], ctx["tp"]
        E = empty(g.device)
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
