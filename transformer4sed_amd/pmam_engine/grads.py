"""The LoRA and narrow weight-gradient routes: `_dw_accum` on the LoRA factors, `_dw_swapped` into the gradient images of
`_grad_slots`, and the encoder block's backward with the LoRA linears' weight gradients redirected."""
import torch

from ..engine import H
from ..ops import BF16, F16, F32, call, h2d, gemm_dw, gemm_dw_tn, pad64, transpose_bf16, is_f16
from . import HD_PAD
from .geometry import SMALL_DW, dw_swapped_tn


class _LoraSlot:
    """What the encoder backward receives in place of a LoRA linear's weight-gradient view: the factors and their gradient views."""
    __slots__ = ("A", "B", "gA", "gB", "r", "s", "shape")

    def __init__(self, A, B, gA, gB, r, s):
        self.A, self.B, self.gA, self.gB, self.r, self.s = A, B, gA, gB, r, s
        self.shape = (B.shape[0], A.shape[1])


class PmamGrads:
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
        return dw_swapped_tn(self.dw_tn, M, n, k)

    def _dw_swapped(self, dy16, x, M, n_valid, k_valid, out=None, image=None):
        """(dy^T x)^T = x^T dy for operand widths that are not multiples of 128 on the x side: returns fp32 [k, n] and the fp32 column
        sums of dy; only [:k_valid, :n_valid] / [:n_valid] are meaningful.  The operands are zero padded to GEMM-friendly widths
        (16 filters sit in 128 columns): only the 64-column groups that hold valid data are transposed, the other rows of the
        transposed images stay uninitialised and only feed output elements nobody reads.  `out` = (zeroed flat fp32 [n k], zeroed
        fp32 [n]): the gradient-image slots of `_grad_slots` (accumulated into; nothing is allocated or filled here).  `image`: the
        `DwImage` of a CNN layer's plan that `out` was laid out by -- its rows, row width, layout and route are taken as planned (the
        operands may be narrower than the image: the 16-column images of the 16-filter layers); without it they follow from the operands."""
        dev = dy16.device
        n, k = (dy16.shape[1], x.shape[1]) if image is None else (image.rows, image.k)
        laid_tn = self._dw_swapped_tn(M, n, k) if image is None else image.tn
        tn = laid_tn and dy16.dtype == BF16 and x.dtype in (F16, BF16)
        if out is not None and tn != laid_tn:
            raise RuntimeError("gradient-image slot laid out for the TN kernel, operands are not 16-bit")
        if image is not None and image.route == SMALL_DW:
            # the streaming reduction (geometry._dw_image has the conditions and the measurements); same [n, k] image layout
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

    def _grad_slots(self, B, dev, G, dec_train, cnn_train, T=None):
        """Gradient images of every padded weight / vector of one backward, as views of ONE zeroed fp32 arena, and the two
        `sed_scatter_add_f32` tables (context network, CNN branch) that return them to the masters' gradients through the forward
        plans -- scale sqrt(2) on the K / P rows, nothing from the padding.  Replaces a `zeros` per image and an `add_` of a sliced /
        permuted view per master (~190 launches per step) by one fill and two launches.  `T`: frames of the forward being differentiated
        (`cnn_train`: the CNN images follow its layer plans, which the views carry as "cnn_plans")."""
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
        cnn_plans = None
        if cnn_train:
            if T is None:
                raise ValueError("_grad_slots: the CNN branch's gradient images need the frame count T of the forward")
            cnn_plans = self._cnn_plan(B, T, dev)
            for i, (g, lp) in enumerate(zip(geo, cnn_plans)):
                co, Np, Kp, Cp = g["co"], g["Np"], g["Kp"], g["Cp"]
                cw, gw = f"cnn.cnn.conv{i}.weight", f"cnn.cnn.cg{i}.linear.weight"
                bplan = self._plan(("b", Np), self.P(f"cnn.cnn.cg{i}.linear.bias").shape, dev, None)
                # the gradient images hold the first ldg of the weight images' Np rows (64 for the 16 / 32 / 64-filter layers: the bf16
                # gradient operands are 64 columns wide there, round 4); the plans are read up to row ldg
                # (dynamic layer: the convolution's image has the 4 co rows of the basis kernels, ldg4 of them in the gradient image)
                Nc = g["Nc"] if g["dyn"] else Np
                for slot, master, plan, im in ((("gate", i), gw, self._plan(("gate", Np, Cp), self.P(gw).shape, dev, None), lp.gate),
                                               (("conv", i), cw, self._plan(("conv", Nc, Kp), self.P(cw).shape, dev, None), lp.conv)):
                    # image element (i, j) of [rows, k] sits at i k + j (TN) or j rows + i
                    items.append(("cnn", slot, im.rows * im.k, master, plan, im.rows * im.k, im.k, im.k if im.tn else 1, 1 if im.tn else im.rows))
                ldg, ldc = lp.gate.rows, lp.conv.rows
                items += [("cnn", ("gate_b", i), ldg, f"cnn.cnn.cg{i}.linear.bias", bplan, ldg, ldg, 0, 1),
                          # (the column sums of a (x) dY that the weight-gradient GEMM also writes have no master in a dynamic layer)
                          ("cnn", ("conv_b", i), ldc, None if g["dyn"] else f"cnn.cnn.conv{i}.bias", None if g["dyn"] else bplan, ldc, ldc, 0, 1),
                          ("cnn", ("bn_s1", i), co, f"cnn.cnn.batchnorm{i}.bias", None, co, co, 0, 1),
                          ("cnn", ("bn_s2", i), co, f"cnn.cnn.batchnorm{i}.weight", None, co, co, 0, 1)]
        if not items:
            return {}, {}
        gp = lambda n: G(n).data_ptr() if (n is not None and G(n) is not None) else 0      # (a master without a gradient slot: its image is formed and dropped)
        key = (B, T, bool(self.dw_tn), str(dev), dec_train, cnn_train, tuple(gp(it[3]) for it in items))
        if getattr(self, "_gslot_key", None) != key:
            total = sum((it[2] + 63) // 64 * 64 for it in items)
            arena = torch.empty(total, dtype=F32, device=dev)
            views, tables, off = {"cnn_plans": cnn_plans}, {}, 0
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
