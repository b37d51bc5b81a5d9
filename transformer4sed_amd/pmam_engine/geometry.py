"""The per-layer plan of the CNN branch: its shapes, its row pitches and which kernel takes each step.  Pure integer functions (no
torch, no `ops`): `cnn_geometry` is what does not depend on the input shape, `cnn_layer_plans` what does.  The forward, the backward,
the gradient-image slots and the weight-gradient routes all read these; none of them derives a copy."""
import collections

# which route fills a weight-gradient image (`DwImage.route`)
SMALL_DW = "sed_small_dw"        # streaming reduction: 16 / 32 filters against <= 32 columns
TN = "tn"                        # TN GEMM on the operands as they lie
COPY = "copy"                    # transposed copies of both operands + NT split-K GEMM
CONV0_DW16 = "sed_conv0_dw16"    # direct first convolution: the patches are gathered from the spectrogram again

# a weight-gradient image of `rows` x `k` fp32 words: element (i, j) sits at i k + j (`tn`) or at j rows + i
DwImage = collections.namedtuple("DwImage", "rows k tn route")
LayerPlan = collections.namedtuple("LayerPlan", "H W M ldy Ho Wo Cpo last direct0 fused16 ldyo gate conv")


def pad128(n):
    return (n + 127) // 128 * 128


def cnn_geometry(filters, pooling, dynamic=None):
    """Per layer, as a dict: the operand widths of a stack of 3x3 convolutions with `filters` output channels (`dynamic[i]`: a
    frequency-dynamic layer, four basis kernels).  Np / Kp / Cp: padded rows and columns of the convolution's and the gate's weight
    images; cpin: channel pitch of the layer's NHWC input; ldg: row width of the bf16 gradient operands (and rows of the gradient
    images)."""
    dynamic = dynamic or (False,) * len(filters)
    assert len(filters) == len(pooling) == len(dynamic)
    geo, cin = [], 1
    for i, co in enumerate(filters):
        Np = pad128(co)
        g = dict(Np=Np, Kp=64 if i == 0 else pad128(9 * cin), Cp=max(64, co), cin=cin, cpin=max(64, cin), co=co, ldg=64 if co <= 64 else Np,
                 dyn=bool(dynamic[i]))
        if g["dyn"]:
            # the four basis kernels [4, co, ci, 3, 3] are one [4 co, 9 ci] operand of Nc padded rows (FDY_cnn.py:44).  Y4 [pixels, ld4]
            # fp32: 64 columns for 16 filters (the GEMM writes only the valid columns), the padded width otherwise; ldg4: row width of
            # the bf16 gradient operand a (x) dY, as ldg for the static layers
            Nc = pad128(4 * co)
            g.update(Nc=Nc, ld4=64 if 4 * co == 64 else Nc, ldg4=64 if 4 * co <= 64 else Nc, hid=max(cin // 4, 4))
        geo.append(g)
        cin = co
    return geo


def dw_swapped_tn(dw_tn, M, n, k):
    """Is the gradient image of dy [M, n]^T x [M, k] laid out [n, k] for the TN kernel, or [k, n] for the transposed-copy path?"""
    # (below 1024 rows the transposed-copy path is the cheaper one -- but its split-K GEMM needs both widths to fill a 128-wide tile:
    #  the 64-wide images of the narrow layers stay on the TN kernel at any row count; the TN kernel takes multiples of 64 only)
    return bool(dw_tn and (M >= 1024 or n < 128 or k < 128) and n % 64 == 0 and k % 64 == 0)


def _dw_image(dw_tn, M, rows, k, n_valid, k_valid, ldx):
    """Image and route of dy[:, :n_valid]^T x[:, :k_valid], x stored `ldx` columns wide."""
    tn = dw_swapped_tn(dw_tn, M, rows, k)
    # 16 / 32 filters against <= 32 columns (the gate Linear, the first convolution's 9 taps): a streaming reduction instead of a
    # 256 x 256 tile's K loop (measured: 429 -> 165 us on layer 0, 207 -> 45 us on layer 1; the 144 / 288-column convolution gradients
    # stay on the TN kernel -- 169 / 457 us here against 164 / 201 there); same [n, k] image layout
    small = tn and n_valid in (16, 32) and k_valid <= 32 and ldx >= (k_valid + 3) // 4 * 4
    return DwImage(rows, k, tn, SMALL_DW if small else TN if tn else COPY)


def cnn_layer_plans(geometry, pooling, B, T, dw_tn):
    """Per layer of `cnn_geometry`, for a [B, 128, T] spectrogram: what depends on the shape.
      H, W, M      the layer's input grid and its pixels B H W;  Ho, Wo: the pooled grid;  Cpo: channel pitch of the pooled output
      ldy          row width of the fp32 convolution output (16 / 32 / 64 filters: the GEMM writes only the valid columns of its tile)
      direct0      first convolution with 16 filters directly on the spectrogram (`sed_conv0_fwd16`: no patch matrix, no GEMM)
      fused16      16 filters: the gate Linear inside the pooling kernel (`sed_cg_gate16_pool`); its narrow z image is an operand
                   `sed_small_dw` alone takes
      ldyo         row width of the bf16 dY (direct0: it only feeds the streaming weight-gradient reduction, 16 columns are all it needs)
      gate, conv   the layer's two weight-gradient images (`DwImage`)."""
    plans, H, W, n = [], T, 128, len(geometry)
    for i, (g, (ph, pw)) in enumerate(zip(geometry, pooling)):
        co, Np, Kp, Cp, ldg = g["co"], g["Np"], g["Kp"], g["Cp"], g["ldg"]
        M = B * H * W
        fused16 = bool(dw_tn and co == 16 and M >= 1024)
        direct0 = fused16 and i == 0
        gate = _dw_image(dw_tn, M, ldg, Cp, co, co, 16 if fused16 else Cp)
        if g["dyn"]:
            conv = _dw_image(dw_tn, M, g["ldg4"], Kp, 4 * co, 9 * g["cin"], Kp)
        elif direct0:
            conv = DwImage(ldg, Kp, dw_swapped_tn(dw_tn, M, ldg, Kp), CONV0_DW16)
            assert conv.tn      # `sed_conv0_dw16` writes a TN-layout image
        else:
            conv = _dw_image(dw_tn, M, ldg, Kp, co, 9 * g["cin"], Kp)
        Ho, Wo = H // ph, W // pw
        plans.append(LayerPlan(H, W, M, co if co < Np else Np, Ho, Wo, Cp, i + 1 == n, direct0, fused16, 16 if direct0 else ldg, gate, conv))
        H, W = Ho, Wo
    assert W == 1      # the frequency axis is pooled away
    return plans
