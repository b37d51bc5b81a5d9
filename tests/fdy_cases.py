"""Shared by tests/test_fdy_cnn_cpu.py and tests/test_gpu_fdy_cnn.py (importable without a GPU): a plain-torch restatement of the
frequency-dynamic convolution (src/models/cnn/FDY_cnn.py:7-116, pool_dim 'freq') and of the whole CNN branch with dynamic layers
(FDY_cnn.py:139-177 with activation 'cg', normalization 'batch'), the kernel-test shapes, and inputs a 16-bit operand holds exactly.

The restatement is dtype-generic: in float64 it is the reference of the kernel tests, in float32 it measures what fp32 arithmetic alone
loses (the bound of tests/test_gpu_conformer.py: |got - ref64| <= 8 max|ref32 - ref64| + half an ulp of the output's storage format), and
autograd gives every backward.  tests/test_fdy_cnn_cpu.py checks it against the recorded outputs of the reference module itself."""
import numpy as np
import torch
import torch.nn.functional as F

from transformer4sed_amd import synth

N_BASIS = 4

# mixing forward / backward: (B, H, W, co)
MIX_CASES = [(1, 2, 1, 16),          # smallest
             (2, 5, 3, 32),          # odd sizes
             (3, 250, 2, 384),       # widest
             (2, 500, 64, 16)]       # longest rows
# attention head and frequency mean: (B, H, W, cin)
HEAD_CASES = [(2, 1, 4, 16),         # one frame: both outer taps fall in the padding; hid = 4
              (1, 2, 1, 16),         # W = 1
              (3, 7, 5, 32),         # hid = 8
              (2, 250, 2, 256),      # hid = 64
              (2, 500, 64, 16)]      # largest
TEMPERATURES = (31.0, 1.0)

FDY_CNN_PARAM = dict(cnn_name="FDY-CNN", n_input_ch=1, activation="cg", conv_dropout=0.5, kernel=[3] * 7, pad=[1] * 7, stride=[1] * 7,
                     nb_filters=list(synth.FDY_FILTERS), pooling=[list(p) for p in synth.FDY_POOLING], normalization="batch",
                     n_basis_kernels=4, DY_layers=list(synth.FDY_DY_LAYERS), temperature=31, pool_dim="freq")
PMAM10_DY = [0] + [1] * 9
FDY10_CNN_PARAM = dict(FDY_CNN_PARAM, kernel=[3] * 10, pad=[1] * 10, stride=[1] * 10, nb_filters=list(synth.PMAM_FILTERS),
                       pooling=[list(p) for p in synth.PMAM_POOLING], DY_layers=PMAM10_DY)


def hid_of(cin):
    return max(cin // 4, 4)


def exact16(key, shape, scale=1.0, steps=32):
    """Deterministic values k / steps * scale, |k| <= steps: exact in bf16 and IEEE half when scale is a power of two."""
    return (np.round(synth.det_uniform(key, shape) * steps) / steps * scale).astype(np.float32)


# ------------------------------------------------------------------------------------------------ one dynamic layer
def attention_head(pm, c1w, bn_w, bn_b, bn_rm, bn_rv, c2w, c2b, temperature, train, eps=1e-5):
    """pm [B, cin, H] (the input's mean over the mel bins) -> (attention [B, 4, H], batch mean, biased batch variance of conv1d1's output)."""
    u = F.conv1d(pm, c1w, padding=1)
    mean, var = u.mean((0, 2)), u.var((0, 2), unbiased=False)
    m_, v_ = (mean, var) if train else (bn_rm, bn_rv)
    n = torch.relu((u - m_[None, :, None]) / torch.sqrt(v_[None, :, None] + eps) * bn_w[None, :, None] + bn_b[None, :, None])
    return torch.softmax(F.conv1d(n, c2w, c2b) / temperature, 1), mean, var


def mix(y4, att):
    """y4 [B, 4 co, H, W] (the four basis convolutions), att [B, 4, H] -> [B, co, H, W]."""
    B, kc, H, W = y4.shape
    return (y4.view(B, N_BASIS, kc // N_BASIS, H, W) * att[:, :, None, :, None]).sum(1)


def _hook(t, qb):
    if qb is not None and t.requires_grad:
        t.register_hook(qb)
    return t


def dynamic_conv(x, p, temperature, train, qb=None):
    """x [B, cin, H, W]; p: weight [4, co, cin, 3, 3] and the attention head's tensors -> (y, attention, mean, var).
    qb: rounding of the gradient of the four basis convolutions' output (the engine's 16-bit GEMM operand a (x) dY)."""
    att, mean, var = attention_head(x.mean(3), p["attention.conv1d1.weight"], p["attention.bn.weight"], p["attention.bn.bias"],
                                    p["attention.bn.running_mean"], p["attention.bn.running_var"], p["attention.conv1d2.weight"],
                                    p["attention.conv1d2.bias"], temperature, train)
    w = p["weight"]
    y4 = _hook(F.conv2d(x, w.reshape(-1, *w.shape[2:]), padding=1), qb)
    return mix(y4, att), att, mean, var


# ------------------------------------------------------------------------------------------------ the branch
def branch(sd, mel, pooling, dy_layers, temperature, train, drop_masks=None, drop_p=0.0, uniform_attention=False, q=None, qb=None):
    """sd: tensors under the names of `cnn.cnn.` (prefix stripped); mel [B, 128, T] -> (features [B, C, T', 1], per-layer records).
    drop_masks: per layer keep-masks [B, C, H, W] (train mode).  q: rounding applied to what the engine stores in 16 bits -- the
    activations between the layers, the GEMM weights and the gate GEMM's input -- to emulate its storage formats on the CPU; qb: rounding of the gradients the engine's backward stores in 16 bits
    (bfloat16): those of the convolution outputs and of the gate logits, the operands of its weight- and input-gradient GEMMs."""
    x = mel.transpose(1, 2).unsqueeze(1)
    rec = []
    if q is not None:
        sd = {k: (q(v) if (k.endswith("weight") and v.dim() >= 2 and ".attention." not in k and not k.startswith("conv0.")) else v)
              for k, v in sd.items()}
    for i, (ph, pw) in enumerate(pooling):
        sub = lambda s, i=i: {k[len(f"{s}{i}."):]: v for k, v in sd.items() if k.startswith(f"{s}{i}.")}
        cv, bn, cg = sub("conv"), sub("batchnorm"), sub("cg")
        r = {}
        if dy_layers[i]:
            if uniform_attention:
                w = cv["weight"]
                y = F.conv2d(x, w.mean(0), padding=1)
            else:
                y, att, mean, var = dynamic_conv(x, cv, temperature, train, qb)
                r.update(att=att, mean=mean, var=var, rows=x.shape[0] * x.shape[2])
        else:
            y = F.conv2d(x, cv["weight"], cv["bias"], padding=1)
        y = _hook(y, qb)
        if train:
            m2, v2 = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
            r.update(mean2=m2, var2=v2, count2=y.numel() // y.shape[1])
        else:
            m2, v2 = bn["running_mean"], bn["running_var"]
        z = (y - m2[None, :, None, None]) / torch.sqrt(v2[None, :, None, None] + 1e-3) * bn["weight"][None, :, None, None] + bn["bias"][None, :, None, None]
        zq = z if (q is None or z.shape[1] == 16) else q(z)      # (16 filters: the gate Linear runs in fp32 inside the pooling kernel)
        lin = _hook(F.linear(zq.permute(0, 2, 3, 1), cg["linear.weight"], cg["linear.bias"]).permute(0, 3, 1, 2), qb)
        z = z * torch.sigmoid(lin)
        if train and drop_masks is not None:
            z = z * drop_masks[i].to(z.dtype) / (1.0 - drop_p)
        x = F.avg_pool2d(z, (ph, pw))
        if q is not None and i + 1 < len(pooling):
            x = q(x)
        rec.append(r)
    return x, rec


def cnn_tensors(sd_np, dtype):
    """The `cnn.cnn.*` tensors of a synthetic state dict as torch tensors of `dtype`, prefix stripped."""
    return {k[len("cnn.cnn."):]: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in sd_np.items()
            if k.startswith("cnn.cnn.") and not k.endswith("num_batches_tracked")}


def drop_masks_np(tag, B, filters, pooling, p, T=1000):
    """Deterministic keep-masks per layer in the engine's layout [B, H, W, C] (bool); `.transpose(0, 3, 1, 2)` is the reference's."""
    out, Hc, Wc = [], T, 128
    for i, co in enumerate(filters):
        out.append(synth.det_uniform(f"{tag}/drop{i}", (B, Hc, Wc, co), 0.0, 1.0) >= p)
        Hc, Wc = Hc // pooling[i][0], Wc // pooling[i][1]
    return out


# ------------------------------------------------------------------------------------------------ kernel-test inputs and reference of the head
def head_inputs(B, H, W, cin, temperature):
    hid = hid_of(cin)
    tag = f"fdy/head/{B}x{H}x{W}x{cin}"
    u = lambda k, shp, s=1.0: torch.from_numpy(synth.det_uniform(f"{tag}/{k}", shp) * s).float()
    return dict(x=torch.from_numpy(exact16(tag + "/x", (B, H, W, cin), 2.0)),
                c1w=u("c1", (hid, cin, 3), 3.0 / np.sqrt(3 * cin)), bn_w=1.0 + u("bnw", (hid,), 0.2), bn_b=u("bnb", (hid,), 0.1),
                bn_rm=u("bnm", (hid,), 0.3), bn_rv=1.0 + u("bnv", (hid,), 0.5),
                c2w=u("c2", (4, hid, 1), 2.0 * temperature / np.sqrt(hid)), c2b=u("c2b", (4,), 0.1),       # logits / temperature of a few units
                da=torch.from_numpy(synth.det_normal(tag + "/da", (B * H, 4), 1.0)), dx0=torch.from_numpy(synth.det_normal(tag + "/dx0", (B, H, W, cin), 1.0)))


def head_ref(inp, temperature, train, dt):
    """-> dict of pm [R, cin], att [R, 4], batch mean / var, and through autograd of sum(att da): dX (on top of dx0), parameter gradients."""
    t = {k: v.to(dt) for k, v in inp.items()}
    B, H, W, cin = t["x"].shape
    x = t["x"].permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    ps = {k: t[k].clone().requires_grad_(True) for k in ("c1w", "bn_w", "bn_b", "c2w", "c2b")}
    pm = x.mean(3)
    att, mean, var = attention_head(pm, ps["c1w"], ps["bn_w"], ps["bn_b"], t["bn_rm"], t["bn_rv"], ps["c2w"], ps["c2b"], temperature, train)
    (att.permute(0, 2, 1).reshape(-1, 4) * t["da"]).sum().backward()
    out = dict(pm=pm.detach().permute(0, 2, 1).reshape(-1, cin), att=att.detach().permute(0, 2, 1).reshape(-1, 4), mean=mean.detach(), var=var.detach(),
               dX=t["dx0"] + x.grad.permute(0, 2, 3, 1))
    out.update({"g_" + k: v.grad for k, v in ps.items()})
    return out
