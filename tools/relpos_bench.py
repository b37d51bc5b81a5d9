"""Rel-pos attention forward / backward microbenchmark at the decoder's shape (developer tool; needs a GPU).  Kernel-level times
come from rocprofv3 (--kernel-trace --stats) around this script.

--win W[,W...] (an int, 'full', or a comma list; default 100,256,full): the local-window entry points (sed_relpos_attn_band_*) against
the unbanded ones in ONE process, alternating, ROUNDS rounds of REPS launches each between device events.  Per W: median time of both,
their ratio, the run-to-run spread (max - min over the rounds, relative to the median) of both, and the ratio of visited to total
tiles per kernel computed from the shapes -- the bound the time ratio is read against."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from transformer4sed_amd.ops import call, pad64
F16, BF16 = torch.float16, torch.bfloat16
B, H, T = 32, 12, 1000
Tpad, R = pad64(T), 2 * T - 1
Rpad = pad64(R)
dev = "cuda"
g = lambda *s, sc=1.0: torch.randn(*s, device=dev) * sc
qu, qv, k = [g(B * H, T, 64).to(F16) for _ in range(3)]
v = g(B * H, T, 64)
tr = lambda t, dt: torch.nn.functional.pad(t.float().transpose(1, 2), (0, Tpad - T)).to(dt).contiguous()
qut, qvt, kt, vt = tr(qu, BF16), tr(qv, BF16), tr(k, BF16), tr(v, F16)
P = torch.zeros(H, Rpad, 64, dtype=F16, device=dev); P[:, :R] = g(H, R, 64, sc=0.7).to(F16)
Pt = P.float().transpose(1, 2).to(BF16).contiguous()
O = torch.empty(B, T, 768, dtype=F16, device=dev); lse = torch.empty(B * H, T, device=dev)
dO = g(B, T, 768).to(BF16)
dqkv = torch.empty(B * T, 2304, dtype=BF16, device=dev); Dt = torch.empty(B * H, T, device=dev)
dOh = torch.empty(B * H, T, 64, dtype=BF16, device=dev); dOt = torch.empty(B * H, 64, Tpad, dtype=BF16, device=dev)
dSt = torch.zeros(B * H, Tpad, Tpad, dtype=BF16, device=dev); dP = torch.zeros(Rpad, 768, device=dev)
du = torch.zeros(H, 64, device=dev); dv = torch.zeros(H, 64, device=dev)
def fwd(): call("sed_relpos_attn_fwd", qu, qv, k, vt, P, O, None, lse, B, H, T, Tpad, Rpad, 1, 0)
Pst = torch.zeros(B * H, Tpad, Tpad, dtype=BF16, device=dev)
vb = v.to(BF16)
def bwd(): call("sed_relpos_attn_bwd", qu, qut, qv, qvt, k, kt, vb, P, Pt, O, dO, lse, Dt, dOh, dOt, dqkv, dSt, Pst, dP, du, dv, B, H, T, Tpad, Rpad, 1, 1, 1)
def bwd_rc(): call("sed_relpos_attn_bwd", qu, qut, qv, qvt, k, kt, vb, P, Pt, O, dO, lse, Dt, dOh, dOt, dqkv, dSt, None, dP, du, dv, B, H, T, Tpad, Rpad, 1, 1, 1)
WIN = None
if "--win" in sys.argv:
    i = sys.argv.index("--win")
    WIN = (sys.argv[i + 1] if i + 1 < len(sys.argv) else "100,256,full").split(",")


def tile_ratios(hw):
    """Visited / total (query block x 64-key tile) pairs per kernel for one half width: the arithmetic of relpos_attention.hip."""
    nt = (T + 63) // 64
    lo = lambda I0: max(I0 - hw, 0) >> 6
    hi = lambda I0, QB: min(I0 + QB - 2 + hw, T - 1) >> 6
    out = {}
    nq = (T + 255) // 256       # forward: 256-query workgroups walk [lo, hi]; a wave (16 queries) computes the tiles its own band meets
    out["fwd walk"] = sum(hi(256 * x, 256) - lo(256 * x) + 1 for x in range(nq)) / (nq * nt)
    waves = [q0 for q0 in range(0, T, 16)]
    out["fwd wave arithmetic"] = sum(sum(1 for t in range(nt) if 64 * t + 63 >= q0 - hw and 64 * t < q0 + 15 + hw) for q0 in waves) / (len(waves) * nt)
    nb = (T + 127) // 128
    out["dQ"] = sum(hi(128 * x, 128) - lo(128 * x) + 1 for x in range(nb)) / (nb * nt)
    vis = lambda X, kt: lo(128 * X) <= kt <= hi(128 * X, 128)
    out["dK/dV stream (slab reads)"] = sum(sum(1 for t in range(nt) if vis(t >> 1, kt)) for kt in range(nt)) / (nt * nt)
    out["dK/dV recompute"] = sum((min(128 * x + 127 + hw, T - 1) >> 6) - (max(128 * x - hw + 1, 0) >> 6) + 1 for x in range(nb)) / (nb * nt)
    out["dP row blocks"] = sum(1 for R0 in range(0, Rpad, 64) if R0 - (T - 1) + 63 >= -hw and R0 - (T - 1) < hw) / (Rpad // 64)
    return out


if WIN is not None:
    import statistics
    ROUNDS, REPS = 7, 8
    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS): f()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / REPS * 1e3
    print(f"rel-pos attention, B={B} H={H} T={T} f16 operands; {ROUNDS} rounds x {REPS} launches, alternating unbanded / band; times in us")
    for wtxt in WIN:
        hwv = 2 * T if wtxt == "full" else int(wtxt) // 2
        hw = torch.full((H,), hwv, dtype=torch.int32, device=dev)
        print(f"--- W = {wtxt} (hw = {hwv}); visited / total tiles: " + ", ".join(f"{k} {v:.3f}" for k, v in tile_ratios(hwv).items()))
        fb = lambda: call("sed_relpos_attn_band_fwd", qu, qv, k, vt, P, O, None, lse, B, H, T, Tpad, Rpad, 1, 0, hw)
        bb = lambda: call("sed_relpos_attn_band_bwd", qu, qut, qv, qvt, k, kt, vb, P, Pt, O, dO, lse, Dt, dOh, dOt, dqkv, dSt, Pst, dP, du, dv, B, H, T, Tpad, Rpad, 1, 1, 1, hw)
        bbr = lambda: call("sed_relpos_attn_band_bwd", qu, qut, qv, qvt, k, kt, vb, P, Pt, O, dO, lse, Dt, dOh, dOt, dqkv, dSt, None, dP, du, dv, B, H, T, Tpad, Rpad, 1, 1, 1, hw)
        for name, f0, f1 in (("fwd", fwd, fb), ("bwd stream", bwd, bb), ("bwd recompute", bwd_rc, bbr)):
            f0(); f1(); torch.cuda.synchronize()      # warm-up of both forms at this shape
            t0, t1 = [], []
            for _ in range(ROUNDS):
                t0.append(timed(f0)); t1.append(timed(f1))
            m0, m1 = statistics.median(t0), statistics.median(t1)
            s0, s1 = (max(t0) - min(t0)) / m0, (max(t1) - min(t1)) / m1
            print(f"{name:14s} unbanded {m0:8.0f} (spread {100 * s0:4.1f} %)   band {m1:8.0f} (spread {100 * s1:4.1f} %)   band / unbanded {m1 / m0:.3f}")
        fwd()      # (leave O / LSE of the full window behind for the next W's unbanded backward)
    sys.exit(0)

for name, f in (("fwd", fwd), ("bwd (dK / dV streamed from the stored slabs)", bwd), ("bwd (dK / dV recomputed)", bwd_rc)):
    f(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3): f()
    e1.record(); torch.cuda.synchronize()
    print(f"relpos {name}: {e0.elapsed_time(e1) / 3 * 1e3:.0f} us")
