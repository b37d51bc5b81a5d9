"""The two counter-based dropout bit generators, restated on the host in numpy uint64 from their definitions, and the case lists the
CPU and the GPU tests share (pure construction helpers; no tests here).

`dasm_keep`  csrc/dasm.hip (drop_hash4 / drop_keep): keep(seed, site, element index), evaluated -- never stored -- by sed_gemm_f32's
             epilogue, sed_xattn_f32_fwd_train, sed_xattn_f32_bwd, sed_gelu_bwd_f32, sed_dropout_f32 and sed_act_drop_res_f32.
               thr  = 0 if p <= 0 else int(fp32(p) * 65536 + 0.5)                      (fp32 arithmetic)
               z0   = (idx >> 2) + (seed ^ (site << 48)) * 0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03 * (site + 1)       mod 2^64
               z    = splitmix64 finaliser of z0
               keep = ((z >> 16 (idx & 3)) & 0xffff) >= thr
`pmam_keep`  csrc/cnn_branch.hip (dropout_mask_kernel behind sed_dropout_mask): z0 = seed + (idx // 4 + 1) * 0x9E3779B97F4A7C15, the same
             finaliser, field choice and threshold.

One hash serves four consecutive elements (its four 16-bit fields), so what can go wrong without any consumer noticing is: fields that
are correlated, a `site` or high seed bits that do not reach the hash, a threshold off by a power of two.  tests/test_dropout_bits_cpu.py
proves the statistics on this restatement; tests/test_gpu_dropout_bits.py demands bit equality of the kernels with it."""
import functools

import numpy as np

U64 = np.uint64
MASK64 = (1 << 64) - 1
GOLDEN_GAMMA = 0x9E3779B97F4A7C15
SITE_GAMMA = 0xD1B54A32D192ED03


# ------------------------------------------------------------------------------------------------ the generators
def thr16(p):
    """16-bit threshold of a drop probability: a 16-bit field below it drops its element."""
    if p <= 0:
        return 0
    return int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))


def scale(p):
    """What a kept element is multiplied by, as the kernels form it: one fp32 division."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def finalise(z):
    """splitmix64's output function on a uint64 array."""
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def fields_of(z, first, n):
    """The 16-bit fields of the hashes z (one per element quad) as a flat uint16 array: elements first .. first + n - 1 of the quads."""
    f = np.empty((z.shape[0], 4), dtype=np.uint16)
    for i in range(4):
        f[:, i] = ((z >> U64(16 * i)) & U64(0xFFFF)).astype(np.uint16)
    return f.reshape(-1)[first:first + n]


def dasm_fields(n, seed, site, start=0):
    """uint16[n]: the field each of the elements start .. start + n - 1 compares with the threshold."""
    q0, q1 = start >> 2, (start + n + 3) >> 2
    key = (((seed & MASK64) ^ ((site << 48) & MASK64)) * GOLDEN_GAMMA + SITE_GAMMA * (site + 1)) & MASK64
    with np.errstate(over="ignore"):
        z = finalise(np.arange(q0, q1, dtype=U64) + U64(key))
    return fields_of(z, start - 4 * q0, n)


def dasm_keep(n, p, seed, site, start=0):
    """uint8[n]: 1 = kept.  `seed` any Python int (taken as two's-complement uint64), `start`: index of the first element."""
    return (dasm_fields(n, seed, site, start) >= thr16(p)).astype(np.uint8)


def pmam_fields(n, seed):
    with np.errstate(over="ignore"):
        z = finalise(U64(seed & MASK64) + np.arange(1, (n + 3) // 4 + 1, dtype=U64) * U64(GOLDEN_GAMMA))
    return fields_of(z, 0, n)


def pmam_keep(n, p, seed):
    return (pmam_fields(n, seed) >= thr16(p)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ cases
N_VALUES = (1, 3, 4, 5, 255, 257, 1000, 1 << 20, (1 << 21) + 5)      # the last: sed_dropout_f32's grid (capped at 8192 x 256) wraps
P_ORDINARY = (0.1, 0.25, 0.5)
P_THR1, P_THR65535, P_THR0 = 2.0 ** -16, 1.0 - 2.0 ** -16, 7e-6      # thresholds 1, 65535 and 0 (keeps everything)
P_VALUES = P_ORDINARY + (P_THR1, P_THR65535, P_THR0)
SEEDS = (0, 1, 2, 424242, (1 << 62) - 1, 0x0123456789ABCDEF, -1)
SITES = (0, 1, 5, 8, 13, 255)

# (n, p, seed, site): a cross-section in which every value above appears at least once
DASM_BIT_CASES = (
    (1, 0.5, 0, 0),
    (3, 0.25, 1, 1),
    (4, 0.1, 2, 5),
    (5, 0.5, 424242, 8),
    (255, P_THR1, (1 << 62) - 1, 13),
    (257, P_THR65535, 0x0123456789ABCDEF, 255),
    (1000, P_THR0, -1, 0),
    (1000, 0.25, -1, 13),
    (1 << 20, 0.1, 0x0123456789ABCDEF, 1),
    (1 << 20, P_THR1, 1, 5),
    (1 << 20, P_THR65535, 424242, 255),
    ((1 << 21) + 5, 0.5, (1 << 62) - 1, 8),
    ((1 << 21) + 5, 0.1, 0, 13),
)
PMAM_BIT_CASES = (      # (n, p, seed); sed_dropout_mask refuses n % 4 != 0
    (4, 0.5, 0),
    (1000, 0.25, (1 << 62) - 1),
    (1000, P_THR65535, -1),
    ((1 << 22) + 4, 0.1, 0x0123456789ABCDEF),
    ((1 << 22) + 4, P_THR1, 424242),
)

# statistics (tests/test_dropout_bits_cpu.py)
STAT_N = 1 << 20
STAT_SITES = (0, 1, 5, 8, 13)
CROSS_SITES = (0, 1, 2, 8, 9, 13)
LAGS = (1, 2, 3, 4, 60, 300, 1188)      # 1 .. 3: the fields of one hash; 4: the next hash; the rest: key-row lengths Nk of the attention kernels


@functools.lru_cache(maxsize=None)
def stat_dasm_fields(seed, site):
    f = dasm_fields(STAT_N, seed, site)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def stat_pmam_fields(seed):
    f = pmam_fields(STAT_N, seed)
    f.setflags(write=False)
    return f


# ------------------------------------------------------------------------------------------------ statistics, in units of sigma
def z_rate(keep, q):
    """|observed keep rate - q| over the standard deviation of the mean of len(keep) Bernoulli(q) draws."""
    n = keep.shape[0]
    return abs(float(keep.mean(dtype=np.float64)) - q) / np.sqrt(q * (1.0 - q) / n)


def z_lag(keep, q, lag):
    """|normalised autocorrelation at `lag`| sqrt(n): the correlation of independent draws has standard deviation 1 / sqrt(n)."""
    x = keep.astype(np.float64) - q
    r = float(np.dot(x[:-lag], x[lag:])) / (x.shape[0] * q * (1.0 - q))
    return abs(r) * np.sqrt(x.shape[0])


def z_cross(keeps, q):
    """[m, m] matrix of |normalised cross-correlation| sqrt(n) between the rows of keeps [m, n] (uint8)."""
    k = np.asarray(keeps, dtype=np.float32)
    n = k.shape[1]
    both = (k @ k.T).astype(np.float64)          # co-occurrence counts: integers below 2^24, exact in fp32
    s = np.diag(both)
    cov = (both - q * (s[:, None] + s[None, :]) + n * q * q) / n
    return np.abs(cov) / (q * (1.0 - q)) * np.sqrt(n)
