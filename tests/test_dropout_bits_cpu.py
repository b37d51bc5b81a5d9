"""Properties of the host restatement of the dropout bit generators (tests/dropout_cases.py).  tests/test_gpu_dropout_bits.py demands bit
equality of the kernels with it, so the statistics are proven once, here, without a GPU; they are deterministic for the fixed inputs.

Every bound is 5 sigma of the statistic under independent Bernoulli(1 - thr / 65536) draws.  Worst values this case list produces
(n = 2^20; p in {0.1, 0.25, 0.5}):
  dasm_keep  rate 2.12, single field 2.94, lag 3.62 (lag 4), cross 3.63 (861 pairs per p)      over 7 seeds x 5 sites (cross: x 6 sites)
  pmam_keep  rate 2.65, single field 3.15, lag 2.31, cross 1.90 (21 pairs per p)              over 7 seeds
  thresholds 1 and 65535: 1.75
Each test prints the worst value of its families and where it occurred (pytest -s)."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dropout_cases as X  # noqa: E402

BOUND = 5.0


def report(family, z, what):
    print(f"{family}: worst {z:.2f} sigma at {what}")


def q_of(p):
    return 1.0 - X.thr16(p) / 65536.0


def test_thresholds_scale_and_case_lists_cover_every_listed_value():
    assert [X.thr16(p) for p in X.P_VALUES] == [6554, 16384, 32768, 1, 65535, 0]
    assert X.thr16(0.0) == 0 and X.thr16(-1.0) == 0
    assert X.scale(0.5) == np.float32(2.0) and X.scale(0.0) == np.float32(1.0) and X.scale(0.1).dtype == np.float32
    assert X.scale(0.1) == np.float32(1.0) / np.float32(0.9)
    for col, values in enumerate((X.N_VALUES, X.P_VALUES, X.SEEDS, X.SITES)):
        assert {c[col] for c in X.DASM_BIT_CASES} == set(values), col
    assert all(n % 4 == 0 for n, _, _ in X.PMAM_BIT_CASES) and (1 << 62) - 1 in {s for _, _, s in X.PMAM_BIT_CASES}
    assert {n for n, _, _ in X.PMAM_BIT_CASES} == {4, 1000, (1 << 22) + 4}


def test_known_hash_values():
    """The finaliser against splitmix64's published first outputs for the seed 1234567 (z0 = seed + k * golden gamma), and one element
    of each generator worked out with Python integers."""
    z0 = (np.uint64(1234567) + np.arange(1, 4, dtype=np.uint64) * np.uint64(X.GOLDEN_GAMMA))
    assert [int(v) for v in X.finalise(z0)] == [6457827717110365317, 3203168211198807973, 9817491932198370423]

    def fin(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & X.MASK64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & X.MASK64
        return z ^ (z >> 31)
    for seed, site, idx in ((0, 0, 0), (-1, 255, 1001), ((1 << 62) - 1, 13, (1 << 21) + 4), (0x0123456789ABCDEF, 8, 7)):
        z = fin(((idx >> 2) + ((seed & X.MASK64) ^ (site << 48)) * X.GOLDEN_GAMMA + X.SITE_GAMMA * (site + 1)) & X.MASK64)
        assert int(X.dasm_fields(1, seed, site, start=idx)[0]) == (z >> (16 * (idx & 3))) & 0xFFFF
        z = fin(((seed & X.MASK64) + (idx // 4 + 1) * X.GOLDEN_GAMMA) & X.MASK64)
        assert int(X.pmam_fields(idx + 1, seed)[idx]) == (z >> (16 * (idx & 3))) & 0xFFFF


def test_threshold_zero_keeps_everything_and_extreme_thresholds_hit_their_rates():
    n = X.STAT_N
    for seed, site in ((0, 0), (-1, 13), (424242, 5)):
        assert int(X.dasm_keep(n, X.P_THR0, seed, site).min()) == 1 and int(X.dasm_keep(n, 0.0, seed, site).min()) == 1
        assert int(X.pmam_keep(n, X.P_THR0, seed).min()) == 1
    worst = 0.0
    # thresholds 1 and 65535: expected drop / keep counts of 16 in 2^20 -- pooled over the seeds and sites of the statistics below (7 x 5
    # masks, 560 expected) so that the 5 sigma band is a band around a Gaussian, not around a count of 16
    for p, q in ((X.P_THR1, 1.0 - 2.0 ** -16), (X.P_THR65535, 2.0 ** -16)):
        assert q_of(p) == q
        pooled = np.concatenate([X.stat_dasm_fields(seed, site) >= X.thr16(p) for seed in X.SEEDS for site in X.STAT_SITES])
        z = X.z_rate(pooled, q)
        worst = max(worst, z)
        assert z < BOUND, ("dasm", p, z)
        pooled = np.concatenate([X.stat_pmam_fields(seed) >= X.thr16(p) for seed in X.SEEDS])
        z = X.z_rate(pooled, q)
        worst = max(worst, z)
        assert z < BOUND, ("pmam", p, z)
        for seed in X.SEEDS:                       # and each mask on its own
            z = X.z_rate(X.stat_dasm_fields(seed, 0) >= X.thr16(p), q)
            worst = max(worst, z)
            assert z < BOUND, ("dasm", p, seed, z)
    report("extreme thresholds", worst, "thr 1 / 65535")


def test_start_is_honoured():
    for n, s, p, seed, site in ((1000, 0, 0.25, 1, 5), (1000, 4, 0.1, 424242, 0), (257, 3, 0.5, -1, 13), (5, 1001, 0.5, (1 << 62) - 1, 8),
                                (64, (1 << 21) + 2, 0.25, 0x0123456789ABCDEF, 255), (1, 2, 0.5, 2, 1)):
        assert np.array_equal(X.dasm_keep(n, p, seed, site, start=s), X.dasm_keep(s + n, p, seed, site)[s:]), (n, s)


@pytest.mark.parametrize("p", X.P_ORDINARY)
def test_dasm_keep_rate_fields_and_lags(p):
    thr, q = X.thr16(p), q_of(p)
    worst = {"rate": (0.0, None), "field": (0.0, None), "lag": (0.0, None)}
    for seed, site in itertools.product(X.SEEDS, X.STAT_SITES):
        k = (X.stat_dasm_fields(seed, site) >= thr).astype(np.uint8)
        zs = [("rate", X.z_rate(k, q), (seed, site))]
        zs += [("field", X.z_rate(k[f::4], q), (seed, site, f)) for f in range(4)]
        zs += [("lag", X.z_lag(k, q, lag), (seed, site, lag)) for lag in X.LAGS]
        for fam, z, what in zs:
            if z > worst[fam][0]:
                worst[fam] = (z, what)
    for fam, (z, what) in worst.items():
        report(f"dasm_keep p={p} {fam}", z, what)
    for fam, (z, what) in worst.items():
        assert z < BOUND, (fam, p, what, z)


@pytest.mark.parametrize("p", X.P_ORDINARY)
def test_dasm_keep_cross_correlation_between_seeds_and_sites(p):
    """Every two distinct (seed, site) of 7 seeds x 6 sites: what breaks if `site` or the high seed bits stop reaching the hash."""
    thr, q = X.thr16(p), q_of(p)
    keys = list(itertools.product(X.SEEDS, X.CROSS_SITES))
    z = X.z_cross(np.stack([X.stat_dasm_fields(seed, site) >= thr for seed, site in keys]), q)
    iu = np.triu_indices(len(keys), 1)
    w = int(np.argmax(z[iu]))
    report(f"dasm_keep p={p} cross ({iu[0].size} pairs)", float(z[iu][w]), (keys[iu[0][w]], keys[iu[1][w]]))
    assert float(z[iu].max()) < BOUND, (p, keys[iu[0][w]], keys[iu[1][w]], float(z[iu][w]))


@pytest.mark.parametrize("p", X.P_ORDINARY)
def test_pmam_keep_rate_fields_lags_and_cross_correlation(p):
    thr, q = X.thr16(p), q_of(p)
    worst = {"rate": (0.0, None), "field": (0.0, None), "lag": (0.0, None)}
    for seed in X.SEEDS:
        k = (X.stat_pmam_fields(seed) >= thr).astype(np.uint8)
        zs = [("rate", X.z_rate(k, q), seed)]
        zs += [("field", X.z_rate(k[f::4], q), (seed, f)) for f in range(4)]
        zs += [("lag", X.z_lag(k, q, lag), (seed, lag)) for lag in X.LAGS]
        for fam, z, what in zs:
            if z > worst[fam][0]:
                worst[fam] = (z, what)
    z = X.z_cross(np.stack([X.stat_pmam_fields(seed) >= thr for seed in X.SEEDS]), q)
    iu = np.triu_indices(len(X.SEEDS), 1)
    w = int(np.argmax(z[iu]))
    worst["cross"] = (float(z[iu][w]), (X.SEEDS[iu[0][w]], X.SEEDS[iu[1][w]]))
    for fam, (zz, what) in worst.items():
        report(f"pmam_keep p={p} {fam}", zz, what)
    for fam, (zz, what) in worst.items():
        assert zz < BOUND, (fam, p, what, zz)
