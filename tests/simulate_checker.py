"""CPU checker of the draws from the fitted model (csrc/edsim.inc, csrc/ed_philox.hpp): Philox4x32-10 and the uniform in
plain Python integers; the draw as the 40-digit quantile checker's cut; how a device draw is judged in probability space; the uniforms the
GPU test plants on the walk's edges; the host loop false_calls_per_sample is held to; and the planted case the pipeline test calls.

For a size n, shapes (a, b) and a uniform u the draw is the smallest x in 0 .. n with C(x) > u (C the running sum of the masses), n when
nothing crosses, 0 for n = 0: quantile_checker.cut at p = u.
"""
import mpmath as mp
import numpy as np

import quantile_checker as qc

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xffffffff
STREAM_NULL, STREAM_PLANTED = 0, 1
_SCIPY_CDF = {}

KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def philox4x32_10(counter, key):
    """the published definition: ten rounds of (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key bumped between them"""
    c0, c1, c2, c3 = (int(v) & MASK for v in counter)
    k0, k1 = (int(v) & MASK for v in key)
    for r in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def u53_of(k):
    """(2 k + 1) 2^-53 of 52 bits: exact in binary64"""
    return float(2 * int(k) + 1) * 2.0 ** -53


def u53(seed, exon, sample, replicate, stream=0):
    seed = int(seed)
    w = philox4x32_10((exon, sample, replicate, stream), (seed & MASK, seed >> 32))
    return u53_of(((w[0] >> 12) << 32) | w[1])


def u53_many(seed, exon, sample, replicate, stream=0):
    ex, sa, re = np.broadcast_arrays(np.asarray(exon, dtype=np.uint64), np.asarray(sample, dtype=np.uint64), np.asarray(replicate, dtype=np.uint64))
    return np.array([u53(seed, int(e), int(s), int(r), stream) for e, s, r in zip(ex.ravel(), sa.ravel(), re.ravel())]).reshape(ex.shape)


shapes = qc.shapes


def planted_prob(expected, ratio):
    """e c / (e c + 1 - e) in binary64, left to right: the caller's own odds rule"""
    e, c = np.float64(expected), np.float64(ratio)
    return float(e * c / (e * c + np.float64(1) - e))


def draw(n, a, b, u):
    """the smallest x with C(x) > u at 40 digits; n where nothing crosses; 0 for n = 0"""
    n = int(n)
    if n == 0:
        return 0
    x = qc.cut(n, a, b, u)
    return n if x is None else x


def C_at(n, a, b, x):
    """C(x) as mpf, 0 for x = -1"""
    return qc.below(n, a, b, x + 1) if x < int(n) else qc.dist(n, a, b)[1][-1]


def bar_at(n, a, b, x):
    return qc.bar(n, x, qc.log_mass_span(n, a, b, x + 4))


def judge(x, n, a, b, u):
    """A device draw x for the uniform u.  It is right if and only if C(x - 1) <= u + bar and (C(x) >= u - bar or x = n), bar =
    quantile_checker.bar(n, x, span) from the walk's own operations.  Returns (the deviation as a share of the bar -- at most 1 for a
    right draw, 0 where x is the checker's own draw --, the bar)."""
    n, x = int(n), int(x)
    assert 0 <= x <= n, (x, n)
    if n == 0:
        return 0.0, 0.0
    tol = bar_at(n, a, b, x)
    with mp.workdps(qc.DPS):
        uu = mp.mpf(float(u))
        dev = max(C_at(n, a, b, x - 1) - uu, mp.mpf(0))
        if x < n:
            dev = max(dev, uu - C_at(n, a, b, x))
        return float(dev) / tol, tol


def step_distance(n, a, b, u):
    """how far u stands from the nearest step of C (a value C(x), x < n), and the bar of the draw there: inside the bar a float64 walk may
    name either neighbour"""
    n = int(n)
    if n == 0:
        return float("inf"), 0.0
    x = draw(n, a, b, u)
    with mp.workdps(qc.DPS):
        uu = mp.mpf(float(u))
        d = [abs(C_at(n, a, b, v) - uu) for v in (x - 1, x) if 0 <= v < n]
        return (float(min(d)) if d else float("inf")), bar_at(n, a, b, x)


def scipy_draw(n, a, b, u):
    """inversion of scipy.stats.betabinom.cdf in float64"""
    from scipy.stats import betabinom
    n = int(n)
    if n == 0:
        return 0
    key = (n, float(a), float(b))
    if key not in _SCIPY_CDF:                                   # (a distribution serves every uniform asked of it)
        _SCIPY_CDF[key] = betabinom.cdf(np.arange(n + 1), n, a, b)
    cdf = _SCIPY_CDF[key]
    above = np.flatnonzero(cdf > u)
    return int(above[0]) if above.size else n


def planted_uniforms(n, a, b):
    """[(name, u, the values a right draw may name)]: uniforms put by this checker where the walk has an edge.  C(x) +- 4 bar at x = 0, 255,
    256, n - 1 (the far side of a step: below it the draw is x, above it x + 1); two in one value; adjacent values of one lane and of two
    lanes; the smallest and the largest uniform the generator makes."""
    n = int(n)
    out = [("smallest", 2.0 ** -53, None), ("largest", 1.0 - 2.0 ** -53, None)]
    if n == 0:
        return out
    pm, C = qc.dist(n, a, b)
    with mp.workdps(qc.DPS):
        for x in sorted({0, 255, 256, n - 1}):
            if not 0 <= x < n:
                continue
            for sign in (-1, 1):
                u = float(C[x] + sign * 4 * bar_at(n, a, b, x))
                if 0.0 < u < 1.0:
                    out.append(("C(%d) %+d bar" % (x, 4 * sign), u, None))

        def mid(x, t=0.5):
            return float(qc.below(n, a, b, x) + t * pm[x])

        if n >= 8:
            x0 = min(max(draw(n, a, b, 0.5), 5), n - 2)         # a value with mass to stand in, by the median
            l0 = 4 * (x0 // 4)                                  # the first value of its lane
            out += [("two in one value", mid(x0, 0.25), None), ("two in one value", mid(x0, 0.75), None),
                    ("adjacent values of one lane", mid(l0), None), ("adjacent values of one lane", mid(l0 + 1), None),
                    ("adjacent values of two lanes", mid(l0 - 1), None), ("adjacent values of two lanes", mid(l0), None)]
    return [(name, u, None) for name, u, _ in out if 0.0 <= u < 1.0]


def false_calls_loop(bf, null_bf, n_null_samples, kind=None, null_kind=None):
    """false_calls_per_sample as a double loop"""
    out = []
    for i, v in enumerate(bf):
        if v != v:
            out.append(float("nan"))
            continue
        k = 0
        for j, w in enumerate(null_bf):
            if kind is not None and null_kind[j] != kind[i]:
                continue
            if w >= v:
                k += 1
        out.append(k / float(n_null_samples))
    return np.array(out, dtype=np.float64)


# ---- the planted case of the pipeline test ------------------------------------------------------------------------------------
# The seed is the first one tried.  With the input first written (phi 0.003 .. 0.005, expected 0.10 .. 0.13: an exon of the row stands
# 2.5 to 3 standard deviations from normal) the checker's own table called the row in every replicate but left an edge exon out in one of
# them -- (40, 50) or (41, 51) -- at this seed and at the nine after it.  The input was changed, not the assertion: phi 0.0005 .. 0.001 and
# expected 0.19 .. 0.22 put every exon of the row more than 5 standard deviations away, and the table then names exactly 40 .. 51 in every
# replicate at this seed; no uniform of the input lies within a bar of a step (the nearest is 6e5 bars away).
PLANT_SEED = 20240611
PLANT_REPLICATES = 3
PLANT_RATIO = 0.5
PLANT_FIRST, PLANT_LAST = 40, 51            # a 12-exon row
PLANT_SAMPLES = (0, 2, 3, 5)                # four of six samples


def planted_case():
    """(chrom_off, start, end, test, ref, phi, expected, rows): 96 exons of one chromosome at totals near 900, six samples; a 12-exon row
    planted at ratio 0.5 in four of them"""
    E, S = 96, 6
    rng = np.random.default_rng(5)
    chrom_off = np.array([0, E], dtype=np.int32)
    start = (10000 + 2000 * np.arange(E)).astype(np.int32)
    end = (start + 150).astype(np.int32)
    total = rng.integers(880, 921, size=(E, S)).astype(np.int32)
    phi = np.array([0.0005, 0.0008, 0.0005, 0.001, 0.0008, 0.0005])
    expected = np.array([0.20, 0.21, 0.19, 0.20, 0.22, 0.21])
    test = np.round(total * expected[None, :]).astype(np.int32)
    ref = (total - test).astype(np.int32)
    rows = np.zeros(len(PLANT_SAMPLES), dtype=[("sample", "<i4"), ("chrom", "<i4"), ("start_exon", "<i4"), ("end_exon", "<i4")])
    rows["sample"], rows["start_exon"], rows["end_exon"] = PLANT_SAMPLES, PLANT_FIRST, PLANT_LAST
    return chrom_off, start, end, test, ref, phi, expected, rows


def planted_draws(case, seed, replicate, samples):
    """the checker's draws of the case's cells for `samples`: {sample: (test* [E], uniforms [E], shapes per exon)}; planted cells on
    stream 1 at the shifted proportion, the others on stream 0"""
    chrom_off, start, end, test, ref, phi, expected, rows = case
    E = test.shape[0]
    out = {}
    for s in samples:
        a0, b0 = shapes(phi[s], expected[s])
        a1, b1 = shapes(phi[s], planted_prob(expected[s], PLANT_RATIO))
        planted = s in set(int(v) for v in rows["sample"])
        xs, us, ab = [], [], []
        for e in range(E):
            inside = planted and PLANT_FIRST <= e <= PLANT_LAST
            a, b = (a1, b1) if inside else (a0, b0)
            u = u53(seed, e, s, replicate, STREAM_PLANTED if inside else STREAM_NULL)
            n = int(test[e, s]) + int(ref[e, s])
            xs.append(draw(n, a, b, u)); us.append(u); ab.append((a, b))
        out[s] = (np.array(xs, dtype=np.int32), np.array(us), ab)
    return out


def cpu_calls(case, oracle, seed, replicate, samples):
    """{sample: [(start_exon, end_exon, type)]}: the oracle's CallCNVs on the checker's draws at the case's own parameters (no refit);
    and the smallest distance of a uniform from a step as a share of its bar"""
    chrom_off, start, end, test, ref, phi, expected, rows = case
    draws = planted_draws(case, seed, replicate, samples)
    calls, nearest = {}, float("inf")
    for s in samples:
        xs, us, ab = draws[s]
        total = (test[:, s] + ref[:, s]).astype(np.int32)
        L, _ = oracle.get_loglike_matrix(phi[s], expected[s], total, xs, 1.0, oracle.PORTABLE)
        _, c = oracle.callcnvs(L, chrom_off, start, end)
        calls[s] = [(int(r[0]) - 1, int(r[1]) - 1, int(r[2])) for r in c]
        for e in range(len(xs)):
            d, tol = step_distance(int(total[e]), ab[e][0], ab[e][1], us[e])
            nearest = min(nearest, d / tol)
    return calls, nearest
