"""CPU checker of the detection-power map (csrc/edpower.inc): the definitions of include/exomedepth_amd.h in mpmath at 40 digits, a plain
numpy / scipy form of the same, the region kernel's summation order and a long-double restatement of a region's price.

Sample (phi, expected, mixture): sd = sqrt((phi expected)(1 - expected)), (a1_j, a2_j) = shape_params(state_props(expected, mixture)[j], sd)
for j = deletion, normal, duplication -- formed in binary64 in the device's operation order, because these doubles ARE the model (the strict
emissions use the same ones); everything behind them runs at 40 digits.  For T in {deletion, duplication} and a total n:
    X ~ BetaBinomial(n, a1_T, a2_T)    D_T(x) = log10(e) [e_T(x) - e_N(x)]    e_j(x) = lnbeta(a1_j + x, a2_j + n - x) - lnbeta(a1_j, a2_j)
    mean_T = E[D_T(X)]    var_T = Var[D_T(X)]    abs_T = E|D_T(X)|    sq_T = E[D_T(X)^2]      (the last two scale the bars)
"""
import math

import mpmath as mp
import numpy as np

DPS = 40
STATES = ("del", "dup")
RTOL = 2e-10          # the walk's bar (test_get_power_betabinom_walk_against_mpmath), here on the absolute terms


def shape_params(phi, expected, mixture=1.0):
    """(a1 [3], a2 [3]) in binary64, states deletion, normal, duplication: csrc/edcore.hip state_props / shape_params, operation by operation"""
    phi, e, m = np.float64(phi), np.float64(expected), np.float64(mixture)
    with np.errstate(all="ignore"):
        sd = np.sqrt((phi * e) * (np.float64(1.0) - e))
        od, ou = np.float64(1.0) - np.float64(0.5) * m, np.float64(1.0) + np.float64(0.5) * m
        ep = [(e * od) / ((e * od + np.float64(1.0)) - e), e, (e * ou) / ((e * ou + np.float64(1.0)) - e)]
        a1 = [((p * p) * (np.float64(1.0) - p)) / (sd * sd) - p for p in ep]
        a2 = [((np.float64(1.0) - p) / p) * a for p, a in zip(ep, a1)]
    return np.array(a1, dtype=np.float64), np.array(a2, dtype=np.float64)


def in_model(a1, a2):
    return bool(np.all(np.isfinite(a1)) and np.all(np.isfinite(a2)) and np.all(a1 > 0) and np.all(a2 > 0))


def _lnbeta(a, b):
    return mp.loggamma(a) + mp.loggamma(b) - mp.loggamma(a + b)


def moments(n, phi, expected, mixture=1.0, direct=False):
    """dict of mean_T, var_T, abs_T, sq_T (floats; T = del, dup) of a total n.  direct: every term from loggamma, as the definition reads;
    else P and D are walked from x = 0 (exact step ratios at 40 digits), which is what makes totals of a thousand affordable."""
    a1f, a2f = shape_params(phi, expected, mixture)
    out = {}
    with mp.workdps(DPS):
        M = 1 / mp.log(10)
        n = int(n)
        aN, bN = mp.mpf(float(a1f[1])), mp.mpf(float(a2f[1]))
        for T, name in ((0, "del"), (2, "dup")):
            aT, bT = mp.mpf(float(a1f[T])), mp.mpf(float(a2f[T]))
            s1 = sa = s2 = mp.mpf(0)
            if direct:
                for x in range(n + 1):
                    eT = _lnbeta(aT + x, bT + n - x) - _lnbeta(aT, bT)
                    eN = _lnbeta(aN + x, bN + n - x) - _lnbeta(aN, bN)
                    P = mp.exp(mp.log(mp.binomial(n, x)) + eT)
                    D = M * (eT - eN)
                    s1 += P * D; sa += P * abs(D); s2 += P * D * D
            else:
                eT0 = _lnbeta(aT, bT + n) - _lnbeta(aT, bT)
                eN0 = _lnbeta(aN, bN + n) - _lnbeta(aN, bN)
                P, R = mp.exp(eT0), mp.exp(eT0 - eN0)          # P(x), exp(e_T(x) - e_N(x))
                for x in range(n + 1):
                    D = M * mp.log(R)
                    s1 += P * D; sa += P * abs(D); s2 += P * D * D
                    if x < n:
                        u, v, w, t = aT + x, bT + (n - x - 1), aN + x, bN + (n - x - 1)
                        P *= (n - x) * u / ((x + 1) * v)
                        R *= (u * t) / (w * v)
            out["mean_" + name], out["abs_" + name], out["sq_" + name] = float(s1), float(sa), float(s2)
            out["var_" + name] = float(s2 - s1 * s1)
    return out


def scipy_moments(n, phi, expected, mixture=1.0):
    """the same four moments by a plain numpy / scipy form (betaln, gammaln), binary64"""
    from scipy.special import betaln, gammaln
    a1, a2 = shape_params(phi, expected, mixture)
    x = np.arange(int(n) + 1, dtype=np.float64)
    e = [betaln(a1[j] + x, a2[j] + n - x) - betaln(a1[j], a2[j]) for j in range(3)]
    lch = gammaln(n + 1.0) - gammaln(x + 1.0) - gammaln(n - x + 1.0)
    out = {}
    for T, name in ((0, "del"), (2, "dup")):
        P = np.exp(lch + e[T])
        D = math.log10(math.e) * (e[T] - e[1])
        mean = float(np.sum(P * D))
        out["mean_" + name], out["var_" + name] = mean, float(np.sum(P * (D - mean) ** 2))
    return out


def region_sum(values, tile=64):
    """the sum of a run's values in the region kernel's order (csrc/ed_power_plan.hpp: region_sum): lane l of `tile` adds values l, l + tile,
    ... starting from +0.0; the lane sums are folded tile / 2, tile / 4, .., 1 apart.  binary64, operation by operation."""
    p = [np.float64(0.0)] * tile
    for i, v in enumerate(values):
        p[i % tile] = p[i % tile] + np.float64(v)
    d = tile // 2
    while d >= 1:
        for l in range(d):
            p[l] = p[l] + p[l + d]
        d //= 2
    return p[0]


def price(tr, a, b):
    """the price of the run a .. b (0-based, inside the chromosome) in long double; tr: that chromosome's entry of
    posterior_checker.transitions().  log10(e) (sum over the gaps a .. b + 1 of N->N - (N->T + sum over the gaps a + 1 .. b of T->T + T->N
    of gap b + 1))"""
    ld = np.longdouble
    stay = ld(b - a + 2) * ld(tr["c0"])
    call = ld(tr["c1"]) + np.sum(np.asarray(tr["B"][a + 1:b + 1], dtype=ld), dtype=ld) + ld(tr["A"][b + 1])
    return float((stay - call) / np.log(ld(10)))
