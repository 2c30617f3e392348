"""CPU checker of the quantile map (csrc/edquant.inc): qbetabinom.ab of the reference (R/tools.R:42-53) in mpmath at 40 digits, by a walk
from x = 0 and by the direct definition from log-gamma; a plain float64 scipy restatement of the same function; the bin rule of
csrc/ed_quant_plan.hpp; the bar of the device's walk and the cases the GPU test plants on the walk's edges.

For a size n, shapes (a, b) and a probability p: pm[x] = the beta-binomial mass at x = 0 .. n, C(x) = pm[0] + .. + pm[x], cut = the smallest
x with C(x) > p,
    q = cut + (p - C(cut - 1)) / pm[cut]     (C(-1) = 0)          below = C(cut - 1)
and NaN (R's NA) when no x has C(x) > p.  q inverts G(q) = C(x - 1) + (q - x) pm[x], x < q <= x + 1, which is continuous in the masses:
|G(q') - p| measures a q' in probability space, with no threshold to excuse.
The shapes of (phi, prob) are formed in binary64 in qbetabinom's operation order (R/tools.R:22-23): those doubles ARE the model; everything
behind them runs at 40 digits.
"""
import math

import mpmath as mp
import numpy as np

from power_checker import region_sum  # noqa: F401  (the order of a region's sums is the power map's)

DPS = 40
U = 2.0 ** -53
_DIST, _SPAN = {}, {}


def shapes(phi, prob):
    """(a, b) of qbetabinom(., ., phi, prob) in binary64: prob * (1 - phi) / phi, (1 - prob) * (1 - phi) / phi, left to right"""
    phi, prob = np.float64(phi), np.float64(prob)
    with np.errstate(all="ignore"):
        return float(prob * (np.float64(1.0) - phi) / phi), float((np.float64(1.0) - prob) * (np.float64(1.0) - phi) / phi)


def _lnbeta(a, b):
    return mp.loggamma(a) + mp.loggamma(b) - mp.loggamma(a + b)


def dist(n, a, b, direct=False):
    """(pm, C): lists of the masses and their running sums at x = 0 .. n (mpf).  direct: every mass from loggamma, as the definition reads;
    else walked from x = 0 by exact step ratios at 40 digits.  Cached: a distribution serves every probability asked of it."""
    key = (int(n), float(a), float(b), bool(direct))
    if key not in _DIST:
        with mp.workdps(DPS):
            n, a, b = int(n), mp.mpf(float(a)), mp.mpf(float(b))
            if direct:
                l0 = _lnbeta(a, b)
                pm = [mp.exp(mp.log(mp.binomial(n, x)) + _lnbeta(a + x, b + n - x) - l0) for x in range(n + 1)]
            else:
                pm = [mp.exp(_lnbeta(a, b + n) - _lnbeta(a, b))]
                for x in range(n):
                    pm.append(pm[-1] * ((n - x) * (a + x)) / ((x + 1) * (b + (n - x - 1))))
            C, s = [], mp.mpf(0)
            for v in pm:
                s += v
                C.append(s)
        _DIST[key] = (pm, C)
    return _DIST[key]


def cut(n, a, b, p, direct=False):
    """the smallest x with C(x) > p, None when there is none: p >= 1 (C(n) = 1 exactly; its 40-digit sum is not asked) or NaN"""
    if not p < 1.0:
        return None
    _, C = dist(n, a, b, direct)
    with mp.workdps(DPS):
        p = mp.mpf(float(p))
        if not C[-1] > p:
            return None
        lo, hi = 0, len(C) - 1              # C ascends: bisect for the first C(x) > p
        while lo < hi:
            mid = (lo + hi) // 2
            if C[mid] > p:
                hi = mid
            else:
                lo = mid + 1
        return lo


def below(n, a, b, x, direct=False):
    """C(x - 1), 0 for x = 0"""
    return dist(n, a, b, direct)[1][x - 1] if x > 0 else mp.mpf(0)


def quantile(n, a, b, p, direct=False):
    """(q, below, cut) as mpf, mpf, int; (None, None, None) where nothing crosses.  n = 0: pm = [1], q = p."""
    x = cut(n, a, b, p, direct)
    if x is None:
        return None, None, None
    pm, _ = dist(n, a, b, direct)
    with mp.workdps(DPS):
        bl = below(n, a, b, x, direct)
        return x + (mp.mpf(float(p)) - bl) / pm[x], bl, x


def G(q, n, a, b, direct=False):
    """the piecewise-linear function q inverts, at any real q: C(x - 1) + (q - x) pm[x] with x = ceil(q) - 1 kept inside 0 .. n"""
    pm, _ = dist(n, a, b, direct)
    with mp.workdps(DPS):
        q = mp.mpf(float(q))
        x = min(max(int(mp.ceil(q)) - 1, 0), int(n))
        return below(n, a, b, x, direct) + (q - x) * pm[x]


def log_mass_span(n, a, b, upto):
    """the largest |log pm[x]| over x = 0 .. min(upto, n): what the walk's log-domain carry has to hold on the way to `upto`"""
    key = (int(n), float(a), float(b))
    if key not in _SPAN:
        pm, _ = dist(n, a, b)
        with mp.workdps(DPS):
            _SPAN[key] = np.maximum.accumulate([abs(float(mp.log(v))) for v in pm])
    return float(_SPAN[key][min(max(int(upto), 0), int(n))])


def bar(n, x, span):
    """The bound on the device walk's error in probability space at a crossing at x of a size n, span = log_mass_span(n, a, b, x + 4)
    (from the walk's own operations, u = 2^-53):
      a step ratio is 4 rounded operations on 2 rounded sums and one reciprocal (2u): 7u; a product of four and its logarithm: 32u,
      8u per value, over the n values of L(0) and the x values walked; the sums of logarithms -- n / 256 per lane and 6 folds for L(0), a
      scan of 6, a carry and a base per tile walked -- each round a partial sum no larger than span, 16 u span per tile generously;
      that is the error d of a lane's log-mass, hence the relative error of its exp (+ 2u) times its product of ratios (+ 12u) = a mass;
      C adds masses: a relative d + 16u, and x / 256 + 16 rounded sums of numbers <= 1;
      q adds (p - below) / mass: below's error once, the mass's relative error on a share of the mass <= 1 once more.
    """
    n, x = float(n), float(x)
    d = 8.0 * U * (n + x + 8.0) + U * span * (n / 256.0 + 8.0 + 16.0 * (x / 256.0 + 1.0))
    return 2.0 * (d + 16.0 * U) + (x / 256.0 + 16.0) * U


def scipy_qbetabinom_ab(p, size, shape1, shape2):
    """qbetabinom.ab line by line in float64 with scipy's betaln / gammaln for dbetabinom.ab; NaN for R's NA"""
    from scipy.special import betaln, gammaln
    n = int(size)
    x = np.arange(n + 1, dtype=np.float64)
    pm = np.exp(gammaln(n + 1.0) - gammaln(x + 1.0) - gammaln(n - x + 1.0) + betaln(shape1 + x, shape2 + n - x) - betaln(shape1, shape2))
    cs = np.cumsum(pm)
    above = np.flatnonzero(cs > p)
    if above.size == 0:
        return float("nan")
    k = int(above[0])                       # 0-based: R's `above` - 1
    return float(k + (p - cs[k - 1]) / pm[k]) if k > 0 else float(p / pm[0])


NO_CUT = 2 ** 63 - 1


def cut_of(q):
    """csrc/ed_quant_plan.hpp cut_of: ceil(q) - 1 for q > 0, 0 at and below 0, NO_CUT for NaN"""
    if q != q:
        return NO_CUT
    return max(int(math.ceil(q)) - 1, 0)


def bin_of(obs, cuts):
    """the number of cuts at or below obs: bins closed below"""
    return sum(1 for c in cuts if obs >= c)


def judge(q_dev, below_dev, n, a, b, p):
    """A device result against the definition, threshold-free.  Returns (fraction of the bar used, the bar).
    q: |G(q_dev) - p|.  below: it must be C(x - 1) of a value x that is a cut within the bar -- C(x - 1) <= p + bar and C(x) >= p - bar --
    among the value q_dev lies in and its two neighbours (next to a tie q_dev may stand on either side of a whole number; then two values
    qualify, and only then).  NaN claims that nothing crosses, C(n) <= p: wrong by 1 - p, which must lie within the bar as well."""
    n = int(n)
    pm, C = dist(n, a, b)
    with mp.workdps(DPS):
        pq = mp.mpf(float(p))
        if below_dev is None:                    # (a surface that gives q alone)
            if q_dev == q_dev:
                x0 = cut_of(q_dev)
                tol = bar(n, min(x0, n), log_mass_span(n, a, b, x0 + 4))
                return float(abs(G(q_dev, n, a, b) - pq)) / tol, tol
            below_dev = q_dev
        if q_dev != q_dev or below_dev != below_dev:
            assert q_dev != q_dev and below_dev != below_dev, "NaN in one of the two only"
            tol = bar(n, n, log_mass_span(n, a, b, n))
            return float(1 - pq) / tol, tol
        x0 = cut_of(q_dev)
        tol = bar(n, min(x0, n), log_mass_span(n, a, b, x0 + 4))
        used = abs(G(q_dev, n, a, b) - pq)
        best = None
        for x in (x0 - 1, x0, x0 + 1):
            if 0 <= x <= n and below(n, a, b, x) <= pq + tol and C[x] >= pq - tol:
                e = abs(mp.mpf(float(below_dev)) - below(n, a, b, x))
                best = e if best is None else min(best, e)
        assert best is not None, "q = %r names no value that is a cut of p = %r within the bar" % (q_dev, p)
        return float(max(used, best)) / tol, tol


def planted_cases():
    """[(name, n, phi, prob, probs, cuts)]: probabilities put by this checker where the walk has an edge; cuts[k] is where probs[k] crosses
    (None: nowhere).  Every probability stands in the middle (or at the quarters) of its cell, a margin of a quarter of a mass or more."""
    out = []

    def mid(n, phi, prob, x, t=0.5):
        a, b = shapes(phi, prob)
        pm, _ = dist(n, a, b)
        with mp.workdps(DPS):
            return float(below(n, a, b, x) + t * pm[x])

    out.append(("crossing at 0: p / pm[0]", 5, 0.2, 0.05, [mid(5, 0.2, 0.05, 0)], [0]))
    out.append(("last value of the first tile", 600, 0.003, 0.4, [mid(600, 0.003, 0.4, 255)], [255]))
    out.append(("first value of the second tile", 600, 0.003, 0.4, [mid(600, 0.003, 0.4, 256)], [256]))
    out.append(("crossing at n", 5, 0.2, 0.4, [mid(5, 0.2, 0.4, 5)], [5]))
    out.append(("crossing at n, the first value of a tile", 256, 0.2, 0.4, [mid(256, 0.2, 0.4, 256)], [256]))
    out.append(("a probability far below a small pm[0]", 600, 0.05, 0.05, [mid(600, 0.05, 0.05, 0, 1e-3)], [0]))
    out.append(("two in one cell", 257, 0.05, 0.11, [mid(257, 0.05, 0.11, 30, 0.25), mid(257, 0.05, 0.11, 30, 0.75)], [30, 30]))
    out.append(("two in adjacent values of one lane", 257, 0.05, 0.11, [mid(257, 0.05, 0.11, 29), mid(257, 0.05, 0.11, 30)], [29, 30]))
    out.append(("adjacent values of two lanes", 257, 0.05, 0.11, [mid(257, 0.05, 0.11, 27), mid(257, 0.05, 0.11, 28)], [27, 28]))
    # the largest double below 1: in exact arithmetic C(n) = 1 crosses it at n; a float64 sum may or may not (judge takes either for what it is)
    out.append(("within rounding of 1, beside one that crosses", 17, 0.05, 0.4, [mid(17, 0.05, 0.4, 7), 1.0 - 2.0 ** -53], [7, 17]))
    return out


def margin(n, a, b, p, x):
    """how far p stands from the ends of the cell of x, in probability: min(p - C(x - 1), C(x) - p)"""
    _, C = dist(n, a, b)
    with mp.workdps(DPS):
        return float(min(mp.mpf(float(p)) - below(n, a, b, x), C[x] - mp.mpf(float(p))))
