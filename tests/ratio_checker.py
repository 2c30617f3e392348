"""CPU checker of the copy-ratio profile (csrc/edratio.inc) and of call_copy_number's objective, in numpy.

Terms: the oracle's get_loglike_matrix at the PORTABLE flavour and mixture |mu| -- the strict mode's values bit for bit -- read in the
deletion column for mu < 0, the normal column for mu = 0 and the duplication column for mu > 0 (as tests/mixture_checker.py::emissions
takes them).  A row's value: math.fsum of its terms, the exact sum rounded once.  The search: call_copy_number(evaluate=evaluator(...)).

The bar of a value.  Write S for the exact sum of the n terms t_i of a row and A = sum |t_i|.  The device adds the terms as a
double-double (hi, lo): adding a term, or another sum's high word, to hi is an error-free TwoSum whose error e, |e| <= 2^-53 |the new hi|,
goes to lo; lo is a plain double that collects these errors and the other sums' low words.  So hi + (the exact sum of what went into
lo) = S, and the only roundings are those of lo's own additions.  An addition that brings in +0 rounds nothing (idle lanes).  Every other
addition belongs to a node of the summation tree -- a lane's chain of at most kSegTiles terms, the six levels of the wave's tree, the
chain of the row's segments -- and a term lies below at most d = min(n, kSegTiles) + 6 + n_segments nodes.  The high word of a node is at
most the sum of |t_i| below it, so all errors that ever reach a low word add up to at most 2^-53 d A, and each addition into a low
word rounds by at most 2^-53 of the low word it makes; summed over the tree again: the carry lost is at most d^2 2^-106 A.  With
kSegTiles = 8 that is below n 2^-100 A for every n >= 4 (d^2 <= 64 n: 11^2 <= 256 at n = 4, (14 + n / 512)^2 <= 64 n up to n = 10^7); for
n <= 3 at most n additions round, each by at most n 2^-106 A.  The value written is fl(hi + lo), one rounding of S + carry, and
math.fsum is fl(S): together
    |dev - fsum| <= 2^-52 |fsum| + n 2^-100 A.
The _dd entries also return tail = (hi + lo) - fl(hi + lo), TwoSum's error term, which is exact: dev + tail = S + carry, so
    |dev + tail - S| <= n 2^-100 A     (tail_gap, in exact rational arithmetic).
"""
import math

import numpy as np


def state_props(e, mixture):
    od, ou = 1 - 0.5 * mixture, 1 + 0.5 * mixture
    return (e * od) / ((e * od + 1) - e), e, (e * ou) / ((e * ou + 1) - e)


def shape_params(ep, sd):
    a1 = ((ep * ep) * (1 - ep)) / (sd * sd) - ep
    return a1, ((1 - ep) / ep) * a1


def dose_ok(mu):
    return bool(mu > -2.0 and mu <= 2.0)


def terms(oracle, obs, tot, phi, expected, mu):
    """the n terms of a row at dose mu (float64, strict bits); the dose must be valid"""
    with np.errstate(all="ignore"):
        m, _ = oracle.get_loglike_matrix(float(phi), float(expected), np.asarray(tot), np.asarray(obs), float(abs(mu)), oracle.PORTABLE)
    return np.array(m[:, 0 if mu < 0 else (2 if mu > 0 else 1)], dtype=np.float64)


def row_counts(test, ref, row, layout=0):
    s, a, b = int(row["sample"]), int(row["start_exon"]), int(row["end_exon"])
    if layout:
        obs, rf = np.asarray(test)[s, a:b + 1], np.asarray(ref)[s, a:b + 1]
    else:
        obs, rf = np.asarray(test)[a:b + 1, s], np.asarray(ref)[a:b + 1, s]
    return obs.astype(np.int64), (obs.astype(np.int64) + rf)


def tail_gap(t, value, tail):
    """(|value + tail - the exact sum of the terms t|, n 2^-100 sum |t_i|): what a double-double value misses, and the carry it may"""
    from fractions import Fraction
    gap = abs(Fraction(float(value)) + Fraction(float(tail)) - sum(Fraction(x) for x in t.tolist()))
    return float(gap), t.size * 2.0 ** -100 * math.fsum(np.abs(t).tolist())


def profile(oracle, rows, test, ref, phi, expected, doses, layout=0, terms_out=None):
    """(L (G, n_rows), bar (G, n_rows)): math.fsum of every row's terms at doses[g, row] and the bar above; NaN (bar 0) for a dose outside
    (-2, 2] and where a term is NaN.  terms_out: a dict that receives the terms of every finite value, by (g, row)."""
    doses = np.asarray(doses, dtype=np.float64)
    G, n = doses.shape
    L, bar = np.full((G, n), np.nan), np.zeros((G, n))
    cache = {}
    for r in range(n):
        obs, tot = row_counts(test, ref, rows[r], layout)
        s = int(rows[r]["sample"])
        for g in range(G):
            mu = float(doses[g, r])
            if not dose_ok(mu):
                continue
            key = (s, int(rows[r]["start_exon"]), int(rows[r]["end_exon"]), mu)
            if key not in cache:
                t = terms(oracle, obs, tot, phi[s], expected[s], mu)
                if np.isnan(t).any():
                    cache[key] = (np.nan, 0.0, None)
                else:
                    v = math.fsum(t.tolist())
                    cache[key] = (v, 2.0 ** -52 * abs(v) + t.size * 2.0 ** -100 * math.fsum(np.abs(t).tolist()), t)
            L[g, r], bar[g, r], t = cache[key]
            if terms_out is not None and t is not None:
                terms_out[(g, r)] = t
    return L, bar


def evaluator(oracle, rows, test, ref, phi, expected, keep=None):
    """doses (G, n_rows) -> L (G, n_rows): what call_copy_number(evaluate=) takes"""
    def evaluate(doses):
        L, _ = profile(oracle, rows, test, ref, phi, expected, doses)
        if keep is not None:
            keep.append((np.array(doses), L.copy()))
        return L
    return evaluate


def draw_rows(ratios, lengths, seed, depth=2000.0, phi=5e-4, expected=0.5):
    """rows drawn from the model, one sample, one chromosome: row r has lengths[r] exons at the planted copy ratio ratios[r], the rows
    stand one behind the other.  Totals are Poisson(depth), the test count beta-binomial with the shape parameters of the expected
    proportion at odds ratios[r] (tests/mixture_checker.py::draw's defaults).  Returns (chrom_off, rows, test, ref (E, 1), phi, expected (1,))."""
    from exomedepth_amd import CALL_DTYPE
    rng = np.random.default_rng(seed)
    lengths = [int(n) for n in lengths]
    E = int(sum(lengths))
    rows = np.zeros(len(lengths), dtype=CALL_DTYPE)
    test, ref = np.zeros((E, 1), dtype=np.int32), np.zeros((E, 1), dtype=np.int32)
    sd = np.sqrt(phi * expected * (1 - expected))
    at = 0
    for r, (ratio, n) in enumerate(zip(ratios, lengths)):
        ep = (expected * ratio) / ((expected * ratio + 1) - expected)
        a1, a2 = shape_params(ep, sd)
        tot = rng.poisson(depth, n)
        obs = rng.binomial(tot, rng.beta(a1, a2, n))
        test[at:at + n, 0], ref[at:at + n, 0] = obs, tot - obs
        rows[r] = (0, 0, at, at + n - 1, 1 if ratio < 1 else 2, n)
        at += n
    return np.array([0, E], dtype=np.int32), rows, test, ref, np.array([phi]), np.array([expected])
