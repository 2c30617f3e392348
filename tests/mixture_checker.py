"""CPU checker of the mixture profile (csrc/edmix.inc) and of fit_prop_tumor's objective, in numpy.

Emissions: the oracle's get_loglike_matrix at the PORTABLE flavour -- the strict mode's values bit for bit -- once per (grid point, pair).
Chains: tests/posterior_checker.py, every (grid point, pair) a column, at np.longdouble (logz) or at float64 by the scaled forward
recursion on probabilities (fast_logz: a few array operations per exon, what a whole fit runs on).  draw() makes counts from the model
at a planted tumour fraction.
"""
import numpy as np

import posterior_checker as pc


def state_props(e, mixture):
    """src/CNV_estimate.cpp:65-66, :75-77: expected proportions of (deletion, normal, duplication)"""
    od, ou = 1 - 0.5 * mixture, 1 + 0.5 * mixture
    return (e * od) / ((e * od + 1) - e), e, (e * ou) / ((e * ou + 1) - e)


def shape_params(ep, sd):
    a1 = ((ep * ep) * (1 - ep)) / (sd * sd) - ep
    return a1, ((1 - ep) / ep) * a1


def emissions(oracle, test, ref, phi, expected, grid):
    """ll (E, 3, G * S), column g * S + s: the likelihood matrix of pair s at mixture grid[g, s]; test, ref (E, S)"""
    test, ref = np.asarray(test), np.asarray(ref)
    E, S = test.shape
    grid = np.asarray(grid, dtype=np.float64)
    G = grid.shape[0]
    ll = np.empty((E, 3, G * S))
    for g in range(G):
        for s in range(S):
            with np.errstate(all="ignore"):
                m, _ = oracle.get_loglike_matrix(phi[s], expected[s], test[:, s] + ref[:, s], test[:, s], float(grid[g, s]), oracle.PORTABLE)
            ll[:, :, g * S + s] = m
    return ll


def logz(ll, chrom_off, trs, G, S, dtype=np.longdouble):
    """(logZ (G, C, S) at dtype with 0 for an empty chromosome, bar (G, C, S) float64: posterior_checker.bar of every chain)"""
    Cn = len(trs)
    out, bar = np.zeros((G, Cn, S), dtype=dtype), np.zeros((G, Cn, S))
    for c, res in enumerate(pc.run(ll, chrom_off, trs, dtype)):
        if res is None:
            continue
        m = int(chrom_off[c + 1]) - int(chrom_off[c])
        out[:, c, :] = res["logZ"].reshape(G, S)
        bar[:, c, :] = pc.bar(m, res["alpha"]).reshape(G, S)
    return out, bar


def fast_logz(ll, chrom_off, trs, G, S):
    """logz() at float64 by the scaled forward recursion (each exon's emissions are scaled by their largest, so nothing underflows for
    finite emissions); the bar from the same alpha.  A column with a NaN emission is NaN."""
    Cn = len(trs)
    out, bar = np.zeros((G, Cn, S)), np.zeros((G, Cn, S))
    N = G * S
    with np.errstate(all="ignore"):
        for c, tr in enumerate(trs):
            if tr is None:
                continue
            lo, m = int(chrom_off[c]), int(chrom_off[c + 1]) - int(chrom_off[c])
            e = np.ascontiguousarray(ll[lo:lo + m][:, pc.COL, :])           # (m, 3, N), HMM state order
            top = e.max(axis=1)                                              # (m, N)
            b = np.exp(e - top[:, None, :])
            a = np.zeros((3, N))
            a[0] = 1.0
            cum = np.zeros(N)
            amax = np.zeros(N)
            for i in range(m):
                P = np.exp(pc._lt(tr, i, np.float64))                        # [from][to]
                a = P.T.dot(a) * b[i]
                nrm = a.sum(axis=0)
                a = a / nrm
                cum = cum + (np.log(nrm) + top[i])
                al = np.log(a) + cum
                amax = np.maximum(amax, np.where(np.isfinite(al), np.abs(al), 0).max(axis=0))
            z = np.exp(pc._lt(tr, m, np.float64))[:, 0].dot(a)
            out[:, c, :] = (cum + np.log(z)).reshape(G, S)
            bar[:, c, :] = (8.0 * (m + 1) * 2.0 ** -52 * np.maximum(1.0, amax)).reshape(G, S)
    return out, bar


def evaluator(oracle, chrom_off, start, end, test, ref, phi, expected, tp=1e-4, L=50000.0, fast=True, keep=None):
    """grid (G, S) -> l (G, S) = the sum over the chromosomes of logZ: what fit_prop_tumor(evaluate=) takes.  keep: a list that
    receives (grid, l, sum of the bars (G, S)) of every evaluation."""
    trs = pc.transitions(chrom_off, start, end, tp, L)
    S = np.asarray(test).shape[1]

    def evaluate(grid):
        grid = np.asarray(grid, dtype=np.float64)
        G = grid.shape[0]
        ll = emissions(oracle, test, ref, phi, expected, grid)
        z, bar = fast_logz(ll, chrom_off, trs, G, S) if fast else logz(ll, chrom_off, trs, G, S)
        l = z.sum(axis=1).astype(np.float64)
        if keep is not None:
            keep.append((grid.copy(), l.copy(), bar.sum(axis=1)))
        return l
    return evaluate


def draw(sizes, fractions, seed, depth=2000.0, phi=5e-4, expected=0.5, segments=3, min_len=8, max_len=40):
    """counts drawn from the model: (chrom_off, start, end, test, ref int32 (E, S), phi, expected (S,)).  Pair s has tumour fraction
    fractions[s]; None plants no segment (and draws every exon from the normal state).  Every chromosome of 100 exons or more gets
    `segments` planted segments of min_len .. max_len exons, deletions and duplications alternating; totals are Poisson(depth), the
    tumour's count beta-binomial with the state's shape parameters."""
    rng = np.random.default_rng(seed)
    sizes = [int(n) for n in sizes]
    chrom_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    E, S = int(chrom_off[-1]), len(fractions)
    gaps = rng.integers(100, 9000, E)
    start = np.empty(E, dtype=np.int64)
    for c in range(len(sizes)):
        lo, hi = chrom_off[c], chrom_off[c + 1]
        start[lo:hi] = 1000 + np.cumsum(gaps[lo:hi])
    end = start + rng.integers(50, 400, E)
    test, ref = np.zeros((E, S), dtype=np.int32), np.zeros((E, S), dtype=np.int32)
    for s, f in enumerate(fractions):
        state = np.ones(E, dtype=np.int64)                                   # matrix column order: 0 deletion, 1 normal, 2 duplication
        if f is not None:
            for c, m in enumerate(sizes):
                if m < 100:
                    continue
                width = m // segments
                for k in range(segments):
                    n = int(rng.integers(min_len, max_len + 1))
                    a = int(chrom_off[c]) + k * width + int(rng.integers(0, width - n))
                    state[a:a + n] = 0 if (k + c + s) % 2 == 0 else 2
        props = np.array(state_props(expected, 0.0 if f is None else f))
        sd = np.sqrt(phi * expected * (1 - expected))
        a1, a2 = shape_params(props, sd)
        tot = rng.poisson(depth, E)
        p = rng.beta(a1[state], a2[state])
        test[:, s] = rng.binomial(tot, p)
        ref[:, s] = tot - test[:, s]
    return chrom_off, start.astype(np.int32), end.astype(np.int32), test, ref, np.full(S, phi), np.full(S, expected)
