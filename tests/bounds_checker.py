"""CPU checker of the breakpoint credible intervals (csrc/edbounds.inc), in numpy at np.longdouble, on posterior_checker.chain.

A row of type T over the chain's exons r0..r1 (0-based, inclusive).  Anchor a: the exon of the row with the largest log gamma(T), ties
to the lowest index, NaN ignored.  The extent of the run of T through the anchor, by the checker's OWN alpha (the device walks
log gamma - beta instead: an independent route to the same number):

    log P(x_i .. x_a = T | data) = alpha_i(T) + sum_{t=i+1..a} (B_t + e_t(T)) + beta_a(T) - logZ            i <= a
    log P(x_a .. x_j = T | data) = alpha_a(T) + sum_{t=a+1..j} (B_t + e_t(T)) + beta_j(T) - logZ            j >= a
    G_L(i), G_R(j) = the above - log gamma_a(T),  G(a) = 0

B_t the stay entry of exon t's gap.  A bound is the last exon, walking outward from a, before the FIRST one whose G is below the
threshold (or NaN) or that lies outside the chain: log1p(-tail) for start_hi / end_lo, log(tail) for start_lo / end_hi,
tail = (1 - level) / 2.

The bar of a G (and of log_anchor, with n = 0): 4 posterior_checker.bar(m, alpha) of the chain -- two beta and two log gamma in the worst
case -- plus 2^-50 (n + 1) max(1, max |partial sum|) for a walk of n steps.
"""
import math

import numpy as np

import posterior_checker as pc


def anchor(res, r0, r1, t, s):
    """(a, log gamma_a(T)); a is None when no exon of the row has a finite log gamma(T)"""
    lg = res["log_gamma"][r0:r1 + 1, t, s]
    v = np.where(np.isnan(lg), -np.inf, lg)
    k = int(np.argmax(v))                                 # the first of equal maxima
    if not np.isfinite(v[k]):
        return None, None
    return r0 + k, lg[k]


def extent(res, ll, tr, a, t, s):
    """dict of GL (a + 1 values, GL[k] at exon a - k), GR (m - a values, GR[k] at exon a + k), barL, barR (float64, the bars of those
    values) for the run of state t through exon a of sample s; ll (m, 3, S) the chain's likelihood block"""
    dtype = res["alpha"].dtype
    m = res["alpha"].shape[0]
    al, be, lz = res["alpha"][:, t, s], res["beta"][:, t, s], res["logZ"][s]
    w = np.asarray(tr["B"][:m], dtype=dtype) + ll[:, pc.COL[t], s].astype(dtype)          # w[x] joins exon x - 1 to x
    lga = res["log_gamma"][a, t, s]
    with np.errstate(invalid="ignore"):
        sl = np.concatenate([np.zeros(1, dtype), np.cumsum(w[a:0:-1], dtype=dtype)])        # sum_{t = a-k+1 .. a}
        sr = np.concatenate([np.zeros(1, dtype), np.cumsum(w[a + 1:], dtype=dtype)])        # sum_{t = a+1 .. a+k}
        GL = ((al[a::-1] + sl) + be[a]) - lz - lga
        GR = ((al[a] + sr) + be[a:]) - lz - lga
    GL[0] = GR[0] = 0
    base = 4.0 * float(pc.bar(m, res["alpha"][:, :, s:s + 1])[0])

    def bars(sums):
        fin = np.where(np.isfinite(sums), np.abs(sums), 0).astype(np.float64)
        return base + 2.0 ** -50 * (np.arange(sums.size) + 1.0) * np.maximum(1.0, np.maximum.accumulate(fin))
    return dict(GL=GL, GR=GR, barL=bars(sl), barR=bars(sr), base=base)


def thresholds(level):
    tail = (1.0 - level) / 2.0
    return math.log1p(-tail), math.log(tail)              # (inner: start_hi / end_lo, outer: start_lo / end_hi)


def first_failure(G, thr):
    """distance of the bound: the last k before the first G[k] that is not >= thr; the walk's end if none fails"""
    with np.errstate(invalid="ignore"):
        bad = np.flatnonzero(~(G >= thr))
    return int(bad[0]) - 1 if bad.size else G.size - 1


def row(res, ll, tr, r0, r1, t, s, levels, forced=None):
    """the checker's record of a row: None for a row that cannot be walked, else dict(anchor, log_anchor, log_keep_start, log_keep_end,
    bar_anchor, bar_keep_start, bar_keep_end, ext, and per level (start_lo, start_hi, end_lo, end_hi) as chain-local exons).
    forced: walk from this exon of the row instead of the row's own anchor (the GPU test hands in the arg-max of the device's log gamma)"""
    if t not in (1, 2):
        return None
    a, lga = anchor(res, r0, r1, t, s)
    if a is None:
        return None
    if forced is not None:
        a, lga = int(forced), res["log_gamma"][int(forced), t, s]
    ext = extent(res, ll, tr, a, t, s)
    out = dict(anchor=a, log_anchor=lga, log_keep_start=ext["GL"][a - r0], log_keep_end=ext["GR"][r1 - a], bar_anchor=ext["base"] + 2.0 ** -50,
               bar_keep_start=float(ext["barL"][a - r0]), bar_keep_end=float(ext["barR"][r1 - a]), ext=ext, bounds={})
    for level in levels:
        thi, tlo = thresholds(level)
        out["bounds"][level] = (a - first_failure(ext["GL"], tlo), a - first_failure(ext["GL"], thi),
                                a + first_failure(ext["GR"], thi), a + first_failure(ext["GR"], tlo))
    return out


def rows(res, ll, tr, specs, levels, window=32):
    """row() for many rows of one chain -- specs a list of (r0, r1, t, s) or (r0, r1, t, s, forced anchor) -- with the walks of all rows of a type evaluated together over
    a window of `window` exons on each side of the anchor (the same sums in the same order, so the same numbers); a row whose walk or
    own edge leaves the window goes through row().  The records' `ext` then holds the window only."""
    dtype = res["alpha"].dtype
    m = res["alpha"].shape[0]
    out = [None] * len(specs)
    K = int(window)
    k = np.arange(K + 1)
    base_s = 4.0 * pc.bar(m, res["alpha"])
    for t in (1, 2):
        idx, anc = [], []
        for n, sp in enumerate(specs):
            if sp[2] != t:
                continue
            a, _ = anchor(res, sp[0], sp[1], t, sp[3])
            if a is not None:
                idx.append(n)
                anc.append(a if len(sp) < 5 else int(sp[4]))
        if not idx:
            continue
        A = np.array(anc)[:, None]
        Sx = np.array([specs[n][3] for n in idx])[:, None]
        al, be = res["alpha"][:, t, :], res["beta"][:, t, :]
        w = np.asarray(tr["B"][:m], dtype=dtype)[:, None] + ll[:, pc.COL[t], :].astype(dtype)
        lga = res["log_gamma"][A, t, Sx]
        zero = np.zeros((len(idx), 1), dtype)
        side = {}
        with np.errstate(invalid="ignore"):
            for name, X in (("L", A - k[None, :]), ("R", A + k[None, :])):
                valid = (X >= 0) & (X < m)
                Xc = np.clip(X, 0, m - 1)
                step = np.where(valid, w[np.clip(Xc + 1, 0, m - 1) if name == "L" else Xc, Sx], 0)[:, 1:]
                sums = np.concatenate([zero, np.cumsum(step, axis=1, dtype=dtype)], axis=1)
                if name == "L":
                    G = ((al[Xc, Sx] + sums) + be[A, Sx]) - res["logZ"][Sx] - lga
                else:
                    G = ((al[A, Sx] + sums) + be[Xc, Sx]) - res["logZ"][Sx] - lga
                G[:, 0] = 0
                G = np.where(valid, G, np.nan)
                fin = np.where(np.isfinite(sums), np.abs(sums), 0).astype(np.float64)
                bar = base_s[Sx] + 2.0 ** -50 * (k[None, :] + 1.0) * np.maximum(1.0, np.maximum.accumulate(fin, axis=1))
                side[name] = (G, bar)
        def ff(G, thr):                                   # first_failure, row by row
            with np.errstate(invalid="ignore"):
                bad = ~(G >= thr)
            return np.where(bad.any(axis=1), np.argmax(bad, axis=1) - 1, K)
        fs = {}
        for level in levels:
            thi, tlo = thresholds(level)
            fs[level] = np.stack([ff(side["L"][0], tlo), ff(side["L"][0], thi), ff(side["R"][0], thi), ff(side["R"][0], tlo)], axis=1)
        for q, n in enumerate(idx):
            r0, r1, _, s = specs[n][:4]
            a = anc[q]
            GL, GR = side["L"][0][q], side["R"][0][q]
            ok = a - r0 <= K and r1 - a <= K
            bounds = {}
            for level in levels:
                f = [int(x) for x in fs[level][q]]
                ok = ok and max(f) < K                    # a walk that passes the whole window is not decided inside it
                bounds[level] = (a - f[0], a - f[1], a + f[2], a + f[3])
            if not ok:
                out[n] = row(res, ll, tr, r0, r1, t, s, levels, forced=a if len(specs[n]) > 4 else None)
                continue
            ext = dict(GL=GL, GR=GR, barL=side["L"][1][q], barR=side["R"][1][q], base=float(base_s[s]))
            out[n] = dict(anchor=a, log_anchor=lga[q, 0], log_keep_start=GL[a - r0], log_keep_end=GR[r1 - a],
                          bar_anchor=ext["base"] + 2.0 ** -50, bar_keep_start=float(ext["barL"][a - r0]),
                          bar_keep_end=float(ext["barR"][r1 - a]), ext=ext, bounds=bounds)
    return out


def excused(rec, level, which, got):
    """may the device's bound `got` (chain-local exon) differ from the checker's?  Only if every exon between the two has
    |G - threshold| within its bar.  which: 0 start_lo, 1 start_hi, 2 end_lo, 3 end_hi"""
    want = rec["bounds"][level][which]
    thi, tlo = thresholds(level)
    thr = (tlo, thi, thi, tlo)[which]
    a, ext = rec["anchor"], rec["ext"]
    G, bar = (ext["GL"], ext["barL"]) if which < 2 else (ext["GR"], ext["barR"])
    k0, k1 = sorted((abs(got - a), abs(want - a)))
    if (got - a) * (want - a) < 0 or k1 >= G.size:
        return False
    with np.errstate(invalid="ignore"):
        d = np.abs((G[k0 + 1:k1 + 1] - thr).astype(np.float64))
    return bool(np.all(d <= bar[k0 + 1:k1 + 1]))


def near_threshold(rec, level):
    """how many of the row's four threshold decisions lie within the bar: for each bound, the last passing and the first failing exon"""
    n = 0
    thi, tlo = thresholds(level)
    a, ext = rec["anchor"], rec["ext"]
    for which, x in enumerate(rec["bounds"][level]):
        thr = (tlo, thi, thi, tlo)[which]
        G, bar = (ext["GL"], ext["barL"]) if which < 2 else (ext["GR"], ext["barR"])
        k = abs(x - a)
        near = False
        for kk in (k, k + 1):
            if 0 < kk < G.size and np.isfinite(G[kk]):
                near = near or abs(float(G[kk] - thr)) <= bar[kk]
        n += int(near)
    return n


def pseudo_rows(res, t, s, lo=0):
    """one (start, end) per maximal run of gamma(t) > 1/2 of sample s (chain-local exons + lo)"""
    with np.errstate(invalid="ignore"):
        on = np.asarray(res["log_gamma"][:, t, s] > math.log(0.5))
    d = np.diff(np.concatenate([[0], on.astype(np.int8), [0]]))
    return [(int(a) + lo, int(b) - 1 + lo) for a, b in zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1))]
