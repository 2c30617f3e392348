"""CPU checker of the transition score (csrc/edscore.inc, csrc/ed_hmm_score.hpp), in numpy, at float64 or np.longdouble.

The model is tests/posterior_checker.py's.  Per gap of distance d, f = exp(-d / L), P_A = f/2 + (1-f)(1-t), P_B = f/2 + (1-f) t/2,
P_C = (1-f) t/2; with f' = f d / L^2

              d/dt                  d/dL
    c0    -1 / (1 - t)               0
    c1     1 / t                     0
    A     -(1 - f) / P_A             f' (t - 1/2) / P_A
    B      (1 - f) / (2 P_B)         f' (1/2 - t/2) / P_B
    C      1 / t                    -f' / (1 - f)              (both 0 where P_C = 0)

and f' = 0 for the two padded gaps of a chromosome (their distance is 2 L by construction: f does not move with L).  The score of a
chain, theta in {t, L}:

    d logZ / d theta = sum_{i=1..m} sum_{k,j} xi_i(k->j) d lt_i[k->j] + sum_k gamma_m(k) d lt_{m+1}[k->0]
    xi_i(k->j) = exp(alpha_{i-1}(k) + lt_i[k->j] + e_i(j) + beta_i(j) - logZ)          (an exponent of -inf contributes 0)

The derivative table is built in double from the formulas above (it IS the model's, as the log-transitions are); the recurrences and
the sums run at the requested precision.  transitions_ld() rebuilds the log-transitions at long double for any (t, L) with the padded
gaps held at the f of a base L: what central differences of logZ need.
"""
import math

import numpy as np

import posterior_checker as pc


def _padded(chrom_off, start, end, c, L):
    lo, hi = int(chrom_off[c]), int(chrom_off[c + 1])
    return [int(float(start[lo]) - 2 * L)] + [int(x) for x in start[lo:hi]] + [int(float(end[hi - 1]) + 2 * L)]


def derivatives(chrom_off, start, end, tp, L):
    """per chromosome None (empty) or dict(dc0, dc1: d/dt of c0, c1; At, Bt, Ct, AL, BL, CL [m + 1]: d/dt and d/dL of the per-gap entries)"""
    out = []
    for c in range(len(chrom_off) - 1):
        m = int(chrom_off[c + 1]) - int(chrom_off[c])
        if m <= 0:
            out.append(None)
            continue
        pos = _padded(chrom_off, start, end, c, L)
        d = {k: np.zeros(m + 1) for k in ("At", "Bt", "Ct", "AL", "BL", "CL")}
        for g in range(m + 1):
            dist = float(pos[g + 1]) - float(pos[g])
            f = math.exp(-dist / L)
            PA, PB, PC = f / 2 + (1 - f) * (1 - tp), f / 2 + (1 - f) * tp / 2, (1 - f) * tp / 2
            fp = 0.0 if g in (0, m) else f * dist / (L * L)
            d["At"][g] = -(1 - f) / PA
            d["Bt"][g] = (1 - f) / (2 * PB)
            d["AL"][g] = fp * (tp - 0.5) / PA
            d["BL"][g] = fp * (0.5 - tp / 2) / PB
            if PC > 0:
                d["Ct"][g] = 1 / tp
                d["CL"][g] = -fp / (1 - f) if fp else 0.0
        d["dc0"], d["dc1"] = -1 / (1 - tp), 1 / tp
        out.append(d)
    return out


def _dlt(dv, g, dtype):
    """([from k][to j] d/dt, the same d/dL) at gap g"""
    dt = np.array([[dv["dc0"], dv["dc1"], dv["dc1"]], [dv["At"][g], dv["Bt"][g], dv["Ct"][g]], [dv["At"][g], dv["Ct"][g], dv["Bt"][g]]], dtype=dtype)
    dL = np.array([[0, 0, 0], [dv["AL"][g], dv["BL"][g], dv["CL"][g]], [dv["AL"][g], dv["CL"][g], dv["BL"][g]]], dtype=dtype)
    return dt, dL


def weight(dv, m):
    """D_q = sum over the gaps g = 0 .. m of max_{k->j} |d_q lt_g[k->j]|, q = t, L: what an absolute error of log xi is multiplied by"""
    Dt = sum(max(abs(dv["dc0"]), abs(dv["dc1"]), abs(dv["At"][g]), abs(dv["Bt"][g]), abs(dv["Ct"][g])) for g in range(m + 1))
    DL = sum(max(abs(dv["AL"][g]), abs(dv["BL"][g]), abs(dv["CL"][g])) for g in range(m + 1))
    return float(Dt), float(DL)


def chain_score(ll, tr, dv, dtype=np.longdouble, res=None):
    """ll (m, 3, S), tr / dv one entry of transitions() / derivatives().  (res of posterior_checker.chain, score (2, S)); the score of a
    sample whose logZ is not finite is NaN"""
    m, _, S = ll.shape
    if res is None:
        res = pc.chain(ll, tr, dtype)
    e = np.ascontiguousarray(ll[:, pc.COL, :]).astype(dtype)
    logZ = res["logZ"]
    score = np.zeros((2, S), dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        prev = np.full((3, S), -np.inf, dtype=dtype)
        prev[0] = 0
        for i in range(m):
            T = pc._lt(tr, i, dtype)
            dt, dL = _dlt(dv, i, dtype)
            # [k][j][s]
            ex = prev[:, None, :] + T[:, :, None] + (e[i] + res["beta"][i])[None, :, :] - logZ[None, None, :]
            xi = np.where(np.isneginf(ex), 0, np.exp(ex))
            score[0] += np.sum(xi * dt[:, :, None], axis=(0, 1))
            score[1] += np.sum(xi * dL[:, :, None], axis=(0, 1))
            prev = res["alpha"][i]
        dt, dL = _dlt(dv, m, dtype)
        gm = np.exp(res["log_gamma"][m - 1])
        gm = np.where(np.isneginf(res["log_gamma"][m - 1]), 0, gm)
        score[0] += np.sum(gm * dt[:, 0, None], axis=0)
        score[1] += np.sum(gm * dL[:, 0, None], axis=0)
    bad = ~np.isfinite(logZ.astype(np.float64))
    score[:, bad] = np.nan
    return res, score


def run(ll, chrom_off, trs, dvs, dtype=np.longdouble):
    """every chain of ll (E, 3, S): list per chromosome of (chain result, score (2, S)), None for an empty one"""
    out = []
    for c, tr in enumerate(trs):
        lo, hi = int(chrom_off[c]), int(chrom_off[c + 1])
        out.append(None if tr is None else chain_score(ll[lo:hi], tr, dvs[c], dtype))
    return out


def transitions_ld(chrom_off, start, end, tp, L, L_pad):
    """posterior_checker.transitions at long double for any (tp, L): the padded positions and the padded gaps' f are those of L_pad"""
    ld = np.longdouble
    tp, L = ld(tp), ld(L)
    with np.errstate(divide="ignore"):
        out = []
        for c in range(len(chrom_off) - 1):
            m = int(chrom_off[c + 1]) - int(chrom_off[c])
            if m <= 0:
                out.append(None)
                continue
            pos = _padded(chrom_off, start, end, c, L_pad)
            dist = np.array([float(pos[g + 1]) - float(pos[g]) for g in range(m + 1)], dtype=ld)
            scale = np.full(m + 1, L, dtype=ld)
            scale[0] = scale[m] = ld(L_pad)
            f = np.exp(-dist / scale)
            out.append(dict(c0=np.log(1 - tp), c1=np.log(tp / 2), A=np.log(f / 2 + (1 - f) * (1 - tp)), B=np.log(f / 2 + (1 - f) * tp / 2),
                            C=np.log((1 - f) * tp / 2)))
    return out


def total_logz(ll, chrom_off, trs, dtype=np.longdouble):
    """logZ (C, S) of every chain, 0 for an empty chromosome"""
    S = ll.shape[2]
    out = np.zeros((len(trs), S), dtype=dtype)
    for c, tr in enumerate(trs):
        if tr is not None:
            lo, hi = int(chrom_off[c]), int(chrom_off[c + 1])
            out[c] = pc.chain(ll[lo:hi], tr, dtype)["logZ"]
    return out


def evaluator(chrom_off, start, end, ll, dtype=np.float64):
    """(t, L) -> (l, dl/dt, dl/dL) summed over every chain of ll: what fit_transitions(evaluate=) takes"""
    def evaluate(t, L):
        trs = pc.transitions(chrom_off, start, end, t, L)
        dvs = derivatives(chrom_off, start, end, t, L)
        tot = np.zeros(3, dtype=dtype)
        for r in run(ll, chrom_off, trs, dvs, dtype):
            if r is not None:
                tot += (r[0]["logZ"].sum(), r[1][0].sum(), r[1][1].sum())
        return float(tot[0]), float(tot[1]), float(tot[2])
    return evaluate


def fast_evaluator(chrom_off, start, end, ll):
    """evaluator() for emissions that do not underflow (draw()'s): the same sums at float64 by the scaled forward-backward recursion on
    probabilities -- a few array operations per exon, so that a whole fit takes seconds.  test_score_host checks it against evaluator()."""
    emis = np.exp(np.ascontiguousarray(ll[:, pc.COL, :]))               # (E, 3, S), HMM state order

    def evaluate(t, L):
        trs = pc.transitions(chrom_off, start, end, t, L)
        dvs = derivatives(chrom_off, start, end, t, L)
        S = ll.shape[2]
        tot = np.zeros(3)
        for c, (tr, dv) in enumerate(zip(trs, dvs)):
            if tr is None:
                continue
            lo, m = int(chrom_off[c]), int(chrom_off[c + 1]) - int(chrom_off[c])
            P = np.empty((m + 1, 3, 3))                               # [gap][from][to]
            P[:, 0, :] = np.exp([tr["c0"], tr["c1"], tr["c1"]])
            P[:, 1, 0] = P[:, 2, 0] = np.exp(tr["A"])
            P[:, 1, 1] = P[:, 2, 2] = np.exp(tr["B"])
            P[:, 1, 2] = P[:, 2, 1] = np.exp(tr["C"])
            Dt, DL = np.zeros((m + 1, 3, 3)), np.zeros((m + 1, 3, 3))
            Dt[:, 0, :] = [dv["dc0"], dv["dc1"], dv["dc1"]]
            Dt[:, 1, 0] = Dt[:, 2, 0] = dv["At"]
            Dt[:, 1, 1] = Dt[:, 2, 2] = dv["Bt"]
            Dt[:, 1, 2] = Dt[:, 2, 1] = dv["Ct"]
            DL[:, 1, 0] = DL[:, 2, 0] = dv["AL"]
            DL[:, 1, 1] = DL[:, 2, 2] = dv["BL"]
            DL[:, 1, 2] = DL[:, 2, 1] = dv["CL"]
            PDt, PDL = P * Dt, P * DL
            b = emis[lo:lo + m]
            ahat = np.empty((m + 1, 3, S))                            # alpha before exon i, normalised per sample
            ahat[0] = 0.0
            ahat[0, 0] = 1.0
            norm = np.empty((m, S))
            for i in range(m):
                a = P[i].T.dot(ahat[i]) * b[i]
                norm[i] = a.sum(axis=0)
                ahat[i + 1] = a / norm[i]
            z = P[m][:, 0].dot(ahat[m])                               # (S,)
            tot[0] += np.log(norm).sum() + np.log(z).sum()
            bh = np.repeat(P[m][:, 0, None], S, axis=1) / z           # sum_k ahat[m](k) bh(k) = 1
            gm = ahat[m] * bh
            tot[1] += (gm * Dt[m][:, 0, None]).sum()
            tot[2] += (gm * DL[m][:, 0, None]).sum()
            for i in range(m - 1, -1, -1):
                v = b[i] * bh / norm[i]                               # [to j][s]
                tot[1] += (ahat[i] * PDt[i].dot(v)).sum()             # sum_{k,j,s} ahat_i(k) P[k,j] D[k,j] v(j)
                tot[2] += (ahat[i] * PDL[i].dot(v)).sum()
                bh = P[i].dot(v)
        return float(tot[0]), float(tot[1]), float(tot[2])
    return evaluate


def draw(sizes, S, tp, L, seed):
    """data drawn from the model: (chrom_off, start, end int32, ll (E, 3, S)).  Gaps of 100 .. 9000; per (chromosome, sample) a path of
    hidden states from the HMM at (tp, L) started in `normal` (the plan's transition rows, leading padded gap included), per exon one of
    six symbols from its state's distribution; ll holds the log-probability of the exon's symbol under every state, in the matrix's
    column order (deletion, normal, duplication)"""
    rng = np.random.default_rng(seed)
    sizes = [int(n) for n in sizes]
    chrom_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    E = int(chrom_off[-1])
    gaps = rng.integers(100, 9000, E)
    start = np.empty(E, dtype=np.int64)
    for c in range(len(sizes)):
        lo, hi = chrom_off[c], chrom_off[c + 1]
        start[lo:hi] = 1000 + np.cumsum(gaps[lo:hi])
    end = start + rng.integers(50, 400, E)
    start, end = start.astype(np.int32), end.astype(np.int32)
    emit = np.array([[0.05, 0.15, 0.30, 0.30, 0.15, 0.05],          # HMM state 0 normal
                     [0.40, 0.30, 0.15, 0.08, 0.05, 0.02],          # 1 deletion
                     [0.02, 0.05, 0.08, 0.15, 0.30, 0.40]])         # 2 duplication
    trs = pc.transitions(chrom_off, start, end, tp, L)
    ll = np.empty((E, 3, S))
    for c, tr in enumerate(trs):
        if tr is None:
            continue
        lo, m = int(chrom_off[c]), sizes[c]
        state = np.zeros(S, dtype=np.int64)
        for i in range(m):
            P = np.exp(pc._lt(tr, i, np.float64))                    # [from][to]
            u = rng.random(S)
            cum = np.cumsum(P[state], axis=1)
            state = np.minimum((u[:, None] > cum).sum(axis=1), 2)
            sym = (rng.random(S)[:, None] > np.cumsum(emit[state], axis=1)).sum(axis=1).clip(0, 5)
            ll[lo + i] = np.log(emit[:, sym])[[1, 0, 2]]            # row = matrix column: (del, normal, dup) = states (1, 0, 2)
    return chrom_off, start, end, ll
