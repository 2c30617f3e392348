"""CPU checker of the forward-backward pass (csrc/edpost.inc), in numpy, at float64 or np.longdouble.

The model is CallCNVs' HMM exactly as the Viterbi kernels implement it: HMM states 0 normal, 1 deletion, 2 duplication; HMM state j reads
likelihood column (1, 0, 2)[j]; per chain of m exons

    alpha_0 = (0, -inf, -inf)                        alpha_i(j) = e_i(j) + LSE_k(alpha_{i-1}(k) + lt_i[k->j]),  i = 1..m
    logZ = LSE_k(alpha_m(k) + lt_{m+1}[k->0])        beta_m(k) = lt_{m+1}[k->0]
    beta_{i-1}(k) = LSE_j(lt_i[k->j] + e_i(j) + beta_i(j)),  i = m..1          (so beta_0(0) = logZ)
    log gamma_i(j) = alpha_i(j) + beta_i(j) - logZ

The log-transitions are rebuilt from the exon positions the way src/hmm.cpp:62-76 does -- in double, with libm's exp and log, because
these doubles ARE the model (the plan's table holds the same computation); only the recurrences run at the requested precision.
Chains are vectorised over samples: a likelihood block is (m, 3, S).
"""
import math

import numpy as np

COL = (1, 0, 2)                    # likelihood column of HMM state j


def transitions(chrom_off, start, end, tp, L):
    """per chromosome None (empty) or dict(c0, c1, A, B, C): c0 = log(1 - t), c1 = log(t / 2) leave `normal`; A / B / C [m + 1] are
    the per-gap entries out of a CNV state (into normal, stay, switch); gap g belongs to exon g (0-based), gap m to the closing step"""
    rows = ((1.0 - tp, tp / 2.0, tp / 2.0), (0.5, 0.5, 0.0), (0.5, 0.0, 0.5))
    lg = lambda x: math.log(x) if x > 0.0 else -math.inf
    out = []
    for c in range(len(chrom_off) - 1):
        lo, hi = int(chrom_off[c]), int(chrom_off[c + 1])
        m = hi - lo
        if m <= 0:
            out.append(None)
            continue
        # as.integer(c(positions[1] - 2 L, positions, end[last] + 2 L))  (R/class_definition.R:368)
        pos = [int(float(start[lo]) - 2 * L)] + [int(x) for x in start[lo:hi]] + [int(float(end[hi - 1]) + 2 * L)]
        A, B, Cs = np.empty(m + 1), np.empty(m + 1), np.empty(m + 1)
        for g in range(m + 1):
            d = math.exp(-(float(pos[g + 1]) - float(pos[g])) / L)
            A[g] = lg(d * rows[1][0] + (1.0 - d) * rows[0][0])
            B[g] = lg(d * rows[1][1] + (1.0 - d) * rows[0][1])
            Cs[g] = lg(d * rows[1][2] + (1.0 - d) * rows[0][2])
        out.append(dict(c0=lg(rows[0][0]), c1=lg(rows[0][1]), A=A, B=B, C=Cs))
    return out


def _lt(tr, g, dtype):
    """[from k][to j] at gap g"""
    return np.array([[tr["c0"], tr["c1"], tr["c1"]], [tr["A"][g], tr["B"][g], tr["C"][g]], [tr["A"][g], tr["C"][g], tr["B"][g]]], dtype=dtype)


def lse(x, axis):
    """log-sum-exp along axis; all -inf gives -inf, a NaN gives NaN, never NaN from inf - inf"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = np.max(x, axis=axis, keepdims=True)
        m0 = np.where(np.isneginf(m), 0, m)
        return np.squeeze(m0, axis=axis) + np.log(np.sum(np.exp(x - m0), axis=axis))


def chain(ll, tr, dtype=np.longdouble):
    """ll (m, 3, S) in the matrix's column order, tr one entry of transitions().  dict of alpha, beta, log_gamma (m, 3, S) in HMM state
    order, logZ (S,), beta0 (S,) = beta_0(0), vit (S,) = joint log-probability of the best path (max-plus, same closing rule)"""
    m, _, S = ll.shape
    e = np.ascontiguousarray(ll[:, COL, :]).astype(dtype)
    ninf = dtype(-np.inf)
    alpha, beta = np.empty((m, 3, S), dtype=dtype), np.empty((m, 3, S), dtype=dtype)
    with np.errstate(invalid="ignore"):
        a = np.full((3, S), ninf, dtype=dtype)
        a[0] = 0
        v = a.copy()
        for i in range(m):
            T = _lt(tr, i, dtype)
            a = e[i] + lse(a[:, None, :] + T[:, :, None], 0)
            v = e[i] + np.max(v[:, None, :] + T[:, :, None], axis=0)
            alpha[i] = a
        T = _lt(tr, m, dtype)
        logZ = lse(a + T[:, 0, None], 0)
        vit = np.max(v + T[:, 0, None], axis=0)
        b = np.repeat(T[:, 0, None], S, axis=1)
        for i in range(m - 1, -1, -1):
            beta[i] = b
            b = lse(_lt(tr, i, dtype)[:, :, None] + (e[i] + b)[None, :, :], 1)
        log_gamma = alpha + beta - logZ[None, None, :]
    return dict(alpha=alpha, beta=beta, log_gamma=log_gamma, logZ=logZ, beta0=b[0], vit=vit)


def bar(m, alpha):
    """the absolute bar of the numerical contract for logZ and every finite log gamma of a chain of m exons, per sample:
    8 (m + 1) 2^-52 max(1, max |finite alpha|); alpha (m, 3, S)"""
    fin = np.where(np.isfinite(alpha), np.abs(alpha), 0).astype(np.float64)
    return 8.0 * (m + 1) * 2.0 ** -52 * np.maximum(1.0, fin.max(axis=(0, 1)))


def call_post(res, ll, tr, a, b, t, s):
    """(post_mean, post_min, log_p_all, log_evidence) of a call of type t over the chain's exons a..b (0-based, inclusive), sample s"""
    dtype = res["alpha"].dtype
    lg = res["log_gamma"][a:b + 1, t, s]
    p = np.exp(lg)
    step = np.asarray(tr["B"][a + 1:b + 1], dtype=dtype) + ll[a + 1:b + 1, COL[t], s].astype(dtype)
    with np.errstate(invalid="ignore"):
        all_ = lg[0] + np.sum(step, dtype=dtype) + res["beta"][b, t, s] - res["beta"][a, t, s]
    return p.mean(dtype=dtype), p.min(), all_, res["logZ"][s]


def run(ll, chrom_off, trs, dtype=np.longdouble):
    """every chain of ll (E, 3, S): list per chromosome of chain() results (None for an empty one)"""
    out = []
    for c, tr in enumerate(trs):
        lo, hi = int(chrom_off[c]), int(chrom_off[c + 1])
        out.append(None if tr is None else chain(ll[lo:hi], tr, dtype))
    return out
