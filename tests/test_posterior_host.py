"""The forward-backward checker (tests/posterior_checker.py) against itself, without a device: the identities of the recurrences on
random chains and on the reference's bundled data through the CPU checker's likelihoods, float64 against long double within the bar of
the numerical contract, the log-evidence against the best path's joint log-probability; and the interface's new symbols."""
import os
import re

import numpy as np
import pytest

import posterior_checker as pc

SETTINGS = ((1e-4, 5e4), (0.05, 3000.0), (0.3, 2000.0))       # tests/test_gpu_chain_geometry.py::SETTINGS
HERE = os.path.dirname(os.path.abspath(__file__))


def _random_case(seed, sizes, S):
    rng = np.random.default_rng(seed)
    chrom_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    E = int(chrom_off[-1])
    gaps = rng.integers(100, 9000, E)
    gaps[rng.integers(0, E, 6)] = 0                   # C = -inf
    gaps[rng.integers(0, E, 6)] = 100_000_000         # rows equal to the from-normal row
    start = np.empty(E, np.int64)
    for c in range(len(sizes)):
        lo, hi = chrom_off[c], chrom_off[c + 1]
        start[lo:hi] = 1000 + np.cumsum(gaps[lo:hi])
    end = start + 100
    ll = -rng.gamma(2.0, 3.0, (E, 3, S))
    ll[rng.integers(0, E, 10), rng.integers(0, 3, 10), rng.integers(0, S, 10)] = -np.inf
    return chrom_off, start, end, ll


def _check_identities(res, m, S):
    """beta_0(0) = logZ, sum_j gamma = 1, logZ >= the best path: within the bar, per sample"""
    bar = pc.bar(m, res["alpha"])
    ok = np.isfinite(res["logZ"].astype(np.float64))
    assert ok.any()
    assert np.all(np.abs((res["beta0"] - res["logZ"]).astype(np.float64))[ok] <= bar[ok])
    assert np.all(np.isneginf(res["beta0"].astype(np.float64))[~ok])
    tot = np.sum(np.exp(res["log_gamma"]), axis=1).astype(np.float64)                  # (m, S)
    assert np.all(np.abs(tot[:, ok] - 1.0) <= np.expm1(bar[ok])[None, :] + 4 * 2.0 ** -52)
    assert np.all((res["vit"] - res["logZ"]).astype(np.float64)[ok] <= bar[ok])
    return bar, ok


@pytest.mark.parametrize("setting", range(3))
def test_identities_on_random_chains(setting):
    sizes, S = (1, 2, 17, 0, 64, 300), 5
    chrom_off, start, end, ll = _random_case(11 + setting, sizes, S)
    tp, L = SETTINGS[setting]
    trs = pc.transitions(chrom_off, start, end, tp, L)
    assert trs[3] is None and any(np.isneginf(tr["C"]).any() for tr in trs if tr)
    hi = pc.run(ll, chrom_off, trs, np.longdouble)
    lo = pc.run(ll, chrom_off, trs, np.float64)
    for c, m in enumerate(sizes):
        if m == 0:
            continue
        bar, ok = _check_identities(hi[c], m, S)
        _check_identities(lo[c], m, S)
        # float64 against long double
        assert np.all(np.abs(lo[c]["logZ"] - hi[c]["logZ"]).astype(np.float64)[ok] <= bar[ok])
        g_hi, g_lo = hi[c]["log_gamma"].astype(np.float64), lo[c]["log_gamma"]
        fin = np.isfinite(g_hi)
        assert np.array_equal(fin[:, :, ok], np.isfinite(g_lo)[:, :, ok])
        with np.errstate(invalid="ignore"):
            d = np.where(fin & ok[None, None, :], np.abs(g_lo - g_hi), 0.0)
        assert np.all(d <= bar[None, None, :])


def test_nan_and_impossible_chains():
    chrom_off, start, end, ll = _random_case(5, (40,), 4)
    ll = np.where(np.isinf(ll), -3.0, ll)
    ll[7, :, 1] = -np.inf              # sample 1: no state can emit exon 7
    ll[20, 0, 2] = np.nan              # sample 2: a NaN emission
    trs = pc.transitions(chrom_off, start, end, 0.05, 3000.0)
    res = pc.chain(ll, trs[0])
    z = res["logZ"].astype(np.float64)
    assert np.isfinite(z[0]) and np.isneginf(z[1]) and np.isnan(z[2]) and np.isfinite(z[3])
    assert np.isneginf(res["beta0"].astype(np.float64)[1]) and np.isnan(res["beta0"].astype(np.float64)[2])


def test_bundled_data_through_the_oracle(oracle):
    """the reference's bundled exome counts (one chromosome, 26 547 exons), Exome1 against the sum of the others at the fitted
    parameters of the stored probe"""
    d = np.load(os.path.join(HERE, "golden", "exomecount_chr1.npz"))
    counts = d["counts"]
    test = counts[:, 0].astype(np.int32)
    ref = counts[:, 1:].sum(axis=1).astype(np.int32)
    p = 1.0 / (1.0 + np.exp(1.36727))
    ell, _ = oracle.get_loglike_matrix(0.0049568, p, test + ref, test, 1.0, oracle.LIBM)
    ll = np.ascontiguousarray(np.asarray(ell, dtype=np.float64).reshape(-1, 3, 1))
    chrom_off = np.array([0, ll.shape[0]], np.int32)
    trs = pc.transitions(chrom_off, d["start"], d["end"], 1e-4, 5e4)
    m = ll.shape[0]
    hi, lo = pc.chain(ll, trs[0], np.longdouble), pc.chain(ll, trs[0], np.float64)
    bar, ok = _check_identities(hi, m, 1)
    _check_identities(lo, m, 1)
    assert ok.all()
    assert abs(float(lo["logZ"][0] - hi["logZ"][0])) <= bar[0]
    g_hi = hi["log_gamma"].astype(np.float64)
    fin = np.isfinite(g_hi)
    assert np.all(np.abs(lo["log_gamma"] - g_hi)[fin] <= bar[0])
    # the checker's posterior agrees with the stored call count's order of magnitude: exons whose CNV posterior exceeds 1/2
    n_cnv = int(np.sum(np.exp(g_hi[:, 1:, 0]).sum(axis=1) > 0.5))
    assert 100 <= n_cnv <= 400, n_cnv          # the Viterbi path of the probe holds 121 + 108 CNV exons


def test_call_summary_of_the_checker():
    """log_p_all of a one-exon call is its log gamma; of a whole chain in one state, that path's joint probability over Z"""
    chrom_off, start, end, ll = _random_case(3, (12,), 2)
    ll = np.where(np.isinf(ll), -2.0, ll)
    trs = pc.transitions(chrom_off, start, end, 0.3, 2000.0)
    res = pc.chain(ll, trs[0])
    tr = trs[0]
    for s in range(2):
        for t in (1, 2):
            mean, mn, all_, z = pc.call_post(res, ll, tr, 4, 4, t, s)
            assert abs(float(all_ - res["log_gamma"][4, t, s])) < 1e-15 and abs(float(mean - mn)) == 0.0 and z == res["logZ"][s]
            mean, mn, all_, z = pc.call_post(res, ll, tr, 0, 11, t, s)
            joint = tr["c1"] + ll[0, pc.COL[t], s] + sum(tr["B"][i] + ll[i, pc.COL[t], s] for i in range(1, 12)) + tr["A"][12]
            assert abs(float(all_ - (joint - res["logZ"][s]))) < 1e-11
            assert float(mn) <= float(mean) and float(all_) <= float(np.log(mn)) + 1e-12


def test_interface_declares_the_posterior_entries():
    from exomedepth_amd import _lib
    names = {n for n, _, _ in _lib.SYMBOLS}
    header = open(os.path.join(os.path.dirname(HERE), "include", "exomedepth_amd.h")).read()
    for sym in ("ed_plan_posterior", "ed_plan_call_posterior", "ed_batch_copy_posterior", "ed_batch_posterior", "ed_batch_copy_log_evidence",
                "ed_batch_copy_call_posterior", "ed_batch_n_posterior_passes"):
        assert sym in names, sym
        assert re.search(r"\b%s\(" % sym, header), sym
    assert "ed_call_post;" in header
    from exomedepth_amd import api
    assert api.CALL_POST_DTYPE.itemsize == 32 and api.CALL_POST_DTYPE.names == ("post_mean", "post_min", "log_p_all", "log_evidence")
