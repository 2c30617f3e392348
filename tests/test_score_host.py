"""The transition score without a device: the checker (tests/score_checker.py) against central differences of its own long-double
log-evidence, the chain whose gaps are all padded, fit_transitions' optimiser driven by the checker on data drawn from the model, the
interface's new symbols and the stand-alone check of the derivative table (tools/hmm_score_check.cpp)."""
import os
import re
import subprocess

import numpy as np
import pytest

import posterior_checker as pc
import score_checker as sc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SETTINGS = ((1e-4, 50000.0), (0.01, 20000.0), (0.04, 6000.0))
SIZES = (1, 2, 3, 17, 0, 33, 257, 513)
GEN = (0.04, 6000.0)
_CACHE = {}


def _data(S=3):
    if S not in _CACHE:
        _CACHE[S] = sc.draw(SIZES, S, GEN[0], GEN[1], 5)
    return _CACHE[S]


@pytest.mark.parametrize("setting", range(3))
def test_score_against_central_differences(setting):
    """step 1e-4 theta, padded gaps held fixed; every chain: relative difference <= 1e-5 (a wrong formula gives order 1; the central
    difference itself is good to ~1e-7 here)"""
    chrom_off, start, end, ll = _data()
    tp, L = SETTINGS[setting]
    trs, dvs = pc.transitions(chrom_off, start, end, tp, L), sc.derivatives(chrom_off, start, end, tp, L)
    got = sc.run(ll, chrom_off, trs, dvs, np.longdouble)
    worst = 0.0
    for q, (theta, other) in enumerate(((tp, L), (L, tp))):
        h = np.longdouble(1e-4) * np.longdouble(theta)
        at = lambda v: sc.transitions_ld(chrom_off, start, end, v if q == 0 else tp, v if q == 1 else L, L)
        hi = sc.total_logz(ll, chrom_off, at(np.longdouble(theta) + h))
        lo = sc.total_logz(ll, chrom_off, at(np.longdouble(theta) - h))
        fd = (hi - lo) / (2 * h)
        for c, r in enumerate(got):
            if r is None:
                assert np.all(fd[c] == 0)
                continue
            s = r[1][q]
            assert np.all(np.isfinite(s.astype(np.float64)))
            if q == 1 and SIZES[c] == 1:
                assert np.all(s == 0) and np.all(fd[c] == 0)
                continue
            rel = (np.abs(s - fd[c]) / np.abs(fd[c])).astype(np.float64)
            print("setting %d, d/d%s, chromosome %d (m = %d): largest relative difference %.3g" % (setting, "tL"[q], c, SIZES[c], rel.max()))
            assert np.all(rel <= 1e-5), (setting, q, c, rel.max())
            worst = max(worst, float(rel.max()))
    print("largest relative difference %.3g" % worst)
    # the long-double transitions at the base point are the double ones, to double's rounding: the differences start from the same model
    base = sc.transitions_ld(chrom_off, start, end, tp, L, L)
    for tr, b in zip(trs, base):
        if tr is not None:
            for k in "ABC":
                fin = np.isfinite(tr[k])
                assert np.array_equal(fin, np.isfinite(b[k].astype(np.float64)))
                assert np.all(np.abs(tr[k][fin] - b[k][fin].astype(np.float64)) <= 1e-12)


def test_float64_checker_agrees_with_long_double():
    chrom_off, start, end, ll = _data()
    tp, L = SETTINGS[2]
    trs, dvs = pc.transitions(chrom_off, start, end, tp, L), sc.derivatives(chrom_off, start, end, tp, L)
    hi, lo = sc.run(ll, chrom_off, trs, dvs, np.longdouble), sc.run(ll, chrom_off, trs, dvs, np.float64)
    for c, (a, b) in enumerate(zip(hi, lo)):
        if a is None:
            assert b is None
            continue
        m = SIZES[c]
        bar = pc.bar(m, a[0]["alpha"])
        for q, D in enumerate(sc.weight(dvs[c], m)):
            d = np.abs(b[1][q] - a[1][q]).astype(np.float64)
            assert np.all(d <= (2 * bar + 2.0 ** -50) * D), (c, q)


def test_a_chain_whose_gaps_are_all_padded_has_no_length_score():
    """m = 1: the leading gap and the closing step are both padded, f' = 0 on both: d logZ / d L is exactly 0, at either precision and
    whatever the emissions"""
    rng = np.random.default_rng(2)
    chrom_off = np.array([0, 1, 2], np.int32)
    start = np.array([5000, 90000], np.int32)
    end = start + 120
    ll = -rng.gamma(2.0, 3.0, (2, 3, 7))
    ll[0, 0, 3] = -np.inf
    for tp, L in SETTINGS:
        trs, dvs = pc.transitions(chrom_off, start, end, tp, L), sc.derivatives(chrom_off, start, end, tp, L)
        for dv in dvs:
            assert np.all(dv["AL"] == 0) and np.all(dv["BL"] == 0) and np.all(dv["CL"] == 0)
            assert sc.weight(dv, 1)[1] == 0.0
        for dtype in (np.float64, np.longdouble):
            for r in sc.run(ll, chrom_off, trs, dvs, dtype):
                assert np.all(r[1][1] == 0)
                assert np.all(np.isfinite(r[1][0].astype(np.float64))) and np.all(r[1][0] != 0)


def test_nan_and_impossible_chains_have_nan_scores():
    chrom_off, start, end, ll = sc.draw((40,), 4, 0.04, 6000.0, 3)
    ll = ll.copy()
    ll[7, :, 1] = -np.inf
    ll[20, 0, 2] = np.nan
    trs, dvs = pc.transitions(chrom_off, start, end, 0.04, 6000.0), sc.derivatives(chrom_off, start, end, 0.04, 6000.0)
    _, s = sc.chain_score(ll, trs[0], dvs[0])
    s = s.astype(np.float64)
    assert np.all(np.isfinite(s[:, [0, 3]])) and np.all(np.isnan(s[:, [1, 2]]))


def test_fit_transitions_with_the_checker_converges():
    """data drawn from the model at t = 0.04, L = 6000 (16 samples); from the defaults the fit reaches a log-evidence no smaller than
    that of the generating parameters and of the start"""
    from exomedepth_amd import fit_transitions
    chrom_off, start, end, ll = _data(16)
    ev = sc.evaluator(chrom_off, start, end, ll, np.float64)
    fit = fit_transitions(chrom_off, start, end, evaluate=ev)
    print({k: v for k, v in fit.items() if k != "trace"})
    assert fit["converged"] and 1 <= fit["iterations"] <= 100 and fit["evaluations"] == len(fit["trace"])
    l_gen, l_start = ev(*GEN)[0], ev(1e-4, 50000.0)[0]
    assert fit["log_evidence_start"] == l_start
    assert fit["log_evidence"] >= l_gen and fit["log_evidence"] >= l_start
    assert fit["log_evidence"] == ev(fit["transition_probability"], fit["expected_CNV_length"])[0]
    assert 0.004 < fit["transition_probability"] < 0.4 and 600.0 < fit["expected_CNV_length"] < 60000.0
    acc = [r["log_evidence"] for r in fit["trace"] if r["accepted"]]
    assert all(b >= a for a, b in zip(acc, acc[1:])) and acc[-1] == fit["log_evidence"]


def test_the_fast_evaluator_is_the_checker():
    """score_checker.fast_evaluator (scaled probabilities, what the GPU test's CPU fit runs on) against evaluator() (the log-space
    checker): both float64, different operation orders -- 1e-10 of the value"""
    chrom_off, start, end, ll = _data(16)
    slow, fast = sc.evaluator(chrom_off, start, end, ll), sc.fast_evaluator(chrom_off, start, end, ll)
    for tp, L in SETTINGS + ((0.3, 300.0),):
        a, b = slow(tp, L), fast(tp, L)
        for x, y in zip(a, b):
            assert abs(x - y) <= 1e-10 * abs(x), (tp, L, a, b)


def test_the_optimiser_treats_a_refused_trial_as_a_failed_step():
    """a concave objective whose evaluation refuses L > 60 000 (as a plan whose padded position leaves 32 bits does): the search steps
    back and still reaches the maximum; an objective that is not finite at the start is an error"""
    from exomedepth_amd import fit_transitions
    refused = []

    def ev(t, L):
        if L > 60000.0:
            refused.append(L)
            return np.inf, 0.0, 0.0
        x, y = np.log(t / (1 - t)), np.log(L)
        x0, y0 = np.log(0.02 / 0.98), np.log(55000.0)
        l = -200.0 * (x - x0) ** 2 - 300.0 * (y - y0) ** 2
        return l, -400.0 * (x - x0) / (t * (1 - t)), -600.0 * (y - y0) / L
    fit = fit_transitions([0, 1], [100], [200], evaluate=ev)
    assert refused and fit["converged"]
    assert abs(fit["transition_probability"] - 0.02) < 1e-6 and abs(fit["expected_CNV_length"] - 55000.0) < 0.1
    assert any(not r["accepted"] for r in fit["trace"])
    with pytest.raises(ValueError):
        fit_transitions([0, 1], [100], [200], evaluate=lambda t, L: (np.nan, 0.0, 0.0))


def test_interface_declares_the_score_entries():
    from exomedepth_amd import _lib
    names = {n for n, _, _ in _lib.SYMBOLS}
    header = open(os.path.join(ROOT, "include", "exomedepth_amd.h")).read()
    source = open(os.path.join(ROOT, "exomedepth_amd", "csrc", "edscore.inc")).read()
    for sym in ("ed_plan_transition_score", "ed_batch_copy_transition_score", "ed_batch_n_score_passes", "ed_plan_n_score_tables",
                "ed_batch_transition_score_ms"):
        assert sym in names, sym
        assert re.search(r"\b%s\(" % sym, header), sym
        assert re.search(r"ED_EXPORT [a-z0-9_]+ %s\(" % sym, source), sym
    assert "k_fb_score" in source
    import exomedepth_amd
    from exomedepth_amd import api
    assert exomedepth_amd.fit_transitions is api.fit_transitions and "fit_transitions" in exomedepth_amd.__all__
    for cls in (api.Plan, api.Batch):
        assert callable(getattr(cls, "transition_score"))
    assert callable(api.ExomeDepth.fit_transitions)


def test_hmm_score_checker(tmp_path):
    """tools/hmm_score_check.cpp compiles (without the sanitizer flags its header comment gives for a run by hand) and exits with 0"""
    cc = os.environ.get("ED_SHIM_CC", "gcc")       # the compiler tests/test_shim.py builds with
    exe = str(tmp_path / "hmm_score_check")
    subprocess.run([cc, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tools", "hmm_score_check.cpp"), "-o", exe, "-lstdc++", "-lm"],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert "ok" in r.stdout
