"""The mixture profile and fit_prop_tumor without a device: the checker (tests/mixture_checker.py) at mixture 0, the search driven by the
checker on data drawn from the model, the search's mechanics on closed-form objectives, the interface's new symbols and the
stand-alone check of the launch geometry (tools/mix_plan_check.cpp)."""
import os
import re
import subprocess

import numpy as np
import pytest

import mixture_checker as mc
import posterior_checker as pc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# the recovery case: the settings the estimator was verified at (totals around 2 000, phi = 5e-4, expected 0.5, plan defaults)
SIZES = (1, 2, 700, 0, 1300)
FRACTIONS = (1.0, 0.6, 0.3, None)
SEED = 3
_CACHE = {}


def recovery_case(oracle, sizes=SIZES, seed=SEED):
    """(data of mixture_checker.draw, the checker-driven fit, the evaluations it made) -- computed once, shared, left unchanged"""
    key = (tuple(sizes), seed)
    if key not in _CACHE:
        from exomedepth_amd import fit_prop_tumor
        data = mc.draw(sizes, FRACTIONS, seed)
        chrom_off, start, end, test, ref, phi, expected = data
        keep = []
        ev = mc.evaluator(oracle, chrom_off, start, end, test, ref, phi, expected, keep=keep)
        fit = fit_prop_tumor(chrom_off, start, end, phi=phi, expected=expected, evaluate=ev)
        _CACHE[key] = (data, fit, keep)
    return _CACHE[key]


def test_equal_columns_at_mixture_zero(oracle):
    """m = 0: the three states' expected proportions are one number, so the emission columns are equal and every path has the same
    emissions: logZ = the normal column's sum + log P(the chain ends in `normal` after the closing step), from the transitions alone.
    (expected is dyadic, so that (e + 1) - e is exactly 1 and the columns are equal to the bit)"""
    sizes = (1, 2, 0, 65, 130)
    chrom_off, start, end, test, ref, phi, _ = mc.draw(sizes, (0.5, None, 1.0), 9, depth=300.0)
    test[3, 0], ref[3, 0] = 0, 40
    test[4, 1], ref[4, 1] = 0, 0
    expected = np.array([0.5, 0.25, 0.375])
    S = 3
    ll = mc.emissions(oracle, test, ref, phi, expected, np.zeros((1, S)))
    assert np.all(np.isfinite(ll))
    assert np.array_equal(ll[:, 0, :], ll[:, 1, :]) and np.array_equal(ll[:, 2, :], ll[:, 1, :])
    trs = pc.transitions(chrom_off, start, end, 1e-4, 50000.0)
    z, bar = mc.logz(ll, chrom_off, trs, 1, S)
    zf, _ = mc.fast_logz(ll, chrom_off, trs, 1, S)
    ld = np.longdouble
    for c, tr in enumerate(trs):
        if tr is None:
            assert np.all(z[0, c] == 0)
            continue
        lo, m = int(chrom_off[c]), sizes[c]
        v = np.array([1, 0, 0], dtype=ld)
        for g in range(m):
            v = np.exp(pc._lt(tr, g, ld)).T.dot(v)
        mass = np.log(np.exp(pc._lt(tr, m, ld))[:, 0].dot(v))
        want = ll[lo:lo + m, 1, :].astype(ld).sum(axis=0) + mass
        assert np.all(np.abs(z[0, c] - want).astype(np.float64) <= bar[0, c]), c
        assert np.all(np.abs(zf[0, c] - want).astype(np.float64) <= 2 * bar[0, c]), c


def test_the_fast_path_is_the_long_double_checker(oracle):
    chrom_off, start, end, test, ref, phi, expected = mc.draw((3, 0, 150), (0.6, None), 4)
    grid = np.array([[0.0, 1.0], [0.3, 0.3], [1.0, 0.55]])
    ll = mc.emissions(oracle, test, ref, phi, expected, grid)
    trs = pc.transitions(chrom_off, start, end, 1e-4, 50000.0)
    a, bar = mc.logz(ll, chrom_off, trs, 3, 2)
    b, bar64 = mc.fast_logz(ll, chrom_off, trs, 3, 2)
    assert np.all(np.abs(a - b).astype(np.float64) <= bar)
    assert np.all(np.abs(bar - bar64) <= 1e-6 * bar)


def test_recovery_with_the_checker(oracle):
    """fractions 1.0 / 0.6 / 0.3 end within 1/15 of the truth with a gain of 100 or more; the pair without a segment gains less than
    min_gain, is not informative and has no estimate"""
    _, fit, keep = recovery_case(oracle)
    print({k: v for k, v in fit.items() if k not in ("trace", "profile")})
    assert fit["evaluations"] == 3 == len(keep) and fit["profile"].shape == (16, 4)
    for s, f in enumerate(FRACTIONS[:3]):
        assert fit["informative"][s] and abs(fit["prop_tumor"][s] - f) <= 1.0 / 15, (s, fit["prop_tumor"][s])
        assert fit["gain"][s] >= 100.0 and (fit["at_bound"][s] or fit["se"][s] > 0)
    assert fit["gain"][3] < 5.41 and not fit["informative"][3] and np.isnan(fit["prop_tumor"][3])
    assert np.array_equal(fit["log_evidence_null"], fit["profile"][0])
    assert np.all(fit["log_evidence"] - fit["log_evidence_null"] == fit["gain"])


def _closed_form(fn):
    return lambda grid: fn(np.asarray(grid))


def test_search_finds_a_maximum_on_a_grid_point():
    from exomedepth_amd import fit_prop_tumor
    fit = fit_prop_tumor([0, 1], [1], [2], evaluate=_closed_form(lambda m: 50.0 - 400.0 * (m - 0.4) ** 2))   # 0.4 = 6 / 15
    assert fit["trace"][0]["k"][0] == 6 and fit["evaluations"] == 3
    assert abs(fit["prop_tumor"][0] - 0.4) <= 1e-12 and fit["informative"][0] and not fit["at_bound"][0]
    h = (2.0 / 15) ** 2 / 15
    assert abs(fit["se"][0] - 1.0 / np.sqrt(800.0)) <= 1e-6 and abs(fit["trace"][2]["grid"][1, 0] - fit["trace"][2]["grid"][0, 0] - h) <= 1e-15
    assert abs(fit["gain"][0] - 64.0) <= 1e-3 and abs(fit["log_evidence_null"][0] + 14.0) <= 1e-12


def test_search_reports_a_maximum_on_the_bound():
    from exomedepth_amd import fit_prop_tumor
    fit = fit_prop_tumor([0, 1], [1], [2], upper=np.array([1.0, 0.8]), evaluate=_closed_form(lambda m: 30.0 * m))
    assert np.all(fit["at_bound"]) and np.array_equal(fit["prop_tumor"], [1.0, 0.8]) and np.all(np.isnan(fit["se"]))
    assert all(np.all(r["k"] == 15) for r in fit["trace"])
    low = fit_prop_tumor([0, 1], [1], [2], lower=0.2, evaluate=_closed_form(lambda m: -30.0 * m))
    assert low["at_bound"][0] and low["estimate"][0] == 0.2 and low["evaluations"] == 4      # l(0) costs one more evaluation
    assert low["log_evidence_null"][0] == 0.0 and not low["informative"][0] and np.isnan(low["prop_tumor"][0])


def test_search_takes_the_first_index_of_a_tie():
    from exomedepth_amd import fit_prop_tumor
    fit = fit_prop_tumor([0, 1], [1], [2], min_gain=-1.0, evaluate=_closed_form(lambda m: np.zeros_like(m)))
    assert all(r["k"][0] == 0 for r in fit["trace"])
    assert fit["estimate"][0] == 0.0 and fit["at_bound"][0] and fit["gain"][0] == 0.0 and fit["informative"][0]
    two = fit_prop_tumor([0, 1], [1], [2], evaluate=_closed_form(lambda m: -np.abs(np.abs(m - 0.5) - 0.1)))   # maxima at 0.4 and 0.6
    assert two["trace"][0]["k"][0] == 6 and abs(two["estimate"][0] - 0.4) < 0.01


def test_a_nan_pair_does_not_disturb_its_neighbours():
    from exomedepth_amd import fit_prop_tumor

    def objective(poison):
        def f(grid):
            l = 50.0 - 400.0 * (np.asarray(grid) - np.array([0.3, 0.5, 0.7])[None, :]) ** 2
            if poison:
                l[:, 1] = np.nan
            return l
        return f
    clean = fit_prop_tumor([0, 1], [1], [2], phi=np.zeros(3), evaluate=objective(False))
    dirty = fit_prop_tumor([0, 1], [1], [2], phi=np.zeros(3), evaluate=objective(True))
    for k in ("prop_tumor", "estimate", "log_evidence", "log_evidence_null", "gain", "se"):
        assert np.isnan(dirty[k][1]), k
        assert np.array_equal(dirty[k][[0, 2]], clean[k][[0, 2]]), k
    assert not dirty["informative"][1] and not dirty["at_bound"][1] and np.all(dirty["informative"][[0, 2]])
    late = fit_prop_tumor([0, 1], [1], [2], evaluate=lambda g: np.where(np.asarray(g) == 0.4, np.nan, -(np.asarray(g) - 0.43) ** 2))
    assert np.isnan(late["estimate"][0]) and not late["informative"][0]      # a NaN at any value evaluated


def test_mix_plan_checker(tmp_path):
    """tools/mix_plan_check.cpp compiles (without the sanitizer flags its header comment gives for a run by hand) and exits with 0"""
    cc = os.environ.get("ED_SHIM_CC", "gcc")       # the compiler tests/test_shim.py builds with
    exe = str(tmp_path / "mix_plan_check")
    subprocess.run([cc, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tools", "mix_plan_check.cpp"), "-o", exe, "-lstdc++", "-lm"],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert "ok" in r.stdout


def test_interface_declares_the_mixture_entries():
    from exomedepth_amd import _lib
    names = {n for n, _, _ in _lib.SYMBOLS}
    header = open(os.path.join(ROOT, "include", "exomedepth_amd.h")).read()
    source = open(os.path.join(ROOT, "exomedepth_amd", "csrc", "edmix.inc")).read()
    for sym in ("ed_plan_mixture_profile", "ed_mix_geometry"):
        assert sym in names, sym
        assert re.search(r"\b%s\(" % sym, header), sym
        assert re.search(r"ED_EXPORT int %s\(" % sym, source), sym
    assert "k_mix_profile" in source and '#include "edmix.inc"' in open(os.path.join(ROOT, "exomedepth_amd", "csrc", "edcore.hip")).read()
    import exomedepth_amd
    from exomedepth_amd import api
    for name in ("fit_prop_tumor", "mixture_geometry"):
        assert getattr(exomedepth_amd, name) is getattr(api, name) and name in exomedepth_amd.__all__
    assert callable(api.Plan.mixture_profile) and callable(api.ExomeDepth.fit_prop_tumor)
